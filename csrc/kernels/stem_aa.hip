// Antialiased random-resized-crop stem (gfx950): mode 3 of stem_s2d with StemParams::antialias.
// Image b's picture is the box rrc[b] of its source resized to Hc x Wc, each axis on its own: an
// axis the box is not shrunk on (n <= N) keeps mode 3's two bilinear taps, a shrunk axis (n > N)
// takes a triangle filter of half-width n / N source pixels with integer weights.  The definition
// is in kernels.h (StemParams::antialias); its arithmetic is aa_axis / aa_hrow / aa_vert below,
// which both kernel forms call, so the forms agree bit for bit.  Flip, mix table, zero padding and
// space-to-depth are mode 3's.
//
//   * stem_aa_pix_kernel : one thread per s2d pixel; every tapped row of each of its four
//                          sub-pixels is filtered from global memory.  Any input type and width
//                          (the fallback, and `set_variant("stem", 0)`); slow by construction.
//   * stem_aa_band_kernel: uint8 input.  One workgroup owns a band of R consecutive s2d rows (2R
//                          picture rows) of one image.  What the bilinear band form never met is a
//                          span of about (2R + 1) n / N + 2 source rows and a variable number of
//                          taps per column, and the three decisions that answer them are:
//       - raw rows are staged whole, once: the span's rows, the box's columns only, as aligned
//         4-byte words (a wave per row, each row with its own alignment shift).  A raw row is
//         3 Win bytes where a filtered fp32 row is 12 Wc, so at 512 -> 224 the span costs less
//         LDS raw than filtered, and a ring would put a workgroup barrier between rows;
//       - horizontal results never reach LDS.  A thread owns a picture column and walks the
//         staged rows from the top: it filters row r to three fp32 values (an exact integer sum,
//         one division) and feeds them at once to the vertical fma chains of the picture rows
//         that tap r.  A source row is tapped by at most two picture rows (the open interval
//         |(2r+1) N - (2o+1) n| < 2n holds at most two odd 2o+1), so two running accumulators per
//         channel are the whole vertical state, top-down is the definition's ascending order, and
//         every source row is filtered once per column however many picture rows share it;
//       - the column's tap list is four registers of its thread (first tap, end, centre, D); the
//         weights follow by an integer recurrence (d += 2N, u = 2n - |d|), so no table is read
//         in the inner loop.  The rows' lists ({first, end, centre, D} or {t0, t1, f}) are 2R
//         entries in LDS, made once while the rows are staged.
//     The finished picture rows go to an fp32 tile [2R][Wc][3] in LDS; lane (i, j) then writes
//     its s2d pixel with two (bf16) or four (fp32) 16-byte stores.  With a mix table the partner's
//     span is staged into the same raw buffer after the own walk, walked with the partner's box
//     and flip, and blended into the tile by the thread that owns the column: a mixed band needs
//     no more LDS than an unmixed one.  A partner of weight 0 over the whole band is not staged.
//     Which path an axis takes depends on the image's box alone: uniform over the workgroup.
#include "common.h"
#include "kernels.h"
#include "stem_common.h"

namespace pddl {

// One output index along one axis.  Lerp axis (n <= N): i0, i1 are mode 3's two taps and f the
// weight.  Weighted axis: taps [i0, i1), c = (2o+1) n the centre, D the sum of the weights.
struct AaAx { int i0, i1, c, D; float f; };
__device__ __forceinline__ int aa_floor(int a, int b) { return a >= 0 ? a / b : -((b - 1 - a) / b); }
__device__ __forceinline__ int aa_u(int i, int n, int N, int c) { return 2 * n - abs((2 * i + 1) * N - c); }
__device__ __forceinline__ AaAx aa_axis(int o, int n, int N) {
  AaAx a;
  if (n <= N) {
    const RrcTap t = rrc_tap(o, n, N);
    a.i0 = t.t0; a.i1 = t.t1; a.f = t.f; a.c = 0; a.D = 1;
    return a;
  }
  a.c = (2 * o + 1) * n;
  a.i0 = max(aa_floor(a.c - 2 * n - N, 2 * N) + 1, 0);     // u_i > 0  <=>  c - 2n < (2i+1) N < c + 2n
  a.i1 = min((a.c + 2 * n + N - 1) / (2 * N), n);
  a.D = 0; a.f = 0.f;
  for (int i = a.i0; i < a.i1; ++i) a.D += aa_u(i, n, N, a.c);
  return a;
}
// The horizontal pass of one source row for one column: `row` is the box's first pixel of the row.
__device__ __forceinline__ void aa_hrow(const uint8_t* row, const AaAx& a, int n, int N, float* h) {
  if (n <= N) {
#pragma unroll
    for (int c = 0; c < 3; ++c) h[c] = rrc_lerp((float)row[a.i0 * 3 + c], (float)row[a.i1 * 3 + c], a.f);
    return;
  }
  int S0 = 0, S1 = 0, S2 = 0, d = (2 * a.i0 + 1) * N - a.c;
  for (int i = a.i0; i < a.i1; ++i, d += 2 * N) {
    const int u = 2 * n - abs(d);
    S0 += u * row[i * 3]; S1 += u * row[i * 3 + 1]; S2 += u * row[i * 3 + 2];
  }
  const float D = (float)a.D;
  h[0] = __fdiv_rn((float)S0, D); h[1] = __fdiv_rn((float)S1, D); h[2] = __fdiv_rn((float)S2, D);
}
__device__ __forceinline__ void aa_hrow(const float* row, const AaAx& a, int n, int N, float* h) {
  if (n <= N) {
#pragma unroll
    for (int c = 0; c < 3; ++c) h[c] = rrc_lerp(row[a.i0 * 3 + c], row[a.i1 * 3 + c], a.f);
    return;
  }
  float S0 = 0.f, S1 = 0.f, S2 = 0.f;
  int d = (2 * a.i0 + 1) * N - a.c;
  for (int i = a.i0; i < a.i1; ++i, d += 2 * N) {
    const float u = (float)(2 * n - abs(d));
    S0 = __fmaf_rn(u, row[i * 3], S0); S1 = __fmaf_rn(u, row[i * 3 + 1], S1); S2 = __fmaf_rn(u, row[i * 3 + 2], S2);
  }
  const float D = (float)a.D;
  h[0] = __fdiv_rn(S0, D); h[1] = __fdiv_rn(S1, D); h[2] = __fdiv_rn(S2, D);
}
// The vertical pass: one step of a weighted row's chain, its end, and the lerp of an unshrunk axis.
__device__ __forceinline__ void aa_vacc(int u, const float* h, float* acc) {
  const float w = (float)u;
#pragma unroll
  for (int c = 0; c < 3; ++c) acc[c] = __fmaf_rn(w, h[c], acc[c]);
}
__device__ __forceinline__ void aa_vend(const float* acc, int D, float scale, float* v) {
  const float d = (float)D;
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = __fdiv_rn(acc[c], d) * scale;
}
__device__ __forceinline__ void aa_vlerp(const float* top, const float* bot, float f, float scale, float* v) {
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = rrc_lerp(top[c], bot[c], f) * scale;
}

// ------------------------------------------------------------------------------ per-pixel form
// One image's view of s2d pixel (i, j): its box and the tap lists of the two picture rows and the
// two (flipped) picture columns the s2d pixel covers.
struct AaQuad { RrcBox box; long base; AaAx ay[2], ax[2]; };
__device__ __forceinline__ AaQuad aa_quad(const StemParams& p, int b, int i, int j) {
  AaQuad r;
  r.box = rrc_box(p, b);
  const bool fl = p.flip && p.flip[b];
  r.base = ((long)b * p.Hin + r.box.y0) * p.Win + r.box.x0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int y = min(max(2 * i + k - 3, 0), p.Hc - 1), x = min(max(2 * j + k - 3, 0), p.Wc - 1);
    r.ay[k] = aa_axis(y, r.box.h, p.Hc);
    r.ax[k] = aa_axis(fl ? p.Wc - 1 - x : x, r.box.w, p.Wc);
  }
  return r;
}
template <typename T>
__device__ __forceinline__ void aa_pix_t(const StemParams& p, const AaQuad& r, int dy, int dx, float* v) {
  const AaAx ay = r.ay[dy], ax = r.ax[dx];
  const T* in = reinterpret_cast<const T*>(p.in);
  const int n = r.box.h, N = p.Hc;
  if (n <= N) {
    float top[3], bot[3];
    aa_hrow(in + (r.base + (long)ay.i0 * p.Win) * 3, ax, r.box.w, p.Wc, top);
    aa_hrow(in + (r.base + (long)ay.i1 * p.Win) * 3, ax, r.box.w, p.Wc, bot);
    aa_vlerp(top, bot, ay.f, p.scale, v);
    return;
  }
  float acc[3] = {0.f, 0.f, 0.f};
  for (int i = ay.i0; i < ay.i1; ++i) {
    float h[3];
    aa_hrow(in + (r.base + (long)i * p.Win) * 3, ax, r.box.w, p.Wc, h);
    aa_vacc(aa_u(i, n, N, ay.c), h, acc);
  }
  aa_vend(acc, ay.D, p.scale, v);
}
__device__ __forceinline__ void aa_pix(const StemParams& p, const AaQuad& r, int dy, int dx, float* v) {
  if (p.in_u8) aa_pix_t<uint8_t>(p, r, dy, dx, v);
  else aa_pix_t<float>(p, r, dy, dx, v);
}

template <typename OutT, bool MIX>
__global__ void stem_aa_pix_kernel(StemParams p, OutT* __restrict__ out, int npix, uint64_t mg_ws, uint64_t mg_hs) {
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += gridDim.x * blockDim.x) {
    const int t = fdiv(q, mg_ws);
    const int j = q - t * p.Ws;
    const int b = fdiv(t, mg_hs);
    const int i = t - b * p.Hs;
    const AaQuad own = aa_quad(p, b, i, j);
    StemMix m{};
    AaQuad par{};
    if (MIX) {
      m = stem_mix_row(p, b);
      par = aa_quad(p, m.pb, i, j);
    }
    float v[16];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int y = 2 * i + (d >> 1) - 3, x = 2 * j + (d & 1) - 3;
      float* vd = v + d * 4;
      vd[0] = vd[1] = vd[2] = vd[3] = 0.f;
      if (y < 0 || y >= p.Hc || x < 0 || x >= p.Wc) continue;
      if (!MIX) {
        aa_pix(p, own, d >> 1, d & 1, vd);
      } else {
        const float w = stem_mix_weight(m, y, x);
        float a[3] = {0.f, 0.f, 0.f}, o[3] = {0.f, 0.f, 0.f};   // a side of weight 0 is not fetched
        if (w != 0.f) aa_pix(p, own, d >> 1, d & 1, a);
        if (w != 1.f) aa_pix(p, par, d >> 1, d & 1, o);
#pragma unroll
        for (int c = 0; c < 3; ++c) vd[c] = stem_mix_blend(w, a[c], o[c]);
      }
    }
    rrc_store<OutT>(out, q, v);
  }
}

// ------------------------------------------------------------------------------ band form
constexpr int AA_THREADS = 256, AA_WAVES = AA_THREADS / 64;
// One image's staged span.  raw, rtab and tile are the workgroup's; the partner reuses raw and rtab.
struct AaSet {
  RrcBox box;
  int r0, nrows;   // first box row staged, rows staged
  long img;
  bool fl;
};
__device__ __forceinline__ const uint8_t* aa_src_row(const StemParams& p, const AaSet& s, int r) {
  return reinterpret_cast<const uint8_t*>(p.in) + ((s.img * p.Hin + s.box.y0 + s.r0 + r) * p.Win + s.box.x0) * 3;
}
// Stage one image: the row table of picture rows ya .. yb, and the box rows their taps span.
__device__ __forceinline__ void aa_stage(const StemParams& p, AaSet& s, uint32_t* raw, int* rtab, int img, int ya,
                                         int yb, int SPAN, int RAWW) {
  s.img = img;
  s.box = rrc_box(p, img);
  s.fl = p.flip && p.flip[img];
  const bool wy = s.box.h > p.Hc;
  const AaAx a = aa_axis(ya, s.box.h, p.Hc), z = aa_axis(yb, s.box.h, p.Hc);
  s.r0 = a.i0;
  s.nrows = min((wy ? z.i1 - 1 : z.i1) - s.r0 + 1, SPAN);   // (<= SPAN by the launcher's bound)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = wave; r < s.nrows; r += AA_WAVES) {
    const uintptr_t src = reinterpret_cast<uintptr_t>(aa_src_row(p, s, r));
    const uint32_t* w = reinterpret_cast<const uint32_t*>(src & ~uintptr_t(3));
    const int nw = min(((int)(src & 3) + s.box.w * 3 + 3) / 4, RAWW);
    for (int k = lane; k < nw; k += 64) raw[r * RAWW + k] = w[k];
  }
  for (int k = threadIdx.x; k <= yb - ya; k += AA_THREADS) {
    const AaAx t = aa_axis(ya + k, s.box.h, p.Hc);
    rtab[k * 4] = t.i0; rtab[k * 4 + 1] = t.i1; rtab[k * 4 + 2] = wy ? t.c : __float_as_int(t.f); rtab[k * 4 + 3] = t.D;
  }
}
// Staged row r (span-relative) at the box's first column.  Its alignment shift follows from row 0's
// (sh0, taken once per walk) by the row pitch modulo 4.  (The launcher's span bound keeps r inside the
// span; the clamp only turns a wrong bound into a wrong picture instead of a stray LDS read.)
__device__ __forceinline__ const uint8_t* aa_lds_row(const StemParams& p, const AaSet& s, const uint32_t* raw, int r,
                                                     int RAWW, int sh0) {
  r = min(max(r, 0), s.nrows - 1);
  return reinterpret_cast<const uint8_t*>(raw + r * RAWW) + ((sh0 + r * (p.Win * 3)) & 3);
}
// A finished picture row k of column x: the own pass fills the tile, the partner's pass blends into it.
template <bool BLEND>
__device__ __forceinline__ void aa_emit(const StemParams& p, const StemMix& m, float* tile, int ya, int k, int x,
                                        const float* v) {
  float* t = tile + (k * p.Wc + x) * 3;
  if (!BLEND) {
    t[0] = v[0]; t[1] = v[1]; t[2] = v[2];
  } else {
    const float w = stem_mix_weight(m, ya + k, x);
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = stem_mix_blend(w, t[c], v[c]);
  }
}
// The walk: every column's thread goes down the staged rows once.
template <bool BLEND>
__device__ __forceinline__ void aa_walk(const StemParams& p, const AaSet& s, const StemMix& m, const uint32_t* raw,
                                        const int* rtab, float* tile, int ya, int nk, int RAWW) {
  const int n = s.box.h, N = p.Hc;
  const int sh0 = (int)(reinterpret_cast<uintptr_t>(aa_src_row(p, s, 0)) & 3);
  for (int x = threadIdx.x; x < p.Wc; x += AA_THREADS) {
    const AaAx ax = aa_axis(s.fl ? p.Wc - 1 - x : x, s.box.w, p.Wc);
    if (n > N) {
      float A[3] = {0.f, 0.f, 0.f}, Bn[3] = {0.f, 0.f, 0.f};   // the chains of picture rows k and k + 1
      int k = 0;
      for (int r = 0; r < s.nrows && k < nk; ++r) {
        float h[3];
        aa_hrow(aa_lds_row(p, s, raw, r, RAWW, sh0), ax, s.box.w, p.Wc, h);
        const int i = s.r0 + r;
        if (i >= rtab[k * 4]) aa_vacc(aa_u(i, n, N, rtab[k * 4 + 2]), h, A);
        if (k + 1 < nk && i >= rtab[k * 4 + 4]) aa_vacc(aa_u(i, n, N, rtab[k * 4 + 6]), h, Bn);
        // row i was picture row k's last tap.  (At most one row ends per source row: the end index
        // ceil(((2o+3) n - N) / 2N) rises by n / N > 1 per output row, and the box's last row ends only row N - 1.)
        if (i == rtab[k * 4 + 1] - 1) {
          float v[3];
          aa_vend(A, rtab[k * 4 + 3], p.scale, v);
          aa_emit<BLEND>(p, m, tile, ya, k, x, v);
#pragma unroll
          for (int c = 0; c < 3; ++c) { A[c] = Bn[c]; Bn[c] = 0.f; }
          ++k;
        }
      }
    } else {
      float ha[3] = {0.f, 0.f, 0.f}, hb[3] = {0.f, 0.f, 0.f};   // the last two rows filtered: ia < ib
      int ia = -1, ib = -1;
      for (int k = 0; k < nk; ++k) {
        const int t0 = rtab[k * 4], t1 = rtab[k * 4 + 1];
        for (int e = 0; e < 2; ++e) {
          const int t = e ? t1 : t0;
          if (t != ia && t != ib) {
            ia = ib;
#pragma unroll
            for (int c = 0; c < 3; ++c) ha[c] = hb[c];
            ib = t;
            aa_hrow(aa_lds_row(p, s, raw, t - s.r0, RAWW, sh0), ax, s.box.w, p.Wc, hb);
          }
        }
        float top[3], bot[3], v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { top[c] = t0 == ia ? ha[c] : hb[c]; bot[c] = t1 == ib ? hb[c] : ha[c]; }
        aa_vlerp(top, bot, __int_as_float(rtab[k * 4 + 2]), p.scale, v);
        aa_emit<BLEND>(p, m, tile, ya, k, x, v);
      }
    }
  }
}

template <typename OutT, bool MIX>
__global__ void __launch_bounds__(AA_THREADS)
stem_aa_band_kernel(StemParams p, OutT* __restrict__ out, int R, int SPAN, int RAWW, int nbands, uint64_t mg_ws) {
  extern __shared__ uint32_t aa_lds[];
  uint32_t* raw = aa_lds;                                             // [SPAN][RAWW]
  float* tile = reinterpret_cast<float*>(raw + SPAN * RAWW);          // [2R][Wc][3]
  int* rtab = reinterpret_cast<int*>(tile + 2 * R * p.Wc * 3);        // [2R][4]
  const int b = blockIdx.x / nbands, band = blockIdx.x - b * nbands;
  const int i0 = band * R, i1 = min(i0 + R, p.Hs);
  const int ya = max(2 * i0 - 3, 0), yb = min(2 * i1 - 4, p.Hc - 1);   // the band's picture rows (none: ya > yb)
  if (ya <= yb) {
    const int nk = yb - ya + 1;
    AaSet s{};
    StemMix m{};
    aa_stage(p, s, raw, rtab, b, ya, yb, SPAN, RAWW);
    __syncthreads();
    aa_walk<false>(p, s, m, raw, rtab, tile, ya, nk, RAWW);
    if (MIX) {
      m = stem_mix_row(p, b);
      if (m.w != 1.f || (m.x0 < m.x1 && m.y0 <= yb && m.y1 > ya)) {   // (uniform over the workgroup)
        __syncthreads();
        aa_stage(p, s, raw, rtab, m.pb, ya, yb, SPAN, RAWW);
        __syncthreads();
        aa_walk<true>(p, s, m, raw, rtab, tile, ya, nk, RAWW);
      }
    }
    __syncthreads();
  }
  const int n = (i1 - i0) * p.Ws;
  for (int q = threadIdx.x; q < n; q += AA_THREADS) {
    const int il = fdiv(q, mg_ws);
    const int j = q - il * p.Ws, i = i0 + il;
    float v[16];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int y = 2 * i + (d >> 1) - 3, x = 2 * j + (d & 1) - 3;
      float* vd = v + d * 4;
      vd[0] = vd[1] = vd[2] = vd[3] = 0.f;
      if (y < ya || y > yb || x < 0 || x >= p.Wc) continue;
      const float* t = tile + ((y - ya) * p.Wc + x) * 3;
      vd[0] = t[0]; vd[1] = t[1]; vd[2] = t[2];
    }
    rrc_store<OutT>(out, ((long)b * p.Hs + i) * p.Ws + j, v);
  }
}

// ------------------------------------------------------------------------------ launcher
constexpr int AA_MAX_BAND = 8;
constexpr int AA_LDS = 40 << 10;   // per workgroup, mixed or not: 4 workgroups of a CU's 160 KB

// int32 headroom of one axis: the tap bounds reach (2N + 2) n + N, and the weights' sum D (times
// the largest pixel value `top` for the horizontal pass of uint8 input) is at most (2n / N + 1) 2n.
static bool aa_overflows(long n, long N, long top) {
  return (2 * N + 2) * n + N >= (1L << 31) || top * (2 * n / N + 1) * 2 * n >= (1L << 31);
}

template <typename OutT>
static const char* stem_aa_go(const StemParams& p, OutT* out, hipStream_t s) {
  if (!p.rrc) return "stem_s2d: mode 3 needs the rrc box table";
  if ((2L * p.Hc + 1) * p.Hin >= (1L << 31) || (2L * p.Wc + 1) * p.Win >= (1L << 31))
    return "stem_s2d: rrc coordinates overflow 32 bits";
  if (aa_overflows(p.Hin, p.Hc, 1) || aa_overflows(p.Win, p.Wc, p.in_u8 ? 255 : 1))
    return "stem_s2d: antialias weights overflow 32 bits";
  const long npix = (long)p.B * p.Hs * p.Ws;
  // the tallest band whose worst-case box (the whole source) fits the LDS budget.  SPAN: the 2R
  // picture rows ya .. yb of a band tap the box rows i with (2ya+1) n - 2n < (2i+1) N < (2yb+1) n + 2n,
  // an open interval of (yb - ya + 2) n / N <= (2R + 1) n / N in i, which holds at most floor + 1
  // integers; n <= Hin.  (An unshrunk axis: mode 3's (2R - 1) n / N + 3.)
  const int RAWW = (p.Win * 3) / 4 + 2;
  int R = 0, SPAN = 0;
  long bytes = 0;
  if (g_stem_variant == 1 && p.in_u8) {
    for (R = g_stem_rrc_band > 0 ? (g_stem_rrc_band < AA_MAX_BAND ? g_stem_rrc_band : AA_MAX_BAND) : AA_MAX_BAND; R > 0; --R) {
      SPAN = (int)lmin(lmax(((2L * R + 1) * p.Hin) / p.Hc + 2, ((2L * R - 1) * p.Hin) / p.Hc + 3), p.Hin);
      bytes = ((long)SPAN * RAWW + 2L * R * p.Wc * 3 + 2 * R * 4) * 4;
      if (bytes <= AA_LDS) break;
    }
  }
  if (R > 0) {
    const int nbands = (p.Hs + R - 1) / R;
    auto k = p.mix ? stem_aa_band_kernel<OutT, true> : stem_aa_band_kernel<OutT, false>;
    hipLaunchKernelGGL(k, dim3(p.B * nbands), dim3(AA_THREADS), (size_t)bytes, s, p, out, R, SPAN, RAWW, nbands,
                       fdiv_magic(p.Ws));
    stem_note_launch(3, R);
  } else {
    const int grid = (int)lmin((npix + 255) / 256, 16384);
    auto k = p.mix ? stem_aa_pix_kernel<OutT, true> : stem_aa_pix_kernel<OutT, false>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, s, p, out, (int)npix, fdiv_magic(p.Ws), fdiv_magic(p.Hs));
    stem_note_launch(4, 0);
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

const char* stem_aa_launch(const StemParams& p, void* out, int out_f32, hipStream_t s) {
  return out_f32 ? stem_aa_go<float>(p, reinterpret_cast<float*>(out), s)
                 : stem_aa_go<uint16_t>(p, reinterpret_cast<uint16_t*>(out), s);
}

}  // namespace pddl
