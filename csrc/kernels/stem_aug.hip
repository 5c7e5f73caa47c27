// RandAugment stem (gfx950): mode 3 of stem_s2d with a [B][16] table.  Image b's picture is the box
// of its row resampled through the row's inverse affine map (rotation, shear, translation; pixels
// that map outside the picture are fill), then its colour chain, then flip / mix / zero padding /
// 2x2 space-to-depth like the other modes.  The definition is in kernels.h (StemParams::rrc, "RandAugment
// rows"); its arithmetic is aug_row / aug_taps / aug_chain below, which both kernel forms call, so the
// forms agree bit for bit, and a row without a map takes rrc_tap and is the box picture bit for bit.
//
// The map is not separable, so the band kernel of stem_rrc.hip (whole source rows, resampled
// horizontally once and shared by neighbouring picture rows) does not apply.  Instead:
//
//   * stem_aug_tile_kernel: a 256-thread workgroup owns a 16 x 16 block of s2d pixels of one image
//       (32 x 32 picture pixels).  The map is affine, so the taps of the block lie in the bounding
//       rectangle of its four corners' pre-images (plus the second tap's row and column), clamped
//       to the box; the fill region needs no taps and is clamped away first.
//       1. stage: the rectangle as aligned 4-byte words, a wave per row, each row with its own
//          alignment shift (as rrc_stage does) -- when it fits the LDS budget; a rectangle that
//          does not (a steep minification) leaves the workgroup on global taps, a workgroup-uniform
//          choice, so no launch is sized by a worst-case box.
//       2. sample: lane (li, lj) maps its four sub-pixels in integers, takes four byte taps per
//          channel from LDS, lerps, runs the colour chain, blends, and writes the s2d pixel with
//          two (bf16) or four (fp32) 16-byte stores.
//       With a mix table the partner's rectangle (its own box, map, chain and mean) is staged into
//       a second buffer; a partner of weight 0 over the whole block is not staged.
//   * stem_aug_pix_kernel : one thread per s2d pixel, the taps from global memory.  It is the
//       faster of the two as measured (the tile form's byte-wide LDS taps and its staging cost more
//       than the cache misses they save), so it is the default; the tile form is `set_variant("stem", 2)`.
//   * stem_gray_mean_kernel: the grey mean of a contrast op, one workgroup per image (kernels.h).
#include "common.h"
#include "kernels.h"
#include "stem_common.h"

namespace pddl {

constexpr int AUG_COLS = 16, AUG_THREADS = 256, AUG_WAVES = AUG_THREADS / 64, AUG_TILE = 16;
constexpr int AUG_LDS_WORDS = 6144;   // per staged rectangle: 24 KB, 6 (3 with a mix table) workgroups of a CU's 160 KB
enum { AUG_BRIGHTNESS = 1, AUG_COLOR = 2, AUG_CONTRAST = 3, AUG_SOLARIZE = 4, AUG_POSTERIZE = 5 };

// ------------------------------------------------------------------------------ the definition
struct AugRow {
  RrcBox box;
  long base;          // source pixel index of the box's first pixel
  int geo, fl, ops;
  int m[6];           // a b c / d e f
  float par[4], mean;
};
__device__ __forceinline__ AugRow aug_row(const StemParams& p, int b) {
  const int32_t* r = p.rrc + (long)b * AUG_COLS;
  AugRow a;
  a.box.y0 = min(max(r[0], 0), p.Hin - 1); a.box.x0 = min(max(r[1], 0), p.Win - 1);
  a.box.h = min(max(r[2], 1), p.Hin - a.box.y0); a.box.w = min(max(r[3], 1), p.Win - a.box.x0);
  a.base = ((long)b * p.Hin + a.box.y0) * p.Win + a.box.x0;
#pragma unroll
  for (int k = 0; k < 6; ++k) a.m[k] = r[4 + k];
  a.ops = r[10] & 0xFFFF;
  a.geo = (r[10] >> 16) & 1;
#pragma unroll
  for (int k = 0; k < 4; ++k) a.par[k] = __int_as_float(r[11 + k]);
  a.mean = __int_as_float(r[15]);
  a.fl = p.flip && p.flip[b];
  return a;
}
// floor(n / d) for 0 <= n < 2^53: the fp64 quotient is off by at most one, the remainder decides.
__device__ __forceinline__ long aug_floordiv(long n, long d, double rd) {
  long q = (long)((double)n * rd);
  const long r = n - q * d;
  return q + (r >= d) - (r < 0);
}
// The doubled, centre-relative Q16 picture coordinates of picture pixel (x, y).
__device__ __forceinline__ void aug_map(const StemParams& p, const AugRow& r, int y, int x, long* U, long* V) {
  const long u = 2 * x + 1 - p.Wc, v = 2 * y + 1 - p.Hc;
  const long uu = r.m[0] * u + r.m[1] * v + r.m[2];
  *U = r.fl ? -uu : uu;
  *V = r.m[3] * u + r.m[4] * v + r.m[5];
}
// A coordinate inside (-N 2^16, N 2^16) -> the Q8 position along a box side of n source pixels.
__device__ __forceinline__ int aug_q8(long U, int n, int N) {
  const long d = (long)N << 9;
  return (int)aug_floordiv((U + ((long)N << 16)) * n, d, 1.0 / (double)d) - 128;
}
__device__ __forceinline__ RrcTap aug_q8_tap(int q8, int n) {
  RrcTap t;
  const int k = q8 >> 8;   // (arithmetic: -1 for the half pixel before the first centre)
  t.t0 = min(max(k, 0), n - 1); t.t1 = min(max(k + 1, 0), n - 1);
  t.f = (float)(q8 & 255) * (1.f / 256.f);
  return t;
}
struct AugTaps { RrcTap ty, tx; bool fill; };
__device__ __forceinline__ AugTaps aug_taps(const StemParams& p, const AugRow& r, int y, int x) {
  AugTaps t;
  t.fill = false;
  if (!r.geo) {
    t.ty = rrc_tap(y, r.box.h, p.Hc);
    t.tx = rrc_tap(r.fl ? p.Wc - 1 - x : x, r.box.w, p.Wc);
    return t;
  }
  long U, V;
  aug_map(p, r, y, x, &U, &V);
  const long NU = (long)p.Wc << 16, NV = (long)p.Hc << 16;
  if (U <= -NU || U >= NU || V <= -NV || V >= NV) {
    t.fill = true;
    t.ty = t.tx = RrcTap{0, 0, 0.f};
    return t;
  }
  t.ty = aug_q8_tap(aug_q8(V, r.box.h, p.Hc), r.box.h);
  t.tx = aug_q8_tap(aug_q8(U, r.box.w, p.Wc), r.box.w);
  return t;
}
__device__ __forceinline__ float aug_clamp(float v) { return fminf(fmaxf(v, 0.f), 255.f); }
// The colour chain on one raw (r, g, b) triple.
__device__ __forceinline__ void aug_chain(const AugRow& r, float* v) {
  if (!r.ops) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int op = (r.ops >> (4 * k)) & 15;
    const float a = r.par[k];
    if (op == AUG_BRIGHTNESS) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = aug_clamp(a * v[c]);
    } else if (op == AUG_COLOR || op == AUG_CONTRAST) {
      const float g = op == AUG_CONTRAST ? r.mean : __fmaf_rn(0.114f, v[2], __fmaf_rn(0.587f, v[1], 0.299f * v[0]));
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = aug_clamp(__fmaf_rn(a, v[c] - g, g));
    } else if (op == AUG_SOLARIZE) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = aug_clamp(v[c] >= a ? 255.f - v[c] : v[c]);
    } else if (op == AUG_POSTERIZE) {
      const int mask = (int)a;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = aug_clamp((float)((int)v[c] & mask));
    }
  }
}

// Where one image's taps come from: its staged rectangle (LDS) or the source itself.
struct AugSrc {
  const uint8_t* lds;          // staged rows, each `pitch` bytes apart, row r shifted by (shift0 + r rowinc) & 3 bytes
  int ry0, rx0, pitch, shift0, rowinc;
};
template <bool LDS>
__device__ __forceinline__ float aug_fetch(const StemParams& p, const AugRow& r, const AugSrc& s, int ty, int tx, int c) {
  if (LDS) {
    const int rr = ty - s.ry0;
    return (float)s.lds[rr * s.pitch + ((s.shift0 + rr * s.rowinc) & 3) + (tx - s.rx0) * 3 + c];
  }
  return (float)reinterpret_cast<const uint8_t*>(p.in)[(r.base + (long)ty * p.Win + tx) * 3 + c];
}
// The three channels of picture pixel (y, x) of one image, before mixing.
template <bool LDS>
__device__ __forceinline__ void aug_pix(const StemParams& p, const AugRow& r, const AugSrc& s, int y, int x, float* v) {
  const AugTaps t = aug_taps(p, r, y, x);
  float raw[3] = {128.f, 128.f, 128.f};
  if (!t.fill) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = rrc_lerp(aug_fetch<LDS>(p, r, s, t.ty.t0, t.tx.t0, c), aug_fetch<LDS>(p, r, s, t.ty.t0, t.tx.t1, c), t.tx.f);
      const float bot = rrc_lerp(aug_fetch<LDS>(p, r, s, t.ty.t1, t.tx.t0, c), aug_fetch<LDS>(p, r, s, t.ty.t1, t.tx.t1, c), t.tx.f);
      raw[c] = rrc_lerp(top, bot, t.ty.f);
    }
  }
  aug_chain(r, raw);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = raw[c] * p.scale;
}

// One s2d pixel (i, j) of image b: its four sub-pixels, blended with the partner's where MIX.
template <bool MIX, bool LA, bool LB>
__device__ __forceinline__ void aug_s2d_pixel(const StemParams& p, const AugRow& own, const AugSrc& sa, const AugRow& par,
                                              const AugSrc& sb, const StemMix& m, int i, int j, float* v) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int y = 2 * i + (d >> 1) - 3, x = 2 * j + (d & 1) - 3;
    float* vd = v + d * 4;
    vd[0] = vd[1] = vd[2] = vd[3] = 0.f;
    if (y < 0 || y >= p.Hc || x < 0 || x >= p.Wc) continue;
    if (!MIX) {
      aug_pix<LA>(p, own, sa, y, x, vd);
    } else {
      const float w = stem_mix_weight(m, y, x);
      float a[3] = {0.f, 0.f, 0.f}, o[3] = {0.f, 0.f, 0.f};   // a side of weight 0 is not sampled
      if (w != 0.f) aug_pix<LA>(p, own, sa, y, x, a);
      if (w != 1.f) aug_pix<LB>(p, par, sb, y, x, o);
#pragma unroll
      for (int c = 0; c < 3; ++c) vd[c] = stem_mix_blend(w, a[c], o[c]);
    }
  }
}

// ------------------------------------------------------------------------------ per-pixel form
template <typename OutT, bool MIX>
__global__ void stem_aug_pix_kernel(StemParams p, OutT* __restrict__ out, int npix, uint64_t mg_ws, uint64_t mg_hs) {
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += gridDim.x * blockDim.x) {
    const int t = fdiv(q, mg_ws);
    const int j = q - t * p.Ws;
    const int b = fdiv(t, mg_hs);
    const int i = t - b * p.Hs;
    const AugRow own = aug_row(p, b);
    const AugSrc none{};
    StemMix m{};
    AugRow par = own;
    if (MIX) {
      m = stem_mix_row(p, b);
      par = aug_row(p, m.pb);
    }
    float v[16];
    aug_s2d_pixel<MIX, false, false>(p, own, none, par, none, m, i, j, v);
    rrc_store<OutT>(out, q, v);
  }
}

// ------------------------------------------------------------------------------ tile form
// The box-relative rectangle the taps of picture pixels [ya, yb] x [xa, xb] lie in (nr = 0: all fill).
struct AugRect { int ry0, rx0, nr, nc; };
__device__ __forceinline__ AugRect aug_rect(const StemParams& p, const AugRow& r, int ya, int yb, int xa, int xb) {
  int ry0, ry1, rx0, rx1;
  if (!r.geo) {
    ry0 = rrc_tap(ya, r.box.h, p.Hc).t0; ry1 = rrc_tap(yb, r.box.h, p.Hc).t1;
    rx0 = rrc_tap(r.fl ? p.Wc - 1 - xb : xa, r.box.w, p.Wc).t0;
    rx1 = rrc_tap(r.fl ? p.Wc - 1 - xa : xb, r.box.w, p.Wc).t1;
  } else {
    const long NU = (long)p.Wc << 16, NV = (long)p.Hc << 16;
    long U0 = NU, U1 = -NU, V0 = NV, V1 = -NV;   // the map is affine: its extremes over the block are at the corners
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      long U, V;
      aug_map(p, r, (k & 2) ? yb : ya, (k & 1) ? xb : xa, &U, &V);
      U0 = lmin(U0, U); U1 = lmax(U1, U); V0 = lmin(V0, V); V1 = lmax(V1, V);
    }
    U0 = lmax(U0, 1 - NU); U1 = lmin(U1, NU - 1); V0 = lmax(V0, 1 - NV); V1 = lmin(V1, NV - 1);   // (fill takes no taps)
    if (U0 > U1 || V0 > V1) return AugRect{0, 0, 0, 0};
    ry0 = aug_q8_tap(aug_q8(V0, r.box.h, p.Hc), r.box.h).t0; ry1 = aug_q8_tap(aug_q8(V1, r.box.h, p.Hc), r.box.h).t1;
    rx0 = aug_q8_tap(aug_q8(U0, r.box.w, p.Wc), r.box.w).t0; rx1 = aug_q8_tap(aug_q8(U1, r.box.w, p.Wc), r.box.w).t1;
  }
  return AugRect{ry0, rx0, ry1 - ry0 + 1, rx1 - rx0 + 1};
}
// Stage one image's rectangle into `words` when it fits (returns whether it did): rows of
// `pitch` bytes, each the aligned words that cover its nc pixels.
__device__ __forceinline__ bool aug_stage(const StemParams& p, const AugRow& r, const AugRect& q, uint32_t* words, AugSrc* s) {
  const int sw = (q.nc * 3 + 3) / 4 + 1;
  if (q.nr == 0 || (long)q.nr * sw > AUG_LDS_WORDS) return false;
  const uint8_t* src0 = reinterpret_cast<const uint8_t*>(p.in) + (r.base + (long)q.ry0 * p.Win + q.rx0) * 3;
  s->lds = reinterpret_cast<const uint8_t*>(words);
  s->ry0 = q.ry0; s->rx0 = q.rx0; s->pitch = sw * 4;
  s->shift0 = (int)(reinterpret_cast<uintptr_t>(src0) & 3);
  s->rowinc = (p.Win * 3) & 3;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = wave; k < q.nr; k += AUG_WAVES) {
    const uintptr_t src = reinterpret_cast<uintptr_t>(src0 + (long)k * p.Win * 3);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(src & ~uintptr_t(3));
    const int nw = ((int)(src & 3) + q.nc * 3 + 3) / 4;   // (<= sw)
    for (int e = lane; e < nw; e += 64) words[k * sw + e] = w[e];
  }
  return true;
}

template <typename OutT, bool MIX>
__global__ void __launch_bounds__(AUG_THREADS)
stem_aug_tile_kernel(StemParams p, OutT* __restrict__ out, int tx_n, int ty_n) {
  extern __shared__ uint32_t aug_lds[];
  const int ntile = tx_n * ty_n;
  const int b = blockIdx.x / ntile, t = blockIdx.x - b * ntile;
  const int ti = t / tx_n, tj = t - ti * tx_n;
  const int i0 = ti * AUG_TILE, j0 = tj * AUG_TILE;
  // the block's picture pixels (none: ya > yb or xa > xb, a block of padding only)
  const int ya = max(2 * i0 - 3, 0), yb = min(2 * (i0 + AUG_TILE) - 4, p.Hc - 1);
  const int xa = max(2 * j0 - 3, 0), xb = min(2 * (j0 + AUG_TILE) - 4, p.Wc - 1);
  const bool any = ya <= yb && xa <= xb;
  const AugRow own = aug_row(p, b);
  AugRow par = own;
  AugSrc sa{}, sb{};
  StemMix m{};
  bool la = false, lb = false, blend = false;   // (all uniform over the workgroup)
  if (any) {
    la = aug_stage(p, own, aug_rect(p, own, ya, yb, xa, xb), aug_lds, &sa);
    if (MIX) {
      m = stem_mix_row(p, b);
      blend = m.w != 1.f || (m.x0 <= xb && m.x1 > xa && m.y0 <= yb && m.y1 > ya);
      if (blend) {
        par = aug_row(p, m.pb);
        lb = aug_stage(p, par, aug_rect(p, par, ya, yb, xa, xb), aug_lds + AUG_LDS_WORDS, &sb);
      }
    }
  }
  __syncthreads();
  const int i = i0 + (threadIdx.x >> 4), j = j0 + (threadIdx.x & 15);
  if (i >= p.Hs || j >= p.Ws) return;
  float v[16];
  // (without `blend` every weight of the block is 1 and the partner is never sampled)
  if (la && (lb || !blend)) aug_s2d_pixel<MIX, true, true>(p, own, sa, par, sb, m, i, j, v);
  else if (la)              aug_s2d_pixel<MIX, true, false>(p, own, sa, par, sb, m, i, j, v);
  else if (lb)              aug_s2d_pixel<MIX, false, true>(p, own, sa, par, sb, m, i, j, v);
  else                      aug_s2d_pixel<MIX, false, false>(p, own, sa, par, sb, m, i, j, v);
  rrc_store<OutT>(out, ((long)b * p.Hs + i) * p.Ws + j, v);
}

// ------------------------------------------------------------------------------ grey mean
__global__ void __launch_bounds__(AUG_THREADS) stem_gray_mean_kernel(StemParams p, int32_t* __restrict__ table) {
  __shared__ uint32_t red[AUG_THREADS];
  const int b = blockIdx.x;
  const int ops = table[(long)b * AUG_COLS + 10];
  bool need = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) need |= ((ops >> (4 * k)) & 15) == AUG_CONTRAST;
  if (!need) return;   // (uniform over the workgroup)
  const AugRow r = aug_row(p, b);
  const uint8_t* src = reinterpret_cast<const uint8_t*>(p.in) + r.base * 3;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t sum = 0;
  for (int y = wave; y < r.box.h; y += AUG_WAVES) {
    const uint8_t* row = src + (long)y * p.Win * 3;
    for (int x = lane; x < r.box.w; x += 64)
      sum += (19595u * row[x * 3] + 38470u * row[x * 3 + 1] + 7471u * row[x * 3 + 2] + 32768u) >> 16;
  }
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int s = AUG_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0)
    table[(long)b * AUG_COLS + 15] = __float_as_int(__fdiv_rn((float)red[0], (float)(r.box.h * r.box.w)));
}

// ------------------------------------------------------------------------------ launchers
static const char* aug_check(const StemParams& p) {
  if (!p.rrc) return "stem_s2d: mode 3 needs the rrc box table";
  if (p.mode != 3 || !p.in_u8) return "stem_s2d: a 16-column (RandAugment) table needs uint8 input and mode 3";
  if (p.antialias) return "stem_s2d: antialias with a 16-column (RandAugment) table is not supported";
  if ((2L * p.Hc + 1) * p.Hin >= (1L << 31) || (2L * p.Wc + 1) * p.Win >= (1L << 31))
    return "stem_s2d: rrc coordinates overflow 32 bits";
  if ((long)p.Hin * p.Win >= (1L << 24)) return "stem_s2d: source too large for the 32-bit grey sum";
  return nullptr;
}

const char* stem_gray_mean_launch(const StemParams& p, int32_t* table, hipStream_t s) {
  if (const char* e = aug_check(p)) return e;
  hipLaunchKernelGGL(stem_gray_mean_kernel, dim3(p.B), dim3(AUG_THREADS), 0, s, p, table);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

template <typename OutT>
static const char* stem_aug_go(const StemParams& p, OutT* out, hipStream_t s) {
  if (const char* e = aug_check(p)) return e;
  const long npix = (long)p.B * p.Hs * p.Ws;
  const int tx_n = (p.Ws + AUG_TILE - 1) / AUG_TILE, ty_n = (p.Hs + AUG_TILE - 1) / AUG_TILE;
  const long nwg = (long)p.B * tx_n * ty_n;
  // The per-pixel form is the default: measured (profiles/randaug_stem.txt) it is 1.65x faster than the tile
  // form without and 2.3x with a mix table at batch 2560; the tile form runs under set_variant("stem", 2).
  if (g_stem_variant == 2 && nwg < (1L << 31)) {
    auto k = p.mix ? stem_aug_tile_kernel<OutT, true> : stem_aug_tile_kernel<OutT, false>;
    const size_t bytes = (size_t)AUG_LDS_WORDS * 4 * (p.mix ? 2 : 1);
    hipLaunchKernelGGL(k, dim3((unsigned)nwg), dim3(AUG_THREADS), bytes, s, p, out, tx_n, ty_n);
    stem_note_launch(5, 0);
  } else {
    const int grid = (int)lmin((npix + 255) / 256, 16384);
    auto k = p.mix ? stem_aug_pix_kernel<OutT, true> : stem_aug_pix_kernel<OutT, false>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, s, p, out, (int)npix, fdiv_magic(p.Ws), fdiv_magic(p.Hs));
    stem_note_launch(6, 0);
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

const char* stem_aug_launch(const StemParams& p, void* out, int out_f32, hipStream_t s) {
  return out_f32 ? stem_aug_go<float>(p, reinterpret_cast<float*>(out), s)
                 : stem_aug_go<uint16_t>(p, reinterpret_cast<uint16_t*>(out), s);
}

}  // namespace pddl
