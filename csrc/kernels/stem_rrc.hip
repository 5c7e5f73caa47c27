// Random-resized-crop stem (gfx950): mode 3 of stem_s2d.  Image b's picture is the box
// rrc[b] = {y0, x0, h, w} of its source, resized to Hc x Wc (bilinear, half-pixel centres, taps
// clamped to the box, no antialias: that is stem_aa.hip), then flipped, mixed, zero-padded and 2x2 space-to-depth'ed
// like the other modes.  The definition is in kernels.h (StemParams::rrc); its arithmetic is
// rrc_box / rrc_tap / rrc_lerp below, which both kernel forms call, so the forms agree bit for bit.
//
//   * stem_rrc_pix_kernel : one thread per s2d pixel, four scattered taps per channel; any input
//                           type and width (the fallback, and `set_variant("stem", 0)`).
//   * stem_rrc_band_kernel: uint8 input.  One workgroup owns a band of R consecutive s2d rows
//                           (2R picture rows) of one image and makes three passes through LDS:
//       1. stage: the source rows the band's taps span (at most SPAN = (2R-1) Hin / Hc + 3 of
//          them), the box's columns only, as aligned 4-byte words (a wave per row, each row with
//          its own alignment shift); meanwhile the column table (two byte offsets and fx per
//          picture column, the flip folded in) and the row table (two staged-row indices and fy
//          per picture row) are built, so no later pass divides;
//       2. horizontal: every staged row is resampled once to Wc x 3 fp32 values in LDS
//          (horizontal-first is what makes this reuse legal: top and bot of the definition are
//          whole-row quantities that neighbouring picture rows share);
//       3. vertical: lane (i, j) lerps the two fp32 rows of each of its four sub-pixels,
//          scales, blends, and writes the s2d pixel with two (bf16) or four (fp32) 16-byte stores.
//     With a mix table the partner's span goes through passes 1 and 2 with the partner's own box
//     and flip into a second set of buffers; a partner of weight 0 over the whole band is not
//     staged and the band runs the unmixed pass 3.
#include "common.h"
#include "kernels.h"
#include "stem_common.h"

namespace pddl {

// (RrcBox, rrc_box, rrc_tap, rrc_lerp, rrc_store: stem_common.h, shared with stem_aa.hip)

// ------------------------------------------------------------------------------ per-pixel form
// One image's view of s2d pixel (i, j): its box's first pixel and the taps of the two picture rows
// and the two (flipped) picture columns the s2d pixel covers, made once for its four sub-pixels.
// (Rows and columns in the padding ring are clamped into the picture; their taps are never read.)
struct RrcQuad { long base; RrcTap ty[2], tx[2]; };
__device__ __forceinline__ RrcQuad rrc_quad(const StemParams& p, int b, int i, int j) {
  const RrcBox q = rrc_box(p, b);
  const bool fl = p.flip && p.flip[b];
  RrcQuad r;
  r.base = ((long)b * p.Hin + q.y0) * p.Win + q.x0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int y = min(max(2 * i + k - 3, 0), p.Hc - 1), x = min(max(2 * j + k - 3, 0), p.Wc - 1);
    r.ty[k] = rrc_tap(y, q.h, p.Hc);
    r.tx[k] = rrc_tap(fl ? p.Wc - 1 - x : x, q.w, p.Wc);
  }
  return r;
}
// The three channels of sub-pixel (dy, dx), before mixing: four scattered taps per channel.
__device__ __forceinline__ void rrc_pix(const StemParams& p, const RrcQuad& r, int dy, int dx, float* v) {
  const RrcTap ty = r.ty[dy], tx = r.tx[dx];
  const long r0 = r.base + (long)ty.t0 * p.Win, r1 = r.base + (long)ty.t1 * p.Win;
  auto fetch = [&](long pix, int c) -> float {
    return p.in_u8 ? (float)reinterpret_cast<const uint8_t*>(p.in)[pix * 3 + c]
                   : reinterpret_cast<const float*>(p.in)[pix * 3 + c];
  };
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = rrc_lerp(fetch(r0 + tx.t0, c), fetch(r0 + tx.t1, c), tx.f);
    const float bot = rrc_lerp(fetch(r1 + tx.t0, c), fetch(r1 + tx.t1, c), tx.f);
    v[c] = rrc_lerp(top, bot, ty.f) * p.scale;
  }
}

template <typename OutT, bool MIX>
__global__ void stem_rrc_pix_kernel(StemParams p, OutT* __restrict__ out, int npix, uint64_t mg_ws, uint64_t mg_hs) {
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += gridDim.x * blockDim.x) {
    const int t = fdiv(q, mg_ws);
    const int j = q - t * p.Ws;
    const int b = fdiv(t, mg_hs);
    const int i = t - b * p.Hs;
    const RrcQuad own = rrc_quad(p, b, i, j);
    StemMix m{};
    RrcQuad par{};
    if (MIX) {
      m = stem_mix_row(p, b);
      par = rrc_quad(p, m.pb, i, j);
    }
    float v[16];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int y = 2 * i + (d >> 1) - 3, x = 2 * j + (d & 1) - 3;
      float* vd = v + d * 4;
      vd[0] = vd[1] = vd[2] = vd[3] = 0.f;
      if (y < 0 || y >= p.Hc || x < 0 || x >= p.Wc) continue;
      if (!MIX) {
        rrc_pix(p, own, d >> 1, d & 1, vd);
      } else {
        const float w = stem_mix_weight(m, y, x);
        float a[3] = {0.f, 0.f, 0.f}, o[3] = {0.f, 0.f, 0.f};   // a side of weight 0 is not fetched
        if (w != 0.f) rrc_pix(p, own, d >> 1, d & 1, a);
        if (w != 1.f) rrc_pix(p, par, d >> 1, d & 1, o);
#pragma unroll
        for (int c = 0; c < 3; ++c) vd[c] = stem_mix_blend(w, a[c], o[c]);
      }
    }
    rrc_store<OutT>(out, q, v);
  }
}

// ------------------------------------------------------------------------------ band form
constexpr int RRC_THREADS = 256, RRC_WAVES = RRC_THREADS / 64;
// The LDS of one image's span, carved out of the workgroup's dynamic LDS (words).
struct RrcSet {
  uint32_t* raw;   // [SPAN][RAWW] staged source rows, aligned words
  float* hrow;     // [SPAN][Wc * 3] horizontally resampled rows
  int* ctab;       // [Wc][3] byte offsets of the two column taps in a staged row, fx bits
  int* rtab;       // [2R][3] staged-row indices of the two row taps, fy bits
  RrcBox box;
  int r0, nrows;   // first box row staged, rows staged
  long img;
};
__device__ __forceinline__ int rrc_set_words(int SPAN, int RAWW, int Wc, int R) {
  return SPAN * RAWW + SPAN * Wc * 3 + Wc * 3 + 2 * R * 3;
}
__device__ __forceinline__ const uint8_t* rrc_src_row(const StemParams& p, const RrcSet& s, int r) {
  return reinterpret_cast<const uint8_t*>(p.in) + ((s.img * p.Hin + s.box.y0 + s.r0 + r) * p.Win + s.box.x0) * 3;
}
// Pass 1 for one image: the tables, and the rows t0(ya) .. t1(yb) of its box as aligned words.
__device__ __forceinline__ void rrc_stage(const StemParams& p, RrcSet& s, uint32_t* base, int img, int ya, int yb,
                                          int R, int SPAN, int RAWW) {
  s.raw = base;
  s.hrow = reinterpret_cast<float*>(base + SPAN * RAWW);
  s.ctab = reinterpret_cast<int*>(s.hrow + SPAN * p.Wc * 3);
  s.rtab = s.ctab + p.Wc * 3;
  s.img = img;
  s.box = rrc_box(p, img);
  s.r0 = rrc_tap(ya, s.box.h, p.Hc).t0;
  s.nrows = min(rrc_tap(yb, s.box.h, p.Hc).t1 - s.r0 + 1, SPAN);   // (<= SPAN by the launcher's bound)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = wave; r < s.nrows; r += RRC_WAVES) {
    const uintptr_t src = reinterpret_cast<uintptr_t>(rrc_src_row(p, s, r));
    const uint32_t* w = reinterpret_cast<const uint32_t*>(src & ~uintptr_t(3));
    const int nw = min(((int)(src & 3) + s.box.w * 3 + 3) / 4, RAWW);
    for (int k = lane; k < nw; k += 64) s.raw[r * RAWW + k] = w[k];
  }
  const bool fl = p.flip && p.flip[img];
  for (int x = threadIdx.x; x < p.Wc; x += RRC_THREADS) {
    const RrcTap t = rrc_tap(fl ? p.Wc - 1 - x : x, s.box.w, p.Wc);
    s.ctab[x * 3] = t.t0 * 3; s.ctab[x * 3 + 1] = t.t1 * 3; s.ctab[x * 3 + 2] = __float_as_int(t.f);
  }
  for (int k = threadIdx.x; k <= yb - ya && k < 2 * R; k += RRC_THREADS) {
    const RrcTap t = rrc_tap(ya + k, s.box.h, p.Hc);
    s.rtab[k * 3] = min(max(t.t0 - s.r0, 0), s.nrows - 1);
    s.rtab[k * 3 + 1] = min(max(t.t1 - s.r0, 0), s.nrows - 1);
    s.rtab[k * 3 + 2] = __float_as_int(t.f);
  }
}
// Pass 2: hrow[r][x] = lerp of staged row r's two column taps, a wave per row.
__device__ __forceinline__ void rrc_hpass(const StemParams& p, const RrcSet& s, int RAWW) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = wave; r < s.nrows; r += RRC_WAVES) {
    const int shift = (int)(reinterpret_cast<uintptr_t>(rrc_src_row(p, s, r)) & 3);
    const uint8_t* rb = reinterpret_cast<const uint8_t*>(s.raw + r * RAWW) + shift;
    float* h = s.hrow + r * p.Wc * 3;
    for (int x = lane; x < p.Wc; x += 64) {
      const int a = s.ctab[x * 3], b = s.ctab[x * 3 + 1];
      const float fx = __int_as_float(s.ctab[x * 3 + 2]);
#pragma unroll
      for (int c = 0; c < 3; ++c) h[x * 3 + c] = rrc_lerp((float)rb[a + c], (float)rb[b + c], fx);
    }
  }
}
// Pass 3 for one picture pixel: row k of the band (y - ya), column x.
__device__ __forceinline__ void rrc_vpass(const StemParams& p, const RrcSet& s, int k, int x, float* v) {
  const float* top = s.hrow + s.rtab[k * 3] * p.Wc * 3 + x * 3;
  const float* bot = s.hrow + s.rtab[k * 3 + 1] * p.Wc * 3 + x * 3;
  const float fy = __int_as_float(s.rtab[k * 3 + 2]);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = rrc_lerp(top[c], bot[c], fy) * p.scale;
}

template <typename OutT, bool MIX>
__global__ void __launch_bounds__(RRC_THREADS)
stem_rrc_band_kernel(StemParams p, OutT* __restrict__ out, int R, int SPAN, int RAWW, int nbands, uint64_t mg_ws) {
  extern __shared__ uint32_t rrc_lds[];
  const int b = blockIdx.x / nbands, band = blockIdx.x - b * nbands;
  const int i0 = band * R, i1 = min(i0 + R, p.Hs);
  const int ya = max(2 * i0 - 3, 0), yb = min(2 * i1 - 4, p.Hc - 1);   // the band's picture rows (none: ya > yb)
  RrcSet own{}, par{};
  StemMix m{};
  bool blend = false;   // (MIX, uniform over the workgroup: the partner's span is staged)
  if (ya <= yb) {
    rrc_stage(p, own, rrc_lds, b, ya, yb, R, SPAN, RAWW);
    if (MIX) {
      m = stem_mix_row(p, b);
      blend = m.w != 1.f || (m.x0 < m.x1 && m.y0 <= yb && m.y1 > ya);
      if (blend) rrc_stage(p, par, rrc_lds + rrc_set_words(SPAN, RAWW, p.Wc, R), m.pb, ya, yb, R, SPAN, RAWW);
    }
    __syncthreads();
    rrc_hpass(p, own, RAWW);
    if (MIX && blend) rrc_hpass(p, par, RAWW);
    __syncthreads();
  }
  const int n = (i1 - i0) * p.Ws;
  for (int q = threadIdx.x; q < n; q += RRC_THREADS) {
    const int il = fdiv(q, mg_ws);
    const int j = q - il * p.Ws, i = i0 + il;
    float v[16];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int y = 2 * i + (d >> 1) - 3, x = 2 * j + (d & 1) - 3;
      float* vd = v + d * 4;
      vd[0] = vd[1] = vd[2] = vd[3] = 0.f;
      if (y < ya || y > yb || x < 0 || x >= p.Wc) continue;
      if (MIX && blend) {
        float a[3], o[3];
        rrc_vpass(p, own, y - ya, x, a);
        rrc_vpass(p, par, y - ya, x, o);
        const float w = stem_mix_weight(m, y, x);
#pragma unroll
        for (int c = 0; c < 3; ++c) vd[c] = stem_mix_blend(w, a[c], o[c]);
      } else {
        rrc_vpass(p, own, y - ya, x, vd);
      }
    }
    rrc_store<OutT>(out, ((long)b * p.Hs + i) * p.Ws + j, v);
  }
}

// ------------------------------------------------------------------------------ launcher
static thread_local int t_last_form = 0, t_last_band = 0;
void stem_note_launch(int form, int band) { t_last_form = form; t_last_band = band; }
void stem_last_launch(int* form, int* band) { *form = t_last_form; *band = t_last_band; }
int g_stem_rrc_band = 0;
constexpr int RRC_MAX_BAND = 8;
constexpr int RRC_LDS = 32 << 10, RRC_LDS_MIX = 64 << 10;   // per workgroup: 5 / 2 workgroups of a CU's 160 KB

template <typename OutT>
static const char* stem_rrc_go(const StemParams& p, OutT* out, hipStream_t s) {
  if (!p.rrc) return "stem_s2d: mode 3 needs the rrc box table";
  if ((2L * p.Hc + 1) * p.Hin >= (1L << 31) || (2L * p.Wc + 1) * p.Win >= (1L << 31))
    return "stem_s2d: rrc coordinates overflow 32 bits";
  const long npix = (long)p.B * p.Hs * p.Ws;
  // the tallest band whose worst-case box (the whole source) fits the LDS budget
  const int RAWW = (p.Win * 3) / 4 + 2;
  int R = 0, SPAN = 0;
  long bytes = 0;
  if (g_stem_variant == 1 && p.in_u8) {
    for (R = g_stem_rrc_band > 0 ? (g_stem_rrc_band < RRC_MAX_BAND ? g_stem_rrc_band : RRC_MAX_BAND) : RRC_MAX_BAND; R > 0; --R) {
      SPAN = (int)lmin(((2L * R - 1) * p.Hin) / p.Hc + 3, p.Hin);
      bytes = ((long)SPAN * RAWW + (long)SPAN * p.Wc * 3 + p.Wc * 3 + 2 * R * 3) * 4 * (p.mix ? 2 : 1);
      if (bytes <= (p.mix ? RRC_LDS_MIX : RRC_LDS)) break;
    }
  }
  if (R > 0) {
    const int nbands = (p.Hs + R - 1) / R;
    auto k = p.mix ? stem_rrc_band_kernel<OutT, true> : stem_rrc_band_kernel<OutT, false>;
    hipLaunchKernelGGL(k, dim3(p.B * nbands), dim3(RRC_THREADS), (size_t)bytes, s, p, out, R, SPAN, RAWW, nbands,
                       fdiv_magic(p.Ws));
    stem_note_launch(2, R);
  } else {
    const int grid = (int)lmin((npix + 255) / 256, 16384);
    auto k = p.mix ? stem_rrc_pix_kernel<OutT, true> : stem_rrc_pix_kernel<OutT, false>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, s, p, out, (int)npix, fdiv_magic(p.Ws), fdiv_magic(p.Hs));
    stem_note_launch(0, 0);
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

const char* stem_rrc_launch(const StemParams& p, void* out, int out_f32, hipStream_t s) {
  if (p.aug) return stem_aug_launch(p, out, out_f32, s);        // [B][16] RandAugment rows: stem_aug.hip
  if (p.antialias) return stem_aa_launch(p, out, out_f32, s);   // triangle-filter forms: stem_aa.hip
  return out_f32 ? stem_rrc_go<float>(p, reinterpret_cast<float*>(out), s)
                 : stem_rrc_go<uint16_t>(p, reinterpret_cast<uint16_t*>(out), s);
}

}  // namespace pddl
