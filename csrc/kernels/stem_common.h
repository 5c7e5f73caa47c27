// Device helpers shared by the stem preprocess kernels (eltwise.hip, stem_rrc.hip).
#pragma once
#include "common.h"
#include "kernels.h"

namespace pddl {

// Mixup / CutMix (MIX forms; p.mix is the per-image table [B][8] of kernels.h): image b's pixel
// becomes w*A_b + (1 - w)*A_partner with w = 0 inside the row's box and w = w_pix outside, both
// A's being stem_pix values (each image's own flip, the batch's crop).  The partner is clamped to
// [0, B) and the box to the image, so a bad table gives a wrong picture, never a stray read.
struct StemMix { int pb, y0, x0, y1, x1; float w; };
__device__ __forceinline__ StemMix stem_mix_row(const StemParams& p, int b) {
  const int32_t* r = p.mix + (long)b * 8;
  StemMix m;
  m.pb = min(max(r[0], 0), p.B - 1);
  m.y0 = min(max(r[1], 0), p.Hc); m.x0 = min(max(r[2], 0), p.Wc);
  m.y1 = min(max(r[3], 0), p.Hc); m.x1 = min(max(r[4], 0), p.Wc);
  m.w = __int_as_float(r[5]);
  return m;
}
__device__ __forceinline__ float stem_mix_weight(const StemMix& m, int y, int x) {
  return (y >= m.y0 && y < m.y1 && x >= m.x0 && x < m.x1) ? 0.f : m.w;
}
// One explicit fma in every stem kernel (the row form stays bitwise equal to the per-pixel form);
// w = 1 returns a and w = 0 returns b bit for bit.
__device__ __forceinline__ float stem_mix_blend(float w, float a, float b) { return __fmaf_rn(w, a, (1.f - w) * b); }

}  // namespace pddl
