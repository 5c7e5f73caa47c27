// Device helpers shared by the stem preprocess kernels (eltwise.hip, stem_rrc.hip, stem_aa.hip).
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

// Random-resized-crop (mode 3; kernels.h, StemParams::rrc), shared by stem_rrc.hip and stem_aa.hip.
struct RrcBox { int y0, x0, h, w; };
__device__ __forceinline__ RrcBox rrc_box(const StemParams& p, int b) {
  const int32_t* r = p.rrc + (long)b * 4;
  RrcBox q;
  q.y0 = min(max(r[0], 0), p.Hin - 1); q.x0 = min(max(r[1], 0), p.Win - 1);
  q.h = min(max(r[2], 1), p.Hin - q.y0); q.w = min(max(r[3], 1), p.Win - q.x0);
  return q;
}
// Output index o of N along a box side of n source pixels: the two taps (box-relative) and the weight.
struct RrcTap { int t0, t1; float f; };
__device__ __forceinline__ RrcTap rrc_tap(int o, int n, int N) {
  const int den = 2 * N, num = (2 * o + 1) * n - N;   // num > -den: the quotient below is floor(num / den)
  const int t = (num + den) / den - 1;
  RrcTap r;
  r.f = __fdiv_rn((float)(num - t * den), (float)den);
  r.t0 = min(max(t, 0), n - 1); r.t1 = min(max(t + 1, 0), n - 1);
  return r;
}
__device__ __forceinline__ float rrc_lerp(float a, float b, float f) { return __fmaf_rn(b - a, f, a); }

template <typename OutT> __device__ __forceinline__ void rrc_store(OutT* out, long q, const float* v);
template <> __device__ __forceinline__ void rrc_store<uint16_t>(uint16_t* out, long q, const float* v) {
  uint4* o = reinterpret_cast<uint4*>(out + q * 16);
  o[0] = pack8(v);
  o[1] = pack8(v + 8);
}
template <> __device__ __forceinline__ void rrc_store<float>(float* out, long q, const float* v) {
  float4* o = reinterpret_cast<float4*>(out + q * 16);
#pragma unroll
  for (int d = 0; d < 4; ++d) o[d] = make_float4(v[d * 4], v[d * 4 + 1], v[d * 4 + 2], v[d * 4 + 3]);
}

}  // namespace pddl
