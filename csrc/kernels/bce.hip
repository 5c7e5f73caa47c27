// Sigmoid binary cross-entropy loss heads (gfx950): the training head (loss sum + accuracy count +
// bf16 / fp32 dlogits, mix table and label smoothing honoured) and the evaluation head (loss sum +
// top-1 / top-k hits).  The definition is in kernels.h ("Sigmoid binary cross-entropy").
//
// Unlike softmax, the loss needs neither the row maximum nor a normaliser, so a head is ONE streaming
// pass over its row.  Work split: one wave per example, four waves per workgroup.  A lane owns 8
// consecutive columns per iteration -- two 16-byte loads of fp32 logits in flight -- does the eight
// loss / sigmoid / argmax updates in registers and writes its 8 dlogits with one 16-byte store (bf16)
// or two (fp32).  At ncls = 1000, ldd = 1024 that is two iterations per lane; the group that
// straddles ncls reads its valid columns one by one and still stores 16 bytes, and the groups past
// it store zeros, so the K padding of the head dgrad falls out of the same stores.
// A row whose logits or dlogits do not start on a 16-byte boundary is walked one column per lane
// (`vec` false); both walks call bce_elem, so their dlogits are the same bits.  Columns >= ncls of
// `logits` are never read.  Per row: one wave reduction of the loss, one of the first-index argmax
// (training) or of the rank (evaluation), and one atomic per statistic.
#include "common.h"
#include "kernels.h"

namespace pddl {

constexpr float BCE_SERIES_BELOW = 0.015625f;   // 2^-6: the truncated series' next term, e^4/5, is < 2^-26

// log1p(e) for e = exp(-|z|) in [0, 1], given r = 1/(1 + e).  Below the cut-off the alternating
// series through e^4 (relative truncation error e^4/5 < 2^-26); above it log(u) with u = fl(1 + e)
// plus the first-order correction (e - (u - 1)) / u for what the rounding of 1 + e lost (u - 1 is
// exact there), so that neither branch loses relative accuracy in e.
__device__ __forceinline__ float bce_log1p(float e, float r) {
  if (e < BCE_SERIES_BELOW) return e * (1.f - e * (0.5f - e * (1.f / 3.f - e * 0.25f)));
  const float u = 1.f + e;
  return __logf(u) + (e - (u - 1.f)) * r;
}
// exp(-a) for a >= 0, to about an ulp at any a: sigmoid(z) ~ exp(z) for z << 0, and dlogits are held
// to a relative bound there, which exp2(x log2(e)) with a once-rounded product misses by |x| ulps.
// With n = rint(x log2(e)), the fraction f = x log2(e) - n, |f| <= 1/2, is taken from the exact product
// by fma (written out: whatever the compiler contracts, the product is never rounded before n is
// subtracted) plus x times the low part of log2(e); exp2 sees only f and ldexp scales, denormal results
// included.  (a > 128: the result is 0 either way; a NaN stays a NaN.)
__device__ __forceinline__ float bce_exp_neg(float a) {
  constexpr float LOG2E = 0x1.715476p+0f, LOG2E_LO = 0x1.4ae0bep-26f;
  const float x = -(a > 128.f ? 128.f : a);
  const float n = rintf(x * LOG2E);
  const float f = fmaf(x, LOG2E_LO, fmaf(x, LOG2E, -n));
  return ldexpf(__builtin_amdgcn_exp2f(f), (int)n);
}
// One element: returns l = max(z, 0) - t z + log1p(exp(-|z|)) and sets sig = sigmoid(z), both from
// the one exponential e = exp(-|z|) <= 1 (no overflow at any z).
__device__ __forceinline__ float bce_elem(float z, float t, float& sig) {
  const float e = bce_exp_neg(fabsf(z));
  const float r = 1.f / (1.f + e);
  sig = z >= 0.f ? r : e * r;
  return fmaxf(z, 0.f) - t * z + bce_log1p(e, r);
}

// The four target values of a row (kernels.h): t_j = own for j == lab, par for j == labp, both when
// the two labels coincide, none elsewhere.
struct BceRow {
  float none, own, par, both;
  int lab, labp;
  __device__ __forceinline__ float target(int j) const {
    return j == lab ? (j == labp ? both : own) : (j == labp ? par : none);
  }
};
// wl: the weight of the row's own label (1 without a mix table: keep*1 + spread is then the unmixed
// keep + spread, rounded once, and par == none, so labp = lab gives the unmixed row).
// thresh >= 0: each constant becomes (value > thresh ? 1 : 0).
__device__ __forceinline__ BceRow bce_row(int lab, int labp, float wl, float keep, float spread, float thresh) {
  const float wp = 1.f - wl;
  BceRow r;
  r.lab = lab, r.labp = labp;
  r.none = spread, r.own = keep * wl + spread, r.par = keep * wp + spread, r.both = keep * (wl + wp) + spread;
  if (thresh >= 0.f) {
    r.none = r.none > thresh ? 1.f : 0.f, r.own = r.own > thresh ? 1.f : 0.f;
    r.par = r.par > thresh ? 1.f : 0.f, r.both = r.both > thresh ? 1.f : 0.f;
  }
  return r;
}

// The walk over columns [0, ncls) of one row by one wave: f(j0, z, n) gets n <= 8 consecutive
// columns from j0 in z[0..n) (z[n..8) are zero).  vec: 8 columns per lane and iteration, two 16-byte
// loads for a whole group and single loads for the group that straddles ncls; otherwise one column
// per lane.  A lane's calls come with j0 increasing.
template <class F>
__device__ __forceinline__ void bce_walk(const float* __restrict__ row, int ncls, int lane, bool vec, F&& f) {
  float z[8];
  if (vec) {
    for (int j0 = lane * 8; j0 < ncls; j0 += 512) {
      const int n = min(8, ncls - j0);
      if (n == 8) {
        const float4 a = *reinterpret_cast<const float4*>(row + j0);
        const float4 b = *reinterpret_cast<const float4*>(row + j0 + 4);
        z[0] = a.x, z[1] = a.y, z[2] = a.z, z[3] = a.w, z[4] = b.x, z[5] = b.y, z[6] = b.z, z[7] = b.w;
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) z[i] = i < n ? row[j0 + i] : 0.f;
      }
      f(j0, z, n);
    }
  } else {
#pragma unroll
    for (int i = 1; i < 8; ++i) z[i] = 0.f;
    for (int j = lane; j < ncls; j += 64) {
      z[0] = row[j];
      f(j, z, 1);
    }
  }
}

__device__ __forceinline__ void bce_store8(uint16_t* p, const float* d) { *reinterpret_cast<uint4*>(p) = pack8(d); }
__device__ __forceinline__ void bce_store8(float* p, const float* d) {
  *reinterpret_cast<float4*>(p) = make_float4(d[0], d[1], d[2], d[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(d[4], d[5], d[6], d[7]);
}
__device__ __forceinline__ void bce_store1(uint16_t* p, float d) { *p = f2bf(d); }
__device__ __forceinline__ void bce_store1(float* p, float d) { *p = d; }
__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// T: the type of dlogits -- bf16_t (the bf16 engines) or float (the fp32 engines).  MIX: the mix
// table of kernels.h (the head gathers labels[partner] itself).  gk = gscale / ncls.
template <typename T, bool MIX>
__global__ void __launch_bounds__(256) sigmoid_bce_kernel(const float* __restrict__ logits, int ldl,
                                                          const int64_t* __restrict__ labels, int B, int ncls,
                                                          float gk, float keep, float spread, float thresh,
                                                          T* __restrict__ dl, int ldd, float* __restrict__ loss_sum,
                                                          float* __restrict__ correct,
                                                          const int32_t* __restrict__ mix) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* row = logits + (long)b * ldl;
  T* drow = dl + (long)b * ldd;
  const int lab = (int)labels[b];
  int labp = lab;
  float wl = 1.f;
  if (MIX) {
    labp = (int)labels[min(max(mix[(long)b * 8], 0), B - 1)];
    wl = __int_as_float(mix[(long)b * 8 + 6]);
  }
  const BceRow tr = bce_row(lab, labp, wl, keep, spread, thresh);
  const bool vec = aligned16(row) && aligned16(drow);
  const int per = vec ? 8 : 1;        // columns a call of the walk owns in dlogits
  float loss = 0.f, mx = -INFINITY;
  int amax = 0x7fffffff;
  bce_walk(row, ncls, lane, vec, [&](int j0, const float* z, int n) {
    float d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      d[i] = 0.f;
      if (i < n) {
        const float t = MIX ? tr.target(j0 + i) : (j0 + i == lab ? tr.own : tr.none);
        float sig;
        loss += bce_elem(z[i], t, sig);
        d[i] = (sig - t) * gk;
        if (z[i] > mx) { mx = z[i]; amax = j0 + i; }
      }
    }
    if (vec && j0 + 8 <= ldd) {
      bce_store8(drow + j0, d);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i < per && j0 + i < ldd) bce_store1(drow + j0 + i, d[i]);
    }
  });
  // the K padding [ncls, ldd) that the walk's stores did not reach
  if (vec) {
    const float zero[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j0 = ((ncls + 7) & ~7) + lane * 8; j0 < ldd; j0 += 512) {
      if (j0 + 8 <= ldd) {
        bce_store8(drow + j0, zero);
      } else {
        for (int j = j0; j < ldd; ++j) bce_store1(drow + j, 0.f);
      }
    }
  } else {
    for (int j = ncls + lane; j < ldd; j += 64) bce_store1(drow + j, 0.f);
  }
  loss = warp_sum(loss);
  // wave argmax (first index among equal maxima)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o, 64);
    const int oa = __shfl_xor(amax, o, 64);
    if (om > mx || (om == mx && oa < amax)) { mx = om; amax = oa; }
  }
  if (lane == 0) {
    unsafeAtomicAdd(loss_sum, loss / (float)ncls);
    unsafeAtomicAdd(correct, amax == (wl >= 0.5f ? lab : labp) ? 1.f : 0.f);
  }
}

// The evaluation head: eval_metrics_kernel's rank (eltwise.hip: equal logits ordered by index, so
// rank == 0 is the training head's "first argmax == label") and the loss of bce_elem, in one pass.
__global__ void __launch_bounds__(256) eval_metrics_bce_kernel(const float* __restrict__ logits, int ldl,
                                                               const int64_t* __restrict__ labels, int B, int ncls,
                                                               int k, float keep, float spread, float thresh,
                                                               float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* row = logits + (long)b * ldl;
  const int lab = (int)labels[b];
  const float vl = row[lab];
  const BceRow tr = bce_row(lab, lab, 1.f, keep, spread, thresh);
  float loss = 0.f;
  int rank = 0;
  bce_walk(row, ncls, lane, aligned16(row), [&](int j0, const float* z, int n) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i < n) {
        const int j = j0 + i;
        float sig;
        loss += bce_elem(z[i], j == lab ? tr.own : tr.none, sig);
        rank += (z[i] > vl || (z[i] == vl && j < lab)) ? 1 : 0;
      }
    }
  });
  loss = warp_sum(loss);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rank += __shfl_xor(rank, o, 64);
  if (lane == 0) {
    unsafeAtomicAdd(out + 0, loss / (float)ncls);
    unsafeAtomicAdd(out + 1, rank == 0 ? 1.f : 0.f);
    unsafeAtomicAdd(out + 2, rank < k ? 1.f : 0.f);
  }
}

namespace {
const char* bce_args_bad(float smoothing, float thresh) {
  if (!(smoothing >= 0.f && smoothing <= 1.f)) return "sigmoid_bce: smoothing outside [0, 1]";   // (or a NaN)
  if (!(thresh < 1.f)) return "sigmoid_bce: thresh is a NaN or >= 1 (negative: off)";
  return nullptr;
}
template <typename T>
const char* sigmoid_bce_launch_t(const float* logits, int ldl, const int64_t* labels, int B, int ncls, float gscale,
                                 T* dlogits, int ldd, float* loss_sum, float* correct, hipStream_t s, float smoothing,
                                 const int32_t* mix, float thresh) {
  if (ncls < 1 || ldl < ncls) return "sigmoid_bce: ldl < ncls";
  if (ldd < ncls) return "sigmoid_bce: ldd < ncls";
  if (const char* bad = bce_args_bad(smoothing, thresh)) return bad;
  if (B <= 0) return nullptr;
  const float keep = 1.f - smoothing, spread = smoothing / (float)ncls, gk = gscale / (float)ncls;
  auto kern = mix ? sigmoid_bce_kernel<T, true> : sigmoid_bce_kernel<T, false>;
  hipLaunchKernelGGL(kern, dim3((B + 3) / 4), dim3(256), 0, s, logits, ldl, labels, B, ncls, gk, keep, spread, thresh,
                     dlogits, ldd, loss_sum, correct, mix);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}
}  // namespace
const char* sigmoid_bce_launch(const float* logits, int ldl, const int64_t* labels, int B, int ncls, float gscale,
                               uint16_t* dlogits, int ldd, float* loss_sum, float* correct, hipStream_t s,
                               float smoothing, const int32_t* mix, float thresh) {
  return sigmoid_bce_launch_t(logits, ldl, labels, B, ncls, gscale, dlogits, ldd, loss_sum, correct, s, smoothing, mix,
                              thresh);
}
const char* sigmoid_bce_launch(const float* logits, int ldl, const int64_t* labels, int B, int ncls, float gscale,
                               float* dlogits, int ldd, float* loss_sum, float* correct, hipStream_t s,
                               float smoothing, const int32_t* mix, float thresh) {
  return sigmoid_bce_launch_t(logits, ldl, labels, B, ncls, gscale, dlogits, ldd, loss_sum, correct, s, smoothing, mix,
                              thresh);
}
const char* eval_metrics_bce_launch(const float* logits, int ldl, const int64_t* labels, int B, int ncls, int k,
                                    float* out, hipStream_t s, float smoothing, float thresh) {
  if (const char* bad = bce_args_bad(smoothing, thresh)) return bad;
  if (B <= 0) return nullptr;
  hipLaunchKernelGGL(eval_metrics_bce_kernel, dim3((B + 3) / 4), dim3(256), 0, s, logits, ldl, labels, B, ncls, k,
                     1.f - smoothing, smoothing / (float)ncls, thresh, out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

}  // namespace pddl
