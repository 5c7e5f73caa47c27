// Fused optimizers over the flat fp32 parameter buffer (gfx950).
//
// Adam follows TF/Keras ResourceApplyAdam exactly (reference: `optimizer='adam'` at
// imagenet-resnet50.py:62, `keras.optimizers.Adam(learning_rate=0.1*hvd.size())` at
// imagenet-resnet50-hvd.py:99): the bias correction is folded into the step
// size ("epsilon hat"):  lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t),
//   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= lr_t * m / (sqrt(v) + eps).
// SGD with momentum follows keras.optimizers.SGD:  v = mu v - lr g;  p += v  (Nesterov:
// p += mu v - lr g), with optional L2 weight decay folded into g.
// One launch updates all 25.6M parameters; 16-byte loads/stores per lane.
// LARS (large global batches) is momentum SGD with a per-layer trust ratio: two launches over a
// segment table of the same buffer, a norm pass and an update pass (below).
#include "common.h"
#include "kernels.h"

namespace pddl {

// Device-resident step hyper-parameters hs = {t, lr, lr_t}: one thread advances the step
// counter and derives the step size, so a captured training step (HIP graph) replays with
// the right bias correction and with learning-rate changes the host writes between replays.
__global__ void opt_hparams_kernel(float* hs, float b1, float b2, int adam) {
  const float t = hs[0] + 1.f;
  hs[0] = t;
  hs[2] = adam ? hs[1] * sqrtf(1.f - powf(b2, t)) / (1.f - powf(b1, t)) : hs[1];
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long n4, float lr_t, float b1, float b2, float eps, float gs,
                            const float* __restrict__ hs, const float* __restrict__ gn) {
  if (hs) lr_t = hs[2];
  if (gn) {   // (see grad_clip_finalize_kernel)
    if (gn[2] != 0.f) return;
    gs *= gn[1];
  }
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
#define ADAM1(c)                                              \
  {                                                           \
    const float gr = gg.c * gs;                               \
    mm.c = b1 * mm.c + (1.f - b1) * gr;                       \
    vv.c = b2 * vv.c + (1.f - b2) * gr * gr;                  \
    pp.c -= lr_t * mm.c / (sqrtf(vv.c) + eps);                \
  }
    ADAM1(x) ADAM1(y) ADAM1(z) ADAM1(w)
#undef ADAM1
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
}

// Parameter-server form with the bf16 wire (--ps-wire bf16): the gradient arrives in bf16
// (the worker's mailbox push) and the update also writes the bf16 snapshot of the new
// parameters that the pulls copy (half the xGMI bytes both ways; the PS keeps fp32 master
// weights and Adam slots).  Same arithmetic as adam_kernel.
__global__ void adam_bf16_wire_kernel(float* __restrict__ p, const uint16_t* __restrict__ g, float* __restrict__ m,
                                      float* __restrict__ v, uint16_t* __restrict__ snap, long n4, float lr_t,
                                      float b1, float b2, float eps) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const uint2 gb = reinterpret_cast<const uint2*>(g)[i];
    const float4 gg = make_float4(__uint_as_float(gb.x << 16), __uint_as_float(gb.x & 0xffff0000u),
                                  __uint_as_float(gb.y << 16), __uint_as_float(gb.y & 0xffff0000u));
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
#define ADAM1(c)                                              \
  {                                                           \
    const float gr = gg.c;                                    \
    mm.c = b1 * mm.c + (1.f - b1) * gr;                       \
    vv.c = b2 * vv.c + (1.f - b2) * gr * gr;                  \
    pp.c -= lr_t * mm.c / (sqrtf(vv.c) + eps);                \
  }
    ADAM1(x) ADAM1(y) ADAM1(z) ADAM1(w)
#undef ADAM1
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    reinterpret_cast<uint2*>(snap)[i] = make_uint2(pack2(pp.x, pp.y), pack2(pp.z, pp.w));
  }
}

__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mom, long n4,
                           float lr, float mu, float wd, int nesterov, float gs, const float* __restrict__ hs,
                           const float* __restrict__ gn) {
  if (hs) lr = hs[2];
  if (gn) {
    if (gn[2] != 0.f) return;
    gs *= gn[1];
  }
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 vv = reinterpret_cast<float4*>(mom)[i];
#define SGD1(c)                                               \
  {                                                           \
    const float gr = gg.c * gs + wd * pp.c;                   \
    vv.c = mu * vv.c - lr * gr;                               \
    pp.c += nesterov ? (mu * vv.c - lr * gr) : vv.c;          \
  }
    SGD1(x) SGD1(y) SGD1(z) SGD1(w)
#undef SGD1
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(mom)[i] = vv;
  }
}

// Scheduled form of opt_hparams_kernel.  hs = {t, lr, lr_t, lr_sched, warmup_steps, total_steps,
// end_lr, -}: linear warm-up from 0 to lr over warmup_steps, polynomial decay (power 2) to end_lr
// at total_steps, end_lr after that.  One thread per step, so the arithmetic is done in double:
// the fp32 result is then the correctly rounded host formula, whatever powf would have lost in
// 1 - b2^t at small t.  hs[3] keeps the scheduled rate before Adam's bias correction.
__global__ void opt_hparams_sched_kernel(float* hs, float b1, float b2, int adam) {
  const float t = hs[0] + 1.f;
  hs[0] = t;
  const double lr = hs[1], wu = hs[4], tot = hs[5], end_lr = hs[6], td = t;
  double s;
  if (td <= wu) {
    s = lr * td / wu;
  } else if (td < tot) {
    const double rem = (tot - td) / (tot - wu);
    s = end_lr + (lr - end_lr) * rem * rem;
  } else {
    s = end_lr;
  }
  hs[3] = (float)s;
  hs[2] = (float)(adam ? s * sqrt(1.0 - pow((double)b2, td)) / (1.0 - pow((double)b1, td)) : s);
}

// ---- LARS (You et al.; the MLPerf ResNet-50 form) over the segment table -------------------
// Every replica runs this on identical all-reduced gradients and nothing re-synchronises the
// parameters afterwards, so the norms must come out bit-identical on every replica and every
// run: no atomics, no arrival-order combine.  Chunk c of segment s is summed by one block in a
// fixed thread -> wave -> block tree, and every block of the update pass folds its segment's
// partials in the same fixed order (lane j takes partials j, j+256, ... in index order, then
// the same tree).  The order is a pure function of the segment table and the chunk size.

// Segment of global chunk b: the last s with segs[s].chunk0 <= b (chunk0 ascends from 0).
__device__ __forceinline__ int lars_find_seg(const LarsSeg* __restrict__ segs, int nseg, int b) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].chunk0 <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Block-wide sums of (a, b) in a fixed order; the result is valid in every thread.
__device__ __forceinline__ float2 lars_block_sum2(float a, float b, float2* red) {
  a = warp_sum(a);
  b = warp_sum(b);
  const int wave = threadIdx.x >> 6;
  __syncthreads();   // (red may still be read from a previous call)
  if ((threadIdx.x & 63) == 0) red[wave] = make_float2(a, b);
  __syncthreads();
  float2 r = red[0];
#pragma unroll
  for (int w = 1; w < 4; w++) { r.x += red[w].x; r.y += red[w].y; }
  return r;
}

__global__ __launch_bounds__(256) void lars_norm_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                        const LarsSeg* __restrict__ segs, int nseg, int chunk,
                                                        float gs, float2* __restrict__ partials,
                                                        const float* __restrict__ gn) {
  __shared__ float2 red[4];
  if (gn) {
    if (gn[2] != 0.f) return;   // (skipped step: the update pass returns before it reads the partials)
    gs *= gn[1];
  }
  const int b = blockIdx.x;
  const LarsSeg sg = segs[lars_find_seg(segs, nseg, b)];
  if (!sg.adapt) return;   // (its partials are never read)
  const long start = (long)(b - sg.chunk0) * chunk;
  const int n4 = (int)lmin((long)chunk, sg.size - start) >> 2;
  const float4* p4 = reinterpret_cast<const float4*>(p + sg.off + start);
  const float4* g4 = reinterpret_cast<const float4*>(g + sg.off + start);
  float sw = 0.f, sgg = 0.f;
  for (int i = threadIdx.x; i < n4; i += 256) {
    const float4 w = p4[i];
    float4 d = g4[i];
    d.x *= gs; d.y *= gs; d.z *= gs; d.w *= gs;
    sw += (w.x * w.x + w.y * w.y) + (w.z * w.z + w.w * w.w);
    sgg += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
  }
  const float2 r = lars_block_sum2(sw, sgg, red);
  if (threadIdx.x == 0) partials[b] = r;
}

__global__ __launch_bounds__(256) void lars_update_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ v, const LarsSeg* __restrict__ segs,
                                                          int nseg, int chunk, const float2* __restrict__ partials,
                                                          float* __restrict__ ratios, float lr, float mu, float wd,
                                                          float eta, float eps, float gs,
                                                          const float* __restrict__ hs,
                                                          const float* __restrict__ gn) {
  __shared__ float2 red[4];
  if (hs) lr = hs[2];
  if (gn) {
    if (gn[2] != 0.f) return;   // (the ratios of the last applied step stay)
    gs *= gn[1];
  }
  const int b = blockIdx.x;
  const int s = lars_find_seg(segs, nseg, b);
  const LarsSeg sg = segs[s];
  float ratio = 1.f;
  if (sg.adapt) {
    const int m = (int)((sg.size + (long)chunk - 1) / chunk);
    float sw = 0.f, sgg = 0.f;
    for (int j = threadIdx.x; j < m; j += 256) {
      const float2 q = partials[sg.chunk0 + j];
      sw += q.x;
      sgg += q.y;
    }
    const float2 r = lars_block_sum2(sw, sgg, red);
    const float wn = sqrtf(r.x), gn = sqrtf(r.y);
    if (wn > 0.f && gn > 0.f) ratio = eta * wn / (gn + wd * wn + eps);
  } else {
    wd = 0.f;   // biases and BN parameters: no decay, no adaptation
  }
  if (b == sg.chunk0 && threadIdx.x == 0) ratios[s] = ratio;
  const float step = lr * ratio;
  const long start = (long)(b - sg.chunk0) * chunk;
  const int n4 = (int)lmin((long)chunk, sg.size - start) >> 2;
  float4* p4 = reinterpret_cast<float4*>(p + sg.off + start);
  const float4* g4 = reinterpret_cast<const float4*>(g + sg.off + start);
  float4* v4 = reinterpret_cast<float4*>(v + sg.off + start);
  for (int i = threadIdx.x; i < n4; i += 256) {
    float4 pp = p4[i];
    const float4 gg = g4[i];
    float4 vv = v4[i];
#define LARS1(c)                                              \
  {                                                           \
    const float u = gg.c * gs + wd * pp.c;                    \
    vv.c = mu * vv.c + step * u;                              \
    pp.c -= vv.c;                                             \
  }
    LARS1(x) LARS1(y) LARS1(z) LARS1(w)
#undef LARS1
    p4[i] = pp;
    v4[i] = vv;
  }
}

// ---- global-norm gradient clipping and non-finite skip ------------------------------------
// The whole-buffer form of the LARS norm pass, under the same rule (above lars_find_seg):
// replicas clip identical all-reduced gradients and nothing re-synchronises the parameters
// afterwards, so the norm comes out bit-identical everywhere.  Block b sums (gs g)^2 over floats
// [b chunk, min(n, (b + 1) chunk)) in the fixed thread -> wave -> block tree and writes
// partials[b]; one block then folds the partials (lane j takes j, j + 256, ... in index order,
// then the same tree).  No atomics: the order is a pure function of (n, chunk), never of the
// grid cap, the CU count or arrival order.
__global__ __launch_bounds__(256) void grad_sqsum_kernel(const float* __restrict__ g, long n, int chunk, float gs,
                                                         float* __restrict__ partials) {
  __shared__ float2 red[4];
  const long start = (long)blockIdx.x * chunk;
  const int n4 = (int)lmin((long)chunk, n - start) >> 2;
  const float4* g4 = reinterpret_cast<const float4*>(g + start);
  float sgg = 0.f;
  for (int i = threadIdx.x; i < n4; i += 256) {
    float4 d = g4[i];
    d.x *= gs; d.y *= gs; d.z *= gs; d.w *= gs;
    sgg += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
  }
  const float2 r = lars_block_sum2(sgg, 0.f, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = r.x;
}

// gn = {norm, scale, skip, clip, skip_enabled, clipped steps, skipped steps, -}: slots 0..2 and
// the two counters are written here, slots 3 and 4 by the host.  norm = sqrt(sum (gs g)^2) of
// this step before clipping; scale = clip / norm when clip > 0 and norm > clip, else exactly
// 1.0f (Keras: clip / max(norm, clip)), so gs * scale is bitwise gs on a step that is not
// clipped; skip = 1 when skip_enabled and the norm is not finite.  The sum of squares is
// non-finite exactly when some gs g is NaN or +-inf or the sum overflows fp32, so the norm is
// also the non-finite detector.  The update kernels that are given gn multiply scale into gs
// and return at once when skip is set: p, the slots and the LARS ratios stay bit-unchanged.
// hs[0] still advances on a skipped step (the hparams kernel runs before this one), so the
// host and device step counts never diverge.  A NaN norm compares false with clip: scale 1.
__global__ __launch_bounds__(256) void grad_clip_finalize_kernel(const float* __restrict__ partials, int m,
                                                                 float* __restrict__ gn) {
  __shared__ float2 red[4];
  float sgg = 0.f;
  for (int j = threadIdx.x; j < m; j += 256) sgg += partials[j];
  const float2 r = lars_block_sum2(sgg, 0.f, red);
  if (threadIdx.x == 0) {
    const float norm = sqrtf(r.x), clip = gn[3];
    const float scale = (clip > 0.f && norm > clip) ? clip / norm : 1.0f;
    const bool skip = gn[4] != 0.f && !isfinite(norm);
    gn[0] = norm;
    gn[1] = scale;
    gn[2] = skip ? 1.f : 0.f;
    if (scale < 1.0f && !skip) gn[5] += 1.f;   // (a skipped step applies nothing, clipped or not)
    if (skip) gn[6] += 1.f;
  }
}

__global__ void scale_kernel(float* __restrict__ x, long n, float a) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) x[i] *= a;
}
__global__ void cast_bf16_kernel(const float* __restrict__ x, uint16_t* __restrict__ y, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = f2bf(x[i]);
}
__global__ void cast_f32_kernel(const uint16_t* __restrict__ x, float* __restrict__ y, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = bf2f(x[i]);
}

// Gradient accumulation over k micro-batches (train/accum.py).  mode 0 store: acc = g (bitwise);
// 1 add: acc += g; 2 fold: g += acc, in place, so the all-reduce and the optimizers keep reading
// the gradient buffer.  A pure streaming pass: 16 bytes per lane, two float4 per operand in
// flight per lane, a grid-stride loop over a grid sized from the CU count.  Bucket slices start
// at any float offset: block 0 peels a scalar head up to acc's next 16-byte boundary and the
// scalar tail; vec = 0 (acc and g misaligned against each other) takes every element scalar.
constexpr int kAccumBlock = 256, kAccumBlocksPerCu = 8, kAccumUnroll = 2;

// dst = src (ADD = 0) or dst += src; fold is add with the operands swapped.
template <int ADD>
__device__ __forceinline__ void grad_accum_body(float* __restrict__ dst, const float* __restrict__ src, long n,
                                                int vec) {
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
  if (!vec) {
    for (long i = tid; i < n; i += nth) dst[i] = ADD ? dst[i] + src[i] : src[i];
    return;
  }
  const long head = lmin((long)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) >> 2, n);
  const long n4 = (n - head) >> 2, tail0 = head + (n4 << 2);
  if (blockIdx.x == 0) {   // at most 3 + 3 scalars: lanes 0..2 the head, lanes 64..66 the tail
    long k = -1;
    if ((long)threadIdx.x < head) k = threadIdx.x;
    else if (threadIdx.x >= 64 && tail0 + (threadIdx.x - 64) < n) k = tail0 + (threadIdx.x - 64);
    if (k >= 0) dst[k] = ADD ? dst[k] + src[k] : src[k];
  }
  v4f* d4 = reinterpret_cast<v4f*>(dst + head);
  const v4f* s4 = reinterpret_cast<const v4f*>(src + head);
  long i = tid;
  for (; i + nth < n4; i += 2 * nth) {   // both lines' loads issue before the first store
    const long j = i + nth;
    const v4f x0 = s4[i], x1 = s4[j];
    if (ADD) {
      const v4f y0 = d4[i], y1 = d4[j];
      d4[i] = y0 + x0;
      d4[j] = y1 + x1;
    } else {
      d4[i] = x0;
      d4[j] = x1;
    }
  }
  if (i < n4) d4[i] = ADD ? d4[i] + s4[i] : s4[i];
}
__global__ __launch_bounds__(kAccumBlock) void grad_accum_kernel(float* acc, float* g, long n, int mode, int vec) {
  if (mode == 0) grad_accum_body<0>(acc, g, n, vec);
  else if (mode == 1) grad_accum_body<1>(acc, g, n, vec);
  else grad_accum_body<1>(g, acc, n, vec);
}

static int grid_of(long n) { return (int)lmin((n + 255) / 256, 4096); }
#define LAUNCH_RET                                        \
  {                                                       \
    hipError_t e = hipGetLastError();                     \
    return e == hipSuccess ? nullptr : hipGetErrorString(e); \
  }

const char* opt_hparams_launch(float* hs, float b1, float b2, int adam, hipStream_t s) {
  hipLaunchKernelGGL(opt_hparams_kernel, dim3(1), dim3(1), 0, s, hs, b1, b2, adam);
  LAUNCH_RET
}
const char* adam_launch(float* p, const float* g, float* m, float* v, long n, float lr_t, float b1, float b2,
                        float eps, float gscale, const float* hs, const float* gn, hipStream_t s) {
  if (n % 4) return "adam: n must be a multiple of 4";
  hipLaunchKernelGGL(adam_kernel, dim3(grid_of(n / 4)), dim3(256), 0, s, p, g, m, v, n / 4, lr_t, b1, b2, eps, gscale,
                     hs, gn);
  LAUNCH_RET
}
const char* sgd_launch(float* p, const float* g, float* mom, long n, float lr, float momentum, float wd, int nesterov,
                       float gscale, const float* hs, const float* gn, hipStream_t s) {
  if (n % 4) return "sgd: n must be a multiple of 4";
  hipLaunchKernelGGL(sgd_kernel, dim3(grid_of(n / 4)), dim3(256), 0, s, p, g, mom, n / 4, lr, momentum, wd, nesterov,
                     gscale, hs, gn);
  LAUNCH_RET
}
const char* opt_hparams_sched_launch(float* hs, float b1, float b2, int adam, hipStream_t s) {
  hipLaunchKernelGGL(opt_hparams_sched_kernel, dim3(1), dim3(1), 0, s, hs, b1, b2, adam);
  LAUNCH_RET
}
// Checks the host copy of the segment table (the device copy holds the same bytes) and returns
// the number of chunks, or -1 with *err set.
long lars_check_table(const LarsSeg* segs, int nseg, long n, int chunk, const char** err) {
  *err = nullptr;
  if (nseg < 1) { *err = "lars: empty segment table"; return -1; }
  if (chunk < 4 || chunk % 4) { *err = "lars: chunk must be a positive multiple of 4"; return -1; }
  long chunks = 0, end = 0;
  for (int i = 0; i < nseg; i++) {
    const LarsSeg& sg = segs[i];
    if (sg.off % 4 || sg.size % 4) { *err = "lars: segment offsets and sizes must be multiples of 4"; return -1; }
    if (sg.size <= 0 || sg.off < end || (long)sg.off + sg.size > n) {
      *err = "lars: segments must be non-empty, ascending, disjoint and inside the buffer";
      return -1;
    }
    if (sg.chunk0 != chunks) { *err = "lars: chunk0 is not the running chunk count for this chunk size"; return -1; }
    end = (long)sg.off + sg.size;
    chunks += (sg.size + (long)chunk - 1) / chunk;
    if (chunks > 0x7fffffffL) { *err = "lars: too many chunks"; return -1; }
  }
  return chunks;
}
const char* lars_launch(float* p, const float* g, float* v, long n, const LarsSeg* segs_dev, const LarsSeg* segs_host,
                        int nseg, int chunk, float* partials, long partials_floats, float* ratios, long ratios_floats,
                        float lr, float momentum, float wd, float eta, float eps, float gscale, const float* hs,
                        const float* gn, hipStream_t s) {
  const char* err;
  const long chunks = lars_check_table(segs_host, nseg, n, chunk, &err);
  if (chunks < 0) return err;
  if (partials_floats < 2 * chunks) return "lars: partials buffer smaller than 2 floats per chunk";
  if (ratios_floats < nseg) return "lars: ratio buffer smaller than the segment table";
  hipLaunchKernelGGL(lars_norm_kernel, dim3((unsigned)chunks), dim3(256), 0, s, p, g, segs_dev, nseg, chunk, gscale,
                     reinterpret_cast<float2*>(partials), gn);
  hipLaunchKernelGGL(lars_update_kernel, dim3((unsigned)chunks), dim3(256), 0, s, p, g, v, segs_dev, nseg, chunk,
                     reinterpret_cast<const float2*>(partials), ratios, lr, momentum, wd, eta, eps, gscale, hs, gn);
  LAUNCH_RET
}
const char* grad_norm_launch(const float* g, long n, float gscale, int chunk, float* partials, long partials_floats,
                             float* gn, hipStream_t s) {
  if (n <= 0 || n % 4) return "grad_norm: n must be a positive multiple of 4";
  if (chunk < 4 || chunk % 4) return "grad_norm: chunk must be a positive multiple of 4";
  const long chunks = (n + (long)chunk - 1) / chunk;
  if (chunks > 0x7fffffffL) return "grad_norm: too many chunks";
  if (partials_floats < chunks) return "grad_norm: partials buffer smaller than one float per chunk";
  hipLaunchKernelGGL(grad_sqsum_kernel, dim3((unsigned)chunks), dim3(256), 0, s, g, n, chunk, gscale, partials);
  hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(256), 0, s, partials, (int)chunks, gn);
  LAUNCH_RET
}
const char* scale_launch(float* x, long n, float a, hipStream_t s) {
  hipLaunchKernelGGL(scale_kernel, dim3(grid_of(n)), dim3(256), 0, s, x, n, a);
  LAUNCH_RET
}
// Floats one full sweep of the accumulation grid covers on the current device (tests pick
// lengths around it).
long grad_accum_sweep() { return (long)num_cus() * kAccumBlocksPerCu * kAccumBlock * 4 * kAccumUnroll; }
const char* grad_accum_launch(float* acc, float* g, long n, int mode, hipStream_t s) {
  if (mode < 0 || mode > 2) return "grad_accum: mode is 0 (store), 1 (add) or 2 (fold)";
  if (n < 0) return "grad_accum: negative length";
  if (n == 0) return nullptr;
  if ((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(g)) & 3) return "grad_accum: pointers are not float-aligned";
  if (acc < g + n && g < acc + n) return "grad_accum: acc and g overlap";
  // (slices at one offset of equally aligned buffers share their misalignment; anything else goes scalar)
  const int vec = ((reinterpret_cast<uintptr_t>(acc) ^ reinterpret_cast<uintptr_t>(g)) & 15) == 0;
  const long per_block = (long)kAccumBlock * (vec ? 4 : 1);
  const long grid = lmin((n + per_block - 1) / per_block, (long)num_cus() * kAccumBlocksPerCu);
  hipLaunchKernelGGL(grad_accum_kernel, dim3((unsigned)grid), dim3(kAccumBlock), 0, s, acc, g, n, mode, vec);
  LAUNCH_RET
}
const char* adam_bf16_wire_launch(float* p, const uint16_t* g, float* m, float* v, uint16_t* snap, long n, float lr_t,
                                  float b1, float b2, float eps, hipStream_t s) {
  if (n % 4) return "adam_bf16_wire: n must be a multiple of 4";
  hipLaunchKernelGGL(adam_bf16_wire_kernel, dim3(grid_of(n / 4)), dim3(256), 0, s, p, g, m, v, snap, n / 4, lr_t, b1,
                     b2, eps);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}
const char* cast_bf16_launch(const float* x, uint16_t* y, long n, hipStream_t s) {
  hipLaunchKernelGGL(cast_bf16_kernel, dim3(grid_of(n)), dim3(256), 0, s, x, y, n);
  LAUNCH_RET
}
const char* cast_f32_launch(const uint16_t* x, float* y, long n, hipStream_t s) {
  hipLaunchKernelGGL(cast_f32_kernel, dim3(grid_of(n)), dim3(256), 0, s, x, y, n);
  LAUNCH_RET
}

}  // namespace pddl
