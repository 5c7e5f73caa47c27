// Cross-layer fusion at a bottleneck boundary (gfx950), two forms: 64 channels wide (stage 2, below)
// and 128 channels wide (stage 3: c3c1_s3_kernel, further down, with its own header).
//
// The 64-channel form: conv3 of block b (1x1, 64 -> 256, folded BN, + residual, ReLU) and conv1
// of block b + 1 (1x1, 256 -> 64, folded BN, ReLU) in one launch.  Block b's 256-channel output is
// still written (it is block b + 1's residual and the backward's input), but block b + 1's conv1
// reads it from LDS instead of HBM: at b2560 that is one 4.1 GB read fewer per boundary (stage 2:
// conv2_block1 -> 2 and 2 -> 3; conv2_block3 feeds the stride-2 projection block and keeps the
// separate launches).  Two kernels:
//
// c3c1_kernel, the plain boundary (conv2_block2 -> 3).  A workgroup owns 64 rows (pixels), 4 waves:
//   phase 1  out[64][256] = y2[64][64] . W3^T  -- wave w: output channels [64 w, 64 w + 64)
//   epilogue relu(acc * scale3 + shift3 (+ res)) -> bf16 into an LDS tile [64][256], then row stores
//            of that tile (+ the ReLU bits of the block output)
//   phase 2  y1[64][64] = out[64][256] . W1^T -- wave w: channels [16 w, 16 w + 16), K = 256 from LDS
//   epilogue relu(acc * scale1 + shift1) -> bf16 -> row stores (+ ReLU bits)
// Both MFMA phases run with the weights as the A operand (fragments loaded once per workgroup from
// L2 into registers), so a lane's accumulator holds 4 consecutive channels of one pixel and the
// epilogues write 8-byte chunks; the residual tile is DMA'd into the output tile's LDS at the start
// and each lane reads its 8 bytes of it where it then writes its 8 bytes of output.  LDS: 8 KiB A
// tile + 32 KiB output tile.
//
// c3c1_s2_kernel, the dual form (conv2_block1 -> 2, out of the stride-1 projection block): phase 1
// is the block's fused conv3 + shortcut GEMM, out = relu(scale ([y2 | x] . Wf^T) + shift) with
// Wf [256][64 + 64] (both BN scales folded in), no residual, and the block input x as a second A
// tile: k-steps 0-1 read y2's tile, 2-3 x's, in the dual-source igemm's order.  Built like the
// 128-channel form: a persistent grid (one 8-wave workgroup per CU, tiles b, b + G, ...), both
// weight matrices in registers for the whole launch, two LDS stages (two A tiles + output tile)
// with the next tile's LDS-DMA issued before phase 1, the folded BN scale / shift in LDS, every LDS
// access of the tile loop inline asm.  Wave w works on channel group cg = w & 3 of row half
// rh = w >> 2: phase 1 channels [64 cg, + 64) of rows [32 rh, + 32), phase 2 channels [16 cg, + 16)
// of the same rows.  LDS 2 x (16 + 32) KiB stages + the 2.5 KiB table = 100,864 B; 192 VGPRs,
// no scratch, 2 waves per SIMD (-Rpass-analysis=kernel-resource-usage).  (An unpipelined
// dual form had measured no gain, 2.77 ms against 1.87 + 0.90 ms at b2560, profiles/r4_c3c1.txt:
// a latency figure, not a byte limit.)
//
// Same arithmetic and k order as the igemm epilogues (fp32 scale / shift / residual, one bf16
// rounding, k ascending in steps of 32 on the same MFMA), so the outputs are those of the separate
// launches bit for bit (tests/test_gpu_c3c1_s2.py).
// Reference: the conv*_block*_3_conv -> add -> relu -> conv*_block*_1_conv chain of the Keras
// ResNet50 (imagenet-resnet50.py:56).
#include "common.h"
#include "kernels.h"

namespace pddl {

namespace {
constexpr int CC_BM = 64;   // rows per workgroup of c3c1_kernel
constexpr int C2_MT = 64;   // rows per tile of c3c1_s2_kernel
// LDS swizzles: [rows][128 B] A tiles -- chunk ^ ((row >> 1) & 7) (igemm / conv3x3c64 images);
// [rows][512 B] output tile -- chunk ^ (row & 15): 16 consecutive rows at one chunk hit 16 distinct
// 16-byte slots of the 256-byte bank row (a 512-byte row pitch is a whole number of bank rows)
__device__ __forceinline__ int cc_sw(int row) { return (row >> 1) & 7; }

typedef unsigned int cc_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ cc_v4u cc_read16(uint32_t a) {
  cc_v4u r;
  asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(a) : "memory");
  return r;
}
__device__ __forceinline__ uint2 cc_read8(uint32_t a) {
  uint2 r;
  asm volatile("ds_read_b64 %0, %1" : "=v"(r) : "v"(a) : "memory");
  return r;
}
__device__ __forceinline__ void cc_write8(uint32_t a, uint2 v) {
  asm volatile("ds_write_b64 %0, %1" ::"v"(a), "v"(v) : "memory");
}
}  // namespace

__global__ void __launch_bounds__(256, 2) c3c1_kernel(C3C1Params p) {
  constexpr int K1 = 64;
  constexpr int A_BYTES = CC_BM * 128;                 // the 64-channel source tile
  __shared__ __attribute__((aligned(16))) char smem[A_BYTES + CC_BM * 512];
  char* at = smem;                                     // A1 tile; later the y1 staging tile
  char* ot = smem + A_BYTES;                           // block-b output tile [64][512 B]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kq = lane >> 4;
  const int m0 = blockIdx.x * CC_BM;

  // ---- A tile by LDS-DMA: 8 pieces of 8 rows, 2 per wave
  {
    const __amdgpu_buffer_rsrc_t ra = make_rsrc_at(p.a, (long)m0 * 64, (long)p.M * 64);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int pc = wave * 2 + q, row = pc * 8 + (lane >> 3);
      const int ch = (lane & 7) ^ cc_sw(row);
      buf_lds16(ra, LDS_PTR(at + pc * 1024), m0 + row < p.M ? (uint32_t)((row * 64 + ch * 8) * 2) : OOB_OFF, 0);
    }
  }
  // ---- residual tile by LDS-DMA straight into the output tile (same swizzled image): the epilogue
  //      reads each lane's 8 bytes of residual where it then writes its 8 bytes of output.
  //      32 pieces of 2 rows x 512 B, 8 per wave.
  const bool has_res = p.res != nullptr;
  if (has_res) {
    const __amdgpu_buffer_rsrc_t rr = make_rsrc_at(p.res, (long)m0 * 256, (long)p.M * 256);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int pc = wave * 8 + q, row = 2 * pc + (lane >> 5);
      const int ch = (lane & 31) ^ (row & 15);
      buf_lds16(rr, LDS_PTR(ot + pc * 1024), m0 + row < p.M ? (uint32_t)((row * 256 + ch * 8) * 2) : OOB_OFF, 0);
    }
  }
  // ---- weight fragments (A operand): W3 rows 64 wave + 16 jb + r16, k = 32 ks + 8 kq .. + 7
  v8bf w3[4][K1 / 32];
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int ks = 0; ks < K1 / 32; ++ks)
      w3[jb][ks] = *reinterpret_cast<const v8bf*>(p.w3 + (64 * wave + 16 * jb + r16) * K1 + 32 * ks + 8 * kq);

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- phase 1
  v4f acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) acc[i][jb] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < K1 / 32; ++ks) {
    const char* src = at + (ks >> 1) * A_BYTES;
    const int ch = (ks & 1) * 4 + kq;
    v8bf bx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 16 * i + r16;
      bx[i] = *reinterpret_cast<const v8bf*>(src + row * 128 + ((ch ^ cc_sw(row)) << 4));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) acc[i][jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w3[jb][ks], bx[i], acc[i][jb], 0, 0, 0);
  }
  // phase-2 weights (loaded while phase 1 drains): W1 rows 16 wave + r16, k = 32 kk + 8 kq .. + 7
  v8bf w1[8];
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) w1[kk] = *reinterpret_cast<const v8bf*>(p.w1 + (16 * wave + r16) * 256 + 32 * kk + 8 * kq);

  // ---- epilogue 1 -> output tile (bf16, 8-byte chunks)
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) {
    const int n = 64 * wave + 16 * jb + 4 * kq;
    const float4 s4 = *reinterpret_cast<const float4*>(p.scale3 + n);
    const float4 h4 = *reinterpret_cast<const float4*>(p.shift3 + n);
    const float sc[4] = {s4.x, s4.y, s4.z, s4.w}, sh[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 16 * i + r16;
      const int chunk = n >> 3;                         // 16-byte chunk of the 512-byte row
      uint2* slot = reinterpret_cast<uint2*>(ot + row * 512 + ((chunk ^ (row & 15)) << 4) + 8 * (kq & 1));
      const uint2 rv = has_res ? *slot : make_uint2(0u, 0u);
      const float r4[4] = {__uint_as_float(rv.x << 16), __uint_as_float(rv.x & 0xffff0000u),
                           __uint_as_float(rv.y << 16), __uint_as_float(rv.y & 0xffff0000u)};
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = acc[i][jb][e] * sc[e] + sh[e] + r4[e];
      *slot = make_uint2(relu_pk2(pack2(v[0], v[1])), relu_pk2(pack2(v[2], v[3])));
    }
  }
  __syncthreads();

  // ---- block-b output: row stores from the tile (32 threads per 512-byte row), + its ReLU bits
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int idx = it * 256 + tid, row = idx >> 5, c = idx & 31;
    const uint4 pk = *reinterpret_cast<const uint4*>(ot + row * 512 + ((c ^ (row & 15)) << 4));
    if (m0 + row < p.M) {
      *reinterpret_cast<uint4*>(p.out + (long)(m0 + row) * 256 + c * 8) = pk;
      if (p.bits3) p.bits3[(long)(m0 + row) * 32 + c] = (uint8_t)pos_bits8(pk);
    }
  }

  // ---- phase 2: y1[64][16 wave .. +16) over K = 256 from the output tile
  v4f acc2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc2[i] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) {
    v8bf bx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 16 * i + r16, ch = kk * 4 + kq;
      bx[i] = *reinterpret_cast<const v8bf*>(ot + row * 512 + ((ch ^ (row & 15)) << 4));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc2[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1[kk], bx[i], acc2[i], 0, 0, 0);
  }
  // ---- epilogue 2 -> y1 staging tile (the A tile's LDS: every wave finished phase 1 before the
  //      barrier above) -> row stores (+ ReLU bits)
  {
    const int n = 16 * wave + 4 * kq;
    const float4 s4 = *reinterpret_cast<const float4*>(p.scale1 + n);
    const float4 h4 = *reinterpret_cast<const float4*>(p.shift1 + n);
    const float sc[4] = {s4.x, s4.y, s4.z, s4.w}, sh[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 16 * i + r16;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = acc2[i][e] * sc[e] + sh[e];
      const int chunk = n >> 3;
      *reinterpret_cast<uint2*>(at + row * 128 + ((chunk ^ cc_sw(row)) << 4) + 8 * (kq & 1)) =
          make_uint2(relu_pk2(pack2(v[0], v[1])), relu_pk2(pack2(v[2], v[3])));
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = it * 256 + tid, row = idx >> 3, c = idx & 7;
    const uint4 pk = *reinterpret_cast<const uint4*>(at + row * 128 + ((c ^ cc_sw(row)) << 4));
    if (m0 + row < p.M) {
      *reinterpret_cast<uint4*>(p.y1 + (long)(m0 + row) * 64 + c * 8) = pk;
      if (p.bits1) p.bits1[(long)(m0 + row) * 8 + c] = (uint8_t)pos_bits8(pk);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The 64-channel persistent dual form (see the header): conv2_block1 -> 2 only.  (With a plain
// instantiation of this kernel -- one A tile, the residual DMA'd into the output tile as in the
// 128-channel form -- on conv2_block2 -> 3 the b2560 step measured 80.14 ms against the parent's
// 80.33 with a spread of 0.31, short of the acceptance rule, so c3c1_kernel above keeps the plain
// boundary: profiles/c3c1_s2_b2560.txt.)
__global__ void __launch_bounds__(512, 1) c3c1_s2_kernel(C3C1Params p) {
  constexpr int MT = C2_MT, F = 64, C = 256, K1 = 2 * F, NI = MT / 32;
  constexpr int AT = MT * 128, A_BYTES = 2 * AT, O_BYTES = MT * 512, STAGE = A_BYTES + O_BYTES;
  constexpr int TAB_BYTES = (2 * C + 2 * F) * 4;         // scale3 | shift3 | scale1 | shift1
  // 8 waves: one 8-row piece of each A tile per wave, 4 + 1 row-store chunks per thread
  static_assert(MT == 64 && 2 * STAGE + TAB_BYTES <= 160 * 1024, "c3c1_s2 tile");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE + TAB_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = wave & 3, rh = wave >> 2;
  const int r16 = lane & 15, kq = lane >> 4;
  const int G = gridDim.x, pid = blockIdx.x;
  const int T = (p.M + MT - 1) / MT;
  const int nit = pid < T ? (T - pid + G - 1) / G : 0;

  // LDS-DMA of one tile into stage `buf`: piece `wave` (8 rows, 1 KiB) of y2's tile and of the block
  // input's.  Lane offsets are relative to the tile's first row and carry the whole offset; rows >= M
  // and tiles past the last are outside the rebased descriptor and read zeros.
  auto load_tile = [&](int tile, int buf) {
    const long m0 = (long)tile * MT;
    char* ab = smem + buf * STAGE;
    const int row = wave * 8 + (lane >> 3);
    const uint32_t off = (uint32_t)(row * 128 + (((lane & 7) ^ cc_sw(row)) << 4));
    buf_lds16(make_rsrc_at(p.a, m0 * F, (long)p.M * F), LDS_PTR(ab + wave * 1024), off, 0);
    buf_lds16(make_rsrc_at(p.a2, m0 * F, (long)p.M * F), LDS_PTR(ab + AT + wave * 1024), off, 0);
  };
  if (nit > 0) load_tile(pid, 0);

  // weight fragments (A operands), held for the whole launch: W3 rows 64 cg + 16 jb + r16,
  // k = 32 ks + 8 kq .. + 7; W1 rows 16 cg + r16, k = 32 kk + 8 kq .. + 7
  v8bf w3[4][K1 / 32], w1[C / 32];
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int ks = 0; ks < K1 / 32; ++ks)
      w3[jb][ks] = *reinterpret_cast<const v8bf*>(p.w3 + (64 * cg + 16 * jb + r16) * K1 + 32 * ks + 8 * kq);
#pragma unroll
  for (int kk = 0; kk < C / 32; ++kk) w1[kk] = *reinterpret_cast<const v8bf*>(p.w1 + (16 * cg + r16) * C + 32 * kk + 8 * kq);
  {
    float* tab = reinterpret_cast<float*>(smem + 2 * STAGE);
    tab[tid] = tid < C ? p.scale3[tid] : p.shift3[tid - C];
    if (tid < 2 * F) tab[2 * C + tid] = tid < F ? p.scale1[tid] : p.shift1[tid - F];
  }
  // (the fragments land here, once: opaque from now on, so no wait for them is placed in the loop)
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int ks = 0; ks < K1 / 32; ++ks) asm volatile("" : "+v"(w3[jb][ks]));
#pragma unroll
  for (int kk = 0; kk < C / 32; ++kk) asm volatile("" : "+v"(w1[kk]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const uint32_t sb = (uint32_t)(uintptr_t)LDS_PTR(smem), tb = sb + 2 * STAGE;
  const int row0 = 32 * rh + r16;                        // this lane's first row of the tile (row & 15 == r16)
  for (int it = 0; it < nit; ++it) {
    const int cur = it & 1, tile = pid + it * G;
    const long m0 = (long)tile * MT;
    load_tile(tile + G, cur ^ 1);   // (unconditional: past the last tile the DMA writes zeros into the idle stage)
    const uint32_t at = sb + cur * STAGE, ot = at + A_BYTES;

    // ---- phase 1 (k-steps 0, 1 from y2's tile, 2, 3 from the block input's)
    v4f acc[NI][4];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) acc[i][jb] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < K1 / 32; ++ks) {
      const uint32_t src = at + (ks >> 1) * AT;
      const int ch = (ks & 1) * 4 + kq;
      cc_v4u bx[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int row = row0 + 16 * i;
        bx[i] = cc_read16(src + row * 128 + ((ch ^ cc_sw(row)) << 4));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
          acc[i][jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w3[jb][ks], __builtin_bit_cast(v8bf, bx[i]), acc[i][jb], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }

    // ---- epilogue 1 -> output tile (bf16, 8-byte chunks; "+ 0.f": the igemm epilogue's absent residual)
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      const int n = 64 * cg + 16 * jb + 4 * kq;
      const uint32_t slot = ot + row0 * 512 + (((n >> 3) ^ r16) << 4) + 8 * (kq & 1);
      const cc_v4u s4 = cc_read16(tb + n * 4), h4 = cc_read16(tb + (C + n) * 4);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[i][jb][e] * __uint_as_float(s4[e]) + __uint_as_float(h4[e]) + 0.f;
        cc_write8(slot + i * 16 * 512, make_uint2(relu_pk2(pack2(v[0], v[1])), relu_pk2(pack2(v[2], v[3]))));
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // ---- block-b output: row stores from the tile (a wave per two 512-byte rows), + its ReLU bits
    {
      cc_v4u gv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int idx = q * 512 + tid, row = idx >> 5, c = idx & 31;
        gv[q] = cc_read16(ot + row * 512 + ((c ^ (row & 15)) << 4));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int idx = q * 512 + tid, c = idx & 31;
        const long gm = m0 + (idx >> 5);
        if (gm < p.M) {
          *reinterpret_cast<cc_v4u*>(p.out + gm * C + c * 8) = gv[q];
          if (p.bits3) p.bits3[gm * (C / 8) + c] = (uint8_t)pos_bits8(make_uint4(gv[q][0], gv[q][1], gv[q][2], gv[q][3]));
        }
      }
    }

    // ---- phase 2: y1 rows [32 rh, + 32) x channels [16 cg, + 16) over K = 256 from the output tile;
    //      the reads of k-step kk + 1 are issued before the MFMAs of kk
    v4f acc2[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) acc2[i] = v4f{0.f, 0.f, 0.f, 0.f};
    cc_v4u bb[2][NI];
    auto read_kk = [&](int kk, cc_v4u (&dst)[NI]) {
      const uint32_t col = (uint32_t)(((kk * 4 + kq) ^ r16) << 4);
#pragma unroll
      for (int i = 0; i < NI; ++i) dst[i] = cc_read16(ot + (row0 + 16 * i) * 512 + col);
    };
    read_kk(0, bb[0]);
#pragma unroll
    for (int kk = 0; kk < C / 32; ++kk) {
      if (kk + 1 < C / 32) {
        read_kk(kk + 1, bb[(kk + 1) & 1]);
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(NI) : "memory");
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < NI; ++i)
        acc2[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1[kk], __builtin_bit_cast(v8bf, bb[kk & 1][i]), acc2[i], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }

    // ---- epilogue 2 -> y1 staging tile (this stage's first A tile: every wave finished phase 1
    //      before the barrier above) -> row stores (+ ReLU bits)
    {
      const int n = 16 * cg + 4 * kq;
      const cc_v4u s4 = cc_read16(tb + (2 * C + n) * 4), h4 = cc_read16(tb + (2 * C + F + n) * 4);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int row = row0 + 16 * i;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc2[i][e] * __uint_as_float(s4[e]) + __uint_as_float(h4[e]);
        cc_write8(at + row * 128 + (((n >> 3) ^ cc_sw(row)) << 4) + 8 * (kq & 1),
                  make_uint2(relu_pk2(pack2(v[0], v[1])), relu_pk2(pack2(v[2], v[3]))));
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    {
      const int row = tid >> 3, c = tid & 7;               // 64 rows x 8 chunks: one per thread
      const cc_v4u yv = cc_read16(at + row * 128 + ((c ^ cc_sw(row)) << 4));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      const long gm = m0 + row;
      if (gm < p.M) {
        *reinterpret_cast<cc_v4u*>(p.y1 + gm * F + c * 8) = yv;
        if (p.bits1) p.bits1[gm * (F / 8) + c] = (uint8_t)pos_bits8(make_uint4(yv[0], yv[1], yv[2], yv[3]));
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // next tile landed
    __syncthreads();                                    // ... and every wave is done with this stage
  }
}

// ---------------------------------------------------------------------------------------------
// The 128-channel form (stage 3: conv3 128 -> 512, + residual, ReLU; the next conv1 512 -> 128).
// W3 and W1 are 128 KiB each, so a workgroup that reloaded them per tile would pull more bytes from
// L2 than its tile moves from HBM: the grid is persistent (one 8-wave workgroup per CU, tiles b,
// b + G, ...) and both weight matrices stay in registers for the whole launch, as MFMA A operands
// like above (64 registers each: wave w holds W3 rows [64 w, 64 w + 64) and W1 rows [16 w, 16 w + 16)).
//   phase 1  out[MT][512] = y2[MT][128] . W3^T -- wave w: output channels [64 w, 64 w + 64)
//   epilogue as above, into the LDS output tile [MT][1024 B] that the residual was DMA'd into
//   phase 2  y1[MT][128] = out[MT][512] . W1^T -- wave w: channels [16 w, 16 w + 16), K = 512 from LDS
// Two LDS stages (A tile + output tile each): the next tile's A and residual LDS-DMA are issued
// before phase 1 and land under the current tile's GEMMs and stores.  The folded BN scale / shift
// (1280 floats) sit in LDS: in registers they would cost 40 per lane on top of the weights.
// Every LDS access inside the tile loop is inline asm (see bwd1x1.hip: the compiler cannot tell
// those addresses from the LDS-DMA targets in flight and would drain the prefetch before each one).
// LDS swizzle of both images: 16-byte chunk ^ (row & 15) within each 256-byte group (row pitches
// of 256 and 1024 bytes are whole bank rows).
// Tile height C3_MT = 32 rows (2 x 40 KiB stages + the 5 KiB table, 206 registers, no scratch).
// Measured at b2560 (profiles/c3c1_s3_b2560.txt): 32 rows 975 / 979 us per boundary, 48 rows
// (2 x 60 KiB, 230 registers) 993 / 985 us, step time the same within its spread; 64 rows do
// not fit (2 x 80 KiB stages are the CU's whole 160 KiB, before the table).  The two launches
// this replaces took 1,069 + 520 us.
template <int MT>
__global__ void __launch_bounds__(512, 1) c3c1_s3_kernel(C3C1Params p) {
  constexpr int F = 128, C = 512, NI = MT / 16;
  constexpr int A_BYTES = MT * 256, O_BYTES = MT * 1024, STAGE = A_BYTES + O_BYTES;
  constexpr int TAB_BYTES = (2 * C + 2 * F) * 4;         // scale3 | shift3 | scale1 | shift1
  static_assert(MT % 16 == 0 && 2 * STAGE + TAB_BYTES <= 160 * 1024, "c3c1_s3 tile");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE + TAB_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kq = lane >> 4;
  const int G = gridDim.x, pid = blockIdx.x;
  const int T = (p.M + MT - 1) / MT;
  const int nit = pid < T ? (T - pid + G - 1) / G : 0;
  const bool has_res = p.res != nullptr;

  // LDS-DMA of one tile into stage `buf`.  A: pieces of 4 rows (1 KiB), piece wave + 8 q; residual:
  // one 1 KiB row per piece, row wave + 8 q.  Lane offsets are relative to the tile's first row and
  // carry the whole offset (the range check does not see a scalar offset); rows >= M and tiles
  // past the last are outside the rebased descriptor and read zeros.
  auto load_tile = [&](int tile, int buf) {
    const long m0 = (long)tile * MT;
    char* ab = smem + buf * STAGE;
    const __amdgpu_buffer_rsrc_t ra = make_rsrc_at(p.a, m0 * F, (long)p.M * F);
#pragma unroll
    for (int q = 0; q < (MT / 4 + 7) / 8; ++q) {
      const int pc = wave + 8 * q, row = pc * 4 + kq;
      if (pc < MT / 4) buf_lds16(ra, LDS_PTR(ab + pc * 1024), (uint32_t)(row * 256 + ((r16 ^ (row & 15)) << 4)), 0);
    }
    if (has_res) {
      const __amdgpu_buffer_rsrc_t rr = make_rsrc_at(p.res, m0 * C, (long)p.M * C);
#pragma unroll
      for (int q = 0; q < MT / 8; ++q) {
        const int row = wave + 8 * q;
        buf_lds16(rr, LDS_PTR(ab + A_BYTES + row * 1024), (uint32_t)(row * 1024 + ((lane ^ (row & 15)) << 4)), 0);
      }
    }
  };
  if (nit > 0) load_tile(pid, 0);

  // weight fragments (A operands), held for the whole launch: W3 rows 64 wave + 16 jb + r16,
  // k = 32 ks + 8 kq .. + 7; W1 rows 16 wave + r16, k = 32 kk + 8 kq .. + 7
  v8bf w3[4][F / 32], w1[C / 32];
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int ks = 0; ks < F / 32; ++ks)
      w3[jb][ks] = *reinterpret_cast<const v8bf*>(p.w3 + (64 * wave + 16 * jb + r16) * F + 32 * ks + 8 * kq);
#pragma unroll
  for (int kk = 0; kk < C / 32; ++kk) w1[kk] = *reinterpret_cast<const v8bf*>(p.w1 + (16 * wave + r16) * C + 32 * kk + 8 * kq);
  {
    float* tab = reinterpret_cast<float*>(smem + 2 * STAGE);
    tab[tid] = p.scale3[tid];
    tab[C + tid] = p.shift3[tid];
    if (tid < F) { tab[2 * C + tid] = p.scale1[tid]; tab[2 * C + F + tid] = p.shift1[tid]; }
  }
  // (the fragments land here, once: opaque from now on, so no wait for them is placed in the loop)
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int ks = 0; ks < F / 32; ++ks) asm volatile("" : "+v"(w3[jb][ks]));
#pragma unroll
  for (int kk = 0; kk < C / 32; ++kk) asm volatile("" : "+v"(w1[kk]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const uint32_t sb = (uint32_t)(uintptr_t)LDS_PTR(smem), tb = sb + 2 * STAGE;
  for (int it = 0; it < nit; ++it) {
    const int cur = it & 1, tile = pid + it * G;
    const long m0 = (long)tile * MT;
    load_tile(tile + G, cur ^ 1);   // (unconditional: past the last tile the DMA writes zeros into the idle stage)
    const uint32_t at = sb + cur * STAGE, ot = at + A_BYTES;
    // (two waves per SIMD leave 256 registers, half of them the weights: the LDS addresses are
    // re-derived per tile -- the opaque copy of the lane id keeps them out of the loop-invariant set)
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int r16 = ln & 15, kq = ln >> 4, tn = wave * 64 + ln;

    // ---- phase 1
    v4f acc[NI][4];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) acc[i][jb] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < F / 32; ++ks) {
      const uint32_t col = (uint32_t)(((ks * 4 + kq) ^ r16) << 4);
      cc_v4u bx[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) bx[i] = cc_read16(at + (16 * i + r16) * 256 + col);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
          acc[i][jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w3[jb][ks], __builtin_bit_cast(v8bf, bx[i]), acc[i][jb], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }

    // ---- epilogue 1 -> output tile (bf16, 8-byte chunks, over the residual)
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      const int n = 64 * wave + 16 * jb + 4 * kq;
      const uint32_t slot = ot + r16 * 1024 + (((n >> 3) ^ r16) << 4) + 8 * (kq & 1);
      const cc_v4u s4 = cc_read16(tb + n * 4), h4 = cc_read16(tb + (C + n) * 4);
      uint2 rv[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) rv[i] = make_uint2(0u, 0u);
      if (has_res) {
#pragma unroll
        for (int i = 0; i < NI; ++i) rv[i] = cc_read8(slot + i * 16 * 1024);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const float r4[4] = {__uint_as_float(rv[i].x << 16), __uint_as_float(rv[i].x & 0xffff0000u),
                             __uint_as_float(rv[i].y << 16), __uint_as_float(rv[i].y & 0xffff0000u)};
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[i][jb][e] * __uint_as_float(s4[e]) + __uint_as_float(h4[e]) + r4[e];
        cc_write8(slot + i * 16 * 1024, make_uint2(relu_pk2(pack2(v[0], v[1])), relu_pk2(pack2(v[2], v[3]))));
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // ---- block-b output: row stores from the tile (one wave per 1 KiB row), + its ReLU bits
    {
      constexpr int GV = MT / 8;
      cc_v4u gv[GV];
#pragma unroll
      for (int q = 0; q < GV; ++q) {
        const int row = q * 8 + wave;
        gv[q] = cc_read16(ot + row * 1024 + ((ln ^ (row & 15)) << 4));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < GV; ++q) {
        const long gm = m0 + q * 8 + wave;
        if (gm < p.M) {
          *reinterpret_cast<cc_v4u*>(p.out + gm * C + lane * 8) = gv[q];
          if (p.bits3) p.bits3[gm * (C / 8) + lane] = (uint8_t)pos_bits8(make_uint4(gv[q][0], gv[q][1], gv[q][2], gv[q][3]));
        }
      }
    }

    // ---- phase 2: y1[MT][16 wave .. + 16) over K = 512 from the output tile; the reads of
    //      k-step kk + 1 are issued before the MFMAs of kk
    v4f acc2[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) acc2[i] = v4f{0.f, 0.f, 0.f, 0.f};
    cc_v4u bb[2][NI];
    auto read_kk = [&](int kk, cc_v4u (&dst)[NI]) {
      const uint32_t col = (uint32_t)(((kk * 4 + kq) ^ r16) << 4);
#pragma unroll
      for (int i = 0; i < NI; ++i) dst[i] = cc_read16(ot + (16 * i + r16) * 1024 + col);
    };
    read_kk(0, bb[0]);
#pragma unroll
    for (int kk = 0; kk < C / 32; ++kk) {
      if (kk + 1 < C / 32) {
        read_kk(kk + 1, bb[(kk + 1) & 1]);
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(NI) : "memory");
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < NI; ++i)
        acc2[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1[kk], __builtin_bit_cast(v8bf, bb[kk & 1][i]), acc2[i], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }

    // ---- epilogue 2 -> y1 staging tile (this stage's A tile: every wave finished phase 1 before
    //      the barrier above) -> row stores (+ ReLU bits)
    {
      const int n = 16 * wave + 4 * kq;
      const cc_v4u s4 = cc_read16(tb + (2 * C + n) * 4), h4 = cc_read16(tb + (2 * C + F + n) * 4);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc2[i][e] * __uint_as_float(s4[e]) + __uint_as_float(h4[e]);
        cc_write8(at + (16 * i + r16) * 256 + (((n >> 3) ^ r16) << 4) + 8 * (kq & 1),
                  make_uint2(relu_pk2(pack2(v[0], v[1])), relu_pk2(pack2(v[2], v[3]))));
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    {
      constexpr int YV = (MT * 16 + 511) / 512;
      cc_v4u yv[YV];
#pragma unroll
      for (int q = 0; q < YV; ++q) {
        const int idx = q * 512 + tn, row = idx >> 4, c = idx & 15;
        yv[q] = cc_v4u{0u, 0u, 0u, 0u};
        if (idx < MT * 16) yv[q] = cc_read16(at + row * 256 + ((c ^ (row & 15)) << 4));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < YV; ++q) {
        const int idx = q * 512 + tn, row = idx >> 4, c = idx & 15;
        const long gm = m0 + row;
        if (idx < MT * 16 && gm < p.M) {
          *reinterpret_cast<cc_v4u*>(p.y1 + gm * F + c * 8) = yv[q];
          if (p.bits1) p.bits1[gm * (F / 8) + c] = (uint8_t)pos_bits8(make_uint4(yv[q][0], yv[q][1], yv[q][2], yv[q][3]));
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // next tile landed
    __syncthreads();                                    // ... and every wave is done with this stage
  }
}

namespace {
constexpr int C3_MT = 32;
}
int g_c3c1_grid = 0;   // test knob: cap on the persistent kernels' workgroup count (0: one per CU), like bwd1x1_grid

const char* c3c1_launch(const C3C1Params& p, hipStream_t s) {
  if (p.M <= 0) return "c3c1: empty";
  if (!p.a || !p.w3 || !p.scale3 || !p.shift3 || !p.out || !p.w1 || !p.scale1 || !p.shift1 || !p.y1)
    return "c3c1: missing operand";
  if (p.a2 && (p.F != 64 || p.res)) return "c3c1: the dual-source form is 64 channels wide and takes no residual";
  long G = num_cus();
  if (g_c3c1_grid > 0 && g_c3c1_grid < G) G = g_c3c1_grid;
  if (p.F == 128) {
    if ((long)p.M * 512 >= (1L << 31)) return "c3c1: block output has more than 2^31 elements";
    const long T = ((long)p.M + C3_MT - 1) / C3_MT;
    const dim3 grid((unsigned)(T < G ? T : G));
    hipLaunchKernelGGL(c3c1_s3_kernel<C3_MT>, grid, dim3(512), 0, s, p);
  } else if (p.F == 64) {
    if ((long)p.M * 256 >= (1L << 31)) return "c3c1: block output has more than 2^31 elements";
    if (p.a2) {
      const long T = ((long)p.M + C2_MT - 1) / C2_MT;
      const dim3 grid((unsigned)(T < G ? T : G));
      hipLaunchKernelGGL(c3c1_s2_kernel, grid, dim3(512), 0, s, p);
    } else {
      const dim3 grid((unsigned)((p.M + CC_BM - 1) / CC_BM));
      hipLaunchKernelGGL(c3c1_kernel, grid, dim3(256), 0, s, p);
    }
  } else {
    return "c3c1: bottleneck width must be 64 or 128";
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}

}  // namespace pddl
