// Split-plane fp32 GEMM: shared device code, instantiated per mode in
// csrc/kernels/gemm_sp{,_dgrad,_wgrad}.hip (the three translation units compile in parallel).
//
//   FWD   C[M,N]  = X[M,K] . W[N,K]^T  (+bias, ReLU, dropout)        A k-contig, B k-contig
//   DGRAD dX[M,K] = dY[M,N] . W[N,K]   (+residual, x relu'/dropout)  A k-contig, B k-major
//   WGRAD dW[N,K] += dY[M,N]^T . X[M,K] (+ bias grad = dY^T 1)       A k-major,  B k-major
//
// Reference precision (fp32 operands, exact products, fp32 accumulation) on the bf16 matrix
// cores.  Both operands arrive PRE-SPLIT as three bf16 planes (x = hi + mid + lo exactly, see
// smi_gemm_sp.h): the weights are split by the optimizer when it updates them
// (csrc/kernels/optim.hip), activations by the kernel that produces them (or once by
// smi_split3).  The k-loop therefore contains no splitting arithmetic at all — it is the
// structure of a bf16 GEMM that issues SIX v_mfma_f32_32x32x16_bf16 per fragment pair
// (hi.hi into the main accumulator; lo.hi, mid.mid, hi.lo, mid.hi, hi.mid into a correction
// accumulator added once at the end: the dropped mid.lo / lo.mid / lo.lo terms are below one
// fp32 rounding of the product).  Per 32-deep k-step a 128 x 128 tile issues 48 MFMAs per wave
// against 48 KiB of staged planes, 32 B/clk/CU at the matrix-core rate.
//
// CDNA4 structure: 512-thread workgroups (2 x 4 waves, two per SIMD: one wave's LDS-DMA /
// fragment-read issue runs beside its partner's MFMAs; a wave owns 64 x 32 = 2 x 1 accumulators
// of 32 x 32), ONE workgroup per CU (144 KiB of LDS: three stages of 2 operands x 3 planes x
// 128 x 32 bf16).  Stages are filled by buffer_load_dwordx4 ... lds (LDS-DMA, no VGPR round trip;
// per-lane source offsets computed once per tile, the k advance is the scalar soffset; one buffer
// descriptor per plane, so out-of-range rows / k read as zero through the descriptor's extent).
// The LDS images (smi_plane_lds.h) carry their XOR swizzles in the per-lane SOURCE offsets (the
// DMA writes lane-linear).  Two k-steps stay in flight (counted vmcnt, raw s_barrier, one barrier
// per k-step).  XCD-aware tile order.  The large problems run 256 x 128 tiles on
// v_mfma_f32_16x16x32_bf16 instead (gemm_sp_tile256m below).
#pragma once
#include "smi_common.h"
#include "smi_gemm_sp.h"
#include "smi_plane_lds.h"
#include "smi_split3.h"

#define SP_BK 32            // k-step depth
#define SP_PL 4096          // bf16 per plane tile (128 x 32)
#define SP_OP (3 * SP_PL)   // one operand's three planes
#define SP_ST (2 * SP_OP)   // one stage: A then B (48 KiB)
#define SP_NS 3
#define SP_EPI_PITCH 132    // LDS pitch (floats) of the staged 128 x 128 fp32 epilogue tile
#define SP_NT 512           // threads of every tile form (8 waves)

#ifdef SP_STAMPS
// diagnostic build only (tools/probes/sp_probe.hip): s_memrealtime (100 MHz) stamps of each
// workgroup's phases, written by thread 0 to a buffer no output depends on
__device__ unsigned long long* g_sp_stamps;
#define SP_STAMP(slot)                                                                     \
  do {                                                                                     \
    if (threadIdx.x == 0) g_sp_stamps[(long)blockIdx.x * 8 + (slot)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define SP_STAMP(slot) do {} while (0)
#endif

enum : int { SE_BIAS = 1, SE_RELU = 2, SE_DROP = 8, SE_RESID = 16, SE_DACT = 32, SE_ACC = 64, SE_DMASK = 256 };
enum : int { SO_C = 1, SO_P = 2, SO_M = 4 };  // epilogue outputs: fp32 C, planes P, positivity mask

typedef __attribute__((address_space(3))) void sp_lds_void;

// Per-lane DMA source offsets (bytes, relative to a plane base, k0 = 0) of the PPW 1-KiB pieces
// wave w stages per plane (pieces PPW w + i of the 8 that make a plane tile):
//   k-contig: a piece = 16 rows; lane L -> row 16 s + L / 4, physical chunk L & 3
//   k-major : a piece = 4 k-rows; lane L -> k-row 4 s + L / 16, physical chunk L & 15
// (the logical chunk is the physical one XOR the swizzle).
template <bool KMAJ, int PPW>
__device__ __forceinline__ void sp_voffs(long ld, int r0, int rlim, int w, int lane, uint32_t (&vo)[PPW]) {
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int s = PPW * w + i;
    if (!KMAJ) {
      const int row = 16 * s + (lane >> 2);
      const int c = (lane & 3) ^ ((row >> 2) & 3);
      vo[i] = (r0 + row < rlim) ? (uint32_t)(((long)(r0 + row) * ld + 8 * c) * 2) : SMI_OOB;
    } else {
      const int kr = 4 * s + (lane >> 4);
      const int col = r0 + 8 * ((lane & 15) ^ sp_swz(kr));
      vo[i] = (col < rlim) ? (uint32_t)(((long)kr * ld + col) * 2) : SMI_OOB;
    }
  }
}

// f32 value -> its three bf16 slices, stored as 4-element groups (8 B per plane)
__device__ __forceinline__ void sp_store4(unsigned short* p, long pps, const float (&v)[4]) {
  uint32_t h0, m0, l0, h1, m1, l1;
  split3_pair(v[0], v[1], h0, m0, l0);
  split3_pair(v[2], v[3], h1, m1, l1);
  *(uint2*)p = make_uint2(h0, h1);
  *(uint2*)(p + pps) = make_uint2(m0, m1);
  *(uint2*)(p + 2 * pps) = make_uint2(l0, l1);
}
__device__ __forceinline__ void sp_store1(unsigned short* p, long pps, float x) {
  const unsigned short h = f2bf(x);
  const float r = x - bf2f(h);
  const unsigned short m = f2bf(r);
  p[0] = h;
  p[pps] = m;
  p[2 * pps] = f2bf(r - bf2f(m));
}

// Epilogue, second half: the staged fp32 tile ep [TM][SP_EPI_PITCH] -> bias / activation / dropout /
// residual / relu'-mask / accumulate -> fp32 C and / or split planes P; thread t owns 4 columns
// of rows (t >> 5) + 16 q (float4 operand loads, 16-B stores of whole row segments).
template <int TM, int EPI, int OUT>
__device__ __forceinline__ void sp_store_tile(const GemmSpArgs& g, const float* ep, int m0, int n0) {
  const int tid = threadIdx.x;
  const int c4 = (tid & 31) * 4, col = n0 + c4;
  const bool hasC = (OUT & SO_C) && g.C;
  const bool vec = ((g.ldc | ((EPI & SE_RESID) ? g.ldr : 0) | ((EPI & SE_DACT) ? g.ldy : 0) |
                     ((OUT & SO_P) ? g.ldp : 0)) & 3) == 0;
  const bool full_cols = vec && col + 3 < g.N;
  const uint32_t seed = (EPI & SE_DROP) ? smi_seed(g.seedp, g.salt) : 0u;
  float bb[4] = {0.f, 0.f, 0.f, 0.f};
  if (EPI & SE_BIAS) {
    if (full_cols) {
      const float4 t = *(const float4*)(g.bias + col);
      bb[0] = t.x; bb[1] = t.y; bb[2] = t.z; bb[3] = t.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col + e < g.N) bb[e] = g.bias[col + e];
    }
  }
  constexpr int RS = SP_NT / 32;  // rows between a thread's consecutive rows
#pragma unroll 4
  for (int q = 0; q < TM / RS; ++q) {
    const int rl = (tid >> 5) + RS * q, row = m0 + rl;
    if (row >= g.M) continue;  // uniform over the 32 lanes that share the row
    if (col >= g.N) continue;
    const float4 t = *(const float4*)(ep + rl * SP_EPI_PITCH + c4);
    float v[4] = {t.x, t.y, t.z, t.w};
    const long cidx = (long)row * g.ldc + col;
    if (full_cols) {
      float4 rs = make_float4(0.f, 0.f, 0.f, 0.f), dy = rs, cc = rs;
      if (EPI & SE_RESID) rs = *(const float4*)(g.resid + (long)row * g.ldr + col);
      if (EPI & SE_DACT) dy = *(const float4*)(g.dact_y + (long)row * g.ldy + col);
      if ((EPI & SE_ACC) && hasC) cc = *(const float4*)(g.C + cidx);
      const unsigned mk = (EPI & SE_DMASK) ? g.mask[(long)row * g.ldm + (col >> 2)] : 0u;
      const float rv[4] = {rs.x, rs.y, rs.z, rs.w}, dv[4] = {dy.x, dy.y, dy.z, dy.w}, cv[4] = {cc.x, cc.y, cc.z, cc.w};
      unsigned bits = 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x = v[e] + bb[e];
        if (EPI & SE_RELU) x = fmaxf(x, 0.f);
        if (EPI & SE_DROP) x = smi_keep(seed, (uint32_t)(cidx + e), g.thresh) ? x * g.dscale : 0.f;
        if (EPI & SE_RESID) x += rv[e];
        if (EPI & SE_DACT) x = dv[e] > 0.f ? x * g.dscale : 0.f;
        if (EPI & SE_DMASK) x = ((mk >> e) & 1u) ? x * g.dscale : 0.f;
        if (EPI & SE_ACC) x += cv[e];
        bits |= (x > 0.f ? 1u : 0u) << e;
        v[e] = x;
      }
      if (hasC) *(float4*)(g.C + cidx) = make_float4(v[0], v[1], v[2], v[3]);
      if (OUT & SO_P) sp_store4(g.P + (long)row * g.ldp + col, g.pps, v);
      if (OUT & SO_M) g.mask[(long)row * g.ldm + (col >> 2)] = (unsigned char)bits;
    } else {
      const unsigned mk = (EPI & SE_DMASK) ? g.mask[(long)row * g.ldm + (col >> 2)] : 0u;
      unsigned bits = 0u;
      for (int e = 0; e < 4 && col + e < g.N; ++e) {
        float x = v[e] + bb[e];
        if (EPI & SE_RELU) x = fmaxf(x, 0.f);
        if (EPI & SE_DROP) x = smi_keep(seed, (uint32_t)(cidx + e), g.thresh) ? x * g.dscale : 0.f;
        if (EPI & SE_RESID) x += g.resid[(long)row * g.ldr + col + e];
        if (EPI & SE_DACT) x = g.dact_y[(long)row * g.ldy + col + e] > 0.f ? x * g.dscale : 0.f;
        if (EPI & SE_DMASK) x = ((mk >> e) & 1u) ? x * g.dscale : 0.f;
        if ((EPI & SE_ACC) && hasC) x += g.C[cidx + e];
        if (hasC) g.C[cidx + e] = x;
        if (OUT & SO_P) sp_store1(g.P + (long)row * g.ldp + col + e, g.pps, x);
        bits |= (x > 0.f ? 1u : 0u) << e;
        v[e] = x;
      }
      if (OUT & SO_M) g.mask[(long)row * g.ldm + (col >> 2)] = (unsigned char)bits;
    }
  }
}

// Bias-gradient row sums of a tile's A fragments (WGRAD, dY^T 1) on v_mfma_f32_16x16x32_bf16.
// Read as a 16x16x32 A operand, a 32x32x16 fragment (lane l: row l & 31, k-half l >> 5) puts
// tile rows r and r + 16 in different k-groups (vk = l >> 4: row vr + 16 (vk & 1), k-half
// vk >> 1), so ONE MFMA against a selector fragment that is 1.0 in column 0 for even k-groups and
// in column 1 for odd ones sums rows 0..15 into column 0 and rows 16..31 into column 1 — all 32
// row sums in 4 accumulator registers.  The hi plane uses columns 0 / 1, mid + lo columns 2 / 3:
// two exact fp32 chains (one rounding per 16 k each), added once at the end.
template <int NI = 2>
struct SpBiasSum {
  f32x4_t c[NI];         // per 32-row fragment i
  bf16x8_t sel_hi, sel_ml;
  __device__ __forceinline__ void init(int lane) {
    const int vk = (lane >> 4) & 1, col = lane & 15;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sel_hi[e] = col == vk ? (short)0x3F80 : (short)0;       // bf16 1.0
      sel_ml[e] = col == 2 + vk ? (short)0x3F80 : (short)0;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) c[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  __device__ __forceinline__ void add(int i, const Split3& f) {
    c[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.l, sel_ml, c[i], 0, 0, 0);
    c[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.m, sel_ml, c[i], 0, 0, 0);
    c[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.h, sel_hi, c[i], 0, 0, 0);
  }
  // lanes with column 0 / 1 own tile rows 16 col + 4 (lane >> 4) + r of fragment i (r = 0..3);
  // their mid + lo chain sits two lanes up (columns 2 / 3)
  __device__ __forceinline__ void store(const GemmSpArgs& g, int row0, int lane, bool accumulate) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ml = __shfl_down(c[i][r], 2, 64);
        const int col = lane & 15;
        const int row = row0 + i * 32 + 16 * col + 4 * (lane >> 4) + r;
        if (col < 2 && row < g.M) {
          const float v = c[i][r] + ml;
          g.bias_grad[row] = accumulate ? g.bias_grad[row] + v : v;
        }
      }
  }
};

// One 128 x 128 output tile: the whole k-loop and the fused epilogue.  8 waves (2 x 4, a wave owns
// 64 rows x 32 columns; one wave per SIMD measured stalled on issue 62 % of its cycles); wave w
// stages piece w of each of a stage's six plane tiles.  BIASG: this workgroup also reduces the bias
// gradient (WGRAD, column block 0; a separate instance keeps the k-loop one basic block for the
// MFMA / LDS-read / DMA interleave).
//
// Accumulation: hi.hi in its own fp32 accumulator (the rounding sequence of a plain fp32 chain,
// one rounding per 16 k), the five correction products (lo.hi, mid.mid, hi.lo, mid.hi, hi.mid) in
// a second one added at the end.  Measured: ONE accumulator for all six (six roundings per 16 k)
// let the 8192-token weight-gradient reduction drift to 1.7x the f32-MFMA kernel's error.
template <bool AK, bool BKM, int EPI, int OUT, bool BIASG = false>
__device__ __forceinline__ void gemm_sp_tile(const GemmSpArgs& g, int tile, unsigned short* lds) {
  SP_STAMP(0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w / 4, wn = w % 4, h = lane >> 5;
  const int ntn = (g.N + 127) / 128;
  const int m0 = (tile / ntn) * 128, n0 = (tile % ntn) * 128;
  const int nk = (g.K + SP_BK - 1) / SP_BK;
  __amdgpu_buffer_rsrc_t ra[3], rb[3];
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    ra[p] = smi_rsrc(g.A + p * g.aps, g.a_bytes);
    rb[p] = smi_rsrc(g.B + p * g.bps, g.b_bytes);
  }
  uint32_t va[1], vb[1];  // this wave's piece (w) of each A / B plane tile
  sp_voffs<AK, 1>(g.lda, m0, g.M, w, lane, va);
  sp_voffs<BKM, 1>(g.ldb, n0, g.N, w, lane, vb);
  f32x16_t acc[2], cacc[2];
  SpBiasSum<> bsum;
  if constexpr (BIASG) bsum.init(lane);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = cacc[i][r] = 0.f;
  // k-steps run in pairs with no exit between the halves; k-steps >= nk (the odd tail and the
  // look-ahead past the end) stage ZEROS: their soffset is pushed past every extent
  const int nk2 = (nk + 1) & ~1;
  auto issue = [&](int kt, int slot) {
    unsigned short* st = lds + slot * SP_ST;
    const bool real = kt < nk;
    const int k0 = kt * SP_BK;
    const uint32_t sa = real ? (AK ? (uint32_t)((long)k0 * g.lda * 2) : (uint32_t)(k0 * 2)) : SMI_OOB;
    const uint32_t sb = real ? (BKM ? (uint32_t)((long)k0 * g.ldb * 2) : (uint32_t)(k0 * 2)) : SMI_OOB;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra[p], (sp_lds_void*)(st + p * SP_PL + w * 512), 16, va[0], sa, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rb[p], (sp_lds_void*)(st + SP_OP + p * SP_PL + w * 512), 16, vb[0], sb,
                                               0, 0);
    }
  };
  auto read = [&](int slot, Split3 (&fa)[2][2], Split3 (&fb)[2]) {
    const unsigned short* st = lds + slot * SP_ST;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[b][i] = frag32<AK>(st, SP_PL, wm * 64 + i * 32, b, lane);
      fb[b] = frag32<BKM>(st + SP_OP, SP_PL, wn * 32, b, lane);
    }
  };
  auto mma = [&](const Split3 (&fa)[2][2], const Split3 (&fb)[2]) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int i = 0; i < 2; ++i) split3_mma2(fa[b][i], fb[b], acc[i], cacc[i]);
      if constexpr (BIASG) {
#pragma unroll
        for (int i = 0; i < 2; ++i) bsum.add(i, fa[b][i]);
      }
    }
  };
  // One k-step: the fragments of stage kt are in registers (read during the previous step).
  // Wait until this wave's fragment reads and its DMA pieces of stage kt + 1 are done (stage
  // kt + 2's may still fly), barrier (every wave's pieces landed, every wave's reads of stage kt
  // retired), then: read stage kt + 1 into the other fragment set, refill stage kt's slot with
  // k-step kt + 3, and run stage kt's MFMAs — reads and DMA issues interleaved between them.
  constexpr int NRD = 2 * (2 * (AK ? 6 : 3) + (BKM ? 6 : 3));  // LDS fragment reads per k-step
  constexpr int NMF = 2 * (2 * 6 + (BIASG ? 6 : 0));           // MFMAs per k-step (incl. bias)
  constexpr int NDMA = 6;                                       // DMA pieces per wave per stage
  Split3 f0a[2][2], f0b[2], f1a[2][2], f1b[2];
  issue(0, 0);
  issue(1, 1);
  issue(2, 2);
  asm volatile("s_waitcnt vmcnt(12)" ::: "memory");  // stage 0's NDMA pieces landed, two stages in flight
  __builtin_amdgcn_s_barrier();
  SP_STAMP(1);
  read(0, f0a, f0b);
  int slot = 0;
  for (int kt = 0; kt < nk2; kt += 2) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");  // one stage (NDMA pieces) in flight
      __builtin_amdgcn_s_barrier();
      const int nxt = slot == SP_NS - 1 ? 0 : slot + 1;
      if (half == 0) read(nxt, f1a, f1b);
      else read(nxt, f0a, f0b);
      issue(kt + half + 3, slot);
      if (half == 0) mma(f0a, f0b);
      else mma(f1a, f1b);
      // fragment reads spread over the first MFMAs, the DMA issues after them
      constexpr int RPM = NRD <= NMF / 2 ? 1 : 2;  // reads per MFMA slot
#pragma unroll
      for (int i = 0; i < NRD / RPM; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, RPM, 0);  // DS read
      }
#pragma unroll
      for (int i = 0; i < NDMA; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // VMEM (LDS-DMA)
      }
      __builtin_amdgcn_sched_group_barrier(0x008, NMF, 0);
      slot = nxt;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the zero look-ahead stages before LDS reuse
  SP_STAMP(2);

  // ---- epilogue: accumulators -> LDS [128][132] -> each thread owns 4 columns of 8 rows ----
#pragma unroll
  for (int i = 0; i < 2; ++i) acc[i] += cacc[i];
  __syncthreads();  // every wave is done reading the k-loop's stages
  float* ep = (float*)lds;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      ep[(wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * SP_EPI_PITCH + wn * 32 + (lane & 31)] = acc[i][r];
  __syncthreads();
  SP_STAMP(3);
  sp_store_tile<128, EPI, OUT>(g, ep, m0, n0);
  SP_STAMP(4);
  if constexpr (BIASG) {
    if (wn == 0) bsum.store(g, m0 + wm * 64, lane, (EPI & SE_ACC) != 0);
  }
}

template <bool AK, bool BKM, int EPI, int OUT>
__global__ __launch_bounds__(SP_NT, 1) void gemm_sp_kernel(GemmSpArgs g) {
  __shared__ __attribute__((aligned(16))) unsigned short lds[SP_NS * SP_ST];
  const int nwg = ((g.M + 127) / 128) * ((g.N + 127) / 128);
  const int tile = smi_xcd_remap(blockIdx.x, nwg);
  if constexpr (AK) {
    if (g.bias_grad && tile % ((g.N + 127) / 128) == 0) {
      gemm_sp_tile<AK, BKM, EPI, OUT, true>(g, tile, lds);
      return;
    }
  }
  gemm_sp_tile<AK, BKM, EPI, OUT, false>(g, tile, lds);
}

// ---------------------------------------------------------------------------------------------
// 256 x 128 output tile (gemm_sp_tm 16, the default where such tiles fill the chip, and the weight
// gradients): 8 waves (4 x 2, each 64 x 64 = 4 x 4 accumulators of 16 x 16, two waves per SIMD),
// two 72 KiB stages.  Per 32-deep k-step a CU stages 72 KiB of planes — a quarter fewer bytes and
// a third fewer LDS fragment reads per MFMA cycle than the 128 x 128 tile, whose k-loop measured
// 1.3 us per k-step against 0.8 us for its MFMAs alone and 0.8 us for its DMA + LDS reads alone
// (tools/probes/sp_probe.hip).  Registers allow one fragment set: the stage a k-step reads is
// refilled (k-step kt + 2) after a second barrier that follows this step's fragment reads.
// On v_mfma_f32_16x16x32_bf16 (one k-step = one MFMA of k 32 per product): the same MFMA cycles per
// FLOP as 32x32x16, but the chip holds a higher clock on the 16 x 16 shape under load (~1.15x
// FLOP/s on random data; the 32x32x16 form of this tile measured 5-8 % slower on forward shapes,
// docs/PERF_NOTES.md).  Fragments and swizzles: frag16 in smi_plane_lds.h.
#define SP_ST256 (3 * (256 + 128) * SP_BK)  // bf16 per stage: A 3 x 256 x 32, B 3 x 128 x 32
static_assert(2 * SP_ST256 == SP_NS * SP_ST, "both tile forms use the same LDS (147456 B)");

// bias row sums of 16-row A fragments: one 16x16x32 MFMA against a fragment that is 1.0 in column
// 0 (hi chain) / column 1 (mid + lo chain) gives all 16 row sums
template <int NI>
struct SpBiasSum16 {
  f32x4_t c[NI];
  bf16x8_t sel_hi, sel_ml;
  __device__ __forceinline__ void init(int lane) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sel_hi[e] = (lane & 15) == 0 ? (short)0x3F80 : (short)0;
      sel_ml[e] = (lane & 15) == 1 ? (short)0x3F80 : (short)0;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) c[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  __device__ __forceinline__ void add(int i, const Split3& f) {
    c[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.l, sel_ml, c[i], 0, 0, 0);
    c[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.m, sel_ml, c[i], 0, 0, 0);
    c[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.h, sel_hi, c[i], 0, 0, 0);
  }
  // lanes of column 0 own rows 4 (lane >> 4) + r of fragment i; the mid + lo chain is one lane up
  __device__ __forceinline__ void store(const GemmSpArgs& g, int row0, int lane, bool accumulate) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ml = __shfl_down(c[i][r], 1, 64);
        const int row = row0 + i * 16 + 4 * (lane >> 4) + r;
        if ((lane & 15) == 0 && row < g.M) {
          const float v = c[i][r] + ml;
          g.bias_grad[row] = accumulate ? g.bias_grad[row] + v : v;
        }
      }
  }
};

#define MF16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

// fp32 operands as hi / mid / lo planes, six slice products per 32-deep k-step.
template <bool AK, bool BKM, int EPI, int OUT, bool BIASG = false>
__device__ __forceinline__ void gemm_sp_tile256m(const GemmSpArgs& g, int tile, unsigned short* lds) {
  constexpr int NB = 4;  // 4 x 4 blocks of 16 x 16 per wave
  constexpr int AOP = 3 * 256 * SP_BK;
  constexpr int APL = 256 * SP_BK;
  constexpr int KSTEP = SP_BK;  // k per stage
  SP_STAMP(0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int ntn = (g.N + 127) / 128;
  const int m0 = (tile / ntn) * 256, n0 = (tile % ntn) * 128;
  const int nk = (g.K + KSTEP - 1) / KSTEP;
  __amdgpu_buffer_rsrc_t ra[3], rb[3];
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    ra[p] = smi_rsrc(g.A + p * g.aps, g.a_bytes);
    rb[p] = smi_rsrc(g.B + p * g.bps, g.b_bytes);
  }
  // A: 16 pieces per plane (pieces 2w, 2w + 1), B: 8 (piece w); k-contig pieces swizzled by sp16_swz
  uint32_t va[2], vb;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int s = 2 * w + i;
    if (!AK) {
      const int row = 16 * s + (lane >> 2);
      const int c = (lane & 3) ^ sp16_swz(row);
      va[i] = (m0 + row < g.M) ? (uint32_t)(((long)(m0 + row) * g.lda + 8 * c) * 2) : SMI_OOB;
    } else {
      const int sub = s >> 3, kr = 4 * (s & 7) + (lane >> 4);
      const int col = m0 + 128 * sub + 8 * ((lane & 15) ^ sp_swz(kr));
      va[i] = (col < g.M) ? (uint32_t)(((long)kr * g.lda + col) * 2) : SMI_OOB;
    }
  }
  if (!BKM) {
    const int row = 16 * w + (lane >> 2);
    const int c = (lane & 3) ^ sp16_swz(row);
    vb = (n0 + row < g.N) ? (uint32_t)(((long)(n0 + row) * g.ldb + 8 * c) * 2) : SMI_OOB;
  } else {
    const int kr = 4 * w + (lane >> 4);
    const int col = n0 + 8 * ((lane & 15) ^ sp_swz(kr));
    vb = (col < g.N) ? (uint32_t)(((long)kr * g.ldb + col) * 2) : SMI_OOB;
  }
  f32x4_t acc[NB][NB], cacc[NB][NB];
  SpBiasSum16<NB> bsum;
  if constexpr (BIASG) bsum.init(lane);
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[i][j] = cacc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  auto issue = [&](int kt, int slot) {
    unsigned short* st = lds + slot * SP_ST256;
    const bool real = kt < nk;
    const int k0 = kt * KSTEP;
    const uint32_t sa = real ? (AK ? (uint32_t)((long)k0 * g.lda * 2) : (uint32_t)(k0 * 2)) : SMI_OOB;
    const uint32_t sb = real ? (BKM ? (uint32_t)((long)k0 * g.ldb * 2) : (uint32_t)(k0 * 2)) : SMI_OOB;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra[p], (sp_lds_void*)(st + p * APL + (2 * w + i) * 512), 16, va[i],
                                                 sa, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rb[p], (sp_lds_void*)(st + AOP + p * SP_PL + w * 512), 16, vb, sb, 0,
                                               0);
    }
  };
  auto frag_a = [&](const unsigned short* st, int c0) -> Split3 {
    // k-major A: sub-image c0 / 128 of each plane ([32][128] images SP_PL apart inside the plane)
    return AK ? frag16<true>(st + (c0 >> 7) * SP_PL, APL, c0 & 127, lane)
              : frag16<false>(st, APL, c0, lane);
  };
  issue(0, 0);
  issue(1, 1);
  for (int kt = 0; kt < nk; ++kt) {
    const int slot = kt & 1;
    // this wave's pieces of stage kt landed (3 DMA instructions per plane and stage; stage kt + 1's
    // still in flight)
    asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const unsigned short* st = lds + slot * SP_ST256;
    Split3 fa[NB], fb[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) fa[i] = frag_a(st, wm * 64 + i * 16);
#pragma unroll
    for (int j = 0; j < NB; ++j) fb[j] = frag16<BKM>(st + AOP, SP_PL, wn * 64 + j * 16, lane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave's reads of this stage retired -> refill it
    issue(kt + 2, slot);
    // product-major: consecutive MFMAs write different accumulators
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[i][j] = MF16(fa[i].h, fb[j].h, acc[i][j]);
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        cacc[i][j] = MF16(fa[i].l, fb[j].h, cacc[i][j]);
        cacc[i][j] = MF16(fa[i].m, fb[j].m, cacc[i][j]);
        cacc[i][j] = MF16(fa[i].h, fb[j].l, cacc[i][j]);
        cacc[i][j] = MF16(fa[i].m, fb[j].h, cacc[i][j]);
        cacc[i][j] = MF16(fa[i].h, fb[j].m, cacc[i][j]);
      }
    if constexpr (BIASG) {
#pragma unroll
      for (int i = 0; i < NB; ++i) bsum.add(i, fa[i]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  SP_STAMP(2);
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[i][j] += cacc[i][j];
  __syncthreads();
  float* ep = (float*)lds;
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ep[(wm * 64 + i * 16 + 4 * (lane >> 4) + r) * SP_EPI_PITCH + wn * 64 + j * 16 + (lane & 15)] = acc[i][j][r];
  __syncthreads();
  SP_STAMP(3);
  sp_store_tile<256, EPI, OUT>(g, ep, m0, n0);
  SP_STAMP(4);
  if constexpr (BIASG) {
    if (wn == 0) bsum.store(g, m0 + wm * 64, lane, (EPI & SE_ACC) != 0);
  }
}

template <bool AK, bool BKM, int EPI, int OUT>
__global__ __launch_bounds__(SP_NT, 1) void gemm_sp256m_kernel(GemmSpArgs g) {
  __shared__ __attribute__((aligned(16))) unsigned short lds[2 * SP_ST256];
  const int nwg = ((g.M + 255) / 256) * ((g.N + 127) / 128);
  gemm_sp_tile256m<AK, BKM, EPI, OUT>(g, smi_xcd_remap(blockIdx.x, nwg), lds);
}

// tile form of the large problems (SMI_SP_TM / gemm_sp_tm): 16 = 256-row tiles where they fill the
// chip (default), 128 = 128-row tiles only
int smi_sp_tm();
// 256 x 128 tiles when they fill the chip and do not lose a partial wave against 128 x 128 tiles:
// (M, N) = (8192, 1536) is 384 tiles of 256 rows (1.5 waves of 256 CUs) but 768 of 128 rows
// (3 full waves) — measured 87 vs 78 us (profiles/r3_gemm_sp_tiles_bench.log).
static inline bool sp_use256(int M, int N) {
  if (smi_sp_tm() == 128) return false;
  const long t256 = (long)((M + 255) / 256) * ((N + 127) / 128);
  const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
  if (t256 < SMI_NUM_CU) return false;
  const long w256 = (t256 + SMI_NUM_CU - 1) / SMI_NUM_CU, w128 = (t128 + SMI_NUM_CU - 1) / SMI_NUM_CU;
  return 2 * w256 <= w128;
}

// the launch of one FWD (BKM false) / DGRAD (BKM true) instance: grid tiles of 256 or 128 rows
template <bool BKM, int EPI, int OUT>
static inline void sp_launch(const GemmSpArgs& g, dim3 grid, bool t256, hipStream_t st) {
  if (t256) hipLaunchKernelGGL((gemm_sp256m_kernel<false, BKM, EPI, OUT>), grid, dim3(SP_NT), 0, st, g);
  else hipLaunchKernelGGL((gemm_sp_kernel<false, BKM, EPI, OUT>), grid, dim3(SP_NT), 0, st, g);
}

// Host-side checks shared by the launchers: 16-B aligned plane rows, descriptor-addressable
// extents (each plane has its own descriptor), chunk (8-element) granularity of each operand's
// contiguous dimension.  k-contig operand: [rows][K]; k-major operand: [K][cols].
static inline bool sp_operand_ok(const unsigned short* p, long ld, long ps, long rows, long cols, bool kmaj, int kpad,
                                 int K, int& bytes) {
  if (!p || ((uintptr_t)p & 15) || ld % 8 || ps % 8 || rows < 1 || cols < 1 || K < 1) return false;
  long ext;
  if (!kmaj) {  // K must be a multiple of 32 or the rows zero-padded to one
    const long kp = (K + 31) / 32 * 32;
    if (K % 32 && !(kpad && ld >= kp)) return false;
    if (ld < K) return false;
    ext = 2 * ((rows - 1) * ld + kp);
  } else {      // cols a multiple of 8 (16-B chunks)
    if (cols % 8 || ld < cols) return false;
    ext = 2 * ((long)(K - 1) * ld + cols);
  }
  if (ext >= (1L << 31)) return false;
  bytes = (int)ext;
  return true;
}
