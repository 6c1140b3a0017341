// LDS images of bf16 hi / mid / lo planes and their MFMA fragment reads, shared by the split-plane
// GEMM (smi_gemm_sp_impl.h), the split-at-stage fp32 GEMM (smi_gemm_f32_impl.h, XS = 2) and the
// transposing reads of the fp32 attention (csrc/kernels/attention_f32.hip).
//
// A plane tile is 32 k deep.  The XOR swizzles below are what the fragment reads undo; whoever
// fills an image (LDS-DMA source offsets, staging stores) applies the same functions.
//   k-contig image [rows][32 k]  : 64-B rows, 16-B chunk ^ (row >> 2) & 3 — conflict-free for the four
//                                  lane groups of a ds_read_b128 of 32x32x16 fragments (rows c0 +
//                                  (lane & 31), chunk 2 b + (lane >> 5)).  The 16x16x32 fragments (row
//                                  lane & 15, chunk lane >> 4) swizzle by S[(row >> 2) & 3], S = {0, 2, 3, 1}:
//                                  the 16-lane groups of a ds_read_b128 ({0-3, 12-15, 20-27}, ...) then
//                                  hit 16 distinct (row % 4, chunk) bank sets.
//   k-major image [32 k][128 cols]: 256-B k-rows, chunk ^ ((k & 3) << 2 | (k >> 2) & 3), read as
//                                  fragments by ds_read_b64_tr_b16 (both MFMA shapes).
#pragma once
#include "smi_common.h"
#include "smi_split3.h"

__device__ __forceinline__ int sp_off(int row, int k) {  // k % 4 == 0
  return row * 32 + ((((k >> 3) ^ (row >> 2)) & 3) << 3) + (k & 7);
}
__device__ __forceinline__ int sp16_swz(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }
__device__ __forceinline__ int sp16_off(int row, int k) {  // k % 8 == 0
  return row * 32 + ((((k >> 3) ^ sp16_swz(row)) & 3) << 3);
}
__device__ __forceinline__ int sp_swz(int k) { return ((k & 3) << 2) | ((k >> 2) & 3); }
__device__ __forceinline__ int sp_koff(int k, int col) {  // col % 4 == 0
  return k * 128 + ((((col >> 3) ^ sp_swz(k)) & 15) << 3) + (col & 7);
}

// Transposing 8-element read: two ds_read_b64_tr_b16.  Per 16-lane group, lane 4q + p addresses
// row q of a 4 x 16 block (elements 4p .. 4p + 3) and lane i receives column i; base + o0 / base + o1 address
// rows 0..3 / 4..7 of the lane's k-run.  Concatenated as one vector op so the two 64-bit reads
// land in adjacent registers.
typedef __attribute__((ext_vector_type(4))) short smi_s16x4_t;
__device__ __forceinline__ bf16x8_t lds_read_tr8(const unsigned short* base, int o0, int o1) {
  const smi_s16x4_t v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) smi_s16x4_t*)(base + o0));
  const smi_s16x4_t v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) smi_s16x4_t*)(base + o1));
  return __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
}
// the same read of the three planes (ps apart) at offsets o0 / o1
__device__ __forceinline__ Split3 lds_read_tr8x3(const unsigned short* img, int ps, int o0, int o1) {
  Split3 r;
  bf16x8_t* outs[3] = {&r.h, &r.m, &r.l};
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) {
    const unsigned short* base = img + pl * ps;
    *outs[pl] = lds_read_tr8(base, o0, o1);
  }
  return r;
}

// The three bf16x8 fragments of a 32-row (k-contig) / 32-column (k-major) block for
// v_mfma_f32_32x32x16_bf16: rows c0 + (lane & 31), k = 16 b + 8 (lane >> 5) + e.  ps = plane stride.
template <bool KMAJ>
__device__ __forceinline__ Split3 frag32(const unsigned short* __restrict__ img, int ps, int c0, int b, int lane) {
  Split3 r;
  if (!KMAJ) {
    const int o = sp_off(c0 + (lane & 31), 16 * b + 8 * (lane >> 5));
    r.h = *(const bf16x8_t*)(img + o);
    r.m = *(const bf16x8_t*)(img + ps + o);
    r.l = *(const bf16x8_t*)(img + 2 * ps + o);
  } else {
    // group g covers columns c0 + 16 (g & 1) + i and k-half g >> 1; the two reads give
    // k = 16 b + 8 h + 0..3 and + 4..7
    const int i = lane & 15, q = i >> 2, p = i & 3, g = lane >> 4;
    const int col = c0 + 16 * (g & 1) + 4 * p;
    const int kb = 16 * b + 8 * (g >> 1) + q;
    const int o0 = sp_koff(kb, col), o1 = sp_koff(kb + 4, col);
    bf16x8_t* outs[3] = {&r.h, &r.m, &r.l};
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
      const unsigned short* base = img + pl * ps;
      *outs[pl] = lds_read_tr8(base, o0, o1);
    }
  }
  return r;
}

// The same for v_mfma_f32_16x16x32_bf16: a 16-row / 16-column block, lane l holds row (column)
// c0 + (l & 15) at k = 8 (l >> 4) .. + 7 (the k-major reads of the two 32-lane groups cover k-rows
// {0-3, 8-11} / {16-19, 24-27}: 16 distinct physical chunks each).
template <bool KMAJ>
__device__ __forceinline__ Split3 frag16(const unsigned short* __restrict__ img, int ps, int c0, int lane) {
  Split3 r;
  if (!KMAJ) {
    const int o = sp16_off(c0 + (lane & 15), 8 * (lane >> 4));
    r.h = *(const bf16x8_t*)(img + o);
    r.m = *(const bf16x8_t*)(img + ps + o);
    r.l = *(const bf16x8_t*)(img + 2 * ps + o);
  } else {
    const int i = lane & 15, q = i >> 2, p = i & 3, g = lane >> 4;
    const int col = c0 + 4 * p;
    const int o0 = sp_koff(8 * g + q, col), o1 = sp_koff(8 * g + 4 + q, col);
    bf16x8_t* outs[3] = {&r.h, &r.m, &r.l};
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
      const unsigned short* base = img + pl * ps;
      *outs[pl] = lds_read_tr8(base, o0, o1);
    }
  }
  return r;
}
