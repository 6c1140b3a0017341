// fp32 GEMM, FORWARD instances and the launcher; the design is described in smi_gemm_f32_impl.h.
#include "smi_gemm_f32_impl.h"

// fp32 product algorithm: 0 = f32 MFMA (v_mfma_f32_32x32x2_f32), 6 = 3-way bf16 split, 6 terms
// (SMI_F32_ALGO; see split3_8)
int smi_f32_launch_dgrad(const GemmF32Args& g, int fe, int algo, dim3 grid2, hipStream_t st);
int smi_f32_launch_wgrad(const GemmF32Args& g, int fe, int algo, dim3 grid2, hipStream_t st);

static int g_f32_algo = -1;
static int smi_f32_algo() {
  if (g_f32_algo < 0) {
    g_f32_algo = 6;
  }
  return g_f32_algo;
}
extern "C" int smi_gemm_f32_algo(int set) {  // set < 0: query only
  if (set == 0 || set == 6) g_f32_algo = set;
  return smi_f32_algo();
}

static int f32_ok(const GemmF32Args& g) {
  if (g.M < 1 || g.N < 1 || g.K < 1) return 0;
  const bool ak = g.mode == 2, bk = g.mode != 0;
  // float4 staging granularity along each operand's contiguous dimension, 16-B aligned rows
  if ((!ak && g.K % 4) || (ak && g.M % 4) || (!bk && g.K % 4) || (bk && g.N % 4)) return 0;
  if (g.lda % 4 || g.ldb % 4) return 0;
  if (((uintptr_t)g.A | (uintptr_t)g.B) & 15) return 0;
  return 1;
}

extern "C" int smi_gemm_f32(const GemmF32Args* args, hipStream_t st) {
  GemmF32Args g = *args;
  if (!f32_ok(g) || g.mode < 0 || g.mode > 2) return -1;
  const bool ak = g.mode == 2;
  if (g.splits < 1) g.splits = 1;
  if (g.splits > 1 && !g.atomic) return -1;
  int kps = (g.K / g.splits + FBK - 1) / FBK * FBK;
  if (kps < FBK) kps = FBK;
  g.k_per_split = kps;
  g.splits = (g.K + kps - 1) / kps;
  const dim3 block(256);
  {  // the software-pipelined one-wave-per-SIMD kernel
    const int nwg128 = ((g.M + 127) / 128) * ((g.N + FBN - 1) / FBN);
    const dim3 grid2((unsigned)(nwg128 * g.splits));
    // specialised epilogues for the feature sets the models use; anything else -> generic (-1)
    int fe = 0;
    if (g.mode == 0) {
      fe = (g.bias ? FE_BIAS : 0) | (g.relu == 1 ? FE_RELU : 0) | (g.relu == 2 ? FE_SIG : 0) | (g.thresh ? FE_DROP : 0);
    } else if (g.mode == 1) {
      fe = (g.resid ? FE_RESID : 0) | (g.dact_y ? FE_DACT : 0);
    }
    fe |= (g.atomic ? FE_ATOMIC : (g.beta_acc ? FE_ACC : 0));
// split path per mode (measured, tools/f32_split_check.py): FWD and DGRAD split once at staging
// into LDS bf16 planes (XS 2; the k-major DGRAD weight through ds_read_b64_tr_b16), WGRAD splits
// the fp32 fragments per wave (XS 1: 520 vs 563 us for a decoder layer's grouped launch)
#define F32P(AKV, BKV, E)                                                                          \
  do {                                                                                             \
    if (smi_f32_algo() == 0) hipLaunchKernelGGL((gemm_f32_pipe_kernel<AKV, BKV, E, 0>), grid2, block, 0, st, g); \
    else hipLaunchKernelGGL((gemm_f32_pipe_kernel<AKV, BKV, E, (AKV ? 1 : 2)>), grid2, block, 0, st, g); \
  } while (0)
    if (g.mode == 0) {
      switch (fe) {
        case 0: F32P(false, false, 0); break;
        case FE_BIAS: F32P(false, false, FE_BIAS); break;
        case FE_BIAS | FE_RELU: F32P(false, false, FE_BIAS | FE_RELU); break;
        case FE_BIAS | FE_RELU | FE_DROP: F32P(false, false, FE_BIAS | FE_RELU | FE_DROP); break;
        default: F32P(false, false, -1); break;
      }
    } else if (g.mode == 1) {
      return smi_f32_launch_dgrad(g, fe, smi_f32_algo(), grid2, st);  // csrc/kernels/gemm_f32_dgrad.hip
    } else {
      return smi_f32_launch_wgrad(g, fe, smi_f32_algo(), grid2, st);  // csrc/kernels/gemm_f32_wgrad.hip
    }
#undef F32P
    SMI_CHECK_LAUNCH();
  }
}

