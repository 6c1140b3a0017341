// Split-plane fp32 GEMM, DGRAD instances (dX = dY . W with the fused residual / relu'-dropout
// epilogues; the weight is read k-major through ds_read_b64_tr_b16).  See smi_gemm_sp_impl.h.
#include "smi_gemm_sp_impl.h"

int smi_sp_launch_dgrad(const GemmSpArgs& g, int epi, int out, dim3 grid, bool t256, hipStream_t st) {
  if (epi == 0 && out == SO_C) sp_launch<true, 0, SO_C>(g, grid, t256, st);
  else if (epi == SE_RESID && out == SO_C) sp_launch<true, SE_RESID, SO_C>(g, grid, t256, st);
  else if (epi == SE_DACT && out == SO_C) sp_launch<true, SE_DACT, SO_C>(g, grid, t256, st);
  // the FFN's hidden gradient dh feeds only linear1's dgrad / wgrad: planes (+ fp32 on request)
  else if (epi == SE_DACT && out == SO_P) sp_launch<true, SE_DACT, SO_P>(g, grid, t256, st);
  else if (epi == SE_DACT && out == (SO_C | SO_P)) sp_launch<true, SE_DACT, SO_C | SO_P>(g, grid, t256, st);
  // the attention output's gradient dO (out-projection dgrad): planes for the attention backward
  // kernels (+ fp32 when a kernel without plane inputs reads it)
  // linear2's dgrad on the FFN hidden mask instead of the fp32 activation
  else if (epi == SE_DMASK && out == SO_P) sp_launch<true, SE_DMASK, SO_P>(g, grid, t256, st);
  else if (epi == SE_DMASK && out == (SO_C | SO_P)) sp_launch<true, SE_DMASK, SO_C | SO_P>(g, grid, t256, st);
  else if (epi == 0 && out == SO_P) sp_launch<true, 0, SO_P>(g, grid, t256, st);
  else if (epi == 0 && out == (SO_C | SO_P)) sp_launch<true, 0, SO_C | SO_P>(g, grid, t256, st);
  else return -1;
  SMI_CHECK_LAUNCH();
}
