// salun_bf16_internal.h - what salun_conv_bf16.hip (K11) and salun_gemm.hip (K16) share beyond the C-ABI: the plans, the
// one launch helper of their dynamic-LDS kernels, and K16's internal launch of the ring form of the convolution forward.
#pragma once
#include "salun_common.h"
#include "salun_bf16_plan.h"

// salun_gemm.hip (not exported): k_conv_bf16_ring<wgm, wgn, nst> on a forward convolution the plan gave that tile form
// (ring_tile); every pointer that is given lies on a 16-byte boundary.
int salun_conv_bf16_ring_launch(int wgm, int wgn, int nst, const uint16_t *x, const uint16_t *wp, const float *bias,
                                const float *nbias, const uint16_t *addend, uint16_t *y, int M, int H, int W, int C, int OH,
                                int OW, int K, int R, int stride, int pad, hipStream_t st);

namespace {

// Launch of a kernel that needs more dynamic LDS than the default limit: the opt-in (hipFuncSetAttribute) is per device
// and is made once per kernel instantiation and device - the once-bits live in this function's instantiation.
template <auto Kernel, typename... Args>
int launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &...args) {
  static unsigned long long configured = 0;  // one bit per device: the opt-in is per device, not per process
  if (salun_once_needed(&configured)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
        hipSuccess)
      return SALUN_EIO;
    salun_once_mark(&configured);
  }
  hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

}  // namespace
