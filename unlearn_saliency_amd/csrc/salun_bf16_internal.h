// salun_bf16_internal.h - what salun_conv_bf16.hip (K11) and salun_gemm.hip (K16) share beyond the C-ABI: the plans, the
// device helpers, and K16's internal launch of the ring form of the convolution forward.
#pragma once
#include "salun_device.h"
#include "salun_bf16_plan.h"

// salun_gemm.hip (not exported): k_conv_bf16_ring<wgm, wgn, nst> on a forward convolution the plan gave that tile form
// (ring_tile); every pointer that is given lies on a 16-byte boundary.
int salun_conv_bf16_ring_launch(int wgm, int wgn, int nst, const uint16_t *x, const uint16_t *wp, const float *bias,
                                const float *nbias, const uint16_t *addend, uint16_t *y, int M, int H, int W, int C, int OH,
                                int OW, int K, int R, int stride, int pad, hipStream_t st);
