// Launchers of conv16.hip for callers inside the library (cnn_encoder.hip): contracts at vsc_conv2d_nhwc_bf16 /
// vsc_stem_rows_u8 / vsc_maxpool3x3s2_nhwc_bf16 in include/vsc_hip.h.  Each names its refusal before anything is launched.
#pragma once
#include "common.h"

constexpr int VSC_STEM_KPAD = 192;   // 7 * 7 * 3 = 147 zero-padded to a multiple of the K-step of 64

// output extent of a convolution with padding (ksize - 1) / 2
int conv16_out_extent(int in, int ksize, int stride);
// res: optional residual in the operand type, added before the ReLU
int launch_conv16(const uint16_t *in, const uint16_t *wgt, const float *bias, const uint16_t *res, uint16_t *out, int64_t n, int h, int w, int cin, int cout, int ksize, int stride, int relu, hipStream_t stream);
// exactly one of frames_u8 [n, h, w, 3] (with mean / std, host arrays of 3) and frames_f32 [n, 3, h, w] (already normalised)
int launch_stem_rows(const uint8_t *frames_u8, const float *frames_f32, uint16_t *rows, int64_t n, int h, int w, const float *mean,
                     const float *std, hipStream_t stream);
int launch_maxpool3x3s2(const uint16_t *in, uint16_t *out, int64_t n, int h, int w, int c, hipStream_t stream);
