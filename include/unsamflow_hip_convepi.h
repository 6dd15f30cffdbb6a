/*
 * unsamflow_hip_convepi.h — the convolution epilogues of libunsamflow_hip.so
 * (same library and contract as unsamflow_hip.h: device pointers to fp32 NCHW
 * tensors, caller-allocated outputs, asynchronous on `stream`, 0 / hipError_t /
 * USF_EINVAL with usf_last_error_string()).
 *
 *   usf_convepi_*  <- conv_block(...) = nn.Sequential(Conv2d(bias=True)[, LeakyReLU(0.1)])
 *                     (models/pwclite.py): the bias add and the activation after
 *                     a bias-free convolution, and their backward with the
 *                     bias gradient, one streaming pass each
 *
 * These entries have their own version (usf_convepi_api_version) and do not
 * change USF_ABI_VERSION.
 */
#ifndef UNSAMFLOW_HIP_CONVEPI_H
#define UNSAMFLOW_HIP_CONVEPI_H

#include "unsamflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define USF_CONVEPI_API_VERSION 1

/* The bias-gradient sum: a workgroup walks tiles of USF_CONVEPI_TILE_SLOTS
 * 16-byte slots, and each of a lane's 16 accumulators takes one term per tile,
 * at most USF_CONVEPI_CHAIN of them in sequence; everything after that is a
 * pairwise tree (accumulators, lanes, waves, and the parts of a split channel). */
#define USF_CONVEPI_TILE_SLOTS 1024
#define USF_CONVEPI_CHAIN 64
/* A workgroup takes one tile; only a shape with more than this many tiles over
 * all channels gives its workgroups several (up to USF_CONVEPI_CHAIN). */
#define USF_CONVEPI_TARGET_WGS 16384

/* Version of the convepi entries of the loaded library (== USF_CONVEPI_API_VERSION). */
int usf_convepi_api_version(void);

/* In place: y[b,c,:] = act(y[b,c,:] + bias[c]), act(v) = v > 0 ? v : v * slope,
 * the arithmetic of add_ followed by leaky_relu_ (bit-identical). slope == 1 is
 * no activation. y: [B,C,H,W] dense, 16-byte aligned; bias: [C], 4-byte
 * aligned. slope > 0. A misaligned pointer is USF_EINVAL. */
int usf_convepi_fwd_f32(float* y, const float* bias, int B, int C, int H, int W, float slope, void* stream);

/* Floats of `workspace` usf_convepi_bwd_f32 needs for the bias gradient of this
 * shape: C * parts where a channel's sum is split over parts > 1 workgroups, 0
 * where one workgroup owns a channel (a single launch); -1 for a shape the
 * backward does not take. */
long long usf_convepi_bwd_workspace(int B, int C, int H, int W);

/* The backward of the above.
 *   slope != 1: grad_in[b,c,:] = grad_out[b,c,:] * (y[b,c,:] > 0 ? 1 : slope)
 *               (leaky_relu_backward on the forward's result, bit-identical),
 *               written dense; grad_bias[c] = sum over b,h,w of grad_in.
 *   slope == 1: y and grad_in are NULL, nothing is written but
 *               grad_bias[c] = sum over b,h,w of grad_out.
 * grad_out: [B,C,H,W] with dense planes and a batch stride of gout_bstride
 * elements (>= C*H*W: a channel slice of a concat gradient), 4-byte aligned.
 * y, grad_in: dense, 16-byte aligned. grad_bias: [C], or NULL for no reduction
 * (slope != 1 only). workspace: usf_convepi_bwd_workspace floats (may be NULL
 * when that is 0 or grad_bias is NULL), no initialisation needed, contents
 * undefined on return. grad_bias, workspace: 4-byte aligned.
 * Deterministic: no atomics, the summation order depends on the shape only. */
int usf_convepi_bwd_f32(const float* grad_out, long long gout_bstride, const float* y, float* grad_in,
                        float* grad_bias, float* workspace, long long workspace_floats, int B, int C, int H, int W,
                        float slope, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNSAMFLOW_HIP_CONVEPI_H */
