/*
 * unsamflow_hip_census.h — the ternary (soft census) photometric term of
 * libunsamflow_hip.so, the companion of the usf_photo_loss_* entries of
 * unsamflow_hip.h (same library, same contract: device pointers to fp32 NCHW
 * tensors, caller-allocated outputs, asynchronous on `stream`, 0 / hipError_t /
 * USF_EINVAL with usf_last_error_string()).
 *
 *   usf_census_loss_* <- the w_ternary term of loss_photomatric
 *                        (losses/flow_loss.py:33-50) with TernaryLoss
 *                        (losses/loss_blocks.py:12-50, max_distance = 1) on the
 *                        warped image of losses/flow_loss.py:127-148; the
 *                        reference's stage-1 loss (configs/*_base.json
 *                        train.stage1.loss: w_ternary = 1, w_l1 = w_ssim = 0)
 *
 * These entries have their own version (usf_census_api_version) and do not
 * change USF_ABI_VERSION.
 */
#ifndef UNSAMFLOW_HIP_CENSUS_H
#define UNSAMFLOW_HIP_CENSUS_H

#include "unsamflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define USF_CENSUS_API_VERSION 1

/* Version of the census entries of the loaded library (== USF_CENSUS_API_VERSION). */
int usf_census_api_version(void);

/* Fused occlusion-aware census loss of one scale and direction:
 *   rec = flow_warp(src, flow, pad_mode);  x = rec * m,  y = tgt * m
 *   L = w_ternary * mean_{b,p} TernaryLoss(x, y) / (mean m + 1e-6)
 * src, tgt: [B,3,H,W] dense (C must be 3; H, W >= 3); mask: [B,1,H,W] dense;
 * flow: [B,2,H,W] with batch stride flow_bstride. partials: caller scratch of
 * usf_census_loss_partials(B,H,W) floats (per direction). out: 2 floats =
 * {L, c_t} (c_t is what the backward needs). grad_basis: NULL (no gradient
 * wanted), or [B,2,H,W] dense, overwritten with the per-pixel flow-gradient
 * basis: dL/dflow = c_t * basis (L is linear in the census sum), computed in
 * the same pass. Deterministic (fixed-order sums, no atomics). partials needs
 * no initialisation and is scratch after return.
 * Alignment (every usf_census_loss_*_fwd entry, per scale in the pyramid
 * form): the images, the masks, partials and grad_basis 16 bytes; flow 4 bytes
 * (a channel slice); out 4 bytes. A misaligned pointer is USF_EINVAL. */
int usf_census_loss_partials(int B, int H, int W);
int usf_census_loss_fwd_f32(const float* src, const float* tgt, const float* mask,
                            const float* flow, long long flow_bstride, float* partials,
                            float* out, float* grad_basis, int B, int C, int H, int W,
                            int pad_mode, float w_ternary, void* stream);

/* Both directions of a with_bk scale in one launch: direction 0 warps im2 by
 * flow[:, 0:2] onto im1 under mask1, direction 1 warps im1 by flow[:, 2:4] onto
 * im2 under mask2. flow: [B,4,H,W] with batch stride flow_bstride >= 4*H*W
 * (dense [4,H,W] per sample); partials: 2 * usf_census_loss_partials(B,H,W)
 * floats; out: 4 floats {L, c_t} per direction; grad_basis: NULL or
 * [B,2,2,H,W] dense. The same numbers as the two one-direction calls. */
int usf_census_loss_pair_fwd_f32(const float* im1, const float* im2, const float* mask1,
                                 const float* mask2, const float* flow, long long flow_bstride,
                                 float* partials, float* out, float* grad_basis, int B, int C,
                                 int H, int W, int pad_mode, float w_ternary, void* stream);

/* grad_flow = c_t * grad_basis * grad_loss per direction: grad_basis
 * [B,2*ndir,H,W], coef = the forward's out (2 floats per direction), grad_loss:
 * ndir floats on the device, grad_flow: [B,2*ndir,H,W] dense, overwritten.
 * ndir = 1 or 2.
 * Alignment (this and the pyramid backward, per scale): grad_basis, grad_flow
 * 16 bytes; coef, grad_loss 4 bytes. */
int usf_census_loss_bwd_f32(const float* grad_basis, const float* coef, const float* grad_loss,
                            float* grad_flow, int B, int H, int W, int ndir, void* stream);

/* usf_census_loss_pair_fwd_f32 for 1 <= nscale <= 4 loss scales in ONE launch
 * (host arrays of nscale device pointers / sizes; give the largest scale
 * first). partials: usf_census_loss_pyramid_partials(nscale,H,W,B) floats;
 * out: nscale * 4 floats ({L, c_t} per direction per scale); grad_basis: NULL
 * or nscale pointers to [B,2,2,H_k,W_k]. Bit-identical to the per-scale calls. */
long long usf_census_loss_pyramid_partials(int nscale, const int* H, const int* W, int B);
int usf_census_loss_pyramid_fwd_f32(int nscale, const float* const* im1, const float* const* im2,
                                    const float* const* mask1, const float* const* mask2,
                                    const float* const* flow, const long long* flow_bstride,
                                    const int* H, const int* W, float* partials,
                                    long long partials_floats, float* out, float* const* grad_basis,
                                    int B, int C, int pad_mode, float w_ternary, void* stream);

/* The backward of every scale of usf_census_loss_pyramid_fwd_f32 in one launch:
 * coef = its out (nscale * 4 floats), grad_loss: nscale * 2 floats on the
 * device, grad_flow: nscale pointers to [B,4,H_k,W_k] dense, overwritten. */
int usf_census_loss_pyramid_bwd_f32(int nscale, const float* const* grad_basis, const float* coef,
                                    const float* grad_loss, float* const* grad_flow, const int* H,
                                    const int* W, int B, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNSAMFLOW_HIP_CENSUS_H */
