/*
 * unsamflow_hip_ar.h — the stage-1 "augmentation as regularisation" branch of
 * libunsamflow_hip.so (same library and contract as unsamflow_hip.h: device
 * pointers to fp32 NCHW tensors, caller-allocated outputs, asynchronous on
 * `stream`, 0 / hipError_t / USF_EINVAL with usf_last_error_string()).
 *
 *   usf_ar_transform_f32 <- RandomAffineFlow.transform_image / transform_flow
 *                           (transforms/ar_transforms/sp_transforms.py:260-290
 *                           with Interp2(clamp=False), interpolation.py:60-149)
 *                           for two frames, one flow and one mask, one launch
 *   usf_ar_loss_*        <- ((pred - target).abs() + ar_eps) ** ar_q * noc,
 *                           .mean() / (noc.mean() + 1e-7)
 *                           (trainer/kitti_trainer_ar.py:169-172, 244-247)
 *
 * These entries have their own version (usf_ar_api_version) and do not change
 * USF_ABI_VERSION.
 */
#ifndef UNSAMFLOW_HIP_AR_H
#define UNSAMFLOW_HIP_AR_H

#include "unsamflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define USF_AR_API_VERSION 1

/* Version of the AR entries of the loaded library (== USF_AR_API_VERSION). */
int usf_ar_api_version(void);

/* The spatial transform of both frames, the flow and the mask by per-sample
 * affine maps. theta: [2,B,6] on the device, theta[k][b] = (a1..a6) of frame
 * k + 1. With xx = 2/(W-1) x - 1, yy = 2/(H-1) y - 1, z = a1 a5 - a2 a4 an
 * output pixel (x, y) samples its source at
 *   xq = 0.5 (W-1) ((a5/z)(xx - a3) + (-a2/z)(yy - a6) + 1)
 *   yq = 0.5 (H-1) ((-a4/z)(xx - a3) + (a1/z)(yy - a6) + 1)
 * bilinearly with taps x0 = clamp(floor(xq), 0, W-1), x1 = clamp(x0 + 1, 0, W-1)
 * (likewise y), fractions xq - x0, yq - y0, and 0 where xq < 0, xq >= W,
 * yq < 0 or yq >= H. img1_t and mask_t use theta[0], img2_t theta[1]. flow_t
 * interpolates at theta[0]'s sample point the re-expressed flow
 *   new(u, v)(x, y) = T2(x + u, y + v) - T1(x, y),
 *   Tk(x, y) = (0.5 (W-1) (ak1 xx + ak2 yy + ak3 + 1), 0.5 (H-1) (ak4 xx + ak5 yy + ak6 + 1))
 * evaluated at each tap's integer position.
 * img1, img2: [B,3,H,W] dense; flow: [B,2,H,W] with batch stride flow_bstride
 * (a dense [2,H,W] block per sample); mask: [B,1,H,W] dense; noise1, noise2:
 * NULL, or [B,3,H,W] dense, already scaled: img_t = clamp(img_t + noise, 0, 1).
 * Outputs dense, overwritten; they must not alias the inputs. H, W >= 2.
 * Alignment: img1, img2, mask, noise1, noise2 and the four outputs 16 bytes;
 * flow (a channel slice) and theta 4 bytes. A misaligned pointer is USF_EINVAL. */
int usf_ar_transform_f32(const float* img1, const float* img2, const float* flow,
                         long long flow_bstride, const float* mask, const float* theta,
                         const float* noise1, const float* noise2, float* img1_t, float* img2_t,
                         float* flow_t, float* mask_t, int B, int H, int W, void* stream);

/* The AR loss:  l = (|pred - target| + eps)^q * noc  (noc broadcast over the 2
 * flow channels),  loss = mean(l over B*2*H*W) / (D + 1e-7),  D = mean(noc), or
 * *denom if denom is not NULL (a device scalar).
 * pred: [B,2,H,W] dense. target: [B,2,H,W] with batch / channel / row strides
 * (elements, >= 0) and unit column stride; noc: [B,1,H,W] with batch / row
 * strides and unit column stride -- a crop view is used in place. partials:
 * caller scratch of usf_ar_loss_partials(B,H,W) floats. out: 2 floats =
 * {loss, c}, c = 1 / (2 B H W (D + 1e-7)) (what the backward needs). q > 0,
 * eps >= 0. Deterministic: per-workgroup sums, then a fixed-order fp64
 * finalisation; no atomics. partials needs no initialisation and is scratch
 * after return.
 * Alignment: pred, target, noc (views), denom and out 4 bytes; partials 16 bytes. */
int usf_ar_loss_partials(int B, int H, int W);
int usf_ar_loss_fwd_f32(const float* pred, const float* target, long long target_bstride,
                        long long target_cstride, long long target_rstride, const float* noc,
                        long long noc_bstride, long long noc_rstride, const float* denom,
                        float* partials, float* out, int B, int H, int W, float eps, float q,
                        void* stream);

/* grad_pred = grad_loss * c * q (|d| + eps)^(q-1) sign(d) noc, d = pred - target,
 * sign(0) = 0: one dense pass recomputing from the forward's inputs. coef = the
 * forward's out; grad_loss: one float on the device; grad_pred: [B,2,H,W] dense,
 * overwritten. The gradient reaches pred only.
 * Alignment: pred, target, noc, coef, grad_loss 4 bytes; grad_pred 16 bytes. */
int usf_ar_loss_bwd_f32(const float* pred, const float* target, long long target_bstride,
                        long long target_cstride, long long target_rstride, const float* noc,
                        long long noc_bstride, long long noc_rstride, const float* coef,
                        const float* grad_loss, float* grad_pred, int B, int H, int W, float eps,
                        float q, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNSAMFLOW_HIP_AR_H */
