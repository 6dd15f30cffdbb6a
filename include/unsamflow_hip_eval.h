/*
 * unsamflow_hip_eval.h — validation on the device, part of libunsamflow_hip.so
 * (same library and contract as unsamflow_hip.h: device pointers to fp32 NCHW
 * tensors, caller-allocated outputs and scratch, asynchronous on `stream`,
 * 0 / hipError_t / USF_EINVAL with usf_last_error_string()).
 *
 *   usf_flow_resize_f32 <- resize_flow (utils/flow_utils.py:62-71): bilinear,
 *                          align_corners=True, then u divided by w/W and v by h/H,
 *                          to a size of its own per sample
 *   usf_flow_eval_f32   <- evaluate_flow (utils/flow_utils.py:117-201) for a
 *                          whole batch of ragged ground truths: the resize fused
 *                          into the error sums, the resized flow never stored
 *
 * Sizes. Sample b has the target size (H_b, W_b) = sizes[2 b], sizes[2 b + 1]
 * (int32 on the device; a null table: every sample is Hmax x Wmax). The batch
 * tensors are padded to [.., Hmax, Wmax] and sample b owns the window
 * [0, H_b) x [0, W_b) of its planes; nothing outside it is read or written.
 * Output pixel (Y, X) reads the prediction [h, w] at
 * (Y (h-1)/(H_b-1), X (w-1)/(W_b-1)), the ratios formed in fp32 as ATen's
 * align_corners bilinear forms them; the weights come from the floor of that
 * position, the upper tap is clamped to the last row / column; then channel 0 is
 * divided by (float)(w / W_b) and channel 1 by (float)(h / H_b) (quotients in
 * fp64 as the reference's Python forms them, the division itself in fp32).
 *
 * These entries have their own version (usf_eval_api_version) and do not change
 * USF_ABI_VERSION.
 */
#ifndef UNSAMFLOW_HIP_EVAL_H
#define UNSAMFLOW_HIP_EVAL_H

#include "unsamflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define USF_EVAL_API_VERSION 1

/* Columns of `sums` (per sample, fp32; epe = |resized prediction - gt|, occ = valid - noc):
 *   0 sum epe valid            1 sum valid
 *   2 sum epe noc              3 sum noc
 *   4 sum epe occ              5 sum occ
 *   6 sum epe valid move       7 sum valid move
 *   8 sum epe valid (1-move)   9 sum valid (1-move)
 *  10 bad pixels under valid  11 bad pixels under noc
 * A pixel is bad under mask m when epe m > 3 && epe m > 0.05f sqrtf(u_gt^2 + v_gt^2)
 * (flow_utils.py:119-124, in fp32). Columns 6-9 are 0 without a move mask. The
 * counts are exact integers (summed as integers, stored as fp32: below 2^24). */
#define USF_EVAL_NACC 12
/* Columns of `metrics` (per sample, fp32), the order evaluate_flow returns:
 * EPE_all, EPE_noc, EPE_occ, Fl_all, Fl_noc, EPE_move, EPE_static. */
#define USF_EVAL_NMETRIC 7

/* Device error flag (usf_device_errors): a sample's size was outside
 * [2, Hmax] x [2, Wmax]. Nothing is addressed with such a size: the sample is
 * skipped (the resize writes nothing for it; its sums are 0 and its metrics NaN).
 * Like USF_DEVERR_FAKEOBJ_BAD_SLOT it reports the caller's data: USF_SYNC_CHECK=1
 * does not turn it into USF_EDEVICE, and it stays set until usf_device_errors
 * clears it. */
#define USF_DEVERR_EVAL_BAD_SIZE 32

/* Version of the evaluation entries of the loaded library (== USF_EVAL_API_VERSION). */
int usf_eval_api_version(void);

/* out[b, :, 0:H_b, 0:W_b] = resize_flow(pred[b], (H_b, W_b)). pred: [B,2,h,w]
 * with batch stride pred_bstride (a dense [2,h,w] block per sample: a channel
 * slice of a [B,4,h,w] tensor qualifies); out: [B,2,Hmax,Wmax] dense. Sample b
 * writes only its own window; the rest of `out` is left untouched. sizes: B x 2
 * int32 on the device, or null. h, w, Hmax, Wmax >= 2 and 1 <= B <= 65535, else
 * USF_EINVAL before any launch. A size outside [2, Hmax] x [2, Wmax] skips the
 * sample and raises USF_DEVERR_EVAL_BAD_SIZE.
 * Alignment: out 16 bytes; pred (a channel slice) and sizes 4 bytes. A
 * misaligned pointer is USF_EINVAL. */
int usf_flow_resize_f32(const float* pred, long long pred_bstride, const int* sizes, float* out, int B, int h, int w,
                        int Hmax, int Wmax, void* stream);

/* Floats of the `partials` scratch of usf_flow_eval_f32 (0 for a non-positive size). */
int usf_flow_eval_partials(int B, int Hmax, int Wmax);

/* The error sums and metrics of every sample in two launches. gt: [B,Cg,Hmax,Wmax]
 * dense and planar, Cg = 2 (u, v; valid = noc = 1) or 4 (u, v, valid, noc);
 * move: [B,1,Hmax,Wmax] dense, or null; pred and sizes as above. Each pixel of a
 * sample's window contributes to the USF_EVAL_NACC sums above (the products in
 * fp32); they are summed per workgroup in fp32 into `partials`, then over the
 * workgroups in one fixed order in fp64: no float atomics, two runs agree bit
 * for bit. sums: [B,USF_EVAL_NACC]; metrics: [B,USF_EVAL_NMETRIC], the ratios
 * formed in fp64 and stored as fp32:
 *   EPE_all = s0/s1, EPE_noc = s2/s3, EPE_occ = s4/max(s5, 1),
 *   Fl_all = 100 s10/s1, Fl_noc = 100 s11/s3, EPE_move = s6/s7, EPE_static = s8/s9.
 * As in the reference an empty mask gives NaN (0/0) there, never an error;
 * EPE_occ alone is guarded. Without a move mask columns 5 and 6 are NaN. A
 * sample with a bad size has sums 0 and all seven metrics NaN, and raises
 * USF_DEVERR_EVAL_BAD_SIZE. partials: caller scratch of
 * usf_flow_eval_partials(B,Hmax,Wmax) floats (no initialisation needed, scratch
 * after return). h, w, Hmax, Wmax >= 2, Cg in {2, 4}, 1 <= B <= 65535, else
 * USF_EINVAL before any launch.
 * Alignment: gt, move, partials, sums, metrics 16 bytes; pred and sizes 4 bytes. */
int usf_flow_eval_f32(const float* pred, long long pred_bstride, const float* gt, int Cg, const float* move,
                      const int* sizes, float* partials, float* sums, float* metrics, int B, int h, int w, int Hmax,
                      int Wmax, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNSAMFLOW_HIP_EVAL_H */
