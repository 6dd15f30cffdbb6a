/*
 * unsamflow_hip_hg.h — the homography smoothness loss of stage 2 (`hg`) of
 * libunsamflow_hip.so (same library and contract as unsamflow_hip.h: device
 * pointers to fp32 tensors, caller-allocated outputs, asynchronous on
 * `stream`, 0 / hipError_t / USF_EINVAL with usf_last_error_string()).
 *
 *   usf_hg_*  <- smooth_homography(flo, full_seg, occ_mask, thr)
 *                (losses/loss_blocks.py:125-200): per sample the six segments
 *                with the most occluded pixels get a homography fitted to
 *                their non-occluded ("reliable") pixels by RANSAC, and the loss
 *                is the L1 distance of the flow to that homography over the
 *                whole segment. The reference fits with cv2.findHomography on
 *                the host; here the fit is this library's own RANSAC
 *                (specified below), on the device, with no host sync.
 *
 * These entries have their own version (usf_hg_api_version) and do not change
 * USF_ABI_VERSION.
 *
 * ---------------------------------------------------------------- records --
 * A call's result is `records`: B * USF_HG_SLOTS records of USF_HG_RECORD_WORDS
 * 32-bit words, one per (sample, slot):
 *
 *   word 0      id       int    segment id of the slot (-1: empty slot)
 *   word 1      status   int    USF_HG_ACCEPTED ... USF_HG_EMPTY
 *   word 2      n_seg    int    pixels of the segment
 *   word 3      n_rel    int    reliable pixels of the segment
 *   word 4      n_inl    int    inliers of the refitted H among the reliable pixels
 *   word 5..13  H        float  row-major 3x3, H[8] = 1 (zeros unless a fit was made)
 *   word 14     best_j   int    index of the winning hypothesis (-1: none)
 *   word 15     offset   int    start of the slot's reliable-pixel list (workspace)
 *
 * Selection (per sample): a pixel is occluded iff occ != 0 and reliable iff
 * 1 - occ != 0. The candidates are the ids 1 .. K-1 (id 0 is the unsegmented
 * background); they are ordered by (occluded count descending, id ascending)
 * and the first USF_HG_SLOTS fill the slots in that order -- ids without an
 * occluded pixel, and ids without any pixel, included, as the reference's
 * argsort takes them. With K - 1 < USF_HG_SLOTS the rest are USF_HG_EMPTY.
 * Drop rules, in this order: n_rel < 4 -> USF_HG_FEW_RELIABLE;
 * 5 * n_rel < n_seg (share below 0.2) -> USF_HG_LOW_RELIABLE.
 *
 * ------------------------------------------------------------------- RANSAC --
 * For a slot that passed the drop rules, pts1 = the reliable pixels' (x, y) in
 * raster order and pts2 = pts1 + flow, both fp32 (x + flow_x rounded to fp32,
 * as the reference forms them).
 *
 * Hypothesis j in [0, n_hyp) draws four list positions q_t, t = 0..3:
 *
 *   mix(z):  z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *            z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)
 *            (splitmix64; all arithmetic modulo 2^64)
 *   c   = ((sample * 8 + slot) << 34) | (j << 2) | t
 *   q_t = ((mix(mix(seed) + c) >> 32) * n_rel) >> 32
 *
 * The 8x8 system of the four pairs in the h33 = 1 form
 *   [x y 1 0 0 0 -x*u -y*u] h = u,   [0 0 0 x y 1 -x*v -y*v] h = v
 * (rows 2t, 2t + 1 for pair t) is solved in fp64 by Gaussian elimination with
 * partial pivoting (first largest |pivot| from the top). A repeated position, a
 * pivot with |pivot| <= 1e-10 or a non-finite solution makes the hypothesis
 * invalid: it scores 0. The hypothesis is rounded to fp32.
 *
 * Score of a hypothesis = the number of reliable pairs with
 *   (X - u*Wd)^2 + (Y - v*Wd)^2 <= thr^2 * Wd^2  and  Wd != 0,
 *   (X, Y, Wd) = H * (x, y, 1)
 * (the squared transfer error against thr^2 without the divide), evaluated in
 * fp32 over ALL reliable pairs. The best hypothesis has the largest score, the
 * lowest j on ties; a best score below 4 makes the slot USF_HG_DEGENERATE.
 *
 * Refit: the inliers of the best hypothesis (the same test in fp64 on the fp32
 * hypothesis) are Hartley-normalised -- each point set moved to its centroid
 * and scaled to mean distance sqrt(2) -- and the inhomogeneous (h33 = 1)
 * least-squares problem is solved through its 8x8 normal equations, accumulated
 * and solved in fp64 by the same elimination (singular: |pivot| <= 1e-11 times
 * the largest diagonal entry), denormalised and divided by its last entry. All
 * sums are taken in one fixed order, so the result is the same bits from call
 * to call. Fewer than 4 inliers, a zero mean distance, a singular system or a
 * non-finite H make the slot USF_HG_DEGENERATE. H is rounded to fp32; n_inl is
 * the fp64 count of reliable pairs within thr of the rounded H; the slot is
 * USF_HG_ACCEPTED iff 2 * n_inl >= n_rel, else USF_HG_LOW_INLIER.
 *
 * cv2's adaptive iteration count and its Levenberg-Marquardt polish are out of
 * scope: this is a fixed-budget RANSAC with a linear refit.
 *
 * Why n_hyp = 256: a slot is only accepted at an inlier share >= 0.5, and at
 * that share a 4-point draw is all-inlier with probability >= 1/16, so the
 * chance that none of 256 draws is all-inlier is (15/16)^256 ~ 7e-8.
 */
#ifndef UNSAMFLOW_HIP_HG_H
#define UNSAMFLOW_HIP_HG_H

#include "unsamflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define USF_HG_API_VERSION 1

/* Largest number of segment ids K per call (== USF_SEGPOOL_MAX_K); a larger K is USF_EINVAL. */
#define USF_HG_MAX_K 1024
/* Segments refined per sample, and the words of one record. */
#define USF_HG_SLOTS 6
#define USF_HG_RECORD_WORDS 16
/* Default and largest number of hypotheses per slot. */
#define USF_HG_DEFAULT_HYP 256
#define USF_HG_MAX_HYP 65536

/* Record status. Only USF_HG_ACCEPTED slots enter the loss. */
#define USF_HG_ACCEPTED 0
#define USF_HG_FEW_RELIABLE 1  /* fewer than 4 reliable pixels */
#define USF_HG_LOW_RELIABLE 2  /* reliable share below 0.2 */
#define USF_HG_LOW_INLIER 3    /* inlier share of the refitted H below 0.5 */
#define USF_HG_DEGENERATE 4    /* no valid hypothesis or a singular refit (cv2 would return None) */
#define USF_HG_EMPTY 5         /* no candidate id left for this slot */

/* Device error flag (usf_device_errors): a pixel's segment id was negative,
 * >= K or not an integer. Such a pixel belongs to no segment: it is not
 * counted, not fitted and gets no loss or gradient. Nothing is indexed with it.
 * Like USF_DEVERR_SEGPOOL_BAD_ID it reports the caller's data: USF_SYNC_CHECK=1
 * does not turn it into USF_EDEVICE, and it stays set until usf_device_errors
 * clears it. */
#define USF_DEVERR_HG_BAD_ID 8

/* Version of the hg entries of the loaded library (== USF_HG_API_VERSION). */
int usf_hg_api_version(void);

/* Bytes of the `workspace` of usf_hg_fit_f32 (segment statistics, reliable-pixel
 * lists, hypotheses and their scores); 0 for arguments the fit would reject. */
long long usf_hg_workspace_bytes(int B, int H, int W, int K, int n_hyp);

/* Select the slots and fit their homographies (above). flow: [B,2,H,W] with
 * dense per-sample [2,H,W] blocks `flow_bstride` elements apart (so
 * flow[:, :2] and flow[:, 2:] of a [B,4,H,W] tensor are read in place); seg,
 * occ: [B,1,H,W] dense fp32, seg holding integer ids in [0, K). records:
 * B * USF_HG_SLOTS * USF_HG_RECORD_WORDS words, overwritten. workspace:
 * usf_hg_workspace_bytes bytes, 8-byte aligned, scratch of this call only.
 * K in [1, USF_HG_MAX_K], thr > 0, n_hyp in [1, USF_HG_MAX_HYP]. No host sync,
 * no float atomics; the records are bit-identical from call to call. workspace
 * needs no initialisation.
 * Alignment: flow 4 bytes (a channel slice); seg, occ 16 bytes; records 4
 * bytes; workspace 8 bytes. A misaligned pointer is USF_EINVAL. */
int usf_hg_fit_f32(const float* flow, long long flow_bstride, const float* seg, const float* occ, int K, float thr,
                   int n_hyp, unsigned long long seed, void* records, void* workspace, long long workspace_bytes,
                   int B, int H, int W, void* stream);

/* Doubles of the `partials` buffer of usf_hg_loss_fwd_f32; 0 for a bad shape. */
int usf_hg_loss_partials(int B, int H, int W);

/* out[0] = sum over the pixels p of the accepted slots' segments, occluded ones
 * included, of |dehom(H * (x, y, 1)) - (p + flow)| (both components) / (H * W * B).
 * H and p + flow are fp32 values, as the reference holds them; the per-pixel
 * arithmetic and the sums are fp64, combined in one fixed order.
 * H is a constant of the loss, as in the reference. partials: caller memory of
 * usf_hg_loss_partials doubles, 8-byte aligned, no initialisation needed,
 * scratch after return.
 * Alignment: flow, records, out 4 bytes; seg 16 bytes; partials 8 bytes. */
int usf_hg_loss_fwd_f32(const float* flow, long long flow_bstride, const float* seg, const void* records,
                        double* partials, float* out, int B, int H, int W, void* stream);

/* grad_flow[b,c,p] = -sign(diff_c) * grad_loss[0] / (H * W * B) on the accepted
 * slots' segments, sign(0) = 0, and 0 elsewhere; diff is recomputed from flow,
 * seg and the records. grad_loss: one device float; grad_flow: [B,2,H,W]
 * dense, overwritten.
 * Alignment: flow, records, grad_loss 4 bytes; seg, grad_flow 16 bytes. */
int usf_hg_loss_bwd_f32(const float* flow, long long flow_bstride, const float* seg, const void* records,
                        const float* grad_loss, float* grad_flow, int B, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNSAMFLOW_HIP_HG_H */
