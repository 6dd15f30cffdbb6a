/*
 * unsamflow_hip_segpool.h — the mask-feature branch's per-segment max pool and
 * spread of libunsamflow_hip.so (same library and contract as unsamflow_hip.h:
 * device pointers to fp32 NCHW tensors, caller-allocated outputs, asynchronous
 * on `stream`, 0 / hipError_t / USF_EINVAL with usf_last_error_string()).
 *
 *   usf_segpool_*  <- onehot = F.one_hot(seg)
 *                     pooled = amax(onehot * proj[..., None], dim=(2, 3))
 *                     spread = (onehot * pooled[:, :, None, None, :]).sum(-1)
 *                     (models/pwclite.py:317-357, add_mask_corr)
 *
 * These entries have their own version (usf_segpool_api_version) and do not
 * change USF_ABI_VERSION.
 */
#ifndef UNSAMFLOW_HIP_SEGPOOL_H
#define UNSAMFLOW_HIP_SEGPOOL_H

#include "unsamflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define USF_SEGPOOL_API_VERSION 1

/* Largest number of segments K per call; a larger K is USF_EINVAL. */
#define USF_SEGPOOL_MAX_K 1024

/* Device error flag (usf_device_errors): a pixel's id was negative, >= K or not
 * an integer. Such a pixel belongs to no segment: spread = 0 there and it
 * neither receives nor contributes gradient. Nothing is indexed with it. Unlike
 * the other flags this one reports the caller's data, so USF_SYNC_CHECK=1 does
 * not turn it into USF_EDEVICE; it stays set until usf_device_errors clears it. */
#define USF_DEVERR_SEGPOOL_BAD_ID 4

/* Version of the segpool entries of the loaded library (== USF_SEGPOOL_API_VERSION). */
int usf_segpool_api_version(void);

/* 32-bit words of the `state` buffer of a [B,C,.,.] call with K segments (the
 * per-(sample, channel, segment) maxima and the per-(sample, segment) pixel
 * counts -- the only K-sized memory of the operation); 0 for B, C < 1 or K
 * outside [1, USF_SEGPOOL_MAX_K]. */
long long usf_segpool_state_words(int B, int C, int K);

/* spread[b,c,p] = pooled[b,c,seg[b,p]]. With S the pixels of sample b whose id
 * is k, n_in = |S| and m = max over S of proj[b,c,.]:
 *   pooled[b,c,k] = m          if S is the whole sample,
 *                   max(m, 0)  if 0 < n_in < H*W (the one-hot product's zeros),
 *                   0          if S is empty.
 * Comparisons and copies only: equal to the torch composition (a zero's sign
 * aside). proj, spread: [B,C,H,W] dense; seg: [B,1,H,W] dense fp32 holding
 * integer ids in [0, K) (see USF_DEVERR_SEGPOOL_BAD_ID). state: caller memory of
 * usf_segpool_state_words(B,C,K) words, 4-byte aligned, written here and read by
 * the backward. Deterministic: the tables are merged with integer atomics (max
 * of order-preserving keys, counts) only. NaNs in proj are not supported.
 * B, C <= 65535. state needs no initialisation: the call initialises it.
 * Alignment: proj, seg, spread 16 bytes; state 4 bytes. A misaligned pointer
 * is USF_EINVAL. */
int usf_segpool_fwd_f32(const float* proj, const float* seg, float* spread, void* state, int B, int C,
                        int H, int W, int K, void* stream);

/* The gradient of the above w.r.t. proj (none reaches seg). amax splits its
 * gradient evenly over all positions equal to the maximum, the zeros outside
 * the segment included. With G = sum over S of grad_spread[b,c,.], t = the
 * number of p in S with proj[b,c,p] == pooled[b,c,k] and z = H*W - n_in if
 * pooled[b,c,k] == 0, else 0:
 *   grad_proj[b,c,p] = G / (t + z)  if proj[b,c,p] == pooled[b,c,k],  else 0.
 * proj, seg and state as the forward saw / left them; grad_spread, grad_proj:
 * [B,C,H,W] dense, grad_proj overwritten. Deterministic: G is summed in one
 * fixed order (row order within a wave step, steps and waves in sequence), no
 * float atomics.
 * Alignment: proj, seg, grad_spread, grad_proj 16 bytes; state 4 bytes. */
int usf_segpool_bwd_f32(const float* proj, const float* seg, const void* state, const float* grad_spread,
                        float* grad_proj, int B, int C, int H, int W, int K, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNSAMFLOW_HIP_SEGPOOL_H */
