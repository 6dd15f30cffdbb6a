/*
 * unsamflow_hip_fakeobj.h — the key-object augmentation of the third pass of
 * libunsamflow_hip.so (same library and contract as unsamflow_hip.h: device
 * pointers to fp32 NCHW tensors, caller-allocated outputs, asynchronous on
 * `stream`, 0 / hipError_t / USF_EINVAL with usf_last_error_string()).
 *
 *   usf_fakeobj_paste_crop_f32 <- K rounds of add_fake_object
 *                                 (transforms/ar_transforms/oc_transforms.py:124-156,
 *                                 trainer/kitti_trainer_ar.py:192-226) on objects
 *                                 popped from the cache with ObjectCache.pop's
 *                                 mirror (trainer/object_cache.py:44-47), then
 *                                 random_crop, in one launch
 *   usf_fakeobj_push_*         <- ObjectCache.push of the step's key objects with
 *                                 their masked mean flow
 *                                 (kitti_trainer_ar.py:252-262, object_cache.py:51-88)
 *
 * The object cache lives on the device: cache_mask [cache_size,1,H,W], cache_img
 * [cache_size,3,H,W], cache_motion [cache_size,2], all dense fp32. Which slot is
 * read or written is the caller's bookkeeping, passed as int32 tables on the
 * device. These entries have their own version (usf_fakeobj_api_version) and do
 * not change USF_ABI_VERSION.
 */
#ifndef UNSAMFLOW_HIP_FAKEOBJ_H
#define UNSAMFLOW_HIP_FAKEOBJ_H

#include "unsamflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define USF_FAKEOBJ_API_VERSION 1

/* Largest number of rounds K per paste; a larger K is USF_EINVAL. */
#define USF_FAKEOBJ_MAX_K 8

/* Device error flag (usf_device_errors): a slot was outside [0, cache_size)
 * (and, for the push, not -1). Nothing is addressed with such a slot: the paste
 * skips that round of that sample, the push skips the sample. Like
 * USF_DEVERR_SEGPOOL_BAD_ID it reports the caller's data: USF_SYNC_CHECK=1 does
 * not turn it into USF_EDEVICE, and it stays set until usf_device_errors clears it. */
#define USF_DEVERR_FAKEOBJ_BAD_SLOT 16

/* Version of the fake-object entries of the loaded library (== USF_FAKEOBJ_API_VERSION). */
int usf_fakeobj_api_version(void);

/* K rounds of object insertion, then the crop. For round k = 0..K-1 in order,
 * sample b takes object j = k B + b: slot[j] names its cache entry and param[j] =
 * (sx, sy, flip, unused) what ObjectCache.pop drew for it: its motion is
 *   (mx, my) = (cache_motion[slot][0] * sx, cache_motion[slot][1] * sy)
 * (sx = sy = the random rescale, sx negated for a mirrored object; the motion
 * itself never leaves the device), and flip != 0 reads the stored mask and image
 * mirrored in x (column W-1-x). With m, s the (mirrored) mask and image:
 *   img1 = m s + (1 - m) img1
 *   m2 = flow_warp(m, const (-mx, -my), zeros), s2 = flow_warp(s, const (-mx, -my), border)
 *   img2 = m2 s2 + (1 - m2) img2
 *   flow = m (mx, my) + (1 - m) flow
 *   noc  = max(noc, m)
 * with flow_warp's coordinates as usf_warp_fwd_f32 forms them (align_corners,
 * the fp32 normalise / unnormalise round trip). The outputs are the window
 * [y0, y0+ch) x [x0, x0+cw) of the results: imgs_ot [B,6,ch,cw] (channels 0-2
 * img1, 3-5 img2), flow_ot [B,2,ch,cw], noc_ot [B,1,ch,cw], dense, overwritten;
 * only the window's pixels are computed. img1, img2: [B,3,H,W] dense; flow:
 * [B,2,H,W] with batch stride flow_bstride (a dense [2,H,W] block per sample);
 * noc: [B,1,H,W] dense; slot: K*B int32 and param: K*B*4 floats on the device.
 * The cache is only read. Outputs must not alias inputs or the cache.
 * 1 <= K <= USF_FAKEOBJ_MAX_K, H, W >= 2, cache_size >= 1, B <= 65535, and the
 * window must lie inside the image (0 <= y0, y0 + ch <= H, ch >= 1; likewise x):
 * anything else is USF_EINVAL before any launch. A slot outside [0, cache_size)
 * skips that round of that sample and raises USF_DEVERR_FAKEOBJ_BAD_SLOT.
 * Alignment: img1, img2, noc and the three outputs 16 bytes; flow (a channel
 * slice), the cache tensors (addressed in place, wherever the caller keeps
 * them), slot and param 4 bytes. A misaligned pointer is USF_EINVAL. */
int usf_fakeobj_paste_crop_f32(const float* img1, const float* img2, const float* flow, long long flow_bstride,
                               const float* noc, const float* cache_mask, const float* cache_img,
                               const float* cache_motion, const int* slot, const float* param, float* imgs_ot,
                               float* flow_ot, float* noc_ot, int B, int H, int W, int K, int cache_size, int y0,
                               int x0, int ch, int cw, void* stream);

/* Floats of the `partials` scratch of a push (0 for a non-positive size). */
int usf_fakeobj_push_partials(int B, int H, int W);

/* For every sample b with slot[b] >= 0: cache_mask[slot[b]] = obj_mask[b],
 * cache_img[slot[b]] = img[b] (bit copies) and
 *   cache_motion[slot[b]] = sum(flow[b] * obj_mask[b]) / sum(obj_mask[b])   per flow channel
 * (the products in fp32, the sums per workgroup in fp32 and then in one fixed
 * order in fp64: deterministic, no float atomics). sum(obj_mask[b]) == 0 is
 * outside the contract (the loader drops masks under 0.5 % of the image); the
 * motion written is then 0, not NaN. slot[b] == -1 skips sample b: no cache byte
 * is touched for it. Any other slot outside [0, cache_size) skips it too and
 * raises USF_DEVERR_FAKEOBJ_BAD_SLOT. Two samples of one call must not name the
 * same slot. obj_mask: [B,1,H,W] dense; img: [B,3,H,W] dense; flow: [B,2,H,W]
 * with batch stride flow_bstride; slot: B int32 on the device; partials: caller
 * scratch of usf_fakeobj_push_partials(B,H,W) floats (no initialisation needed,
 * scratch after return). The inputs must not alias the cache. B <= 65535.
 * Alignment: obj_mask, img, partials 16 bytes; flow (a channel slice), slot and
 * the cache tensors 4 bytes. */
int usf_fakeobj_push_f32(const float* obj_mask, const float* img, const float* flow, long long flow_bstride,
                         const int* slot, float* cache_mask, float* cache_img, float* cache_motion, float* partials,
                         int B, int H, int W, int cache_size, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UNSAMFLOW_HIP_FAKEOBJ_H */
