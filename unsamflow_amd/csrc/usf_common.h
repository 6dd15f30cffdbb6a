// Shared helpers for the gfx950 kernels of libunsamflow_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "unsamflow_hip.h"

namespace usf {

// Device-side error flags (warp.hip): read and optionally cleared after a
// stream sync; -1 if the sync or the copy failed. Only the flags in `mask` are
// reported and cleared.
int device_errors(hipStream_t s, bool clear, int mask = ~0);
// One code object's flag word (a __device__ int per source file: no relocatable
// device code): its flags in `mask`, cleared when `clear`; -1 if a copy failed.
template <class Sym>
int read_clear_flags(const Sym& word, bool clear, int mask = ~0) {
  int v = 0;
  if (hipMemcpyFromSymbol(&v, word, sizeof(int)) != hipSuccess) return -1;
  if (clear && (v & mask) != 0) {
    const int z = v & ~mask;
    if (hipMemcpyToSymbol(word, &z, sizeof(int)) != hipSuccess) return -1;
  }
  return v & mask;
}

// Thread-local error slot behind usf_last_error_string().
void set_error(const char* fmt, ...);
void clear_error();

// Round n up to a multiple of m (compile-time helper).
__host__ __device__ constexpr int round_up(int n, int m) { return ((n + m - 1) / m) * m; }

// Tuning override of usf_set_variant (op 0: corr fwd, 1: corr bwd, 2: warp grad_x; -1 = default).
int variant_override(int op);
int variant_count(int op);
void set_variant_override(int op, int index);

// Workgroups are dealt round-robin over the 8 XCDs, so blocks b and b + 8 share
// an L2 (MI355X_MICROARCH.md §Workgroup dispatch; a speed property, never a
// correctness one). Renumber the linear block id so that CONSECUTIVE work items
// -- which share staged data (a tile's displacement-row groups / channel
// groups, neighbouring tiles' halos) -- run on one XCD. Bijective on [0, n).
// Used by the correlation forward (L3 16.7 vs 18.6 us, FETCH traffic 3.9x -> 1.0x
// of algorithmic) and the photometric kernels. USF_XCD_REMAP=0
// (tools/ab_build.py A/B builds) turns it off.
#ifndef USF_XCD_REMAP
#define USF_XCD_REMAP 1
#endif
__device__ __forceinline__ int xcd_remap(int lin, int n) {
  if (!USF_XCD_REMAP) return lin;
  const int full = n & ~7;
  if (lin >= full) return lin;
  return (lin & 7) * (full >> 3) + (lin >> 3);
}

// Chunked variant: Q consecutive work items per XCD, chunks dealt round-robin
// (block lin runs on XCD lin % 8 and gets item Q (8 m + x) + j). Neighbouring
// items share one L2 a few at a time while every XCD still sees the whole
// range (a whole contiguous 1/8 per XCD -- xcd_remap -- measured slower for
// the correlation backward). Bijective on [0, n).
__device__ __forceinline__ int xcd_chunk(int lin, int n, int Q) {
  const int full = (n / (8 * Q)) * (8 * Q);
  if (Q <= 0 || lin >= full) return lin;
  const int x = lin & 7, r = lin >> 3;
  return Q * (8 * (r / Q) + x) + r % Q;
}

__device__ __forceinline__ int linear_block() {
  return blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
}

// Launchers implemented in the .hip files (corr.hip, warp.hip, occ.hip and the
// files named below). They assume validated arguments (capi.cpp checks shapes,
// d and pointers) and return the hipError_t of the launch.
// Correlation epilogues: output / gradient batch strides (elements; a channel
// slice of a concat buffer) and an optional LeakyReLU (act = 1, slope).
struct FwdEpi {
  long long out_bstride;
  int act;
  float slope;
  // channel split (set by the dispatcher): groups > 1 -> every workgroup sums
  // a channel group and writes raw partials to part[g][b][k][p]; a reduce
  // kernel applies the mean and the epilogue. Not part of the C ABI.
  float* part = nullptr;
  int groups = 1;
  // LeakyReLU sign mask (act != 0, W % 4 == 0): word [b][dy][y][x / 4] holds
  // bit 4 dx + (x % 4) = (activated output at (dy, dx, y, x) > 0). The backward
  // applies the derivative from it instead of re-reading the activated output.
  unsigned long long* mask = nullptr;
};
struct BwdEpi {
  long long g_bstride;
  const unsigned long long* mask = nullptr;  // FwdEpi::mask of the forward: derivative in the prologue
  float slope = 0.f;
};
// words of the sign mask (0: layout unsupported, W % 4 != 0)
long long corr_act_mask_words(int B, int H, int W, int d);
hipError_t leaky_bwd_gather_launch(const float* g, const float* act, long long g_bstride,
                                   float slope, float* out, int B, int K2, int H, int W,
                                   hipStream_t s);
hipError_t corr_fwd_launch(const float* x1, const float* x2, float* out, int B, int C,
                           int H, int W, int d, hipStream_t s, FwdEpi ep, float* workspace = nullptr,
                           long long workspace_floats = 0);
// floats of workspace that lets the forward split its channel loop (0: no split)
long long corr_fwd_workspace(int B, int C, int H, int W, int d);
hipError_t corr_bwd_launch(const float* x1, const float* x2, const float* gout,
                           float* gx1, float* gx2, int B, int C, int H, int W, int d,
                           hipStream_t s, BwdEpi ep);
// the decoder's x2 flow upsampling fused into the warp forward: up = [B,2,H,W]
// = F.interpolate(coarse * 2, scale_factor=2, bilinear, align_corners=True)
// of coarse = [B,2,H/2,W/2] (H, W even), out = flow_warp(x, up)
hipError_t warp_fwd_up_launch(const float* x, const float* coarse, float* up, float* out, int B, int C, int H, int W,
                              int pad_mode, hipStream_t s);
hipError_t warp_fwd_launch(const float* x, const float* flow, long long flow_bstride,
                           float* out, int B, int C, int H, int W, int pad_mode,
                           hipStream_t s);
hipError_t warp_bwd_launch(const float* x, const float* flow, long long flow_bstride,
                           const float* gout, float* gx, float* gflow, int B, int C, int H,
                           int W, int pad_mode, hipStream_t s, void* workspace = nullptr,
                           long long workspace_bytes = 0, bool persist = false);
// bytes of workspace for the binned-gather grad_x (usf_warp_bwd_ex_f32)
long long warp_bwd_workspace(int B, int H, int W);
// bytes of the persistent workspace of usf_warp_bwd_persist_f32
long long warp_bwd_persist_workspace(int B, int C, int H, int W);
// USF_SYNC_CHECK only: raise USF_DEVERR_WORKSPACE_DIRTY unless a persistent
// workspace is back in the state the next call expects (warp: the next call's
// count buffer, the dirty words and the overflow buffer all zero; occlusion:
// the splat map zero)
hipError_t warp_persist_check_launch(void* ws, int B, int C, int H, int W, hipStream_t s);
hipError_t zero_check_launch(const void* p, long long bytes, hipStream_t s);
// warp.hip: zero `bytes` (a multiple of 4) at p as a kernel on the stream, never a memset node
hipError_t zero_fill(void* p, size_t bytes, hipStream_t s);

// occ.hip: the forward splat and the occlusion masks
hipError_t splat_launch(const float* flow, long long flow_bstride, float* map, int B, int H, int W,
                        bool absolute, hipStream_t s);
hipError_t occ_backward_launch(const float* flow, long long flow_bstride, float* occ, int B, int H,
                               int W, float th, hipStream_t s);
hipError_t splat_scatter(const float* flow, long long flow_bstride, float* map, int B, int H, int W,
                         bool absolute, hipStream_t s);
hipError_t occ_vis_pair_persist_launch(const float* flow4, float* vis, float* map, int B, int H, int W, float th,
                                      hipStream_t s);
hipError_t occ_backward_persist_launch(const float* flow, long long flow_bstride, float* occ, float* map, int B,
                                       int H, int W, float th, hipStream_t s);
hipError_t occ_bidirection_launch(const float* flow12, long long bs12, const float* flow21, long long bs21,
                                  float* occ, int B, int H, int W, float scale, float bias, hipStream_t s);

// photo.hip: the L1 + SSIM photometric term; partials per direction
int photo_partials(int B, int H, int W);
hipError_t photo_fwd_launch(const float* src, const float* tgt, const float* mask, const float* flow,
                            long long flow_bstride, float* partials, float* out, float* basis, int B,
                            int C, int H, int W, int pad_mode, float w_l1, float w_ssim, hipStream_t s);
hipError_t photo_pair_fwd_launch(const float* im1, const float* im2, const float* mask1,
                                 const float* mask2, const float* flow, long long flow_bstride,
                                 float* partials, float* out, float* basis, int B, int C, int H,
                                 int W, int pad_mode, float w_l1, float w_ssim, hipStream_t s);
hipError_t photo_pyr_fwd_launch(int nscale, const float* const* im1, const float* const* im2,
                                const float* const* mask1, const float* const* mask2, const float* const* flow,
                                const long long* fbs, const int* H, const int* W, float* partials, float* out,
                                float* const* basis, int B, int C, int pad_mode, float w_l1, float w_ssim,
                                hipStream_t s);
// every scale's [B, 4 ndir, H, W] basis -> [B, 2 ndir, H, W] gradient in one launch (ndir = 1 or 2)
hipError_t photo_pyr_bwd_launch(int nscale, const float* const* basis, const float* coef, const float* gloss,
                                float* const* gflow, const int* H, const int* W, int B, int ndir, hipStream_t s);

// census.hip: the ternary (census) photometric term; partials per direction
int census_partials(int B, int H, int W);
hipError_t census_fwd_launch(const float* src, const float* tgt, const float* mask, const float* flow,
                             long long flow_bstride, float* partials, float* out, float* basis, int B, int H,
                             int W, int pad_mode, float w_ternary, hipStream_t s);
hipError_t census_pair_fwd_launch(const float* im1, const float* im2, const float* mask1, const float* mask2,
                                  const float* flow, long long flow_bstride, float* partials, float* out,
                                  float* basis, int B, int H, int W, int pad_mode, float w_ternary, hipStream_t s);
hipError_t census_pyr_fwd_launch(int nscale, const float* const* im1, const float* const* im2,
                                 const float* const* mask1, const float* const* mask2, const float* const* flow,
                                 const long long* fbs, const int* H, const int* W, float* partials, float* out,
                                 float* const* basis, int B, int pad_mode, float w_ternary, hipStream_t s);
// every scale's [B, 2 ndir, H, W] basis -> gradient in one launch (ndir = 1 or 2)
hipError_t census_pyr_bwd_launch(int nscale, const float* const* basis, const float* coef, const float* gloss,
                                 float* const* gflow, const int* H, const int* W, int B, int ndir, hipStream_t s);

// ar.hip: the stage-1 augmentation branch (spatial transform, AR loss)
hipError_t ar_transform_launch(const float* img1, const float* img2, const float* flow, long long flow_bstride,
                               const float* mask, const float* theta, const float* noise1, const float* noise2,
                               float* img1_t, float* img2_t, float* flow_t, float* mask_t, int B, int H, int W,
                               hipStream_t s);
int ar_loss_partials(int B, int H, int W);
hipError_t ar_loss_fwd_launch(const float* pred, const float* target, long long tbs, long long tcs, long long trs,
                              const float* noc, long long nbs, long long nrs, const float* denom, float* partials,
                              float* out, int B, int H, int W, float eps, float q, hipStream_t s);
hipError_t ar_loss_bwd_launch(const float* pred, const float* target, long long tbs, long long tcs, long long trs,
                              const float* noc, long long nbs, long long nrs, const float* coef, const float* gloss,
                              float* gpred, int B, int H, int W, float eps, float q, hipStream_t s);

// segpool.hip: the mask-feature branch's per-segment max pool and spread
int segpool_device_errors(bool clear);  // this code object's flags (device_errors() adds them)
long long segpool_state_words(int B, int C, int K);
hipError_t segpool_fwd_launch(const float* proj, const float* seg, float* spread, unsigned* state, int B, int C,
                              int H, int W, int K, hipStream_t s);
hipError_t segpool_bwd_launch(const float* proj, const float* seg, const unsigned* state, const float* gs, float* gp,
                              int B, int C, int H, int W, int K, hipStream_t s);

// hg.hip: the homography smoothness loss (segment selection, RANSAC fit, loss)
int hg_device_errors(bool clear);  // this code object's flags (device_errors() adds them)
long long hg_workspace_bytes(int B, int H, int W, int K, int n_hyp);
hipError_t hg_fit_launch(const float* flow, long long fbs, const float* seg, const float* occ, int K, float thr,
                         int n_hyp, unsigned long long seed, int* records, void* workspace, int B, int H, int W,
                         hipStream_t s);
int hg_loss_partials(int B, int H, int W);
hipError_t hg_loss_fwd_launch(const float* flow, long long fbs, const float* seg, const int* records, double* partials,
                              float* out, int B, int H, int W, hipStream_t s);
hipError_t hg_loss_bwd_launch(const float* flow, long long fbs, const float* seg, const int* records,
                              const float* gloss, float* gflow, int B, int H, int W, hipStream_t s);

// fakeobj.hip: the key-object augmentation (paste + crop from the device cache, push into it)
int fakeobj_device_errors(bool clear);  // this code object's flags (device_errors() adds them)
hipError_t fakeobj_paste_crop_launch(const float* img1, const float* img2, const float* flow, long long fbs,
                                     const float* noc, const float* cmask, const float* cimg, const float* cmotion,
                                     const int* slot, const float* param, float* imgs_ot, float* flow_ot,
                                     float* noc_ot, int B, int H, int W, int K, int cache_size, int y0, int x0, int ch,
                                     int cw, hipStream_t s);
int fakeobj_push_partials(int B, int H, int W);
hipError_t fakeobj_push_launch(const float* mask, const float* img, const float* flow, long long fbs, const int* slot,
                               float* cmask, float* cimg, float* cmotion, float* partials, int B, int H, int W,
                               int cache_size, hipStream_t s);

// eval.hip: validation (per-sample flow resize; the fused EPE / Fl sums and their finalisation)
int eval_device_errors(bool clear);  // this code object's flags (device_errors() adds them)
hipError_t flow_resize_launch(const float* pred, long long pbs, const int* sizes, float* out, int B, int h, int w,
                              int Hmax, int Wmax, hipStream_t s);
int flow_eval_partials(int B, int Hmax, int Wmax);
hipError_t flow_eval_launch(const float* pred, long long pbs, const float* gt, int Cg, const float* move,
                            const int* sizes, float* partials, float* sums, float* metrics, int B, int h, int w,
                            int Hmax, int Wmax, hipStream_t s);

// convepi.hip: the conv epilogues (bias + LeakyReLU in place; their backward with the bias gradient)
long long convepi_bwd_workspace(int B, int C, int H, int W);  // floats; -1: shape not taken
hipError_t convepi_fwd_launch(float* y, const float* bias, int B, int C, int H, int W, float slope, hipStream_t s);
hipError_t convepi_bwd_launch(const float* gout, long long gbs, const float* y, float* gin, float* gbias,
                              float* workspace, int B, int C, int H, int W, float slope, hipStream_t s);

hipError_t upsample_fwd_launch(const float* x, float* out, int B, int C, int H, int W, int k,
                               hipStream_t s);
hipError_t upsample_bwd_launch(const float* gout, float* gx, int B, int C, int H, int W, int k,
                               hipStream_t s, const float* gout2 = nullptr);
int convex_pyramid_max_levels();
hipError_t convex_pyr_fwd_launch(int n, const float* const* flow, const float* const* mask, float* const* out,
                                 const int* H, const int* W, int B, int factor, float mask_scale, hipStream_t s);
hipError_t convex_pyr_bwd_launch(int n, const float* const* flow, const float* const* mask,
                                 const float* const* gout, float* const* gflow, float* const* gmask, float* scratch,
                                 const int* H, const int* W, int B, int factor, float mask_scale, hipStream_t s);
bool convex_factor_ok(int factor);
long long convex_bwd_scratch(int B, int H, int W);
hipError_t convex_fwd_launch(const float* flow, const float* mask, float* out, int B, int H, int W,
                             int factor, float mask_scale, hipStream_t s);
hipError_t convex_bwd_launch(const float* flow, const float* mask, const float* gout, float* gflow,
                             float* gmask, float* scratch, int B, int H, int W, int factor,
                             float mask_scale, hipStream_t s);
hipError_t stream_copy_launch(const float* src, float* dst, long long n, hipStream_t s);
hipError_t area_pyramid_launch(const float* x, float* o1, float* o2, float* o3, long long planes,
                               int H, int W, hipStream_t s);

}  // namespace usf
