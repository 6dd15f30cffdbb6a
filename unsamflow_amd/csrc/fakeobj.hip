// Key-object augmentation of the third pass (add_fake_object,
// transforms/ar_transforms/oc_transforms.py:124-156, K rounds as
// trainer/kitti_trainer_ar.py:192-226, then random_crop) for gfx950 (CDNA4),
// reading the objects in place from a device-resident cache, and the push of a
// step's own key objects into that cache (kitti_trainer_ar.py:252-262,
// trainer/object_cache.py:51-88).
//
// Paste + crop. Every operation of add_fake_object is pointwise in the output
// pixel given the object's two bilinear taps, so one thread makes one pixel of
// the crop window: it loads the 9 base values (two frames, flow, noc) at
// (x0 + cx, y0 + cy), applies the K rounds in order in registers
//   img1 = m s + (1 - m) img1
//   m2 = warp(m, (-mx, -my), zeros), s2 = warp(s, (-mx, -my), border)
//   img2 = m2 s2 + (1 - m2) img2
//   flow = m (mx, my) + (1 - m) flow,   noc = max(noc, m)
// and stores the 9 cropped values. Round k of sample b reads object slot[k B + b]
// of the cache, with the motion cache_motion[slot] * (sx, sy) of param[k B + b]
// (the pop's random rescale); its x mirror is index arithmetic (column W-1-x of
// the stored row), applied to the pixel's own read and to each tap corner. The warp is
// flow_warp's coordinate chain (warp_tap.h: the fp32 normalise / unnormalise
// round trip) with the constant flow (-mx, -my); the taps of neighbouring lanes
// are neighbours, so the 4 shifted reads per channel hit the lines the wave
// just fetched. A workgroup lies inside one sample, so slot and motion are
// uniform. Contraction is off: the fp32 result is the torch composition's.
//
// Push. One pass over the sample copies the mask and the frame into their cache
// slot and sums m, u m, v m per workgroup; a fixed-order fp64 finalisation
// writes the masked mean flow into cache_motion[slot] (no float atomics; two
// runs agree bit for bit). slot = -1 skips the sample: no cache byte is touched.
//
// A slot outside [0, cache_size) is never dereferenced: the round (paste) or
// the sample (push) is skipped and USF_DEVERR_FAKEOBJ_BAD_SLOT raised.
#include <cstdint>

#include "usf_common.h"
#include "warp_tap.h"
#include "wave.h"

#include "../../include/unsamflow_hip_fakeobj.h"

namespace usf {
namespace {

constexpr int kNT = 256;    // threads per workgroup
constexpr int kPushPx = 4;  // pixels per thread of the push kernel (stride kNT)

// bad slots seen by this code object's kernels (usf_device_errors)
__device__ int g_fakeobj_errors = 0;

struct PasteArgs {
  const float *img1, *img2, *flow, *noc, *cmask, *cimg, *cmotion, *param;
  const int* slot;
  float *imgs_ot, *flow_ot, *noc_ot;
  long long fbs;  // flow batch stride (elements)
  int B, H, W, K, cache_size, y0, x0, ch, cw;
};

// the bilinear sample of one plane at a tap whose corner columns are mirrored when `flip`
__device__ __forceinline__ float tap_sample(const Tap& t, const float* __restrict__ pl, bool flip, int W) {
#pragma clang fp contract(off)
  const int xw = flip ? W - 1 - t.xw : t.xw, xe = flip ? W - 2 - t.xw : t.xw + 1;
  const int rn = t.yn * W, rs = rn + W;
  // a corner outside the image is never addressed
  const float vnw = t.m_nw ? pl[rn + xw] : 0.f;
  const float vne = t.m_ne ? pl[rn + xe] : 0.f;
  const float vsw = t.m_sw ? pl[rs + xw] : 0.f;
  const float vse = t.m_se ? pl[rs + xe] : 0.f;
  return vnw * (t.s * t.e) + vne * (t.s * t.w) + vsw * (t.n * t.e) + vse * (t.n * t.w);
}

__global__ __launch_bounds__(kNT) void fakeobj_paste_crop_kernel(PasteArgs a) {
  const int b = blockIdx.y, H = a.H, W = a.W, cHW = a.ch * a.cw;
  const size_t HWs = (size_t)H * W, cHWs = (size_t)cHW;
  const int cp = blockIdx.x * kNT + threadIdx.x;
  if (cp >= cHW) return;
  const int cy = cp / a.cw, cx = cp - cy * a.cw;
  const int X = a.x0 + cx, Y = a.y0 + cy, p = Y * W + X;

  float i1[3], i2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    i1[c] = a.img1[((size_t)b * 3 + c) * HWs + p];
    i2[c] = a.img2[((size_t)b * 3 + c) * HWs + p];
  }
  float fu = a.flow[(size_t)b * a.fbs + p], fv = a.flow[(size_t)b * a.fbs + HWs + p];
  float n = a.noc[(size_t)b * HWs + p];

  for (int k = 0; k < a.K; ++k) {
#pragma clang fp contract(off)
    const int j = k * a.B + b;  // uniform over the workgroup
    const int slot = a.slot[j];
    if ((unsigned)slot >= (unsigned)a.cache_size) {
      if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&g_fakeobj_errors, USF_DEVERR_FAKEOBJ_BAD_SLOT);
      continue;
    }
    // ObjectCache.pop: the stored motion times the drawn scale (x negated by the mirror)
    const float mx = a.cmotion[2 * (size_t)slot] * a.param[4 * j];
    const float my = a.cmotion[2 * (size_t)slot + 1] * a.param[4 * j + 1];
    const bool flip = a.param[4 * j + 2] != 0.f;
    const float* cm = a.cmask + (size_t)slot * HWs;
    const float* ci = a.cimg + (size_t)slot * 3 * HWs;
    const int q = Y * W + (flip ? W - 1 - X : X);
    const float m = cm[q], g = 1.0f - m;
    const Tap tz = make_tap(-mx, -my, X, Y, H, W, false);
    const Tap tb = make_tap(-mx, -my, X, Y, H, W, true);
    const float m2 = tap_sample(tz, cm, flip, W), g2 = 1.0f - m2;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* pl = ci + c * HWs;
      i1[c] = m * pl[q] + g * i1[c];
      i2[c] = m2 * tap_sample(tb, pl, flip, W) + g2 * i2[c];
    }
    fu = m * mx + g * fu;
    fv = m * my + g * fv;
    n = fmaxf(n, m);
  }

#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a.imgs_ot[((size_t)b * 6 + c) * cHWs + cp] = i1[c];
    a.imgs_ot[((size_t)b * 6 + 3 + c) * cHWs + cp] = i2[c];
  }
  a.flow_ot[(size_t)b * 2 * cHWs + cp] = fu;
  a.flow_ot[(size_t)b * 2 * cHWs + cHWs + cp] = fv;
  a.noc_ot[(size_t)b * cHWs + cp] = n;
}

// -------------------------------------------------------------------- push --
struct PushArgs {
  const float *mask, *img, *flow;
  const int* slot;
  float *cmask, *cimg;
  long long fbs;
  int B, H, W, cache_size, nchunk;
};

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int k = 0; k < kNT / 64; ++k) r += red[k];
  __syncthreads();
  return r;
}

// copies the chunk's pixels into slot[b]; partials[3 (b nchunk + chunk)] = {sum m, sum u m, sum v m}
__global__ __launch_bounds__(kNT) void fakeobj_push_kernel(PushArgs a, float* __restrict__ partials) {
  __shared__ float red[kNT / 64];
  const int b = blockIdx.y, HW = a.H * a.W;
  const size_t HWs = (size_t)HW;
  const int slot = a.slot[b];  // uniform over the workgroup
  if (slot == -1) return;
  if ((unsigned)slot >= (unsigned)a.cache_size) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&g_fakeobj_errors, USF_DEVERR_FAKEOBJ_BAD_SLOT);
    return;
  }
  const float* mk = a.mask + (size_t)b * HWs;
  const float* im = a.img + (size_t)b * 3 * HWs;
  const float* fl = a.flow + (size_t)b * a.fbs;
  float* cm = a.cmask + (size_t)slot * HWs;
  float* ci = a.cimg + (size_t)slot * 3 * HWs;
  float sm = 0.f, su = 0.f, sv = 0.f;
#pragma unroll
  for (int k = 0; k < kPushPx; ++k) {
#pragma clang fp contract(off)
    const int p = (blockIdx.x * kPushPx + k) * kNT + threadIdx.x;
    if (p < HW) {
      const float m = mk[p];
      cm[p] = m;
#pragma unroll
      for (int c = 0; c < 3; ++c) ci[c * HWs + p] = im[c * HWs + p];
      sm += m;
      su += fl[p] * m;
      sv += fl[HWs + p] * m;
    }
  }
  const float tm = block_sum(sm, red), tu = block_sum(su, red), tv = block_sum(sv, red);
  if (threadIdx.x == 0) {
    float* po = partials + 3 * ((size_t)b * a.nchunk + blockIdx.x);
    po[0] = tm;
    po[1] = tu;
    po[2] = tv;
  }
}

// cache_motion[slot[b]] = (sum u m, sum v m) / sum m, or 0 where sum m == 0.
// One workgroup per sample, fixed order, fp64.
__global__ __launch_bounds__(kNT) void fakeobj_push_final_kernel(const float* __restrict__ partials,
                                                                 const int* __restrict__ slots, int nchunk,
                                                                 int cache_size, float* __restrict__ cmotion) {
  __shared__ double red[3][kNT / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  const int slot = slots[b];
  if ((unsigned)slot >= (unsigned)cache_size) return;  // skipped (-1) or flagged by the copy pass
  const float* pp = partials + 3 * (size_t)b * nchunk;
  double s[3] = {0, 0, 0};
  for (int i = t; i < nchunk; i += kNT) {
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += pp[3 * i + c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) s[c] += __shfl_xor(s[c], sh);
    if ((t & 63) == 0) red[c][t >> 6] = s[c];
  }
  __syncthreads();
  if (t == 0) {
    double r[3] = {0, 0, 0};
    for (int k = 0; k < kNT / 64; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) r[c] += red[c][k];
    }
    const bool empty = !(r[0] != 0.0);
    cmotion[2 * (size_t)slot] = empty ? 0.f : (float)(r[1] / r[0]);
    cmotion[2 * (size_t)slot + 1] = empty ? 0.f : (float)(r[2] / r[0]);
  }
}

int push_chunks(int H, int W) { return (int)(((long long)H * W + kNT * kPushPx - 1) / (kNT * kPushPx)); }

}  // namespace

int fakeobj_device_errors(bool clear) { return read_clear_flags(HIP_SYMBOL(g_fakeobj_errors), clear); }

hipError_t fakeobj_paste_crop_launch(const float* img1, const float* img2, const float* flow, long long fbs,
                                     const float* noc, const float* cmask, const float* cimg, const float* cmotion,
                                     const int* slot, const float* param, float* imgs_ot, float* flow_ot,
                                     float* noc_ot, int B, int H, int W, int K, int cache_size, int y0, int x0, int ch,
                                     int cw, hipStream_t s) {
  PasteArgs a{};
  a.img1 = img1;
  a.img2 = img2;
  a.flow = flow;
  a.noc = noc;
  a.cmask = cmask;
  a.cimg = cimg;
  a.cmotion = cmotion;
  a.param = param;
  a.slot = slot;
  a.imgs_ot = imgs_ot;
  a.flow_ot = flow_ot;
  a.noc_ot = noc_ot;
  a.fbs = fbs;
  a.B = B;
  a.H = H;
  a.W = W;
  a.K = K;
  a.cache_size = cache_size;
  a.y0 = y0;
  a.x0 = x0;
  a.ch = ch;
  a.cw = cw;
  const dim3 grid((unsigned)(((long long)ch * cw + kNT - 1) / kNT), (unsigned)B);
  hipLaunchKernelGGL(fakeobj_paste_crop_kernel, grid, dim3(kNT), 0, s, a);
  return hipGetLastError();
}

int fakeobj_push_partials(int B, int H, int W) { return 3 * B * push_chunks(H, W); }

hipError_t fakeobj_push_launch(const float* mask, const float* img, const float* flow, long long fbs, const int* slot,
                               float* cmask, float* cimg, float* cmotion, float* partials, int B, int H, int W,
                               int cache_size, hipStream_t s) {
  PushArgs a{};
  a.mask = mask;
  a.img = img;
  a.flow = flow;
  a.slot = slot;
  a.cmask = cmask;
  a.cimg = cimg;
  a.fbs = fbs;
  a.B = B;
  a.H = H;
  a.W = W;
  a.cache_size = cache_size;
  a.nchunk = push_chunks(H, W);
  hipLaunchKernelGGL(fakeobj_push_kernel, dim3((unsigned)a.nchunk, (unsigned)B), dim3(kNT), 0, s, a, partials);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fakeobj_push_final_kernel, dim3((unsigned)B), dim3(kNT), 0, s, partials, slot, a.nchunk,
                     cache_size, cmotion);
  return hipGetLastError();
}

}  // namespace usf
