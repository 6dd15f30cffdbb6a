// The stage-1 "augmentation as regularisation" branch (ARFlow) for gfx950
// (CDNA4): the spatial transform of RandomAffineFlow
// (transforms/ar_transforms/sp_transforms.py, interpolation.py) for two frames,
// one flow and one mask in ONE launch, and the AR loss of
// trainer/kitti_trainer_ar.py:169-172 / 244-247 as a forward and a backward pass.
//
// Transform. theta = (a1..a6) per sample and frame. For an output pixel (x, y):
//   xx = 2/(W-1) x - 1, yy = 2/(H-1) y - 1, z = a1 a5 - a2 a4
//   xq = 0.5 (W-1) ((a5/z)(xx - a3) + (-a2/z)(yy - a6) + 1)        (transform_coords)
//   yq = 0.5 (H-1) ((-a4/z)(xx - a3) + (a1/z)(yy - a6) + 1)
//   x0 = clamp(floor(xq), 0, W-1), x1 = clamp(x0 + 1, 0, W-1), fx = xq - x0  (Interp2, clamp=False)
//   out = (1-fy)(1-fx) v00 + (1-fy) fx v01 + fy (1-fx) v10 + fy fx v11, 0 where (xq, yq) is outside
// img1_t and mask_t sample at theta1's coordinates, img2_t at theta2's. flow_t
// samples, at theta1's coordinates, the re-expressed flow
//   new(u, v)(x, y) = T2(x + u, y + v) - T1(x, y),   Tk = denorm(ak1 xx + ak2 yy + ak3, ak4 xx + ak5 yy + ak6)
// (transform_flow, inverse_transform_coords), evaluated at each tap's integer
// position, so that field never reaches memory. One thread makes one output
// pixel of all 9 planes; a workgroup lies inside one sample, so theta is
// uniform; every store is a coalesced row segment. The taps of neighbouring
// pixels are neighbours (the maps are near-identity affine), so the gathers
// read whole cache lines. The arithmetic keeps the reference's operation order
// with contraction off: the fp32 result is the torch composition's.
//
// Loss. l = (|pred - target| + eps)^q noc, loss = mean(l) / (D + 1e-7),
// D = mean(noc) or a caller's device scalar. Forward: one pass writing per-
// workgroup partial sums, then a fixed-order fp64 finalisation (no float
// atomics; two runs agree bit for bit). Backward: one dense pass recomputing
// from pred, target and noc; sign(0) = 0; q == 1 takes a path without powf.
#include <cstdint>

#include "usf_common.h"

namespace usf {
namespace {

constexpr int kNT = 256;   // threads per workgroup
constexpr int kLossPx = 4;  // pixels per thread of the loss kernels (stride kNT)

// per-sample, per-frame coordinate maps (uniform over a workgroup)
struct Affine {
  float a1, a2, a3, a4, a5, a6;  // the forward map of inverse_transform_coords
  float b1, b2, b4, b5;          // its inverse's linear part (transform_coords)
};

__device__ __forceinline__ Affine load_affine(const float* __restrict__ t) {
#pragma clang fp contract(off)
  Affine m;
  m.a1 = t[0];
  m.a2 = t[1];
  m.a3 = t[2];
  m.a4 = t[3];
  m.a5 = t[4];
  m.a6 = t[5];
  const float z = m.a1 * m.a5 - m.a2 * m.a4;
  m.b1 = m.a5 / z;
  m.b2 = -m.a2 / z;
  m.b4 = -m.a4 / z;
  m.b5 = m.a1 / z;
  return m;
}

// the four taps of Interp2(clamp=False) at (xq, yq)
struct Taps {
  int x0, x1, y0, y1;
  float w00, w01, w10, w11;
  bool valid;
};

__device__ __forceinline__ Taps make_taps(const Affine& m, float xx, float yy, float hx, float hy, int H, int W) {
#pragma clang fp contract(off)
  const float xhat = xx - m.a3, yhat = yy - m.a6;
  const float xq = hx * ((m.b1 * xhat + m.b2 * yhat) + 1.0f);
  const float yq = hy * ((m.b4 * xhat + m.b5 * yhat) + 1.0f);
  Taps t;
  // the comparisons are false for NaN (a singular theta): such a pixel keeps
  // its in-range clamped taps, as the reference does
  t.valid = !(xq < 0.f || xq >= (float)W || yq < 0.f || yq >= (float)H);
  const float fx0 = fminf(fmaxf(floorf(xq), 0.f), (float)(W - 1));
  const float fy0 = fminf(fmaxf(floorf(yq), 0.f), (float)(H - 1));
  t.x0 = min(max((int)fx0, 0), W - 1);
  t.y0 = min(max((int)fy0, 0), H - 1);
  t.x1 = min(t.x0 + 1, W - 1);
  t.y1 = min(t.y0 + 1, H - 1);
  const float fx = xq - (float)t.x0, fy = yq - (float)t.y0;
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  t.w00 = gy * gx;
  t.w01 = gy * fx;
  t.w10 = fy * gx;
  t.w11 = fy * fx;
  return t;
}

__device__ __forceinline__ float blend(const Taps& t, float v00, float v01, float v10, float v11) {
#pragma clang fp contract(off)
  const float v = v00 * t.w00 + v01 * t.w01 + v10 * t.w10 + v11 * t.w11;
  return t.valid ? v : 0.f;
}

__device__ __forceinline__ float gather(const Taps& t, const float* __restrict__ p, int W) {
  const float* r0 = p + (size_t)t.y0 * W;
  const float* r1 = p + (size_t)t.y1 * W;
  return blend(t, r0[t.x0], r0[t.x1], r1[t.x0], r1[t.x1]);
}

struct TransformArgs {
  const float *img1, *img2, *flow, *mask, *theta, *noise1, *noise2;
  float *img1_t, *img2_t, *flow_t, *mask_t;
  long long fbs;  // flow batch stride (elements)
  int B, H, W;
  float sx, sy, hx, hy;  // 2/(W-1), 2/(H-1), 0.5 (W-1), 0.5 (H-1) rounded from double
};

__global__ __launch_bounds__(kNT) void ar_transform_kernel(TransformArgs a) {
  const int b = blockIdx.y, H = a.H, W = a.W, HW = H * W;
  const int p = blockIdx.x * kNT + threadIdx.x;
  if (p >= HW) return;
  const int y = p / W, x = p - y * W;
  const Affine m1 = load_affine(a.theta + (size_t)b * 6);
  const Affine m2 = load_affine(a.theta + ((size_t)a.B + b) * 6);
  float xx, yy;
  {
#pragma clang fp contract(off)
    xx = a.sx * (float)x - 1.0f;
    yy = a.sy * (float)y - 1.0f;
  }
  const Taps t1 = make_taps(m1, xx, yy, a.hx, a.hy, H, W);
  const Taps t2 = make_taps(m2, xx, yy, a.hx, a.hy, H, W);
  const size_t HWs = (size_t)HW, o3 = (size_t)b * 3 * HWs + p;

#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v1 = gather(t1, a.img1 + (size_t)b * 3 * HWs + c * HWs, W);
    float v2 = gather(t2, a.img2 + (size_t)b * 3 * HWs + c * HWs, W);
    if (a.noise1) v1 = fminf(fmaxf(v1 + a.noise1[o3 + c * HWs], 0.f), 1.f);
    if (a.noise2) v2 = fminf(fmaxf(v2 + a.noise2[o3 + c * HWs], 0.f), 1.f);
    a.img1_t[o3 + c * HWs] = v1;
    a.img2_t[o3 + c * HWs] = v2;
  }
  a.mask_t[(size_t)b * HWs + p] = gather(t1, a.mask + (size_t)b * HWs, W);

  // the re-expressed flow at the four integer taps of theta1's sample point
  const float* fu = a.flow + (size_t)b * a.fbs;
  const float* fv = fu + HWs;
  float nu[4], nv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma clang fp contract(off)
    const int tx = (k & 1) ? t1.x1 : t1.x0, ty = (k & 2) ? t1.y1 : t1.y0;
    const size_t o = (size_t)ty * W + tx;
    const float u = fu[o], v = fv[o];
    const float gx0 = a.sx * (float)tx - 1.0f, gy0 = a.sy * (float)ty - 1.0f;
    const float gx1 = a.sx * ((float)tx + u) - 1.0f, gy1 = a.sy * ((float)ty + v) - 1.0f;
    const float X0 = a.hx * (((m1.a1 * gx0 + m1.a2 * gy0) + m1.a3) + 1.0f);
    const float Y0 = a.hy * (((m1.a4 * gx0 + m1.a5 * gy0) + m1.a6) + 1.0f);
    const float X1 = a.hx * (((m2.a1 * gx1 + m2.a2 * gy1) + m2.a3) + 1.0f);
    const float Y1 = a.hy * (((m2.a4 * gx1 + m2.a5 * gy1) + m2.a6) + 1.0f);
    nu[k] = X1 - X0;
    nv[k] = Y1 - Y0;
  }
  a.flow_t[(size_t)b * 2 * HWs + p] = blend(t1, nu[0], nu[1], nu[2], nu[3]);
  a.flow_t[(size_t)b * 2 * HWs + HWs + p] = blend(t1, nv[0], nv[1], nv[2], nv[3]);
}

// ------------------------------------------------------------------ AR loss --
struct LossArgs {
  const float *pred, *target, *noc;
  long long tbs, tcs, trs;  // target batch / channel / row strides (elements)
  long long nbs, nrs;       // noc batch / row strides
  int B, H, W, nchunk;      // nchunk workgroups per sample
  float eps, q;
};

__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int k = 0; k < kNT / 64; ++k) r += red[k];
  __syncthreads();
  return r;
}

// partials[2 (b nchunk + chunk)] = {sum l, sum noc} of the chunk's pixels
template <bool Q1>
__global__ __launch_bounds__(kNT) void ar_loss_fwd_kernel(LossArgs a, float* __restrict__ partials) {
  __shared__ float red[kNT / 64];
  const int b = blockIdx.y, W = a.W, HW = a.H * a.W;
  const size_t HWs = (size_t)HW;
  const float* pr = a.pred + (size_t)b * 2 * HWs;
  const float* tg = a.target + (size_t)b * a.tbs;
  const float* nc = a.noc + (size_t)b * a.nbs;
  float ls = 0.f, ns = 0.f;
#pragma unroll
  for (int k = 0; k < kLossPx; ++k) {
    const int p = (blockIdx.x * kLossPx + k) * kNT + threadIdx.x;
    if (p < HW) {
      const int y = p / W, x = p - y * W;
      const float n = nc[(size_t)y * a.nrs + x];
      const size_t to = (size_t)y * a.trs + x;
      float l0 = fabsf(pr[p] - tg[to]) + a.eps;
      float l1 = fabsf(pr[HWs + p] - tg[to + a.tcs]) + a.eps;
      if constexpr (!Q1) {
        l0 = powf(l0, a.q);
        l1 = powf(l1, a.q);
      }
      ls += l0 * n + l1 * n;
      ns += n;
    }
  }
  const float lsum = block_sum(ls, red), nsum = block_sum(ns, red);
  if (threadIdx.x == 0) {
    float* po = partials + 2 * ((size_t)b * a.nchunk + blockIdx.x);
    po[0] = lsum;
    po[1] = nsum;
  }
}

// out = {loss, c}: loss = (S_l / N) / (D + 1e-7), c = 1 / (N (D + 1e-7)),
// N = 2 B H W, D = S_n / (B H W) or *denom. One workgroup, fixed order, fp64.
__global__ __launch_bounds__(kNT) void ar_loss_final_kernel(const float* __restrict__ partials, int nblk, double npix,
                                                            const float* __restrict__ denom,
                                                            float* __restrict__ out) {
  __shared__ double red[2][kNT / 64];
  const int t = threadIdx.x;
  double s0 = 0, s1 = 0;
  for (int i = t; i < nblk; i += kNT) {
    s0 += partials[2 * i];
    s1 += partials[2 * i + 1];
  }
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) {
    s0 += __shfl_xor(s0, sh);
    s1 += __shfl_xor(s1, sh);
  }
  if ((t & 63) == 0) {
    red[0][t >> 6] = s0;
    red[1][t >> 6] = s1;
  }
  __syncthreads();
  if (t == 0) {
    double l = 0, n = 0;
    for (int k = 0; k < kNT / 64; ++k) {
      l += red[0][k];
      n += red[1][k];
    }
    const double d = (denom ? (double)denom[0] : n / npix) + 1e-7;
    out[0] = (float)(l / (2.0 * npix) / d);
    out[1] = (float)(1.0 / (2.0 * npix * d));
  }
}

// gpred = g c q (|d| + eps)^(q-1) sign(d) noc, d = pred - target
template <bool Q1>
__global__ __launch_bounds__(kNT) void ar_loss_bwd_kernel(LossArgs a, const float* __restrict__ coef,
                                                          const float* __restrict__ gloss,
                                                          float* __restrict__ gpred) {
  const int b = blockIdx.y, W = a.W, HW = a.H * a.W;
  const size_t HWs = (size_t)HW;
  const float* pr = a.pred + (size_t)b * 2 * HWs;
  float* gp = gpred + (size_t)b * 2 * HWs;
  const float* tg = a.target + (size_t)b * a.tbs;
  const float* nc = a.noc + (size_t)b * a.nbs;
  const float k0 = gloss[0] * coef[1] * a.q;
#pragma unroll
  for (int k = 0; k < kLossPx; ++k) {
    const int p = (blockIdx.x * kLossPx + k) * kNT + threadIdx.x;
    if (p < HW) {
      const int y = p / W, x = p - y * W;
      const float kn = k0 * nc[(size_t)y * a.nrs + x];
      const size_t to = (size_t)y * a.trs + x;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float d = pr[c * HWs + p] - tg[to + c * a.tcs];
        float g = d > 0.f ? kn : (d < 0.f ? -kn : 0.f);
        if constexpr (!Q1) {
          if (d != 0.f) g *= powf(fabsf(d) + a.eps, a.q - 1.0f);
        }
        gp[c * HWs + p] = g;
      }
    }
  }
}

int loss_chunks(int H, int W) { return (int)(((long long)H * W + kNT * kLossPx - 1) / (kNT * kLossPx)); }

LossArgs loss_args(const float* pred, const float* target, long long tbs, long long tcs, long long trs,
                   const float* noc, long long nbs, long long nrs, int B, int H, int W, float eps, float q) {
  LossArgs a{};
  a.pred = pred;
  a.target = target;
  a.noc = noc;
  a.tbs = tbs;
  a.tcs = tcs;
  a.trs = trs;
  a.nbs = nbs;
  a.nrs = nrs;
  a.B = B;
  a.H = H;
  a.W = W;
  a.nchunk = loss_chunks(H, W);
  a.eps = eps;
  a.q = q;
  return a;
}

}  // namespace

hipError_t ar_transform_launch(const float* img1, const float* img2, const float* flow, long long fbs,
                               const float* mask, const float* theta, const float* noise1, const float* noise2,
                               float* img1_t, float* img2_t, float* flow_t, float* mask_t, int B, int H, int W,
                               hipStream_t s) {
  TransformArgs a{};
  a.img1 = img1;
  a.img2 = img2;
  a.flow = flow;
  a.mask = mask;
  a.theta = theta;
  a.noise1 = noise1;
  a.noise2 = noise2;
  a.img1_t = img1_t;
  a.img2_t = img2_t;
  a.flow_t = flow_t;
  a.mask_t = mask_t;
  a.fbs = fbs;
  a.B = B;
  a.H = H;
  a.W = W;
  a.sx = (float)(2.0 / (W - 1.0));
  a.sy = (float)(2.0 / (H - 1.0));
  a.hx = (float)(0.5 * (W - 1.0));
  a.hy = (float)(0.5 * (H - 1.0));
  const dim3 grid((unsigned)(((long long)H * W + kNT - 1) / kNT), (unsigned)B);
  hipLaunchKernelGGL(ar_transform_kernel, grid, dim3(kNT), 0, s, a);
  return hipGetLastError();
}

int ar_loss_partials(int B, int H, int W) { return 2 * B * loss_chunks(H, W); }

hipError_t ar_loss_fwd_launch(const float* pred, const float* target, long long tbs, long long tcs, long long trs,
                              const float* noc, long long nbs, long long nrs, const float* denom, float* partials,
                              float* out, int B, int H, int W, float eps, float q, hipStream_t s) {
  const LossArgs a = loss_args(pred, target, tbs, tcs, trs, noc, nbs, nrs, B, H, W, eps, q);
  const dim3 grid((unsigned)a.nchunk, (unsigned)B);
  if (q == 1.0f)
    hipLaunchKernelGGL(ar_loss_fwd_kernel<true>, grid, dim3(kNT), 0, s, a, partials);
  else
    hipLaunchKernelGGL(ar_loss_fwd_kernel<false>, grid, dim3(kNT), 0, s, a, partials);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ar_loss_final_kernel, dim3(1), dim3(kNT), 0, s, partials, B * a.nchunk, (double)B * H * W, denom,
                     out);
  return hipGetLastError();
}

hipError_t ar_loss_bwd_launch(const float* pred, const float* target, long long tbs, long long tcs, long long trs,
                              const float* noc, long long nbs, long long nrs, const float* coef, const float* gloss,
                              float* gpred, int B, int H, int W, float eps, float q, hipStream_t s) {
  const LossArgs a = loss_args(pred, target, tbs, tcs, trs, noc, nbs, nrs, B, H, W, eps, q);
  const dim3 grid((unsigned)a.nchunk, (unsigned)B);
  if (q == 1.0f)
    hipLaunchKernelGGL(ar_loss_bwd_kernel<true>, grid, dim3(kNT), 0, s, a, coef, gloss, gpred);
  else
    hipLaunchKernelGGL(ar_loss_bwd_kernel<false>, grid, dim3(kNT), 0, s, a, coef, gloss, gpred);
  return hipGetLastError();
}

}  // namespace usf
