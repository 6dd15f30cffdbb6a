// The occlusion masks for gfx950 (get_occu_mask_backward / _bidirection).
// Forward bilinear splat of unit mass (warp_utils.py:26-94 get_corresponding_map,
// used by get_occu_mask_backward :120-126): source pixel p of sample b lands at
// (x, y) = (px + u, py + v) (ABS: (u, v) are absolute coordinates already) and
// adds (1-|x-cx|)(1-|y-cy|) to each of its 4 integer neighbours (cx, cy) that
// lies inside the image, with cx in {x0 = floor(x), x0 + 1}, computed in the
// reference's fp32 order (contraction off). Same reduce-by-key scatter as the
// warp's grad_x (scatter_rows.h; lanes = consecutive source pixels): ~2 atomics
// per pixel.
#include "scatter_rows.h"
#include "usf_common.h"
#include "warp_tap.h"

namespace usf {
namespace {

// (The tap arithmetic is splat_tap's, kept in line here: written on splat_tap the
// kernel compiled to different code with one VGPR more, 31 against 30.)
template <bool ABS>
__global__ __launch_bounds__(256) void splat_kernel(const float* __restrict__ flow, long long fbs,
                                                    float* __restrict__ map, int H, int W) {
#pragma clang fp contract(off)
  const int HW = H * W;
  const int t = threadIdx.x;
  const int lane = t & 63;
  int bx, b;
  warp_block(bx, b);
  const int p = bx * 256 + t;
  const bool valid = p < HW;
  float x = 0.f, y = 0.f;
  if (valid) {
    const float* fb = flow + b * fbs;
    const int py = p / W, px = p - py * W;
    x = ABS ? fb[p] : (float)px + fb[p];
    y = ABS ? fb[HW + p] : (float)py + fb[HW + p];
  }
  const float fx = floorf(x), fy = floorf(y);
  const float fx1 = fx + 1.f, fy1 = fy + 1.f;
  const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
  // corner inside the image <=> clamp(c, 0, size-1) == c (the reference's test)
  const bool vx0 = fx >= 0.f && fx <= wm1, vx1 = fx1 >= 0.f && fx1 <= wm1;
  const bool vy0 = valid && fy >= 0.f && fy <= hm1, vy1 = valid && fy1 >= 0.f && fy1 <= hm1;
  const float ax0 = 1.f - fabsf(x - fx), ax1 = 1.f - fabsf(x - fx1);
  const float ay0 = 1.f - fabsf(y - fy), ay1 = 1.f - fabsf(y - fy1);
  // integer corner indices, saturated so far-away targets cannot overflow
  const int xi = fx < -1.f ? -2 : (fx > wm1 ? W : (int)fx);
  const int yi = fy < -1.f ? -2 : (fy > hm1 ? H : (int)fy);
  const bool kx = xi >= -1 && xi < W;  // keys alias nothing only for x0 in [-1, W-1]
  const int kn = (vy0 && kx) ? yi * (W + 1) + xi + 1 : -(lane + 2);
  const int ks = (vy1 && kx) ? (yi + 1) * (W + 1) + xi + 1 : -(lane + 2);
  const bool has_left = lane != 0, has_right = lane != 63;
  const bool m_nw = vx0 && vy0, m_ne = vx1 && vy0, m_sw = vx0 && vy1, m_se = vx1 && vy1;
  const RowRuns rn = row_runs(kn, m_nw, m_ne, has_left, has_right);
  const RowRuns rs = row_runs(ks, m_sw, m_se, has_left, has_right);
  const int o_nw = m_nw || m_ne ? yi * W + xi : 0;
  const int o_sw = m_sw || m_se ? (yi + 1) * W + xi : 0;
  float* mb = map + (size_t)b * HW;
  scatter_row(mb, o_nw, o_nw + 1, m_nw, m_ne, ax0 * ay0, ax1 * ay0, rn);
  scatter_row(mb, o_sw, o_sw + 1, m_sw, m_se, ax0 * ay1, ax1 * ay1, rs);
}

// The splat over vertically adjacent pixel pairs (as warp_bwd_pair_kernel): a
// lane owns rows 2j and 2j + 1 of one column; when both land on the same west
// column and consecutive (unsaturated) corner rows, the shared row's four
// weights are added in the lane and the pair scatters 3 rows instead of 4.
struct SplatTap {
  int xi, yi;  // integer north-west corner, saturated so far-away targets cannot overflow
  bool m_nw, m_ne, m_sw, m_se, kx, ky;  // ky: yi in [-1, H-1] (not saturated)
  float ax0, ax1, ay0, ay1;
};
template <bool ABS>
__device__ __forceinline__ SplatTap splat_tap(const float* __restrict__ fb, int p, int px, int py, bool valid,
                                              int H, int W) {
#pragma clang fp contract(off)
  const int HW = H * W;
  float x = 0.f, y = 0.f;
  if (valid) {
    x = ABS ? fb[p] : (float)px + fb[p];
    y = ABS ? fb[HW + p] : (float)py + fb[HW + p];
  }
  SplatTap s;
  const float fx = floorf(x), fy = floorf(y);
  const float fx1 = fx + 1.f, fy1 = fy + 1.f;
  const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
  const bool vx0 = fx >= 0.f && fx <= wm1, vx1 = fx1 >= 0.f && fx1 <= wm1;
  const bool vy0 = valid && fy >= 0.f && fy <= hm1, vy1 = valid && fy1 >= 0.f && fy1 <= hm1;
  s.ax0 = 1.f - fabsf(x - fx);
  s.ax1 = 1.f - fabsf(x - fx1);
  s.ay0 = 1.f - fabsf(y - fy);
  s.ay1 = 1.f - fabsf(y - fy1);
  s.xi = fx < -1.f ? -2 : (fx > wm1 ? W : (int)fx);
  s.yi = fy < -1.f ? -2 : (fy > hm1 ? H : (int)fy);
  s.kx = s.xi >= -1 && s.xi < W;
  s.ky = valid && s.yi >= -1 && s.yi < H;
  s.m_nw = vx0 && vy0;
  s.m_ne = vx1 && vy0;
  s.m_sw = vx0 && vy1;
  s.m_se = vx1 && vy1;
  return s;
}

template <bool ABS>
__global__ __launch_bounds__(256) void splat_pair_kernel(const float* __restrict__ flow, long long fbs,
                                                         float* __restrict__ map, int H, int W) {
#pragma clang fp contract(off)
  const int HW = H * W, H2 = (H + 1) >> 1;
  const int t = threadIdx.x;
  const int lane = t & 63;
  int bx, b;
  warp_block(bx, b);
  const int pp = bx * 256 + t;
  const bool v0 = pp < W * H2;
  const int px = v0 ? pp % W : 0, py = v0 ? 2 * (pp / W) : 0;
  const bool v1 = v0 && py + 1 < H;
  const float* fb = flow + b * fbs;
  const int p0 = py * W + px;
  const SplatTap s0 = splat_tap<ABS>(fb, p0, px, py, v0, H, W);
  const SplatTap s1 = splat_tap<ABS>(fb, v1 ? p0 + W : p0, px, py + 1, v1, H, W);
  const bool merged = v1 && s0.kx && s0.ky && s1.ky && s0.xi == s1.xi && s0.yi + 1 == s1.yi;
  const bool split = __any(v1 && !merged);
  const bool has_left = lane != 0, has_right = lane != 63;
  auto key = [&](const SplatTap& s, int row, bool rowok) {
    return rowok && s.kx ? row * (W + 1) + s.xi + 1 : -(lane + 2);
  };
  // rows: yi (north, valid iff its corners' row is in the image) and yi + 1
  const RowRuns r0 = row_runs(key(s0, s0.yi, v0 && s0.yi >= 0 && s0.yi < H), s0.m_nw, s0.m_ne, has_left, has_right);
  const RowRuns r1 = row_runs(key(s0, s0.yi + 1, v0 && s0.yi + 1 >= 0 && s0.yi + 1 < H), s0.m_sw, s0.m_se,
                              has_left, has_right);
  const RowRuns r2 = row_runs(key(s1, s1.yi + 1, v1 && s1.yi + 1 >= 0 && s1.yi + 1 < H), s1.m_sw, s1.m_se,
                              has_left, has_right);
  const bool own1 = v1 && !merged;
  RowRuns r3{};
  if (split)
    r3 = row_runs(key(s1, s1.yi, own1 && s1.yi >= 0 && s1.yi < H), s1.m_nw && own1, s1.m_ne && own1,
                  has_left, has_right);
  float* mb = map + (size_t)b * HW;
  const int o0 = s0.yi * W + s0.xi, o1 = s1.yi * W + s1.xi;
  const int on0 = s0.m_nw || s0.m_ne ? o0 : 0, os0 = s0.m_sw || s0.m_se ? o0 + W : 0;
  const int on1 = s1.m_nw || s1.m_ne ? o1 : 0, os1 = s1.m_sw || s1.m_se ? o1 + W : 0;
  scatter_row(mb, on0, on0 + 1, s0.m_nw, s0.m_ne, s0.ax0 * s0.ay0, s0.ax1 * s0.ay0, r0);
  const float vw = merged ? s0.ax0 * s0.ay1 + s1.ax0 * s1.ay0 : s0.ax0 * s0.ay1;
  const float ve = merged ? s0.ax1 * s0.ay1 + s1.ax1 * s1.ay0 : s0.ax1 * s0.ay1;
  scatter_row(mb, os0, os0 + 1, s0.m_sw, s0.m_se, vw, ve, r1);
  scatter_row(mb, os1, os1 + 1, s1.m_sw, s1.m_se, s1.ax0 * s1.ay1, s1.ax1 * s1.ay1, r2);
  if (split) scatter_row(mb, on1, on1 + 1, s1.m_nw && own1, s1.m_ne && own1, s1.ax0 * s1.ay0, s1.ax1 * s1.ay0, r3);
}

// occ = clamp(map, 0, 1) < th ? 1 : 0 (get_occu_mask_backward :124-126); in
// place (occ == map), or (REZERO) from a persistent map that is zeroed as read
template <bool REZERO>
__global__ __launch_bounds__(256) void occ_threshold_kernel(float* m, float* occ, long long n, float th) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = m[i];
  if (REZERO) m[i] = 0.f;
  occ[i] = fminf(fmaxf(v, 0.f), 1.f) < th ? 1.f : 0.f;
}

// Both directions of a with_bk loss at once (usf_occ_vis_pair_persist_f32):
// the splat map is interleaved [B][2][H][W] (half j = 0: the splat of
// flow12 = top[:, :2], j = 1: of flow21 = top[:, 2:]), and the threshold pass
// writes the visibility masks the loss uses, 1 - occ, direction-major:
// vis[0][b] = 1 - occ(flow21) (flow_loss.py:102 vis_mask1), vis[1][b] =
// 1 - occ(flow12) (:103 vis_mask2), each a contiguous [B,1,H,W]; the map is
// re-zeroed as read (its only reader).
__global__ __launch_bounds__(256) void occ_vis_pair_kernel(float* __restrict__ m, float* __restrict__ vis, int HW,
                                                           int B, float th) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n = 2LL * B * HW;
  if (i >= n) return;
  const int b2 = (int)(i / HW), p = (int)(i - (long long)b2 * HW);
  const int b = b2 >> 1, j = b2 & 1;
  const float v = m[i];
  m[i] = 0.f;
  const float occ = fminf(fmaxf(v, 0.f), 1.f) < th ? 1.f : 0.f;
  vis[((long long)(1 - j) * B + b) * HW + p] = 1.f - occ;
}

// Forward-backward consistency occlusion (get_occu_mask_bidirection,
// warp_utils.py:109-117), one thread per pixel:
//   w21  = flow_warp(flow21, flow12, pad="zeros")            (:110)
//   diff = flow12 + w21                                        (:111)
//   mag  = (f12_u^2 + f12_v^2) + (w21_u^2 + w21_v^2)           (:112-114)
//   occ  = (diff_u^2 + diff_v^2) > 0.01 * mag + 0.5 ? 1 : 0    (:115-117)
// Each product and sum is rounded separately, as torch evaluates them (the
// channel sums over 2 elements are a + b), so the mask decision is the
// reference's bit for bit where the warp is.
__global__ __launch_bounds__(256) void occ_bidir_kernel(const float* __restrict__ f12, long long bs12,
                                                        const float* __restrict__ f21, long long bs21,
                                                        float* __restrict__ occ, int H, int W,
                                                        float scale, float bias) {
#pragma clang fp contract(off)
  const int HW = H * W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (p >= HW) return;
  const int y = p / W, x = p - y * W;
  const float* a = f12 + b * bs12;
  const float* c = f21 + b * bs21;
  const float u = a[p], v = a[HW + p];
  const Tap t = make_tap(u, v, x, y, H, W, false);
  const float wnw = t.s * t.e, wne = t.s * t.w, wsw = t.n * t.e, wse = t.n * t.w;
  float w[2];
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    const float* cc = c + ch * HW;
    const float vnw = t.m_nw ? cc[t.o_nw] : 0.f, vne = t.m_ne ? cc[t.o_ne] : 0.f;
    const float vsw = t.m_sw ? cc[t.o_sw] : 0.f, vse = t.m_se ? cc[t.o_se] : 0.f;
    w[ch] = vnw * wnw + vne * wne + vsw * wsw + vse * wse;
  }
  const float du = u + w[0], dv = v + w[1];
  const float mag = (u * u + v * v) + (w[0] * w[0] + w[1] * w[1]);
  const float th = scale * mag + bias;
  occ[(size_t)b * HW + p] = (du * du + dv * dv) > th ? 1.f : 0.f;
}

}  // namespace

hipError_t splat_launch(const float* flow, long long fbs, float* map, int B, int H, int W,
                        bool absolute, hipStream_t s) {
  hipError_t e = zero_fill(map, (size_t)B * H * W * sizeof(float), s);
  if (e != hipSuccess) return e;
  return splat_scatter(flow, fbs, map, B, H, W, absolute, s);
}

// the splat's scatter into a map that is already zero
hipError_t splat_scatter(const float* flow, long long fbs, float* map, int B, int H, int W, bool absolute,
                         hipStream_t s) {
  const long pairs = (long)W * ((H + 1) / 2);
  if (pairs >= 4096 && variant_override(2) != 0) {  // pixel pairs (as the warp backward)
    const dim3 grid((unsigned)((pairs + 255) / 256), (unsigned)B);
    if (absolute)
      hipLaunchKernelGGL((splat_pair_kernel<true>), grid, dim3(256), 0, s, flow, fbs, map, H, W);
    else
      hipLaunchKernelGGL((splat_pair_kernel<false>), grid, dim3(256), 0, s, flow, fbs, map, H, W);
    return hipGetLastError();
  }
  const dim3 grid((unsigned)((H * W + 255) / 256), (unsigned)B);
  if (absolute)
    hipLaunchKernelGGL((splat_kernel<true>), grid, dim3(256), 0, s, flow, fbs, map, H, W);
  else
    hipLaunchKernelGGL((splat_kernel<false>), grid, dim3(256), 0, s, flow, fbs, map, H, W);
  return hipGetLastError();
}

hipError_t occ_backward_persist_launch(const float* flow, long long fbs, float* occ, float* map, int B, int H,
                                       int W, float th, hipStream_t s) {
  // map: the caller's persistent splat buffer, zero on entry; the threshold pass
  // is its only reader and leaves it zero again (no fill launch)
  hipError_t e = splat_scatter(flow, fbs, map, B, H, W, false, s);
  if (e != hipSuccess) return e;
  const long long n = (long long)B * H * W;
  hipLaunchKernelGGL(occ_threshold_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, map, occ, n,
                     th);
  return hipGetLastError();
}

hipError_t occ_vis_pair_persist_launch(const float* flow4, float* vis, float* map, int B, int H, int W, float th,
                                      hipStream_t s) {
  // a dense [B,4,H,W] flow is a [2B,2,H,W] batch of (flow12, flow21) pairs: one
  // splat launch over 2B samples fills the interleaved map
  const long long HW = (long long)H * W;
  hipError_t e = splat_scatter(flow4, 2 * HW, map, 2 * B, H, W, false, s);
  if (e != hipSuccess) return e;
  const long long n = 2LL * B * HW;
  hipLaunchKernelGGL(occ_vis_pair_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, map, vis, (int)HW, B,
                     th);
  return hipGetLastError();
}

hipError_t occ_backward_launch(const float* flow, long long fbs, float* occ, int B, int H, int W,
                               float th, hipStream_t s) {
  hipError_t e = splat_launch(flow, fbs, occ, B, H, W, false, s);
  if (e != hipSuccess) return e;
  const long long n = (long long)B * H * W;
  hipLaunchKernelGGL(occ_threshold_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, occ, occ, n,
                     th);
  return hipGetLastError();
}

hipError_t occ_bidirection_launch(const float* flow12, long long bs12, const float* flow21, long long bs21,
                                  float* occ, int B, int H, int W, float scale, float bias, hipStream_t s) {
  const int HW = H * W;
  hipLaunchKernelGGL(occ_bidir_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)B), dim3(256), 0, s,
                     flow12, bs12, flow21, bs21, occ, H, W, scale, bias);
  return hipGetLastError();
}

}  // namespace usf
