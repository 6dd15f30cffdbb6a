// Fused occlusion-aware ternary (soft census) photometric loss of unFlowLoss
// for gfx950 (CDNA4): the w_ternary term of loss_photomatric
// (losses/flow_loss.py:33-50) with TernaryLoss (losses/loss_blocks.py:12-50,
// max_distance = 1), for one flow direction, for both directions of a with_bk
// scale, or for up to 4 scales, in one launch:
//
//   rec  = flow_warp(src, flow, pad)                      (warp_utils.py:97-106)
//   x    = rec * m,  y = tgt * m
//   gray(z) = 255 (0.2989 z0 + 0.5870 z1 + 0.1140 z2)
//   for every interior pixel q and each of its 8 neighbours k (offset dk):
//     tx = gray_x(q + dk) - gray_x(q),  nx = tx / sqrt(0.81 + tx^2)   (ty, ny from y)
//     d  = (nx - ny)^2,  e = d / (0.1 + d)
//   T    = sum_q sum_k e / 9            (the patch's centre channel contributes 0)
//   L    = w_ternary * T / (B H W) / (mean_{b,p} m + 1e-6)
//
// Border pixels are masked out of T (_valid_mask) but still feed their interior
// neighbours' patches, so conv2d's zero padding never reaches the result.
//
// As in photo.hip the mask and tgt carry no gradient and L is linear in T, so
// the forward pass writes a per-pixel basis and the backward is a dense pass:
//   a(q,k) = (1/9) 0.1 / (0.1 + d)^2 * 2 (nx - ny) * 0.81 / (0.81 + tx^2)^1.5   (= d(e/9)/d tx)
//   G(p)   = sum_k [p - dk interior] a(p - dk, k)  -  [p interior] sum_k a(p, k)  (= dT/d gray_x(p))
//   basis_p = G(p) * m_p * 255 * sum_c coef_c * dI_pc/dflow      (2 floats, 8 B/pixel)
//   dL/dflow_p = c_t * basis_p,   c_t = w_ternary / (B H W (mean m + 1e-6))
// dI/dflow is the bilinear tap's coordinate derivative incl. norm_grid and the
// border clip (warp_tap.h), the warp's own sample point.
//
// The forward streams photo.hip's column strips (strip.h): 64 lanes = 64 staged columns
// (the 60 middle ones are the strip's own pixels), one staged row per step.
// Here one wave runs a whole strip: the previous gray row, the pending G row
// and the rows' flow derivatives live in registers, horizontal neighbours come
// through DPP, and there is no LDS and no barrier. Each staged pixel is warped
// once. The patches are evaluated per edge (census_body), which halves the
// divisions and square roots and needs a halo of one row and one column only.
// Deterministic: fixed-order sums, no atomics. Division and sqrt are the
// correctly rounded ones.
#include <algorithm>
#include <cstdint>

#include "strip.h"
#include "usf_common.h"
#include "warp_tap.h"
#include "wave.h"

namespace usf {
namespace {

constexpr float kGrayR = 0.2989f, kGrayG = 0.5870f, kGrayB = 0.1140f;

// one flow direction: rec = warp(src, flow), compared with tgt under mask
struct CensusDir {
  const float* src;
  const float* tgt;
  const float* mask;
  const float* flow;  // [2,H,W] block per sample at flow + b * fbs
  float* basis;       // 2 planes per sample at basis + b * bbs, or null (forward only)
};
struct CensusArgs {
  CensusDir dir[2];
  long long fbs, bbs;  // flow / basis batch strides (elements)
  int B, H, W, nsx, nsy, ndir;
};
// scale s owns workgroups [start[s], start[s + 1]); unused scales: start = total
struct CensusPyr {
  CensusArgs sc[kMaxScales];
  float* part[kMaxScales];
  int start[kMaxScales + 1];
};

__device__ __forceinline__ float ld(__amdgpu_buffer_rsrc_t r, int off, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, soff, 0));
}
__device__ __forceinline__ float gray3(float r, float g, float b) {
  return (r * kGrayR + g * kGrayG + b * kGrayB) * 255.f;
}

// e = d / (0.1 + d) of one (pixel, neighbour) and with GRAD a = d(e / 9)/d tx
template <bool GRAD>
__device__ __forceinline__ float census_term(float tx, float ty, float& a) {
  const float rx = 1.0f / sqrtf(fmaf(tx, tx, 0.81f));
  const float ry = 1.0f / sqrtf(fmaf(ty, ty, 0.81f));
  const float df = tx * rx - ty * ry;
  const float d = df * df;
  const float inv = 1.0f / (0.1f + d);
  if constexpr (GRAD) a = (0.1f * 2.f * 0.81f / 9.f) * (inv * inv) * df * (rx * rx * rx);
  return d * inv;
}

// the loads of one staged row (issued one step before they are used)
struct RowLoads {
  float gv[3][4], tt[3], m;
  float n, w, mx, my;
};

// The strip stream of one scale's workgroup blk of nblk.
template <bool BORDER, bool GRAD>
__device__ __forceinline__ void census_body(const CensusArgs& a, float* __restrict__ partials, int blk, int nblk) {
  const int lane = threadIdx.x;
  // workgroup -> (sample, strip row, strip column, direction)
  const int npx = a.ndir * a.nsx;
  const int g = xcd_remap(blk, nblk);
  const int gx = g % npx, rest = g / npx;
  const int sy = rest % a.nsy, b = rest / a.nsy;
  const int dirn = gx % a.ndir, sx = gx / a.ndir;
  const int H = a.H, W = a.W, HW = H * W;
  const size_t HWs = (size_t)HW;
  const int y0 = (int)((long long)sy * H / a.nsy);
  const int rown = (int)((long long)(sy + 1) * H / a.nsy) - y0;
  const int nsteps = rown + 2;  // rows y0 - 1 .. y0 + rown
  const CensusDir dr = a.dir[dirn];
  const int col = sx * kSO - 2 + lane;
  const int cc = min(max(col, 0), W - 1);
  const bool col_in = col >= 0 && col < W;
  const bool lane_own = lane >= 2 && lane < 2 + kSO && col < W;
  const bool col_int = col >= 1 && col <= W - 2;  // interior column

  const float* srcb = dr.src + (size_t)b * 3 * HWs;
  __amdgpu_buffer_rsrc_t rs[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    rs[c] = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(srcb + c * HWs), 0, 4 * HW, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t rtgt =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dr.tgt + (size_t)b * 3 * HWs), 0, 12 * HW, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t rmask =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dr.mask + (size_t)b * HWs), 0, 4 * HW, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t rflow =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dr.flow + b * a.fbs), 0, 8 * HW, kRsrcWord3);
  __amdgpu_buffer_rsrc_t rbas = rmask;
  if constexpr (GRAD) rbas = __builtin_amdgcn_make_buffer_rsrc(dr.basis + b * a.bbs, 0, 8 * HW, kRsrcWord3);
  const float fxs = 2.0f / (float)(W - 1), fys = 2.0f / (float)(H - 1);

  // rows outside the image (and rows past the strip's last step) read 0
  auto row_off = [&](int r, bool ok) { return ok && r >= 0 && r < H ? 4 * (r * W + cc) : kOffNone; };
  auto load_flow = [&](int r, bool ok, float& u, float& v) {
    const int o = row_off(r, ok);
    u = ld(rflow, o, 0);
    v = ld(rflow, o, 4 * HW);
  };
  auto issue = [&](int r, bool ok, float u, float v, RowLoads& L) {
    const TapB tp = make_tap_b<BORDER>(u, v, cc, r, H, W);
    const int o = row_off(r, ok);
    const bool in = o != kOffNone;
    const int onw = in ? tp.onw : kOffNone, one = in ? tp.one : kOffNone;
    const int osw = in ? tp.osw : kOffNone, ose = in ? tp.ose : kOffNone;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      L.gv[c][0] = ld(rs[c], onw, 0);
      L.gv[c][1] = ld(rs[c], one, 0);
      L.gv[c][2] = ld(rs[c], osw, 0);
      L.gv[c][3] = ld(rs[c], ose, 0);
      L.tt[c] = ld(rtgt, o, 4 * c * HW);
    }
    L.m = ld(rmask, o, 0);
    L.n = tp.n;
    L.w = tp.w;
    L.mx = tp.mx;
    L.my = tp.my;
  };

  // Edge form. Neighbouring pixels u, v (8-connected) see each other with
  // opposite differences, t(v, u) = -t(u, v), so e is the same from both ends
  // and a flips its sign: one evaluation per EDGE, counted once per interior
  // end (cnt = 0, 1 or 2), gives  T += cnt e / 9,  G(v) += cnt a,  G(u) -= cnt a
  // with t = gray(v) - gray(u). Each step takes row r's four edge kinds per lane
  // (u at this lane): H (r,x)-(r,x+1), V (r-1,x)-(r,x), D1 (r-1,x)-(r,x+1),
  // D2 (r-1,x)-(r,x-1). An edge needs only its two ends, so lanes 1 .. 62 and one
  // row above and below the strip suffice (lanes 0 and 63 are spare).
  const bool own_next = lane + 1 >= 2 && lane + 1 < 2 + kSO && col + 1 < W;
  const bool own_prev = lane - 1 >= 2 && lane - 1 < 2 + kSO && col - 1 < W;
  // interior column: this lane, the next, the previous; o*: ... and an own column
  const float ci = col_int ? 1.f : 0.f;
  const float cin = col + 1 >= 1 && col + 1 <= W - 2 ? 1.f : 0.f;
  const float cip = col - 1 >= 1 && col - 1 <= W - 2 ? 1.f : 0.f;
  const float oi = lane_own ? ci : 0.f, oin = own_next ? cin : 0.f, oip = own_prev ? cip : 0.f;
  float g1x = 0.f, g1y = 0.f;  // gray of row r-1
  float D1x = 0.f, D1y = 0.f;  // m 255 sum_c coef_c dI_c/dflow of row r-1
  float G1 = 0.f;              // dT/d gray_x of row r-1 as far as summed
  float tsum = 0.f, msum = 0.f;

  RowLoads cur, nxt;
  float fu1, fv1, fu2, fv2;
  load_flow(y0 - 1, true, fu1, fv1);
  issue(y0 - 1, true, fu1, fv1, cur);
  load_flow(y0, true, fu1, fv1);
  for (int i = 0; i < nsteps; ++i) {
    const int r = y0 - 1 + i;  // the row staged in this step
    load_flow(r + 2, i + 2 < nsteps, fu2, fv2);
    issue(r + 1, i + 1 < nsteps, fu1, fv1, nxt);
    // ---- stage row r: x = rec m, y = tgt m -> gray_x, gray_y, the flow derivative
    float gx_, gy_, D0x = 0.f, D0y = 0.f;
    {
      const float n = cur.n, w = cur.w, m = cur.m;
      const float me = col_in ? m : 0.f;
      float s, e, rec[3];
      {
#pragma clang fp contract(off)
        s = 1.0f - n;
        e = 1.0f - w;
        const float wnw = s * e, wne = s * w, wsw = n * e, wse = n * w;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          rec[c] = cur.gv[c][0] * wnw + cur.gv[c][1] * wne + cur.gv[c][2] * wsw + cur.gv[c][3] * wse;
      }
      gx_ = gray3(rec[0] * me, rec[1] * me, rec[2] * me);
      gy_ = gray3(cur.tt[0] * me, cur.tt[1] * me, cur.tt[2] * me);
      const bool own_row = i >= 1 && i <= rown;
      msum += own_row && lane_own ? m : 0.f;
      if constexpr (GRAD) {
        float dix = 0.f, diy = 0.f;
        const float cf[3] = {kGrayR, kGrayG, kGrayB};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float(&v)[4] = cur.gv[c];
          dix = fmaf(cf[c], (v[1] - v[0]) * s + (v[3] - v[2]) * n, dix);
          diy = fmaf(cf[c], (v[2] - v[0]) * e + (v[3] - v[1]) * w, diy);
        }
        const float k255 = 255.f * me;
        D0x = dix * (k255 * cur.mx * fxs);
        D0y = diy * (k255 * cur.my * fys);
      }
    }
    if (i >= 1) {  // wave-uniform; row r-1 is staged
      const float gxn = from_next(gx_), gxp = from_prev(gx_), gyn = from_next(gy_), gyp = from_prev(gy_);
      // interior / own rows r and r-1 (wave-uniform)
      const float ri = r >= 1 && r <= H - 2 ? 1.f : 0.f, r1i = r - 1 >= 1 && r - 1 <= H - 2 ? 1.f : 0.f;
      const float ro = i <= rown ? ri : 0.f, r1o = i >= 2 ? r1i : 0.f;
      float aH = 0.f, aV = 0.f, aD1 = 0.f, aD2 = 0.f;
      const float eH = census_term<GRAD>(gxn - gx_, gyn - gy_, aH);
      const float eV = census_term<GRAD>(gx_ - g1x, gy_ - g1y, aV);
      const float eD1 = census_term<GRAD>(gxn - g1x, gyn - g1y, aD1);
      const float eD2 = census_term<GRAD>(gxp - g1x, gyp - g1y, aD2);
      // own interior ends per edge: T (each strip sums its own pixels' terms)
      const float u1 = r1o * oi;
      tsum += (eH * (ro * oi + ro * oin) + eV * (u1 + ro * oi) + eD1 * (u1 + ro * oin) + eD2 * (u1 + ro * oip)) *
              (1.0f / 9.0f);
      if constexpr (GRAD) {
        const float c1 = r1i * ci;
        const float wH = aH * (ri * ci + ri * cin), wV = aV * (c1 + ri * ci);
        const float wD1 = aD1 * (c1 + ri * cin), wD2 = aD2 * (c1 + ri * cip);
        const float g0 = from_prev(wH) - wH + wV + from_prev(wD1) + from_next(wD2);  // row r so far
        G1 -= wV + wD1 + wD2;                                                        // row r-1: complete
        const int p = r - 1;
        const bool pown = i >= 2;  // p = y0 .. y0 + rown - 1
        const int o = pown && lane_own ? 4 * (p * W + col) : kOffNone;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, G1 * D1x), rbas, o, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, G1 * D1y), rbas, o, 4 * HW, 0);
        G1 = g0;
      }
    }
    g1x = gx_;
    g1y = gy_;
    D1x = D0x;
    D1y = D0y;
    cur = nxt;
    fu1 = fu2;
    fv1 = fv2;
  }
  const float ts = wave_sum(tsum), ms = wave_sum(msum);
  if (lane == 0) {
    float* po = partials + 2 * (((size_t)dirn * a.B + b) * a.nsy * a.nsx + (size_t)sy * a.nsx + sx);
    po[0] = ts;
    po[1] = ms;
  }
}

// One launch for 1..4 scales (a single scale for the one-direction and pair
// entries): the largest scale first, so the small scales' few strips fill the
// chip's tail. Every scale runs the same code on the same strips whichever
// entry launched it, so the pyramid's numbers are the per-scale calls' bit for bit.
template <bool BORDER, bool GRAD>
__global__ __launch_bounds__(kSL) void census_fwd_kernel(CensusPyr m) {
  const int blk = blockIdx.x;
  const int s = strip_scale(m.start, blk);
  census_body<BORDER, GRAD>(m.sc[s], m.part[s], blk - m.start[s], m.start[s + 1] - m.start[s]);
}

// One block per (direction, scale): fixed-order fp64 sum of its partials ->
// out[2 (ndir s + dir) ..] = {loss, c_t}, c_t = w / (N (mean(m) + 1e-6)).
constexpr int kFinNT = 256;
struct CensusFin {
  const float* part[kMaxScales];
  int nblk[kMaxScales];
  double n[kMaxScales];
};
__global__ __launch_bounds__(kFinNT) void census_final_kernel(CensusFin f, float* __restrict__ out, float w) {
  __shared__ double red[2][kFinNT / 64];
  const int t = threadIdx.x, dirn = blockIdx.x, s = blockIdx.y, nblk = f.nblk[s];
  const float* p = f.part[s] + (size_t)2 * nblk * dirn;
  double a = 0, b = 0;
  for (int i = t; i < nblk; i += kFinNT) {
    a += p[2 * i];
    b += p[2 * i + 1];
  }
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) {
    a += __shfl_xor(a, sh);
    b += __shfl_xor(b, sh);
  }
  if ((t & 63) == 0) {
    red[0][t >> 6] = a;
    red[1][t >> 6] = b;
  }
  __syncthreads();
  if (t == 0) {
    double s0 = 0, s1 = 0;
    for (int k = 0; k < kFinNT / 64; ++k) {
      s0 += red[0][k];
      s1 += red[1][k];
    }
    const double n = f.n[s];
    const double den = s1 / n + 1e-6;
    float* o = out + 2 * ((size_t)gridDim.x * s + dirn);
    o[0] = (float)(w * (s0 / n) / den);
    o[1] = (float)(w / (n * den));
  }
}

// gflow[b, 2 dir + j, p] = c_t[dir] g[dir] basis[b, 2 dir + j, p]: the basis and
// the gradient share one layout, so each (sample, direction) is a dense 2 HW run.
// blockIdx.z = ndir s + dir.
struct CensusBwd {
  const float* basis[kMaxScales];
  float* gflow[kMaxScales];
  int HW[kMaxScales];
};
__global__ __launch_bounds__(256) void census_bwd_kernel(CensusBwd m, const float* __restrict__ coef,
                                                         const float* __restrict__ gloss, int ndir) {
  const int s = blockIdx.z / ndir, dirn = blockIdx.z % ndir, b = blockIdx.y;
  const int n2 = 2 * m.HW[s];
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n2) return;
  const float k = coef[2 * blockIdx.z + 1] * gloss[blockIdx.z];
  const size_t base = ((size_t)b * ndir + dirn) * n2;
  const float* a = m.basis[s] + base;
  float* o = m.gflow[s] + base;
  if ((n2 & 3) == 0) {
    const float4 u = *reinterpret_cast<const float4*>(a + i);
    *reinterpret_cast<float4*>(o + i) = make_float4(k * u.x, k * u.y, k * u.z, k * u.w);
  } else {
    for (int e = i; e < i + 4 && e < n2; ++e) o[e] = k * a[e];
  }
}

// Strip heights, as photo.hip's strip_plan: every wave streams R + 2 rows, so a
// launch takes about (R + 2) steps times the rounds of strips the chip holds
// (kWaves per SIMD, 1024 SIMDs). The strips of a column are balanced; the
// cheapest count wins, ties to fewer strips. The plan never depends on the
// number of directions in the launch (it is made for two), so a pair and its
// two single-direction calls sum the same partials.
constexpr int kWaves = 4;  // resident strips per SIMD the plan assumes

int strip_count(int B, int H, int W) {
  const long long cols = 2LL * B * ((W + kSO - 1) / kSO);
  const long long slots = (long long)kWaves * kSimds;
  int best = 1;
  double best_cost = -1.0;
  for (int nsy = 1; nsy <= (H + kMinStripRows - 1) / kMinStripRows; ++nsy) {
    const int R = (H + nsy - 1) / nsy;
    if ((H + R - 1) / R != nsy) continue;  // the same R as a smaller count
    const long long waves = cols * nsy;
    const long long rounds = (waves + slots - 1) / slots;
    const double cost = (double)rounds * (R + 2);
    if (best_cost < 0 || cost < best_cost) {
      best_cost = cost;
      best = nsy;
    }
  }
  return best;
}

struct Scale {
  CensusDir dir[2];
  long long fbs, bbs;
  int H, W;
};

hipError_t census_launch(int nscale, const Scale* sc, int ndir, int B, int pad_mode, float* partials, float* out,
                         float w, hipStream_t s) {
  CensusPyr m{};
  CensusFin f{};
  bool grad = false;
  unsigned total = 0;
  long long poff = 0;
  for (int k = 0; k < nscale; ++k) {
    CensusArgs& a = m.sc[k];
    a.dir[0] = sc[k].dir[0];
    a.dir[1] = sc[k].dir[ndir - 1];
    a.fbs = sc[k].fbs;
    a.bbs = sc[k].bbs;
    a.B = B;
    a.H = sc[k].H;
    a.W = sc[k].W;
    a.nsx = (a.W + kSO - 1) / kSO;
    a.nsy = strip_count(B, a.H, a.W);
    a.ndir = ndir;
    grad = grad || a.dir[0].basis != nullptr;
    m.part[k] = partials + poff;
    m.start[k] = (int)total;
    total += (unsigned)(B * a.nsy * a.nsx * ndir);
    f.part[k] = partials + poff;
    f.nblk[k] = B * a.nsx * a.nsy;
    f.n[k] = (double)B * a.H * a.W;
    poff += (long long)ndir * census_partials(B, a.H, a.W);
  }
  strip_pad_scales(m, nscale, total);
  const dim3 grid(total), block(kSL);
  if (pad_mode == 1) {
    if (grad)
      hipLaunchKernelGGL((census_fwd_kernel<true, true>), grid, block, 0, s, m);
    else
      hipLaunchKernelGGL((census_fwd_kernel<true, false>), grid, block, 0, s, m);
  } else {
    if (grad)
      hipLaunchKernelGGL((census_fwd_kernel<false, true>), grid, block, 0, s, m);
    else
      hipLaunchKernelGGL((census_fwd_kernel<false, false>), grid, block, 0, s, m);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(census_final_kernel, dim3((unsigned)ndir, (unsigned)nscale), dim3(kFinNT), 0, s, f, out, w);
  return hipGetLastError();
}

}  // namespace

int census_partials(int B, int H, int W) {
  // any strip height (the smallest R has the most strips), per direction
  return 2 * B * ((H + kMinStripRows - 1) / kMinStripRows) * ((W + kSO - 1) / kSO);
}

hipError_t census_fwd_launch(const float* src, const float* tgt, const float* mask, const float* flow, long long fbs,
                             float* partials, float* out, float* basis, int B, int H, int W, int pad_mode, float w,
                             hipStream_t s) {
  Scale sc{};
  sc.dir[0] = CensusDir{src, tgt, mask, flow, basis};
  sc.fbs = fbs;
  sc.bbs = 2LL * H * W;
  sc.H = H;
  sc.W = W;
  return census_launch(1, &sc, 1, B, pad_mode, partials, out, w, s);
}

namespace {
// both directions of a with_bk scale: dir 0 warps im2 by flow[:, 0:2] onto im1
// (mask1), dir 1 warps im1 by flow[:, 2:4] onto im2 (mask2) (flow_loss.py:130-131).
// basis: [B, 2, 2, H, W] (= [B,4,H,W]) or null.
Scale pair_scale(const float* im1, const float* im2, const float* mask1, const float* mask2, const float* flow,
                 long long fbs, float* basis, int H, int W) {
  Scale sc{};
  const size_t HW = (size_t)H * W;
  sc.dir[0] = CensusDir{im2, im1, mask1, flow, basis};
  sc.dir[1] = CensusDir{im1, im2, mask2, flow + 2 * HW, basis ? basis + 2 * HW : nullptr};
  sc.fbs = fbs;
  sc.bbs = 4LL * H * W;
  sc.H = H;
  sc.W = W;
  return sc;
}
}  // namespace

hipError_t census_pair_fwd_launch(const float* im1, const float* im2, const float* mask1, const float* mask2,
                                  const float* flow, long long fbs, float* partials, float* out, float* basis, int B,
                                  int H, int W, int pad_mode, float w, hipStream_t s) {
  const Scale sc = pair_scale(im1, im2, mask1, mask2, flow, fbs, basis, H, W);
  return census_launch(1, &sc, 2, B, pad_mode, partials, out, w, s);
}

hipError_t census_pyr_fwd_launch(int nscale, const float* const* im1, const float* const* im2,
                                 const float* const* mask1, const float* const* mask2, const float* const* flow,
                                 const long long* fbs, const int* H, const int* W, float* partials, float* out,
                                 float* const* basis, int B, int pad_mode, float w, hipStream_t s) {
  if (nscale < 1 || nscale > kMaxScales) return hipErrorInvalidValue;
  Scale sc[kMaxScales];
  for (int k = 0; k < nscale; ++k)
    sc[k] = pair_scale(im1[k], im2[k], mask1[k], mask2[k], flow[k], fbs[k], basis ? basis[k] : nullptr, H[k], W[k]);
  return census_launch(nscale, sc, 2, B, pad_mode, partials, out, w, s);
}

hipError_t census_pyr_bwd_launch(int nscale, const float* const* basis, const float* coef, const float* gloss,
                                 float* const* gflow, const int* H, const int* W, int B, int ndir, hipStream_t s) {
  if (nscale < 1 || nscale > kMaxScales) return hipErrorInvalidValue;
  CensusBwd m{};
  int hwmax = 0;
  for (int k = 0; k < nscale; ++k) {
    m.basis[k] = basis[k];
    m.gflow[k] = gflow[k];
    m.HW[k] = H[k] * W[k];
    hwmax = std::max(hwmax, m.HW[k]);
  }
  const dim3 grid((unsigned)((2 * hwmax + 1023) / 1024), (unsigned)B, (unsigned)(ndir * nscale));
  hipLaunchKernelGGL(census_bwd_kernel, grid, dim3(256), 0, s, m, coef, gloss, ndir);
  return hipGetLastError();
}

}  // namespace usf
