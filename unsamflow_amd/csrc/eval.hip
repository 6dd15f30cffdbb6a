// Validation on the device for gfx950 (CDNA4): the reference's resize_flow
// (utils/flow_utils.py:62-71) to a size of its own per sample, and
// evaluate_flow (flow_utils.py:117-201) for a whole batch of ragged ground
// truths with the resize fused in.
//
// Layout. The batch tensors are padded to [.., Hmax, Wmax]; sample b owns the
// window [0, H_b) x [0, W_b) of its planes (sizes[2 b], sizes[2 b + 1]; a null
// table: the whole plane). A thread takes V consecutive elements of the padded
// plane (V = 4 with 16-byte loads / stores where Hmax Wmax % 4 == 0, so that
// every plane starts on a 16-byte boundary; else V = 1), kIter such groups, and
// tests each element against its sample's window: nothing outside the window is
// used or written, whatever the padding holds. The prediction [h, w] is small
// and its four taps per pixel come from cache (resize_tap.h).
//
// Evaluation. Per window pixel: gt (u, v), valid, noc (1 with 2-channel gt),
// the optional move mask, the resized prediction, epe = sqrtf(du^2 + dv^2), the
// ten masked sums and the two bad-pixel counts of unsamflow_hip_eval.h, all in
// fp32 with contraction off (the numbers numpy forms). Reduction as the
// key-object push (fakeobj.hip): wave_sum, then LDS, one row of USF_EVAL_NACC
// words per workgroup in caller scratch (the counts as integers); a workgroup
// outside the window, or of a skipped sample, writes zeros, so the scratch needs
// no initialisation. A second launch sums each sample's rows in one fixed order
// in fp64 and forms the ratios there: no float atomics, two runs agree bit for
// bit.
//
// A size outside [2, Hmax] x [2, Wmax] is never used for addressing: the sample
// is skipped and USF_DEVERR_EVAL_BAD_SIZE raised.
#include <cstdint>

#include "resize_tap.h"
#include "usf_common.h"
#include "wave.h"

#include "../../include/unsamflow_hip_eval.h"

namespace usf {
namespace {

constexpr int kNT = 256;   // threads per workgroup
constexpr int kIter = 2;   // element groups per thread (stride kNT groups)
constexpr int kNAcc = USF_EVAL_NACC;
constexpr int kNSum = 10;  // the float sums; the two counts follow

// bad sizes seen by this code object's kernels (usf_device_errors)
__device__ int g_eval_errors = 0;

struct Window {
  int H, W;
  bool ok;
};

__device__ __forceinline__ Window sample_window(const int* __restrict__ sizes, int b, int Hmax, int Wmax) {
  Window s{Hmax, Wmax, true};
  if (sizes) {
    s.H = sizes[2 * b];
    s.W = sizes[2 * b + 1];
    s.ok = s.H >= 2 && s.H <= Hmax && s.W >= 2 && s.W <= Wmax;
    if (!s.ok && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&g_eval_errors, USF_DEVERR_EVAL_BAD_SIZE);
  }
  return s;
}

template <int V>
struct Vec;
template <>
struct Vec<4> {
  using type = float4;
};
template <>
struct Vec<1> {
  using type = float;
};

// V consecutive floats at p (16-byte aligned for V = 4)
template <int V>
__device__ __forceinline__ void load_v(const float* __restrict__ p, float (&r)[V]) {
  using T = typename Vec<V>::type;
  const T t = *reinterpret_cast<const T*>(p);
  __builtin_memcpy(r, &t, sizeof(T));
}

// ------------------------------------------------------------------ resize --
struct ResizeArgs {
  const float* pred;
  const int* sizes;
  float* out;
  long long pbs;  // prediction batch stride (elements)
  int h, w, Hmax, Wmax;
};

template <int V>
__global__ __launch_bounds__(kNT) void flow_resize_kernel(ResizeArgs a) {
  const int b = blockIdx.y, HW = a.Hmax * a.Wmax;
  const Window win = sample_window(a.sizes, b, a.Hmax, a.Wmax);  // uniform over the workgroup
  if (!win.ok) return;
  const ResizeGeom g = resize_geom(a.h, a.w, win.H, win.W);
  const float* pu = a.pred + (size_t)b * a.pbs;
  const float* pv = pu + (size_t)a.h * a.w;
  float* ou = a.out + (size_t)b * 2 * HW;
  float* ov = ou + HW;
#pragma unroll
  for (int it = 0; it < kIter; ++it) {
    const int p0 = ((blockIdx.x * kIter + it) * kNT + threadIdx.x) * V;
    if (p0 >= HW) break;  // HW % V == 0: a group is whole
    int Y = p0 / a.Wmax, X = p0 - Y * a.Wmax;
    if (Y >= win.H) break;  // every later element lies below the window too
    float u[V], v[V];
    bool in[V], all = true;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      in[k] = Y < win.H && X < win.W;
      if (in[k])
        resize_sample(pu, pv, a.w, resize_tap(Y, g.sy, a.h), resize_tap(X, g.sx, a.w), g, u[k], v[k]);
      else
        all = false;
      if (++X == a.Wmax) {
        X = 0;
        ++Y;
      }
    }
    if (V == 4 && all) {
      *reinterpret_cast<float4*>(ou + p0) = make_float4(u[0], u[1], u[2], u[3]);
      *reinterpret_cast<float4*>(ov + p0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (in[k]) {
          ou[p0 + k] = u[k];
          ov[p0 + k] = v[k];
        }
    }
  }
}

// -------------------------------------------------------------------- eval --
struct EvalArgs {
  const float *pred, *gt, *move;
  const int* sizes;
  long long pbs;
  int Cg, h, w, Hmax, Wmax;
};

// partials[kNAcc (b gridDim.x + blockIdx.x)] = this workgroup's sums (fp32) and counts (int32)
template <int V>
__global__ __launch_bounds__(kNT) void flow_eval_kernel(EvalArgs a, float* __restrict__ partials) {
  __shared__ float red[kNAcc][kNT / 64];
  const int b = blockIdx.y, HW = a.Hmax * a.Wmax;
  const Window win = sample_window(a.sizes, b, a.Hmax, a.Wmax);  // uniform over the workgroup
  float acc[kNAcc];
#pragma unroll
  for (int c = 0; c < kNAcc; ++c) acc[c] = 0.f;

  if (win.ok) {
    const ResizeGeom g = resize_geom(a.h, a.w, win.H, win.W);
    const float* pu = a.pred + (size_t)b * a.pbs;
    const float* pv = pu + (size_t)a.h * a.w;
    const float* gp = a.gt + (size_t)b * a.Cg * HW;
    const float* mp = a.move ? a.move + (size_t)b * HW : nullptr;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
#pragma clang fp contract(off)
      const int p0 = ((blockIdx.x * kIter + it) * kNT + threadIdx.x) * V;
      if (p0 >= HW) break;  // HW % V == 0: a group is whole
      int Y = p0 / a.Wmax, X = p0 - Y * a.Wmax;
      if (Y >= win.H) break;  // every later element lies below the window too
      bool in[V], any = false;
      int ys[V], xs[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        ys[k] = Y;
        xs[k] = X;
        in[k] = Y < win.H && X < win.W;
        any = any || in[k];
        if (++X == a.Wmax) {
          X = 0;
          ++Y;
        }
      }
      if (!any) continue;
      float gu[V], gv[V], va[V], no[V], mv[V];
      load_v<V>(gp + p0, gu);
      load_v<V>(gp + HW + p0, gv);
      if (a.Cg == 4) {
        load_v<V>(gp + 2 * (size_t)HW + p0, va);
        load_v<V>(gp + 3 * (size_t)HW + p0, no);
      }
      if (mp) load_v<V>(mp + p0, mv);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if (!in[k]) continue;  // the padding is never used, whatever it holds
        const float valid = a.Cg == 4 ? va[k] : 1.f, noc = a.Cg == 4 ? no[k] : 1.f;
        float u, v;
        resize_sample(pu, pv, a.w, resize_tap(ys[k], g.sy, a.h), resize_tap(xs[k], g.sx, a.w), g, u, v);
        const float du = u - gu[k], dv = v - gv[k];
        const float epe = sqrtf(du * du + dv * dv);
        const float thr = 0.05f * sqrtf(gu[k] * gu[k] + gv[k] * gv[k]);
        const float ev = epe * valid, en = epe * noc, occ = valid - noc;
        acc[0] += ev;
        acc[1] += valid;
        acc[2] += en;
        acc[3] += noc;
        acc[4] += epe * occ;
        acc[5] += occ;
        if (mp) {
          const float st = 1.0f - mv[k];
          acc[6] += ev * mv[k];
          acc[7] += valid * mv[k];
          acc[8] += ev * st;
          acc[9] += valid * st;
        }
        // at most kIter V per thread and kNT kIter V per workgroup: exact in fp32
        acc[10] += (ev > 3.f && ev > thr) ? 1.f : 0.f;
        acc[11] += (en > 3.f && en > thr) ? 1.f : 0.f;
      }
    }
  }

#pragma unroll
  for (int c = 0; c < kNAcc; ++c) {
    const float s = wave_sum(acc[c]);
    if ((threadIdx.x & 63) == 0) red[c][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < kNAcc / 4) {
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 4 * threadIdx.x + j;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < kNT / 64; ++k) s += red[c][k];
      r[j] = c < kNSum ? s : __int_as_float((int)s);
    }
    float* row = partials + kNAcc * ((size_t)b * gridDim.x + blockIdx.x);
    reinterpret_cast<float4*>(row)[threadIdx.x] = make_float4(r[0], r[1], r[2], r[3]);
  }
}

// sums[b] and metrics[b] from the sample's nchunk rows. One workgroup per
// sample, fixed order, fp64.
__global__ __launch_bounds__(kNT) void flow_eval_final_kernel(const float* __restrict__ partials,
                                                              const int* __restrict__ sizes, int nchunk, int Hmax,
                                                              int Wmax, int has_move, float* __restrict__ sums,
                                                              float* __restrict__ metrics) {
  __shared__ double red[kNAcc][kNT / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* pp = partials + kNAcc * (size_t)b * nchunk;
  double s[kNAcc];
#pragma unroll
  for (int c = 0; c < kNAcc; ++c) s[c] = 0.0;
  for (int i = t; i < nchunk; i += kNT) {
    float r[kNAcc];
#pragma unroll
    for (int q = 0; q < kNAcc / 4; ++q) {
      const float4 v = reinterpret_cast<const float4*>(pp + kNAcc * (size_t)i)[q];
      r[4 * q] = v.x;
      r[4 * q + 1] = v.y;
      r[4 * q + 2] = v.z;
      r[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int c = 0; c < kNAcc; ++c) s[c] += c < kNSum ? (double)r[c] : (double)__float_as_int(r[c]);
  }
#pragma unroll
  for (int c = 0; c < kNAcc; ++c) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) s[c] += __shfl_xor(s[c], sh);
    if ((t & 63) == 0) red[c][t >> 6] = s[c];
  }
  __syncthreads();
  if (t != 0) return;
  double r[kNAcc];
#pragma unroll
  for (int c = 0; c < kNAcc; ++c) {
    r[c] = 0.0;
    for (int k = 0; k < kNT / 64; ++k) r[c] += red[c][k];
    sums[kNAcc * (size_t)b + c] = (float)r[c];
  }
  bool ok = true;
  if (sizes) {
    const int H = sizes[2 * b], W = sizes[2 * b + 1];
    ok = H >= 2 && H <= Hmax && W >= 2 && W <= Wmax;
  }
  const float nan = __int_as_float(0x7FC00000);
  float* m = metrics + USF_EVAL_NMETRIC * (size_t)b;
  // the reference's ratios: an empty mask is 0/0 = NaN; EPE_occ alone is guarded
  m[0] = ok ? (float)(r[0] / r[1]) : nan;
  m[1] = ok ? (float)(r[2] / r[3]) : nan;
  m[2] = ok ? (float)(r[4] / fmax(r[5], 1.0)) : nan;
  m[3] = ok ? (float)(r[10] / r[1] * 100.0) : nan;
  m[4] = ok ? (float)(r[11] / r[3] * 100.0) : nan;
  m[5] = ok && has_move ? (float)(r[6] / r[7]) : nan;
  m[6] = ok && has_move ? (float)(r[8] / r[9]) : nan;
}

int group_width(int Hmax, int Wmax) { return ((long long)Hmax * Wmax) % 4 == 0 ? 4 : 1; }

int eval_chunks(int Hmax, int Wmax) {
  const long long per_wg = (long long)kNT * kIter * group_width(Hmax, Wmax);
  return (int)(((long long)Hmax * Wmax + per_wg - 1) / per_wg);
}

}  // namespace

int eval_device_errors(bool clear) { return read_clear_flags(HIP_SYMBOL(g_eval_errors), clear); }

hipError_t flow_resize_launch(const float* pred, long long pbs, const int* sizes, float* out, int B, int h, int w,
                              int Hmax, int Wmax, hipStream_t s) {
  const ResizeArgs a{pred, sizes, out, pbs, h, w, Hmax, Wmax};
  const dim3 grid((unsigned)eval_chunks(Hmax, Wmax), (unsigned)B);
  if (group_width(Hmax, Wmax) == 4)
    hipLaunchKernelGGL(flow_resize_kernel<4>, grid, dim3(kNT), 0, s, a);
  else
    hipLaunchKernelGGL(flow_resize_kernel<1>, grid, dim3(kNT), 0, s, a);
  return hipGetLastError();
}

int flow_eval_partials(int B, int Hmax, int Wmax) { return kNAcc * B * eval_chunks(Hmax, Wmax); }

hipError_t flow_eval_launch(const float* pred, long long pbs, const float* gt, int Cg, const float* move,
                            const int* sizes, float* partials, float* sums, float* metrics, int B, int h, int w,
                            int Hmax, int Wmax, hipStream_t s) {
  const EvalArgs a{pred, gt, move, sizes, pbs, Cg, h, w, Hmax, Wmax};
  const int nchunk = eval_chunks(Hmax, Wmax);
  const dim3 grid((unsigned)nchunk, (unsigned)B);
  if (group_width(Hmax, Wmax) == 4)
    hipLaunchKernelGGL(flow_eval_kernel<4>, grid, dim3(kNT), 0, s, a, partials);
  else
    hipLaunchKernelGGL(flow_eval_kernel<1>, grid, dim3(kNT), 0, s, a, partials);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(flow_eval_final_kernel, dim3((unsigned)B), dim3(kNT), 0, s, partials, sizes, nchunk, Hmax, Wmax,
                     move ? 1 : 0, sums, metrics);
  return hipGetLastError();
}

}  // namespace usf
