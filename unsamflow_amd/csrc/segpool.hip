// The mask-feature branch's per-segment max pool and spread
// (include/unsamflow_hip_segpool.h; models/pwclite.py:317-357 of the reference):
//
//   pooled[b,c,k] = amax over the sample of onehot(seg)[.,k] * proj[b,c,.]
//   spread[b,c,p] = pooled[b,c,seg[b,p]]
//
// without the [B,C,h,w,K] products the torch composition builds. The only
// K-sized buffers are the per-(sample, channel, segment) tables of `state`:
//
//   state[0 .. B*C*K)        the segment maxima, as order-preserving uint keys
//   state[B*C*K .. +B*K)     n_in, the pixel count of every segment
//
// Forward: (0) a fill kernel zeroes the tables. (1) workgroups over (sample, channel group, 1024-pixel chunk) keep a
// [channels][K] key table in LDS. Segment maps are piecewise constant, so a
// wave step of 64 pixels mostly holds one to three ids: up to four ids are
// peeled off, each reduced across the wave (DPP) and merged with ONE LDS atomic
// max per channel; lanes of further ids (noise maps) issue their own. The
// tables merge into `state` with global atomic max / integer add -- both
// order-independent, so the result is deterministic. (2) a dense pass applies
// the one-hot product's zero (the n_out rule) and writes `spread`.
//
// Backward: one workgroup per (sample, channel) walks the plane in row order.
// Every 64-pixel step reduces grad_spread by key with the segmented shuffle
// scan of wave.h (wave_runs / run_sum) and adds the runs to the wave's own LDS
// bins one after another in lane order; the waves' bins are combined in wave
// order. The float sum G therefore has one fixed summation order and no float
// atomics. The tie count t is an integer LDS atomic. The same workgroup then
// re-walks the plane (L2-resident: 112 KB at Sintel L4) and writes grad_proj.
#include <algorithm>

#include "seg_key.h"
#include "usf_common.h"
#include "wave.h"

#include "../../include/unsamflow_hip_segpool.h"

namespace usf {
namespace {

constexpr int kFwdNT = 256;       // forward threads per workgroup
constexpr int kFwdSteps = 4;      // 64-pixel steps per wave: 1024 pixels per workgroup
constexpr int kFwdLdsKeys = 8192; // LDS key table budget (words): channels per group = 8192 / K, at most 32
constexpr int kSpreadCh = 8;      // channels per workgroup of the dense pass
constexpr int kBwdNT = 512;       // backward threads per workgroup: 8 waves, 8 bin sets
constexpr int kPeel = 4;          // ids reduced across the wave per step

// bad segment ids seen by this code object's kernels (usf_device_errors)
__device__ int g_seg_errors = 0;

// order-preserving float -> uint key, 0 = "no value yet" (below every float)
__device__ __forceinline__ unsigned enc_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec_key(unsigned e) {
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

// the pooled value of a segment with n_in pixels of HW: the maximum itself when
// the segment covers the sample, else the maximum with the one-hot product's
// zeros outside; 0 for an absent segment
__device__ __forceinline__ float pooled_value(unsigned e, int n_in, int HW) {
  if (n_in <= 0 || e == 0u) return 0.f;
  const float m = dec_key(e);
  if (n_in == HW) return m;
  return m > 0.f ? m : 0.f;
}

// ---------------------------------------------------------------- forward --
// the tables' zero fill as a kernel: a hipMemsetAsync node raced the kernel after
// it on graph replay (zero_fill_kernel in warp.hip has the history)
__global__ __launch_bounds__(256) void seg_clear_kernel(unsigned* __restrict__ state, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) state[i] = 0u;
}

// grid (pixel chunks, channel groups, B); LDS: CG * K keys, then K counts
__global__ __launch_bounds__(kFwdNT) void seg_max_kernel(const float* __restrict__ proj,
                                                         const float* __restrict__ seg,
                                                         unsigned* __restrict__ state, int B, int C, int HW, int K,
                                                         int CG) {
  extern __shared__ unsigned lds[];
  const int b = blockIdx.z, c0 = blockIdx.y * CG, nc = min(CG, C - c0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool count = blockIdx.y == 0;
  unsigned* tab = lds;
  int* cnt = reinterpret_cast<int*>(lds + CG * K);
  for (int i = threadIdx.x; i < CG * K + K; i += kFwdNT) lds[i] = 0u;
  __syncthreads();

  const float* sg = seg + (long long)b * HW;
  const float* pj = proj + ((long long)b * C + c0) * HW;
  const int chunk0 = blockIdx.x * (kFwdNT * kFwdSteps);
  bool bad = false;
  for (int st = 0; st < kFwdSteps; ++st) {
    const int p0 = chunk0 + (st * (kFwdNT / 64) + wave) * 64;
    if (p0 >= HW) break;  // wave-uniform
    const int p = p0 + lane;
    const bool valid = p < HW;
    const int key = valid ? seg_key(sg[p], K) : -1;
    bad |= valid && key < 0;
    // peel up to kPeel ids off the wave: (id, lanes) in scalar registers
    unsigned long long rem = __ballot(key >= 0);
    int pk[kPeel];
    unsigned long long pm[kPeel];
#pragma unroll
    for (int j = 0; j < kPeel; ++j) {
      pk[j] = 0;
      pm[j] = 0ull;
      if (rem) {
        const int l = __ffsll((long long)rem) - 1;
        pk[j] = __shfl(key, l);
        pm[j] = __ballot(key == pk[j] && key >= 0);
        rem &= ~pm[j];
      }
    }
    const bool mine = (rem >> lane) & 1ull;  // my id was not peeled
    if (count) {
#pragma unroll
      for (int j = 0; j < kPeel; ++j)
        if (pm[j] && lane == 0) atomicAdd(&cnt[pk[j]], __popcll(pm[j]));
      if (mine) atomicAdd(&cnt[key], 1);
    }
    for (int cb = 0; cb < nc; cb += 4) {
      unsigned e[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        e[i] = (key >= 0 && cb + i < nc) ? enc_key(pj[(long long)(cb + i) * HW + p]) : 0u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (cb + i >= nc) break;  // uniform
        unsigned* row = tab + (cb + i) * K;
#pragma unroll
        for (int j = 0; j < kPeel; ++j) {
          if (pm[j]) {  // uniform: every lane takes part in the reduction
            const unsigned r = wave_max_u32(((pm[j] >> lane) & 1ull) ? e[i] : 0u);
            if (lane == 0) atomicMax(&row[pk[j]], r);
          }
        }
        if (mine) atomicMax(&row[key], e[i]);
      }
    }
  }
  if (__any(bad) && lane == 0) atomicOr(&g_seg_errors, USF_DEVERR_SEGPOOL_BAD_ID);
  __syncthreads();

  unsigned* gtab = state + ((long long)b * C + c0) * K;
  for (int i = threadIdx.x; i < nc * K; i += kFwdNT) {
    const unsigned e = tab[i];
    if (e) atomicMax(&gtab[i], e);
  }
  if (count) {
    int* gcnt = reinterpret_cast<int*>(state + (long long)B * C * K) + (long long)b * K;
    for (int k = threadIdx.x; k < K; k += kFwdNT) {
      const int n = cnt[k];
      if (n) atomicAdd(&gcnt[k], n);
    }
  }
}

// grid (pixel chunks of 256 * V, channel groups of kSpreadCh, B); V = 4 needs HW % 4 == 0
template <int V>
__global__ __launch_bounds__(256) void seg_spread_kernel(const float* __restrict__ seg,
                                                         const unsigned* __restrict__ state,
                                                         float* __restrict__ out, int B, int C, int HW, int K) {
  const int b = blockIdx.z, c0 = blockIdx.y * kSpreadCh, nc = min(kSpreadCh, C - c0);
  const int p = (blockIdx.x * 256 + threadIdx.x) * V;
  if (p >= HW) return;
  const int* gcnt = reinterpret_cast<const int*>(state + (long long)B * C * K) + (long long)b * K;
  int key[V], n_in[V];
  if (V == 4) {
    const float4 s = *reinterpret_cast<const float4*>(seg + (long long)b * HW + p);
    key[0] = seg_key(s.x, K);
    key[1 % V] = seg_key(s.y, K);
    key[2 % V] = seg_key(s.z, K);
    key[3 % V] = seg_key(s.w, K);
  } else {
    key[0] = seg_key(seg[(long long)b * HW + p], K);
  }
#pragma unroll
  for (int j = 0; j < V; ++j) n_in[j] = key[j] >= 0 ? gcnt[key[j]] : 0;
  const unsigned* tab = state + ((long long)b * C + c0) * K;
  float* o = out + ((long long)b * C + c0) * HW + p;
#pragma unroll 4
  for (int c = 0; c < nc; ++c) {
    float v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = key[j] >= 0 ? pooled_value(tab[c * K + key[j]], n_in[j], HW) : 0.f;
    if (V == 4)
      *reinterpret_cast<float4*>(o + (long long)c * HW) = make_float4(v[0], v[1 % V], v[2 % V], v[3 % V]);
    else
      o[(long long)c * HW] = v[0];
  }
}

// --------------------------------------------------------------- backward --
// grid (C, B); LDS: NW * K float bins, K tie counts, K pooled values
__global__ __launch_bounds__(kBwdNT) void seg_bwd_kernel(const float* __restrict__ proj,
                                                         const float* __restrict__ seg,
                                                         const unsigned* __restrict__ state,
                                                         const float* __restrict__ gs, float* __restrict__ gp,
                                                         int B, int C, int HW, int K) {
  constexpr int NW = kBwdNT / 64;
  extern __shared__ unsigned lds[];
  float* bins = reinterpret_cast<float*>(lds);          // [NW][K]; bins[0] becomes G / (t + z)
  int* tcnt = reinterpret_cast<int*>(lds + NW * K);     // [K]
  float* pv = reinterpret_cast<float*>(lds + (NW + 1) * K);  // [K]
  const int c = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned* tab = state + ((long long)b * C + c) * K;
  const int* gcnt = reinterpret_cast<const int*>(state + (long long)B * C * K) + (long long)b * K;
  for (int i = threadIdx.x; i < (NW + 1) * K; i += kBwdNT) lds[i] = 0u;
  for (int k = threadIdx.x; k < K; k += kBwdNT) pv[k] = pooled_value(tab[k], gcnt[k], HW);
  __syncthreads();

  const float* sg = seg + (long long)b * HW;
  const long long plane = ((long long)b * C + c) * HW;
  const float* x = proj + plane;
  const float* g = gs + plane;
  float* mybin = bins + wave * K;
  for (int p0 = wave * 64; p0 < HW; p0 += kBwdNT) {
    const int p = p0 + lane;
    const bool valid = p < HW;
    const int key = valid ? seg_key(sg[p], K) : -1;
    float v = key >= 0 ? g[p] : 0.f;
    if (key >= 0 && x[p] == pv[key]) atomicAdd(&tcnt[key], 1);
    // runs of equal ids in lane order (every shuffle runs in all lanes)
    const int kl = __shfl_up(key, 1);
    const WaveRuns r = wave_runs<true>(lane == 0 || kl != key);
    v = run_sum(v, r);
    // one run after another: two runs of a step may carry the same id
    unsigned long long tails = __ballot(r.tail && key >= 0);
    while (tails) {
      const int l = __ffsll((long long)tails) - 1;
      if (lane == l) mybin[key] += v;
      tails &= tails - 1;
    }
  }
  __syncthreads();

  for (int k = threadIdx.x; k < K; k += kBwdNT) {
    float G = bins[k];
#pragma unroll
    for (int w = 1; w < NW; ++w) G += bins[w * K + k];
    const int n_in = gcnt[k];
    const int den = tcnt[k] + (pv[k] == 0.f ? HW - n_in : 0);
    bins[k] = (n_in > 0 && den > 0) ? G / (float)den : 0.f;
  }
  __syncthreads();

  float* o = gp + plane;
  for (int p = threadIdx.x; p < HW; p += kBwdNT) {
    const int key = seg_key(sg[p], K);
    o[p] = (key >= 0 && x[p] == pv[key]) ? bins[key] : 0.f;
  }
}

int fwd_channels_per_group(int C, int K) { return std::max(1, std::min(std::min(C, 32), kFwdLdsKeys / K)); }

}  // namespace

int segpool_device_errors(bool clear) {
  return read_clear_flags(HIP_SYMBOL(g_seg_errors), clear);
}

long long segpool_state_words(int B, int C, int K) { return (long long)B * C * K + (long long)B * K; }

hipError_t segpool_fwd_launch(const float* proj, const float* seg, float* spread, unsigned* state, int B, int C,
                              int H, int W, int K, hipStream_t s) {
  const int HW = H * W;
  const long long words = segpool_state_words(B, C, K);
  hipLaunchKernelGGL(seg_clear_kernel, dim3((unsigned)std::min<long long>((words + 255) / 256, 2048)), dim3(256), 0, s,
                     state, words);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int CG = fwd_channels_per_group(C, K);
  const dim3 g1((HW + kFwdNT * kFwdSteps - 1) / (kFwdNT * kFwdSteps), (C + CG - 1) / CG, B);
  hipLaunchKernelGGL(seg_max_kernel, g1, dim3(kFwdNT), (size_t)(CG * K + K) * 4, s, proj, seg, state, B, C, HW, K,
                     CG);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int ngrp = (C + kSpreadCh - 1) / kSpreadCh;
  const bool vec = HW % 4 == 0 && ((reinterpret_cast<uintptr_t>(seg) | reinterpret_cast<uintptr_t>(spread)) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(seg_spread_kernel<4>, dim3((HW / 4 + 255) / 256, ngrp, B), dim3(256), 0, s, seg, state, spread,
                       B, C, HW, K);
  else
    hipLaunchKernelGGL(seg_spread_kernel<1>, dim3((HW + 255) / 256, ngrp, B), dim3(256), 0, s, seg, state, spread, B,
                       C, HW, K);
  return hipGetLastError();
}

hipError_t segpool_bwd_launch(const float* proj, const float* seg, const unsigned* state, const float* gs, float* gp,
                              int B, int C, int H, int W, int K, hipStream_t s) {
  constexpr int NW = kBwdNT / 64;
  hipLaunchKernelGGL(seg_bwd_kernel, dim3(C, B), dim3(kBwdNT), (size_t)(NW + 2) * K * 4, s, proj, seg, state, gs, gp,
                     B, C, H * W, K);
  return hipGetLastError();
}

}  // namespace usf
