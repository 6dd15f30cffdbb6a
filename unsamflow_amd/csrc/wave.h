// Wave-level (64-lane) helpers: reductions and the "runs of equal keys"
// primitive behind every reduce-by-key. Device-only. Every cross-lane read runs
// in ALL lanes: call these from wave-uniform control flow only (a ds_bpermute
// from an inactive lane returns garbage).
#pragma once
#include <hip/hip_runtime.h>

namespace usf {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
  return v;
}

template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned x) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, false);
}

// maximum over the 64 lanes, in every lane; all lanes must be active
__device__ __forceinline__ unsigned wave_max_u32(unsigned x) {
  x = max(x, dpp_u32<0xB1>(x));   // quad_perm [1,0,3,2]
  x = max(x, dpp_u32<0x4E>(x));   // quad_perm [2,3,0,1]
  x = max(x, dpp_u32<0x141>(x));  // row_half_mirror
  x = max(x, dpp_u32<0x140>(x));  // row_mirror
  x = max(x, (unsigned)__shfl_xor((int)x, 16));
  x = max(x, (unsigned)__shfl_xor((int)x, 32));
  return x;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long x) {
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)x, sh);
    x = o > x ? o : x;
  }
  return x;
}

// Runs of equal keys along the wave: a run reaches from a HEAD lane (the caller's
// test: its key differs from its left neighbour's) to the lane before the next head.
struct WaveRuns {
  int pos;      // lane's distance from its run head
  int maxlen;   // longest run in the wave (wave-uniform)
  bool tail;    // last lane of its run
};
// DPP_MAX: the longest run by wave_max_u32 (as segpool's backward was measured)
// instead of the shuffle butterfly (as the warp scatters were); the same numbers.
template <bool DPP_MAX = false>
__device__ __forceinline__ WaveRuns wave_runs(bool head) {
  const int lane = threadIdx.x & 63;
  const unsigned long long heads = __ballot(head);
  const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);
  WaveRuns r;
  r.pos = lane - (63 - __clzll(heads & upto));
  r.tail = lane == 63 || ((heads >> (lane + 1)) & 1ull) != 0;
  if (DPP_MAX) {
    r.maxlen = (int)wave_max_u32((unsigned)r.pos) + 1;
  } else {
    int m = r.pos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
    r.maxlen = m + 1;
  }
  return r;
}

// segmented inclusive scan: lane l ends with the sum over [its run head, l]
__device__ __forceinline__ float run_sum(float v, const WaveRuns& r) {
  for (int d = 1; d < r.maxlen; d <<= 1) {
    const float u = __shfl_up(v, d);
    if (r.pos >= d) v += u;
  }
  return v;
}

}  // namespace usf
