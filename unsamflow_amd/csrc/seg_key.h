// The segment id of a pixel, as segpool.hip and hg.hip both read a segment map.
#pragma once
#include <hip/hip_runtime.h>

namespace usf {

// id of a pixel, -1 for anything that is not an integer in [0, K)
__device__ __forceinline__ int seg_key(float s, int K) {
  if (!(s >= 0.f && s < (float)K)) return -1;
  const int k = (int)s;
  return (float)k == s ? k : -1;
}

}  // namespace usf
