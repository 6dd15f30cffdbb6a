// The column-strip stream shared by the photometric forward kernels (photo.hip,
// census.hip): a strip is 64 staged columns (one per lane; the 60 middle ones
// are its own pixels) streamed down the image one staged row per step, and one
// launch covers 1..4 scales, each owning a contiguous range of workgroups.
// What the two files do per row, and how tall they cut their strips (measured
// cost models that differ), stays with them.
#pragma once
#include <hip/hip_runtime.h>

namespace usf {

constexpr int kSL = 64;        // lanes of a strip = staged columns
constexpr int kSO = kSL - 4;   // own columns per strip (lanes 2 .. 61)
constexpr int kRsrcWord3 = 0x00020000;
constexpr int kMaxScales = 4;     // scales of one launch
constexpr int kSimds = 1024;      // 256 CUs x 4 SIMDs
constexpr int kMinStripRows = 4;  // the partials buffer holds ceil(H / 4) strips per column

// lane l reads lane l+1 / l-1 of the wave (DPP wave_shl:1 / wave_shr:1;
// the missing neighbour of lane 63 / 0 reads 0). Every lane must be active.
// mov_dpp with bound_ctrl (no "old" operand to materialise), so the compiler
// folds it into the add that consumes it (v_add_f32_dpp).
__device__ __forceinline__ float from_next(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x130, 0xf, 0xf, true));
}
__device__ __forceinline__ float from_prev(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x138, 0xf, 0xf, true));
}

// Scale s owns workgroups [start[s], start[s + 1]) -- the largest scale first,
// so the small scales' few strips fill the chip's tail instead of each paying a
// launch and a drain of their own. The scale of workgroup blk:
__device__ __forceinline__ int strip_scale(const int (&start)[kMaxScales + 1], int blk) {
  return (blk >= start[1]) + (blk >= start[2]) + (blk >= start[3]);
}

// Host: close the workgroup ranges of a launch of nscale scales and total
// workgroups (Pyr = {sc[kMaxScales], ..., start[kMaxScales + 1]}): the unused
// scales start at total, so strip_scale never selects them.
template <class Pyr>
void strip_pad_scales(Pyr& m, int nscale, unsigned total) {
  for (int k = nscale; k <= kMaxScales; ++k) m.start[k] = (int)total;
  for (int k = nscale; k < kMaxScales; ++k) m.sc[k] = m.sc[0];
}

}  // namespace usf
