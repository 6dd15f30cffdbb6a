// The wave-level reduce-by-key scatter of one corner row, shared by the warp
// backward's grad_x scatters (warp.hip) and the occlusion splats (occ.hip),
// with the workgroup numbering both use.
#pragma once
#include "usf_common.h"
#include "wave.h"

namespace usf {

// Work split: a 256-thread workgroup covers PXB = 256/CS consecutive pixels x
// CS channel slices (thread t: pixel t % PXB, channels t/PXB, t/PXB + CS, ...),
// so consecutive lanes stay on consecutive pixels (coalesced flow/out/gout and
// near-contiguous corner gathers / atomics) while small, channel-heavy pyramid
// levels still spread over many workgroups instead of looping C channels per
// lane.
// (pixel block, sample) of this workgroup; with USF_WARP_CHUNK > 0 runs of
// neighbouring pixel blocks (shared source rows / scatter targets) go to one XCD.
// 16 blocks per chunk: warp forward L4 14.3 -> 12.6 us, L2 8.7 -> 7.9 us; the
// backward and the splat are unchanged (profiles/ab_r01/warp_chunk_*.json)
#ifndef USF_WARP_CHUNK
#define USF_WARP_CHUNK 16
#endif
__device__ __forceinline__ void warp_block(int& bx, int& b) {
  if (USF_WARP_CHUNK > 0) {
    const int w = xcd_chunk(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y, USF_WARP_CHUNK);
    bx = w % gridDim.x;
    b = w / gridDim.x;
  } else {
    bx = blockIdx.x;
    b = blockIdx.y;
  }
}

// grad_x scatter of one corner row (north: nw/ne, or south: sw/se) as a
// wave-level reduce-by-key. Consecutive lanes are consecutive pixels, so along
// a wave the target cells of a row are (nearly) monotone: lanes whose west
// corner hits the same cell (the flow compresses, or floor() of a coordinate
// that round-trips a hair below an integer) form a RUN, and a run's east cell
// is usually the next run's west cell. Each run is summed onto its last lane
// (log-step segmented scan over shuffles; the bound is the longest run in the
// wave, channel-invariant, so the common no-collision case costs 2 shuffles),
// the next run's head adds the previous run's east total into its west value,
// and only run tails issue atomics: ~1 global atomic per cell and channel, and
// no two lanes of one atomic instruction on the same address (those serialise).
struct RowRuns : WaveRuns {  // tail: issues the run's atomics
  bool take;    // run head that adds the previous run's east total (cells chain)
  bool give;    // run tail whose east total the next run's head takes
};

// key: row * (W + 1) + west column + 1, or a lane-unique negative value when the
// row is outside the image (no atomics); has_left/has_right: the neighbour lane
// exists and belongs to the same channel slice.
__device__ __forceinline__ RowRuns row_runs(int key, bool m_w, bool m_e, bool has_left,
                                            bool has_right) {
  const int kl = __shfl_up(key, 1);
  const int me = m_e ? 1 : 0;
  const bool head = !(has_left && kl == key);
  RowRuns r{wave_runs(head)};
  // every cross-lane read executes in all lanes (never behind a short-circuit:
  // a ds_bpermute from an inactive lane returns garbage)
  const bool left_me = __shfl_up(me, 1) != 0;
  r.take = head && has_left && m_w && left_me && kl + 1 == key;
  const bool right_takes = __shfl_down(r.take ? 1 : 0, 1) != 0;
  r.give = r.tail && has_right && right_takes;
  return r;
}

__device__ __forceinline__ void scatter_row(float* gc, int o_w, int o_e, bool m_w, bool m_e,
                                            float vw, float ve, const RowRuns& r) {
  const float se = run_sum(ve, r);
  const float lt = __shfl_up(se, 1);
  const float sw = run_sum(vw + (r.take ? lt : 0.f), r);
  if (r.tail) {
    if (m_w) atomicAdd(gc + o_w, sw);
    if (m_e && !r.give) atomicAdd(gc + o_e, se);
  }
}

// a corner row's key: keys alias nothing only for west columns in [-1, W-1];
// elsewhere both cells are off-image
__device__ __forceinline__ int row_key(bool ok, int row, int xw, int H, int W, int lane) {
  return ok && xw >= -1 && xw < W && (unsigned)row < (unsigned)H ? row * (W + 1) + xw + 1 : -(lane + 2);
}

}  // namespace usf
