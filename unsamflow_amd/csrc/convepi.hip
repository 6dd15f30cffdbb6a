// The convolution epilogues of PWCLite's conv_block as streaming kernels
// (include/unsamflow_hip_convepi.h): bias add + LeakyReLU in place after the
// conv, and their backward with the bias gradient summed on the way, instead of
// four torch passes per convolution. fp32 NCHW, dense planes.
//
// Both kernels walk 16-byte SLOTS: four floats at a 16-byte aligned address of
// the dense tensor. A slot inside one plane is one dwordx4 access; a slot that
// straddles a plane's edge (H*W % 4 != 0: plane starts are then not 16-byte
// aligned) is done float by float. A workgroup takes TILE_SLOTS consecutive
// slots as four coalesced rounds of 256 lanes, all four loads issued before the
// first use (the scheme of stream.hip).
//
// The bias gradient is deterministic: no atomics, an order fixed by the shape.
// A channel's slots (sample-major, USF_CONVEPI_TILE_SLOTS per tile) are cut into
// `parts` runs of at most USF_CONVEPI_CHAIN tiles. A lane keeps 16 accumulators
// (round x float4 component), each fed one term per tile -- a sequential chain
// of at most USF_CONVEPI_CHAIN terms -- then adds them as a tree, the wave as a
// shuffle tree (wave.h), the four waves through LDS. parts == 1 writes gbias
// itself; otherwise the partials go to the caller's workspace [C][parts] and a
// second launch adds them, 64 lanes strided over the parts and a shuffle tree.
#include "usf_common.h"
#include "wave.h"

#include "unsamflow_hip_convepi.h"

namespace usf {
namespace {

using f4 = float __attribute__((ext_vector_type(4)));
// a gradient slice's planes start wherever the concat put them: 4-byte aligned
typedef f4 f4u __attribute__((aligned(4)));

constexpr int THREADS = 256;
constexpr int ROUNDS = 4;
constexpr int TILE_SLOTS = USF_CONVEPI_TILE_SLOTS;
static_assert(TILE_SLOTS == THREADS * ROUNDS, "a tile is four rounds of the workgroup");
// One tile per workgroup until the grid passes this many workgroups (64 per CU),
// only then several tiles in sequence: as stream.hip found for the plain copy,
// many short workgroups stream faster than a resident grid that loops (the
// 16x128x64x208 backward measured 72 us with 4 tiles per workgroup).
constexpr long long TARGET_WGS = USF_CONVEPI_TARGET_WGS;

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : v * slope; }

// y = act(raw + bias[c]) in place over the dense [P = B*C][HW] array of n floats
// (16-byte aligned): slot i holds floats 4i .. 4i+3.
__global__ __launch_bounds__(THREADS) void convepi_fwd_kernel(float* __restrict__ y, const float* __restrict__ bias,
                                                             long long n, int C, int HW, float slope) {
  // the tile's first float -> (plane, offset, channel), once per workgroup
  const long long tile0 = (long long)blockIdx.x * (TILE_SLOTS * 4);
  const long long p0 = tile0 / HW;
  const int r0 = (int)(tile0 - p0 * HW);
  const int c0 = (int)(p0 % C);
  f4 v[ROUNDS];
  int rr[ROUNDS], cc[ROUNDS];
#pragma unroll
  for (int k = 0; k < ROUNDS; ++k) {
    const int off = 4 * (k * THREADS + (int)threadIdx.x);  // float offset in the tile, < 4096
    const long long i = tile0 + off;
    int r = r0 + off, c = c0;
    if (HW >= TILE_SLOTS * 4) {  // at most one plane edge inside a tile
      if (r >= HW) {
        r -= HW;
        c = c + 1 == C ? 0 : c + 1;
      }
    } else {
      const int dp = r / HW;
      r -= dp * HW;
      c = (c + dp) % C;
    }
    rr[k] = r;
    cc[k] = c;
    if (i + 4 <= n) v[k] = *reinterpret_cast<const f4*>(y + i);
  }
#pragma unroll
  for (int k = 0; k < ROUNDS; ++k) {
    const long long i = tile0 + 4 * (k * THREADS + (int)threadIdx.x);
    int r = rr[k], c = cc[k];
    if (i + 4 <= n && r + 4 <= HW) {  // the whole slot in one plane
      const float b = bias[c];
      f4 o;
      o.x = leaky(v[k].x + b, slope);
      o.y = leaky(v[k].y + b, slope);
      o.z = leaky(v[k].z + b, slope);
      o.w = leaky(v[k].w + b, slope);
      *reinterpret_cast<f4*>(y + i) = o;
    } else {  // a plane edge inside the slot, or the array's last floats
      for (int e = 0; e < 4; ++e) {
        if (i + e < n) y[i + e] = leaky(y[i + e] + bias[c], slope);
        if (++r == HW) {
          r = 0;
          c = c + 1 == C ? 0 : c + 1;
        }
      }
    }
  }
}

// One (channel, part) per workgroup. ACT: gin = gout * (y > 0 ? 1 : slope),
// written dense; otherwise gout is only summed. RED: the channel sum of what
// was written (ACT) or read. The channel's slot space is [B][nsm] with nsm =
// ceil((HW + 3) / 4): slot j of sample b covers plane floats 4j - shift ..
// 4j - shift + 3, shift = the plane start's offset from 16-byte alignment in
// the dense tensors (y, gin); slots past the plane's end are empty.
template <bool ACT, bool RED>
__global__ __launch_bounds__(THREADS) void convepi_bwd_kernel(const float* __restrict__ gout, long long gbs,
                                                             const float* __restrict__ y, float* __restrict__ gin,
                                                             float* __restrict__ sums, int B, int C, int HW, int nsm,
                                                             int tiles, int tpp, int parts, float slope) {
  const int c = blockIdx.x / parts, part = blockIdx.x - c * parts;
  const int t_end = min(tiles, (part + 1) * tpp);
  // this lane's slot (sample b, slot j), stepped by THREADS from round to round
  const unsigned L0 = (unsigned)part * tpp * TILE_SLOTS + threadIdx.x;  // < 2^31 (bwd_split)
  int b = (int)(L0 / (unsigned)nsm);
  int j = (int)(L0 - (unsigned)b * nsm);
  f4 acc[ROUNDS];
#pragma unroll
  for (int k = 0; k < ROUNDS; ++k) acc[k] = f4{0.f, 0.f, 0.f, 0.f};
  for (int t = part * tpp; t < t_end; ++t) {
    f4 g[ROUNDS], a[ROUNDS];
    long long dense[ROUNDS], go[ROUNDS];
    int e0s[ROUNDS];
    bool full[ROUNDS], live[ROUNDS];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
      const long long start = ((long long)b * C + c) * HW;  // plane start in y / gin
      const int e0 = 4 * j - (int)(start & 3);
      live[k] = b < B && e0 < HW;
      full[k] = live[k] && e0 >= 0 && e0 + 4 <= HW;
      e0s[k] = e0;
      dense[k] = start + e0;
      go[k] = (long long)b * gbs + (long long)c * HW + e0;
      j += THREADS;
      if (nsm >= THREADS) {
        if (j >= nsm) {
          j -= nsm;
          ++b;
        }
      } else {
        const int db = j / nsm;
        j -= db * nsm;
        b += db;
      }
      if (full[k]) {
        g[k] = *reinterpret_cast<const f4u*>(gout + go[k]);
        if (ACT) a[k] = *reinterpret_cast<const f4*>(y + dense[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
      if (full[k]) {
        f4 o = g[k];
        if (ACT) {
          o.x = a[k].x > 0.f ? o.x : o.x * slope;
          o.y = a[k].y > 0.f ? o.y : o.y * slope;
          o.z = a[k].z > 0.f ? o.z : o.z * slope;
          o.w = a[k].w > 0.f ? o.w : o.w * slope;
          *reinterpret_cast<f4*>(gin + dense[k]) = o;
        }
        if (RED) acc[k] += o;
      } else if (live[k]) {  // the plane's head or tail: the floats inside it
        float edge = 0.f;
        for (int e = 0; e < 4; ++e) {
          const int pe = e0s[k] + e;
          if (pe < 0 || pe >= HW) continue;
          float v = gout[go[k] + e];
          if (ACT) {
            v = y[dense[k] + e] > 0.f ? v : v * slope;
            gin[dense[k] + e] = v;
          }
          edge += v;
        }
        if (RED) acc[k].x += edge;  // one term of the chain, like a whole slot
      }
    }
  }
  if (!RED) return;
  // 16 accumulators -> lane -> wave -> workgroup, each a fixed tree
  const f4 s4 = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  const float lane_sum = wave_sum((s4.x + s4.y) + (s4.z + s4.w));
  __shared__ float wsum[THREADS / 64];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = lane_sum;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// gbias[c] = the channel's partials in part order: lane l adds parts l, l + 64,
// ... (at most USF_CONVEPI_CHAIN of them), then the shuffle tree. One wave per channel.
__global__ __launch_bounds__(64) void convepi_finish_kernel(const float* __restrict__ partials,
                                                           float* __restrict__ gbias, int parts) {
  const float* p = partials + (long long)blockIdx.x * parts;
  float s = 0.f;
  for (int i = threadIdx.x; i < parts; i += 64) s += p[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) gbias[blockIdx.x] = s;
}

struct Split {
  int nsm, tiles, tpp, parts;
};

// the backward's decomposition for a shape (tiles > CHAIN * 64 * CHAIN: no split fits)
bool bwd_split(int B, int C, int H, int W, Split* sp) {
  const long long HW = (long long)H * W;
  const long long nsm = (HW + 3 + 3) / 4;
  if ((long long)B * nsm > 0x7FF00000LL) return false;  // slot indices are 32-bit in the kernel
  const long long tiles = ((long long)B * nsm + TILE_SLOTS - 1) / TILE_SLOTS;
  long long tpp = (tiles * C + TARGET_WGS - 1) / TARGET_WGS;
  if (tpp > USF_CONVEPI_CHAIN) tpp = USF_CONVEPI_CHAIN;
  if (tpp < 1) tpp = 1;
  const long long parts = (tiles + tpp - 1) / tpp;
  if (parts > 64 * USF_CONVEPI_CHAIN || parts * C > 0x7FFFFFFFLL) return false;
  *sp = Split{(int)nsm, (int)tiles, (int)tpp, (int)parts};
  return true;
}

}  // namespace

long long convepi_bwd_workspace(int B, int C, int H, int W) {
  Split sp;
  if (!bwd_split(B, C, H, W, &sp)) return -1;
  return sp.parts > 1 ? (long long)C * sp.parts : 0;
}

hipError_t convepi_fwd_launch(float* y, const float* bias, int B, int C, int H, int W, float slope, hipStream_t s) {
  const long long n = (long long)B * C * H * W;
  const long long tiles = (n + TILE_SLOTS * 4 - 1) / (TILE_SLOTS * 4);
  hipLaunchKernelGGL(convepi_fwd_kernel, dim3((unsigned)tiles), dim3(THREADS), 0, s, y, bias, n, C, H * W, slope);
  return hipGetLastError();
}

hipError_t convepi_bwd_launch(const float* gout, long long gbs, const float* y, float* gin, float* gbias,
                              float* workspace, int B, int C, int H, int W, float slope, hipStream_t s) {
  Split sp;
  if (!bwd_split(B, C, H, W, &sp)) return hipErrorInvalidValue;
  const bool act = slope != 1.f, red = gbias != nullptr;
  float* sums = sp.parts > 1 ? workspace : gbias;
  const dim3 grid((unsigned)(C * sp.parts)), block(THREADS);
#define USF_CONVEPI_BWD(ACT, RED)                                                                                  \
  hipLaunchKernelGGL((convepi_bwd_kernel<ACT, RED>), grid, block, 0, s, gout, gbs, y, gin, sums, B, C, H * W, sp.nsm, \
                     sp.tiles, sp.tpp, sp.parts, slope)
  if (act && red) USF_CONVEPI_BWD(true, true);
  else if (act) USF_CONVEPI_BWD(true, false);
  else USF_CONVEPI_BWD(false, true);
#undef USF_CONVEPI_BWD
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && red && sp.parts > 1) {
    hipLaunchKernelGGL(convepi_finish_kernel, dim3((unsigned)C), dim3(64), 0, s, workspace, gbias, sp.parts);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace usf
