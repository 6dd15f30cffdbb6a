// The homography smoothness loss of stage 2 (include/unsamflow_hip_hg.h;
// losses/loss_blocks.py:125-200 of the reference): per sample the six segments
// with the most occluded pixels get a homography fitted by RANSAC to their
// reliable pixels, and the loss is the L1 distance of the flow to it.
//
// The fit is seven launches on the caller's stream, no host sync in between:
//
//   clear      zero the statistics and the hypothesis scores (a kernel, not a
//              memset node: segpool.hip has the history)
//   stats      per (sample, id) pixel / occluded / reliable counts: [3][K] tables
//              in LDS, one LDS atomic per distinct id of a wave step, merged with
//              integer atomics
//   select     one workgroup per sample: six rounds of a block-wide maximum over
//              (occluded count, -id) keys, the drop rules, the records
//   compact    one workgroup per sample walks the image in raster order; ballot
//              ranks inside a wave, wave totals in LDS, a running offset per
//              slot: a scan, so every list is raster ordered
//   hypotheses one lane per hypothesis: four hashed list positions, the 8x8
//              system in fp64 registers (fully unrolled elimination)
//   score      workgroups over (point chunk, slot x hypothesis group, sample):
//              points tiled through LDS as float4 (x, y, u, v), every lane keeps
//              its hypothesis in registers and reads the points as LDS
//              broadcasts; one integer atomic per (workgroup, hypothesis)
//   refit      one workgroup per (sample, slot): best hypothesis, four passes
//              over the slot's list (centroids, mean distances, normal equations,
//              recount), fp64 sums in one fixed order (strided per thread, xor
//              butterfly per wave, waves in sequence), the solve in one lane
//
// The loss is a dense pass with per-workgroup fp64 partials and a fixed-order
// finalisation; its backward recomputes diff from flow, seg and the records.
#include <algorithm>

#include "seg_key.h"
#include "usf_common.h"
#include "wave.h"

#include "../../include/unsamflow_hip_hg.h"

namespace usf {
namespace {

constexpr int kSlots = USF_HG_SLOTS;
constexpr int kRec = USF_HG_RECORD_WORDS;
constexpr int kPending = -1;        // status between select and refit; never leaves usf_hg_fit_f32
constexpr int kHypWords = 12;       // H[9], valid, 2 pad: 48-byte hypotheses
constexpr int kStatNT = 256;        // statistics: threads, pixels per workgroup
constexpr int kStatPix = 1024;
constexpr int kSelNT = 256;         // selection: K <= 4 * kSelNT
constexpr int kCompNT = 1024;       // compaction: one workgroup per sample
constexpr int kHypNT = 64;          // hypotheses per workgroup of the solve
constexpr int kScoreNT = 256;       // hypotheses per workgroup of the scoring
constexpr int kScoreTile = 1024;    // points per LDS tile (16 KB)
constexpr int kScoreChunk = 1024;   // points per workgroup: one tile (8 workgroups per 8k-point slot fill the chip)
constexpr int kRefitNT = 512;
constexpr int kLossNT = 256;        // loss: threads, pixels per thread
constexpr int kLossPix = 4;

static_assert(USF_HG_MAX_K <= 4 * kSelNT, "selection keeps four candidate ids per thread");

// bad segment ids seen by this code object's kernels (usf_device_errors)
__device__ int g_hg_errors = 0;

__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7fc00000u); }

// the pair of pixel p: pts1 = (x, y), pts2 = pts1 + flow, fp32 as the reference forms them
// (p comes from a list in the workspace: nothing is read outside the sample whatever it holds)
__device__ __forceinline__ float4 pixel_pair(const float* __restrict__ fl, int HW, int W, int p) {
  p = (unsigned)p < (unsigned)HW ? p : 0;
  const int y = p / W, x = p - y * W;
  return make_float4((float)x, (float)y, (float)x + fl[p], (float)y + fl[HW + p]);
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// maximum of x over the workgroup, in every thread; red: NT / 64 words
template <int NT>
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long x, unsigned long long* red) {
  x = wave_max_u64(x);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  unsigned long long m = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) m = red[w] > m ? red[w] : m;
  __syncthreads();
  return m;
}

// v[i] summed over the workgroup in one fixed order (xor butterfly per wave, waves in sequence),
// left in red[0 .. N); red: (NT / 64) * N doubles, N <= NT
template <int N, int NT>
__device__ __forceinline__ void block_sum_lds(double (&v)[N], double* red) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) v[i] += __shfl_xor(v[i], sh);
  }
  __syncthreads();  // the previous call's readers are done
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[(threadIdx.x >> 6) * N + i] = v[i];
  }
  __syncthreads();
  if (threadIdx.x < N) {  // column i is read by thread i alone
    double s = red[threadIdx.x];
    for (int w = 1; w < NT / 64; ++w) s += red[w * N + threadIdx.x];
    red[threadIdx.x] = s;
  }
  __syncthreads();
}

// the same, the sums in every thread
template <int N, int NT>
__device__ __forceinline__ void block_sum(double (&v)[N], double* red) {
  block_sum_lds<N, NT>(v, red);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = red[i];
}

// A h = A[.][8] by Gaussian elimination with partial pivoting (the first largest
// |pivot| from the top); false if a pivot is <= tol. Fully unrolled: A stays in registers.
__device__ __forceinline__ bool solve8(double (&A)[8][9], double tol, double (&h)[8]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    int p = k;
    double best = fabs(A[k][k]);
#pragma unroll
    for (int r = k + 1; r < 8; ++r) {
      const double a = fabs(A[r][k]);
      if (a > best) {
        best = a;
        p = r;
      }
    }
    ok = ok && best > tol;
#pragma unroll
    for (int r = k + 1; r < 8; ++r) {
      const bool sw = p == r;
#pragma unroll
      for (int c = k; c < 9; ++c) {
        const double a = A[k][c], b = A[r][c];
        A[k][c] = sw ? b : a;
        A[r][c] = sw ? a : b;
      }
    }
    const double inv = 1.0 / (ok ? A[k][k] : 1.0);
#pragma unroll
    for (int r = k + 1; r < 8; ++r) {
      const double f = A[r][k] * inv;
#pragma unroll
      for (int c = k + 1; c < 9; ++c) A[r][c] -= f * A[k][c];
    }
  }
#pragma unroll
  for (int k = 7; k >= 0; --k) {
    double s = A[k][8];
#pragma unroll
    for (int c = k + 1; c < 8; ++c) s -= A[k][c] * h[c];
    h[k] = s / (ok ? A[k][k] : 1.0);
  }
  return ok;
}

// the transfer-error test of the header, fp64
__device__ __forceinline__ bool inlier64(const double (&H)[9], const float4 q, double thr2) {
  const double x = q.x, y = q.y, u = q.z, v = q.w;
  const double X = H[0] * x + H[1] * y + H[2], Y = H[3] * x + H[4] * y + H[5], Wd = H[6] * x + H[7] * y + H[8];
  const double dx = X - u * Wd, dy = Y - v * Wd;
  return Wd != 0.0 && dx * dx + dy * dy <= thr2 * Wd * Wd;
}

// ------------------------------------------------------------------- fit --
__global__ __launch_bounds__(256) void hg_clear_kernel(int* __restrict__ w, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) w[i] = 0;
}

// grid (pixel chunks, B); LDS: [3][K] counts (pixels, occluded, reliable)
__global__ __launch_bounds__(kStatNT) void hg_stats_kernel(const float* __restrict__ seg,
                                                           const float* __restrict__ occ, int* __restrict__ stats,
                                                           int HW, int K) {
  extern __shared__ int tab[];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < 3 * K; i += kStatNT) tab[i] = 0;
  __syncthreads();

  const float* sg = seg + (long long)b * HW;
  const float* oc = occ + (long long)b * HW;
  const int chunk0 = blockIdx.x * kStatPix;
  bool bad = false;
  for (int st = 0; st < kStatPix / kStatNT; ++st) {
    const int p0 = chunk0 + (st * (kStatNT / 64) + wave) * 64;
    if (p0 >= HW) break;  // wave-uniform
    const int p = p0 + lane;
    const bool valid = p < HW;
    const int key = valid ? seg_key(sg[p], K) : -1;
    bad |= valid && key < 0;
    const float o = valid ? oc[p] : 0.f;
    const unsigned long long mo = __ballot(key >= 0 && o != 0.f);
    const unsigned long long mr = __ballot(key >= 0 && (1.f - o) != 0.f);
    // one id after another (segment maps are piecewise constant: mostly one to three per step)
    unsigned long long rem = __ballot(key >= 0);
    while (rem) {
      const int l = __ffsll((long long)rem) - 1;
      const int k = __shfl(key, l);
      const unsigned long long m = __ballot(key == k) & rem;
      if (lane == l) {
        atomicAdd(&tab[k], __popcll(m));
        if (m & mo) atomicAdd(&tab[K + k], __popcll(m & mo));
        if (m & mr) atomicAdd(&tab[2 * K + k], __popcll(m & mr));
      }
      rem &= ~m;
    }
  }
  if (__any(bad) && lane == 0) atomicOr(&g_hg_errors, USF_DEVERR_HG_BAD_ID);
  __syncthreads();

  int* g = stats + (long long)b * 3 * K;
  for (int i = threadIdx.x; i < 3 * K; i += kStatNT) {
    const int n = tab[i];
    if (n) atomicAdd(&g[i], n);
  }
}

// grid (B): the six slots by (occluded count descending, id ascending, id != 0), the drop rules
__global__ __launch_bounds__(kSelNT) void hg_select_kernel(const int* __restrict__ stats, int* __restrict__ records,
                                                           int K) {
  __shared__ unsigned long long red[kSelNT / 64];
  __shared__ int chosen[kSlots];
  const int b = blockIdx.x;
  const int* st = stats + (long long)b * 3 * K;
  unsigned long long key[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = threadIdx.x + i * kSelNT;
    key[i] = (id >= 1 && id < K) ? (((unsigned long long)(unsigned)st[K + id] << 32) | (0xFFFFFFFFu - (unsigned)id))
                                 : 0ull;
  }
  for (int r = 0; r < kSlots; ++r) {
    unsigned long long m = key[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) m = key[i] > m ? key[i] : m;
    const unsigned long long best = block_max_u64<kSelNT>(m, red);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (best && key[i] == best) key[i] = 0ull;
    if (threadIdx.x == 0) chosen[r] = best ? (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)) : -1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int off = 0;
    for (int s = 0; s < kSlots; ++s) {
      int* rec = records + ((long long)b * kSlots + s) * kRec;
      const int id = chosen[s];
      const int n_seg = id < 0 ? 0 : st[id], n_rel = id < 0 ? 0 : st[2 * K + id];
      int status = kPending;
      if (id < 0)
        status = USF_HG_EMPTY;
      else if (n_rel < 4)
        status = USF_HG_FEW_RELIABLE;
      else if (5ll * n_rel < (long long)n_seg)
        status = USF_HG_LOW_RELIABLE;
      rec[0] = id;
      rec[1] = status;
      rec[2] = n_seg;
      rec[3] = n_rel;
      rec[4] = 0;
      for (int i = 5; i < 14; ++i) rec[i] = 0;
      rec[14] = -1;
      rec[15] = off;
      if (status == kPending) off += n_rel;
    }
  }
}

// grid (B): the raster-ordered reliable-pixel lists of the pending slots, one after another
__global__ __launch_bounds__(kCompNT) void hg_compact_kernel(const float* __restrict__ seg,
                                                             const float* __restrict__ occ,
                                                             const int* __restrict__ records, int* __restrict__ list,
                                                             int HW) {
  constexpr int NW = kCompNT / 64;
  __shared__ int tot[NW][kSlots];
  __shared__ int run[kSlots];
  __shared__ float sid[kSlots];
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < kSlots) {
    const int* rec = records + ((long long)b * kSlots + threadIdx.x) * kRec;
    sid[threadIdx.x] = rec[1] == kPending ? (float)rec[0] : quiet_nan();  // a NaN matches no pixel
    run[threadIdx.x] = rec[15];
  }
  __syncthreads();
  float ids[kSlots];
#pragma unroll
  for (int k = 0; k < kSlots; ++k) ids[k] = sid[k];
  const float* sg = seg + (long long)b * HW;
  const float* oc = occ + (long long)b * HW;
  int* out = list + (long long)b * HW;
  const unsigned long long below = (1ull << lane) - 1;
  for (int p0 = 0; p0 < HW; p0 += kCompNT) {
    const int p = p0 + threadIdx.x;
    const bool valid = p < HW;
    const float s = valid ? sg[p] : quiet_nan();
    const bool rel = valid && (1.f - oc[valid ? p : 0]) != 0.f;
    int slot = -1;
#pragma unroll
    for (int k = 0; k < kSlots; ++k)
      if (rel && s == ids[k]) slot = k;
    int rank = 0;
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
      const unsigned long long m = __ballot(slot == k);
      if (slot == k) rank = __popcll(m & below);
      if (lane == 0) tot[wave][k] = __popcll(m);
    }
    __syncthreads();
    if (slot >= 0) {
      int at = run[slot] + rank;
      for (int w = 0; w < wave; ++w) at += tot[w][slot];
      if (at < HW) out[at] = p;  // always true: the lists partition a subset of the pixels
    }
    __syncthreads();
    if (threadIdx.x < kSlots) {
      int a = 0;
      for (int w = 0; w < NW; ++w) a += tot[w][threadIdx.x];
      run[threadIdx.x] += a;
    }
    __syncthreads();
  }
}

// grid (hypothesis groups, slots, B): one lane per hypothesis
__global__ __launch_bounds__(kHypNT) void hg_hypothesis_kernel(const float* __restrict__ flow, long long fbs,
                                                               const int* __restrict__ records,
                                                               const int* __restrict__ list, float* __restrict__ hyp,
                                                               int HW, int W, int n_hyp, unsigned long long seed) {
  const int b = blockIdx.z, slot = blockIdx.y;
  const int j = blockIdx.x * kHypNT + threadIdx.x;
  const int* rec = records + ((long long)b * kSlots + slot) * kRec;
  if (rec[1] != kPending || j >= n_hyp) return;
  const int n_rel = rec[3];
  const int* lst = list + (long long)b * HW + rec[15];
  const float* fl = flow + (long long)b * fbs;

  const unsigned long long base = mix64(seed);
  const unsigned long long c0 = ((unsigned long long)(b * 8 + slot) << 34) | ((unsigned long long)j << 2);
  int q[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) q[t] = (int)(((mix64(base + (c0 | (unsigned)t)) >> 32) * (unsigned long long)n_rel) >> 32);
  bool ok = q[0] != q[1] && q[0] != q[2] && q[0] != q[3] && q[1] != q[2] && q[1] != q[3] && q[2] != q[3];

  double A[8][9];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float4 pp = pixel_pair(fl, HW, W, lst[q[t]]);
    const double x = pp.x, y = pp.y, u = pp.z, v = pp.w;
    A[2 * t][0] = x, A[2 * t][1] = y, A[2 * t][2] = 1.0, A[2 * t][3] = 0.0, A[2 * t][4] = 0.0, A[2 * t][5] = 0.0;
    A[2 * t][6] = -x * u, A[2 * t][7] = -y * u, A[2 * t][8] = u;
    A[2 * t + 1][0] = 0.0, A[2 * t + 1][1] = 0.0, A[2 * t + 1][2] = 0.0, A[2 * t + 1][3] = x, A[2 * t + 1][4] = y;
    A[2 * t + 1][5] = 1.0, A[2 * t + 1][6] = -x * v, A[2 * t + 1][7] = -y * v, A[2 * t + 1][8] = v;
  }
  double h[8];
  ok = solve8(A, 1e-10, h) && ok;
#pragma unroll
  for (int i = 0; i < 8; ++i) ok = ok && isfinite(h[i]);
  float* o = hyp + (((long long)b * kSlots + slot) * n_hyp + j) * kHypWords;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = ok ? (float)h[i] : 0.f;
  o[8] = 1.f;
  o[9] = ok ? 1.f : 0.f;
}

// grid (point chunks, slots * hypothesis groups, B)
__global__ __launch_bounds__(kScoreNT) void hg_score_kernel(const float* __restrict__ flow, long long fbs,
                                                            const int* __restrict__ records,
                                                            const int* __restrict__ list,
                                                            const float* __restrict__ hyp, int* __restrict__ score,
                                                            int HW, int W, int n_hyp, int ngrp, float thr2) {
  __shared__ float4 pts[kScoreTile];
  const int b = blockIdx.z, slot = blockIdx.y / ngrp, grp = blockIdx.y - slot * ngrp;
  const int* rec = records + ((long long)b * kSlots + slot) * kRec;
  if (rec[1] != kPending) return;  // uniform
  const int n_rel = rec[3];
  const int start = blockIdx.x * kScoreChunk;
  if (start >= n_rel) return;  // uniform
  const int end = min(start + kScoreChunk, n_rel);
  const int* lst = list + (long long)b * HW + rec[15];
  const float* fl = flow + (long long)b * fbs;

  const int j = grp * kScoreNT + threadIdx.x;
  float H[9];
  bool live = j < n_hyp;
  if (live) {
    const float* h = hyp + (((long long)b * kSlots + slot) * n_hyp + j) * kHypWords;
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = h[i];
    live = h[9] != 0.f;
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = 0.f;
  }
  int cnt = 0;
  for (int t0 = start; t0 < end; t0 += kScoreTile) {
    const int n = min(kScoreTile, end - t0);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kScoreNT) pts[i] = pixel_pair(fl, HW, W, lst[t0 + i]);
    __syncthreads();
    if (live) {
      for (int i = 0; i < n; ++i) {
        const float4 q = pts[i];  // the same address in every lane: an LDS broadcast
        const float X = H[0] * q.x + H[1] * q.y + H[2], Y = H[3] * q.x + H[4] * q.y + H[5];
        const float Wd = H[6] * q.x + H[7] * q.y + H[8];
        const float dx = X - q.z * Wd, dy = Y - q.w * Wd;
        cnt += (Wd != 0.f && dx * dx + dy * dy <= thr2 * Wd * Wd) ? 1 : 0;
      }
    }
  }
  if (live && cnt) atomicAdd(&score[((long long)b * kSlots + slot) * n_hyp + j], cnt);
}

// grid (slots, B): best hypothesis, Hartley-normalised least-squares refit on its inliers, recount
__global__ __launch_bounds__(kRefitNT) void hg_refit_kernel(const float* __restrict__ flow, long long fbs,
                                                            int* __restrict__ records, const int* __restrict__ list,
                                                            const float* __restrict__ hyp,
                                                            const int* __restrict__ score, int HW, int W, int n_hyp,
                                                            float thr) {
  constexpr int NW = kRefitNT / 64;
  __shared__ double red[NW * 44];
  __shared__ unsigned long long redk[NW];
  __shared__ float Hs[9];
  __shared__ int fail;
  const int slot = blockIdx.x, b = blockIdx.y;
  int* rec = records + ((long long)b * kSlots + slot) * kRec;
  if (rec[1] != kPending) return;  // uniform
  const int n_rel = rec[3];
  const int* lst = list + (long long)b * HW + rec[15];
  const float* fl = flow + (long long)b * fbs;
  const long long hs = ((long long)b * kSlots + slot) * n_hyp;

  // the largest score, the lowest j on ties
  unsigned long long key = 0ull;
  for (int j = threadIdx.x; j < n_hyp; j += kRefitNT) {
    const unsigned long long k = ((unsigned long long)(unsigned)score[hs + j] << 32) | (0xFFFFFFFFu - (unsigned)j);
    key = k > key ? k : key;
  }
  key = block_max_u64<kRefitNT>(key, redk);
  const int best_n = (int)(key >> 32), best_j = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
  if (best_n < 4) {  // uniform
    if (threadIdx.x == 0) {
      rec[1] = USF_HG_DEGENERATE;
      rec[14] = best_n > 0 ? best_j : -1;
    }
    return;
  }
  double H0[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) H0[i] = (double)hyp[(hs + best_j) * kHypWords + i];
  const double thr2 = (double)thr * (double)thr;

  // pass 1: the inliers' count and centroids
  double s5[5] = {0, 0, 0, 0, 0};
  for (int q = threadIdx.x; q < n_rel; q += kRefitNT) {
    const float4 pp = pixel_pair(fl, HW, W, lst[q]);
    if (inlier64(H0, pp, thr2)) {
      s5[0] += 1.0;
      s5[1] += (double)pp.x;
      s5[2] += (double)pp.y;
      s5[3] += (double)pp.z;
      s5[4] += (double)pp.w;
    }
  }
  block_sum<5, kRefitNT>(s5, red);
  const double n = s5[0];
  const double c1x = s5[1] / n, c1y = s5[2] / n, c2x = s5[3] / n, c2y = s5[4] / n;

  // pass 2: mean distances to the centroids
  double s2[2] = {0, 0};
  for (int q = threadIdx.x; q < n_rel; q += kRefitNT) {
    const float4 pp = pixel_pair(fl, HW, W, lst[q]);
    if (inlier64(H0, pp, thr2)) {
      const double ax = (double)pp.x - c1x, ay = (double)pp.y - c1y, bx = (double)pp.z - c2x, by = (double)pp.w - c2y;
      s2[0] += sqrt(ax * ax + ay * ay);
      s2[1] += sqrt(bx * bx + by * by);
    }
  }
  block_sum<2, kRefitNT>(s2, red);
  const double d1 = s2[0] / n, d2 = s2[1] / n;
  if (!(n >= 4.0) || !(d1 > 0.0) || !(d2 > 0.0)) {  // uniform
    if (threadIdx.x == 0) {
      rec[1] = USF_HG_DEGENERATE;
      rec[14] = best_j;
    }
    return;
  }
  const double sc1 = sqrt(2.0) / d1, sc2 = sqrt(2.0) / d2;

  // pass 3: the normal equations of the h33 = 1 system: upper triangle of A^T A (36), A^T b (8)
  double acc[44];
#pragma unroll
  for (int i = 0; i < 44; ++i) acc[i] = 0.0;
  for (int q = threadIdx.x; q < n_rel; q += kRefitNT) {
    const float4 pp = pixel_pair(fl, HW, W, lst[q]);
    if (inlier64(H0, pp, thr2)) {
      const double x = sc1 * ((double)pp.x - c1x), y = sc1 * ((double)pp.y - c1y);
      const double u = sc2 * ((double)pp.z - c2x), v = sc2 * ((double)pp.w - c2y);
      const double r1[8] = {x, y, 1.0, 0.0, 0.0, 0.0, -x * u, -y * u};
      const double r2[8] = {0.0, 0.0, 0.0, x, y, 1.0, -x * v, -y * v};
      int t = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int k = i; k < 8; ++k) acc[t++] += r1[i] * r1[k] + r2[i] * r2[k];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[36 + i] += r1[i] * u + r2[i] * v;
    }
  }
  block_sum_lds<44, kRefitNT>(acc, red);

  if (threadIdx.x == 0) {
    double A[8][9];
    int t = 0;
    double dmax = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int k = i; k < 8; ++k) {
        A[i][k] = red[t];
        A[k][i] = red[t];
        ++t;
      }
      A[i][8] = red[36 + i];
      dmax = fmax(dmax, fabs(A[i][i]));
    }
    double h[8];
    bool ok = solve8(A, 1e-11 * dmax, h);
    // H = T2^-1 * Hn * T1
    const double Hn[3][3] = {{h[0], h[1], h[2]}, {h[3], h[4], h[5]}, {h[6], h[7], 1.0}};
    double M[3][3], Hd[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      M[r][0] = Hn[r][0] * sc1;
      M[r][1] = Hn[r][1] * sc1;
      M[r][2] = Hn[r][2] - sc1 * (Hn[r][0] * c1x + Hn[r][1] * c1y);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Hd[c] = M[0][c] / sc2 + c2x * M[2][c];
      Hd[3 + c] = M[1][c] / sc2 + c2y * M[2][c];
      Hd[6 + c] = M[2][c];
    }
    const double w = Hd[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      Hd[i] /= w;
      ok = ok && isfinite(Hd[i]);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) Hs[i] = ok ? (float)Hd[i] : 0.f;
    fail = ok ? 0 : 1;
  }
  __syncthreads();
  if (fail) {  // uniform
    if (threadIdx.x == 0) {
      rec[1] = USF_HG_DEGENERATE;
      rec[14] = best_j;
    }
    return;
  }

  // pass 4: the reliable pairs within thr of the rounded H
  double H1[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) H1[i] = (double)Hs[i];
  double s1[1] = {0};
  for (int q = threadIdx.x; q < n_rel; q += kRefitNT)
    if (inlier64(H1, pixel_pair(fl, HW, W, lst[q]), thr2)) s1[0] += 1.0;
  block_sum<1, kRefitNT>(s1, red);
  if (threadIdx.x == 0) {
    const int n_inl = (int)s1[0];
    rec[1] = 2ll * n_inl >= (long long)n_rel ? USF_HG_ACCEPTED : USF_HG_LOW_INLIER;
    rec[4] = n_inl;
#pragma unroll
    for (int i = 0; i < 9; ++i) rec[5 + i] = __float_as_int(Hs[i]);
    rec[14] = best_j;
  }
}

// ------------------------------------------------------------------ loss --
// the accepted slots of a sample: id (NaN: not accepted) and H, 10 floats per slot
__device__ __forceinline__ void load_slots(const int* __restrict__ records, int b, float (*sl)[10]) {
  if (threadIdx.x < kSlots * 10) {
    const int s = threadIdx.x / 10, i = threadIdx.x - s * 10;
    const int* rec = records + ((long long)b * kSlots + s) * kRec;
    sl[s][i] = i == 0 ? (rec[1] == USF_HG_ACCEPTED ? (float)rec[0] : quiet_nan()) : __int_as_float(rec[4 + i]);
  }
  __syncthreads();
}

// diff = dehom(H (x, y, 1)) - (p + flow) of pixel p, false outside the accepted segments. H and
// p + flow are the fp32 values the reference holds; the product, the divide and the difference are
// taken in fp64, so the loss carries no per-pixel rounding and sign(diff) is the exact one
__device__ __forceinline__ bool pixel_diff(const float (*sl)[10], const float* __restrict__ sg,
                                           const float* __restrict__ fl, int HW, int W, int p, double& dx,
                                           double& dy) {
  const float s = sg[p];
  int slot = -1;
#pragma unroll
  for (int k = 0; k < kSlots; ++k)
    if (s == sl[k][0]) slot = k;
  if (slot < 0) return false;
  const float* H = &sl[slot][1];
  const float4 q = pixel_pair(fl, HW, W, p);
  const double x = q.x, y = q.y;
  const double X = (double)H[0] * x + (double)H[1] * y + (double)H[2];
  const double Y = (double)H[3] * x + (double)H[4] * y + (double)H[5];
  const double Wd = (double)H[6] * x + (double)H[7] * y + (double)H[8];
  dx = X / Wd - (double)q.z;
  dy = Y / Wd - (double)q.w;
  return true;
}

// grid (pixel chunks, B)
__global__ __launch_bounds__(kLossNT) void hg_loss_fwd_kernel(const float* __restrict__ flow, long long fbs,
                                                              const float* __restrict__ seg,
                                                              const int* __restrict__ records,
                                                              double* __restrict__ partials, int HW, int W) {
  __shared__ float sl[kSlots][10];
  __shared__ double red[kLossNT / 64];
  const int b = blockIdx.y;
  load_slots(records, b, sl);
  const float* sg = seg + (long long)b * HW;
  const float* fl = flow + (long long)b * fbs;
  double v[1] = {0.0};
#pragma unroll
  for (int i = 0; i < kLossPix; ++i) {
    const int p = (blockIdx.x * kLossPix + i) * kLossNT + threadIdx.x;
    double dx, dy;
    if (p < HW && pixel_diff(sl, sg, fl, HW, W, p, dx, dy)) v[0] += fabs(dx) + fabs(dy);
  }
  block_sum<1, kLossNT>(v, red);
  if (threadIdx.x == 0) partials[(long long)b * gridDim.x + blockIdx.x] = v[0];
}

__global__ __launch_bounds__(kLossNT) void hg_loss_final_kernel(const double* __restrict__ partials, int n,
                                                                double denom, float* __restrict__ out) {
  __shared__ double red[kLossNT / 64];
  double v[1] = {0.0};
  for (int i = threadIdx.x; i < n; i += kLossNT) v[0] += partials[i];
  block_sum<1, kLossNT>(v, red);
  if (threadIdx.x == 0) out[0] = (float)(v[0] / denom);
}

// grid (pixel chunks, B)
__global__ __launch_bounds__(kLossNT) void hg_loss_bwd_kernel(const float* __restrict__ flow, long long fbs,
                                                              const float* __restrict__ seg,
                                                              const int* __restrict__ records,
                                                              const float* __restrict__ gloss,
                                                              float* __restrict__ gflow, int HW, int W, double denom) {
  __shared__ float sl[kSlots][10];
  const int b = blockIdx.y;
  load_slots(records, b, sl);
  const float* sg = seg + (long long)b * HW;
  const float* fl = flow + (long long)b * fbs;
  float* g = gflow + (long long)b * 2 * HW;
  const float coef = (float)((double)gloss[0] / denom);
#pragma unroll
  for (int i = 0; i < kLossPix; ++i) {
    const int p = (blockIdx.x * kLossPix + i) * kLossNT + threadIdx.x;
    if (p >= HW) continue;
    double dx, dy;
    float gx = 0.f, gy = 0.f;
    if (pixel_diff(sl, sg, fl, HW, W, p, dx, dy)) {
      gx = dx > 0.0 ? -coef : (dx < 0.0 ? coef : 0.f);
      gy = dy > 0.0 ? -coef : (dy < 0.0 ? coef : 0.f);
    }
    g[p] = gx;
    g[HW + p] = gy;
  }
}

// workspace, in 32-bit words: statistics [B][3][K] | scores [B][6][n_hyp] (both zeroed per call)
//                             | hypotheses [B][6][n_hyp][12] | lists [B][HW]
struct Layout {
  long long stats, score, hyp, list, words;
};
Layout layout(int B, int HW, int K, int n_hyp) {
  Layout l;
  l.stats = 0;
  l.score = l.stats + (long long)B * 3 * K;
  l.hyp = l.score + (long long)B * kSlots * n_hyp;
  l.list = l.hyp + (long long)B * kSlots * n_hyp * kHypWords;
  l.words = l.list + (long long)B * HW;
  l.words += l.words & 1;
  return l;
}

int loss_chunks(int HW) { return (HW + kLossNT * kLossPix - 1) / (kLossNT * kLossPix); }

}  // namespace

int hg_device_errors(bool clear) {
  return read_clear_flags(HIP_SYMBOL(g_hg_errors), clear);
}

long long hg_workspace_bytes(int B, int H, int W, int K, int n_hyp) { return layout(B, H * W, K, n_hyp).words * 4; }

hipError_t hg_fit_launch(const float* flow, long long fbs, const float* seg, const float* occ, int K, float thr,
                         int n_hyp, unsigned long long seed, int* records, void* workspace, int B, int H, int W,
                         hipStream_t s) {
  const int HW = H * W;
  const Layout l = layout(B, HW, K, n_hyp);
  int* ws = static_cast<int*>(workspace);
  int* stats = ws + l.stats;
  int* score = ws + l.score;
  float* hyp = reinterpret_cast<float*>(ws + l.hyp);
  int* list = ws + l.list;
  hipError_t e;
#define USF_HG_CHECK()       \
  e = hipGetLastError();     \
  if (e != hipSuccess) return e
  hipLaunchKernelGGL(hg_clear_kernel, dim3((unsigned)std::min<long long>((l.hyp + 255) / 256, 2048)), dim3(256), 0, s,
                     ws, l.hyp);
  USF_HG_CHECK();
  hipLaunchKernelGGL(hg_stats_kernel, dim3((HW + kStatPix - 1) / kStatPix, B), dim3(kStatNT), (size_t)3 * K * 4, s, seg,
                     occ, stats, HW, K);
  USF_HG_CHECK();
  hipLaunchKernelGGL(hg_select_kernel, dim3(B), dim3(kSelNT), 0, s, stats, records, K);
  USF_HG_CHECK();
  hipLaunchKernelGGL(hg_compact_kernel, dim3(B), dim3(kCompNT), 0, s, seg, occ, records, list, HW);
  USF_HG_CHECK();
  hipLaunchKernelGGL(hg_hypothesis_kernel, dim3((n_hyp + kHypNT - 1) / kHypNT, kSlots, B), dim3(kHypNT), 0, s, flow,
                     fbs, records, list, hyp, HW, W, n_hyp, seed);
  USF_HG_CHECK();
  const int ngrp = (n_hyp + kScoreNT - 1) / kScoreNT;
  hipLaunchKernelGGL(hg_score_kernel, dim3((HW + kScoreChunk - 1) / kScoreChunk, kSlots * ngrp, B), dim3(kScoreNT), 0,
                     s, flow, fbs, records, list, hyp, score, HW, W, n_hyp, ngrp, thr * thr);
  USF_HG_CHECK();
  hipLaunchKernelGGL(hg_refit_kernel, dim3(kSlots, B), dim3(kRefitNT), 0, s, flow, fbs, records, list, hyp, score, HW,
                     W, n_hyp, thr);
#undef USF_HG_CHECK
  return hipGetLastError();
}

int hg_loss_partials(int B, int H, int W) { return B * loss_chunks(H * W); }

hipError_t hg_loss_fwd_launch(const float* flow, long long fbs, const float* seg, const int* records, double* partials,
                              float* out, int B, int H, int W, hipStream_t s) {
  const int HW = H * W, nchunk = loss_chunks(HW);
  hipLaunchKernelGGL(hg_loss_fwd_kernel, dim3(nchunk, B), dim3(kLossNT), 0, s, flow, fbs, seg, records, partials, HW,
                     W);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hg_loss_final_kernel, dim3(1), dim3(kLossNT), 0, s, partials, B * nchunk, (double)HW * B, out);
  return hipGetLastError();
}

hipError_t hg_loss_bwd_launch(const float* flow, long long fbs, const float* seg, const int* records,
                              const float* gloss, float* gflow, int B, int H, int W, hipStream_t s) {
  const int HW = H * W;
  hipLaunchKernelGGL(hg_loss_bwd_kernel, dim3(loss_chunks(HW), B), dim3(kLossNT), 0, s, flow, fbs, seg, records, gloss,
                     gflow, HW, W, (double)HW * B);
  return hipGetLastError();
}

}  // namespace usf
