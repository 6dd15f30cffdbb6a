// C ABI of libunsamflow_hip.so (declared in include/unsamflow_hip.h).
// Argument validation + error reporting; the launches live in the .hip files
// beside it (usf_common.h declares them, grouped by file).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../include/unsamflow_hip.h"
#include "../../include/unsamflow_hip_ar.h"
#include "../../include/unsamflow_hip_census.h"
#include "../../include/unsamflow_hip_convepi.h"
#include "../../include/unsamflow_hip_eval.h"
#include "../../include/unsamflow_hip_fakeobj.h"
#include "../../include/unsamflow_hip_hg.h"
#include "../../include/unsamflow_hip_segpool.h"
#include "usf_common.h"

namespace usf {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

void clear_error() { g_err[0] = '\0'; }

static bool check_dims(const char* fn, int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) {
    set_error("%s: non-positive shape B=%d C=%d H=%d W=%d", fn, B, C, H, W);
    return false;
  }
  // per-sample BYTE offsets are 32-bit inside the kernels (the correlation's
  // LDS-DMA descriptors span one sample and park masked lanes at 0x7FFFFFF0)
  const long long per_sample = (long long)C * H * W;
  const long long max_elems = 0x7FFFFFF0LL / 4 - 1;
  if (per_sample > max_elems || (long long)H * W * 81 > max_elems) {
    set_error("%s: per-sample tensor too large (C*H*W=%lld)", fn, per_sample);
    return false;
  }
  return true;
}

// The alignment contract of the headers: {parameter name, pointer, required
// alignment in bytes}. The kernels choose their 8- and 16-byte paths from the
// shape, so the address must hold what the shape promises; this runs after the
// other argument checks and before any launch. A null pointer passes (whether
// it may be null is checked before).
struct PtrAlign {
  const char* name;
  const void* p;
  unsigned align;
};

static bool check_align(const char* fn, std::initializer_list<PtrAlign> ps) {
  for (const PtrAlign& a : ps)
    if (a.p && (reinterpret_cast<uintptr_t>(a.p) & (a.align - 1u))) {
      set_error("%s: %s must be %u-byte aligned", fn, a.name, a.align);
      return false;
    }
  return true;
}

// check_align of the per-level (per-scale) pointers of a host array; nullable array
static bool check_align_each(const char* fn, const char* name, const void* const* ps, int n, unsigned align) {
  if (!ps) return true;
  for (int k = 0; k < n; ++k)
    if (!check_align(fn, {{name, ps[k], align}})) return false;
  return true;
}

// A channel slice of a dense NCHW buffer starts c0 * H*W floats into it: it is
// 16-byte aligned whenever H*W % 4 == 0, and only such shapes take a vector
// path through a slice pointer. Any other shape needs 4 bytes.
static unsigned slice_align(int H, int W) { return ((long long)H * W) % 4 == 0 ? 16u : 4u; }

// USF_SYNC_CHECK=1: synchronise the stream after every launch and report any
// asynchronous fault against the launch that caused it (debug only).
static bool sync_check() {
  static const bool on = [] {
    const char* v = getenv("USF_SYNC_CHECK");
    return v && v[0] == '1';
  }();
  return on;
}

// A stream under graph capture cannot be synchronised: the debug checks skip it
// (the replays of the graph run the same kernels unchecked).
static bool capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

static bool sync_check_on(hipStream_t s) { return sync_check() && !capturing(s); }

// With USF_SYNC_CHECK=1 every entry point first drains the stream, so a fault
// raised by an EARLIER (non-usf) kernel is reported as such, not blamed on us.
static int pre_check(const char* fn, hipStream_t s) {
  if (!sync_check_on(s)) return 0;
  const hipError_t e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    fprintf(stderr, "[usf] %s: stream already faulted BEFORE this launch: %s\n", fn, hipGetErrorString(e));
    set_error("%s: stream faulted before launch: %s (%d)", fn, hipGetErrorString(e), (int)e);
    return (int)e;
  }
  return 0;
}

static int finish(const char* fn, hipError_t e, hipStream_t s) {
  if (e == hipSuccess && sync_check_on(s)) {
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) fprintf(stderr, "[usf] %s: fault after launch: %s\n", fn, hipGetErrorString(e));
    // a bad segment id, cache slot or sample size is the caller's data, not a failed launch: left for
    // usf_device_errors
    const int flags = e == hipSuccess ? device_errors(s, true,
                                                      ~(USF_DEVERR_SEGPOOL_BAD_ID | USF_DEVERR_HG_BAD_ID |
                                                        USF_DEVERR_FAKEOBJ_BAD_SLOT | USF_DEVERR_EVAL_BAD_SIZE))
                                      : 0;
    if (flags > 0) {
      fprintf(stderr, "[usf] %s: device error flags 0x%x\n", fn, flags);
      set_error("%s: device error flags 0x%x", fn, flags);
      return USF_EDEVICE;
    }
  }
  if (e != hipSuccess) {
    set_error("%s: HIP launch failed: %s (%d)", fn, hipGetErrorString(e), (int)e);
    return (int)e;
  }
  return 0;
}

}  // namespace usf

using namespace usf;

extern "C" {

int usf_abi_version(void) { return USF_ABI_VERSION; }

#ifndef USF_BUILD_ID
#define USF_BUILD_ID "unstamped"
#endif
const char* usf_build_id(void) { return USF_BUILD_ID; }

const char* usf_last_error_string(void) { return g_err; }

int usf_corr_fwd_f32(const float* x1, const float* x2, float* out, int B, int C, int H, int W,
                     int d, void* stream) {
  clear_error();
  if (!check_dims("usf_corr_fwd_f32", B, C, H, W)) return USF_EINVAL;
  if (d < 1 || d > 4) {
    set_error("usf_corr_fwd_f32: max_displacement %d not in [1,4]", d);
    return USF_EINVAL;
  }
  if (!x1 || !x2 || !out) {
    set_error("usf_corr_fwd_f32: null pointer");
    return USF_EINVAL;
  }
  if (!check_align("usf_corr_fwd_f32", {{"x1", x1, 16}, {"x2", x2, 16}, {"out", out, 16}})) return USF_EINVAL;
  if (const int pe = pre_check("usf_corr_fwd_f32", (hipStream_t)stream)) return pe;
  const long long k2 = (long long)(2 * d + 1) * (2 * d + 1);
  return finish("usf_corr_fwd_f32",
                corr_fwd_launch(x1, x2, out, B, C, H, W, d, (hipStream_t)stream,
                                FwdEpi{k2 * H * W, 0, 0.f}),
                (hipStream_t)stream);
}

long long usf_corr_fwd_workspace(int B, int C, int H, int W, int d) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || d < 1 || d > 4) return 0;
  return corr_fwd_workspace(B, C, H, W, d);
}

long long usf_corr_act_mask_words(int B, int H, int W, int d) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return corr_act_mask_words(B, H, W, d);
}

int usf_corr_fwd_ex_f32(const float* x1, const float* x2, float* out, long long out_bstride,
                        int act, float slope, unsigned long long* act_mask, float* workspace,
                        long long workspace_floats, int B, int C, int H, int W, int d, void* stream) {
  clear_error();
  if (!check_dims("usf_corr_fwd_ex_f32", B, C, H, W)) return USF_EINVAL;
  if (d < 1 || d > 4) {
    set_error("usf_corr_fwd_ex_f32: max_displacement %d not in [1,4]", d);
    return USF_EINVAL;
  }
  if (!x1 || !x2 || !out) {
    set_error("usf_corr_fwd_ex_f32: null pointer");
    return USF_EINVAL;
  }
  const long long k2 = (long long)(2 * d + 1) * (2 * d + 1);
  if (out_bstride < k2 * H * W && B > 1) {
    set_error("usf_corr_fwd_ex_f32: out batch stride %lld < (2d+1)^2*H*W", out_bstride);
    return USF_EINVAL;
  }
  if (act != USF_ACT_NONE && act != USF_ACT_LEAKY_RELU) {
    set_error("usf_corr_fwd_ex_f32: unknown act %d", act);
    return USF_EINVAL;
  }
  if (act_mask && act != USF_ACT_LEAKY_RELU) {
    set_error("usf_corr_fwd_ex_f32: act_mask needs act = LeakyReLU (act=%d)", act);
    return USF_EINVAL;
  }
  if (!check_align("usf_corr_fwd_ex_f32", {{"x1", x1, 16},
                                           {"x2", x2, 16},
                                           {"out", out, slice_align(H, W)},
                                           {"act_mask", act_mask, 16},
                                           {"workspace", workspace, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check("usf_corr_fwd_ex_f32", (hipStream_t)stream)) return pe;
  FwdEpi ep{out_bstride, act, slope};
  ep.mask = act_mask;
  return finish("usf_corr_fwd_ex_f32",
                corr_fwd_launch(x1, x2, out, B, C, H, W, d, (hipStream_t)stream, ep, workspace,
                                workspace_floats),
                (hipStream_t)stream);
}

int usf_corr_bwd_f32(const float* x1, const float* x2, const float* gout, float* gx1,
                     float* gx2, int B, int C, int H, int W, int d, void* stream) {
  clear_error();
  if (!check_dims("usf_corr_bwd_f32", B, C, H, W)) return USF_EINVAL;
  if (d < 1 || d > 4) {
    set_error("usf_corr_bwd_f32: max_displacement %d not in [1,4]", d);
    return USF_EINVAL;
  }
  if (!gout || (gx1 && !x2) || (gx2 && !x1)) {
    set_error("usf_corr_bwd_f32: null input pointer");
    return USF_EINVAL;
  }
  if (!check_align("usf_corr_bwd_f32", {{"x1", x1, 16}, {"x2", x2, 16}, {"gout", gout, 16}, {"gx1", gx1, 16}, {"gx2", gx2, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check("usf_corr_bwd_f32", (hipStream_t)stream)) return pe;
  const long long k2 = (long long)(2 * d + 1) * (2 * d + 1);
  return finish("usf_corr_bwd_f32",
                corr_bwd_launch(x1, x2, gout, gx1, gx2, B, C, H, W, d, (hipStream_t)stream,
                                BwdEpi{k2 * H * W}),
                (hipStream_t)stream);
}

int usf_corr_bwd_ex_f32(const float* x1, const float* x2, const float* gout, long long g_bstride,
                        const float* act_out, const unsigned long long* act_mask, float slope,
                        float* scratch, float* gx1, float* gx2, int B, int C, int H, int W, int d,
                        void* stream) {
  clear_error();
  if (!check_dims("usf_corr_bwd_ex_f32", B, C, H, W)) return USF_EINVAL;
  if (d < 1 || d > 4) {
    set_error("usf_corr_bwd_ex_f32: max_displacement %d not in [1,4]", d);
    return USF_EINVAL;
  }
  if (!gout || (gx1 && !x2) || (gx2 && !x1)) {
    set_error("usf_corr_bwd_ex_f32: null input pointer");
    return USF_EINVAL;
  }
  const long long k2 = (long long)(2 * d + 1) * (2 * d + 1);
  if (g_bstride < k2 * H * W && B > 1) {
    set_error("usf_corr_bwd_ex_f32: gradient batch stride %lld < (2d+1)^2*H*W", g_bstride);
    return USF_EINVAL;
  }
  const auto aligned = [&] {
    return check_align("usf_corr_bwd_ex_f32", {{"x1", x1, 16},
                                               {"x2", x2, 16},
                                               {"gout", gout, slice_align(H, W)},
                                               {"act_out", act_mask ? nullptr : act_out, slice_align(H, W)},
                                               {"act_mask", act_mask, 16},
                                               {"scratch", act_mask || !act_out ? nullptr : scratch, 16},
                                               {"gx1", gx1, 16},
                                               {"gx2", gx2, 16}});
  };
  if (act_mask) {  // derivative from the forward's sign mask, inside the backward's g loads
    if (!aligned()) return USF_EINVAL;
    if (const int pe = pre_check("usf_corr_bwd_ex_f32", (hipStream_t)stream)) return pe;
    BwdEpi ep{g_bstride};
    ep.mask = act_mask;
    ep.slope = slope;
    return finish("usf_corr_bwd_ex_f32",
                  corr_bwd_launch(x1, x2, gout, gx1, gx2, B, C, H, W, d, (hipStream_t)stream, ep),
                  (hipStream_t)stream);
  }
  if (act_out && !scratch) {
    set_error("usf_corr_bwd_ex_f32: act_out needs a scratch of usf_corr_bwd_ex_scratch() floats here");
    return USF_EINVAL;
  }
  if (!aligned()) return USF_EINVAL;
  if (const int pe = pre_check("usf_corr_bwd_ex_f32", (hipStream_t)stream)) return pe;
  const BwdEpi ep{g_bstride};
  if (act_out) {  // derivative + de-concat in one dense pass, then the plain backward
    const hipError_t e = leaky_bwd_gather_launch(gout, act_out, g_bstride, slope, scratch, B,
                                                 (int)k2, H, W, (hipStream_t)stream);
    if (e != hipSuccess) return finish("usf_corr_bwd_ex_f32", e, (hipStream_t)stream);
    return finish("usf_corr_bwd_ex_f32",
                  corr_bwd_launch(x1, x2, scratch, gx1, gx2, B, C, H, W, d, (hipStream_t)stream,
                                  BwdEpi{k2 * H * W}),
                  (hipStream_t)stream);
  }
  return finish("usf_corr_bwd_ex_f32",
                corr_bwd_launch(x1, x2, gout, gx1, gx2, B, C, H, W, d, (hipStream_t)stream, ep),
                (hipStream_t)stream);
}

long long usf_corr_bwd_ex_scratch(int B, int C, int H, int W, int d) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || d < 1 || d > 4) return 0;
  return (long long)B * (2 * d + 1) * (2 * d + 1) * H * W;
}

int usf_warp_fwd_f32(const float* x, const float* flow, long long flow_bstride, float* out,
                     int B, int C, int H, int W, int pad_mode, void* stream) {
  clear_error();
  if (!check_dims("usf_warp_fwd_f32", B, C, H, W)) return USF_EINVAL;
  if (pad_mode != USF_PAD_ZEROS && pad_mode != USF_PAD_BORDER) {
    set_error("usf_warp_fwd_f32: unknown pad_mode %d", pad_mode);
    return USF_EINVAL;
  }
  if (!x || !flow || !out) {
    set_error("usf_warp_fwd_f32: null pointer");
    return USF_EINVAL;
  }
  if (flow_bstride < 2LL * H * W && B > 1) {
    set_error("usf_warp_fwd_f32: flow batch stride %lld < 2*H*W", flow_bstride);
    return USF_EINVAL;
  }
  if (!check_align("usf_warp_fwd_f32", {{"x", x, 16}, {"flow", flow, 4}, {"out", out, 16}})) return USF_EINVAL;
  if (const int pe = pre_check("usf_warp_fwd_f32", (hipStream_t)stream)) return pe;
  return finish("usf_warp_fwd_f32",
                warp_fwd_launch(x, flow, flow_bstride, out, B, C, H, W, pad_mode, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_warp_fwd_up_f32(const float* x, const float* coarse_flow, float* up_flow, float* out, int B, int C, int H,
                        int W, int pad_mode, void* stream) {
  clear_error();
  const char* fn = "usf_warp_fwd_up_f32";
  if (!check_dims(fn, B, C, H, W)) return USF_EINVAL;
  if (pad_mode != USF_PAD_ZEROS && pad_mode != USF_PAD_BORDER) {
    set_error("%s: unknown pad_mode %d", fn, pad_mode);
    return USF_EINVAL;
  }
  if ((H & 1) || (W & 1) || H < 2 || W < 2) {
    set_error("%s: H=%d W=%d must be even (the coarse flow is [B,2,H/2,W/2])", fn, H, W);
    return USF_EINVAL;
  }
  if (!x || !coarse_flow || !up_flow || !out) {
    set_error("%s: null pointer", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"x", x, 16}, {"coarse_flow", coarse_flow, 16}, {"up_flow", up_flow, 16}, {"out", out, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn, warp_fwd_up_launch(x, coarse_flow, up_flow, out, B, C, H, W, pad_mode, (hipStream_t)stream),
                (hipStream_t)stream);
}

static int warp_bwd_common(const char* fn, const float* x, const float* flow, long long flow_bstride,
                           const float* gout, float* gx, float* gflow, void* ws, long long ws_bytes, int B,
                           int C, int H, int W, int pad_mode, void* stream, bool persist = false) {
  clear_error();
  if (!check_dims(fn, B, C, H, W)) return USF_EINVAL;
  if (pad_mode != USF_PAD_ZEROS && pad_mode != USF_PAD_BORDER) {
    set_error("%s: unknown pad_mode %d", fn, pad_mode);
    return USF_EINVAL;
  }
  if (!flow || !gout || (gflow && !x)) {
    set_error("%s: null input pointer", fn);
    return USF_EINVAL;
  }
  if (flow_bstride < 2LL * H * W && B > 1) {
    set_error("%s: flow batch stride %lld < 2*H*W", fn, flow_bstride);
    return USF_EINVAL;
  }
  if (ws_bytes < 0) {
    set_error("%s: negative workspace size", fn);
    return USF_EINVAL;
  }
  if (ws && (reinterpret_cast<uintptr_t>(ws) & 15)) {  // the binned gather reads it with 16-byte loads
    set_error("%s: workspace must be 16-byte aligned", fn);
    return USF_EINVAL;
  }
  if (persist) {
    if (!ws || ws_bytes < warp_bwd_persist_workspace(B, C, H, W)) {
      set_error("%s: persistent workspace of %lld bytes < usf_warp_bwd_persist_workspace = %lld", fn, ws_bytes,
                warp_bwd_persist_workspace(B, C, H, W));
      return USF_EINVAL;
    }
    if (C > 256 || H >= 32768 || W >= 65536) {  // gather channel groups fit a 32-bit dirty mask; packed (y, x)
      set_error("%s: C=%d H=%d W=%d beyond the persistent form (C <= 256, H < 32768, W < 65536)", fn, C, H, W);
      return USF_EINVAL;
    }
    // the gather reads both count buffers through one buffer descriptor with
    // 32-bit byte offsets: 2 x 4 bytes per cell must stay below 2^31
    if (8LL * B * (H + 1) * (W + 1) >= (1LL << 31)) {
      set_error("%s: B=%d H=%d W=%d: 8*B*(H+1)*(W+1) >= 2^31 (count buffers past 32-bit offsets)", fn, B, H, W);
      return USF_EINVAL;
    }
  }
  if (!check_align(fn, {{"x", x, 16}, {"flow", flow, 4}, {"gout", gout, 16}, {"gx", gx, 16}, {"gflow", gflow, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  hipError_t e = warp_bwd_launch(x, flow, flow_bstride, gout, gx, gflow, B, C, H, W, pad_mode, (hipStream_t)stream,
                                 ws, ws_bytes, persist);
  if (e == hipSuccess && persist && gx && sync_check_on((hipStream_t)stream))
    e = warp_persist_check_launch(ws, B, C, H, W, (hipStream_t)stream);
  return finish(fn, e, (hipStream_t)stream);
}

int usf_warp_bwd_f32(const float* x, const float* flow, long long flow_bstride,
                     const float* gout, float* gx, float* gflow, int B, int C, int H, int W,
                     int pad_mode, void* stream) {
  return warp_bwd_common("usf_warp_bwd_f32", x, flow, flow_bstride, gout, gx, gflow, nullptr, 0, B, C, H, W,
                         pad_mode, stream);
}

int usf_warp_bwd_ex_f32(const float* x, const float* flow, long long flow_bstride, const float* gout,
                        float* gx, float* gflow, void* workspace, long long workspace_bytes, int B, int C,
                        int H, int W, int pad_mode, void* stream) {
  return warp_bwd_common("usf_warp_bwd_ex_f32", x, flow, flow_bstride, gout, gx, gflow, workspace,
                         workspace ? workspace_bytes : 0, B, C, H, W, pad_mode, stream);
}

long long usf_warp_bwd_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return warp_bwd_workspace(B, H, W);
}

int usf_warp_bwd_persist_f32(const float* x, const float* flow, long long flow_bstride, const float* gout,
                             float* gx, float* gflow, void* workspace, long long workspace_bytes, int B, int C,
                             int H, int W, int pad_mode, void* stream) {
  return warp_bwd_common("usf_warp_bwd_persist_f32", x, flow, flow_bstride, gout, gx, gflow, workspace,
                         workspace_bytes, B, C, H, W, pad_mode, stream, true);
}

long long usf_warp_bwd_persist_workspace(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return warp_bwd_persist_workspace(B, C, H, W);
}

static bool check_splat(const char* fn, const float* flow, long long fbs, const float* out, int B,
                        int H, int W) {
  if (!check_dims(fn, B, 2, H, W)) return false;
  if (!flow || !out) {
    set_error("%s: null pointer", fn);
    return false;
  }
  if (fbs < 2LL * H * W && B > 1) {
    set_error("%s: flow batch stride %lld < 2*H*W", fn, fbs);
    return false;
  }
  return true;
}

int usf_splat_map_f32(const float* flow, long long flow_bstride, float* map, int B, int H, int W,
                      int absolute, void* stream) {
  clear_error();
  if (!check_splat("usf_splat_map_f32", flow, flow_bstride, map, B, H, W)) return USF_EINVAL;
  if (!check_align("usf_splat_map_f32", {{"flow", flow, 4}, {"map", map, 16}})) return USF_EINVAL;
  if (const int pe = pre_check("usf_splat_map_f32", (hipStream_t)stream)) return pe;
  return finish("usf_splat_map_f32",
                splat_launch(flow, flow_bstride, map, B, H, W, absolute != 0, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_occ_backward_f32(const float* flow21, long long flow_bstride, float* occ, int B, int H,
                         int W, float th, void* stream) {
  clear_error();
  if (!check_splat("usf_occ_backward_f32", flow21, flow_bstride, occ, B, H, W)) return USF_EINVAL;
  if (!check_align("usf_occ_backward_f32", {{"flow21", flow21, 4}, {"occ", occ, 16}})) return USF_EINVAL;
  if (const int pe = pre_check("usf_occ_backward_f32", (hipStream_t)stream)) return pe;
  return finish("usf_occ_backward_f32",
                occ_backward_launch(flow21, flow_bstride, occ, B, H, W, th, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_occ_backward_persist_f32(const float* flow21, long long flow_bstride, float* occ, float* map,
                                 long long map_bytes, int B, int H, int W, float th, void* stream) {
  clear_error();
  const char* fn = "usf_occ_backward_persist_f32";
  if (!check_splat(fn, flow21, flow_bstride, occ, B, H, W)) return USF_EINVAL;
  if (!map || map_bytes < 4LL * B * H * W || map == occ) {
    set_error("%s: map must be a separate buffer of >= 4*B*H*W = %lld bytes (got %lld)", fn, 4LL * B * H * W,
              map_bytes);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"flow21", flow21, 4}, {"occ", occ, 16}, {"map", map, 16}})) return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  hipError_t e = occ_backward_persist_launch(flow21, flow_bstride, occ, map, B, H, W, th, (hipStream_t)stream);
  if (e == hipSuccess && sync_check_on((hipStream_t)stream))
    e = zero_check_launch(map, 4LL * B * H * W, (hipStream_t)stream);
  return finish(fn, e, (hipStream_t)stream);
}

int usf_occ_vis_pair_persist_f32(const float* flow4, long long flow_bstride, float* vis, float* map,
                                 long long map_bytes, int B, int H, int W, float th, void* stream) {
  clear_error();
  const char* fn = "usf_occ_vis_pair_persist_f32";
  if (!check_dims(fn, B, 4, H, W)) return USF_EINVAL;
  if (!flow4 || !vis) {
    set_error("%s: null pointer", fn);
    return USF_EINVAL;
  }
  if (B > 1 && flow_bstride != 4LL * H * W) {
    set_error("%s: flow4 must be a dense [B,4,H,W] tensor (batch stride %lld != 4*H*W)", fn, flow_bstride);
    return USF_EINVAL;
  }
  if (!map || map_bytes < 8LL * B * H * W || map == vis) {
    set_error("%s: map must be a separate buffer of >= 8*B*H*W = %lld bytes (got %lld)", fn, 8LL * B * H * W,
              map_bytes);
    return USF_EINVAL;
  }
  if (2LL * B * H * W >= (1LL << 31)) {
    set_error("%s: 2*B*H*W beyond 32-bit indexing", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"flow4", flow4, 4}, {"vis", vis, 16}, {"map", map, 16}})) return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  hipError_t e = occ_vis_pair_persist_launch(flow4, vis, map, B, H, W, th, (hipStream_t)stream);
  if (e == hipSuccess && sync_check_on((hipStream_t)stream))
    e = zero_check_launch(map, 8LL * B * H * W, (hipStream_t)stream);
  return finish(fn, e, (hipStream_t)stream);
}

int usf_occ_bidirection_f32(const float* flow12, long long flow12_bstride, const float* flow21,
                            long long flow21_bstride, float* occ, int B, int H, int W, float scale,
                            float bias, void* stream) {
  clear_error();
  if (!check_splat("usf_occ_bidirection_f32", flow12, flow12_bstride, occ, B, H, W) ||
      !check_splat("usf_occ_bidirection_f32", flow21, flow21_bstride, occ, B, H, W))
    return USF_EINVAL;
  if (!check_align("usf_occ_bidirection_f32", {{"flow12", flow12, 4}, {"flow21", flow21, 4}, {"occ", occ, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check("usf_occ_bidirection_f32", (hipStream_t)stream)) return pe;
  return finish("usf_occ_bidirection_f32",
                occ_bidirection_launch(flow12, flow12_bstride, flow21, flow21_bstride, occ, B, H, W, scale,
                                       bias, (hipStream_t)stream),
                (hipStream_t)stream);
}

// ------------------- the photometric losses: usf_photo_loss_*, usf_census_loss_* --
// The two families take the same arguments in the same order (the census one
// has one weight and fixes C = 3) and differ here only in what LossKind holds.
struct LossKind {
  const char* name;                      // usf_<name>_loss_*
  bool census;                           // C == 3 and an interior pixel; else C <= 3
  int basis_planes;                      // of the gradient basis, per direction
  int (*partials)(int B, int H, int W);  // floats per direction
  hipError_t (*bwd_launch)(int, const float* const*, const float*, const float*, float* const*, const int*,
                           const int*, int, int, hipStream_t);
};
static const LossKind kPhoto{"photo", false, 4, photo_partials, photo_pyr_bwd_launch};
static const LossKind kCensus{"census", true, 2, census_partials, census_pyr_bwd_launch};

// one scale's inputs; planes = flow planes per sample: 2 (one direction; pass
// mask2 = mask) or 4 (a pair)
static bool check_loss_inputs(const char* fn, const LossKind& kind, const float* src, const float* tgt,
                              const float* mask, const float* mask2, const float* flow, long long fbs, int planes,
                              int B, int C, int H, int W, int pad_mode) {
  if (!check_dims(fn, B, C, H, W)) return false;
  if (kind.census && C != 3) {
    set_error("%s: C=%d image channels (the census transform needs 3)", fn, C);
    return false;
  }
  if (C > 3) {
    set_error("%s: C=%d image channels > 3", fn, C);
    return false;
  }
  if (kind.census && (H < 3 || W < 3)) {
    set_error("%s: H=%d W=%d has no interior pixel (H, W >= 3)", fn, H, W);
    return false;
  }
  if (pad_mode != USF_PAD_ZEROS && pad_mode != USF_PAD_BORDER) {
    set_error("%s: unknown pad_mode %d", fn, pad_mode);
    return false;
  }
  if (!src || !tgt || !mask || !mask2 || !flow) {
    set_error("%s: null input pointer", fn);
    return false;
  }
  if (fbs < (long long)planes * H * W && B > 1) {
    set_error("%s: flow batch stride %lld < %d*H*W", fn, fbs, planes);
    return false;
  }
  return true;
}

static bool check_loss_outputs(const char* fn, const float* partials, const float* out) {
  if (!partials || !out) set_error("%s: null output pointer", fn);
  return partials && out;
}

// alignment of one scale's pointers (pair: the names of the with_bk forms)
static bool check_loss_align(const char* fn, bool pair, const float* a, const float* b, const float* m1,
                             const float* m2, const float* flow, const float* partials, const float* out,
                             const float* basis) {
  return check_align(fn, {{pair ? "im1" : "src", a, 16},
                          {pair ? "im2" : "tgt", b, 16},
                          {pair ? "mask1" : "mask", m1, 16},
                          {"mask2", m2, 16},
                          {"flow", flow, 4},
                          {"partials", partials, 16},
                          {"out", out, 4},
                          {"grad_basis", basis, 16}});
}

static long long loss_pyramid_partials(const LossKind& kind, int nscale, const int* H, const int* W, int B) {
  if (nscale < 1 || nscale > 4 || !H || !W || B <= 0) return 0;
  long long n = 0;
  for (int k = 0; k < nscale; ++k) {
    if (H[k] <= 0 || W[k] <= 0) return 0;
    n += 2LL * kind.partials(B, H[k], W[k]);
  }
  return n;
}

static bool check_loss_pyramid(const char* fn, const LossKind& kind, int nscale, const float* const* im1,
                               const float* const* im2, const float* const* mask1, const float* const* mask2,
                               const float* const* flow, const long long* fbs, const int* H, const int* W,
                               const float* partials, long long partials_floats, const float* out,
                               float* const* grad_basis, int B, int C, int pad_mode) {
  if (nscale < 1 || nscale > 4 || !im1 || !im2 || !mask1 || !mask2 || !flow || !fbs || !H || !W) {
    set_error("%s: nscale %d not in [1,4] or a null array", fn, nscale);
    return false;
  }
  for (int k = 0; k < nscale; ++k) {
    if (!check_loss_inputs(fn, kind, im1[k], im2[k], mask1[k], mask2[k], flow[k], fbs[k], 4, B, C, H[k], W[k],
                           pad_mode))
      return false;
    if (grad_basis && !grad_basis[k]) {
      set_error("%s: scale %d: grad_basis given for some scales only", fn, k);
      return false;
    }
  }
  const long long need = loss_pyramid_partials(kind, nscale, H, W, B);
  if (!partials || !out || partials_floats < need) {
    set_error("%s: partials of %lld floats < usf_%s_loss_pyramid_partials = %lld, or null out", fn, partials_floats,
              kind.name, need);
    return false;
  }
  for (int k = 0; k < nscale; ++k)
    if (!check_loss_align(fn, true, im1[k], im2[k], mask1[k], mask2[k], flow[k], partials, out,
                          grad_basis ? grad_basis[k] : nullptr))
      return false;
  return true;
}

// the backward of nscale scales of ndir directions each: checks and launch
static int loss_bwd(const char* fn, const LossKind& kind, int nscale, const float* const* grad_basis,
                    const float* coef, const float* grad_loss, float* const* grad_flow, const int* H, const int* W,
                    int B, int ndir, void* stream) {
  clear_error();
  if (nscale < 1 || nscale > 4) {
    set_error("%s: nscale %d not in [1,4]", fn, nscale);
    return USF_EINVAL;
  }
  if (!grad_basis || !grad_flow || !H || !W || !coef || !grad_loss) {
    set_error("%s: null pointer", fn);
    return USF_EINVAL;
  }
  for (int k = 0; k < nscale; ++k) {
    if (!check_dims(fn, B, 2 * kind.basis_planes, H[k], W[k])) return USF_EINVAL;
    if (!grad_basis[k] || !grad_flow[k]) {
      set_error("%s: scale %d: null pointer", fn, k);
      return USF_EINVAL;
    }
  }
  if (ndir != 1 && ndir != 2) {
    set_error("%s: ndir=%d (1 or 2)", fn, ndir);
    return USF_EINVAL;
  }
  for (int k = 0; k < nscale; ++k)
    if (!check_align(fn, {{"grad_basis", grad_basis[k], 16},
                          {"coef", coef, 4},
                          {"grad_loss", grad_loss, 4},
                          {"grad_flow", grad_flow[k], 16}}))
      return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn, kind.bwd_launch(nscale, grad_basis, coef, grad_loss, grad_flow, H, W, B, ndir, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_photo_loss_partials(int B, int H, int W) {
  return (B > 0 && H > 0 && W > 0) ? photo_partials(B, H, W) : 0;
}

int usf_photo_loss_fwd_f32(const float* src, const float* tgt, const float* mask, const float* flow,
                           long long flow_bstride, float* partials, float* out, float* grad_basis,
                           int B, int C, int H, int W, int pad_mode, float w_l1, float w_ssim,
                           void* stream) {
  clear_error();
  const char* fn = "usf_photo_loss_fwd_f32";
  if (!check_loss_inputs(fn, kPhoto, src, tgt, mask, mask, flow, flow_bstride, 2, B, C, H, W, pad_mode) ||
      !check_loss_outputs(fn, partials, out) ||
      !check_loss_align(fn, false, src, tgt, mask, nullptr, flow, partials, out, grad_basis))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                photo_fwd_launch(src, tgt, mask, flow, flow_bstride, partials, out, grad_basis, B, C, H, W, pad_mode,
                                 w_l1, w_ssim, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_photo_loss_pair_fwd_f32(const float* im1, const float* im2, const float* mask1,
                                const float* mask2, const float* flow, long long flow_bstride,
                                float* partials, float* out, float* grad_basis, int B, int C, int H,
                                int W, int pad_mode, float w_l1, float w_ssim, void* stream) {
  clear_error();
  const char* fn = "usf_photo_loss_pair_fwd_f32";
  if (!check_loss_inputs(fn, kPhoto, im1, im2, mask1, mask2, flow, flow_bstride, 4, B, C, H, W, pad_mode) ||
      !check_loss_outputs(fn, partials, out) ||
      !check_loss_align(fn, true, im1, im2, mask1, mask2, flow, partials, out, grad_basis))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                photo_pair_fwd_launch(im1, im2, mask1, mask2, flow, flow_bstride, partials, out, grad_basis, B, C, H,
                                      W, pad_mode, w_l1, w_ssim, (hipStream_t)stream),
                (hipStream_t)stream);
}

long long usf_photo_loss_pyramid_partials(int nscale, const int* H, const int* W, int B) {
  return loss_pyramid_partials(kPhoto, nscale, H, W, B);
}

int usf_photo_loss_pyramid_fwd_f32(int nscale, const float* const* im1, const float* const* im2,
                                   const float* const* mask1, const float* const* mask2, const float* const* flow,
                                   const long long* flow_bstride, const int* H, const int* W, float* partials,
                                   long long partials_floats, float* out, float* const* grad_basis, int B, int C,
                                   int pad_mode, float w_l1, float w_ssim, void* stream) {
  clear_error();
  const char* fn = "usf_photo_loss_pyramid_fwd_f32";
  if (!check_loss_pyramid(fn, kPhoto, nscale, im1, im2, mask1, mask2, flow, flow_bstride, H, W, partials,
                          partials_floats, out, grad_basis, B, C, pad_mode))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                photo_pyr_fwd_launch(nscale, im1, im2, mask1, mask2, flow, flow_bstride, H, W, partials, out,
                                     grad_basis, B, C, pad_mode, w_l1, w_ssim, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_photo_loss_pyramid_bwd_f32(int nscale, const float* const* grad_basis, const float* coef,
                                   const float* grad_loss, float* const* grad_flow, const int* H, const int* W, int B,
                                   void* stream) {
  return loss_bwd("usf_photo_loss_pyramid_bwd_f32", kPhoto, nscale, grad_basis, coef, grad_loss, grad_flow, H, W, B, 2,
                  stream);
}

int usf_photo_loss_bwd_f32(const float* grad_basis, const float* coef, const float* grad_loss,
                           float* grad_flow, int B, int H, int W, int ndir, void* stream) {
  return loss_bwd("usf_photo_loss_bwd_f32", kPhoto, 1, &grad_basis, coef, grad_loss, &grad_flow, &H, &W, B, ndir,
                  stream);
}

// ------------------------------------------------- unsamflow_hip_census.h --
int usf_census_api_version(void) { return USF_CENSUS_API_VERSION; }

int usf_census_loss_partials(int B, int H, int W) {
  return (B > 0 && H > 0 && W > 0) ? census_partials(B, H, W) : 0;
}

int usf_census_loss_fwd_f32(const float* src, const float* tgt, const float* mask, const float* flow,
                            long long flow_bstride, float* partials, float* out, float* grad_basis, int B, int C,
                            int H, int W, int pad_mode, float w_ternary, void* stream) {
  clear_error();
  const char* fn = "usf_census_loss_fwd_f32";
  if (!check_loss_inputs(fn, kCensus, src, tgt, mask, mask, flow, flow_bstride, 2, B, C, H, W, pad_mode) ||
      !check_loss_outputs(fn, partials, out) ||
      !check_loss_align(fn, false, src, tgt, mask, nullptr, flow, partials, out, grad_basis))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                census_fwd_launch(src, tgt, mask, flow, flow_bstride, partials, out, grad_basis, B, H, W, pad_mode,
                                  w_ternary, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_census_loss_pair_fwd_f32(const float* im1, const float* im2, const float* mask1, const float* mask2,
                                 const float* flow, long long flow_bstride, float* partials, float* out,
                                 float* grad_basis, int B, int C, int H, int W, int pad_mode, float w_ternary,
                                 void* stream) {
  clear_error();
  const char* fn = "usf_census_loss_pair_fwd_f32";
  if (!check_loss_inputs(fn, kCensus, im1, im2, mask1, mask2, flow, flow_bstride, 4, B, C, H, W, pad_mode) ||
      !check_loss_outputs(fn, partials, out) ||
      !check_loss_align(fn, true, im1, im2, mask1, mask2, flow, partials, out, grad_basis))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                census_pair_fwd_launch(im1, im2, mask1, mask2, flow, flow_bstride, partials, out, grad_basis, B, H, W,
                                       pad_mode, w_ternary, (hipStream_t)stream),
                (hipStream_t)stream);
}

long long usf_census_loss_pyramid_partials(int nscale, const int* H, const int* W, int B) {
  return loss_pyramid_partials(kCensus, nscale, H, W, B);
}

int usf_census_loss_pyramid_fwd_f32(int nscale, const float* const* im1, const float* const* im2,
                                    const float* const* mask1, const float* const* mask2, const float* const* flow,
                                    const long long* flow_bstride, const int* H, const int* W, float* partials,
                                    long long partials_floats, float* out, float* const* grad_basis, int B, int C,
                                    int pad_mode, float w_ternary, void* stream) {
  clear_error();
  const char* fn = "usf_census_loss_pyramid_fwd_f32";
  if (!check_loss_pyramid(fn, kCensus, nscale, im1, im2, mask1, mask2, flow, flow_bstride, H, W, partials,
                          partials_floats, out, grad_basis, B, C, pad_mode))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                census_pyr_fwd_launch(nscale, im1, im2, mask1, mask2, flow, flow_bstride, H, W, partials, out,
                                      grad_basis, B, pad_mode, w_ternary, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_census_loss_pyramid_bwd_f32(int nscale, const float* const* grad_basis, const float* coef,
                                    const float* grad_loss, float* const* grad_flow, const int* H, const int* W,
                                    int B, void* stream) {
  return loss_bwd("usf_census_loss_pyramid_bwd_f32", kCensus, nscale, grad_basis, coef, grad_loss, grad_flow, H, W, B,
                  2, stream);
}

int usf_census_loss_bwd_f32(const float* grad_basis, const float* coef, const float* grad_loss, float* grad_flow,
                            int B, int H, int W, int ndir, void* stream) {
  return loss_bwd("usf_census_loss_bwd_f32", kCensus, 1, &grad_basis, coef, grad_loss, &grad_flow, &H, &W, B, ndir,
                  stream);
}

// ----------------------------------------------------- unsamflow_hip_ar.h --
int usf_ar_api_version(void) { return USF_AR_API_VERSION; }

// shape of the AR entries: [B,C,H,W] within the 32-bit per-sample offsets, H, W >= 2
static bool check_ar_dims(const char* fn, int B, int C, int H, int W) {
  if (!check_dims(fn, B, C, H, W)) return false;
  if (H < 2 || W < 2) {
    set_error("%s: H=%d W=%d (the normalised coordinates need H, W >= 2)", fn, H, W);
    return false;
  }
  return true;
}

int usf_ar_transform_f32(const float* img1, const float* img2, const float* flow, long long flow_bstride,
                         const float* mask, const float* theta, const float* noise1, const float* noise2,
                         float* img1_t, float* img2_t, float* flow_t, float* mask_t, int B, int H, int W,
                         void* stream) {
  clear_error();
  const char* fn = "usf_ar_transform_f32";
  if (!check_ar_dims(fn, B, 3, H, W)) return USF_EINVAL;
  if (B > 65535) {
    set_error("%s: B=%d > 65535", fn, B);
    return USF_EINVAL;
  }
  if (!img1 || !img2 || !flow || !mask || !theta) {
    set_error("%s: null input pointer", fn);
    return USF_EINVAL;
  }
  if (!img1_t || !img2_t || !flow_t || !mask_t) {
    set_error("%s: null output pointer", fn);
    return USF_EINVAL;
  }
  if (flow_bstride < 2LL * H * W && B > 1) {
    set_error("%s: flow batch stride %lld < 2*H*W", fn, flow_bstride);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"img1", img1, 16},     {"img2", img2, 16},     {"flow", flow, 4},      {"mask", mask, 16},
                        {"theta", theta, 4},    {"noise1", noise1, 16}, {"noise2", noise2, 16}, {"img1_t", img1_t, 16},
                        {"img2_t", img2_t, 16}, {"flow_t", flow_t, 16}, {"mask_t", mask_t, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                ar_transform_launch(img1, img2, flow, flow_bstride, mask, theta, noise1, noise2, img1_t, img2_t,
                                    flow_t, mask_t, B, H, W, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_ar_loss_partials(int B, int H, int W) { return (B > 0 && H > 0 && W > 0) ? ar_loss_partials(B, H, W) : 0; }

static bool check_ar_loss(const char* fn, const float* pred, const float* target, long long tbs, long long tcs,
                          long long trs, const float* noc, long long nbs, long long nrs, int B, int H, int W,
                          float eps, float q) {
  if (!check_ar_dims(fn, B, 2, H, W)) return false;
  if (B > 65535) {
    set_error("%s: B=%d > 65535", fn, B);
    return false;
  }
  if (!pred || !target || !noc) {
    set_error("%s: null input pointer", fn);
    return false;
  }
  if (tbs < 0 || tcs < 0 || trs < 0 || nbs < 0 || nrs < 0) {
    set_error("%s: negative stride (target %lld/%lld/%lld, noc %lld/%lld)", fn, tbs, tcs, trs, nbs, nrs);
    return false;
  }
  if (!(q > 0.f) || !(eps >= 0.f)) {
    set_error("%s: q=%g eps=%g (need q > 0, eps >= 0)", fn, (double)q, (double)eps);
    return false;
  }
  return true;
}

int usf_ar_loss_fwd_f32(const float* pred, const float* target, long long target_bstride, long long target_cstride,
                        long long target_rstride, const float* noc, long long noc_bstride, long long noc_rstride,
                        const float* denom, float* partials, float* out, int B, int H, int W, float eps, float q,
                        void* stream) {
  clear_error();
  const char* fn = "usf_ar_loss_fwd_f32";
  if (!check_ar_loss(fn, pred, target, target_bstride, target_cstride, target_rstride, noc, noc_bstride, noc_rstride,
                     B, H, W, eps, q))
    return USF_EINVAL;
  if (!partials || !out) {
    set_error("%s: null output pointer", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"pred", pred, 4}, {"target", target, 4}, {"noc", noc, 4}, {"denom", denom, 4},
                        {"partials", partials, 16}, {"out", out, 4}}))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                ar_loss_fwd_launch(pred, target, target_bstride, target_cstride, target_rstride, noc, noc_bstride,
                                   noc_rstride, denom, partials, out, B, H, W, eps, q, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_ar_loss_bwd_f32(const float* pred, const float* target, long long target_bstride, long long target_cstride,
                        long long target_rstride, const float* noc, long long noc_bstride, long long noc_rstride,
                        const float* coef, const float* grad_loss, float* grad_pred, int B, int H, int W, float eps,
                        float q, void* stream) {
  clear_error();
  const char* fn = "usf_ar_loss_bwd_f32";
  if (!check_ar_loss(fn, pred, target, target_bstride, target_cstride, target_rstride, noc, noc_bstride, noc_rstride,
                     B, H, W, eps, q))
    return USF_EINVAL;
  if (!coef || !grad_loss) {
    set_error("%s: null input pointer", fn);
    return USF_EINVAL;
  }
  if (!grad_pred) {
    set_error("%s: null output pointer", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"pred", pred, 4}, {"target", target, 4}, {"noc", noc, 4}, {"coef", coef, 4},
                        {"grad_loss", grad_loss, 4}, {"grad_pred", grad_pred, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                ar_loss_bwd_launch(pred, target, target_bstride, target_cstride, target_rstride, noc, noc_bstride,
                                   noc_rstride, coef, grad_loss, grad_pred, B, H, W, eps, q, (hipStream_t)stream),
                (hipStream_t)stream);
}

// ------------------------------------------------ unsamflow_hip_fakeobj.h --
int usf_fakeobj_api_version(void) { return USF_FAKEOBJ_API_VERSION; }

// shape, flow stride and cache size of both fake-object entries
static bool check_fakeobj(const char* fn, int B, int H, int W, long long fbs, int cache_size) {
  if (!check_ar_dims(fn, B, 6, H, W)) return false;
  if (B > 65535) {
    set_error("%s: B=%d > 65535", fn, B);
    return false;
  }
  if (fbs < 2LL * H * W && B > 1) {
    set_error("%s: flow batch stride %lld < 2*H*W", fn, fbs);
    return false;
  }
  if (cache_size < 1) {
    set_error("%s: cache_size=%d (need >= 1)", fn, cache_size);
    return false;
  }
  return true;
}

int usf_fakeobj_paste_crop_f32(const float* img1, const float* img2, const float* flow, long long flow_bstride,
                               const float* noc, const float* cache_mask, const float* cache_img,
                               const float* cache_motion, const int* slot, const float* param, float* imgs_ot,
                               float* flow_ot, float* noc_ot, int B, int H, int W, int K, int cache_size, int y0,
                               int x0, int ch, int cw, void* stream) {
  clear_error();
  const char* fn = "usf_fakeobj_paste_crop_f32";
  if (!check_fakeobj(fn, B, H, W, flow_bstride, cache_size)) return USF_EINVAL;
  if (K < 1 || K > USF_FAKEOBJ_MAX_K) {
    set_error("%s: K=%d outside [1, %d]", fn, K, USF_FAKEOBJ_MAX_K);
    return USF_EINVAL;
  }
  if (y0 < 0 || x0 < 0 || ch < 1 || cw < 1 || (long long)y0 + ch > H || (long long)x0 + cw > W) {
    set_error("%s: crop window y0=%d x0=%d %dx%d outside the %dx%d image", fn, y0, x0, ch, cw, H, W);
    return USF_EINVAL;
  }
  if (!img1 || !img2 || !flow || !noc || !cache_mask || !cache_img || !cache_motion || !slot || !param) {
    set_error("%s: null input pointer", fn);
    return USF_EINVAL;
  }
  if (!imgs_ot || !flow_ot || !noc_ot) {
    set_error("%s: null output pointer", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"img1", img1, 16},
                        {"img2", img2, 16},
                        {"flow", flow, 4},
                        {"noc", noc, 16},
                        {"cache_mask", cache_mask, 4},
                        {"cache_img", cache_img, 4},
                        {"cache_motion", cache_motion, 4},
                        {"slot", slot, 4},
                        {"param", param, 4},
                        {"imgs_ot", imgs_ot, 16},
                        {"flow_ot", flow_ot, 16},
                        {"noc_ot", noc_ot, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                fakeobj_paste_crop_launch(img1, img2, flow, flow_bstride, noc, cache_mask, cache_img, cache_motion, slot,
                                          param, imgs_ot, flow_ot, noc_ot, B, H, W, K, cache_size, y0, x0, ch, cw,
                                          (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_fakeobj_push_partials(int B, int H, int W) {
  return (B > 0 && H > 0 && W > 0) ? fakeobj_push_partials(B, H, W) : 0;
}

int usf_fakeobj_push_f32(const float* obj_mask, const float* img, const float* flow, long long flow_bstride,
                         const int* slot, float* cache_mask, float* cache_img, float* cache_motion, float* partials,
                         int B, int H, int W, int cache_size, void* stream) {
  clear_error();
  const char* fn = "usf_fakeobj_push_f32";
  if (!check_fakeobj(fn, B, H, W, flow_bstride, cache_size)) return USF_EINVAL;
  if (!obj_mask || !img || !flow || !slot) {
    set_error("%s: null input pointer", fn);
    return USF_EINVAL;
  }
  if (!cache_mask || !cache_img || !cache_motion || !partials) {
    set_error("%s: null output pointer", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"obj_mask", obj_mask, 16},
                        {"img", img, 16},
                        {"flow", flow, 4},
                        {"slot", slot, 4},
                        {"cache_mask", cache_mask, 4},
                        {"cache_img", cache_img, 4},
                        {"cache_motion", cache_motion, 4},
                        {"partials", partials, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                fakeobj_push_launch(obj_mask, img, flow, flow_bstride, slot, cache_mask, cache_img, cache_motion,
                                    partials, B, H, W, cache_size, (hipStream_t)stream),
                (hipStream_t)stream);
}

// --------------------------------------------------- unsamflow_hip_eval.h --
int usf_eval_api_version(void) { return USF_EVAL_API_VERSION; }

// shapes and the prediction's stride of both evaluation entries
static bool check_eval(const char* fn, int B, int h, int w, int Hmax, int Wmax, long long pbs) {
  if (B < 1 || B > 65535) {
    set_error("%s: B=%d outside [1, 65535]", fn, B);
    return false;
  }
  if (h < 2 || w < 2 || Hmax < 2 || Wmax < 2) {
    set_error("%s: h=%d w=%d Hmax=%d Wmax=%d (the align_corners resize needs every size >= 2)", fn, h, w, Hmax, Wmax);
    return false;
  }
  if (!check_dims(fn, B, 2, h, w) || !check_dims(fn, B, 5, Hmax, Wmax)) return false;
  if (pbs < 2LL * h * w && B > 1) {
    set_error("%s: prediction batch stride %lld < 2*h*w", fn, pbs);
    return false;
  }
  return true;
}

int usf_flow_resize_f32(const float* pred, long long pred_bstride, const int* sizes, float* out, int B, int h, int w,
                        int Hmax, int Wmax, void* stream) {
  clear_error();
  const char* fn = "usf_flow_resize_f32";
  if (!check_eval(fn, B, h, w, Hmax, Wmax, pred_bstride)) return USF_EINVAL;
  if (!pred) {
    set_error("%s: null input pointer", fn);
    return USF_EINVAL;
  }
  if (!out) {
    set_error("%s: null output pointer", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"pred", pred, 4}, {"sizes", sizes, 4}, {"out", out, 16}})) return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn, flow_resize_launch(pred, pred_bstride, sizes, out, B, h, w, Hmax, Wmax, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_flow_eval_partials(int B, int Hmax, int Wmax) {
  return (B > 0 && Hmax > 0 && Wmax > 0) ? flow_eval_partials(B, Hmax, Wmax) : 0;
}

int usf_flow_eval_f32(const float* pred, long long pred_bstride, const float* gt, int Cg, const float* move,
                      const int* sizes, float* partials, float* sums, float* metrics, int B, int h, int w, int Hmax,
                      int Wmax, void* stream) {
  clear_error();
  const char* fn = "usf_flow_eval_f32";
  if (!check_eval(fn, B, h, w, Hmax, Wmax, pred_bstride)) return USF_EINVAL;
  if (Cg != 2 && Cg != 4) {
    set_error("%s: Cg=%d ground-truth channels (2: u, v; 4: u, v, valid, noc)", fn, Cg);
    return USF_EINVAL;
  }
  if (!pred || !gt) {
    set_error("%s: null input pointer", fn);
    return USF_EINVAL;
  }
  if (!partials || !sums || !metrics) {
    set_error("%s: null output pointer", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"pred", pred, 4},
                        {"gt", gt, 16},
                        {"move", move, 16},
                        {"sizes", sizes, 4},
                        {"partials", partials, 16},
                        {"sums", sums, 16},
                        {"metrics", metrics, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                flow_eval_launch(pred, pred_bstride, gt, Cg, move, sizes, partials, sums, metrics, B, h, w, Hmax, Wmax,
                                 (hipStream_t)stream),
                (hipStream_t)stream);
}

// ------------------------------------------------ unsamflow_hip_segpool.h --
int usf_segpool_api_version(void) { return USF_SEGPOOL_API_VERSION; }

static bool check_segpool(const char* fn, int B, int C, int H, int W, int K) {
  if (!check_dims(fn, B, C, H, W)) return false;
  if (B > 65535 || C > 65535) {
    set_error("%s: B=%d C=%d (at most 65535 each)", fn, B, C);
    return false;
  }
  if (K < 1 || K > USF_SEGPOOL_MAX_K) {
    set_error("%s: K=%d outside [1, %d]", fn, K, USF_SEGPOOL_MAX_K);
    return false;
  }
  return true;
}

long long usf_segpool_state_words(int B, int C, int K) {
  return (B > 0 && C > 0 && K >= 1 && K <= USF_SEGPOOL_MAX_K) ? segpool_state_words(B, C, K) : 0;
}

int usf_segpool_fwd_f32(const float* proj, const float* seg, float* spread, void* state, int B, int C, int H, int W,
                        int K, void* stream) {
  clear_error();
  const char* fn = "usf_segpool_fwd_f32";
  if (!check_segpool(fn, B, C, H, W, K)) return USF_EINVAL;
  if (!proj || !seg) {
    set_error("%s: null input pointer", fn);
    return USF_EINVAL;
  }
  if (!spread || !state) {
    set_error("%s: null output pointer", fn);
    return USF_EINVAL;
  }
  if ((uintptr_t)state % 4 != 0) {
    set_error("%s: state not 4-byte aligned", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"proj", proj, 16}, {"seg", seg, 16}, {"spread", spread, 16}})) return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                segpool_fwd_launch(proj, seg, spread, static_cast<unsigned*>(state), B, C, H, W, K,
                                   (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_segpool_bwd_f32(const float* proj, const float* seg, const void* state, const float* grad_spread,
                        float* grad_proj, int B, int C, int H, int W, int K, void* stream) {
  clear_error();
  const char* fn = "usf_segpool_bwd_f32";
  if (!check_segpool(fn, B, C, H, W, K)) return USF_EINVAL;
  if (!proj || !seg || !state || !grad_spread) {
    set_error("%s: null input pointer", fn);
    return USF_EINVAL;
  }
  if (!grad_proj) {
    set_error("%s: null output pointer", fn);
    return USF_EINVAL;
  }
  if ((uintptr_t)state % 4 != 0) {
    set_error("%s: state not 4-byte aligned", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"proj", proj, 16}, {"seg", seg, 16}, {"grad_spread", grad_spread, 16}, {"grad_proj", grad_proj, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                segpool_bwd_launch(proj, seg, static_cast<const unsigned*>(state), grad_spread, grad_proj, B, C, H, W,
                                   K, (hipStream_t)stream),
                (hipStream_t)stream);
}

// ----------------------------------------------------- unsamflow_hip_hg.h --
int usf_hg_api_version(void) { return USF_HG_API_VERSION; }

// shape and flow stride of every hg entry
static bool check_hg(const char* fn, int B, int H, int W, long long fbs) {
  if (!check_dims(fn, B, 2, H, W)) return false;
  if (B > 65535) {
    set_error("%s: B=%d (at most 65535)", fn, B);
    return false;
  }
  if (fbs < 2ll * H * W) {
    set_error("%s: flow_bstride=%lld below 2*H*W=%lld", fn, fbs, 2ll * H * W);
    return false;
  }
  return true;
}

static bool check_hg_fit(const char* fn, int K, float thr, int n_hyp) {
  if (K < 1 || K > USF_HG_MAX_K) {
    set_error("%s: K=%d outside [1, %d]", fn, K, USF_HG_MAX_K);
    return false;
  }
  if (n_hyp < 1 || n_hyp > USF_HG_MAX_HYP) {
    set_error("%s: n_hyp=%d outside [1, %d]", fn, n_hyp, USF_HG_MAX_HYP);
    return false;
  }
  if (!(thr > 0.f) || !(thr < 1e18f)) {
    set_error("%s: thr=%g (need a finite thr > 0)", fn, (double)thr);
    return false;
  }
  return true;
}

long long usf_hg_workspace_bytes(int B, int H, int W, int K, int n_hyp) {
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || (long long)H * W > 0x1FFFFFFFLL || K < 1 || K > USF_HG_MAX_K ||
      n_hyp < 1 || n_hyp > USF_HG_MAX_HYP)
    return 0;
  return hg_workspace_bytes(B, H, W, K, n_hyp);
}

int usf_hg_fit_f32(const float* flow, long long flow_bstride, const float* seg, const float* occ, int K, float thr,
                   int n_hyp, unsigned long long seed, void* records, void* workspace, long long workspace_bytes,
                   int B, int H, int W, void* stream) {
  clear_error();
  const char* fn = "usf_hg_fit_f32";
  if (!check_hg(fn, B, H, W, flow_bstride) || !check_hg_fit(fn, K, thr, n_hyp)) return USF_EINVAL;
  if (!flow || !seg || !occ) {
    set_error("%s: null input pointer", fn);
    return USF_EINVAL;
  }
  if (!records || !workspace) {
    set_error("%s: null output pointer", fn);
    return USF_EINVAL;
  }
  if ((uintptr_t)records % 4 != 0 || (uintptr_t)workspace % 8 != 0) {
    set_error("%s: records not 4-byte or workspace not 8-byte aligned", fn);
    return USF_EINVAL;
  }
  const long long need = hg_workspace_bytes(B, H, W, K, n_hyp);
  if (workspace_bytes < need) {
    set_error("%s: workspace of %lld bytes, need %lld (usf_hg_workspace_bytes)", fn, workspace_bytes, need);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"flow", flow, 4}, {"seg", seg, 16}, {"occ", occ, 16}})) return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                hg_fit_launch(flow, flow_bstride, seg, occ, K, thr, n_hyp, seed, static_cast<int*>(records), workspace,
                              B, H, W, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_hg_loss_partials(int B, int H, int W) {
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || (long long)H * W > 0x1FFFFFFFLL) return 0;
  return hg_loss_partials(B, H, W);
}

int usf_hg_loss_fwd_f32(const float* flow, long long flow_bstride, const float* seg, const void* records,
                        double* partials, float* out, int B, int H, int W, void* stream) {
  clear_error();
  const char* fn = "usf_hg_loss_fwd_f32";
  if (!check_hg(fn, B, H, W, flow_bstride)) return USF_EINVAL;
  if (!flow || !seg || !records) {
    set_error("%s: null input pointer", fn);
    return USF_EINVAL;
  }
  if (!partials || !out) {
    set_error("%s: null output pointer", fn);
    return USF_EINVAL;
  }
  if ((uintptr_t)records % 4 != 0 || (uintptr_t)partials % 8 != 0) {
    set_error("%s: records not 4-byte or partials not 8-byte aligned", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"flow", flow, 4}, {"seg", seg, 16}, {"out", out, 4}})) return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                hg_loss_fwd_launch(flow, flow_bstride, seg, static_cast<const int*>(records), partials, out, B, H, W,
                                   (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_hg_loss_bwd_f32(const float* flow, long long flow_bstride, const float* seg, const void* records,
                        const float* grad_loss, float* grad_flow, int B, int H, int W, void* stream) {
  clear_error();
  const char* fn = "usf_hg_loss_bwd_f32";
  if (!check_hg(fn, B, H, W, flow_bstride)) return USF_EINVAL;
  if (!flow || !seg || !records || !grad_loss) {
    set_error("%s: null input pointer", fn);
    return USF_EINVAL;
  }
  if (!grad_flow) {
    set_error("%s: null output pointer", fn);
    return USF_EINVAL;
  }
  if ((uintptr_t)records % 4 != 0) {
    set_error("%s: records not 4-byte aligned", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"flow", flow, 4}, {"seg", seg, 16}, {"grad_loss", grad_loss, 4}, {"grad_flow", grad_flow, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                hg_loss_bwd_launch(flow, flow_bstride, seg, static_cast<const int*>(records), grad_loss, grad_flow, B,
                                   H, W, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_flow_upsample_f32(const float* flow, float* out, int B, int C, int H, int W, int factor,
                          void* stream) {
  clear_error();
  if (!check_dims("usf_flow_upsample_f32", B, C, H, W)) return USF_EINVAL;
  if (factor < 1 || factor > 16 || (long long)C * H * W * factor * factor > 0x1FFFFFFBLL) {
    set_error("usf_flow_upsample_f32: bad factor %d", factor);
    return USF_EINVAL;
  }
  if (!flow || !out) {
    set_error("usf_flow_upsample_f32: null pointer");
    return USF_EINVAL;
  }
  if (!check_align("usf_flow_upsample_f32", {{"flow", flow, 16}, {"out", out, 16}})) return USF_EINVAL;
  if (const int pe = pre_check("usf_flow_upsample_f32", (hipStream_t)stream)) return pe;
  return finish("usf_flow_upsample_f32",
                upsample_fwd_launch(flow, out, B, C, H, W, factor, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_flow_upsample_bwd_f32(const float* grad_out, float* grad_flow, int B, int C, int H, int W,
                              int factor, void* stream) {
  clear_error();
  if (!check_dims("usf_flow_upsample_bwd_f32", B, C, H, W)) return USF_EINVAL;
  if (factor < 1 || factor > 16 || (long long)C * H * W * factor * factor > 0x1FFFFFFBLL) {
    set_error("usf_flow_upsample_bwd_f32: bad factor %d", factor);
    return USF_EINVAL;
  }
  if (!grad_out || !grad_flow) {
    set_error("usf_flow_upsample_bwd_f32: null pointer");
    return USF_EINVAL;
  }
  if (!check_align("usf_flow_upsample_bwd_f32", {{"grad_out", grad_out, 16}, {"grad_flow", grad_flow, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check("usf_flow_upsample_bwd_f32", (hipStream_t)stream)) return pe;
  return finish("usf_flow_upsample_bwd_f32",
                upsample_bwd_launch(grad_out, grad_flow, B, C, H, W, factor, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_flow_upsample_bwd_sum_f32(const float* grad_a, const float* grad_b, float* grad_flow, int B, int C, int H,
                                  int W, int factor, void* stream) {
  clear_error();
  const char* fn = "usf_flow_upsample_bwd_sum_f32";
  if (!check_dims(fn, B, C, H, W)) return USF_EINVAL;
  if (factor < 1 || factor > 16 || (long long)C * H * W * factor * factor > 0x1FFFFFFBLL) {
    set_error("%s: bad factor %d", fn, factor);
    return USF_EINVAL;
  }
  if (!grad_a || !grad_b || !grad_flow) {
    set_error("%s: null pointer", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"grad_a", grad_a, 16}, {"grad_b", grad_b, 16}, {"grad_flow", grad_flow, 16}})) return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn, upsample_bwd_launch(grad_a, grad_flow, B, C, H, W, factor, (hipStream_t)stream, grad_b),
                (hipStream_t)stream);
}

static bool check_convex(const char* fn, int B, int H, int W, int factor) {
  if (!check_dims(fn, B, 2, H, W)) return false;
  if (!convex_factor_ok(factor)) {
    set_error("%s: factor %d (2, 4 or 8)", fn, factor);
    return false;
  }
  if ((long long)9 * factor * factor * H * W > 0x1FFFFFFFLL) {
    set_error("%s: mask plane block too large", fn);
    return false;
  }
  return true;
}

int usf_convex_upsample_f32(const float* flow, const float* mask, float* out, int B, int H, int W,
                            int factor, float mask_scale, void* stream) {
  clear_error();
  const char* fn = "usf_convex_upsample_f32";
  if (!check_convex(fn, B, H, W, factor)) return USF_EINVAL;
  if (!flow || !mask || !out) {
    set_error("%s: null pointer", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"flow", flow, 16}, {"mask", mask, 16}, {"out", out, 16}})) return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn, convex_fwd_launch(flow, mask, out, B, H, W, factor, mask_scale, (hipStream_t)stream),
                (hipStream_t)stream);
}

long long usf_convex_upsample_bwd_scratch(int B, int H, int W) {
  if (B < 0 || H < 0 || W < 0) return 0;
  return convex_bwd_scratch(B, H, W);
}

int usf_convex_upsample_bwd_f32(const float* flow, const float* mask, const float* grad_out,
                                float* grad_flow, float* grad_mask, float* scratch, int B, int H,
                                int W, int factor, float mask_scale, void* stream) {
  clear_error();
  const char* fn = "usf_convex_upsample_bwd_f32";
  if (!check_convex(fn, B, H, W, factor)) return USF_EINVAL;
  if (!flow || !mask || !grad_out) {
    set_error("%s: null input pointer", fn);
    return USF_EINVAL;
  }
  if (grad_flow && !scratch) {
    set_error("%s: grad_flow needs scratch (usf_convex_upsample_bwd_scratch floats)", fn);
    return USF_EINVAL;
  }
  if (!grad_flow && !grad_mask) return 0;
  if (!check_align(fn, {{"flow", flow, 16},
                        {"mask", mask, 16},
                        {"grad_out", grad_out, 16},
                        {"grad_flow", grad_flow, 16},
                        {"grad_mask", grad_mask, 16},
                        {"scratch", grad_flow ? scratch : nullptr, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                convex_bwd_launch(flow, mask, grad_out, grad_flow, grad_mask, scratch, B, H, W, factor,
                                  mask_scale, (hipStream_t)stream),
                (hipStream_t)stream);
}

static bool check_convex_pyr(const char* fn, int n, const int* H, const int* W, int B, int factor) {
  if (n < 1 || n > convex_pyramid_max_levels() || !H || !W) {
    set_error("%s: nlevel %d not in [1,%d] or null size arrays", fn, n, convex_pyramid_max_levels());
    return false;
  }
  if (factor != 4) {
    set_error("%s: factor %d (the pyramid form takes 4, the decoder's)", fn, factor);
    return false;
  }
  for (int l = 0; l < n; ++l)
    if (!check_convex(fn, B, H[l], W[l], factor)) return false;
  return true;
}

long long usf_convex_upsample_pyramid_bwd_scratch(int nlevel, const int* H, const int* W, int B) {
  if (nlevel < 1 || nlevel > convex_pyramid_max_levels() || !H || !W || B <= 0) return 0;
  long long n = 0;
  for (int l = 0; l < nlevel; ++l) n += convex_bwd_scratch(B, H[l], W[l]);
  return n;
}

int usf_convex_upsample_pyramid_f32(int nlevel, const float* const* flow, const float* const* mask, float* const* out,
                                    const int* H, const int* W, int B, int factor, float mask_scale, void* stream) {
  clear_error();
  const char* fn = "usf_convex_upsample_pyramid_f32";
  if (!check_convex_pyr(fn, nlevel, H, W, B, factor)) return USF_EINVAL;
  if (!flow || !mask || !out) {
    set_error("%s: null pointer array", fn);
    return USF_EINVAL;
  }
  for (int l = 0; l < nlevel; ++l)
    if (!flow[l] || !mask[l] || !out[l]) {
      set_error("%s: level %d: null pointer", fn, l);
      return USF_EINVAL;
    }
  if (!check_align_each(fn, "flow", (const void* const*)flow, nlevel, 16) ||
      !check_align_each(fn, "mask", (const void* const*)mask, nlevel, 16) ||
      !check_align_each(fn, "out", (const void* const*)out, nlevel, 16))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn, convex_pyr_fwd_launch(nlevel, flow, mask, out, H, W, B, factor, mask_scale, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_convex_upsample_pyramid_bwd_f32(int nlevel, const float* const* flow, const float* const* mask,
                                        const float* const* grad_out, float* const* grad_flow,
                                        float* const* grad_mask, float* scratch, long long scratch_floats,
                                        const int* H, const int* W, int B, int factor, float mask_scale,
                                        void* stream) {
  clear_error();
  const char* fn = "usf_convex_upsample_pyramid_bwd_f32";
  if (!check_convex_pyr(fn, nlevel, H, W, B, factor)) return USF_EINVAL;
  if (!flow || !mask || !grad_out) {
    set_error("%s: null input pointer array", fn);
    return USF_EINVAL;
  }
  for (int l = 0; l < nlevel; ++l)
    if (!flow[l] || !mask[l] || !grad_out[l] || (grad_flow && !grad_flow[l]) || (grad_mask && !grad_mask[l])) {
      set_error("%s: level %d: null pointer", fn, l);
      return USF_EINVAL;
    }
  if (grad_flow && (!scratch || scratch_floats < usf_convex_upsample_pyramid_bwd_scratch(nlevel, H, W, B))) {
    set_error("%s: grad_flow needs scratch of usf_convex_upsample_pyramid_bwd_scratch floats", fn);
    return USF_EINVAL;
  }
  if (!grad_flow && !grad_mask) return 0;
  if (!check_align_each(fn, "flow", (const void* const*)flow, nlevel, 16) ||
      !check_align_each(fn, "mask", (const void* const*)mask, nlevel, 16) ||
      !check_align_each(fn, "grad_out", (const void* const*)grad_out, nlevel, 16) ||
      !check_align_each(fn, "grad_flow", (const void* const*)grad_flow, nlevel, 16) ||
      !check_align_each(fn, "grad_mask", (const void* const*)grad_mask, nlevel, 16) ||
      !check_align(fn, {{"scratch", grad_flow ? scratch : nullptr, 16}}))
    return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                convex_pyr_bwd_launch(nlevel, flow, mask, grad_out, grad_flow, grad_mask, scratch, H, W, B, factor,
                                      mask_scale, (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_area_pyramid_f32(const float* x, float* out1, float* out2, float* out3, int B, int C, int H,
                         int W, void* stream) {
  clear_error();
  const char* fn = "usf_area_pyramid_f32";
  if (!check_dims(fn, B, C, H, W)) return USF_EINVAL;
  if (H % 8 != 0 || W % 8 != 0) {
    set_error("%s: H=%d and W=%d must be multiples of 8", fn, H, W);
    return USF_EINVAL;
  }
  if (!x || !out1 || !out2 || !out3) {
    set_error("%s: null pointer", fn);
    return USF_EINVAL;
  }
  if (!check_align(fn, {{"x", x, 16}, {"out1", out1, 16}, {"out2", out2, 16}, {"out3", out3, 16}})) return USF_EINVAL;
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn, area_pyramid_launch(x, out1, out2, out3, (long long)B * C, H, W, (hipStream_t)stream),
                (hipStream_t)stream);
}

// ------------------------------------------------ unsamflow_hip_convepi.h --
int usf_convepi_api_version(void) { return USF_CONVEPI_API_VERSION; }

static bool check_convepi(const char* fn, int B, int C, int H, int W, float slope) {
  if (!check_dims(fn, B, C, H, W)) return false;
  if (!(slope > 0.f)) {  // the sign of y is the sign of the pre-activation only then
    set_error("%s: slope=%g (must be > 0)", fn, (double)slope);
    return false;
  }
  return true;
}

int usf_convepi_fwd_f32(float* y, const float* bias, int B, int C, int H, int W, float slope, void* stream) {
  clear_error();
  const char* fn = "usf_convepi_fwd_f32";
  if (!check_convepi(fn, B, C, H, W, slope)) return USF_EINVAL;
  if (!y || !bias) {
    set_error("%s: null pointer", fn);
    return USF_EINVAL;
  }
  if ((uintptr_t)y % 16 != 0 || (uintptr_t)bias % 4 != 0) {
    set_error("%s: y must be 16-byte and bias 4-byte aligned", fn);
    return USF_EINVAL;
  }
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn, convepi_fwd_launch(y, bias, B, C, H, W, slope, (hipStream_t)stream), (hipStream_t)stream);
}

long long usf_convepi_bwd_workspace(int B, int C, int H, int W) {
  return (B > 0 && C > 0 && H > 0 && W > 0) ? convepi_bwd_workspace(B, C, H, W) : -1;
}

int usf_convepi_bwd_f32(const float* grad_out, long long gout_bstride, const float* y, float* grad_in,
                        float* grad_bias, float* workspace, long long workspace_floats, int B, int C, int H, int W,
                        float slope, void* stream) {
  clear_error();
  const char* fn = "usf_convepi_bwd_f32";
  if (!check_convepi(fn, B, C, H, W, slope)) return USF_EINVAL;
  const long long need = convepi_bwd_workspace(B, C, H, W);
  if (need < 0) {
    set_error("%s: shape B=%d C=%d H=%d W=%d too large for the bias-gradient split", fn, B, C, H, W);
    return USF_EINVAL;
  }
  const bool act = slope != 1.f;
  if (!grad_out || (uintptr_t)grad_out % 4 != 0 || gout_bstride < (long long)C * H * W) {
    set_error("%s: grad_out null or misaligned, or gout_bstride=%lld < C*H*W", fn, gout_bstride);
    return USF_EINVAL;
  }
  if (act ? (!y || !grad_in || (uintptr_t)y % 16 != 0 || (uintptr_t)grad_in % 16 != 0) : (y || grad_in)) {
    set_error("%s: y and grad_in must be 16-byte aligned tensors with an activation, NULL without (slope=%g)", fn,
              (double)slope);
    return USF_EINVAL;
  }
  if (!grad_bias && !act) {
    set_error("%s: nothing to compute (no activation and no grad_bias)", fn);
    return USF_EINVAL;
  }
  if (grad_bias && ((uintptr_t)grad_bias % 4 != 0 ||
                    (need > 0 && (!workspace || workspace_floats < need || (uintptr_t)workspace % 4 != 0)))) {
    set_error("%s: grad_bias misaligned, or workspace of %lld floats null, misaligned or short (%lld given)", fn,
              need, workspace_floats);
    return USF_EINVAL;
  }
  if (const int pe = pre_check(fn, (hipStream_t)stream)) return pe;
  return finish(fn,
                convepi_bwd_launch(grad_out, gout_bstride, y, grad_in, grad_bias, workspace, B, C, H, W, slope,
                                   (hipStream_t)stream),
                (hipStream_t)stream);
}

int usf_stream_copy_f32(const float* src, float* dst, long long n, void* stream) {
  clear_error();
  if (!src || !dst || n <= 0 || n % 4 != 0 || (reinterpret_cast<uintptr_t>(src) & 15) ||
      (reinterpret_cast<uintptr_t>(dst) & 15)) {
    set_error("usf_stream_copy_f32: need 16-byte aligned pointers and n %% 4 == 0 (n=%lld)", n);
    return USF_EINVAL;
  }
  if (const int pe = pre_check("usf_stream_copy_f32", (hipStream_t)stream)) return pe;
  return finish("usf_stream_copy_f32", stream_copy_launch(src, dst, n, (hipStream_t)stream), (hipStream_t)stream);
}

int usf_device_errors(void* stream, int clear) {
  clear_error();
  const int v = device_errors((hipStream_t)stream, clear != 0);
  if (v < 0) set_error("usf_device_errors: stream sync or flag read failed");
  return v;
}

int usf_set_variant(int op, int index) {
  clear_error();
  if (op < 0 || op > 3 || index < -1 || index >= variant_count(op)) {
    set_error("usf_set_variant: bad op %d / index %d", op, index);
    return USF_EINVAL;
  }
  set_variant_override(op, index);
  return variant_count(op);
}

}  // extern "C"
