// Coordinates of the reference's resize_flow (utils/flow_utils.py:62-71) to a
// per-sample target size, shared by the resize kernel and the fused evaluation
// (eval.hip) so both compute the same numbers: ATen's align_corners bilinear
// tap (interp_tap.h: scale (in - 1) / (out - 1) in fp32, weights from the floor
// of the source position, upper tap clamped), then u / (float)(w / W_b) and
// v / (float)(h / H_b): the quotient in fp64 as Python forms it, the division in
// fp32 as ATen's CPU kernel does it (not a multiplication by the inverse).
#pragma once
#include "interp_tap.h"

namespace usf {

struct ResizeGeom {
  float sy, sx;      // source scale per axis
  float div_u, div_v;  // what channel 0 / channel 1 are divided by
};

__device__ __forceinline__ ResizeGeom resize_geom(int h, int w, int Hb, int Wb) {
  ResizeGeom g;
  g.sy = ac_scale(h, Hb);
  g.sx = ac_scale(w, Wb);
  g.div_u = (float)((double)w / (double)Wb);
  g.div_v = (float)((double)h / (double)Hb);
  return g;
}

// lin_tap with both taps held inside [0, in): the source of the last output
// index may round one ulp past in - 1
__device__ __forceinline__ Lin resize_tap(int dst, float scale, int in) {
  Lin t = lin_tap(dst, scale, in);
  t.i0 = min(t.i0, in - 1);
  t.i1 = min(t.i1, in - 1);
  return t;
}

// the resized (u, v) at taps (ty, tx) of one sample's prediction planes pu, pv ([h][w])
__device__ __forceinline__ void resize_sample(const float* __restrict__ pu, const float* __restrict__ pv, int w,
                                              const Lin& ty, const Lin& tx, const ResizeGeom& g, float& u, float& v) {
#pragma clang fp contract(off)
  u = up_bilinear(pu, w, ty, tx, 1.f) / g.div_u;
  v = up_bilinear(pv, w, ty, tx, 1.f) / g.div_v;
}

}  // namespace usf
