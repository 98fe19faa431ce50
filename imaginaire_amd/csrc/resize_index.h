// Source-index rules of the resizes, shared by the k12 resize kernels (resize.hip) and the k19
// label expansion (label.hip), which reads its index maps through the same nearest rule: one
// definition, so "expand, then resize" and "resize while expanding" cannot drift apart.
#pragma once

#include "common.h"

namespace iamd {

// One spatial axis of a resize: sizes, PyTorch's source scale (in / out or 1 / scale_factor,
// as the caller computed it) and align_corners.
struct Axis {
  int in, out;
  float scale;
  bool ac;
};

inline Axis make_axis(int64_t in, int64_t out, double scale, bool ac) {
  Axis a;
  a.in = (int)in;
  a.out = (int)out;
  a.scale = (float)scale;
  a.ac = ac;
  return a;
}

// ---- nearest (PyTorch's nearest_idx: exact 2x -> o >> 1, same size -> o, otherwise
// min(floor(o * scale), in - 1) in float) --------------------------------------------------
__device__ __forceinline__ int nearest_src(const Axis& a, int o) {
  if (a.out == a.in) return o;
  if (a.out == 2 * a.in) return o >> 1;
  return min((int)floorf((float)o * a.scale), a.in - 1);
}

}  // namespace iamd
