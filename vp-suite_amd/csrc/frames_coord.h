// frames_coord.h — the source coordinate of a bilinear resize (align_corners = False, no antialiasing), shared by every kernel that
// resizes frames (frames.hip: stored sequences to a batch; adapt.hip: planar float frames between a model and a test set), so that the
// resizes cannot drift apart. Per axis, in float32 (ATen's area_pixel_compute_source_index):
//   s = float(in) / float(out) (formed by the host);  src = max(s * (d + 0.5f) - 0.5f, 0);  i0 = int(src);  i1 = min(i0 + 1, in - 1);  l = src - i0.
#pragma once
#include <hip/hip_runtime.h>

// Every operation is rounded on its own: no a * b + c becomes a fused multiply-add (the includers ask for the same).
#pragma clang fp contract(off)

namespace vpx {

// The first tap, the second one and the weight of the second. i0 is clamped to the box for memory safety only: src < in holds for every d < out.
__device__ __forceinline__ void fr_coord(float s, int d, int in, int& i0, int& i1, float& l) {
    float src = s * ((float)d + 0.5f) - 0.5f;
    src = src < 0.0f ? 0.0f : src;
    i0 = (int)src;
    i0 = i0 > in - 1 ? in - 1 : i0;
    i1 = i0 + 1 > in - 1 ? in - 1 : i0 + 1;
    l = src - (float)i0;
}

}  // namespace vpx
