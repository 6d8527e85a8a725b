// frames_byte.h — a float32 frame value to a byte, shared by every kernel that writes frames as bytes (frames.hip: vpx_frames_postprocess;
// vis.hip: vpx_vis_compose), so that a visualization shows exactly the bytes postprocess() returns. In float32, each step rounded on its own:
//   v = ((x - lo) / scale) * 255.0f with scale = float(hi - lo) (formed by the host), clamped to [0, 255], truncated toward zero; NaN gives 0.
#pragma once
#include <hip/hip_runtime.h>

// Every operation is rounded on its own: no a * b + c becomes a fused multiply-add (the includers ask for the same).
#pragma clang fp contract(off)

namespace vpx {

__device__ __forceinline__ unsigned fr_byte(float lo, float scale, float x) {
    float v = x - lo;
    v = v / scale;
    v = v * 255.0f;
    if (!(v == v)) return 0u;                                          // NaN: 0 by definition (the reference's conversion is undefined)
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    return (unsigned)v;                                                // truncation toward zero
}

}  // namespace vpx
