// oss_pixel_stage.h -- the two per-pixel stages of MambaRealSR.feed_data that the degradation kernels (oss_degrade.hip, oss_jpeg.hip)
// carry as their first or last step: clamp to [0, 1] (:190, :235, :240) and the final quantisation (:248), with torch's bits.
#pragma once
#include <hip/hip_runtime.h>

namespace oss {

// torch divides a device tensor by a Python scalar as a multiplication by the scalar's reciprocal, formed in double and rounded to
// the tensor's type (BinaryDivTrueKernel.cu); ":248" on the device is therefore q * fp32(1 / 255), one unit in the last place from
// the true quotient at some of the 256 levels
constexpr float kInv255 = (float)(1.0 / 255.0);

// torch's clamp gives +0 for -0 and for everything below 0; the "+ 0.0f" makes that independent of the max instruction's operand
// order.  A NaN stays a NaN.
__host__ __device__ __forceinline__ float clamp_unit(float v) {
    return v != v ? v : fminf(fmaxf(v, 0.0f), 1.0f) + 0.0f;
}

// clamp(round(v * 255), 0, 255) / 255 with round-half-even
__host__ __device__ __forceinline__ float quantise_255(float v) {
#pragma clang fp contract(off)
    const float r = rintf(v * 255.0f);
    return (r != r ? r : fminf(fmaxf(r, 0.0f), 255.0f) + 0.0f) * kInv255;
}

}  // namespace oss
