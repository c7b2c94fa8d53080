// oss_metric_load.h -- how the metric kernels (oss_metrics.hip, oss_niqe.hip) turn an element of a network tensor into the pixel
// the reference's metric functions see: tensor2img's quantisation and to_y_channel's BT.601 luma, both applied on load.
#pragma once
#include "oss_device.h"

namespace oss {

template <bool QUANT> __device__ __forceinline__ float metric_units(float v) {
    if (QUANT) {
        v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
        v = __builtin_rintf(v * 255.0f);   // v_rndne_f32: half to even, torch.round
    }
    return v;
}

// metrics.to_y_channel on one pixel in [0, 255] units: the row of bgr2ycbcr's y_only branch, three rounded products and two sums.
// Any association is the reference's to a unit of fp64 round-off; this one -- (B + R) + G, the even-indexed terms of the B, G, R
// row first -- is the one torch's CPU matrix-vector product evaluates for the restatement, so that the fp32 cast that follows
// rounds the very same fp64 number (checked bit for bit on 2 million pixels).
__device__ __forceinline__ float metric_luma(float r, float g, float b) {
#pragma clang fp contract(off)
    const float rf = r / 255.0f, gf = g / 255.0f, bf = b / 255.0f;
    double y = (double)bf * 24.966 + (double)rf * 65.481;
    y = y + (double)gf * 128.553;
    y = (y + 16.0) / 255.0;
    return (float)y * 255.0f;
}

template <typename T, bool QUANT, bool LUMA>
__device__ __forceinline__ float metric_pixel(const T *p, int64_t cs) {
    if (LUMA)
        return metric_luma(metric_units<QUANT>(to_f32(p[0])), metric_units<QUANT>(to_f32(p[cs])), metric_units<QUANT>(to_f32(p[2 * cs])));
    return metric_units<QUANT>(to_f32(p[0]));
}

}  // namespace oss
