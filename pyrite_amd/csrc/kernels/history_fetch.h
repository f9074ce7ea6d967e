// history_fetch.h -- the history fetch of the accumulation over frames (include/pyrite_gpu.h "motion records and accumulation over
// frames"), stated once for the two kernels that must fetch the same bits: reproject_kernel
// (kernels/reproject.hip) and temporal_kernel (kernels/temporal.hip). The header spells the f32 operations and their order out; the
// function keeps both. The independent statements it is held against are the tests' (tests/motion_restatement.py,
// tests/temporal_restatement.py).
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/pyrite_gpu.h"

namespace pyr {

// What the up to four bilinear taps around a pixel's previous position gave: the summed weight of the taps kept, their weighted
// colours, their weighted frame counts. weight == 0.0f: no history for this pixel.
struct HistoryFetch {
    float weight, sum[3], frames;
};

// `lo` is the first half of the pixel's record (prev_x, prev_y, prev_depth, depth), `shape` and `flags` come from the second. No tap is
// read unless `start` holds, there is a history and the record says the surface was in front of the previous camera at a finite place.
__device__ inline HistoryFetch fetch_history(const float* history, const PyrMotionPixel* history_motion, const float* history_count, uint32_t image_width,
                                             uint32_t image_height, float depth_tolerance, float4 lo, uint32_t shape, uint32_t flags, bool start) {
    HistoryFetch f = {0.0f, {0.0f, 0.0f, 0.0f}, 0.0f};
    if (!(start && history != nullptr && (flags & PYR_MOTION_IN_FRONT) != 0u && isfinite(lo.x) && isfinite(lo.y))) return f;
    const float width = (float)image_width, height = (float)image_height;
    const float gx = lo.x - 0.5f, gy = lo.y - 0.5f;
    const float x0 = floorf(gx), y0 = floorf(gy);
    const float fx = gx - x0, fy = gy - y0;
    const float tap_x[4] = {x0, x0 + 1.0f, x0, x0 + 1.0f}, tap_y[4] = {y0, y0, y0 + 1.0f, y0 + 1.0f};
    const float tap_w[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
    for (int k = 0; k < 4; ++k) {
        if (!(tap_x[k] >= 0.0f && tap_x[k] < width && tap_y[k] >= 0.0f && tap_y[k] < height)) continue; // in float: 1e30 never reaches a cast
        const uint32_t tx = (uint32_t)tap_x[k], ty = (uint32_t)tap_y[k];
        if (tx >= image_width || ty >= image_height) continue; // (float)width rounds up beyond 2^24: never an address outside the image
        const size_t tap = (size_t)ty * image_width + tx;
        const float4* theirs = reinterpret_cast<const float4*>(history_motion + tap);
        if (__float_as_uint(theirs[1].x) != shape) continue;
        if ((flags & PYR_MOTION_HIT) != 0u) {
            const float their_depth = theirs[0].w;
            if (!(fabsf(their_depth - lo.z) <= depth_tolerance * fmaxf(their_depth, lo.z))) continue;
        }
        const float count = history_count[tap];
        if (!(count > 0.0f)) continue;
        const float h[3] = {history[3 * tap], history[3 * tap + 1], history[3 * tap + 2]};
        if (!(isfinite(h[0]) && isfinite(h[1]) && isfinite(h[2]))) continue;
        const float w = tap_w[k];
        f.weight = f.weight + w;
        for (int c = 0; c < 3; ++c) f.sum[c] = f.sum[c] + w * h[c];
        f.frames = f.frames + w * count;
    }
    return f;
}

} // namespace pyr
