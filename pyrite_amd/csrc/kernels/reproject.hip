// reproject.hip -- accumulation over frames (include/pyrite_gpu.h "motion records and accumulation over frames", DESIGN.md section
// 9i), a unit of its own: the header spells the f32 operations and their order out, the kernel keeps both. One thread per pixel: it
// reads 12 B of the current image and its 32 B record, at most four history taps of 12 + 32 + 4 B each through the cache, and
// writes 16 B -- bound by bytes, nothing to stage. Nothing here touches the render, film, feature or motion kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../api_internal.h"
#include "../device_scene.h"

namespace pyr {

namespace {
constexpr uint32_t PIXEL_BLOCK = 256;
}

__global__ __launch_bounds__(PIXEL_BLOCK) void reproject_kernel(ReprojectLaunch L) {
    const size_t pixels = (size_t)L.width * L.height;
    const float width = (float)L.width, height = (float)L.height;
    for (size_t px = (size_t)blockIdx.x * PIXEL_BLOCK + threadIdx.x; px < pixels; px += (size_t)gridDim.x * PIXEL_BLOCK) {
        const float current[3] = {L.current[3 * px], L.current[3 * px + 1], L.current[3 * px + 2]};
        const float4* record = reinterpret_cast<const float4*>(L.motion + px);
        const float4 lo = record[0], hi = record[1]; // prev_x, prev_y, prev_depth, depth; shape, flags
        const uint32_t shape = __float_as_uint(hi.x), flags = __float_as_uint(hi.y);
        float weight = 0.0f, sum[3] = {0.0f, 0.0f, 0.0f}, frames = 0.0f;
        if (L.history != nullptr && (flags & PYR_MOTION_IN_FRONT) != 0u && isfinite(lo.x) && isfinite(lo.y)) {
            const float gx = lo.x - 0.5f, gy = lo.y - 0.5f;
            const float x0 = floorf(gx), y0 = floorf(gy);
            const float fx = gx - x0, fy = gy - y0;
            const float tap_x[4] = {x0, x0 + 1.0f, x0, x0 + 1.0f}, tap_y[4] = {y0, y0, y0 + 1.0f, y0 + 1.0f};
            const float tap_w[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
            for (int k = 0; k < 4; ++k) {
                if (!(tap_x[k] >= 0.0f && tap_x[k] < width && tap_y[k] >= 0.0f && tap_y[k] < height)) continue; // in float: 1e30 never reaches a cast
                const uint32_t tx = (uint32_t)tap_x[k], ty = (uint32_t)tap_y[k];
                if (tx >= L.width || ty >= L.height) continue; // (float)width rounds up beyond 2^24: never an address outside the image
                const size_t tap = (size_t)ty * L.width + tx;
                const float4* theirs = reinterpret_cast<const float4*>(L.history_motion + tap);
                if (__float_as_uint(theirs[1].x) != shape) continue;
                if ((flags & PYR_MOTION_HIT) != 0u) {
                    const float their_depth = theirs[0].w;
                    if (!(fabsf(their_depth - lo.z) <= L.depth_tolerance * fmaxf(their_depth, lo.z))) continue;
                }
                const float count = L.history_count[tap];
                if (!(count > 0.0f)) continue;
                const float h[3] = {L.history[3 * tap], L.history[3 * tap + 1], L.history[3 * tap + 2]};
                if (!(isfinite(h[0]) && isfinite(h[1]) && isfinite(h[2]))) continue;
                const float w = tap_w[k];
                weight = weight + w;
                for (int c = 0; c < 3; ++c) sum[c] = sum[c] + w * h[c];
                frames = frames + w * count;
            }
        }
        if (weight > 0.0f) {
            const float n = fminf(frames / weight, L.max_history);
            for (int c = 0; c < 3; ++c) {
                const float mean = sum[c] / weight;
                L.out[3 * px + c] = mean + (current[c] - mean) / (n + 1.0f);
            }
            L.count_out[px] = n + 1.0f;
        } else {
            for (int c = 0; c < 3; ++c) L.out[3 * px + c] = current[c];
            L.count_out[px] = 1.0f;
        }
    }
}

int launch_reproject(const ReprojectLaunch& launch, void* stream) {
    const size_t pixels = (size_t)launch.width * launch.height;
    if (pixels == 0) return PYR_OK;
    const uint32_t grid = (uint32_t)std::min<size_t>((pixels + PIXEL_BLOCK - 1) / PIXEL_BLOCK, 256 * 16);
    hipLaunchKernelGGL(reproject_kernel, dim3(grid), dim3(PIXEL_BLOCK), 0, (hipStream_t)stream, launch);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("reproject kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

} // namespace pyr
