// reproject.hip -- accumulation over frames (include/pyrite_gpu.h "motion records and accumulation over frames", DESIGN.md section
// 9i), a unit of its own: the header spells the f32 operations and their order out, the kernel keeps both. One thread per pixel: it
// reads 12 B of the current image and its 32 B record, at most four history taps of 12 + 32 + 4 B each through the cache (the fetch:
// kernels/history_fetch.h, which the temporal resolve calls too), and writes 16 B -- bound by bytes, nothing to stage. Nothing here
// touches the render, film, feature or motion kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../api_internal.h"
#include "../device_scene.h"
#include "history_fetch.h"

namespace pyr {

namespace {
constexpr uint32_t PIXEL_BLOCK = 256;
}

__global__ __launch_bounds__(PIXEL_BLOCK) void reproject_kernel(ReprojectLaunch L) {
    const size_t pixels = (size_t)L.width * L.height;
    for (size_t px = (size_t)blockIdx.x * PIXEL_BLOCK + threadIdx.x; px < pixels; px += (size_t)gridDim.x * PIXEL_BLOCK) {
        const float current[3] = {L.current[3 * px], L.current[3 * px + 1], L.current[3 * px + 2]};
        const float4* record = reinterpret_cast<const float4*>(L.motion + px);
        const float4 lo = record[0], hi = record[1]; // prev_x, prev_y, prev_depth, depth; shape, flags
        const uint32_t shape = __float_as_uint(hi.x), flags = __float_as_uint(hi.y);
        const HistoryFetch f = fetch_history(L.history, L.history_motion, L.history_count, L.width, L.height, L.depth_tolerance, lo, shape, flags, true);
        if (f.weight > 0.0f) {
            const float n = fminf(f.frames / f.weight, L.max_history);
            for (int c = 0; c < 3; ++c) {
                const float mean = f.sum[c] / f.weight;
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
