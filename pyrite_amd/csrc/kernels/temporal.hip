// temporal.hip -- the temporal resolve (include/pyrite_gpu.h "temporal resolve"), a unit of its own: the
// header spells the f32 operations and their order out, the kernel keeps both. The history fetch is the one reproject_kernel
// calls (kernels/history_fetch.h): where nothing is clipped the two kernels write the same bits because they run the same
// function, started here only for a usable pixel. What is new is the neighbourhood of `current`, (2*radius+1)^2 pixels read twice
// by every pixel, and that is staged: a workgroup owns a 16 x 16 tile and loads it with its
// radius-wide ring once into LDS, one 16-byte slot a pixel -- the three floats and the usable flag, decided at load time -- and a
// second slot array for |noise| in the build that reads one. Both walks run from LDS.
//   Layout. A wave is a strip of 4 rows x 16 pixels: the lanes of a row read consecutive slots, and a tile row is kPitch = 32
// slots = 512 B, twice the 256-B bank row. ds_read_b128 serves 16 lanes at a time, 8 from one row of the strip and 8 from the
// next, at columns 0..3, 12..15 and 4..11 (or the complement): with a pitch that is a multiple of 16 slots they fall on 16
// different slots of the bank row whatever (dx, dy) is. An 8 x 8 square would put columns 0..7 of two rows into one group, and the
// unpadded pitch of 16 + 2*radius slots puts two of a group's lanes on one slot at every radius.
//   A slot that is not kept (outside the image, or not usable) holds zeros and the flag 0.0f: the first walk adds it like any
// other -- a sum that starts from +0.0f is never -0.0f, so adding +0.0f changes no bit -- and k is the sum of the flags. The
// second walk selects on the flag, since 0 - mean need not be 0. The radius is a loop bound, uniform over the launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../api_internal.h"
#include "../device_scene.h"
#include "history_fetch.h"

namespace pyr {

namespace {
constexpr uint32_t kTile = 16;                                  // pixels a side; 256 lanes, four waves
constexpr uint32_t kRows = kTile + 2 * PYR_TEMPORAL_MOST_RADIUS; // 22: the tile and its ring at the largest radius
constexpr uint32_t kPitch = 32;                                 // slots a tile row: >= kRows and a multiple of 16 (above)
constexpr uint32_t kMostBlocks = 256 * 32;                      // one tile a workgroup up to 1920 x 1080
static_assert(kPitch >= kRows && kPitch % 16 == 0, "the LDS rows hold the ring and keep the bank argument");
} // namespace

// One slot in one ds_read_b128. A plain float4 read is taken apart by the optimiser where the flag and the colour are used apart --
// into ds_read_b96 + ds_read_b32 or four ds_read_b32 -- and a 4-byte read of every fourth dword is a 4-way bank conflict on this
// layout; a volatile read is left whole.
__device__ inline float4 read_slot(const float4* slot) {
    typedef float vec4 __attribute__((ext_vector_type(4)));
    const vec4 v = *(const volatile __attribute__((address_space(3))) vec4*)slot; // named as LDS: a volatile read is not moved there from the flat space
    return make_float4(v.x, v.y, v.z, v.w);
}

template <bool NOISE>
__global__ __launch_bounds__(kTile* kTile) void temporal_kernel(TemporalLaunch L) {
    __shared__ float4 tile[kRows * kPitch];
    __shared__ float4 tile_noise[NOISE ? kRows * kPitch : 1];
    const uint32_t tiles_x = (L.width - 1) / kTile + 1, tiles_y = (L.height - 1) / kTile + 1; // width * height < 2^32: so is the product
    const uint32_t tiles = tiles_x * tiles_y;
    const uint32_t radius = L.radius, span = kTile + 2 * radius, side = 2 * radius + 1;
    const uint32_t lx = threadIdx.x % kTile, ly = threadIdx.x / kTile;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t tile_y = t / tiles_x, tile_x = t - tile_y * tiles_x;
        const int64_t x_first = (int64_t)tile_x * kTile - radius, y_first = (int64_t)tile_y * kTile - radius;
        for (uint32_t i = threadIdx.x; i < span * span; i += kTile * kTile) {
            const uint32_t row = i / span, col = i - row * span;
            const int64_t qx = x_first + col, qy = y_first + row;
            float4 slot = make_float4(0.0f, 0.0f, 0.0f, 0.0f), slot_noise = slot;
            if (qx >= 0 && qx < (int64_t)L.width && qy >= 0 && qy < (int64_t)L.height) {
                const size_t q = (size_t)qy * L.width + (size_t)qx;
                const float c0 = L.current[3 * q], c1 = L.current[3 * q + 1], c2 = L.current[3 * q + 2];
                bool usable = isfinite(c0) && isfinite(c1) && isfinite(c2);
                if (NOISE) {
                    const float n0 = L.noise[3 * q], n1 = L.noise[3 * q + 1], n2 = L.noise[3 * q + 2];
                    usable = usable && isfinite(n0) && isfinite(n1) && isfinite(n2);
                    if (usable) slot_noise = make_float4(fabsf(n0), fabsf(n1), fabsf(n2), 0.0f);
                }
                if (usable) slot = make_float4(c0, c1, c2, 1.0f);
            }
            tile[row * kPitch + col] = slot;
            if (NOISE) tile_noise[row * kPitch + col] = slot_noise;
        }
        __syncthreads();
        const uint32_t x = tile_x * kTile + lx, y = tile_y * kTile + ly;
        if (x < L.width && y < L.height) {
            const size_t px = (size_t)y * L.width + x;
            const float4 own = tile[(ly + radius) * kPitch + lx + radius];
            const float4* record = reinterpret_cast<const float4*>(L.motion + px);
            const float4 lo = record[0], hi = record[1]; // prev_x, prev_y, prev_depth, depth; shape, flags
            const uint32_t shape = __float_as_uint(hi.x), flags = __float_as_uint(hi.y);
            const HistoryFetch f = fetch_history(L.history, L.history_motion, L.history_count, L.width, L.height, L.depth_tolerance, lo, shape, flags, own.w != 0.0f);
            if (f.weight > 0.0f) { // usable, and a history to clip: only these pixels walk the neighbourhood
                const float current[3] = {own.x, own.y, own.z};
                float total[3] = {0.0f, 0.0f, 0.0f}, total_noise[3] = {0.0f, 0.0f, 0.0f}, kept = 0.0f;
                for (uint32_t dy = 0; dy < side; ++dy)
                    for (uint32_t dx = 0; dx < side; ++dx) {
                        const uint32_t at = (ly + dy) * kPitch + lx + dx;
                        const float4 q = read_slot(&tile[at]);
                        total[0] = total[0] + q.x, total[1] = total[1] + q.y, total[2] = total[2] + q.z;
                        kept = kept + q.w;
                        if (NOISE) {
                            const float4 n = read_slot(&tile_noise[at]);
                            total_noise[0] = total_noise[0] + n.x, total_noise[1] = total_noise[1] + n.y, total_noise[2] = total_noise[2] + n.z;
                        }
                    }
                const float mean[3] = {total[0] / kept, total[1] / kept, total[2] / kept};
                float squares[3] = {0.0f, 0.0f, 0.0f};
                for (uint32_t dy = 0; dy < side; ++dy)
                    for (uint32_t dx = 0; dx < side; ++dx) {
                        const float4 q = read_slot(&tile[(ly + dy) * kPitch + lx + dx]);
                        const float d0 = q.x - mean[0], d1 = q.y - mean[1], d2 = q.z - mean[2];
                        const bool keep = q.w != 0.0f; // selects, not a branch: a branch on the flag splits the slot's read into 4 + 12 bytes
                        squares[0] = keep ? squares[0] + d0 * d0 : squares[0];
                        squares[1] = keep ? squares[1] + d1 * d1 : squares[1];
                        squares[2] = keep ? squares[2] + d2 * d2 : squares[2];
                    }
                const float n = fminf(f.frames / f.weight, L.max_history);
                float clipped[3], r = 0.0f;
                for (int c = 0; c < 3; ++c) {
                    const float sigma = sqrtf(squares[c] / kept);
                    const float nbar = NOISE ? total_noise[c] / kept : 0.0f;
                    const float e = L.gamma * sigma + L.noise_scale * nbar;
                    const float low = mean[c] - e, high = mean[c] + e;
                    const float H = f.sum[c] / f.weight;
                    clipped[c] = fminf(fmaxf(H, low), high);
                    const float q = fabsf(H - clipped[c]) / fmaxf(e, 1e-30f);
                    r = c == 0 ? q : fmaxf(r, q);
                }
                r = fminf(r, 1e30f);
                const float n2 = n / (1.0f + L.response * r);
                for (int c = 0; c < 3; ++c) L.out[3 * px + c] = clipped[c] + (current[c] - clipped[c]) / (n2 + 1.0f);
                L.count_out[px] = n2 + 1.0f;
                if (L.clip_out != nullptr) L.clip_out[px] = r;
            } else { // not usable, or no history: the pixel's own bits, which the tile holds only of a usable pixel
                for (int c = 0; c < 3; ++c) L.out[3 * px + c] = L.current[3 * px + c];
                L.count_out[px] = 1.0f;
                if (L.clip_out != nullptr) L.clip_out[px] = 0.0f;
            }
        }
        __syncthreads(); // before the next tile overwrites this one
    }
}

int launch_temporal(const TemporalLaunch& launch, void* stream) {
    if (launch.width == 0 || launch.height == 0) return PYR_OK;
    if (launch.radius < 1 || launch.radius > PYR_TEMPORAL_MOST_RADIUS) return fail(PYR_ERR_INVALID_ARGUMENT, "temporal resolve: radius must be 1..3"); // the LDS tile holds no wider ring
    const uint64_t tiles = (uint64_t)((launch.width - 1) / kTile + 1) * ((launch.height - 1) / kTile + 1);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(tiles, kMostBlocks);
    if (launch.noise != nullptr)
        hipLaunchKernelGGL(temporal_kernel<true>, dim3(grid), dim3(kTile * kTile), 0, (hipStream_t)stream, launch);
    else
        hipLaunchKernelGGL(temporal_kernel<false>, dim3(grid), dim3(kTile * kTile), 0, (hipStream_t)stream, launch);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("temporal kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

} // namespace pyr
