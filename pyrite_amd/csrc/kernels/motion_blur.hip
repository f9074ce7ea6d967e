// motion_blur.hip -- motion blur as a post filter over the motion records (include/pyrite_gpu.h "motion blur over the motion
// records"), a unit of its own: the header spells the f32 operations and their order out, the kernels keep
// both. Three launches on one stream, each reading what the one before wrote:
//   velocity_kernel   one workgroup per tile of max_radius x max_radius pixels: the 32-byte record of a pixel becomes the 16 bytes
//                     (hx, hy, len, z) a tap reads, and the tile's maximum is reduced on the 64-bit key (len, ~pixel index) --
//                     across a wave by shuffles, across the workgroup's waves through LDS -- so the tie rule survives the reduction;
//   neighbour_kernel  one thread per tile: the largest of the up to nine tile maxima around it, on the key (len, ~tile index);
//   gather_kernel     one thread per pixel, a workgroup 16 x 16 pixels, each of its four waves an 8 x 8 square, so the taps of
//                     neighbouring lanes fall on shared cache lines. A pixel whose neighbour maximum is below half a pixel copies;
//                     where max_radius is a multiple of 16 that decision is uniform over the workgroup.
// Bound by bytes: nothing is staged. Nothing here touches the render, film, feature, motion or reprojection kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>

#include "../api_internal.h"
#include "../device_scene.h"

namespace pyr {

namespace {

constexpr uint32_t VELOCITY_BLOCK = 256; // four waves: a 16 x 16 tile is one pixel a lane
constexpr uint32_t VELOCITY_WAVES = VELOCITY_BLOCK / 64;
constexpr uint32_t TILE_BLOCK = 64;
constexpr uint32_t GATHER_EDGE = 16, GATHER_BLOCK = GATHER_EDGE * GATHER_EDGE;
constexpr uint32_t MAX_GRID = 1u << 20;

struct BlurGeometry {
    uint32_t width, height, edge, tiles_x, tiles_y;
};

// Larger len first, then the smaller index: len is never negative, so its bits order as it does.
__device__ inline unsigned long long reduce_key(float len, uint32_t index) { return ((unsigned long long)__float_as_uint(len) << 32) | (0xFFFFFFFFu - index); }

__device__ inline unsigned long long wave_max(unsigned long long v) {
    for (int offset = 32; offset > 0; offset >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, offset), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), offset);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        v = other > v ? other : v;
    }
    return v;
}

__device__ inline float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ inline float front_of(float a, float b, float e) { return clamp01(1.0f - (a - b) / e); }
__device__ inline float cone(float d, float l) { return clamp01(1.0f - d / l); }
__device__ inline float cylinder(float d, float l) {
    const float lo = 0.95f * l, hi = 1.05f * l;
    const float u = clamp01((d - lo) / (hi - lo));
    return 1.0f - (u * u) * (3.0f - 2.0f * u);
}

} // namespace

__global__ __launch_bounds__(VELOCITY_BLOCK) void motion_blur_velocity_kernel(const PyrMotionPixel* motion, BlurGeometry G, float half_shutter, float radius, float4* velocity,
                                                                              float4* tile_max) {
    __shared__ unsigned long long wave_best[VELOCITY_WAVES];
    const uint32_t tiles = G.tiles_x * G.tiles_y;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t x_begin = (tile % G.tiles_x) * G.edge, y_begin = (tile / G.tiles_x) * G.edge;
        const uint32_t cols = min(G.edge, G.width - x_begin), rows = min(G.edge, G.height - y_begin);
        unsigned long long best = 0; // below every pixel's key: no pixel has the index 2^32 - 1
        float best_x = 0.0f, best_y = 0.0f, best_len = 0.0f;
        for (uint32_t k = threadIdx.x; k < cols * rows; k += VELOCITY_BLOCK) { // row-major in the tile: ascending pixel indices
            const uint32_t x = x_begin + k % cols, y = y_begin + k / cols;
            const size_t px = (size_t)y * G.width + x;
            const float4* record = reinterpret_cast<const float4*>(motion + px);
            const float4 lo = record[0], hi = record[1]; // prev_x, prev_y, prev_depth, depth; shape, flags
            const uint32_t flags = __float_as_uint(hi.y);
            const float dx = ((float)x + 0.5f) - lo.x, dy = ((float)y + 0.5f) - lo.y;
            float hx = dx * half_shutter, hy = dy * half_shutter;
            float len = sqrtf(hx * hx + hy * hy);
            if ((flags & PYR_MOTION_IN_FRONT) == 0u || !isfinite(lo.x) || !isfinite(lo.y) || !isfinite(len)) {
                hx = hy = len = 0.0f;
            } else if (len > radius) {
                const float scale = radius / len;
                hx = hx * scale, hy = hy * scale, len = radius;
            }
            velocity[px] = make_float4(hx, hy, len, (flags & PYR_MOTION_HIT) != 0u ? lo.w : FLT_MAX);
            const unsigned long long key = reduce_key(len, (uint32_t)px);
            if (key > best) best = key, best_x = hx, best_y = hy, best_len = len;
        }
        const unsigned long long in_wave = wave_max(best);
        if ((threadIdx.x & 63u) == 0u) wave_best[threadIdx.x >> 6] = in_wave;
        __syncthreads();
        unsigned long long winner = wave_best[0];
        for (uint32_t w = 1; w < VELOCITY_WAVES; ++w) winner = wave_best[w] > winner ? wave_best[w] : winner;
        if (best == winner && best != 0) tile_max[tile] = make_float4(best_x, best_y, best_len, 0.0f); // keys hold the index: one lane has it
        __syncthreads(); // wave_best is written again for the next tile
    }
}

__global__ __launch_bounds__(TILE_BLOCK) void motion_blur_neighbour_kernel(const float4* tile_max, BlurGeometry G, float4* neighbour_max) {
    const uint32_t tiles = G.tiles_x * G.tiles_y;
    for (uint32_t tile = blockIdx.x * TILE_BLOCK + threadIdx.x; tile < tiles; tile += gridDim.x * TILE_BLOCK) {
        const uint32_t tx = tile % G.tiles_x, ty = tile / G.tiles_x;
        const uint32_t x0 = tx > 0 ? tx - 1 : 0, x1 = min(tx + 1, G.tiles_x - 1), y0 = ty > 0 ? ty - 1 : 0, y1 = min(ty + 1, G.tiles_y - 1);
        unsigned long long best = 0;
        float4 chosen = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (uint32_t y = y0; y <= y1; ++y)
            for (uint32_t x = x0; x <= x1; ++x) {
                const uint32_t other = y * G.tiles_x + x;
                const float4 m = tile_max[other];
                const unsigned long long key = reduce_key(m.z, other);
                if (key > best) best = key, chosen = m;
            }
        neighbour_max[tile] = chosen;
    }
}

__global__ __launch_bounds__(GATHER_BLOCK) void motion_blur_gather_kernel(MotionBlurLaunch L, BlurGeometry G, const float4* velocity, const float4* neighbour_max,
                                                                          uint32_t blocks_x, uint32_t blocks) {
    const float width = (float)L.width, height = (float)L.height;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t in_x = (wave & 1u) * 8u + (lane & 7u), in_y = (wave >> 1) * 8u + (lane >> 3); // four 8 x 8 squares
    for (uint32_t block = blockIdx.x; block < blocks; block += gridDim.x) {
        const uint32_t x = (block % blocks_x) * GATHER_EDGE + in_x, y = (block / blocks_x) * GATHER_EDGE + in_y;
        if (x >= L.width || y >= L.height) continue;
        const size_t px = (size_t)y * L.width + x;
        const float mine[3] = {L.image[3 * px], L.image[3 * px + 1], L.image[3 * px + 2]};
        const float4 n = neighbour_max[(y / G.edge) * G.tiles_x + x / G.edge];
        if (n.z < 0.5f || !(isfinite(mine[0]) && isfinite(mine[1]) && isfinite(mine[2]))) { // nothing moves near this pixel: its bits
            L.out[3 * px] = mine[0], L.out[3 * px + 1] = mine[1], L.out[3 * px + 2] = mine[2];
            continue;
        }
        const float4 vx = velocity[px];
        const float len_x = fmaxf(vx.z, 0.5f), z_x = vx.w;
        const float w0 = 1.0f / len_x;
        float weight = w0, sum[3] = {w0 * mine[0], w0 * mine[1], w0 * mine[2]};
        uint32_t k = (uint32_t)px + L.seed * 0x9E3779B1u;
        k ^= k >> 16, k *= 0x7FEB352Du, k ^= k >> 15, k *= 0x846CA68Bu, k ^= k >> 16;
        const float jitter = (float)(k >> 8) * 0x1p-24f - 0.5f;
        const float centre_x = (float)x + 0.5f, centre_y = (float)y + 0.5f, samples = (float)L.samples;
        for (uint32_t i = 0; i < L.samples; ++i) {
            const float t = ((((float)i + 0.5f) + jitter) / samples) * 2.0f - 1.0f;
            const float ox = n.x * t, oy = n.y * t;
            const float ax = floorf(centre_x + ox), ay = floorf(centre_y + oy);
            if (!(ax >= 0.0f && ax < width && ay >= 0.0f && ay < height)) continue; // in float: nothing unbounded reaches a cast
            const uint32_t tx = (uint32_t)ax, ty = (uint32_t)ay;
            if (tx >= L.width || ty >= L.height) continue; // (float)width rounds up beyond 2^24: never an address outside the image
            const size_t tap = (size_t)ty * L.width + tx;
            const float theirs[3] = {L.image[3 * tap], L.image[3 * tap + 1], L.image[3 * tap + 2]};
            if (!(isfinite(theirs[0]) && isfinite(theirs[1]) && isfinite(theirs[2]))) continue;
            const float4 vy = velocity[tap];
            const float dist = sqrtf(ox * ox + oy * oy), len_y = fmaxf(vy.z, 0.5f), z_y = vy.w;
            const float e = L.depth_softness * fmaxf(z_x, z_y);
            const float w = (front_of(z_y, z_x, e) * cone(dist, len_y) + front_of(z_x, z_y, e) * cone(dist, len_x)) + (cylinder(dist, len_y) * cylinder(dist, len_x)) * 2.0f;
            weight = weight + w;
            for (int c = 0; c < 3; ++c) sum[c] = sum[c] + w * theirs[c];
        }
        for (int c = 0; c < 3; ++c) L.out[3 * px + c] = sum[c] / weight;
    }
}

size_t motion_blur_work_bytes(uint32_t width, uint32_t height, uint32_t max_radius) {
    const size_t tiles = (size_t)((width + max_radius - 1) / max_radius) * ((height + max_radius - 1) / max_radius);
    return ((size_t)width * height + 2 * tiles) * sizeof(float4);
}

int launch_motion_blur(const MotionBlurLaunch& L, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const size_t pixels = (size_t)L.width * L.height;
    if (pixels == 0) return PYR_OK;
    const uint32_t edge = L.max_radius;
    const uint32_t tiles_x = (uint32_t)(((uint64_t)L.width + edge - 1) / edge), tiles_y = (uint32_t)(((uint64_t)L.height + edge - 1) / edge);
    const BlurGeometry G{L.width, L.height, edge, tiles_x, tiles_y};
    const uint32_t tiles = tiles_x * tiles_y; // at most the pixels: 32 bits hold it
    float4* velocity = reinterpret_cast<float4*>(L.work);
    float4* tile_max = velocity + pixels;
    float4* neighbour_max = tile_max + tiles;
    const auto launched = [](const char* what) {
        const hipError_t err = hipGetLastError();
        return err == hipSuccess ? PYR_OK : fail(PYR_ERR_DEVICE, std::string(what) + " kernel launch: " + hipGetErrorString(err));
    };
    int rc;
    hipLaunchKernelGGL(motion_blur_velocity_kernel, dim3(std::min(tiles, MAX_GRID)), dim3(VELOCITY_BLOCK), 0, stream, L.motion, G, 0.5f * L.shutter, (float)L.max_radius, velocity,
                       tile_max);
    if ((rc = launched("motion blur velocity")) != PYR_OK) return rc;
    hipLaunchKernelGGL(motion_blur_neighbour_kernel, dim3(std::min((tiles + TILE_BLOCK - 1) / TILE_BLOCK, MAX_GRID)), dim3(TILE_BLOCK), 0, stream, tile_max, G, neighbour_max);
    if ((rc = launched("motion blur neighbour maximum")) != PYR_OK) return rc;
    const uint32_t blocks_x = (uint32_t)(((uint64_t)L.width + GATHER_EDGE - 1) / GATHER_EDGE), blocks_y = (uint32_t)(((uint64_t)L.height + GATHER_EDGE - 1) / GATHER_EDGE);
    const uint32_t blocks = blocks_x * blocks_y;
    hipLaunchKernelGGL(motion_blur_gather_kernel, dim3(std::min(blocks, MAX_GRID)), dim3(GATHER_BLOCK), 0, stream, L, G, velocity, neighbour_max, blocks_x, blocks);
    return launched("motion blur gather");
}

} // namespace pyr
