// lens_blur.hip -- lens blur as a post filter over the feature records (include/pyrite_gpu.h "lens blur over the feature records",
// DESIGN.md section 9o), a unit of its own: the header spells the f32 operations and their order out, the kernel keeps both. One
// launch. A workgroup owns a 16 x 16 tile and stages it with its max_radius-wide ring once in LDS, as temporal.hip does; everything
// a tap needs is decided at load time, so the gather has no division and no global load:
//   colour[]  one 16-byte slot a pixel: the three floats and c, its circle of confusion. A pixel that is outside the image or whose
//             colour is not finite holds (0, 0, 0, -2): with c = -2 the rule's weight clamp01((c_e - d) + 1) is 0 on either branch
//             (fminf(-2, c_p) = -2), so the flag costs nothing in the loop;
//   lens[]    8 bytes beside it: inv, one over the disc's area, and z, the axial depth (0 and FLT_MAX where the slot is not usable).
//   The rule says a tap with w == 0 adds nothing, and here every tap is added: w = 0 times a finite colour is a zero of either
// sign, and a sum that starts from +0.0f is never -0.0f, so adding it changes no bit. (The staged colours are all finite.) The
// front and the back sums take the tap's weight or 0 by a select, for the same reason.
//   The bound. While staging, the workgroup reduces the largest c of its slots. (c_e - d) + 1 is monotone in c_e, so no tap with
// (c_max - d) + 1 <= 0 weighs, and none beyond reach = ceil(c_max) in x or y: the rows run to the reach, not to max_radius, each row
// as far as that test holds in it (d grows with |ox|; seventeen lanes find the rows' ends once per tile, so that the tap loop has
// no test in it and its three LDS reads -- d from a 17 x 17 table, one address for the wave, and the slot's two -- are in flight
// together), and a tile whose reach is 0 copies its input. Which taps are visited cannot show in the bits.
//   Layout. A wave is a strip of 4 rows x 16 pixels and a tile row is kPitch = 48 slots, a multiple of 16: temporal.hip's argument
// holds for the 16-byte slots (768 B a row, three bank rows: the 16 lanes a ds_read_b128 serves at a time fall on 16 different
// slots of a bank row whatever the offset is). ds_read_b64 serves 32 lanes at a time, two rows of the strip: a row's 16 slots are
// 128 contiguous bytes, 32 banks, and the next row starts 384 B = 96 banks on, in the other half of the bank row.
//   LDS: 48 * 48 * 24 B + the table, the rows' ends and four floats = 56,560 B of the 64 KB a workgroup may have, at every radius.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>

#include "../api_internal.h"
#include "../device_scene.h"

namespace pyr {

namespace {
constexpr uint32_t kTile = 16;                                    // pixels a side; 256 lanes, four waves
constexpr uint32_t kRows = kTile + 2 * PYR_LENS_BLUR_MOST_RADIUS; // 48: the tile and its ring at the largest radius
constexpr uint32_t kPitch = 48;                                   // slots a tile row: >= kRows and a multiple of 16 (above)
constexpr uint32_t kDist = PYR_LENS_BLUR_MOST_RADIUS + 1;         // the table of d: |ox|, |oy| = 0..16
constexpr uint32_t kMostBlocks = 256 * 32;                        // one tile a workgroup up to 1920 x 1080
constexpr float kPi = 3.14159265f;
static_assert(kPitch >= kRows && kPitch % 16 == 0, "the LDS rows hold the ring and keep the bank argument");

// One slot in one ds_read_b128 (temporal.hip's read_slot: a plain float4 read is taken apart where c and the colour are used apart).
__device__ inline float4 read_colour(const float4* slot) {
    typedef float vec4 __attribute__((ext_vector_type(4)));
    const vec4 v = *(const volatile __attribute__((address_space(3))) vec4*)slot;
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ inline float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ inline float uniform(float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); } // the same in every lane: say so
} // namespace

__global__ __launch_bounds__(kTile* kTile) void lens_blur_kernel(LensBlurLaunch L) {
    __shared__ float4 colour[kRows * kPitch];
    __shared__ float2 lens[kRows * kPitch];
    __shared__ float dist[kDist * kDist];
    __shared__ float wave_most[kTile * kTile / 64];
    __shared__ int row_reach[kDist];
    const uint32_t tiles_x = (L.width - 1) / kTile + 1, tiles_y = (L.height - 1) / kTile + 1; // width * height < 2^32: so is the product
    const uint32_t tiles = tiles_x * tiles_y;
    const uint32_t radius = L.max_radius, span = kTile + 2 * radius;
    const uint32_t lx = threadIdx.x % kTile, ly = threadIdx.x / kTile;
    const float m = (float)max(L.width, L.height) * 0.5f;
    const float A = (sqrtf(L.aperture) * (L.view_plane / L.focus_distance)) * m, R = (float)radius;
    const float half_w = (float)L.width * 0.5f, half_h = (float)L.height * 0.5f, half_size = (1.0f / m) * 0.5f;
    const float vv = L.view_plane * L.view_plane;
    for (uint32_t i = threadIdx.x; i < kDist * kDist; i += kTile * kTile) {
        const uint32_t ay = i / kDist, ax = i - ay * kDist;
        dist[i] = sqrtf((float)(ax * ax + ay * ay));
    }
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t tile_y = t / tiles_x, tile_x = t - tile_y * tiles_x;
        const int64_t x_first = (int64_t)tile_x * kTile - radius, y_first = (int64_t)tile_y * kTile - radius;
        float most = 0.0f; // the largest c of the slots this lane stages; c is never negative where a slot is usable
        for (uint32_t i = threadIdx.x; i < span * span; i += kTile * kTile) {
            const uint32_t row = i / span, col = i - row * span;
            const int64_t qx = x_first + col, qy = y_first + row;
            float4 slot = make_float4(0.0f, 0.0f, 0.0f, -2.0f);
            float2 beside = make_float2(0.0f, FLT_MAX);
            if (qx >= 0 && qx < (int64_t)L.width && qy >= 0 && qy < (int64_t)L.height) {
                const size_t q = (size_t)qy * L.width + (size_t)qx;
                const float c0 = L.image[3 * q], c1 = L.image[3 * q + 1], c2 = L.image[3 * q + 2];
                if (isfinite(c0) && isfinite(c1) && isfinite(c2)) {
                    const float4* record = reinterpret_cast<const float4*>(L.pixels + q);
                    const float4 lo = record[0], hi = record[1]; // normal, depth; coverage, shape, material
                    const float depth = lo.w, coverage = hi.x;
                    float z = FLT_MAX, c = fminf(A, R);
                    if (!(coverage == 0.0f || !isfinite(depth) || depth <= 0.0f)) {
                        const float px = ((float)(uint32_t)qx + -half_w) / m + half_size, py = ((float)(uint32_t)qy + -half_h) / m + half_size;
                        const float tt = (px * px + py * py) / vv;
                        z = depth / sqrtf(1.0f + tt);
                        c = fminf(A * fabsf(1.0f - L.focus_distance / z), R);
                    }
                    const float inv = 1.0f / fmaxf(kPi * ((c + 0.5f) * (c + 0.5f)), 1.0f);
                    slot = make_float4(c0, c1, c2, c);
                    beside = make_float2(inv, z);
                    most = fmaxf(most, c);
                }
            }
            colour[row * kPitch + col] = slot;
            lens[row * kPitch + col] = beside;
        }
        for (int offset = 32; offset > 0; offset >>= 1) most = fmaxf(most, __shfl_xor(most, offset));
        if ((threadIdx.x & 63u) == 0u) wave_most[threadIdx.x >> 6] = most;
        __syncthreads();
        const float c_most = uniform(fmaxf(fmaxf(wave_most[0], wave_most[1]), fmaxf(wave_most[2], wave_most[3])));
        const int reach = (int)min(radius, (uint32_t)ceilf(c_most)); // 0 <= c_most <= max_radius
        if (threadIdx.x <= (uint32_t)reach) { // per row of the window, how far it runs: d grows with |ox| and the test is monotone in d
            int last = -1;                    // -1: not even the row's middle weighs
            for (int ax = 0; ax <= reach; ++ax)
                if ((c_most - dist[threadIdx.x * kDist + (uint32_t)ax]) + 1.0f > 0.0f) last = ax;
            row_reach[threadIdx.x] = last;
        }
        __syncthreads();
        const uint32_t x = tile_x * kTile + lx, y = tile_y * kTile + ly;
        if (x < L.width && y < L.height) {
            const size_t px = (size_t)y * L.width + x;
            const float mine[3] = {L.image[3 * px], L.image[3 * px + 1], L.image[3 * px + 2]}; // the tile holds only a usable pixel's bits
            const uint32_t centre = (ly + radius) * kPitch + lx + radius;
            const float c_p = colour[centre].w;
            float result[3] = {mine[0], mine[1], mine[2]};
            if (reach > 0 && c_p >= 0.0f) {
                const float2 own = lens[centre];
                const float inv_p = own.x, z_p = own.y, tolerance = L.depth_tolerance * z_p;
                float weight_f = 0.0f, weight_b = 0.0f, sum_f[3] = {0.0f, 0.0f, 0.0f}, sum_b[3] = {0.0f, 0.0f, 0.0f};
                bool others = false;
                for (int oy = -reach; oy <= reach; ++oy) {
                    const int across = __builtin_amdgcn_readfirstlane(row_reach[abs(oy)]); // beyond it no slot of this tile weighs in this row
                    for (int ox = -across; ox <= across; ++ox) {
                        const float d = dist[(uint32_t)abs(oy) * kDist + (uint32_t)abs(ox)]; // one address for the wave: a broadcast, in flight with the slot's two reads
                        const uint32_t at = (uint32_t)((int)centre + oy * (int)kPitch + ox);
                        const float4 q = read_colour(&colour[at]);
                        const float2 b = lens[at];
                        const bool front = (z_p - b.y) > tolerance;
                        const float c_e = front ? q.w : fminf(q.w, c_p);
                        const float inv_e = (front || q.w < c_p) ? b.x : inv_p;
                        const float w = clamp01((c_e - d) + 1.0f) * inv_e;
                        const float w_f = front ? w : 0.0f, w_b = front ? 0.0f : w;
                        weight_f = weight_f + w_f, weight_b = weight_b + w_b;
                        sum_f[0] = sum_f[0] + w_f * q.x, sum_f[1] = sum_f[1] + w_f * q.y, sum_f[2] = sum_f[2] + w_f * q.z;
                        sum_b[0] = sum_b[0] + w_b * q.x, sum_b[1] = sum_b[1] + w_b * q.y, sum_b[2] = sum_b[2] + w_b * q.z;
                        if (ox != 0 || oy != 0) others = others || w > 0.0f;
                    }
                }
                if (others) {
                    for (int c = 0; c < 3; ++c) result[c] = sum_b[c] / weight_b;
                    if (weight_f != 0.0f) {
                        const float a = fminf(weight_f, 1.0f);
                        for (int c = 0; c < 3; ++c) result[c] = a * (sum_f[c] / weight_f) + (1.0f - a) * result[c];
                    }
                }
            }
            L.out[3 * px] = result[0], L.out[3 * px + 1] = result[1], L.out[3 * px + 2] = result[2];
        }
        __syncthreads(); // before the next tile overwrites this one
    }
}

int launch_lens_blur(const LensBlurLaunch& launch, void* stream) {
    if (launch.width == 0 || launch.height == 0) return PYR_OK;
    if (launch.max_radius < 1 || launch.max_radius > PYR_LENS_BLUR_MOST_RADIUS) return fail(PYR_ERR_INVALID_ARGUMENT, "lens blur: max_radius must be 1..16"); // the LDS tile holds no wider ring
    const uint64_t tiles = (uint64_t)((launch.width - 1) / kTile + 1) * ((launch.height - 1) / kTile + 1);
    hipLaunchKernelGGL(lens_blur_kernel, dim3((uint32_t)std::min<uint64_t>(tiles, kMostBlocks)), dim3(kTile * kTile), 0, (hipStream_t)stream, launch);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("lens blur kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

} // namespace pyr
