// glare.hip -- the glare of a linear image (include/pyrite_gpu.h "glare"), a unit of its own: the header
// spells the f32 operations and their order out, the kernels keep both. It is the first image pass here that is a hierarchy: L
// downs over shrinking levels, L - 1 ups that add a level on the way back, and the compose, one launch each in the plain form. The levels 1..L live
// in working memory, kPixelFloats floats a pixel; the source S0 of level 0 is never written: the first down computes it while it
// loads, the compose computes it again from `image`.
//   Down. A workgroup owns a 16 x 16 tile of the destination level and stages the 34 x 34 source patch (taps 2x-1 .. 2x+2 of its
// 16 columns, each coordinate clamped to the level) in LDS once, one 16-byte slot a pixel; the row pass writes 34 x 16 row results
// to a second LDS array, the column pass reads four of them. A lane of the row pass wants the patch columns 2cx .. 2cx+3: in raster
// order the lanes of a row would be two slots apart and two of every 16 would share a slot of the 256-B bank row. So the patch is
// stored by parity: a row is kPatchPitch = 48 slots, even columns at 0..16, odd ones at kOddAt..kOddAt+16, and the four taps are
// slots cx, kOddAt+cx, cx+1, kOddAt+cx+1 -- consecutive lanes on consecutive slots in every one of the four reads. Both pitches
// (48 and 16 slots) are multiples of the 16 slots of a bank row, as kernels/temporal.hip's is and for its reason: the 16 lanes one
// ds_read_b128 cycle serves come from two rows of the lane grid at complementary columns. The patch is stored by eight consecutive
// lanes a cycle on the 128-B bank row of a store, four even and four odd columns: kOddAt is 4 mod 8, so that the two fours fall on
// different halves of it (with 24 every store of the patch was a 2-way conflict: DESIGN.md section 9l has the counter).
//   Up. A workgroup owns a 16 x 16 tile of level l and stages the 10 x 10 patch of T_{l+1} (i-1 .. i+1 of its 8 columns, clamped);
// rows first into LDS, 10 x 16, then columns. A lane owns a pixel: it reads its own S_l and writes T_l over it, nothing else of
// level l. The compose is the same up with the multiply by 1/G, S0 recomputed from `image`, and the blend written to `out`.
//   The small levels. A down or an up of a level of a few thousand pixels takes 3 to 5 us whatever it moves: glare_tail_kernel (below)
// runs everything under the first level that fits its LDS in one workgroup. The rule is per pixel, so both forms write the same
// bytes; the tail is the default because tools/bench_glare.py shows it the faster at 1920 x 1080 (glare_uses_tail).
//   Grid-stride loops over tiles, 64-bit indices into the buffers. No atomics: two calls write the same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "../api_internal.h"
#include "../device_scene.h"

#ifndef PYR_GLARE_PIXEL_FLOATS
#define PYR_GLARE_PIXEL_FLOATS 4 // 4: one 16-byte access a pixel; 3: three 4-byte ones and a quarter less memory (DESIGN.md 9l has both)
#endif

namespace pyr {

namespace {
constexpr uint32_t kPixelFloats = PYR_GLARE_PIXEL_FLOATS;
static_assert(kPixelFloats == 3 || kPixelFloats == 4, "a level holds three floats a pixel, bare or padded to 16 bytes");
constexpr uint32_t kTile = 16;                // pixels a side; 256 lanes, four waves
constexpr uint32_t kThreads = kTile * kTile;
constexpr uint32_t kMostBlocks = 256 * 32;    // one tile a workgroup up to 1920 x 1080
constexpr uint32_t kPatch = 2 * kTile + 2;    // 34: the source columns (rows) under a destination tile
constexpr uint32_t kPatchPitch = 48;          // slots a patch row: the 17 even columns, then at kOddAt the 17 odd ones
constexpr uint32_t kOddAt = 20;               // 4 mod 8: the eight lanes of a store group, four even and four odd columns, on eight slots
constexpr uint32_t kUpPatch = kTile / 2 + 2;  // 10: the coarse columns (rows) under a fine tile
constexpr uint32_t kPitch = 16;               // slots a row of the row results, and of the up's patch
static_assert(kOddAt >= kPatch / 2 && kOddAt + kPatch / 2 <= kPatchPitch && kOddAt % 8 == 4 && kPatchPitch % 16 == 0 && kPitch >= kUpPatch, "the LDS rows hold what they stage");

struct DownLaunch {
    const float* image; // FIRST: level 0 is made from it
    const float* from;  // otherwise: level l
    uint32_t from_width, from_height;
    float* to; // level l + 1
    uint32_t to_width, to_height;
    float threshold;
    float scale; // g_L
    bool last;   // level l + 1 is level L: T_L = S_L * g_L is what is written
};
struct UpLaunch {
    const float* coarse; // T_{l+1}
    uint32_t coarse_width, coarse_height;
    float* fine; // S_l, T_l written over it (not the compose)
    uint32_t width, height; // of level l
    float weight;           // g_l; the compose: 1 / G
    const float* image;     // the compose
    float* out;
    float strength, threshold;
};
} // namespace

// One slot in one ds_read_b128: a plain float4 read of which only x, y, z are used is taken apart (kernels/temporal.hip, read_slot).
__device__ inline float4 glare_slot(const float4* slot) {
    typedef float vec4 __attribute__((ext_vector_type(4)));
    const vec4 v = *(const volatile __attribute__((address_space(3))) vec4*)slot;
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ inline float4 level_pixel(const float* level, size_t q) {
    if (kPixelFloats == 4) return *reinterpret_cast<const float4*>(level + 4 * q);
    return make_float4(level[3 * q], level[3 * q + 1], level[3 * q + 2], 0.0f);
}
__device__ inline void set_level_pixel(float* level, size_t q, float4 v) {
    if (kPixelFloats == 4)
        *reinterpret_cast<float4*>(level + 4 * q) = v;
    else
        level[3 * q] = v.x, level[3 * q + 1] = v.y, level[3 * q + 2] = v.z;
}
__device__ inline bool glare_kept(float r, float g, float b) { return isfinite(r) && isfinite(g) && isfinite(b); }
// S0 of a kept pixel.
__device__ inline float4 glare_source(float r, float g, float b, float threshold) {
    if (threshold == 0.0f) return make_float4(r, g, b, 0.0f);
    const float y = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    const float k = fminf(fmaxf((y - threshold) / fmaxf(y, 1e-30f), 0.0f), 1.0f);
    return make_float4(r * k, g * k, b * k, 0.0f);
}
__device__ inline float4 down_taps(float4 a, float4 b, float4 c, float4 d) {
    return make_float4((a.x + d.x) * 0.125f + (b.x + c.x) * 0.375f, (a.y + d.y) * 0.125f + (b.y + c.y) * 0.375f, (a.z + d.z) * 0.125f + (b.z + c.z) * 0.375f, 0.0f);
}
__device__ inline float4 up_taps(float4 near, float4 far) {
    return make_float4(near.x * 0.75f + far.x * 0.25f, near.y * 0.75f + far.y * 0.25f, near.z * 0.75f + far.z * 0.25f, 0.0f);
}
__device__ inline int64_t clamp_to(int64_t v, uint32_t size) { return v < 0 ? 0 : (v > (int64_t)size - 1 ? (int64_t)size - 1 : v); }

template <bool FIRST>
__global__ __launch_bounds__(kThreads) void glare_down_kernel(DownLaunch L) {
    __shared__ float4 patch[kPatch * kPatchPitch];
    __shared__ float4 rows[kPatch * kPitch];
    const uint32_t tiles_x = (L.to_width - 1) / kTile + 1, tiles_y = (L.to_height - 1) / kTile + 1;
    const uint32_t tiles = tiles_x * tiles_y;
    const uint32_t lx = threadIdx.x % kTile, ly = threadIdx.x / kTile;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t tile_y = t / tiles_x, tile_x = t - tile_y * tiles_x;
        const int64_t x_first = 2 * (int64_t)tile_x * kTile - 1, y_first = 2 * (int64_t)tile_y * kTile - 1;
        for (uint32_t i = threadIdx.x; i < kPatch * kPatch; i += kThreads) {
            const uint32_t row = i / kPatch, col = i - row * kPatch;
            const size_t q = (size_t)clamp_to(y_first + row, L.from_height) * L.from_width + (size_t)clamp_to(x_first + col, L.from_width);
            float4 v;
            if (FIRST) {
                const float r = L.image[3 * q], g = L.image[3 * q + 1], b = L.image[3 * q + 2];
                v = glare_kept(r, g, b) ? glare_source(r, g, b, L.threshold) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            } else {
                v = level_pixel(L.from, q);
            }
            patch[row * kPatchPitch + (col & 1u) * kOddAt + (col >> 1)] = v;
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < kPatch * kTile; i += kThreads) {
            const uint32_t row = i / kTile, cx = i - row * kTile;
            const float4* at = patch + row * kPatchPitch + cx; // columns 2cx, 2cx+1, 2cx+2, 2cx+3 of the patch
            rows[row * kPitch + cx] = down_taps(glare_slot(at), glare_slot(at + kOddAt), glare_slot(at + 1), glare_slot(at + kOddAt + 1));
        }
        __syncthreads();
        const uint32_t x = tile_x * kTile + lx, y = tile_y * kTile + ly;
        if (x < L.to_width && y < L.to_height) {
            const float4* at = rows + (2 * ly) * kPitch + lx;
            float4 v = down_taps(glare_slot(at), glare_slot(at + kPitch), glare_slot(at + 2 * kPitch), glare_slot(at + 3 * kPitch));
            if (L.last) v = make_float4(v.x * L.scale, v.y * L.scale, v.z * L.scale, 0.0f);
            set_level_pixel(L.to, (size_t)y * L.to_width + x, v);
        }
        __syncthreads(); // before the next tile overwrites this one
    }
}

template <bool COMPOSE>
__global__ __launch_bounds__(kThreads) void glare_up_kernel(UpLaunch L) {
    __shared__ float4 patch[kUpPatch * kPitch];
    __shared__ float4 rows[kUpPatch * kPitch];
    const uint32_t tiles_x = (L.width - 1) / kTile + 1, tiles_y = (L.height - 1) / kTile + 1;
    const uint32_t tiles = tiles_x * tiles_y;
    const uint32_t lx = threadIdx.x % kTile, ly = threadIdx.x / kTile;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t tile_y = t / tiles_x, tile_x = t - tile_y * tiles_x;
        const int64_t x_first = (int64_t)tile_x * (kTile / 2) - 1, y_first = (int64_t)tile_y * (kTile / 2) - 1;
        if (threadIdx.x < kUpPatch * kUpPatch) {
            const uint32_t row = threadIdx.x / kUpPatch, col = threadIdx.x - row * kUpPatch;
            const size_t q = (size_t)clamp_to(y_first + row, L.coarse_height) * L.coarse_width + (size_t)clamp_to(x_first + col, L.coarse_width);
            patch[row * kPitch + col] = level_pixel(L.coarse, q);
        }
        __syncthreads();
        if (threadIdx.x < kUpPatch * kTile) { // rows: the patch column of i = x >> 1 is (lx >> 1) + 1, its neighbour one to the left (even x) or right
            const float4* at = patch + ly * kPitch + (lx >> 1) + 1;
            rows[ly * kPitch + lx] = up_taps(glare_slot(at), (lx & 1u) ? glare_slot(at + 1) : glare_slot(at - 1));
        }
        __syncthreads();
        const uint32_t x = tile_x * kTile + lx, y = tile_y * kTile + ly;
        if (x < L.width && y < L.height) {
            const float4* at = rows + ((ly >> 1) + 1) * kPitch + lx;
            const float4 up = up_taps(glare_slot(at), (ly & 1u) ? glare_slot(at + kPitch) : glare_slot(at - kPitch));
            const size_t p = (size_t)y * L.width + x;
            if (COMPOSE) {
                const float r = L.image[3 * p], g = L.image[3 * p + 1], b = L.image[3 * p + 2];
                if (glare_kept(r, g, b)) {
                    const float4 s = glare_source(r, g, b, L.threshold);
                    L.out[3 * p] = (r - L.strength * s.x) + L.strength * (up.x * L.weight);
                    L.out[3 * p + 1] = (g - L.strength * s.y) + L.strength * (up.y * L.weight);
                    L.out[3 * p + 2] = (b - L.strength * s.z) + L.strength * (up.z * L.weight);
                } else { // its own bits
                    L.out[3 * p] = r, L.out[3 * p + 1] = g, L.out[3 * p + 2] = b;
                }
            } else {
                const float4 s = level_pixel(L.fine, p);
                set_level_pixel(L.fine, p, make_float4(s.x * L.weight + up.x, s.y * L.weight + up.y, s.z * L.weight + up.z, 0.0f));
            }
        }
        __syncthreads(); // before the next tile overwrites this one
    }
}

// The tail: the levels too small to fill the machine, in one launch of one workgroup. It is given level `first` (S, in working
// memory) and keeps the levels first+1 .. last in LDS: the downs, then the ups, then T of level `first` written over its S -- the
// only thing it writes. Nothing is staged and no row result is stored: a pixel of a down computes its four row results itself (16
// taps), one of an up its two (4 taps). A row result is the same f32 whoever computes it, so the bits are those of the plain form.
template <class Source>
__device__ inline float4 tail_down_pixel(Source source, uint32_t from_width, uint32_t from_height, uint32_t x, uint32_t y) {
    float4 r[4];
    const size_t x0 = (size_t)clamp_to(2 * (int64_t)x - 1, from_width), x1 = (size_t)clamp_to(2 * (int64_t)x, from_width),
                 x2 = (size_t)clamp_to(2 * (int64_t)x + 1, from_width), x3 = (size_t)clamp_to(2 * (int64_t)x + 2, from_width);
    for (int k = 0; k < 4; ++k) {
        const size_t row = (size_t)clamp_to(2 * (int64_t)y - 1 + k, from_height) * from_width;
        r[k] = down_taps(source(row + x0), source(row + x1), source(row + x2), source(row + x3));
    }
    return down_taps(r[0], r[1], r[2], r[3]);
}
__device__ inline float4 tail_up_pixel(const float4* coarse, uint32_t coarse_width, uint32_t coarse_height, uint32_t x, uint32_t y) {
    const uint32_t i = x >> 1, j = y >> 1;
    const uint32_t io = (x & 1u) ? (i + 1 < coarse_width ? i + 1 : coarse_width - 1) : (i ? i - 1 : 0);
    const uint32_t jo = (y & 1u) ? (j + 1 < coarse_height ? j + 1 : coarse_height - 1) : (j ? j - 1 : 0);
    const float4* near = coarse + j * coarse_width;
    const float4* far = coarse + jo * coarse_width;
    return up_taps(up_taps(glare_slot(near + i), glare_slot(near + io)), up_taps(glare_slot(far + i), glare_slot(far + io)));
}

namespace {
constexpr uint32_t kTailThreads = 1024;
constexpr uint32_t kTailSlots = 4096; // 64 KB of LDS: the levels below the tail's first, a 16-byte slot a pixel
struct TailLaunch {
    float* top; // level `first`: S read, T written
    uint32_t first, last; // first < last = L
    uint32_t width[PYR_GLARE_MOST_LEVELS + 1], height[PYR_GLARE_MOST_LEVELS + 1];
    uint32_t at[PYR_GLARE_MOST_LEVELS + 1]; // slots before level l in LDS, l = first+1 .. last
    float g[PYR_GLARE_MOST_LEVELS + 1];
};
} // namespace

__global__ __launch_bounds__(kTailThreads) void glare_tail_kernel(TailLaunch L) {
    __shared__ float4 levels[kTailSlots];
    for (uint32_t l = L.first; l < L.last; ++l) { // S_{l+1} from S_l
        const uint32_t w = L.width[l + 1], h = L.height[l + 1];
        float4* to = levels + L.at[l + 1];
        for (uint32_t p = threadIdx.x; p < w * h; p += kTailThreads) {
            const uint32_t y = p / w, x = p - y * w;
            float4 v;
            if (l == L.first) {
                const float* top = L.top;
                v = tail_down_pixel([top](size_t q) { return level_pixel(top, q); }, L.width[l], L.height[l], x, y);
            } else {
                const float4* from = levels + L.at[l];
                v = tail_down_pixel([from](size_t q) { return glare_slot(from + q); }, L.width[l], L.height[l], x, y);
            }
            if (l + 1 == L.last) v = make_float4(v.x * L.g[L.last], v.y * L.g[L.last], v.z * L.g[L.last], 0.0f);
            to[p] = v;
        }
        __syncthreads();
    }
    for (uint32_t l = L.last - 1; l > L.first; --l) { // T_l over S_l, in LDS
        const uint32_t w = L.width[l], h = L.height[l];
        float4* fine = levels + L.at[l];
        const float4* coarse = levels + L.at[l + 1];
        const float weight = L.g[l];
        for (uint32_t p = threadIdx.x; p < w * h; p += kTailThreads) {
            const uint32_t y = p / w, x = p - y * w;
            const float4 up = tail_up_pixel(coarse, L.width[l + 1], L.height[l + 1], x, y);
            const float4 s = glare_slot(fine + p);
            fine[p] = make_float4(s.x * weight + up.x, s.y * weight + up.y, s.z * weight + up.z, 0.0f);
        }
        __syncthreads();
    }
    const uint32_t w = L.width[L.first], h = L.height[L.first]; // at most 4 * kTailSlots + what the odd sides add: w * h fits 32 bits
    const float4* coarse = levels + L.at[L.first + 1];
    const float weight = L.g[L.first];
    for (uint32_t p = threadIdx.x; p < w * h; p += kTailThreads) {
        const uint32_t y = p / w, x = p - y * w;
        const float4 up = tail_up_pixel(coarse, L.width[L.first + 1], L.height[L.first + 1], x, y);
        const float4 s = level_pixel(L.top, p);
        set_level_pixel(L.top, p, make_float4(s.x * weight + up.x, s.y * weight + up.y, s.z * weight + up.z, 0.0f));
    }
}

namespace {
struct Pyramid {
    uint32_t count;                                  // L
    uint32_t width[PYR_GLARE_MOST_LEVELS + 1], height[PYR_GLARE_MOST_LEVELS + 1];
    size_t at[PYR_GLARE_MOST_LEVELS + 2];            // pixels before level l in the working memory; at[1] = 0
};
Pyramid pyramid_of(uint32_t width, uint32_t height, uint32_t levels) {
    Pyramid P{};
    P.width[0] = width, P.height[0] = height;
    P.at[0] = P.at[1] = 0;
    while (P.count < levels && P.count < PYR_GLARE_MOST_LEVELS && (P.width[P.count] > 1 || P.height[P.count] > 1)) {
        const uint32_t l = P.count++;
        P.width[l + 1] = P.width[l] / 2 + (P.width[l] & 1u), P.height[l + 1] = P.height[l] / 2 + (P.height[l] & 1u); // (w + 1) / 2 without the carry
        P.at[l + 2] = P.at[l + 1] + (size_t)P.width[l + 1] * P.height[l + 1];
    }
    return P;
}
// The level the tail starts from: the first level m >= 1 below which everything -- the levels m+1 .. L -- fits kTailSlots; 0 when
// there is none or nothing lies below it (m = L), and then every step is a launch of its own.
uint32_t tail_level(const Pyramid& P) {
    for (uint32_t m = 1; m < P.count; ++m)
        if (P.at[P.count + 1] - P.at[m + 1] <= kTailSlots) return m;
    return 0;
}
// Which form a call runs. Both write the same bytes (tests/test_gpu_glare.py runs each); the tail is the default because it is the
// faster at 1920 x 1080 with 11 levels (0.093 against 0.115 ms) and no slower with 6 (DESIGN.md section 9l has both).
// PYRITE_GLARE_TAIL=0|1 overrides, read at every call (development: tools/bench_glare.py times one against the other).
bool glare_uses_tail() {
    const char* e = std::getenv("PYRITE_GLARE_TAIL");
    return !(e && std::string(e) == "0");
}
uint32_t grid_of(uint32_t width, uint32_t height) {
    const uint64_t tiles = (uint64_t)((width - 1) / kTile + 1) * ((height - 1) / kTile + 1);
    return (uint32_t)std::min<uint64_t>(tiles, kMostBlocks);
}
} // namespace

size_t glare_work_bytes(uint32_t width, uint32_t height, uint32_t levels) {
    const Pyramid P = pyramid_of(width, height, levels);
    return std::max<size_t>(P.at[P.count + 1], 1) * kPixelFloats * sizeof(float); // a 1 x 1 image has no level: one pixel, unused
}

int launch_glare(const GlareLaunch& launch, void* stream_) {
    if (launch.width == 0 || launch.height == 0) return PYR_OK;
    if (launch.levels < 1 || launch.levels > PYR_GLARE_MOST_LEVELS) return fail(PYR_ERR_INVALID_ARGUMENT, "glare: levels must be 1..12"); // Pyramid holds no more
    hipStream_t stream = (hipStream_t)stream_;
    const Pyramid P = pyramid_of(launch.width, launch.height, launch.levels);
    const uint32_t L = P.count;
    if (L == 0) { // 1 x 1: out = image
        const hipError_t err = hipMemcpyAsync(launch.out, launch.image, 3 * sizeof(float), hipMemcpyDeviceToDevice, stream);
        if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("glare copy: ") + hipGetErrorString(err));
        return PYR_OK;
    }
    float g[PYR_GLARE_MOST_LEVELS + 1];
    g[1] = 1.0f;
    float total = g[1];
    for (uint32_t l = 2; l <= L; ++l) {
        g[l] = g[l - 1] * launch.falloff;
        total = total + g[l];
    }
    const float inv = 1.0f / total;
    auto level = [&](uint32_t l) { return launch.work + P.at[l] * kPixelFloats; };
    const uint32_t tail = glare_uses_tail() ? tail_level(P) : 0;
    const uint32_t plain_to = tail ? tail : L; // the levels 1 .. plain_to are written by a down of their own, the ups start below it
    for (uint32_t l = 0; l < plain_to; ++l) {
        const DownLaunch D{launch.image, l ? level(l) : nullptr, P.width[l], P.height[l], level(l + 1), P.width[l + 1], P.height[l + 1], launch.threshold, g[L], l + 1 == L};
        const dim3 grid(grid_of(P.width[l + 1], P.height[l + 1]));
        if (l == 0)
            hipLaunchKernelGGL(glare_down_kernel<true>, grid, dim3(kThreads), 0, stream, D);
        else
            hipLaunchKernelGGL(glare_down_kernel<false>, grid, dim3(kThreads), 0, stream, D);
    }
    if (tail) {
        TailLaunch T{};
        T.top = level(tail), T.first = tail, T.last = L;
        for (uint32_t l = tail; l <= L; ++l) {
            T.width[l] = P.width[l], T.height[l] = P.height[l], T.g[l] = g[l];
            T.at[l] = l > tail ? (uint32_t)(P.at[l] - P.at[tail + 1]) : 0;
        }
        hipLaunchKernelGGL(glare_tail_kernel, dim3(1), dim3(kTailThreads), 0, stream, T);
    }
    for (uint32_t l = plain_to - 1; l >= 1; --l) {
        const UpLaunch U{level(l + 1), P.width[l + 1], P.height[l + 1], level(l), P.width[l], P.height[l], g[l], nullptr, nullptr, 0.0f, 0.0f};
        hipLaunchKernelGGL(glare_up_kernel<false>, dim3(grid_of(P.width[l], P.height[l])), dim3(kThreads), 0, stream, U);
    }
    const UpLaunch C{level(1), P.width[1], P.height[1], nullptr, launch.width, launch.height, inv, launch.image, launch.out, launch.strength, launch.threshold};
    hipLaunchKernelGGL(glare_up_kernel<true>, dim3(grid_of(launch.width, launch.height)), dim3(kThreads), 0, stream, C);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("glare kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

} // namespace pyr
