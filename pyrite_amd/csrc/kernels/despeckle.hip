// despeckle.hip -- the firefly clamp of two developed half images, a unit of its own: include/pyrite_gpu.h
// spells the f32 operations and their order out, the kernel keeps both. Nothing here touches the render, film, feature, tone or any
// other image kernel.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <utility>

#include "../api_internal.h"
#include "../device_scene.h"
#include "despeckle_tile.h"

namespace pyr {

namespace {
constexpr uint32_t TILE_BLOCK = kDespeckleTile * kDespeckleTile;

int launched(const char* what) {
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess) return PYR_OK;
    return fail(PYR_ERR_DEVICE, std::string(what) + " kernel launch: " + hipGetErrorString(err));
}

// The statistics' luminance; the + 0.0f turns a -0 into +0, so that no -0 enters an ordering. What is not finite is staged as +inf,
// the sentinel of an empty slot: "finite" is "below +inf" from here on.
__device__ inline float luminance_or_inf(const float* rgb) {
    const float y = ((0.2126f * rgb[0] + 0.7152f * rgb[1]) + 0.0722f * rgb[2]) + 0.0f;
    return fabsf(y) < INFINITY ? y : INFINITY;
}

// The two networks of despeckle_tile.h run over a register array, ascending. The values are finite or +inf, never NaN, never -0, so
// v_min_f32 / v_max_f32 order them as a comparison would. Selections only: whatever network sorts, the median has the same bits.
__device__ inline int exchange(float& a, float& b) {
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo, b = hi;
    return 0;
}
template <uint32_t S, bool MERGE, size_t... I>
__device__ inline void run_network(float (&v)[S], std::index_sequence<I...>) {
    constexpr DespeckleNetwork<S> net = MERGE ? despeckle_merge_network<S>() : despeckle_sort_network<S>();
    const int done[] = {exchange(v[net.lo[I]], v[net.hi[I]])...}; // a braced list: evaluated left to right
    (void)done;
}
template <uint32_t S>
__device__ inline void sort_ascending(float (&v)[S]) { // any list
    run_network<S, false>(v, std::make_index_sequence<despeckle_sort_network<S>().count>());
}
template <uint32_t S>
__device__ inline void merge_ascending(float (&v)[S]) { // a list that falls and then rises
    run_network<S, true>(v, std::make_index_sequence<despeckle_merge_network<S>().count>());
}

// Element `rank` of a sorted register array without an indexed load, which would send the array to scratch: the bits of the one
// element whose index matches, or-ed out of zeros. (A chain of selects between the elements themselves is folded by the optimiser
// into a select between their addresses and one load -- the indexed load again.)
template <uint32_t S>
__device__ inline float pick(const float (&v)[S], uint32_t rank) {
    uint32_t bits = 0;
#pragma unroll
    for (uint32_t i = 0; i < S; ++i) bits |= rank == i ? __float_as_uint(v[i]) : 0u;
    return __uint_as_float(bits);
}
} // namespace

// A workgroup owns a 16 x 16 tile and stages {Y_a, Y_b} of the tile and its halo of RADIUS pixels in LDS (despeckle_tile.h: the
// addressing and its banking); a cell that stands for no pixel, a luminance that is not finite and every Y_b without a second half
// hold +inf. Then a thread owns a pixel: it gathers the 2 * ((2 RADIUS + 1)^2 - 1) values around it into registers, counts the
// finite ones, sorts, picks the lower median, forms the deviations, merges them into order, picks theirs, and clamps what the rule
// calls a firefly. Plain stores. The counts are summed per wave by a ballot, per workgroup in LDS, and reach memory as at most two integer
// atomics a workgroup: one atomic a clamped pixel, all on two addresses, cost more than the rest of the kernel on a noisy render.
// LDS: (16 + 2 RADIUS) * 48 * 8 B and two words: 6,920 B at radius 1, 7,688 B at radius 2.
template <uint32_t RADIUS>
__global__ __launch_bounds__(TILE_BLOCK) void despeckle_kernel(DespeckleLaunch L) {
    constexpr uint32_t ROWS = kDespeckleTile + 2 * RADIUS, SLOTS = 2 * ((2 * RADIUS + 1) * (2 * RADIUS + 1) - 1);
    __shared__ __attribute__((aligned(16))) float2 yy[ROWS * kDespecklePitch];
    __shared__ uint32_t tally[2];
    if (threadIdx.x < 2) tally[threadIdx.x] = 0;
    const uint32_t tile_x = blockIdx.x % L.tiles_x, tile_y = blockIdx.x / L.tiles_x;
    const uint32_t x0 = tile_x * kDespeckleTile, y0 = tile_y * kDespeckleTile;
    for (uint32_t c = threadIdx.x; c < ROWS * ROWS; c += TILE_BLOCK) {
        const int32_t lx = (int32_t)(c % ROWS) - (int32_t)RADIUS, ly = (int32_t)(c / ROWS) - (int32_t)RADIUS;
        const DespeckleCell cell = despeckle_cell(L.width, L.height, x0, y0, RADIUS, lx, ly);
        float2 y = make_float2(INFINITY, INFINITY);
        if (cell.inside) {
            y.x = luminance_or_inf(L.a + 3 * cell.pixel);
            if (L.b) y.y = luminance_or_inf(L.b + 3 * cell.pixel);
        }
        yy[cell.lds] = y;
    }
    __syncthreads();
    const int32_t lx = (int32_t)(threadIdx.x % kDespeckleTile), ly = (int32_t)(threadIdx.x / kDespeckleTile);
    const DespeckleCell self = despeckle_cell(L.width, L.height, x0, y0, RADIUS, lx, ly);
    bool clamp_a = false, clamp_b = false;
    if (self.inside) { // threads outside the image stay for the tally's barrier
        const size_t p = self.pixel;

        float v[SLOTS];
        uint32_t n = 0;
#pragma unroll
        for (uint32_t w = 0; w < SLOTS / 2; ++w) { // the window in raster order without its centre
            constexpr uint32_t SIDE = 2 * RADIUS + 1;
            const uint32_t at = w < SIDE * SIDE / 2 ? w : w + 1;
            const int32_t ox = (int32_t)(at % SIDE) - (int32_t)RADIUS, oy = (int32_t)(at / SIDE) - (int32_t)RADIUS;
            const float2 y = yy[despeckle_cell(L.width, L.height, x0, y0, RADIUS, lx + ox, ly + oy).lds];
            v[2 * w] = y.x, v[2 * w + 1] = y.y;
            n += (y.x < INFINITY) + (y.y < INFINITY);
        }
        const float2 own = yy[self.lds];
        const uint32_t rank = (n - 1) / 2; // n >= PYR_DESPECKLE_LEAST_SAMPLES where it is used
        sort_ascending(v);
        const float m = pick(v, rank);
#pragma unroll
        for (uint32_t i = 0; i < SLOTS; ++i) v[i] = fabsf(v[i] - m); // an empty slot stays +inf; the list falls to 0 at the median and rises
        merge_ascending(v);
        const float s = pick(v, rank);
        const float spread = fmaxf(fmaxf(s * 1.4826f, L.relative * m), L.floor);
        const float limit = m + L.k * spread;
        const bool enough = n >= PYR_DESPECKLE_LEAST_SAMPLES;
        const bool above_a = own.x < INFINITY && own.x > limit, above_b = own.y < INFINITY && own.y > limit;
        clamp_a = enough && above_a && !above_b, clamp_b = enough && above_b && !above_a;

        float removed[3] = {0.0f, 0.0f, 0.0f};
        {
            const float g = limit / own.x;
            for (int c = 0; c < 3; ++c) {
                const float in = L.a[3 * p + c], out = clamp_a ? in * g : in;
                L.a_out[3 * p + c] = out;
                if (clamp_a) removed[c] = in - out;
            }
        }
        if (L.b) {
            const float g = limit / own.y;
            for (int c = 0; c < 3; ++c) {
                const float in = L.b[3 * p + c], out = clamp_b ? in * g : in;
                L.b_out[3 * p + c] = out;
                removed[c] = (removed[c] + (clamp_b ? in - out : 0.0f)) * 0.5f;
            }
        }
        if (L.removed)
            for (int c = 0; c < 3; ++c) L.removed[3 * p + c] = removed[c];
    }
    if (L.counts) { // uniform
        const unsigned long long wave_a = __ballot(clamp_a), wave_b = __ballot(clamp_b);
        if ((threadIdx.x & (warpSize - 1)) == 0) {
            if (wave_a) atomicAdd(&tally[0], (uint32_t)__popcll(wave_a));
            if (wave_b) atomicAdd(&tally[1], (uint32_t)__popcll(wave_b));
        }
        __syncthreads();
        if (threadIdx.x < 2 && tally[threadIdx.x]) atomicAdd(&L.counts[threadIdx.x], tally[threadIdx.x]);
    }
}

int launch_despeckle(const DespeckleLaunch& launch, void* stream) {
    DespeckleLaunch L = launch;
    if (L.width == 0 || L.height == 0) return PYR_OK;
    if (L.radius < 1 || L.radius > kDespeckleMostRadius) return fail(PYR_ERR_INVALID_ARGUMENT, "despeckle: radius out of range"); // the LDS tile is sized by it
    L.tiles_x = (L.width - 1) / kDespeckleTile + 1; // no wrap at the widest image
    const uint64_t tiles = (uint64_t)L.tiles_x * ((L.height - 1) / kDespeckleTile + 1);
    if (tiles > 0x7FFFFFFFull) return fail(PYR_ERR_UNSUPPORTED, "despeckle: more tiles than a grid holds");
    if (L.counts && hipMemsetAsync(L.counts, 0, 2 * sizeof(uint32_t), (hipStream_t)stream) != hipSuccess) return fail(PYR_ERR_DEVICE, "despeckle: hipMemsetAsync of the counts failed");
    if (L.radius == 1)
        hipLaunchKernelGGL(despeckle_kernel<1>, dim3((uint32_t)tiles), dim3(TILE_BLOCK), 0, (hipStream_t)stream, L);
    else
        hipLaunchKernelGGL(despeckle_kernel<2>, dim3((uint32_t)tiles), dim3(TILE_BLOCK), 0, (hipStream_t)stream, L);
    return launched("despeckle");
}

} // namespace pyr
