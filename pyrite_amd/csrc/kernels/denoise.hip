// denoise.hip -- the cross filter of two developed half images, a unit of its own: include/pyrite_gpu.h spells
// the f32 operations and their order out, the kernels keep both. Nothing here touches the render, film, feature or tone kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../api_internal.h"
#include "../device_scene.h"
#include "denoise_tile.h"

namespace pyr {

namespace {
constexpr uint32_t PIXEL_BLOCK = 256;
constexpr uint32_t TILE_BLOCK = kDenoiseTile * kDenoiseTile;

int launched(const char* what) {
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess) return PYR_OK;
    return fail(PYR_ERR_DEVICE, std::string(what) + " kernel launch: " + hipGetErrorString(err));
}
} // namespace

// ------------------------------------------------------------------------------------------------ the variance of one half
// V_c(p) = 0.5f * (sum of (a_c - b_c)^2 over p's 3 x 3 neighbourhood clipped to the image, raster order, / the pixels summed); NaN
// where that is +inf.
// One thread per pixel, the neighbours through the cache: 54 loads a pixel against the thousands of operations of the filter.
__global__ __launch_bounds__(PIXEL_BLOCK) void denoise_variance_kernel(const float* a, const float* b, uint32_t width, uint32_t height, float* variance) {
    const size_t pixels = (size_t)width * height;
    for (size_t px = (size_t)blockIdx.x * PIXEL_BLOCK + threadIdx.x; px < pixels; px += (size_t)gridDim.x * PIXEL_BLOCK) {
        const uint32_t x = (uint32_t)(px % width), y = (uint32_t)(px / width);
        const uint32_t y_lo = y > 0 ? y - 1 : 0, y_hi = y + 1 < height ? y + 1 : height - 1;
        const uint32_t x_lo = x > 0 ? x - 1 : 0, x_hi = x + 1 < width ? x + 1 : width - 1;
        float sum[3] = {0.0f, 0.0f, 0.0f};
        for (uint32_t ny = y_lo; ny <= y_hi; ++ny)
            for (uint32_t nx = x_lo; nx <= x_hi; ++nx) {
                const size_t q = (size_t)ny * width + nx;
                for (int c = 0; c < 3; ++c) {
                    const float d = a[3 * q + c] - b[3 * q + c];
                    sum[c] = sum[c] + d * d;
                }
            }
        const float count = (float)((y_hi - y_lo + 1) * (x_hi - x_lo + 1));
        for (int c = 0; c < 3; ++c) {
            const float v = 0.5f * (sum[c] / count);
            variance[3 * px + c] = v == INFINITY ? NAN : v; // an infinite pixel poisons its neighbourhood as a NaN one does
        }
    }
}

// ------------------------------------------------------------------------------------------------ one half filtered by the other's weights
// A workgroup owns a 16 x 16 tile and stages {H, V} of the tile and its halo of radius + patch pixels in LDS, a plane per channel
// (denoise_tile.h: the addressing and its banking); cells that stand for no pixel hold zeros and are never read, the skip rule of
// the colour distance -- p + t or q + t outside the image -- is DenoiseCell::inside of the same function. Then a thread owns a pixel:
// it walks the window in raster order, the patch in raster order inside it, the channels innermost, with one IEEE division a term, and
// sums the half being averaged through the cache (one pixel per window offset, and the guides likewise). No atomics, plain stores.
// LDS: (16 + 2 * halo) * 48 * 3 * 8 B: 32,256 B at (radius, patch) = (5, 1), 48,384 B at (10, 3).
__global__ __launch_bounds__(TILE_BLOCK) void denoise_filter_kernel(DenoiseLaunch L) {
    extern __shared__ __attribute__((aligned(16))) float2 hv[]; // [3][rows][kDenoisePitch] of {H, V}
    const uint32_t halo = L.radius + L.patch, rows = denoise_tile_rows(halo), plane = denoise_plane_cells(halo);
    const uint32_t tile_x = blockIdx.x % L.tiles_x, tile_y = blockIdx.x / L.tiles_x;
    const uint32_t x0 = tile_x * kDenoiseTile, y0 = tile_y * kDenoiseTile;
    for (uint32_t k = threadIdx.x; k < rows * rows; k += TILE_BLOCK) {
        const int32_t lx = (int32_t)(k % rows) - (int32_t)halo, ly = (int32_t)(k / rows) - (int32_t)halo;
        const DenoiseCell cell = denoise_cell(L.width, L.height, x0, y0, halo, lx, ly);
        for (uint32_t c = 0; c < 3; ++c)
            hv[c * plane + cell.lds] = cell.inside ? make_float2(L.weights_from[3 * cell.pixel + c], L.variance[3 * cell.pixel + c]) : make_float2(0.0f, 0.0f);
    }
    __syncthreads(); // the only barrier: threads outside the image leave after it
    const int32_t lx = (int32_t)(threadIdx.x % kDenoiseTile), ly = (int32_t)(threadIdx.x / kDenoiseTile);
    const DenoiseCell self = denoise_cell(L.width, L.height, x0, y0, halo, lx, ly);
    if (!self.inside) return;
    const size_t p = self.pixel;
    const int32_t radius = (int32_t)L.radius, patch = (int32_t)L.patch;
    float albedo_p[3] = {0.0f, 0.0f, 0.0f}, normal_p[3] = {0.0f, 0.0f, 0.0f}, depth_p = 0.0f;
    if (L.albedo)
        for (int c = 0; c < 3; ++c) albedo_p[c] = L.albedo[3 * p + c];
    if (L.pixels) {
        for (int c = 0; c < 3; ++c) normal_p[c] = L.pixels[p].normal[c];
        depth_p = L.pixels[p].depth;
    }
    float num[3] = {0.0f, 0.0f, 0.0f}, den = 0.0f;
    for (int32_t oy = -radius; oy <= radius; ++oy)
        for (int32_t ox = -radius; ox <= radius; ++ox) {
            const DenoiseCell q = denoise_cell(L.width, L.height, x0, y0, halo, lx + ox, ly + oy);
            if (!q.inside) continue;
            float w = 1.0f; // o = 0 by definition
            if (ox != 0 || oy != 0) {
                float S = 0.0f;
                uint32_t n = 0;
                for (int32_t dy = -patch; dy <= patch; ++dy)
                    for (int32_t dx = -patch; dx <= patch; ++dx) {
                        const DenoiseCell pt = denoise_cell(L.width, L.height, x0, y0, halo, lx + dx, ly + dy);
                        const DenoiseCell qt = denoise_cell(L.width, L.height, x0, y0, halo, lx + ox + dx, ly + oy + dy);
                        if (!pt.inside || !qt.inside) continue;
                        n += 1;
                        for (uint32_t c = 0; c < 3; ++c) {
                            const float2 a = hv[c * plane + pt.lds], b = hv[c * plane + qt.lds];
                            const float d = a.x - b.x;
                            S = S + (d * d - (a.y + fminf(a.y, b.y))) / (L.epsilon + L.kk * (a.y + b.y));
                        }
                    }
                float D = S / (3.0f * (float)n); // n >= 1: t = 0 is always kept
                bool nan = D != D;
                D = fmaxf(D, 0.0f);
                if (L.albedo && L.albedo_div > 0.0f) {
                    float g = 0.0f;
                    for (int c = 0; c < 3; ++c) {
                        const float d = albedo_p[c] - L.albedo[3 * q.pixel + c];
                        g = g + d * d;
                    }
                    g = g / L.albedo_div;
                    nan = nan || g != g;
                    D = fmaxf(D, g);
                }
                if (L.pixels && L.normal_div > 0.0f) {
                    float g = 0.0f;
                    for (int c = 0; c < 3; ++c) {
                        const float d = normal_p[c] - L.pixels[q.pixel].normal[c];
                        g = g + d * d;
                    }
                    g = g / L.normal_div;
                    nan = nan || g != g;
                    D = fmaxf(D, g);
                }
                if (L.pixels && L.depth_div > 0.0f) {
                    const float depth_q = L.pixels[q.pixel].depth;
                    const float m = fmaxf(fmaxf(depth_p, depth_q), 1e-30f);
                    const float r = (depth_p - depth_q) / m;
                    const float g = (r * r) / L.depth_div;
                    nan = nan || g != g;
                    D = fmaxf(D, g);
                }
                w = nan ? 0.0f : expf(-D);
            }
            if (w > 0.0f) { // a weight of 0 adds nothing: 0 * NaN would be NaN
                for (int c = 0; c < 3; ++c) num[c] = num[c] + w * L.averaged[3 * q.pixel + c];
                den = den + w;
            }
        }
    for (int c = 0; c < 3; ++c) L.out[3 * p + c] = num[c] / den;
}

// out = (FA + FB) * 0.5f, error_out = fabsf(FA - FB) * 0.5f
__global__ __launch_bounds__(PIXEL_BLOCK) void denoise_combine_kernel(const float* fa, const float* fb, size_t floats, float* out, float* error_out) {
    for (size_t i = (size_t)blockIdx.x * PIXEL_BLOCK + threadIdx.x; i < floats; i += (size_t)gridDim.x * PIXEL_BLOCK) {
        const float a = fa[i], b = fb[i];
        out[i] = (a + b) * 0.5f;
        if (error_out) error_out[i] = fabsf(a - b) * 0.5f;
    }
}

int launch_denoise_variance(const float* a, const float* b, uint32_t width, uint32_t height, float* variance, void* stream) {
    const size_t pixels = (size_t)width * height;
    if (pixels == 0) return PYR_OK;
    const uint32_t grid = (uint32_t)std::min<size_t>((pixels + PIXEL_BLOCK - 1) / PIXEL_BLOCK, 256 * 16);
    hipLaunchKernelGGL(denoise_variance_kernel, dim3(grid), dim3(PIXEL_BLOCK), 0, (hipStream_t)stream, a, b, width, height, variance);
    return launched("denoise variance");
}

int launch_denoise_filter(const DenoiseLaunch& launch, void* stream) {
    DenoiseLaunch L = launch;
    if (L.width == 0 || L.height == 0) return PYR_OK;
    if (L.radius < 1 || L.radius > kDenoiseMaxRadius || L.patch > kDenoiseMaxPatch) // the LDS tile is sized by these
        return fail(PYR_ERR_INVALID_ARGUMENT, "denoise filter: radius or patch out of range");
    L.tiles_x = (L.width + kDenoiseTile - 1) / kDenoiseTile;
    const uint64_t tiles = (uint64_t)L.tiles_x * ((L.height + kDenoiseTile - 1) / kDenoiseTile);
    if (tiles > 0x7FFFFFFFull) return fail(PYR_ERR_UNSUPPORTED, "denoise filter: more tiles than a grid holds");
    const size_t lds = (size_t)3 * denoise_plane_cells(L.radius + L.patch) * sizeof(float2);
    hipLaunchKernelGGL(denoise_filter_kernel, dim3((uint32_t)tiles), dim3(TILE_BLOCK), lds, (hipStream_t)stream, L);
    return launched("denoise filter");
}

int launch_denoise_combine(const float* fa, const float* fb, size_t pixels, float* out, float* error_out, void* stream) {
    if (pixels == 0) return PYR_OK;
    const size_t floats = 3 * pixels;
    const uint32_t grid = (uint32_t)std::min<size_t>((floats + PIXEL_BLOCK - 1) / PIXEL_BLOCK, 256 * 16);
    hipLaunchKernelGGL(denoise_combine_kernel, dim3(grid), dim3(PIXEL_BLOCK), 0, (hipStream_t)stream, fa, fb, floats, out, error_out);
    return launched("denoise combine");
}

} // namespace pyr
