// tone.hip -- the film as an image in linear light, and what follows it, a unit of its own: development to
// three f32 per pixel (XYZ or linear sRGB), the luminance statistics of such an image, and its tone mapping to 8-bit sRGB.
// Nothing here touches the render kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../api_internal.h"
#include "../device_scene.h"

namespace pyr {

namespace {
constexpr uint32_t WAVE = 64;
constexpr uint32_t PIXEL_BLOCK = 256;
constexpr uint32_t STATS_BLOCK = 256;
constexpr uint32_t TONE_BLOCK = 256;

__device__ __forceinline__ float develop_grain(float acc, float weight) { return weight > 0.0f ? acc / weight : 0.0f; } // Grain::develop, film.rs:132-143

// spectrum_to_xyz (main.rs:352-418) of one pixel, develop_kernel's operations in develop_kernel's order (kernels/main.hip) up to
// the point where the 8-bit kernels clamp: `bin(index)` is the pixel's developed grain. Both forms below walk through here.
template <class Bin>
__device__ __forceinline__ void develop_walk(const DevelopLaunch& D, Bin bin, float xyz[3], float rgb[3]) {
    const uint32_t bins = D.film.bins;
    const float min = D.film.wl_start, max = D.film.wl_start + D.film.wl_width;
    auto xyz_get = [&](int channel, float w) {
        const float* d = D.xyz_table;
        const uint32_t n = D.xyz_count;
        if (w <= D.xyz_min) return d[channel];
        if (w >= D.xyz_max) return d[3 * (n - 1) + channel];
        float normalized = (w - D.xyz_min) / (D.xyz_max - D.xyz_min);
        float fi = normalized * ((float)n - 1.0f);
        float fmin_ = truncf(fi);
        uint32_t i0 = (uint32_t)fmin_;
        float mix = fi - fmin_;
        return d[3 * i0 + channel] * (1.0f - mix) + d[3 * (i0 + 1) + channel] * mix;
    };
    auto sample = [&](float w, uint32_t i) {
        float intensity;
        if (w < min || w > max) {
            intensity = 0.0f;
        } else {
            float normalized = (w - min) / (max - min);
            float float_index = normalized * (float)bins;
            uint32_t index = (uint32_t)fminf(floorf(float_index), (float)(bins - 1));
            intensity = bin(index);
        }
        if (D.filter) intensity = intensity * D.filter[i];
        if (D.white_div) intensity = (intensity / D.white_div[i]) * D.white_mul[i];
        return intensity;
    };
    float sum[3] = {0, 0, 0}, weight = 0.0f;
    float wl_min = min;
    uint32_t i = 0;
    float spectrum_min = sample(wl_min, i);
    float start[3] = {xyz_get(0, wl_min), xyz_get(1, wl_min), xyz_get(2, wl_min)};
    while (wl_min < max) {
        float wl_max = wl_min + D.step_size;
        i += 1;
        float spectrum_max = sample(wl_max, i < D.sample_count ? i : D.sample_count - 1);
        float end[3] = {xyz_get(0, wl_max), xyz_get(1, wl_max), xyz_get(2, wl_max)};
        float w = wl_max - wl_min;
        for (int c = 0; c < 3; ++c) sum[c] += (start[c] * spectrum_min + end[c] * spectrum_max) * 0.5f * w;
        weight += w;
        wl_min = wl_max;
        spectrum_min = spectrum_max;
        for (int c = 0; c < 3; ++c) start[c] = end[c];
    }
    for (int c = 0; c < 3; ++c) xyz[c] = (weight == 0.0f ? sum[c] : sum[c] / weight) * D.xyz_scale;
    rgb[0] = 3.2404542f * xyz[0] + -1.5371385f * xyz[1] + -0.4985314f * xyz[2];
    rgb[1] = -0.9692660f * xyz[0] + 1.8760108f * xyz[1] + 0.0415560f * xyz[2];
    rgb[2] = 0.0556434f * xyz[0] + -0.2040259f * xyz[1] + 1.0572252f * xyz[2];
}

// The sRGB encoding of develop_kernel: a linear value already inside [0, 1] -> a byte.
__device__ __forceinline__ uint8_t encode_srgb(float v) {
    float e = v <= 0.0031308f ? 12.92f * v : 1.055f * (float)pow((double)v, 1.0 / 2.4) - 0.055f;
    e = fminf(fmaxf(e, 0.0f), 1.0f);
    return (uint8_t)(e * 255.0f + 0.5f);
}

__device__ __forceinline__ float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
} // namespace

// ------------------------------------------------------------------------------------------------ linear development, wave per pixel run
// develop_wave_kernel's shape (kernels/film.hip): a workgroup is ONE wave and takes runs of 64 consecutive pixels, the run's grains
// go through LDS as quotients acc / weight (of A + B with two half films), row p of pixel p, rows bins + 1 floats apart, and lane p
// walks pixel p. What the lane holds then -- xyz[] after xyz_scale or rgb[] before the clamp -- is three f32 of a run whose
// 64 * 3 floats are contiguous in the image: the lanes put them at floats 3p .. 3p + 2 of the LDS the walk has finished with (stride
// 3 is odd: no two lanes of a pass share a bank) and 48 lanes store 16 B apiece, 768 B in one wave instruction. The ragged last run
// and an image that is not 16-byte aligned go out dword by dword, still from LDS and still coalesced.
// LDS: 64 * (bins + 1) * 4 B per wave, at least the 768 B of the staged run.
__global__ __launch_bounds__(WAVE) void develop_linear_kernel(LinearLaunch L) {
    extern __shared__ __attribute__((aligned(16))) float spectrum[]; // [64][bins + 1], then [64][3]
    const DevelopLaunch& D = L.develop;
    const size_t pixels = (size_t)D.film.width * D.film.height;
    const uint32_t bins = D.film.bins, row = bins + 1u, lane = threadIdx.x;
    const size_t runs = (pixels + WAVE - 1) / WAVE;
    const uint32_t step_p = (2u * WAVE) / bins, step_b = (2u * WAVE) % bins; // what 128 grains further means in (pixel, bin)
    const bool aligned = (reinterpret_cast<uintptr_t>(L.out) & 15u) == 0;
    for (size_t run = blockIdx.x; run < runs; run += gridDim.x) {
        const size_t base = run * WAVE;
        const uint32_t np = (uint32_t)std::min<size_t>(WAVE, pixels - base);
        const uint32_t n = np * bins, pairs = n / 2u; // grains of the run; base * bins is even, so every pair is 16-byte aligned
        const float4* a4 = reinterpret_cast<const float4*>(D.grains + base * bins);
        const float4* b4 = D.grains_b ? reinterpret_cast<const float4*>(D.grains_b + base * bins) : nullptr;
        uint32_t p = (2u * lane) / bins, b = (2u * lane) % bins;
        for (uint32_t q = lane; q < pairs; q += WAVE) {
            float4 g = a4[q];
            if (b4) {
                const float4 h = b4[q];
                g.x += h.x, g.y += h.y, g.z += h.z, g.w += h.w;
            }
            spectrum[p * row + b] = develop_grain(g.x, g.y);
            uint32_t p1 = p, b1 = b + 1u;
            if (b1 == bins) b1 = 0u, p1 += 1u;
            spectrum[p1 * row + b1] = develop_grain(g.z, g.w);
            p += step_p, b += step_b;
            if (b >= bins) b -= bins, p += 1u;
        }
        if ((n & 1u) && lane == 0) { // odd bins and an odd number of pixels: the run's last grain
            PyrGrain g = D.grains[base * bins + n - 1u];
            if (D.grains_b) {
                const PyrGrain h = D.grains_b[base * bins + n - 1u];
                g.acc += h.acc, g.weight += h.weight;
            }
            spectrum[(np - 1u) * row + bins - 1u] = develop_grain(g.acc, g.weight);
        }
        __syncthreads();
        float value[3] = {0.0f, 0.0f, 0.0f};
        if (lane < np && base + lane + 1 < pixels) { // the last pixel stays black: film.rs:299
            const float* g = spectrum + lane * row;
            float xyz[3], rgb[3];
            develop_walk(D, [&](uint32_t index) { return g[index]; }, xyz, rgb);
            for (int c = 0; c < 3; ++c) value[c] = L.space == PYR_LINEAR_XYZ ? xyz[c] : rgb[c];
        }
        __syncthreads(); // every row has been read: the run's image floats take their place
        for (int c = 0; c < 3; ++c) spectrum[3u * lane + c] = value[c];
        __syncthreads();
        float* out = L.out + base * 3u;
        if (np == WAVE && aligned) {
            if (lane < 3u * WAVE / 4u) reinterpret_cast<float4*>(out)[lane] = reinterpret_cast<const float4*>(spectrum)[lane];
        } else {
            for (uint32_t k = lane; k < 3u * np; k += WAVE) out[k] = spectrum[k];
        }
        __syncthreads(); // the next run overwrites the rows
    }
}

// The same walk for films of more bins than the LDS rows hold: one thread per pixel, the grains read where they lie.
__global__ __launch_bounds__(PIXEL_BLOCK) void develop_linear_pixel_kernel(LinearLaunch L) {
    const DevelopLaunch& D = L.develop;
    const size_t pixels = (size_t)D.film.width * D.film.height;
    const uint32_t bins = D.film.bins;
    for (size_t px = (size_t)blockIdx.x * PIXEL_BLOCK + threadIdx.x; px < pixels; px += (size_t)gridDim.x * PIXEL_BLOCK) {
        float value[3] = {0.0f, 0.0f, 0.0f};
        if (px + 1 < pixels) {
            const PyrGrain* ga = D.grains + px * bins;
            const PyrGrain* gb = D.grains_b ? D.grains_b + px * bins : nullptr;
            float xyz[3], rgb[3];
            develop_walk(
                D,
                [&](uint32_t index) {
                    PyrGrain g = ga[index];
                    if (gb) g.acc += gb[index].acc, g.weight += gb[index].weight;
                    return develop_grain(g.acc, g.weight);
                },
                xyz, rgb);
            for (int c = 0; c < 3; ++c) value[c] = L.space == PYR_LINEAR_XYZ ? xyz[c] : rgb[c];
        }
        for (int c = 0; c < 3; ++c) L.out[3 * px + c] = value[c];
    }
}

int launch_develop_linear(const LinearLaunch& launch, void* stream) {
    const DevelopLaunch& D = launch.develop;
    const size_t pixels = (size_t)D.film.width * D.film.height;
    if (pixels == 0) return PYR_OK;
    if (D.film.bins >= 1u && D.film.bins <= kWaveDevelopMaxBins) {
        const size_t lds = (size_t)WAVE * std::max(D.film.bins + 1u, 3u) * sizeof(float);
        const uint32_t grid = (uint32_t)std::min<size_t>((pixels + WAVE - 1) / WAVE, 256 * 32);
        hipLaunchKernelGGL(develop_linear_kernel, dim3(grid), dim3(WAVE), lds, (hipStream_t)stream, launch);
    } else {
        const uint32_t grid = (uint32_t)std::min<size_t>((pixels + PIXEL_BLOCK - 1) / PIXEL_BLOCK, 256 * 16);
        hipLaunchKernelGGL(develop_linear_pixel_kernel, dim3(grid), dim3(PIXEL_BLOCK), 0, (hipStream_t)stream, launch);
    }
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("linear develop kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

// ------------------------------------------------------------------------------------------------ luminance statistics
// Every counter is a uint32 and every fold an integer add, max or min: the sums commute, two calls give the same bits. A workgroup
// keeps the 256 bins in LDS (ds atomics), every thread its own lit / dark counts and extremes in registers; at the end the workgroup
// folds what it holds into the one record in global memory with integer atomics, a bin it never touched costs nothing.
// Four pixels are 48 B = three 16-byte loads of a lane; the tail, and an image that is not 16-byte aligned, go pixel by pixel.
// `min_lit` travels as the complement of its bits, so that the record starts as all zeros and one atomicMax serves both extremes;
// image_stats_finish_kernel turns it back (and leaves 0.0f when nothing is lit).
struct StatsAcc {
    uint32_t lit = 0, dark = 0, lo = 0xFFFFFFFFu, hi = 0;
};
__device__ __forceinline__ void stats_pixel(float r, float g, float b, uint32_t* bins, StatsAcc& acc) {
    const float y = luminance(r, g, b);
    if (y > 0.0f) {
        const uint32_t bits = __float_as_uint(y);
        const int bin = std::min(std::max((int)(bits >> 20) - 888, 0), 255);
        atomicAdd(&bins[bin], 1u);
        acc.lit += 1u;
        acc.lo = std::min(acc.lo, bits), acc.hi = std::max(acc.hi, bits);
    } else {
        acc.dark += 1u;
    }
}

__global__ __launch_bounds__(STATS_BLOCK) void image_stats_kernel(const float* image, size_t pixels, PyrImageStats* out) {
    __shared__ uint32_t bins[256];
    __shared__ uint32_t folded[4]; // lit, dark, ~min bits, max bits
    bins[threadIdx.x] = 0u;
    if (threadIdx.x < 4) folded[threadIdx.x] = 0u;
    __syncthreads();
    StatsAcc acc;
    const size_t thread = (size_t)blockIdx.x * STATS_BLOCK + threadIdx.x, threads = (size_t)gridDim.x * STATS_BLOCK;
    const size_t quads = (reinterpret_cast<uintptr_t>(image) & 15u) == 0 ? pixels / 4 : 0;
    const float4* image4 = reinterpret_cast<const float4*>(image);
    for (size_t q = thread; q < quads; q += threads) {
        const float4 a = image4[3 * q], b = image4[3 * q + 1], c = image4[3 * q + 2];
        stats_pixel(a.x, a.y, a.z, bins, acc);
        stats_pixel(a.w, b.x, b.y, bins, acc);
        stats_pixel(b.z, b.w, c.x, bins, acc);
        stats_pixel(c.y, c.z, c.w, bins, acc);
    }
    for (size_t px = 4 * quads + thread; px < pixels; px += threads) stats_pixel(image[3 * px], image[3 * px + 1], image[3 * px + 2], bins, acc);
    if (acc.lit) {
        atomicAdd(&folded[0], acc.lit);
        atomicMax(&folded[2], ~acc.lo);
        atomicMax(&folded[3], acc.hi);
    }
    if (acc.dark) atomicAdd(&folded[1], acc.dark);
    __syncthreads();
    if (bins[threadIdx.x]) atomicAdd(&out->histogram[threadIdx.x], bins[threadIdx.x]);
    if (threadIdx.x == 0) {
        if (folded[0]) {
            atomicAdd(&out->lit, folded[0]);
            atomicMax(reinterpret_cast<uint32_t*>(&out->min_lit), folded[2]);
            atomicMax(reinterpret_cast<uint32_t*>(&out->max_lit), folded[3]);
        }
        if (folded[1]) atomicAdd(&out->dark, folded[1]);
    }
}

__global__ void image_stats_finish_kernel(PyrImageStats* out) {
    uint32_t* lo = reinterpret_cast<uint32_t*>(&out->min_lit);
    *lo = out->lit ? ~*lo : 0u;
}

int launch_image_stats(const float* image, size_t pixels, PyrImageStats* out, void* stream) {
    hipError_t err = hipMemsetAsync(out, 0, sizeof(PyrImageStats), (hipStream_t)stream);
    if (err == hipSuccess && pixels != 0) {
        // a thread takes four pixels a turn; enough workgroups to fill the device, few enough that the final fold stays small
        const uint32_t grid = (uint32_t)std::min<size_t>((pixels + 4 * STATS_BLOCK - 1) / (4 * STATS_BLOCK), 256 * 8);
        hipLaunchKernelGGL(image_stats_kernel, dim3(grid), dim3(STATS_BLOCK), 0, (hipStream_t)stream, image, pixels, out);
        hipLaunchKernelGGL(image_stats_finish_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, out);
        err = hipGetLastError();
    }
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("image stats kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

// ------------------------------------------------------------------------------------------------ tone mapping
// include/pyrite_gpu.h spells the f32 operations out; clamp(x) is fminf(fmaxf(x, 0), 1), which turns a NaN into 0.
// Four pixels a thread where the buffers allow it: three 16-byte loads, three 4-byte stores of packed bytes.
__device__ __forceinline__ void tone_pixel(float r, float g, float b, const ToneLaunch& T, uint8_t out[3]) {
    float v[3] = {T.exposure * r, T.exposure * g, T.exposure * b};
    if (T.op == PYR_TONE_REINHARD) {
        const float y = luminance(r, g, b);
        if (!(y > 0.0f)) {
            out[0] = out[1] = out[2] = 0;
            return;
        }
        const float l = T.exposure * y;
        const float ld = (l * (1.0f + l / (T.white * T.white))) / (1.0f + l);
        const float scale = ld / l;
        for (int c = 0; c < 3; ++c) v[c] = v[c] * scale;
    }
    for (int c = 0; c < 3; ++c) out[c] = encode_srgb(fminf(fmaxf(v[c], 0.0f), 1.0f));
}

__global__ __launch_bounds__(TONE_BLOCK) void tonemap_kernel(ToneLaunch T) {
    const size_t thread = (size_t)blockIdx.x * TONE_BLOCK + threadIdx.x, threads = (size_t)gridDim.x * TONE_BLOCK;
    const bool aligned = (reinterpret_cast<uintptr_t>(T.image) & 15u) == 0 && (reinterpret_cast<uintptr_t>(T.rgb_out) & 3u) == 0;
    const size_t quads = aligned ? T.pixels / 4 : 0;
    const float4* image4 = reinterpret_cast<const float4*>(T.image);
    uint32_t* out4 = reinterpret_cast<uint32_t*>(T.rgb_out);
    for (size_t q = thread; q < quads; q += threads) {
        const float4 a = image4[3 * q], b = image4[3 * q + 1], c = image4[3 * q + 2];
        uint8_t px[12];
        tone_pixel(a.x, a.y, a.z, T, px);
        tone_pixel(a.w, b.x, b.y, T, px + 3);
        tone_pixel(b.z, b.w, c.x, T, px + 6);
        tone_pixel(c.y, c.z, c.w, T, px + 9);
        for (int k = 0; k < 3; ++k)
            out4[3 * q + k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    }
    for (size_t i = 4 * quads + thread; i < T.pixels; i += threads) {
        uint8_t px[3];
        tone_pixel(T.image[3 * i], T.image[3 * i + 1], T.image[3 * i + 2], T, px);
        for (int c = 0; c < 3; ++c) T.rgb_out[3 * i + c] = px[c];
    }
}

int launch_tonemap(const ToneLaunch& launch, void* stream) {
    if (launch.pixels == 0) return PYR_OK;
    const uint32_t grid = (uint32_t)std::min<size_t>((launch.pixels + 4 * TONE_BLOCK - 1) / (4 * TONE_BLOCK), 256 * 16);
    hipLaunchKernelGGL(tonemap_kernel, dim3(grid), dim3(TONE_BLOCK), 0, (hipStream_t)stream, launch);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("tonemap kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

} // namespace pyr
