// film.hip -- the kernels of a progressive session's film, a unit of its own: film development shaped for
// the film's layout, the sum of two half films, and the per-tile noise estimate from them. Nothing here touches the render kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../api_internal.h"
#include "../device_scene.h"

namespace pyr {

namespace {
constexpr uint32_t WAVE = 64;
constexpr uint32_t NOISE_BLOCK = 256;

__device__ __forceinline__ float develop_grain(float acc, float weight) { return weight > 0.0f ? acc / weight : 0.0f; } // Grain::develop, film.rs:132-143
} // namespace

// ------------------------------------------------------------------------------------------------ film development, wave per pixel run
// The film is pixel-major, `bins` grains of 8 B per pixel. A workgroup is ONE wave and takes runs of 64 consecutive pixels:
//   1. the run's grains are one contiguous span of 64 * bins * 8 B; the lanes walk it two grains (16 B) apiece, 1 KB per wave
//      instruction, whatever `bins` is. acc / weight is formed per grain right there -- of A + B when there are two half films,
//      accs added and weights added -- and the quotient (4 B) goes to LDS, row p of pixel p, rows bins + 1 floats apart: in
//      step 2 all lanes read the same bin of their own pixel, and the odd stride spreads those 64 reads over the banks;
//   2. lane p walks pixel p's trapezoid rule out of LDS with develop_kernel's operations in develop_kernel's order
//      (kernels/main.hip), so the bytes are the same. The per-wavelength tables are wave-uniform reads.
// LDS: 64 * (bins + 1) * 4 B per wave, 16.6 KB at the contract's 64 bins (nine waves a CU); launch_develop keeps films of
// more than kWaveDevelopMaxBins bins on develop_kernel.
__global__ __launch_bounds__(WAVE) void develop_wave_kernel(DevelopLaunch D) {
    extern __shared__ __attribute__((aligned(16))) float spectrum[]; // [64][bins + 1]
    const size_t pixels = (size_t)D.film.width * D.film.height;
    const uint32_t bins = D.film.bins, row = bins + 1u, lane = threadIdx.x;
    const float min = D.film.wl_start, max = D.film.wl_start + D.film.wl_width;
    const size_t runs = (pixels + WAVE - 1) / WAVE;
    const uint32_t step_p = (2u * WAVE) / bins, step_b = (2u * WAVE) % bins; // what 128 grains further means in (pixel, bin)
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
        const size_t px = base + lane;
        if (lane < np) {
            uint8_t out[3] = {0, 0, 0};
            if (px + 1 < pixels) { // the last pixel stays black: film.rs:299
                const float* g = spectrum + lane * row;
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
                        intensity = g[index];
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
                float xyz[3];
                for (int c = 0; c < 3; ++c) xyz[c] = (weight == 0.0f ? sum[c] : sum[c] / weight) * D.xyz_scale;
                const float rgb[3] = {3.2404542f * xyz[0] + -1.5371385f * xyz[1] + -0.4985314f * xyz[2],
                                      -0.9692660f * xyz[0] + 1.8760108f * xyz[1] + 0.0415560f * xyz[2],
                                      0.0556434f * xyz[0] + -0.2040259f * xyz[1] + 1.0572252f * xyz[2]};
                for (int c = 0; c < 3; ++c) {
                    float v = fminf(fmaxf(rgb[c], 0.0f), 1.0f);
                    float e = v <= 0.0031308f ? 12.92f * v : 1.055f * (float)pow((double)v, 1.0 / 2.4) - 0.055f;
                    e = fminf(fmaxf(e, 0.0f), 1.0f);
                    out[c] = (uint8_t)(e * 255.0f + 0.5f);
                }
            }
            D.rgb_out[3 * px + 0] = out[0];
            D.rgb_out[3 * px + 1] = out[1];
            D.rgb_out[3 * px + 2] = out[2];
        }
        __syncthreads(); // the next run overwrites the rows
    }
}

bool develop_wave_serves(const DevelopLaunch& launch) { return launch.film.bins >= 1u && launch.film.bins <= kWaveDevelopMaxBins; }

int launch_develop_wave(const DevelopLaunch& launch, void* stream) {
    const size_t pixels = (size_t)launch.film.width * launch.film.height;
    if (pixels == 0) return PYR_OK;
    if (!develop_wave_serves(launch)) return fail(PYR_ERR_UNSUPPORTED, "develop_wave_kernel: more bins than its LDS rows hold");
    const size_t lds = (size_t)WAVE * (launch.film.bins + 1u) * sizeof(float);
    const uint32_t grid = (uint32_t)std::min<size_t>((pixels + WAVE - 1) / WAVE, 256 * 32);
    hipLaunchKernelGGL(develop_wave_kernel, dim3(grid), dim3(WAVE), lds, (hipStream_t)stream, launch);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("develop kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

// ------------------------------------------------------------------------------------------------ A + B
// The film of a session with halves: accs added, weights added, grain by grain (two grains, 16 B, per lane and turn).
__global__ __launch_bounds__(256) void film_sum_kernel(const float2* a, const float2* b, float2* out, size_t grains) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < grains; i += (size_t)gridDim.x * 256) {
        const float2 x = a[i], y = b[i];
        out[i] = make_float2(x.x + y.x, x.y + y.y);
    }
}

int launch_film_sum(const PyrGrain* a, const PyrGrain* b, PyrGrain* out, size_t grains, void* stream) {
    if (grains == 0) return PYR_OK;
    const uint32_t grid = (uint32_t)std::min<size_t>((grains + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(film_sum_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float2*>(a), reinterpret_cast<const float2*>(b),
                       reinterpret_cast<float2*>(out), grains);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("film sum kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

// ------------------------------------------------------------------------------------------------ noise from two half films
// One workgroup per tile of the make_tiles grid, no atomics: every thread sums its grains of the tile in f64 in a fixed order,
// the wave folds its 64 sums with DPP-free shuffles in a fixed tree, the four wave sums meet in LDS and thread 0 adds them in
// order -- two runs give the same bits. A tile's pixel rows are contiguous spans of w * bins grains in both films: the threads
// walk a row side by side (8 B a lane, coalesced).
//   a, b = the f32 quotients acc / weight of the halves (0 where the weight is 0);  num = sum (a - b)^2, den = sum ((a + b) / 2)^2
// in f64;  out[tile] = (float)sqrt(num / den), 0 when den == 0.
__global__ __launch_bounds__(NOISE_BLOCK) void noise_kernel(NoiseLaunch N) {
    __shared__ double wave_num[NOISE_BLOCK / WAVE], wave_den[NOISE_BLOCK / WAVE];
    const uint32_t tile = blockIdx.x;
    const uint32_t ty = tile / N.tiles_x, tx = tile - ty * N.tiles_x;
    const uint32_t x0 = tx * N.tile_size, y0 = ty * N.tile_size;
    const uint32_t w = min(N.film.width - x0, N.tile_size), h = min(N.film.height - y0, N.tile_size);
    const uint32_t bins = N.film.bins;
    const uint64_t row_grains = (uint64_t)w * bins, total = row_grains * h;
    double num = 0.0, den = 0.0;
    for (uint64_t i = threadIdx.x; i < total; i += NOISE_BLOCK) {
        const uint32_t r = (uint32_t)(i / row_grains);
        const uint64_t in_row = i - (uint64_t)r * row_grains;
        const size_t at = ((size_t)(y0 + r) * N.film.width + x0) * bins + in_row;
        const PyrGrain ga = N.a[at], gb = N.b[at];
        const double a = (double)develop_grain(ga.acc, ga.weight), b = (double)develop_grain(gb.acc, gb.weight);
        const double d = a - b, m = (a + b) * 0.5;
        num += d * d;
        den += m * m;
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        num += __shfl_down(num, off, WAVE);
        den += __shfl_down(den, off, WAVE);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        wave_num[threadIdx.x / WAVE] = num;
        wave_den[threadIdx.x / WAVE] = den;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double n = 0.0, d = 0.0;
        for (uint32_t k = 0; k < NOISE_BLOCK / WAVE; ++k) n += wave_num[k], d += wave_den[k];
        N.out[tile] = d == 0.0 ? 0.0f : (float)sqrt(n / d);
    }
}

int launch_noise(const NoiseLaunch& launch, void* stream) {
    const uint32_t tiles = launch.tiles_x * launch.tiles_y;
    if (tiles == 0) return PYR_OK;
    hipLaunchKernelGGL(noise_kernel, dim3(tiles), dim3(NOISE_BLOCK), 0, (hipStream_t)stream, launch);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("noise kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

} // namespace pyr
