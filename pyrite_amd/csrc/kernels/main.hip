// main.hip -- the unit of every kernel but the interpreter builds of render_kernel_sm, and of every launcher.
#include "../kernels.hip"

#include "../api_internal.h"

namespace pyr {

// ------------------------------------------------------------------------------------------------ film development
// main.rs:315-327: every pixel spectrum -> spectrum_to_xyz (main.rs:352-418, trapezoid rule against the CIE observer
// tables) -> linear sRGB -> sRGB u8. One thread per pixel; the film is read once (bins * 8 B per pixel), HBM-bound.
// The last pixel is skipped as in DevelopedPixels::next (film.rs:299).
__global__ __launch_bounds__(BLOCK) void develop_kernel(DevelopLaunch D) {
    const size_t pixels = (size_t)D.film.width * D.film.height;
    const uint32_t bins = D.film.bins;
    const float min = D.film.wl_start, max = D.film.wl_start + D.film.wl_width;
    for (size_t px = (size_t)blockIdx.x * BLOCK + threadIdx.x; px < pixels; px += (size_t)gridDim.x * BLOCK) {
        uint8_t out[3] = {0, 0, 0};
        if ((px + 1) * bins < pixels * bins) {
            const PyrGrain* g = D.grains + px * bins;
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
                    const PyrGrain gr = g[index];
                    intensity = gr.weight > 0.0f ? gr.acc / gr.weight : 0.0f; // Grain::develop, film.rs:132-143
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
}

int launch_develop(const DevelopLaunch& launch, void* stream) {
    const size_t pixels = (size_t)launch.film.width * launch.film.height;
    if (pixels == 0) return PYR_OK;
    uint32_t grid = (uint32_t)std::min<size_t>((pixels + BLOCK - 1) / BLOCK, 256 * 16);
    hipLaunchKernelGGL(develop_kernel, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, launch);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("develop kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

// ------------------------------------------------------------------------------------------------ film blocks -> film
// Rank 0's side of the multi-GPU gather: the blocks a rank rendered (PYR_FILM_TILE_BLOCKS: the tile's pixels plus a ring of
// one pixel) are added into the whole-image film. The pixels of a tile belong to one block of the set only, so they are
// plain read-modify-writes, one grain (8 bytes) per thread, contiguous along a pixel row in both buffers: HBM-bound, two
// reads and one write of 8 B per grain. Ring pixels lie inside neighbouring tiles -- which may be in the same set -- so
// they go second, as atomics, and only where something was exposed (about one sample in 1e6 lands there).
__global__ __launch_bounds__(BLOCK) void assemble_interior_kernel(AssembleLaunch A) {
    const uint32_t ts = A.tile_size, side = ts + 2u, bins = A.film.bins;
    const uint64_t row_grains = (uint64_t)ts * bins, tile_grains = row_grains * ts, total = tile_grains * A.tile_count;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t k = (uint32_t)(i / tile_grains);
        const uint64_t r = i - (uint64_t)k * tile_grains;
        const uint32_t row = (uint32_t)(r / row_grains), in_row = (uint32_t)(r - (uint64_t)row * row_grains);
        const uint32_t col = in_row / bins, bin = in_row - col * bins;
        const uint32_t tile = A.tile_begin + k * A.tile_stride;
        const uint32_t ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
        const uint32_t x = tx * ts + col, y = ty * ts + row;
        if (x >= A.film.width || y >= A.film.height) continue; // a tile cut by the image border
        const PyrGrain g = A.blocks[(((size_t)k * side + row + 1u) * side + col + 1u) * bins + bin];
        PyrGrain* out = A.film_out + ((size_t)x + (size_t)y * A.film.width) * bins + bin;
        PyrGrain f = *out;
        f.acc += g.acc;
        f.weight += g.weight;
        *out = f;
    }
}
__global__ __launch_bounds__(BLOCK) void assemble_ring_kernel(AssembleLaunch A) {
    const uint32_t ts = A.tile_size, side = ts + 2u, bins = A.film.bins;
    const uint32_t ring = 4u * (ts + 1u); // pixels of the ring
    const uint64_t tile_grains = (uint64_t)ring * bins, total = tile_grains * A.tile_count;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t k = (uint32_t)(i / tile_grains);
        const uint32_t r = (uint32_t)(i - (uint64_t)k * tile_grains);
        const uint32_t q = r / bins, bin = r - q * bins;
        // ring pixel q: top row (side pixels), bottom row (side), then the left and right columns without their corners
        uint32_t bx, by;
        if (q < side)
            bx = q, by = 0u;
        else if (q < 2u * side)
            bx = q - side, by = side - 1u;
        else if (q < 2u * side + ts)
            bx = 0u, by = q - 2u * side + 1u;
        else
            bx = side - 1u, by = q - 2u * side - ts + 1u;
        const PyrGrain g = A.blocks[(((size_t)k * side + by) * side + bx) * bins + bin];
        if (g.acc == 0.0f && g.weight == 0.0f) continue;
        const uint32_t tile = A.tile_begin + k * A.tile_stride;
        const uint32_t ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
        const uint32_t x = tx * ts + bx - 1u, y = ty * ts + by - 1u; // wraps for the ring left of / above the image
        if (x >= A.film.width || y >= A.film.height) continue;
        float* out = reinterpret_cast<float*>(A.film_out + ((size_t)x + (size_t)y * A.film.width) * bins + bin);
        atomicAdd(out, g.acc);
        atomicAdd(out + 1, g.weight);
    }
}

int launch_assemble(const AssembleLaunch& launch, void* stream) {
    if (launch.tile_count == 0) return PYR_OK;
    const uint64_t interior = (uint64_t)launch.tile_size * launch.tile_size * launch.film.bins * launch.tile_count;
    const uint64_t ring = (uint64_t)4 * (launch.tile_size + 1) * launch.film.bins * launch.tile_count;
    const uint32_t grid_i = (uint32_t)std::min<uint64_t>((interior + BLOCK - 1) / BLOCK, 256 * 32);
    const uint32_t grid_r = (uint32_t)std::min<uint64_t>((ring + BLOCK - 1) / BLOCK, 256 * 32);
    hipLaunchKernelGGL(assemble_interior_kernel, dim3(grid_i), dim3(BLOCK), 0, (hipStream_t)stream, launch);
    hipLaunchKernelGGL(assemble_ring_kernel, dim3(grid_r), dim3(BLOCK), 0, (hipStream_t)stream, launch);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("assemble kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

// ------------------------------------------------------------------------------------------------ launchers
constexpr size_t kLdsSceneBytes = 8 * 1024; // nodes + primitives staged in LDS when they fit (C1, C2: < 3 KB)
static bool scene_fits_lds(const DevScene& scene) { return (size_t)scene.num_nodes * 64 + (size_t)scene.num_prims * 48 <= kLdsSceneBytes; }
// Levels of the traversal stack kept in LDS. The synchronous walk keeps the whole stack there (its scenes are shallow). The
// resumable walk spills deeper levels to scratch (TravStack) and keeps as many levels in LDS as still let `workgroups`
// workgroups share a CU's 160 KB next to `other_bytes` of LDS each -- on C3 the render runs at 103 / 135 / 160 Msamples/s
// with 2 / 3 / 4 workgroups per CU and did not care whether 4 or 12 levels are in LDS (an early round; today it does: 660 / 635 / 611 /
// 569 Msamples/s at 14 / 12 / 10 / 6 levels, profiles/r27_replay_pairs.txt -- a KB of LDS is a level). PYRITE_LDS_STACK overrides.
constexpr uint32_t kShortStackMax = 16;
static uint32_t short_stack_levels(const DevScene& scene, size_t other_bytes, uint32_t workgroups) {
    const char* e = std::getenv("PYRITE_LDS_STACK");
    uint32_t levels;
    if (e && *e) {
        levels = (uint32_t)std::strtoul(e, nullptr, 10);
    } else {
        const size_t budget = (160 * 1024) / std::max(workgroups, 1u);
        levels = budget > other_bytes ? (uint32_t)((budget - other_bytes) / (BLOCK * sizeof(int))) : 0u;
        levels = std::min(levels, kShortStackMax);
    }
    return std::max(1u, std::min(levels, scene.wide_nodes ? scene.wide_stack_depth : scene.stack_depth));
}
// Records a path can append: one MUL and one SCALE per bounce, light_samples ADDs in each of the two next-event estimations
// (tracer.rs:257), one closing ADD (emission or sky).
// A contribution whose colour program is HIT_RGB is four records (three coefficients and the factor).
uint32_t tape_ops_bound(const DevScene& scene, const RenderLaunch& launch) {
    return (launch.bounces + 2u * launch.light_samples + 1u) * (scene.micro_records ? 4u : 1u) + launch.bounces; // HIT_RGB: four records a contribution; PRODUCT: two to four
}
uint32_t tape_lanes_bound(int num_cus) { return (uint32_t)num_cus * 8u * BLOCK; } // launch_render never starts more than 8 blocks per CU
constexpr uint32_t kTapeProgramsLds = 128; // prepared programs kept in LDS for the replay (4 KB); scenes with more use the HBM records
static uint32_t tape_programs_in_lds(const DevScene& scene) { return scene.num_programs <= kTapeProgramsLds ? scene.num_programs : 0u; }
// Interpreter scenes record a tape when their colour programs allow it (DevScene::hit_tape) and there are wavelengths to share a
// hit's work among: with one or two per sample the online form wins (diamonds.lua, one wavelength, 256 bounces: 538 against 486).
static bool uses_hit_tape(const DevScene& scene, const RenderLaunch& launch) {
    static const char* const least = std::getenv("PYRITE_HIT_TAPE_WAVELENGTHS"); // development: the fewest wavelengths per sample a hit tape is recorded for
    return scene.needs_interpreter != 0 && scene.hit_tape != 0 && launch.spectrum_samples >= (least && *least ? (uint32_t)std::strtoul(least, nullptr, 10) : 4u);
}
// The tape a launch records, as PyrPathInfo::tape counts: 0 none, 1 the spectral tape of a scene without interpreter programs, 2 a hit tape.
uint32_t launch_tape(const DevScene& scene, const RenderLaunch& launch) {
    if (launch.scheduler != 1) return 0u;
    return scene.needs_interpreter == 0 ? 1u : uses_hit_tape(scene, launch) ? 2u : 0u;
}
static bool uses_tape(const DevScene& scene, const RenderLaunch& launch) { return launch_tape(scene, launch) != 0u; }
static size_t render_lds_bytes(const DevScene& scene, const RenderLaunch& launch) {
    const size_t spectral_rows = uses_tape(scene, launch) ? tape_spectral_rows(launch.spectrum_samples, scene.tape_value_rows, scene.needs_interpreter != 0) : 3 * launch.spectrum_samples;
    size_t bytes = (spectral_rows + launch.stack_lds) * BLOCK * sizeof(float);
    if (scene_fits_lds(scene)) bytes += (size_t)scene.num_nodes * 64 + (size_t)scene.num_prims * 48;
    bytes += (size_t)scene.lds_table_floats * sizeof(float);
    if (uses_tape(scene, launch)) bytes += ((size_t)tape_programs_in_lds(scene) * 8 + kTapeMaxValueRows) * sizeof(uint32_t) + tape_lane_list_bytes(scene.needs_interpreter != 0);
    return bytes;
}


// A scene staged in LDS never has its tables staged too (scene_pack.cpp pack_records: lds_table_floats is only set for scenes that do not live in
// LDS), so that combination is never instantiated.
static RenderKernel pick_kernel(bool sm, bool with_counters, bool interp, bool lds_scene, bool lds_tables, bool hit_tape, bool product, bool wide_vm) {
    if (interp && wide_vm) return pick_wide_kernel(with_counters, lds_scene, lds_tables);
    if (interp) return pick_interp_kernel(with_counters, lds_scene, lds_tables, hit_tape, product);
    auto pick = [&](auto counters) -> RenderKernel {
        constexpr bool C = decltype(counters)::value;
        if (lds_scene) return sm ? render_kernel_sm<C, false, true, false> : render_kernel<C, true, false>;
        if (sm) return lds_tables ? render_kernel_sm<C, false, false, true> : render_kernel_sm<C, false, false, false>;
        return lds_tables ? render_kernel<C, false, true> : render_kernel<C, false, false>;
    };
    return with_counters ? pick(std::true_type{}) : pick(std::false_type{});
}

bool scene_is_lds_resident(const DevScene& scene) { return scene_fits_lds(scene); }

int launch_render(const DevScene& scene, const RenderLaunch& launch_in, bool with_counters, void* stream, int num_cus, bool wide_vm) {
    if (scene.stack_depth > kMaxStackDepth) return fail(PYR_ERR_UNSUPPORTED, "BVH deeper than kMaxStackDepth");
    if (wide_vm && (launch_in.scheduler != 1 || scene.needs_interpreter == 0 || uses_tape(scene, launch_in)))
        return fail(PYR_ERR_INVALID_ARGUMENT, "the wide interpreter build runs the stage scheduler's online form only");
    RenderLaunch launch = launch_in;
    launch.stack_lds = 0;
    launch.tape_programs_lds = uses_tape(scene, launch) ? tape_programs_in_lds(scene) : 0u;
    launch.stack_lds = launch.scheduler == 1 ? short_stack_levels(scene, render_lds_bytes(scene, launch), (uint32_t)sm_waves(scene.needs_interpreter != 0))
                                             : scene.stack_depth;
    // a scene staged in LDS is a few dozen nodes: its whole stack is kept in LDS (the kernels built for such scenes have no
    // scratch part: TravStack::deep is one entry), whatever the budget or PYRITE_LDS_STACK say; the 160 KB check below applies
    if (scene_fits_lds(scene)) launch.stack_lds = std::max(launch.stack_lds, scene.stack_depth);
    const size_t lds = render_lds_bytes(scene, launch);
    if (lds > 160 * 1024) return fail(PYR_ERR_UNSUPPORTED, "spectrum_samples + BVH depth need more than 160 KB of LDS per workgroup");
    const uint32_t chunks = launch.chunk_end - launch.chunk_begin;
    if (chunks == 0) return PYR_OK;
    RenderKernel kernel = pick_kernel(launch.scheduler == 1, with_counters, scene.needs_interpreter != 0, scene_fits_lds(scene), scene.lds_table_floats != 0,
                                      launch.scheduler == 1 && uses_hit_tape(scene, launch), scene.product_records != 0, wide_vm);
    if (kernel == nullptr) return fail(PYR_ERR_UNSUPPORTED, "a program of this scene needs the wide interpreter build, which this one-unit build of the kernels does not hold");
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("hipFuncSetAttribute: ") + hipGetErrorString(err));
    // Residency of a 256-thread block (one wave per SIMD): waves per SIMD allowed by the 512-entry register file
    // (8-register granules, MI355X_MICROARCH.md "Register files") and by the 160 KB of LDS. The grid is persistent but needs
    // no co-residency (no inter-block hand-off), so an over-estimate only queues blocks.
    hipFuncAttributes attr{};
    int blocks_per_cu = 4;
    if (hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(kernel)) == hipSuccess && attr.numRegs > 0) {
        int regs = ((attr.numRegs + 7) / 8) * 8;
        blocks_per_cu = std::min(8, 512 / regs);
    }
    blocks_per_cu = std::max(1, std::min<int>(blocks_per_cu, (int)((160 * 1024) / std::max<size_t>(lds, 1))));
    uint32_t grid = (uint32_t)num_cus * (uint32_t)blocks_per_cu;
    const uint32_t path_waves = BLOCK / 64; // waves of a workgroup that take chunks
    uint32_t blocks_needed = (chunks + path_waves - 1) / path_waves;
    if (grid > blocks_needed) grid = blocks_needed;
    if (uses_tape(scene, launch) && (launch.tape == nullptr || (size_t)grid * BLOCK > launch.tape_lanes || launch.tape_max_ops < tape_ops_bound(scene, launch)))
        return fail(PYR_ERR_INVALID_ARGUMENT, "the spectral tape is missing or too small for this launch");
    if (PYR_SAMPLE_QUEUE != 0 && uses_tape(scene, launch) && scene.needs_interpreter == 0 &&
        (launch.start_queue == nullptr || launch.start_queue_stride < start_queue_words(launch.spectrum_samples) * kStartQueueEntries))
        return fail(PYR_ERR_INVALID_ARGUMENT, "the queue of ready sample starts is missing or too small for this launch"); // one slab per wave the tape has columns for: checked above
    if (const char* cut = std::getenv("PYRITE_TEST_TAPE_OPS")) // test switch: pretend the bound were smaller, to see the overflow word work
        if (uses_tape(scene, launch) && *cut) launch.tape_max_ops = std::min<uint32_t>(launch.tape_max_ops, (uint32_t)std::strtoul(cut, nullptr, 10));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), lds, (hipStream_t)stream, scene, launch);
    err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("render kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

int launch_intersect(const DevScene& scene, const IntersectLaunch& launch, bool with_counters, void* stream) {
    if (launch.n == 0) return PYR_OK;
    if (scene.stack_depth > kMaxStackDepth) return fail(PYR_ERR_UNSUPPORTED, "BVH deeper than kMaxStackDepth");
    const uint32_t stack_lds = short_stack_levels(scene, 0, 8);
    const size_t lds = (size_t)stack_lds * BLOCK * sizeof(int);
    auto kernel = with_counters ? intersect_kernel<true> : intersect_kernel<false>;
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("hipFuncSetAttribute: ") + hipGetErrorString(err));
    // persistent grid: as many workgroups as the registers and the LDS stack let a CU hold (no co-residency is required)
    int blocks_per_cu = std::max(1, std::min<int>(8, (int)((160 * 1024) / std::max<size_t>(lds, 1))));
    uint32_t grid = (uint32_t)launch.num_cus * (uint32_t)blocks_per_cu;
    uint32_t needed = (launch.n + BLOCK - 1) / BLOCK;
    if (grid > needed) grid = needed;
    IntersectLaunch sized = launch;
    sized.stack_lds = stack_lds;
    // reservation per atomic: about a quarter of a wave's share of the batch, a multiple of 64, at most 2048
    const uint32_t waves = grid * (BLOCK / 64);
    sized.reserve = std::max<uint32_t>(64, std::min<uint32_t>(2048, (launch.n / std::max<uint32_t>(waves * 4, 1)) & ~63u));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), lds, (hipStream_t)stream, scene, sized);
    err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("intersect kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

} // namespace pyr
