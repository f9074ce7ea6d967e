// features.hip -- the first-hit feature pass (include/pyrite_gpu.h "first-hit feature images"): per pixel the
// albedo spectrum, shading normal, depth, shape and material id and coverage of what the camera sees, without random numbers.
// kernels/features_wide.hip compiles this file once more with PYR_WIDE_VM for scenes whose programs need the wide register file.
#ifdef PYR_PHASE_PROFILE
#undef PYR_PHASE_PROFILE // the phase counters belong to the render kernels' one unit (kernels/profile.hip); nothing here is profiled
#endif
#include "../kernels.hip"

#include "../api_internal.h"

namespace pyr {
#ifdef PYR_WIDE_VM
namespace wide {
#endif

// Item number -> pixel. 64 consecutive items are an 8 x 8 pixel square (ragged at the right and bottom edges: false), so that the
// primary rays a wave starts together share tree nodes and texels in both directions; -DPYR_FEATURES_ROW_MAJOR numbers the pixels
// row by row instead (the A/B of tools/bench_features.py).
DEV bool feature_pixel(const FeatureLaunch& L, uint32_t item, uint32_t& x, uint32_t& y) {
#ifdef PYR_FEATURES_ROW_MAJOR
    y = item / L.film.width;
    x = item - y * L.film.width;
    return true;
#else
    const uint32_t square = item >> 6, within = item & 63u;
    const uint32_t sy = square / L.squares_x, sx = square - sy * L.squares_x;
    x = sx * 8u + (within & 7u);
    y = sy * 8u + (within >> 3);
    return x < L.film.width && y < L.film.height;
#endif
}

// The ray of sub-sample j of pixel (x, y): Camera::to_view_area of the pixel (cameras.rs:57-68), the sub-sample's place in it, and
// Camera::ray_towards (cameras.rs:70-97) through the centre of the lens -- start_sample's arithmetic without its random numbers.
DEV void feature_ray(const FeatureLaunch& L, uint32_t x, uint32_t y, uint32_t j, f3& o, f3& d) {
    const TileArea area = to_view_area(x, y, 1u, 1u, L.film.width, L.film.height);
    const uint32_t jy = j / L.grid, jx = j - jy * L.grid;
    const float fx = __fdiv_rn(__fadd_rn((float)jx, 0.5f), (float)L.grid), fy = __fdiv_rn(__fadd_rn((float)jy, 0.5f), (float)L.grid);
    const float px = __fadd_rn(area.from_x, __fmul_rn(area.size_x, fx));
    const float py = __fadd_rn(area.from_y, __fmul_rn(area.size_y, fy));
    const float focus_x = px / L.camera.view_plane * L.camera.focus_distance;
    const float focus_y = py / L.camera.view_plane * L.camera.focus_distance;
    const f3 target = mk(focus_x, -focus_y, -L.camera.focus_distance);
    o = transform_point(L.camera.cam_to_world, mk(0, 0, 0));
    d = transform_vector(L.camera.cam_to_world, normalize(target));
}

// What a lane keeps of its pixel between sub-samples.
struct FeaturePixelState {
    uint32_t x, y, j;
    f3 normal;
    float depth;
    uint32_t hits, shape, material;
};

// One finished sub-sample: surface data and shading normal at the hit, the sums of the record, and the sub-sample's albedo added
// to the pixel's own grains -- bins outermost, components inside, one grain read, changed and written back at a time, so no lane
// holds a spectrum in registers. The lane owns the pixel: plain loads and stores.
template <bool INTERP>
DEV void feature_shade(const DevScene& S, const FeatureLaunch& L, const Trav& t, FeaturePixelState& p) {
    const bool hit = t.shape != PYR_HIT_NONE;
    f3 normal = mk(0, 0, 0);
    uint32_t material = 0xFFFFFFFFu;
    float tx = 0.0f, ty = 0.0f;
    if (hit) {
        const Hit h{t.closest, t.shape, t.u, t.v};
        f3 position;
        if constexpr (INTERP)
            surface_textured(S, h, t.o, t.d, position, normal, material, tx, ty, L.film.wl_start + L.film.wl_width * 0.5f);
        else
            surface_at(S, h, t.o, t.d, position, normal, material);
        p.normal = p.normal + normal;
        p.depth += t.closest;
        p.hits += 1u;
    }
    if (p.j == (L.grid * L.grid) / 2u) {
        p.shape = t.shape;
        p.material = material;
    }
    if (L.albedo == nullptr) return;
    PyrGrain* grains = L.albedo + ((size_t)p.x + (size_t)p.y * L.film.width) * L.albedo_bins;
    PyrMaterial m{};
    if (hit) m = S.materials[material];
    const float bin_width = L.film.wl_width / (float)L.albedo_bins;
    for (uint32_t b = 0; b < L.albedo_bins; ++b) {
        float a = 0.0f;
        if (hit && m.num_components != 0u) {
            const VmInput in{L.film.wl_start + ((float)b + 0.5f) * bin_width, normal, t.d, tx, ty};
            float sum = 0.0f;
            for (uint32_t c = 0; c < m.num_components; ++c) {
                const PyrComponent comp = S.components[m.first_component + c];
                if (comp.bsdf == PYR_BSDF_EMISSIVE) continue;
                const float probability = get_probability<false, INTERP>(S, comp, in).value;
                sum += probability * run_program<INTERP>(S, comp.color_program, in);
            }
            a = sum / (float)m.num_components;
        }
        PyrGrain g = grains[b];
        g.acc += a;
        g.weight += 1.0f;
        grains[b] = g;
    }
}

DEV void feature_write(const FeatureLaunch& L, const FeaturePixelState& p) {
    if (L.pixels == nullptr) return;
    const float n = (float)p.hits;
    const bool any = p.hits != 0u;
    const float4 lo = make_float4(any ? p.normal.x / n : 0.0f, any ? p.normal.y / n : 0.0f, any ? p.normal.z / n : 0.0f, any ? p.depth / n : 0.0f);
    const float4 hi = make_float4(n / (float)(L.grid * L.grid), __uint_as_float(p.shape), __uint_as_float(p.material), 0.0f);
    float4* out = reinterpret_cast<float4*>(L.pixels + ((size_t)p.x + (size_t)p.y * L.film.width)); // a record is 32 bytes: two vector stores
    out[0] = lo;
    out[1] = hi;
}

// Persistent waves over the pixels of the image, intersect_kernel's work feed and resumable traversal (the pair tree and the
// straight-line step where the scene has them, the wide or the binary tree otherwise). A lane keeps its pixel: it walks the
// pixel's sub-samples one after the other, sums in registers and writes the record when the last one is done. Finished rays wait
// until kShadeLanes of the wave have one (or nobody is left walking), so that surface data, textures and programs run on more
// than a lane or two at a time.
template <bool INTERP>
__global__ __launch_bounds__(BLOCK, INTERP ? 3 : 4) void features_kernel(DevScene S, FeatureLaunch L) {
    extern __shared__ int lds_stack[];
    TravStack stack;
    int deep_levels[kMaxStackDepth];
    stack.deep = deep_levels;
    stack.lds = (lds_int*)(lds_stack + threadIdx.x);
    stack.lds_entries = (int)L.stack_lds;
    Counters cnt{};
    SceneView view = wide_or_binary_view(S);
    const bool lean = S.wide_nodes != nullptr && S.pair_prims != nullptr;
    if (lean) {
        view.nodes = reinterpret_cast<const float4*>(S.wide_pair_nodes);
        view.pairs = reinterpret_cast<const float4*>(S.pair_prims);
    }
    const uint32_t lane = threadIdx.x & 63u;
    constexpr int kRefillLanes = 16, kShadeLanes = 16, kSteps = 4;
    enum : uint32_t { IDLE = 0, WALK = 1, SHADE = 2 };
    const uint32_t subsamples = L.grid * L.grid;
    uint32_t state = IDLE;
    FeaturePixelState p{};
    Trav t{};
    auto start_ray = [&]() {
        f3 o, d;
        feature_ray(L, p.x, p.y, p.j, o, d);
        trav_begin<false>(S, t, o, d, false, 0.0f, cnt);
        t.inv = box_reciprocal(t.d);
        trav_ray_signs(t);
        state = WALK;
    };
    WorkFeed feed;
    feed.segment = blockIdx.x % kFeedSegments;
    for (;;) {
        const unsigned long long idle_mask = ballot64(state == IDLE);
        const int idle = __popcll(idle_mask);
        if (!feed.drained && (idle >= kRefillLanes || idle == 64)) {
            feed_reserve(feed, L.next, L.n, L.reserve, lane);
            if (!feed.drained) {
                const uint32_t available = feed.end - feed.next;
                const uint32_t rank = (uint32_t)__popcll(idle_mask & ((1ull << lane) - 1ull));
                if (state == IDLE && rank < available && feature_pixel(L, feed.next + rank, p.x, p.y)) {
                    p.j = 0u;
                    p.normal = mk(0, 0, 0);
                    p.depth = 0.0f;
                    p.hits = 0u;
                    p.shape = PYR_HIT_NONE;
                    p.material = 0xFFFFFFFFu;
                    start_ray();
                }
                feed.next += min((uint32_t)idle, available);
            }
        }
        const unsigned long long walking = ballot64(state == WALK), waiting = ballot64(state == SHADE);
        if ((walking | waiting) == 0ull) {
            if (feed.drained) break;
            continue;
        }
        if (__popcll(waiting) >= kShadeLanes || walking == 0ull) {
            if (state == SHADE) {
                feature_shade<INTERP>(S, L, t, p);
                p.j += 1u;
                if (p.j < subsamples) {
                    start_ray();
                } else {
                    feature_write(L, p);
                    state = IDLE;
                }
            }
        }
        for (int step = 0; step < kSteps; ++step) {
            bool busy = state == WALK;
            if (lean ? trav_step_lean<false>(view, t, stack, cnt, busy) : trav_step_voted<false>(view, t, stack, cnt, busy)) state = SHADE;
        }
    }
}

#ifdef PYR_WIDE_VM
} // namespace wide

FeatureKernel pick_wide_features_kernel() { return wide::features_kernel<true>; }
#else

int launch_features(const DevScene& scene, const FeatureLaunch& launch, void* stream, int num_cus, bool wide_vm) {
    if (scene.stack_depth > kMaxStackDepth) return fail(PYR_ERR_UNSUPPORTED, "BVH deeper than kMaxStackDepth");
    FeatureLaunch sized = launch;
#ifdef PYR_FEATURES_ROW_MAJOR
    const uint64_t items = (uint64_t)launch.film.width * launch.film.height;
    sized.squares_x = 0;
#else
    sized.squares_x = (launch.film.width + 7u) / 8u;
    const uint64_t items = (uint64_t)sized.squares_x * ((launch.film.height + 7u) / 8u) * 64u;
#endif
    if (items >= 0xFFFFFFFFull) return fail(PYR_ERR_INVALID_ARGUMENT, "film: 2^32 pixels or more (counted in 8 x 8 squares)");
    if (items == 0) return PYR_OK;
    sized.n = (uint32_t)items;
    // traversal stack levels in LDS: at most 16 (16 KB a workgroup, eight workgroups a CU), the rest in the lane's scratch
    sized.stack_lds = std::max(1u, std::min(16u, scene.wide_nodes ? scene.wide_stack_depth : scene.stack_depth));
    const size_t lds = (size_t)sized.stack_lds * BLOCK * sizeof(int);
    FeatureKernel kernel = wide_vm ? pick_wide_features_kernel() : (scene.needs_interpreter != 0 ? features_kernel<true> : features_kernel<false>);
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("hipFuncSetAttribute: ") + hipGetErrorString(err));
    // persistent grid: the workgroups the registers and the LDS stack let a CU hold (no co-residency is required)
    hipFuncAttributes attr{};
    int blocks_per_cu = 4;
    if (hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(kernel)) == hipSuccess && attr.numRegs > 0) blocks_per_cu = std::min(8, 512 / (((attr.numRegs + 7) / 8) * 8));
    blocks_per_cu = std::max(1, std::min<int>(blocks_per_cu, (int)((160 * 1024) / lds)));
    const uint32_t grid = std::min<uint32_t>((uint32_t)num_cus * (uint32_t)blocks_per_cu, (sized.n + BLOCK - 1) / BLOCK);
    // pixels a wave reserves per atomic: about a quarter of its share of the image, whole squares, at most 1024
    const uint32_t waves = grid * (BLOCK / 64);
    sized.reserve = std::max<uint32_t>(64, std::min<uint32_t>(1024, (sized.n / std::max<uint32_t>(waves * 4, 1)) & ~63u));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), lds, (hipStream_t)stream, scene, sized);
    err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("feature kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}
#endif

} // namespace pyr
