// motion.hip -- the motion pass (include/pyrite_gpu.h "motion records and accumulation over frames"): per
// pixel, where the surface point the camera sees was one frame ago -- the same material point (shape, u, v) in the snapshot of the
// previous frame's geometry, projected into the previous camera. The feature pass's work feed, pixel squares and resumable
// traversal with one ray a pixel; no material program runs, so one build serves every scene and there is no wide twin.
#ifdef PYR_PHASE_PROFILE
#undef PYR_PHASE_PROFILE // the phase counters belong to the render kernels' one unit (kernels/profile.hip); nothing here is profiled
#endif
#include "../kernels.hip"

#include "../api_internal.h"

namespace pyr {

// Item number -> pixel: features.hip's feature_pixel, 64 consecutive items an 8 x 8 square, ragged at the right and bottom edges.
DEV bool motion_pixel(const MotionLaunch& L, uint32_t item, uint32_t& x, uint32_t& y) {
    const uint32_t square = item >> 6, within = item & 63u;
    const uint32_t sy = square / L.squares_x, sx = square - sy * L.squares_x;
    x = sx * 8u + (within & 7u);
    y = sy * 8u + (within >> 3);
    return x < L.width && y < L.height;
}

// The ray through the centre of pixel (x, y) and the centre of the lens: features.hip's feature_ray for sub-sample 0 of grid 1,
// whose place in the pixel, (0 + 0.5f) / 1.0f, is 0.5f exactly.
DEV void motion_ray(const MotionLaunch& L, uint32_t x, uint32_t y, f3& o, f3& d) {
    const TileArea area = to_view_area(x, y, 1u, 1u, L.width, L.height);
    const float px = __fadd_rn(area.from_x, __fmul_rn(area.size_x, 0.5f));
    const float py = __fadd_rn(area.from_y, __fmul_rn(area.size_y, 0.5f));
    const float focus_x = px / L.camera.view_plane * L.camera.focus_distance;
    const float focus_y = py / L.camera.view_plane * L.camera.focus_distance;
    const f3 target = mk(focus_x, -focus_y, -L.camera.focus_distance);
    o = transform_point(L.camera.cam_to_world, mk(0, 0, 0));
    d = transform_vector(L.camera.cam_to_world, normalize(target));
}

// The position surface_at reports for a hit, without the normal and the material it also fetches.
DEV f3 motion_position(const DevScene& S, const Trav& t, uint32_t kind, uint32_t index) {
    f3 position = t.o + t.d * t.closest;
    float dist;
    if (kind == PYR_SHAPE_SPHERE) {
        const float4 sp = reinterpret_cast<const float4*>(S.spheres)[index];
        sphere_test(mk(sp.x, sp.y, sp.z), sp.w, t.o, t.d, dist, position);
    } else if (kind == PYR_SHAPE_PLANE) {
        const float* pl = S.planes + 8 * index;
        plane_test(ld3(pl), ld3(pl + 3), t.o, t.d, dist, position);
    }
    return position;
}

// One finished ray -> the pixel's record: pyrite_gpu.h's formulas in their order. The lane owns the pixel: two 16-byte stores.
DEV void motion_write(const DevScene& S, const MotionLaunch& L, const Trav& t, uint32_t x, uint32_t y) {
    const bool hit = t.shape != PYR_HIT_NONE;
    const float* W = L.previous_w;
    f3 q;
    float depth = 0.0f, prev_depth = 0.0f;
    uint32_t flags = 0u;
    if (hit) {
        const uint32_t kind = t.shape >> 30, index = t.shape & 0x3FFFFFFFu;
        f3 Q;
        if (kind == PYR_SHAPE_TRIANGLE && L.previous_positions != nullptr) {
            const float* p = L.previous_positions + 9 * (size_t)index;
            const f3 a = ld3(p), e1 = ld3(p + 3) - a, e2 = ld3(p + 6) - a;
            Q = (a + e1 * t.u) + e2 * t.v;
        } else {
            Q = motion_position(S, t, kind, index);
            if (kind == PYR_SHAPE_SPHERE && L.previous_spheres != nullptr) {
                const float4 now = reinterpret_cast<const float4*>(S.spheres)[index], then = reinterpret_cast<const float4*>(L.previous_spheres)[index];
                Q = mk(then.x, then.y, then.z) + (Q - mk(now.x, now.y, now.z)) * (then.w / now.w);
            }
        }
        q = mk(W[0] * Q.x + W[4] * Q.y + W[8] * Q.z + W[12], W[1] * Q.x + W[5] * Q.y + W[9] * Q.z + W[13], W[2] * Q.x + W[6] * Q.y + W[10] * Q.z + W[14]);
        depth = t.closest;
        prev_depth = sqrt32((q.x * q.x + q.y * q.y) + q.z * q.z);
        flags = PYR_MOTION_HIT;
    } else {
        q = transform_vector(W, t.d); // a point at infinity
    }
    const float zc = -q.z;
    float prev_x = 0.0f, prev_y = 0.0f;
    if (zc > 0.0f) {
        const float vx = (q.x / zc) * L.previous_view_plane, vy = (-q.y / zc) * L.previous_view_plane;
        const float w = (float)L.width, h = (float)L.height, m = fmaxf(w, h) * 0.5f;
        prev_x = vx * m + w * 0.5f;
        prev_y = vy * m + h * 0.5f;
        flags |= PYR_MOTION_IN_FRONT;
        if (prev_x >= 0.0f && prev_x < w && prev_y >= 0.0f && prev_y < h) flags |= PYR_MOTION_INSIDE;
    }
    float4* out = reinterpret_cast<float4*>(L.pixels + ((size_t)x + (size_t)y * L.width)); // a record is 32 bytes: two vector stores
    out[0] = make_float4(prev_x, prev_y, prev_depth, depth);
    out[1] = make_float4(__uint_as_float(t.shape), __uint_as_float(flags), 0.0f, 0.0f);
}

// Persistent waves over the pixels, features_kernel's loop with one ray a pixel: a lane that has finished its ray writes its
// record at the end of the turn -- a few dozen operations, nothing worth gathering lanes for -- and is idle again.
__global__ __launch_bounds__(BLOCK, 4) void motion_kernel(DevScene S, MotionLaunch L) {
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
    constexpr int kRefillLanes = 16, kSteps = 4;
    enum : uint32_t { IDLE = 0, WALK = 1, DONE = 2 };
    uint32_t state = IDLE, x = 0, y = 0;
    Trav t{};
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
                if (state == IDLE && rank < available && motion_pixel(L, feed.next + rank, x, y)) {
                    f3 o, d;
                    motion_ray(L, x, y, o, d);
                    trav_begin<false>(S, t, o, d, false, 0.0f, cnt);
                    t.inv = box_reciprocal(t.d);
                    trav_ray_signs(t);
                    state = WALK;
                }
                feed.next += min((uint32_t)idle, available);
            }
        }
        if (ballot64(state == WALK) == 0ull) {
            if (feed.drained) break;
            continue;
        }
        for (int step = 0; step < kSteps; ++step) {
            bool busy = state == WALK;
            if (lean ? trav_step_lean<false>(view, t, stack, cnt, busy) : trav_step_voted<false>(view, t, stack, cnt, busy)) state = DONE;
        }
        if (state == DONE) { // before the next turn looks for idle lanes: no lane leaves the loop with a record unwritten
            motion_write(S, L, t, x, y);
            state = IDLE;
        }
    }
}

int launch_motion(const DevScene& scene, const MotionLaunch& launch, void* stream, int num_cus) {
    if (scene.stack_depth > kMaxStackDepth) return fail(PYR_ERR_UNSUPPORTED, "BVH deeper than kMaxStackDepth");
    MotionLaunch sized = launch;
    sized.squares_x = (launch.width + 7u) / 8u;
    const uint64_t items = (uint64_t)sized.squares_x * ((launch.height + 7u) / 8u) * 64u;
    if (items >= 0xFFFFFFFFull) return fail(PYR_ERR_INVALID_ARGUMENT, "film: 2^32 pixels or more (counted in 8 x 8 squares)");
    if (items == 0) return PYR_OK;
    sized.n = (uint32_t)items;
    // traversal stack levels in LDS: at most 16 (16 KB a workgroup), the rest in the lane's scratch -- as the feature pass
    sized.stack_lds = std::max(1u, std::min(16u, scene.wide_nodes ? scene.wide_stack_depth : scene.stack_depth));
    const size_t lds = (size_t)sized.stack_lds * BLOCK * sizeof(int);
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(motion_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("hipFuncSetAttribute: ") + hipGetErrorString(err));
    // persistent grid: the workgroups the registers and the LDS stack let a CU hold (no co-residency is required)
    hipFuncAttributes attr{};
    int blocks_per_cu = 4;
    if (hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(motion_kernel)) == hipSuccess && attr.numRegs > 0) blocks_per_cu = std::min(8, 512 / (((attr.numRegs + 7) / 8) * 8));
    blocks_per_cu = std::max(1, std::min<int>(blocks_per_cu, (int)((160 * 1024) / lds)));
    const uint32_t grid = std::min<uint32_t>((uint32_t)num_cus * (uint32_t)blocks_per_cu, (sized.n + BLOCK - 1) / BLOCK);
    // pixels a wave reserves per atomic: about a quarter of its share of the image, whole squares, at most 1024
    const uint32_t waves = grid * (BLOCK / 64);
    sized.reserve = std::max<uint32_t>(64, std::min<uint32_t>(1024, (sized.n / std::max<uint32_t>(waves * 4, 1)) & ~63u));
    hipLaunchKernelGGL(motion_kernel, dim3(grid), dim3(BLOCK), lds, (hipStream_t)stream, scene, sized);
    err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("motion kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

} // namespace pyr
