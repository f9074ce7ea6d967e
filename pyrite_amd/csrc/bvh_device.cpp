// bvh_device.cpp -- host driver of the device BVH builder: memory, the level loop, and the hand-over to finish_levelwise.
#include "bvh_device.h"

#include <chrono>
#include <cstring>

#include "../../include/pyrite_gpu.h"
#include "kernels/build_launch.h"

namespace pyr {

namespace {

struct Arena { // one allocation, carved up; freed on every way out
    char* base = nullptr;
    size_t used = 0;
    ~Arena() {
        if (base) (void)hipFree(base);
    }
    template <class T>
    T* take(size_t count) {
        T* p = (T*)(base + used);
        used += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

} // namespace

bool build_bvh_device(const std::vector<PrimBounds>& prims, bool leaves_tested_in_pairs, BuiltBvh& out, DeviceBuildReport& report, std::string& error) {
    using namespace devbuild;
    report = DeviceBuildReport{};
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t n = (uint32_t)prims.size();
    if (n <= kMaxLeafPrims) { // one leaf under the root: nothing to build
        out = single_leaf_bvh(prims);
        report.tree_ms = ms_since(t0);
        return true;
    }
    auto check = [&error](hipError_t e, const char* what) {
        if (e == hipSuccess) return true;
        error = std::string("device BVH build: ") + what + ": " + hipGetErrorString(e);
        return false;
    };

    Ctx c{};
    c.n = n;
    c.max_tasks = 2 * n;
    c.max_large = n / (kSmallNode + 1) + 2;
    c.max_small = n + 2;
    c.max_chunks = n / kChunk + c.max_large + 2;
    c.in_pairs = (PYR_SAH_PAIRS && leaves_tested_in_pairs) ? 1u : 0u;
    c.depth_bound = kMaxBvhDepth;
    Arena arena;
    {
        Arena sizing; // the same carving on a null base gives the size
        auto carve = [&](Arena& a) {
            c.tasks = a.take<lvl::Task>(c.max_tasks);
            c.refs[0] = a.take<PrimBounds>(n), c.refs[1] = a.take<PrimBounds>(n);
            c.leaf_shapes = a.take<uint32_t>(n);
            c.bins = a.take<uint32_t>((size_t)c.max_large * kBinWords);
            for (int p = 0; p < 2; ++p) {
                c.large_list[p] = a.take<uint32_t>(c.max_large);
                c.small_list[p] = a.take<uint32_t>(c.max_small);
                c.chunks[p] = a.take<Chunk>(c.max_chunks);
            }
            c.counters = a.take<Counters>(1);
        };
        carve(sizing);
        const size_t bytes = sizing.used;
        sizing.base = nullptr;
        if (!check(hipMalloc((void**)&arena.base, bytes), "hipMalloc")) return false;
        carve(arena);
    }
    if (!check(hipMemcpy(c.refs[0], prims.data(), (size_t)n * sizeof(PrimBounds), hipMemcpyHostToDevice), "upload of the primitive bounds")) return false;
    if (!check(hipMemset(c.leaf_shapes, 0xFF, (size_t)n * 4), "hipMemset")) return false;
    if (!check(launch_setup(c, nullptr), "setup")) return false;

    // The level loop is the host's: one small read-back per level, at most kMaxBvhDepth + 1 levels (a node's depth never exceeds
    // kMaxBvhDepth: the depth rule of bvh_level.h). No kernel waits for another.
    Counters counters{};
    uint32_t level = 0;
    for (;; ++level) {
        if (!check(hipMemcpy(&counters, c.counters, sizeof(Counters), hipMemcpyDeviceToHost), "read-back of the level's counts")) return false;
        const uint32_t p = level & 1u;
        if (counters.giveup != GIVEUP_NONE) {
            report.fallback_reason = counters.giveup == GIVEUP_MEDIAN_TOO_LARGE ? PYR_BUILD_FALLBACK_MEDIAN_TOO_LARGE : PYR_BUILD_FALLBACK_INTERNAL;
            return true;
        }
        if (counters.num_large[p] == 0 && counters.num_small[p] == 0) break;
        if (level > kMaxBvhDepth) {
            report.fallback_reason = PYR_BUILD_FALLBACK_INTERNAL; // (the depth rule keeps every node within kMaxBvhDepth)
            return true;
        }
        if (counters.num_large[p] > c.max_large || counters.num_small[p] > c.max_small || counters.num_chunks[p] > c.max_chunks) { // (give-up would have said so)
            report.fallback_reason = PYR_BUILD_FALLBACK_INTERNAL;
            return true;
        }
        if (!check(launch_level(c, p, counters.num_large[p], counters.num_small[p], counters.num_chunks[p], nullptr), "level kernels")) return false;
    }
    report.levels = level;
    if (counters.num_tasks > c.max_tasks) {
        report.fallback_reason = PYR_BUILD_FALLBACK_INTERNAL;
        return true;
    }
    std::vector<lvl::Task> tasks(counters.num_tasks);
    std::vector<uint32_t> leaf_shapes(n);
    if (!check(hipMemcpy(tasks.data(), c.tasks, tasks.size() * sizeof(lvl::Task), hipMemcpyDeviceToHost), "download of the tasks")) return false;
    if (!check(hipMemcpy(leaf_shapes.data(), c.leaf_shapes, (size_t)n * 4, hipMemcpyDeviceToHost), "download of the leaf order")) return false;
    report.tree_ms = ms_since(t0);

    const auto t1 = std::chrono::steady_clock::now();
    LevelBuildStats stats;
    bool ok = finish_levelwise(tasks, leaf_shapes, bvh_padding(prims), out, &stats);
    // the leaves name every primitive once (spheres come before triangles in `prims`, each kind in index order: pack_and_upload)
    if (ok) {
        uint32_t first_of_kind[4] = {0, 0, 0, 0}, seen_kind[4] = {0, 0, 0, 0};
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t kind = prims[i].shape >> 30;
            if (!seen_kind[kind]) seen_kind[kind] = 1, first_of_kind[kind] = i - (prims[i].shape & 0x3FFFFFFFu);
        }
        std::vector<uint8_t> named(n, 0);
        for (const uint32_t shape : out.prim_order) {
            const uint64_t at = (uint64_t)first_of_kind[shape >> 30] + (shape & 0x3FFFFFFFu);
            if (!seen_kind[shape >> 30] || at >= n || prims[at].shape != shape || named[at]) {
                ok = false;
                break;
            }
            named[at] = 1;
        }
    }
    report.finish_ms = ms_since(t1);
    if (!ok) {
        report.fallback_reason = PYR_BUILD_FALLBACK_INTERNAL;
        return true;
    }
    report.median_splits = stats.median_splits;
    return true;
}

} // namespace pyr
