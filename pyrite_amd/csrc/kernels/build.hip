// build.hip -- the BVH builder on the device, a unit of its own: level-synchronous binned SAH with
// build_bvh's rules (bvh_level.h), so that the tree is the host builder's. Nothing here touches the render kernels.
//
// One level = the nodes of one depth. Per level: bin (large nodes: a private histogram in LDS per workgroup, flushed with integer
// atomics on order-preserving keys), choose (one thread per large node), partition (references move to their side of the next
// level's array while the children's boxes accumulate); a node of at most a wave's worth of references does all three in one
// wave. No kernel waits for another workgroup: every atomic is a min, a max or an add whose result nobody spins on, and the level
// loop is the host's (bvh_device.cpp).
#include "build_launch.h"

namespace pyr {
namespace devbuild {

namespace {

using lvl::Task;

__device__ __forceinline__ void give_up(const Ctx& c, uint32_t why) { atomicMax(&c.counters->giveup, why); }

// bins of one node as choose_split reads them, from keys in LDS or in global memory
struct KeyBins {
    const uint32_t* w;
    __device__ __forceinline__ lvl::Box3 box(int a, int k) const {
        lvl::Box3 b;
        const uint32_t* lo = w + (a * lvl::kBins + k) * 3;
        const uint32_t* hi = lo + 3 * lvl::kBins * 3;
        for (int j = 0; j < 3; ++j) b.lo[j] = lvl::float_of(lo[j]), b.hi[j] = lvl::float_of(hi[j]);
        return b;
    }
    __device__ __forceinline__ uint32_t count(int a, int k) const { return w[2 * 3 * lvl::kBins * 3 + a * lvl::kBins + k]; }
};
constexpr uint32_t kLoWords = 3 * lvl::kBins * 3; // 144 lower keys, then 144 upper keys, then 48 counts

__device__ __forceinline__ uint32_t empty_bin_word(uint32_t w) { return w < kLoWords ? lvl::kKeyPosInf : w < 2 * kLoWords ? lvl::kKeyNegInf : 0u; }

// one reference into a node's bins in LDS
__device__ __forceinline__ void bin_reference(uint32_t* h, const PrimBounds& r, const lvl::Box3& cbox, const float* scale, const bool* valid) {
    for (int a = 0; a < 3; ++a) {
        if (!valid[a]) continue;
        const int k = lvl::bin_index(lvl::centroid(r.lo[a], r.hi[a]), cbox.lo[a], scale[a]);
        uint32_t* lo = h + (a * lvl::kBins + k) * 3;
        for (int j = 0; j < 3; ++j) {
            atomicMin(lo + j, lvl::key_of(r.lo[j]));
            atomicMax(lo + kLoWords + j, lvl::key_of(r.hi[j]));
        }
        atomicAdd(h + 2 * kLoWords + a * lvl::kBins + k, 1u);
    }
}

// a reference into its side's box and centroid box: kb[side][0..5] box keys, [6..11] centroid keys (LDS)
__device__ __forceinline__ void grow_side(uint32_t* kb, const PrimBounds& r) {
    for (int a = 0; a < 3; ++a) {
        atomicMin(kb + a, lvl::key_of(r.lo[a]));
        atomicMax(kb + 3 + a, lvl::key_of(r.hi[a]));
        const uint32_t ck = lvl::key_of(lvl::centroid(r.lo[a], r.hi[a]));
        atomicMin(kb + 6 + a, ck);
        atomicMax(kb + 9 + a, ck);
    }
}
__device__ __forceinline__ uint32_t empty_side_word(uint32_t w) { return (w % 6) < 3 ? lvl::kKeyPosInf : lvl::kKeyNegInf; }

// puts a new task on the next level's lists; a large one with its chunks
__device__ void enqueue(const Ctx& c, uint32_t next, uint32_t task, uint32_t begin, uint32_t end) {
    const uint32_t count = end - begin;
    if (count <= kSmallNode) {
        const uint32_t i = atomicAdd(&c.counters->num_small[next], 1u);
        if (i >= c.max_small) return give_up(c, GIVEUP_CAPACITY);
        c.small_list[next][i] = task;
        return;
    }
    const uint32_t li = atomicAdd(&c.counters->num_large[next], 1u);
    const uint32_t chunks = (count + kChunk - 1) / kChunk;
    const uint32_t first = atomicAdd(&c.counters->num_chunks[next], chunks);
    if (li >= c.max_large || first + chunks > c.max_chunks) return give_up(c, GIVEUP_CAPACITY);
    c.large_list[next][li] = task;
    for (uint32_t k = 0; k < chunks; ++k) {
        const uint32_t b = begin + k * kChunk;
        c.chunks[next][first + k] = Chunk{task, li, b, b + kChunk < end ? b + kChunk : end};
    }
}

// the two children of task `ti` (decision `d` taken): allocates and initialises them (boxes empty), returns child0 or 0 when the
// task array is full
__device__ uint32_t make_children(const Ctx& c, uint32_t ti, const Task& t, const lvl::Decision& d) {
    const uint32_t child0 = atomicAdd(&c.counters->num_tasks, 2u);
    if (child0 + 2 > c.max_tasks) {
        give_up(c, GIVEUP_CAPACITY);
        return 0;
    }
    for (uint32_t s = 0; s < 2; ++s) {
        Task k;
        k.begin = s == 0 ? t.begin : t.begin + d.left_count;
        k.end = s == 0 ? t.begin + d.left_count : t.end;
        k.parent = (int32_t)ti, k.slot = s, k.depth = t.depth + 1, k.kind = lvl::KIND_PENDING, k.child0 = 0;
        k.axis = 0, k.bin = 0, k.lo = 0.0f, k.scale = 0.0f, k.cursor[0] = k.cursor[1] = 0;
        lvl::empty_keys(k.box), lvl::empty_keys(k.cbox);
        c.tasks[child0 + s] = k;
    }
    return child0;
}

// ---- setup: task 0 and level 0's lists; then the root's bounds, chunk by chunk
__global__ void setup_kernel(Ctx c) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    Task t;
    t.begin = 0, t.end = c.n, t.parent = -1, t.slot = 0, t.depth = 0, t.kind = lvl::KIND_PENDING, t.child0 = 0;
    t.axis = 0, t.bin = 0, t.lo = 0.0f, t.scale = 0.0f, t.cursor[0] = t.cursor[1] = 0;
    lvl::empty_keys(t.box), lvl::empty_keys(t.cbox);
    c.tasks[0] = t;
    Counters z{};
    z.num_tasks = 1;
    *c.counters = z;
    enqueue(c, 0, 0, 0, c.n);
}

__global__ __launch_bounds__(kBlock) void root_bounds_kernel(Ctx c) {
    __shared__ uint32_t kb[12];
    if (threadIdx.x < 12) kb[threadIdx.x] = empty_side_word(threadIdx.x);
    __syncthreads();
    const uint32_t begin = blockIdx.x * kChunk, end = begin + kChunk < c.n ? begin + kChunk : c.n;
    for (uint32_t i = begin + threadIdx.x; i < end; i += kBlock) grow_side(kb, c.refs[0][i]);
    __syncthreads();
    if (threadIdx.x < 12) {
        uint32_t* dst = threadIdx.x < 6 ? c.tasks[0].box + threadIdx.x : c.tasks[0].cbox + (threadIdx.x - 6);
        if ((threadIdx.x % 6) < 3)
            atomicMin(dst, kb[threadIdx.x]);
        else
            atomicMax(dst, kb[threadIdx.x]);
    }
}

// ---- a level's own start: nothing is queued for the next level yet
__global__ void begin_level_kernel(Ctx c, uint32_t next) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    c.counters->num_large[next] = c.counters->num_small[next] = c.counters->num_chunks[next] = 0;
}

__global__ __launch_bounds__(kBlock) void clear_bins_kernel(Ctx c, uint32_t num_large) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < num_large * kBinWords) c.bins[i] = empty_bin_word(i % kBinWords);
}

// ---- bin, large nodes: one chunk of one node per workgroup
__global__ __launch_bounds__(kBlock) void bin_large_kernel(Ctx c, uint32_t parity, uint32_t num_chunks) {
    __shared__ uint32_t h[kBinWords];
    if (blockIdx.x >= num_chunks) return;
    const Chunk ch = c.chunks[parity][blockIdx.x];
    for (uint32_t w = threadIdx.x; w < kBinWords; w += kBlock) h[w] = empty_bin_word(w);
    const lvl::Box3 cbox = lvl::box_of_keys(c.tasks[ch.task].cbox);
    float scale[3];
    bool valid[3];
    for (int a = 0; a < 3; ++a) {
        const float extent = cbox.hi[a] - cbox.lo[a];
        valid[a] = extent > 0.0f;
        scale[a] = valid[a] ? lvl::bin_scale(extent) : 0.0f;
    }
    __syncthreads();
    const PrimBounds* refs = c.refs[parity];
    for (uint32_t i = ch.begin + threadIdx.x; i < ch.end; i += kBlock) bin_reference(h, refs[i], cbox, scale, valid);
    __syncthreads();
    uint32_t* g = c.bins + (size_t)ch.large_index * kBinWords;
    for (uint32_t w = threadIdx.x; w < kBinWords; w += kBlock) {
        const uint32_t v = h[w];
        if (v == empty_bin_word(w)) continue;
        if (w < kLoWords)
            atomicMin(g + w, v);
        else if (w < 2 * kLoWords)
            atomicMax(g + w, v);
        else
            atomicAdd(g + w, v);
    }
}

// ---- choose, large nodes: one thread per node (more than kSmallNode references: never a leaf)
__global__ __launch_bounds__(64) void choose_large_kernel(Ctx c, uint32_t parity, uint32_t num_large) {
    const uint32_t li = blockIdx.x * 64 + threadIdx.x;
    if (li >= num_large) return;
    const uint32_t ti = c.large_list[parity][li];
    Task t = c.tasks[ti];
    const KeyBins bins{c.bins + (size_t)li * kBinWords};
    const lvl::Decision d = lvl::choose_split(t.end - t.begin, t.depth, lvl::box_of_keys(t.box), lvl::box_of_keys(t.cbox), bins, c.in_pairs != 0, c.depth_bound);
    if (d.kind == lvl::KIND_LEAF || d.left_count == 0 || d.left_count >= t.end - t.begin) return give_up(c, GIVEUP_CAPACITY); // (cannot happen)
    if (d.kind == lvl::KIND_MEDIAN && t.end - t.begin > kMedianMax) return give_up(c, GIVEUP_MEDIAN_TOO_LARGE);
    const uint32_t child0 = make_children(c, ti, t, d);
    if (!child0) return;
    t.kind = d.kind, t.axis = d.axis, t.bin = d.bin, t.lo = d.lo, t.scale = d.scale, t.child0 = child0;
    c.tasks[ti] = t;
    enqueue(c, parity ^ 1u, child0, t.begin, t.begin + d.left_count);
    enqueue(c, parity ^ 1u, child0 + 1, t.begin + d.left_count, t.end);
}

__device__ __forceinline__ void flush_sides(const Ctx& c, uint32_t child0, const uint32_t (*kb)[12]) {
    if (threadIdx.x < 24) {
        const uint32_t s = threadIdx.x / 12, w = threadIdx.x % 12;
        Task& kid = c.tasks[child0 + s];
        uint32_t* dst = w < 6 ? kid.box + w : kid.cbox + (w - 6);
        const uint32_t v = kb[s][w];
        if (v == empty_side_word(w)) return;
        if ((w % 6) < 3)
            atomicMin(dst, v);
        else
            atomicMax(dst, v);
    }
}

// ---- partition, large nodes split by bins: one chunk per workgroup. Two cursors per node, advanced once per chunk; inside the
// chunk the places come from LDS counters. Where a reference lands inside its side is free: the tree does not depend on it.
__global__ __launch_bounds__(kBlock) void partition_large_kernel(Ctx c, uint32_t parity, uint32_t num_chunks) {
    __shared__ uint32_t lefts, base[2], local[2];
    __shared__ uint32_t kb[2][12];
    if (blockIdx.x >= num_chunks) return;
    const Chunk ch = c.chunks[parity][blockIdx.x];
    const Task t = c.tasks[ch.task];
    if (t.kind != lvl::KIND_SPLIT) return; // the median rule has a kernel of its own; a build that gave up made no decision
    if (threadIdx.x < 24) kb[threadIdx.x / 12][threadIdx.x % 12] = empty_side_word(threadIdx.x % 12);
    if (threadIdx.x == 0) lefts = 0, local[0] = local[1] = 0;
    __syncthreads();
    const PrimBounds* refs = c.refs[parity];
    PrimBounds* out = c.refs[parity ^ 1u];
    uint32_t sides = 0, mine = 0; // bit k: my k-th reference goes to slot 1
    {
        uint32_t k = 0;
        for (uint32_t i = ch.begin + threadIdx.x; i < ch.end; i += kBlock, ++k) {
            const PrimBounds& r = refs[i];
            const bool right = lvl::bin_index(lvl::centroid(r.lo[t.axis], r.hi[t.axis]), t.lo, t.scale) > t.bin;
            sides |= (right ? 1u : 0u) << k;
            mine += right ? 0u : 1u;
        }
    }
    if (mine) atomicAdd(&lefts, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        base[0] = atomicAdd(&c.tasks[ch.task].cursor[0], lefts);
        base[1] = atomicAdd(&c.tasks[ch.task].cursor[1], (ch.end - ch.begin) - lefts);
    }
    __syncthreads();
    const uint32_t side_begin[2] = {c.tasks[t.child0].begin, c.tasks[t.child0 + 1].begin};
    const uint32_t side_end[2] = {c.tasks[t.child0].end, c.tasks[t.child0 + 1].end};
    {
        uint32_t k = 0;
        for (uint32_t i = ch.begin + threadIdx.x; i < ch.end; i += kBlock, ++k) {
            const PrimBounds r = refs[i];
            const uint32_t s = (sides >> k) & 1u;
            const uint32_t dst = side_begin[s] + base[s] + atomicAdd(&local[s], 1u);
            if (dst < side_end[s] && dst < c.n)
                out[dst] = r;
            else
                give_up(c, GIVEUP_CAPACITY); // (cannot happen: the bins counted with the same bin_index)
            grow_side(kb[s], r);
        }
    }
    __syncthreads();
    flush_sides(c, t.child0, kb);
}

// ---- partition, large nodes split by the median rule: one node per workgroup, at most kMedianMax references. A reference's
// place is its rank by (centroid, shape code): the count / 2 smallest go to slot 0, whatever order they were held in.
__global__ __launch_bounds__(kBlock) void median_large_kernel(Ctx c, uint32_t parity, uint32_t num_large) {
    __shared__ float kc[kMedianMax];
    __shared__ uint32_t ks[kMedianMax];
    __shared__ uint32_t kb[2][12];
    if (blockIdx.x >= num_large) return;
    const Task t = c.tasks[c.large_list[parity][blockIdx.x]];
    const uint32_t count = t.end - t.begin;
    if (t.kind != lvl::KIND_MEDIAN || count > kMedianMax) return;
    const PrimBounds* refs = c.refs[parity] + t.begin;
    PrimBounds* out = c.refs[parity ^ 1u];
    if (threadIdx.x < 24) kb[threadIdx.x / 12][threadIdx.x % 12] = empty_side_word(threadIdx.x % 12);
    for (uint32_t i = threadIdx.x; i < count; i += kBlock) kc[i] = lvl::centroid(refs[i].lo[t.axis], refs[i].hi[t.axis]), ks[i] = refs[i].shape;
    __syncthreads();
    const uint32_t left = count / 2;
    for (uint32_t i = threadIdx.x; i < count; i += kBlock) {
        const float ci = kc[i];
        const uint32_t si = ks[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < count; ++j) rank += lvl::median_before(kc[j], ks[j], ci, si) ? 1u : 0u;
        const PrimBounds r = refs[i];
        if (rank < count && t.begin + rank < c.n) out[t.begin + rank] = r;
        grow_side(kb[rank < left ? 0 : 1], r);
    }
    __syncthreads();
    flush_sides(c, t.child0, kb);
}

// ---- small nodes: bin, choose and partition of one node in one wave (one workgroup of 64 lanes, lane = reference)
__global__ __launch_bounds__(64) void small_kernel(Ctx c, uint32_t parity, uint32_t num_small) {
    __shared__ uint32_t h[kBinWords];
    __shared__ uint32_t kb[2][12];
    __shared__ float kc[kSmallNode];
    __shared__ uint32_t ks[kSmallNode];
    __shared__ lvl::Decision decision;
    if (blockIdx.x >= num_small) return;
    const uint32_t ti = c.small_list[parity][blockIdx.x];
    Task t = c.tasks[ti];
    const uint32_t count = t.end - t.begin, lane = threadIdx.x;
    if (count > kSmallNode || t.end > c.n) return give_up(c, GIVEUP_CAPACITY); // (cannot happen)
    const bool has = lane < count;
    PrimBounds r{};
    if (has) r = c.refs[parity][t.begin + lane];
    for (uint32_t w = lane; w < kBinWords; w += 64) h[w] = empty_bin_word(w);
    if (lane < 24) kb[lane / 12][lane % 12] = empty_side_word(lane % 12);
    const lvl::Box3 box = lvl::box_of_keys(t.box), cbox = lvl::box_of_keys(t.cbox);
    float scale[3];
    bool valid[3];
    for (int a = 0; a < 3; ++a) {
        const float extent = cbox.hi[a] - cbox.lo[a];
        valid[a] = extent > 0.0f;
        scale[a] = valid[a] ? lvl::bin_scale(extent) : 0.0f;
    }
    __syncthreads();
    if (has) bin_reference(h, r, cbox, scale, valid);
    __syncthreads();
    if (lane == 0) decision = lvl::choose_split(count, t.depth, box, cbox, KeyBins{h}, c.in_pairs != 0, c.depth_bound);
    __syncthreads();
    const lvl::Decision d = decision;
    if (d.kind == lvl::KIND_LEAF) {
        if (has) c.leaf_shapes[t.begin + lane] = r.shape;
        if (lane == 0) c.tasks[ti].kind = lvl::KIND_LEAF;
        return;
    }
    uint32_t side = 0;
    if (d.kind == lvl::KIND_SPLIT) {
        side = has && lvl::bin_index(lvl::centroid(r.lo[d.axis], r.hi[d.axis]), d.lo, d.scale) > d.bin ? 1u : 0u;
    } else {
        if (has) kc[lane] = lvl::centroid(r.lo[d.axis], r.hi[d.axis]), ks[lane] = r.shape;
        __syncthreads();
        uint32_t rank = 0;
        if (has)
            for (uint32_t j = 0; j < count; ++j) rank += lvl::median_before(kc[j], ks[j], kc[lane], ks[lane]) ? 1u : 0u;
        side = has && rank >= d.left_count ? 1u : 0u;
    }
    if (has) grow_side(kb[side], r);
    const unsigned long long left_mask = __ballot(has && side == 0), right_mask = __ballot(has && side == 1);
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t left_count = (uint32_t)__popcll(left_mask);
    if (left_count != d.left_count) return give_up(c, GIVEUP_CAPACITY); // (cannot happen: the bins counted with the same bin_index)
    const uint32_t dst = side == 0 ? t.begin + (uint32_t)__popcll(left_mask & below) : t.begin + left_count + (uint32_t)__popcll(right_mask & below);
    if (has && dst < t.end) c.refs[parity ^ 1u][dst] = r;
    __syncthreads();
    if (lane == 0) {
        const uint32_t child0 = make_children(c, ti, t, d);
        if (!child0) return;
        for (uint32_t s = 0; s < 2; ++s)
            for (uint32_t w = 0; w < 6; ++w) c.tasks[child0 + s].box[w] = kb[s][w], c.tasks[child0 + s].cbox[w] = kb[s][6 + w];
        t.kind = d.kind, t.axis = d.axis, t.bin = d.bin, t.lo = d.lo, t.scale = d.scale, t.child0 = child0;
        c.tasks[ti] = t;
        enqueue(c, parity ^ 1u, child0, t.begin, t.begin + left_count);
        enqueue(c, parity ^ 1u, child0 + 1, t.begin + left_count, t.end);
    }
}

} // namespace

hipError_t launch_setup(const Ctx& c, hipStream_t stream) {
    hipLaunchKernelGGL(setup_kernel, dim3(1), dim3(64), 0, stream, c);
    hipLaunchKernelGGL(root_bounds_kernel, dim3((c.n + kChunk - 1) / kChunk), dim3(kBlock), 0, stream, c);
    return hipGetLastError();
}

hipError_t launch_level(const Ctx& c, uint32_t parity, uint32_t num_large, uint32_t num_small, uint32_t num_chunks, hipStream_t stream) {
    hipLaunchKernelGGL(begin_level_kernel, dim3(1), dim3(64), 0, stream, c, parity ^ 1u);
    if (num_large) {
        hipLaunchKernelGGL(clear_bins_kernel, dim3((num_large * kBinWords + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, c, num_large);
        hipLaunchKernelGGL(bin_large_kernel, dim3(num_chunks), dim3(kBlock), 0, stream, c, parity, num_chunks);
        hipLaunchKernelGGL(choose_large_kernel, dim3((num_large + 63) / 64), dim3(64), 0, stream, c, parity, num_large);
        hipLaunchKernelGGL(partition_large_kernel, dim3(num_chunks), dim3(kBlock), 0, stream, c, parity, num_chunks);
        hipLaunchKernelGGL(median_large_kernel, dim3(num_large), dim3(kBlock), 0, stream, c, parity, num_large);
    }
    if (num_small) hipLaunchKernelGGL(small_kernel, dim3(num_small), dim3(64), 0, stream, c, parity, num_small);
    return hipGetLastError();
}

} // namespace devbuild
} // namespace pyr
