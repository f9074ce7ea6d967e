// bvh_level.h -- the binned-SAH rules of every BVH builder, as functions of one reference or one node: build_bvh, the object split
// of build_bvh_spatial and build_bvh_levelwise (bvh.cpp) and the device builder (kernels/build.hip) all call these, so what they
// decide can differ only in what is not in here -- how a builder walks its nodes and holds its references, atomics and scans, and
// the median rule's tie-breaking (build_bvh's nth_element against median_before below).
//
// Every quantity a node accumulates is a min, a max or a count, so a node's bins and its children's boxes do not depend on the
// order its references arrive in, and the split is a pure function of the bins (choose_split). Units that include this header are
// built with -ffp-contract=off and IEEE division. It is compiled for the device too: no standard container in here.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PYR_HD __host__ __device__ __forceinline__
#else
#define PYR_HD inline
#endif

namespace pyr {
namespace lvl {

// The builders' constants, defined here once (bvh.h names the last three kMaxLeafPrims, kMaxBvhDepth and kSahNodeCost).
#ifndef PYR_SAH_BINS
#define PYR_SAH_BINS 16
#endif
#ifndef PYR_MAX_LEAF
#define PYR_MAX_LEAF 4
#endif
#ifndef PYR_SAH_NODE_COST
#define PYR_SAH_NODE_COST 1.0f
#endif
constexpr int kBins = PYR_SAH_BINS;             // bins per axis of the object split
constexpr uint32_t kLeafMax = PYR_MAX_LEAF;     // primitives of a leaf; <= 7: the leaf code keeps the count in 3 bits
constexpr uint32_t kDepthMax = 40;              // edges from the root to a leaf, at most
constexpr float kNodeCost = PYR_SAH_NODE_COST;  // one node visit in units of one primitive test (SAH termination)

PYR_HD float pos_inf() { return __builtin_inff(); }

struct Box3 {
    float lo[3], hi[3];
};
PYR_HD Box3 empty_box() {
    Box3 b;
    for (int a = 0; a < 3; ++a) b.lo[a] = pos_inf(), b.hi[a] = -pos_inf();
    return b;
}
// as std::min / std::max would: the new bound wins only when it is strictly smaller (larger), so of -0 and +0 the first one stays
PYR_HD void grow(Box3& b, const float* l, const float* h) {
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = l[a] < b.lo[a] ? l[a] : b.lo[a];
        b.hi[a] = b.hi[a] < h[a] ? h[a] : b.hi[a];
    }
}
PYR_HD float half_area(const Box3& b) {
    float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    if (dx < 0 || dy < 0 || dz < 0) return 0.0f;
    return dx * dy + dx * dz + dy * dz;
}

// Floats as unsigned keys of the same order (-inf lowest, -0 just below +0), so that integer atomicMin / atomicMax accumulate
// float bounds. No NaN reaches a builder (pyr_scene_create refuses coordinates that are not finite).
PYR_HD uint32_t float_bits(float f) {
    union {
        float f;
        uint32_t u;
    } v;
    v.f = f;
    return v.u;
}
PYR_HD float bits_float(uint32_t u) {
    union {
        float f;
        uint32_t u;
    } v;
    v.u = u;
    return v.f;
}
PYR_HD uint32_t key_of(float f) {
    const uint32_t u = float_bits(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
PYR_HD float float_of(uint32_t k) { return bits_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
constexpr uint32_t kKeyPosInf = 0xFF800000u; // key_of(+inf): an empty lower bound
constexpr uint32_t kKeyNegInf = 0x007FFFFFu; // key_of(-inf): an empty upper bound

PYR_HD float centroid(float lo, float hi) { return 0.5f * lo + 0.5f * hi; }

// (int)x as the host builder's compiler converts it (x86 cvttss2si: what does not fit an int becomes INT_MIN), spelled out so
// that the device agrees where a degenerate extent makes `scale` infinite
PYR_HD int to_int(float x) { return (x >= -2147483648.0f && x < 2147483648.0f) ? (int)x : (-2147483647 - 1); }
PYR_HD float bin_scale(float extent) { return (float)kBins / extent; }
PYR_HD int bin_index(float c, float cbox_lo, float scale) {
    const int b = to_int((c - cbox_lo) * scale);
    const int clamped = b > 0 ? b : 0;
    return clamped < kBins - 1 ? clamped : kBins - 1;
}

PYR_HD uint32_t ceil_log2(uint32_t n) {
    uint32_t l = 0;
    while ((1u << l) < n) ++l;
    return l;
}
PYR_HD float leaf_tests(uint32_t count, bool in_pairs) { return in_pairs ? (float)((count + 1u) & ~1u) : (float)count; }
PYR_HD bool force_median(uint32_t count, uint32_t depth, uint32_t depth_bound) {
    return depth + ceil_log2((count + kLeafMax - 1) / kLeafMax) + 1 >= depth_bound;
}

enum : uint32_t { KIND_PENDING = 0, KIND_LEAF = 1, KIND_SPLIT = 2, KIND_MEDIAN = 3 };

struct Decision {
    uint32_t kind; // KIND_LEAF, KIND_SPLIT (bins <= `bin` on `axis` go to slot 0), KIND_MEDIAN (count / 2 smallest on `axis`)
    int axis, bin;
    float lo, scale;     // KIND_SPLIT: bin_index(c, lo, scale)
    uint32_t left_count; // references of slot 0
};

// The candidate loop of the object split: the cheapest of the (kBins - 1) x 3 planes between bins that have references on both
// sides -- axis 0..2, bins ascending, the first of equal costs. `bins.box(axis, bin)` / `bins.count(axis, bin)` are read only for
// axes whose centroid extent is positive. axis < 0: no such plane (every centroid extent is zero).
struct Candidate {
    float cost; // left area x left tests + right area x right tests
    int axis, bin;
    uint32_t left_count; // references in bins <= `bin`
};
template <class Bins>
PYR_HD Candidate best_candidate(const Box3& cbox, const Bins& bins, bool in_pairs) {
    Candidate best;
    best.cost = pos_inf(), best.axis = -1, best.bin = -1, best.left_count = 0;
    for (int a = 0; a < 3; ++a) {
        float extent = cbox.hi[a] - cbox.lo[a];
        if (!(extent > 0.0f)) continue;
        float right_area[kBins];
        uint32_t right_count[kBins];
        Box3 acc = empty_box();
        uint32_t cnt = 0;
        for (int b = kBins - 1; b > 0; --b) {
            const Box3 bb = bins.box(a, b);
            grow(acc, bb.lo, bb.hi);
            cnt += bins.count(a, b);
            right_area[b] = half_area(acc);
            right_count[b] = cnt;
        }
        Box3 left = empty_box();
        uint32_t lcnt = 0;
        for (int b = 0; b < kBins - 1; ++b) {
            const Box3 bb = bins.box(a, b);
            grow(left, bb.lo, bb.hi);
            lcnt += bins.count(a, b);
            if (lcnt == 0 || right_count[b + 1] == 0) continue;
            float cost = half_area(left) * leaf_tests(lcnt, in_pairs) + right_area[b + 1] * leaf_tests(right_count[b + 1], in_pairs);
            if (cost < best.cost) {
                best.cost = cost;
                best.axis = a;
                best.bin = b;
                best.left_count = lcnt;
            }
        }
    }
    return best;
}

// SAH termination: a leaf costs its primitive tests, a split one node visit plus the children's share of the parent's area
PYR_HD float split_cost(float children_cost, const Box3& box) {
    float parent_area = half_area(box);
    return kNodeCost + (parent_area > 0.0f ? children_cost / parent_area : pos_inf());
}
// the median rule's axis: the widest centroid extent, the first of equals
PYR_HD int widest_axis(const Box3& cbox) {
    int a = 0;
    float w = -1.0f;
    for (int k = 0; k < 3; ++k) {
        float e = cbox.hi[k] - cbox.lo[k];
        if (e > w) {
            w = e;
            a = k;
        }
    }
    return a;
}

// What becomes of one node, from its bins (not read when the depth rule forces the median): a leaf, a SAH split, or the median
// split (coincident centroids, or depth budget exhausted). The candidates of a SAH split have references on both sides by the
// same bin_index the partition uses, so a chosen split never leaves a side empty.
template <class Bins>
PYR_HD Decision choose_split(uint32_t count, uint32_t depth, const Box3& box, const Box3& cbox, const Bins& bins, bool in_pairs, uint32_t depth_bound) {
    Decision d;
    d.kind = KIND_LEAF, d.axis = 0, d.bin = -1, d.lo = 0.0f, d.scale = 0.0f, d.left_count = 0;
    if (count <= 1) return d;
    if (!force_median(count, depth, depth_bound)) {
        const Candidate best = best_candidate(cbox, bins, in_pairs);
        if (best.axis >= 0) {
            if (count <= kLeafMax && leaf_tests(count, in_pairs) <= split_cost(best.cost, box)) return d;
            float extent = cbox.hi[best.axis] - cbox.lo[best.axis];
            d.kind = KIND_SPLIT, d.axis = best.axis, d.bin = best.bin;
            d.lo = cbox.lo[best.axis], d.scale = bin_scale(extent), d.left_count = best.left_count;
            return d;
        }
    }
    if (count <= kLeafMax) return d;
    d.kind = KIND_MEDIAN, d.axis = widest_axis(cbox), d.left_count = count / 2;
    return d;
}

// The median rule's order: by centroid on the axis, then by shape code. Shape codes are distinct within a tree without spatial
// splits, so this is a strict total order and the count / 2 smallest are the same set whatever order the references are held in.
PYR_HD bool median_before(float c, uint32_t shape, float other_c, uint32_t other_shape) { return c < other_c || (c == other_c && shape < other_shape); }

// One node of a level-wise build, in the order the builders made them (task 0 is the root's range; its children are the two
// slots of node 0). What the finishing pass (finish_levelwise, bvh.cpp) turns into a BuiltBvh.
struct Task {
    uint32_t begin, end;  // references [begin, end) of the level's reference array
    int32_t parent;       // task whose node holds this one as a child, -1 for the root's range
    uint32_t slot;        // which child of it
    uint32_t depth;       // edges from the root node
    uint32_t kind;        // KIND_*
    uint32_t child0;      // KIND_SPLIT / KIND_MEDIAN: the task of slot 0; slot 1 is child0 + 1
    int32_t axis, bin;    // the decision, for the partition
    float lo, scale;
    uint32_t cursor[2];   // device: references placed so far on each side
    uint32_t box[6];      // lo xyz, hi xyz as keys (key_of)
    uint32_t cbox[6];     // centroid bounds, likewise
};
static_assert(sizeof(Task) == 100, "Task is shared with the device as 25 words");

PYR_HD Box3 box_of_keys(const uint32_t* k) {
    Box3 b;
    for (int a = 0; a < 3; ++a) b.lo[a] = float_of(k[a]), b.hi[a] = float_of(k[3 + a]);
    return b;
}
PYR_HD void empty_keys(uint32_t* k) {
    for (int a = 0; a < 3; ++a) k[a] = kKeyPosInf, k[3 + a] = kKeyNegInf;
}

// ---------------------------------------------------------------------------------------------------------------- refit
// The rules of a refit: the boxes of a tree whose topology stays, from primitives that moved. The host
// rehearsal (refit_bvh / refit_wide, bvh.cpp) and the device kernels (kernels/refit.hip) call these and nothing else, and scene
// creation takes its primitive bounds, its padding and a stored box's padding from here too.

// Bounded::aabb of a triangle [3][3] and of a sphere (centre, radius), as std::min / std::max nest them at scene creation
PYR_HD void triangle_bounds(const float* p, float* lo, float* hi) {
    for (int a = 0; a < 3; ++a) {
        const float l = p[6 + a] < p[3 + a] ? p[6 + a] : p[3 + a], h = p[3 + a] < p[6 + a] ? p[6 + a] : p[3 + a];
        lo[a] = l < p[a] ? l : p[a];
        hi[a] = p[a] < h ? h : p[a];
    }
}
PYR_HD void sphere_bounds(const float* s, float* lo, float* hi) {
    for (int a = 0; a < 3; ++a) lo[a] = s[a] - s[3], hi[a] = s[a] + s[3];
}
// the largest coordinate of a set of boxes, one box at a time (never negative, so its bits order like the floats do)
PYR_HD float grow_max_abs(float m, const float* lo, const float* hi) {
    for (int a = 0; a < 3; ++a) {
        const float l = lo[a] < 0.0f ? -lo[a] : lo[a], h = hi[a] < 0.0f ? -hi[a] : hi[a];
        const float w = l < h ? h : l;
        m = m < w ? w : m;
    }
    return m;
}
// the padding of every stored box: 16 ulps of the largest coordinate (bvh.cpp bvh_padding says why)
PYR_HD float padding_of(float max_abs) { return 16.0f * 1.1920929e-7f * max_abs; }
// a stored box: the exact box moved outward by the padding. x - pad and x + pad are monotone in x, so the union of padded boxes
// is the padded union, bit for bit
PYR_HD Box3 padded(const Box3& b, float pad) {
    Box3 r;
    for (int a = 0; a < 3; ++a) r.lo[a] = b.lo[a] - pad, r.hi[a] = b.hi[a] + pad;
    return r;
}
// a leaf's stored box: the exact min / max of its primitives' bounds, padded. `bounds.get(i, lo, hi)`: the bounds of the
// primitive at leaf-order position i
template <class Bounds>
PYR_HD Box3 refit_leaf_box(const Bounds& bounds, uint32_t first, uint32_t count, float pad) {
    Box3 b = empty_box();
    for (uint32_t i = 0; i < count; ++i) {
        float lo[3], hi[3];
        bounds.get(first + i, lo, hi);
        grow(b, lo, hi);
    }
    return padded(b, pad);
}
constexpr int32_t kNoChild = -2147483647 - 1; // bvh.h kEmptyChild: a slot of a four-child node that holds nothing (its box is NaN)
PYR_HD uint32_t leaf_first(int32_t code) { return (uint32_t)(-1 - code) >> 3; }
PYR_HD uint32_t leaf_count(int32_t code) { return (uint32_t)(-1 - code) & 7u; }
// an inner child's stored box: the union of the boxes that child stores (Node64: two slots, Node128: four). An empty slot of a
// four-child node is skipped; an empty leaf of a two-child node holds the empty box, which grows nothing
template <class Node>
PYR_HD Box3 refit_inner_box(const Node& child, int slots) {
    Box3 b = empty_box();
    for (int k = 0; k < slots; ++k) {
        if (child.child[k] == kNoChild) continue;
        const float lo[3] = {child.lo_x[k], child.lo_y[k], child.lo_z[k]}, hi[3] = {child.hi_x[k], child.hi_y[k], child.hi_z[k]};
        grow(b, lo, hi);
    }
    return b;
}
// One node of a refit: every slot's box anew -- a leaf's from the primitives, an inner child's from that child's node, which a
// bottom-up order has finished already. Empty slots and empty leaves keep their boxes.
template <class Node, class Bounds>
PYR_HD void refit_node(Node& node, int slots, const Node* nodes, const Bounds& bounds, float pad) {
    for (int k = 0; k < slots; ++k) {
        const int32_t code = node.child[k];
        if (code == kNoChild || (code < 0 && leaf_count(code) == 0)) continue;
        const Box3 b = code >= 0 ? refit_inner_box(nodes[code], slots) : refit_leaf_box(bounds, leaf_first(code), leaf_count(code), pad);
        node.lo_x[k] = b.lo[0], node.lo_y[k] = b.lo[1], node.lo_z[k] = b.lo[2];
        node.hi_x[k] = b.hi[0], node.hi_y[k] = b.hi[1], node.hi_z[k] = b.hi[2];
    }
}
// a node's height in the refit schedule: 0 when every child is a leaf, else one more than its highest inner child's
template <class Node>
PYR_HD uint32_t refit_height(const Node& node, int slots, const uint32_t* heights) {
    uint32_t h = 0;
    for (int k = 0; k < slots; ++k)
        if (node.child[k] >= 0 && heights[node.child[k]] + 1 > h) h = heights[node.child[k]] + 1;
    return h;
}

} // namespace lvl
} // namespace pyr
