// bvh.h -- host-side builder of the acceleration structure the HIP kernels traverse.
//
// Replaces Bvh::new (pyrite/src/spatial/bvh.rs:13-155). The reference builds a binary tree with one item per leaf,
// 6 SAH buckets on the widest centroid axis, flattened pre-order with skip counts and traversed without near/far
// ordering. None of that layout survives here: the kernels want few, wide, aligned fetches and an ordered
// traversal, so this builder emits 64-byte nodes that hold BOTH children's boxes (one visit = one 64 B fetch =
// two slab tests), leaves of up to 4 primitives stored contiguously in leaf order, 16-bin SAH over all three
// axes, and a hard depth bound so the per-lane traversal stack in LDS can be sized from the tree itself.
// Closest-hit results do not depend on the tree (only exact-distance ties do).
#pragma once
#include <cstdint>
#include <climits>
#include <cstddef>
#include <vector>

#include "bvh_level.h"

namespace pyr {

struct PrimBounds {
    float lo[3], hi[3];
    uint32_t shape; // (PyrShapeKind << 30) | index
};

// Two-child node, 64 bytes, read by the kernels as four float4. The two children's bounds are interleaved so that each
// float4 holds two (child 0, child 1) pairs: the kernels test both boxes with packed-fp32 instructions (v_pk_fma_f32) and a
// pair must sit in an aligned register pair. Boxes are padded by a few ulps of the scene's extent at build time
// (build_bvh), which makes the kernels' `t = bound * inv - origin * inv` form of the slab test conservative.
struct alignas(64) Node64 {
    float lo_x[2], lo_y[2]; // [child]
    float lo_z[2], hi_x[2];
    float hi_y[2], hi_z[2];
    int32_t child[2]; // >= 0: node index; < 0: leaf, -1 - ((first_prim << 3) | count), count 0..4 (0 = empty)
    uint32_t pad[2];
};
static_assert(sizeof(Node64) == 64, "node must be 64 bytes");

struct BuiltBvh {
    std::vector<Node64> nodes;        // nodes[0] is the root
    std::vector<uint32_t> prim_order; // shape codes in leaf order
    uint32_t max_depth = 0;           // edges on the longest root-to-leaf path = stack entries an ordered traversal can need
    uint32_t num_leaves = 0;
};

// The builders' constants are defined in bvh_level.h (with their -D knobs), which the device builder compiles too
constexpr uint32_t kMaxLeafPrims = lvl::kLeafMax; // <= 7: the leaf code keeps the count in 3 bits
constexpr uint32_t kMaxBvhDepth = lvl::kDepthMax;
// The SAH counts a leaf's primitives in pairs (an odd one costs a whole test): the render kernels test the triangles of a
// leaf two per step (device_scene.h DevPrimPair). Measured against counting singly: C3 451 -> 457, C5 393 -> 397 Msamples/s
// with the same number of triangle tests (fewer steps); C2's 71-node tree does not change.
#ifndef PYR_SAH_PAIRS
#define PYR_SAH_PAIRS 1
#endif
constexpr float kSahNodeCost = lvl::kNodeCost; // cost of one node visit in units of one primitive test (SAH termination)

inline int32_t encode_leaf(uint32_t first, uint32_t count) { return -1 - (int32_t)((first << 3) | count); }

// `leaves_tested_in_pairs`: the tree's leaves will be tested two triangles per step (the four-child pair tree of a
// triangle-only scene that does not live in LDS), so the SAH counts a leaf of n primitives as n rounded up to even -- only
// when PYR_SAH_PAIRS is on; everything else (sphere scenes, LDS-resident scenes, the binary walk) counts singly.
// `median_splits`, if given, receives how many nodes were split by the median fallback (coincident centroids, or the depth rule).
BuiltBvh build_bvh(const std::vector<PrimBounds>& prims, bool leaves_tested_in_pairs = false, uint32_t* median_splits = nullptr);

// The same tree built level by level: the sequential rehearsal of the device builder (kernels/build.hip).
// Both, like build_bvh, decide by the functions of bvh_level.h. Where no node needs the median fallback the tree is
// build_bvh's (tree_digest below is equal); where one does, the count / 2 references smallest by (centroid, shape code) go to
// slot 0, which may break ties differently from build_bvh's nth_element. `depth_bound` stands in for kMaxBvhDepth in the depth
// rule (tests lower it to reach the forced median on small inputs).
// How the device builder divides a level's nodes (kernels/build_launch.h takes them from here): a node of at most
// kLevelSmallNode references is one wave's; a larger one is shared out in chunks of kLevelChunk references.
constexpr uint32_t kLevelSmallNode = 64;
constexpr uint32_t kLevelChunk = 2048;
struct LevelBuildStats {
    uint32_t levels = 0;        // iterations of the level loop
    uint32_t median_splits = 0; // nodes split by the median rule
    // which paths of the device builder the input takes (tools/bvh_quality.cpp `level` prints them; no builder reads them)
    uint32_t largest_median = 0;           // references of the largest node split by the median rule
    uint32_t medians_positive_small = 0;   // median splits whose centroid extent on the chosen axis is positive: nodes of at most
    uint32_t medians_positive_large = 0;   // kLevelSmallNode references, and larger ones
    uint32_t medians_infinite_scale = 0;   // of both, those whose extent is so small that bin_scale(extent) is infinite
    uint32_t largest_forced_median = 0;    // references of the largest node the depth rule (force_median) sent to the median rule
    uint32_t most_large_nodes = 0;         // nodes of more than kLevelSmallNode references in one level, at most
    uint32_t most_chunks = 0;              // chunks of kLevelChunk references of one such node, at most
    uint32_t degenerate_axis_splits = 0;   // SAH splits of such nodes with a zero centroid extent on one or two axes
    float root_centroid_extent[3] = {0, 0, 0};
};
BuiltBvh build_bvh_levelwise(const std::vector<PrimBounds>& prims, bool leaves_tested_in_pairs = false, uint32_t depth_bound = kMaxBvhDepth,
                             LevelBuildStats* stats = nullptr);
// The padding build_bvh gives every stored box: 16 ulps of the largest coordinate.
float bvh_padding(const std::vector<PrimBounds>& prims);
// A scene of at most kMaxLeafPrims primitives: one leaf under the root, as build_bvh makes it (shape codes ascending).
BuiltBvh single_leaf_bvh(const std::vector<PrimBounds>& prims);
// The tasks of a level-wise build (host rehearsal or device) -> build_bvh's layout: nodes numbered in pre-order, slot 0 first;
// prim_order in the same leaf order, each leaf's shape codes ascending (`leaf_shapes[i]`: the shape code at reference position
// i of the leaf that covers it). False when the tasks do not describe a tree over `leaf_shapes` (nothing is trusted blindly:
// the device builder's output passes through here).
bool finish_levelwise(const std::vector<lvl::Task>& tasks, const std::vector<uint32_t>& leaf_shapes, float pad, BuiltBvh& out, LevelBuildStats* stats);
// Pre-order walk of the binary tree: every child's stored box (-0.0f read as +0.0f), depth and slot, and a leaf's shape codes
// sorted. Node numbers and the order inside a leaf do not enter, so equal digests mean the same tree.
uint64_t tree_digest(const BuiltBvh& bvh);

// Spatial splits (SBVH, Stich et al. 2009) for a triangle-only pair tree: at every node where the best object split's two
// children overlap by more than `alpha` x the root's area, a binned split of space (kSpatialBins planes per axis) competes
// with it; a triangle that straddles the chosen plane is clipped against it -- the triangle itself, not its box -- and goes
// to both sides, unless keeping it whole on one side is cheaper. The references may then repeat a triangle (never twice in
// one leaf), at most `max_duplication` x the triangles in all: each node passes the budget it has left on to its children in
// proportion to their references, so the tree is the same whatever order it were built in. Clipped boxes are rounded
// outward and never leave the triangle's own box, so build_bvh's padding argument holds for them unchanged.
struct SpatialSplits {
    const float* tri_positions = nullptr; // 9 floats per triangle, indexed by the shape code's index
    float alpha = 1.0e-5f;
    float max_duplication = 1.4f;
};
constexpr int kSpatialBins = 32;
BuiltBvh build_bvh_spatial(const std::vector<PrimBounds>& prims, const SpatialSplits& spatial);
// PYRITE_SPATIAL_SPLITS=1 (read at scene creation) builds the pair tree with spatial splits; unset or "0", with build_bvh's
// object splits. Off by default: on C3's mesh they raise the tree's SAH cost instead of lowering it (DESIGN §8b,
// profiles/r05_bvh_quality.txt) and take 10x as long to build.
bool spatial_splits_wanted();

// Four-child node, 128 bytes = one L2 line, read as eight float4: lo.x[4] lo.y[4] lo.z[4] hi.x[4] hi.y[4] hi.z[4] child[4]
// pad[4]. Built by collapsing the binary tree (collapse_to_wide: the child with the largest surface area is replaced by its own
// two children until the node has four; the pair tree: collapse_to_wide_sah below): a ray then makes about half as many dependent
// node fetches. Used by the resumable traversal on scenes that do not live in LDS, where the walk is latency bound; unused slots
// hold kEmptyChild and are never entered.
struct alignas(128) Node128 {
    float lo_x[4], lo_y[4], lo_z[4], hi_x[4], hi_y[4], hi_z[4];
    int32_t child[4]; // >= 0: Node128 index; < 0: leaf code as in Node64; kEmptyChild: nothing
    uint32_t pad[4];
};
static_assert(sizeof(Node128) == 128, "wide node must be 128 bytes");
constexpr int32_t kEmptyChild = INT32_MIN;

struct WideBvh {
    std::vector<Node128> nodes; // nodes[0] is the root
    uint32_t max_depth = 0;     // node levels on the longest path
    uint32_t stack_need = 0;    // entries an ordered traversal can hold at once: max over paths of sum(children - 1)
};
WideBvh collapse_to_wide(const BuiltBvh& bvh);
// The cost-driven collapse (Ylitie et al. 2017, for four-child nodes): dynamic programming over the binary tree decides for
// every subtree whether it becomes a wide node, a leaf (at most kMaxLeafPrims references, tested two per step) or is spread
// over up to four slots of its parent, by surface area x (kWideNodeCost per visit, kWidePairCost per pair step). Unlike
// the greedy rule above it weighs opening a node against stopping, and may turn a small subtree into one leaf. A pair step is
// weighed at 1.5 node visits: at 1.0 the collapse merges leaves freely (two leaves of two triangles into one of four: the same
// pair records, but all four triangles are tested whenever the merged box is hit) -- C3 +16 % triangle tests for -8 % box tests;
// from 1.2 on the steps per ray are the same (tools/bvh_quality.cpp) and the triangle tests within 3 % of the greedy tree's.
constexpr float kWideNodeCost = 1.0f;
constexpr float kWidePairCost = 1.5f;
WideBvh collapse_to_wide_sah(const BuiltBvh& bvh);
// PYRITE_WIDE_COLLAPSE (read at scene creation): "greedy" collapses the pair tree by the greedy rule (A/B); anything else,
// or unset, by cost
bool cost_driven_collapse_wanted();

// ---- refit: new boxes for a tree whose topology, prim_order and leaf sizes stay. `prims` are the scene's
// primitives in pack order (spheres, then triangles, each kind by index: what the tree was built from), with their new bounds.
// Sequential rehearsals of kernels/refit.hip on bvh_level.h's refit rules: a leaf's box is the exact box of its primitives,
// padded by bvh_padding(prims); an inner child's the union of that child's stored boxes. With unchanged bounds the nodes come
// out byte for byte as the builder stored them. Not for trees with spatial splits, whose leaves hold clipped boxes.
void refit_bvh(BuiltBvh& bvh, const std::vector<PrimBounds>& prims);
// The four-child tree collapsed from `bvh` (its leaf codes index bvh.prim_order), likewise.
void refit_wide(WideBvh& wide, const BuiltBvh& bvh, const std::vector<PrimBounds>& prims);
// The order a refit visits a tree's nodes in: grouped by height (lvl::refit_height), nodes whose children are all leaves first.
// order[begin[h] .. begin[h + 1]) are the nodes of height h; a node's inner children all have smaller heights.
struct RefitSchedule {
    std::vector<uint32_t> order, begin;
};
RefitSchedule refit_schedule(const Node64* nodes, size_t count);
RefitSchedule refit_schedule(const Node128* nodes, size_t count);
// Sum of lvl::half_area over every stored child box of the binary tree, in f64 in node order: the SAH's measure of what a
// refit has done to the tree (PyrUpdateInfo::area_ratio is this now over this at the last build).
double child_area_sum(const Node64* nodes, size_t count);

} // namespace pyr
