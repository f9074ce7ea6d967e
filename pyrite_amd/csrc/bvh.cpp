// bvh.cpp -- binned-SAH builders for the 64-byte two-child node layout (see bvh.h). The SAH rules are bvh_level.h's.
#include "bvh.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>

namespace pyr {
namespace {

constexpr int kBins = lvl::kBins;
constexpr float kInf = std::numeric_limits<float>::infinity();

// lvl::Box3 that starts empty; the arithmetic is bvh_level.h's
struct Box : lvl::Box3 {
    Box() : lvl::Box3(lvl::empty_box()) {}
    void grow(const float* l, const float* h) { lvl::grow(*this, l, h); }
    void grow(const lvl::Box3& b) { lvl::grow(*this, b.lo, b.hi); }
    float half_area() const { return lvl::half_area(*this); }
};

// The object split's bins of one node on the host: what lvl::best_candidate and lvl::choose_split read
struct Bins {
    Box b[3][kBins];
    uint32_t c[3][kBins] = {};
    void add(int a, int k, const float* lo, const float* hi) {
        b[a][k].grow(lo, hi);
        c[a][k]++;
    }
    const lvl::Box3& box(int a, int k) const { return b[a][k]; }
    uint32_t count(int a, int k) const { return c[a][k]; }
};

Node64 empty_node64() {
    Node64 nd{};
    for (int c = 0; c < 2; ++c) {
        nd.lo_x[c] = nd.lo_y[c] = nd.lo_z[c] = kInf; // an empty child leads to an empty leaf at worst
        nd.hi_x[c] = nd.hi_y[c] = nd.hi_z[c] = -kInf;
        nd.child[c] = encode_leaf(0, 0);
    }
    return nd;
}

void set_child64(Node64& p, int slot, int32_t code, const lvl::Box3& box, float pad) {
    const lvl::Box3 stored = lvl::padded(box, pad);
    p.child[slot] = code;
    p.lo_x[slot] = stored.lo[0], p.lo_y[slot] = stored.lo[1], p.lo_z[slot] = stored.lo[2];
    p.hi_x[slot] = stored.hi[0], p.hi_y[slot] = stored.hi[1], p.hi_z[slot] = stored.hi[2];
}

} // namespace

// Padding of every stored box: 16 ulps of the largest coordinate in the scene. The kernels compute slab distances as
// fma(bound, 1/d, -(o * 1/d)), whose error is half an ulp of |o / d| -- in world units half an ulp of the ray origin,
// which lies inside the scene -- so a padded box is never missed by a ray that hits something inside the exact box.
float bvh_padding(const std::vector<PrimBounds>& prims) {
    float max_abs = 0.0f;
    for (const PrimBounds& p : prims) max_abs = lvl::grow_max_abs(max_abs, p.lo, p.hi);
    return lvl::padding_of(max_abs);
}

BuiltBvh build_bvh(const std::vector<PrimBounds>& prims, bool leaves_tested_in_pairs, uint32_t* median_splits) {
    struct Ref {
        float lo[3], hi[3], c[3];
        uint32_t shape;
    };
    // Build the subtree of [begin, end) and store it as child `slot` of node `parent`; parent < 0: the range of the root, whose two
    // halves become the children of node 0. Depth counts edges from the root node: its children sit at depth 1.
    struct Task {
        uint32_t begin, end, depth;
        int32_t parent;
        int slot;
    };
    BuiltBvh out;
    if (median_splits) *median_splits = 0;
    const uint32_t n = (uint32_t)prims.size();
    std::vector<Ref> refs(n);
    for (uint32_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) {
            refs[i].lo[a] = prims[i].lo[a];
            refs[i].hi[a] = prims[i].hi[a];
            refs[i].c[a] = lvl::centroid(prims[i].lo[a], prims[i].hi[a]);
        }
        refs[i].shape = prims[i].shape;
    }
    const float pad = bvh_padding(prims);
    // The root is always a node; a scene with <= kMaxLeafPrims primitives hangs one leaf under it.
    out.nodes.push_back(empty_node64());
    if (n == 0) return out;

    // PYR_SAH_PAIRS=1: the render kernels test a leaf's triangles two per step (DevPrimPair), so an odd triangle costs a whole step.
    const bool in_pairs = PYR_SAH_PAIRS && leaves_tested_in_pairs;
    auto make_leaf = [&](const Task& t, const Box& box) {
        const uint32_t first = (uint32_t)out.prim_order.size();
        for (uint32_t i = t.begin; i < t.end; ++i) out.prim_order.push_back(refs[i].shape);
        set_child64(out.nodes[t.parent], t.slot, encode_leaf(first, t.end - t.begin), box, pad);
        out.num_leaves++;
        out.max_depth = std::max(out.max_depth, t.depth);
    };
    if (n <= kMaxLeafPrims) {
        Box box;
        for (const Ref& r : refs) box.grow(r.lo, r.hi);
        make_leaf(Task{0, n, 1, 0, 0}, box);
        return out;
    }
    std::vector<Task> stack{Task{0, n, 0, -1, 0}}; // more than kMaxLeafPrims references: choose_split never makes this one a leaf
    while (!stack.empty()) {
        const Task t = stack.back();
        stack.pop_back();
        Box box, cbox;
        for (uint32_t i = t.begin; i < t.end; ++i) {
            box.grow(refs[i].lo, refs[i].hi);
            cbox.grow(refs[i].c, refs[i].c);
        }
        Bins bins;
        for (int a = 0; a < 3; ++a) {
            const float extent = cbox.hi[a] - cbox.lo[a];
            if (!(extent > 0.0f)) continue;
            const float scale = lvl::bin_scale(extent);
            for (uint32_t i = t.begin; i < t.end; ++i) bins.add(a, lvl::bin_index(refs[i].c[a], cbox.lo[a], scale), refs[i].lo, refs[i].hi);
        }
        const lvl::Decision d = lvl::choose_split(t.end - t.begin, t.depth, box, cbox, bins, in_pairs, kMaxBvhDepth);
        if (d.kind == lvl::KIND_LEAF) {
            make_leaf(t, box);
            continue;
        }
        const uint32_t mid = t.begin + d.left_count;
        const int a = d.axis;
        if (d.kind == lvl::KIND_SPLIT) { // both sides have references: the candidates were counted by this very bin_index
            std::partition(refs.begin() + t.begin, refs.begin() + t.end, [&](const Ref& r) { return lvl::bin_index(r.c[a], d.lo, d.scale) <= d.bin; });
        } else {
            if (median_splits) ++*median_splits;
            std::nth_element(refs.begin() + t.begin, refs.begin() + mid, refs.begin() + t.end, [a](const Ref& x, const Ref& y) { return x.c[a] < y.c[a]; });
        }
        int32_t id = 0;
        if (t.parent >= 0) {
            id = (int32_t)out.nodes.size();
            out.nodes.push_back(empty_node64());
            set_child64(out.nodes[t.parent], t.slot, id, box, pad);
        }
        stack.push_back(Task{mid, t.end, t.depth + 1, id, 1});
        stack.push_back(Task{t.begin, mid, t.depth + 1, id, 0});
    }
    return out;
}

namespace {

struct SRef {
    Box box; // the part of the triangle this reference stands for (its whole box unless it was clipped)
    uint32_t shape;
    float c(int a) const { return lvl::centroid(box.lo[a], box.hi[a]); }
};

bool box_valid(const Box& b) { return b.lo[0] <= b.hi[0] && b.lo[1] <= b.hi[1] && b.lo[2] <= b.hi[2]; }

Box box_and(const Box& x, const Box& y) {
    Box r;
    for (int a = 0; a < 3; ++a) r.lo[a] = std::max(x.lo[a], y.lo[a]), r.hi[a] = std::min(x.hi[a], y.hi[a]);
    return r;
}

// Bounds of the part of triangle `v` whose coordinate `axis` lies in [a, b], intersected with `clip`; an invalid box when that part
// is empty. The polygon's corners are the triangle's corners inside the slab and the edges' crossings of its two planes; the
// crossings are computed in double and rounded outward (with a margin far above the double rounding error), and on `axis` the
// bounds are the float corners and planes themselves, so the box contains every point of the part.
Box clip_triangle(const float* v, int axis, float a, float b, const Box& clip) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double mag = 0.0;
    for (int k = 0; k < 9; ++k) mag = std::max(mag, (double)std::fabs(v[k]));
    auto add = [&](const double* p) {
        for (int k = 0; k < 3; ++k) lo[k] = std::min(lo[k], p[k]), hi[k] = std::max(hi[k], p[k]);
    };
    for (int e = 0; e < 3; ++e) {
        const float* p = v + 3 * e;
        const float* q = v + 3 * ((e + 1) % 3);
        const double P[3] = {p[0], p[1], p[2]}, Q[3] = {q[0], q[1], q[2]};
        if (P[axis] >= a && P[axis] <= b) add(P);
        for (const float plane : {a, b}) {
            if ((P[axis] < plane && Q[axis] > plane) || (P[axis] > plane && Q[axis] < plane)) {
                const double t = ((double)plane - P[axis]) / (Q[axis] - P[axis]);
                double X[3];
                for (int k = 0; k < 3; ++k) X[k] = P[k] + t * (Q[k] - P[k]);
                X[axis] = plane;
                add(X);
            }
        }
    }
    Box r;
    if (!(lo[0] <= hi[0])) return r;
    const double slack = 1.0e-12 * mag;
    for (int k = 0; k < 3; ++k) {
        if (k == axis) { // corners and planes: float values already
            r.lo[k] = (float)lo[k], r.hi[k] = (float)hi[k];
            continue;
        }
        const double l = lo[k] - slack, h = hi[k] + slack;
        float fl = (float)l, fh = (float)h;
        if ((double)fl > l) fl = std::nextafter(fl, -kInf);
        if ((double)fh < h) fh = std::nextafter(fh, kInf);
        r.lo[k] = fl, r.hi[k] = fh;
    }
    return box_and(r, clip);
}

} // namespace

bool spatial_splits_wanted() {
    const char* e = std::getenv("PYRITE_SPATIAL_SPLITS");
    return e && e[0] == '1';
}

bool cost_driven_collapse_wanted() {
    const char* e = std::getenv("PYRITE_WIDE_COLLAPSE");
    return !(e && std::strcmp(e, "greedy") == 0);
}

BuiltBvh build_bvh_spatial(const std::vector<PrimBounds>& prims, const SpatialSplits& spatial) {
    BuiltBvh out;
    const uint32_t n = (uint32_t)prims.size();
    const float* tri = spatial.tri_positions;
    std::vector<SRef> refs(n);
    for (uint32_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) refs[i].box.lo[a] = prims[i].lo[a], refs[i].box.hi[a] = prims[i].hi[a];
        refs[i].shape = prims[i].shape;
    }
    const float pad = bvh_padding(prims); // clipped boxes lie inside the triangles' own boxes, so the largest coordinate is the same
    out.nodes.push_back(empty_node64());
    if (n == 0) return out;

    const bool in_pairs = PYR_SAH_PAIRS != 0;
    auto leaf_tests = [in_pairs](uint32_t count) { return lvl::leaf_tests(count, in_pairs); };
    Box root_box;
    for (const SRef& r : refs) root_box.grow(r.box);
    const float min_overlap = spatial.alpha * root_box.half_area();
    const uint64_t budget = (uint64_t)std::max(0.0, std::floor((double)spatial.max_duplication * n) - n);

    auto make_leaf = [&](const std::vector<SRef>& rs, uint32_t depth, int32_t parent, int slot, const Box& box) {
        const uint32_t first = (uint32_t)out.prim_order.size();
        for (const SRef& r : rs) out.prim_order.push_back(r.shape);
        set_child64(out.nodes[parent], slot, encode_leaf(first, (uint32_t)rs.size()), box, pad);
        out.num_leaves++;
        out.max_depth = std::max(out.max_depth, depth);
    };

    // Builds the subtree of `rs` as child `slot` of `parent` (depth counts edges from the root; the root's own range is split
    // into its two children at depth 1, as in build_bvh). `extra`: references this subtree may add by splitting.
    auto build = [&](auto&& self, std::vector<SRef>& rs, uint32_t depth, int32_t parent, int slot, uint64_t extra) -> void {
        const uint32_t count = (uint32_t)rs.size();
        Box box, cbox;
        for (const SRef& r : rs) {
            box.grow(r.box);
            const float c[3] = {r.c(0), r.c(1), r.c(2)};
            cbox.grow(c, c);
        }
        const bool is_root = parent < 0;
        if (!is_root && count <= 1) return make_leaf(rs, depth, parent, slot, box);
        // the binned object split over the references' centroids, by build_bvh's rules
        lvl::Candidate obj;
        obj.cost = kInf, obj.axis = -1, obj.bin = -1, obj.left_count = 0;
        Box obj_left, obj_right;
        if (!lvl::force_median(count, depth, kMaxBvhDepth)) {
            Bins bins;
            for (int a = 0; a < 3; ++a) {
                const float extent = cbox.hi[a] - cbox.lo[a];
                if (!(extent > 0.0f)) continue;
                const float scale = lvl::bin_scale(extent);
                for (const SRef& r : rs) bins.add(a, lvl::bin_index(r.c(a), cbox.lo[a], scale), r.box.lo, r.box.hi);
            }
            obj = lvl::best_candidate(cbox, bins, in_pairs);
            if (obj.axis >= 0) { // its two children's boxes, grown in the candidate loop's order
                for (int b = 0; b <= obj.bin; ++b) obj_left.grow(bins.box(obj.axis, b));
                for (int b = kBins - 1; b > obj.bin; --b) obj_right.grow(bins.box(obj.axis, b));
            }
        }
        // binned spatial split, where the object split's children overlap
        float sp_cost = kInf;
        int sp_axis = -1;
        uint32_t sp_left_n = 0, sp_right_n = 0;
        Box sp_left, sp_right;
        float sp_plane = 0.0f;
        const Box overlap = box_and(obj_left, obj_right);
        if (obj.axis >= 0 && extra > 0 && box_valid(overlap) && overlap.half_area() > min_overlap) {
            for (int a = 0; a < 3; ++a) {
                const float extent = box.hi[a] - box.lo[a];
                if (!(extent > 0.0f)) continue;
                float plane[kSpatialBins + 1];
                for (int b = 0; b <= kSpatialBins; ++b) plane[b] = box.lo[a] + extent * ((float)b / (float)kSpatialBins);
                plane[kSpatialBins] = box.hi[a];
                const float scale = (float)kSpatialBins / extent;
                auto bin_of = [&](float x) {
                    int b = std::min(kSpatialBins - 1, std::max(0, (int)((x - box.lo[a]) * scale)));
                    while (b > 0 && x < plane[b]) --b;
                    while (b < kSpatialBins - 1 && x >= plane[b + 1]) ++b;
                    return b;
                };
                Box bin_box[kSpatialBins];
                uint32_t entry[kSpatialBins] = {0}, exit[kSpatialBins] = {0};
                for (const SRef& r : rs) {
                    const int b0 = bin_of(r.box.lo[a]);
                    int b1 = bin_of(r.box.hi[a]);
                    while (b1 > b0 && r.box.hi[a] <= plane[b1]) --b1;
                    entry[b0]++, exit[b1]++;
                    if (b0 == b1) {
                        bin_box[b0].grow(r.box);
                        continue;
                    }
                    const float* v = tri + 9 * (size_t)(r.shape & 0x3FFFFFFFu);
                    for (int b = b0; b <= b1; ++b) {
                        const Box part = clip_triangle(v, a, plane[b], plane[b + 1], r.box);
                        if (box_valid(part)) bin_box[b].grow(part);
                    }
                }
                Box right_box[kSpatialBins];
                uint32_t right_count[kSpatialBins];
                Box acc;
                uint32_t cnt = 0;
                for (int b = kSpatialBins - 1; b > 0; --b) {
                    acc.grow(bin_box[b]);
                    cnt += exit[b];
                    right_box[b] = acc;
                    right_count[b] = cnt;
                }
                Box left;
                uint32_t lcnt = 0;
                for (int b = 0; b < kSpatialBins - 1; ++b) {
                    left.grow(bin_box[b]);
                    lcnt += entry[b];
                    const uint32_t rcnt = right_count[b + 1];
                    if (lcnt == 0 || rcnt == 0 || lcnt >= count || rcnt >= count || lcnt + rcnt - count > extra) continue;
                    const float cost = left.half_area() * leaf_tests(lcnt) + right_box[b + 1].half_area() * leaf_tests(rcnt);
                    if (cost < sp_cost)
                        sp_cost = cost, sp_axis = a, sp_left = left, sp_right = right_box[b + 1], sp_left_n = lcnt, sp_right_n = rcnt,
                        sp_plane = plane[b + 1];
                }
            }
        }
        // this builder's own termination: the better of the two splits decides, and the root always splits
        const bool use_spatial = sp_axis >= 0 && sp_cost < obj.cost;
        if (!is_root && (obj.axis >= 0 || use_spatial) && count <= kMaxLeafPrims &&
            leaf_tests(count) <= lvl::split_cost(use_spatial ? sp_cost : obj.cost, box))
            return make_leaf(rs, depth, parent, slot, box);
        std::vector<SRef> left, right;
        if (use_spatial) {
            // references that straddle the plane are clipped to both sides, or kept whole on one side where that is cheaper
            // (the "unsplitting" of the SBVH paper, judged against the binned children)
            Box bl = sp_left, br = sp_right;
            uint32_t nl = sp_left_n, nr = sp_right_n;
            const int a = sp_axis;
            for (const SRef& r : rs) {
                if (r.box.hi[a] <= sp_plane) {
                    left.push_back(r);
                    continue;
                }
                if (r.box.lo[a] >= sp_plane) {
                    right.push_back(r);
                    continue;
                }
                const float* v = tri + 9 * (size_t)(r.shape & 0x3FFFFFFFu);
                const Box lb = clip_triangle(v, a, -kInf, sp_plane, r.box), rb = clip_triangle(v, a, sp_plane, kInf, r.box);
                if (!box_valid(lb) || !box_valid(rb)) {
                    (box_valid(lb) ? left : right).push_back(SRef{box_valid(lb) ? lb : rb, r.shape});
                    continue;
                }
                Box bl_whole = bl, br_whole = br;
                bl_whole.grow(r.box), br_whole.grow(r.box);
                const float c_split = bl.half_area() * (float)nl + br.half_area() * (float)nr;
                const float c_left = bl_whole.half_area() * (float)nl + br.half_area() * (float)(nr - 1);
                const float c_right = bl.half_area() * (float)(nl - 1) + br_whole.half_area() * (float)nr;
                if (c_left < c_split && c_left <= c_right) {
                    left.push_back(r), bl = bl_whole, nr--;
                } else if (c_right < c_split) {
                    right.push_back(r), br = br_whole, nl--;
                } else {
                    left.push_back(SRef{lb, r.shape});
                    right.push_back(SRef{rb, r.shape});
                }
            }
        } else {
            uint32_t mid = obj.left_count;
            if (obj.axis >= 0) { // both sides have references: the candidates were counted by this very bin_index
                const int a = obj.axis;
                const float lo = cbox.lo[a], scale = lvl::bin_scale(cbox.hi[a] - cbox.lo[a]);
                std::partition(rs.begin(), rs.end(), [&](const SRef& r) { return lvl::bin_index(r.c(a), lo, scale) <= obj.bin; });
            } else { // coincident centroids, or the depth rule: the median on the widest centroid axis
                if (!is_root && count <= kMaxLeafPrims) return make_leaf(rs, depth, parent, slot, box);
                const int a = lvl::widest_axis(cbox);
                mid = count / 2;
                std::nth_element(rs.begin(), rs.begin() + mid, rs.end(), [a](const SRef& x, const SRef& y) { return x.c(a) < y.c(a); });
            }
            left.assign(rs.begin(), rs.begin() + mid);
            right.assign(rs.begin() + mid, rs.end());
        }
        std::vector<SRef>().swap(rs);
        const uint64_t added = left.size() + right.size() - count;
        const uint64_t rest = extra - std::min(extra, added);
        const uint64_t rest_left = rest * left.size() / (left.size() + right.size());
        int32_t id = 0;
        if (!is_root) {
            id = (int32_t)out.nodes.size();
            out.nodes.push_back(empty_node64());
            set_child64(out.nodes[parent], slot, id, box, pad);
        }
        self(self, left, depth + 1, id, 0, rest_left);
        self(self, right, depth + 1, id, 1, rest - rest_left);
    };
    if (n <= kMaxLeafPrims) {
        Box box;
        for (const SRef& r : refs) box.grow(r.box);
        make_leaf(refs, 1, 0, 0, box);
        return out;
    }
    build(build, refs, 0, -1, 0, budget);
    return out;
}

namespace {

// One child of a binary node, as a candidate for a slot of a wide node
struct Slot {
    float lo[3], hi[3];
    int32_t code; // Node64 child code
};
Slot slot_of(const BuiltBvh& bvh, int32_t node, int k) {
    const Node64& n = bvh.nodes[node];
    return Slot{{n.lo_x[k], n.lo_y[k], n.lo_z[k]}, {n.hi_x[k], n.hi_y[k], n.hi_z[k]}, n.child[k]};
}
uint32_t leaf_count(int32_t code) { return (uint32_t)(-1 - code) & 7u; }

// The wide tree whose node for binary node n holds the (at most four) slots `slots_of(n)` gives it -- the rule of a collapse --
// numbered in the order a depth-first walk, last inner slot first, reaches them.
WideBvh emit_wide(const std::function<void(int32_t, std::vector<Slot>&)>& slots_of) {
    WideBvh out;
    struct Task {
        int32_t binary_node; // Node64 index this wide node stands for
        int32_t wide_index;
        uint32_t depth, stack_before;
    };
    out.nodes.emplace_back();
    std::vector<Task> todo{{0, 0, 1, 0}};
    std::vector<Slot> kids;
    while (!todo.empty()) {
        const Task t = todo.back();
        todo.pop_back();
        kids.clear();
        slots_of(t.binary_node, kids);
        Node128 node{};
        for (int k = 0; k < 4; ++k) {
            // an unused slot's box is NaN: every comparison of the slab test fails on it, so the traversal needs no "is there a
            // child" test of its own (an inverted box would not do: the slab test orders each pair of planes itself)
            node.lo_x[k] = node.lo_y[k] = node.lo_z[k] = std::numeric_limits<float>::quiet_NaN();
            node.hi_x[k] = node.hi_y[k] = node.hi_z[k] = std::numeric_limits<float>::quiet_NaN();
            node.child[k] = kEmptyChild;
        }
        const uint32_t pushes = kids.empty() ? 0u : (uint32_t)kids.size() - 1u;
        out.max_depth = std::max(out.max_depth, t.depth);
        out.stack_need = std::max(out.stack_need, t.stack_before + pushes);
        for (size_t k = 0; k < kids.size(); ++k) {
            node.lo_x[k] = kids[k].lo[0], node.lo_y[k] = kids[k].lo[1], node.lo_z[k] = kids[k].lo[2];
            node.hi_x[k] = kids[k].hi[0], node.hi_y[k] = kids[k].hi[1], node.hi_z[k] = kids[k].hi[2];
            if (kids[k].code >= 0) {
                const int32_t index = (int32_t)out.nodes.size();
                out.nodes.emplace_back();
                node.child[k] = index;
                todo.push_back(Task{kids[k].code, index, t.depth + 1, t.stack_before + pushes});
            } else {
                node.child[k] = kids[k].code;
            }
        }
        out.nodes[t.wide_index] = node;
    }
    return out;
}

} // namespace

WideBvh collapse_to_wide(const BuiltBvh& bvh) {
    auto area = [](const Slot& c) { // (0 for a box that is flat on all axes but one)
        float dx = c.hi[0] - c.lo[0], dy = c.hi[1] - c.lo[1], dz = c.hi[2] - c.lo[2];
        return (dx > 0 && dy >= 0 && dz >= 0) || (dy > 0 && dx >= 0 && dz >= 0) || (dz > 0 && dx >= 0 && dy >= 0) ? dx * dy + dy * dz + dz * dx : 0.0f;
    };
    // the inner child with the largest surface area is replaced by its own two children until the node has four
    return emit_wide([&](int32_t n, std::vector<Slot>& real) {
        std::vector<Slot> kids{slot_of(bvh, n, 0), slot_of(bvh, n, 1)};
        while (kids.size() < 4) {
            int best = -1;
            float best_area = -1.0f;
            for (size_t i = 0; i < kids.size(); ++i)
                if (kids[i].code >= 0 && area(kids[i]) > best_area) best_area = area(kids[i]), best = (int)i;
            if (best < 0) break;
            const int32_t inner = kids[best].code;
            kids[best] = slot_of(bvh, inner, 0);
            kids.push_back(slot_of(bvh, inner, 1));
        }
        // drop empty leaves (a binary node with fewer than two real children)
        for (const Slot& c : kids)
            if (c.code >= 0 || leaf_count(c.code) != 0) real.push_back(c);
    });
}

WideBvh collapse_to_wide_sah(const BuiltBvh& bvh) {
    const size_t nn = bvh.nodes.size();
    auto area = [](const Slot& c) {
        const float dx = c.hi[0] - c.lo[0], dy = c.hi[1] - c.lo[1], dz = c.hi[2] - c.lo[2];
        return dx >= 0 && dy >= 0 && dz >= 0 ? dx * dy + dy * dz + dz * dx : 0.0f;
    };
    auto leaf_first = [](int32_t code) { return (uint32_t)(-1 - code) >> 3; };
    auto leaf_cost = [](uint32_t count) { return kWidePairCost * (float)((count + 1u) / 2u); };

    // Per binary node, bottom-up (a child's index is always larger than its parent's): the references under it -- contiguous in
    // prim_order, the builder emits leaves depth first -- and cost[n][i], the least cost of its subtree when it may take up i
    // slots of the wide node above it: i = 1 is one wide node or one leaf, i > 1 also spreads its children over the slots.
    std::vector<uint32_t> total(nn, 0), first(nn, UINT32_MAX);
    std::vector<float> node_area(nn, 0.0f);
    std::vector<std::array<float, 5>> cost(nn);
    std::vector<std::array<int8_t, 5>> pick(nn); // i >= 2: k slots to child 0 (0: child 0 is empty), -1: use i - 1 slots; i = 1: 1 leaf, 0 node
    auto slot_cost = [&](const Slot& c, int i) -> float {
        if (c.code >= 0) return cost[c.code][i];
        const uint32_t cnt = leaf_count(c.code);
        return cnt ? area(c) * leaf_cost(cnt) : 0.0f;
    };
    auto real = [&](const Slot& c) { return c.code >= 0 || leaf_count(c.code) != 0; };
    // least cost of node n's two children spread over exactly up to j slots, and how many of them go to child 0
    auto distribute = [&](size_t n, int j, int& k_best) {
        const Slot c0 = slot_of(bvh, (int32_t)n, 0), c1 = slot_of(bvh, (int32_t)n, 1);
        const bool r0 = real(c0), r1 = real(c1);
        k_best = -1;
        if (!r0 && !r1) return k_best = 0, 0.0f;
        if (!r1) return k_best = j, slot_cost(c0, j);
        if (!r0) return k_best = 0, slot_cost(c1, j);
        float best = kInf;
        for (int k = 1; k < j; ++k) {
            const float c = slot_cost(c0, k) + slot_cost(c1, j - k);
            if (c < best) best = c, k_best = k;
        }
        return best;
    };
    for (size_t n = 0; n < nn; ++n)
        for (int k = 0; k < 2; ++k)
            if (bvh.nodes[n].child[k] >= 0) node_area[bvh.nodes[n].child[k]] = area(slot_of(bvh, (int32_t)n, k));
    for (size_t n = nn; n-- > 0;) {
        for (int k = 0; k < 2; ++k) {
            const Slot c = slot_of(bvh, (int32_t)n, k);
            if (c.code >= 0) {
                total[n] += total[c.code];
                first[n] = std::min(first[n], first[c.code]);
            } else if (leaf_count(c.code)) {
                total[n] += leaf_count(c.code);
                first[n] = std::min(first[n], leaf_first(c.code));
            }
        }
        int k4;
        const float as_node = node_area[n] * kWideNodeCost + distribute(n, 4, k4);
        const float as_leaf = total[n] <= kMaxLeafPrims ? node_area[n] * leaf_cost(total[n]) : kInf;
        cost[n][0] = kInf;
        cost[n][1] = as_leaf < as_node ? as_leaf : as_node;
        pick[n][1] = as_leaf < as_node ? 1 : 0;
        for (int i = 2; i <= 4; ++i) {
            int k;
            const float spread = distribute(n, i, k);
            if (spread < cost[n][i - 1]) {
                cost[n][i] = spread, pick[n][i] = (int8_t)k;
            } else {
                cost[n][i] = cost[n][i - 1], pick[n][i] = -1;
            }
        }
    }
    // the slots a wide node gets for binary node n's children, spread over at most j of them
    auto gather = [&](auto&& self, int32_t n, int j, std::vector<Slot>& kids) -> void {
        int k;
        distribute((size_t)n, j, k);
        for (int side = 0; side < 2; ++side) {
            const Slot c = slot_of(bvh, n, side);
            int i = side == 0 ? k : j - k;
            if (!real(c) || i <= 0) continue;
            if (c.code < 0) {
                kids.push_back(c);
                continue;
            }
            while (i > 1 && pick[c.code][i] < 0) --i;
            if (i > 1) {
                self(self, c.code, i, kids);
            } else if (pick[c.code][1] == 1) {
                Slot leaf = c;
                leaf.code = encode_leaf(first[c.code], total[c.code]);
                kids.push_back(leaf);
            } else {
                kids.push_back(c);
            }
        }
    };
    return emit_wide([&](int32_t n, std::vector<Slot>& kids) { gather(gather, n, 4, kids); });
}

// ------------------------------------------------------------------------------------------------ level-wise build
namespace {

void grow_keys(uint32_t* box, uint32_t* cbox, const PrimBounds& r) {
    for (int a = 0; a < 3; ++a) {
        box[a] = std::min(box[a], lvl::key_of(r.lo[a]));
        box[3 + a] = std::max(box[3 + a], lvl::key_of(r.hi[a]));
        const uint32_t c = lvl::key_of(lvl::centroid(r.lo[a], r.hi[a]));
        cbox[a] = std::min(cbox[a], c);
        cbox[3 + a] = std::max(cbox[3 + a], c);
    }
}

} // namespace

BuiltBvh single_leaf_bvh(const std::vector<PrimBounds>& prims) {
    BuiltBvh out;
    out.nodes.push_back(empty_node64());
    if (prims.empty()) return out;
    lvl::Box3 box = lvl::empty_box();
    for (const PrimBounds& p : prims) {
        lvl::grow(box, p.lo, p.hi);
        out.prim_order.push_back(p.shape);
    }
    std::sort(out.prim_order.begin(), out.prim_order.end());
    set_child64(out.nodes[0], 0, encode_leaf(0, (uint32_t)prims.size()), box, bvh_padding(prims));
    out.num_leaves = 1;
    out.max_depth = 1;
    return out;
}

bool finish_levelwise(const std::vector<lvl::Task>& tasks, const std::vector<uint32_t>& leaf_shapes, float pad, BuiltBvh& out, LevelBuildStats* stats) {
    out = BuiltBvh{};
    out.nodes.push_back(empty_node64());
    const size_t nt = tasks.size();
    if (nt == 0 || tasks[0].kind < lvl::KIND_SPLIT || (size_t)tasks[0].child0 + 1 >= nt) return false;
    out.nodes.reserve(nt / 2 + 1); // every inner task is a node, every other one a leaf
    out.prim_order.reserve(leaf_shapes.size());
    uint32_t medians = 0;
    struct Item {
        uint32_t task;
        int32_t node;
    };
    std::vector<Item> stack{{tasks[0].child0 + 1, 0}, {tasks[0].child0, 0}};
    medians += tasks[0].kind == lvl::KIND_MEDIAN;
    size_t visited = 1;
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        const lvl::Task& t = tasks[it.task];
        if (++visited > nt || t.slot > 1) return false; // (a cycle would visit more tasks than there are)
        const lvl::Box3 box = lvl::box_of_keys(t.box);
        if (t.kind == lvl::KIND_LEAF) {
            if (t.end < t.begin || t.end > leaf_shapes.size() || t.end - t.begin > kMaxLeafPrims) return false;
            const uint32_t first = (uint32_t)out.prim_order.size();
            out.prim_order.insert(out.prim_order.end(), leaf_shapes.begin() + t.begin, leaf_shapes.begin() + t.end);
            std::sort(out.prim_order.begin() + first, out.prim_order.end());
            set_child64(out.nodes[it.node], (int)t.slot, encode_leaf(first, t.end - t.begin), box, pad);
            out.num_leaves++;
            out.max_depth = std::max(out.max_depth, t.depth);
        } else if (t.kind == lvl::KIND_SPLIT || t.kind == lvl::KIND_MEDIAN) {
            if ((size_t)t.child0 + 1 >= nt || t.child0 <= it.task) return false;
            medians += t.kind == lvl::KIND_MEDIAN;
            const int32_t id = (int32_t)out.nodes.size();
            out.nodes.push_back(empty_node64());
            set_child64(out.nodes[it.node], (int)t.slot, id, box, pad);
            stack.push_back(Item{t.child0 + 1, id});
            stack.push_back(Item{t.child0, id});
        } else {
            return false;
        }
    }
    if (out.prim_order.size() != leaf_shapes.size()) return false;
    if (stats) stats->median_splits = medians;
    return true;
}

BuiltBvh build_bvh_levelwise(const std::vector<PrimBounds>& prims, bool leaves_tested_in_pairs, uint32_t depth_bound, LevelBuildStats* stats) {
    const uint32_t n = (uint32_t)prims.size();
    if (stats) *stats = LevelBuildStats{};
    if (n <= kMaxLeafPrims) return single_leaf_bvh(prims);
    const bool in_pairs = PYR_SAH_PAIRS && leaves_tested_in_pairs;
    std::vector<PrimBounds> cur = prims, next(n);
    std::vector<uint32_t> leaf_shapes(n, 0);
    std::vector<lvl::Task> tasks(1);
    std::memset(&tasks[0], 0, sizeof(lvl::Task));
    tasks[0].end = n, tasks[0].parent = -1;
    lvl::empty_keys(tasks[0].box), lvl::empty_keys(tasks[0].cbox);
    for (const PrimBounds& r : cur) grow_keys(tasks[0].box, tasks[0].cbox, r);

    std::vector<uint32_t> level{0}, following;
    uint32_t levels = 0;
    LevelBuildStats paths; // which paths of the device builder this input takes; nothing below reads them
    {
        const lvl::Box3 root = lvl::box_of_keys(tasks[0].cbox);
        for (int a = 0; a < 3; ++a) paths.root_centroid_extent[a] = root.hi[a] - root.lo[a];
    }
    while (!level.empty()) {
        ++levels;
        following.clear();
        uint32_t large_nodes = 0;
        for (const uint32_t ti : level) {
            lvl::Task t = tasks[ti];
            const uint32_t count = t.end - t.begin;
            if (count > kLevelSmallNode) {
                paths.most_large_nodes = std::max(paths.most_large_nodes, ++large_nodes);
                paths.most_chunks = std::max(paths.most_chunks, (count + kLevelChunk - 1) / kLevelChunk);
            }
            const lvl::Box3 box = lvl::box_of_keys(t.box), cbox = lvl::box_of_keys(t.cbox);
            // bin phase
            Bins bins;
            for (int a = 0; a < 3; ++a) {
                const float extent = cbox.hi[a] - cbox.lo[a];
                if (!(extent > 0.0f)) continue;
                const float scale = lvl::bin_scale(extent);
                for (uint32_t i = t.begin; i < t.end; ++i) bins.add(a, lvl::bin_index(lvl::centroid(cur[i].lo[a], cur[i].hi[a]), cbox.lo[a], scale), cur[i].lo, cur[i].hi);
            }
            // choose phase
            const lvl::Decision d = lvl::choose_split(count, t.depth, box, cbox, bins, in_pairs, depth_bound);
            t.kind = d.kind, t.axis = d.axis, t.bin = d.bin, t.lo = d.lo, t.scale = d.scale;
            if (d.kind == lvl::KIND_LEAF) {
                for (uint32_t i = t.begin; i < t.end; ++i) leaf_shapes[i] = cur[i].shape;
                tasks[ti] = t;
                continue;
            }
            if (d.kind == lvl::KIND_MEDIAN) {
                const float extent = cbox.hi[d.axis] - cbox.lo[d.axis];
                paths.largest_median = std::max(paths.largest_median, count);
                if (extent > 0.0f) {
                    (count > kLevelSmallNode ? paths.medians_positive_large : paths.medians_positive_small)++;
                    if (lvl::bin_scale(extent) == lvl::pos_inf()) paths.medians_infinite_scale++;
                }
                if (lvl::force_median(count, t.depth, depth_bound)) paths.largest_forced_median = std::max(paths.largest_forced_median, count);
            } else if (count > kLevelSmallNode) {
                int degenerate = 0;
                for (int a = 0; a < 3; ++a) degenerate += !(cbox.hi[a] - cbox.lo[a] > 0.0f);
                paths.degenerate_axis_splits += degenerate > 0;
            }
            // partition phase
            t.child0 = (uint32_t)tasks.size();
            tasks[ti] = t;
            lvl::Task kids[2];
            for (uint32_t s = 0; s < 2; ++s) {
                std::memset(&kids[s], 0, sizeof(lvl::Task));
                kids[s].begin = s == 0 ? t.begin : t.begin + d.left_count;
                kids[s].end = s == 0 ? t.begin + d.left_count : t.end;
                kids[s].parent = (int32_t)ti, kids[s].slot = s, kids[s].depth = t.depth + 1;
                lvl::empty_keys(kids[s].box), lvl::empty_keys(kids[s].cbox);
            }
            uint32_t cursor[2] = {kids[0].begin, kids[1].begin};
            for (uint32_t i = t.begin; i < t.end; ++i) {
                const PrimBounds& r = cur[i];
                const float c = lvl::centroid(r.lo[d.axis], r.hi[d.axis]);
                uint32_t side;
                if (d.kind == lvl::KIND_SPLIT) {
                    side = lvl::bin_index(c, d.lo, d.scale) <= d.bin ? 0u : 1u;
                } else {
                    uint32_t rank = 0;
                    for (uint32_t j = t.begin; j < t.end; ++j)
                        rank += lvl::median_before(lvl::centroid(cur[j].lo[d.axis], cur[j].hi[d.axis]), cur[j].shape, c, r.shape) ? 1u : 0u;
                    side = rank < d.left_count ? 0u : 1u;
                }
                next[cursor[side]++] = r;
                grow_keys(kids[side].box, kids[side].cbox, r);
            }
            tasks.push_back(kids[0]);
            tasks.push_back(kids[1]);
            following.push_back(t.child0), following.push_back(t.child0 + 1);
        }
        cur.swap(next);
        level.swap(following);
    }
    BuiltBvh out;
    LevelBuildStats st = paths;
    if (!finish_levelwise(tasks, leaf_shapes, bvh_padding(prims), out, &st)) return BuiltBvh{};
    st.levels = levels;
    if (stats) *stats = st;
    return out;
}

// ---------------------------------------------------------------------------------------------------------------- refit
namespace {

// the primitives' bounds by leaf-order position, as lvl::refit_leaf_box reads them
struct OrderedBounds {
    const std::vector<PrimBounds>& prims;
    const std::vector<uint32_t>& order;
    size_t first_of_kind[4] = {0, 0, 0, 0}; // where a kind's index 0 sits in `prims` (pack order: each kind by index)
    OrderedBounds(const std::vector<PrimBounds>& p, const std::vector<uint32_t>& o) : prims(p), order(o) {
        bool seen[4] = {false, false, false, false};
        for (size_t i = 0; i < p.size(); ++i) {
            const uint32_t kind = p[i].shape >> 30;
            if (!seen[kind]) seen[kind] = true, first_of_kind[kind] = i - (p[i].shape & 0x3FFFFFFFu);
        }
    }
    const PrimBounds& at(uint32_t i) const { return prims[first_of_kind[order[i] >> 30] + (order[i] & 0x3FFFFFFFu)]; }
    void get(uint32_t i, float* lo, float* hi) const {
        const PrimBounds& b = at(i);
        for (int a = 0; a < 3; ++a) lo[a] = b.lo[a], hi[a] = b.hi[a];
    }
};

template <class Node>
RefitSchedule schedule_of(const Node* nodes, size_t count, int slots) {
    RefitSchedule s;
    std::vector<uint32_t> height(count, 0);
    uint32_t top = 0;
    for (size_t n = count; n-- > 0;) { // a child's index is larger than its parent's in both trees
        height[n] = lvl::refit_height(nodes[n], slots, height.data());
        top = std::max(top, height[n]);
    }
    s.begin.assign(count ? top + 2 : 1, 0);
    for (size_t n = 0; n < count; ++n) s.begin[height[n] + 1]++;
    for (size_t h = 1; h < s.begin.size(); ++h) s.begin[h] += s.begin[h - 1];
    s.order.resize(count);
    std::vector<uint32_t> cursor(s.begin.begin(), s.begin.end());
    for (size_t n = 0; n < count; ++n) s.order[cursor[height[n]]++] = (uint32_t)n;
    return s;
}

template <class Node>
void refit_nodes(std::vector<Node>& nodes, int slots, const OrderedBounds& bounds, float pad) {
    const RefitSchedule s = schedule_of(nodes.data(), nodes.size(), slots);
    for (const uint32_t n : s.order) lvl::refit_node(nodes[n], slots, nodes.data(), bounds, pad);
}

} // namespace

RefitSchedule refit_schedule(const Node64* nodes, size_t count) { return schedule_of(nodes, count, 2); }
RefitSchedule refit_schedule(const Node128* nodes, size_t count) { return schedule_of(nodes, count, 4); }

void refit_bvh(BuiltBvh& bvh, const std::vector<PrimBounds>& prims) { refit_nodes(bvh.nodes, 2, OrderedBounds(prims, bvh.prim_order), bvh_padding(prims)); }

void refit_wide(WideBvh& wide, const BuiltBvh& bvh, const std::vector<PrimBounds>& prims) {
    refit_nodes(wide.nodes, 4, OrderedBounds(prims, bvh.prim_order), bvh_padding(prims));
}

double child_area_sum(const Node64* nodes, size_t count) {
    double sum = 0.0;
    for (size_t n = 0; n < count; ++n)
        for (int k = 0; k < 2; ++k) {
            lvl::Box3 b;
            b.lo[0] = nodes[n].lo_x[k], b.lo[1] = nodes[n].lo_y[k], b.lo[2] = nodes[n].lo_z[k];
            b.hi[0] = nodes[n].hi_x[k], b.hi[1] = nodes[n].hi_y[k], b.hi[2] = nodes[n].hi_z[k];
            sum += (double)lvl::half_area(b);
        }
    return sum;
}

uint64_t tree_digest(const BuiltBvh& bvh) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](const void* p, size_t bytes) { // FNV-1a over 32-bit words (every item hashed is a whole number of them)
        uint32_t w;
        for (size_t i = 0; i < bytes; i += 4) {
            std::memcpy(&w, (const unsigned char*)p + i, 4);
            h = (h ^ w) * 1099511628211ull;
        }
    };
    struct Item {
        int32_t node;
        uint32_t slot, depth;
    };
    if (bvh.nodes.empty()) return h;
    std::vector<Item> stack{{0, 1, 1}, {0, 0, 1}};
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        const Node64& n = bvh.nodes[it.node];
        const uint32_t k = it.slot;
        float box[6] = {n.lo_x[k], n.lo_y[k], n.lo_z[k], n.hi_x[k], n.hi_y[k], n.hi_z[k]};
        for (float& f : box)
            if (f == 0.0f) f = 0.0f; // -0.0f reads as +0.0f
        mix(box, sizeof(box));
        mix(&it.depth, 4), mix(&it.slot, 4);
        const int32_t code = n.child[k];
        if (code >= 0) {
            const uint32_t inner = 0xFFFFFFFFu;
            mix(&inner, 4);
            stack.push_back(Item{code, 1, it.depth + 1});
            stack.push_back(Item{code, 0, it.depth + 1});
        } else {
            const uint32_t first = (uint32_t)(-1 - code) >> 3, count = (uint32_t)(-1 - code) & 7u;
            uint32_t shapes[8] = {0};
            for (uint32_t j = 0; j < count; ++j) shapes[j] = bvh.prim_order[first + j];
            std::sort(shapes, shapes + count);
            mix(&count, 4);
            mix(shapes, 4 * count);
        }
    }
    return h;
}

} // namespace pyr
