// refit_check.cpp -- the host rehearsal of the refit (bvh.cpp refit_bvh / refit_wide, on bvh_level.h's rules), a program of its
// own for tests/test_scene_update_cpu.py, which builds it with -fsanitize=address,undefined and runs it as a child process.
//
//   refit_check FILE...      FILE: u32 num_spheres, u32 num_triangles, spheres [n][4], triangles [m][9], float32
//
// Per input and for both collapses of its binary tree: (a) a refit with unchanged bounds leaves the Node64 and Node128 arrays byte
// for byte; (b) after a rigid move and after a random displacement of every vertex by up to a tenth of the extent, the topology
// is the same, every stored box contains the boxes stored beneath it and every leaf's box contains its primitives' bounds moved
// outward by the padding -- checked here with comparisons of this file's own, not with the rules under test; (c) the area ratio
// is 1 for (a) and finite and positive for (b); the values are printed. Exit status 0 when everything holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pyrite_amd/csrc/bvh.h"

using namespace pyr;

namespace {

int failures = 0;
void expect(bool ok, const char* input, const char* what) {
    if (ok) return;
    ++failures;
    std::printf("FAIL %s: %s\n", input, what);
}

struct Input {
    std::vector<float> spheres, tris;
};

bool load(const char* path, Input& in) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint32_t n[2] = {0, 0};
    bool ok = std::fread(n, 4, 2, f) == 2;
    in.spheres.resize(4 * (size_t)n[0]);
    in.tris.resize(9 * (size_t)n[1]);
    ok = ok && std::fread(in.spheres.data(), 4, in.spheres.size(), f) == in.spheres.size();
    ok = ok && std::fread(in.tris.data(), 4, in.tris.size(), f) == in.tris.size();
    std::fclose(f);
    return ok;
}

// the scene's primitives in pack order: spheres, then triangles
std::vector<PrimBounds> bounds_of(const Input& in) {
    std::vector<PrimBounds> out;
    for (size_t i = 0; i < in.spheres.size() / 4; ++i) {
        PrimBounds b;
        const float* s = &in.spheres[4 * i];
        for (int a = 0; a < 3; ++a) b.lo[a] = s[a] - s[3], b.hi[a] = s[a] + s[3];
        b.shape = (0u << 30) | (uint32_t)i;
        out.push_back(b);
    }
    for (size_t i = 0; i < in.tris.size() / 9; ++i) {
        PrimBounds b;
        const float* p = &in.tris[9 * i];
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = std::fmin(p[a], std::fmin(p[3 + a], p[6 + a]));
            b.hi[a] = std::fmax(p[a], std::fmax(p[3 + a], p[6 + a]));
        }
        b.shape = (1u << 30) | (uint32_t)i;
        out.push_back(b);
    }
    return out;
}

const PrimBounds& bounds_at(const std::vector<PrimBounds>& prims, size_t num_spheres, uint32_t shape) {
    return prims[((shape >> 30) == 1u ? num_spheres : 0) + (shape & 0x3FFFFFFFu)];
}

struct Rng {
    uint64_t s;
    float unit() { // [0, 1)
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (float)((s >> 40) & 0xFFFFFF) / 16777216.0f;
    }
};

float extent_of(const std::vector<PrimBounds>& prims) {
    float lo = INFINITY, hi = -INFINITY;
    for (const PrimBounds& b : prims)
        for (int a = 0; a < 3; ++a) lo = std::fmin(lo, b.lo[a]), hi = std::fmax(hi, b.hi[a]);
    return prims.empty() ? 1.0f : hi - lo;
}

Input rigid_move(const Input& in) { // a rotation about (1, 2, 3) / sqrt(14) by 0.7 rad, then a translation
    const float ax[3] = {1.0f / std::sqrt(14.0f), 2.0f / std::sqrt(14.0f), 3.0f / std::sqrt(14.0f)}, c = std::cos(0.7f), s = std::sin(0.7f);
    auto move = [&](float* p) {
        const float d = ax[0] * p[0] + ax[1] * p[1] + ax[2] * p[2];
        const float cr[3] = {ax[1] * p[2] - ax[2] * p[1], ax[2] * p[0] - ax[0] * p[2], ax[0] * p[1] - ax[1] * p[0]};
        const float t[3] = {1.5f, -0.75f, 2.25f};
        for (int a = 0; a < 3; ++a) p[a] = p[a] * c + cr[a] * s + ax[a] * d * (1.0f - c) + t[a];
    };
    Input out = in;
    for (size_t i = 0; i < out.spheres.size() / 4; ++i) move(&out.spheres[4 * i]);
    for (size_t i = 0; i < out.tris.size() / 3; ++i) move(&out.tris[3 * i]);
    return out;
}

Input shaken(const Input& in, float amplitude, uint64_t seed) {
    Rng rng{seed};
    Input out = in;
    for (size_t i = 0; i < out.spheres.size() / 4; ++i)
        for (int a = 0; a < 3; ++a) out.spheres[4 * i + a] += amplitude * (2.0f * rng.unit() - 1.0f);
    for (float& x : out.tris) x += amplitude * (2.0f * rng.unit() - 1.0f);
    return out;
}

struct StoredBox {
    float lo[3], hi[3];
};
template <class Node>
StoredBox stored(const Node& n, int k) {
    return StoredBox{{n.lo_x[k], n.lo_y[k], n.lo_z[k]}, {n.hi_x[k], n.hi_y[k], n.hi_z[k]}};
}
bool holds(const StoredBox& outer, const float* lo, const float* hi) {
    for (int a = 0; a < 3; ++a)
        if (!(outer.lo[a] <= lo[a] && outer.hi[a] >= hi[a])) return false;
    return true;
}

// every stored box contains what lies beneath it
template <class Node>
bool contained(const std::vector<Node>& nodes, int slots, const std::vector<uint32_t>& prim_order, const std::vector<PrimBounds>& prims, size_t num_spheres, float pad) {
    for (const Node& n : nodes)
        for (int k = 0; k < slots; ++k) {
            const int32_t code = n.child[k];
            if (code == kEmptyChild) continue;
            const StoredBox box = stored(n, k);
            if (code >= 0) {
                for (int j = 0; j < slots; ++j) {
                    const Node& child = nodes[(size_t)code];
                    if (child.child[j] == kEmptyChild || (child.child[j] < 0 && ((uint32_t)(-1 - child.child[j]) & 7u) == 0)) continue;
                    const StoredBox inner = stored(child, j);
                    if (!holds(box, inner.lo, inner.hi)) return false;
                }
            } else {
                const uint32_t first = (uint32_t)(-1 - code) >> 3, count = (uint32_t)(-1 - code) & 7u;
                for (uint32_t i = 0; i < count; ++i) {
                    const PrimBounds& b = bounds_at(prims, num_spheres, prim_order[first + i]);
                    const float lo[3] = {b.lo[0] - pad, b.lo[1] - pad, b.lo[2] - pad}, hi[3] = {b.hi[0] + pad, b.hi[1] + pad, b.hi[2] + pad};
                    if (!holds(box, lo, hi)) return false;
                }
            }
        }
    return true;
}

template <class Node>
bool same_topology(const std::vector<Node>& a, const std::vector<Node>& b, int slots) {
    if (a.size() != b.size()) return false;
    for (size_t n = 0; n < a.size(); ++n)
        for (int k = 0; k < slots; ++k)
            if (a[n].child[k] != b[n].child[k]) return false;
    return true;
}

template <class Node>
bool same_bytes(const std::vector<Node>& a, const std::vector<Node>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(Node)) == 0);
}

// PyrUpdateInfo::area_ratio as pyr_scene_update_info states it: a tree whose boxes had no area at its build (subnormal extents) reports 1
double area_ratio(double now, double built_area) { return built_area > 0.0 ? now / built_area : 1.0; }

void check(const char* name, const Input& in) {
    const size_t num_spheres = in.spheres.size() / 4;
    const std::vector<PrimBounds> prims = bounds_of(in);
    const bool in_pairs = num_spheres == 0 && prims.size() * 48 > 8 * 1024; // as scene creation decides
    const BuiltBvh built = build_bvh(prims, in_pairs);
    const WideBvh wides[2] = {collapse_to_wide(built), collapse_to_wide_sah(built)};
    const double built_area = child_area_sum(built.nodes.data(), built.nodes.size());

    // (a) unchanged bounds: the same bytes
    {
        BuiltBvh again = built;
        refit_bvh(again, prims);
        expect(same_bytes(again.nodes, built.nodes), name, "identity refit changed the Node64 array");
        const double ratio = area_ratio(child_area_sum(again.nodes.data(), again.nodes.size()), built_area);
        std::printf("%s identity area_ratio %.17g\n", name, ratio);
        expect(built_area > 0.0 ? ratio == 1.0 : true, name, "identity area_ratio is not 1");
        for (int w = 0; w < 2; ++w) {
            WideBvh wide = wides[w];
            refit_wide(wide, built, prims);
            expect(same_bytes(wide.nodes, wides[w].nodes), name, w == 0 ? "identity refit changed the greedy Node128 array" : "identity refit changed the cost-driven Node128 array");
        }
    }
    // (b), (c) moved: containment, the topology, a finite positive area ratio
    const float extent = extent_of(prims);
    const Input moves[2] = {rigid_move(in), shaken(in, 0.1f * extent, 77)};
    const char* move_names[2] = {"rigid", "shaken"};
    for (int m = 0; m < 2; ++m) {
        const std::vector<PrimBounds> moved = bounds_of(moves[m]);
        const float pad = bvh_padding(moved);
        BuiltBvh tree = built;
        refit_bvh(tree, moved);
        expect(same_topology(tree.nodes, built.nodes, 2), name, "a refit changed the binary tree's topology");
        expect(contained(tree.nodes, 2, tree.prim_order, moved, num_spheres, pad), name, "a Node64 box does not contain what lies beneath it");
        const double ratio = area_ratio(child_area_sum(tree.nodes.data(), tree.nodes.size()), built_area);
        std::printf("%s %s area_ratio %.6g\n", name, move_names[m], ratio);
        expect(built_area > 0.0 ? (std::isfinite(ratio) && ratio > 0.0) : true, name, "area_ratio of a moved tree is not finite and positive");
        for (int w = 0; w < 2; ++w) {
            WideBvh wide = wides[w];
            refit_wide(wide, built, moved);
            expect(same_topology(wide.nodes, wides[w].nodes, 4), name, "a refit changed the four-child tree's topology");
            expect(contained(wide.nodes, 4, built.prim_order, moved, num_spheres, pad), name, "a Node128 box does not contain what lies beneath it");
        }
        // twice the same arrays: the same bytes
        BuiltBvh twice = tree;
        refit_bvh(twice, moved);
        expect(same_bytes(twice.nodes, tree.nodes), name, "a second refit with the same arrays wrote other bytes");
    }
}

} // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: refit_check FILE...\n");
        return 2;
    }
    for (int i = 1; i < argc; ++i) {
        Input in;
        if (!load(argv[i], in)) {
            std::fprintf(stderr, "cannot read %s\n", argv[i]);
            return 2;
        }
        const char* slash = std::strrchr(argv[i], '/');
        check(slash ? slash + 1 : argv[i], in);
    }
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
