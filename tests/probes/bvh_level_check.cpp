// Stand-alone host program (no GPU): runs every BVH builder of pyrite_amd/csrc/bvh.cpp -- all of them decide by the functions of
// bvh_level.h, which the device builder's kernels compile too -- on the primitive files given on the command line
// (tools/bvh_quality.py write_prims): the recursive builder; the level-wise one with the depth bound of the scene builder and lowered
// to 8, twice each; on inputs without spheres the spatial-split builder, twice; and collapses every tree both ways. Built with
// -fsanitize=address,undefined together with bvh.cpp, an index out of range or an undefined conversion in any of them stops the
// program where it happens.
// Exit status 0: every build gave a tree over all its primitives, twice the same digest.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pyrite_amd/csrc/bvh.h"

using namespace pyr;

namespace {

struct Prim {
    float kind, v[9];
};

// `tri_positions`: nine floats per triangle, in the order of the triangles' shape codes
bool read_prims(const char* path, std::vector<PrimBounds>& bounds, std::vector<float>& tri_positions) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint32_t n = 0;
    if (std::fread(&n, 4, 1, f) != 1) return std::fclose(f), false;
    std::vector<Prim> prims(n);
    if (n && std::fread(prims.data(), sizeof(Prim), n, f) != n) return std::fclose(f), false;
    std::fclose(f);
    uint32_t spheres = 0, triangles = 0;
    for (const Prim& p : prims) {
        PrimBounds b;
        if (p.kind == 1.0f) {
            for (int a = 0; a < 3; ++a) {
                b.lo[a] = std::min(p.v[a], std::min(p.v[3 + a], p.v[6 + a]));
                b.hi[a] = std::max(p.v[a], std::max(p.v[3 + a], p.v[6 + a]));
            }
            b.shape = (1u << 30) | triangles++;
            tri_positions.insert(tri_positions.end(), p.v, p.v + 9);
        } else {
            for (int a = 0; a < 3; ++a) b.lo[a] = p.v[a] - p.v[3], b.hi[a] = p.v[a] + p.v[3];
            b.shape = spheres++;
        }
        bounds.push_back(b);
    }
    return true;
}

bool collapses(const BuiltBvh& tree) {
    const WideBvh greedy = collapse_to_wide(tree), by_cost = collapse_to_wide_sah(tree);
    return !greedy.nodes.empty() && !by_cost.nodes.empty();
}

} // namespace

int main(int argc, char** argv) {
    size_t builds = 0;
    for (int i = 1; i < argc; ++i) {
        std::vector<PrimBounds> bounds;
        std::vector<float> tri_positions;
        if (!read_prims(argv[i], bounds, tri_positions)) {
            std::fprintf(stderr, "cannot read %s\n", argv[i]);
            return 2;
        }
        for (const bool in_pairs : {false, true}) {
            uint32_t medians = 0;
            const BuiltBvh recursive = build_bvh(bounds, in_pairs, &medians);
            if (recursive.nodes.empty() || recursive.prim_order.size() != bounds.size() || recursive.max_depth > kMaxBvhDepth || !collapses(recursive)) {
                std::fprintf(stderr, "%s: pairs %d: the recursive builder gave no tree over every primitive\n", argv[i], (int)in_pairs);
                return 1;
            }
            builds += 1;
            for (const uint32_t depth_bound : {kMaxBvhDepth, 8u}) {
                LevelBuildStats stats, again_stats;
                const BuiltBvh tree = build_bvh_levelwise(bounds, in_pairs, depth_bound, &stats);
                const BuiltBvh again = build_bvh_levelwise(bounds, in_pairs, depth_bound, &again_stats);
                if (tree.nodes.empty() || tree.prim_order.size() != bounds.size() || tree_digest(tree) != tree_digest(again) || tree.max_depth > kMaxBvhDepth) {
                    std::fprintf(stderr, "%s: pairs %d, depth bound %u: no tree over every primitive, or two builds differ\n", argv[i], (int)in_pairs, depth_bound);
                    return 1;
                }
                if (medians == 0 && depth_bound == kMaxBvhDepth && tree_digest(tree) != tree_digest(recursive)) {
                    std::fprintf(stderr, "%s: pairs %d: the level-wise tree is not the recursive builder's\n", argv[i], (int)in_pairs);
                    return 1;
                }
                if (!collapses(tree)) return 1;
                builds += 2;
            }
        }
        if (!bounds.empty() && tri_positions.size() == 9 * bounds.size()) { // triangles only: what spatial splits are for
            SpatialSplits sp;
            sp.tri_positions = tri_positions.data();
            const BuiltBvh tree = build_bvh_spatial(bounds, sp), again = build_bvh_spatial(bounds, sp);
            if (tree.nodes.empty() || tree.prim_order.size() < bounds.size() || tree.prim_order.size() > (size_t)(1.4 * bounds.size()) + 1 ||
                tree.max_depth > kMaxBvhDepth || tree_digest(tree) != tree_digest(again) || !collapses(tree)) {
                std::fprintf(stderr, "%s: spatial splits: no tree within the duplication budget, or two builds differ\n", argv[i]);
                return 1;
            }
            builds += 2;
        }
    }
    std::printf("ok: %zu builds of %d inputs\n", builds, argc - 1);
    return 0;
}
