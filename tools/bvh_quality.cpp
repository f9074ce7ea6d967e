// bvh_quality.cpp -- the mesh BVH's quality on the CPU: builds the four-child pair tree the ways pyr_scene_create can -- old
// (object splits + greedy collapse), cost-driven collapse, spatial splits -- and walks it with the render kernels'
// semantics -- ordered four-child visits (children sorted by entry distance, pruned by the closest hit so far), leaves tested
// two triangles per step, any-hit for shadow rays -- counting what the kernels' PYR_FLAG_COUNTERS count.
//
//   bvh_quality report TRIS NAME:RAYS...   the table: per tree, its size and build time, per ray set the walk's counts
//   bvh_quality check TRIS RAYS object|spatial
//                                          invariants of the cost-collapsed tree over object (or spatial) splits and its walk
//                                          against brute force (tests/test_bvh_build.py)
//   bvh_quality hash TRIS                  hashes of the tree PYRITE_SPATIAL_SPLITS / PYRITE_WIDE_COLLAPSE select and of the
//                                          old, the cost-collapsed and the spatial-split trees
//   bvh_quality level PRIMS RAYS|- [DEPTH_BOUND|- [deep]]
//                                          the level-wise builder (build_bvh_levelwise, the device builder's rehearsal) next to
//                                          the recursive one: both trees' digests and median splits, then the invariants of the
//                                          level-wise tree and its walk against brute force (tests/test_bvh_device_cpu.py), and in
//                                          a last line which paths of the device builder the input takes (LevelBuildStats). `deep`:
//                                          a wide tree that needs a deeper stack than the kernels have is reported, not refused
//
// PRIMS: uint32 count, then count x 10 float32: kind (0 sphere: centre, radius; 1 triangle: three vertices), nine values.
// TRIS: uint32 count, then count x 9 float32 (three vertices). RAYS: uint32 count, then count x 8 float32: origin, direction,
// limit (the shadow ray's squared blocking distance, or -1 for a closest-hit ray), unused. tools/bvh_quality.py writes both.
#include "../pyrite_amd/csrc/bvh.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace pyr;

namespace {

struct Ray {
    float o[3], d[3], limit, unused;
};

template <class T>
std::vector<T> read_file(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    uint32_t n = 0;
    if (std::fread(&n, 4, 1, f) != 1) std::exit(2);
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) std::exit(2);
    std::fclose(f);
    return v;
}

struct Tri {
    float v[9];
};

std::vector<PrimBounds> bounds_of(const std::vector<Tri>& tris) {
    std::vector<PrimBounds> b(tris.size());
    for (size_t i = 0; i < tris.size(); ++i) {
        const float* p = tris[i].v;
        for (int a = 0; a < 3; ++a) {
            b[i].lo[a] = std::min(p[a], std::min(p[3 + a], p[6 + a]));
            b[i].hi[a] = std::max(p[a], std::max(p[3 + a], p[6 + a]));
        }
        b[i].shape = (1u << 30) | (uint32_t)i; // PYR_SHAPE_TRIANGLE
    }
    return b;
}

struct Trees {
    BuiltBvh bvh;
    WideBvh wide;
    double build_ms = 0, collapse_ms = 0;
};

Trees build(const std::vector<Tri>& tris, bool spatial_splits, bool cost_driven) {
    const std::vector<PrimBounds> b = bounds_of(tris);
    Trees t;
    auto t0 = std::chrono::steady_clock::now();
    if (spatial_splits) {
        SpatialSplits sp;
        sp.tri_positions = tris.empty() ? nullptr : tris[0].v;
        if (const char* e = std::getenv("BVH_QUALITY_ALPHA")) sp.alpha = (float)std::atof(e); // parameter sweeps
        if (const char* e = std::getenv("BVH_QUALITY_DUPLICATION")) sp.max_duplication = (float)std::atof(e);
        t.bvh = build_bvh_spatial(b, sp);
    } else {
        t.bvh = build_bvh(b, true);
    }
    auto t1 = std::chrono::steady_clock::now();
    t.wide = cost_driven ? collapse_to_wide_sah(t.bvh) : collapse_to_wide(t.bvh);
    auto t2 = std::chrono::steady_clock::now();
    t.build_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t.collapse_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    return t;
}

uint64_t fnv(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* c = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
    return h;
}
uint64_t hash_of(const Trees& t) {
    uint64_t h = fnv(t.bvh.nodes.data(), t.bvh.nodes.size() * sizeof(Node64));
    h = fnv(t.bvh.prim_order.data(), t.bvh.prim_order.size() * 4, h);
    return fnv(t.wide.nodes.data(), t.wide.nodes.size() * sizeof(Node128), h);
}

// Moller-Trumbore in double: the same function for the walk and for brute force, so their distances compare exactly
bool hit_triangle(const float* v, const Ray& r, double& dist) {
    const double e1[3] = {(double)v[3] - v[0], (double)v[4] - v[1], (double)v[5] - v[2]};
    const double e2[3] = {(double)v[6] - v[0], (double)v[7] - v[1], (double)v[8] - v[2]};
    const double d[3] = {r.d[0], r.d[1], r.d[2]};
    const double p[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
    const double det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
    if (det == 0.0) return false;
    const double inv = 1.0 / det;
    const double s[3] = {(double)r.o[0] - v[0], (double)r.o[1] - v[1], (double)r.o[2] - v[2]};
    const double u = (s[0] * p[0] + s[1] * p[1] + s[2] * p[2]) * inv;
    if (u < 0.0 || u > 1.0) return false;
    const double q[3] = {s[1] * e1[2] - s[2] * e1[1], s[2] * e1[0] - s[0] * e1[2], s[0] * e1[1] - s[1] * e1[0]};
    const double w = (d[0] * q[0] + d[1] * q[1] + d[2] * q[2]) * inv;
    if (w < 0.0 || u + w > 1.0) return false;
    dist = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) * inv;
    return dist > 1.0e-4; // DIST_EPSILON
}

struct Counts {
    uint64_t visits = 0, box_tests = 0, pair_steps = 0, tri_tests = 0;
};
struct Hit {
    double dist = INFINITY;
    int64_t tri = -1;
    bool blocked = false;
};

// One ray through the wide tree, as the kernels walk it (trav_step_wide, the pair steps of trav_step_lean).
template <class HitShape> // hit(shape code, ray, distance)
Hit walk(const Trees& t, const HitShape& hit_shape, const Ray& r, Counts& cnt) {
    const bool shadow = r.limit >= 0.0f;
    Hit h;
    double closest = shadow ? std::sqrt((double)r.limit) * 1.001 + 1.0e-3 : INFINITY; // shadow_cutoff
    double inv[3];
    for (int a = 0; a < 3; ++a) inv[a] = 1.0 / (double)r.d[a];
    std::vector<int32_t> stack;
    int32_t node = 0;
    for (;;) {
        if (node >= 0) {
            const Node128& n = t.wide.nodes[node];
            cnt.visits++;
            double e[4];
            int32_t c[4];
            int hits = 0;
            for (int k = 0; k < 4; ++k) {
                if (n.child[k] == kEmptyChild) continue;
                cnt.box_tests++;
                const float lo[3] = {n.lo_x[k], n.lo_y[k], n.lo_z[k]}, hi[3] = {n.hi_x[k], n.hi_y[k], n.hi_z[k]};
                double tmin = 0.0, tmax = INFINITY;
                for (int a = 0; a < 3; ++a) {
                    double t0 = ((double)lo[a] - r.o[a]) * inv[a], t1 = ((double)hi[a] - r.o[a]) * inv[a];
                    if (std::isnan(t0) || std::isnan(t1)) continue; // d = 0 on a plane of the box: the axis does not constrain
                    if (t0 > t1) std::swap(t0, t1);
                    tmin = std::max(tmin, t0), tmax = std::min(tmax, t1);
                }
                if (tmax >= tmin && tmin < closest) e[hits] = tmin, c[hits] = n.child[k], hits++;
            }
            for (int i = 1; i < hits; ++i) // ascending entry, stable
                for (int j = i; j > 0 && e[j] < e[j - 1]; --j) std::swap(e[j], e[j - 1]), std::swap(c[j], c[j - 1]);
            if (hits == 0) {
                if (stack.empty()) break;
                node = stack.back();
                stack.pop_back();
                continue;
            }
            for (int i = hits - 1; i > 0; --i) stack.push_back(c[i]);
            node = c[0];
            continue;
        }
        const uint32_t first = (uint32_t)(-1 - node) >> 3, count = (uint32_t)(-1 - node) & 7u;
        bool done = false;
        for (uint32_t j = 0; j < count && !done; j += 2) {
            cnt.pair_steps++;
            for (uint32_t k = j; k < std::min(count, j + 2); ++k) {
                cnt.tri_tests++;
                const uint32_t shape = t.bvh.prim_order[first + k], tri = shape & 0x3FFFFFFFu;
                double dist;
                if (!hit_shape(shape, r, dist)) continue;
                if (shadow && dist * dist < r.limit) h.blocked = done = true;
                if (!shadow && dist < closest) closest = h.dist = dist, h.tri = tri;
            }
        }
        if (done || stack.empty()) break;
        node = stack.back();
        stack.pop_back();
    }
    return h;
}

Hit walk(const Trees& t, const std::vector<Tri>& tris, const Ray& r, Counts& cnt) {
    return walk(t, [&tris](uint32_t shape, const Ray& ray, double& dist) { return hit_triangle(tris[shape & 0x3FFFFFFFu].v, ray, dist); }, r, cnt);
}

Hit brute(const std::vector<Tri>& tris, const Ray& r) {
    Hit h;
    for (size_t i = 0; i < tris.size(); ++i) {
        double dist;
        if (!hit_triangle(tris[i].v, r, dist)) continue;
        if (r.limit >= 0.0f && dist * dist < r.limit) h.blocked = true;
        if (dist < h.dist) h.dist = dist, h.tri = (int64_t)i;
    }
    return h;
}

// SAH cost of the wide tree in steps per ray that enters the root: node visits + pair steps, weighted by surface area
double sah_cost(const Trees& t) {
    auto area = [](float dx, float dy, float dz) { return (double)dx * dy + (double)dy * dz + (double)dz * dx; };
    double root = 0;
    {
        const Node128& n = t.wide.nodes[0];
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = 0; k < 4; ++k)
            if (n.child[k] != kEmptyChild) {
                lo[0] = std::min(lo[0], n.lo_x[k]), lo[1] = std::min(lo[1], n.lo_y[k]), lo[2] = std::min(lo[2], n.lo_z[k]);
                hi[0] = std::max(hi[0], n.hi_x[k]), hi[1] = std::max(hi[1], n.hi_y[k]), hi[2] = std::max(hi[2], n.hi_z[k]);
            }
        root = area(hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]);
    }
    double cost = 1.0;
    for (const Node128& n : t.wide.nodes)
        for (int k = 0; k < 4; ++k) {
            if (n.child[k] == kEmptyChild) continue;
            const double a = area(n.hi_x[k] - n.lo_x[k], n.hi_y[k] - n.lo_y[k], n.hi_z[k] - n.lo_z[k]) / root;
            cost += n.child[k] >= 0 ? a : a * (double)((((uint32_t)(-1 - n.child[k]) & 7u) + 1u) / 2u);
        }
    return cost;
}

// the same for the binary tree: node visits + primitive tests in pairs
double binary_sah_cost(const Trees& t) {
    auto area = [](float dx, float dy, float dz) { return (double)dx * dy + (double)dy * dz + (double)dz * dx; };
    const Node64& r = t.bvh.nodes[0];
    const double root = area(std::max(r.hi_x[0], r.hi_x[1]) - std::min(r.lo_x[0], r.lo_x[1]), std::max(r.hi_y[0], r.hi_y[1]) - std::min(r.lo_y[0], r.lo_y[1]),
                             std::max(r.hi_z[0], r.hi_z[1]) - std::min(r.lo_z[0], r.lo_z[1]));
    double cost = 1.0;
    for (const Node64& n : t.bvh.nodes)
        for (int k = 0; k < 2; ++k) {
            const uint32_t cnt = n.child[k] >= 0 ? 0u : ((uint32_t)(-1 - n.child[k]) & 7u);
            if (n.child[k] < 0 && cnt == 0) continue;
            const double a = area(n.hi_x[k] - n.lo_x[k], n.hi_y[k] - n.lo_y[k], n.hi_z[k] - n.lo_z[k]) / root;
            cost += n.child[k] >= 0 ? a : a * (double)((cnt + 1u) & ~1u);
        }
    return cost;
}

uint64_t pair_records(const Trees& t) {
    uint64_t r = 0;
    for (const Node128& n : t.wide.nodes)
        for (int k = 0; k < 4; ++k)
            if (n.child[k] < 0 && n.child[k] != kEmptyChild) r += std::max(1u, ((((uint32_t)(-1 - n.child[k]) & 7u) + 1u) / 2u));
    return r;
}

int report(int argc, char** argv) {
    const std::vector<Tri> tris = read_file<Tri>(argv[2]);
    struct Set {
        std::string name;
        std::vector<Ray> rays;
    };
    std::vector<Set> sets;
    for (int i = 3; i < argc; ++i) {
        const char* colon = std::strchr(argv[i], ':');
        if (!colon) return 2;
        sets.push_back(Set{std::string(argv[i], (size_t)(colon - argv[i])), read_file<Ray>(colon + 1)});
    }
    std::printf("%zu triangles\n\n", tris.size());
    const struct {
        const char* name;
        bool spatial, cost_driven;
    } variants[] = {{"old: object splits, greedy collapse", false, false},
                    {"new: object splits, cost-driven collapse", false, true},
                    {"spatial splits, greedy collapse", true, false},
                    {"spatial splits, cost-driven collapse", true, true}};
    for (const auto& v : variants) {
        const Trees t = build(tris, v.spatial, v.cost_driven);
        std::printf("%s\n", v.name);
        std::printf("  references %zu (%.3fx)  binary nodes %zu  wide nodes %zu  pair records %llu  depth %u  stack %u\n", t.bvh.prim_order.size(),
                    (double)t.bvh.prim_order.size() / (double)tris.size(), t.bvh.nodes.size(), t.wide.nodes.size(), (unsigned long long)pair_records(t),
                    t.wide.max_depth, t.wide.stack_need);
        std::printf("  build %.0f ms + collapse %.0f ms   wide nodes %.1f MB + pair records %.1f MB   SAH %.2f steps (binary %.2f)\n", t.build_ms, t.collapse_ms,
                    t.wide.nodes.size() * 128.0 / 1e6, pair_records(t) * 80.0 / 1e6, sah_cost(t), binary_sah_cost(t));
        std::printf("  %-8s %10s %12s %10s %10s %10s %10s\n", "rays", "count", "node visits", "box tests", "pair steps", "tri tests", "steps");
        for (const Set& s : sets) {
            Counts c;
            for (const Ray& r : s.rays) walk(t, tris, r, c);
            const double n = (double)s.rays.size();
            std::printf("  %-8s %10zu %12.2f %10.2f %10.2f %10.2f %10.2f\n", s.name.c_str(), s.rays.size(), c.visits / n, c.box_tests / n, c.pair_steps / n,
                        c.tri_tests / n, (c.visits + c.pair_steps) / n);
        }
        std::printf("\n");
    }
    return 0;
}

int fail(const char* what) {
    std::printf("FAIL %s\n", what);
    return 1;
}

int check(int, char** argv) {
    const std::vector<Tri> tris = read_file<Tri>(argv[2]);
    const std::vector<Ray> rays = read_file<Ray>(argv[3]);
    const bool spatial = !std::strcmp(argv[4], "spatial");
    const Trees t = build(tris, spatial, true), again = build(tris, spatial, true);
    if (hash_of(t) != hash_of(again)) return fail("two builds differ");
    if (t.bvh.max_depth > kMaxBvhDepth) return fail("binary depth");
    if (t.wide.stack_need > 64) return fail("stack need"); // kMaxStackDepth (device_scene.h)
    if (t.bvh.prim_order.size() > (size_t)(1.4 * tris.size()) + 1) return fail("duplication budget");
    // every leaf reference is a triangle of the mesh, no leaf names one twice, and every triangle is covered: points spread over
    // it lie in the union of the (padded) boxes of the wide leaves that name it
    std::vector<std::vector<const float*>> boxes(tris.size()); // lo[3], hi[3] of every leaf slot per triangle
    std::vector<float> store;
    store.reserve(t.bvh.prim_order.size() * 6 + 6);
    for (const Node128& n : t.wide.nodes)
        for (int k = 0; k < 4; ++k) {
            const int32_t code = n.child[k];
            if (code >= 0 || code == kEmptyChild) continue;
            const uint32_t first = (uint32_t)(-1 - code) >> 3, count = (uint32_t)(-1 - code) & 7u;
            if (count > kMaxLeafPrims || first + count > t.bvh.prim_order.size()) return fail("leaf code out of range");
            const float* b = store.data() + store.size();
            const float box[6] = {n.lo_x[k], n.lo_y[k], n.lo_z[k], n.hi_x[k], n.hi_y[k], n.hi_z[k]};
            store.insert(store.end(), box, box + 6);
            for (uint32_t j = 0; j < count; ++j) {
                const uint32_t shape = t.bvh.prim_order[first + j];
                if ((shape >> 30) != 1 || (shape & 0x3FFFFFFFu) >= tris.size()) return fail("leaf reference is not a triangle of the mesh");
                for (uint32_t i = 0; i < j; ++i)
                    if (t.bvh.prim_order[first + i] == shape) return fail("a triangle twice in one leaf");
                boxes[shape & 0x3FFFFFFFu].push_back(b);
            }
        }
    for (size_t i = 0; i < tris.size(); ++i) {
        const float* v = tris[i].v;
        const int m = 12;
        for (int a = 0; a <= m; ++a)
            for (int b = 0; a + b <= m; ++b) {
                const double u = (double)a / m, w = (double)b / m;
                double p[3];
                for (int k = 0; k < 3; ++k) p[k] = v[k] + u * ((double)v[3 + k] - v[k]) + w * ((double)v[6 + k] - v[k]);
                bool in = false;
                for (const float* bx : boxes[i])
                    in = in || (p[0] >= bx[0] && p[1] >= bx[1] && p[2] >= bx[2] && p[0] <= bx[3] && p[1] <= bx[4] && p[2] <= bx[5]);
                if (!in) {
                    std::printf("triangle %zu point (%g %g %g) in none of its %zu leaf boxes\n", i, p[0], p[1], p[2], boxes[i].size());
                    return fail("coverage");
                }
            }
    }
    size_t hits = 0, blocked = 0;
    for (const Ray& r : rays) {
        Counts c;
        const Hit a = walk(t, tris, r, c), b = brute(tris, r);
        if (r.limit >= 0.0f) {
            if (a.blocked != b.blocked) return fail("any-hit differs from brute force");
            blocked += b.blocked;
        } else {
            if (a.dist != b.dist) return fail("closest hit differs from brute force");
            hits += b.tri >= 0;
        }
    }
    std::printf("OK %zu triangles, %zu references, depth %u, stack %u, %zu rays (%zu closest hits, %zu blocked)\n", tris.size(), t.bvh.prim_order.size(),
                t.bvh.max_depth, t.wide.stack_need, rays.size(), hits, blocked);
    return 0;
}

// ---- level-wise builder: spheres and triangles
struct Prim {
    float kind, v[9];
};

bool hit_sphere(const float* s, const Ray& r, double& dist) { // centre, radius; nearest root beyond DIST_EPSILON
    const double oc[3] = {(double)r.o[0] - s[0], (double)r.o[1] - s[1], (double)r.o[2] - s[2]};
    const double d[3] = {r.d[0], r.d[1], r.d[2]};
    const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], b = oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2];
    const double c = oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2] - (double)s[3] * s[3];
    const double disc = b * b - a * c;
    if (disc < 0.0 || a == 0.0) return false;
    const double q = std::sqrt(disc), t0 = (-b - q) / a, t1 = (-b + q) / a;
    dist = t0 > 1.0e-4 ? t0 : t1;
    return dist > 1.0e-4;
}

struct LevelScene {
    std::vector<Prim> prims;
    std::vector<PrimBounds> bounds;
    std::vector<uint32_t> prim_of_sphere, prim_of_triangle; // shape index -> record
    const Prim* find(uint32_t shape) const {
        const uint32_t index = shape & 0x3FFFFFFFu;
        const std::vector<uint32_t>& table = (shape >> 30) == 1 ? prim_of_triangle : prim_of_sphere;
        return (shape >> 30) <= 1 && index < table.size() ? &prims[table[index]] : nullptr;
    }
    bool hit(uint32_t shape, const Ray& r, double& dist) const {
        const Prim* p = find(shape);
        return (shape >> 30) == 1 ? hit_triangle(p->v, r, dist) : hit_sphere(p->v, r, dist);
    }
};

LevelScene read_prims(const char* path) {
    LevelScene sc;
    sc.prims = read_file<Prim>(path);
    for (size_t i = 0; i < sc.prims.size(); ++i) {
        const float* p = sc.prims[i].v;
        PrimBounds b;
        if (sc.prims[i].kind == 1.0f) {
            for (int a = 0; a < 3; ++a) {
                b.lo[a] = std::min(p[a], std::min(p[3 + a], p[6 + a]));
                b.hi[a] = std::max(p[a], std::max(p[3 + a], p[6 + a]));
            }
            b.shape = (1u << 30) | (uint32_t)sc.prim_of_triangle.size();
            sc.prim_of_triangle.push_back((uint32_t)i);
        } else {
            for (int a = 0; a < 3; ++a) b.lo[a] = p[a] - p[3], b.hi[a] = p[a] + p[3]; // pack_and_upload's sphere bounds
            b.shape = (uint32_t)sc.prim_of_sphere.size();
            sc.prim_of_sphere.push_back((uint32_t)i);
        }
        sc.bounds.push_back(b);
    }
    return sc;
}

int level(int argc, char** argv) {
    const LevelScene sc = read_prims(argv[2]);
    const std::vector<Ray> rays = std::strcmp(argv[3], "-") ? read_file<Ray>(argv[3]) : std::vector<Ray>();
    const uint32_t depth_bound = argc > 4 && std::strcmp(argv[4], "-") ? (uint32_t)std::atoi(argv[4]) : kMaxBvhDepth;
    const bool deep_allowed = argc > 5; // "deep": a wide tree whose stack need exceeds kMaxStackDepth is reported, not refused
    // as pack_and_upload decides it: leaves are tested in pairs in a triangle-only scene too big to live in LDS
    const bool in_pairs = sc.prim_of_sphere.empty() && sc.bounds.size() * 48 > 8 * 1024;
    uint32_t recursive_medians = 0;
    const BuiltBvh recursive = build_bvh(sc.bounds, in_pairs, &recursive_medians);
    LevelBuildStats stats, stats_again;
    Trees t, again;
    t.bvh = build_bvh_levelwise(sc.bounds, in_pairs, depth_bound, &stats);
    again.bvh = build_bvh_levelwise(sc.bounds, in_pairs, depth_bound, &stats_again);
    std::printf("recursive %016llx median_splits %u\n", (unsigned long long)tree_digest(recursive), recursive_medians);
    std::printf("levelwise %016llx median_splits %u levels %u nodes %zu leaves %u depth %u\n", (unsigned long long)tree_digest(t.bvh), stats.median_splits,
                stats.levels, t.bvh.nodes.size(), t.bvh.num_leaves, t.bvh.max_depth);
    if (recursive_medians == 0 && depth_bound == kMaxBvhDepth) { // the same tree in the same layout, up to the order inside a leaf
        if (recursive.nodes.size() != t.bvh.nodes.size() || recursive.num_leaves != t.bvh.num_leaves || recursive.max_depth != t.bvh.max_depth) return fail("layout differs from the recursive builder's");
        for (size_t i = 0; i < recursive.nodes.size(); ++i)
            if (std::memcmp(recursive.nodes[i].child, t.bvh.nodes[i].child, sizeof(recursive.nodes[i].child))) return fail("node numbering differs from the recursive builder's");
    }
    if (t.bvh.nodes.empty()) return fail("the level-wise tasks are no tree");
    t.wide = in_pairs ? collapse_to_wide_sah(t.bvh) : collapse_to_wide(t.bvh);
    again.wide = in_pairs ? collapse_to_wide_sah(again.bvh) : collapse_to_wide(again.bvh);
    if (hash_of(t) != hash_of(again)) return fail("two builds differ");
    if (t.bvh.max_depth > kMaxBvhDepth) return fail("binary depth");
    if (t.wide.stack_need > 64 && !deep_allowed) return fail("stack need"); // (scene creation keeps the binary tree of such a scene)
    if (t.bvh.prim_order.size() != sc.bounds.size()) return fail("reference count");
    // every primitive is named by exactly one leaf, whose (padded) box holds its bounds
    std::vector<uint32_t> named(sc.prims.size(), 0);
    for (const Node128& n : t.wide.nodes)
        for (int k = 0; k < 4; ++k) {
            const int32_t code = n.child[k];
            if (code >= 0 || code == kEmptyChild) continue;
            const uint32_t first = (uint32_t)(-1 - code) >> 3, count = (uint32_t)(-1 - code) & 7u;
            if (count > kMaxLeafPrims || first + count > t.bvh.prim_order.size()) return fail("leaf code out of range");
            for (uint32_t j = 0; j < count; ++j) {
                const Prim* p = sc.find(t.bvh.prim_order[first + j]);
                if (!p) return fail("leaf reference is not a primitive of the scene");
                const PrimBounds& b = sc.bounds[(size_t)(p - sc.prims.data())];
                named[(size_t)(p - sc.prims.data())]++;
                if (!(b.lo[0] >= n.lo_x[k] && b.lo[1] >= n.lo_y[k] && b.lo[2] >= n.lo_z[k] && b.hi[0] <= n.hi_x[k] && b.hi[1] <= n.hi_y[k] && b.hi[2] <= n.hi_z[k]))
                    return fail("coverage");
            }
        }
    for (const uint32_t c : named)
        if (c != 1) return fail("a primitive is not named exactly once");
    size_t hits = 0, blocked = 0;
    auto hit = [&](uint32_t shape, const Ray& r, double& dist) { return sc.hit(shape, r, dist); };
    for (const Ray& r : rays) {
        Counts c;
        const Hit a = walk(t, hit, r, c);
        Hit b;
        for (const PrimBounds& pb : sc.bounds) {
            double dist;
            if (!sc.hit(pb.shape, r, dist)) continue;
            if (r.limit >= 0.0f && dist * dist < r.limit) b.blocked = true;
            if (dist < b.dist) b.dist = dist, b.tri = pb.shape;
        }
        if (r.limit >= 0.0f) {
            if (a.blocked != b.blocked) return fail("any-hit differs from brute force");
            blocked += b.blocked;
        } else {
            if (a.dist != b.dist) return fail("closest hit differs from brute force");
            hits += b.tri >= 0;
        }
    }
    std::printf("OK %zu primitives, depth %u, stack %u, %zu rays (%zu closest hits, %zu blocked)\n", sc.prims.size(), t.bvh.max_depth, t.wide.stack_need, rays.size(), hits, blocked);
    // after everything the tool printed before: which paths of the device builder the input takes
    std::printf("paths largest_median %u medians_positive_small %u medians_positive_large %u medians_infinite_scale %u largest_forced_median %u most_large_nodes %u "
                "most_chunks %u degenerate_axis_splits %u root_centroid_extent %a %a %a\n",
                stats.largest_median, stats.medians_positive_small, stats.medians_positive_large, stats.medians_infinite_scale, stats.largest_forced_median,
                stats.most_large_nodes, stats.most_chunks, stats.degenerate_axis_splits, (double)stats.root_centroid_extent[0], (double)stats.root_centroid_extent[1],
                (double)stats.root_centroid_extent[2]);
    return 0;
}

int hash(int, char** argv) {
    const std::vector<Tri> tris = read_file<Tri>(argv[2]);
    std::printf("selected %016llx\n", (unsigned long long)hash_of(build(tris, spatial_splits_wanted(), cost_driven_collapse_wanted())));
    std::printf("old %016llx\n", (unsigned long long)hash_of(build(tris, false, false)));
    std::printf("cost %016llx\n", (unsigned long long)hash_of(build(tris, false, true)));
    std::printf("spatial %016llx\n", (unsigned long long)hash_of(build(tris, true, true)));
    return 0;
}

} // namespace

int main(int argc, char** argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "report")) return report(argc, argv);
    if (argc == 5 && !std::strcmp(argv[1], "check")) return check(argc, argv);
    if (argc == 3 && !std::strcmp(argv[1], "hash")) return hash(argc, argv);
    if ((argc == 4 || argc == 5 || (argc == 6 && !std::strcmp(argv[5], "deep"))) && !std::strcmp(argv[1], "level")) return level(argc, argv);
    std::fprintf(stderr, "usage: bvh_quality report TRIS NAME:RAYS... | check TRIS RAYS object|spatial | hash TRIS | level PRIMS RAYS|- [DEPTH_BOUND|- [deep]]\n");
    return 2;
}
