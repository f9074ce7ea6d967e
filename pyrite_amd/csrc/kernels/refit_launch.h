// refit_launch.h -- what the refit kernels (kernels/refit.hip) and their host driver (live_scene.cpp pyr_scene_update) share.
#pragma once
#include <hip/hip_runtime.h>

#include "../bvh.h"
#include "../bvh_level.h"

namespace pyr {
namespace devrefit {

constexpr uint32_t kBlock = 256;

// The scene's records and the arrays they are rewritten from, all on the device. `tri_positions` and `spheres` are the
// primitives as they are NOW (the bounds of every leaf come from them, moved or not); `write_*` say which records the call
// rewrites. Every count is the scene's own: the kernels index nothing they have not compared against one of them.
struct Ctx {
    float* prims;      // DevPrim[num_prims], leaf order
    float* pair_prims; // DevPrimPair[num_pairs] or nullptr
    float* tri_shade;  // DevTriShade[num_triangles]
    float* tri_tex;    // DevTriTex[num_triangles] or nullptr
    float* sphere_table; // [num_spheres][4]
    const float* tri_positions; // [num_triangles][3][3]
    const float* tri_normals;   // [num_triangles][3][3] or nullptr: normals stay
    const float* tri_frames;    // [num_triangles][3][4] or nullptr: frames stay
    const float* spheres;       // [num_spheres][4]
    uint32_t num_prims, num_pairs, num_triangles, num_spheres;
    uint32_t write_triangles, write_spheres;
    float* bounds;          // [num_prims][8]: lo.xyz, 0, hi.xyz, 0 of the primitive at each leaf-order position
    uint32_t* max_abs_bits; // one word: the largest coordinate's float bits (zeroed before the call)
    Node64* nodes;
    uint32_t num_nodes;
    Node128* wide_nodes;      // or nullptr
    Node128* wide_pair_nodes; // the same topology with other leaf codes, or nullptr: gets the same boxes
    uint32_t num_wide_nodes;
};

// Each enqueues on `stream` and returns hipGetLastError().
hipError_t launch_repack(const Ctx& c, hipStream_t stream); // records, the primitives' bounds and the largest coordinate
// one height of a tree's schedule (bvh.h RefitSchedule): `order` on the device, `count` nodes
hipError_t launch_refit_binary(const Ctx& c, const uint32_t* order, uint32_t count, hipStream_t stream);
hipError_t launch_refit_wide(const Ctx& c, const uint32_t* order, uint32_t count, hipStream_t stream);

} // namespace devrefit
} // namespace pyr
