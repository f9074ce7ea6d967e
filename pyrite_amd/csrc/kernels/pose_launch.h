// pose_launch.h -- what the kernels of a live scene's deformation pipeline (kernels/pose.hip: morph, skin, pose, smooth, lamps) and
// their host driver (live_scene.cpp scene_pose) share: the records and contexts on the device, and the launchers. The bits of the
// flag word all of them raise are pose_rules.h's Flag -- that header states which failure raises which, and it is compiled where
// this one cannot be (the host rehearsal) -- named here as devpose::Flag for the two sides of the bus.
#pragma once
#include <hip/hip_runtime.h>

#include "../pose_rules.h"

namespace pyr {
struct DevLamp;
namespace devpose {

constexpr uint32_t kBlock = 256;
using Flag = pose::Flag; // kBeyondRange, kMorphedNormal, kSmoothedNormal, kBlendedRotation

// One object on the device: its pose, its primitive ranges, and where its lanes begin in the launches over all objects'
// triangles and spheres (the running sums of the counts, in object order). 96 bytes.
struct DevObject {
    pose::Pose pose;
    uint32_t first_triangle, num_triangles, first_sphere, num_spheres;
    uint32_t triangle_lane, sphere_lane;
};

// One skin on the device: its object's pose and triangles, where its lanes begin in the launch over all
// skinned triangles -- which is also where its bindings begin, the skins' bindings lying one after the other in skin order -- its
// rows of the joint table, and whether every one of them is exactly the identity (the host decides; such a skin is copied from
// rest). 96 bytes. The launch over the objects' triangles leaves a skinned object's triangles out.
struct DevSkin {
    pose::Pose pose;
    uint32_t first_triangle, num_triangles, lane;
    uint32_t first_joint, num_joints, identity;
};

// The rest pose, the scene's staging arrays the posed geometry is written to (the ones pyr_scene_update's host form uploads
// into and the refit reads), and the lamp records. Every count is the scene's own: the kernels index nothing they have not
// compared against one of them.
struct Ctx {
    const float* rest_positions; // [num_triangles][3][3]
    const float* rest_normals;   // [num_triangles][3][3]
    const float* rest_frames;    // [num_triangles][3][4] or nullptr: the scene keeps none
    const float* rest_spheres;   // [num_spheres][4]
    float* positions;            // staging, the same shapes
    float* normals;
    float* frames;
    float* spheres;
    const DevObject* objects;
    uint32_t num_objects;
    uint32_t num_triangles, num_spheres;         // the scene's counts
    uint32_t posed_triangles, posed_spheres;     // lanes: the objects' counts summed
    uint32_t* beyond_range; // the flag word, zeroed before the call: kBeyondRange when a bound of a moved primitive fails the coordinate check
    DevLamp* lamps;
    uint32_t num_lamps;
    // the skins (none: num_skins 0 and the rest unused)
    const DevSkin* skins;
    uint32_t num_skins;
    uint32_t skinned_triangles;   // lanes: the skins' triangle counts summed, and the rows of the two binding arrays
    uint32_t num_joints;          // rows of `joints`: the skins' joint counts summed
    const float* joints;          // [num_joints][12]: a joint's upper three rows, column by column
    const float* skin_weights;    // [skinned_triangles][3][4]
    const uint16_t* skin_joints;  // [skinned_triangles][3][4], relative to the skin's first joint
    // the dual-quaternion skins (none: dual_skins nullptr and joint_quats unused). Each of the two skin kernels
    // has a table of its own with num_skins records and the same lanes: a skin of the other kind has no triangles in it, so its
    // lanes do nothing there, as a skinned object's do in the launch over the objects' triangles.
    const DevSkin* dual_skins;
    const float* joint_quats;     // [num_joints][8]: a joint's unit dual quaternion (r, d), parallel to `joints`
};

// One morph on the device: its object's triangles, where its lanes begin in the launch over all morphed
// triangles, where its targets begin in the two delta buffers -- in rows of nine floats, a target being num_triangles rows and a
// morph's targets lying one after the other -- and its active targets of this frame in the pair table. 48 bytes.
struct DevMorph {
    uint32_t first_triangle, num_triangles, lane;
    uint32_t num_targets, has_normals;
    uint32_t first_active, num_active; // none active: the morph is at rest and its triangles are copied from rest
    uint32_t unused;
    uint64_t position_row, normal_row;
};
// One active target of a frame: the host packs every morph's targets whose weight is not zero, in ascending order.
struct ActiveTarget {
    uint32_t target;
    float weight;
};

// What the morph kernel reads and writes: the rest pose, the morphed rest (which the pose and skin kernels then take for their
// rest pose), the morphs, the frame's pairs and the deltas as uploaded, [target][triangle][3][3]. The kernel compares a triangle
// index against num_triangles and a target's row against the buffer's row count before it uses either.
struct MorphCtx {
    const float* rest_positions; // [num_triangles][3][3]
    const float* rest_normals;
    const float* rest_frames;    // or nullptr: the scene keeps none
    float* positions;            // the morphed rest, the same shapes
    float* normals;
    float* frames;
    const DevMorph* morphs;
    const ActiveTarget* active;
    const float* position_deltas; // [position_rows][3][3]
    const float* normal_deltas;   // [normal_rows][3][3]
    uint64_t position_rows, normal_rows;
    uint32_t num_morphs, num_active;
    uint32_t num_triangles;     // the scene's count
    uint32_t morphed_triangles; // lanes: the morphs' triangle counts summed
    uint32_t* flag; // the pose kernels' word: kBeyondRange as there; kMorphedNormal: a morphed normal or tangent that cannot be normalised
};

// What the smoothing kernel reads and writes: the staged positions as the morph, skin and pose kernels left
// them, the staged normals and frames it rewrites for the corners of smoothed objects, and the groups as a CSR -- group g's corners
// are group_corners[group_begin[g] .. group_begin[g + 1]), ascending. A corner is 3 * triangle + vertex over the scene's triangles,
// with bit 31 set where the triangle's face vector is negated (kNegated). The kernel compares a row against num_corners and a
// corner's triangle against num_triangles before it uses either.
constexpr uint32_t kNegated = 0x80000000u;
struct SmoothCtx {
    const float* positions; // staging, [num_triangles][3][3]
    float* normals;         // staging, the same shape
    float* frames;          // staging, [num_triangles][3][4], or nullptr: the scene keeps none
    const uint32_t* group_begin;   // [num_groups + 1]
    const uint32_t* group_corners; // [num_corners]
    uint32_t num_groups, num_corners;
    uint32_t num_triangles; // the scene's count
    uint32_t* flag; // the pose kernels' word: kBeyondRange as there; kSmoothedNormal: a recomputed normal or tangent that cannot be normalised
};

// Each enqueues on `stream` and returns hipGetLastError().
hipError_t launch_morph(const MorphCtx& c, hipStream_t stream); // every morph's triangles from rest into the morphed rest
hipError_t launch_pose(const Ctx& c, hipStream_t stream);  // triangles and spheres of every object, skinned or posed, into the staging arrays
hipError_t launch_smooth(const SmoothCtx& c, hipStream_t stream); // the normals and frames of every smoothed object from the staged positions
hipError_t launch_lamps(const Ctx& c, hipStream_t stream); // the records of shape lamps from the staging arrays

} // namespace devpose
} // namespace pyr
