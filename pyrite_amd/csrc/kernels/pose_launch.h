// pose_launch.h -- what the pose kernels (kernels/pose.hip) and their host driver (live_scene.cpp pyr_scene_pose) share.
#pragma once
#include <hip/hip_runtime.h>

#include "../pose_rules.h"

namespace pyr {
struct DevLamp;
namespace devpose {

constexpr uint32_t kBlock = 256;

// One object on the device: its pose, its primitive ranges, and where its lanes begin in the launches over all objects'
// triangles and spheres (the running sums of the counts, in object order). 96 bytes.
struct DevObject {
    pose::Pose pose;
    uint32_t first_triangle, num_triangles, first_sphere, num_spheres;
    uint32_t triangle_lane, sphere_lane;
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
    uint32_t* beyond_range; // one word, zeroed before the call: set when a bound of a moved primitive fails the coordinate check
    DevLamp* lamps;
    uint32_t num_lamps;
};

// Each enqueues on `stream` and returns hipGetLastError().
hipError_t launch_pose(const Ctx& c, hipStream_t stream);  // triangles and spheres of every object into the staging arrays
hipError_t launch_lamps(const Ctx& c, hipStream_t stream); // the records of shape lamps from the staging arrays

} // namespace devpose
} // namespace pyr
