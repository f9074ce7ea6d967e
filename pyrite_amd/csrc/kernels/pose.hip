// pose.hip -- a live scene's deformation pipeline on the device, morph -> skin -> pose -> smooth -> lamps (DESIGN.md sections 9g,
// 9h, 9p, 9q, 9r and 9s), a unit of its own: every primitive of an object is computed from the rest pose (where the scene has morphs:
// from the morphed rest, which the morph kernel writes first) and written to the scene's staging arrays, from where the refit of
// section 9f (kernels/refit.hip) rewrites the records and the boxes; the records of shape lamps follow from the staging arrays
// too. Nothing here touches a record the render kernels read except the lamp records, and those only after the host has seen
// the flag clear.
//
// What a lane computes is pose_rules.h's "one lane's walk", which the host rehearsal compiles too. This unit keeps what is the
// kernels' own: lane -> record -> index and its range checks, the loads and stores with their widths, the bounds checks on tables
// in memory, and the flag reduction.
//
// One lane per primitive of an object, each lane stores to its own primitive only (the smoothing kernel, which runs after them:
// one lane per group of corners, each lane stores to its own group's corners only); the only word two lanes share is the flag,
// which is an OR. No kernel waits for another workgroup.
#include "pose_launch.h"

#include "../bvh_level.h"
#include "../device_scene.h"

namespace pyr {
namespace devpose {

namespace {

typedef float float4_t __attribute__((ext_vector_type(4)));
typedef uint32_t uint2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float4_t load4(const float* p) { return *(const float4_t*)p; }
__device__ __forceinline__ void store4(float* p, float4_t v) { *(float4_t*)p = v; }

// the object whose lanes hold `lane`: the last one that begins at or before it (an object without lanes begins where the next
// one does, so it is never the last such one unless it is the last object, which begins at the lane count)
template <class Record, uint32_t Record::*kBegin>
__device__ __forceinline__ uint32_t object_of(const Record* objects, uint32_t num_objects, uint32_t lane) {
    uint32_t lo = 0, hi = num_objects;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (objects[mid].*kBegin <= lane)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__device__ __forceinline__ pose::Pose load_pose(const pose::Pose& from) {
    pose::Pose p;
    const float4_t c0 = load4(from.m), c1 = load4(from.m + 4), c2 = load4(from.m + 8), c3 = load4(from.m + 12);
    p.m[0] = c0.x, p.m[1] = c0.y, p.m[2] = c0.z, p.m[3] = c0.w;
    p.m[4] = c1.x, p.m[5] = c1.y, p.m[6] = c1.z, p.m[7] = c1.w;
    p.m[8] = c2.x, p.m[9] = c2.y, p.m[10] = c2.z, p.m[11] = c2.w;
    p.m[12] = c3.x, p.m[13] = c3.y, p.m[14] = c3.z, p.m[15] = c3.w;
    p.scale = from.scale;
    p.identity = from.identity;
    return p;
}

// the workgroup's OR of `mine` in LDS, then one atomic of the workgroup on the scene's word (every lane of the workgroup arrives here)
__device__ __forceinline__ void raise_flag(uint32_t mine, uint32_t* block_flag, uint32_t* flag) {
    if (mine) atomicOr(block_flag, mine);
    __syncthreads();
    if (threadIdx.x == 0 && *block_flag != 0u) atomicOr(flag, *block_flag);
}

// ---- what the three triangle kernels share (Ctx and MorphCtx name these arrays alike). 36 bytes a triangle, so only every fourth
// starts on a 16-byte boundary: dword loads and stores for positions and normals; a triangle's frames are 48 bytes: 16-byte loads
// and stores. A scene that keeps no frames gives a vertex a frame of zeros, which nothing reads.
template <class C>
__device__ __forceinline__ void load_positions(const C& c, uint32_t index, float* p) {
    const float* rest_p = c.rest_positions + 9 * (size_t)index;
    for (int k = 0; k < 9; ++k) p[k] = rest_p[k];
}
template <class C>
__device__ __forceinline__ void load_normal_frame(const C& c, uint32_t index, int v, float* n, float* q) {
    const float* rest_n = c.rest_normals + 9 * (size_t)index + 3 * v;
    n[0] = rest_n[0], n[1] = rest_n[1], n[2] = rest_n[2];
    q[0] = q[1] = q[2] = q[3] = 0.0f;
    if (c.rest_frames) {
        const float4_t f = load4(c.rest_frames + 12 * (size_t)index + 4 * v);
        q[0] = f.x, q[1] = f.y, q[2] = f.z, q[3] = f.w;
    }
}
template <class C>
__device__ __forceinline__ void store_normal_frame(const C& c, uint32_t index, int v, const float* n, const float* q) {
    if (c.rest_frames) store4(c.frames + 12 * (size_t)index + 4 * v, float4_t{q[0], q[1], q[2], q[3]});
    float* out_n = c.normals + 9 * (size_t)index + 3 * v;
    out_n[0] = n[0], out_n[1] = n[1], out_n[2] = n[2];
}
// the triangle's positions out, and the coordinate check on its box
template <class C>
__device__ __forceinline__ uint32_t store_positions(const C& c, uint32_t index, const float* p) {
    float* out_p = c.positions + 9 * (size_t)index;
    for (int k = 0; k < 9; ++k) out_p[k] = p[k];
    float lo[3], hi[3];
    lvl::triangle_bounds(p, lo, hi);
    return pose::bounds_flag(lo, hi);
}

// ---- one lane per triangle of an object: a vertex at a time through pose_rules.h pose_vertex
__global__ __launch_bounds__(kBlock) void pose_triangles_kernel(Ctx c) {
    __shared__ uint32_t block_flag;
    if (threadIdx.x == 0) block_flag = 0u;
    __syncthreads();
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
    uint32_t bad = 0u;
    if (lane < c.posed_triangles && c.num_objects != 0u) {
        const DevObject& object = c.objects[object_of<DevObject, &DevObject::triangle_lane>(c.objects, c.num_objects, lane)];
        const uint32_t within = lane - object.triangle_lane, index = object.first_triangle + within;
        if (within < object.num_triangles && index >= object.first_triangle && index < c.num_triangles) {
            const pose::Pose pose = load_pose(object.pose);
            float p[9];
            load_positions(c, index, p);
            for (int v = 0; v < 3; ++v) {
                float n[3], q[4];
                load_normal_frame(c, index, v, n, q);
                pose::pose_vertex(pose, p + 3 * v, n, q, c.rest_frames != nullptr);
                store_normal_frame(c, index, v, n, q);
            }
            bad = store_positions(c, index, p);
        }
    }
    raise_flag(bad, &block_flag, c.beyond_range);
}

// ---- one lane per triangle of a skin: a vertex at a time through pose_rules.h skin_vertex. A triangle's
// weights are 48 bytes: 16-byte loads; its joint indices are 24 bytes: 8-byte loads. The binding row is the lane. A skin at rest
// reads no binding.
__global__ __launch_bounds__(kBlock) void skin_triangles_kernel(Ctx c) {
    __shared__ uint32_t block_flag;
    if (threadIdx.x == 0) block_flag = 0u;
    __syncthreads();
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
    uint32_t bad = 0u;
    if (lane < c.skinned_triangles && c.num_skins != 0u) {
        const DevSkin& skin = c.skins[object_of<DevSkin, &DevSkin::lane>(c.skins, c.num_skins, lane)];
        const uint32_t within = lane - skin.lane, index = skin.first_triangle + within;
        const bool joints_inside = skin.num_joints != 0u && skin.first_joint < c.num_joints && skin.num_joints <= c.num_joints - skin.first_joint;
        if (within < skin.num_triangles && index >= skin.first_triangle && index < c.num_triangles && joints_inside) {
            const pose::Pose pose = load_pose(skin.pose);
            const uint32_t num_joints = skin.num_joints, rest_skin = skin.identity;
            const float* joints = c.joints + 12 * (size_t)skin.first_joint;
            float p[9];
            load_positions(c, index, p);
            for (int v = 0; v < 3; ++v) {
                float n[3], q[4], w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                uint32_t j[4] = {0u, 0u, 0u, 0u};
                load_normal_frame(c, index, v, n, q);
                if (!rest_skin) {
                    const float4_t wv = load4(c.skin_weights + 12 * (size_t)lane + 4 * v);
                    const uint2_t jv = *(const uint2_t*)(c.skin_joints + 12 * (size_t)lane + 4 * v);
                    w[0] = wv.x, w[1] = wv.y, w[2] = wv.z, w[3] = wv.w;
                    j[0] = jv.x & 0xFFFFu, j[1] = jv.x >> 16, j[2] = jv.y & 0xFFFFu, j[3] = jv.y >> 16;
                }
                bad |= pose::skin_vertex(joints, num_joints, rest_skin != 0u, j, w, pose, p + 3 * v, n, q, c.rest_frames != nullptr);
                store_normal_frame(c, index, v, n, q);
            }
            bad |= store_positions(c, index, p);
        }
    }
    raise_flag(bad, &block_flag, c.beyond_range);
}

// ---- the same lanes for the dual-quaternion skins, through pose_rules.h skin_vertex_dual: a kernel of its
// own, not a branch in the one above, whose code and registers stay what they were. The two read the same bindings and each its
// own skin table (Ctx::skins, Ctx::dual_skins), in which a skin of the other kind has no triangles, so that its lanes do nothing;
// each is launched only when a skin of its kind exists. A joint's dual quaternion is eight floats read as two 16-byte loads: 128
// bytes a vertex against the 192 of four linear joints.
__global__ __launch_bounds__(kBlock) void skin_triangles_dual_kernel(Ctx c) {
    __shared__ uint32_t block_flag;
    if (threadIdx.x == 0) block_flag = 0u;
    __syncthreads();
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
    uint32_t bad = 0u;
    if (lane < c.skinned_triangles && c.num_skins != 0u) {
        const DevSkin& skin = c.dual_skins[object_of<DevSkin, &DevSkin::lane>(c.dual_skins, c.num_skins, lane)];
        const uint32_t within = lane - skin.lane, index = skin.first_triangle + within;
        const bool joints_inside = skin.num_joints != 0u && skin.first_joint < c.num_joints && skin.num_joints <= c.num_joints - skin.first_joint;
        if (within < skin.num_triangles && index >= skin.first_triangle && index < c.num_triangles && joints_inside) {
            const pose::Pose pose = load_pose(skin.pose);
            const uint32_t num_joints = skin.num_joints, rest_skin = skin.identity;
            const float* quats = c.joint_quats + 8 * (size_t)skin.first_joint;
            float p[9];
            load_positions(c, index, p);
            for (int v = 0; v < 3; ++v) {
                float n[3], q[4], w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                uint32_t j[4] = {0u, 0u, 0u, 0u};
                load_normal_frame(c, index, v, n, q);
                if (!rest_skin) {
                    const float4_t wv = load4(c.skin_weights + 12 * (size_t)lane + 4 * v);
                    const uint2_t jv = *(const uint2_t*)(c.skin_joints + 12 * (size_t)lane + 4 * v);
                    w[0] = wv.x, w[1] = wv.y, w[2] = wv.z, w[3] = wv.w;
                    j[0] = jv.x & 0xFFFFu, j[1] = jv.x >> 16, j[2] = jv.y & 0xFFFFu, j[3] = jv.y >> 16;
                }
                bad |= pose::skin_vertex_dual(quats, num_joints, rest_skin != 0u, j, w, pose, p + 3 * v, n, q, c.rest_frames != nullptr);
                store_normal_frame(c, index, v, n, q);
            }
            bad |= store_positions(c, index, p);
        }
    }
    raise_flag(bad, &block_flag, c.beyond_range);
}

// ---- one lane per triangle of a morph: the triangle from rest into the morphed rest, which the two kernels
// above then read as their rest pose. Positions accumulate over the morph's active targets in nine registers; normals and frame go
// a vertex at a time (pose_rules.h add_delta and morphed_normal). The host has packed the active targets as (target, weight)
// pairs, so no inactive target's deltas are read, and a wave that lies inside one morph walks the pairs uniformly. A pair's target
// is compared against the morph's count and its row against the buffer's rows before any delta is read (pyr_scene_set_morphs and
// the host's packing make both hold: kBeyondRange otherwise, and the target is left out). The morphed rest is no moved primitive:
// its box is not checked here.
__global__ __launch_bounds__(kBlock) void morph_triangles_kernel(MorphCtx c) {
    __shared__ uint32_t block_flag;
    if (threadIdx.x == 0) block_flag = 0u;
    __syncthreads();
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
    uint32_t bad = 0u;
    if (lane < c.morphed_triangles && c.num_morphs != 0u) {
        const DevMorph& morph = c.morphs[object_of<DevMorph, &DevMorph::lane>(c.morphs, c.num_morphs, lane)];
        const uint32_t within = lane - morph.lane, index = morph.first_triangle + within;
        const uint32_t first_active = morph.first_active, num_active = morph.num_active, num_targets = morph.num_targets, rows = morph.num_triangles;
        const bool pairs_inside = first_active <= c.num_active && num_active <= c.num_active - first_active;
        if (within < rows && index >= morph.first_triangle && index < c.num_triangles && pairs_inside) {
            const ActiveTarget* active = c.active + first_active;
            const uint64_t position_row = morph.position_row + within, normal_row = morph.normal_row + within;
            const bool with_normals = pose::morph_moves_normals(morph.has_normals, num_active);
            float p[9];
            load_positions(c, index, p);
            for (uint32_t a = 0; a < num_active; ++a) {
                const uint32_t target = active[a].target;
                const float w = active[a].weight;
                const uint64_t row = position_row + (uint64_t)target * rows;
                if (target >= num_targets || row >= c.position_rows) {
                    bad |= pose::kBeyondRange;
                    continue;
                }
                pose::add_delta(p, w, c.position_deltas + 9 * row, 9);
            }
            float* out_p = c.positions + 9 * (size_t)index;
            for (int k = 0; k < 9; ++k) out_p[k] = p[k];
            for (int v = 0; v < 3; ++v) {
                float n[3], q[4];
                load_normal_frame(c, index, v, n, q);
                if (with_normals) {
                    for (uint32_t a = 0; a < num_active; ++a) {
                        const uint32_t target = active[a].target;
                        const float w = active[a].weight;
                        const uint64_t row = normal_row + (uint64_t)target * rows;
                        if (target >= num_targets || row >= c.normal_rows) {
                            bad |= pose::kBeyondRange;
                            continue;
                        }
                        pose::add_delta(n, w, c.normal_deltas + 9 * row + 3 * v, 3);
                    }
                    bad |= pose::morphed_normal(n, q, c.rest_frames != nullptr);
                }
                store_normal_frame(c, index, v, n, q);
            }
        }
    }
    raise_flag(bad, &block_flag, c.flag);
}

// ---- one lane per group of a smoothing, after the kernels above have written the staging arrays: the lane
// walks its row of the corner table twice. First it sums the signed face vectors of the corners' triangles (pose_rules.h add_face
// over the triangle's nine staged position dwords), in the row's order. Then it gives every corner of the row the normalised sum
// -- three dwords into the corner's slot of the staged normals -- and, where the scene keeps frames, rebuilds the corner's 16-byte
// staged frame against it (finish_corner; a scene without frames finishes the sum once, every corner getting the same three
// words). A lane stores to the corners of its own group only and reads positions only, which this kernel does not write; sums are
// in a fixed order, so there is no float atomic. The row is compared against the table's size and every corner's triangle against
// the scene's count before either is used (the host's packing makes both hold: kBeyondRange otherwise, and the corner is left out).
__global__ __launch_bounds__(kBlock) void smooth_normals_kernel(SmoothCtx c) {
    __shared__ uint32_t block_flag;
    if (threadIdx.x == 0) block_flag = 0u;
    __syncthreads();
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
    uint32_t bad = 0u;
    if (lane < c.num_groups) {
        const uint32_t begin = c.group_begin[lane], end = c.group_begin[lane + 1];
        if (begin <= end && end <= c.num_corners) {
            float m[3] = {0.0f, 0.0f, 0.0f};
            bool any = false;
            for (uint32_t k = begin; k < end; ++k) {
                const uint32_t word = c.group_corners[k], triangle = (word & ~kNegated) / 3u;
                if (triangle >= c.num_triangles) {
                    bad |= pose::kBeyondRange;
                    continue;
                }
                const float* from = c.positions + 9 * (size_t)triangle;
                float p[9];
                for (int a = 0; a < 9; ++a) p[a] = from[a];
                pose::add_face(p, (word & kNegated) != 0u, m, any);
            }
            float shared[3] = {m[0], m[1], m[2]};
            if (any && !c.frames) bad |= pose::finish_corner(m, shared, nullptr, false);
            for (uint32_t k = begin; any && k < end; ++k) {
                const uint32_t corner = c.group_corners[k] & ~kNegated;
                if (corner / 3u >= c.num_triangles) continue;
                float n[3] = {shared[0], shared[1], shared[2]};
                if (c.frames) {
                    const float4_t q4 = load4(c.frames + 4 * (size_t)corner);
                    float q[4] = {q4.x, q4.y, q4.z, q4.w};
                    bad |= pose::finish_corner(m, n, q, true);
                    store4(c.frames + 4 * (size_t)corner, float4_t{q[0], q[1], q[2], q[3]});
                }
                float* out = c.normals + 3 * (size_t)corner;
                out[0] = n[0], out[1] = n[1], out[2] = n[2];
            }
        } else {
            bad |= pose::kBeyondRange;
        }
    }
    raise_flag(bad, &block_flag, c.flag);
}

// ---- one lane per sphere of an object
__global__ __launch_bounds__(kBlock) void pose_spheres_kernel(Ctx c) {
    __shared__ uint32_t block_flag;
    if (threadIdx.x == 0) block_flag = 0u;
    __syncthreads();
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
    uint32_t bad = 0u;
    if (lane < c.posed_spheres && c.num_objects != 0u) {
        const DevObject& object = c.objects[object_of<DevObject, &DevObject::sphere_lane>(c.objects, c.num_objects, lane)];
        const uint32_t within = lane - object.sphere_lane, index = object.first_sphere + within;
        if (within < object.num_spheres && index >= object.first_sphere && index < c.num_spheres) {
            const pose::Pose pose = load_pose(object.pose);
            const float4_t r = load4(c.rest_spheres + 4 * (size_t)index);
            float s[4] = {r.x, r.y, r.z, r.w};
            pose::pose_sphere(pose, s);
            store4(c.spheres + 4 * (size_t)index, float4_t{s[0], s[1], s[2], s[3]});
            float lo[3], hi[3];
            lvl::sphere_bounds(s, lo, hi);
            bad = pose::bounds_flag(lo, hi);
        }
    }
    raise_flag(bad, &block_flag, c.beyond_range);
}

// ---- one lane per lamp: a shape lamp's record takes its shape from the staging arrays; directional and point lamps stay
__global__ __launch_bounds__(kBlock) void pose_lamps_kernel(Ctx c) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= c.num_lamps) return;
    DevLamp& lamp = c.lamps[i];
    if (lamp.kind != PYR_LAMP_SHAPE) return;
    const uint32_t index = lamp.shape_index;
    pose::LampShape shape;
    if (lamp.shape_kind == PYR_SHAPE_SPHERE && index < c.num_spheres) {
        const float4_t r = load4(c.spheres + 4 * (size_t)index);
        const float s[4] = {r.x, r.y, r.z, r.w};
        pose::lamp_of_sphere(s, shape);
        for (int a = 0; a < 3; ++a) lamp.v[a] = shape.v[a];
        lamp.width = shape.width;
        lamp.area = shape.area;
    } else if (lamp.shape_kind == PYR_SHAPE_TRIANGLE && index < c.num_triangles) {
        float p[9], n[9];
        for (int k = 0; k < 9; ++k) p[k] = c.positions[9 * (size_t)index + k], n[k] = c.normals[9 * (size_t)index + k];
        pose::lamp_of_triangle(p, n, shape);
        for (int a = 0; a < 3; ++a) {
            lamp.p1[a] = shape.p[a], lamp.p2[a] = shape.p[3 + a], lamp.p3[a] = shape.p[6 + a];
            lamp.n1[a] = shape.n[a], lamp.n2[a] = shape.n[3 + a], lamp.n3[a] = shape.n[6 + a];
        }
        lamp.area = shape.area;
    }
}

uint32_t blocks_for(uint32_t n) { return (n + kBlock - 1) / kBlock; }

} // namespace

hipError_t launch_morph(const MorphCtx& c, hipStream_t stream) {
    if (c.morphed_triangles) hipLaunchKernelGGL(morph_triangles_kernel, dim3(blocks_for(c.morphed_triangles)), dim3(kBlock), 0, stream, c);
    return hipGetLastError();
}

hipError_t launch_pose(const Ctx& c, hipStream_t stream) {
    if (c.posed_triangles) hipLaunchKernelGGL(pose_triangles_kernel, dim3(blocks_for(c.posed_triangles)), dim3(kBlock), 0, stream, c);
    if (c.skinned_triangles && c.skins) hipLaunchKernelGGL(skin_triangles_kernel, dim3(blocks_for(c.skinned_triangles)), dim3(kBlock), 0, stream, c);
    if (c.skinned_triangles && c.dual_skins) hipLaunchKernelGGL(skin_triangles_dual_kernel, dim3(blocks_for(c.skinned_triangles)), dim3(kBlock), 0, stream, c);
    if (c.posed_spheres) hipLaunchKernelGGL(pose_spheres_kernel, dim3(blocks_for(c.posed_spheres)), dim3(kBlock), 0, stream, c);
    return hipGetLastError();
}

hipError_t launch_smooth(const SmoothCtx& c, hipStream_t stream) {
    if (c.num_groups) hipLaunchKernelGGL(smooth_normals_kernel, dim3(blocks_for(c.num_groups)), dim3(kBlock), 0, stream, c);
    return hipGetLastError();
}

hipError_t launch_lamps(const Ctx& c, hipStream_t stream) {
    if (c.num_lamps) hipLaunchKernelGGL(pose_lamps_kernel, dim3(blocks_for(c.num_lamps)), dim3(kBlock), 0, stream, c);
    return hipGetLastError();
}

} // namespace devpose
} // namespace pyr
