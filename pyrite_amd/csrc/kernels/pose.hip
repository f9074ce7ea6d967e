// pose.hip -- posing a live scene's objects, skinning its meshes, morphing them and recomputing their normals on the device (DESIGN.md sections 9g, 9h, 9p and 9q), a unit of its own: every primitive of an object
// is computed from the rest pose (where the scene has morphs: from the morphed rest, which the morph kernel writes first) by pose_rules.h and written to the scene's staging arrays, from where the refit of section 9f
// (kernels/refit.hip) rewrites the records and the boxes; the records of shape lamps follow from the staging arrays too. Nothing
// here touches a record the render kernels read except the lamp records, and those only after the host has seen the flag clear.
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

__device__ __forceinline__ bool box_beyond_range(const float* lo, const float* hi) {
    bool bad = false;
    for (int a = 0; a < 3; ++a) bad = bad || pose::beyond_range(lo[a]) || pose::beyond_range(hi[a]);
    return bad;
}

// the workgroup's OR in LDS, then one atomic of the workgroup on the scene's word (every lane of the workgroup arrives here)
__device__ __forceinline__ void raise_flag(bool mine, uint32_t* block_flag, uint32_t* flag) {
    if (mine) atomicOr(block_flag, 1u);
    __syncthreads();
    if (threadIdx.x == 0 && *block_flag != 0u) atomicOr(flag, 1u);
}

// ---- one lane per triangle of an object. 36 bytes a triangle, so only every fourth starts on a 16-byte boundary: dword loads
// and stores for positions and normals; a triangle's frames are 48 bytes: 16-byte loads and stores.
__global__ __launch_bounds__(kBlock) void pose_triangles_kernel(Ctx c) {
    __shared__ uint32_t block_flag;
    if (threadIdx.x == 0) block_flag = 0u;
    __syncthreads();
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
    bool bad = false;
    if (lane < c.posed_triangles && c.num_objects != 0u) {
        const DevObject& object = c.objects[object_of<DevObject, &DevObject::triangle_lane>(c.objects, c.num_objects, lane)];
        const uint32_t within = lane - object.triangle_lane, index = object.first_triangle + within;
        if (within < object.num_triangles && index >= object.first_triangle && index < c.num_triangles) {
            const pose::Pose pose = load_pose(object.pose);
            const float* rest_p = c.rest_positions + 9 * (size_t)index;
            const float* rest_n = c.rest_normals + 9 * (size_t)index;
            float* out_p = c.positions + 9 * (size_t)index;
            float* out_n = c.normals + 9 * (size_t)index;
            float p[9];
            for (int k = 0; k < 9; ++k) p[k] = rest_p[k];
            if (!pose.identity)
                for (int v = 0; v < 3; ++v) pose::pose_point(pose, p + 3 * v);
            for (int k = 0; k < 9; ++k) out_p[k] = p[k];
            float lo[3], hi[3];
            lvl::triangle_bounds(p, lo, hi);
            bad = box_beyond_range(lo, hi);
            for (int v = 0; v < 3; ++v) { // a vertex at a time: its normal and, where the scene keeps them, its frame
                float n[3] = {rest_n[3 * v], rest_n[3 * v + 1], rest_n[3 * v + 2]};
                if (c.rest_frames) {
                    const float4_t f = load4(c.rest_frames + 12 * (size_t)index + 4 * v);
                    float q[4] = {f.x, f.y, f.z, f.w};
                    if (!pose.identity) pose::pose_normal_frame(pose, n, q);
                    store4(c.frames + 12 * (size_t)index + 4 * v, float4_t{q[0], q[1], q[2], q[3]});
                } else if (!pose.identity) {
                    pose::pose_normal(pose, n);
                }
                out_n[3 * v] = n[0], out_n[3 * v + 1] = n[1], out_n[3 * v + 2] = n[2];
            }
        }
    }
    raise_flag(bad, &block_flag, c.beyond_range);
}

// ---- one lane per triangle of a skin: a vertex at a time, its matrix blended from the joints its binding
// names (pose_rules.h blend_joints), the per-vertex rule with that matrix, then the object's own pose as above. A triangle's
// weights are 48 bytes: 16-byte loads; its joint indices are 24 bytes: 8-byte loads. The binding row is the lane. A joint index is
// compared against the skin's count before it is used (pyr_scene_set_skins has refused such a binding: the flag, and joint 0).
__global__ __launch_bounds__(kBlock) void skin_triangles_kernel(Ctx c) {
    __shared__ uint32_t block_flag;
    if (threadIdx.x == 0) block_flag = 0u;
    __syncthreads();
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
    bool bad = false;
    if (lane < c.skinned_triangles && c.num_skins != 0u) {
        const DevSkin& skin = c.skins[object_of<DevSkin, &DevSkin::lane>(c.skins, c.num_skins, lane)];
        const uint32_t within = lane - skin.lane, index = skin.first_triangle + within;
        const bool joints_inside = skin.num_joints != 0u && skin.first_joint < c.num_joints && skin.num_joints <= c.num_joints - skin.first_joint;
        if (within < skin.num_triangles && index >= skin.first_triangle && index < c.num_triangles && joints_inside) {
            const pose::Pose pose = load_pose(skin.pose);
            const uint32_t num_joints = skin.num_joints, rest_skin = skin.identity;
            const float* joints = c.joints + 12 * (size_t)skin.first_joint;
            const float* rest_p = c.rest_positions + 9 * (size_t)index;
            const float* rest_n = c.rest_normals + 9 * (size_t)index;
            float* out_p = c.positions + 9 * (size_t)index;
            float* out_n = c.normals + 9 * (size_t)index;
            float p[9];
            for (int v = 0; v < 3; ++v) {
                float n[3] = {rest_n[3 * v], rest_n[3 * v + 1], rest_n[3 * v + 2]};
                float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int a = 0; a < 3; ++a) p[3 * v + a] = rest_p[3 * v + a];
                if (c.rest_frames) {
                    const float4_t f = load4(c.rest_frames + 12 * (size_t)index + 4 * v);
                    q[0] = f.x, q[1] = f.y, q[2] = f.z, q[3] = f.w;
                }
                if (!rest_skin) {
                    const float4_t wv = load4(c.skin_weights + 12 * (size_t)lane + 4 * v);
                    const uint2_t jv = *(const uint2_t*)(c.skin_joints + 12 * (size_t)lane + 4 * v);
                    const float w[4] = {wv.x, wv.y, wv.z, wv.w};
                    uint32_t j[4] = {jv.x & 0xFFFFu, jv.x >> 16, jv.y & 0xFFFFu, jv.y >> 16};
                    for (int k = 0; k < 4; ++k)
                        if (j[k] >= num_joints) j[k] = 0u, bad = true;
                    pose::Pose blended;
                    pose::blend_joints(joints, j, w, blended);
                    pose::pose_point(blended, p + 3 * v);
                    if (c.rest_frames)
                        pose::pose_normal_frame(blended, n, q);
                    else
                        pose::pose_normal(blended, n);
                }
                if (!pose.identity) {
                    pose::pose_point(pose, p + 3 * v);
                    if (c.rest_frames)
                        pose::pose_normal_frame(pose, n, q);
                    else
                        pose::pose_normal(pose, n);
                }
                if (c.rest_frames) store4(c.frames + 12 * (size_t)index + 4 * v, float4_t{q[0], q[1], q[2], q[3]});
                out_n[3 * v] = n[0], out_n[3 * v + 1] = n[1], out_n[3 * v + 2] = n[2];
            }
            for (int k = 0; k < 9; ++k) out_p[k] = p[k];
            float lo[3], hi[3];
            lvl::triangle_bounds(p, lo, hi);
            bad = bad || box_beyond_range(lo, hi);
        }
    }
    raise_flag(bad, &block_flag, c.beyond_range);
}

// ---- one lane per triangle of a morph: the triangle from rest into the morphed rest, which the two kernels
// above then read as their rest pose. Positions accumulate over the morph's active targets in nine registers; normals and frame go
// a vertex at a time through pose_rules.h morph_normal_frame. The host has packed the active targets as (target, weight) pairs, so
// no inactive target's deltas are read, and a wave that lies inside one morph walks the pairs uniformly. A pair's target is
// compared against the morph's count and its row against the buffer's rows before any delta is read (pyr_scene_set_morphs and the
// host's packing make both hold: bit 0 of the flag otherwise, and the target is left out). A morph with no active target is
// copied from rest, and so are normals and frames of a morph without normal deltas.
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
            const bool with_normals = morph.has_normals != 0u && num_active != 0u;
            const float* rest_p = c.rest_positions + 9 * (size_t)index;
            const float* rest_n = c.rest_normals + 9 * (size_t)index;
            float* out_p = c.positions + 9 * (size_t)index;
            float* out_n = c.normals + 9 * (size_t)index;
            float p[9];
            for (int k = 0; k < 9; ++k) p[k] = rest_p[k];
            for (uint32_t a = 0; a < num_active; ++a) {
                const uint32_t target = active[a].target;
                const float w = active[a].weight;
                const uint64_t row = position_row + (uint64_t)target * rows;
                if (target >= num_targets || row >= c.position_rows) {
                    bad |= 1u;
                    continue;
                }
                const float* d = c.position_deltas + 9 * row;
                for (int k = 0; k < 9; ++k) p[k] = p[k] + w * d[k];
            }
            for (int k = 0; k < 9; ++k) out_p[k] = p[k];
            for (int v = 0; v < 3; ++v) {
                float n[3] = {rest_n[3 * v], rest_n[3 * v + 1], rest_n[3 * v + 2]};
                float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (c.rest_frames) {
                    const float4_t f = load4(c.rest_frames + 12 * (size_t)index + 4 * v);
                    q[0] = f.x, q[1] = f.y, q[2] = f.z, q[3] = f.w;
                }
                if (with_normals) {
                    for (uint32_t a = 0; a < num_active; ++a) {
                        const uint32_t target = active[a].target;
                        const float w = active[a].weight;
                        const uint64_t row = normal_row + (uint64_t)target * rows;
                        if (target >= num_targets || row >= c.normal_rows) {
                            bad |= 1u;
                            continue;
                        }
                        const float* d = c.normal_deltas + 9 * row + 3 * v;
                        for (int k = 0; k < 3; ++k) n[k] = n[k] + w * d[k];
                    }
                    const bool outside = c.rest_frames ? pose::morph_normal_frame(n, q) : pose::morph_normal_frame(n, nullptr);
                    if (outside) bad |= 2u;
                }
                if (c.rest_frames) store4(c.frames + 12 * (size_t)index + 4 * v, float4_t{q[0], q[1], q[2], q[3]});
                out_n[3 * v] = n[0], out_n[3 * v + 1] = n[1], out_n[3 * v + 2] = n[2];
            }
        }
    }
    if (bad) atomicOr(&block_flag, bad);
    __syncthreads();
    if (threadIdx.x == 0 && block_flag != 0u) atomicOr(c.flag, block_flag);
}

// raise_flag for a kernel whose lanes raise more than bit 0: the workgroup's OR of `mine` in LDS, then one atomic on the scene's word
__device__ __forceinline__ void raise_flag_bits(uint32_t mine, uint32_t* block_flag, uint32_t* flag) {
    if (mine) atomicOr(block_flag, mine);
    __syncthreads();
    if (threadIdx.x == 0 && *block_flag != 0u) atomicOr(flag, *block_flag);
}

// ---- one lane per group of a smoothing, after the kernels above have written the staging arrays: the lane
// walks its row of the corner table twice. First it sums the signed face vectors of the corners' triangles (pose_rules.h
// signed_face_vector over the triangle's nine staged position dwords), in the row's order, starting from the first one. Then it
// gives every corner of the row the normalised sum -- three dwords into the corner's slot of the staged normals -- and, where the
// scene keeps frames, rebuilds the corner's 16-byte staged frame against it (morph_normal_frame). A lane stores to the corners of
// its own group only and reads positions only, which this kernel does not write; sums are in a fixed order, so there is no float
// atomic. The row is compared against the table's size and every corner's triangle against the scene's count before either is
// used (the host's packing makes both hold: bit 0 of the flag otherwise, and the corner is left out).
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
                    bad |= 1u;
                    continue;
                }
                const float* from = c.positions + 9 * (size_t)triangle;
                float p[9], f[3];
                for (int a = 0; a < 9; ++a) p[a] = from[a];
                pose::signed_face_vector(p, (word & kNegated) != 0u, f);
                if (any)
                    m[0] = m[0] + f[0], m[1] = m[1] + f[1], m[2] = m[2] + f[2];
                else
                    m[0] = f[0], m[1] = f[1], m[2] = f[2], any = true;
            }
            float shared[3] = {m[0], m[1], m[2]}; // a scene without frames: every corner gets the same three words
            if (any && !c.frames && pose::morph_normal_frame(shared, nullptr)) bad |= 4u;
            for (uint32_t k = begin; any && k < end; ++k) {
                const uint32_t corner = c.group_corners[k] & ~kNegated;
                if (corner / 3u >= c.num_triangles) continue;
                float n[3] = {shared[0], shared[1], shared[2]};
                if (c.frames) {
                    const float4_t q4 = load4(c.frames + 4 * (size_t)corner);
                    float q[4] = {q4.x, q4.y, q4.z, q4.w};
                    if (pose::morph_normal_frame(n, q)) bad |= 4u;
                    store4(c.frames + 4 * (size_t)corner, float4_t{q[0], q[1], q[2], q[3]});
                }
                float* out = c.normals + 3 * (size_t)corner;
                out[0] = n[0], out[1] = n[1], out[2] = n[2];
            }
        } else {
            bad |= 1u;
        }
    }
    raise_flag_bits(bad, &block_flag, c.flag);
}

// ---- one lane per sphere of an object
__global__ __launch_bounds__(kBlock) void pose_spheres_kernel(Ctx c) {
    __shared__ uint32_t block_flag;
    if (threadIdx.x == 0) block_flag = 0u;
    __syncthreads();
    const uint32_t lane = blockIdx.x * kBlock + threadIdx.x;
    bool bad = false;
    if (lane < c.posed_spheres && c.num_objects != 0u) {
        const DevObject& object = c.objects[object_of<DevObject, &DevObject::sphere_lane>(c.objects, c.num_objects, lane)];
        const uint32_t within = lane - object.sphere_lane, index = object.first_sphere + within;
        if (within < object.num_spheres && index >= object.first_sphere && index < c.num_spheres) {
            const pose::Pose pose = load_pose(object.pose);
            const float4_t r = load4(c.rest_spheres + 4 * (size_t)index);
            float s[4] = {r.x, r.y, r.z, r.w};
            if (!pose.identity) pose::pose_sphere(pose, s);
            store4(c.spheres + 4 * (size_t)index, float4_t{s[0], s[1], s[2], s[3]});
            float lo[3], hi[3];
            lvl::sphere_bounds(s, lo, hi);
            bad = box_beyond_range(lo, hi);
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
    if (c.skinned_triangles) hipLaunchKernelGGL(skin_triangles_kernel, dim3(blocks_for(c.skinned_triangles)), dim3(kBlock), 0, stream, c);
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
