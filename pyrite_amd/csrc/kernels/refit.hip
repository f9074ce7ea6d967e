// refit.hip -- moving a live scene's geometry on the device, a unit of its own: the records that hold
// positions rewrite themselves from the new arrays, and every stored box of the trees is recomputed bottom-up by bvh_level.h's
// refit rules, the ones the host rehearsal (bvh.cpp refit_bvh / refit_wide) runs. Nothing here touches the render kernels.
//
// Repack: one lane per record, each lane stores to its own record only. Refit: one launch per height of a tree's schedule,
// deepest nodes first, one lane per node; a node reads the primitives' bounds and nodes of smaller heights, which earlier
// launches finished. No kernel waits for another workgroup, and every reduction is a min or a max, so the bytes written do not
// depend on scheduling.
#include "refit_launch.h"

#include "../device_scene.h"

namespace pyr {
namespace devrefit {

namespace {

typedef float float4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4_t load4(const float* p) { return *(const float4_t*)p; }
__device__ __forceinline__ void store4(float* p, float4_t v) { *(float4_t*)p = v; }

// a triangle's nine floats: 36 bytes a record, so only every fourth starts on a 16-byte boundary -- dword loads
__device__ __forceinline__ void load_triangle(const float* positions, uint32_t index, float* p) {
    const float* src = positions + 9 * (size_t)index;
    for (int k = 0; k < 9; ++k) p[k] = src[k];
}

// ---- DevPrim records in leaf order, their bounds, and the largest coordinate of the scene
__global__ __launch_bounds__(kBlock) void repack_prims_kernel(Ctx c) {
    __shared__ uint32_t block_max;
    if (threadIdx.x == 0) block_max = 0u;
    __syncthreads();
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    float mine = 0.0f;
    if (k < c.num_prims) {
        float* rec = c.prims + 12 * (size_t)k;
        const float4_t a = load4(rec);
        const uint32_t shape = lvl::float_bits(a.w), index = shape & 0x3FFFFFFFu, kind = shape >> 30;
        float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
        if (kind == PYR_SHAPE_TRIANGLE && index < c.num_triangles) {
            float p[9];
            load_triangle(c.tri_positions, index, p);
            lvl::triangle_bounds(p, lo, hi);
            if (c.write_triangles) { // edge1 = v2 - v1, edge2 = v3 - v1, as at creation
                store4(rec, float4_t{p[0], p[1], p[2], a.w});
                store4(rec + 4, float4_t{p[3] - p[0], p[4] - p[1], p[5] - p[2], 0.0f});
                store4(rec + 8, float4_t{p[6] - p[0], p[7] - p[1], p[8] - p[2], 0.0f});
            }
        } else if (kind == PYR_SHAPE_SPHERE && index < c.num_spheres) {
            const float4_t s = load4(c.spheres + 4 * (size_t)index);
            const float sp[4] = {s.x, s.y, s.z, s.w};
            lvl::sphere_bounds(sp, lo, hi);
            if (c.write_spheres) {
                store4(rec, float4_t{s.x, s.y, s.z, a.w});
                store4(rec + 4, float4_t{s.w, 0.0f, 0.0f, 0.0f});
                store4(rec + 8, float4_t{0.0f, 0.0f, 0.0f, 0.0f});
            }
        }
        store4(c.bounds + 8 * (size_t)k, float4_t{lo[0], lo[1], lo[2], 0.0f});
        store4(c.bounds + 8 * (size_t)k + 4, float4_t{hi[0], hi[1], hi[2], 0.0f});
        mine = lvl::grow_max_abs(0.0f, lo, hi);
    }
    // a coordinate's magnitude is never negative: its bits order like the floats, and a max does not care who comes first
    if (mine > 0.0f) atomicMax(&block_max, lvl::float_bits(mine));
    __syncthreads();
    if (threadIdx.x == 0 && block_max != 0u) atomicMax(c.max_abs_bits, block_max);
}

// ---- DevPrimPair records: both triangles of a record, from the shape codes it holds
__global__ __launch_bounds__(kBlock) void repack_pairs_kernel(Ctx c) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= c.num_pairs) return;
    float* rec = c.pair_prims + 20 * (size_t)r;
    float q[5][4];
    for (int j = 0; j < 5; ++j) {
        const float4_t v = load4(rec + 4 * j);
        q[j][0] = v.x, q[j][1] = v.y, q[j][2] = v.z, q[j][3] = v.w;
    }
    for (int h = 0; h < 2; ++h) {
        const uint32_t shape = lvl::float_bits(q[1][2 + h]), index = shape & 0x3FFFFFFFu;
        if (shape == PYR_HIT_NONE || (shape >> 30) != PYR_SHAPE_TRIANGLE || index >= c.num_triangles) continue; // the odd one out
        float p[9];
        load_triangle(c.tri_positions, index, p);
        q[0][0 + h] = p[0], q[0][2 + h] = p[1], q[1][0 + h] = p[2];
        q[2][0 + h] = p[3] - p[0], q[2][2 + h] = p[4] - p[1], q[3][0 + h] = p[5] - p[2];
        q[3][2 + h] = p[6] - p[0], q[4][0 + h] = p[7] - p[1], q[4][2 + h] = p[8] - p[2];
    }
    for (int j = 0; j < 5; ++j) store4(rec + 4 * j, float4_t{q[j][0], q[j][1], q[j][2], q[j][3]});
}

// ---- DevTriShade normals and DevTriTex frames, by original triangle index
__global__ __launch_bounds__(kBlock) void repack_shade_kernel(Ctx c) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= c.num_triangles) return;
    if (c.tri_normals) {
        float n[9];
        load_triangle(c.tri_normals, i, n);
        float* rec = c.tri_shade + 12 * (size_t)i;
        const float material = load4(rec).w;
        store4(rec, float4_t{n[0], n[1], n[2], material});
        store4(rec + 4, float4_t{n[3], n[4], n[5], 0.0f});
        store4(rec + 8, float4_t{n[6], n[7], n[8], 0.0f});
    }
    if (c.tri_frames && c.tri_tex) { // 48 bytes a triangle: three 16-byte loads
        const float* f = c.tri_frames + 12 * (size_t)i;
        float* rec = c.tri_tex + 20 * (size_t)i;
        store4(rec + 8, load4(f));
        store4(rec + 12, load4(f + 4));
        store4(rec + 16, load4(f + 8));
    }
}

__global__ __launch_bounds__(kBlock) void repack_spheres_kernel(Ctx c) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < c.num_spheres) store4(c.sphere_table + 4 * (size_t)i, load4(c.spheres + 4 * (size_t)i));
}

// the primitives' bounds as lvl::refit_leaf_box reads them: two 16-byte loads a primitive
struct DeviceBounds {
    const float* b;
    __device__ __forceinline__ void get(uint32_t i, float* lo, float* hi) const {
        const float4_t l = load4(b + 8 * (size_t)i), h = load4(b + 8 * (size_t)i + 4);
        lo[0] = l.x, lo[1] = l.y, lo[2] = l.z;
        hi[0] = h.x, hi[1] = h.y, hi[2] = h.z;
    }
};

// every child code of `node` names something that exists: the trees are the library's own, but nothing is indexed unchecked
template <class Node>
__device__ __forceinline__ bool codes_in_range(const Node& node, int slots, uint32_t num_nodes, uint32_t num_prims) {
    for (int k = 0; k < slots; ++k) {
        const int32_t code = node.child[k];
        if (code == lvl::kNoChild) continue;
        if (code >= 0 ? (uint32_t)code >= num_nodes : lvl::leaf_first(code) + lvl::leaf_count(code) > num_prims) return false;
    }
    return true;
}

// ---- one height of the binary tree: one lane per node
__global__ __launch_bounds__(kBlock) void refit_binary_kernel(Ctx c, const uint32_t* order, uint32_t count) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t n = order[i];
    if (n >= c.num_nodes) return;
    Node64 node = c.nodes[n];
    if (!codes_in_range(node, 2, c.num_nodes, c.num_prims)) return;
    const float pad = lvl::padding_of(lvl::bits_float(*c.max_abs_bits));
    lvl::refit_node(node, 2, (const Node64*)c.nodes, DeviceBounds{c.bounds}, pad);
    float* dst = (float*)(c.nodes + n); // the boxes: the node's first 48 bytes
    store4(dst, float4_t{node.lo_x[0], node.lo_x[1], node.lo_y[0], node.lo_y[1]});
    store4(dst + 4, float4_t{node.lo_z[0], node.lo_z[1], node.hi_x[0], node.hi_x[1]});
    store4(dst + 8, float4_t{node.hi_y[0], node.hi_y[1], node.hi_z[0], node.hi_z[1]});
}

// ---- one height of the four-child tree: one lane per node; the pair tree shares the topology and gets the same boxes
__global__ __launch_bounds__(kBlock) void refit_wide_kernel(Ctx c, const uint32_t* order, uint32_t count) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t n = order[i];
    if (n >= c.num_wide_nodes) return;
    Node128 node = c.wide_nodes[n];
    if (!codes_in_range(node, 4, c.num_wide_nodes, c.num_prims)) return;
    const float pad = lvl::padding_of(lvl::bits_float(*c.max_abs_bits));
    lvl::refit_node(node, 4, (const Node128*)c.wide_nodes, DeviceBounds{c.bounds}, pad);
    const float* rows[6] = {node.lo_x, node.lo_y, node.lo_z, node.hi_x, node.hi_y, node.hi_z};
    float* dst = (float*)(c.wide_nodes + n);
    float* twin = c.wide_pair_nodes ? (float*)(c.wide_pair_nodes + n) : nullptr;
    for (int r = 0; r < 6; ++r) { // the boxes: the node's first 96 bytes
        const float4_t v{rows[r][0], rows[r][1], rows[r][2], rows[r][3]};
        store4(dst + 4 * r, v);
        if (twin) store4(twin + 4 * r, v);
    }
}

uint32_t blocks_for(uint32_t n) { return (n + kBlock - 1) / kBlock; }

} // namespace

hipError_t launch_repack(const Ctx& c, hipStream_t stream) {
    if (c.num_prims) hipLaunchKernelGGL(repack_prims_kernel, dim3(blocks_for(c.num_prims)), dim3(kBlock), 0, stream, c);
    if (c.write_triangles && c.pair_prims && c.num_pairs) hipLaunchKernelGGL(repack_pairs_kernel, dim3(blocks_for(c.num_pairs)), dim3(kBlock), 0, stream, c);
    if (c.num_triangles && (c.tri_normals || (c.tri_frames && c.tri_tex)))
        hipLaunchKernelGGL(repack_shade_kernel, dim3(blocks_for(c.num_triangles)), dim3(kBlock), 0, stream, c);
    if (c.write_spheres && c.num_spheres) hipLaunchKernelGGL(repack_spheres_kernel, dim3(blocks_for(c.num_spheres)), dim3(kBlock), 0, stream, c);
    return hipGetLastError();
}

hipError_t launch_refit_binary(const Ctx& c, const uint32_t* order, uint32_t count, hipStream_t stream) {
    if (count) hipLaunchKernelGGL(refit_binary_kernel, dim3(blocks_for(count)), dim3(kBlock), 0, stream, c, order, count);
    return hipGetLastError();
}

hipError_t launch_refit_wide(const Ctx& c, const uint32_t* order, uint32_t count, hipStream_t stream) {
    if (count) hipLaunchKernelGGL(refit_wide_kernel, dim3(blocks_for(count)), dim3(kBlock), 0, stream, c, order, count);
    return hipGetLastError();
}

} // namespace devrefit
} // namespace pyr
