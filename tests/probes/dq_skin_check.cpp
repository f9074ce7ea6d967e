// dq_skin_check.cpp -- the host rehearsal of the skin stage where a skin may blend its joints as dual quaternions (DESIGN.md section
// 9s): the walk of one lane of kernels/pose.hip's two skin kernels, as pose_rules.h states it, run on the CPU. A joint's dual
// quaternion comes from joint_dual_quaternion as live_scene.cpp makes it; a vertex goes through skin_vertex_dual or, for a linear
// skin, skin_vertex; an object without a skin is a skin at rest. What is this program's own is what is the kernels' own there: which
// record a lane has, and the loads and stores. A program of its own (tests/test_scene_dq_skin_cpu.py builds it with
// -fsanitize=address,undefined and compares what it writes, as bits, with tests/dq_skin_restatement.py).
//
//   dq_skin_check INPUT OUTPUT
//   INPUT   u32 num_triangles, has_frames, num_objects, num_skins;
//           f32 positions[nt][9], normals[nt][9], frames[nt][12] (if has_frames);
//           per object: u32 first_triangle, num_triangles; f32 transform[16], scale;
//           per skin: u32 object, num_joints, mode (0 linear, 1 dual quaternion); f32 joints[num_joints][16]; f32 weights[T][3][4];
//                     u16 indices[T][3][4] (T: the object's)
//   OUTPUT  the arrays in the same order; u32 flag (pose_rules.h Flag)
//   exit status 4: a joint of a dual-quaternion skin is no rotation (joint_is_rotation: what pyr_scene_skin refuses)
//
//   dq_skin_check raw INPUT OUTPUT       one blend per vertex from a table of dual quaternions taken as it is
//   INPUT   u32 num_joints, num_vertices; f32 table[num_joints][8]; f32 weights[V][4]; u16 indices[V][4]; f32 positions[V][3]
//   OUTPUT  f32 positions[V][3]; u32 flags[V]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../pyrite_amd/csrc/bvh_level.h"
#include "../../pyrite_amd/csrc/pose_rules.h"

namespace pose = pyr::pose;
using pose::Pose;

namespace {

template <class T>
bool read_n(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
bool write_n(FILE* f, const std::vector<T>& v) {
    return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

struct Object {
    uint32_t first_triangle, num_triangles;
    Pose pose;
    int skin; // index into the skins, or -1
};
struct Skin {
    uint32_t object, num_joints, mode;
    bool identity;            // every joint exactly the identity: copied from rest
    std::vector<float> table; // linear: twelve floats a joint, the upper three rows column by column; dual quaternion: eight
    std::vector<float> weights;
    std::vector<uint16_t> indices;
};

int raw(const char* source, const char* result) {
    FILE* in = std::fopen(source, "rb");
    if (!in) return 2;
    uint32_t head[2];
    if (std::fread(head, 4, 2, in) != 2) return 2;
    const uint32_t num_joints = head[0], count = head[1];
    std::vector<float> table, weights, positions;
    std::vector<uint16_t> indices;
    if (num_joints == 0 || !read_n(in, table, 8 * (size_t)num_joints) || !read_n(in, weights, 4 * (size_t)count) || !read_n(in, indices, 4 * (size_t)count) ||
        !read_n(in, positions, 3 * (size_t)count))
        return 2;
    std::fclose(in);
    Pose rest;
    std::memcpy(rest.m, kIdentity, sizeof(kIdentity));
    rest.scale = 1.0f, rest.identity = 1u;
    std::vector<uint32_t> flags(count);
    for (uint32_t v = 0; v < count; ++v) {
        float n[3] = {0.0f, 0.0f, 1.0f}, q[4] = {0, 0, 0, 0};
        const uint32_t j[4] = {indices[4 * (size_t)v], indices[4 * (size_t)v + 1], indices[4 * (size_t)v + 2], indices[4 * (size_t)v + 3]};
        flags[v] = pose::skin_vertex_dual(table.data(), num_joints, false, j, &weights[4 * (size_t)v], rest, &positions[3 * (size_t)v], n, q, false);
    }
    FILE* out = std::fopen(result, "wb");
    if (!out) return 2;
    const bool ok = write_n(out, positions) && write_n(out, flags);
    std::fclose(out);
    return ok ? 0 : 2;
}

} // namespace

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "raw") return raw(argv[2], argv[3]);
    if (argc != 3) {
        std::fprintf(stderr, "usage: dq_skin_check [raw] INPUT OUTPUT\n");
        return 2;
    }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t head[4];
    if (std::fread(head, 4, 4, in) != 4) return 2;
    const uint32_t nt = head[0], has_frames = head[1], num_objects = head[2], num_skins = head[3];
    std::vector<float> positions, normals, frames;
    if (!read_n(in, positions, 9 * (size_t)nt) || !read_n(in, normals, 9 * (size_t)nt) || !read_n(in, frames, has_frames ? 12 * (size_t)nt : 0)) return 2;
    std::vector<Object> objects(num_objects);
    for (Object& o : objects) {
        uint32_t range[2];
        float pose[17];
        if (std::fread(range, 4, 2, in) != 2 || std::fread(pose, 4, 17, in) != 17) return 2;
        o.first_triangle = range[0], o.num_triangles = range[1];
        if ((uint64_t)o.first_triangle + o.num_triangles > nt) return 3;
        bool same = pose[16] == 1.0f;
        for (int k = 0; k < 16; ++k) o.pose.m[k] = pose[k], same = same && pose[k] == kIdentity[k];
        o.pose.scale = pose[16];
        o.pose.identity = same ? 1u : 0u;
        o.skin = -1;
    }
    std::vector<Skin> skins(num_skins);
    for (uint32_t k = 0; k < num_skins; ++k) {
        Skin& s = skins[k];
        uint32_t word[3];
        if (std::fread(word, 4, 3, in) != 3) return 2;
        s.object = word[0], s.num_joints = word[1], s.mode = word[2];
        if (s.object >= num_objects || s.num_joints == 0 || s.mode > 1u) return 3;
        std::vector<float> joints;
        const size_t words = 12 * (size_t)objects[s.object].num_triangles;
        if (!read_n(in, joints, 16 * (size_t)s.num_joints) || !read_n(in, s.weights, words) || !read_n(in, s.indices, words)) return 2;
        s.identity = true;
        s.table.resize((s.mode ? 8 : 12) * (size_t)s.num_joints);
        for (size_t j = 0; j < s.num_joints; ++j) {
            for (int e = 0; e < 16; ++e) s.identity = s.identity && joints[16 * j + e] == kIdentity[e];
            if (s.mode) {
                if (!pose::joint_is_rotation(&joints[16 * j])) return 4;
                pose::joint_dual_quaternion(&joints[16 * j], &s.table[8 * j]);
                continue;
            }
            for (int col = 0; col < 4; ++col)
                for (int row = 0; row < 3; ++row) s.table[12 * j + 3 * col + row] = joints[16 * j + 4 * col + row];
        }
        objects[s.object].skin = (int)k;
    }
    std::fclose(in);

    std::vector<float> out_p = positions, out_n = normals, out_f = frames;
    uint32_t flag = 0;
    for (const Object& o : objects) {
        const Skin* skin = o.skin >= 0 ? &skins[(size_t)o.skin] : nullptr;
        const bool at_rest = !skin || skin->identity;
        for (uint32_t t = 0; t < o.num_triangles; ++t) {
            const size_t index = (size_t)o.first_triangle + t;
            float p[9], lo[3], hi[3];
            std::memcpy(p, &positions[9 * index], sizeof(p));
            for (int v = 0; v < 3; ++v) {
                float n[3], q[4] = {0, 0, 0, 0}, w[4] = {0, 0, 0, 0};
                uint32_t j[4] = {0, 0, 0, 0};
                std::memcpy(n, &normals[9 * index + 3 * v], sizeof(n));
                if (has_frames) std::memcpy(q, &frames[12 * index + 4 * v], sizeof(q));
                if (!at_rest) {
                    std::memcpy(w, &skin->weights[12 * (size_t)t + 4 * v], sizeof(w));
                    for (int k = 0; k < 4; ++k) j[k] = skin->indices[12 * (size_t)t + 4 * v + k];
                }
                if (skin && skin->mode)
                    flag |= pose::skin_vertex_dual(skin->table.data(), skin->num_joints, at_rest, j, w, o.pose, p + 3 * v, n, q, has_frames != 0);
                else
                    flag |= pose::skin_vertex(skin ? skin->table.data() : nullptr, skin ? skin->num_joints : 0u, at_rest, j, w, o.pose, p + 3 * v, n, q, has_frames != 0);
                if (has_frames) std::memcpy(&out_f[12 * index + 4 * v], q, sizeof(q));
                std::memcpy(&out_n[9 * index + 3 * v], n, sizeof(n));
            }
            std::memcpy(&out_p[9 * index], p, sizeof(p));
            pyr::lvl::triangle_bounds(p, lo, hi);
            flag |= pose::bounds_flag(lo, hi);
        }
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const bool ok = write_n(out, out_p) && write_n(out, out_n) && write_n(out, out_f) && std::fwrite(&flag, 4, 1, out) == 1;
    std::fclose(out);
    std::printf("dq_skin_check: %u triangles, %u objects, %u skins, flag %u\n", nt, num_objects, num_skins, flag);
    return ok ? 0 : 2;
}
