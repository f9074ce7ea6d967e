// deform_check.cpp -- the host rehearsal of a live scene's deformation pipeline, morph -> skin -> pose -> smooth -> lamps (DESIGN.md
// sections 9g, 9h, 9p, 9q and 9r): the walk of one lane, as pose_rules.h states it and kernels/pose.hip compiles it, run on the CPU
// over rest arrays, poses, bindings, joint tables, targets, weights and corner labels read from a file. Every stage calls the
// function its kernel calls -- add_delta and morphed_normal, skin_vertex (which is pose_vertex for an object without a skin),
// pose_sphere, bounds_flag, add_face and finish_corner, lamp_of_* -- one triangle, one sphere, one group at a time; what is this
// program's own is what is the kernels' own there: which record a lane has, and the loads and stores. A stage a case does not use
// has a count of zero. A program of its own (tests/deform_probe.py builds it with -fsanitize=address,undefined; the four
// tests/test_scene_*_cpu.py compare what it writes, as bits, with the numpy restatements).
//
//   deform_check INPUT OUTPUT
//   INPUT   u32 num_triangles, num_spheres, has_frames, num_objects, num_lamps, num_skins, num_morphs, num_smoothings;
//           f32 positions[nt][9], normals[nt][9], frames[nt][12] (if has_frames), spheres[ns][4];
//           per object: u32 first_triangle, num_triangles, first_sphere, num_spheres; f32 transform[16], scale;
//           per lamp: u32 shape_kind (0 sphere, 1 triangle), shape_index;
//           per skin: u32 object, num_joints; f32 joints[num_joints][16]; f32 weights[T][3][4]; u16 indices[T][3][4] (T: the object's)
//           per morph: u32 object, num_targets, has_normals; f32 weights[num_targets]; f32 position_deltas[num_targets][T][9];
//                      f32 normal_deltas[num_targets][T][9] (if has_normals)
//           per smoothing: u32 object; u32 vertex_ids[T][3]
//   OUTPUT  the arrays in the same order; per lamp f32 v[3], width, p[9], n[9], area; u32 flag (pose_rules.h Flag)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>
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
    uint32_t first_triangle, num_triangles, first_sphere, num_spheres;
    Pose pose;
    int skin; // index into the skins, or -1
};
struct Skin {
    uint32_t object, num_joints;
    bool identity;             // every joint exactly the identity: copied from rest
    std::vector<float> rows;   // twelve floats a joint: the upper three rows, column by column
    std::vector<float> weights;
    std::vector<uint16_t> indices;
};
struct Smoothing {
    uint32_t object;
    std::vector<uint32_t> ids;
};
struct Morph {
    uint32_t object, num_targets, has_normals;
    std::vector<std::pair<uint32_t, float>> active; // the targets whose weight is not zero, ascending
    std::vector<float> position_deltas, normal_deltas;
};

} // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: deform_check INPUT OUTPUT\n");
        return 2;
    }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t head[8];
    if (std::fread(head, 4, 8, in) != 8) return 2;
    const uint32_t nt = head[0], ns = head[1], has_frames = head[2], num_objects = head[3], num_lamps = head[4], num_skins = head[5], num_morphs = head[6], num_smoothings = head[7];
    std::vector<float> positions, normals, frames, spheres;
    if (!read_n(in, positions, 9 * (size_t)nt) || !read_n(in, normals, 9 * (size_t)nt) || !read_n(in, frames, has_frames ? 12 * (size_t)nt : 0) || !read_n(in, spheres, 4 * (size_t)ns))
        return 2;
    std::vector<Object> objects(num_objects);
    for (Object& o : objects) {
        uint32_t range[4];
        float pose[17];
        if (std::fread(range, 4, 4, in) != 4 || std::fread(pose, 4, 17, in) != 17) return 2;
        o.first_triangle = range[0], o.num_triangles = range[1], o.first_sphere = range[2], o.num_spheres = range[3];
        if ((uint64_t)o.first_triangle + o.num_triangles > nt || (uint64_t)o.first_sphere + o.num_spheres > ns) return 3;
        bool same = pose[16] == 1.0f;
        for (int k = 0; k < 16; ++k) o.pose.m[k] = pose[k], same = same && pose[k] == kIdentity[k];
        o.pose.scale = pose[16];
        o.pose.identity = same ? 1u : 0u;
        o.skin = -1;
    }
    std::vector<uint32_t> lamps;
    if (!read_n(in, lamps, 2 * (size_t)num_lamps)) return 2;
    std::vector<Skin> skins(num_skins);
    for (uint32_t k = 0; k < num_skins; ++k) {
        Skin& s = skins[k];
        uint32_t word[2];
        if (std::fread(word, 4, 2, in) != 2) return 2;
        s.object = word[0], s.num_joints = word[1];
        if (s.object >= num_objects || s.num_joints == 0) return 3;
        std::vector<float> table;
        const size_t words = 12 * (size_t)objects[s.object].num_triangles;
        if (!read_n(in, table, 16 * (size_t)s.num_joints) || !read_n(in, s.weights, words) || !read_n(in, s.indices, words)) return 2;
        s.identity = true;
        s.rows.resize(12 * (size_t)s.num_joints);
        for (size_t j = 0; j < s.num_joints; ++j) {
            for (int e = 0; e < 16; ++e) s.identity = s.identity && table[16 * j + e] == kIdentity[e];
            for (int col = 0; col < 4; ++col)
                for (int row = 0; row < 3; ++row) s.rows[12 * j + 3 * col + row] = table[16 * j + 4 * col + row];
        }
        objects[s.object].skin = (int)k;
    }
    std::vector<Morph> morphs(num_morphs);
    for (Morph& m : morphs) {
        uint32_t word[3];
        if (std::fread(word, 4, 3, in) != 3) return 2;
        m.object = word[0], m.num_targets = word[1], m.has_normals = word[2];
        if (m.object >= num_objects || m.num_targets == 0 || m.num_targets > 256u) return 3;
        std::vector<float> weights;
        const size_t words = 9 * (size_t)objects[m.object].num_triangles * m.num_targets;
        if (!read_n(in, weights, m.num_targets) || !read_n(in, m.position_deltas, words) || !read_n(in, m.normal_deltas, m.has_normals ? words : 0)) return 2;
        for (uint32_t t = 0; t < m.num_targets; ++t)
            if (weights[t] != 0.0f) m.active.emplace_back(t, weights[t]);
    }
    std::vector<Smoothing> smoothings(num_smoothings);
    for (Smoothing& s : smoothings) {
        if (std::fread(&s.object, 4, 1, in) != 1) return 2;
        if (s.object >= num_objects) return 3;
        if (!read_n(in, s.ids, 3 * (size_t)objects[s.object].num_triangles)) return 2;
    }
    std::fclose(in);

    // ---- the morph: every morph's triangles from rest into the morphed rest (a copy of rest to begin with)
    std::vector<float> morphed_p = positions, morphed_n = normals, morphed_f = frames;
    uint32_t flag = 0;
    for (const Morph& m : morphs) {
        const Object& o = objects[m.object];
        const size_t rows = o.num_triangles;
        const bool with_normals = pose::morph_moves_normals(m.has_normals, (uint32_t)m.active.size());
        for (uint32_t t = 0; t < o.num_triangles; ++t) {
            const size_t index = (size_t)o.first_triangle + t;
            float p[9];
            std::memcpy(p, &positions[9 * index], sizeof(p));
            for (const auto& [target, w] : m.active) pose::add_delta(p, w, &m.position_deltas[9 * (target * rows + t)], 9);
            std::memcpy(&morphed_p[9 * index], p, sizeof(p));
            for (int v = 0; v < 3; ++v) {
                float n[3], q[4] = {0, 0, 0, 0};
                std::memcpy(n, &normals[9 * index + 3 * v], sizeof(n));
                if (has_frames) std::memcpy(q, &frames[12 * index + 4 * v], sizeof(q));
                if (with_normals) {
                    for (const auto& [target, w] : m.active) pose::add_delta(n, w, &m.normal_deltas[9 * (target * rows + t) + 3 * v], 3);
                    flag |= pose::morphed_normal(n, q, has_frames != 0);
                }
                if (has_frames) std::memcpy(&morphed_f[12 * index + 4 * v], q, sizeof(q));
                std::memcpy(&morphed_n[9 * index + 3 * v], n, sizeof(n));
            }
        }
    }

    // ---- the skins and the poses, from the morphed rest into the staging arrays: an object without a skin is a skin at rest
    std::vector<float> out_p = morphed_p, out_n = morphed_n, out_f = morphed_f, out_s = spheres;
    for (const Object& o : objects) {
        const Skin* skin = o.skin >= 0 ? &skins[(size_t)o.skin] : nullptr;
        const bool at_rest = !skin || skin->identity;
        for (uint32_t t = 0; t < o.num_triangles; ++t) {
            const size_t index = (size_t)o.first_triangle + t;
            float p[9], lo[3], hi[3];
            std::memcpy(p, &morphed_p[9 * index], sizeof(p));
            for (int v = 0; v < 3; ++v) {
                float n[3], q[4] = {0, 0, 0, 0}, w[4] = {0, 0, 0, 0};
                uint32_t j[4] = {0, 0, 0, 0};
                std::memcpy(n, &morphed_n[9 * index + 3 * v], sizeof(n));
                if (has_frames) std::memcpy(q, &morphed_f[12 * index + 4 * v], sizeof(q));
                if (!at_rest) {
                    std::memcpy(w, &skin->weights[12 * (size_t)t + 4 * v], sizeof(w));
                    for (int k = 0; k < 4; ++k) j[k] = skin->indices[12 * (size_t)t + 4 * v + k];
                }
                flag |= pose::skin_vertex(skin ? skin->rows.data() : nullptr, skin ? skin->num_joints : 0u, at_rest, j, w, o.pose, p + 3 * v, n, q, has_frames != 0);
                if (has_frames) std::memcpy(&out_f[12 * index + 4 * v], q, sizeof(q));
                std::memcpy(&out_n[9 * index + 3 * v], n, sizeof(n));
            }
            std::memcpy(&out_p[9 * index], p, sizeof(p));
            pyr::lvl::triangle_bounds(p, lo, hi);
            flag |= pose::bounds_flag(lo, hi);
        }
        for (uint32_t k = 0; k < o.num_spheres; ++k) { // neither a morph nor a skin touches its object's spheres
            const size_t index = (size_t)o.first_sphere + k;
            float s[4], lo[3], hi[3];
            std::memcpy(s, &spheres[4 * index], sizeof(s));
            pose::pose_sphere(o.pose, s);
            std::memcpy(&out_s[4 * index], s, sizeof(s));
            pyr::lvl::sphere_bounds(s, lo, hi);
            flag |= pose::bounds_flag(lo, hi);
        }
    }
    // ---- the smoothing: a group at a time, from the final positions into the normals and frames of its corners
    for (const Smoothing& s : smoothings) {
        const Object& o = objects[s.object];
        std::map<uint32_t, std::vector<uint32_t>> rows; // label -> its corners within the object, ascending
        for (uint32_t i = 0; i < (uint32_t)s.ids.size(); ++i) rows[s.ids[i]].push_back(i);
        for (const auto& [label, corners] : rows) {
            (void)label;
            float m[3] = {0, 0, 0};
            bool any = false;
            for (uint32_t i : corners) {
                const size_t index = (size_t)o.first_triangle + i / 3;
                pose::add_face(&out_p[9 * index], pose::face_negated(&positions[9 * index], &normals[9 * index]), m, any);
            }
            for (uint32_t i : corners) {
                const size_t corner = 3 * (size_t)o.first_triangle + i;
                flag |= pose::finish_corner(m, &out_n[3 * corner], has_frames ? &out_f[4 * corner] : nullptr, has_frames != 0);
            }
        }
    }
    std::vector<float> lamp_records;
    for (uint32_t i = 0; i < num_lamps; ++i) {
        const uint32_t kind = lamps[2 * i], index = lamps[2 * i + 1];
        pose::LampShape shape;
        std::memset(&shape, 0, sizeof(shape));
        if (kind == 0) {
            if (index >= ns) return 3;
            pose::lamp_of_sphere(&out_s[4 * (size_t)index], shape);
        } else {
            if (index >= nt) return 3;
            pose::lamp_of_triangle(&out_p[9 * (size_t)index], &out_n[9 * (size_t)index], shape);
        }
        lamp_records.insert(lamp_records.end(), shape.v, shape.v + 3);
        lamp_records.push_back(shape.width);
        lamp_records.insert(lamp_records.end(), shape.p, shape.p + 9);
        lamp_records.insert(lamp_records.end(), shape.n, shape.n + 9);
        lamp_records.push_back(shape.area);
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const bool ok = write_n(out, out_p) && write_n(out, out_n) && write_n(out, out_f) && write_n(out, out_s) && write_n(out, lamp_records) && std::fwrite(&flag, 4, 1, out) == 1;
    std::fclose(out);
    std::printf("deform_check: %u triangles, %u objects, %u skins, %u morphs, %u smoothings, %u lamps, flag %u\n", nt, num_objects, num_skins, num_morphs, num_smoothings, num_lamps, flag);
    return ok ? 0 : 2;
}
