// pack_check.cpp -- scene creation's deciding half (pyrite_amd/csrc/scene_pack.h) without a device, for tests/test_scene_pack_cpu.py:
// reads a flat dump of a PyrSceneDesc (tests/scene_dump.py), runs validate, the register allocation, the tables step, the build-plan
// step, the host tree and the records step as scene_create.cpp does, and prints one line per packed table (name, bytes, FNV-1a-64
// of the bytes) and one per scalar of DevScene, PyrBvhInfo and PyrProgramInfo; for a refusal, the code and the message. Built with
// the sanitizers together with scene_pack.cpp, bvh.cpp, program_regs.cpp and error.cpp.
//
//   pack_check <dump>          (the build switches come from the environment, as they do at scene creation)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../pyrite_amd/csrc/scene_pack.h"

using namespace pyr;

namespace {

struct Reader {
    std::vector<char> bytes;
    size_t at = 0;
    std::vector<std::vector<char>> arrays; // the description borrows these
    bool ok = true;
    template <class T>
    void scalar(T& out) {
        if (at + sizeof(T) > bytes.size()) {
            ok = false;
            return;
        }
        std::memcpy(&out, bytes.data() + at, sizeof(T));
        at += sizeof(T);
    }
    template <class T>
    void array(const T*& out) { // a byte count and the bytes; 0: NULL
        uint64_t n = 0;
        scalar(n);
        out = nullptr;
        if (!ok || n == 0) return;
        if (n > bytes.size() - at) {
            ok = false;
            return;
        }
        arrays.emplace_back(bytes.begin() + (long)at, bytes.begin() + (long)(at + n)); // (operator new aligns for every record here)
        at += n;
        out = reinterpret_cast<const T*>(arrays.back().data());
    }
};

// PyrSceneDesc's fields in declaration order
void read_desc(Reader& r, PyrSceneDesc& d) {
    r.scalar(d.num_triangles), r.array(d.tri_positions), r.array(d.tri_normals), r.array(d.tri_uvs), r.array(d.tri_material);
    r.scalar(d.num_spheres), r.array(d.spheres), r.array(d.sphere_tex_scale), r.array(d.sphere_material);
    r.scalar(d.num_planes), r.array(d.planes), r.array(d.plane_material);
    r.scalar(d.num_lamps), r.array(d.lamps);
    r.scalar(d.num_materials), r.array(d.materials);
    r.scalar(d.num_components), r.array(d.components);
    r.scalar(d.num_programs), r.array(d.programs);
    r.scalar(d.num_instrs), r.array(d.instrs);
    r.scalar(d.num_spectra), r.array(d.spectra);
    r.scalar(d.num_spectrum_floats), r.array(d.spectrum_data);
    r.array(d.rgb_basis), r.scalar(d.rgb_basis_count), r.scalar(d.rgb_basis_min), r.scalar(d.rgb_basis_max);
    r.scalar(d.sky_program);
    r.scalar(d.num_textures), r.array(d.textures), r.scalar(d.num_texture_floats), r.array(d.texture_data);
    r.array(d.tri_frames), r.array(d.plane_frames);
}

void table(const char* name, View v) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* p = static_cast<const unsigned char*>(v.data);
    for (size_t i = 0; i < v.bytes; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    std::printf("table %s %zu %016" PRIx64 "\n", name, v.bytes, h);
}
void scalar(const char* name, uint64_t v) { std::printf("scalar %s %" PRIu64 "\n", name, v); }
void scalar_f(const char* name, float v) { // a float by its bits
    uint32_t b;
    std::memcpy(&b, &v, 4);
    std::printf("scalar %s 0x%08x\n", name, b);
}

int refused(int code) {
    std::printf("refused %d %s\n", code, pyr_last_error());
    return 0;
}

} // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    Reader r;
    {
        std::ifstream f(argv[1], std::ios::binary);
        if (!f) return 2;
        r.bytes.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    }
    PyrSceneDesc desc{};
    read_desc(r, desc);
    if (!r.ok || r.at != r.bytes.size()) return 3;

    int rc = validate(&desc);
    if (rc != PYR_OK) return refused(rc);
    PyrSceneDesc allocated = desc;
    std::vector<PyrProgram> programs;
    std::vector<PyrInstr> instrs;
    PyrProgramInfo info{};
    if ((rc = allocate_scene_registers(&desc, programs, instrs, info)) != PYR_OK) return refused(rc);
    allocated.programs = programs.data();
    allocated.instrs = instrs.data();
    allocated.num_instrs = (uint32_t)instrs.size();

    PackedTables t;
    if ((rc = pack_tables(&allocated, info, t)) != PYR_OK) return refused(rc);
    BuildPlan plan;
    if ((rc = plan_build(&allocated, plan)) != PYR_OK) return refused(rc);
    uint32_t median_splits = 0;
    const BuiltBvh bvh = build_planned_tree(&allocated, plan, median_splits);
    PackedRecords g;
    if ((rc = pack_records(&allocated, bvh, plan, t.scene.needs_interpreter != 0, t.table_floats, g)) != PYR_OK) return refused(rc);

    table("sphere_tex_scale", t.sphere_scale), table("plane_frames", t.plane_frames), table("textures", t.textures), table("texture_data", t.texture_data);
    table("sphere_material", t.sphere_material), table("planes", t.planes), table("plane_material", t.plane_material);
    table("materials", t.materials), table("components", t.components), table("programs", t.programs), table("instrs", t.instrs);
    table("spectra", t.spectra), table("spectrum_data", t.spectrum_data), table("rgb_basis", t.rgb_basis);
    table("tri_tex", g.tri_tex), table("nodes", bvh.nodes), table("pair_prims", g.pairs), table("wide_pair_nodes", g.pair_nodes), table("wide_nodes", g.wide.nodes);
    table("prims", g.prims), table("tri_shade", g.shade), table("spheres", g.spheres), table("lamps", g.lamps);

    const DevScene& v = t.scene;
    scalar("dev.num_planes", v.num_planes), scalar("dev.num_lamps", v.num_lamps), scalar("dev.rgb_count", v.rgb_count);
    scalar_f("dev.rgb_min", v.rgb_min), scalar_f("dev.rgb_max", v.rgb_max);
    scalar("dev.sky_program", v.sky_program), scalar("dev.stack_depth", g.stack_depth), scalar("dev.needs_interpreter", v.needs_interpreter);
    scalar("dev.num_nodes", g.num_nodes), scalar("dev.num_prims", g.num_prims), scalar("dev.num_spectra", v.num_spectra);
    scalar("dev.num_spectrum_floats", v.num_spectrum_floats), scalar("dev.num_programs", v.num_programs), scalar("dev.num_materials", v.num_materials);
    scalar("dev.num_components", v.num_components), scalar("dev.lds_table_floats", g.lds_table_floats), scalar("dev.wide_stack_depth", g.wide_stack_depth);
    scalar("dev.uses_textures", v.uses_textures), scalar("dev.hero_only_records", v.hero_only_records), scalar("dev.hit_tape", v.hit_tape);
    scalar("dev.rgb_records", v.rgb_records), scalar("dev.product_records", v.product_records), scalar("dev.micro_records", v.micro_records);
    scalar_f("dev.shadow_margin", v.shadow_margin), scalar("dev.tape_value_rows", v.tape_value_rows);
    scalar("dev.wide_nodes", !g.wide.nodes.empty()), scalar("dev.pair_prims", !g.pairs.empty()), scalar("dev.wide_pair_nodes", !g.pairs.empty()); // the pointers that may be null: 1 where set
    const PyrBvhInfo& b = g.info;
    scalar("bvh.num_nodes", b.num_nodes), scalar("bvh.num_leaves", b.num_leaves), scalar("bvh.max_depth", b.max_depth), scalar("bvh.num_primitives", b.num_primitives);
    scalar("bvh.node_bytes", b.node_bytes), scalar("bvh.primitive_bytes", b.primitive_bytes), scalar("bvh.num_wide_nodes", b.num_wide_nodes);
    scalar("bvh.num_pair_records", b.num_pair_records), scalar("bvh.wide_node_bytes", b.wide_node_bytes), scalar("bvh.pair_record_bytes", b.pair_record_bytes);
    scalar("program.declared_numbers", info.declared_numbers), scalar("program.declared_vectors", info.declared_vectors), scalar("program.declared_rgbs", info.declared_rgbs);
    scalar("program.allocated_numbers", info.allocated_numbers), scalar("program.allocated_vectors", info.allocated_vectors), scalar("program.allocated_rgbs", info.allocated_rgbs);
    scalar("program.wide", info.wide);
    scalar("scene.table_floats", t.table_floats), scalar("scene.spatial_splits", plan.spatial), scalar("scene.caller_programs", desc.num_programs);
    return 0;
}
