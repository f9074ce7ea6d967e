// scene_pack.h -- scene creation's deciding half, on the host alone: what a description is refused for, and every table, record and
// scalar the kernels later trust without checking -- a program's fast shape and tape form, the PRODUCT split, hit_tape and its
// companions, which trees a scene gets, the pair records, lamp areas, plane frames, the staged tables' size. No HIP: scene_pack.cpp
// builds with a plain C++ compiler, and tests/probes/pack_check.cpp runs all of it without a device. scene_create.cpp uploads what
// comes out of here.
//
// Three steps: pack_tables (description -> programs, textures, frames and the scene's scalars), plan_build (description ->
// primitive bounds and the build switches), then -- the tree is built in between, by build_planned_tree or on the device --
// pack_records (description + tree -> the records in leaf order, the wide tree, the pair records).
#pragma once
#include <chrono>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/pyrite_gpu.h"
#include "bvh.h"
#include "device_scene.h"
#include "error.h"

namespace pyr {

double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b);

// pyrite_gpu.h "Coordinates": what plan_build, pyr_scene_update and pyr_scene_pose refuse, in the same words. The test runs
// once per primitive of every creation and update, so it is the one body here: a call into another unit costs a millisecond
// per million triangles.
constexpr float kMaxCoordinate = 1.0e15f;
extern const char* const kCoordinateRangeMessage;
inline bool within_coordinate_range(const PrimBounds& b) {
    for (int a = 0; a < 3; ++a)
        if (!(std::fabs(b.lo[a]) <= kMaxCoordinate && std::fabs(b.hi[a]) <= kMaxCoordinate)) return false;
    return true;
}

// What creation runs before the three steps, and the pieces of the steps that stand alone (each is described where it is defined).
int validate(const PyrSceneDesc* d);
int allocate_scene_registers(const PyrSceneDesc* desc, std::vector<PyrProgram>& programs, std::vector<PyrInstr>& instrs, PyrProgramInfo& info);
bool instr_reads_wavelength(const PyrInstr& ins);
DevProgram pack_program(const PyrInstr* instrs, const PyrProgram& p); // fast shape and tape form, but for PRODUCT
bool split_product(std::vector<PyrInstr>& instrs, const PyrProgram& p, PyrProgram& hit, PyrProgram& lambda, std::vector<uint32_t>& chain);
void plane_frame_from_normal(const float n[3], float q[4]);
DevLamp pack_lamp(const PyrSceneDesc* d, uint32_t i); // `d` needs its geometry fields and lamps

// Bytes that go to the device as they are: an array of the description (no copy is made), or a vector packed here.
struct View {
    const void* data = nullptr;
    size_t bytes = 0;
    View() = default;
    View(const void* data_, size_t bytes_) : data(data_), bytes(bytes_) {}
    template <class T>
    View(const std::vector<T>& v) : data(v.data()), bytes(v.size() * sizeof(T)) {}
};

// ---- the tables step: everything that does not depend on where the primitives are. `d` is the allocated description.
struct PackedTables {
    std::vector<DevProgram> programs; // the caller's, and behind them the two halves of every PRODUCT program
    std::vector<PyrInstr> instrs;     // the allocated description's, and behind them the halves' instructions
    std::vector<DevTexture> textures;
    std::vector<float> sphere_scale, plane_frames; // interpreter scenes only
    View texture_data, sphere_material, planes, plane_material, materials, components, spectra, spectrum_data, rgb_basis; // of the description
    DevScene scene{};          // every scalar of DevScene but the five of PackedRecords; the pointers are null
    uint64_t table_floats = 0; // the small tables the kernels stage into LDS, in floats (pack_records decides whether the scene is big enough to stage them)
};
int pack_tables(const PyrSceneDesc* d, const PyrProgramInfo& info, PackedTables& out);

// ---- the build-plan step: the primitives' bounds and the switches of one build, each read once per creation and per rebuild.
struct BuildPlan {
    std::vector<PrimBounds> bounds; // spheres, then triangles, each kind by index
    bool wide_allowed = true;       // PYRITE_WIDE_BVH is not 0: scenes that do not live in LDS get the four-child tree
    bool pairs_allowed = true;      // PYRITE_PAIR_PRIMS is not 0: a triangle-only wide tree gets pair records
    bool pair_tree_expected = false; // predicted before the tree exists (predicts_pair_tree): the builder counts leaves in pairs
    bool spatial = false;            // ... and splits space (PYRITE_SPATIAL_SPLITS, bvh.h): the host builder only
    bool cost_driven_collapse = false; // ... and the wide tree is collapsed by cost (PYRITE_WIDE_COLLAPSE, bvh.h)
};
int plan_build(const PyrSceneDesc* d, BuildPlan& plan); // refuses a primitive outside the coordinate range
// The host builders as the plan asks; `median_splits` receives build_bvh's count (the spatial builder does not count its own: 0).
BuiltBvh build_planned_tree(const PyrSceneDesc* d, const BuildPlan& plan, uint32_t& median_splits);

// "Too big to live in LDS": the binary tree and its primitive records outgrow the 8 KB the LDS-resident walk allows. Such a scene
// gets the four-child tree and stages its small tables instead of itself.
constexpr bool outgrows_lds(size_t nodes, size_t prims) { return nodes * 64 + prims * 48 > 8 * 1024; }

// ---- the records step: everything that depends on the tree. Refuses trees the kernels cannot walk or index.
struct PackedRecords {
    std::vector<DevPrim> prims; // in leaf order (spatial splits repeat some)
    std::vector<DevTriShade> shade;
    std::vector<DevTriTex> tri_tex; // interpreter scenes only
    std::vector<DevLamp> lamps;
    WideBvh wide;                     // empty: the scene lives in LDS, the tree is switched off, too deep or past 4 GB
    std::vector<DevPrimPair> pairs;   // empty: no wide tree, a sphere in the scene, or switched off
    std::vector<Node128> pair_nodes;  // the wide tree with leaf codes that count in pair records
    View spheres;                     // of the description
    uint32_t stack_depth = 1, wide_stack_depth = 1, num_nodes = 0, num_prims = 0, lds_table_floats = 0; // DevScene's fields of these names
    PyrBvhInfo info{};
    double collapse_ms = 0.0;
};
int pack_records(const PyrSceneDesc* d, const BuiltBvh& bvh, const BuildPlan& plan, bool needs_interpreter, uint64_t table_floats, PackedRecords& out);

} // namespace pyr
