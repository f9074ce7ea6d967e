// scene_create.cpp -- scene creation's device half: pyr_scene_create[_with] and pyr_scene_destroy, and pack_geometry, which a
// rebuild runs again (live_scene.cpp rebuild_from). Everything is decided and packed on the host by scene_pack.cpp; the tree is
// built there or on the device (bvh_device.cpp); then every buffer is uploaded and every DevScene pointer set, here and nowhere
// else. Nothing of a PyrScene is written before the last refusal is behind it. DeviceBuffer's methods live here too.
#include <hip/hip_runtime.h>

#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "api_internal.h"
#include "bvh_device.h"
#include "scene_internal.h"

using namespace pyr;
using Clock = std::chrono::steady_clock;

namespace pyr {

void DeviceBuffer::release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    bytes = 0;
}
int DeviceBuffer::upload(const void* src, size_t n) {
    release();
    bytes = n;
    if (n == 0) n = 16; // keep pointers non-null
    HIP_TRY(hipMalloc(&ptr, n));
    if (bytes) HIP_TRY(hipMemcpy(ptr, src, bytes, hipMemcpyHostToDevice));
    return PYR_OK;
}
int DeviceBuffer::alloc(size_t n) {
    release();
    bytes = n;
    HIP_TRY(hipMalloc(&ptr, n ? n : 16));
    return PYR_OK;
}
int DeviceBuffer::reserve(size_t n) {
    if (ptr && bytes >= n) return PYR_OK;
    return alloc(n);
}

} // namespace pyr

PyrScene::~PyrScene() {
    if (tail_count) (void)hipFree(tail_count);
}

namespace {

// The geometry part of scene creation, decided: everything that depends on where the primitives are -- their bounds, the tree,
// the records in leaf order, the shading and texture-space records, the lamp records -- and the stage times so far.
struct Geometry {
    BuildPlan plan;
    BuiltBvh bvh;
    PackedRecords records;
    PyrBuildInfo build{};
};

// Build-plan step, tree, records step (scene_pack.h). Reads what the programs decided (needs_interpreter, the staged tables' size)
// and nothing else of a scene, and writes none: every refusal of the geometry part comes from here.
int make_geometry(const PyrSceneDesc* d, uint32_t builder, bool needs_interpreter, uint64_t table_floats, Geometry& g) {
    const auto t_start = Clock::now();
    PyrBuildInfo& build = g.build;
    build.builder_asked = builder;
    build.builder_used = PYR_BUILD_HOST;
    int rc = plan_build(d, g.plan);
    if (rc != PYR_OK) return rc;
    const auto t_bounds = Clock::now();
    bool built = false;
    if (builder == PYR_BUILD_DEVICE && g.plan.spatial) build.fallback_reason = PYR_BUILD_FALLBACK_SPATIAL_SPLITS; // only the host splits space
    if (builder == PYR_BUILD_DEVICE && !g.plan.spatial) {
        DeviceBuildReport report;
        std::string error;
        if (!build_bvh_device(g.plan.bounds, g.plan.pair_tree_expected, g.bvh, report, error)) return fail(PYR_ERR_DEVICE, error);
        build.fallback_reason = report.fallback_reason;
        build.finish_ms = (float)report.finish_ms;
        if (report.fallback_reason == PYR_BUILD_FALLBACK_NONE) {
            built = true;
            build.builder_used = PYR_BUILD_DEVICE;
            build.levels = report.levels;
            build.median_splits = report.median_splits;
        }
    }
    if (!built) g.bvh = build_planned_tree(d, g.plan, build.median_splits);
    const auto t_tree = Clock::now();
    build.bounds_ms = (float)ms_between(t_start, t_bounds);
    build.tree_ms = (float)ms_between(t_bounds, t_tree) - build.finish_ms;
    if ((rc = pack_records(d, g.bvh, g.plan, needs_interpreter, table_floats, g.records)) != PYR_OK) return rc;
    build.collapse_ms = (float)g.records.collapse_ms;
    return PYR_OK;
}

// One device buffer of a scene: `from` goes into `buffer`, and the DevScene pointer follows it -- or stays null where the
// kernels read "none" from that (`present` false).
template <class T>
int put(DeviceBuffer& buffer, View from, const T*& pointer, bool present = true) {
    const int rc = buffer.upload(from.data, from.bytes);
    pointer = rc == PYR_OK && present ? (const T*)buffer.ptr : nullptr;
    return rc;
}

int upload_geometry(PyrScene* s, Geometry& g) {
    const PackedRecords& r = g.records;
    DevScene& v = s->dev;
    int rc;
    if ((rc = put(s->tri_tex, r.tri_tex, v.tri_tex))) return rc;
    if ((rc = put(s->nodes, g.bvh.nodes, v.nodes))) return rc;
    if ((rc = put(s->pair_prims, r.pairs, v.pair_prims, !r.pairs.empty()))) return rc;
    if ((rc = put(s->wide_pair_nodes, r.pair_nodes, v.wide_pair_nodes, !r.pairs.empty()))) return rc;
    if ((rc = put(s->wide_nodes, r.wide.nodes, v.wide_nodes, !r.wide.nodes.empty()))) return rc;
    if ((rc = put(s->prims, r.prims, v.prims))) return rc;
    if ((rc = put(s->tri_shade, r.shade, v.tri_shade))) return rc;
    if ((rc = put(s->spheres, r.spheres, v.spheres))) return rc;
    if ((rc = put(s->lamps, r.lamps, v.lamps))) return rc;
    v.stack_depth = r.stack_depth;
    v.wide_stack_depth = r.wide_stack_depth;
    v.num_nodes = r.num_nodes;
    v.num_prims = r.num_prims;
    v.lds_table_floats = r.lds_table_floats;
    s->info = r.info;
    s->spatial_splits = g.plan.spatial;
    s->digest_source.reset(new BuiltBvh(std::move(g.bvh)));
    return PYR_OK;
}

int upload_tables(PyrScene* s, const PackedTables& t) {
    DevScene& v = s->dev;
    v = t.scene; // the scalars; every pointer follows its buffer below and in upload_geometry
    s->table_floats = t.table_floats;
    int rc;
    if ((rc = put(s->sphere_tex_scale, t.sphere_scale, v.sphere_tex_scale))) return rc;
    if ((rc = put(s->plane_frames, t.plane_frames, v.plane_frames))) return rc;
    if ((rc = put(s->textures, t.textures, v.textures))) return rc;
    if ((rc = put(s->texture_data, t.texture_data, v.texture_data))) return rc;
    if ((rc = put(s->sphere_material, t.sphere_material, v.sphere_material))) return rc;
    if ((rc = put(s->planes, t.planes, v.planes))) return rc;
    if ((rc = put(s->plane_material, t.plane_material, v.plane_material))) return rc;
    if ((rc = put(s->materials, t.materials, v.materials))) return rc;
    if ((rc = put(s->components, t.components, v.components))) return rc;
    if ((rc = put(s->programs, t.programs, v.programs))) return rc;
    if ((rc = put(s->instrs, t.instrs, v.instrs))) return rc;
    if ((rc = put(s->spectra, t.spectra, v.spectra))) return rc;
    if ((rc = put(s->spectrum_data, t.spectrum_data, v.spectrum_data))) return rc;
    if ((rc = put(s->rgb_basis, t.rgb_basis, v.rgb_basis))) return rc;
    return s->counters.alloc(sizeof(PyrCounters));
}

// The stage times of a creation or a rebuild that began at `t_start`: pack_upload_ms is what the named stages leave of the total.
void keep_build_info(PyrScene* s, PyrBuildInfo build, Clock::time_point t_start) {
    build.total_ms = (float)ms_between(t_start, Clock::now());
    build.pack_upload_ms = build.total_ms - build.bounds_ms - build.tree_ms - build.finish_ms - build.collapse_ms;
    s->build_info = build;
}

} // namespace

namespace pyr {

// Creation runs the geometry part once; pyr_scene_update(PYR_UPDATE_REBUILD) runs it again here on the same description with the
// new arrays, which is why a rebuilt scene is the scene creation makes. `d` needs its geometry fields and lamps only. A refusal
// leaves the scene as it was, build_info included.
int pack_geometry(const PyrSceneDesc* d, PyrScene* s, uint32_t builder) {
    const auto t_start = Clock::now();
    Geometry g;
    int rc = make_geometry(d, builder, s->dev.needs_interpreter != 0, s->table_floats, g);
    if (rc != PYR_OK) return rc;
    if ((rc = upload_geometry(s, g)) != PYR_OK) return rc;
    keep_build_info(s, g.build, t_start);
    return PYR_OK;
}

} // namespace pyr

extern "C" {

int pyr_scene_create(const PyrSceneDesc* desc, int device, PyrScene** out_scene) { return pyr_scene_create_with(desc, device, nullptr, out_scene); }

int pyr_scene_create_with(const PyrSceneDesc* desc, int device, const PyrBuildParams* build, PyrScene** out_scene) {
    if (!out_scene) return fail(PYR_ERR_INVALID_ARGUMENT, "null out pointer");
    *out_scene = nullptr;
    uint32_t builder = PYR_BUILD_HOST;
    if (build) { // checked before the description and before any device is looked for
        if (build->builder != PYR_BUILD_HOST && build->builder != PYR_BUILD_DEVICE) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrBuildParams.builder is neither PYR_BUILD_HOST nor PYR_BUILD_DEVICE");
        for (uint32_t word : build->reserved)
            if (word != 0) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrBuildParams.reserved must be zero");
        builder = build->builder;
    }
    int rc = validate(desc);
    if (rc != PYR_OK) return rc;
    // programs that declare more registers than the interpreter's in-register file get theirs renumbered (program_regs.h) before
    // anything else looks at them: the fast shapes, the tape forms and the kernels all see the allocated programs
    PyrSceneDesc allocated = *desc;
    std::vector<PyrProgram> programs;
    std::vector<PyrInstr> instrs;
    PyrProgramInfo info{};
    rc = allocate_scene_registers(desc, programs, instrs, info);
    if (rc != PYR_OK) return rc;
    allocated.programs = programs.data();
    allocated.instrs = instrs.data();
    allocated.num_instrs = (uint32_t)instrs.size(); // the caller's instructions and the renumbered programs' copies behind them
    int n = pyr_device_count();
    if (n <= 0) return fail(PYR_ERR_DEVICE, "no HIP device is visible; pyrite_gpu has no CPU path");
    if (device < 0 || device >= n) return fail(PYR_ERR_INVALID_ARGUMENT, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    const auto t_start = Clock::now();
    PackedTables tables;
    Geometry geometry;
    if ((rc = pack_tables(&allocated, info, tables)) != PYR_OK) return rc;
    if ((rc = make_geometry(&allocated, builder, tables.scene.needs_interpreter != 0, tables.table_floats, geometry)) != PYR_OK) return rc;
    std::unique_ptr<PyrScene> s(new PyrScene());
    s->device = device;
    s->num_cus = prop.multiProcessorCount;
    s->program_info = info;
    s->builder = builder;
    if ((rc = upload_tables(s.get(), tables)) != PYR_OK) return rc;
    if ((rc = upload_geometry(s.get(), geometry)) != PYR_OK) return rc;
    s->live.keep(&allocated);
    keep_build_info(s.get(), geometry.build, t_start); // all of scene creation, not the geometry part alone
    *out_scene = s.release();
    return PYR_OK;
}

void pyr_scene_destroy(PyrScene* scene) {
    if (!scene) return;
    (void)hipSetDevice(scene->device);
    delete scene;
}

} // extern "C"
