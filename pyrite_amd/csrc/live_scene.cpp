// live_scene.cpp -- everything that moves a scene after creation: pyr_scene_update[_device], pyr_scene_set_objects, pyr_scene_pose,
// pyr_scene_set_skins, pyr_scene_set_skin_blend, pyr_scene_skin, pyr_scene_set_morphs, pyr_scene_morph, pyr_scene_set_smoothing,
// pyr_scene_geometry, pyr_scene_update_info -- and pyr_scene_keep_previous, which copies where the geometry is now for the motion pass (api.cpp
// enqueues that one). LiveGeometry (scene_internal.h) says where the geometry is and which copies are valid; rebuild_from and
// refit_from are the two ways new arrays reach the records and trees on the device. The three calls that give a frame -- pose, skin,
// morph -- are one frame (Frame), one check (check_frame) and one run (scene_pose); the three that attach something to objects --
// skins, morphs, a smoothing -- are one check of the attachment (check_attachments) and one skeleton (set_attachments).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>

#include "bvh_level.h"
#include "kernels/refit_launch.h"
#include "scene_internal.h"

using namespace pyr;

// ------------------------------------------------------------------------------------------------ the live state
void LiveGeometry::keep(const PyrSceneDesc* d) {
    num_triangles = d->num_triangles, num_spheres = d->num_spheres;
    const float* const from[NUM_ARRAYS] = {d->tri_positions, d->tri_normals, d->tri_frames, d->spheres};
    arrays[FRAMES].kept = d->tri_frames != nullptr;
    for (int k = 0; k < NUM_ARRAYS; ++k)
        if (arrays[k].kept) arrays[k].host.assign(from[k], from[k] + floats(k));
    tri_material.assign(d->tri_material, d->tri_material + num_triangles);
    has_uvs = d->tri_uvs != nullptr, has_tex_scale = d->sphere_tex_scale != nullptr;
    if (has_uvs) tri_uvs.assign(d->tri_uvs, d->tri_uvs + 6 * (size_t)num_triangles);
    sphere_material.assign(d->sphere_material, d->sphere_material + num_spheres);
    if (has_tex_scale) sphere_tex_scale.assign(d->sphere_tex_scale, d->sphere_tex_scale + 2 * (size_t)num_spheres);
    lamps.assign(d->lamps, d->lamps + d->num_lamps);
}

PyrSceneDesc LiveGeometry::view(const float* const with[NUM_ARRAYS]) const {
    const float* a[NUM_ARRAYS];
    for (int k = 0; k < NUM_ARRAYS; ++k) a[k] = with && with[k] ? with[k] : arrays[k].kept ? arrays[k].host.data() : nullptr;
    PyrSceneDesc d{};
    d.num_triangles = num_triangles, d.num_spheres = num_spheres, d.num_lamps = (uint32_t)lamps.size();
    d.tri_positions = a[POSITIONS], d.tri_normals = a[NORMALS], d.tri_frames = a[FRAMES], d.spheres = a[SPHERES];
    d.tri_material = tri_material.data(), d.sphere_material = sphere_material.data();
    d.tri_uvs = has_uvs ? tri_uvs.data() : nullptr;
    d.sphere_tex_scale = has_tex_scale ? sphere_tex_scale.data() : nullptr;
    d.lamps = lamps.data();
    return d;
}

// (the description is current: whoever forgets the objects has fetched it)
void LiveGeometry::recount_lanes() {
    posed_triangles = posed_spheres = 0;
    for (const devpose::DevObject& o : pose_table) posed_triangles += o.num_triangles, posed_spheres += o.num_spheres;
    posed_triangles -= skin.triangles; // a skinned object's triangles have their lanes in the skin kernel's launch
}

void LiveGeometry::forget_skins() {
    skin.clear();
    recount_lanes(); // the launch over the objects' triangles has every object's again
}

void LiveGeometry::forget_morphs() { morph.clear(); }

void LiveGeometry::forget_smoothing() {
    smooth.clear();
}

void LiveGeometry::forget_objects() {
    pose_table.clear();
    forget_skins();
    forget_morphs();
    forget_smoothing();
    for (LiveArray& a : arrays) a.rest.release();
    pose_objects.release();
}

void LiveGeometry::adopted(const float* const given[NUM_ARRAYS], bool staged) {
    if (given[POSITIONS] || given[NORMALS] || given[FRAMES] || given[SPHERES]) forget_objects(); // new arrays are a new geometry, not a pose of the old one
    for (int k = 0; k < NUM_ARRAYS; ++k)
        if (given[k]) arrays[k].host.assign(given[k], given[k] + floats(k)), arrays[k].kept = true;
    if (given[POSITIONS]) positions_staged_ = staged;
}

namespace {

using Clock = std::chrono::steady_clock;
const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
enum { POSITIONS = LiveGeometry::POSITIONS, NORMALS = LiveGeometry::NORMALS, FRAMES = LiveGeometry::FRAMES, SPHERES = LiveGeometry::SPHERES, NUM_ARRAYS = LiveGeometry::NUM_ARRAYS };

// What every way of moving a scene refuses, around what only one of them does (`specific`, which also refuses a null scene where
// its entry point has not done so before): an unknown mode and a reserved word first; a live session and the refit of a
// split-space tree last. `name`: the update's struct; `noun`: what the session's message calls the call.
template <class Update, class Specific>
int check_move(const PyrScene* scene, const Update* u, const std::string& name, const char* noun, Specific specific) {
    if (u->mode != PYR_UPDATE_REFIT && u->mode != PYR_UPDATE_REBUILD) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".mode is neither PYR_UPDATE_REFIT nor PYR_UPDATE_REBUILD");
    for (uint32_t word : u->reserved)
        if (word != 0) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".reserved must be zero");
    const int rc = specific();
    if (rc != PYR_OK) return rc;
    if (scene->live_sessions != 0) return fail(PYR_ERR_INVALID_ARGUMENT, std::string("the scene has a live PyrSession: destroy it before the ") + noun);
    if (u->mode == PYR_UPDATE_REFIT && scene->spatial_splits)
        return fail(PYR_ERR_UNSUPPORTED, "the scene's tree was built with spatial splits (PYRITE_SPATIAL_SPLITS=1): its leaves hold clipped boxes, ask for PYR_UPDATE_REBUILD");
    return PYR_OK;
}

// What both forms of pyr_scene_update refuse before any device is looked for, in the order pyrite_gpu.h gives.
int check_update_args(const PyrScene* scene, const PyrGeometryUpdate* u) {
    if (!u) return fail(PYR_ERR_INVALID_ARGUMENT, "null update");
    return check_move(scene, u, "PyrGeometryUpdate", "update", [&]() {
        if (u->num_triangles == 0 && (u->tri_positions || u->tri_normals || u->tri_frames)) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrGeometryUpdate.num_triangles is 0 but a triangle array is given");
        if (u->num_spheres == 0 && u->spheres) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrGeometryUpdate.num_spheres is 0 but spheres are given");
        if (!scene) return fail(PYR_ERR_INVALID_ARGUMENT, "null scene");
        if (u->num_triangles != scene->live.num_triangles) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrGeometryUpdate.num_triangles is not the scene's");
        if (u->num_spheres != scene->live.num_spheres) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrGeometryUpdate.num_spheres is not the scene's");
        return (int)PYR_OK;
    });
}

// One frame of a live scene as pyr_scene_pose, pyr_scene_skin and pyr_scene_morph give it: the mode, and the three tables of which a
// NULL one keeps what the scene is in. An entry point fills what its update has and leaves the rest null.
struct Frame {
    uint32_t mode = 0;
    const PyrObjectPose* poses = nullptr;
    uint32_t num_objects = 0;
    const float* joints = nullptr;
    uint32_t num_joints = 0;
    const float* weights = nullptr;
    uint32_t num_weights = 0;
};
// What an entry point's update has of the three tables: none at all, one it must give, or one it may leave NULL. `name`: the
// update's struct in the messages; `noun`: what the session's message calls the call.
enum Part { ABSENT, REQUIRED, MAY_KEEP };
struct FrameRules {
    const char *name, *noun;
    Part poses, joints, weights;
};
const FrameRules kPoseFrame{"PyrPoseUpdate", "pose", REQUIRED, ABSENT, ABSENT}, kSkinFrame{"PyrSkinUpdate", "skin", MAY_KEEP, REQUIRED, ABSENT},
    kMorphFrame{"PyrMorphUpdate", "morph", MAY_KEEP, MAY_KEEP, MAY_KEEP};

bool affine(const float* m) { return m[3] == 0.0f && m[7] == 0.0f && m[11] == 0.0f && m[15] == 1.0f; }

// What the three refuse before any device is looked for, in the order pyrite_gpu.h gives: the poses; that the scene has morphs,
// where the update has weights; the joint table where it must be or is given; the weight table where it is given.
template <class Update>
int check_frame(const PyrScene* scene, const Update* u, const Frame& f, const FrameRules& r) {
    if (!u) return fail(PYR_ERR_INVALID_ARGUMENT, "null update");
    if (!scene) return fail(PYR_ERR_INVALID_ARGUMENT, "null scene");
    const std::string name = r.name;
    return check_move(scene, u, name, r.noun, [&]() {
        const LiveGeometry& live = scene->live;
        if (f.poses)
            for (uint32_t i = 0; i < f.num_objects; ++i)
                for (uint32_t word : f.poses[i].reserved)
                    if (word != 0) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrObjectPose.reserved must be zero");
        if (live.pose_table.empty()) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".num_objects: the scene has no objects (pyr_scene_set_objects names them)");
        if (f.num_objects != live.pose_table.size()) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".num_objects is not the scene's");
        if (!f.poses && r.poses == REQUIRED) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".poses is null");
        for (uint32_t i = 0; f.poses && i < f.num_objects; ++i) {
            for (float x : f.poses[i].transform)
                if (!std::isfinite(x)) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrObjectPose.transform has an entry that is not finite");
            if (!std::isfinite(f.poses[i].scale)) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrObjectPose.scale is not finite");
        }
        for (uint32_t i = 0; f.poses && i < f.num_objects; ++i)
            if (!affine(f.poses[i].transform)) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrObjectPose.transform: the last row must be 0, 0, 0, 1");
        if (r.weights != ABSENT && !live.morph.set()) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".num_weights: the scene has no morphs (pyr_scene_set_morphs sets them)");
        if (r.joints == REQUIRED || f.joints) {
            if (!live.skin.set()) return fail(PYR_ERR_INVALID_ARGUMENT, name + (r.joints == REQUIRED ? ".num_joints" : ".joints") + ": the scene has no skins (pyr_scene_set_skins binds them)");
            if ((size_t)f.num_joints * 16 != live.skin.joints.size()) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".num_joints is not the scene's");
            if (!f.joints) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".joints is null");
            for (size_t k = 0; k < live.skin.joints.size(); ++k)
                if (!std::isfinite(f.joints[k])) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".joints has an entry that is not finite");
            for (uint32_t j = 0; j < f.num_joints; ++j)
                if (!affine(f.joints + 16 * (size_t)j)) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".joints: the last row must be 0, 0, 0, 1");
            for (const LiveGeometry::Skin& skin : live.skin.table)
                for (uint32_t j = skin.first_joint; skin.blend == PYR_SKIN_DUAL_QUATERNION && j < skin.first_joint + skin.num_joints; ++j)
                    if (!pose::joint_is_rotation(f.joints + 16 * (size_t)j))
                        return fail(PYR_ERR_INVALID_ARGUMENT, name + ".joints: a joint of a dual-quaternion skin must have a rotation for its upper 3x3 (orthonormal columns within 1e-3, right-handed)");
        }
        if (f.weights) {
            if (f.num_weights != live.morph.weights.size()) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".num_weights is not the scene's");
            for (uint32_t k = 0; k < f.num_weights; ++k)
                if (!std::isfinite(f.weights[k])) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".weights has a weight that is not finite");
        }
        return (int)PYR_OK;
    });
}

// The refit's schedules and scratch, made from the trees on the device at the first refit after a build -- scene creation pays
// nothing for them. The binary tree is fetched for it anyway, so its area sum at the build is taken here too.
int prepare_refit(PyrScene* s) {
    LiveGeometry& live = s->live;
    if (live.schedule_current()) return PYR_OK;
    std::vector<Node64> nodes(s->info.num_nodes);
    HIP_TRY(hipMemcpy(nodes.data(), s->nodes.ptr, nodes.size() * sizeof(Node64), hipMemcpyDeviceToHost));
    if (!live.area_known()) live.area_at_build(child_area_sum(nodes.data(), nodes.size()));
    const RefitSchedule binary = refit_schedule(nodes.data(), nodes.size());
    int rc;
    if ((rc = live.order_binary.upload(binary.order.data(), binary.order.size() * 4)) != PYR_OK) return rc;
    live.sched_binary = binary.begin;
    live.sched_wide.clear();
    if (s->info.num_wide_nodes) {
        std::vector<Node128> wide(s->info.num_wide_nodes);
        HIP_TRY(hipMemcpy(wide.data(), s->wide_nodes.ptr, wide.size() * sizeof(Node128), hipMemcpyDeviceToHost));
        const RefitSchedule sched = refit_schedule(wide.data(), wide.size());
        if ((rc = live.order_wide.upload(sched.order.data(), sched.order.size() * 4)) != PYR_OK) return rc;
        live.sched_wide = sched.begin;
    }
    if ((rc = live.bounds.alloc((size_t)s->dev.num_prims * 32)) != PYR_OK) return rc;
    if ((rc = live.max_abs.alloc(4)) != PYR_OK) return rc;
    live.scheduled();
    return PYR_OK;
}

// Every record and every box from `sources` on the device (nullptr: that array stays; the positions are the triangles as they are
// NOW, moved or not: the bounds of every leaf need them). The records first, then one launch per height and tree, deepest nodes
// first. `waits`: the blocking form, whose stage times are the device's. `uploaded_at`: when the sources were complete, or nullptr:
// now, once the uploads enqueued on `stream` are in. Fills the rest of `info` and makes it the scene's.
int refit_from(PyrScene* s, const float* const sources[NUM_ARRAYS], bool write_triangles, bool write_spheres, bool waits, hipStream_t stream, Clock::time_point t_start,
               const Clock::time_point* uploaded_at, PyrUpdateInfo info) {
    LiveGeometry& live = s->live;
    devrefit::Ctx c{};
    c.prims = (float*)s->prims.ptr, c.num_prims = s->dev.num_prims;
    c.pair_prims = s->info.num_pair_records ? (float*)s->pair_prims.ptr : nullptr, c.num_pairs = s->info.num_pair_records;
    c.tri_shade = (float*)s->tri_shade.ptr;
    c.tri_tex = s->tri_tex.bytes ? (float*)s->tri_tex.ptr : nullptr;
    c.sphere_table = (float*)s->spheres.ptr;
    c.num_triangles = live.num_triangles, c.num_spheres = live.num_spheres;
    c.bounds = (float*)live.bounds.ptr, c.max_abs_bits = (uint32_t*)live.max_abs.ptr;
    c.nodes = (Node64*)s->nodes.ptr, c.num_nodes = s->info.num_nodes;
    c.wide_nodes = s->info.num_wide_nodes ? (Node128*)s->wide_nodes.ptr : nullptr, c.num_wide_nodes = s->info.num_wide_nodes;
    c.wide_pair_nodes = s->info.num_pair_records ? (Node128*)s->wide_pair_nodes.ptr : nullptr;
    c.write_triangles = write_triangles ? 1u : 0u, c.write_spheres = write_spheres ? 1u : 0u;
    c.tri_positions = sources[POSITIONS], c.tri_normals = sources[NORMALS], c.tri_frames = sources[FRAMES];
    c.spheres = sources[SPHERES] ? sources[SPHERES] : (const float*)s->spheres.ptr;
    HIP_TRY(hipMemsetAsync(live.max_abs.ptr, 0, 4, stream));
    if (waits) HIP_TRY(hipStreamSynchronize(stream));
    const auto t_uploaded = uploaded_at ? *uploaded_at : Clock::now();
    hipError_t e = devrefit::launch_repack(c, stream);
    if (e != hipSuccess) return hip_fail(e, "refit: repack kernels");
    if (waits) HIP_TRY(hipStreamSynchronize(stream));
    const auto t_prims = Clock::now();
    for (size_t h = 0; h + 1 < live.sched_binary.size(); ++h) {
        e = devrefit::launch_refit_binary(c, (const uint32_t*)live.order_binary.ptr + live.sched_binary[h], live.sched_binary[h + 1] - live.sched_binary[h], stream);
        if (e != hipSuccess) return hip_fail(e, "refit: binary tree");
    }
    for (size_t h = 0; h + 1 < live.sched_wide.size(); ++h) {
        e = devrefit::launch_refit_wide(c, (const uint32_t*)live.order_wide.ptr + live.sched_wide[h], live.sched_wide[h + 1] - live.sched_wide[h], stream);
        if (e != hipSuccess) return hip_fail(e, "refit: four-child tree");
    }
    if (waits) HIP_TRY(hipStreamSynchronize(stream));
    const auto t_end = Clock::now();
    info.levels = live.sched_binary.empty() ? 0u : (uint32_t)live.sched_binary.size() - 1u;
    info.updates = live.update_info.updates + 1u;
    info.upload_ms = (float)ms_between(t_start, t_uploaded);
    info.prims_ms = (float)ms_between(t_uploaded, t_prims);
    info.refit_ms = (float)ms_between(t_prims, t_end);
    info.total_ms = (float)ms_between(t_start, t_end);
    live.update_info = info;
    return PYR_OK;
}

// The geometry part of scene creation over the description with `arrays` on the host in place of its own (nullptr: that array
// stays) and the scene's builder: the only call of pack_geometry after creation. Every buffer it uploads is replaced, so the caller
// has waited for whatever of this scene was in flight. A refusal leaves the scene as it was; otherwise the description adopts the
// arrays (and so forgets the objects, if there is one), the refit starts over, and `info` becomes the scene's.
int rebuild_from(PyrScene* s, const float* const arrays[NUM_ARRAYS], Clock::time_point t_start, PyrUpdateInfo info) {
    const PyrSceneDesc d = s->live.view(arrays);
    const int rc = pack_geometry(&d, s, s->builder);
    if (rc != PYR_OK) return rc;
    s->live.adopted(arrays, false);
    s->live.built();
    info.updates = 0;
    info.total_ms = (float)ms_between(t_start, Clock::now());
    s->live.update_info = info;
    return PYR_OK;
}

// The host description follows the staging arrays a pose wrote (nothing else leaves it behind).
int fetch_live_geometry(PyrScene* s) {
    LiveGeometry& live = s->live;
    if (live.host_current()) return PYR_OK;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    for (int k = 0; k < NUM_ARRAYS; ++k)
        if (const size_t n = live.kept_floats(k)) HIP_TRY(hipMemcpy(live.arrays[k].host.data(), live.arrays[k].staging.ptr, n * 4, hipMemcpyDeviceToHost));
    live.fetched();
    return PYR_OK;
}

// ------------------------------------------------------------------------------------------------ pyr_scene_update
int scene_update(PyrScene* s, const PyrGeometryUpdate* u, bool device_arrays, hipStream_t stream) {
    const auto t_start = Clock::now();
    HIP_TRY(hipSetDevice(s->device));
    LiveGeometry& live = s->live;
    int rc = fetch_live_geometry(s); // a pose left the description behind: what stays comes from it
    if (rc != PYR_OK) return rc;
    // ---- the new arrays on the host: the caller's own, or copies of the device arrays
    const float* const given[NUM_ARRAYS] = {u->tri_positions, u->tri_normals, u->tri_frames, u->spheres};
    const float* host[NUM_ARRAYS] = {given[0], given[1], given[2], given[3]};
    std::vector<float> fetched[NUM_ARRAYS];
    if (device_arrays) {
        for (int k = 0; k < NUM_ARRAYS; ++k) {
            if (!given[k]) continue;
            fetched[k].resize(live.floats(k));
            HIP_TRY(hipMemcpyAsync(fetched[k].data(), given[k], live.floats(k) * 4, hipMemcpyDeviceToHost, stream));
            host[k] = fetched[k].data();
        }
        HIP_TRY(hipStreamSynchronize(stream));
    }
    // ---- the coordinate check of scene creation, on the bounds of what moved, before anything of the scene is written
    for (int k : {(int)SPHERES, (int)POSITIONS}) {
        if (!host[k]) continue;
        for (const float *p = host[k], *end = p + live.floats(k); p != end; p += live.arrays[k].width) {
            PrimBounds b;
            k == SPHERES ? lvl::sphere_bounds(p, b.lo, b.hi) : lvl::triangle_bounds(p, b.lo, b.hi);
            if (!within_coordinate_range(b)) return fail(PYR_ERR_UNSUPPORTED, kCoordinateRangeMessage);
        }
    }
    PyrUpdateInfo info{};
    info.mode_used = u->mode;
    info.area_ratio = 1.0;

    if (u->mode == PYR_UPDATE_REBUILD) {
        HIP_TRY(hipDeviceSynchronize());
        return rebuild_from(s, host, t_start, info);
    }

    // ---- refit: where the kernels read the arrays -- the caller's device arrays, or the scene's own copies of the host arrays
    if ((rc = prepare_refit(s)) != PYR_OK) return rc;
    const float* source[NUM_ARRAYS] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < NUM_ARRAYS; ++k) {
        if (!given[k]) continue;
        if (device_arrays) {
            source[k] = given[k];
        } else {
            DeviceBuffer& own = live.arrays[k].staging;
            if ((rc = own.reserve(live.floats(k) * 4)) != PYR_OK) return rc;
            HIP_TRY(hipMemcpyAsync(own.ptr, given[k], live.floats(k) * 4, hipMemcpyHostToDevice, stream));
            source[k] = (const float*)own.ptr;
        }
    }
    if (!given[POSITIONS] && live.num_triangles) { // the triangles stay: their positions as the scene keeps them
        LiveArray& positions = live.arrays[POSITIONS];
        if (!live.positions_staged()) {
            if ((rc = positions.staging.reserve(live.floats(POSITIONS) * 4)) != PYR_OK) return rc;
            HIP_TRY(hipMemcpyAsync(positions.staging.ptr, positions.host.data(), live.floats(POSITIONS) * 4, hipMemcpyHostToDevice, stream));
            live.staged_positions();
        }
        source[POSITIONS] = (const float*)positions.staging.ptr;
    }
    live.adopted(host, !device_arrays); // the description the scene keeps follows the device
    // the lamp records, on the host with creation's arithmetic (lamps are few)
    bool shape_lamps = false;
    for (const PyrLamp& l : live.lamps) shape_lamps = shape_lamps || l.kind == PYR_LAMP_SHAPE;
    if (shape_lamps) {
        HIP_TRY(hipStreamSynchronize(stream)); // an earlier update's copy may still read lamp_records
        const PyrSceneDesc d = live.view();
        live.lamp_records.resize(live.lamps.size());
        for (uint32_t i = 0; i < (uint32_t)live.lamps.size(); ++i) live.lamp_records[i] = pack_lamp(&d, i);
        HIP_TRY(hipMemcpyAsync(s->lamps.ptr, live.lamp_records.data(), live.lamp_records.size() * sizeof(DevLamp), hipMemcpyHostToDevice, stream));
    }
    return refit_from(s, source, given[POSITIONS] != nullptr, given[SPHERES] != nullptr, !device_arrays, stream, t_start, nullptr, info);
}

// ------------------------------------------------------------------------------------------------ pyr_scene_pose
void set_pose(devpose::DevObject& o, const float* transform, float scale) {
    bool same = scale == 1.0f;
    for (int k = 0; k < 16; ++k) o.pose.m[k] = transform[k], same = same && transform[k] == kIdentity[k];
    o.pose.scale = scale;
    o.pose.identity = same ? 1u : 0u;
}

devpose::Ctx pose_context(PyrScene* s) {
    const LiveGeometry& live = s->live;
    // (while morphs are set, the rest pose of the pose and skin kernels is what the morph kernel wrote)
    const auto rest = [&](int k) { return !live.arrays[k].kept ? nullptr : live.morph.set() && k < 3 ? (const float*)live.morph.rest[k].ptr : (const float*)live.arrays[k].rest.ptr; };
    const auto staging = [&](int k) { return (float*)live.arrays[k].staging.ptr; };
    devpose::Ctx c{};
    c.rest_positions = rest(POSITIONS), c.rest_normals = rest(NORMALS), c.rest_frames = rest(FRAMES), c.rest_spheres = rest(SPHERES);
    c.positions = staging(POSITIONS), c.normals = staging(NORMALS), c.frames = staging(FRAMES), c.spheres = staging(SPHERES);
    c.objects = (const devpose::DevObject*)live.pose_objects.ptr, c.num_objects = (uint32_t)live.pose_table.size();
    c.num_triangles = live.num_triangles, c.num_spheres = live.num_spheres;
    c.posed_triangles = live.posed_triangles, c.posed_spheres = live.posed_spheres;
    c.beyond_range = (uint32_t*)live.pose_flag.ptr;
    c.lamps = (DevLamp*)s->lamps.ptr, c.num_lamps = (uint32_t)live.lamps.size();
    // (each skin kernel is launched only where a skin of its kind exists: the table of the other one is null)
    c.skins = live.skin.any(PYR_SKIN_LINEAR) ? (const devpose::DevSkin*)live.skin.records.ptr : nullptr, c.num_skins = (uint32_t)live.skin.table.size();
    c.dual_skins = live.skin.any(PYR_SKIN_DUAL_QUATERNION) ? (const devpose::DevSkin*)live.skin.dual_records.ptr : nullptr;
    c.joint_quats = (const float*)live.skin.quats.ptr;
    c.skinned_triangles = live.skin.triangles, c.num_joints = (uint32_t)(live.skin.joints.size() / 16);
    c.joints = (const float*)live.skin.rows.ptr;
    c.skin_weights = (const float*)live.skin.weights.ptr, c.skin_joints = (const uint16_t*)live.skin.indices.ptr;
    return c;
}

devpose::MorphCtx morph_context(PyrScene* s, uint32_t num_active) {
    const LiveGeometry& live = s->live;
    devpose::MorphCtx c{};
    c.rest_positions = (const float*)live.arrays[POSITIONS].rest.ptr, c.rest_normals = (const float*)live.arrays[NORMALS].rest.ptr;
    c.rest_frames = live.arrays[FRAMES].kept ? (const float*)live.arrays[FRAMES].rest.ptr : nullptr;
    c.positions = (float*)live.morph.rest[POSITIONS].ptr, c.normals = (float*)live.morph.rest[NORMALS].ptr;
    c.frames = live.arrays[FRAMES].kept ? (float*)live.morph.rest[FRAMES].ptr : nullptr;
    c.morphs = (const devpose::DevMorph*)live.morph.records.ptr, c.active = (const devpose::ActiveTarget*)live.morph.active.ptr;
    c.position_deltas = (const float*)live.morph.positions.ptr, c.normal_deltas = (const float*)live.morph.normals.ptr;
    c.position_rows = live.morph.position_rows, c.normal_rows = live.morph.normal_rows;
    c.num_morphs = (uint32_t)live.morph.table.size(), c.num_active = num_active;
    c.num_triangles = live.num_triangles, c.morphed_triangles = live.morph.triangles;
    c.flag = (uint32_t*)live.pose_flag.ptr;
    return c;
}

devpose::SmoothCtx smooth_context(PyrScene* s) {
    const LiveGeometry& live = s->live;
    devpose::SmoothCtx c{};
    c.positions = (const float*)live.arrays[POSITIONS].staging.ptr, c.normals = (float*)live.arrays[NORMALS].staging.ptr;
    c.frames = live.arrays[FRAMES].kept ? (float*)live.arrays[FRAMES].staging.ptr : nullptr;
    c.group_begin = (const uint32_t*)live.smooth.begin.ptr, c.group_corners = (const uint32_t*)live.smooth.corner_table.ptr;
    c.num_groups = live.smooth.groups, c.num_corners = live.smooth.corners;
    c.num_triangles = live.num_triangles;
    c.flag = (uint32_t*)live.pose_flag.ptr;
    return c;
}

// Every object's primitives from the rest pose into the staging arrays under `table` and, where the scene has skins, under
// `joints` ([joints][16]), and the flag back: the one wait. Where the scene has morphs, their triangles go from the rest pose into
// the morphed rest under `weights` first (the morphs' targets one after the other), and the other kernels start from there. A skinned object's triangles have their lanes in the skin kernel's
// launch, so the table the pose kernels read gives that object none. Where the scene has a smoothing, the normals and frames of
// its objects are recomputed from the staged positions last.
int run_pose(PyrScene* s, const std::vector<devpose::DevObject>& table, const std::vector<float>& joints, const std::vector<float>& weights, hipStream_t stream,
             uint32_t& flag) {
    const LiveGeometry& live = s->live;
    std::vector<devpose::DevMorph> morphs(live.morph.table.size()); // (these two live until the wait below as well)
    std::vector<devpose::ActiveTarget> active;
    for (size_t k = 0; k < morphs.size(); ++k) {
        const LiveGeometry::Morph& from = live.morph.table[k];
        devpose::DevMorph& to = morphs[k];
        to.first_triangle = table[from.object].first_triangle, to.num_triangles = table[from.object].num_triangles, to.lane = from.lane;
        to.num_targets = from.num_targets, to.has_normals = from.has_normals ? 1u : 0u;
        to.first_active = (uint32_t)active.size();
        for (uint32_t t = 0; t < from.num_targets; ++t)
            if (weights[from.first_weight + t] != 0.0f) active.push_back({t, weights[from.first_weight + t]});
        to.num_active = (uint32_t)active.size() - to.first_active;
        to.unused = 0;
        to.position_row = from.position_row, to.normal_row = from.normal_row;
    }
    std::vector<devpose::DevObject> unskinned; // (these three live until the wait below)
    std::vector<devpose::DevSkin> skins(live.skin.table.size());
    std::vector<float> rows(joints.size() / 16 * 12);
    std::vector<devpose::DevSkin> dual_skins; // (and these two, which only a scene with a dual-quaternion skin fills)
    std::vector<float> quats;
    if (live.skin.set()) {
        unskinned = table;
        for (size_t k = 0; k < skins.size(); ++k) {
            const LiveGeometry::Skin& from = live.skin.table[k];
            devpose::DevSkin& to = skins[k];
            to.pose = table[from.object].pose;
            to.first_triangle = table[from.object].first_triangle, to.num_triangles = table[from.object].num_triangles, to.lane = from.lane;
            to.first_joint = from.first_joint, to.num_joints = from.num_joints;
            bool same = true;
            for (size_t j = from.first_joint; j < (size_t)from.first_joint + from.num_joints; ++j)
                for (int e = 0; e < 16; ++e) same = same && joints[16 * j + e] == kIdentity[e];
            to.identity = same ? 1u : 0u;
            unskinned[from.object].num_triangles = 0;
        }
        uint32_t lane = 0;
        for (devpose::DevObject& o : unskinned) o.triangle_lane = lane, lane += o.num_triangles;
        for (size_t j = 0; j < rows.size() / 12; ++j)
            for (int col = 0; col < 4; ++col)
                for (int row = 0; row < 3; ++row) rows[12 * j + 3 * col + row] = joints[16 * j + 4 * col + row];
        HIP_TRY(hipMemcpyAsync(live.skin.rows.ptr, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, stream));
        if (live.skin.any(PYR_SKIN_DUAL_QUATERNION)) {
            // Each kernel its own table over the same lanes: a skin of the other kind has no triangles there. The joints of the
            // dual-quaternion skins as unit dual quaternions, eight floats a joint, parallel to `rows`.
            dual_skins = skins;
            quats.assign(joints.size() / 16 * 8, 0.0f);
            for (size_t k = 0; k < skins.size(); ++k) {
                const LiveGeometry::Skin& from = live.skin.table[k];
                if (from.blend != PYR_SKIN_DUAL_QUATERNION) {
                    dual_skins[k].num_triangles = 0;
                    continue;
                }
                skins[k].num_triangles = 0;
                for (size_t j = from.first_joint; j < (size_t)from.first_joint + from.num_joints; ++j) pose::joint_dual_quaternion(&joints[16 * j], &quats[8 * j]);
            }
            HIP_TRY(hipMemcpyAsync(live.skin.dual_records.ptr, dual_skins.data(), dual_skins.size() * sizeof(devpose::DevSkin), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(live.skin.quats.ptr, quats.data(), quats.size() * 4, hipMemcpyHostToDevice, stream));
        }
        HIP_TRY(hipMemcpyAsync(live.skin.records.ptr, skins.data(), skins.size() * sizeof(devpose::DevSkin), hipMemcpyHostToDevice, stream));
    }
    const std::vector<devpose::DevObject>& objects = !live.skin.set() ? table : unskinned;
    HIP_TRY(hipMemcpyAsync(s->live.pose_objects.ptr, objects.data(), objects.size() * sizeof(devpose::DevObject), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(s->live.pose_flag.ptr, 0, 4, stream));
    if (!morphs.empty()) {
        HIP_TRY(hipMemcpyAsync(live.morph.records.ptr, morphs.data(), morphs.size() * sizeof(devpose::DevMorph), hipMemcpyHostToDevice, stream));
        if (!active.empty()) HIP_TRY(hipMemcpyAsync(live.morph.active.ptr, active.data(), active.size() * sizeof(devpose::ActiveTarget), hipMemcpyHostToDevice, stream));
        const hipError_t em = devpose::launch_morph(morph_context(s, (uint32_t)active.size()), stream);
        if (em != hipSuccess) return hip_fail(em, "morph kernel");
    }
    const hipError_t e = devpose::launch_pose(pose_context(s), stream);
    if (e != hipSuccess) return hip_fail(e, "pose kernels");
    if (live.smooth.groups) {
        const hipError_t es = devpose::launch_smooth(smooth_context(s), stream);
        if (es != hipSuccess) return hip_fail(es, "smoothing kernel");
    }
    HIP_TRY(hipMemcpyAsync(&flag, s->live.pose_flag.ptr, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PYR_OK;
}

// pyr_scene_pose, pyr_scene_skin and pyr_scene_morph, after check_frame: a table the frame leaves null stays as the scene has it.
int scene_pose(PyrScene* s, const Frame& f, hipStream_t stream) {
    const auto t_start = Clock::now();
    HIP_TRY(hipSetDevice(s->device));
    LiveGeometry& live = s->live;
    const uint32_t mode = f.mode;
    int rc;
    if (mode == PYR_UPDATE_REFIT && (rc = prepare_refit(s)) != PYR_OK) return rc;
    std::vector<devpose::DevObject> table = live.pose_table;
    if (f.poses)
        for (size_t i = 0; i < table.size(); ++i) set_pose(table[i], f.poses[i].transform, f.poses[i].scale);
    std::vector<float> joints = live.skin.joints;
    if (f.joints) joints.assign(f.joints, f.joints + joints.size());
    std::vector<float> weights = live.morph.weights;
    if (f.weights) weights.assign(f.weights, f.weights + weights.size());
    uint32_t flag = 0;
    if ((rc = run_pose(s, table, joints, weights, stream, flag)) != PYR_OK) return rc;
    const auto refused = [&](int why) { // no record has been touched: the staging arrays go back to the poses, joints and weights the scene is in
        const int back = run_pose(s, live.pose_table, live.skin.joints, live.morph.weights, stream, flag);
        return back != PYR_OK ? back : why;
    };
    const struct { // what each bit of the flag word refuses the frame with; the first one raised decides
        uint32_t bit;
        const char* message;
    } raised[] = {
        {devpose::Flag::kBeyondRange, kCoordinateRangeMessage},
        {devpose::Flag::kMorphedNormal,
         "a morphed normal or the tangent frame rebuilt against it has a squared length outside 1e-30 .. 1e30 and cannot be normalised (pyrite_gpu.h, pyr_scene_morph)"},
        {devpose::Flag::kSmoothedNormal,
         "a recomputed normal or the tangent frame rebuilt against it has a squared length outside 1e-30 .. 1e30 and cannot be normalised (pyrite_gpu.h, pyr_scene_set_smoothing)"},
        {devpose::Flag::kBlendedRotation,
         "a blended joint rotation of a dual-quaternion skin has a squared length outside 1e-30 .. 1e30 and cannot be normalised: the rotations of a vertex's joints cancel (pyrite_gpu.h, pyr_scene_set_skin_blend)"},
    };
    for (const auto& r : raised)
        if (flag & r.bit) return refused(fail(PYR_ERR_UNSUPPORTED, r.message));
    PyrUpdateInfo info{};
    info.mode_used = mode;
    info.area_ratio = 1.0;
    const auto t_posed = Clock::now();

    if (mode == PYR_UPDATE_REBUILD) { // the staging arrays are the geometry now: the description follows them, then a rebuild over it
        const float* const none[NUM_ARRAYS] = {nullptr, nullptr, nullptr, nullptr};
        info.upload_ms = (float)ms_between(t_start, t_posed);
        live.posed();
        if ((rc = fetch_live_geometry(s)) == PYR_OK) rc = rebuild_from(s, none, t_start, info);
        if (rc != PYR_OK) { // (and the description follows them again when it is next read)
            live.posed();
            return refused(rc);
        }
        live.pose_table.swap(table), live.skin.joints.swap(joints), live.morph.weights.swap(weights);
        return PYR_OK;
    }

    // ---- refit: every record and box from the staging arrays, as the host form of pyr_scene_update given all four arrays
    live.pose_table.swap(table), live.skin.joints.swap(joints), live.morph.weights.swap(weights);
    live.posed();
    const float* source[NUM_ARRAYS];
    for (int k = 0; k < NUM_ARRAYS; ++k) source[k] = live.kept_floats(k) ? (const float*)live.arrays[k].staging.ptr : nullptr;
    const hipError_t e = devpose::launch_lamps(pose_context(s), stream);
    if (e != hipSuccess) return hip_fail(e, "pose: lamp records");
    return refit_from(s, source, live.num_triangles != 0, live.num_spheres != 0, false, stream, t_start, &t_posed, info);
}

// What every attachment to an object refuses first -- a skin, a morph, a smoothing: reserved words, the object, an object without
// triangles, two on one object. `name`: the struct; `plural`: what two of them are called.
inline bool reserved_clear(const PyrSmoothing& s) { return s.reserved0 == 0 && std::all_of(std::begin(s.reserved), std::end(s.reserved), [](uint32_t w) { return w == 0; }); }
template <class T>
bool reserved_clear(const T& t) {
    return std::all_of(std::begin(t.reserved), std::end(t.reserved), [](uint32_t w) { return w == 0; });
}
template <class T>
int check_attachments(const LiveGeometry& live, const T* items, uint32_t n, const std::string& name, const char* plural) {
    for (uint32_t k = 0; k < n; ++k)
        if (!reserved_clear(items[k])) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".reserved must be zero");
    for (uint32_t k = 0; k < n; ++k)
        if (items[k].object >= live.pose_table.size()) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".object is not one of the scene's objects");
    for (uint32_t k = 0; k < n; ++k)
        if (live.pose_table[items[k].object].num_triangles == 0) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".object: the object has no triangles");
    std::vector<uint32_t> taken;
    for (uint32_t k = 0; k < n; ++k) taken.push_back(items[k].object);
    std::sort(taken.begin(), taken.end());
    if (std::adjacent_find(taken.begin(), taken.end()) != taken.end()) return fail(PYR_ERR_INVALID_ARGUMENT, name + ".object: two " + plural + " on one object");
    return PYR_OK;
}

// What pyr_scene_set_skins refuses of the skins themselves, in the order pyrite_gpu.h gives.
int check_skins(const LiveGeometry& live, const PyrSkin* skins, uint32_t n) {
    const auto triangles_of = [&](const PyrSkin& s) { return (size_t)live.pose_table[s.object].num_triangles; };
    const int rc = check_attachments(live, skins, n, "PyrSkin", "skins");
    if (rc != PYR_OK) return rc;
    for (uint32_t k = 0; k < n; ++k)
        if (skins[k].num_joints == 0 || skins[k].num_joints > 65536u) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrSkin.num_joints must be 1 to 65,536");
    for (uint32_t k = 0; k < n; ++k) {
        if (!skins[k].joints) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrSkin.joints is null");
        if (!skins[k].weights) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrSkin.weights is null");
    }
    for (uint32_t k = 0; k < n; ++k)
        for (size_t i = 0, end = 12 * triangles_of(skins[k]); i < end; ++i)
            if (skins[k].joints[i] >= skins[k].num_joints) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrSkin.joints names a joint index that is not below num_joints");
    for (uint32_t k = 0; k < n; ++k)
        for (size_t i = 0, end = 12 * triangles_of(skins[k]); i < end; ++i)
            if (!std::isfinite(skins[k].weights[i]) || skins[k].weights[i] < 0.0f) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrSkin.weights has a weight that is not finite or is negative");
    for (uint32_t k = 0; k < n; ++k)
        for (size_t i = 0, end = 12 * triangles_of(skins[k]); i < end; i += 4) {
            const float* w = skins[k].weights + i;
            const float sum = ((w[0] + w[1]) + w[2]) + w[3];
            if (!(std::fabs(sum - 1.0f) <= 1.0e-3f)) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrSkin.weights: a vertex's weights do not sum to 1 within 1e-3");
        }
    return PYR_OK;
}

// What pyr_scene_set_morphs refuses of the morphs themselves, in the order pyrite_gpu.h gives.
int check_morphs(const LiveGeometry& live, const PyrMorph* morphs, uint32_t n) {
    const int rc = check_attachments(live, morphs, n, "PyrMorph", "morphs");
    if (rc != PYR_OK) return rc;
    for (uint32_t k = 0; k < n; ++k)
        if (morphs[k].num_targets == 0 || morphs[k].num_targets > 256u) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrMorph.num_targets must be 1 to 256");
    for (uint32_t k = 0; k < n; ++k)
        if (!morphs[k].position_deltas) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrMorph.position_deltas is null");
    for (uint32_t k = 0; k < n; ++k) {
        const size_t words = 9 * (size_t)live.pose_table[morphs[k].object].num_triangles * morphs[k].num_targets;
        for (const float* deltas : {morphs[k].position_deltas, morphs[k].normal_deltas})
            for (size_t i = 0; deltas && i < words; ++i)
                if (!std::isfinite(deltas[i])) return fail(PYR_ERR_INVALID_ARGUMENT, deltas == morphs[k].position_deltas ? "PyrMorph.position_deltas has a delta that is not finite" : "PyrMorph.normal_deltas has a delta that is not finite");
    }
    return PYR_OK;
}

// What pyr_scene_set_smoothing refuses of the smoothings themselves, in the order pyrite_gpu.h gives.
int check_smoothings(const LiveGeometry& live, const PyrSmoothing* smoothings, uint32_t n) {
    const int rc = check_attachments(live, smoothings, n, "PyrSmoothing", "smoothings");
    if (rc != PYR_OK) return rc;
    for (uint32_t k = 0; k < n; ++k)
        if (!smoothings[k].vertex_ids) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrSmoothing.vertex_ids is null");
    return PYR_OK;
}

// pyr_scene_set_skins, once it has skins to set: the bindings one skin after the other.
int install_skins(LiveGeometry& live, const PyrSkin* skins, uint32_t num_skins) {
    int rc;
    // the bindings one skin after the other, on the device before anything of the old skins is let go
    std::vector<LiveGeometry::Skin> table(num_skins);
    std::vector<float> weights;
    std::vector<uint16_t> indices;
    uint32_t lane = 0, joint = 0;
    for (uint32_t k = 0; k < num_skins; ++k) {
        const size_t words = 12 * (size_t)live.pose_table[skins[k].object].num_triangles;
        table[k] = {skins[k].object, skins[k].num_joints, joint, lane};
        weights.insert(weights.end(), skins[k].weights, skins[k].weights + words);
        indices.insert(indices.end(), skins[k].joints, skins[k].joints + words);
        lane += live.pose_table[skins[k].object].num_triangles, joint += skins[k].num_joints; // disjoint ranges: below 2^28; at most 2^16 a skin
    }
    LiveGeometry::Skins fresh;
    if ((rc = fresh.weights.upload(weights.data(), weights.size() * 4)) != PYR_OK) return rc;
    if ((rc = fresh.indices.upload(indices.data(), indices.size() * 2)) != PYR_OK) return rc;
    if ((rc = fresh.records.alloc((size_t)num_skins * sizeof(devpose::DevSkin))) != PYR_OK) return rc;
    if ((rc = fresh.rows.alloc((size_t)joint * 48)) != PYR_OK) return rc;
    fresh.table.swap(table);
    for (uint32_t j = 0; j < joint; ++j) fresh.joints.insert(fresh.joints.end(), kIdentity, kIdentity + 16);
    fresh.triangles = lane;
    live.skin.swap(fresh);
    live.recount_lanes();
    return PYR_OK;
}

// pyr_scene_set_morphs, once it has morphs to set: the deltas one morph after the other, and the morphed rest as a copy of rest.
int install_morphs(LiveGeometry& live, const PyrMorph* morphs, uint32_t num_morphs) {
    int rc;
    // the deltas one morph after the other, on the device before anything of the old morphs is let go
    std::vector<LiveGeometry::Morph> table(num_morphs);
    std::vector<float> positions, normals;
    uint32_t lane = 0, weight = 0;
    for (uint32_t k = 0; k < num_morphs; ++k) {
        const uint32_t triangles = live.pose_table[morphs[k].object].num_triangles;
        const size_t words = 9 * (size_t)triangles * morphs[k].num_targets;
        table[k] = {morphs[k].object, morphs[k].num_targets, weight, lane, positions.size() / 9, normals.size() / 9, morphs[k].normal_deltas != nullptr};
        positions.insert(positions.end(), morphs[k].position_deltas, morphs[k].position_deltas + words);
        if (morphs[k].normal_deltas) normals.insert(normals.end(), morphs[k].normal_deltas, morphs[k].normal_deltas + words);
        lane += triangles, weight += morphs[k].num_targets; // disjoint ranges: below 2^28; at most 256 a morph
    }
    LiveGeometry::Morphs fresh;
    if ((rc = fresh.positions.upload(positions.data(), positions.size() * 4)) != PYR_OK) return rc;
    if (!normals.empty() && (rc = fresh.normals.upload(normals.data(), normals.size() * 4)) != PYR_OK) return rc;
    if ((rc = fresh.records.alloc((size_t)num_morphs * sizeof(devpose::DevMorph))) != PYR_OK) return rc;
    if ((rc = fresh.active.alloc((size_t)weight * sizeof(devpose::ActiveTarget))) != PYR_OK) return rc;
    for (int k = 0; k < 3; ++k) {
        const size_t bytes = live.kept_floats(k) * 4;
        if (!bytes) continue;
        if ((rc = fresh.rest[k].alloc(bytes)) != PYR_OK) return rc;
        HIP_TRY(hipMemcpy(fresh.rest[k].ptr, live.arrays[k].rest.ptr, bytes, hipMemcpyDeviceToDevice));
    }
    fresh.table.swap(table);
    fresh.weights.assign(weight, 0.0f);
    fresh.triangles = lane;
    fresh.position_rows = positions.size() / 9, fresh.normal_rows = normals.size() / 9;
    live.morph.swap(fresh);
    return PYR_OK;
}

// pyr_scene_set_smoothing, once it has smoothings to set: the groups of corners as a CSR.
int install_smoothings(LiveGeometry& live, const PyrSmoothing* smoothings, uint32_t num_smoothings) {
    int rc;
    // the groups one smoothing after the other: a group's number is its rank by first corner within its object, so neighbouring
    // lanes touch neighbouring triangles whatever the caller's labels are; rows are filled in ascending corner order
    std::vector<uint32_t> objects, begin(1, 0u), corners;
    std::vector<float> rest_p, rest_n;
    for (uint32_t k = 0; k < num_smoothings; ++k) {
        const devpose::DevObject& o = live.pose_table[smoothings[k].object];
        const size_t words = 9 * (size_t)o.num_triangles, count = 3 * (size_t)o.num_triangles;
        rest_p.resize(words), rest_n.resize(words); // the orientation is the rest pose's: the device copy taken when objects were named
        HIP_TRY(hipMemcpy(rest_p.data(), (const float*)live.arrays[POSITIONS].rest.ptr + 9 * (size_t)o.first_triangle, words * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(rest_n.data(), (const float*)live.arrays[NORMALS].rest.ptr + 9 * (size_t)o.first_triangle, words * 4, hipMemcpyDeviceToHost));
        const uint32_t* ids = smoothings[k].vertex_ids;
        std::unordered_map<uint32_t, uint32_t> group_of; // label -> group within this object, numbered by first appearance
        std::vector<uint32_t> group(count), size;
        for (size_t i = 0; i < count; ++i) {
            const auto found = group_of.emplace(ids[i], (uint32_t)size.size());
            if (found.second) size.push_back(0u);
            group[i] = found.first->second, ++size[group[i]];
        }
        std::vector<uint32_t> fill(size.size());
        for (size_t g = 0; g < size.size(); ++g) fill[g] = begin.back(), begin.push_back(begin.back() + size[g]);
        corners.resize(begin.back());
        for (size_t i = 0; i < count; ++i) {
            const size_t t = i / 3;
            const bool negated = pose::face_negated(&rest_p[9 * t], &rest_n[9 * t]);
            corners[fill[group[i]]++] = (3u * o.first_triangle + (uint32_t)i) | (negated ? devpose::kNegated : 0u); // below 3 * 2^28
        }
        objects.push_back(smoothings[k].object);
    }
    LiveGeometry::Smooth fresh; // on the device before anything of the old smoothing is let go
    if ((rc = fresh.begin.upload(begin.data(), begin.size() * 4)) != PYR_OK) return rc;
    if ((rc = fresh.corner_table.upload(corners.data(), corners.size() * 4)) != PYR_OK) return rc;
    fresh.objects.swap(objects);
    fresh.groups = (uint32_t)begin.size() - 1u, fresh.corners = (uint32_t)corners.size();
    live.smooth.swap(fresh);
    return PYR_OK;
}

// The skeleton of pyr_scene_set_skins, pyr_scene_set_morphs and pyr_scene_set_smoothing: what all three refuse, `check` for the
// attachments themselves, nothing to do where none are set and none are given, the wait (an earlier call's kernels may still read
// what is about to go), then `forget` for none or `install` for new ones -- which has everything on the device before it lets
// anything of the old ones go. `plural`: the argument's name; `entry`: the entry point's.
template <class T, class State, class Check, class Install>
int set_attachments(PyrScene* scene, const T* items, uint32_t n, const std::string& plural, const char* entry, State LiveGeometry::*state, void (LiveGeometry::*forget)(), Check check,
                    Install install) {
    if (n != 0 && !items) return fail(PYR_ERR_INVALID_ARGUMENT, "null " + plural + " with a non-zero num_" + plural);
    if (!scene) return fail(PYR_ERR_INVALID_ARGUMENT, "null scene");
    LiveGeometry& live = scene->live;
    if (live.pose_table.empty()) return fail(PYR_ERR_INVALID_ARGUMENT, std::string(entry) + ": the scene has no objects (pyr_scene_set_objects names them)");
    const int rc = check(live, items, n);
    if (rc != PYR_OK) return rc;
    if (n == 0 && !(live.*state).set()) return PYR_OK;
    HIP_TRY(hipSetDevice(scene->device));
    HIP_TRY(hipDeviceSynchronize());
    if (n == 0) {
        (live.*forget)();
        return PYR_OK;
    }
    return install(live, items, n);
}

// ranges inside the counts and pairwise disjoint, triangles and spheres each
int check_ranges(const PyrScene* scene, const PyrObjectRange* ranges, uint32_t n) {
    std::vector<std::pair<uint64_t, uint64_t>> tri, sph;
    for (uint32_t i = 0; i < n; ++i) {
        const PyrObjectRange& r = ranges[i];
        if ((uint64_t)r.first_triangle + r.num_triangles > scene->live.num_triangles) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrObjectRange: a triangle range reaches past the scene's triangles");
        if ((uint64_t)r.first_sphere + r.num_spheres > scene->live.num_spheres) return fail(PYR_ERR_INVALID_ARGUMENT, "PyrObjectRange: a sphere range reaches past the scene's spheres");
        if (r.num_triangles) tri.emplace_back(r.first_triangle, (uint64_t)r.first_triangle + r.num_triangles);
        if (r.num_spheres) sph.emplace_back(r.first_sphere, (uint64_t)r.first_sphere + r.num_spheres);
    }
    for (auto* list : {&tri, &sph}) {
        std::sort(list->begin(), list->end());
        for (size_t k = 1; k < list->size(); ++k)
            if ((*list)[k].first < (*list)[k - 1].second) return fail(PYR_ERR_INVALID_ARGUMENT, list == &tri ? "PyrObjectRange: two triangle ranges overlap" : "PyrObjectRange: two sphere ranges overlap");
    }
    return PYR_OK;
}

} // namespace

extern "C" {

int pyr_scene_set_objects(PyrScene* scene, const PyrObjectRange* ranges, uint32_t num_objects) {
    if (num_objects != 0 && !ranges) return fail(PYR_ERR_INVALID_ARGUMENT, "null ranges with a non-zero num_objects");
    if (!scene) return fail(PYR_ERR_INVALID_ARGUMENT, "null scene");
    int rc = check_ranges(scene, ranges, num_objects);
    if (rc != PYR_OK) return rc;
    LiveGeometry& live = scene->live;
    if (num_objects == 0 && live.pose_table.empty()) return PYR_OK;
    HIP_TRY(hipSetDevice(scene->device));
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = fetch_live_geometry(scene)) != PYR_OK) return rc; // the rest pose is the geometry as it is now
    live.forget_objects();
    if (num_objects == 0) return PYR_OK;
    for (int k = 0; k < NUM_ARRAYS; ++k) { // the rest pose, and a staging array that holds a copy of it
        LiveArray& a = live.arrays[k];
        const size_t bytes = live.kept_floats(k) * 4;
        if ((rc = a.rest.upload(a.host.data(), bytes)) != PYR_OK) return rc;
        if ((rc = a.staging.reserve(bytes)) != PYR_OK) return rc;
        if (bytes) HIP_TRY(hipMemcpy(a.staging.ptr, a.rest.ptr, bytes, hipMemcpyDeviceToDevice));
    }
    live.staged_positions();
    if ((rc = live.pose_objects.alloc((size_t)num_objects * sizeof(devpose::DevObject))) != PYR_OK) return rc;
    if (!live.pose_flag.ptr && (rc = live.pose_flag.alloc(4)) != PYR_OK) return rc;
    live.pose_table.resize(num_objects);
    uint32_t triangle_lane = 0, sphere_lane = 0;
    for (uint32_t i = 0; i < num_objects; ++i) {
        devpose::DevObject& o = live.pose_table[i];
        set_pose(o, kIdentity, 1.0f);
        o.first_triangle = ranges[i].first_triangle, o.num_triangles = ranges[i].num_triangles;
        o.first_sphere = ranges[i].first_sphere, o.num_spheres = ranges[i].num_spheres;
        o.triangle_lane = triangle_lane, o.sphere_lane = sphere_lane;
        triangle_lane += o.num_triangles, sphere_lane += o.num_spheres; // disjoint ranges inside the counts: below 2^28 in all
    }
    live.recount_lanes();
    return PYR_OK;
}

int pyr_scene_pose(PyrScene* scene, const PyrPoseUpdate* update, void* hip_stream) {
    Frame f;
    if (update) f.mode = update->mode, f.poses = update->poses, f.num_objects = update->num_objects;
    const int rc = check_frame(scene, update, f, kPoseFrame);
    return rc != PYR_OK ? rc : scene_pose(scene, f, (hipStream_t)hip_stream);
}

int pyr_scene_set_skins(PyrScene* scene, const PyrSkin* skins, uint32_t num_skins) {
    return set_attachments(scene, skins, num_skins, "skins", "pyr_scene_set_skins", &LiveGeometry::skin, &LiveGeometry::forget_skins, check_skins, install_skins);
}

int pyr_scene_set_skin_blend(PyrScene* scene, const uint32_t* modes, uint32_t num_skins) {
    if (!modes) return fail(PYR_ERR_INVALID_ARGUMENT, "null modes");
    if (!scene) return fail(PYR_ERR_INVALID_ARGUMENT, "null scene");
    LiveGeometry::Skins& skin = scene->live.skin;
    if (!skin.set()) return fail(PYR_ERR_INVALID_ARGUMENT, "pyr_scene_set_skin_blend: the scene has no skins (pyr_scene_set_skins binds them)");
    if (num_skins != skin.table.size()) return fail(PYR_ERR_INVALID_ARGUMENT, "pyr_scene_set_skin_blend: num_skins is not the scene's");
    bool dual = false;
    for (uint32_t k = 0; k < num_skins; ++k) {
        if (modes[k] != PYR_SKIN_LINEAR && modes[k] != PYR_SKIN_DUAL_QUATERNION) return fail(PYR_ERR_INVALID_ARGUMENT, "pyr_scene_set_skin_blend: a mode is neither PYR_SKIN_LINEAR nor PYR_SKIN_DUAL_QUATERNION");
        dual = dual || modes[k] == PYR_SKIN_DUAL_QUATERNION;
    }
    HIP_TRY(hipSetDevice(scene->device));
    HIP_TRY(hipDeviceSynchronize()); // an earlier call's kernels may still read the tables that go
    DeviceBuffer records, quats; // on the device before anything of the scene changes; a scene without such a skin holds neither
    int rc;
    if (dual && (rc = records.alloc(skin.table.size() * sizeof(devpose::DevSkin))) != PYR_OK) return rc;
    if (dual && (rc = quats.alloc(skin.joints.size() / 16 * 32)) != PYR_OK) return rc;
    skin.dual_records.swap(records), skin.quats.swap(quats);
    for (uint32_t k = 0; k < num_skins; ++k) skin.table[k].blend = modes[k];
    for (size_t j = 0; j < skin.joints.size(); j += 16) std::copy(kIdentity, kIdentity + 16, skin.joints.begin() + j);
    return PYR_OK;
}

int pyr_scene_skin(PyrScene* scene, const PyrSkinUpdate* update, void* hip_stream) {
    Frame f;
    if (update) f.mode = update->mode, f.poses = update->poses, f.num_objects = update->num_objects, f.joints = update->joints, f.num_joints = update->num_joints;
    const int rc = check_frame(scene, update, f, kSkinFrame);
    return rc != PYR_OK ? rc : scene_pose(scene, f, (hipStream_t)hip_stream);
}

int pyr_scene_set_morphs(PyrScene* scene, const PyrMorph* morphs, uint32_t num_morphs) {
    return set_attachments(scene, morphs, num_morphs, "morphs", "pyr_scene_set_morphs", &LiveGeometry::morph, &LiveGeometry::forget_morphs, check_morphs, install_morphs);
}

int pyr_scene_morph(PyrScene* scene, const PyrMorphUpdate* update, void* hip_stream) {
    Frame f;
    if (update)
        f.mode = update->mode, f.poses = update->poses, f.num_objects = update->num_objects, f.joints = update->joints, f.num_joints = update->num_joints, f.weights = update->weights,
        f.num_weights = update->num_weights;
    const int rc = check_frame(scene, update, f, kMorphFrame);
    return rc != PYR_OK ? rc : scene_pose(scene, f, (hipStream_t)hip_stream);
}

int pyr_scene_set_smoothing(PyrScene* scene, const PyrSmoothing* smoothings, uint32_t num_smoothings) {
    return set_attachments(scene, smoothings, num_smoothings, "smoothings", "pyr_scene_set_smoothing", &LiveGeometry::smooth, &LiveGeometry::forget_smoothing, check_smoothings, install_smoothings);
}

int pyr_scene_geometry(PyrScene* scene, float* tri_positions, float* tri_normals, float* tri_frames, float* spheres) {
    if (!scene) return fail(PYR_ERR_INVALID_ARGUMENT, "null scene");
    const LiveGeometry& live = scene->live;
    if (tri_frames && !live.arrays[FRAMES].kept) return fail(PYR_ERR_INVALID_ARGUMENT, "tri_frames: the scene was created without frames and keeps none");
    int rc = fetch_live_geometry(scene);
    if (rc != PYR_OK) return rc;
    float* const out[NUM_ARRAYS] = {tri_positions, tri_normals, tri_frames, spheres};
    for (int k = 0; k < NUM_ARRAYS; ++k)
        if (out[k] && live.kept_floats(k)) std::memcpy(out[k], live.arrays[k].host.data(), live.kept_floats(k) * 4);
    return PYR_OK;
}

int pyr_scene_keep_previous(PyrScene* scene, int keep) {
    if (!scene) return fail(PYR_ERR_INVALID_ARGUMENT, "null scene");
    LiveGeometry& live = scene->live;
    HIP_TRY(hipSetDevice(scene->device));
    HIP_TRY(hipDeviceSynchronize()); // blocking: a motion pass in flight may read the old snapshot, a pose may still write the staging arrays
    if (!keep) {
        live.previous_positions.release(), live.previous_spheres.release();
        live.previous_kept = false;
        return PYR_OK;
    }
    // Positions and spheres are always kept. After a refit pose the staging arrays hold both in full and are the truth; otherwise
    // the description is, and the staging arrays may hold an older update or nothing.
    const std::pair<int, DeviceBuffer*> pairs[2] = {{POSITIONS, &live.previous_positions}, {SPHERES, &live.previous_spheres}};
    live.previous_kept = false; // (a copy that fails leaves no snapshot, not half of one)
    for (const auto& [k, to] : pairs) {
        const size_t bytes = live.floats(k) * 4;
        int rc;
        if (live.host_current()) {
            if ((rc = to->upload(live.arrays[k].host.data(), bytes)) != PYR_OK) return rc;
        } else {
            if ((rc = to->reserve(bytes)) != PYR_OK) return rc;
            if (bytes) HIP_TRY(hipMemcpy(to->ptr, live.arrays[k].staging.ptr, bytes, hipMemcpyDeviceToDevice));
        }
    }
    live.previous_kept = true;
    return PYR_OK;
}

int pyr_scene_update(PyrScene* scene, const PyrGeometryUpdate* update) {
    int rc = check_update_args(scene, update);
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(scene->device));
    HIP_TRY(hipDeviceSynchronize()); // blocking: nothing of this scene is in flight while its records change
    return scene_update(scene, update, false, nullptr);
}

int pyr_scene_update_device(PyrScene* scene, const PyrGeometryUpdate* update, void* hip_stream) {
    int rc = check_update_args(scene, update);
    if (rc != PYR_OK) return rc;
    return scene_update(scene, update, true, (hipStream_t)hip_stream);
}

int pyr_scene_update_info(PyrScene* scene, PyrUpdateInfo* out) {
    if (!scene || !out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(scene->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<Node64> nodes(scene->info.num_nodes);
    HIP_TRY(hipMemcpy(nodes.data(), scene->nodes.ptr, nodes.size() * sizeof(Node64), hipMemcpyDeviceToHost));
    const double now = child_area_sum(nodes.data(), nodes.size());
    if (!scene->live.area_known()) scene->live.area_at_build(now); // no refit since the build: this is the built tree
    *out = scene->live.update_info;
    out->area_ratio = scene->live.built_area > 0.0 ? now / scene->live.built_area : 1.0;
    return PYR_OK;
}

} // extern "C"
