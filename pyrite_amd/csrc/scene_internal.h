// scene_internal.h -- what scene_create.cpp (creation), api.cpp (renders, feature passes), live_scene.cpp (everything that moves
// a scene after creation) and session.cpp (progressive sessions) all see of a PyrScene. Declarations only; what packs a scene
// on the host -- pack_lamp and the coordinate test among it -- comes with scene_pack.h.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "api_internal.h"
#include "kernels/pose_launch.h"
#include "scene_pack.h"

namespace pyr {

// The geometry part of scene creation, once more over a scene that exists (scene_create.cpp): `d` needs its geometry fields and lamps.
int pack_geometry(const PyrSceneDesc* d, PyrScene* s, uint32_t builder);

// The render side, for the units that enqueue renders and feature passes of a scene (api.cpp defines it, session.cpp calls it).
struct TilePlan {
    uint32_t tiles_x = 0, tiles_y = 0;
    uint32_t tile_begin = 0, tile_stride = 1, tile_count = 0;
    uint32_t chunks_per_tile = 0;
    uint32_t chunk_begin = 0, chunk_end = 0; // chunk numbers of the call's tiles (device_scene.h RenderLaunch)
};
int plan_tiles(const PyrFilmDesc* film, const PyrRenderParams* p, TilePlan& plan);
int check_render_args(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrRenderParams* p, const void* film_ptr);
RenderLaunch make_launch(const PyrCamera* camera, const PyrFilmDesc* film, const PyrRenderParams* p, const TilePlan& plan);
int render_batches(PyrScene* scene, RenderLaunch L, bool count, hipStream_t stream); // picks the schedule, reserves the tape, launches
int check_tape_overflow(PyrScene* scene); // after a render has been waited for: PYR_ERR_DEVICE if a path outgrew the spectral tape
// What the feature entries refuse before a device is looked for (`what` names the scene or session argument), and the pass
// enqueued on `stream`: the buffers are on the scene's device, either may be null.
int check_feature_args(const void* owner, const char* what, const PyrCamera* camera, bool need_camera, const PyrFilmDesc* film, const PyrFeatureParams* fp,
                       const void* albedo, const void* pixels);
int enqueue_features(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrFeatureParams* fp, PyrGrain* albedo, PyrFeaturePixel* pixels,
                     hipStream_t stream);
// The same for the motion entries: the checks (previous_w receives pyr_camera_world_to_cam of the previous camera), and the pass
// enqueued on `stream` with `pixels` on the scene's device.
int check_motion_args(const void* owner, const char* what, const PyrCamera* camera, bool need_camera, const PyrCamera* previous_camera, const PyrFilmDesc* film,
                      const void* pixels, float previous_w[16]);
int enqueue_motion(PyrScene* scene, const PyrCamera* camera, const PyrCamera* previous_camera, const float previous_w[16], const PyrFilmDesc* film,
                   PyrMotionPixel* pixels, hipStream_t stream);

struct LiveArray {       // one of the arrays that move, and its homes
    uint32_t width;      // floats per primitive
    bool per_sphere;     // scales with num_spheres, not num_triangles
    bool kept = true;    // the scene keeps it (frames: only a description that has them, or an update that brought them)
    std::vector<float> host;
    DeviceBuffer staging, rest;
};

// Where a scene's geometry is now, and which of its copies are valid (live_scene.cpp). Four arrays move -- positions, normals,
// frames, spheres -- and each has up to three homes in the scene: `host`, the description a rebuild packs from and a refit's
// lamp records need; `staging`, the device array a host update uploads into, the pose and skin kernels write and the refit reads; `rest`,
// the device copy taken when objects were named, which every pose starts from. What never moves (uvs, materials, the lamp
// list) are plain members.
//
// What holds between the copies, and the only methods that change it:
//  - host_current: `host` is the geometry the records on the device were made from. Only a refit pose leaves it behind
//    (posed()): the staging arrays are the truth then, and whoever reads `host` calls fetch_live_geometry first (fetched()).
//  - positions_staged: staging positions equal host positions, so a refit that moves no triangle reads them without an upload.
//    True after they were uploaded or captured from `host` (staged_positions(), adopted() of host arrays); false after
//    device arrays were adopted and after every build (built(): conservative, costs one upload at most).
//  - schedule_current: the refit schedules and scratch belong to the trees on the device (scheduled(); built() ends it).
//  - area_known: built_area is the binary tree's child_area_sum at the last build (area_at_build(); built() ends it).
//  - While host_current is false, objects are set and every kept array's staging buffer holds the whole array.
struct LiveGeometry {
    enum { POSITIONS, NORMALS, FRAMES, SPHERES, NUM_ARRAYS };
    LiveArray arrays[NUM_ARRAYS] = {{9, false}, {9, false}, {12, false}, {4, true}}; // the one table of what moves
    uint32_t num_triangles = 0, num_spheres = 0;
    std::vector<float> tri_uvs, sphere_tex_scale;
    std::vector<uint32_t> tri_material, sphere_material;
    std::vector<PyrLamp> lamps;
    bool has_uvs = false, has_tex_scale = false;
    // the refit's scratch and its schedules (made at the first refit after a build): RefitSchedule::order and ::begin of either tree
    DeviceBuffer bounds, max_abs, order_binary, order_wide;
    std::vector<uint32_t> sched_binary, sched_wide;
    std::vector<DevLamp> lamp_records; // of the last host update (the copy to the device may still read them)
    double built_area = 0.0;
    PyrUpdateInfo update_info{};
    // the objects with the poses the scene is in (identity when they are set)
    std::vector<devpose::DevObject> pose_table;
    uint32_t posed_triangles = 0, posed_spheres = 0;
    DeviceBuffer pose_objects, pose_flag;
    // the skins in skin order (pyr_scene_set_skins): whose triangles, which rows of the joint table, where the lanes and bindings
    // begin, and how its joints are blended (PYR_SKIN_*: linear when the skins are set, pyr_scene_set_skin_blend says otherwise); and
    // the joint matrices the scene is in, [joints][16] (identity when the skins are set). `dual_records` and `quats` exist only
    // while some skin is dual-quaternion.
    struct Skin {
        uint32_t object, num_joints, first_joint, lane, blend;
    };
    struct Skins {
        std::vector<Skin> table;
        std::vector<float> joints;
        uint32_t triangles = 0;                         // lanes of the skin kernels
        DeviceBuffer records, weights, indices, rows;   // DevSkin records, the two binding arrays, twelve floats a joint
        DeviceBuffer dual_records, quats;               // the dual-quaternion kernel's DevSkin records, eight floats a joint
        bool set() const { return !table.empty(); }
        bool any(uint32_t blend) const {
            for (const Skin& s : table)
                if (s.blend == blend) return true;
            return false;
        }
        void clear() {
            table.clear(), joints.clear();
            triangles = 0;
            for (DeviceBuffer* b : {&records, &weights, &indices, &rows, &dual_records, &quats}) b->release();
        }
        void swap(Skins& o) {
            table.swap(o.table), joints.swap(o.joints), std::swap(triangles, o.triangles);
            records.swap(o.records), weights.swap(o.weights), indices.swap(o.indices), rows.swap(o.rows);
            dual_records.swap(o.dual_records), quats.swap(o.quats);
        }
    } skin;
    // the morphs in morph order (pyr_scene_set_morphs): whose triangles, how many targets, where its weights begin in the weight
    // table, its lanes in the morph kernel's launch and its targets in the two delta buffers (rows of nine floats); and the weights
    // the scene is in, the morphs' targets one after the other (zero when the morphs are set). `rest`: positions, normals and
    // frames after the morph, which the pose and skin kernels read as their rest pose while morphs are set.
    struct Morph {
        uint32_t object, num_targets, first_weight, lane;
        uint64_t position_row, normal_row;
        bool has_normals;
    };
    struct Morphs {
        std::vector<Morph> table;
        std::vector<float> weights;
        uint32_t triangles = 0; // lanes of the morph kernel
        uint64_t position_rows = 0, normal_rows = 0;
        DeviceBuffer records, active, positions, normals; // DevMorph records, a frame's pairs, the deltas as uploaded
        DeviceBuffer rest[3];
        bool set() const { return !table.empty(); }
        void clear() {
            table.clear(), weights.clear();
            triangles = 0;
            position_rows = normal_rows = 0;
            for (DeviceBuffer* b : {&records, &active, &positions, &normals, &rest[0], &rest[1], &rest[2]}) b->release();
        }
        void swap(Morphs& o) {
            table.swap(o.table), weights.swap(o.weights), std::swap(triangles, o.triangles);
            std::swap(position_rows, o.position_rows), std::swap(normal_rows, o.normal_rows);
            records.swap(o.records), active.swap(o.active), positions.swap(o.positions), normals.swap(o.normals);
            for (int k = 0; k < 3; ++k) rest[k].swap(o.rest[k]);
        }
    } morph;
    // the smoothing (pyr_scene_set_smoothing): which objects have their normals recomputed, and the groups of their corners as a
    // CSR on the device -- begin [groups + 1], corner_table [corners], a corner being 3 * triangle + vertex over the scene's
    // triangles with devpose::kNegated set where the triangle's face vector is negated
    struct Smooth {
        std::vector<uint32_t> objects;
        uint32_t groups = 0, corners = 0;
        DeviceBuffer begin, corner_table;
        bool set() const { return !objects.empty(); }
        void clear() {
            objects.clear();
            groups = corners = 0;
            begin.release(), corner_table.release();
        }
        void swap(Smooth& o) {
            objects.swap(o.objects), std::swap(groups, o.groups), std::swap(corners, o.corners);
            begin.swap(o.begin), corner_table.swap(o.corner_table);
        }
    } smooth;
    // the previous frame (pyr_scene_keep_previous): positions and spheres as they were when it was called, the description's order.
    // Nothing that moves the scene touches them -- counts and indices never change -- and only the motion pass reads them.
    DeviceBuffer previous_positions, previous_spheres;
    bool previous_kept = false;

    size_t floats(int k) const { return (size_t)arrays[k].width * (arrays[k].per_sphere ? num_spheres : num_triangles); } // of array k in full, kept or not
    size_t kept_floats(int k) const { return arrays[k].kept ? floats(k) : 0; }
    void keep(const PyrSceneDesc* d); // scene creation: the description's geometry
    PyrSceneDesc view(const float* const with[NUM_ARRAYS] = nullptr) const; // what pack_geometry and pack_lamp read; `with`: arrays in place of the scene's own
    void forget_objects(); // (adopted() does it: new arrays are a new geometry, not a pose of the old one); forgets the skins, the morphs and the smoothing too
    void forget_skins();
    void forget_morphs();
    void forget_smoothing();
    void recount_lanes(); // the pose kernels' lanes: every object's spheres, and the triangles no skin has taken
    bool host_current() const { return host_current_; }
    bool positions_staged() const { return positions_staged_; }
    bool schedule_current() const { return schedule_current_; }
    bool area_known() const { return area_known_; }
    void built() { host_current_ = true, positions_staged_ = schedule_current_ = area_known_ = false; } // pack_geometry made new trees from `host`
    void adopted(const float* const given[NUM_ARRAYS], bool staged); // `host` takes the arrays an update gave; staged: they are in staging too
    void staged_positions() { positions_staged_ = true; }
    void posed() { host_current_ = false; }
    void fetched() { host_current_ = true; }
    void scheduled() { schedule_current_ = true; }
    void area_at_build(double area) { built_area = area, area_known_ = true; }

private:
    bool host_current_ = true, positions_staged_ = false, schedule_current_ = false, area_known_ = false;
};

} // namespace pyr

struct PyrScene {
    int device = 0;
    int num_cus = 0;
    pyr::DevScene dev{};
    PyrBvhInfo info{};
    PyrBuildInfo build_info{}; // pyr_scene_build_info
    std::unique_ptr<pyr::BuiltBvh> digest_source; // the binary tree, kept until the first pyr_scene_build_info has hashed it (tree_digest walks the whole tree: not on every scene creation's bill)
    pyr::DeviceBuffer wide_nodes, wide_pair_nodes, pair_prims, nodes, prims, tri_shade, spheres, sphere_material, planes, plane_material, lamps, materials, components, programs, instrs, spectra,
        spectrum_data, rgb_basis, counters, tri_tex, sphere_tex_scale, plane_frames, textures, texture_data;
    PyrCounters last_counters{};
    bool have_counters = false;
    PyrProgramInfo program_info{}; // pyr_scene_program_info; program_info.wide: the kernels are the wide interpreter build (kernels/wide.hip)
    uint32_t* tail_count = nullptr; // device, kFeedBytes: the work-feed cursors of the intersect kernel
    pyr::DeviceBuffer tape; // spectral tape of the stage-scheduled kernel (grown on demand, kept between renders)
    pyr::DeviceBuffer start_queue; // the waves' rings of ready sample starts (RenderLaunch::start_queue; scenes without interpreter programs), kept like the tape
    pyr::DeviceBuffer tape_overflow; // one word the kernels set when a path outgrew the tape (checked after blocking renders and by pyr_scene_counters)
    uint32_t builder = PYR_BUILD_HOST; // who builds this scene's trees: at creation, and at every PYR_UPDATE_REBUILD
    bool spatial_splits = false;       // the last build split space: its leaves hold clipped boxes, which a refit cannot recompute
    uint64_t table_floats = 0;         // floats of the small tables a big scene stages into LDS (DevScene::lds_table_floats)
    uint32_t live_sessions = 0;        // PyrSessions on this scene: an update is refused while there is one
    pyr::LiveGeometry live;            // where the geometry is now (pyr_scene_update, pyr_scene_set_objects / pyr_scene_pose)
    ~PyrScene();
};
