// api.cpp -- the render side of the C ABI declared in include/pyrite_gpu.h: tile plans, launches, the tape's reservation, the
// choice of schedule, and the entries that render, intersect or look at a scene. No radiance is ever computed on the host; without
// a gfx950 device every render / intersect entry point fails with PYR_ERR_DEVICE. What makes a scene is scene_pack.cpp (deciding,
// on the host alone) and scene_create.cpp (uploading), what moves one after creation is live_scene.cpp, progressive sessions are
// session.cpp, and what develops, tone-maps or denoises an image without a scene is image_ops.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "api_internal.h"
#include "bvh.h"
#include "device_scene.h"
#include "scene_internal.h"

using namespace pyr;

namespace pyr {

int hip_fail(hipError_t e, const char* what) { return fail(PYR_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); }

int scene_device(const PyrScene* scene) { return scene->device; }

} // namespace pyr

namespace {

uint64_t film_buffer_grains(const PyrFilmDesc* film, const PyrRenderParams* p, const TilePlan& plan) {
    if (p->film_layout == PYR_FILM_TILE_BLOCKS) return (uint64_t)plan.tile_count * (p->tile_size + 2ull) * (p->tile_size + 2ull) * film->bins;
    const uint32_t rows = p->film_row_count ? p->film_row_count : film->height;
    return (uint64_t)rows * film->width * film->bins;
}

// Scheduler choice (kernels.hip): the bounce-synchronous walk wins when the scene lives in LDS and traversal is cheap
// (C2: 573 vs 300 Msamples/s); the stage scheduler wins when traversal lengths are heavy tailed (C3: 110 vs 91).
// PYRITE_SCHEDULER=sync|sm overrides; PYRITE_SM_LANES / PYRITE_SM_STEPS tune the stage scheduler.

// The spectral tape ([tape_max_ops][tape_lanes] 8-byte records), the queues of ready sample starts and the overflow word, kept on the scene between renders.
int reserve_tape(PyrScene* scene, RenderLaunch& L, hipStream_t stream) {
    const size_t bytes = (size_t)L.tape_lanes * L.tape_max_ops * sizeof(unsigned long long);
    if (bytes > scene->tape.bytes) {
        HIP_TRY(hipStreamSynchronize(stream)); // an earlier render of this scene may still be reading the old tape
        scene->tape.release();
        int rc = scene->tape.alloc(bytes);
        if (rc != PYR_OK) return rc;
    }
    L.tape = (unsigned long long*)scene->tape.ptr;
    if (scene->dev.needs_interpreter == 0) { // a ring of ready starts for every wave the tape has columns for (tape_lanes_bound)
        L.start_queue_stride = start_queue_words(L.spectrum_samples) * kStartQueueEntries;
        const size_t queue_bytes = (size_t)(L.tape_lanes / 64u) * L.start_queue_stride * sizeof(uint32_t);
        if (queue_bytes > scene->start_queue.bytes) {
            HIP_TRY(hipStreamSynchronize(stream));
            scene->start_queue.release();
            int rc = scene->start_queue.alloc(queue_bytes);
            if (rc != PYR_OK) return rc;
        }
        L.start_queue = (uint32_t*)scene->start_queue.ptr;
    }
    if (!scene->tape_overflow.ptr) {
        int rc = scene->tape_overflow.alloc(sizeof(uint32_t));
        if (rc != PYR_OK) return rc;
        // cleared on the stream the render is enqueued on: a null-stream memset is not ordered against a kernel on a
        // hipStreamNonBlocking stream (the multi-device entries use such streams)
        HIP_TRY(hipMemsetAsync(scene->tape_overflow.ptr, 0, sizeof(uint32_t), stream));
    }
    L.tape_overflow = (uint32_t*)scene->tape_overflow.ptr;
    return PYR_OK;
}

// Which schedule a render of this scene runs, and with which phase thresholds (defaults and the development switches).
void choose_schedule(const PyrScene* scene, RenderLaunch& L) {
    const char* e = std::getenv("PYRITE_SCHEDULER");
    if (e && std::string(e) == "sm")
        L.scheduler = 1;
    else if (e && std::string(e) == "sync")
        L.scheduler = 0;
    else // the synchronous walk for scenes that live in LDS -- unless they run interpreter programs: the stage scheduler keeps the
         // interpreter in line and memoised (spheres example 572 -> 737, lamps 549 -> 724 Msamples/s against the synchronous walk)
        L.scheduler = scene_is_lds_resident(scene->dev) && scene->dev.needs_interpreter == 0 ? 0u : 1u;
    // the program interpreter (and with it texture coordinates and normal maps) lives in the resumable integrator (Walker), in
    // line; the synchronous walk is built without it: PYRITE_SCHEDULER=sync on such a scene runs the stage scheduler
    if (L.scheduler == 0 && scene->dev.needs_interpreter != 0) L.scheduler = 1;
    const char* lanes = std::getenv("PYRITE_SM_LANES");
    const char* steps = std::getenv("PYRITE_SM_STEPS");
    // lanes that make a phase run: 16 on the BASELINE meshes (swept in rounds 2 and 3); 32 where the phases are heavy and the rays
    // short -- scenes that run the program interpreter (round 4, every example scene of the reference: textures 755 -> 859, spheres
    // 887 -> 969, lamps 726 -> 812, diamonds 543 -> 564 Msamples/s; flat from 28 to 48)
    L.sm_phase_lanes = lanes && *lanes ? (uint32_t)std::strtoul(lanes, nullptr, 10) : (scene->dev.needs_interpreter != 0 ? 32u : 16u);
    L.sm_trav_steps = steps && *steps ? (uint32_t)std::strtoul(steps, nullptr, 10) : 8u;
    const char* expose = std::getenv("PYRITE_SM_EXPOSE_LANES");
    L.sm_expose_lanes = expose && *expose ? (uint32_t)std::strtoul(expose, nullptr, 10) : L.sm_phase_lanes;
}

} // namespace

namespace pyr {

int plan_tiles(const PyrFilmDesc* film, const PyrRenderParams* p, TilePlan& plan) {
    // make_tiles, renderer/algorithm.rs:158-166
    const uint32_t ts = p->tile_size;
    plan.tiles_x = (film->width + ts - 1) / ts;
    plan.tiles_y = (film->height + ts - 1) / ts;
    const uint64_t total = (uint64_t)plan.tiles_x * plan.tiles_y;
    const uint64_t begin = p->tile_begin, end = p->tile_end ? p->tile_end : total;
    if (total >= 0xFFFFFFFFull || begin > end || end > total) return fail(PYR_ERR_INVALID_ARGUMENT, "tile range out of bounds");
    plan.tile_begin = (uint32_t)begin;
    plan.tile_stride = std::max(1u, p->tile_stride);
    plan.tile_count = (uint32_t)((end - begin + plan.tile_stride - 1) / plan.tile_stride);
    const uint64_t per_tile = ((uint64_t)ts * ts * p->pixel_samples + 63) / 64; // iterations of a full tile: simple.rs:73
    if (per_tile * plan.tile_count >= 0xFFFFFFFFull) return fail(PYR_ERR_UNSUPPORTED, "too many samples for one call: more than 2^32 chunks");
    // a window [sample_begin, sample_begin + pixel_samples) must end where a one-shot call of that many samples could: same bound
    const uint64_t window_end = (uint64_t)p->sample_begin + p->pixel_samples;
    if (p->sample_begin != 0 && (window_end > 0xFFFFFFFFull || (((uint64_t)ts * ts * window_end + 63) / 64) * plan.tile_count >= 0xFFFFFFFFull))
        return fail(PYR_ERR_UNSUPPORTED, "sample window ends beyond what one call can render: more than 2^32 chunks");
    plan.chunks_per_tile = (uint32_t)std::max<uint64_t>(per_tile, 1); // pixel_samples == 0: no chunk at all
    plan.chunk_begin = 0;
    plan.chunk_end = (uint32_t)(per_tile * plan.tile_count);
    return PYR_OK;
}

int check_render_args(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrRenderParams* p, const void* film_ptr) {
    if (!scene || !camera || !film || !p || !film_ptr) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    if (film->width == 0 || film->height == 0 || film->bins == 0 || p->tile_size == 0 || p->spectrum_samples == 0)
        return fail(PYR_ERR_INVALID_ARGUMENT, "zero-sized parameter");
    if (!(film->wl_width > 0.0f)) return fail(PYR_ERR_INVALID_ARGUMENT, "empty wavelength span");
    uint32_t rows = p->film_row_count ? p->film_row_count : film->height;
    if ((uint64_t)p->film_row_begin + rows > film->height) return fail(PYR_ERR_INVALID_ARGUMENT, "film window exceeds the image");
    if (p->spectrum_samples > 64) return fail(PYR_ERR_UNSUPPORTED, "spectrum_samples > 64");
    // a pixel is a 32-bit index into the call's film buffer (0xFFFFFFFF stands for "none"): 65,535 x 65,535 still fits
    if ((uint64_t)film->width * film->height >= 0xFFFFFFFFull) return fail(PYR_ERR_UNSUPPORTED, "image too large: 2^32 pixels or more");
    if (p->film_layout == PYR_FILM_TILE_BLOCKS) {
        const uint64_t tiles = (uint64_t)((film->width + p->tile_size - 1) / p->tile_size) * ((film->height + p->tile_size - 1) / p->tile_size);
        if (tiles * (p->tile_size + 2ull) * (p->tile_size + 2ull) >= 0xFFFFFFFFull) return fail(PYR_ERR_UNSUPPORTED, "image too large for a film of tile blocks");
    }
    if (p->film_layout > PYR_FILM_TILE_BLOCKS) return fail(PYR_ERR_INVALID_ARGUMENT, "unknown film layout");
    if (p->film_layout == PYR_FILM_TILE_BLOCKS && (p->film_row_begin || p->film_row_count))
        return fail(PYR_ERR_INVALID_ARGUMENT, "a film of tile blocks has no row window");
    return PYR_OK;
}

int render_batches(PyrScene* scene, RenderLaunch L, bool count, hipStream_t stream) {
    if (L.chunk_end == L.chunk_begin) return PYR_OK;
    choose_schedule(scene, L);
    if (launch_tape(scene->dev, L) != 0u) {
        L.tape_lanes = tape_lanes_bound(scene->num_cus);
        L.tape_max_ops = tape_ops_bound(scene->dev, L);
        int rc = reserve_tape(scene, L, stream);
        if (rc != PYR_OK) return rc;
    }
    return launch_render(scene->dev, L, count, stream, scene->num_cus, scene->program_info.wide != 0);
}

// After a render has been waited for: did a path outgrow the spectral tape (kernels.hip tape_push)? The film is wrong then.
int check_tape_overflow(PyrScene* scene) {
    if (!scene->tape_overflow.ptr) return PYR_OK;
    uint32_t word = 0;
    HIP_TRY(hipMemcpy(&word, scene->tape_overflow.ptr, sizeof(word), hipMemcpyDeviceToHost));
    if (word == 0) return PYR_OK;
    HIP_TRY(hipMemset(scene->tape_overflow.ptr, 0, sizeof(uint32_t)));
    if (word == 2) return fail(PYR_ERR_DEVICE, "a wave gave up waiting on its workgroup's LDS queues (spin limit): the film of that render is invalid");
    return fail(PYR_ERR_DEVICE, "a path appended more records than the spectral tape's bound allows: the film of that render is invalid");
}

// For the translation units that enqueue renders without waiting for them (multi.cpp): the word itself, and its check.
uint32_t* scene_overflow_word(PyrScene* scene) { return scene ? (uint32_t*)scene->tape_overflow.ptr : nullptr; }
int scene_check_overflow(PyrScene* scene) { return check_tape_overflow(scene); }

RenderLaunch make_launch(const PyrCamera* camera, const PyrFilmDesc* film, const PyrRenderParams* p, const TilePlan& plan) {
    RenderLaunch L{};
    L.camera = *camera;
    L.film = *film;
    L.bounces = p->bounces;
    L.light_samples = p->light_samples;
    L.spectrum_samples = p->spectrum_samples;
    L.tile_size = p->tile_size;
    L.pixel_samples = p->pixel_samples;
    L.sample_begin = p->sample_begin;
    L.tiles_x = plan.tiles_x;
    L.tiles_y = plan.tiles_y;
    L.tile_begin = plan.tile_begin;
    L.tile_stride = plan.tile_stride;
    L.tile_count = plan.tile_count;
    L.chunks_per_tile = plan.chunks_per_tile;
    L.chunk_begin = plan.chunk_begin;
    L.chunk_end = plan.chunk_end;
    L.film_layout = p->film_layout;
    L.film_row_begin = p->film_row_begin;
    L.film_row_count = p->film_row_count ? p->film_row_count : film->height;
    L.seed = p->seed;
    L.grains_per_wavelength = (float)film->bins / film->wl_width; // film.rs:38
    return L;
}

// What the three feature entries refuse before a device is looked for. `what` names the scene or session argument.
int check_feature_args(const void* owner, const char* what, const PyrCamera* camera, bool need_camera, const PyrFilmDesc* film, const PyrFeatureParams* fp,
                       const void* albedo, const void* pixels) {
    if (!owner) return fail(PYR_ERR_INVALID_ARGUMENT, std::string("null argument: ") + what);
    if (need_camera && !camera) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: camera");
    if (!film) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: film");
    if (!fp) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: fp");
    if (!albedo && !pixels) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: the albedo and the pixel buffer are both null");
    if (fp->grid < 1 || fp->grid > 8) return fail(PYR_ERR_INVALID_ARGUMENT, "fp->grid must be 1..8");
    if (albedo && (fp->albedo_bins < 1 || fp->albedo_bins > 64)) return fail(PYR_ERR_INVALID_ARGUMENT, "fp->albedo_bins must be 1..64");
    if (film->width == 0 || film->height == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "film: zero-sized image");
    if (albedo && !(film->wl_width > 0.0f)) return fail(PYR_ERR_INVALID_ARGUMENT, "film: empty wavelength span");
    if ((uint64_t)film->width * film->height >= 0xFFFFFFFFull) return fail(PYR_ERR_INVALID_ARGUMENT, "film: 2^32 pixels or more");
    if (pyr_device_count() <= 0) return fail(PYR_ERR_DEVICE, "no HIP device is visible; pyrite_gpu has no CPU path");
    return PYR_OK;
}

// Enqueues the pass on `stream`; the buffers are on the scene's device (either may be null).
int enqueue_features(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrFeatureParams* fp, PyrGrain* albedo, PyrFeaturePixel* pixels,
                     hipStream_t stream) {
    if (!scene->tail_count) HIP_TRY(hipMalloc((void**)&scene->tail_count, kFeedBytes));
    HIP_TRY(hipMemsetAsync(scene->tail_count, 0, kFeedBytes, stream));
    FeatureLaunch L{};
    L.camera = *camera;
    L.film = *film;
    L.grid = fp->grid;
    L.albedo_bins = albedo ? fp->albedo_bins : 0u;
    L.albedo = albedo;
    L.pixels = pixels;
    L.next = scene->tail_count;
    return launch_features(scene->dev, L, stream, scene->num_cus, scene->program_info.wide != 0);
}

// What the three motion entries refuse before a device is looked for. `what` names the scene or session argument.
int check_motion_args(const void* owner, const char* what, const PyrCamera* camera, bool need_camera, const PyrCamera* previous_camera, const PyrFilmDesc* film,
                      const void* pixels, float previous_w[16]) {
    if (!owner) return fail(PYR_ERR_INVALID_ARGUMENT, std::string("null argument: ") + what);
    if (need_camera && !camera) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: camera");
    if (!previous_camera) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: previous_camera");
    if (!film) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: film");
    if (!pixels) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: pixels");
    if (film->width == 0 || film->height == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "film: zero-sized image");
    if ((uint64_t)film->width * film->height >= 0xFFFFFFFFull) return fail(PYR_ERR_INVALID_ARGUMENT, "film: 2^32 pixels or more");
    if (pyr_camera_world_to_cam(previous_camera, previous_w) != PYR_OK) return fail(PYR_ERR_INVALID_ARGUMENT, std::string("previous_camera: ") + pyr_last_error());
    if (pyr_device_count() <= 0) return fail(PYR_ERR_DEVICE, "no HIP device is visible; pyrite_gpu has no CPU path");
    return PYR_OK;
}

// Enqueues the pass on `stream`; `pixels` is on the scene's device.
int enqueue_motion(PyrScene* scene, const PyrCamera* camera, const PyrCamera* previous_camera, const float previous_w[16], const PyrFilmDesc* film,
                   PyrMotionPixel* pixels, hipStream_t stream) {
    if (!scene->tail_count) HIP_TRY(hipMalloc((void**)&scene->tail_count, kFeedBytes));
    HIP_TRY(hipMemsetAsync(scene->tail_count, 0, kFeedBytes, stream));
    const LiveGeometry& live = scene->live;
    MotionLaunch L{};
    L.camera = *camera;
    std::memcpy(L.previous_w, previous_w, sizeof(L.previous_w));
    L.previous_view_plane = previous_camera->view_plane;
    L.width = film->width, L.height = film->height;
    L.previous_positions = live.previous_kept && live.num_triangles ? (const float*)live.previous_positions.ptr : nullptr;
    L.previous_spheres = live.previous_kept && live.num_spheres ? (const float*)live.previous_spheres.ptr : nullptr;
    L.pixels = pixels;
    L.next = scene->tail_count;
    return launch_motion(scene->dev, L, stream, scene->num_cus);
}

} // namespace pyr

extern "C" {

int pyr_abi_version(void) { return PYR_ABI_VERSION; }

int pyr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pyr_render_simple_device(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrRenderParams* params,
                             PyrGrain* film_device, void* hip_stream) {
    int rc = check_render_args(scene, camera, film, params, film_device);
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(scene->device));
    TilePlan plan;
    if ((rc = plan_tiles(film, params, plan)) != PYR_OK) return rc;
    if (plan.chunk_end == plan.chunk_begin) return PYR_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    RenderLaunch L = make_launch(camera, film, params, plan);
    L.film_out = film_device;
    const bool count = (params->flags & PYR_FLAG_COUNTERS) != 0;
    if (count) {
        HIP_TRY(hipMemsetAsync(scene->counters.ptr, 0, sizeof(PyrCounters), stream));
        L.counters = (unsigned long long*)scene->counters.ptr;
        scene->have_counters = true;
    }
    return render_batches(scene, L, count, stream);
}

int pyr_render_simple(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrRenderParams* params, PyrGrain* film_inout,
                      PyrProgressFn on_status, void* user) {
    int rc = check_render_args(scene, camera, film, params, film_inout);
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(scene->device));
    TilePlan plan;
    if ((rc = plan_tiles(film, params, plan)) != PYR_OK) return rc;
    const char* message = "Rendering"; // simple.rs:30
    if (on_status) on_status(user, 0, message);
    const size_t bytes = (size_t)film_buffer_grains(film, params, plan) * sizeof(PyrGrain);
    DeviceBuffer film_dev;
    if ((rc = film_dev.upload(film_inout, bytes)) != PYR_OK) return rc;
    RenderLaunch L = make_launch(camera, film, params, plan);
    L.film_out = (PyrGrain*)film_dev.ptr;
    const bool count = (params->flags & PYR_FLAG_COUNTERS) != 0;
    if (count) {
        HIP_TRY(hipMemset(scene->counters.ptr, 0, sizeof(PyrCounters)));
        L.counters = (unsigned long long*)scene->counters.ptr;
        scene->have_counters = true;
    }
    // With a progress callback the chunk range is cut into slices so the caller hears back between launches
    // (the reference reports after every finished tile, simple.rs:49-55); results do not depend on the slicing.
    const uint32_t total_chunks = plan.chunk_end - plan.chunk_begin;
    const uint32_t slices = on_status ? std::min<uint32_t>(20, std::max<uint32_t>(1, total_chunks / 4096)) : 1;
    for (uint32_t sidx = 0; sidx < slices; ++sidx) {
        RenderLaunch part = L;
        part.chunk_begin = plan.chunk_begin + (uint32_t)((uint64_t)total_chunks * sidx / slices);
        part.chunk_end = plan.chunk_begin + (uint32_t)((uint64_t)total_chunks * (sidx + 1) / slices);
        rc = render_batches(scene, part, count, nullptr);
        if (rc != PYR_OK) return rc;
        HIP_TRY(hipDeviceSynchronize());
        if (on_status) on_status(user, (uint8_t)((sidx + 1) * 100 / slices), message);
    }
    if ((rc = check_tape_overflow(scene)) != PYR_OK) return rc;
    HIP_TRY(hipMemcpy(film_inout, film_dev.ptr, bytes, hipMemcpyDeviceToHost));
    return PYR_OK;
}

uint64_t pyr_film_blocks_grains(const PyrFilmDesc* film, const PyrRenderParams* params) {
    if (!film || !params || film->width == 0 || film->height == 0 || film->bins == 0 || params->tile_size == 0) {
        fail(PYR_ERR_INVALID_ARGUMENT, "zero-sized parameter");
        return 0;
    }
    TilePlan plan;
    PyrRenderParams p = *params;
    if (p.pixel_samples == 0) p.pixel_samples = 1; // the size does not depend on it
    if (plan_tiles(film, &p, plan) != PYR_OK) return 0;
    p.film_layout = PYR_FILM_TILE_BLOCKS;
    return film_buffer_grains(film, &p, plan);
}

int pyr_film_blocks_assemble_device(const PyrFilmDesc* film, const PyrRenderParams* params, const PyrGrain* blocks_device, PyrGrain* film_device, int device,
                                    void* hip_stream) {
    if (!film || !params || !blocks_device || !film_device) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    if (film->width == 0 || film->height == 0 || film->bins == 0 || params->tile_size == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "zero-sized parameter");
    if (pyr_device_count() <= device || device < 0) return fail(PYR_ERR_DEVICE, "no such HIP device; pyrite_gpu has no CPU path");
    TilePlan plan;
    PyrRenderParams p = *params;
    if (p.pixel_samples == 0) p.pixel_samples = 1;
    int rc = plan_tiles(film, &p, plan);
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    AssembleLaunch A{};
    A.film = *film;
    A.tile_size = params->tile_size;
    A.tiles_x = plan.tiles_x;
    A.tile_begin = plan.tile_begin;
    A.tile_stride = plan.tile_stride;
    A.tile_count = plan.tile_count;
    A.blocks = blocks_device;
    A.film_out = film_device;
    return launch_assemble(A, hip_stream);
}

int pyr_scene_counters(PyrScene* scene, PyrCounters* out) {
    if (!scene || !out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    if (!scene->have_counters) return fail(PYR_ERR_INVALID_ARGUMENT, "no render with PYR_FLAG_COUNTERS has run on this scene");
    HIP_TRY(hipSetDevice(scene->device));
    HIP_TRY(hipDeviceSynchronize());
    int rc = check_tape_overflow(scene);
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipMemcpy(out, scene->counters.ptr, sizeof(PyrCounters), hipMemcpyDeviceToHost));
    return PYR_OK;
}

int pyr_scene_intersect_device(PyrScene* scene, const float* rays_device, uint32_t n, PyrHit* hits_device, void* hip_stream) {
    if (!scene || (n && (!rays_device || !hits_device))) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(scene->device));
    if (!scene->tail_count) HIP_TRY(hipMalloc((void**)&scene->tail_count, kFeedBytes));
    HIP_TRY(hipMemsetAsync(scene->tail_count, 0, kFeedBytes, (hipStream_t)hip_stream));
    IntersectLaunch L{rays_device, hits_device, n, nullptr, scene->tail_count, (uint32_t)scene->num_cus};
    return launch_intersect(scene->dev, L, false, hip_stream);
}

int pyr_scene_intersect(PyrScene* scene, const float* rays, uint32_t n, PyrHit* hits, float* elapsed_ms, PyrCounters* counters) {
    if (!scene || (n && (!rays || !hits))) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(scene->device));
    if (elapsed_ms) *elapsed_ms = 0.0f;
    if (counters) std::memset(counters, 0, sizeof(*counters));
    if (n == 0) return PYR_OK;
    DeviceBuffer rays_dev, hits_dev;
    int rc;
    if ((rc = rays_dev.upload(rays, (size_t)n * 24)) != PYR_OK) return rc;
    if ((rc = hits_dev.alloc((size_t)n * sizeof(PyrHit))) != PYR_OK) return rc;
    if (!scene->tail_count) HIP_TRY(hipMalloc((void**)&scene->tail_count, kFeedBytes));
    IntersectLaunch L{(const float*)rays_dev.ptr, (PyrHit*)hits_dev.ptr, n, nullptr, scene->tail_count, (uint32_t)scene->num_cus};
    if (counters) {
        HIP_TRY(hipMemset(scene->tail_count, 0, kFeedBytes));
        HIP_TRY(hipMemset(scene->counters.ptr, 0, sizeof(PyrCounters)));
        L.counters = (unsigned long long*)scene->counters.ptr;
        if ((rc = launch_intersect(scene->dev, L, true, nullptr)) != PYR_OK) return rc;
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(counters, scene->counters.ptr, sizeof(PyrCounters), hipMemcpyDeviceToHost));
        L.counters = nullptr;
    }
    hipEvent_t start, stop;
    HIP_TRY(hipEventCreate(&start));
    HIP_TRY(hipEventCreate(&stop));
    HIP_TRY(hipMemset(scene->tail_count, 0, kFeedBytes));
    HIP_TRY(hipEventRecord(start, nullptr));
    if ((rc = launch_intersect(scene->dev, L, false, nullptr)) != PYR_OK) return rc;
    HIP_TRY(hipEventRecord(stop, nullptr));
    HIP_TRY(hipEventSynchronize(stop));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, start, stop));
    (void)hipEventDestroy(start);
    (void)hipEventDestroy(stop);
    if (elapsed_ms) *elapsed_ms = ms;
    HIP_TRY(hipMemcpy(hits, hits_dev.ptr, (size_t)n * sizeof(PyrHit), hipMemcpyDeviceToHost));
    return PYR_OK;
}

int pyr_scene_path_info(PyrScene* scene, const PyrRenderParams* params, PyrPathInfo* out) {
    if (!scene || !params || !out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    RenderLaunch L{};
    L.spectrum_samples = params->spectrum_samples;
    choose_schedule(scene, L);
    *out = PyrPathInfo{};
    out->stage_scheduler = L.scheduler;
    out->interpreter = scene->dev.needs_interpreter;
    out->scene_in_lds = scene_is_lds_resident(scene->dev) ? 1u : 0u;
    out->tape = launch_tape(scene->dev, L);
    out->phase_lanes = L.scheduler != 0 ? L.sm_phase_lanes : 0u;
    return PYR_OK;
}

int pyr_scene_program_info(PyrScene* scene, PyrProgramInfo* out) {
    if (!scene || !out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    *out = scene->program_info;
    return PYR_OK;
}

int pyr_scene_build_info(PyrScene* scene, PyrBuildInfo* out) {
    if (!scene || !out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    if (scene->digest_source) { // first call: hash the tree, then let it go
        scene->build_info.tree_digest = pyr::tree_digest(*scene->digest_source);
        scene->digest_source.reset();
    }
    *out = scene->build_info;
    return PYR_OK;
}

int pyr_scene_bvh_info(PyrScene* scene, PyrBvhInfo* out) {
    if (!scene || !out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    *out = scene->info;
    return PYR_OK;
}

// ------------------------------------------------------------------------------------------------ first-hit feature images
int pyr_render_features_device(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrFeatureParams* fp, PyrGrain* albedo_device,
                               PyrFeaturePixel* pixels_device, void* hip_stream) {
    if (((uintptr_t)pixels_device & 15u) != 0) return fail(PYR_ERR_INVALID_ARGUMENT, "pixels_device must be 16-byte aligned"); // records are written as 16-byte vectors
    int rc = check_feature_args(scene, "scene", camera, true, film, fp, albedo_device, pixels_device);
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(scene->device));
    return enqueue_features(scene, camera, film, fp, albedo_device, pixels_device, (hipStream_t)hip_stream);
}

int pyr_render_features(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrFeatureParams* fp, PyrGrain* albedo_inout,
                        PyrFeaturePixel* pixels_out) {
    int rc = check_feature_args(scene, "scene", camera, true, film, fp, albedo_inout, pixels_out);
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(scene->device));
    const size_t pixels = (size_t)film->width * film->height;
    const size_t albedo_bytes = albedo_inout ? pixels * fp->albedo_bins * sizeof(PyrGrain) : 0, pixel_bytes = pixels_out ? pixels * sizeof(PyrFeaturePixel) : 0;
    DeviceBuffer albedo_dev, pixels_dev;
    if (albedo_inout && (rc = albedo_dev.upload(albedo_inout, albedo_bytes)) != PYR_OK) return rc;
    if (pixels_out && (rc = pixels_dev.alloc(pixel_bytes)) != PYR_OK) return rc;
    if ((rc = enqueue_features(scene, camera, film, fp, (PyrGrain*)albedo_dev.ptr, (PyrFeaturePixel*)pixels_dev.ptr, nullptr)) != PYR_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (albedo_inout) HIP_TRY(hipMemcpy(albedo_inout, albedo_dev.ptr, albedo_bytes, hipMemcpyDeviceToHost));
    if (pixels_out) HIP_TRY(hipMemcpy(pixels_out, pixels_dev.ptr, pixel_bytes, hipMemcpyDeviceToHost));
    return PYR_OK;
}

// ------------------------------------------------------------------------------------------------ motion records
int pyr_camera_world_to_cam(const PyrCamera* camera, float out[16]) {
    if (!camera || !out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    const float* m = camera->cam_to_world;
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(m[k])) return fail(PYR_ERR_INVALID_ARGUMENT, "cam_to_world has an entry that is not finite");
    if (!(m[3] == 0.0f && m[7] == 0.0f && m[11] == 0.0f && m[15] == 1.0f)) return fail(PYR_ERR_INVALID_ARGUMENT, "cam_to_world: the last row must be 0, 0, 0, 1");
    double a[3][3], t[3]; // a[row][column]
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) a[r][c] = (double)m[4 * c + r];
        t[r] = (double)m[12 + r];
    }
    double cof[3][3]; // cof[r][c]: the cofactor of a[r][c]
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            cof[r][c] = a[r1][c1] * a[r2][c2] - a[r1][c2] * a[r2][c1];
        }
    const double det = a[0][0] * cof[0][0] + a[0][1] * cof[0][1] + a[0][2] * cof[0][2];
    if (det == 0.0 || !std::isfinite(det)) return fail(PYR_ERR_INVALID_ARGUMENT, "cam_to_world: the determinant of its 3 x 3 part is 0 or not finite");
    for (int r = 0; r < 3; ++r) {
        double inv[3];
        for (int c = 0; c < 3; ++c) inv[c] = cof[c][r] / det; // the inverse is the transposed cofactors over the determinant
        for (int c = 0; c < 3; ++c) out[4 * c + r] = (float)inv[c];
        out[12 + r] = (float)-(inv[0] * t[0] + inv[1] * t[1] + inv[2] * t[2]);
    }
    out[3] = out[7] = out[11] = 0.0f;
    out[15] = 1.0f;
    return PYR_OK;
}

int pyr_render_motion_device(PyrScene* scene, const PyrCamera* camera, const PyrCamera* previous_camera, const PyrFilmDesc* film, PyrMotionPixel* pixels_device,
                             void* hip_stream) {
    if (((uintptr_t)pixels_device & 15u) != 0) return fail(PYR_ERR_INVALID_ARGUMENT, "pixels_device must be 16-byte aligned"); // records are written as 16-byte vectors
    float w[16];
    int rc = check_motion_args(scene, "scene", camera, true, previous_camera, film, pixels_device, w);
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(scene->device));
    return enqueue_motion(scene, camera, previous_camera, w, film, pixels_device, (hipStream_t)hip_stream);
}

int pyr_render_motion(PyrScene* scene, const PyrCamera* camera, const PyrCamera* previous_camera, const PyrFilmDesc* film, PyrMotionPixel* pixels_out) {
    float w[16];
    int rc = check_motion_args(scene, "scene", camera, true, previous_camera, film, pixels_out, w);
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(scene->device));
    const size_t bytes = (size_t)film->width * film->height * sizeof(PyrMotionPixel);
    DeviceBuffer pixels_dev;
    if ((rc = pixels_dev.alloc(bytes)) != PYR_OK) return rc;
    rc = enqueue_motion(scene, camera, previous_camera, w, film, (PyrMotionPixel*)pixels_dev.ptr, nullptr);
    HIP_TRY(hipDeviceSynchronize()); // before the buffer above is freed, whatever happened
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipMemcpy(pixels_out, pixels_dev.ptr, bytes, hipMemcpyDeviceToHost));
    return PYR_OK;
}

} // extern "C"
