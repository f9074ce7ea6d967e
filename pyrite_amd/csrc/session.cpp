// session.cpp -- progressive sessions (include/pyrite_gpu.h "progressive sessions"): PyrSession and every
// entry point that takes one, and pyr_render_simple_progressive, which runs one. An entry is the session's films, then the image
// pipeline on the session's stream, then one wait. The render side comes from api.cpp through scene_internal.h, the image side from
// image_ops.cpp through image_internal.h.
#include <algorithm>
#include <chrono>
#include <memory>
#include <new>
#include <vector>

#include "image_internal.h"
#include "scene_internal.h"

using namespace pyr;

struct PyrSession {
    PyrScene* scene = nullptr;
    PyrCamera camera{};
    PyrFilmDesc film{};
    PyrRenderParams params{}; // pixel_samples = the whole budget
    bool halves = false;
    hipStream_t stream = nullptr;
    DeviceBuffer film_a, film_b, sum, rgb, tables, noise, linear, stats;
    std::vector<float> host_tables;
    size_t grains = 0;
    uint32_t samples_done = 0, passes = 0;
    uint32_t tiles_x = 0, tiles_y = 0;
    ~PyrSession() {
        if (scene) scene->live_sessions--; // (pyr_scene_update refuses a scene that has one)
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

int session_ready(PyrSession* s) {
    if (!s) return fail(PYR_ERR_INVALID_ARGUMENT, "null session");
    HIP_TRY(hipSetDevice(s->scene->device));
    return PYR_OK;
}

// The film of the session on its device, valid in stream order: A, or A + B in the session's sum buffer.
int session_film(PyrSession* s, const PyrGrain** out) {
    *out = (const PyrGrain*)s->film_a.ptr;
    if (!s->halves) return PYR_OK;
    if (!s->sum.ptr) {
        int rc = s->sum.alloc(s->grains * sizeof(PyrGrain));
        if (rc != PYR_OK) return rc;
    }
    int rc = launch_film_sum((const PyrGrain*)s->film_a.ptr, (const PyrGrain*)s->film_b.ptr, (PyrGrain*)s->sum.ptr, s->grains, s->stream);
    if (rc != PYR_OK) return rc;
    *out = (const PyrGrain*)s->sum.ptr;
    return PYR_OK;
}

int session_sync(PyrSession* s) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    return check_tape_overflow(s->scene);
}

// The session's development tables on its device, in stream order, and the launch record that reads them (grains: A, and B with halves).
int session_develop_launch(PyrSession* s, const PyrDevelopParams* p, DevelopLaunch& D) {
    const size_t floats = develop_table_floats(p);
    if (floats * sizeof(float) > s->tables.bytes || !s->tables.ptr) {
        HIP_TRY(hipStreamSynchronize(s->stream)); // an earlier preview may still read the old tables
        s->tables.release();
        if (int rc = s->tables.alloc(floats * sizeof(float))) return rc;
    }
    D = develop_launch(&s->film, p, (float*)s->tables.ptr, s->host_tables);
    HIP_TRY(hipMemcpyAsync(s->tables.ptr, s->host_tables.data(), floats * sizeof(float), hipMemcpyHostToDevice, s->stream));
    D.grains = (const PyrGrain*)s->film_a.ptr;
    D.grains_b = s->halves ? (const PyrGrain*)s->film_b.ptr : nullptr;
    return PYR_OK;
}

// What pyr_session_create and pyr_render_simple_progressive refuse before anything runs.
int check_session_args(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrRenderParams* p) {
    if (!scene || !camera || !film || !p) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    if (film->width == 0 || film->height == 0 || film->bins == 0 || p->tile_size == 0 || p->spectrum_samples == 0 || p->pixel_samples == 0)
        return fail(PYR_ERR_INVALID_ARGUMENT, "zero-sized parameter");
    if (p->sample_begin != 0) return fail(PYR_ERR_INVALID_ARGUMENT, "a session starts its own sample windows: sample_begin must be 0");
    if (p->film_layout != PYR_FILM_ROWS || p->film_row_begin != 0 || (p->film_row_count != 0 && p->film_row_count != film->height))
        return fail(PYR_ERR_INVALID_ARGUMENT, "a session holds the whole image in the film.rs:56 layout");
    if (p->flags & PYR_FLAG_COUNTERS) return fail(PYR_ERR_INVALID_ARGUMENT, "a session keeps no counters");
    if (pyr_device_count() <= 0) return fail(PYR_ERR_DEVICE, "no HIP device is visible; pyrite_gpu has no CPU path");
    return PYR_OK;
}

// The session's film developed into its linear image buffer, enqueued on its stream.
int session_linear(PyrSession* s, const PyrDevelopParams* p, uint32_t space) {
    int rc;
    const size_t bytes = (size_t)s->film.width * s->film.height * 3 * sizeof(float);
    if (!s->linear.ptr && (rc = s->linear.alloc(bytes)) != PYR_OK) return rc;
    LinearLaunch L{};
    if ((rc = session_develop_launch(s, p, L.develop)) != PYR_OK) return rc;
    L.out = (float*)s->linear.ptr;
    L.space = space;
    return launch_develop_linear(L, s->stream);
}

// Runs `enqueue`, waits for the session's stream whatever happened -- the caller's buffers are freed after that -- and returns the first failure.
template <class Enqueue>
int enqueue_then_sync(PyrSession* s, Enqueue enqueue) {
    const int rc = enqueue();
    const int synced = session_sync(s);
    return rc != PYR_OK ? rc : synced;
}

// What pyr_session_denoised refuses, pyr_session_upsampled with it: the arguments, then a session without halves or with one pass.
int check_denoised_args(PyrSession* s, const PyrDevelopParams* develop_params, const PyrFeatureParams* feature_params, const PyrDenoiseParams* denoise_params,
                        const void* out) {
    int rc = check_linear_args(&s->film, s, develop_params, PYR_LINEAR_SRGB, out);
    if (rc != PYR_OK || (rc = check_denoise_params(denoise_params)) != PYR_OK) return rc;
    if (feature_params && (rc = check_feature_args(s, "session", nullptr, false, &s->film, feature_params, s, s)) != PYR_OK) return rc;
    if ((rc = session_ready(s)) != PYR_OK) return rc;
    if (!s->halves) return fail(PYR_ERR_INVALID_ARGUMENT, "denoising needs the two half films: create the session with PYR_SESSION_HALVES");
    if (s->passes < 2) return fail(PYR_ERR_INVALID_ARGUMENT, "denoising needs at least two passes: one half film is still empty");
    return PYR_OK;
}

// The feature pass with the session's camera over `film` -- the session's own, or one of more pixels over the same view -- and its
// albedo film developed with `p` into `albedo_out`, on the session's stream. The two buffers are allocated here and belong to the
// caller, who frees them after the wait.
int session_feature_images(PyrSession* s, const PyrFilmDesc* film, const PyrDevelopParams* p, const PyrFeatureParams* fp, DeviceBuffer& albedo_film, DeviceBuffer& records,
                           float* albedo_out) {
    int rc;
    const size_t count = (size_t)film->width * film->height, albedo_bytes = count * fp->albedo_bins * sizeof(PyrGrain);
    if ((rc = albedo_film.alloc(albedo_bytes)) != PYR_OK || (rc = records.alloc(count * sizeof(PyrFeaturePixel))) != PYR_OK) return rc;
    HIP_TRY(hipMemsetAsync(albedo_film.ptr, 0, albedo_bytes, s->stream));
    if ((rc = enqueue_features(s->scene, &s->camera, film, fp, (PyrGrain*)albedo_film.ptr, (PyrFeaturePixel*)records.ptr, s->stream)) != PYR_OK) return rc;
    LinearLaunch L{};
    if ((rc = session_develop_launch(s, p, L.develop)) != PYR_OK) return rc;
    L.space = PYR_LINEAR_SRGB;
    L.develop.film = *film;
    L.develop.film.bins = fp->albedo_bins; // the same span, tables and parameters
    L.develop.grains = (const PyrGrain*)albedo_film.ptr, L.develop.grains_b = nullptr, L.out = albedo_out;
    return launch_develop_linear(L, s->stream);
}

// The device side of pyr_session_denoised. `images`: eight images of the film's size in one allocation, made by the caller --
// 0, 1: the halves developed; 2: the developed albedo (with features); 3..5: the filter's working images; 6: the result; 7: the
// error image, when it is asked for.
struct DenoisedImages {
    DeviceBuffer images, albedo_film, records;
    float* at(const PyrSession* s, size_t i) const { return (float*)images.ptr + i * (size_t)s->film.width * s->film.height * 3; }
};
// Half film A alone and half film B alone developed to linear sRGB into `a_out` and `b_out`, on the session's stream.
int session_develop_halves(PyrSession* s, const PyrDevelopParams* develop_params, float* a_out, float* b_out) {
    int rc;
    LinearLaunch L{};
    if ((rc = session_develop_launch(s, develop_params, L.develop)) != PYR_OK) return rc;
    L.space = PYR_LINEAR_SRGB;
    L.develop.grains = (const PyrGrain*)s->film_a.ptr, L.develop.grains_b = nullptr, L.out = a_out;
    if ((rc = launch_develop_linear(L, s->stream)) != PYR_OK) return rc;
    L.develop.grains = (const PyrGrain*)s->film_b.ptr, L.out = b_out;
    return launch_develop_linear(L, s->stream);
}
// The cross filter of the half images at 0 and 1 of `D`, the feature pass before it when it steers.
int session_denoise_halves(PyrSession* s, const PyrDevelopParams* develop_params, const PyrFeatureParams* feature_params, const PyrDenoiseParams* denoise_params,
                           bool with_error, DenoisedImages& D) {
    int rc;
    if (feature_params && (rc = session_feature_images(s, &s->film, develop_params, feature_params, D.albedo_film, D.records, D.at(s, 2))) != PYR_OK) return rc;
    return enqueue_denoise(D.at(s, 0), D.at(s, 1), feature_params ? D.at(s, 2) : nullptr, feature_params ? (const PyrFeaturePixel*)D.records.ptr : nullptr, s->film.width,
                           s->film.height, denoise_params, D.at(s, 3), D.at(s, 6), with_error ? D.at(s, 7) : nullptr, s->stream);
}
int session_denoised(PyrSession* s, const PyrDevelopParams* develop_params, const PyrFeatureParams* feature_params, const PyrDenoiseParams* denoise_params, bool with_error,
                     DenoisedImages& D) {
    if (int rc = session_develop_halves(s, develop_params, D.at(s, 0), D.at(s, 1))) return rc;
    return session_denoise_halves(s, develop_params, feature_params, denoise_params, with_error, D);
}

} // namespace

extern "C" {

int pyr_session_create(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrRenderParams* params, uint32_t flags,
                       const PyrGrain* film_host, PyrSession** out_session) {
    if (!out_session) return fail(PYR_ERR_INVALID_ARGUMENT, "null out pointer");
    *out_session = nullptr;
    int rc = check_session_args(scene, camera, film, params);
    if (rc != PYR_OK) return rc;
    if (flags & ~PYR_SESSION_HALVES) return fail(PYR_ERR_INVALID_ARGUMENT, "unknown session flag");
    if ((rc = check_render_args(scene, camera, film, params, scene)) != PYR_OK) return rc;
    TilePlan plan;
    if ((rc = plan_tiles(film, params, plan)) != PYR_OK) return rc; // the whole budget must be one a single call could render
    HIP_TRY(hipSetDevice(scene->device));
    std::unique_ptr<PyrSession> s(new (std::nothrow) PyrSession());
    if (!s) return fail(PYR_ERR_OUT_OF_MEMORY, "out of host memory");
    s->scene = scene;
    scene->live_sessions++;
    s->camera = *camera;
    s->film = *film;
    s->params = *params;
    s->halves = (flags & PYR_SESSION_HALVES) != 0;
    s->tiles_x = plan.tiles_x, s->tiles_y = plan.tiles_y;
    s->grains = (size_t)film->width * film->height * film->bins;
    const size_t bytes = s->grains * sizeof(PyrGrain);
    HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    if (film_host) {
        if ((rc = s->film_a.upload(film_host, bytes)) != PYR_OK) return rc;
    } else {
        if ((rc = s->film_a.alloc(bytes)) != PYR_OK) return rc;
        HIP_TRY(hipMemsetAsync(s->film_a.ptr, 0, bytes, s->stream));
    }
    if (s->halves) {
        if ((rc = s->film_b.alloc(bytes)) != PYR_OK) return rc;
        HIP_TRY(hipMemsetAsync(s->film_b.ptr, 0, bytes, s->stream));
    }
    if ((rc = s->rgb.alloc((size_t)film->width * film->height * 3)) != PYR_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    *out_session = s.release();
    return PYR_OK;
}

void pyr_session_destroy(PyrSession* session) {
    if (!session) return;
    (void)hipSetDevice(session->scene->device);
    (void)hipStreamSynchronize(session->stream); // a pass may still be writing the films
    delete session;
}

int pyr_session_render(PyrSession* session, uint32_t samples) {
    int rc = session_ready(session);
    if (rc != PYR_OK) return rc;
    if (samples == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "zero-sized parameter");
    const uint32_t left = session->params.pixel_samples - session->samples_done;
    if (left == 0) return PYR_OK; // the budget is spent
    PyrRenderParams p = session->params;
    p.sample_begin = session->samples_done;
    p.pixel_samples = std::min(samples, left);
    TilePlan plan;
    if ((rc = plan_tiles(&session->film, &p, plan)) != PYR_OK) return rc;
    RenderLaunch L = make_launch(&session->camera, &session->film, &p, plan);
    L.film_out = (PyrGrain*)((session->halves && (session->passes & 1u)) ? session->film_b.ptr : session->film_a.ptr);
    if ((rc = render_batches(session->scene, L, false, session->stream)) != PYR_OK) return rc;
    session->samples_done += p.pixel_samples;
    session->passes += 1;
    return PYR_OK;
}

int pyr_session_sync(PyrSession* session) {
    int rc = session_ready(session);
    if (rc != PYR_OK) return rc;
    return session_sync(session);
}

int pyr_session_samples_done(PyrSession* session, uint32_t* out_samples) {
    if (!session || !out_samples) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    *out_samples = session->samples_done;
    return PYR_OK;
}

int pyr_session_preview(PyrSession* session, const PyrDevelopParams* develop_params, uint8_t* rgb_out) {
    if (!session || !develop_params || !rgb_out || !develop_params->xyz_table) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    int rc = session_ready(session);
    if (rc != PYR_OK) return rc;
    if ((rc = check_develop_params(develop_params)) != PYR_OK) return rc;
    PyrSession* s = session;
    DevelopLaunch D{};
    if ((rc = session_develop_launch(s, develop_params, D)) != PYR_OK) return rc;
    D.rgb_out = (uint8_t*)s->rgb.ptr;
    const PyrGrain* summed = nullptr;
    if (!develop_uses_wave(D)) { // the per-pixel kernel (of A + B where there are halves and the film has more bins than the wave kernel's rows)
        if ((rc = session_film(s, &summed)) != PYR_OK) return rc;
        D.grains = summed, D.grains_b = nullptr;
        rc = launch_develop(D, s->stream);
    } else {
        rc = launch_develop_wave(D, s->stream);
    }
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(rgb_out, s->rgb.ptr, (size_t)s->film.width * s->film.height * 3, hipMemcpyDeviceToHost, s->stream));
    return session_sync(s);
}

int pyr_session_film_device(PyrSession* session, PyrGrain* film_out_device) {
    if (!session || !film_out_device) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    int rc = session_ready(session);
    if (rc != PYR_OK) return rc;
    if (session->halves) {
        rc = launch_film_sum((const PyrGrain*)session->film_a.ptr, (const PyrGrain*)session->film_b.ptr, film_out_device, session->grains, session->stream);
        if (rc != PYR_OK) return rc;
    } else {
        HIP_TRY(hipMemcpyAsync(film_out_device, session->film_a.ptr, session->grains * sizeof(PyrGrain), hipMemcpyDeviceToDevice, session->stream));
    }
    return session_sync(session);
}

int pyr_session_film(PyrSession* session, PyrGrain* film_out) {
    if (!session || !film_out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    int rc = session_ready(session);
    if (rc != PYR_OK) return rc;
    const PyrGrain* film = nullptr;
    if ((rc = session_film(session, &film)) != PYR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(film_out, film, session->grains * sizeof(PyrGrain), hipMemcpyDeviceToHost, session->stream));
    return session_sync(session);
}

int pyr_session_halves(PyrSession* session, PyrGrain* film_a_out, PyrGrain* film_b_out) {
    if (!session || !film_a_out || !film_b_out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    int rc = session_ready(session);
    if (rc != PYR_OK) return rc;
    if (!session->halves) return fail(PYR_ERR_INVALID_ARGUMENT, "the session was created without PYR_SESSION_HALVES");
    HIP_TRY(hipMemcpyAsync(film_a_out, session->film_a.ptr, session->grains * sizeof(PyrGrain), hipMemcpyDeviceToHost, session->stream));
    HIP_TRY(hipMemcpyAsync(film_b_out, session->film_b.ptr, session->grains * sizeof(PyrGrain), hipMemcpyDeviceToHost, session->stream));
    return session_sync(session);
}

int pyr_session_noise(PyrSession* session, float* out_per_tile) {
    if (!session || !out_per_tile) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    int rc = session_ready(session);
    if (rc != PYR_OK) return rc;
    if (!session->halves) return fail(PYR_ERR_INVALID_ARGUMENT, "the noise estimate needs the two half films: create the session with PYR_SESSION_HALVES");
    if (session->passes < 2) return fail(PYR_ERR_INVALID_ARGUMENT, "the noise estimate needs at least two passes: one half film is still empty");
    const size_t tiles = (size_t)session->tiles_x * session->tiles_y;
    if (!session->noise.ptr && (rc = session->noise.alloc(tiles * sizeof(float))) != PYR_OK) return rc;
    NoiseLaunch N{};
    N.film = session->film;
    N.tile_size = session->params.tile_size;
    N.tiles_x = session->tiles_x, N.tiles_y = session->tiles_y;
    N.a = (const PyrGrain*)session->film_a.ptr;
    N.b = (const PyrGrain*)session->film_b.ptr;
    N.out = (float*)session->noise.ptr;
    if ((rc = launch_noise(N, session->stream)) != PYR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out_per_tile, session->noise.ptr, tiles * sizeof(float), hipMemcpyDeviceToHost, session->stream));
    return session_sync(session);
}

int pyr_render_simple_progressive(PyrScene* scene, const PyrCamera* camera, const PyrFilmDesc* film, const PyrRenderParams* params, PyrGrain* film_inout,
                                  uint32_t pass_samples, PyrProgressFn on_status, PyrPreviewFn on_preview, double preview_min_interval_s,
                                  const PyrDevelopParams* preview_develop_params, void* user) {
    if (!film_inout) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    if (on_preview && (!preview_develop_params || !preview_develop_params->xyz_table)) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: a preview needs development parameters");
    if (!scene || !camera || !film || !params) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    if (pass_samples == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "zero-sized parameter: pass_samples");
    if (!(preview_min_interval_s >= 0.0)) return fail(PYR_ERR_INVALID_ARGUMENT, "negative preview interval");
    int rc = check_session_args(scene, camera, film, params);
    if (rc != PYR_OK) return rc;
    PyrSession* raw = nullptr;
    if ((rc = pyr_session_create(scene, camera, film, params, 0u, film_inout, &raw)) != PYR_OK) return rc;
    struct Closer {
        PyrSession* s;
        ~Closer() { pyr_session_destroy(s); }
    } closer{raw};
    const char* message = "Rendering"; // simple.rs:30
    if (on_status) on_status(user, 0, message);
    std::vector<uint8_t> rgb;
    if (on_preview) rgb.resize((size_t)film->width * film->height * 3);
    const uint32_t budget = params->pixel_samples;
    auto last_preview = std::chrono::steady_clock::now(); // main.rs:261: the first preview comes one interval into the render
    while (raw->samples_done < budget) {
        if ((rc = pyr_session_render(raw, pass_samples)) != PYR_OK) return rc;
        if ((rc = session_sync(raw)) != PYR_OK) return rc;
        if (on_status) on_status(user, (uint8_t)((uint64_t)raw->samples_done * 100u / budget), message);
        const auto now = std::chrono::steady_clock::now();
        if (on_preview && std::chrono::duration<double>(now - last_preview).count() >= preview_min_interval_s) {
            if ((rc = pyr_session_preview(raw, preview_develop_params, rgb.data())) != PYR_OK) return rc;
            on_preview(user, rgb.data(), film->width, film->height, raw->samples_done);
            last_preview = std::chrono::steady_clock::now();
        }
    }
    return pyr_session_film(raw, film_inout);
}

int pyr_session_features(PyrSession* session, const PyrFeatureParams* fp, PyrGrain* albedo_out, PyrFeaturePixel* pixels_out) {
    int rc = check_feature_args(session, "session", nullptr, false, session ? &session->film : nullptr, fp, albedo_out, pixels_out);
    if (rc != PYR_OK) return rc;
    if ((rc = session_ready(session)) != PYR_OK) return rc;
    const size_t pixels = (size_t)session->film.width * session->film.height;
    const size_t albedo_bytes = albedo_out ? pixels * fp->albedo_bins * sizeof(PyrGrain) : 0, pixel_bytes = pixels_out ? pixels * sizeof(PyrFeaturePixel) : 0;
    DeviceBuffer albedo_dev, pixels_dev;
    if (albedo_out) {
        if ((rc = albedo_dev.alloc(albedo_bytes)) != PYR_OK) return rc;
        HIP_TRY(hipMemsetAsync(albedo_dev.ptr, 0, albedo_bytes, session->stream));
    }
    if (pixels_out && (rc = pixels_dev.alloc(pixel_bytes)) != PYR_OK) return rc;
    return enqueue_then_sync(session, [&]() -> int {
        int rc = enqueue_features(session->scene, &session->camera, &session->film, fp, (PyrGrain*)albedo_dev.ptr, (PyrFeaturePixel*)pixels_dev.ptr, session->stream);
        if (rc != PYR_OK) return rc;
        if (albedo_out && hipMemcpyAsync(albedo_out, albedo_dev.ptr, albedo_bytes, hipMemcpyDeviceToHost, session->stream) != hipSuccess)
            return fail(PYR_ERR_DEVICE, "hipMemcpyAsync of the albedo film failed");
        if (pixels_out && hipMemcpyAsync(pixels_out, pixels_dev.ptr, pixel_bytes, hipMemcpyDeviceToHost, session->stream) != hipSuccess)
            return fail(PYR_ERR_DEVICE, "hipMemcpyAsync of the feature records failed");
        return PYR_OK;
    });
}

int pyr_session_motion(PyrSession* session, const PyrCamera* previous_camera, PyrMotionPixel* pixels_out) {
    float w[16];
    int rc = check_motion_args(session, "session", nullptr, false, previous_camera, session ? &session->film : nullptr, pixels_out, w);
    if (rc != PYR_OK) return rc;
    if ((rc = session_ready(session)) != PYR_OK) return rc;
    const size_t bytes = (size_t)session->film.width * session->film.height * sizeof(PyrMotionPixel);
    DeviceBuffer pixels_dev;
    if ((rc = pixels_dev.alloc(bytes)) != PYR_OK) return rc;
    return enqueue_then_sync(session, [&]() -> int {
        int rc = enqueue_motion(session->scene, &session->camera, previous_camera, w, &session->film, (PyrMotionPixel*)pixels_dev.ptr, session->stream);
        if (rc != PYR_OK) return rc;
        if (hipMemcpyAsync(pixels_out, pixels_dev.ptr, bytes, hipMemcpyDeviceToHost, session->stream) != hipSuccess)
            return fail(PYR_ERR_DEVICE, "hipMemcpyAsync of the motion records failed");
        return PYR_OK;
    });
}

int pyr_session_motion_blurred(PyrSession* session, const PyrCamera* previous_camera, const PyrDevelopParams* develop_params, const PyrMotionBlurParams* blur_params,
                               float* out) {
    float w[16];
    if (!session) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: session");
    if (!develop_params) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: develop_params");
    if (!out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: out");
    int rc = check_motion_blur_params(blur_params, "blur_params"); // what needs no session comes first: before a device is looked for
    if (rc != PYR_OK || (rc = check_motion_args(session, "session", nullptr, false, previous_camera, &session->film, out, w)) != PYR_OK) return rc;
    if ((rc = check_linear_args(&session->film, session, develop_params, PYR_LINEAR_SRGB, out)) != PYR_OK || (rc = session_ready(session)) != PYR_OK) return rc;
    PyrSession* s = session;
    const size_t pixels = (size_t)s->film.width * s->film.height, image_bytes = pixels * 3 * sizeof(float);
    DeviceBuffer records_dev, out_dev;
    if ((rc = records_dev.alloc(pixels * sizeof(PyrMotionPixel))) != PYR_OK || (rc = out_dev.alloc(image_bytes)) != PYR_OK) return rc;
    return enqueue_then_sync(s, [&]() -> int {
        int rc = session_linear(s, develop_params, PYR_LINEAR_SRGB);
        if (rc != PYR_OK) return rc;
        if ((rc = enqueue_motion(s->scene, &s->camera, previous_camera, w, &s->film, (PyrMotionPixel*)records_dev.ptr, s->stream)) != PYR_OK) return rc;
        rc = enqueue_motion_blur((const float*)s->linear.ptr, (const PyrMotionPixel*)records_dev.ptr, s->film.width, s->film.height, blur_params, (float*)out_dev.ptr, s->stream);
        if (rc != PYR_OK) return rc;
        if (hipMemcpyAsync(out, out_dev.ptr, image_bytes, hipMemcpyDeviceToHost, s->stream) != hipSuccess) return fail(PYR_ERR_DEVICE, "hipMemcpyAsync of the blurred image failed");
        return PYR_OK;
    });
}

int pyr_session_glared(PyrSession* session, const PyrDevelopParams* develop_params, const PyrGlareParams* glare_params, float* out) {
    if (!session) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: session");
    if (!develop_params) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: develop_params");
    if (!out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: out");
    int rc = check_glare_params(glare_params, "glare_params"); // what needs no session comes first: before a device is looked for
    if (rc != PYR_OK || (rc = check_linear_args(&session->film, session, develop_params, PYR_LINEAR_SRGB, out)) != PYR_OK || (rc = session_ready(session)) != PYR_OK) return rc;
    PyrSession* s = session;
    const size_t image_bytes = (size_t)s->film.width * s->film.height * 3 * sizeof(float);
    DeviceBuffer out_dev;
    if ((rc = out_dev.alloc(image_bytes)) != PYR_OK) return rc;
    return enqueue_then_sync(s, [&]() -> int {
        int rc = session_linear(s, develop_params, PYR_LINEAR_SRGB);
        if (rc != PYR_OK) return rc;
        if ((rc = enqueue_glare((const float*)s->linear.ptr, s->film.width, s->film.height, glare_params, (float*)out_dev.ptr, s->stream)) != PYR_OK) return rc;
        if (hipMemcpyAsync(out, out_dev.ptr, image_bytes, hipMemcpyDeviceToHost, s->stream) != hipSuccess) return fail(PYR_ERR_DEVICE, "hipMemcpyAsync of the glared image failed");
        return PYR_OK;
    });
}

int pyr_session_lens_blurred(PyrSession* session, const PyrDevelopParams* develop_params, const PyrFeatureParams* feature_params, const PyrLensBlurParams* blur_params,
                             float* out) {
    if (!session) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: session");
    if (!develop_params) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: develop_params");
    if (!feature_params) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: feature_params");
    if (!out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: out");
    int rc = check_lens_blur_params(blur_params, "blur_params"); // what needs no session comes first: before a device is looked for
    if (rc != PYR_OK || (rc = check_feature_args(session, "session", nullptr, false, &session->film, feature_params, nullptr, out)) != PYR_OK) return rc;
    if ((rc = check_linear_args(&session->film, session, develop_params, PYR_LINEAR_SRGB, out)) != PYR_OK || (rc = session_ready(session)) != PYR_OK) return rc;
    PyrSession* s = session;
    const size_t pixels = (size_t)s->film.width * s->film.height, image_bytes = pixels * 3 * sizeof(float);
    DeviceBuffer records_dev, out_dev;
    if ((rc = records_dev.alloc(pixels * sizeof(PyrFeaturePixel))) != PYR_OK || (rc = out_dev.alloc(image_bytes)) != PYR_OK) return rc;
    return enqueue_then_sync(s, [&]() -> int {
        int rc = session_linear(s, develop_params, PYR_LINEAR_SRGB);
        if (rc != PYR_OK) return rc;
        if ((rc = enqueue_features(s->scene, &s->camera, &s->film, feature_params, nullptr, (PyrFeaturePixel*)records_dev.ptr, s->stream)) != PYR_OK) return rc;
        rc = enqueue_lens_blur((const float*)s->linear.ptr, (const PyrFeaturePixel*)records_dev.ptr, s->film.width, s->film.height, blur_params, (float*)out_dev.ptr, s->stream);
        if (rc != PYR_OK) return rc;
        if (hipMemcpyAsync(out, out_dev.ptr, image_bytes, hipMemcpyDeviceToHost, s->stream) != hipSuccess) return fail(PYR_ERR_DEVICE, "hipMemcpyAsync of the blurred image failed");
        return PYR_OK;
    });
}

int pyr_session_linear(PyrSession* session, const PyrDevelopParams* develop_params, uint32_t space, float* out) {
    if (!session) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check_linear_args(&session->film, session, develop_params, space, out);
    if (rc != PYR_OK || (rc = session_ready(session)) != PYR_OK) return rc;
    if ((rc = session_linear(session, develop_params, space)) != PYR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, session->linear.ptr, (size_t)session->film.width * session->film.height * 3 * sizeof(float), hipMemcpyDeviceToHost, session->stream));
    return session_sync(session);
}

int pyr_session_preview_tone(PyrSession* session, const PyrDevelopParams* develop_params, const PyrToneParams* tone, uint8_t* rgb_out, PyrImageStats* stats_out) {
    if (!session || !tone) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check_tone_params(tone);
    if (rc != PYR_OK || (rc = check_linear_args(&session->film, session, develop_params, PYR_LINEAR_SRGB, rgb_out)) != PYR_OK || (rc = session_ready(session)) != PYR_OK) return rc;
    PyrSession* s = session;
    const size_t pixels = (size_t)s->film.width * s->film.height;
    if ((rc = session_linear(s, develop_params, PYR_LINEAR_SRGB)) != PYR_OK) return rc;
    PyrImageStats stats{};
    if (tone_needs_stats(tone) || stats_out) {
        if (!s->stats.ptr && (rc = s->stats.alloc(sizeof(PyrImageStats))) != PYR_OK) return rc;
        if ((rc = launch_image_stats((const float*)s->linear.ptr, pixels, (PyrImageStats*)s->stats.ptr, s->stream)) != PYR_OK) return rc;
        HIP_TRY(hipMemcpyAsync(&stats, s->stats.ptr, sizeof(PyrImageStats), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream)); // the rule is host arithmetic on 1 KB
        if (stats_out) *stats_out = stats;
    }
    ToneLaunch T{(const float*)s->linear.ptr, (uint8_t*)s->rgb.ptr, pixels, tone->op, 0.0f, 0.0f};
    if ((rc = pyr_tone_resolve(&stats, tone, &T.exposure, &T.white)) != PYR_OK) return rc;
    if ((rc = launch_tonemap(T, s->stream)) != PYR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(rgb_out, s->rgb.ptr, pixels * 3, hipMemcpyDeviceToHost, s->stream));
    return session_sync(s);
}

int pyr_session_denoised(PyrSession* session, const PyrDevelopParams* develop_params, const PyrFeatureParams* feature_params, const PyrDenoiseParams* denoise_params,
                         float* out, float* error_out) {
    if (!session) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: session");
    PyrSession* s = session;
    int rc = check_denoised_args(s, develop_params, feature_params, denoise_params, out);
    if (rc != PYR_OK) return rc;
    const size_t image_bytes = (size_t)s->film.width * s->film.height * 3 * sizeof(float);
    DenoisedImages D;
    if ((rc = D.images.alloc(8 * image_bytes)) != PYR_OK) return rc;
    return enqueue_then_sync(s, [&]() -> int {
        int rc = session_denoised(s, develop_params, feature_params, denoise_params, error_out != nullptr, D);
        if (rc != PYR_OK) return rc;
        HIP_TRY(hipMemcpyAsync(out, D.at(s, 6), image_bytes, hipMemcpyDeviceToHost, s->stream));
        if (error_out) HIP_TRY(hipMemcpyAsync(error_out, D.at(s, 7), image_bytes, hipMemcpyDeviceToHost, s->stream));
        return PYR_OK;
    });
}

int pyr_session_upsampled(PyrSession* session, uint32_t scale, const PyrDevelopParams* develop_params, const PyrFeatureParams* feature_params,
                          const PyrDenoiseParams* denoise_params, const PyrUpsampleParams* upsample_params, float* out) {
    if (!session) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: session");
    if (!develop_params) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: develop_params");
    if (!out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: out");
    PyrSession* s = session;
    int rc = check_upsample_scale(scale); // what needs no session comes first: before a device is looked for
    if (rc != PYR_OK || (rc = check_upsample_params(upsample_params, "upsample_params", feature_params != nullptr)) != PYR_OK) return rc;
    if ((rc = check_upsample_size(s->film.width, s->film.height, scale)) != PYR_OK) return rc;
    PyrFilmDesc high = s->film; // the same camera over scale * scale as many pixels: Camera::to_view_area maps a block of them onto one of the film's
    high.width *= scale, high.height *= scale;
    if (denoise_params)
        rc = check_denoised_args(s, develop_params, feature_params, denoise_params, out);
    else if ((rc = check_linear_args(&s->film, s, develop_params, PYR_LINEAR_SRGB, out)) == PYR_OK && feature_params)
        rc = check_feature_args(s, "session", nullptr, false, &s->film, feature_params, s, s);
    if (rc == PYR_OK && feature_params) rc = check_feature_args(s, "session", nullptr, false, &high, feature_params, s, s);
    if (rc != PYR_OK || (rc = session_ready(s)) != PYR_OK) return rc;
    const size_t low_count = (size_t)s->film.width * s->film.height, count = low_count * scale * scale, low_bytes = low_count * 3 * sizeof(float), image_bytes = count * 3 * sizeof(float);
    DenoisedImages D;
    DeviceBuffer high_albedo_film, high_records, high_images; // high_images: the developed albedo (with features), then out
    if (denoise_params && (rc = D.images.alloc(8 * low_bytes)) != PYR_OK) return rc;
    if (!denoise_params && feature_params && (rc = D.images.alloc(3 * low_bytes)) != PYR_OK) return rc; // only image 2, the low albedo, is used
    if ((rc = high_images.alloc(2 * image_bytes)) != PYR_OK) return rc;
    float *albedo = (float*)high_images.ptr, *out_dev = albedo + count * 3;
    return enqueue_then_sync(s, [&]() -> int {
        int rc;
        const float* low = nullptr;
        if (denoise_params) {
            if ((rc = session_denoised(s, develop_params, feature_params, denoise_params, false, D)) != PYR_OK) return rc;
            low = D.at(s, 6);
        } else {
            if ((rc = session_linear(s, develop_params, PYR_LINEAR_SRGB)) != PYR_OK) return rc;
            low = (const float*)s->linear.ptr;
            if (feature_params && (rc = session_feature_images(s, &s->film, develop_params, feature_params, D.albedo_film, D.records, D.at(s, 2))) != PYR_OK) return rc;
        }
        if (feature_params && (rc = session_feature_images(s, &high, develop_params, feature_params, high_albedo_film, high_records, albedo)) != PYR_OK) return rc;
        rc = enqueue_upsample(low, feature_params ? D.at(s, 2) : nullptr, feature_params ? (const PyrFeaturePixel*)D.records.ptr : nullptr, s->film.width, s->film.height, scale,
                              feature_params ? albedo : nullptr, feature_params ? (const PyrFeaturePixel*)high_records.ptr : nullptr, upsample_params, out_dev, s->stream);
        if (rc != PYR_OK) return rc;
        if (hipMemcpyAsync(out, out_dev, image_bytes, hipMemcpyDeviceToHost, s->stream) != hipSuccess) return fail(PYR_ERR_DEVICE, "hipMemcpyAsync of the upsampled image failed");
        return PYR_OK;
    });
}

int pyr_session_despeckled(PyrSession* session, const PyrDevelopParams* develop_params, const PyrDespeckleParams* despeckle_params,
                           const PyrFeatureParams* feature_params, const PyrDenoiseParams* denoise_params, float* out, float* error_out, float* removed_out,
                           uint32_t* counts_out) {
    if (!session) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: session");
    if (!develop_params) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: develop_params");
    if (!out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: out");
    PyrSession* s = session;
    int rc = check_despeckle_params(despeckle_params, "despeckle_params"); // what needs no session comes first: before a device is looked for
    if (rc != PYR_OK || (rc = check_linear_args(&s->film, s, develop_params, PYR_LINEAR_SRGB, out)) != PYR_OK) return rc;
    if (denoise_params && (rc = check_denoise_params(denoise_params)) != PYR_OK) return rc;
    if (denoise_params && feature_params && (rc = check_feature_args(s, "session", nullptr, false, &s->film, feature_params, s, s)) != PYR_OK) return rc;
    if ((rc = session_ready(s)) != PYR_OK) return rc;
    if (!s->halves) return fail(PYR_ERR_INVALID_ARGUMENT, "despeckling needs the two half films: create the session with PYR_SESSION_HALVES");
    if (s->passes < 2) return fail(PYR_ERR_INVALID_ARGUMENT, "despeckling needs at least two passes: one half film is still empty");
    const uint32_t width = s->film.width, height = s->film.height;
    const size_t pixels = (size_t)width * height, image_bytes = pixels * 3 * sizeof(float);
    DenoisedImages D; // 0, 1: the cleaned halves; 2..5: the denoiser's; 6: out; 7: the error image
    DeviceBuffer raw, counts; // raw: the halves as developed, then what the clamp removed
    if ((rc = D.images.alloc(8 * image_bytes)) != PYR_OK || (rc = raw.alloc(3 * image_bytes)) != PYR_OK || (rc = counts.alloc(2 * sizeof(uint32_t))) != PYR_OK) return rc;
    float *raw_a = (float*)raw.ptr, *raw_b = raw_a + pixels * 3, *removed = raw_b + pixels * 3;
    return enqueue_then_sync(s, [&]() -> int {
        int rc = session_develop_halves(s, develop_params, raw_a, raw_b);
        if (rc != PYR_OK) return rc;
        rc = enqueue_despeckle(raw_a, raw_b, width, height, despeckle_params, D.at(s, 0), D.at(s, 1), removed_out ? removed : nullptr, (uint32_t*)counts.ptr, s->stream);
        if (rc != PYR_OK) return rc;
        if (denoise_params)
            rc = session_denoise_halves(s, develop_params, feature_params, denoise_params, error_out != nullptr, D);
        else
            rc = launch_denoise_combine(D.at(s, 0), D.at(s, 1), pixels, D.at(s, 6), error_out ? D.at(s, 7) : nullptr, s->stream); // the mean and half the difference
        if (rc != PYR_OK) return rc;
        HIP_TRY(hipMemcpyAsync(out, D.at(s, 6), image_bytes, hipMemcpyDeviceToHost, s->stream));
        if (error_out) HIP_TRY(hipMemcpyAsync(error_out, D.at(s, 7), image_bytes, hipMemcpyDeviceToHost, s->stream));
        if (removed_out) HIP_TRY(hipMemcpyAsync(removed_out, removed, image_bytes, hipMemcpyDeviceToHost, s->stream));
        if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, counts.ptr, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        return PYR_OK;
    });
}

} // extern "C"
