// image_ops.cpp -- the entry points of include/pyrite_gpu.h that take a device number and never see a scene: a film developed to
// an 8-bit or a linear image, an image's luminance statistics, its tone mapping, the denoising of two half images, the
// accumulation of linear images over frames along their motion records (plain, and as the temporal resolve), the motion blur of
// one along them, the glare of one, the guided upsampling of one, the firefly clamp of two halves, the lens blur of one over its
// feature records. Every operation is stated in three parts, each once ("adding an image entry"):
//   its checks, composed from the pieces below in the order that entry refuses in (tests/golden/image_refusals.json pins it);
//   one enqueue_... function: device pointers, the public parameter block, a stream -- the one place its launch record is built;
//   two entries: the _device form is checks, use_device, enqueue; the host form is checks, use_device and Staging::finish, which
//   runs the same enqueue on the null stream between the staged inputs and the copies back.
// What a progressive session does with its own film through the same checks and launches (session.cpp) is declared in
// image_internal.h.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "image_internal.h"

using namespace pyr;

namespace {

constexpr uint64_t kMaxImagePixels = 0xFFFFFFFFull; // PyrImageStats counts in 32 bits
bool percentile_ok(float p) { return p > 0.0f && p <= 1.0f; }
int check_tone_operator(uint32_t op) { // shared by what pyr_tone_resolve and what pyr_image_tonemap refuse
    if (op != PYR_TONE_CLIP && op != PYR_TONE_REINHARD) return fail(PYR_ERR_INVALID_ARGUMENT, "unknown tone operator: PYR_TONE_CLIP or PYR_TONE_REINHARD");
    return PYR_OK;
}

// `bytes` of device memory for what `run` enqueues on `stream`, allocated and freed in stream order around it: the free stands
// behind everything `run` enqueued. A failure of `run` is reported before a failure of the free.
template <class Run>
int with_stream_memory(size_t bytes, hipStream_t stream, Run run) {
    void* memory = nullptr;
    HIP_TRY(hipMallocAsync(&memory, bytes, stream));
    const int rc = run(memory);
    const hipError_t freed = hipFreeAsync(memory, stream);
    if (rc != PYR_OK) return rc;
    if (freed != hipSuccess) return hip_fail(freed, "hipFreeAsync");
    return PYR_OK;
}

// The device side of a host entry: copies of the inputs, buffers for the outputs, then the enqueue, the wait and the copies back.
// `rc` holds the first failure; after one nothing more is staged and nothing is enqueued. The buffers are freed when the Staging
// goes out of scope, which finish() makes safe: it has waited for the device by then, whatever happened.
struct Staging {
    DeviceBuffer buffers[9]; // the temporal resolve's six inputs and three outputs: the most any entry stages
    void* host_of[9] = {};   // where finish() copies buffers[i] back to; nullptr: an input
    int used = 0, rc = PYR_OK;

    // A device copy of `bytes` at `host`; nullptr where the caller gave none (an optional input).
    template <class T>
    const T* in(const T* host, size_t bytes) {
        if (rc != PYR_OK || !host) return nullptr;
        rc = buffers[used].upload(host, bytes);
        return (const T*)buffers[used++].ptr;
    }
    // A device buffer of `bytes` that finish() copies to `host`; nullptr where the caller asked for none (an optional output).
    template <class T>
    T* out(T* host, size_t bytes) {
        if (rc != PYR_OK || !host) return nullptr;
        rc = buffers[used].alloc(bytes);
        host_of[used] = host;
        return (T*)buffers[used++].ptr;
    }
    // enqueue(args...) unless the staging failed -- the arguments, the staged pointers among them, are complete before this is
    // entered -- then the wait, the first failure, and only without one every output copied back.
    template <class Enqueue, class... Args>
    int finish(Enqueue enqueue, Args... args) {
        if (rc == PYR_OK) rc = enqueue(args...);
        const hipError_t waited = hipDeviceSynchronize();
        if (rc != PYR_OK) return rc;
        if (waited != hipSuccess) return hip_fail(waited, "hipDeviceSynchronize()");
        for (int i = 0; i < used; ++i)
            if (host_of[i]) HIP_TRY(hipMemcpy(host_of[i], buffers[i].ptr, buffers[i].bytes, hipMemcpyDeviceToHost));
        return PYR_OK;
    }
};

} // namespace

namespace pyr {

// Which develop kernel a launch runs. Both write the same bytes (tests/test_gpu_session.py); the choice is the measured one (DESIGN.md
// section 9a, C3-sized film): develop_wave_kernel (kernels/film.hip: one wave per run of pixels, the whole film read in full lines) when
// the trapezoid walk touches most bins -- step 2: 2.90 against 4.85 ms -- and develop_kernel (kernels/main.hip: one thread per pixel,
// reads only the bins it samples) when it touches fewer than half of them -- step 30, 15 of 64 bins: 0.44 against 0.65 ms. Two half films
// are developed by the wave kernel, which adds them as it reads; films of more bins than its LDS rows hold by develop_kernel.
// PYRITE_DEVELOP_KERNEL=pixel|wave overrides (development: tools/bench_session.py times one against the other).
bool develop_uses_wave(const DevelopLaunch& D) {
    if (!develop_wave_serves(D)) return false;
    if (D.grains_b) return true;
    const char* e = std::getenv("PYRITE_DEVELOP_KERNEL");
    if (e && std::string(e) == "pixel") return false;
    if (e && std::string(e) == "wave") return true;
    return 2ull * D.sample_count > D.film.bins;
}

size_t develop_table_floats(const PyrDevelopParams* p) { return 3 * (size_t)p->sample_count + 3 * (size_t)p->xyz_count; }

// The launch record of a development with the per-wavelength tables at `tables` (device: filter, white_div, white_mul -- sample_count
// floats each -- then the observer table); `host` receives the same floats for the caller to copy there.
DevelopLaunch develop_launch(const PyrFilmDesc* film, const PyrDevelopParams* p, float* tables, std::vector<float>& host) {
    const size_t n = p->sample_count;
    host.assign(develop_table_floats(p), 0.0f);
    if (p->filter) std::memcpy(host.data(), p->filter, n * 4);
    if (p->white_div) {
        std::memcpy(host.data() + n, p->white_div, n * 4);
        std::memcpy(host.data() + 2 * n, p->white_mul, n * 4);
    }
    std::memcpy(host.data() + 3 * n, p->xyz_table, 3 * (size_t)p->xyz_count * 4);
    DevelopLaunch D{};
    D.film = *film;
    D.step_size = p->step_size, D.xyz_scale = p->xyz_scale, D.sample_count = p->sample_count;
    D.filter = p->filter ? tables : nullptr;
    D.white_div = p->white_div ? tables + n : nullptr, D.white_mul = p->white_div ? tables + 2 * n : nullptr;
    D.xyz_table = tables + 3 * n, D.xyz_count = p->xyz_count, D.xyz_min = p->xyz_min, D.xyz_max = p->xyz_max;
    return D;
}

int check_develop_params(const PyrDevelopParams* p) {
    if (!(p->step_size > 0.0f) || p->sample_count == 0 || p->xyz_count < 2) return fail(PYR_ERR_INVALID_ARGUMENT, "bad development parameters");
    if ((p->white_div == nullptr) != (p->white_mul == nullptr)) return fail(PYR_ERR_INVALID_ARGUMENT, "white_div and white_mul go together");
    return PYR_OK;
}
int check_image_size(uint32_t width, uint32_t height) {
    if ((uint64_t)width * height > kMaxImagePixels) return fail(PYR_ERR_UNSUPPORTED, "an image of more than 2^32 - 1 pixels");
    return PYR_OK;
}
int check_device(int device) {
    if (pyr_device_count() <= device || device < 0) return fail(PYR_ERR_DEVICE, "no such HIP device; pyrite_gpu has no CPU path");
    return PYR_OK;
}
int check_linear_args(const PyrFilmDesc* film, const void* grains, const PyrDevelopParams* p, uint32_t space, const void* out) {
    if (!film || !grains || !p || !out || !p->xyz_table) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    if (space != PYR_LINEAR_XYZ && space != PYR_LINEAR_SRGB) return fail(PYR_ERR_INVALID_ARGUMENT, "unknown space: PYR_LINEAR_XYZ or PYR_LINEAR_SRGB");
    if (int bad = check_develop_params(p)) return bad;
    if (film->bins == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "film: no bins");
    return check_image_size(film->width, film->height);
}
// What pyr_tone_resolve refuses.
int check_tone_params(const PyrToneParams* t) {
    if (int bad = check_tone_operator(t->op)) return bad;
    if (!percentile_ok(t->percentile) || !percentile_ok(t->white_percentile)) return fail(PYR_ERR_INVALID_ARGUMENT, "a percentile outside (0, 1]");
    if (!(t->exposure > 0.0f) && !(t->key > 0.0f)) return fail(PYR_ERR_INVALID_ARGUMENT, "an automatic exposure needs a positive key");
    return PYR_OK;
}
bool tone_needs_stats(const PyrToneParams* t) { return !(t->exposure > 0.0f) || (t->op == PYR_TONE_REINHARD && !(t->white > 0.0f)); }

// What the three denoise entries refuse before a device is looked for.
int check_denoise_params(const PyrDenoiseParams* p) {
    if (!p) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: params");
    if (p->radius < 1 || p->radius > PYR_DENOISE_MAX_RADIUS) return fail(PYR_ERR_INVALID_ARGUMENT, "params->radius must be 1..10");
    if (p->patch > PYR_DENOISE_MAX_PATCH) return fail(PYR_ERR_INVALID_ARGUMENT, "params->patch must be 0..3");
    if (!(p->k > 0.0f)) return fail(PYR_ERR_INVALID_ARGUMENT, "params->k must be positive");
    if (!(p->epsilon > 0.0f)) return fail(PYR_ERR_INVALID_ARGUMENT, "params->epsilon must be positive");
    if (p->reserved != 0) return fail(PYR_ERR_INVALID_ARGUMENT, "params->reserved must be 0");
    return PYR_OK;
}

// What the three motion blur entries refuse of their parameters before a device is looked for (`what`: params or blur_params).
int check_motion_blur_params(const PyrMotionBlurParams* p, const char* what) {
    const std::string name = std::string(what) + "->";
    if (!p) return fail(PYR_ERR_INVALID_ARGUMENT, std::string("null argument: ") + what);
    if (!(p->shutter > 0.0f && p->shutter <= 1.0f)) return fail(PYR_ERR_INVALID_ARGUMENT, name + "shutter must be in (0, 1]");
    if (p->samples < 1 || p->samples > PYR_MOTION_BLUR_MOST_SAMPLES) return fail(PYR_ERR_INVALID_ARGUMENT, name + "samples must be 1..64");
    if (p->max_radius < 1 || p->max_radius > PYR_MOTION_BLUR_MOST_RADIUS) return fail(PYR_ERR_INVALID_ARGUMENT, name + "max_radius must be 1..64");
    if (!(p->depth_softness > 0.0f) || !std::isfinite(p->depth_softness)) return fail(PYR_ERR_INVALID_ARGUMENT, name + "depth_softness must be finite and positive");
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return fail(PYR_ERR_INVALID_ARGUMENT, name + "reserved must be 0");
    return PYR_OK;
}

// What the three lens blur entries refuse of their parameters before a device is looked for (`what`: params or blur_params).
int check_lens_blur_params(const PyrLensBlurParams* p, const char* what) {
    const std::string name = std::string(what) + "->";
    if (!p) return fail(PYR_ERR_INVALID_ARGUMENT, std::string("null argument: ") + what);
    if (!(p->focus_distance > 0.0f) || !std::isfinite(p->focus_distance)) return fail(PYR_ERR_INVALID_ARGUMENT, name + "focus_distance must be finite and positive");
    if (!(p->aperture >= 0.0f) || !std::isfinite(p->aperture)) return fail(PYR_ERR_INVALID_ARGUMENT, name + "aperture must be finite and not negative");
    if (!(p->view_plane > 0.0f) || !std::isfinite(p->view_plane)) return fail(PYR_ERR_INVALID_ARGUMENT, name + "view_plane must be finite and positive");
    if (p->max_radius < 1 || p->max_radius > PYR_LENS_BLUR_MOST_RADIUS) return fail(PYR_ERR_INVALID_ARGUMENT, name + "max_radius must be 1..16");
    if (!(p->depth_tolerance >= 0.0f && p->depth_tolerance < 1.0f)) return fail(PYR_ERR_INVALID_ARGUMENT, name + "depth_tolerance must be in [0, 1)");
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return fail(PYR_ERR_INVALID_ARGUMENT, name + "reserved must be 0");
    return PYR_OK;
}

// What the three glare entries refuse of their parameters before a device is looked for (`what`: params or glare_params).
int check_glare_params(const PyrGlareParams* p, const char* what) {
    const std::string name = std::string(what) + "->";
    if (!p) return fail(PYR_ERR_INVALID_ARGUMENT, std::string("null argument: ") + what);
    if (!(p->strength > 0.0f && p->strength <= 1.0f)) return fail(PYR_ERR_INVALID_ARGUMENT, name + "strength must be in (0, 1]");
    if (p->levels < 1 || p->levels > PYR_GLARE_MOST_LEVELS) return fail(PYR_ERR_INVALID_ARGUMENT, name + "levels must be 1..12");
    if (!(p->threshold >= 0.0f) || !std::isfinite(p->threshold)) return fail(PYR_ERR_INVALID_ARGUMENT, name + "threshold must be finite and not negative");
    if (!(p->falloff > 0.0f && p->falloff <= 4.0f)) return fail(PYR_ERR_INVALID_ARGUMENT, name + "falloff must be in (0, 4]");
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0 || p->reserved[3] != 0) return fail(PYR_ERR_INVALID_ARGUMENT, name + "reserved must be 0");
    return PYR_OK;
}

// What the three upsample entries refuse of their parameters before a device is looked for (`what`: params or upsample_params).
// The floor and the gain are read only with the albedo pair, so only then are they held to their ranges.
int check_upsample_params(const PyrUpsampleParams* p, const char* what, bool with_albedo) {
    const std::string name = std::string(what) + "->";
    if (!p) return fail(PYR_ERR_INVALID_ARGUMENT, std::string("null argument: ") + what);
    if (p->radius < 1 || p->radius > PYR_UPSAMPLE_MOST_RADIUS) return fail(PYR_ERR_INVALID_ARGUMENT, name + "radius must be 1..3");
    if (p->flags & ~PYR_UPSAMPLE_MATCH_MATERIAL) return fail(PYR_ERR_INVALID_ARGUMENT, name + "flags has an unknown bit: PYR_UPSAMPLE_MATCH_MATERIAL or 0");
    if (with_albedo && !(p->albedo_floor > 0.0f)) return fail(PYR_ERR_INVALID_ARGUMENT, name + "albedo_floor must be positive");
    if (with_albedo && !(p->max_gain >= 1.0f)) return fail(PYR_ERR_INVALID_ARGUMENT, name + "max_gain must be at least 1");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(PYR_ERR_INVALID_ARGUMENT, name + "reserved must be 0");
    return PYR_OK;
}
// What the three despeckle entries refuse of their parameters before a device is looked for (`what`: params or despeckle_params).
int check_despeckle_params(const PyrDespeckleParams* p, const char* what) {
    const std::string name = std::string(what) + "->";
    if (!p) return fail(PYR_ERR_INVALID_ARGUMENT, std::string("null argument: ") + what);
    if (p->radius < 1 || p->radius > PYR_DESPECKLE_MOST_RADIUS) return fail(PYR_ERR_INVALID_ARGUMENT, name + "radius must be 1..2");
    if (!(p->k > 0.0f) || !std::isfinite(p->k)) return fail(PYR_ERR_INVALID_ARGUMENT, name + "k must be finite and positive");
    if (!(p->relative >= 0.0f) || !std::isfinite(p->relative)) return fail(PYR_ERR_INVALID_ARGUMENT, name + "relative must be finite and not negative");
    if (!(p->floor > 0.0f) || !std::isfinite(p->floor)) return fail(PYR_ERR_INVALID_ARGUMENT, name + "floor must be finite and positive");
    if (p->flags != 0) return fail(PYR_ERR_INVALID_ARGUMENT, name + "flags has an unknown bit: none is defined");
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return fail(PYR_ERR_INVALID_ARGUMENT, name + "reserved must be 0");
    return PYR_OK;
}
int check_upsample_scale(uint32_t scale) {
    if (scale < 2 || scale > PYR_UPSAMPLE_MOST_SCALE) return fail(PYR_ERR_INVALID_ARGUMENT, "scale must be 2..8");
    return PYR_OK;
}
// The size of the upsampled image: 2^32 - 1 pixels at the most, and neither side above 2^24, up to which the rule's f32 coordinates are exact.
int check_upsample_size(uint32_t low_width, uint32_t low_height, uint32_t scale) {
    const uint64_t width = (uint64_t)low_width * scale, height = (uint64_t)low_height * scale;
    if (width * height > kMaxImagePixels) return fail(PYR_ERR_UNSUPPORTED, "an upsampled image of more than 2^32 - 1 pixels");
    if (width > (1u << 24) || height > (1u << 24)) return fail(PYR_ERR_UNSUPPORTED, "an upsampled image with a side of more than 2^24 pixels");
    return PYR_OK;
}

// Variance, the two filter launches with the halves exchanged, the combine: everything on `stream`, every buffer on the current
// device; `work` holds three images of width * height * 3 floats (V, FA, FB).
int enqueue_denoise(const float* a, const float* b, const float* albedo, const PyrFeaturePixel* pixels, uint32_t width, uint32_t height, const PyrDenoiseParams* p,
                    float* work, float* out, float* error_out, hipStream_t stream) {
    const size_t floats = (size_t)width * height * 3;
    float *variance = work, *fa = work + floats, *fb = work + 2 * floats;
    int rc;
    if ((rc = launch_denoise_variance(a, b, width, height, variance, stream)) != PYR_OK) return rc;
    DenoiseLaunch L{};
    L.variance = variance;
    L.albedo = albedo, L.pixels = pixels;
    L.width = width, L.height = height, L.radius = p->radius, L.patch = p->patch;
    L.kk = p->k * p->k, L.epsilon = p->epsilon;
    L.albedo_div = 2.0f * (p->sigma_albedo * p->sigma_albedo), L.normal_div = 2.0f * (p->sigma_normal * p->sigma_normal), L.depth_div = 2.0f * (p->sigma_depth * p->sigma_depth);
    if (!(p->sigma_albedo > 0.0f)) L.albedo_div = 0.0f;
    if (!(p->sigma_normal > 0.0f)) L.normal_div = 0.0f;
    if (!(p->sigma_depth > 0.0f)) L.depth_div = 0.0f;
    L.weights_from = b, L.averaged = a, L.out = fa; // FA: a under the weights of b
    if ((rc = launch_denoise_filter(L, stream)) != PYR_OK) return rc;
    L.weights_from = a, L.averaged = b, L.out = fb;
    if ((rc = launch_denoise_filter(L, stream)) != PYR_OK) return rc;
    return launch_denoise_combine(fa, fb, (size_t)width * height, out, error_out, stream);
}

// The blur of `image` along `motion` into `out`, every buffer on the current device, enqueued on `stream`; the working memory is
// allocated and freed in stream order around the three launches.
int enqueue_motion_blur(const float* image, const PyrMotionPixel* motion, uint32_t width, uint32_t height, const PyrMotionBlurParams* p, float* out, hipStream_t stream) {
    return with_stream_memory(motion_blur_work_bytes(width, height, p->max_radius), stream, [&](void* work) {
        const MotionBlurLaunch L{image, motion, width, height, p->shutter, p->depth_softness, p->samples, p->max_radius, p->seed, (float*)work, out};
        return launch_motion_blur(L, stream);
    });
}

// The glare of `image` into `out`, both on the current device, enqueued on `stream`; the pyramid's levels are allocated and freed
// in stream order around the launches.
int enqueue_glare(const float* image, uint32_t width, uint32_t height, const PyrGlareParams* p, float* out, hipStream_t stream) {
    return with_stream_memory(glare_work_bytes(width, height, p->levels), stream, [&](void* work) {
        const GlareLaunch L{image, width, height, p->strength, p->threshold, p->falloff, p->levels, (float*)work, out};
        return launch_glare(L, stream);
    });
}

// The lens blur of `image` over the records `pixels` into `out` (kernels/lens_blur.hip): every buffer on the current device, one
// launch on `stream`, no working memory.
int enqueue_lens_blur(const float* image, const PyrFeaturePixel* pixels, uint32_t width, uint32_t height, const PyrLensBlurParams* p, float* out, hipStream_t stream) {
    const LensBlurLaunch L{image, pixels, width, height, p->focus_distance, p->aperture, p->view_plane, p->depth_tolerance, p->max_radius, out};
    return launch_lens_blur(L, stream);
}

// The upsampling of `low` to scale times its size into `out` (kernels/upsample.hip): every buffer on the current device, one launch
// on `stream`, no working memory. Either pair is null or given whole.
int enqueue_upsample(const float* low, const float* low_albedo, const PyrFeaturePixel* low_pixels, uint32_t low_width, uint32_t low_height, uint32_t scale,
                     const float* albedo, const PyrFeaturePixel* pixels, const PyrUpsampleParams* p, float* out, hipStream_t stream) {
    UpsampleLaunch L{};
    L.low = low, L.low_albedo = low_albedo, L.low_pixels = low_pixels;
    L.low_width = low_width, L.low_height = low_height, L.scale = scale;
    L.albedo = albedo, L.pixels = pixels;
    L.radius = p->radius;
    L.use_normal = p->sigma_normal > 0.0f, L.use_depth = p->sigma_depth > 0.0f, L.match_material = (p->flags & PYR_UPSAMPLE_MATCH_MATERIAL) != 0;
    L.normal_div = 2.0f * (p->sigma_normal * p->sigma_normal), L.depth_div = 2.0f * (p->sigma_depth * p->sigma_depth);
    L.albedo_floor = p->albedo_floor, L.max_gain = p->max_gain;
    L.out = out;
    return launch_upsample(L, stream);
}

// The firefly clamp of `a` and, when given, `b` (kernels/despeckle.hip): every buffer on the current device, the counts zeroed and
// one launch on `stream`, no working memory.
int enqueue_despeckle(const float* a, const float* b, uint32_t width, uint32_t height, const PyrDespeckleParams* p, float* a_out, float* b_out, float* removed_out,
                      uint32_t* counts_out, hipStream_t stream) {
    const DespeckleLaunch L{a, b, width, height, p->radius, p->k, p->relative, p->floor, a_out, b_out, removed_out, counts_out, 0u};
    return launch_despeckle(L, stream);
}

} // namespace pyr

namespace {

// A buffer as the checks name it.
struct Range {
    const void* at;
    uint64_t bytes;
    const char* name;
};
// The first of the named pointers that is null.
int check_given(std::initializer_list<Range> arguments) {
    for (const Range& a : arguments)
        if (!a.at) return fail(PYR_ERR_INVALID_ARGUMENT, std::string("null argument: ") + a.name);
    return PYR_OK;
}
int check_not_empty(uint32_t width, uint32_t height) {
    if (width == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "width: an empty image");
    if (height == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "height: an empty image");
    return PYR_OK;
}
// The extent of an image that is given as width and height. (The temporal resolve takes the two halves apart: its parameters and
// the alignment of its records are refused between them.)
int check_extent(uint32_t width, uint32_t height) {
    if (int bad = check_not_empty(width, height)) return bad;
    return check_image_size(width, height);
}

// The buffers of a frame and its history, as the reprojection and the temporal resolve take them.
int check_frame_buffers(const void* current, const void* motion, const void* history, const void* history_motion, const void* history_count, const void* params,
                        const void* out, const void* count_out) {
    if (int bad = check_given({{current, 0, "current"}, {motion, 0, "motion"}, {params, 0, "params"}, {out, 0, "out"}, {count_out, 0, "count_out"}})) return bad;
    const int given = (history != nullptr) + (history_motion != nullptr) + (history_count != nullptr);
    if (given != 0 && given != 3) return fail(PYR_ERR_INVALID_ARGUMENT, "history, history_motion and history_count are all null or all given");
    return PYR_OK;
}
int check_not_negative(float value, const char* field) {
    if (!(value >= 0.0f) || !std::isfinite(value)) return fail(PYR_ERR_INVALID_ARGUMENT, std::string("params->") + field + " must be finite and not negative");
    return PYR_OK;
}
int check_history_params(float depth_tolerance, float max_history) {
    if (int bad = check_not_negative(depth_tolerance, "depth_tolerance")) return bad;
    if (!(max_history >= 1.0f) || !std::isfinite(max_history)) return fail(PYR_ERR_INVALID_ARGUMENT, "params->max_history must be finite and at least 1");
    return PYR_OK;
}
int check_reserved(const uint32_t (&reserved)[2]) {
    if (reserved[0] != 0 || reserved[1] != 0) return fail(PYR_ERR_INVALID_ARGUMENT, "params->reserved must be 0");
    return PYR_OK;
}
int check_records_aligned(const void* motion_device, const void* history_motion_device) { // records are read as 16-byte vectors
    if ((((uintptr_t)motion_device | (uintptr_t)history_motion_device) & 15u) != 0)
        return fail(PYR_ERR_INVALID_ARGUMENT, "motion_device and history_motion_device must be 16-byte aligned");
    return PYR_OK;
}

// No output may lie over an input or over another output: the first pair that does, outputs in their order, is named. A range
// at nullptr is an optional buffer that was not given.
bool ranges_overlap(const Range& a, const Range& b) {
    const uint64_t a0 = (uint64_t)(uintptr_t)a.at, b0 = (uint64_t)(uintptr_t)b.at;
    return a.at && b.at && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}
int check_overlap(std::initializer_list<Range> outputs, std::initializer_list<Range> inputs) {
    for (const Range* a = outputs.begin(); a != outputs.end(); ++a) {
        for (const Range& b : inputs)
            if (ranges_overlap(*a, b)) return fail(PYR_ERR_INVALID_ARGUMENT, std::string(a->name) + " overlaps " + b.name);
        for (const Range* b = a + 1; b != outputs.end(); ++b)
            if (ranges_overlap(*a, *b)) return fail(PYR_ERR_INVALID_ARGUMENT, std::string(a->name) + " overlaps " + b->name);
    }
    return PYR_OK;
}

// The end of every entry's checks: what they refused, or else the device, which has to exist and becomes the current one.
int use_device(int refused, int device) {
    if (refused != PYR_OK) return refused;
    if (int bad = check_device(device)) return bad;
    HIP_TRY(hipSetDevice(device));
    return PYR_OK;
}

int check_develop_args(const PyrFilmDesc* film, const void* grains, const PyrDevelopParams* p, const void* rgb) {
    if (!film || !grains || !p || !rgb || !p->xyz_table) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    return PYR_OK;
}
int check_stats_args(const void* image, uint32_t width, uint32_t height, const void* out) {
    if (!image || !out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    return check_image_size(width, height);
}
int check_tonemap_args(const void* image, uint32_t width, uint32_t height, const PyrToneParams* t, const void* rgb) {
    if (!image || !t || !rgb) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    if (int bad = check_tone_operator(t->op)) return bad;
    if (!(t->exposure > 0.0f) || (t->op == PYR_TONE_REINHARD && !(t->white > 0.0f)))
        return fail(PYR_ERR_INVALID_ARGUMENT, "unresolved tone parameters: pyr_tone_resolve gives the exposure and the white point");
    return check_image_size(width, height);
}
int check_denoise_args(const void* a, const void* b, uint32_t width, uint32_t height, const PyrDenoiseParams* p, const void* out) {
    if (int bad = check_given({{a, 0, "a"}, {b, 0, "b"}, {out, 0, "out"}})) return bad;
    if (int bad = check_denoise_params(p)) return bad;
    return check_extent(width, height);
}
// Parameters before the extent.
int check_reproject_args(const void* current, const void* motion, const void* history, const void* history_motion, const void* history_count, uint32_t width,
                         uint32_t height, const PyrReprojectParams* p, const void* out, const void* count_out) {
    if (int bad = check_frame_buffers(current, motion, history, history_motion, history_count, p, out, count_out)) return bad;
    if (int bad = check_history_params(p->depth_tolerance, p->max_history)) return bad;
    if (int bad = check_reserved(p->reserved)) return bad;
    return check_extent(width, height);
}
// An empty image before the parameters; the size of the image is left to the entry, which refuses it after the alignment.
int check_temporal_args(const void* current, const void* motion, const void* history, const void* history_motion, const void* history_count, uint32_t width,
                        uint32_t height, const PyrTemporalParams* p, const void* out, const void* count_out) {
    if (int bad = check_frame_buffers(current, motion, history, history_motion, history_count, p, out, count_out)) return bad;
    if (int bad = check_not_empty(width, height)) return bad;
    if (int bad = check_history_params(p->depth_tolerance, p->max_history)) return bad;
    if (p->radius < 1 || p->radius > PYR_TEMPORAL_MOST_RADIUS) return fail(PYR_ERR_INVALID_ARGUMENT, "params->radius must be 1..3");
    if (int bad = check_not_negative(p->gamma, "gamma")) return bad;
    if (int bad = check_not_negative(p->noise_scale, "noise_scale")) return bad;
    if (int bad = check_not_negative(p->response, "response")) return bad;
    return check_reserved(p->reserved);
}
int check_motion_blur_args(const void* image, const void* motion, uint32_t width, uint32_t height, const PyrMotionBlurParams* p, const void* out) {
    if (int bad = check_given({{image, 0, "image"}, {motion, 0, "motion"}, {out, 0, "out"}})) return bad;
    if (int bad = check_motion_blur_params(p, "params")) return bad;
    return check_extent(width, height);
}
int check_lens_blur_args(const void* image, const void* pixels, uint32_t width, uint32_t height, const PyrLensBlurParams* p, const void* out) {
    if (int bad = check_given({{image, 0, "image"}, {pixels, 0, "pixels"}, {out, 0, "out"}})) return bad;
    if (int bad = check_lens_blur_params(p, "params")) return bad;
    return check_extent(width, height);
}

int check_glare_args(const void* image, uint32_t width, uint32_t height, const PyrGlareParams* p, const void* out) {
    if (int bad = check_given({{image, 0, "image"}, {p, 0, "params"}, {out, 0, "out"}})) return bad;
    if (int bad = check_not_empty(width, height)) return bad;
    return check_glare_params(p, "params");
}

// Half a pair before the extent, the scale and the parameters; the size is left to the entries, which refuse it last.
int check_upsample_args(const void* low, const void* low_albedo, const void* low_pixels, uint32_t low_width, uint32_t low_height, uint32_t scale, const void* albedo,
                        const void* pixels, const PyrUpsampleParams* p, const void* out) {
    if (int bad = check_given({{low, 0, "low"}, {p, 0, "params"}, {out, 0, "out"}})) return bad;
    if ((low_albedo != nullptr) != (albedo != nullptr)) return fail(PYR_ERR_INVALID_ARGUMENT, "low_albedo and albedo are both null or both given");
    if ((low_pixels != nullptr) != (pixels != nullptr)) return fail(PYR_ERR_INVALID_ARGUMENT, "low_pixels and pixels are both null or both given");
    if (low_width == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "low_width: an empty image");
    if (low_height == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "low_height: an empty image");
    if (int bad = check_upsample_scale(scale)) return bad;
    return check_upsample_params(p, "params", albedo != nullptr);
}

// Nulls, half a pair, the extent and its size, the parameters, then the overlaps: `names` are those of a, b, a_out, b_out,
// removed_out and counts_out as the entry calls them.
int check_despeckle_args(const void* a, const void* b, uint32_t width, uint32_t height, const PyrDespeckleParams* p, const void* a_out, const void* b_out,
                         const void* removed_out, const void* counts_out, const char* const (&names)[6]) {
    if (int bad = check_given({{a, 0, names[0]}, {p, 0, "params"}, {a_out, 0, names[2]}})) return bad;
    if ((b != nullptr) != (b_out != nullptr)) return fail(PYR_ERR_INVALID_ARGUMENT, std::string(names[1]) + " and " + names[3] + " are both null or both given");
    if (int bad = check_extent(width, height)) return bad;
    if (int bad = check_despeckle_params(p, "params")) return bad;
    const uint64_t bytes = (uint64_t)width * height * 12;
    return check_overlap({{a_out, bytes, names[2]}, {b_out, bytes, names[3]}, {removed_out, bytes, names[4]}, {counts_out, 8, names[5]}}, {{a, bytes, names[0]}, {b, bytes, names[1]}});
}

// A development with its small per-wavelength tables copied for the call: allocated in stream order, filled, handed to `launch`
// in the launch record that reads them, freed in stream order behind what `launch` enqueued.
template <class Launch>
int develop_with_call_tables(const PyrFilmDesc* film, const PyrDevelopParams* p, hipStream_t stream, Launch launch) {
    const size_t bytes = develop_table_floats(p) * sizeof(float);
    return with_stream_memory(bytes, stream, [&](void* tables) {
        std::vector<float> host;
        const DevelopLaunch D = develop_launch(film, p, (float*)tables, host);
        const hipError_t copied = hipMemcpy(tables, host.data(), bytes, hipMemcpyHostToDevice); // synchronous: `host` dies with this frame
        if (copied != hipSuccess) return hip_fail(copied, "hipMemcpy(development tables)");
        return launch(D);
    });
}

int develop_common(const PyrFilmDesc* film, const PyrGrain* grains, const PyrDevelopParams* p, uint8_t* rgb, hipStream_t stream) {
    if (int bad = check_develop_params(p)) return bad;
    return develop_with_call_tables(film, p, stream, [&](DevelopLaunch D) {
        D.grains = grains;
        D.rgb_out = rgb;
        return develop_uses_wave(D) ? launch_develop_wave(D, stream) : launch_develop(D, stream);
    });
}

// Development to a linear image, as develop_common does for the 8-bit image.
int develop_linear_common(const PyrFilmDesc* film, const PyrGrain* grains, const PyrGrain* grains_b, const PyrDevelopParams* p, uint32_t space, float* out,
                          hipStream_t stream) {
    return develop_with_call_tables(film, p, stream, [&](DevelopLaunch D) {
        D.grains = grains;
        D.grains_b = grains_b;
        return launch_develop_linear(LinearLaunch{D, out, space}, stream);
    });
}

int enqueue_image_stats(const float* image, uint32_t width, uint32_t height, PyrImageStats* out, hipStream_t stream) {
    return launch_image_stats(image, (size_t)width * height, out, stream);
}

int enqueue_tonemap(const float* image, uint32_t width, uint32_t height, const PyrToneParams* resolved, uint8_t* rgb, hipStream_t stream) {
    const ToneLaunch T{image, rgb, (size_t)width * height, resolved->op, resolved->exposure, resolved->white};
    return launch_tonemap(T, stream);
}

// enqueue_denoise with its three working images allocated and freed in stream order around it.
int enqueue_image_denoise(const float* a, const float* b, const float* albedo, const PyrFeaturePixel* pixels, uint32_t width, uint32_t height,
                          const PyrDenoiseParams* p, float* out, float* error_out, hipStream_t stream) {
    return with_stream_memory((size_t)width * height * 9 * sizeof(float), stream,
                              [&](void* work) { return enqueue_denoise(a, b, albedo, pixels, width, height, p, (float*)work, out, error_out, stream); });
}

int enqueue_reproject(const float* current, const PyrMotionPixel* motion, const float* history, const PyrMotionPixel* history_motion, const float* history_count,
                      uint32_t width, uint32_t height, const PyrReprojectParams* p, float* out, float* count_out, hipStream_t stream) {
    const ReprojectLaunch L{current, motion, history, history_motion, history_count, width, height, p->depth_tolerance, p->max_history, out, count_out};
    return launch_reproject(L, stream);
}

int enqueue_temporal(const float* current, const PyrMotionPixel* motion, const float* noise, const float* history, const PyrMotionPixel* history_motion,
                     const float* history_count, uint32_t width, uint32_t height, const PyrTemporalParams* p, float* out, float* count_out, float* clip_out,
                     hipStream_t stream) {
    const TemporalLaunch L{current, motion, noise, history, history_motion, history_count, width, height, p->depth_tolerance, p->max_history, p->radius,
                           p->gamma, p->noise_scale, p->response, out, count_out, clip_out};
    return launch_temporal(L, stream);
}

float upper_edge(uint32_t bin) {
    const uint32_t bits = (bin + 889u) << 20;
    float f;
    std::memcpy(&f, &bits, sizeof(f));
    return f;
}
uint32_t percentile_bin(const PyrImageStats* s, float percentile) {
    uint64_t target = (uint64_t)std::ceil((double)percentile * (double)s->lit);
    target = std::min<uint64_t>(std::max<uint64_t>(target, 1), s->lit);
    uint64_t seen = 0;
    for (uint32_t k = 0; k < 256; ++k) {
        seen += s->histogram[k];
        if (seen >= target) return k;
    }
    return 255; // a histogram that holds fewer than `lit` pixels
}

} // namespace

extern "C" {

int pyr_film_develop_device(const PyrFilmDesc* film, const PyrGrain* grains_device, const PyrDevelopParams* params, uint8_t* rgb_device, int device,
                            void* hip_stream) {
    if (int bad = use_device(check_develop_args(film, grains_device, params, rgb_device), device)) return bad;
    return develop_common(film, grains_device, params, rgb_device, (hipStream_t)hip_stream);
}

int pyr_film_develop(const PyrFilmDesc* film, const PyrGrain* grains, const PyrDevelopParams* params, uint8_t* rgb_out, int device) {
    if (int bad = use_device(check_develop_args(film, grains, params, rgb_out), device)) return bad;
    const size_t pixels = (size_t)film->width * film->height;
    Staging S;
    return S.finish(develop_common, film, S.in(grains, pixels * film->bins * sizeof(PyrGrain)), params, S.out(rgb_out, pixels * 3), nullptr);
}

int pyr_film_develop_linear_device(const PyrFilmDesc* film, const PyrGrain* grains_device, const PyrGrain* grains_b_device, const PyrDevelopParams* params,
                                   uint32_t space, float* out_device, int device, void* hip_stream) {
    if (int bad = use_device(check_linear_args(film, grains_device, params, space, out_device), device)) return bad;
    return develop_linear_common(film, grains_device, grains_b_device, params, space, out_device, (hipStream_t)hip_stream);
}

int pyr_film_develop_linear(const PyrFilmDesc* film, const PyrGrain* grains, const PyrGrain* grains_b, const PyrDevelopParams* params, uint32_t space, float* out,
                            int device) {
    if (int bad = use_device(check_linear_args(film, grains, params, space, out), device)) return bad;
    const size_t pixels = (size_t)film->width * film->height, film_bytes = pixels * film->bins * sizeof(PyrGrain);
    Staging S;
    return S.finish(develop_linear_common, film, S.in(grains, film_bytes), S.in(grains_b, film_bytes), params, space, S.out(out, pixels * 3 * sizeof(float)), nullptr);
}

int pyr_image_stats_device(const float* linear_srgb_device, uint32_t width, uint32_t height, PyrImageStats* out_device, int device, void* hip_stream) {
    if (int bad = use_device(check_stats_args(linear_srgb_device, width, height, out_device), device)) return bad;
    return enqueue_image_stats(linear_srgb_device, width, height, out_device, (hipStream_t)hip_stream);
}

int pyr_image_stats(const float* linear_srgb, uint32_t width, uint32_t height, PyrImageStats* out, int device) {
    if (int bad = use_device(check_stats_args(linear_srgb, width, height, out), device)) return bad;
    Staging S;
    return S.finish(enqueue_image_stats, S.in(linear_srgb, (size_t)width * height * 3 * sizeof(float)), width, height, S.out(out, sizeof(PyrImageStats)), nullptr);
}

int pyr_tone_resolve(const PyrImageStats* stats, const PyrToneParams* tone, float* exposure_out, float* white_out) {
    if (!tone || !exposure_out || !white_out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    if (int bad = check_tone_params(tone)) return bad;
    if (tone_needs_stats(tone) && !stats) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: an automatic exposure or white point needs the statistics");
    float exposure = tone->exposure;
    if (!(exposure > 0.0f)) exposure = stats->lit ? tone->key / upper_edge(percentile_bin(stats, tone->percentile)) : 1.0f;
    float white = 1.0f;
    if (tone->op == PYR_TONE_REINHARD) {
        if (tone->white > 0.0f)
            white = tone->white;
        else if (stats->lit)
            white = exposure * upper_edge(percentile_bin(stats, tone->white_percentile));
    }
    *exposure_out = exposure;
    *white_out = white;
    return PYR_OK;
}

int pyr_image_tonemap_device(const float* linear_srgb_device, uint32_t width, uint32_t height, const PyrToneParams* resolved, uint8_t* rgb_device, int device,
                             void* hip_stream) {
    if (int bad = use_device(check_tonemap_args(linear_srgb_device, width, height, resolved, rgb_device), device)) return bad;
    return enqueue_tonemap(linear_srgb_device, width, height, resolved, rgb_device, (hipStream_t)hip_stream);
}

int pyr_image_tonemap(const float* linear_srgb, uint32_t width, uint32_t height, const PyrToneParams* resolved, uint8_t* rgb_out, int device) {
    if (int bad = use_device(check_tonemap_args(linear_srgb, width, height, resolved, rgb_out), device)) return bad;
    const size_t pixels = (size_t)width * height;
    Staging S;
    return S.finish(enqueue_tonemap, S.in(linear_srgb, pixels * 3 * sizeof(float)), width, height, resolved, S.out(rgb_out, pixels * 3), nullptr);
}

int pyr_image_denoise_device(const float* a_device, const float* b_device, const float* albedo_device, const PyrFeaturePixel* pixels_device, uint32_t width,
                             uint32_t height, const PyrDenoiseParams* params, float* out_device, float* error_out_device, int device, void* hip_stream) {
    if (int bad = use_device(check_denoise_args(a_device, b_device, width, height, params, out_device), device)) return bad;
    return enqueue_image_denoise(a_device, b_device, albedo_device, pixels_device, width, height, params, out_device, error_out_device, (hipStream_t)hip_stream);
}

int pyr_image_denoise(const float* a, const float* b, const float* albedo, const PyrFeaturePixel* pixels, uint32_t width, uint32_t height,
                      const PyrDenoiseParams* params, float* out, float* error_out, int device) {
    if (int bad = use_device(check_denoise_args(a, b, width, height, params, out), device)) return bad;
    const size_t count = (size_t)width * height, image_bytes = count * 3 * sizeof(float);
    Staging S;
    return S.finish(enqueue_image_denoise, S.in(a, image_bytes), S.in(b, image_bytes), S.in(albedo, image_bytes), S.in(pixels, count * sizeof(PyrFeaturePixel)), width,
                    height, params, S.out(out, image_bytes), S.out(error_out, image_bytes), nullptr);
}

int pyr_image_reproject_device(const float* current_device, const PyrMotionPixel* motion_device, const float* history_device,
                               const PyrMotionPixel* history_motion_device, const float* history_count_device, uint32_t width, uint32_t height,
                               const PyrReprojectParams* params, float* out_device, float* count_out_device, int device, void* hip_stream) {
    if (int bad = check_records_aligned(motion_device, history_motion_device)) return bad; // here before anything else
    const int rc = check_reproject_args(current_device, motion_device, history_device, history_motion_device, history_count_device, width, height, params, out_device, count_out_device);
    if (int bad = use_device(rc, device)) return bad;
    return enqueue_reproject(current_device, motion_device, history_device, history_motion_device, history_count_device, width, height, params, out_device,
                             count_out_device, (hipStream_t)hip_stream);
}

int pyr_image_reproject(const float* current, const PyrMotionPixel* motion, const float* history, const PyrMotionPixel* history_motion, const float* history_count,
                        uint32_t width, uint32_t height, const PyrReprojectParams* params, float* out, float* count_out, int device) {
    if (int bad = use_device(check_reproject_args(current, motion, history, history_motion, history_count, width, height, params, out, count_out), device)) return bad;
    const size_t count = (size_t)width * height, image_bytes = count * 3 * sizeof(float), record_bytes = count * sizeof(PyrMotionPixel);
    Staging S;
    return S.finish(enqueue_reproject, S.in(current, image_bytes), S.in(motion, record_bytes), S.in(history, image_bytes), S.in(history_motion, record_bytes),
                    S.in(history_count, count * sizeof(float)), width, height, params, S.out(out, image_bytes), S.out(count_out, count * sizeof(float)), nullptr);
}

int pyr_image_temporal_resolve_device(const float* current_device, const PyrMotionPixel* motion_device, const float* noise_device, const float* history_device,
                                      const PyrMotionPixel* history_motion_device, const float* history_count_device, uint32_t width, uint32_t height,
                                      const PyrTemporalParams* params, float* out_device, float* count_out_device, float* clip_out_device, int device,
                                      void* hip_stream) {
    int rc = check_temporal_args(current_device, motion_device, history_device, history_motion_device, history_count_device, width, height, params, out_device, count_out_device);
    if (rc != PYR_OK || (rc = check_records_aligned(motion_device, history_motion_device)) != PYR_OK) return rc; // here after the shared checks
    if ((rc = check_image_size(width, height)) != PYR_OK) return rc; // before the byte counts below are formed
    const uint64_t pixels = (uint64_t)width * height, records = pixels * sizeof(PyrMotionPixel);
    rc = check_overlap({{out_device, pixels * 12, "out_device"}, {count_out_device, pixels * 4, "count_out_device"}, {clip_out_device, pixels * 4, "clip_out_device"}},
                       {{current_device, pixels * 12, "current_device"}, {motion_device, records, "motion_device"}, {noise_device, pixels * 12, "noise_device"},
                        {history_device, pixels * 12, "history_device"}, {history_motion_device, records, "history_motion_device"},
                        {history_count_device, pixels * 4, "history_count_device"}});
    if (int bad = use_device(rc, device)) return bad;
    return enqueue_temporal(current_device, motion_device, noise_device, history_device, history_motion_device, history_count_device, width, height, params, out_device,
                            count_out_device, clip_out_device, (hipStream_t)hip_stream);
}

int pyr_image_temporal_resolve(const float* current, const PyrMotionPixel* motion, const float* noise, const float* history, const PyrMotionPixel* history_motion,
                               const float* history_count, uint32_t width, uint32_t height, const PyrTemporalParams* params, float* out, float* count_out,
                               float* clip_out, int device) {
    int rc = check_temporal_args(current, motion, history, history_motion, history_count, width, height, params, out, count_out);
    if (rc == PYR_OK) rc = check_image_size(width, height);
    if (int bad = use_device(rc, device)) return bad;
    const size_t count = (size_t)width * height, image_bytes = count * 3 * sizeof(float), record_bytes = count * sizeof(PyrMotionPixel);
    Staging S;
    return S.finish(enqueue_temporal, S.in(current, image_bytes), S.in(motion, record_bytes), S.in(noise, image_bytes), S.in(history, image_bytes),
                    S.in(history_motion, record_bytes), S.in(history_count, count * sizeof(float)), width, height, params, S.out(out, image_bytes),
                    S.out(count_out, count * sizeof(float)), S.out(clip_out, count * sizeof(float)), nullptr);
}

int pyr_image_motion_blur_device(const float* image_device, const PyrMotionPixel* motion_device, uint32_t width, uint32_t height, const PyrMotionBlurParams* params,
                                 float* out_device, int device, void* hip_stream) {
    int rc = check_motion_blur_args(image_device, motion_device, width, height, params, out_device);
    if (rc != PYR_OK) return rc;
    if (((uintptr_t)motion_device & 15u) != 0) return fail(PYR_ERR_INVALID_ARGUMENT, "motion_device must be 16-byte aligned"); // records are read as 16-byte vectors
    const uint64_t pixels = (uint64_t)width * height;
    rc = check_overlap({{out_device, pixels * 12, "out_device"}}, {{image_device, pixels * 12, "image_device"}, {motion_device, pixels * sizeof(PyrMotionPixel), "motion_device"}});
    if (int bad = use_device(rc, device)) return bad;
    return enqueue_motion_blur(image_device, motion_device, width, height, params, out_device, (hipStream_t)hip_stream);
}

int pyr_image_motion_blur(const float* image, const PyrMotionPixel* motion, uint32_t width, uint32_t height, const PyrMotionBlurParams* params, float* out, int device) {
    if (int bad = use_device(check_motion_blur_args(image, motion, width, height, params, out), device)) return bad;
    const size_t count = (size_t)width * height, image_bytes = count * 3 * sizeof(float);
    Staging S;
    return S.finish(enqueue_motion_blur, S.in(image, image_bytes), S.in(motion, count * sizeof(PyrMotionPixel)), width, height, params, S.out(out, image_bytes), nullptr);
}

int pyr_image_lens_blur_device(const float* image_device, const PyrFeaturePixel* pixels_device, uint32_t width, uint32_t height, const PyrLensBlurParams* params,
                               float* out_device, int device, void* hip_stream) {
    int rc = check_lens_blur_args(image_device, pixels_device, width, height, params, out_device);
    if (rc != PYR_OK) return rc;
    if (((uintptr_t)pixels_device & 15u) != 0) return fail(PYR_ERR_INVALID_ARGUMENT, "pixels_device must be 16-byte aligned"); // records are read as 16-byte vectors
    const uint64_t pixels = (uint64_t)width * height;
    rc = check_overlap({{out_device, pixels * 12, "out_device"}}, {{image_device, pixels * 12, "image_device"}, {pixels_device, pixels * sizeof(PyrFeaturePixel), "pixels_device"}});
    if (int bad = use_device(rc, device)) return bad;
    return enqueue_lens_blur(image_device, pixels_device, width, height, params, out_device, (hipStream_t)hip_stream);
}

int pyr_image_lens_blur(const float* image, const PyrFeaturePixel* pixels, uint32_t width, uint32_t height, const PyrLensBlurParams* params, float* out, int device) {
    if (int bad = use_device(check_lens_blur_args(image, pixels, width, height, params, out), device)) return bad;
    const size_t count = (size_t)width * height, image_bytes = count * 3 * sizeof(float);
    Staging S;
    return S.finish(enqueue_lens_blur, S.in(image, image_bytes), S.in(pixels, count * sizeof(PyrFeaturePixel)), width, height, params, S.out(out, image_bytes), nullptr);
}

int pyr_image_glare_device(const float* image_device, uint32_t width, uint32_t height, const PyrGlareParams* params, float* out_device, int device, void* hip_stream) {
    if (int bad = check_glare_args(image_device, width, height, params, out_device)) return bad;
    // the overlap before the size; an image that is refused next for its size is taken as 2^32 pixels here, so that the byte counts fit 64 bits
    const uint64_t pixels = std::min<uint64_t>((uint64_t)width * height, kMaxImagePixels + 1);
    if (int bad = check_overlap({{out_device, pixels * 12, "out_device"}}, {{image_device, pixels * 12, "image_device"}})) return bad;
    if (int bad = use_device(check_image_size(width, height), device)) return bad;
    return enqueue_glare(image_device, width, height, params, out_device, (hipStream_t)hip_stream);
}

int pyr_image_glare(const float* image, uint32_t width, uint32_t height, const PyrGlareParams* params, float* out, int device) {
    int rc = check_glare_args(image, width, height, params, out);
    if (rc == PYR_OK) rc = check_image_size(width, height);
    if (int bad = use_device(rc, device)) return bad;
    const size_t image_bytes = (size_t)width * height * 3 * sizeof(float);
    Staging S;
    return S.finish(enqueue_glare, S.in(image, image_bytes), width, height, params, S.out(out, image_bytes), nullptr);
}

int pyr_image_upsample_device(const float* low_device, const float* low_albedo_device, const PyrFeaturePixel* low_pixels_device, uint32_t low_width,
                              uint32_t low_height, uint32_t scale, const float* albedo_device, const PyrFeaturePixel* pixels_device, const PyrUpsampleParams* params,
                              float* out_device, int device, void* hip_stream) {
    int rc = check_upsample_args(low_device, low_albedo_device, low_pixels_device, low_width, low_height, scale, albedo_device, pixels_device, params, out_device);
    if (rc != PYR_OK) return rc;
    if ((((uintptr_t)low_pixels_device | (uintptr_t)pixels_device) & 15u) != 0) // records are read as 16-byte vectors
        return fail(PYR_ERR_INVALID_ARGUMENT, "low_pixels_device and pixels_device must be 16-byte aligned");
    if (int bad = use_device(check_upsample_size(low_width, low_height, scale), device)) return bad;
    return enqueue_upsample(low_device, low_albedo_device, low_pixels_device, low_width, low_height, scale, albedo_device, pixels_device, params, out_device,
                            (hipStream_t)hip_stream);
}

int pyr_image_upsample(const float* low, const float* low_albedo, const PyrFeaturePixel* low_pixels, uint32_t low_width, uint32_t low_height, uint32_t scale,
                       const float* albedo, const PyrFeaturePixel* pixels, const PyrUpsampleParams* params, float* out, int device) {
    int rc = check_upsample_args(low, low_albedo, low_pixels, low_width, low_height, scale, albedo, pixels, params, out);
    if (rc == PYR_OK) rc = check_upsample_size(low_width, low_height, scale);
    if (int bad = use_device(rc, device)) return bad;
    const size_t low_count = (size_t)low_width * low_height, count = low_count * scale * scale, pixel_bytes = 3 * sizeof(float);
    Staging S;
    return S.finish(enqueue_upsample, S.in(low, low_count * pixel_bytes), S.in(low_albedo, low_count * pixel_bytes), S.in(low_pixels, low_count * sizeof(PyrFeaturePixel)),
                    low_width, low_height, scale, S.in(albedo, count * pixel_bytes), S.in(pixels, count * sizeof(PyrFeaturePixel)), params, S.out(out, count * pixel_bytes),
                    nullptr);
}

int pyr_image_despeckle_device(const float* a_device, const float* b_device, uint32_t width, uint32_t height, const PyrDespeckleParams* params, float* a_out_device,
                               float* b_out_device, float* removed_out_device, uint32_t* counts_out_device, int device, void* hip_stream) {
    static const char* const names[6] = {"a_device", "b_device", "a_out_device", "b_out_device", "removed_out_device", "counts_out_device"};
    const int rc = check_despeckle_args(a_device, b_device, width, height, params, a_out_device, b_out_device, removed_out_device, counts_out_device, names);
    if (int bad = use_device(rc, device)) return bad;
    return enqueue_despeckle(a_device, b_device, width, height, params, a_out_device, b_out_device, removed_out_device, counts_out_device, (hipStream_t)hip_stream);
}

int pyr_image_despeckle(const float* a, const float* b, uint32_t width, uint32_t height, const PyrDespeckleParams* params, float* a_out, float* b_out,
                        float* removed_out, uint32_t* counts_out, int device) {
    static const char* const names[6] = {"a", "b", "a_out", "b_out", "removed_out", "counts_out"};
    if (int bad = use_device(check_despeckle_args(a, b, width, height, params, a_out, b_out, removed_out, counts_out, names), device)) return bad;
    const size_t image_bytes = (size_t)width * height * 3 * sizeof(float);
    Staging S;
    return S.finish(enqueue_despeckle, S.in(a, image_bytes), S.in(b, image_bytes), width, height, params, S.out(a_out, image_bytes), S.out(b_out, image_bytes),
                    S.out(removed_out, image_bytes), S.out(counts_out, 2 * sizeof(uint32_t)), nullptr);
}

} // extern "C"
