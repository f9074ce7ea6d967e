// image_ops.cpp -- the entry points of include/pyrite_gpu.h that take a device number and never see a scene: a film developed to
// an 8-bit or a linear image, an image's luminance statistics, its tone mapping, the denoising of two half images, the
// accumulation of linear images over frames along their motion records (plain, and with the history clipped to the current
// frame's neighbourhood: the temporal resolve), the motion blur of one along them. What a
// progressive session does with its own film through the same checks and launches (session.cpp) is declared in image_internal.h.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "image_internal.h"

using namespace pyr;

namespace {

constexpr uint64_t kMaxImagePixels = 0xFFFFFFFFull; // PyrImageStats counts in 32 bits
bool percentile_ok(float p) { return p > 0.0f && p <= 1.0f; }

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
    D.step_size = p->step_size;
    D.xyz_scale = p->xyz_scale;
    D.sample_count = p->sample_count;
    D.filter = p->filter ? tables : nullptr;
    D.white_div = p->white_div ? tables + n : nullptr;
    D.white_mul = p->white_div ? tables + 2 * n : nullptr;
    D.xyz_table = tables + 3 * n;
    D.xyz_count = p->xyz_count;
    D.xyz_min = p->xyz_min;
    D.xyz_max = p->xyz_max;
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
    if (t->op != PYR_TONE_CLIP && t->op != PYR_TONE_REINHARD) return fail(PYR_ERR_INVALID_ARGUMENT, "unknown tone operator: PYR_TONE_CLIP or PYR_TONE_REINHARD");
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

} // namespace pyr

namespace {

// What pyr_image_tonemap refuses.
int check_resolved_tone(const PyrToneParams* t) {
    if (t->op != PYR_TONE_CLIP && t->op != PYR_TONE_REINHARD) return fail(PYR_ERR_INVALID_ARGUMENT, "unknown tone operator: PYR_TONE_CLIP or PYR_TONE_REINHARD");
    if (!(t->exposure > 0.0f) || (t->op == PYR_TONE_REINHARD && !(t->white > 0.0f)))
        return fail(PYR_ERR_INVALID_ARGUMENT, "unresolved tone parameters: pyr_tone_resolve gives the exposure and the white point");
    return PYR_OK;
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

// A development with its small per-wavelength tables copied for the call: allocated in stream order, filled, handed to `launch`
// in the launch record that reads them, freed in stream order behind what `launch` enqueued. A failed copy frees the tables and
// reports the copy; a failed launch is reported before a failed free; the wait, where the caller asks for one, comes last.
template <class Launch>
int develop_with_call_tables(const PyrFilmDesc* film, const PyrDevelopParams* p, hipStream_t stream, bool blocking, Launch launch) {
    float* tables = nullptr;
    const size_t bytes = develop_table_floats(p) * sizeof(float);
    HIP_TRY(hipMallocAsync((void**)&tables, bytes, stream));
    std::vector<float> host;
    const DevelopLaunch D = develop_launch(film, p, tables, host);
    const hipError_t copied = hipMemcpy(tables, host.data(), bytes, hipMemcpyHostToDevice); // synchronous: `host` dies with this frame
    if (copied != hipSuccess) {
        (void)hipFreeAsync(tables, stream);
        return hip_fail(copied, "hipMemcpy(development tables)");
    }
    const int rc = launch(D);
    const hipError_t freed = hipFreeAsync(tables, stream);
    if (rc != PYR_OK) return rc;
    if (freed != hipSuccess) return hip_fail(freed, "hipFreeAsync");
    if (blocking) HIP_TRY(hipStreamSynchronize(stream));
    return PYR_OK;
}

int develop_common(const PyrFilmDesc* film, const PyrGrain* grains_device, const PyrDevelopParams* p, uint8_t* rgb_device, hipStream_t stream, bool blocking) {
    if (int bad = check_develop_params(p)) return bad;
    return develop_with_call_tables(film, p, stream, blocking, [&](DevelopLaunch D) {
        D.grains = grains_device;
        D.rgb_out = rgb_device;
        return develop_uses_wave(D) ? launch_develop_wave(D, stream) : launch_develop(D, stream);
    });
}

// Development to a linear image, as develop_common does for the 8-bit image.
int develop_linear_common(const PyrFilmDesc* film, const PyrGrain* grains_device, const PyrGrain* grains_b_device, const PyrDevelopParams* p, uint32_t space,
                          float* out_device, hipStream_t stream, bool blocking) {
    return develop_with_call_tables(film, p, stream, blocking, [&](DevelopLaunch D) {
        D.grains = grains_device;
        D.grains_b = grains_b_device;
        return launch_develop_linear(LinearLaunch{D, out_device, space}, stream);
    });
}

int check_denoise_args(const void* a, const void* b, uint32_t width, uint32_t height, const PyrDenoiseParams* p, const void* out) {
    if (!a) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: a");
    if (!b) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: b");
    if (!out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: out");
    if (int bad = check_denoise_params(p)) return bad;
    if (width == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "width: an empty image");
    if (height == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "height: an empty image");
    return check_image_size(width, height);
}

// What both reproject entries refuse before a device is looked for.
int check_reproject_args(const void* current, const void* motion, const void* history, const void* history_motion, const void* history_count, uint32_t width,
                         uint32_t height, const PyrReprojectParams* p, const void* out, const void* count_out) {
    if (!current) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: current");
    if (!motion) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: motion");
    if (!p) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: params");
    if (!out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: out");
    if (!count_out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: count_out");
    const int given = (history != nullptr) + (history_motion != nullptr) + (history_count != nullptr);
    if (given != 0 && given != 3) return fail(PYR_ERR_INVALID_ARGUMENT, "history, history_motion and history_count are all null or all given");
    if (!(p->depth_tolerance >= 0.0f) || !std::isfinite(p->depth_tolerance)) return fail(PYR_ERR_INVALID_ARGUMENT, "params->depth_tolerance must be finite and not negative");
    if (!(p->max_history >= 1.0f) || !std::isfinite(p->max_history)) return fail(PYR_ERR_INVALID_ARGUMENT, "params->max_history must be finite and at least 1");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(PYR_ERR_INVALID_ARGUMENT, "params->reserved must be 0");
    if (width == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "width: an empty image");
    if (height == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "height: an empty image");
    return check_image_size(width, height);
}

// What both temporal resolve entries refuse before a device is looked for.
int check_temporal_args(const void* current, const void* motion, const void* history, const void* history_motion, const void* history_count, uint32_t width,
                        uint32_t height, const PyrTemporalParams* p, const void* out, const void* count_out) {
    if (!current) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: current");
    if (!motion) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: motion");
    if (!p) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: params");
    if (!out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: out");
    if (!count_out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: count_out");
    const int given = (history != nullptr) + (history_motion != nullptr) + (history_count != nullptr);
    if (given != 0 && given != 3) return fail(PYR_ERR_INVALID_ARGUMENT, "history, history_motion and history_count are all null or all given");
    if (width == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "width: an empty image");
    if (height == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "height: an empty image");
    if (!(p->depth_tolerance >= 0.0f) || !std::isfinite(p->depth_tolerance)) return fail(PYR_ERR_INVALID_ARGUMENT, "params->depth_tolerance must be finite and not negative");
    if (!(p->max_history >= 1.0f) || !std::isfinite(p->max_history)) return fail(PYR_ERR_INVALID_ARGUMENT, "params->max_history must be finite and at least 1");
    if (p->radius < 1 || p->radius > PYR_TEMPORAL_MOST_RADIUS) return fail(PYR_ERR_INVALID_ARGUMENT, "params->radius must be 1..3");
    if (!(p->gamma >= 0.0f) || !std::isfinite(p->gamma)) return fail(PYR_ERR_INVALID_ARGUMENT, "params->gamma must be finite and not negative");
    if (!(p->noise_scale >= 0.0f) || !std::isfinite(p->noise_scale)) return fail(PYR_ERR_INVALID_ARGUMENT, "params->noise_scale must be finite and not negative");
    if (!(p->response >= 0.0f) || !std::isfinite(p->response)) return fail(PYR_ERR_INVALID_ARGUMENT, "params->response must be finite and not negative");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(PYR_ERR_INVALID_ARGUMENT, "params->reserved must be 0");
    return PYR_OK;
}

} // namespace

namespace pyr {

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

// The blur of `image` along `motion` into `out`, every buffer on the current device, enqueued on `stream`; the working memory is
// allocated and freed in stream order around the three launches.
int enqueue_motion_blur(const float* image, const PyrMotionPixel* motion, uint32_t width, uint32_t height, const PyrMotionBlurParams* p, float* out, hipStream_t stream) {
    float* work = nullptr;
    HIP_TRY(hipMallocAsync((void**)&work, motion_blur_work_bytes(width, height, p->max_radius), stream));
    const MotionBlurLaunch L{image, motion, width, height, p->shutter, p->depth_softness, p->samples, p->max_radius, p->seed, work, out};
    const int rc = launch_motion_blur(L, stream);
    const hipError_t freed = hipFreeAsync(work, stream);
    if (rc != PYR_OK) return rc;
    if (freed != hipSuccess) return hip_fail(freed, "hipFreeAsync");
    return PYR_OK;
}

} // namespace pyr

namespace {

// What both image entries of the motion blur refuse before a device is looked for.
int check_motion_blur_args(const void* image, const void* motion, uint32_t width, uint32_t height, const PyrMotionBlurParams* p, const void* out) {
    if (!image) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: image");
    if (!motion) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: motion");
    if (!out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument: out");
    if (int bad = check_motion_blur_params(p, "params")) return bad;
    if (width == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "width: an empty image");
    if (height == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "height: an empty image");
    return check_image_size(width, height);
}

bool ranges_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uint64_t a0 = (uint64_t)(uintptr_t)a, b0 = (uint64_t)(uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

} // namespace

extern "C" {

int pyr_image_motion_blur_device(const float* image_device, const PyrMotionPixel* motion_device, uint32_t width, uint32_t height, const PyrMotionBlurParams* params,
                                 float* out_device, int device, void* hip_stream) {
    int rc = check_motion_blur_args(image_device, motion_device, width, height, params, out_device);
    if (rc != PYR_OK) return rc;
    if (((uintptr_t)motion_device & 15u) != 0) return fail(PYR_ERR_INVALID_ARGUMENT, "motion_device must be 16-byte aligned"); // records are read as 16-byte vectors
    const uint64_t pixels = (uint64_t)width * height;
    if (ranges_overlap(out_device, pixels * 12, image_device, pixels * 12)) return fail(PYR_ERR_INVALID_ARGUMENT, "out_device overlaps image_device");
    if (ranges_overlap(out_device, pixels * 12, motion_device, pixels * sizeof(PyrMotionPixel))) return fail(PYR_ERR_INVALID_ARGUMENT, "out_device overlaps motion_device");
    if ((rc = check_device(device)) != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    return enqueue_motion_blur(image_device, motion_device, width, height, params, out_device, (hipStream_t)hip_stream);
}

int pyr_image_motion_blur(const float* image, const PyrMotionPixel* motion, uint32_t width, uint32_t height, const PyrMotionBlurParams* params, float* out, int device) {
    int rc = check_motion_blur_args(image, motion, width, height, params, out);
    if (rc != PYR_OK || (rc = check_device(device)) != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t count = (size_t)width * height, image_bytes = count * 3 * sizeof(float);
    DeviceBuffer image_dev, motion_dev, out_dev;
    if ((rc = image_dev.upload(image, image_bytes)) != PYR_OK || (rc = motion_dev.upload(motion, count * sizeof(PyrMotionPixel))) != PYR_OK) return rc;
    if ((rc = out_dev.alloc(image_bytes)) != PYR_OK) return rc;
    rc = enqueue_motion_blur((const float*)image_dev.ptr, (const PyrMotionPixel*)motion_dev.ptr, width, height, params, (float*)out_dev.ptr, nullptr);
    HIP_TRY(hipDeviceSynchronize()); // before the buffers above are freed, whatever happened
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipMemcpy(out, out_dev.ptr, image_bytes, hipMemcpyDeviceToHost));
    return PYR_OK;
}

int pyr_image_reproject_device(const float* current_device, const PyrMotionPixel* motion_device, const float* history_device,
                               const PyrMotionPixel* history_motion_device, const float* history_count_device, uint32_t width, uint32_t height,
                               const PyrReprojectParams* params, float* out_device, float* count_out_device, int device, void* hip_stream) {
    if ((((uintptr_t)motion_device | (uintptr_t)history_motion_device) & 15u) != 0) // records are read as 16-byte vectors
        return fail(PYR_ERR_INVALID_ARGUMENT, "motion_device and history_motion_device must be 16-byte aligned");
    int rc = check_reproject_args(current_device, motion_device, history_device, history_motion_device, history_count_device, width, height, params, out_device, count_out_device);
    if (rc != PYR_OK || (rc = check_device(device)) != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    const ReprojectLaunch L{current_device, motion_device, history_device, history_motion_device, history_count_device, width, height,
                            params->depth_tolerance, params->max_history, out_device, count_out_device};
    return launch_reproject(L, hip_stream);
}

int pyr_image_reproject(const float* current, const PyrMotionPixel* motion, const float* history, const PyrMotionPixel* history_motion, const float* history_count,
                        uint32_t width, uint32_t height, const PyrReprojectParams* params, float* out, float* count_out, int device) {
    int rc = check_reproject_args(current, motion, history, history_motion, history_count, width, height, params, out, count_out);
    if (rc != PYR_OK || (rc = check_device(device)) != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t count = (size_t)width * height, image_bytes = count * 3 * sizeof(float), record_bytes = count * sizeof(PyrMotionPixel);
    DeviceBuffer current_dev, motion_dev, history_dev, history_motion_dev, history_count_dev, out_dev, count_dev;
    if ((rc = current_dev.upload(current, image_bytes)) != PYR_OK || (rc = motion_dev.upload(motion, record_bytes)) != PYR_OK) return rc;
    if (history && ((rc = history_dev.upload(history, image_bytes)) != PYR_OK || (rc = history_motion_dev.upload(history_motion, record_bytes)) != PYR_OK ||
                    (rc = history_count_dev.upload(history_count, count * sizeof(float))) != PYR_OK))
        return rc;
    if ((rc = out_dev.alloc(image_bytes)) != PYR_OK || (rc = count_dev.alloc(count * sizeof(float))) != PYR_OK) return rc;
    const ReprojectLaunch L{(const float*)current_dev.ptr, (const PyrMotionPixel*)motion_dev.ptr, history ? (const float*)history_dev.ptr : nullptr,
                            history ? (const PyrMotionPixel*)history_motion_dev.ptr : nullptr, history ? (const float*)history_count_dev.ptr : nullptr, width, height,
                            params->depth_tolerance, params->max_history, (float*)out_dev.ptr, (float*)count_dev.ptr};
    rc = launch_reproject(L, nullptr);
    HIP_TRY(hipDeviceSynchronize()); // before the buffers above are freed, whatever happened
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipMemcpy(out, out_dev.ptr, image_bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(count_out, count_dev.ptr, count * sizeof(float), hipMemcpyDeviceToHost));
    return PYR_OK;
}

int pyr_image_temporal_resolve_device(const float* current_device, const PyrMotionPixel* motion_device, const float* noise_device, const float* history_device,
                                      const PyrMotionPixel* history_motion_device, const float* history_count_device, uint32_t width, uint32_t height,
                                      const PyrTemporalParams* params, float* out_device, float* count_out_device, float* clip_out_device, int device,
                                      void* hip_stream) {
    int rc = check_temporal_args(current_device, motion_device, history_device, history_motion_device, history_count_device, width, height, params, out_device, count_out_device);
    if (rc != PYR_OK) return rc;
    if ((((uintptr_t)motion_device | (uintptr_t)history_motion_device) & 15u) != 0) // records are read as 16-byte vectors
        return fail(PYR_ERR_INVALID_ARGUMENT, "motion_device and history_motion_device must be 16-byte aligned");
    if ((rc = check_image_size(width, height)) != PYR_OK) return rc; // before the byte counts below are formed
    const uint64_t pixels = (uint64_t)width * height;
    const struct {
        const void* at;
        uint64_t bytes;
        const char* name;
    } outputs[3] = {{out_device, pixels * 12, "out_device"}, {count_out_device, pixels * 4, "count_out_device"}, {clip_out_device, pixels * 4, "clip_out_device"}},
      inputs[6] = {{current_device, pixels * 12, "current_device"}, {motion_device, pixels * sizeof(PyrMotionPixel), "motion_device"},
                   {noise_device, pixels * 12, "noise_device"},     {history_device, pixels * 12, "history_device"},
                   {history_motion_device, pixels * sizeof(PyrMotionPixel), "history_motion_device"}, {history_count_device, pixels * 4, "history_count_device"}};
    for (int a = 0; a < 3; ++a) {
        if (!outputs[a].at) continue; // clip_out_device is optional
        for (int b = 0; b < 6; ++b)
            if (inputs[b].at && ranges_overlap(outputs[a].at, outputs[a].bytes, inputs[b].at, inputs[b].bytes))
                return fail(PYR_ERR_INVALID_ARGUMENT, std::string(outputs[a].name) + " overlaps " + inputs[b].name);
        for (int b = a + 1; b < 3; ++b)
            if (outputs[b].at && ranges_overlap(outputs[a].at, outputs[a].bytes, outputs[b].at, outputs[b].bytes))
                return fail(PYR_ERR_INVALID_ARGUMENT, std::string(outputs[a].name) + " overlaps " + outputs[b].name);
    }
    if ((rc = check_device(device)) != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    const TemporalLaunch L{current_device, motion_device, noise_device, history_device, history_motion_device, history_count_device, width, height,
                           params->depth_tolerance, params->max_history, params->radius, params->gamma, params->noise_scale, params->response,
                           out_device, count_out_device, clip_out_device};
    return launch_temporal(L, hip_stream);
}

int pyr_image_temporal_resolve(const float* current, const PyrMotionPixel* motion, const float* noise, const float* history, const PyrMotionPixel* history_motion,
                               const float* history_count, uint32_t width, uint32_t height, const PyrTemporalParams* params, float* out, float* count_out,
                               float* clip_out, int device) {
    int rc = check_temporal_args(current, motion, history, history_motion, history_count, width, height, params, out, count_out);
    if (rc != PYR_OK || (rc = check_image_size(width, height)) != PYR_OK || (rc = check_device(device)) != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t count = (size_t)width * height, image_bytes = count * 3 * sizeof(float), record_bytes = count * sizeof(PyrMotionPixel);
    DeviceBuffer current_dev, motion_dev, noise_dev, history_dev, history_motion_dev, history_count_dev, out_dev, count_dev, clip_dev;
    if ((rc = current_dev.upload(current, image_bytes)) != PYR_OK || (rc = motion_dev.upload(motion, record_bytes)) != PYR_OK) return rc;
    if (noise && (rc = noise_dev.upload(noise, image_bytes)) != PYR_OK) return rc;
    if (history && ((rc = history_dev.upload(history, image_bytes)) != PYR_OK || (rc = history_motion_dev.upload(history_motion, record_bytes)) != PYR_OK ||
                    (rc = history_count_dev.upload(history_count, count * sizeof(float))) != PYR_OK))
        return rc;
    if ((rc = out_dev.alloc(image_bytes)) != PYR_OK || (rc = count_dev.alloc(count * sizeof(float))) != PYR_OK) return rc;
    if (clip_out && (rc = clip_dev.alloc(count * sizeof(float))) != PYR_OK) return rc;
    const TemporalLaunch L{(const float*)current_dev.ptr, (const PyrMotionPixel*)motion_dev.ptr, noise ? (const float*)noise_dev.ptr : nullptr,
                           history ? (const float*)history_dev.ptr : nullptr, history ? (const PyrMotionPixel*)history_motion_dev.ptr : nullptr,
                           history ? (const float*)history_count_dev.ptr : nullptr, width, height, params->depth_tolerance, params->max_history, params->radius,
                           params->gamma, params->noise_scale, params->response, (float*)out_dev.ptr, (float*)count_dev.ptr, clip_out ? (float*)clip_dev.ptr : nullptr};
    rc = launch_temporal(L, nullptr);
    HIP_TRY(hipDeviceSynchronize()); // before the buffers above are freed, whatever happened
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipMemcpy(out, out_dev.ptr, image_bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(count_out, count_dev.ptr, count * sizeof(float), hipMemcpyDeviceToHost));
    if (clip_out) HIP_TRY(hipMemcpy(clip_out, clip_dev.ptr, count * sizeof(float), hipMemcpyDeviceToHost));
    return PYR_OK;
}

int pyr_film_develop_device(const PyrFilmDesc* film, const PyrGrain* grains_device, const PyrDevelopParams* params, uint8_t* rgb_device, int device,
                            void* hip_stream) {
    if (!film || !grains_device || !params || !rgb_device || !params->xyz_table) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    if (int bad = check_device(device)) return bad;
    HIP_TRY(hipSetDevice(device));
    return develop_common(film, grains_device, params, rgb_device, (hipStream_t)hip_stream, false);
}

int pyr_film_develop(const PyrFilmDesc* film, const PyrGrain* grains, const PyrDevelopParams* params, uint8_t* rgb_out, int device) {
    if (!film || !grains || !params || !rgb_out || !params->xyz_table) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    if (int bad = check_device(device)) return bad;
    HIP_TRY(hipSetDevice(device));
    const size_t pixels = (size_t)film->width * film->height;
    DeviceBuffer film_dev, rgb_dev;
    int rc;
    if ((rc = film_dev.upload(grains, pixels * film->bins * sizeof(PyrGrain))) != PYR_OK) return rc;
    if ((rc = rgb_dev.alloc(pixels * 3)) != PYR_OK) return rc;
    if ((rc = develop_common(film, (const PyrGrain*)film_dev.ptr, params, (uint8_t*)rgb_dev.ptr, nullptr, true)) != PYR_OK) return rc;
    HIP_TRY(hipMemcpy(rgb_out, rgb_dev.ptr, pixels * 3, hipMemcpyDeviceToHost));
    return PYR_OK;
}

int pyr_film_develop_linear_device(const PyrFilmDesc* film, const PyrGrain* grains_device, const PyrGrain* grains_b_device, const PyrDevelopParams* params,
                                   uint32_t space, float* out_device, int device, void* hip_stream) {
    int rc = check_linear_args(film, grains_device, params, space, out_device);
    if (rc != PYR_OK || (rc = check_device(device)) != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    return develop_linear_common(film, grains_device, grains_b_device, params, space, out_device, (hipStream_t)hip_stream, false);
}

int pyr_film_develop_linear(const PyrFilmDesc* film, const PyrGrain* grains, const PyrGrain* grains_b, const PyrDevelopParams* params, uint32_t space, float* out,
                            int device) {
    int rc = check_linear_args(film, grains, params, space, out);
    if (rc != PYR_OK || (rc = check_device(device)) != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t pixels = (size_t)film->width * film->height;
    DeviceBuffer a_dev, b_dev, out_dev;
    if ((rc = a_dev.upload(grains, pixels * film->bins * sizeof(PyrGrain))) != PYR_OK) return rc;
    if (grains_b && (rc = b_dev.upload(grains_b, pixels * film->bins * sizeof(PyrGrain))) != PYR_OK) return rc;
    if ((rc = out_dev.alloc(pixels * 3 * sizeof(float))) != PYR_OK) return rc;
    rc = develop_linear_common(film, (const PyrGrain*)a_dev.ptr, grains_b ? (const PyrGrain*)b_dev.ptr : nullptr, params, space, (float*)out_dev.ptr, nullptr, true);
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipMemcpy(out, out_dev.ptr, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return PYR_OK;
}

int pyr_image_stats_device(const float* linear_srgb_device, uint32_t width, uint32_t height, PyrImageStats* out_device, int device, void* hip_stream) {
    if (!linear_srgb_device || !out_device) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check_image_size(width, height);
    if (rc != PYR_OK || (rc = check_device(device)) != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    return launch_image_stats(linear_srgb_device, (size_t)width * height, out_device, hip_stream);
}

int pyr_image_stats(const float* linear_srgb, uint32_t width, uint32_t height, PyrImageStats* out, int device) {
    if (!linear_srgb || !out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check_image_size(width, height);
    if (rc != PYR_OK || (rc = check_device(device)) != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t pixels = (size_t)width * height;
    DeviceBuffer image_dev, stats_dev;
    if ((rc = image_dev.upload(linear_srgb, pixels * 3 * sizeof(float))) != PYR_OK) return rc;
    if ((rc = stats_dev.alloc(sizeof(PyrImageStats))) != PYR_OK) return rc;
    if ((rc = launch_image_stats((const float*)image_dev.ptr, pixels, (PyrImageStats*)stats_dev.ptr, nullptr)) != PYR_OK) return rc;
    HIP_TRY(hipMemcpy(out, stats_dev.ptr, sizeof(PyrImageStats), hipMemcpyDeviceToHost));
    return PYR_OK;
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
    if (!linear_srgb_device || !resolved || !rgb_device) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check_resolved_tone(resolved);
    if (rc != PYR_OK || (rc = check_image_size(width, height)) != PYR_OK || (rc = check_device(device)) != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    const ToneLaunch T{linear_srgb_device, rgb_device, (size_t)width * height, resolved->op, resolved->exposure, resolved->white};
    return launch_tonemap(T, hip_stream);
}

int pyr_image_tonemap(const float* linear_srgb, uint32_t width, uint32_t height, const PyrToneParams* resolved, uint8_t* rgb_out, int device) {
    if (!linear_srgb || !resolved || !rgb_out) return fail(PYR_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check_resolved_tone(resolved);
    if (rc != PYR_OK || (rc = check_image_size(width, height)) != PYR_OK || (rc = check_device(device)) != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t pixels = (size_t)width * height;
    DeviceBuffer image_dev, rgb_dev;
    if ((rc = image_dev.upload(linear_srgb, pixels * 3 * sizeof(float))) != PYR_OK) return rc;
    if ((rc = rgb_dev.alloc(pixels * 3)) != PYR_OK) return rc;
    const ToneLaunch T{(const float*)image_dev.ptr, (uint8_t*)rgb_dev.ptr, pixels, resolved->op, resolved->exposure, resolved->white};
    if ((rc = launch_tonemap(T, nullptr)) != PYR_OK) return rc;
    HIP_TRY(hipMemcpy(rgb_out, rgb_dev.ptr, pixels * 3, hipMemcpyDeviceToHost));
    return PYR_OK;
}

int pyr_image_denoise_device(const float* a_device, const float* b_device, const float* albedo_device, const PyrFeaturePixel* pixels_device, uint32_t width,
                             uint32_t height, const PyrDenoiseParams* params, float* out_device, float* error_out_device, int device, void* hip_stream) {
    int rc = check_denoise_args(a_device, b_device, width, height, params, out_device);
    if (rc != PYR_OK || (rc = check_device(device)) != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)hip_stream;
    float* work = nullptr;
    HIP_TRY(hipMallocAsync((void**)&work, (size_t)width * height * 9 * sizeof(float), stream));
    rc = enqueue_denoise(a_device, b_device, albedo_device, pixels_device, width, height, params, work, out_device, error_out_device, stream);
    const hipError_t e = hipFreeAsync(work, stream);
    if (rc != PYR_OK) return rc;
    if (e != hipSuccess) return hip_fail(e, "hipFreeAsync");
    return PYR_OK;
}

int pyr_image_denoise(const float* a, const float* b, const float* albedo, const PyrFeaturePixel* pixels, uint32_t width, uint32_t height,
                      const PyrDenoiseParams* params, float* out, float* error_out, int device) {
    int rc = check_denoise_args(a, b, width, height, params, out);
    if (rc != PYR_OK || (rc = check_device(device)) != PYR_OK) return rc;
    HIP_TRY(hipSetDevice(device));
    const size_t count = (size_t)width * height, image_bytes = count * 3 * sizeof(float);
    DeviceBuffer a_dev, b_dev, albedo_dev, pixels_dev, work_dev, out_dev, error_dev;
    if ((rc = a_dev.upload(a, image_bytes)) != PYR_OK || (rc = b_dev.upload(b, image_bytes)) != PYR_OK) return rc;
    if (albedo && (rc = albedo_dev.upload(albedo, image_bytes)) != PYR_OK) return rc;
    if (pixels && (rc = pixels_dev.upload(pixels, count * sizeof(PyrFeaturePixel))) != PYR_OK) return rc;
    if ((rc = work_dev.alloc(3 * image_bytes)) != PYR_OK || (rc = out_dev.alloc(image_bytes)) != PYR_OK) return rc;
    if (error_out && (rc = error_dev.alloc(image_bytes)) != PYR_OK) return rc;
    rc = enqueue_denoise((const float*)a_dev.ptr, (const float*)b_dev.ptr, albedo ? (const float*)albedo_dev.ptr : nullptr,
                         pixels ? (const PyrFeaturePixel*)pixels_dev.ptr : nullptr, width, height, params, (float*)work_dev.ptr, (float*)out_dev.ptr,
                         error_out ? (float*)error_dev.ptr : nullptr, nullptr);
    HIP_TRY(hipDeviceSynchronize()); // before the buffers above are freed, whatever happened
    if (rc != PYR_OK) return rc;
    HIP_TRY(hipMemcpy(out, out_dev.ptr, image_bytes, hipMemcpyDeviceToHost));
    if (error_out) HIP_TRY(hipMemcpy(error_out, error_dev.ptr, image_bytes, hipMemcpyDeviceToHost));
    return PYR_OK;
}

} // extern "C"
