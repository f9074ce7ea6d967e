// image_internal.h -- what image_ops.cpp (film development, linear images, tone mapping, denoising and the filters over motion
// records, without a scene) lets session.cpp use on a session's own buffers and stream: the checks of the parameter blocks, the
// launch record of a development, and the enqueues that take a stream. Declarations only: image_ops.cpp defines them all; its
// staging of host buffers and the pieces its entries' checks are composed from stay private to it.
#pragma once
#include <vector>

#include "api_internal.h"
#include "device_scene.h"

namespace pyr {

// What every entry that takes them refuses: the size of an image, the device number, the parameter blocks.
int check_image_size(uint32_t width, uint32_t height);
int check_device(int device);
int check_develop_params(const PyrDevelopParams* p);
int check_linear_args(const PyrFilmDesc* film, const void* grains, const PyrDevelopParams* p, uint32_t space, const void* out);
int check_tone_params(const PyrToneParams* t); // what pyr_tone_resolve refuses
bool tone_needs_stats(const PyrToneParams* t);
int check_denoise_params(const PyrDenoiseParams* p);
int check_motion_blur_params(const PyrMotionBlurParams* p, const char* what); // `what` names the argument: params, blur_params
int check_glare_params(const PyrGlareParams* p, const char* what);            // likewise: params, glare_params
int check_lens_blur_params(const PyrLensBlurParams* p, const char* what);     // likewise: params, blur_params
int check_despeckle_params(const PyrDespeckleParams* p, const char* what);    // likewise: params, despeckle_params
int check_upsample_params(const PyrUpsampleParams* p, const char* what, bool with_albedo); // likewise: params, upsample_params; the floor and the gain only with the albedo pair
int check_upsample_scale(uint32_t scale);
int check_upsample_size(uint32_t low_width, uint32_t low_height, uint32_t scale); // of the upsampled image

// The per-wavelength tables of a development -- filter, white_div, white_mul, sample_count floats each, then the observer table --
// are develop_table_floats(p) floats. develop_launch makes the launch record that reads them at `tables` (device); `host` receives
// the same floats for the caller to copy there.
size_t develop_table_floats(const PyrDevelopParams* p);
DevelopLaunch develop_launch(const PyrFilmDesc* film, const PyrDevelopParams* p, float* tables, std::vector<float>& host);
bool develop_uses_wave(const DevelopLaunch& D); // launch_develop_wave, not launch_develop: read at every call (PYRITE_DEVELOP_KERNEL)

// Variance, the two filter launches with the halves exchanged, the combine: everything on `stream`, every buffer on the current
// device; `work` holds three images of width * height * 3 floats (V, FA, FB).
int enqueue_denoise(const float* a, const float* b, const float* albedo, const PyrFeaturePixel* pixels, uint32_t width, uint32_t height, const PyrDenoiseParams* p,
                    float* work, float* out, float* error_out, hipStream_t stream);

// The motion blur of `image` along `motion` into `out` (kernels/motion_blur.hip): every buffer on the current device, the working
// memory allocated and freed in stream order on `stream`.
int enqueue_motion_blur(const float* image, const PyrMotionPixel* motion, uint32_t width, uint32_t height, const PyrMotionBlurParams* p, float* out, hipStream_t stream);

// The glare of `image` into `out` (kernels/glare.hip): both on the current device, the pyramid's levels allocated and freed in
// stream order on `stream`.
int enqueue_glare(const float* image, uint32_t width, uint32_t height, const PyrGlareParams* p, float* out, hipStream_t stream);

// The lens blur of `image` over the feature records `pixels` into `out` (kernels/lens_blur.hip): every buffer on the current
// device, one launch on `stream`, no working memory.
int enqueue_lens_blur(const float* image, const PyrFeaturePixel* pixels, uint32_t width, uint32_t height, const PyrLensBlurParams* p, float* out, hipStream_t stream);

// The upsampling of `low` to scale times its size into `out` (kernels/upsample.hip): every buffer on the current device, one
// launch on `stream`. Either pair is null or given whole.
int enqueue_upsample(const float* low, const float* low_albedo, const PyrFeaturePixel* low_pixels, uint32_t low_width, uint32_t low_height, uint32_t scale,
                     const float* albedo, const PyrFeaturePixel* pixels, const PyrUpsampleParams* p, float* out, hipStream_t stream);

// The firefly clamp of `a` and, when given, `b` into `a_out` and `b_out` (kernels/despeckle.hip): every buffer on the current
// device, one launch on `stream`, no working memory. `removed_out` and `counts_out` (two words, zeroed here) are optional.
int enqueue_despeckle(const float* a, const float* b, uint32_t width, uint32_t height, const PyrDespeckleParams* p, float* a_out, float* b_out, float* removed_out,
                      uint32_t* counts_out, hipStream_t stream);

} // namespace pyr
