// Test driver (tests/test_lens_blur_cpu.py::test_the_cpp_wrappers): the lens blur wrappers of include/pyrite_host.hpp, compiled
// against libpyrite_host.so into a stand-alone program. pyrite::lens_blur must refuse buffers of the wrong size with a ProjectError
// before the library sees them, hand a parameter out of range on as a GpuError of status PYR_ERR_INVALID_ARGUMENT that names it, and
// with good arguments either blur -- an aperture of 0 gives the input's bits back -- or, where there is no GPU, fail with
// PYR_ERR_DEVICE. Prints "ok <devices>"; any other outcome is a non-zero exit status with a line on stderr.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/pyrite_host.hpp"

using namespace pyrite;

static int failed(const char* what) {
    std::fprintf(stderr, "lens_blur_driver: %s\n", what);
    return 1;
}

int main() {
    const uint32_t width = 13, height = 7;
    const size_t count = (size_t)width * height;
    std::vector<float> image(count * 3);
    for (size_t k = 0; k < image.size(); ++k) image[k] = 0.25f + 0.001f * (float)k;
    std::vector<PyrFeaturePixel> pixels(count);
    for (size_t k = 0; k < count; ++k) {
        PyrFeaturePixel r{};
        r.normal[2] = 1.0f, r.depth = 1.0f + 0.05f * (float)k, r.coverage = 1.0f, r.shape = 7, r.material = 1;
        pixels[k] = r;
    }

    Camera camera;
    camera.c.view_plane = 2.5f, camera.c.focus_distance = 3.0f, camera.c.aperture = 0.01f;
    const PyrLensBlurParams from_camera = lens_blur_params(camera);
    if (from_camera.focus_distance != 3.0f || from_camera.aperture != 0.01f || from_camera.view_plane != 2.5f || from_camera.max_radius != PYR_LENS_BLUR_MAX_RADIUS ||
        from_camera.depth_tolerance != PYR_REPROJECT_DEPTH_TOLERANCE || from_camera.reserved[0] || from_camera.reserved[1] || from_camera.reserved[2])
        return failed("lens_blur_params(camera) is not the camera's lens under the header's defaults");
    const PyrLensBlurParams by_number = lens_blur_params(3.0f, 0.01f, 2.5f, 5u, 0.1f);
    if (by_number.max_radius != 5u || by_number.depth_tolerance != 0.1f || by_number.focus_distance != 3.0f) return failed("lens_blur_params(numbers) lost one");

    for (int which = 0; which < 2; ++which) { // an image, then records, of the wrong size
        std::vector<float> short_image(image.begin(), image.end() - (which == 0 ? 3 : 0));
        std::vector<PyrFeaturePixel> short_pixels(pixels.begin(), pixels.end() - (which == 1 ? 1 : 0));
        try {
            (void)lens_blur(short_image, short_pixels, width, height, from_camera);
            return failed("a buffer of the wrong size was accepted");
        } catch (const ProjectError& e) {
            if (!std::strstr(e.what(), "buffer size")) return failed("the ProjectError does not name the buffer size");
        } catch (const std::exception&) {
            return failed("a buffer of the wrong size did not raise a ProjectError");
        }
    }

    try {
        (void)lens_blur(image, pixels, width, height, lens_blur_params(camera, 17u));
        return failed("a radius of 17 was accepted");
    } catch (const GpuError& e) {
        if (e.status != PYR_ERR_INVALID_ARGUMENT || !std::strstr(e.what(), "max_radius")) return failed("a radius of 17: not PYR_ERR_INVALID_ARGUMENT naming max_radius");
    } catch (const std::exception&) {
        return failed("a radius of 17 did not raise a GpuError");
    }

    if (!lens_blur_flag_problem(false, std::nullopt).empty() || !lens_blur_flag_problem(true, 16).empty() || lens_blur_flag_problem(false, 4).empty() ||
        lens_blur_flag_problem(true, 0).empty() || lens_blur_flag_problem(true, 17).empty())
        return failed("lens_blur_flag_problem");

    const int devices = pyr_device_count();
    camera.c.aperture = 0.0f; // the identity
    try {
        const std::vector<float> out = lens_blur(image, pixels, width, height, lens_blur_params(camera));
        if (devices <= 0) return failed("good arguments succeeded without a device");
        if (out.size() != image.size() || std::memcmp(out.data(), image.data(), image.size() * sizeof(float)) != 0) return failed("an aperture of 0 changed the image");
    } catch (const GpuError& e) {
        if (devices > 0) return failed(e.what());
        if (e.status != PYR_ERR_DEVICE) return failed("good arguments without a device: not PYR_ERR_DEVICE");
    } catch (const std::exception& e) {
        return failed(e.what());
    }
    std::printf("ok %d\n", devices > 0 ? devices : 0);
    return 0;
}
