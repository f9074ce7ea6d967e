// Test driver (tests/test_motion_blur_cpu.py::test_the_cpp_wrappers): the motion blur wrappers of include/pyrite_host.hpp, compiled
// against libpyrite_host.so into a stand-alone program. pyrite::motion_blur must refuse buffers of the wrong size with a
// ProjectError before the library sees them, hand a parameter out of range on as a GpuError of status PYR_ERR_INVALID_ARGUMENT that
// names it, and with good arguments either blur -- records without motion give the input's bits back -- or, where there is no GPU,
// fail with PYR_ERR_DEVICE. Prints "ok <devices>"; any other outcome is a non-zero exit status with a line on stderr.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/pyrite_host.hpp"

using namespace pyrite;

static int failed(const char* what) {
    std::fprintf(stderr, "motion_blur_driver: %s\n", what);
    return 1;
}

int main() {
    const uint32_t width = 13, height = 7;
    const size_t count = (size_t)width * height;
    std::vector<float> image(count * 3);
    for (size_t k = 0; k < image.size(); ++k) image[k] = 0.25f + 0.001f * (float)k;
    std::vector<PyrMotionPixel> motion(count);
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            PyrMotionPixel r{};
            r.prev_x = (float)x + 0.5f, r.prev_y = (float)y + 0.5f, r.prev_depth = r.depth = 2.0f;
            r.shape = 7, r.flags = PYR_MOTION_HIT | PYR_MOTION_IN_FRONT | PYR_MOTION_INSIDE;
            motion[(size_t)y * width + x] = r;
        }

    const PyrMotionBlurParams defaults = motion_blur_params();
    if (defaults.shutter != PYR_MOTION_BLUR_SHUTTER || defaults.samples != PYR_MOTION_BLUR_SAMPLES || defaults.max_radius != PYR_MOTION_BLUR_MAX_RADIUS ||
        defaults.depth_softness != PYR_MOTION_BLUR_DEPTH_SOFTNESS || defaults.seed != 0 || defaults.reserved[0] || defaults.reserved[1] || defaults.reserved[2])
        return failed("motion_blur_params() is not the header's defaults");

    for (int which = 0; which < 2; ++which) { // an image, then records, of the wrong size
        std::vector<float> short_image(image.begin(), image.end() - (which == 0 ? 3 : 0));
        std::vector<PyrMotionPixel> short_motion(motion.begin(), motion.end() - (which == 1 ? 1 : 0));
        try {
            (void)motion_blur(short_image, short_motion, width, height);
            return failed("a buffer of the wrong size was accepted");
        } catch (const ProjectError& e) {
            if (!std::strstr(e.what(), "buffer size")) return failed("the ProjectError does not name the buffer size");
        } catch (const std::exception&) {
            return failed("a buffer of the wrong size did not raise a ProjectError");
        }
    }

    try {
        (void)motion_blur(image, motion, width, height, motion_blur_params(0.5f, 65u));
        return failed("65 samples were accepted");
    } catch (const GpuError& e) {
        if (e.status != PYR_ERR_INVALID_ARGUMENT || !std::strstr(e.what(), "samples")) return failed("65 samples: not PYR_ERR_INVALID_ARGUMENT naming samples");
    } catch (const std::exception&) {
        return failed("65 samples did not raise a GpuError");
    }

    const int devices = pyr_device_count();
    try {
        const std::vector<float> out = motion_blur(image, motion, width, height);
        if (devices <= 0) return failed("good arguments succeeded without a device");
        if (out.size() != image.size() || std::memcmp(out.data(), image.data(), image.size() * sizeof(float)) != 0) return failed("records without motion changed the image");
    } catch (const GpuError& e) {
        if (devices > 0) return failed(e.what());
        if (e.status != PYR_ERR_DEVICE) return failed("good arguments without a device: not PYR_ERR_DEVICE");
    } catch (const std::exception& e) {
        return failed(e.what());
    }
    std::printf("ok %d\n", devices > 0 ? devices : 0);
    return 0;
}
