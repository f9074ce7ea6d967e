// Test driver (tests/test_temporal_cpu.py::test_the_cpp_wrappers): the temporal resolve wrappers of include/pyrite_host.hpp, compiled
// against libpyrite_host.so into a stand-alone program. pyrite::resolve must refuse buffers of the wrong size with a ProjectError
// before the library sees them, hand a parameter out of range on as a GpuError of status PYR_ERR_INVALID_ARGUMENT that names it, and
// with good arguments either resolve -- a first frame gives the input's bits back, count 1 and clip 0 -- or, where there is no
// GPU, fail with PYR_ERR_DEVICE. Prints "ok <devices>"; any other outcome is a non-zero exit status with a line on stderr.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/pyrite_host.hpp"

using namespace pyrite;

static int failed(const char* what) {
    std::fprintf(stderr, "temporal_driver: %s\n", what);
    return 1;
}

int main() {
    const uint32_t width = 13, height = 7;
    const size_t count = (size_t)width * height;
    std::vector<float> image(count * 3), noise(count * 3, 0.01f);
    for (size_t k = 0; k < image.size(); ++k) image[k] = 0.25f + 0.001f * (float)k;
    std::vector<PyrMotionPixel> motion(count);
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            PyrMotionPixel r{};
            r.prev_x = (float)x + 0.5f, r.prev_y = (float)y + 0.5f, r.prev_depth = r.depth = 2.0f;
            r.shape = 7, r.flags = PYR_MOTION_HIT | PYR_MOTION_IN_FRONT | PYR_MOTION_INSIDE;
            motion[(size_t)y * width + x] = r;
        }
    const Accumulated history{image, std::vector<float>(count, 4.0f)};

    const PyrTemporalParams defaults = temporal_params();
    if (defaults.depth_tolerance != PYR_REPROJECT_DEPTH_TOLERANCE || defaults.max_history != PYR_REPROJECT_MAX_HISTORY || defaults.radius != PYR_TEMPORAL_RADIUS ||
        defaults.gamma != PYR_TEMPORAL_GAMMA || defaults.noise_scale != PYR_TEMPORAL_NOISE_SCALE || defaults.response != PYR_TEMPORAL_RESPONSE || defaults.reserved[0] ||
        defaults.reserved[1])
        return failed("temporal_params() is not the header's defaults");

    for (int which = 0; which < 6; ++which) { // each buffer in turn of the wrong size
        std::vector<float> short_image(image.begin(), image.end() - (which == 0 ? 3 : 0)), short_noise(noise.begin(), noise.end() - (which == 2 ? 3 : 0));
        std::vector<PyrMotionPixel> short_motion(motion.begin(), motion.end() - (which == 1 ? 1 : 0)), short_history_motion(motion.begin(), motion.end() - (which == 5 ? 1 : 0));
        Accumulated short_history = history;
        if (which == 3) short_history.image.pop_back();
        if (which == 4) short_history.count.pop_back();
        try {
            (void)resolve(short_image, short_motion, width, height, &short_history, &short_history_motion, &short_noise);
            return failed("a buffer of the wrong size was accepted");
        } catch (const ProjectError& e) {
            if (!std::strstr(e.what(), "buffer size")) return failed("the ProjectError does not name the buffer size");
        } catch (const std::exception&) {
            return failed("a buffer of the wrong size did not raise a ProjectError");
        }
    }
    try {
        (void)resolve(image, motion, width, height, &history, nullptr);
        return failed("a history without its records was accepted");
    } catch (const ProjectError&) {
    } catch (const std::exception&) {
        return failed("a history without its records did not raise a ProjectError");
    }

    try {
        (void)resolve(image, motion, width, height, &history, &motion, &noise, temporal_params(0.02f, 32.0f, 4u));
        return failed("a radius of 4 was accepted");
    } catch (const GpuError& e) {
        if (e.status != PYR_ERR_INVALID_ARGUMENT || !std::strstr(e.what(), "radius")) return failed("radius 4: not PYR_ERR_INVALID_ARGUMENT naming radius");
    } catch (const std::exception&) {
        return failed("a radius of 4 did not raise a GpuError");
    }

    const int devices = pyr_device_count();
    try {
        const Resolved first = resolve(image, motion, width, height);
        if (devices <= 0) return failed("good arguments succeeded without a device");
        if (first.image.size() != image.size() || std::memcmp(first.image.data(), image.data(), image.size() * sizeof(float)) != 0) return failed("a first frame changed the image");
        for (size_t k = 0; k < count; ++k)
            if (first.count[k] != 1.0f || first.clip[k] != 0.0f) return failed("a first frame: count is not 1 or clip is not 0");
        const Accumulated carried{first.image, first.count};
        const Resolved second = resolve(image, motion, width, height, &carried, &motion, &noise);
        for (size_t k = 0; k < count; ++k) // the same image again over static records: the history lies in the box
            if (second.count[k] != 2.0f || second.clip[k] != 0.0f) return failed("a second frame of the same image: count is not 2 or clip is not 0");
    } catch (const GpuError& e) {
        if (devices > 0) return failed(e.what());
        if (e.status != PYR_ERR_DEVICE) return failed("good arguments without a device: not PYR_ERR_DEVICE");
    } catch (const std::exception& e) {
        return failed(e.what());
    }
    std::printf("ok %d\n", devices > 0 ? devices : 0);
    return 0;
}
