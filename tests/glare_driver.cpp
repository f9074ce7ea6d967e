// Test driver (tests/test_glare_cpu.py::test_the_cpp_wrappers): the glare wrappers of include/pyrite_host.hpp, compiled against
// libpyrite_host.so into a stand-alone program. pyrite::glare must refuse a buffer of the wrong size with a ProjectError before the
// library sees it, hand a parameter out of range on as a GpuError of status PYR_ERR_INVALID_ARGUMENT that names it, and with good
// arguments either glare -- a constant image stays constant within 4 ulp, a 1 x 1 image comes back bit for bit -- or, where there is
// no GPU, fail with PYR_ERR_DEVICE.
// Prints "ok <devices>"; any other outcome is a non-zero exit status with a line on stderr.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "../include/pyrite_host.hpp"

using namespace pyrite;

static int failed(const char* what) {
    std::fprintf(stderr, "glare_driver: %s\n", what);
    return 1;
}

int main() {
    const uint32_t width = 13, height = 7;
    const size_t count = (size_t)width * height;
    const std::vector<float> image(count * 3, 3.7f);

    const PyrGlareParams defaults = glare_params();
    if (defaults.strength != PYR_GLARE_STRENGTH || defaults.levels != PYR_GLARE_LEVELS || defaults.threshold != PYR_GLARE_THRESHOLD || defaults.falloff != PYR_GLARE_FALLOFF ||
        defaults.reserved[0] || defaults.reserved[1] || defaults.reserved[2] || defaults.reserved[3])
        return failed("glare_params() is not the header's defaults");
    const std::optional<PyrGlareParams> from_flags = glare_from_flags(std::string("0.5"), 3L, 0.25);
    if (!from_flags || from_flags->strength != 0.5f || from_flags->levels != 3u || from_flags->threshold != 0.25f || from_flags->falloff != PYR_GLARE_FALLOFF)
        return failed("glare_from_flags does not carry the flags");
    if (glare_from_flags(std::nullopt, std::nullopt, std::nullopt)) return failed("glare_from_flags without --glare gave parameters");

    try {
        (void)glare(std::vector<float>(image.begin(), image.end() - 3), width, height);
        return failed("a buffer of the wrong size was accepted");
    } catch (const ProjectError& e) {
        if (!std::strstr(e.what(), "buffer size")) return failed("the ProjectError does not name the buffer size");
    } catch (const std::exception&) {
        return failed("a buffer of the wrong size did not raise a ProjectError");
    }
    try {
        (void)glare(image, width, height, glare_params(0.1f, 13u));
        return failed("13 levels were accepted");
    } catch (const GpuError& e) {
        if (e.status != PYR_ERR_INVALID_ARGUMENT || !std::strstr(e.what(), "levels")) return failed("13 levels: not PYR_ERR_INVALID_ARGUMENT naming levels");
    } catch (const std::exception&) {
        return failed("13 levels did not raise a GpuError");
    }
    try {
        (void)glare(image, width, height, glare_params(1.5f));
        return failed("a strength of 1.5 was accepted");
    } catch (const GpuError& e) {
        if (e.status != PYR_ERR_INVALID_ARGUMENT || !std::strstr(e.what(), "strength")) return failed("strength 1.5: not PYR_ERR_INVALID_ARGUMENT naming strength");
    } catch (const std::exception&) {
        return failed("a strength of 1.5 did not raise a GpuError");
    }

    const int devices = pyr_device_count();
    try {
        const std::vector<float> out = glare(image, width, height);
        if (devices <= 0) return failed("good arguments succeeded without a device");
        if (out.size() != image.size()) return failed("the glared image has another size");
        for (size_t k = 0; k < out.size(); ++k) {
            int32_t a, b;
            std::memcpy(&a, &out[k], 4), std::memcpy(&b, &image[k], 4);
            if (std::abs(a - b) > 4) return failed("a constant image did not stay constant within 4 ulp");
        }
        const std::vector<float> one{0.25f, 7.0f, 1e30f};
        const std::vector<float> same = glare(one, 1, 1, glare_params(1.0f, 12u, 0.5f, 2.0f));
        if (std::memcmp(same.data(), one.data(), 12) != 0) return failed("a 1 x 1 image changed");
    } catch (const GpuError& e) {
        if (devices > 0) return failed(e.what());
        if (e.status != PYR_ERR_DEVICE) return failed("good arguments without a device: not PYR_ERR_DEVICE");
    } catch (const std::exception& e) {
        return failed(e.what());
    }
    std::printf("ok %d\n", devices > 0 ? devices : 0);
    return 0;
}
