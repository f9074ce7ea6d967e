// Test driver (tests/test_upsample_cpu.py::test_the_cpp_wrappers): the upsample wrappers of include/pyrite_host.hpp, compiled
// against libpyrite_host.so into a stand-alone program. pyrite::upsample must refuse a buffer of the wrong size and half a pair
// with a ProjectError before the library sees them, hand a scale or a parameter out of range on as a GpuError of status
// PYR_ERR_INVALID_ARGUMENT that names it, and with good arguments either upsample -- a constant image stays constant within 2 ulp
// at twice the size -- or, where there is no GPU, fail with PYR_ERR_DEVICE.
// Prints "ok <devices>"; any other outcome is a non-zero exit status with a line on stderr.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "../include/pyrite_host.hpp"

using namespace pyrite;

static int failed(const char* what) {
    std::fprintf(stderr, "upsample_driver: %s\n", what);
    return 1;
}

// 0 when `call` raises a GpuError of PYR_ERR_INVALID_ARGUMENT whose text holds `name`
template <class Call>
static int refused(Call call, const char* name) {
    try {
        call();
    } catch (const GpuError& e) {
        return e.status == PYR_ERR_INVALID_ARGUMENT && std::strstr(e.what(), name) ? 0 : 1;
    } catch (const std::exception&) {
        return 1;
    }
    return 1;
}
template <class Call>
static int project_error(Call call, const char* text) {
    try {
        call();
    } catch (const ProjectError& e) {
        return std::strstr(e.what(), text) ? 0 : 1;
    } catch (const std::exception&) {
        return 1;
    }
    return 1;
}

int main() {
    const uint32_t width = 5, height = 3, scale = 2;
    const size_t count = (size_t)width * height, high = count * scale * scale;
    const std::vector<float> low(count * 3, 3.7f), low_albedo(count * 3, 0.5f), albedo(high * 3, 0.5f);
    PyrFeaturePixel record{};
    record.normal[2] = 1.0f, record.depth = 2.0f, record.coverage = 1.0f, record.material = 4u;
    const std::vector<PyrFeaturePixel> low_pixels(count, record), pixels(high, record);

    const PyrUpsampleParams d = upsample_params();
    if (d.radius != PYR_UPSAMPLE_RADIUS || d.flags != PYR_UPSAMPLE_MATCH_MATERIAL || d.sigma_normal != PYR_UPSAMPLE_SIGMA_NORMAL || d.sigma_depth != PYR_UPSAMPLE_SIGMA_DEPTH ||
        d.albedo_floor != PYR_UPSAMPLE_ALBEDO_FLOOR || d.max_gain != PYR_UPSAMPLE_MAX_GAIN || d.reserved[0] || d.reserved[1] || sizeof(d) != 32)
        return failed("upsample_params() is not the header's defaults");
    if (upsample_params(2u, false).flags != 0u || upsample_params(2u, false).radius != 2u) return failed("upsample_params does not carry its arguments");
    const std::optional<PyrUpsampleParams> from_flags = upsample_from_flags(4L, 3L);
    if (!from_flags || from_flags->radius != 3u || from_flags->flags != PYR_UPSAMPLE_MATCH_MATERIAL) return failed("upsample_from_flags does not carry the flags");
    if (upsample_from_flags(std::nullopt, std::nullopt)) return failed("upsample_from_flags without --upsample gave parameters");
    if (!upsample_flag_problem(2L, std::nullopt, 64u, 64u).empty() || upsample_flag_problem(3L, std::nullopt, 64u, 63u) != "--upsample 3 does not divide the image size 64x63" ||
        upsample_flag_problem(std::nullopt, 2L) != "--upsample-radius needs --upsample" || upsample_flag_problem(9L, std::nullopt) != "--upsample must be 2 to 8" ||
        upsample_flag_problem(2L, 4L) != "--upsample-radius must be 1 to 3")
        return failed("upsample_flag_problem");

    // wrong sizes and half pairs: ProjectError, before the library
    if (project_error([&] { (void)upsample(std::vector<float>(low.begin(), low.end() - 3), width, height, scale); }, "buffer size")) return failed("a short low image was accepted");
    if (project_error([&] { (void)upsample(low, width, height, scale, d, &low_albedo, nullptr, &low_albedo); }, "buffer size")) return failed("an albedo of the low size was accepted");
    if (project_error([&] { (void)upsample(low, width, height, scale, d, nullptr, &low_pixels, nullptr, &low_pixels); }, "buffer size")) return failed("records of the low size were accepted");
    if (project_error([&] { (void)upsample(low, width, height, scale, d, &albedo); }, "half a pair")) return failed("half an albedo pair was accepted");
    if (project_error([&] { (void)upsample(low, width, height, scale, d, nullptr, nullptr, nullptr, &low_pixels); }, "half a pair")) return failed("half a records pair was accepted");
    // range errors: GpuError, from the library
    if (refused([&] { (void)upsample(low, width, height, 1u); }, "scale")) return failed("scale 1: not PYR_ERR_INVALID_ARGUMENT naming scale");
    if (refused([&] { (void)upsample(low, width, height, 9u); }, "scale")) return failed("scale 9: not PYR_ERR_INVALID_ARGUMENT naming scale");
    if (refused([&] { (void)upsample(low, width, height, scale, upsample_params(4u)); }, "radius")) return failed("radius 4: not PYR_ERR_INVALID_ARGUMENT naming radius");
    if (refused([&] { (void)upsample(low, width, height, scale, upsample_params(1u, true, 0.1f, 0.02f, 0.0f), &albedo, nullptr, &low_albedo); }, "albedo_floor"))
        return failed("albedo_floor 0: not PYR_ERR_INVALID_ARGUMENT naming albedo_floor");
    if (refused([&] { (void)upsample(low, width, height, scale, upsample_params(1u, true, 0.1f, 0.02f, 0.01f, 0.5f), &albedo, nullptr, &low_albedo); }, "max_gain"))
        return failed("max_gain 0.5: not PYR_ERR_INVALID_ARGUMENT naming max_gain");

    const int devices = pyr_device_count();
    try {
        const std::vector<float> out = upsample(low, width, height, scale, d, &albedo, &pixels, &low_albedo, &low_pixels);
        if (devices <= 0) return failed("good arguments succeeded without a device");
        if (out.size() != high * 3) return failed("the upsampled image has another size");
        for (size_t k = 0; k < out.size(); ++k) {
            int32_t a, b;
            std::memcpy(&a, &out[k], 4), std::memcpy(&b, &low[0], 4);
            if (std::abs(a - b) > 2) return failed("a constant image did not stay constant within 2 ulp");
        }
        if (upsample(low, width, height, 3u).size() != count * 9 * 3) return failed("scale 3 without guides: another size");
    } catch (const GpuError& e) {
        if (devices > 0) return failed(e.what());
        if (e.status != PYR_ERR_DEVICE) return failed("good arguments without a device: not PYR_ERR_DEVICE");
    } catch (const std::exception& e) {
        return failed(e.what());
    }
    std::printf("ok %d\n", devices > 0 ? devices : 0);
    return 0;
}
