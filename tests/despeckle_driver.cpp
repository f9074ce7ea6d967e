// Test driver (tests/test_despeckle_cpu.py::test_the_cpp_wrappers): the despeckle wrappers of include/pyrite_host.hpp, compiled
// against libpyrite_host.so into a stand-alone program. pyrite::despeckle must refuse a buffer of the wrong size with a
// ProjectError before the library sees it, hand a parameter out of range on as a GpuError of status PYR_ERR_INVALID_ARGUMENT that
// names it, and with good arguments either despeckle -- a constant image comes back bit for bit with nothing counted, and one
// planted pixel in one half lands on the limit -- or, where there is no GPU, fail with PYR_ERR_DEVICE.
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
    std::fprintf(stderr, "despeckle_driver: %s\n", what);
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
    const uint32_t width = 7, height = 5;
    const size_t floats = (size_t)width * height * 3;
    const std::vector<float> a(floats, 3.7f), b(floats, 3.7f);

    const PyrDespeckleParams d = despeckle_params();
    if (d.radius != PYR_DESPECKLE_RADIUS || d.k != PYR_DESPECKLE_K || d.relative != PYR_DESPECKLE_RELATIVE || d.floor != PYR_DESPECKLE_FLOOR || d.flags != 0u || d.reserved[0] ||
        d.reserved[1] || d.reserved[2] || sizeof(d) != 32)
        return failed("despeckle_params() is not the header's defaults");
    if (despeckle_params(1u, 4.0f).radius != 1u || despeckle_params(1u, 4.0f).k != 4.0f) return failed("despeckle_params does not carry its arguments");
    const std::optional<PyrDespeckleParams> from_flags = despeckle_from_flags(std::string("4.5"), 1L);
    if (!from_flags || from_flags->radius != 1u || from_flags->k != 4.5f || from_flags->relative != PYR_DESPECKLE_RELATIVE) return failed("despeckle_from_flags does not carry the flags");
    if (despeckle_from_flags(std::nullopt, std::nullopt)) return failed("despeckle_from_flags without --despeckle gave parameters");
    if (!despeckle_flag_problem(std::string("6"), std::nullopt, 8u, 2L).empty() || despeckle_flag_problem(std::nullopt, 2L) != "--despeckle-radius needs --despeckle" ||
        despeckle_flag_problem(std::string("0"), std::nullopt) != "--despeckle must be a finite number above 0" ||
        despeckle_flag_problem(std::string("x"), std::nullopt) != "--despeckle must be a finite number above 0" ||
        despeckle_flag_problem(std::string("6"), 3L) != "--despeckle-radius must be 1 to 2" ||
        despeckle_flag_problem(std::string("6"), std::nullopt, 7u) != "--despeckle needs an even number of samples per pixel: the two half films must be equal")
        return failed("despeckle_flag_problem");

    // wrong sizes: ProjectError, before the library
    if (project_error([&] { (void)despeckle(std::vector<float>(a.begin(), a.end() - 3), &b, width, height); }, "buffer size")) return failed("a short first half was accepted");
    if (project_error([&] { const std::vector<float> small(3, 0.0f); (void)despeckle(a, &small, width, height); }, "buffer size")) return failed("a short second half was accepted");
    // range errors: GpuError, from the library
    if (refused([&] { (void)despeckle(a, &b, width, height, despeckle_params(0u)); }, "radius")) return failed("radius 0: not PYR_ERR_INVALID_ARGUMENT naming radius");
    if (refused([&] { (void)despeckle(a, &b, width, height, despeckle_params(3u)); }, "radius")) return failed("radius 3: not PYR_ERR_INVALID_ARGUMENT naming radius");
    if (refused([&] { (void)despeckle(a, &b, width, height, despeckle_params(2u, 0.0f)); }, "params->k ")) return failed("k 0: not PYR_ERR_INVALID_ARGUMENT naming k");
    if (refused([&] { (void)despeckle(a, nullptr, width, height, despeckle_params(2u, 6.0f, -1.0f)); }, "relative")) return failed("relative -1: not PYR_ERR_INVALID_ARGUMENT naming relative");
    if (refused([&] { (void)despeckle(a, nullptr, width, height, despeckle_params(2u, 6.0f, 0.1f, INFINITY)); }, "floor")) return failed("floor inf: not PYR_ERR_INVALID_ARGUMENT naming floor");

    const int devices = pyr_device_count();
    try {
        const Despeckled same = despeckle(a, &b, width, height);
        if (devices <= 0) return failed("good arguments succeeded without a device");
        if (same.a.size() != floats || same.b.size() != floats || same.removed.size() != floats) return failed("an output has another size");
        if (std::memcmp(same.a.data(), a.data(), floats * 4) || std::memcmp(same.b.data(), b.data(), floats * 4) || same.counts[0] || same.counts[1])
            return failed("a constant image did not come back bit for bit");
        std::vector<float> lit = a;
        for (int c = 0; c < 3; ++c) lit[3 * (2 * width + 3) + c] = 740.0f;
        const Despeckled cleaned = despeckle(lit, &b, width, height);
        const float limit = 3.7f + 6.0f * (0.1f * 3.7f); // the median of a constant neighbourhood plus six times a tenth of it, near enough
        if (cleaned.counts[0] != 1u || cleaned.counts[1] != 0u || std::fabs(cleaned.a[3 * (2 * width + 3)] - limit) > 1e-3f * limit) return failed("the planted pixel was not clamped to the limit");
        if (std::memcmp(cleaned.b.data(), b.data(), floats * 4)) return failed("the other half changed");
        const Despeckled one = despeckle(lit, nullptr, width, height, despeckle_params(1u));
        if (!one.b.empty() || one.counts[0] != 1u || one.counts[1] != 0u) return failed("one image, radius 1: the planted pixel was not clamped");
    } catch (const GpuError& e) {
        if (devices > 0) return failed(e.what());
        if (e.status != PYR_ERR_DEVICE) return failed("good arguments without a device: not PYR_ERR_DEVICE");
    } catch (const std::exception& e) {
        return failed(e.what());
    }
    std::printf("ok %d\n", devices > 0 ? devices : 0);
    return 0;
}
