// profile.hip -- the -DPYR_PHASE_PROFILE build (tools/phase_profile.py) in one unit: its device-side counters, g_phase_prof, are one
// variable. It has no wide interpreter build: launch_render refuses a scene that needs it.
#include "main.hip"
#include "interp.hip"
#include "product.hip"

namespace pyr {
RenderKernel pick_wide_kernel(bool, bool, bool) { return nullptr; }
} // namespace pyr

extern "C" int pyr_debug_phase_profile(unsigned long long* out16, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(pyr::g_phase_prof), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long zero[16] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(pyr::g_phase_prof), zero, sizeof(zero)) != hipSuccess) return -1;
    }
    return 0;
}
