// wide.hip -- the unit of the wide interpreter build (kernels.hip PYR_WIDE_VM).
#define PYR_WIDE_VM
#include "../kernels.hip"

namespace pyr {

// The wide interpreter build: the three layouts of the online form, with and without counters. Waves per SIMD as every interpreter
// build (sm_waves); the register files live in scratch.
RenderKernel pick_wide_kernel(bool with_counters, bool lds_scene, bool lds_tables) {
    auto pick = [&](auto counters) -> RenderKernel {
        constexpr bool C = decltype(counters)::value;
        if (lds_scene) return wide::render_kernel_sm<C, true, true, false>;
        return lds_tables ? wide::render_kernel_sm<C, true, false, true> : wide::render_kernel_sm<C, true, false, false>;
    };
    return with_counters ? pick(std::true_type{}) : pick(std::false_type{});
}

} // namespace pyr
