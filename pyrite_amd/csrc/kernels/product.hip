// product.hip -- the unit of the PRODUCT forms of the hit-tape interpreter builds.
#include "../kernels.hip"

namespace pyr {

// The hit-tape interpreter builds for scenes with TAPE_FORM_PRODUCT colour programs: builds of their own (Walker::tape_pending says why)
RenderKernel pick_product_kernel(bool with_counters, bool lds_scene, bool lds_tables) {
    auto pick = [&](auto counters) -> RenderKernel {
        constexpr bool C = decltype(counters)::value;
        if (lds_scene) return render_kernel_sm<C, true, true, false, true, true>;
        return lds_tables ? render_kernel_sm<C, true, false, true, true, true> : render_kernel_sm<C, true, false, false, true, true>;
    };
    return with_counters ? pick(std::true_type{}) : pick(std::false_type{});
}

} // namespace pyr
