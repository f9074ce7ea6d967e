// interp.hip -- the unit of the interpreter builds of the stage scheduler.
#include "../kernels.hip"

namespace pyr {

// The interpreter builds of the stage scheduler (the synchronous walk is built without the interpreter: a scene with interpreter
// programs always runs on the stage scheduler, which keeps the interpreter in line). HIT_TAPE: see device_scene.h TapeForm.
RenderKernel pick_interp_kernel(bool with_counters, bool lds_scene, bool lds_tables, bool hit_tape, bool product) {
    auto pick = [&](auto counters) -> RenderKernel {
        constexpr bool C = decltype(counters)::value;
        if (hit_tape && product) return pick_product_kernel(C, lds_scene, lds_tables);
        if (lds_scene) return hit_tape ? render_kernel_sm<C, true, true, false, true> : render_kernel_sm<C, true, true, false>;
        if (hit_tape) return lds_tables ? render_kernel_sm<C, true, false, true, true> : render_kernel_sm<C, true, false, false, true>;
        return lds_tables ? render_kernel_sm<C, true, false, true> : render_kernel_sm<C, true, false, false>;
    };
    return with_counters ? pick(std::true_type{}) : pick(std::false_type{});
}

} // namespace pyr
