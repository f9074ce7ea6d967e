// bvh_device.h -- the device BVH builder's host driver (bvh_device.cpp; kernels in kernels/build.hip).
#pragma once
#include <string>
#include <vector>

#include "bvh.h"

namespace pyr {

struct DeviceBuildReport {
    uint32_t levels = 0, median_splits = 0;
    uint32_t fallback_reason = 0; // PYR_BUILD_FALLBACK_* (pyrite_gpu.h): not 0 when the builder stepped aside and `out` is not valid
    double tree_ms = 0, finish_ms = 0;
};

// build_bvh's tree (bvh.h) built on the current HIP device: level-synchronous binned SAH over `prims`, finished on the host into
// build_bvh's layout (finish_levelwise). Synchronous. Returns false with `error` set when a HIP call failed; true otherwise, with
// either the tree in `out` or report.fallback_reason saying why the caller should build on the host instead.
bool build_bvh_device(const std::vector<PrimBounds>& prims, bool leaves_tested_in_pairs, BuiltBvh& out, DeviceBuildReport& report, std::string& error);

} // namespace pyr
