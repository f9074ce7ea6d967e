// error.h -- the one error channel of libpyrite_gpu.so, free of HIP: the units that only decide (scene_pack.cpp) report through it
// as the units that talk to the device do (api_internal.h adds hip_fail and HIP_TRY on top).
#pragma once
#include <string>

namespace pyr {

// Records the thread-local message pyr_last_error() returns and hands `code` back. Everything that refuses or fails reports
// here -- entry points, checks, the kernels' launchers -- so whoever gets a code back passes it on and the message is the failure's.
int fail(int code, const std::string& message);

} // namespace pyr
