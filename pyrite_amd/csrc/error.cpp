// error.cpp -- the thread-local message behind fail() and pyr_last_error() (error.h).
#include "error.h"

#include "../../include/pyrite_gpu.h"

namespace {
thread_local std::string g_error;
}

namespace pyr {
int fail(int code, const std::string& message) {
    g_error = message;
    return code;
}
} // namespace pyr

extern "C" const char* pyr_last_error(void) { return g_error.c_str(); }
