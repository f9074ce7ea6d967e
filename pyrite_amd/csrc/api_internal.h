// api_internal.h -- what the host-side translation units of libpyrite_gpu.so that talk to the device and the launchers under
// kernels/ share besides the public ABI: the one error channel (error.h) with HIP's errors on it, and a device allocation that
// frees itself (scene_create.cpp defines its methods).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/pyrite_gpu.h"
#include "error.h"

namespace pyr {

int hip_fail(hipError_t e, const char* what); // fail(PYR_ERR_DEVICE, what + ": " + HIP's words for e)

#define HIP_TRY(expr)                                          \
    do {                                                       \
        hipError_t e_ = (expr);                                \
        if (e_ != hipSuccess) return pyr::hip_fail(e_, #expr); \
    } while (0)

struct DeviceBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
    ~DeviceBuffer() { release(); }
    void release();
    int upload(const void* src, size_t n); // (over an earlier allocation: that one is freed -- a rebuild uploads into the scene's buffers again)
    int alloc(size_t n);
    int reserve(size_t n); // holds `n` bytes afterwards: allocated once, kept while it is large enough
    void swap(DeviceBuffer& other) { std::swap(ptr, other.ptr), std::swap(bytes, other.bytes); }
};

// Device a scene was created on.
int scene_device(const PyrScene* scene);
// The device word the kernels set when a render's film is invalid (a path outgrew the spectral tape: 1; a wave
// gave up waiting on its workgroup's LDS queues: 2), or nullptr while the scene has none. Stays set until somebody clears it.
uint32_t* scene_overflow_word(PyrScene* scene);
// Reads that word after the scene's renders have been waited for: PYR_OK, or PYR_ERR_DEVICE with the message set (and the
// word cleared). What pyr_render_simple does before it hands the film back.
int scene_check_overflow(PyrScene* scene);

} // namespace pyr
