// upsample.hip -- the guided upsampling of a low-resolution linear image (include/pyrite_gpu.h "upsample"), a
// unit of its own: the header spells the f32 operations and their order out, the kernel keeps both.
//   A 256-lane workgroup owns a kTileW x kTileH = 32 x 8 tile of output pixels and stages the low-resolution patch under it in LDS
// once: the columns x0(X) - (radius-1) .. x0(X) + radius of its first and last X (x0 is monotone in X, so every lane's taps lie
// between them), the rows likewise -- at most 23 x 11 low pixels (scale 2, radius 3; kPatchW x kPatchH holds one more each way).
// A low pixel is kSlot = 3 slots of 16 bytes: {R, G, B, material}, {d_0, d_1, d_2, -} with d_c = 1 / (max(low_albedo_c, 0) + floor) -- the
// division done once per low pixel per workgroup, not per tap -- and {normal, depth}, the record's first 16 bytes as they were
// loaded. A lane reads a tap as up to three ds_read_b128. The 16 lanes one such read serves a cycle lie in one output row and reach
// at most 16 consecutive low pixels (scale >= 2); those are 48 bytes apart, 12 k mod 64 banks for k = 0..15: sixteen different
// quads of banks, so the tap rows of neighbouring lanes never pile onto one bank. Pixels of the patch that lie outside the low
// image are not staged and not read: the rule skips those taps.
//   Then each lane reads its own full-size albedo (12 B) and record (16 B and the material word), walks its (2 radius)^2 taps out
// of LDS and writes 12 B. The radius and which pairs are given are template parameters; the scale and the guide switches are
// wave-uniform launch constants. Grid-stride loop over tiles, 64-bit indices into the buffers, plain stores, no atomics: two
// calls write the same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../api_internal.h"
#include "../device_scene.h"

namespace pyr {

namespace {
constexpr uint32_t kTileW = 32, kTileH = 8; // output pixels a workgroup; a wave is two rows of 32
constexpr uint32_t kThreads = kTileW * kTileH;
constexpr uint32_t kMostBlocks = 256 * 32; // one tile a workgroup up to 1920 x 1080
// the low pixels under a tile: x0 moves by at most (kTileW - 1) / 2 + 1 over it (scale >= 2, one more for the rounding of lx), and
// 2 * radius - 1 <= 5 columns lie around it
constexpr uint32_t kPatchW = (kTileW - 1) / 2 + 2 + 2 * PYR_UPSAMPLE_MOST_RADIUS; // 23 + 1
constexpr uint32_t kPatchH = (kTileH - 1) / 2 + 2 + 2 * PYR_UPSAMPLE_MOST_RADIUS; // 11
constexpr uint32_t kSlot = 3;
static_assert(kPatchW == 23 && kPatchH == 11 && kPatchW * kPatchH * kSlot * 16 <= 16 * 1024, "the patch of the widest case, in 16 KB of LDS");

// x0 of the header for the output coordinate X: (int)floorf(lx), and lx itself
__device__ __forceinline__ int low_floor(uint32_t X, float scale, float& l) {
    l = ((float)X + 0.5f) / scale - 0.5f;
    return (int)floorf(l);
}

template <uint32_t RADIUS, bool ALBEDO, bool RECORDS>
__global__ __launch_bounds__(kThreads) void upsample_kernel(UpsampleLaunch L) {
    __shared__ float4 patch[kPatchW * kPatchH * kSlot];
    const uint32_t W = L.low_width * L.scale, H = L.low_height * L.scale;
    const uint32_t tiles_x = (W - 1) / kTileW + 1, tiles_y = (H - 1) / kTileH + 1;
    const uint64_t tiles = (uint64_t)tiles_x * tiles_y;
    const float scale = (float)L.scale, radius = (float)RADIUS;
    const int reach = (int)RADIUS - 1;
    const uint32_t tid = threadIdx.x;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t X0 = (uint32_t)(tile % tiles_x) * kTileW, Y0 = (uint32_t)(tile / tiles_x) * kTileH;
        float unused;
        const int px0 = low_floor(X0, scale, unused) - reach, py0 = low_floor(Y0, scale, unused) - reach;
        const int px1 = low_floor(min(X0 + kTileW - 1, W - 1), scale, unused) + (int)RADIUS;
        const int py1 = low_floor(min(Y0 + kTileH - 1, H - 1), scale, unused) + (int)RADIUS;
        const uint32_t pw = min((uint32_t)(px1 - px0 + 1), kPatchW), ph = min((uint32_t)(py1 - py0 + 1), kPatchH);
        __syncthreads(); // the tile before this one has been read
        for (uint32_t i = tid; i < pw * ph; i += kThreads) {
            const int qx = px0 + (int)(i % pw), qy = py0 + (int)(i / pw);
            if (qx < 0 || qy < 0 || qx >= (int)L.low_width || qy >= (int)L.low_height) continue; // never read: the rule skips the tap
            const uint64_t q = (uint64_t)qy * L.low_width + (uint32_t)qx;
            float4 first = make_float4(L.low[q * 3], L.low[q * 3 + 1], L.low[q * 3 + 2], 0.0f);
            if (RECORDS) {
                first.w = __uint_as_float(L.low_pixels[q].material);
                patch[i * kSlot + 2] = *reinterpret_cast<const float4*>(&L.low_pixels[q]); // normal[3], depth
            }
            patch[i * kSlot] = first;
            if (ALBEDO)
                patch[i * kSlot + 1] = make_float4(1.0f / (fmaxf(L.low_albedo[q * 3], 0.0f) + L.albedo_floor), 1.0f / (fmaxf(L.low_albedo[q * 3 + 1], 0.0f) + L.albedo_floor),
                                                   1.0f / (fmaxf(L.low_albedo[q * 3 + 2], 0.0f) + L.albedo_floor), 0.0f);
        }
        __syncthreads();
        const uint32_t X = X0 + tid % kTileW, Y = Y0 + tid / kTileW;
        if (X >= W || Y >= H) continue;
        const uint64_t P = (uint64_t)Y * W + X;
        float lx, ly;
        const int x0 = low_floor(X, scale, lx), y0 = low_floor(Y, scale, ly);
        float own[3] = {0.0f, 0.0f, 0.0f}; // fmaxf(albedo_c(P), 0) + albedo_floor
        if (ALBEDO) {
            own[0] = fmaxf(L.albedo[P * 3], 0.0f) + L.albedo_floor;
            own[1] = fmaxf(L.albedo[P * 3 + 1], 0.0f) + L.albedo_floor;
            own[2] = fmaxf(L.albedo[P * 3 + 2], 0.0f) + L.albedo_floor;
        }
        float4 here = make_float4(0.0f, 0.0f, 0.0f, 0.0f); // normal, depth of P
        uint32_t material = 0;
        if (RECORDS) {
            here = *reinterpret_cast<const float4*>(&L.pixels[P]);
            material = L.pixels[P].material;
        }
        float weight = 0.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, tent = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
#pragma unroll
        for (uint32_t j = 0; j < 2 * RADIUS; ++j) {
            const int qy = y0 - reach + (int)j;
            if (qy < 0 || qy >= (int)L.low_height) continue;
            const float sy = fmaxf(1.0f - fabsf((float)qy - ly) / radius, 0.0f);
#pragma unroll
            for (uint32_t i = 0; i < 2 * RADIUS; ++i) {
                const int qx = x0 - reach + (int)i;
                if (qx < 0 || qx >= (int)L.low_width) continue;
                const float sx = fmaxf(1.0f - fabsf((float)qx - lx) / radius, 0.0f);
                const float sp = sy * sx;
                if (sp == 0.0f) continue;
                const uint32_t column = min((uint32_t)(qx - px0), pw - 1), row = min((uint32_t)(qy - py0), ph - 1); // inside the patch by its construction
                const uint32_t slot = (row * pw + column) * kSlot;
                const float4 low = patch[slot];
                float gw = 1.0f;
                if (RECORDS) {
                    const float4 there = patch[slot + 2];
                    float D = 0.0f;
                    bool nan = false;
                    if (L.use_normal) {
                        const float e0 = here.x - there.x, e1 = here.y - there.y, e2 = here.z - there.z;
                        const float g = (((0.0f + e0 * e0) + e1 * e1) + e2 * e2) / L.normal_div;
                        nan = nan || g != g;
                        D = g > D ? g : D; // fmaxf(D, g) of a g that is no NaN
                    }
                    if (L.use_depth) {
                        const float m = fmaxf(fmaxf(here.w, there.w), 1e-30f);
                        const float r = (here.w - there.w) / m;
                        const float g = (r * r) / L.depth_div;
                        nan = nan || g != g;
                        D = g > D ? g : D;
                    }
                    const float t = 1.0f - D;
                    gw = (!nan && t > 0.0f) ? t * t : 0.0f;
                    if (L.match_material && __float_as_uint(low.w) != material) gw = 0.0f;
                }
                const float w = sp * gw;
                tent = tent + sp;
                b0 = b0 + sp * low.x, b1 = b1 + sp * low.y, b2 = b2 + sp * low.z;
                if (w > 0.0f) {
                    float v0 = low.x, v1 = low.y, v2 = low.z;
                    if (ALBEDO) {
                        const float4 d = patch[slot + 1];
                        const float k0 = own[0] * d.x, k1 = own[1] * d.y, k2 = own[2] * d.z;
                        v0 = low.x * (k0 < L.max_gain ? k0 : L.max_gain); // fminf(k, max_gain), a NaN counting as max_gain
                        v1 = low.y * (k1 < L.max_gain ? k1 : L.max_gain);
                        v2 = low.z * (k2 < L.max_gain ? k2 : L.max_gain);
                    }
                    weight = weight + w;
                    a0 = a0 + w * v0, a1 = a1 + w * v1, a2 = a2 + w * v2;
                }
            }
        }
        const bool guided = weight > 0.0f;
        const float over = guided ? weight : tent;
        L.out[P * 3] = (guided ? a0 : b0) / over;
        L.out[P * 3 + 1] = (guided ? a1 : b1) / over;
        L.out[P * 3 + 2] = (guided ? a2 : b2) / over;
    }
}

using UpsampleKernel = void (*)(UpsampleLaunch);
template <uint32_t RADIUS>
UpsampleKernel kernel_of(bool albedo, bool records) {
    if (albedo) return records ? upsample_kernel<RADIUS, true, true> : upsample_kernel<RADIUS, true, false>;
    return records ? upsample_kernel<RADIUS, false, true> : upsample_kernel<RADIUS, false, false>;
}
} // namespace

int launch_upsample(const UpsampleLaunch& launch, void* stream) {
    if (launch.low_width == 0 || launch.low_height == 0) return PYR_OK;
    if (launch.scale < 2 || launch.scale > PYR_UPSAMPLE_MOST_SCALE) return fail(PYR_ERR_INVALID_ARGUMENT, "upsample: scale must be 2..8"); // the patch holds no more
    if ((launch.low_albedo == nullptr) != (launch.albedo == nullptr) || (launch.low_pixels == nullptr) != (launch.pixels == nullptr))
        return fail(PYR_ERR_INVALID_ARGUMENT, "upsample: half a pair");
    const uint64_t width = (uint64_t)launch.low_width * launch.scale, height = (uint64_t)launch.low_height * launch.scale;
    if (width * height > 0xFFFFFFFFull) return fail(PYR_ERR_UNSUPPORTED, "upsample: an image of more than 2^32 - 1 pixels");
    const bool albedo = launch.albedo != nullptr, records = launch.pixels != nullptr;
    UpsampleKernel kernel = nullptr;
    switch (launch.radius) {
    case 1: kernel = kernel_of<1>(albedo, records); break;
    case 2: kernel = kernel_of<2>(albedo, records); break;
    case 3: kernel = kernel_of<3>(albedo, records); break;
    default: return fail(PYR_ERR_INVALID_ARGUMENT, "upsample: radius must be 1..3");
    }
    const uint64_t tiles = ((width - 1) / kTileW + 1) * ((height - 1) / kTileH + 1);
    hipLaunchKernelGGL(kernel, dim3((uint32_t)std::min<uint64_t>(tiles, kMostBlocks)), dim3(kThreads), 0, (hipStream_t)stream, launch);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(PYR_ERR_DEVICE, std::string("upsample kernel launch: ") + hipGetErrorString(err));
    return PYR_OK;
}

} // namespace pyr
