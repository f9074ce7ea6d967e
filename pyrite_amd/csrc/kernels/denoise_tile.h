// denoise_tile.h -- the one place where denoise.hip turns a pixel into an address. A workgroup owns a
// kDenoiseTile x kDenoiseTile tile of the image and keeps, in LDS, the tile plus a halo of radius + patch pixels on every side:
// rows of kDenoisePitch cells, one {H, V} pair per cell and channel. Host and device compile the same function, so a stand-alone
// host program (tests/probes/denoise_address_check.cpp) can walk every image size under a sanitizer before a kernel ever runs.
#ifndef PYRITE_DENOISE_TILE_H
#define PYRITE_DENOISE_TILE_H

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PYR_TILE_FN __host__ __device__ inline
#else
#define PYR_TILE_FN inline
#endif

namespace pyr {

constexpr uint32_t kDenoiseTile = 16;
constexpr uint32_t kDenoiseMaxRadius = 10, kDenoiseMaxPatch = 3;
// A ds_read_b64 serves 32 lanes a cycle over 64 banks; 32 lanes are two tile rows of 16 cells = 32 dwords each. With rows
// 48 cells = 96 dwords apart the second row starts 32 banks after the first: no two lanes of a group share a bank. 48 also holds the
// widest tile, 16 + 2 * (10 + 3) = 42 cells; the cells beyond 16 + 2 * halo of a row are never written or read.
constexpr uint32_t kDenoisePitch = 48;

PYR_TILE_FN uint32_t denoise_tile_rows(uint32_t halo) { return kDenoiseTile + 2u * halo; }
// {H, V} pairs of one channel plane, and of the three planes a workgroup holds
PYR_TILE_FN uint32_t denoise_plane_cells(uint32_t halo) { return denoise_tile_rows(halo) * kDenoisePitch; }

struct DenoiseCell {
    uint32_t lds;  // cell of a channel plane, < denoise_plane_cells(halo)
    size_t pixel;  // y * width + x, meaningful only when `inside`
    bool inside;   // the cell stands for a pixel of the image; a cell outside is staged as zeros and never read
};

// The cell (lx, ly) of the tile whose first pixel is (x0, y0), lx and ly counted from that pixel: -halo .. kDenoiseTile + halo - 1.
// Arguments beyond that range are clamped to it, so whatever a caller passes the LDS cell is one of the staged ones; the pixel
// index is formed only for coordinates inside the image.
PYR_TILE_FN DenoiseCell denoise_cell(uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t halo, int32_t lx, int32_t ly) {
    const int32_t lo = -(int32_t)halo, hi = (int32_t)(kDenoiseTile + halo) - 1;
    lx = lx < lo ? lo : lx > hi ? hi : lx;
    ly = ly < lo ? lo : ly > hi ? hi : ly;
    const int64_t x = (int64_t)x0 + lx, y = (int64_t)y0 + ly;
    DenoiseCell c;
    c.lds = (uint32_t)(ly + (int32_t)halo) * kDenoisePitch + (uint32_t)(lx + (int32_t)halo);
    c.inside = x >= 0 && y >= 0 && x < (int64_t)width && y < (int64_t)height;
    c.pixel = c.inside ? (size_t)y * width + (size_t)x : 0;
    return c;
}

} // namespace pyr

#endif // PYRITE_DENOISE_TILE_H
