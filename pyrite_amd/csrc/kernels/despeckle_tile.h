// despeckle_tile.h -- the one place where despeckle.hip turns a pixel into an address. A workgroup owns a
// kDespeckleTile x kDespeckleTile tile of the image and keeps, in LDS, the luminances of the tile plus a halo of `radius` pixels on
// every side: rows of kDespecklePitch cells, one {Y_a, Y_b} pair per cell. Host and device compile the same function, so a
// stand-alone host program (tests/probes/despeckle_address_check.cpp) can walk every image size under a sanitizer before a kernel
// ever runs. The kernel's two sorting networks are stated here too, as lists that the same program runs against std::sort.
#ifndef PYRITE_DESPECKLE_TILE_H
#define PYRITE_DESPECKLE_TILE_H

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PYR_DESPECKLE_FN __host__ __device__ inline
#else
#define PYR_DESPECKLE_FN inline
#endif

namespace pyr {

constexpr uint32_t kDespeckleTile = 16;
constexpr uint32_t kDespeckleMostRadius = 2;
// A ds_read_b64 serves 32 lanes a cycle over 64 banks; 32 lanes are two tile rows of 16 cells = 32 dwords each. With rows
// 48 cells = 96 dwords apart the second row starts 32 banks after the first: no two lanes of a group share a bank. 48 also holds the
// widest tile, 16 + 2 * 2 = 20 cells; the cells beyond 16 + 2 * radius of a row are never written or read.
constexpr uint32_t kDespecklePitch = 48;

PYR_DESPECKLE_FN uint32_t despeckle_tile_rows(uint32_t radius) { return kDespeckleTile + 2u * radius; }
PYR_DESPECKLE_FN uint32_t despeckle_tile_cells(uint32_t radius) { return despeckle_tile_rows(radius) * kDespecklePitch; } // {Y_a, Y_b} pairs a workgroup holds

struct DespeckleCell {
    uint32_t lds; // cell of the tile, < despeckle_tile_cells(radius)
    size_t pixel; // y * width + x, meaningful only when `inside`
    bool inside;  // the cell stands for a pixel of the image; a cell outside is staged as a pair of +inf, which no sample set keeps
};

// The cell (lx, ly) of the tile whose first pixel is (x0, y0), lx and ly counted from that pixel: -radius .. kDespeckleTile + radius - 1.
// Arguments beyond that range are clamped to it, so whatever a caller passes the LDS cell is one of the staged ones; the pixel
// index is formed only for coordinates inside the image.
PYR_DESPECKLE_FN DespeckleCell despeckle_cell(uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t radius, int32_t lx, int32_t ly) {
    const int32_t lo = -(int32_t)radius, hi = (int32_t)(kDespeckleTile + radius) - 1;
    lx = lx < lo ? lo : lx > hi ? hi : lx;
    ly = ly < lo ? lo : ly > hi ? hi : ly;
    const int64_t x = (int64_t)x0 + lx, y = (int64_t)y0 + ly;
    DespeckleCell c;
    c.lds = (uint32_t)(ly + (int32_t)radius) * kDespecklePitch + (uint32_t)(lx + (int32_t)radius);
    c.inside = x >= 0 && y >= 0 && x < (int64_t)width && y < (int64_t)height;
    c.pixel = c.inside ? (size_t)y * width + (size_t)x : 0;
    return c;
}

// The kernel's two sorts as lists of compare-exchanges (lo, hi) made at compile time: the kernel expands a list with constant
// indices, so its values stay in registers whatever the optimiser's unroller decides, and the host program runs the same lists
// against std::sort. S: the slots, 16 at radius 1 and 48 at radius 2; an empty slot holds +inf.
template <uint32_t S>
struct DespeckleNetwork {
    uint8_t lo[S * 8], hi[S * 8]; // S * 8 bounds the count for S <= 64 (16 slots: 63 and 32 exchanges; 48: 384 and 128)
    uint32_t count;
};
// Batcher's merge exchange for S slots (Knuth, TAOCP 3, 5.2.2 M): sorts any list ascending.
template <uint32_t S>
constexpr DespeckleNetwork<S> despeckle_sort_network() {
    DespeckleNetwork<S> net{};
    for (uint32_t p = 1; p < S; p <<= 1)
        for (uint32_t k = p; k >= 1; k >>= 1)
            for (uint32_t j = k % p; j + k < S; j += 2 * k)
                for (uint32_t i = 0; i < k && i + j + k < S; ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) net.lo[net.count] = (uint8_t)(i + j), net.hi[net.count] = (uint8_t)(i + j + k), net.count += 1;
    return net;
}
// The bitonic merge for S slots padded to the next power of two: it sorts a list that falls and then rises -- what the deviations
// from the median of a sorted list are, because x -> fabsf(x - m) rounds monotonically on either side of m -- in log2 stages of
// exchanges (i, i + k). The padding stands for +inf, which the empty slots at the end already hold: an exchange that would reach
// into it moves nothing and is left out.
template <uint32_t S>
constexpr DespeckleNetwork<S> despeckle_merge_network() {
    DespeckleNetwork<S> net{};
    uint32_t padded = 1;
    while (padded < S) padded <<= 1;
    for (uint32_t k = padded / 2; k >= 1; k >>= 1)
        for (uint32_t i = 0; i + k < S; ++i)
            if ((i & k) == 0) net.lo[net.count] = (uint8_t)i, net.hi[net.count] = (uint8_t)(i + k), net.count += 1;
    return net;
}

} // namespace pyr

#endif // PYRITE_DESPECKLE_TILE_H
