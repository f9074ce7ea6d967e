// Stand-alone host program (no GPU): walks the tile and halo addressing of kernels/despeckle.hip -- pyr::despeckle_cell of
// kernels/despeckle_tile.h, the very function the kernel compiles -- over every image from 1 x 1 to 40 x 40 at radius 1 and 2, with
// real arrays of the kernel's sizes behind every index, so that built with -fsanitize=address,undefined an index out of range stops
// the program where it happens. The staging loop and the gather loop are the kernel's: every LDS index the kernel reads is
// despeckle_cell(lx + ox, ly + oy) for the offsets of the window, and every image index it reads or writes is DespeckleCell::pixel
// of a staged cell or of the thread's own.
// Exit status 0: every staged and every read index was in range, every cell read had been staged, every pixel was owned once, and
// the cells of a window that lie inside the image are the clipped window of the rule. Then the kernel's two comparator lists
// (despeckle_sort_network, despeckle_merge_network) are run on arrays of 16 and 48 slots against std::sort: random counts of finite
// values with ties, +inf in the empty slots, the deviations from the lower median merged as the kernel merges them.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pyrite_amd/csrc/kernels/despeckle_tile.h"

using namespace pyr;

#define CHECK(cond)                                                                                                             \
    do {                                                                                                                        \
        if (!(cond)) {                                                                                                          \
            std::fprintf(stderr, "%s:%d: %s failed at %u x %u, radius %u\n", __FILE__, __LINE__, #cond, width, height, radius); \
            return 1;                                                                                                           \
        }                                                                                                                       \
    } while (0)

// Every index of a list lies inside the array it is run on (the sanitizer sees it if not), the sort list sorts whatever it is given,
// and the merge list sorts the deviations from the lower median of a sorted list. 0 when all of it holds.
template <uint32_t S>
static int check_networks(uint32_t* state) {
    const DespeckleNetwork<S> sorter = despeckle_sort_network<S>(), merger = despeckle_merge_network<S>();
    auto next = [&]() { return *state = *state * 1664525u + 1013904223u, *state >> 8; };
    auto run = [](const DespeckleNetwork<S>& net, std::vector<float>& v) {
        for (uint32_t c = 0; c < net.count; ++c) {
            const float a = v[net.lo[c]], b = v[net.hi[c]];
            v[net.lo[c]] = std::fmin(a, b), v[net.hi[c]] = std::fmax(a, b);
        }
    };
    if (sorter.count > S * 8 || merger.count > S * 8) return 1;
    for (uint32_t trial = 0; trial < 20000; ++trial) {
        std::vector<float> v(S, INFINITY);
        const uint32_t filled = next() % (S + 1);
        for (uint32_t i = 0; i < filled; ++i) v[next() % S] = (float)(next() % 40) * ((trial & 1) ? 0.37f : 1.0f); // few values: ties
        std::vector<float> want = v;
        std::sort(want.begin(), want.end());
        run(sorter, v);
        if (v != want) return 1;
        const uint32_t n = (uint32_t)std::count_if(v.begin(), v.end(), [](float x) { return x < INFINITY; });
        if (n == 0) continue;
        const float m = v[(n - 1) / 2];
        for (float& x : v) x = std::fabs(x - m);
        want = v;
        std::sort(want.begin(), want.end());
        run(merger, v);
        if (v != want) return 1;
    }
    return 0;
}

int main() {
    uint64_t staged_cells = 0, read_cells = 0;
    for (uint32_t radius = 1; radius <= kDespeckleMostRadius; ++radius) {
        const uint32_t rows = despeckle_tile_rows(radius), cells = despeckle_tile_cells(radius);
        for (uint32_t height = 1; height <= 40; ++height)
            for (uint32_t width = 1; width <= 40; ++width) {
                const size_t pixels = (size_t)width * height;
                std::vector<float> image(3 * pixels, 1.0f), out(3 * pixels, 0.0f); // a half and an output: the same index serves a, b, a_out, b_out and removed
                std::vector<uint8_t> owned(pixels, 0);
                const uint32_t tiles_x = (width - 1) / kDespeckleTile + 1, tiles_y = (height - 1) / kDespeckleTile + 1;
                for (uint32_t tile = 0; tile < tiles_x * tiles_y; ++tile) {
                    const uint32_t x0 = (tile % tiles_x) * kDespeckleTile, y0 = (tile / tiles_x) * kDespeckleTile;
                    std::vector<float> lds(2 * (size_t)cells, 0.0f); // [rows][kDespecklePitch] of {Y_a, Y_b}
                    std::vector<uint8_t> staged(cells, 0);
                    for (uint32_t k = 0; k < rows * rows; ++k) { // the staging loop of every thread of the workgroup
                        const int32_t lx = (int32_t)(k % rows) - (int32_t)radius, ly = (int32_t)(k / rows) - (int32_t)radius;
                        const DespeckleCell cell = despeckle_cell(width, height, x0, y0, radius, lx, ly);
                        CHECK(cell.lds < cells && !staged[cell.lds]);
                        CHECK(!cell.inside || cell.pixel < pixels);
                        lds[2 * (size_t)cell.lds] = cell.inside ? image[3 * cell.pixel] : 0.0f;
                        lds[2 * (size_t)cell.lds + 1] = cell.inside ? image[3 * cell.pixel + 2] : 0.0f; // the first and the last float of the pixel bound the middle one
                        staged[cell.lds] = 1;
                        staged_cells += 1;
                    }
                    for (uint32_t thread = 0; thread < kDespeckleTile * kDespeckleTile; ++thread) {
                        const int32_t lx = (int32_t)(thread % kDespeckleTile), ly = (int32_t)(thread / kDespeckleTile);
                        const DespeckleCell self = despeckle_cell(width, height, x0, y0, radius, lx, ly);
                        if (!self.inside) continue; // the kernel's threads outside the image leave here
                        CHECK(self.pixel < pixels && !owned[self.pixel] && staged[self.lds]);
                        CHECK(self.pixel == (size_t)(y0 + ly) * width + (x0 + lx));
                        owned[self.pixel] = 1;
                        float sum = lds[2 * (size_t)self.lds] + lds[2 * (size_t)self.lds + 1];
                        uint32_t inside = 0;
                        const uint32_t side = 2 * radius + 1;
                        for (uint32_t w = 0; w < side * side - 1; ++w) { // the kernel's gather: the window in raster order without its centre
                            const uint32_t at = w < side * side / 2 ? w : w + 1;
                            const int32_t ox = (int32_t)(at % side) - (int32_t)radius, oy = (int32_t)(at / side) - (int32_t)radius;
                            CHECK(ox != 0 || oy != 0);
                            const DespeckleCell cell = despeckle_cell(width, height, x0, y0, radius, lx + ox, ly + oy);
                            CHECK(cell.lds < cells && staged[cell.lds]); // read whether inside or not: a cell outside holds +inf
                            sum += lds[2 * (size_t)cell.lds] + lds[2 * (size_t)cell.lds + 1];
                            read_cells += 1;
                            const int64_t x = (int64_t)x0 + lx + ox, y = (int64_t)y0 + ly + oy;
                            CHECK(cell.inside == (x >= 0 && y >= 0 && x < (int64_t)width && y < (int64_t)height));
                            if (cell.inside) CHECK(cell.pixel == (size_t)y * width + (size_t)x);
                            inside += cell.inside;
                        }
                        const int64_t px = (int64_t)x0 + lx, py = (int64_t)y0 + ly; // the clipped window of the rule, counted directly
                        const int64_t wx = std::min<int64_t>(px + radius, width - 1) - std::max<int64_t>(px - radius, 0) + 1;
                        const int64_t wy = std::min<int64_t>(py + radius, height - 1) - std::max<int64_t>(py - radius, 0) + 1;
                        CHECK((int64_t)inside == wx * wy - 1);
                        for (uint32_t c = 0; c < 3; ++c) out[3 * self.pixel + c] = image[3 * self.pixel + c] + sum;
                    }
                }
                for (size_t p = 0; p < pixels; ++p) CHECK(owned[p] && out[3 * p + 2] > 0.0f);
            }
    }
    // beyond the documented range the function clamps: whatever a caller passes, the cell is one of the staged ones
    {
        const uint32_t width = 40, height = 40, radius = 2;
        for (int32_t l : {-1000000, -3, 18, 1000000}) {
            const DespeckleCell cell = despeckle_cell(width, height, 32, 32, radius, l, l);
            CHECK(cell.lds < despeckle_tile_cells(radius) && (!cell.inside || cell.pixel < (size_t)width * height));
        }
        const DespeckleCell far = despeckle_cell(0xFFFFFFFFu, 1, 0xFFFFFFF0u, 0, radius, 17, 0); // no wrap at the end of the widest image
        CHECK(!far.inside);
    }
    {
        const uint32_t width = 0, height = 0, radius = 0;
        uint32_t state = 12345u;
        CHECK(check_networks<16>(&state) == 0);
        CHECK(check_networks<48>(&state) == 0);
    }
    std::printf("ok: %llu cells staged, %llu cells read\n", (unsigned long long)staged_cells, (unsigned long long)read_cells);
    return 0;
}
