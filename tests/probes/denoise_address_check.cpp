// Stand-alone host program (no GPU): walks the tile and halo addressing of kernels/denoise.hip -- pyr::denoise_cell of
// kernels/denoise_tile.h, the very function the kernel compiles -- over every image from 1 x 1 to 40 x 40 for
// (radius, patch) = (1, 0), (3, 1), (10, 3), with real arrays of the kernel's sizes behind every index, so that built with
// -fsanitize=address,undefined an index out of range stops the program where it happens. The staging loop is the kernel's. Every
// LDS index the kernel reads is denoise_cell(lx + ox + dx, ly + oy + dy) and every image index it reads is DenoiseCell::pixel of
// such a cell (the patch centres: dx = dy = 0); the program forms that cell for every value the sum of the two offsets takes.
// Exit status 0: every staged and every read index was in range, every cell read had been staged, every tile pixel was owned once.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pyrite_amd/csrc/kernels/denoise_tile.h"

using namespace pyr;

#define CHECK(cond)                                                                                                                  \
    do {                                                                                                                             \
        if (!(cond)) {                                                                                                               \
            std::fprintf(stderr, "%s:%d: %s failed at %u x %u, radius %u, patch %u\n", __FILE__, __LINE__, #cond, width, height, radius, patch); \
            return 1;                                                                                                                \
        }                                                                                                                            \
    } while (0)

int main() {
    const uint32_t cases[3][2] = {{1, 0}, {3, 1}, {10, 3}};
    uint64_t staged_cells = 0, read_cells = 0;
    for (const auto& rp : cases) {
        const uint32_t radius = rp[0], patch = rp[1], halo = radius + patch;
        const uint32_t rows = denoise_tile_rows(halo), plane = denoise_plane_cells(halo);
        for (uint32_t height = 1; height <= 40; ++height)
            for (uint32_t width = 1; width <= 40; ++width) {
                const size_t pixels = (size_t)width * height;
                std::vector<float> image(3 * pixels, 1.0f); // a half, V, the averaged half, the albedo: the same index serves them
                std::vector<uint8_t> owned(pixels, 0);       // the records are indexed by the pixel alone
                const uint32_t tiles_x = (width + kDenoiseTile - 1) / kDenoiseTile, tiles_y = (height + kDenoiseTile - 1) / kDenoiseTile;
                for (uint32_t tile = 0; tile < tiles_x * tiles_y; ++tile) {
                    const uint32_t x0 = (tile % tiles_x) * kDenoiseTile, y0 = (tile / tiles_x) * kDenoiseTile;
                    std::vector<float> lds(3 * (size_t)plane * 2, 0.0f); // [3][rows][kDenoisePitch] of {H, V}
                    std::vector<uint8_t> staged(plane, 0);
                    for (uint32_t k = 0; k < rows * rows; ++k) { // the staging loop of every thread of the workgroup
                        const int32_t lx = (int32_t)(k % rows) - (int32_t)halo, ly = (int32_t)(k / rows) - (int32_t)halo;
                        const DenoiseCell cell = denoise_cell(width, height, x0, y0, halo, lx, ly);
                        CHECK(cell.lds < plane && !staged[cell.lds]);
                        CHECK(!cell.inside || cell.pixel < pixels);
                        for (uint32_t c = 0; c < 3; ++c) {
                            lds[2 * ((size_t)c * plane + cell.lds)] = cell.inside ? image[3 * cell.pixel + c] : 0.0f;
                            lds[2 * ((size_t)c * plane + cell.lds) + 1] = cell.inside ? image[3 * cell.pixel + c] : 0.0f;
                        }
                        staged[cell.lds] = 1;
                        staged_cells += 1;
                    }
                    for (uint32_t thread = 0; thread < kDenoiseTile * kDenoiseTile; ++thread) {
                        const int32_t lx = (int32_t)(thread % kDenoiseTile), ly = (int32_t)(thread / kDenoiseTile);
                        const DenoiseCell self = denoise_cell(width, height, x0, y0, halo, lx, ly);
                        if (!self.inside) continue; // the kernel's threads outside the image leave here
                        CHECK(self.pixel < pixels && !owned[self.pixel]);
                        owned[self.pixel] = 1;
                        float sum = 0.0f;
                        for (int32_t sy = -(int32_t)halo; sy <= (int32_t)halo; ++sy)
                            for (int32_t sx = -(int32_t)halo; sx <= (int32_t)halo; ++sx) {
                                const DenoiseCell cell = denoise_cell(width, height, x0, y0, halo, lx + sx, ly + sy);
                                CHECK(cell.lds < plane);
                                if (!cell.inside) continue; // the skip rule: such a cell is never read
                                CHECK(staged[cell.lds] && cell.pixel < pixels);
                                CHECK(cell.pixel == (size_t)(y0 + ly + sy) * width + (x0 + lx + sx));
                                for (uint32_t c = 0; c < 3; c += 2) sum += lds[2 * ((size_t)c * plane + cell.lds) + 1] + image[3 * cell.pixel + c]; // the first and the last plane bound the middle one
                                read_cells += 1;
                            }
                        CHECK(sum > 0.0f);
                    }
                }
                for (size_t p = 0; p < pixels; ++p) CHECK(owned[p]);
            }
    }
    // beyond the documented range the function clamps: whatever a caller passes, the cell is one of the staged ones
    {
        const uint32_t width = 40, height = 40, radius = 10, patch = 3, halo = 13;
        for (int32_t l : {-1000000, -14, 29, 1000000}) {
            const DenoiseCell cell = denoise_cell(width, height, 32, 32, halo, l, l);
            CHECK(cell.lds < denoise_plane_cells(halo) && (!cell.inside || cell.pixel < (size_t)width * height));
        }
        const DenoiseCell far = denoise_cell(0xFFFFFFFFu, 1, 0xFFFFFFF0u, 0, halo, 28, 0); // no wrap at the end of the widest image
        CHECK(!far.inside);
    }
    std::printf("ok: %llu cells staged, %llu cells read\n", (unsigned long long)staged_cells, (unsigned long long)read_cells);
    return 0;
}
