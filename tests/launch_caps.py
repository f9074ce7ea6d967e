"""The image kernels past their launch caps: every kernel that caps its grid walks `for (t = blockIdx.x; t <
tiles; t += gridDim.x)`, and the small images of the other test modules never enter that loop's second trip. Here are the sizes that
do, derived from the caps and tile edges as the kernel sources state them and not typed: if someone moves a cap the size follows,
and tests/test_launch_caps_cpu.py says so. Beside them the inputs of the cases (the random generators of the kernels' own test
modules, at these sizes), the restatements' results -- computed once and shared by whoever asks, never written to -- and the mapping
from a pixel to the trip of the loop that writes it, which tests/test_gpu_launch_caps.py uses to say where a difference lies.

The read of the sources is a read of numeric constants only: kMostBlocks, kTile, kTileW, kTileH, MAX_GRID, the `256 * N` of a
launch_* function, PIXEL_BLOCK, STATS_BLOCK, TONE_BLOCK. It looks for nothing else in them."""
import functools
import os
import re
import sys

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
KERNELS = os.path.join(ROOT, "pyrite_amd", "csrc", "kernels")
for _p in (ROOT, TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

f32 = np.float32
SENTINEL = 0x7FC0BEEF  # a quiet NaN with a payload no kernel here computes or copies: what every output buffer holds before the call
TILE_MARGIN, FLAT_MARGIN = 256, 1024  # tiles (pixels of a flat kernel) past the cap: a second trip that is more than one ragged corner


# ------------------------------------------------------------------------------------------------------------------------ the constants
@functools.lru_cache(maxsize=None)
def source(name):
    with open(os.path.join(KERNELS, name)) as f:
        return f.read()


def _value(text):
    """`256 * 32`, `1u << 20`, `16`: a product of integer literals, shifted."""
    text = text.strip()
    assert re.fullmatch(r"[0-9uU\s*<]+", text), text
    factors = [int(re.sub(r"[uU]", "", part)) for part in re.split(r"\*|<<", text)]
    if "<<" in text:
        assert len(factors) == 2 and "*" not in text, text
        return factors[0] << factors[1]
    return int(np.prod(factors, dtype=np.int64))


def constant(name, identifier):
    """The value `identifier` is initialised with in kernels/`name`: `constexpr uint32_t kTileW = 32, kTileH = 8;` gives either."""
    found = re.findall(r"\b%s\s*=\s*([0-9uU\s*<]+?)\s*[;,]" % re.escape(identifier), source(name))
    assert len(found) == 1, "%s: %d initialisations of %s" % (name, len(found), identifier)
    return _value(found[0])


def launch_blocks(name, launcher, nth=0):
    """The `256 * N` a launch_* function of kernels/`name` caps its grid with (the `nth` of them in the function)."""
    body = re.search(r"^int %s\(.*?^}" % re.escape(launcher), source(name), re.S | re.M)
    assert body, "%s: no %s" % (name, launcher)
    found = re.findall(r"\b256 \* \d+\b", body.group(0))
    assert len(found) > nth, "%s: %s holds %d caps" % (name, launcher, len(found))
    return _value(found[nth])


def launch_bound(name, kernel):
    """The integer in `__launch_bounds__(N) void kernel`."""
    found = re.findall(r"__launch_bounds__\((\d+)\)\s+void\s+%s\b" % re.escape(kernel), source(name))
    assert len(found) == 1, (name, kernel)
    return int(found[0])


class Tiled:
    """A kernel whose workgroup takes tiles of `tile_w` x `tile_h` pixels, at most `cap` workgroups a launch."""

    def __init__(self, name, cap, tile_w, tile_h=None):
        self.name, self.cap, self.tile_w, self.tile_h = name, cap, tile_w, tile_h or tile_w

    def tiles(self, width, height):
        return -(-width // self.tile_w), -(-height // self.tile_h)

    def height_for(self, width, trips=2, multiple=1):
        """The smallest height (a multiple of `multiple`) at `width` whose tiles exceed (trips - 1) caps by TILE_MARGIN, its last
        tile row ragged. The last tile column is ragged by the choice of `width`, and there are two tile columns at least."""
        tiles_x = -(-width // self.tile_w)
        assert tiles_x >= 2 and width % self.tile_w != 0, (self.name, width)
        rows = -(-((trips - 1) * self.cap + TILE_MARGIN) // tiles_x)
        height = (rows - 1) * self.tile_h + 1
        while height % multiple != 0 or height % self.tile_h == 0:
            height += 1
        assert -(-height // self.tile_h) == rows
        return height

    def trips(self, width, height):
        """int [height, width]: the trip of the grid-stride loop in which a pixel's tile is taken, 0 the first."""
        tiles_x, tiles_y = self.tiles(width, height)
        grid = min(tiles_x * tiles_y, self.cap)
        tile = (np.arange(height)[:, None] // self.tile_h) * tiles_x + np.arange(width)[None, :] // self.tile_w
        return tile // grid

    def where(self, width, height, x, y):
        """What a failing comparison says of the pixel (x, y)."""
        tiles_x, tiles_y = self.tiles(width, height)
        tx, ty = x // self.tile_w, y // self.tile_h
        tile = ty * tiles_x + tx
        grid = min(tiles_x * tiles_y, self.cap)
        return "%s: pixel (%d, %d) lies in tile (%d, %d), number %d of %d, trip %d of workgroup %d (a grid of %d)" % (
            self.name, x, y, tx, ty, tile, tiles_x * tiles_y, tile // grid, tile % grid, grid)


class Flat:
    """A kernel whose thread takes `per_thread` consecutive items a trip, at most `blocks` workgroups of `block` threads."""

    def __init__(self, name, blocks, block, per_thread=1):
        self.name, self.blocks, self.block, self.per_thread = name, blocks, block, per_thread

    @property
    def cap(self):
        return self.blocks * self.block * self.per_thread

    def height_for(self, width, items_per_pixel=1, margin=FLAT_MARGIN):
        """The smallest height at `width` whose items exceed the cap by `margin` pixels' worth."""
        pixels = -(-self.cap // items_per_pixel) + margin
        return -(-pixels // width)

    def trips(self, count):
        """int [count]: the trip in which an item is taken: a thread takes groups of per_thread items, group g in trip g // threads.
        The ragged end of such a kernel, fewer items than a group, goes item by item in a loop of its own: -1 here."""
        groups = count // self.per_thread
        threads = min(-(-count // (self.block * self.per_thread)), self.blocks) * self.block
        out = np.full(count, -1, dtype=np.int64)
        out[: groups * self.per_thread] = np.repeat(np.arange(groups) // threads, self.per_thread)
        return out

    def where(self, count, item):
        return "%s: item %d of %d, trip %d (a cap of %d items a trip)" % (self.name, item, count, int(self.trips(count)[item]), self.cap)


TEMPORAL = Tiled("temporal_kernel", constant("temporal.hip", "kMostBlocks"), constant("temporal.hip", "kTile"))
LENS_BLUR = Tiled("lens_blur_kernel", constant("lens_blur.hip", "kMostBlocks"), constant("lens_blur.hip", "kTile"))
UPSAMPLE = Tiled("upsample_kernel", constant("upsample.hip", "kMostBlocks"), constant("upsample.hip", "kTileW"), constant("upsample.hip", "kTileH"))
GLARE = Tiled("glare kernels", constant("glare.hip", "kMostBlocks"), constant("glare.hip", "kTile"))
VELOCITY = Tiled("motion_blur_velocity_kernel", constant("motion_blur.hip", "MAX_GRID"), 1)  # max_radius 1: a tile is a pixel
REPROJECT = Flat("reproject_kernel", launch_blocks("reproject.hip", "launch_reproject"), constant("reproject.hip", "PIXEL_BLOCK"))
VARIANCE = Flat("denoise_variance_kernel", launch_blocks("denoise.hip", "launch_denoise_variance"), constant("denoise.hip", "PIXEL_BLOCK"))
COMBINE = Flat("denoise_combine_kernel", launch_blocks("denoise.hip", "launch_denoise_combine"), constant("denoise.hip", "PIXEL_BLOCK"))  # over floats
STATS = Flat("image_stats_kernel", launch_blocks("tone.hip", "launch_image_stats"), constant("tone.hip", "STATS_BLOCK"), 4)
TONEMAP = Flat("tonemap_kernel", launch_blocks("tone.hip", "launch_tonemap"), constant("tone.hip", "TONE_BLOCK"), 4)
FILM_SUM = Flat("film_sum_kernel", launch_blocks("film.hip", "launch_film_sum"), launch_bound("film.hip", "film_sum_kernel"))  # over grains
ASSEMBLE = Flat("assemble kernels", launch_blocks("main.hip", "launch_assemble", 0), constant(os.path.join("..", "kernels.hip"), "BLOCK"))  # over grains

NARROW = 40  # three tiles of 16 a row, the last 8 wide; two of 32 for the upsampler's output
TEMPORAL_SIZE = (NARROW, TEMPORAL.height_for(NARROW))
LENS_BLUR_SIZE = (NARROW, LENS_BLUR.height_for(NARROW))
UPSAMPLE_SCALE = 2
UPSAMPLE_LOW_SIZE = (NARROW // UPSAMPLE_SCALE, UPSAMPLE.height_for(NARROW, multiple=UPSAMPLE_SCALE) // UPSAMPLE_SCALE)
FLAT_WIDTH = 1025
MOTION_BLUR_SIZE = (FLAT_WIDTH, -(-(VELOCITY.cap + FLAT_MARGIN) // FLAT_WIDTH))
REPROJECT_SIZE = (FLAT_WIDTH, REPROJECT.height_for(FLAT_WIDTH))
DENOISE_SIZE = (NARROW, max(VARIANCE.height_for(NARROW), COMBINE.height_for(NARROW, items_per_pixel=3)))
STATS_SIZE = (2049, STATS.height_for(2049, margin=FLAT_MARGIN + 1))  # more than the margin: a last group of fewer than four pixels too
TONEMAP_SIZE = (2897, TONEMAP.height_for(2897, margin=FLAT_MARGIN + 1))
FILM_SUM_CASE = dict(width=192, height=176, bins=64)  # Session.film() of a session with halves


def glare_height(width=NARROW):
    """The compose walks the image's tiles, the down to level 1 and the up from level 2 walk level 1's: tall enough for the
    compose's third trip and for level 1's second."""
    compose = GLARE.height_for(width, trips=3)
    level_1 = GLARE.height_for(-(-width // 2), trips=2)  # of level 1: two tile columns, both edges ragged
    return max(compose, 2 * level_1 - 1)  # the odd height whose half, rounded up, is level_1


GLARE_SIZE = (NARROW, glare_height())
GLARE_DEEP_WIDTH = 17  # level 2 is 5 wide, one tile column: the narrowest image whose level 2 still has a ragged column


def glare_deep_height(width=GLARE_DEEP_WIDTH):
    """glare_down_kernel<false> first runs from level 1 to level 2: the height whose level 2 exceeds the cap by TILE_MARGIN tiles."""
    w2 = -(-(-(-width // 2)) // 2)
    rows = -(-(GLARE.cap + TILE_MARGIN) // -(-w2 // GLARE.tile_w))
    h2 = (rows - 1) * GLARE.tile_h + 1
    return 4 * h2 - 3  # halves twice, rounding up, to h2


GLARE_DEEP_SIZE = (GLARE_DEEP_WIDTH, glare_deep_height())


def level_size(size, level):
    width, height = size
    for _ in range(level):
        width, height = -(-width // 2), -(-height // 2)
    return width, height


# ------------------------------------------------------------------------------------------------------------------------ the inputs
def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def temporal_frame():
    from test_gpu_temporal import random_frame

    return frozen(*random_frame(*TEMPORAL_SIZE, seed=71))


@functools.lru_cache(maxsize=None)
def temporal_wanted(with_noise):
    import temporal_restatement as R

    frame = temporal_frame()
    return frozen(*R.resolve(*frame[:5], frame[5] if with_noise else None, radius=1))


def lens_blur_focus_rows():
    """The rows of the first tiles of the workgroups that take a second one: tile t + grid follows tile t in workgroup t."""
    width, height = LENS_BLUR_SIZE
    tiles_x, tiles_y = LENS_BLUR.tiles(width, height)
    second = tiles_x * tiles_y - LENS_BLUR.cap
    return (-(-second // tiles_x)) * LENS_BLUR.tile_h


@functools.lru_cache(maxsize=None)
def lens_blur_frame():
    """test_gpu_lens_blur's random frame without its strip; then the top band -- the first tiles of every workgroup that takes a
    second -- lies exactly at the focus distance (c = 0, a reach of 0: the tile copies), and the bottom band, the second trip, is
    the random one, out of focus: the largest c and the rows' reach a workgroup found for its first tile are wrong for its second."""
    import test_gpu_lens_blur as T

    width, height = LENS_BLUR_SIZE
    image, rec = T.random_frame(width, height, seed=72, strip=False)
    top = lens_blur_focus_rows()
    rec["depth"][:top] = T.depths_in_focus(width, height, T.PLANE, T.FOCUS)[:top]
    rec["coverage"][:top] = 1
    return frozen(image, rec)


def lens_blur_params(max_radius):
    import test_gpu_lens_blur as T

    width, height = LENS_BLUR_SIZE
    return dict(focus_distance=T.FOCUS, aperture=T.aperture_for(T.SCALE, width, height, T.FOCUS, T.PLANE), view_plane=T.PLANE, max_radius=max_radius)


@functools.lru_cache(maxsize=None)
def lens_blur_wanted(max_radius):
    import lens_blur_restatement as R

    return frozen(R.lens_blur(*lens_blur_frame(), **lens_blur_params(max_radius)))[0]


@functools.lru_cache(maxsize=None)
def upsample_inputs():
    from test_gpu_upsample import random_inputs

    inputs = random_inputs(*UPSAMPLE_LOW_SIZE, UPSAMPLE_SCALE, seed=73)
    frozen(*inputs.values())
    return inputs


@functools.lru_cache(maxsize=None)
def upsample_wanted(radius):
    """(out, guided, clamped): the image and which path a pixel took, with both pairs given and the material rule on."""
    import upsample_restatement as R

    inputs = upsample_inputs()
    return frozen(*R.upsample(inputs["low"], UPSAMPLE_SCALE, radius=radius, flags=R.MATCH_MATERIAL, paths=True, albedo=inputs["albedo"], pixels=inputs["pixels"],
                              low_albedo=inputs["low_albedo"], low_pixels=inputs["low_pixels"]))


@functools.lru_cache(maxsize=None)
def glare_image(deep=False):
    from test_gpu_glare import random_image

    return frozen(random_image(*(GLARE_DEEP_SIZE if deep else GLARE_SIZE), seed=75 if deep else 74))[0]


@functools.lru_cache(maxsize=None)
def glare_wanted(levels, deep=False):
    import glare_restatement as R

    return frozen(R.glare(glare_image(deep), levels=levels, threshold=1.0, falloff=0.5, strength=0.5))[0]


GLARE_PARAMS = dict(threshold=1.0, falloff=0.5, strength=0.5)


@functools.lru_cache(maxsize=None)
def motion_blur_frame():
    from test_gpu_motion_blur import random_frame

    return frozen(*random_frame(*MOTION_BLUR_SIZE, seed=76))


MOTION_BLUR_PARAMS = dict(samples=1, max_radius=1, seed=5)


@functools.lru_cache(maxsize=None)
def motion_blur_wanted():
    import motion_blur_restatement as R

    return frozen(R.motion_blur(*motion_blur_frame(), **MOTION_BLUR_PARAMS))[0]


REPROJECT_DENSE_ENDS, REPROJECT_DENSE_SHARE = 2048, 0.05


@functools.lru_cache(maxsize=None)
def reproject_frame():
    """test_gpu_motion's random frame, thinned for the restatement's per-pixel loop: the first and the last 2,048 pixels and a seeded
    5 % of the rest keep their records; every other pixel's record loses IN_FRONT and ends at the kernel's first early-out."""
    from pyrite_amd import abi
    from test_gpu_motion import random_frame

    width, height = REPROJECT_SIZE
    current, now, history, then, counts = random_frame(width, height, seed=77)
    dense = np.random.default_rng(78).random(width * height) < REPROJECT_DENSE_SHARE
    dense[:REPROJECT_DENSE_ENDS] = dense[-REPROJECT_DENSE_ENDS:] = True
    flags = now["flags"].reshape(-1)
    flags[~dense] &= ~np.uint32(abi.PYR_MOTION_IN_FRONT)
    return frozen(current, now, history, then, counts) + (dense.reshape(height, width),)


@functools.lru_cache(maxsize=None)
def reproject_wanted():
    import motion_restatement as R

    return frozen(*R.reproject(*reproject_frame()[:5]))


@functools.lru_cache(maxsize=None)
def denoise_halves():
    from test_gpu_denoise import hdr_halves

    return frozen(*hdr_halves(*DENOISE_SIZE, seed=79))


DENOISE_PARAMS = dict(radius=1, patch=0, sigma_albedo=0.0, sigma_normal=0.0, sigma_depth=0.0)


@functools.lru_cache(maxsize=None)
def denoise_wanted():
    import denoise_restatement as R

    a, b, _, _ = denoise_halves()
    return frozen(*R.denoise(a, b, None, None, None, **DENOISE_PARAMS))


@functools.lru_cache(maxsize=None)
def stats_case():
    from test_gpu_tone import stats_image

    return frozen(stats_image(*STATS_SIZE, seed=80))[0]


@functools.lru_cache(maxsize=None)
def tonemap_case():
    """test_gpu_tone's tone_image() tiled and cut ragged to TONEMAP_SIZE: its 2,145 pixels over and over in raster order, so that every
    run of that many pixels -- the second trip is longer -- holds each of its planted ones."""
    from test_gpu_tone import tone_image

    width, height = TONEMAP_SIZE
    return frozen(np.ascontiguousarray(np.resize(tone_image().reshape(-1, 3), (height * width, 3)).reshape(height, width, 3)))[0]


def ring_of(mask, radius):
    """bool [h, w]: the pixels outside `mask` within `radius` of it in x and y."""
    height, width = mask.shape
    grown = np.zeros_like(mask)
    padded = np.zeros((height + 2 * radius, width + 2 * radius), dtype=bool)
    padded[radius:radius + height, radius:radius + width] = mask
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            grown |= padded[dy:dy + height, dx:dx + width]
    return grown & ~mask
