"""Conditions on the inputs of tests/test_gpu_launch_caps.py, checked without a GPU (tests/launch_caps.py has the sizes and the
inputs): every case crosses its kernel's launch cap, by the caps and tile edges the kernel sources state today -- raise a cap and
the size assertion here fails unless the case follows; the pixels of the second trip are not degenerate, judged from the numpy
restatements alone; a pixel that is not finite lies in a second-trip tile and one in such a tile's ring; and the mapping from a pixel
to its trip, which the GPU tests print when a comparison fails, is the loop's own `t, t + grid, ...`."""
import numpy as np
import pytest

import launch_caps as lc

f32 = np.float32
SHARE = 0.05  # of the second trip's pixels, for every path a case is meant to show (tests/test_gpu_upsample.py test_the_inputs_take_every_path)


# ------------------------------------------------------------------------------------------------------------------------ 1. the sizes
def crosses(kernel, size, trips=2):
    """The tiles of `size` exceed (trips - 1) caps by the margin, both edges ragged, two tile columns at least."""
    width, height = size
    tiles_x, tiles_y = kernel.tiles(width, height)
    return tiles_x * tiles_y >= (trips - 1) * kernel.cap + lc.TILE_MARGIN and tiles_x >= 2 and width % kernel.tile_w != 0 and height % kernel.tile_h != 0


def test_the_constants_are_the_sources_own():
    """What the regular expressions found: today's values, so that a changed source shows here first and as what it is."""
    assert (lc.TEMPORAL.cap, lc.TEMPORAL.tile_w, lc.TEMPORAL.tile_h) == (8192, 16, 16) and (lc.LENS_BLUR.cap, lc.LENS_BLUR.tile_w) == (8192, 16)
    assert (lc.UPSAMPLE.cap, lc.UPSAMPLE.tile_w, lc.UPSAMPLE.tile_h) == (8192, 32, 8) and (lc.GLARE.cap, lc.GLARE.tile_w) == (8192, 16)
    assert lc.VELOCITY.cap == 1 << 20
    assert [k.cap for k in (lc.REPROJECT, lc.VARIANCE, lc.COMBINE, lc.STATS, lc.TONEMAP, lc.FILM_SUM, lc.ASSEMBLE)] == [
        4096 * 256, 4096 * 256, 4096 * 256, 2048 * 256 * 4, 4096 * 256 * 4, 8192 * 256, 8192 * 256]
    assert lc._value("1u << 20") == 1 << 20 and lc._value("256 * 32") == 8192 and lc._value(" 16") == 16


def test_every_case_crosses_its_cap():
    assert crosses(lc.TEMPORAL, lc.TEMPORAL_SIZE) and crosses(lc.LENS_BLUR, lc.LENS_BLUR_SIZE)
    low_w, low_h = lc.UPSAMPLE_LOW_SIZE
    assert crosses(lc.UPSAMPLE, (low_w * lc.UPSAMPLE_SCALE, low_h * lc.UPSAMPLE_SCALE))
    assert crosses(lc.GLARE, lc.GLARE_SIZE, trips=3), "the compose's third trip"
    assert crosses(lc.GLARE, lc.level_size(lc.GLARE_SIZE, 1)), "level 1: glare_down_kernel<true> and glare_up_kernel<false>"
    assert not crosses(lc.GLARE, lc.level_size(lc.GLARE_SIZE, 2)), "level 2 of this image stays below the cap: the deep image is for it"
    deep_w, deep_h = lc.level_size(lc.GLARE_DEEP_SIZE, 2)  # one tile column: tiles_x is 1 here, as the narrow image has it
    assert -(-deep_w // lc.GLARE.tile_w) * -(-deep_h // lc.GLARE.tile_h) >= lc.GLARE.cap + lc.TILE_MARGIN and deep_w % 16 != 0 and deep_h % 16 != 0
    assert lc.GLARE_DEEP_SIZE[0] * lc.GLARE_DEEP_SIZE[1] * 12 <= 111 * 10 ** 6  # what a case may move
    pixels = lambda size: size[0] * size[1]  # noqa: E731
    assert pixels(lc.MOTION_BLUR_SIZE) >= lc.VELOCITY.cap + lc.FLAT_MARGIN and lc.MOTION_BLUR_SIZE[0] >= 2  # max_radius 1: a tile is a pixel
    assert pixels(lc.REPROJECT_SIZE) >= lc.REPROJECT.cap + lc.FLAT_MARGIN
    assert pixels(lc.DENOISE_SIZE) >= lc.VARIANCE.cap + lc.FLAT_MARGIN and 3 * pixels(lc.DENOISE_SIZE) >= lc.COMBINE.cap + 3 * lc.FLAT_MARGIN
    assert pixels(lc.STATS_SIZE) > lc.STATS.cap + lc.FLAT_MARGIN and pixels(lc.STATS_SIZE) % 4 != 0
    assert pixels(lc.TONEMAP_SIZE) > lc.TONEMAP.cap + lc.FLAT_MARGIN and pixels(lc.TONEMAP_SIZE) % 4 != 0
    film = lc.FILM_SUM_CASE
    assert film["width"] * film["height"] * film["bins"] >= lc.FILM_SUM.cap + lc.FLAT_MARGIN
    # the widths divide nothing: no tile edge, no group of four pixels
    assert all(size[0] % 16 for size in (lc.TEMPORAL_SIZE, lc.LENS_BLUR_SIZE, lc.GLARE_SIZE, lc.DENOISE_SIZE, lc.REPROJECT_SIZE, lc.STATS_SIZE, lc.TONEMAP_SIZE))


def test_a_moved_cap_moves_the_size():
    """The derivation, at made-up caps: the height follows the cap, and at today's it is the committed one."""
    for cap in (100, 8192, 8193, 20000):
        kernel = lc.Tiled("made up", cap, 16)
        for trips in (2, 3):
            height = kernel.height_for(40, trips=trips)
            assert crosses(kernel, (40, height), trips) and not crosses(kernel, (40, height - 16), trips)
    wide = lc.Tiled("made up", 8192, 32, 8)
    height = wide.height_for(40, multiple=2)
    assert height % 2 == 0 and crosses(wide, (40, height)) and not crosses(wide, (40, height - 8))
    flat = lc.Flat("made up", 7, 256, 4)
    assert flat.cap == 7168 and 33 * flat.height_for(33) >= flat.cap + lc.FLAT_MARGIN > 33 * (flat.height_for(33) - 1)
    assert lc.Tiled("made up", 8192, 16).height_for(40) == lc.TEMPORAL_SIZE[1]


# ------------------------------------------------------------------------------------------------------------------------ 2. the mapping
@pytest.mark.parametrize("tile", [(16, 16), (32, 8), (1, 1)], ids=lambda t: "%dx%d" % t)
def test_the_trip_of_a_pixel_is_the_loop_s_own(tile):
    """A made-up cap of 5 workgroups: workgroup b takes the tiles b, b + grid, ... in turn, and every pixel of a tile is its tile's."""
    kernel = lc.Tiled("made up", 5, *tile)
    width, height = 2 * tile[0] + 1, 6 * tile[1] + 3
    tiles_x, tiles_y = kernel.tiles(width, height)
    tiles = tiles_x * tiles_y
    grid = min(tiles, kernel.cap)
    direct = np.full((height, width), -1)
    for block in range(grid):
        for trip, t in enumerate(range(block, tiles, grid)):
            ty, tx = divmod(t, tiles_x)
            direct[ty * tile[1]:(ty + 1) * tile[1], tx * tile[0]:(tx + 1) * tile[0]] = trip
    assert (direct >= 0).all() and np.array_equal(direct, kernel.trips(width, height)) and direct.max() == -(-tiles // grid) - 1
    assert "trip %d " % direct[height - 1, width - 1] in kernel.where(width, height, width - 1, height - 1)
    one = lc.Tiled("made up", 1000, *tile)  # below the cap: one trip
    assert not one.trips(width, height).any()


@pytest.mark.parametrize("per_thread", [1, 4])
def test_the_trip_of_an_item_is_the_loop_s_own(per_thread):
    kernel = lc.Flat("made up", 3, 8, per_thread)
    count = 5 * kernel.cap // 2 + 3
    threads = min(-(-count // (8 * per_thread)), 3) * 8
    direct = np.full(count, -1)
    groups = count // per_thread
    for thread in range(threads):
        for trip, g in enumerate(range(thread, groups, threads)):
            direct[g * per_thread:(g + 1) * per_thread] = trip
    assert np.array_equal(direct, kernel.trips(count)) and direct.max() == 2 and (direct[groups * per_thread:] == -1).all()


# ------------------------------------------------------------------------------------------------------------------------ 3. the second trips
def second_trip(kernel, size):
    trips = kernel.trips(*size)
    assert trips.max() >= 1
    return trips >= 1


def shares(masks, where):
    return {name: float(mask[where].mean()) for name, mask in masks.items()}


def assert_not_finite_in_and_around(not_finite, second, radius, what):
    ring = lc.ring_of(second, radius)
    print("%s: %d pixels that are not finite in the second trip's tiles, %d in their ring of %d" % (what, int((not_finite & second).sum()), int((not_finite & ring).sum()), radius))
    assert (not_finite & second).any() and (not_finite & ring).any(), what


def test_the_temporal_frame_clips_and_keeps_in_its_second_trip():
    current, now, history, then, counts, noise = lc.temporal_frame()
    second = second_trip(lc.TEMPORAL, lc.TEMPORAL_SIZE)
    for with_noise in (True, False):
        _, count, clip = lc.temporal_wanted(with_noise)
        found = shares({"clipped": clip > 0, "blended and not clipped": (count != 1) & (clip == 0), "no history": (count == 1) & (clip == 0)}, second)
        print("temporal, %s: of the %d pixels of the second trip %r" % ("with noise" if with_noise else "without noise", int(second.sum()), found))
        assert found["clipped"] >= SHARE and found["blended and not clipped"] >= SHARE, found
    assert_not_finite_in_and_around(~np.isfinite(current).all(axis=-1), second, 1, "temporal, current")
    assert_not_finite_in_and_around(~np.isfinite(noise).all(axis=-1), second, 1, "temporal, noise")


def test_the_lens_blur_frame_is_sharp_on_the_first_trip_and_blurred_on_the_second():
    import lens_blur_restatement as R

    image, rec = lc.lens_blur_frame()
    second = second_trip(lc.LENS_BLUR, lc.LENS_BLUR_SIZE)
    top = lc.lens_blur_focus_rows()
    assert 0 < top and not second[:top].any(), "the band in focus is the first tiles of the workgroups that take a second"
    tiles_x, tiles_y = lc.LENS_BLUR.tiles(*lc.LENS_BLUR_SIZE)
    assert top // lc.LENS_BLUR.tile_h * tiles_x >= tiles_x * tiles_y - lc.LENS_BLUR.cap  # every workgroup with a second tile starts in the band
    finite = np.isfinite(image).all(axis=-1)
    for max_radius in (1, 2):
        params = lc.lens_blur_params(max_radius)
        c = R.circles(rec, params["focus_distance"], params["aperture"], params["view_plane"], max_radius)[0]
        want = lc.lens_blur_wanted(max_radius)
        changed = (want.view(np.uint32) != image.view(np.uint32)).any(axis=-1)
        inner = top - max_radius  # rows a blurred pixel below the band cannot reach
        print("lens blur, radius %d: c is 0 in the first %d rows, %.3g at most below; %.1f %% of the second trip's pixels change, %.1f %% keep their bits" % (
            max_radius, top, float(c[top:].max()), 100 * changed[second].mean(), 100 * (~changed & finite)[second].mean()))
        assert not c[:top].any() and not changed[:inner].any(), "the first tiles copy: a reach of 0"
        assert np.ceil(c[second].max()) == max_radius, "the second tiles reach max_radius"
        assert changed[second].mean() >= SHARE
    assert_not_finite_in_and_around(~finite, second, 2, "lens blur")


def test_the_upsampler_s_inputs_take_every_path_in_the_second_trip():
    inputs = lc.upsample_inputs()
    low_w, low_h = lc.UPSAMPLE_LOW_SIZE
    size = (low_w * lc.UPSAMPLE_SCALE, low_h * lc.UPSAMPLE_SCALE)
    second = second_trip(lc.UPSAMPLE, size)
    for radius in (1, 3):
        _, guided, clamped = lc.upsample_wanted(radius)
        found = shares({"guided": guided, "fallback": ~guided, "a gain clamped": clamped}, second)
        print("upsample radius %d: of the %d pixels of the second trip %r" % (radius, int(second.sum()), found))
        assert min(found.values()) >= SHARE, found
    low_second = second[::lc.UPSAMPLE_SCALE, ::lc.UPSAMPLE_SCALE]  # the low pixels under the second trip's tiles
    assert_not_finite_in_and_around(~np.isfinite(inputs["low"]).all(axis=-1), low_second, 3, "upsample, low")


def test_the_motion_blur_frame_moves_and_rests_in_the_second_trip():
    import motion_blur_restatement as R

    image, rec = lc.motion_blur_frame()
    width, height = lc.MOTION_BLUR_SIZE
    second = second_trip(lc.VELOCITY, lc.MOTION_BLUR_SIZE)
    assert int(second.sum()) == width * height - lc.VELOCITY.cap >= lc.FLAT_MARGIN
    _, _, length, _ = R.velocities(rec, R.DEFAULTS["shutter"], lc.MOTION_BLUR_PARAMS["max_radius"])
    found = shares({"moves": length >= f32(0.5), "rests": length < f32(0.5)}, second)
    print("motion blur: of the %d tiles of the second trip %r" % (int(second.sum()), found))
    assert min(found.values()) >= SHARE, found
    want = lc.motion_blur_wanted()
    changed = (want.view(np.uint32) != image.view(np.uint32)).any(axis=-1)
    assert changed[second].mean() >= SHARE and (~changed)[second].mean() >= SHARE
    assert_not_finite_in_and_around(~np.isfinite(image).all(axis=-1), second, 1, "motion blur")


def test_the_reprojection_s_sparse_frame_is_dense_where_the_second_trip_is():
    current, now, history, then, counts, dense = lc.reproject_frame()
    width, height = lc.REPROJECT_SIZE
    trips = lc.REPROJECT.trips(width * height)
    second = trips >= 1
    assert int(second.sum()) == width * height - lc.REPROJECT.cap == lc.FLAT_MARGIN
    assert dense.reshape(-1)[second].all() and dense.reshape(-1)[:lc.REPROJECT_DENSE_ENDS].all()
    assert abs(dense.mean() - lc.REPROJECT_DENSE_SHARE) < 0.01
    _, count = lc.reproject_wanted()
    found = float((count.reshape(-1)[second] > 1).mean())
    print("reproject: %.1f %% of the second trip's %d pixels find history; %.2f %% of the frame" % (100 * found, int(second.sum()), 100 * float((count > 1).mean())))
    assert SHARE <= found <= 1 - SHARE
    assert (count.reshape(-1)[~dense.reshape(-1)] == 1).all(), "a record without IN_FRONT ends at the first early-out"
    assert (~np.isfinite(history.reshape(-1, 3)[-3 * width:]).all(axis=-1)).any()  # history the second trip's taps can reach


def test_the_flat_cases_hold_what_their_small_cases_hold():
    a, b, _, _ = lc.denoise_halves()
    width, height = lc.DENOISE_SIZE
    second = lc.VARIANCE.trips(width * height).reshape(height, width) >= 1
    not_finite = ~(np.isfinite(a).all(axis=-1) & np.isfinite(b).all(axis=-1))
    assert second.sum() >= lc.FLAT_MARGIN and (not_finite & second).any(), "hdr_halves plants its inf three rows from the end"
    out, error = lc.denoise_wanted()
    smooth = np.isfinite(out).all(axis=-1) & second
    assert smooth.mean() > 0 and (out[smooth] != a[smooth]).any()
    stats = lc.stats_case().reshape(-1, 3)
    second = lc.STATS.trips(len(stats)) >= 1
    assert second.sum() >= lc.FLAT_MARGIN and (lc.STATS.trips(len(stats)) == -1).sum() == len(stats) % 4
    with np.errstate(all="ignore"):
        y = (f32(0.2126) * stats[:, 0] + f32(0.7152) * stats[:, 1]) + f32(0.0722) * stats[:, 2]
    assert (y[second] > 0).mean() >= SHARE and len(np.unique(y[second].view(np.uint32) >> 20)) > 30  # many bins of the histogram
    tone = lc.tonemap_case().reshape(-1, 3)
    second = lc.TONEMAP.trips(len(tone)) >= 1
    assert second.sum() >= lc.FLAT_MARGIN and not np.isfinite(tone[second]).all() and (tone[second] > 1).mean() >= SHARE and (tone[second] < 1).mean() >= SHARE
