"""The temporal resolve on the GPU (include/pyrite_gpu.h "temporal resolve") -- run with `-m gpu` on an MI355X.

The kernel is held against the numpy restatement (tests/temporal_restatement.py) bit for bit -- `out`, `count_out` and `clip_out`:
the header spells every f32 operation and its order out, contraction is off on both sides, and sqrt32 and the compiler's division
round as numpy does. Then against pyr_image_reproject on the GPU where nothing is clipped, and against what it is for: a box that
slides through the Cornell box drags its shadow over the floor, and the resolve must follow it where the running mean cannot."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_restatement as R  # noqa: E402

from pyrite_amd import abi, develop, motion, scenes  # noqa: E402
from pyrite_amd._lib import check, lib  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = [(1, 1), (1, 5), (13, 7), (17, 33), (64, 36)]  # 17 x 33: one pixel past a 16-pixel workgroup in x and in y


# ------------------------------------------------------------------------------------------------------------------------ helpers
def random_frame(width, height, seed, spread=0.15):
    """(current, motion, history, history_motion, history_count, noise): colours around 0.5 and a history `spread` away, so that
    some of it lies in the box and some outside; fractional motion of up to two pixels, some of it onto a pixel centre; three
    shapes and the sky, so that taps meet foreign shapes; history depths on both sides of the 2 % tolerance; records without
    IN_FRONT; NaN, inf and 1e30 in the colours, the noise, the history and in prev_x / prev_y; counts from 0 up."""
    rng = np.random.default_rng(seed)
    n = width * height
    current = (0.5 + 0.1 * rng.standard_normal((height, width, 3))).astype(f32)
    history = (current + spread * rng.standard_normal((height, width, 3))).astype(f32)
    noise = (0.05 * rng.standard_normal((height, width, 3))).astype(f32)
    for image in (current, noise, history):
        for value in (np.nan, np.inf, -np.inf, 1e30, -1e30):
            image.reshape(-1)[rng.integers(0, 3 * n, n // 40)] = value  # none in the smallest images, whose few pixels should blend
    shapes = np.array([(1 << 30) | 3] * 5 + [(1 << 30) | 4, abi.HIT_NONE], dtype=np.uint32)  # mostly one surface, so that most taps count
    x, y = np.meshgrid(np.arange(width, dtype=f32), np.arange(height, dtype=f32))
    now, then = np.zeros((height, width), dtype=motion.RECORD), np.zeros((height, width), dtype=motion.RECORD)
    now["shape"] = shapes[rng.integers(0, 7, (height, width))]
    then["shape"] = np.where(rng.random((height, width)) < 0.8, now["shape"], shapes[rng.integers(0, 7, (height, width))])
    now["prev_x"] = x + f32(0.5) + rng.uniform(-2, 2, (height, width)).astype(f32)
    now["prev_y"] = y + f32(0.5) + rng.uniform(-2, 2, (height, width)).astype(f32)
    whole = rng.random((height, width)) < 0.3  # the pixel's own centre: one tap of weight 1, three of weight 0
    now["prev_x"][whole], now["prev_y"][whole] = x[whole] + f32(0.5), y[whole] + f32(0.5)
    for field, value in (("prev_x", np.nan), ("prev_y", np.inf), ("prev_x", 1e30), ("prev_y", -1e30), ("prev_x", -np.inf)):
        now[field][rng.random((height, width)) < 0.02] = value
    hit = now["shape"] != abi.HIT_NONE
    now["flags"] = np.where(hit, abi.PYR_MOTION_HIT, 0) | np.where(rng.random((height, width)) < 0.9, abi.PYR_MOTION_IN_FRONT, 0)
    now["depth"] = np.where(hit, rng.uniform(1, 50, (height, width)), 0).astype(f32)
    then["depth"] = f32(10)
    now["prev_depth"] = np.where(hit, (10 * (1 + rng.uniform(-0.03, 0.03, (height, width)))).astype(f32), f32(0))  # |d| <= 3 % around the 2 % line
    then["depth"][rng.random((height, width)) < 0.03] = np.nan
    counts = rng.integers(0, 40, (height, width)).astype(f32)
    return current, now, history, then, counts, noise


def resolve_on_device(current, now, history, then, counts, noise, clip=True, out_bits=None, **params):
    """`out_bits`: the 32 bits every float of the three outputs holds before the call (default: 0.0f, 0.0f and -7.0f)."""
    import torch

    h, w, _ = current.shape
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    buffers = [dev(a) for a in (current, now, noise, history, then, counts)]
    out = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
    count, clipped = torch.zeros(h * w, dtype=torch.float32, device="cuda"), torch.full((h * w,), -7.0, dtype=torch.float32, device="cuda")
    if out_bits is not None:
        out, count, clipped = (torch.full((n,), out_bits, dtype=torch.int32, device="cuda").view(torch.float32) for n in (h * w * 3, h * w, h * w))
    p = develop.temporal_params(**params)
    stream = torch.cuda.current_stream()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    check(lib().pyr_image_temporal_resolve_device(*[ptr(b) for b in buffers], w, h, C.byref(p), ptr(out), ptr(count), ptr(clipped) if clip else None, 0,
                                                  C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    return out.cpu().numpy().reshape(h, w, 3), count.cpu().numpy().reshape(h, w), clipped.cpu().numpy().reshape(h, w)


def same_bits(a, b):
    return a.tobytes() == b.tobytes()


def assert_same(got, want, what):
    for name, a, b in zip(("out", "count_out", "clip_out"), got, want):
        differs = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
        assert len(differs) == 0, "%s: %s differs in %d of %d floats, first %s: GPU %r, restatement %r" % (
            what, name, len(differs), a.size, tuple(differs[0]), a[tuple(differs[0])], b[tuple(differs[0])])


# ------------------------------------------------------------------------------------------------------------------------ A. bit for bit
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_resolve_is_the_restatement_bit_for_bit(size, gpu_lib):
    width, height = size
    current, now, history, then, counts, noise = random_frame(width, height, seed=100 + width)
    for radius in (1, 2, 3):
        for given in (noise, None):
            what = "%dx%d radius %d %s" % (width, height, radius, "with noise" if given is not None else "without noise")
            want = R.resolve(current, now, history, then, counts, given, radius=radius)
            got = develop.resolve(current, now, history, then, counts, noise=given, radius=radius)
            assert_same(got, want, what)
            if radius == 1:
                blended, clipped = int(((want[1] != 1) | (want[2] > 0)).sum()), int((want[2] > 0).sum())  # a history far outside its box leaves a count of 1
                print("resolve %s: %d of %d pixels blended, %d of them clipped" % (what, blended, width * height, clipped))
                assert width * height < 50 or (0 < clipped < blended < width * height)
            first = develop.resolve(current, now, noise=given, radius=radius)  # no history: the image's bits, NaN and all
            assert same_bits(first[0], current) and same_bits(first[1], np.ones((height, width), dtype=f32)) and not first[2].any(), what
            assert_same(first, R.resolve(current, now, noise=given, radius=radius), what + ", no history")
    for params in (dict(gamma=0.0, noise_scale=0.0), dict(response=0.0, radius=2), dict(gamma=2.5, noise_scale=0.25, response=4.0, depth_tolerance=0.0, max_history=3.0)):
        assert_same(develop.resolve(current, now, history, then, counts, noise=noise, **params), R.resolve(current, now, history, then, counts, noise, **params), str(params))


@pytest.mark.parametrize("size", [(17, 33), (64, 36)], ids=lambda s: "%dx%d" % s)
def test_the_device_entry_writes_the_host_entry_bytes_and_two_calls_agree(size, gpu_lib):
    width, height = size
    frame = random_frame(width, height, seed=7)
    for radius, with_noise in ((1, True), (3, True), (2, False)):
        args = frame[:5] + (frame[5] if with_noise else None,)
        host = develop.resolve(*args[:5], noise=args[5], radius=radius)
        again = develop.resolve(*args[:5], noise=args[5], radius=radius)
        assert all(same_bits(a, b) for a, b in zip(host, again)), "two calls differ"
        on_device = resolve_on_device(*args, radius=radius)
        assert all(same_bits(a, b) for a, b in zip(host, on_device)), "the device entry differs from the host entry"
        out, count, untouched = resolve_on_device(*args, clip=False, radius=radius)  # a NULL clip_out
        assert same_bits(out, host[0]) and same_bits(count, host[1]) and (untouched == -7).all()
        first = resolve_on_device(frame[0], frame[1], None, None, None, args[5], radius=radius)
        assert same_bits(first[0], frame[0]) and (first[1] == 1).all() and not first[2].any()


def real_records(name):
    """(records now, records then) from the motion pass: `cornell`, 64 x 64, the tall box posed aside with the snapshot kept, so
    that its pixels and the ones it uncovered fetch from elsewhere; `lamps`, 13 x 7, spheres and a plane under a sky, the camera turned a little against the previous one."""
    import pose_cases

    if name == "cornell":
        world, cam, r, _ = scenes.build(scenes.c2_cornell(64, 64, 16), seed=5)
        size = (64, 64)
        world.set_objects([pose_cases.triangles(0, 12), pose_cases.triangles(12, 12)])
        world.scene(0)
        then = r.motion(size, cam, world)
        world.keep_previous()
        world.pose({0: (pose_cases.rotation4((0, 0, 1), 0.2, translation=(0.3, 0.0, 0.0)), 1.0)})
    else:
        from test_gpu_motion import turned

        world, cam, r, _ = scenes.build(scenes.lamps_example(13, 7, 16), seed=5)
        size = (13, 7)
        cam = turned(cam, 0.15, axis=(1, 0, 0))  # up by 8.6 degrees: at 13 x 7 the scene's own camera sees no sky
        then = r.motion(size, cam, world)
        now = r.motion(size, cam, world, previous_camera=turned(cam, 0.03))  # the camera turned by a pixel and a half: the sky follows it
        world.close()
        return now, then
    now = r.motion(size, cam, world)
    world.close()
    return now, then


@pytest.mark.parametrize("name", ["cornell", "lamps"])
def test_records_of_real_passes(name, gpu_lib):
    now, then = real_records(name)
    height, width = now.shape
    rng = np.random.default_rng(3)
    x, y = np.meshgrid(np.arange(width, dtype=f32) + f32(0.5), np.arange(height, dtype=f32) + f32(0.5))
    moved = (np.abs(now["prev_x"] - x) > 0.25) | (np.abs(now["prev_y"] - y) > 0.25)
    if name == "cornell":
        assert moved.any() and (~moved).any()
    else:
        assert (now["shape"] == abi.HIT_NONE).any() and (now["shape"] != abi.HIT_NONE).any()  # sky and surfaces
    current = (0.5 + 0.1 * rng.standard_normal((height, width, 3))).astype(f32)
    history = (current + 0.15 * rng.standard_normal((height, width, 3))).astype(f32)
    noise = (0.05 * rng.standard_normal((height, width, 3))).astype(f32)
    counts = rng.integers(1, 40, (height, width)).astype(f32)
    for radius, given in ((1, noise), (3, noise), (2, None)):
        want = R.resolve(current, now, history, then, counts, given, radius=radius)
        assert_same(develop.resolve(current, now, history, then, counts, noise=given, radius=radius), want, "%s radius %d" % (name, radius))
    fresh = int((want[1] == 1).sum())
    print("resolve on the records of %s: %d of %d pixels moved, %d start again" % (name, int(moved.sum()), moved.size, fresh))
    assert name != "cornell" or 0 < fresh < moved.size  # what the box uncovered


# ------------------------------------------------------------------------------------------------------------------------ B. against the reprojection
def test_where_nothing_is_clipped_the_resolve_writes_the_reprojection_s_values(gpu_lib):
    current, now, history, then, counts, noise = random_frame(64, 36, seed=11)
    out, count, clip = develop.resolve(current, now, history, then, counts, noise=noise)
    ref_out, ref_count = develop.reproject(current, now, history, then, counts)
    usable = R.usable_pixels(current, noise)
    kept = (clip == 0) & usable  # a pixel that is not usable is the resolve's own rule: the reprojection knows no such pixel
    share = float(kept.mean())
    print("clip_out == 0 in %.1f %% of the pixels, %.1f %% of them with history" % (100 * share, 100 * float((count[kept] > 1).mean())))
    assert 0.1 <= share <= 0.9 and (count[kept] > 1).any()
    assert np.array_equal(out[kept], ref_out[kept], equal_nan=True) and np.array_equal(count[kept], ref_count[kept])  # zeros as values: fmaxf(-0, +0) may be either
    assert same_bits(out[~usable], current[~usable]) and (count[~usable] == 1).all()
    assert (count[clip > 0] <= ref_count[clip > 0]).all() and (count[clip > 0] < ref_count[clip > 0]).any()  # a clipped pixel forgets


# ------------------------------------------------------------------------------------------------------------------------ C. what it is for
SIZE, FRAMES, SPP, TRUTH_SPP = (64, 64), 12, 64, 4096
FIRST, STEP = -0.7, 0.15  # the tall box's offset along x in frame 0 and what a frame adds to it


@functools.lru_cache(maxsize=None)
def sliding_box():
    """Twelve frames of the Cornell box at 64 x 64 with the tall box sliding along x, rendered once for the tests below: each frame
    64 samples a pixel, denoised from its half films with its error image, accumulated once by develop.reproject and once by
    develop.resolve with defaults; 4,096 samples a pixel of the first and of the last pose. The box spans x = -4.72 .. -2.65 at
    rest between a wall at -5.5 and the short box, whose corner (-2.4, 2.72) it passes at an offset of 1.02: offsets -0.7 .. 0.95
    keep clear of both. A pixel is about 0.12 there, so a frame moves the box 1.2 pixels and the twelve frames 13."""
    world, cam, r, _ = scenes.build(scenes.c2_cornell(SIZE[0], SIZE[1], SPP), seed=3)
    world.set_objects([dict(first_triangle=0, num_triangles=12, first_sphere=0, num_spheres=0), dict(first_triangle=12, num_triangles=12, first_sphere=0, num_spheres=0)])
    world.scene(0)

    def pose(frame):
        m = np.eye(4, dtype=f32)
        m[0, 3] = FIRST + STEP * frame
        world.pose({0: (m, 1.0)})

    def frame_image(spp, seed, halves):
        r.pixel_samples, r.seed = spp, seed
        with r.session(SIZE, cam, world, halves=halves) as s:
            for _ in range(2):
                s.render(spp // 2)
            return s.denoised() if halves else s.linear()

    x, y = np.meshgrid(np.arange(SIZE[0], dtype=f32) + f32(0.5), np.arange(SIZE[1], dtype=f32) + f32(0.5))
    static = np.ones((SIZE[1], SIZE[0]), dtype=bool)
    plain = resolved = previous = None
    for frame in range(FRAMES):
        pose(frame)
        image, error = frame_image(SPP, 100 + frame, True)
        records = r.motion(SIZE, cam, world)
        static &= ((records["flags"] & abi.PYR_MOTION_HIT) != 0) & (np.abs(records["prev_x"] - x) <= 1e-3) & (np.abs(records["prev_y"] - y) <= 1e-3)
        if previous is None:
            plain, resolved = develop.reproject(image, records), develop.resolve(image, records, noise=error)
        else:
            static &= records["shape"] == previous["shape"]
            plain = develop.reproject(image, records, plain[0], previous, plain[1])
            resolved = develop.resolve(image, records, resolved[0], previous, resolved[1], noise=error)
        previous = records
        world.keep_previous()
    truth_last = frame_image(TRUTH_SPP, 7, False)
    pose(0)
    truth_first = frame_image(TRUTH_SPP, 8, False)
    world.close()
    return dict(static=static, last=image, plain=plain, resolved=resolved, truth_last=truth_last, truth_first=truth_first)


def luminance(image):
    return image.astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])


def rmse(a, b, where):
    return float(np.sqrt(np.mean((a[where].astype(np.float64) - b[where].astype(np.float64)) ** 2)))


def test_a_sliding_box_s_shadow_leaves_no_trail(gpu_lib):
    """Region A: the pixels whose records were static in every frame and whose true luminance differs between the first and the last
    pose by more than 20 % of the larger -- the floor and the walls the shadow crossed. Region B: the static pixels where it
    differs by less than 2 %. Over A the resolve must beat the running mean; over B it must beat the last denoised frame alone."""
    s = sliding_box()
    first, last = luminance(s["truth_first"]), luminance(s["truth_last"])
    change = np.abs(first - last) / np.maximum(np.maximum(first, last), 1e-12)
    A, B = s["static"] & (change > 0.20), s["static"] & (change < 0.02)
    print("static pixels %d of %d; region A %d pixels, region B %d" % (int(s["static"].sum()), s["static"].size, int(A.sum()), int(B.sum())))
    assert A.sum() >= 41 and B.sum() >= 41  # 1 % of the image
    figures = {(name, region): rmse(s[key][0] if key != "last" else s[key], s["truth_last"], where)
               for name, key in (("last frame alone", "last"), ("reprojection", "plain"), ("resolve", "resolved")) for region, where in (("A", A), ("B", B))}
    for (name, region), value in sorted(figures.items()):
        print("  RMSE over %s, %-17s %.5f" % (region, name, value))
    print("  resolve / reprojection over B: %.3f; mean count over A: reprojection %.2f, resolve %.2f; over B: %.2f, %.2f" % (
        figures["resolve", "B"] / figures["reprojection", "B"], float(s["plain"][1][A].mean()), float(s["resolved"][1][A].mean()), float(s["plain"][1][B].mean()),
        float(s["resolved"][1][B].mean())))
    dim = (s["truth_last"].max(axis=-1) < 1.0) & (s["truth_first"].max(axis=-1) < 1.0)  # recorded, not asserted: without the lamp and the fireflies both truths still hold
    for region, where in (("A", A & dim), ("B", B & dim)):
        print("  over the %d pixels of %s below 1.0 in both truths: last frame alone %.5f, reprojection %.5f, resolve %.5f" % (
            int(where.sum()), region, rmse(s["last"], s["truth_last"], where), rmse(s["plain"][0], s["truth_last"], where), rmse(s["resolved"][0], s["truth_last"], where)))
    assert figures["resolve", "A"] < figures["reprojection", "A"]
    assert figures["resolve", "B"] < figures["last frame alone", "B"]
