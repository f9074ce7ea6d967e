"""Motion blur over the motion records without a GPU (include/pyrite_gpu.h "motion blur over the motion records", DESIGN.md section
9j): the new names of the ABI in the header, abi.py and the library, every argument check before a device is looked for, the C++
wrappers through a stand-alone program, and the numpy restatement (tests/motion_blur_restatement.py, which
tests/test_gpu_motion_blur.py holds the kernels against) on properties of the rule itself."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import motion_blur_restatement as R
from pyrite_amd import abi, motion
from pyrite_amd import build as gpu_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pyrite_gpu.h")
f32 = np.float32
NEW_ENTRIES = ["pyr_image_motion_blur", "pyr_image_motion_blur_device", "pyr_session_motion_blurred"]
MOVING = R.MOTION_HIT | R.MOTION_IN_FRONT | 4


@pytest.fixture(scope="module")
def lib():
    gpu_build.build()
    return abi.bind(C.CDLL(gpu_build.OUT))


# ------------------------------------------------------------------------------------------------------------------------ the ABI
def test_header_abi_and_library_agree(lib, tmp_path):
    header = open(HEADER).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in abi.ENTRY_POINTS and hasattr(lib, name)
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "%s"' % HEADER, "int main(void){", 'printf("size %zu\\n", sizeof(PyrMotionBlurParams));']
    for field, _ in abi.PyrMotionBlurParams._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(PyrMotionBlurParams, %s));' % (field, field))
    lines += ['printf("shutter_default %.9g\\n", (double)PYR_MOTION_BLUR_SHUTTER);', 'printf("softness_default %.9g\\n", (double)PYR_MOTION_BLUR_DEPTH_SOFTNESS);',
              'printf("ints %u %u %u %u\\n", PYR_MOTION_BLUR_SAMPLES, PYR_MOTION_BLUR_MAX_RADIUS, PYR_MOTION_BLUR_MOST_SAMPLES, PYR_MOTION_BLUR_MOST_RADIUS);', "return 0;}"]
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines))
    subprocess.check_call(["gcc", "-o", exe, src])
    seen = dict(line.split(None, 1) for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(seen["size"]) == C.sizeof(abi.PyrMotionBlurParams) == 32
    for field, _ in abi.PyrMotionBlurParams._fields_:
        assert int(seen[field]) == getattr(abi.PyrMotionBlurParams, field).offset, field
    assert f32(float(seen["shutter_default"])) == f32(abi.PYR_MOTION_BLUR_SHUTTER) and f32(float(seen["softness_default"])) == f32(abi.PYR_MOTION_BLUR_DEPTH_SOFTNESS)
    assert [int(v) for v in seen["ints"].split()] == [abi.PYR_MOTION_BLUR_SAMPLES, abi.PYR_MOTION_BLUR_MAX_RADIUS, abi.PYR_MOTION_BLUR_MOST_SAMPLES, abi.PYR_MOTION_BLUR_MOST_RADIUS]
    assert f32(abi.PYR_MOTION_BLUR_DEPTH_SOFTNESS) == f32(abi.PYR_REPROJECT_DEPTH_TOLERANCE)
    assert R.RECORD == motion.RECORD
    assert "#define PYR_ABI_VERSION 5\n" in header and abi.PYR_ABI_VERSION == 5 and lib.pyr_abi_version() == 5  # additions only


# ------------------------------------------------------------------------------------------------------------------------ the argument checks
def blur_call(lib, entry="pyr_image_motion_blur", image=True, records=True, params=True, out=True, width=4, height=3, device=99, misalign=False, overlap=None, **fields):
    pixels = np.zeros((3, 4, 3), dtype=f32)
    store = np.zeros(3 * 4 * 32 + 16, dtype=np.uint8)
    start = store.ctypes.data + (-store.ctypes.data) % 16 + (4 if misalign else 0)
    p = abi.PyrMotionBlurParams(abi.PYR_MOTION_BLUR_SHUTTER, abi.PYR_MOTION_BLUR_SAMPLES, abi.PYR_MOTION_BLUR_MAX_RADIUS, abi.PYR_MOTION_BLUR_DEPTH_SOFTNESS, 0)
    for name, value in fields.items():
        if name == "reserved":
            p.reserved[value] = 1
        else:
            setattr(p, name, value)
    result = np.zeros((3, 4, 3), dtype=f32)
    target = {None: result.ctypes.data, "image": pixels.ctypes.data + 12 * 11, "motion": start + 32 * 11 + 16}[overlap]  # the last pixel of either input
    args = [pixels.ctypes.data if image else None, start if records else None, width, height, C.byref(p) if params else None, target if out else None, device]
    if entry.endswith("_device"):
        args.append(None)
    rc = getattr(lib, entry)(*args)
    return rc, lib.pyr_last_error().decode()


NAN, INF = float("nan"), float("inf")
BLUR_REFUSED = [
    (dict(image=False), "image"), (dict(records=False), "motion"), (dict(params=False), "params"), (dict(out=False), "out"), (dict(width=0), "width"), (dict(height=0), "height"),
    (dict(shutter=0.0), "shutter"), (dict(shutter=-0.5), "shutter"), (dict(shutter=1.5), "shutter"), (dict(shutter=NAN), "shutter"), (dict(shutter=INF), "shutter"),
    (dict(samples=0), "samples"), (dict(samples=65), "samples"), (dict(max_radius=0), "max_radius"), (dict(max_radius=65), "max_radius"),
    (dict(depth_softness=0.0), "depth_softness"), (dict(depth_softness=-1.0), "depth_softness"), (dict(depth_softness=NAN), "depth_softness"), (dict(depth_softness=INF), "depth_softness"),
    (dict(reserved=0), "reserved"), (dict(reserved=1), "reserved"), (dict(reserved=2), "reserved"),
]


def names_in(message):
    return message.replace("params->", " ").replace(":", " ").replace(",", " ").split()


@pytest.mark.parametrize("entry", ["pyr_image_motion_blur", "pyr_image_motion_blur_device"])
@pytest.mark.parametrize("change,name", BLUR_REFUSED)
def test_motion_blur_refuses_bad_arguments_by_name_before_a_device_is_looked_for(change, name, entry, lib):
    rc, message = blur_call(lib, entry=entry, **change)  # no device 99: the argument is still what is reported
    assert rc == abi.PYR_ERR_INVALID_ARGUMENT
    assert name in names_in(message), message


def test_the_device_form_refuses_misaligned_records_and_an_overlapping_out(lib):
    rc, message = blur_call(lib, entry="pyr_image_motion_blur_device", misalign=True)
    assert rc == abi.PYR_ERR_INVALID_ARGUMENT and "motion_device" in message and "16-byte" in message
    for which in ("image", "motion"):
        rc, message = blur_call(lib, entry="pyr_image_motion_blur_device", overlap=which)
        assert rc == abi.PYR_ERR_INVALID_ARGUMENT and "out_device overlaps %s_device" % which in message, message


@pytest.mark.parametrize("entry", ["pyr_image_motion_blur", "pyr_image_motion_blur_device"])
def test_motion_blur_size_then_device(entry, lib):
    rc, message = blur_call(lib, entry=entry, width=65536, height=65536)
    assert rc == abi.PYR_ERR_UNSUPPORTED and "2^32" in message
    assert blur_call(lib, entry=entry)[0] == abi.PYR_ERR_DEVICE
    assert blur_call(lib, entry=entry, shutter=1.0, samples=64, max_radius=64)[0] == abi.PYR_ERR_DEVICE  # the edges of the ranges are inside
    assert blur_call(lib, entry=entry, samples=1, max_radius=1, depth_softness=1e-30)[0] == abi.PYR_ERR_DEVICE
    if lib.pyr_device_count() <= 0:  # valid arguments where there is no GPU
        assert blur_call(lib, entry=entry, device=0)[0] == abi.PYR_ERR_DEVICE


def test_the_session_entry_refuses_by_name_before_a_device_is_looked_for(lib):
    stand_in = (C.c_char * 4096)()
    session = C.addressof(stand_in)
    develop, out = abi.PyrDevelopParams(), np.zeros(3, dtype=f32)
    good = abi.PyrMotionBlurParams(0.5, 15, 16, 0.02, 0)
    call = lib.pyr_session_motion_blurred
    assert call(None, None, C.byref(develop), C.byref(good), out.ctypes.data) == abi.PYR_ERR_INVALID_ARGUMENT and b"session" in lib.pyr_last_error()
    assert call(session, None, None, C.byref(good), out.ctypes.data) == abi.PYR_ERR_INVALID_ARGUMENT and b"develop_params" in lib.pyr_last_error()
    assert call(session, None, C.byref(develop), C.byref(good), None) == abi.PYR_ERR_INVALID_ARGUMENT and b"out" in lib.pyr_last_error()
    assert call(session, None, C.byref(develop), None, out.ctypes.data) == abi.PYR_ERR_INVALID_ARGUMENT and b"blur_params" in lib.pyr_last_error()
    bad = abi.PyrMotionBlurParams(0.5, 0, 16, 0.02, 0)
    assert call(session, None, C.byref(develop), C.byref(bad), out.ctypes.data) == abi.PYR_ERR_INVALID_ARGUMENT and b"blur_params->samples" in lib.pyr_last_error()
    assert call(session, None, C.byref(develop), C.byref(good), out.ctypes.data) == abi.PYR_ERR_INVALID_ARGUMENT and b"previous_camera" in lib.pyr_last_error()


# ------------------------------------------------------------------------------------------------------------------------ the C++ wrappers
def test_the_cpp_wrappers(lib, tmp_path):
    """pyrite::motion_blur and pyrite::motion_blur_params from a stand-alone program (tests/motion_blur_driver.cpp) linked against
    libpyrite_host.so: the ProjectError for buffers of the wrong size, the GpuError and its status for a parameter out of range, and
    with good arguments PYR_ERR_DEVICE here -- or, where there is a GPU, the input's bits for records without motion."""
    exe = str(tmp_path / "motion_blur_driver")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "motion_blur_driver.cpp"), "-L" + gpu_build.HOST_DIR, "-lpyrite_host", "-L" + gpu_build.CSRC, "-lpyrite_gpu",
                           "-Wl,-rpath," + gpu_build.HOST_DIR, "-Wl,-rpath," + gpu_build.CSRC])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-2000:]
    assert run.stdout.split()[0] == "ok"


# ------------------------------------------------------------------------------------------------------------------------ the rule itself
def records(width, height, dx=0.0, dy=0.0, depth=2.0, flags=MOVING):
    """Every pixel a hit whose point was (dx, dy) pixels further LEFT and UP a frame ago: it moves right and down by that much a frame."""
    rec = np.zeros((height, width), dtype=R.RECORD)
    x, y = np.meshgrid(np.arange(width, dtype=f32), np.arange(height, dtype=f32))
    rec["prev_x"], rec["prev_y"] = (x + f32(0.5)) - f32(dx), (y + f32(0.5)) - f32(dy)
    rec["prev_depth"] = rec["depth"] = f32(depth)
    rec["shape"], rec["flags"] = 7, flags
    return rec


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=f32).view(np.uint32), np.asarray(b, dtype=f32).view(np.uint32))


def test_records_without_motion_return_the_input_s_bits():
    rng = np.random.default_rng(19)
    image = rng.random((9, 21, 3), dtype=f32)
    image[3, 4] = (np.nan, -0.0, np.inf)
    assert same_bits(R.motion_blur(image, records(21, 9)), image)
    for name, value, flags in [("flags", None, R.MOTION_HIT), ("prev_x", np.nan, MOVING), ("prev_x", np.inf, MOVING), ("prev_y", -np.inf, MOVING), ("prev_y", np.nan, MOVING)]:
        rec = records(21, 9, dx=5.0, dy=-3.0, flags=flags)
        if value is not None:
            rec[name] = value
        assert same_bits(R.motion_blur(image, rec, max_radius=8), image), (name, value)
    below = records(21, 9, dx=1.9)  # half a shutter of 0.5: a half velocity of 0.475 pixels, below half a pixel
    assert same_bits(R.motion_blur(image, below), image)


@pytest.mark.parametrize("samples", [1, 2, 15, 64])
def test_a_constant_image_stays_constant_under_any_motion(samples):
    """out = S / W with W = w0 + w_1 + ... and S = w0*c + w_1*c + ..., all weights >= 0. Each of W's terms passes through at most
    `samples` additions, each of S's through one multiplication and at most `samples` additions, so W = sum w_k (1 + a_k) and
    S = c sum w_k (1 + b_k) with |a_k| <= samples u and |b_k| <= (samples + 1) u to first order, u = 2^-24. With weights of one sign
    S / W = c (1 + e), |e| <= (2 samples + 1) u, and the division rounds once more: (2 samples + 2) u, taken as (2 samples + 3) u
    for the terms of second order."""
    rng = np.random.default_rng(samples)
    height, width = 17, 33
    rec = records(width, height)
    rec["prev_x"] += rng.uniform(-40, 40, (height, width)).astype(f32)
    rec["prev_y"] += rng.uniform(-40, 40, (height, width)).astype(f32)
    rec["depth"] = rng.uniform(1, 10, (height, width)).astype(f32)
    rec["flags"][rng.random((height, width)) < 0.2] = R.MOTION_IN_FRONT  # misses among them
    colour = np.array([0.37, 1.0, 7.25], dtype=f32)
    image = np.broadcast_to(colour, (height, width, 3)).copy()
    out = R.motion_blur(image, rec, shutter=0.7, samples=samples, max_radius=8, seed=3)
    bound = (2 * samples + 3) * 2.0 ** -24
    worst = float((np.abs(out.astype(np.float64) - colour) / colour).max())
    print("constant image, %d taps: at most %.3g relative, bound %.3g" % (samples, worst, bound))
    assert worst <= bound


FOREGROUND, BACKGROUND = np.array([1, 0, 0], dtype=f32), np.array([0, 0, 1], dtype=f32)


def moving_square(samples=32):
    """A 4 x 4 square (depth 2, red) that moves 8 pixels a frame to the right over a static blue background (depth 10) in a 48 x 32
    image; shutter 1, so its half velocity is 4 pixels; tiles of 8."""
    width, height = 48, 32
    rec = records(width, height, depth=10.0)
    rec["shape"] = 3
    image = np.broadcast_to(BACKGROUND, (height, width, 3)).copy()
    rows, cols = slice(12, 16), slice(20, 24)
    moving = records(width, height, dx=8.0, depth=2.0)
    rec[rows, cols] = moving[rows, cols]
    image[rows, cols] = FOREGROUND
    out = R.motion_blur(image, rec, shutter=1.0, samples=samples, max_radius=8, seed=1)
    return image, rec, out, rows, cols


def test_a_square_that_moves_over_a_static_background():
    image, rec, out, rows, cols = moving_square()
    hx, hy, length, z = R.velocities(rec, 1.0, 8)
    assert np.array_equal(length[rows, cols], np.full((4, 4), 4, dtype=f32)) and np.count_nonzero(length) == 16
    neighbours = R.neighbour_of_pixels(R.neighbour_maxima(R.tile_maxima(hx, hy, length, 8)), 48, 32, 8)
    far = neighbours[..., 2] < 0.5
    assert far.any() and not far[rows, cols].any()
    assert same_bits(out[far], image[far])  # tiles nothing moves near: the copy
    assert not far[:24, 8:32].any() and far[:, :8].all() and far[:, 32:].all() and far[24:, :].all()  # the 3 x 3 block around the square's tile
    assert np.isfinite(out).all()
    red = out[..., 0]
    assert (red[12:16, 17:20] > 0).all() and (red[12:16, 24:27] > 0).all()  # behind the square and in front of it
    assert not red[:12].any() and not red[16:].any()  # the motion is horizontal
    assert (red[12:16, 20:24] < 1).all() and (out[12:16, 20:24, 2] > 0).all()  # the square lets the background through
    # The foreground's colour summed over the image: 16 before. The filter normalises per pixel, so it is not exactly conserved;
    # the weights bound it. A foreground pixel (l = 4, own weight 1/4): its taps fall on the square for offsets in an interval of
    # width 4 of the 8 the taps span -- samples/2 of them, one more or less -- at distance d <= 3.5 with
    # w = 2 (1 - d/4) + 2 cyl(d, 4)^2 >= 2.25; the others fall on the background at d >= 0.5 with w = (1 - d/4) <= 0.875, but for at
    # most one tap with d in [0.5, 0.525), where the cylinder term adds at most 1. It keeps at least
    # 2.25 (s/2 - 1) / (2.25 (s/2 - 1) + 0.875 (s/2 + 1) + 1) of its red: 0.68 at s = 32, so the sum is at least 0.68 * 16.
    # A background pixel (l = 0.5, own weight 2) receives red only through taps on the square, at most s/2 + 1 of them with
    # w = (1 - d/4) <= 1: at most (s/2 + 1) / (2 + s/2 + 1) = 0.895 of it is red, and only the 8 columns within 4 pixels of
    # the square in its 4 rows can be reached: at most 16 + 32 * 0.895.
    s = 32
    lower = 16 * 2.25 * (s / 2 - 1) / (2.25 * (s / 2 - 1) + 0.875 * (s / 2 + 1) + 1)
    upper = 16 + 32 * (s / 2 + 1) / (2 + s / 2 + 1)
    total = float(red.astype(np.float64).sum())
    print("red over the image: 16 before, %.3f after; bounds %.2f .. %.2f" % (total, lower, upper))
    assert lower <= total <= upper
    assert not red[12:16, :16].any() and not red[12:16, 28:].any()  # nothing beyond 4 pixels of the square


def test_a_velocity_of_a_thousand_pixels_is_clamped_and_its_taps_stay_in_the_3_x_3_block():
    width, height, edge = 48, 32, 8
    rec = records(width, height)
    rec[13, 21] = records(width, height, dx=2000.0, dy=-1200.0)[13, 21]  # a half velocity of (500, -300) at shutter 0.5
    hx, hy, length, z = R.velocities(rec, 0.5, edge)
    assert length[13, 21] == f32(edge) and np.count_nonzero(length) == 1
    assert abs(float(np.hypot(hx[13, 21], hy[13, 21])) - edge) <= 1e-5 and hx[13, 21] > 0 > hy[13, 21]
    rng = np.random.default_rng(5)
    taps = []
    out = R.motion_blur(rng.random((height, width, 3), dtype=f32), rec, samples=15, max_radius=edge, taps_out=taps)
    assert np.isfinite(out).all() and len(taps) == 15
    tile_x, tile_y = np.arange(width)[None, :] // edge, np.arange(height)[:, None] // edge
    for ax, ay, counted in taps:
        assert counted.any()
        assert (np.abs(ax[counted] // edge - np.broadcast_to(tile_x, ax.shape)[counted]) <= 1).all()
        assert (np.abs(ay[counted] // edge - np.broadcast_to(tile_y, ay.shape)[counted]) <= 1).all()


def test_the_tie_rules():
    width, height, edge = 24, 16, 8
    rec = records(width, height)
    moved = lambda dx, dy: records(width, height, dx=dx, dy=dy)  # noqa: E731
    rec[2, 5], rec[2, 3], rec[6, 1] = moved(0.0, 12.0)[2, 5], moved(12.0, 0.0)[2, 3], moved(-12.0, 0.0)[6, 1]  # equal lengths in tile 0: (3, 2) has the lowest index
    rec[10, 20] = moved(0.0, -12.0)[10, 20]  # tile 5, the same length again
    hx, hy, length, z = R.velocities(rec, 0.5, edge)
    assert length[2, 5] == length[2, 3] == length[6, 1] == length[10, 20] == f32(3)
    tiles = R.tile_maxima(hx, hy, length, edge)
    assert tuple(tiles[0, 0]) == (3, 0, 3) and tuple(tiles[1, 2]) == (0, -3, 3) and not tiles[0, 1:].any() and not tiles[1, :2].any()
    neighbours = R.neighbour_maxima(tiles)
    assert tuple(neighbours[0, 1]) == (3, 0, 3) and tuple(neighbours[1, 1]) == (3, 0, 3)  # tiles 0 and 5 tie in both blocks: tile 0 wins
    assert tuple(neighbours[0, 0]) == (3, 0, 3) and tuple(neighbours[0, 2]) == (0, -3, 3) and tuple(neighbours[1, 2]) == (0, -3, 3)
    rec[10, 20] = moved(0.0, -12.5)[10, 20]  # a little longer: now it wins where it is in reach
    hx, hy, length, z = R.velocities(rec, 0.5, edge)
    assert tuple(R.neighbour_maxima(R.tile_maxima(hx, hy, length, edge))[0, 1]) == (0, f32(-3.125), f32(3.125))


def test_a_tap_with_a_nan_colour_is_skipped_and_poisons_nothing():
    rng = np.random.default_rng(11)
    width, height = 24, 16
    image = rng.random((height, width, 3), dtype=f32)
    rec = records(width, height, dx=10.0, dy=6.0)
    clean = R.motion_blur(image, rec, shutter=1.0, max_radius=8)
    assert np.isfinite(clean).all() and not same_bits(clean, image)
    dirty = image.copy()
    dirty[7, 11, 1], dirty[9, 3, 0] = np.nan, np.inf
    out = R.motion_blur(dirty, rec, shutter=1.0, max_radius=8)
    bad = np.zeros((height, width), dtype=bool)
    bad[7, 11] = bad[9, 3] = True
    assert same_bits(out[bad], dirty[bad])  # a pixel that is not finite itself keeps its bits
    assert np.isfinite(out[~bad]).all()
    assert (out[~bad] != clean[~bad]).any()  # its neighbours went without it
