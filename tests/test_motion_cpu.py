"""Motion records and accumulation over frames without a GPU (include/pyrite_gpu.h "motion records and accumulation over frames",
DESIGN.md section 9i): the new names of the ABI in the header, abi.py and the library, every argument check before a device is
looked for, pyr_camera_world_to_cam against numpy's f64 inverse, and the numpy restatement (tests/motion_restatement.py, which
tests/test_gpu_motion.py holds the kernels against) pinned on cases worked out by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import motion_restatement as R
from pyrite_amd import abi, motion, scenes
from pyrite_amd import build as gpu_build
from pyrite_amd.renderer import Camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW_ENTRIES = ["pyr_scene_keep_previous", "pyr_camera_world_to_cam", "pyr_render_motion", "pyr_render_motion_device", "pyr_session_motion", "pyr_image_reproject",
               "pyr_image_reproject_device"]


@pytest.fixture(scope="module")
def lib():
    gpu_build.build()
    return abi.bind(C.CDLL(gpu_build.OUT))


# ------------------------------------------------------------------------------------------------------------------------ the ABI
def test_header_abi_and_library_agree(lib):
    header = open(os.path.join(ROOT, "include", "pyrite_gpu.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in abi.ENTRY_POINTS and hasattr(lib, name)
    assert C.sizeof(abi.PyrMotionPixel) == 32 == motion.RECORD.itemsize == R.RECORD.itemsize
    assert [(n, motion.RECORD.fields[n][1]) for n in motion.RECORD.names] == [(n, getattr(abi.PyrMotionPixel, n).offset) for n, _ in abi.PyrMotionPixel._fields_]
    assert motion.RECORD == R.RECORD
    assert C.sizeof(abi.PyrReprojectParams) == 16
    for name, value in [("MOTION_HIT", "1u"), ("MOTION_IN_FRONT", "2u"), ("MOTION_INSIDE", "4u"), ("REPROJECT_DEPTH_TOLERANCE", "0.02f"), ("REPROJECT_MAX_HISTORY", "32.0f")]:
        assert re.search(r"#define PYR_%s %s\b" % (name, re.escape(value)), header), name
    assert (abi.PYR_MOTION_HIT, abi.PYR_MOTION_IN_FRONT, abi.PYR_MOTION_INSIDE) == (1, 2, 4) == (R.MOTION_HIT, R.MOTION_IN_FRONT, R.MOTION_INSIDE)
    assert (abi.PYR_REPROJECT_DEPTH_TOLERANCE, abi.PYR_REPROJECT_MAX_HISTORY) == (0.02, 32.0)
    assert f32(abi.PYR_REPROJECT_DEPTH_TOLERANCE) == f32(abi.PYR_DENOISE_SIGMA_DEPTH)
    assert "#define PYR_ABI_VERSION 5\n" in header and abi.PYR_ABI_VERSION == 5 and lib.pyr_abi_version() == 5  # additions only


# ------------------------------------------------------------------------------------------------------------------------ the camera helper
def cornell_camera():
    return Camera.from_project(scenes.c2_cornell(64, 64, 1)["camera"])


def camera_of(matrix, view_plane=1.5):
    """abi.PyrCamera with the 4x4 `matrix` (as written on paper) as cam_to_world."""
    c = abi.PyrCamera()
    c.cam_to_world = (C.c_float * 16)(*[float(v) for v in np.asarray(matrix, dtype=f32).T.reshape(-1)])
    c.view_plane, c.focus_distance, c.aperture = view_plane, 5.0, 0.0
    return c


def random_camera(rng):
    """A rotation about a random axis, a uniform scale in [0.25, 4] and a translation of up to 50 units."""
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    angle = rng.uniform(-np.pi, np.pi)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    rotation = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    m = np.eye(4)
    m[:3, :3] = rotation * rng.uniform(0.25, 4.0)
    m[:3, 3] = rng.uniform(-50, 50, 3)
    return camera_of(m)


def ulps_apart(a, b):
    """How many float32 steps lie between a and b, element by element (same sign or zero)."""
    ia, ib = a.astype(f32).view(np.int32).astype(np.int64), b.astype(f32).view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def test_world_to_cam_is_the_f64_inverse_rounded_once(lib):
    rng = np.random.default_rng(18)
    cameras = [cornell_camera().c] + [random_camera(rng) for _ in range(100)]
    worst = 0
    for c in cameras:
        got = motion.world_to_cam(c)
        m = np.array(c.cam_to_world[:], dtype=np.float64).reshape(4, 4).T
        want = np.linalg.inv(m).astype(f32).T.reshape(-1)  # column-major
        assert got[3] == 0 and got[7] == 0 and got[11] == 0 and got[15] == 1
        rows = [k for k in range(16) if k % 4 != 3]
        worst = max(worst, int(ulps_apart(got[rows], want[rows]).max()))
    print("world_to_cam against numpy's f64 inverse: at most %d ulp apart" % worst)
    assert worst <= 1
    identity = motion.world_to_cam(camera_of(np.eye(4)))
    assert np.array_equal(identity, np.eye(4, dtype=f32).reshape(-1))


def test_world_to_cam_refusals(lib):
    out = (C.c_float * 16)()
    good = camera_of(np.eye(4))
    assert lib.pyr_camera_world_to_cam(None, out) == abi.PYR_ERR_INVALID_ARGUMENT
    assert lib.pyr_camera_world_to_cam(C.byref(good), None) == abi.PYR_ERR_INVALID_ARGUMENT
    for bad_value in (float("nan"), float("inf")):
        m = np.eye(4)
        m[1, 3] = bad_value
        assert lib.pyr_camera_world_to_cam(C.byref(camera_of(m)), out) == abi.PYR_ERR_INVALID_ARGUMENT and b"finite" in lib.pyr_last_error()
    for row in ([0, 0, 0, 2], [0, 1e-30, 0, 1], [1, 0, 0, 1]):
        m = np.eye(4)
        m[3] = row
        assert lib.pyr_camera_world_to_cam(C.byref(camera_of(m)), out) == abi.PYR_ERR_INVALID_ARGUMENT and b"last row" in lib.pyr_last_error()
    singular = np.eye(4)
    singular[2, :3] = singular[1, :3]
    assert lib.pyr_camera_world_to_cam(C.byref(camera_of(singular)), out) == abi.PYR_ERR_INVALID_ARGUMENT and b"determinant" in lib.pyr_last_error()
    assert lib.pyr_camera_world_to_cam(C.byref(good), out) == abi.PYR_OK


# ------------------------------------------------------------------------------------------------------------------------ the argument checks
def motion_call(lib, entry="pyr_render_motion", scene=True, camera=True, previous=True, film=True, pixels=True, width=4, height=3, previous_matrix=None):
    """One motion entry with a stand-in scene: every refusal below comes before the scene is read and before a device is looked for."""
    stand_in = (C.c_char * 4096)()
    cam = camera_of(np.eye(4))
    prev = camera_of(np.eye(4) if previous_matrix is None else previous_matrix)
    desc = abi.PyrFilmDesc(width, height, 64, 380.0, 400.0)
    out = np.zeros((3, 4), dtype=motion.RECORD)
    args = [C.addressof(stand_in) if scene else None, C.byref(cam) if camera else None, C.byref(prev) if previous else None, C.byref(desc) if film else None,
            out.ctypes.data if pixels else None]
    if entry.endswith("_device"):
        args.append(None)
    rc = getattr(lib, entry)(*args)
    return rc, lib.pyr_last_error().decode()


NAN_CAMERA = np.eye(4)
NAN_CAMERA[0, 0] = np.nan
MOTION_REFUSED = [
    (dict(scene=False), "scene"), (dict(camera=False), "camera"), (dict(previous=False), "previous_camera"), (dict(film=False), "film"), (dict(pixels=False), "pixels"),
    (dict(width=0), "zero-sized"), (dict(height=0), "zero-sized"), (dict(width=65536, height=65536), "2^32"),
    (dict(previous_matrix=NAN_CAMERA), "previous_camera"), (dict(previous_matrix=np.zeros((4, 4))), "previous_camera"),
]


@pytest.mark.parametrize("entry", ["pyr_render_motion", "pyr_render_motion_device"])
@pytest.mark.parametrize("change,name", MOTION_REFUSED)
def test_the_motion_entries_refuse_bad_arguments_by_name_before_a_device_is_looked_for(change, name, entry, lib):
    rc, message = motion_call(lib, entry=entry, **change)
    assert rc == abi.PYR_ERR_INVALID_ARGUMENT
    assert name in message, message


def test_the_motion_entries_without_a_device(lib):
    assert lib.pyr_scene_keep_previous(None, 1) == abi.PYR_ERR_INVALID_ARGUMENT and b"null scene" in lib.pyr_last_error()
    assert lib.pyr_scene_keep_previous(None, 0) == abi.PYR_ERR_INVALID_ARGUMENT
    assert lib.pyr_session_motion(None, None, None) == abi.PYR_ERR_INVALID_ARGUMENT and b"session" in lib.pyr_last_error()
    stand_in = (C.c_char * 4096)()
    assert lib.pyr_session_motion(C.addressof(stand_in), None, None) == abi.PYR_ERR_INVALID_ARGUMENT and b"previous_camera" in lib.pyr_last_error()
    misaligned = np.zeros(64, dtype=np.uint8)
    cam, desc = camera_of(np.eye(4)), abi.PyrFilmDesc(1, 1, 64, 380.0, 400.0)
    rc = lib.pyr_render_motion_device(C.addressof(stand_in), C.byref(cam), C.byref(cam), C.byref(desc), misaligned.ctypes.data + 4, None)
    assert rc == abi.PYR_ERR_INVALID_ARGUMENT and b"16-byte" in lib.pyr_last_error()
    if lib.pyr_device_count() <= 0:  # valid arguments where there is no GPU: the device is what is missing, and the scene is never read
        for entry in ("pyr_render_motion", "pyr_render_motion_device"):
            rc, message = motion_call(lib, entry=entry)
            assert rc == abi.PYR_ERR_DEVICE, message


def reproject_call(lib, entry="pyr_image_reproject", current=True, records=True, history=(False, False, False), params=True, out=True, count=True, width=4, height=3,
                   device=99, **fields):
    image, rec, counts = np.zeros((3, 4, 3), dtype=f32), np.zeros((3, 4), dtype=motion.RECORD), np.ones((3, 4), dtype=f32)
    p = abi.PyrReprojectParams(abi.PYR_REPROJECT_DEPTH_TOLERANCE, abi.PYR_REPROJECT_MAX_HISTORY)
    for name, value in fields.items():
        if name == "reserved":
            p.reserved[1] = value
        else:
            setattr(p, name, value)
    result, result_count = np.zeros((3, 4, 3), dtype=f32), np.zeros((3, 4), dtype=f32)
    args = [image.ctypes.data if current else None, rec.ctypes.data if records else None, image.ctypes.data if history[0] else None, rec.ctypes.data if history[1] else None,
            counts.ctypes.data if history[2] else None, width, height, C.byref(p) if params else None, result.ctypes.data if out else None,
            result_count.ctypes.data if count else None, device]
    if entry.endswith("_device"):
        args.append(None)
    rc = getattr(lib, entry)(*args)
    return rc, lib.pyr_last_error().decode()


REPROJECT_REFUSED = [
    (dict(current=False), "current"), (dict(records=False), "motion"), (dict(params=False), "params"), (dict(out=False), "out"), (dict(count=False), "count_out"),
    (dict(history=(True, False, False)), "history"), (dict(history=(True, True, False)), "history"), (dict(history=(False, True, True)), "history"),
    (dict(history=(False, False, True)), "history"),
    (dict(width=0), "width"), (dict(height=0), "height"),
    (dict(depth_tolerance=-0.5), "depth_tolerance"), (dict(depth_tolerance=float("nan")), "depth_tolerance"), (dict(depth_tolerance=float("inf")), "depth_tolerance"),
    (dict(max_history=0.5), "max_history"), (dict(max_history=float("nan")), "max_history"), (dict(max_history=float("inf")), "max_history"),
    (dict(reserved=1), "reserved"),
]


@pytest.mark.parametrize("entry", ["pyr_image_reproject", "pyr_image_reproject_device"])
@pytest.mark.parametrize("change,name", REPROJECT_REFUSED)
def test_reproject_refuses_bad_arguments_by_name_before_a_device_is_looked_for(change, name, entry, lib):
    rc, message = reproject_call(lib, entry=entry, **change)  # no device 99: the argument is still what is reported
    assert rc == abi.PYR_ERR_INVALID_ARGUMENT
    assert name in message.replace("params->", " ").replace(":", " ").replace(",", " ").split(), message


@pytest.mark.parametrize("entry", ["pyr_image_reproject", "pyr_image_reproject_device"])
def test_reproject_size_then_device(entry, lib):
    rc, message = reproject_call(lib, entry=entry, width=65536, height=65536)
    assert rc == abi.PYR_ERR_UNSUPPORTED and "2^32" in message
    assert reproject_call(lib, entry=entry)[0] == abi.PYR_ERR_DEVICE
    assert reproject_call(lib, entry=entry, history=(True, True, True), depth_tolerance=0.0, max_history=1.0)[0] == abi.PYR_ERR_DEVICE  # the edges of the ranges are inside
    if lib.pyr_device_count() <= 0:  # valid arguments where there is no GPU
        assert reproject_call(lib, entry=entry, device=0)[0] == abi.PYR_ERR_DEVICE


# ------------------------------------------------------------------------------------------------------------------------ the restatement by hand
def records(width, height, dx=0.0, dy=0.0, shape=7, depth=2.0):
    """Every pixel a hit of one shape whose point was (dx, dy) pixels further right and down a frame ago."""
    rec = np.zeros((height, width), dtype=R.RECORD)
    x, y = np.meshgrid(np.arange(width, dtype=f32), np.arange(height, dtype=f32))
    rec["prev_x"], rec["prev_y"] = x + f32(0.5) + f32(dx), y + f32(0.5) + f32(dy)
    rec["prev_depth"] = rec["depth"] = f32(depth)
    rec["shape"], rec["flags"] = shape, R.MOTION_HIT | R.MOTION_IN_FRONT | R.MOTION_INSIDE
    return rec


def test_the_restatement_on_identity_motion():
    rng = np.random.default_rng(1)
    current, history = rng.random((5, 6, 3), dtype=f32), rng.random((5, 6, 3), dtype=f32)
    rec = records(6, 5)
    first, one = R.reproject(current, rec)
    assert np.array_equal(first, current) and np.array_equal(one, np.ones((5, 6), dtype=f32))
    out, count = R.reproject(current, rec, history, rec, np.full((5, 6), 3, dtype=f32))
    assert np.array_equal(count, np.full((5, 6), 4, dtype=f32))
    assert np.array_equal(out, history + (current - history) / f32(4))  # one tap of weight 1: H = history exactly
    capped, count = R.reproject(current, rec, history, rec, np.full((5, 6), 40, dtype=f32), max_history=8.0)
    assert np.array_equal(count, np.full((5, 6), 9, dtype=f32)) and np.array_equal(capped, history + (current - history) / f32(9))


def test_the_restatement_on_a_one_pixel_shift():
    current = np.zeros((4, 7, 3), dtype=f32)
    history = np.zeros((4, 7, 3), dtype=f32)
    history[2, 3] = (8, 4, 2)  # an impulse
    rec_then, rec_now = records(7, 4), records(7, 4, dx=-1.0)  # every point was one pixel further left
    out, count = R.reproject(current, rec_now, history, rec_then, np.ones((4, 7), dtype=f32))
    want = np.zeros((4, 7, 3), dtype=f32)
    want[2, 4] = (4, 2, 1)  # moved one pixel right, averaged with a black frame
    assert np.array_equal(out, want)
    assert np.array_equal(count[:, 1:], np.full((4, 6), 2, dtype=f32)) and np.array_equal(count[:, 0], np.ones(4, dtype=f32))  # column 0 came in from outside


@pytest.mark.parametrize("dx,dy,lost", [(-0.5, 0.0, "left"), (0.5, 0.0, "right"), (0.0, -0.5, "top"), (0.0, 0.5, "bottom")])
def test_the_restatement_drops_a_tap_outside_each_border(dx, dy, lost):
    """Half a pixel of motion: two taps of weight 0.5 (the other two weigh 0). At the border the motion comes from, one of the
    two lies outside; what is left is renormalised, so a constant history stays that constant and the count stays whole."""
    width, height = 5, 4
    current = np.zeros((height, width, 3), dtype=f32)
    history = np.full((height, width, 3), 6, dtype=f32)
    ramp = np.arange(width * height, dtype=f32).reshape(height, width)
    history[..., 0] = ramp
    rec = records(width, height, dx=dx, dy=dy)
    out, count = R.reproject(current, rec, history, records(width, height), np.full((height, width), 2, dtype=f32))
    assert np.array_equal(count, np.full((height, width), 3, dtype=f32))
    assert np.array_equal(out[..., 1], np.full((height, width), 4, dtype=f32))  # 6 + (0 - 6) / 3
    border = {"left": np.s_[:, 0], "right": np.s_[:, -1], "top": np.s_[0, :], "bottom": np.s_[-1, :]}[lost]
    assert np.array_equal(out[..., 0][border], (ramp + (0 - ramp) / f32(3))[border])  # the one tap inside is the pixel itself
    inner = {"left": np.s_[:, 1:], "right": np.s_[:, :-1], "top": np.s_[1:, :], "bottom": np.s_[:-1, :]}[lost]
    step = {"left": -1, "right": 1, "top": -width, "bottom": width}[lost]
    mean = ramp + f32(0.5 * step)  # the mean of the pixel and its neighbour on the side the motion comes from
    assert np.array_equal(out[..., 0][inner], (mean + (0 - mean) / f32(3))[inner])


def test_the_restatement_s_tap_rules():
    current = np.full((3, 3, 3), 1, dtype=f32)
    history = np.full((3, 3, 3), 5, dtype=f32)
    rec = records(3, 3)
    ones = np.ones((3, 3), dtype=f32)
    then = records(3, 3)
    then["shape"][0, 0] = 8  # another surface
    then["depth"][0, 1] = f32(2.0) * f32(1.03)  # beyond the tolerance of 2 %
    then["depth"][0, 2] = f32(2.0) * f32(1.01)  # within it
    counts = ones.copy()
    counts[1, 0] = 0  # no frames behind it
    bad = history.copy()
    bad[1, 1, 2] = np.nan
    bad[1, 2, 0] = np.inf
    now = rec.copy()
    now["prev_x"][2, 0] = np.nan
    now["prev_y"][2, 1] = f32(1e30)
    now["flags"][2, 2] = R.MOTION_HIT  # behind the previous camera
    out, count = R.reproject(current, now, bad, then, counts)
    fresh = np.array([[1, 1, 0], [1, 1, 1], [1, 1, 1]], dtype=bool)
    assert np.array_equal(count, np.where(fresh, f32(1), f32(2)))
    assert np.array_equal(out[fresh], current[fresh]) and np.array_equal(out[0, 2], np.full(3, 3, dtype=f32))
    sky = records(3, 3, shape=R.HIT_NONE, depth=0.0)
    sky["flags"] = R.MOTION_IN_FRONT | R.MOTION_INSIDE
    sky_then = sky.copy()
    sky_then["depth"][1, 1] = 9  # a miss compares no depth
    out, count = R.reproject(current, sky, history, sky_then, ones)
    assert np.array_equal(count, 2 * ones) and np.array_equal(out, np.full((3, 3, 3), 3, dtype=f32))


def test_the_restated_rays_and_records_of_a_camera_that_did_not_move():
    """A wall of one triangle pair at z = -4 in front of an identity camera: every hit point projects back to its own pixel
    centre, a miss follows its direction, and depth is the distance."""
    width, height = 8, 6
    cam = camera_of(np.eye(4), view_plane=1.5)
    rays = R.pixel_rays(cam.cam_to_world[:], cam.view_plane, cam.focus_distance, width, height)
    assert np.array_equal(rays[..., :3], np.zeros((height, width, 3), dtype=f32))
    assert np.allclose(np.linalg.norm(rays[..., 3:], axis=-1), 1, atol=1e-6) and (rays[..., 5] < 0).all()
    assert (rays[0, :, 4] > 0).all() and (rays[-1, :, 4] < 0).all() and (rays[:, 0, 3] < 0).all()  # y up, x right
    hits = np.zeros((height, width), dtype=np.dtype([("distance", "<f4"), ("shape", "<u4"), ("u", "<f4"), ("v", "<f4")]))
    t = f32(-4) / rays[..., 5]
    hits["distance"], hits["shape"] = t, (R.SHAPE_PLANE << 30) | 0
    hits["shape"][:, -1] = R.HIT_NONE
    planes = np.array([[0, 0, -4, 0, 0, 1, 1, 1]], dtype=f32)
    w = motion.world_to_cam(cam)
    rec = R.motion_records(rays, hits, w, cam.view_plane, planes=planes)
    x, y = np.meshgrid(np.arange(width, dtype=f32) + f32(0.5), np.arange(height, dtype=f32) + f32(0.5))
    assert np.abs(rec["prev_x"] - x).max() <= 1e-4 and np.abs(rec["prev_y"] - y).max() <= 1e-4
    assert np.array_equal(rec["flags"][:, :-1], np.full((height, width - 1), 7)) and np.array_equal(rec["flags"][:, -1], np.full(height, 6))
    assert np.abs(rec["depth"][:, :-1] - t[:, :-1]).max() == 0 and np.abs(rec["prev_depth"][:, :-1] - t[:, :-1]).max() <= 1e-5
    assert not rec["depth"][:, -1].any() and not rec["prev_depth"][:, -1].any() and not rec["reserved"].any()
    behind = np.eye(4)
    behind[:3, :3] = np.diag([-1.0, 1.0, -1.0])  # turned half round about y: the wall is behind it
    rec = R.motion_records(rays, hits, motion.world_to_cam(camera_of(behind)), 1.5, planes=planes)
    assert np.array_equal(rec["flags"][:, :-1], np.full((height, width - 1), 1)) and not rec["flags"][:, -1].any()
    assert not rec["prev_x"].any() and not rec["prev_y"].any()
