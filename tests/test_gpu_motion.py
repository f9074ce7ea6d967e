"""The motion pass and the accumulation over frames on the GPU (include/pyrite_gpu.h "motion records and accumulation over
frames") -- run with `-m gpu` on an MI355X.

Both kernels are held against the numpy restatement (tests/motion_restatement.py) bit for bit: the header spells every f32
operation and its order out, contraction is off on both sides, and sqrt32 and the compiler's division round as numpy does. The
restatement is fed with pyr_scene_intersect's hits of its own pixel-centre rays and with pyr_camera_world_to_cam's matrix, so what
is compared is the arithmetic after the hit -- and, through `shape` and `depth`, that the pass walks the ray the feature pass does."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_restatement as R  # noqa: E402
import pose_cases  # noqa: E402
import skin_cases  # noqa: E402

from pyrite_amd import abi, develop, motion, scenes  # noqa: E402
from pyrite_amd._lib import check, lib  # noqa: E402
from pyrite_amd.features import RECORD as FEATURE_RECORD  # noqa: E402
from pyrite_amd.renderer import Camera, Renderer, World  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------ helpers
def c2_world(width=64, height=64):
    world, cam, r, _ = scenes.build(scenes.c2_cornell(width, height, 16), seed=5)
    return world, cam, r


def c3_world():  # tests/test_gpu_features.py c3_case: the pair tree, 8 x 8 squares ragged at the bottom
    project = scenes.c3_mesh_in_box(width=64, height=36, pixel_samples=16)
    return World(scenes.c3_flat(segments=96, sides=48)), Camera.from_project(project["camera"]), Renderer.from_project(project["renderer"], seed=6)


def lamps_world():  # spheres and a plane, sky pixels
    world, cam, r, _ = scenes.build(scenes.lamps_example(96, 64, 16), seed=5)
    return world, cam, r


STATIC = {"c2_cornell": (c2_world, (64, 64)), "c3_shaped": (c3_world, (64, 36)), "lamps_example": (lamps_world, (96, 64)), "c2_13x7": (c2_world, (13, 7)),
          "c2_1x5": (c2_world, (1, 5))}


@functools.lru_cache(maxsize=None)
def static_case(name):
    """(world, camera, renderer, (width, height)), built once: the tests of case A keep or drop its snapshot and change nothing else."""
    make, size = STATIC[name]
    return make() + (size,)


def planes_of(world):
    d = world.desc
    return np.ctypeslib.as_array(d.planes, shape=(d.num_planes, 8)).copy() if d.num_planes else np.zeros((0, 8), dtype=f32)


def restated(world, cam, previous_cam, size, previous=None):
    """The records the header asks for, from the scene's own hits of the restated rays. `previous`: the geometry() kept, or None."""
    width, height = size
    c = cam.c
    rays = R.pixel_rays(c.cam_to_world[:], c.view_plane, c.focus_distance, width, height)
    hits, _, _ = world.intersect(rays.reshape(-1, 6))
    now = world.geometry()
    return R.motion_records(rays, hits.reshape(height, width), motion.world_to_cam(previous_cam), previous_cam.c.view_plane, spheres=now["spheres"], planes=planes_of(world),
                            previous_positions=None if previous is None else previous["positions"], previous_spheres=None if previous is None else previous["spheres"])


def feature_records(world, cam, size):
    """pyr_render_features with grid = 1 and no albedo buffer."""
    width, height = size
    desc, fp = abi.PyrFilmDesc(width, height, 64, 380.0, 400.0), abi.PyrFeatureParams(1, 0)
    out = np.zeros((height, width), dtype=FEATURE_RECORD)
    check(lib().pyr_render_features(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(fp), None, out.ctypes.data))
    return out


def assert_records_equal(got, want, what):
    for field in R.RECORD.names:
        a, b = got[field].view(np.uint32), want[field].view(np.uint32)
        differs = np.argwhere(a != b)
        assert len(differs) == 0, "%s: %s differs in %d of %d pixels, first %s: GPU %r, restatement %r" % (
            what, field, len(differs), got.size, tuple(differs[0]), got[field][tuple(differs[0][:2])], want[field][tuple(differs[0][:2])])
    assert got.tobytes() == want.tobytes(), what


def turned(cam, angle, axis=(0, 1, 0), shift=(0.0, 0.0, 0.0)):
    """`cam` turned about an axis of its own by `angle` and moved by `shift` in its own frame."""
    m = np.array(cam.c.cam_to_world[:], dtype=np.float64).reshape(4, 4).T @ pose_cases.rotation4(axis, angle, translation=shift).astype(np.float64)
    c = abi.PyrCamera.from_buffer_copy(cam.c)
    c.cam_to_world = (C.c_float * 16)(*[float(v) for v in m.astype(f32).T.reshape(-1)])
    return Camera(c)


# ------------------------------------------------------------------------------------------------------------------------ A. static scenes
@pytest.mark.parametrize("snapshot", [False, True], ids=["no_snapshot", "snapshot"])
@pytest.mark.parametrize("name", sorted(STATIC))
def test_a_scene_that_did_not_move(name, snapshot, gpu_lib):
    world, cam, r, size = static_case(name)
    width, height = size
    world.keep_previous(snapshot)
    got = r.motion(size, cam, world)
    features = feature_records(world, cam, size)
    assert np.array_equal(got["shape"], features["shape"]), "shape against the feature pass: %d pixels differ" % int((got["shape"] != features["shape"]).sum())
    assert got["depth"].tobytes() == features["depth"].tobytes(), "depth against the feature pass: %d pixels differ" % int((got["depth"] != features["depth"]).sum())
    want = restated(world, cam, cam, size, world.geometry() if snapshot else None)
    hit = got["shape"] != abi.HIT_NONE
    x, y = np.meshgrid(np.arange(width, dtype=f32) + f32(0.5), np.arange(height, dtype=f32) + f32(0.5))
    ex, ey = np.abs(got["prev_x"] - x)[hit], np.abs(got["prev_y"] - y)[hit]
    print("motion %s %s: %d of %d pixels hit, |prev - centre| max %.3g, %.3g pixel; bit-equal to the restatement: %s" % (
        name, "with a snapshot" if snapshot else "without", int(hit.sum()), hit.size, float(ex.max()) if hit.any() else 0.0, float(ey.max()) if hit.any() else 0.0,
        got.tobytes() == want.tobytes()))
    assert_records_equal(got, want, name)
    assert hit.any() and (ex <= 1e-2).all() and (ey <= 1e-2).all()
    assert ((got["flags"][hit] & 7) == 7).all()  # a point the camera sees is in front of it and inside the image
    assert not got["reserved"].any()
    if name == "lamps_example":
        assert (~hit).any() and (got["flags"][~hit] == (abi.PYR_MOTION_IN_FRONT | abi.PYR_MOTION_INSIDE)).all()  # the sky follows the camera
        assert not got["depth"][~hit].any() and not got["prev_depth"][~hit].any()
        assert (np.abs(got["prev_x"] - x)[~hit] <= 1e-2).all() and (np.abs(got["prev_y"] - y)[~hit] <= 1e-2).all()
    world.keep_previous(False)


# ------------------------------------------------------------------------------------------------------------------------ B. moved geometry
BOX_POSES = {0: (pose_cases.rotation4((0, 0, 1), 0.2, translation=(0.3, 0.0, 0.0)), 1.0), 1: (pose_cases.rotation4((1, 2, 3), 0.1, translation=(-0.2, 0.3, 0.25)), 1.0)}


def check_moved(world, cam, r, size, previous, what, expect_moved=True):
    """The pass against the restatement for the camera itself and for a previous camera turned so far that part of the scene is
    behind it; the flags are what the restatement says, and both kinds occur."""
    still = r.motion(size, cam, world)
    assert_records_equal(still, restated(world, cam, cam, size, previous), what)
    if expect_moved:
        hit = still["shape"] != abi.HIT_NONE
        x, y = np.meshgrid(np.arange(size[0], dtype=f32) + f32(0.5), np.arange(size[1], dtype=f32) + f32(0.5))
        moved = hit & ((np.abs(still["prev_x"] - x) > 0.25) | (np.abs(still["prev_y"] - y) > 0.25))
        print("%s: %d of %d hit pixels moved by more than a quarter pixel" % (what, int(moved.sum()), int(hit.sum())))
        assert moved.any() and (hit & ~moved).any()
    away = turned(cam, 1.5, shift=(0.3, 0.1, -0.2))
    got = r.motion(size, cam, world, previous_camera=away)
    want = restated(world, cam, away, size, previous)
    assert np.array_equal(got["flags"], want["flags"])
    assert_records_equal(got, want, what + ", previous camera turned away")
    front, inside = (want["flags"] & abi.PYR_MOTION_IN_FRONT) != 0, (want["flags"] & abi.PYR_MOTION_INSIDE) != 0
    assert front.any() and (~front).any() and (front & ~inside).any(), what  # (the camera itself, above, has the points inside)
    assert not got["prev_x"][~front].any() and not got["prev_y"][~front].any()


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_posed_boxes_are_found_where_they_were(mode, gpu_lib):
    world, cam, r = c2_world()
    world.set_objects([pose_cases.triangles(0, 12), pose_cases.triangles(12, 12)])  # cornell_box.obj: the tall box, the short box, then the walls
    world.scene(0)
    previous = world.geometry()
    world.keep_previous()
    world.pose(BOX_POSES, mode=mode)  # the snapshot survives the rebuild: indices are the description's
    assert not np.array_equal(world.geometry()["positions"], previous["positions"])
    check_moved(world, cam, r, (64, 64), previous, "c2 boxes posed, " + mode)
    # a second frame: the snapshot is replaced by the posed geometry, the boxes go back
    previous = world.geometry()
    world.keep_previous()
    world.pose({}, mode=mode)
    check_moved(world, cam, r, (64, 64), previous, "c2 boxes back at rest, " + mode)
    world.close()


def test_a_skinned_mesh_is_found_where_it_was(gpu_lib):
    world, cam, r, _, ranges, rest, skins = skin_cases.build("cornell", "bend")
    (index, _), = skins.items()
    world.skin({index: skin_cases.THREE})
    previous = world.geometry()
    world.keep_previous()
    world.skin({index: skin_cases.THREE[::-1].copy()})  # another table of the same three joints
    assert not np.array_equal(world.geometry()["positions"], previous["positions"])
    check_moved(world, cam, r, (64, 64), previous, "cornell skinned, two joint tables", expect_moved=False)
    world.close()


def test_a_sphere_that_moved_and_grew_is_found_where_it_was(gpu_lib):
    world, cam, r, _, ranges = pose_cases.build("three_spheres")
    world.scene(0)
    previous = world.geometry()
    world.keep_previous()
    world.pose({0: (pose_cases.rotation4((0, 0, 1), 0.0, translation=(0.2, 0.1, -0.15)), 1.25), 2: (pose_cases.rotation4((0, 1, 0), 0.4), 0.8)})
    now = world.geometry()
    assert not np.array_equal(now["spheres"][:, :3], previous["spheres"][:, :3]) and not np.array_equal(now["spheres"][:, 3], previous["spheres"][:, 3])
    check_moved(world, cam, r, (64, 64), previous, "three spheres moved and scaled")
    world.keep_previous(False)  # without a snapshot only the camera moves
    assert_records_equal(r.motion((64, 64), cam, world), restated(world, cam, cam, (64, 64), None), "three spheres, snapshot dropped")
    world.close()


# ------------------------------------------------------------------------------------------------------------------------ C. entry forms
def test_the_device_entry_writes_the_host_entry_bytes_and_two_calls_agree(gpu_lib):
    import torch

    world, cam, r, size = static_case("c3_shaped")
    width, height = size
    away = turned(cam, 0.1, shift=(0.2, 0.0, 0.0))
    first, second = r.motion(size, cam, world, previous_camera=away), r.motion(size, cam, world, previous_camera=away)
    assert first.tobytes() == second.tobytes(), "two calls differ"
    desc = abi.PyrFilmDesc(width, height, 64, 380.0, 400.0)
    records = torch.full((height, width, 8), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    check(lib().pyr_render_motion_device(world.scene(0), C.byref(cam.c), C.byref(away.c), C.byref(desc), C.c_void_p(records.data_ptr()), C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    assert records.cpu().numpy().tobytes() == first.tobytes()
    rc = lib().pyr_render_motion_device(world.scene(0), C.byref(cam.c), C.byref(away.c), C.byref(desc), C.c_void_p(records.data_ptr() + 8), C.c_void_p(stream.cuda_stream))
    assert rc == abi.PYR_ERR_INVALID_ARGUMENT and b"16-byte" in lib().pyr_last_error()


def test_a_session_gives_the_same_records_and_keeps_its_film(gpu_lib):
    world, cam, r = c2_world()  # a world of its own: a session takes the scene
    r.pixel_samples = 8
    away = turned(cam, 0.05, shift=(0.0, 0.1, 0.0))
    world.keep_previous()
    plain = r.motion((64, 64), cam, world, previous_camera=away)
    with r.session((64, 64), cam, world) as s:
        before = s.motion(away)
        s.render(4)
        s.sync()
        film = s.film()
        world.keep_previous()  # a live session does not forbid it: it only reads
        between = s.motion(away)
        again = s.film()
        assert film.grains.tobytes() == again.grains.tobytes(), "the session's film changed under a motion pass"
    assert before.tobytes() == plain.tobytes() and between.tobytes() == plain.tobytes()
    world.close()


def test_the_render_is_untouched_by_a_motion_pass(gpu_lib):
    from test_gpu_features import assert_same_film

    world, cam, r = c2_world()
    before, after = r.new_film(64, 64), r.new_film(64, 64)
    r.render(before, cam, world)
    world.keep_previous()
    r.motion((64, 64), cam, world, previous_camera=turned(cam, 0.1))
    r.render(after, cam, world)
    assert_same_film(after, before, "C2 render after a motion pass against the render before it")
    world.close()


# ------------------------------------------------------------------------------------------------------------------------ D. pyr_image_reproject
def random_frame(width, height, seed):
    """(current, motion, history, history_motion, history_count): fractional motion of up to three pixels, three shapes and the
    sky, history depths on both sides of the 2 % tolerance, NaN and inf in the history and in prev_x / prev_y, counts from 0 up."""
    rng = np.random.default_rng(seed)
    n = width * height
    current, history = rng.random((height, width, 3), dtype=f32), (4 * rng.random((height, width, 3), dtype=f32)).astype(f32)
    for value in (np.nan, np.inf, -np.inf):
        history.reshape(-1)[rng.integers(0, 3 * n, max(1, n // 20))] = value
    shapes = np.array([(1 << 30) | 3, (1 << 30) | 4, 5, abi.HIT_NONE], dtype=np.uint32)
    x, y = np.meshgrid(np.arange(width, dtype=f32), np.arange(height, dtype=f32))
    now, then = np.zeros((height, width), dtype=motion.RECORD), np.zeros((height, width), dtype=motion.RECORD)
    now["shape"], then["shape"] = shapes[rng.integers(0, 4, (height, width))], shapes[rng.integers(0, 4, (height, width))]
    now["prev_x"] = x + f32(0.5) + rng.uniform(-3, 3, (height, width)).astype(f32)
    now["prev_y"] = y + f32(0.5) + rng.uniform(-3, 3, (height, width)).astype(f32)
    whole = rng.random((height, width)) < 0.2  # some land on a pixel centre exactly: one tap of weight 1, three of weight 0
    now["prev_x"][whole], now["prev_y"][whole] = np.floor(now["prev_x"][whole]) + f32(0.5), np.floor(now["prev_y"][whole]) + f32(0.5)
    for field, value in (("prev_x", np.nan), ("prev_y", np.inf), ("prev_x", 1e30), ("prev_y", -1e30), ("prev_x", -np.inf)):
        now[field][rng.random((height, width)) < 0.03] = value
    hit = now["shape"] != abi.HIT_NONE
    now["flags"] = np.where(hit, abi.PYR_MOTION_HIT, 0) | np.where(rng.random((height, width)) < 0.9, abi.PYR_MOTION_IN_FRONT, 0)
    now["prev_depth"] = np.where(hit, rng.uniform(1, 50, (height, width)), 0).astype(f32)
    now["depth"] = now["prev_depth"]
    then["depth"] = f32(10)
    now["prev_depth"] = np.where(hit, (10 * (1 + rng.uniform(-0.04, 0.04, (height, width)))).astype(f32), f32(0))  # |d| <= 4 % around the 2 % line
    then["depth"][rng.random((height, width)) < 0.03] = np.nan
    counts = rng.integers(0, 6, (height, width)).astype(f32)
    return current, now, history, then, counts


def reproject_on_device(current, now, history, then, counts, out_bits=None, **params):
    """`out_bits`: the 32 bits every float of the two outputs holds before the call (default: 0.0f)."""
    import torch

    h, w, _ = current.shape
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    buffers = [dev(a) for a in (current, now, history, then, counts)]
    out, count = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda"), torch.zeros(h * w, dtype=torch.float32, device="cuda")
    if out_bits is not None:
        out, count = (torch.full((n,), out_bits, dtype=torch.int32, device="cuda").view(torch.float32) for n in (h * w * 3, h * w))
    p = abi.PyrReprojectParams(params.get("depth_tolerance", abi.PYR_REPROJECT_DEPTH_TOLERANCE), params.get("max_history", abi.PYR_REPROJECT_MAX_HISTORY))
    stream = torch.cuda.current_stream()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    check(lib().pyr_image_reproject_device(*[ptr(b) for b in buffers], w, h, C.byref(p), ptr(out), ptr(count), 0, C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    return out.cpu().numpy().reshape(h, w, 3), count.cpu().numpy().reshape(h, w)


def same_bits(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("size", [(13, 7), (1, 5), (64, 36)], ids=lambda s: "%dx%d" % s)
def test_reproject_is_the_restatement_bit_for_bit(size, gpu_lib):
    width, height = size
    frame = random_frame(width, height, seed=width)
    want, want_count = R.reproject(*frame)
    got, got_count = develop.reproject(*frame)
    kept = int((want_count > 1).sum())
    print("reproject %dx%d: %d of %d pixels found history" % (width, height, kept, width * height))
    assert width * height < 50 or 0 < kept < width * height
    differs = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(differs) == 0, "out differs in %d floats, first %s: GPU %r, restatement %r" % (len(differs), tuple(differs[0]), got[tuple(differs[0])], want[tuple(differs[0])])
    assert same_bits(got_count, want_count)
    on_device, on_device_count = reproject_on_device(*frame)
    assert same_bits(on_device, got) and same_bits(on_device_count, got_count), "the device entry differs from the host entry"
    again, again_count = develop.reproject(*frame)
    assert same_bits(again, got) and same_bits(again_count, got_count), "two calls differ"
    # a first frame, and other parameters
    first, ones = develop.reproject(frame[0], frame[1])
    assert same_bits(first, frame[0]) and same_bits(ones, np.ones((height, width), dtype=f32))
    for params in (dict(depth_tolerance=0.0, max_history=1.0), dict(depth_tolerance=0.05, max_history=3.0)):
        want, want_count = R.reproject(*frame, **params)
        got, got_count = develop.reproject(*frame, **params)
        assert same_bits(got, want) and same_bits(got_count, want_count), params


def identity_records(width, height, dx=0.0):
    rec = np.zeros((height, width), dtype=motion.RECORD)
    x, y = np.meshgrid(np.arange(width, dtype=f32), np.arange(height, dtype=f32))
    rec["prev_x"], rec["prev_y"] = x + f32(0.5) + f32(dx), y + f32(0.5)
    rec["prev_depth"] = rec["depth"] = f32(3)
    rec["shape"], rec["flags"] = 9, 7
    return rec


@pytest.mark.parametrize("max_history", [32.0, 4.0])
def test_identity_motion_accumulates_the_running_mean(max_history, gpu_lib):
    """The update H + (c - H) / (n + 1) is the running mean in exact arithmetic; in f32 each of the K = 8 steps rounds three times
    on values no larger than the largest input: 8 ulps of that value bound the drift."""
    width, height, frames = 13, 7, 8
    rng = np.random.default_rng(8)
    images = (16 * rng.random((frames, height, width, 3), dtype=f32)).astype(f32)
    rec = identity_records(width, height)
    out, count = develop.reproject(images[0], rec)
    for k in range(1, frames):
        out, count = develop.reproject(images[k], rec, out, rec, count, max_history=max_history)
        assert np.array_equal(count, np.full((height, width), min(k + 1, max_history + 1), dtype=f32))
    if max_history >= frames:
        mean = images.astype(np.float64).mean(axis=0)
        bound = 8 * float(np.spacing(images.max()))
        worst = float(np.abs(out.astype(np.float64) - mean).max())
        print("running mean of %d frames: worst %.3g, bound %.3g" % (frames, worst, bound))
        assert worst <= bound
    else:
        assert float(count.max()) == 5.0


def test_a_translation_carries_an_impulse_one_pixel_and_failed_taps_start_again(gpu_lib):
    width, height = 13, 7
    history = np.zeros((height, width, 3), dtype=f32)
    history[3, 5] = (8, 4, 2)
    current = np.zeros((height, width, 3), dtype=f32)
    ones = np.ones((height, width), dtype=f32)
    out, count = develop.reproject(current, identity_records(width, height, dx=-1.0), history, identity_records(width, height), ones)
    want = np.zeros((height, width, 3), dtype=f32)
    want[3, 6] = (4, 2, 1)
    assert np.array_equal(out, want)
    assert np.array_equal(count[:, 1:], 2 * ones[:, 1:]) and np.array_equal(count[:, 0], ones[:, 0])  # column 0 came in from outside
    # four taps that all fail: another shape all around, a depth beyond the tolerance, no frames behind them, a NaN in each
    current = np.full((height, width, 3), 2, dtype=f32)
    history = np.full((height, width, 3), 7, dtype=f32)
    now, then = identity_records(width, height, dx=0.4), identity_records(width, height)
    now["prev_y"] += f32(0.3)  # four taps with weight each
    now["shape"][1, :] = 10
    now["prev_depth"][2, :] = f32(3.2)
    counts = ones.copy()
    counts[3:5, :] = 0
    history[5:7, :, 1] = np.nan
    out, count = develop.reproject(current, now, history, then, counts)
    assert np.array_equal(count[1:3], ones[1:3]) and np.array_equal(out[1:3], current[1:3])
    assert np.array_equal(count[3, :], ones[3, :]) and np.array_equal(count[5, :], ones[5, :]) and np.array_equal(out[3], current[3]) and np.array_equal(out[5], current[5])
    assert (count[0, :-1] == 2).all() and np.allclose(out[0, :-1], 4.5, atol=1e-5)  # the row above them keeps its history: 7 + (2 - 7) / 2
    want, want_count = R.reproject(current, now, history, then, counts)
    assert same_bits(out, want) and same_bits(count, want_count)
