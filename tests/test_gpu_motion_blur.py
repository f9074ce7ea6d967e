"""Motion blur over the motion records on the GPU (include/pyrite_gpu.h "motion blur over the motion records", DESIGN.md section
9j) -- run with `-m gpu` on an MI355X.

The three kernels are held against the numpy restatement (tests/motion_blur_restatement.py) bit for bit on the output image: the
header spells every f32 operation and its order out, contraction is off on both sides, and the compiler's sqrt and division round
as numpy's do. Then the filter is held against what motion blur is: the mean of renders over the exposure."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_blur_restatement as R  # noqa: E402
import pose_cases  # noqa: E402

from pyrite_amd import abi, develop, motion, scenes  # noqa: E402
from pyrite_amd._lib import check, lib  # noqa: E402
from pyrite_amd.renderer import Camera, Renderer, World  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def assert_same_image(got, want, what):
    differs = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(differs) == 0, "%s: out differs in %d of %d floats, first %s: GPU %r, restatement %r" % (
        what, len(differs), got.size, tuple(differs[0]), got[tuple(differs[0])], want[tuple(differs[0])])


def blur_on_device(image, records, out_bits=None, **params):
    """`out_bits`: the 32 bits every float of `out` holds before the call (default: those of -1.0f)."""
    import torch

    h, w, _ = image.shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    image_dev, records_dev = dev(image), dev(records)
    out = torch.full((h * w * 3,), -1.0, dtype=torch.float32, device="cuda")
    if out_bits is not None:
        out = torch.full((h * w * 3,), out_bits, dtype=torch.int32, device="cuda").view(torch.float32)
    p = develop.motion_blur_params(**params)
    stream = torch.cuda.current_stream()
    check(lib().pyr_image_motion_blur_device(C.c_void_p(image_dev.data_ptr()), C.c_void_p(records_dev.data_ptr()), w, h, C.byref(p), C.c_void_p(out.data_ptr()), 0,
                                             C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    return out.cpu().numpy().reshape(h, w, 3)


# ------------------------------------------------------------------------------------------------------------------------ A. random records
def random_frame(width, height, seed):
    """(image, records): fractional motion of up to 100 pixels a frame in six pixels of ten -- beyond either clamp at shutter 0.5 --
    the rest still; misses, IN_FRONT clear, NaN, inf and 1e30 positions, runs of equal lengths in several directions, depths from a
    few values (so equal ones occur) and from a range, and a few colours that are not finite."""
    rng = np.random.default_rng(seed)
    shape = (height, width)
    n = width * height
    image = (4 * rng.random((height, width, 3), dtype=f32)).astype(f32)
    for value in (np.nan, np.inf, -np.inf):
        image.reshape(-1)[rng.integers(0, 3 * n, max(1, n // 40))] = value
    x, y = np.meshgrid(np.arange(width, dtype=f32), np.arange(height, dtype=f32))
    rec = np.zeros(shape, dtype=motion.RECORD)
    reach = np.where(rng.random(shape) < 0.5, 12.0, 100.0)
    moving = rng.random(shape) < 0.6
    dx, dy = np.where(moving, rng.uniform(-1, 1, shape) * reach, 0).astype(f32), np.where(moving, rng.uniform(-1, 1, shape) * reach, 0).astype(f32)
    ties = rng.random(shape) < 0.15  # (+-6, +-2.5) and (+-2.5, +-6): one length in eight directions
    swap = rng.random(shape) < 0.5
    tx, ty = np.where(swap, 6.0, 2.5) * rng.choice([-1.0, 1.0], shape), np.where(swap, 2.5, 6.0) * rng.choice([-1.0, 1.0], shape)
    dx, dy = np.where(ties, tx, dx).astype(f32), np.where(ties, ty, dy).astype(f32)
    rec["prev_x"], rec["prev_y"] = (x + f32(0.5)) - dx, (y + f32(0.5)) - dy
    for field, value in (("prev_x", np.nan), ("prev_y", np.inf), ("prev_x", 1e30), ("prev_y", -1e30), ("prev_x", -np.inf)):
        rec[field][rng.random(shape) < 0.02] = value
    hit = rng.random(shape) < 0.85
    rec["shape"] = np.where(hit, (1 << 30) | 3, abi.HIT_NONE)
    rec["flags"] = np.where(hit, abi.PYR_MOTION_HIT, 0) | np.where(rng.random(shape) < 0.9, abi.PYR_MOTION_IN_FRONT | abi.PYR_MOTION_INSIDE, 0)
    depth = np.where(rng.random(shape) < 0.5, rng.choice([2.0, 2.02, 2.05, 7.0], shape), rng.uniform(1, 50, shape))
    rec["depth"] = rec["prev_depth"] = np.where(hit, depth, 0).astype(f32)
    return image, rec


@pytest.mark.parametrize("max_radius", [8, 16])
@pytest.mark.parametrize("size", [(1, 1), (1, 5), (13, 7), (33, 17), (64, 36)], ids=lambda s: "%dx%d" % s)
def test_the_blur_is_the_restatement_bit_for_bit(size, max_radius, gpu_lib):
    width, height = size
    image, rec = random_frame(width, height, seed=100 * width + max_radius)
    for samples in (1, 2, 15):
        params = dict(samples=samples, max_radius=max_radius, seed=samples)
        want = R.motion_blur(image, rec, **params)
        got = develop.motion_blur(image, rec, **params)
        finite = np.isfinite(image).all(axis=-1)
        changed = int((got.view(np.uint32) != image.view(np.uint32)).any(axis=-1).sum())
        print("blur %dx%d, radius %d, %d taps: %d of %d pixels changed" % (width, height, max_radius, samples, changed, width * height))
        assert_same_image(got, want, "%dx%d radius %d taps %d" % (width, height, max_radius, samples))
        assert np.isfinite(got[finite]).all()
        assert width * height < 50 or 0 < changed
    assert_same_image(blur_on_device(image, rec, **params), got, "the device entry against the host entry")
    assert_same_image(develop.motion_blur(image, rec, **params), got, "two calls")
    other = dict(shutter=1.0, samples=7, max_radius=max_radius, depth_softness=0.1, seed=0xDEADBEEF)
    assert_same_image(develop.motion_blur(image, rec, **other), R.motion_blur(image, rec, **other), "other parameters")


@pytest.mark.parametrize("max_radius", [1, 5, 64])
def test_other_tile_edges(max_radius, gpu_lib):
    """Tiles of one pixel, tiles that divide neither the image nor the gather's 16 x 16 blocks, and one tile of 4,096 pixels: sixteen
    passes of the velocity kernel's workgroup over it."""
    image, rec = random_frame(70, 67, seed=max_radius)
    params = dict(shutter=1.0, samples=5, max_radius=max_radius)
    assert_same_image(develop.motion_blur(image, rec, **params), R.motion_blur(image, rec, **params), "radius %d" % max_radius)


def test_static_records_return_the_input_s_bits(gpu_lib):
    image, rec = random_frame(70, 37, seed=4)
    x, y = np.meshgrid(np.arange(70, dtype=f32), np.arange(37, dtype=f32))
    rec["prev_x"], rec["prev_y"] = x + f32(0.5), y + f32(0.5)
    assert_same_image(develop.motion_blur(image, rec), image, "records without motion")
    assert_same_image(blur_on_device(image, rec), image, "records without motion, device entry")
    rec["prev_x"][:, 50:] -= f32(30)  # the right of the image moves: the tiles out of its reach still copy
    got = develop.motion_blur(image, rec, max_radius=8)
    assert_same_image(got, R.motion_blur(image, rec, max_radius=8), "a static half")
    assert_same_image(got[:, :40], image[:, :40], "the tiles out of reach")
    assert (got[:, 50:].view(np.uint32) != image[:, 50:].view(np.uint32)).any()


# ------------------------------------------------------------------------------------------------------------------------ B. real records
def turned(cam, angle, axis=(0, 1, 0), shift=(0.0, 0.0, 0.0)):
    """`cam` turned about an axis of its own by `angle` and moved by `shift` in its own frame."""
    m = np.array(cam.c.cam_to_world[:], dtype=np.float64).reshape(4, 4).T @ pose_cases.rotation4(axis, angle, translation=shift).astype(np.float64)
    c = abi.PyrCamera.from_buffer_copy(cam.c)
    c.cam_to_world = (C.c_float * 16)(*[float(v) for v in m.astype(f32).T.reshape(-1)])
    return Camera(c)


def linear_render(r, size, cam, world, samples, seed):
    r.pixel_samples, r.seed = samples, seed
    film = r.new_film(*size)
    r.render(film, cam, world)
    return develop.develop_linear(film)


def camera_right(cam):
    """The world direction of the camera's x axis."""
    m = np.array(cam.c.cam_to_world[:], dtype=np.float64).reshape(4, 4).T
    return m[:3, 0] / np.linalg.norm(m[:3, 0])


def box_slide(cam, world, r, size, pixels):
    """The world translation along the camera's x axis that moves the tall box of the Cornell box (triangles 0..11) by `pixels`
    pixels: from the depth the motion pass sees it at and the inverse of to_view_area, pixels = shift / depth * view_plane * max(w, h)/2."""
    rec = r.motion(size, cam, world)
    box = (rec["shape"] >> 30 == 1) & ((rec["shape"] & 0x3FFFFFFF) < 12)
    assert box.sum() > 50
    depth = float(np.median(rec["depth"][box]))
    return camera_right(cam) * (pixels * depth / (cam.c.view_plane * max(size) / 2)), box


def test_real_records_of_a_posed_box(gpu_lib):
    world, cam, r, _ = scenes.build(scenes.c2_cornell(64, 64, 16), seed=5)
    size = (64, 64)
    world.set_objects([pose_cases.triangles(0, 12), pose_cases.triangles(12, 12)])
    world.scene(0)
    shift, box = box_slide(cam, world, r, size, 6.0)
    world.keep_previous()
    world.pose({0: (pose_cases.rotation4((0, 0, 1), 0.0, translation=tuple(shift)), 1.0)})
    rec = r.motion(size, cam, world)
    image = linear_render(r, size, cam, world, 16, 7)
    x = np.arange(64, dtype=f32)[None, :] + f32(0.5)
    moved = np.abs(x - rec["prev_x"]) > 3
    print("cornell, the tall box 6 pixels aside: %d pixels moved by more than 3" % int(moved.sum()))
    assert 50 < moved.sum() < 64 * 64 // 2
    for params in (dict(shutter=1.0, max_radius=8), dict()):
        got = develop.motion_blur(image, rec, **params)
        assert_same_image(got, R.motion_blur(image, rec, **params), "cornell posed %r" % (params,))
        assert (got.view(np.uint32) != image.view(np.uint32)).any() and (got.view(np.uint32) == image.view(np.uint32)).all(axis=-1).any()
    world.close()


def test_real_records_of_a_turning_camera_and_of_a_sky(gpu_lib):
    project = scenes.c3_mesh_in_box(width=64, height=36, pixel_samples=16)  # the pair tree
    world, cam, r = World(scenes.c3_flat(segments=96, sides=48)), Camera.from_project(project["camera"]), Renderer.from_project(project["renderer"], seed=6)
    rec = r.motion((64, 36), cam, world, previous_camera=turned(cam, 0.1))
    image = linear_render(r, (64, 36), cam, world, 16, 6)
    hx, hy, length, z = R.velocities(rec, 1.0, 16)
    print("c3, camera turned by 0.1: half velocities %.2f .. %.2f pixels" % (float(length.min()), float(length.max())))
    assert length.min() > 0.5  # every pixel moves
    for params in (dict(shutter=1.0), dict(max_radius=4, samples=9)):
        assert_same_image(develop.motion_blur(image, rec, **params), R.motion_blur(image, rec, **params), "c3 turned %r" % (params,))
    world.close()
    world, cam, r, _ = scenes.build(scenes.lamps_example(13, 7, 16), seed=5)  # spheres and a plane under a sky, 13 x 7
    level = cam
    for pitch in (0.0, 0.15, 0.3, 0.45, 0.6, 0.75, 0.9):  # the image is flatter than the example's: look up until the sky comes into it
        cam = turned(level, pitch, axis=(1, 0, 0))
        rec = r.motion((13, 7), cam, world, previous_camera=turned(cam, 0.2, shift=(0.3, 0.0, 0.0)))
        if (rec["shape"] == abi.HIT_NONE).any():
            break
    print("lamps 13x7: %d of 91 pixels see the sky" % int((rec["shape"] == abi.HIT_NONE).sum()))
    assert (rec["shape"] == abi.HIT_NONE).any() and (rec["shape"] != abi.HIT_NONE).any()
    image = linear_render(r, (13, 7), cam, world, 16, 5)
    for params in (dict(shutter=1.0, max_radius=8), dict(max_radius=3)):
        got = develop.motion_blur(image, rec, **params)
        assert_same_image(got, R.motion_blur(image, rec, **params), "lamps 13x7 %r" % (params,))
        assert (got.view(np.uint32) != image.view(np.uint32)).any()
    world.close()


def test_a_session_blurs_its_own_frame_and_keeps_its_film(gpu_lib):
    world, cam, r, _ = scenes.build(scenes.c2_cornell(64, 64, 16), seed=5)  # a world of its own: a session takes the scene
    r.pixel_samples = 16
    away = turned(cam, 0.05, shift=(0.0, 0.1, 0.0))
    params = dict(shutter=1.0, samples=11, max_radius=8, seed=2)
    with r.session((64, 64), cam, world) as s:
        s.render(8)
        film = s.film()
        got = s.motion_blurred(away, **params)
        want = develop.motion_blur(s.linear(), s.motion(away), **params)
        assert_same_image(got, want, "the session entry against its parts")
        assert (got.view(np.uint32) != s.linear().view(np.uint32)).any()
        assert film.grains.tobytes() == s.film().grains.tobytes(), "the session's film changed under the blur"
        assert_same_image(s.motion_blurred(away, **params), got, "two calls")
        s.render(8)  # a pass may follow
        s.sync()
        assert s.samples_done == 16 and film.grains.tobytes() != s.film().grains.tobytes()
    world.close()


# ------------------------------------------------------------------------------------------------------------------------ C. against what motion blur is
def exposure_case():
    """The Cornell box at 64 x 64 whose tall box slides 8 pixels a frame along the image's x axis, shutter 1: (truth, frame, records),
    the truth the mean of 16 renders of 64 samples a pixel at poses spaced evenly over [t - 1/2, t + 1/2], the frame the render at t
    with 1,024 samples a pixel, the records those of t against the pose at t - 1."""
    size = (64, 64)
    world, cam, r, _ = scenes.build(scenes.c2_cornell(64, 64, 16), seed=5)
    world.set_objects([pose_cases.triangles(0, 12), pose_cases.triangles(12, 12)])
    world.scene(0)
    shift, _ = box_slide(cam, world, r, size, 8.0)
    at = lambda tau: {0: (pose_cases.rotation4((0, 0, 1), 0.0, translation=tuple(shift * tau)), 1.0)}  # noqa: E731
    truth = np.zeros((64, 64, 3), dtype=np.float64)
    for k in range(16):
        world.pose(at(-0.5 + (k + 0.5) / 16))
        truth += linear_render(r, size, cam, world, 64, 100 + k)
    truth /= 16
    world.pose(at(-1.0))
    world.keep_previous()
    world.pose(at(0.0))
    rec = r.motion(size, cam, world)
    frame = linear_render(r, size, cam, world, 1024, 99)
    world.close()
    return truth, frame, rec


def test_the_blurred_frame_is_nearer_the_exposure_than_the_frame(gpu_lib):
    """RMSE against the mean of renders over the exposure, over the pixels whose neighbour maximum is at least one pixel: the
    blurred frame's must be the smaller. An inequality, not a tolerance. Measured on an MI355X: 0.10216 for the frame, 0.09739 for
    the blurred frame, over 1,856 pixels (profiles/r19_motion_blur.txt)."""
    truth, frame, rec = exposure_case()
    params = dict(shutter=1.0, samples=15, max_radius=8)
    blurred = develop.motion_blur(frame, rec, **params)
    assert_same_image(blurred, R.motion_blur(frame, rec, **params), "the frame of the exposure case")
    hx, hy, length, z = R.velocities(rec, 1.0, 8)
    near = R.neighbour_of_pixels(R.neighbour_maxima(R.tile_maxima(hx, hy, length, 8)), 64, 64, 8)[..., 2] >= 1
    rmse = lambda a: float(np.sqrt(((a.astype(np.float64) - truth)[near] ** 2).mean()))  # noqa: E731
    plain, ours = rmse(frame), rmse(blurred)
    print("exposure of the sliding box: largest half velocity %.2f pixels, %d of 4096 pixels near motion; RMSE against the mean of 16 renders: frame %.5f, blurred frame %.5f"
          % (float(length.max()), int(near.sum()), plain, ours))
    assert 3 <= length.max() <= 5 and near.any() and not near.all()
    assert ours < plain
