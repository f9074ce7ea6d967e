"""Lens blur over the feature records on the GPU (include/pyrite_gpu.h "lens blur over the feature records")
-- run with `-m gpu` on an MI355X.

The kernel is held against the numpy restatement (tests/lens_blur_restatement.py) bit for bit on the output image: the header
spells every f32 operation and its order out, contraction is off on both sides, and the compiler's sqrt and division round as
numpy's do. The restatement visits every offset of the window; the kernel stops at its workgroup's reach, which may not show. Then
the filter is held against what lens blur is: a render through the lens."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lens_blur_restatement as R  # noqa: E402
import pose_cases  # noqa: E402

from pyrite_amd import abi, develop, features, scenes  # noqa: E402
from pyrite_amd._lib import check, lib  # noqa: E402
from pyrite_amd.renderer import Camera  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
FAR_PLANE = float(2 ** 20)  # a view plane so far off that 1 + t rounds to 1 at every pixel: z is the record's depth, bit for bit


def assert_same_image(got, want, what):
    differs = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(differs) == 0, "%s: out differs in %d of %d floats, first %s: GPU %r, restatement %r" % (
        what, len(differs), got.size, tuple(differs[0]), got[tuple(differs[0])], want[tuple(differs[0])])


def kept(got, image):
    """[height, width] bool: the pixels that carry the input's bits."""
    return (got.view(np.uint32) == image.view(np.uint32)).all(axis=-1)


def blur_on_device(image, records, out_bits=None, **params):
    """`out_bits`: the 32 bits every float of `out` holds before the call (default: those of -1.0f)."""
    import torch

    h, w, _ = image.shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    image_dev, records_dev = dev(image), dev(records)
    out = torch.full((h * w * 3,), -1.0, dtype=torch.float32, device="cuda")
    if out_bits is not None:
        out = torch.full((h * w * 3,), out_bits, dtype=torch.int32, device="cuda").view(torch.float32)
    p = develop.lens_blur_params(**params)
    stream = torch.cuda.current_stream()
    check(lib().pyr_image_lens_blur_device(C.c_void_p(image_dev.data_ptr()), C.c_void_p(records_dev.data_ptr()), w, h, C.byref(p), C.c_void_p(out.data_ptr()), 0,
                                           C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    return out.cpu().numpy().reshape(h, w, 3)


def aperture_for(A, width, height, focus_distance, view_plane):
    """The aperture whose scale is A pixels of blur per unit of |1 - f/z|."""
    return (A * focus_distance / (view_plane * max(width, height) * 0.5)) ** 2


# ------------------------------------------------------------------------------------------------------------------------ A. random records
FOCUS, PLANE, SCALE = 5.0, 2.4, 10.0


def depths_in_focus(width, height, view_plane, focus_distance):
    """float32 [height, width]: per pixel a ray depth whose axial depth is focus_distance bit for bit, so that c is 0 exactly. z =
    depth / s with s = sqrt(1 + t) in [1, 1.2): while depth stays in focus_distance's binade a step of one ulp of depth moves the
    quotient by less than one ulp, so one of the few neighbours of focus_distance * s lands on it."""
    rec = np.zeros((height, width), dtype=R.RECORD)
    rec["coverage"] = 1
    rec["depth"] = 1
    s = f32(1) / R.circles(rec, focus_distance, 0.0, view_plane, 1)[2]  # z of depth 1 is 1 / s
    best = (f32(focus_distance) * s).astype(f32)
    found = np.zeros((height, width), dtype=bool)
    for step in (0, 1, -1, 2, -2, 3, -3):
        trial = best.copy()
        for _ in range(abs(step)):
            trial = np.nextafter(trial, f32(np.inf if step > 0 else 0))
        rec["depth"] = trial
        hit = (R.circles(rec, focus_distance, 0.0, view_plane, 1)[2] == f32(focus_distance)) & ~found
        best[hit], found = trial[hit], found | hit
    assert found.all()
    return best


def random_frame(width, height, seed, strip=True):
    """(image, records). Hits and misses, partial coverage, depths from a few values on either side of the focus distance (so ties
    at the tolerance occur) and from a range that runs from in front of it to far behind, depth 0, NaN and inf, and a few colours
    that are not finite. With `strip` the left third lies exactly at the focus distance and, among the rest, what is nearer than
    the focus stays below c = 2.5 -- but for a few pixels at c = 9 in the last columns of an image at least 33 wide -- so that
    the strip's far side is out of every blur's reach: there sharp and blurred pixels meet and some keep their bits. Without it
    anything goes."""
    rng = np.random.default_rng(seed)
    shape = (height, width)
    n = width * height
    image = (4 * rng.random((height, width, 3), dtype=f32)).astype(f32)
    rec = np.zeros(shape, dtype=features.RECORD)
    rec["normal"] = rng.standard_normal((height, width, 3)).astype(f32)
    rec["shape"], rec["material"] = (1 << 30) | 3, 2
    near = [FOCUS / (1 + 2.5 / SCALE), FOCUS / (1 + 1.0 / SCALE), FOCUS * 0.98, FOCUS * 0.9799] if strip else [0.8, 1.0, 2.0, 2.04, FOCUS * 0.98]
    few = np.array(near + [FOCUS, FOCUS * 1.02, FOCUS * 1.0201, 7.0, 7.14, 50.0], dtype=f32)
    low = FOCUS / (1 + 2.5 / SCALE) if strip else 0.5
    depth = np.where(rng.random(shape) < 0.5, rng.choice(few, shape), rng.uniform(low, 60.0, shape)).astype(f32)
    if strip and width >= 33:
        last = np.zeros(shape, dtype=bool)
        last[:, width - 4:] = rng.random((height, 4)) < 0.3
        depth[last] = f32(FOCUS / (1 + 9.0 / SCALE))
    rec["depth"] = depth
    rec["coverage"] = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 1.0, 1.0], dtype=f32), shape)
    for value in (0.0, np.nan, np.inf, -1.0):
        rec["depth"][rng.random(shape) < 0.02] = value
    if strip:
        cols = slice(0, max(width // 3, 1))
        rec["depth"][:, cols] = depths_in_focus(width, height, PLANE, FOCUS)[:, cols]
        rec["coverage"][:, cols] = 1
    for value in (np.nan, np.inf, -np.inf):
        image.reshape(-1)[rng.integers(0, 3 * n, max(1, n // 40))] = value
    return image, rec


@pytest.mark.parametrize("max_radius", [1, 5, 16])
@pytest.mark.parametrize("size", [(1, 1), (1, 5), (13, 7), (33, 17), (64, 36)], ids=lambda s: "%dx%d" % s)
def test_the_blur_is_the_restatement_bit_for_bit(size, max_radius, gpu_lib):
    width, height = size
    image, rec = random_frame(width, height, seed=100 * width + max_radius)
    params = dict(focus_distance=FOCUS, aperture=aperture_for(SCALE, width, height, FOCUS, PLANE), view_plane=PLANE, max_radius=max_radius)
    want = R.lens_blur(image, rec, **params)
    got = develop.lens_blur(image, rec, **params)
    finite = np.isfinite(image).all(axis=-1)
    same = kept(got, image)
    c = R.circles(rec, FOCUS, params["aperture"], PLANE, max_radius)[0]
    print("blur %dx%d, radius %d: %d of %d pixels changed, %d finite ones kept their bits; c %.3g .. %.3g" % (width, height, max_radius, int((~same).sum()), width * height,
                                                                                                             int((same & finite).sum()), float(c.min()), float(c.max())))
    assert_same_image(got, want, "%dx%d radius %d" % (width, height, max_radius))
    assert np.isfinite(got[finite]).all() and same[~finite].all()
    assert width * height < 50 or ((~same).any() and (same & finite).any())  # sharp and blurred pixels meet
    assert_same_image(blur_on_device(image, rec, **params), got, "the device entry against the host entry")
    assert_same_image(develop.lens_blur(image, rec, **params), got, "two calls")
    image, rec = random_frame(width, height, seed=7 * width + max_radius, strip=False)  # anything goes: near pixels at the clamp, in front of everything
    other = dict(focus_distance=2.0, aperture=aperture_for(23.0, width, height, 2.0, 0.9), view_plane=0.9, max_radius=max_radius, depth_tolerance=0.0201)
    got = develop.lens_blur(image, rec, **other)
    assert_same_image(got, R.lens_blur(image, rec, **other), "other parameters")
    assert width * height < 50 or not kept(got, image).all()


def test_the_workgroup_bound(gpu_lib):
    """70 x 67, five tiles by five: the left half lies exactly at the focus distance, the right half so near that its circle is the
    clamp, 8. The tiles of columns 0..15 are out of every blur's reach and copy; the tile columns in between run to a reach below
    max_radius; the output is the restatement's, which knows of no reach."""
    width, height = 70, 67
    image, rec = random_frame(width, height, seed=28, strip=False)
    rec["coverage"] = 1
    rec["depth"][:, :35], rec["depth"][:, 35:] = f32(3), f32(0.5)
    params = dict(focus_distance=3.0, aperture=aperture_for(6.0, width, height, 3.0, FAR_PLANE), view_plane=FAR_PLANE, max_radius=8)
    c = R.circles(rec, 3.0, params["aperture"], FAR_PLANE, 8)[0]
    assert not c[:, :35].any() and (c[:, 35:] == 8).all()
    got = develop.lens_blur(image, rec, **params)
    assert_same_image(got, R.lens_blur(image, rec, **params), "a half in focus")
    assert_same_image(got[:, :26], image[:, :26], "the tiles out of reach, and the pixels")  # the near half spreads 9 pixels: columns 26..34 see it
    finite = np.isfinite(image).all(axis=-1)
    assert not kept(got, image)[:, 27:][finite[:, 27:]].all() and (~kept(got, image)[:, 40:] | ~finite[:, 40:]).mean() > 0.9
    assert_same_image(blur_on_device(image, rec, **params), got, "the device entry")
    params["max_radius"] = 16  # the clamp moves out: every tile of the right half now reaches 16, and columns 18..34 see it
    got = develop.lens_blur(image, rec, **params)
    assert_same_image(got, R.lens_blur(image, rec, **params), "a half in focus, radius 16")
    assert_same_image(got[:, :16], image[:, :16], "the first tile column")


# ------------------------------------------------------------------------------------------------------------------------ B. real records
def turned(cam, angle, axis=(0, 1, 0), shift=(0.0, 0.0, 0.0)):
    """`cam` turned about an axis of its own by `angle` and moved by `shift` in its own frame."""
    m = np.array(cam.c.cam_to_world[:], dtype=np.float64).reshape(4, 4).T @ pose_cases.rotation4(axis, angle, translation=shift).astype(np.float64)
    c = abi.PyrCamera.from_buffer_copy(cam.c)
    c.cam_to_world = (C.c_float * 16)(*[float(v) for v in m.astype(f32).T.reshape(-1)])
    return Camera(c)


def with_lens(cam, focus_distance, aperture):
    c = abi.PyrCamera.from_buffer_copy(cam.c)
    c.focus_distance, c.aperture = focus_distance, aperture
    return Camera(c)


def linear_render(r, size, cam, world, samples, seed):
    r.pixel_samples, r.seed = samples, seed
    film = r.new_film(*size)
    r.render(film, cam, world)
    return develop.develop_linear(film)


def cornell_lens(r, size, cam, world, on_back_wall):
    """(focus_distance, aperture, records): the focus on the tall box of the Cornell box (triangles 0..11) -- the median axial depth of
    its pixels -- and the aperture that gives the farthest surface in view, the back wall, a circle of `on_back_wall` pixels."""
    rec = r.features(size, cam, world).records
    box = (rec["shape"] >> 30 == 1) & ((rec["shape"] & 0x3FFFFFFF) < 12)
    assert box.sum() > 50
    z = R.circles(rec, 1.0, 0.0, cam.c.view_plane, 1)[2]
    focus = float(np.median(z[box]))
    hit = rec["coverage"] > 0
    far = float(z[hit].max())
    assert far > 1.2 * focus
    A = on_back_wall / abs(1 - focus / far)
    return focus, aperture_for(A, size[0], size[1], focus, cam.c.view_plane), rec


def test_real_records_of_the_cornell_box_and_of_a_sky(gpu_lib):
    world, cam, r, _ = scenes.build(scenes.c2_cornell(64, 64, 16), seed=5)
    size = (64, 64)
    focus, aperture, rec = cornell_lens(r, size, cam, world, 4.5)
    image = linear_render(r, size, cam, world, 16, 7)
    for params in (dict(max_radius=8), dict(max_radius=3, depth_tolerance=0.1), dict(max_radius=16, aperture=4 * aperture)):
        params = dict(dict(focus_distance=focus, aperture=aperture, view_plane=cam.c.view_plane), **params)
        got = develop.lens_blur(image, rec, **params)
        c = R.circles(rec, params["focus_distance"], params["aperture"], params["view_plane"], params["max_radius"])[0]
        print("cornell focused on the tall box at %.3f: c %.3g .. %.3g, %d of 4096 pixels changed" % (focus, float(c.min()), float(c.max()), int((~kept(got, image)).sum())))
        assert_same_image(got, R.lens_blur(image, rec, **params), "cornell %r" % (params,))
        assert not kept(got, image).all()
    assert_same_image(develop.lens_blur(image, rec, camera=with_lens(cam, focus, aperture)), develop.lens_blur(image, rec, focus_distance=focus, aperture=aperture, view_plane=cam.c.view_plane),
                      "the parameters read from a camera")
    world.close()
    world, cam, r, _ = scenes.build(scenes.lamps_example(13, 7, 16), seed=5)  # spheres and a plane under a sky, 13 x 7
    level = cam
    for pitch in (0.0, 0.15, 0.3, 0.45, 0.6, 0.75, 0.9):  # the image is flatter than the example's: look up until the sky comes into it
        cam = turned(level, pitch, axis=(1, 0, 0))
        rec = r.features((13, 7), cam, world).records
        if (rec["coverage"] == 0).any():
            break
    print("lamps 13x7: %d of 91 pixels see the sky" % int((rec["coverage"] == 0).sum()))
    assert (rec["coverage"] == 0).any() and (rec["coverage"] > 0).any()
    image = linear_render(r, (13, 7), cam, world, 16, 5)
    focus = float(np.median(rec["depth"][rec["coverage"] > 0]))
    for params in (dict(max_radius=8), dict(max_radius=2)):
        params = dict(dict(focus_distance=focus, aperture=aperture_for(4.0, 13, 7, focus, cam.c.view_plane), view_plane=cam.c.view_plane), **params)
        got = develop.lens_blur(image, rec, **params)
        assert_same_image(got, R.lens_blur(image, rec, **params), "lamps 13x7 %r" % (params,))
        assert not kept(got, image).all()
    world.close()


def test_a_session_blurs_its_own_frame_and_keeps_its_film(gpu_lib):
    world, cam, r, _ = scenes.build(scenes.c2_cornell(64, 64, 16), seed=5)  # a world of its own: a session takes the scene
    r.pixel_samples = 16
    focus, aperture, _ = cornell_lens(r, (64, 64), cam, world, 4.5)
    params = dict(focus_distance=focus, aperture=aperture, view_plane=cam.c.view_plane, max_radius=6)
    with r.session((64, 64), cam, world) as s:
        s.render(8)
        film = s.film()
        got = s.lens_blurred(**params)
        want = develop.lens_blur(s.linear(), s.features().records, **params)
        assert_same_image(got, want, "the session entry against its parts")
        assert (got.view(np.uint32) != s.linear().view(np.uint32)).any()
        assert_same_image(s.lens_blurred(grid=2, **params), develop.lens_blur(s.linear(), s.features(grid=2).records, **params), "the session entry with a grid of 2")
        assert film.grains.tobytes() == s.film().grains.tobytes(), "the session's film changed under the blur"
        assert_same_image(s.lens_blurred(**params), got, "two calls")
        s.render(8)  # a pass may follow
        s.sync()
        assert s.samples_done == 16 and film.grains.tobytes() != s.film().grains.tobytes()
    world.close()


# ------------------------------------------------------------------------------------------------------------------------ the command lines
def read_pfm(path):
    data = open(path, "rb").read()
    magic, size, scale, pixels = data.split(b"\n", 3)
    w, h = (int(x) for x in size.split())
    assert magic == b"PF" and float(scale) < 0
    return np.frombuffer(pixels, dtype="<f4").reshape(h, w, 3)[::-1].astype(f32)


def test_both_command_lines_render_a_pinhole_and_put_the_lens_back(gpu_lib, tmp_path):
    """tests/golden/projects/gallery.lua has a camera with focus_distance 8 and aperture 0.001. With --lens-blur the frame is the
    render of that camera with aperture 0, blurred over the full-size records by the camera's own lens; without the flag nothing
    changes. The film is summed with float atomics whose order is not fixed, so two renders of one seed agree to rounding only (nine
    floats of 4,608 differed by one ulp when this was written): images of two renders are held together to 1e-4 relative -- three
    orders above that, and far below what a missing stage or another lens would move -- and their 8-bit forms to one level."""
    import subprocess

    from pyrite_amd import build as gpu_build
    from pyrite_amd import lua_project
    from pyrite_amd.__main__ import main
    from test_gpu_session import read_png

    def assert_close(got, want, what):
        assert np.allclose(got, want, rtol=1e-4, atol=1e-6), "%s: largest difference %g" % (what, float(np.abs(got.astype(np.float64) - want).max()))

    def assert_same_png(a, b, what):
        assert np.abs(read_png(a).astype(np.int32) - read_png(b).astype(np.int32)).max() <= 1, what

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    project_file = os.path.join(root, "tests", "golden", "projects", "gallery.lua")
    common = [project_file, "--seed", "7", "--spp", "4", "--size", "48x32"]
    plain, blurred, pfm, cpp_pfm = (str(tmp_path / name) for name in ("plain.png", "blurred.png", "blurred.pfm", "cpp.pfm"))
    assert main(common + ["-o", plain]) == 0
    assert main(common + ["-o", blurred, "--lens-blur", "--hdr", pfm]) == 0

    project, base_dir = lua_project.load_project(project_file)
    project.setdefault("image", {}).update(width=48, height=32)
    project["renderer"] = project["renderer"].with_(pixel_samples=4)
    world, cam, r, film = scenes.build(project, seed=7, base_dir=base_dir)
    assert cam.c.aperture > 0
    r.render(film, cam, world)
    image = project.get("image") or {}
    expected = str(tmp_path / "expected.png")
    develop.save_png(expected, develop.develop(film, filter=image.get("filter"), white=image.get("white")))
    assert_same_png(plain, expected, "without --lens-blur the PNG changed")
    pinhole = with_lens(cam, cam.c.focus_distance, 0.0)
    film = r.new_film(48, 32)
    r.render(film, pinhole, world)
    linear = develop.develop_linear(film, "srgb", filter=image.get("filter"), white=image.get("white"))
    rec = r.features((48, 32), pinhole, world).records
    want = develop.lens_blur(linear, rec, camera=cam)
    assert_close(read_pfm(pfm), want, "the --hdr file against develop.lens_blur of the pinhole render")
    c = R.circles(rec, cam.c.focus_distance, cam.c.aperture, cam.c.view_plane, 8)[0]
    sharpest = c <= np.percentile(c, 10)  # what is nearest the focus moves least: where c is small the weights of the neighbours are c / area
    moved = np.abs(want.astype(np.float64) - linear).max(axis=-1)
    print("gallery 48x32 through its lens: c %.3g .. %.3g; the filter moves the sharpest tenth by at most %.3g, the image by at most %.3g" % (
        float(c.min()), float(c.max()), float(moved[sharpest].max()), float(moved.max())))
    assert (want.view(np.uint32) != linear.view(np.uint32)).any()
    develop.save_png(expected, develop.tonemap(want))
    assert_same_png(blurred, expected, "the PNG of --lens-blur against the tone curve of that image")
    assert (read_png(blurred) != read_png(plain)).any()
    assert main(common + ["-o", blurred, "--lens-blur", "--lens-blur-radius", "2", "--hdr", pfm]) == 0
    assert_close(read_pfm(pfm), develop.lens_blur(linear, rec, camera=cam, max_radius=2), "--lens-blur-radius")
    assert main(common + ["-o", blurred, "--lens-blur-radius", "2"]) == 2 and main(common + ["-o", blurred, "--lens-blur", "--lens-blur-radius", "17"]) == 2
    world.close()
    subprocess.run([gpu_build.HOST_TOOL, "render-project", project_file, "-", "7", str(tmp_path / "cpp.png"), "--spp", "4", "--size", "48x32", "--lens-blur", "--lens-blur-radius", "2",
                    "--hdr", cpp_pfm], check=True, cwd=root, timeout=600, capture_output=True)
    assert_close(read_pfm(cpp_pfm), read_pfm(pfm), "pyrite_host_tool --lens-blur against python -m pyrite_amd --lens-blur")
    assert_same_png(str(tmp_path / "cpp.png"), blurred, "the two tools' PNGs")


# ------------------------------------------------------------------------------------------------------------------------ C. against what lens blur is
def test_the_filtered_pinhole_frame_is_nearer_the_lens_render_than_the_pinhole_frame(gpu_lib):
    """The Cornell box at 64 x 64, focus on the tall box, the aperture that gives the back wall a circle of 4.5 pixels. Truth: the
    mean of four renders through that lens of 4,096 samples a pixel each, 16,384 in all, a quarter of the frame's noise deviation.
    Frame: the render with aperture 0 at 1,024 samples a pixel. Over the pixels with c >= 1 the filtered frame's RMSE against the
    truth must be the smaller. An inequality, not a tolerance. Measured on an MI355X: 0.66816 for the pinhole frame, 0.44677 for the
    filtered frame, over the 3,353 pixels with c >= 1; focus 10.725, aperture 5.956, c up to 6.83 pixels (profiles/r28_lens_blur.txt)."""
    size = (64, 64)
    world, cam, r, _ = scenes.build(scenes.c2_cornell(64, 64, 16), seed=5)
    focus, aperture, rec = cornell_lens(r, size, cam, world, 4.5)
    lens = with_lens(cam, focus, aperture)
    truth = np.zeros((64, 64, 3), dtype=np.float64)
    for k in range(4):
        truth += linear_render(r, size, lens, world, 4096, 200 + k)
    truth /= 4
    frame = linear_render(r, size, with_lens(cam, focus, 0.0), world, 1024, 99)
    world.close()
    params = dict(camera=lens, max_radius=8)
    filtered = develop.lens_blur(frame, rec, **params)
    assert_same_image(filtered, R.lens_blur(frame, rec, focus, aperture, cam.c.view_plane, max_radius=8), "the frame of the lens case")
    c = R.circles(rec, focus, aperture, cam.c.view_plane, 8)[0]
    blurred = c >= 1
    rmse = lambda a: float(np.sqrt(((a.astype(np.float64) - truth)[blurred] ** 2).mean()))  # noqa: E731
    plain, ours = rmse(frame), rmse(filtered)
    on_wall = float(c[rec["coverage"] > 0][np.argmax(rec["depth"][rec["coverage"] > 0])])
    print("cornell through a lens focused at %.3f, aperture %.4g: c up to %.2f pixels (%.2f on the back wall), %d of 4096 pixels with c >= 1; RMSE against 16,384 samples "
          "through the lens: pinhole frame %.5f, filtered frame %.5f" % (focus, aperture, float(c.max()), on_wall, int(blurred.sum()), plain, ours))
    assert 3 <= on_wall <= 6 and blurred.any() and not blurred.all()
    assert ours < plain
