"""The glare of a linear image on the GPU (include/pyrite_gpu.h "glare") -- run with `-m gpu` on an MI355X.

The kernels are held against the numpy restatement (tests/glare_restatement.py) bit for bit: the header spells every f32 operation
and its order out, contraction is off on both sides, and the compiler's division rounds as numpy's does. Both kernel forms -- one
launch a step, and the small levels in one workgroup (PYRITE_GLARE_TAIL, read at every call) -- must write the restatement's bits.
Then the session entry and the command line are held against the plain entry."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glare_restatement as R  # noqa: E402

from pyrite_amd import develop, scenes  # noqa: E402
from pyrite_amd._lib import check, lib  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("plain", "tail")


def assert_same_image(got, want, what):
    differs = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(differs) == 0, "%s: out differs in %d of %d floats, first %s: GPU %r, expected %r" % (
        what, len(differs), got.size, tuple(differs[0]), got[tuple(differs[0])], want[tuple(differs[0])])


@pytest.fixture(params=FORMS)
def form(request, monkeypatch):
    monkeypatch.setenv("PYRITE_GLARE_TAIL", "1" if request.param == "tail" else "0")
    return request.param


def glare_on_device(image, out_bits=None, **params):
    """`out_bits`: the 32 bits every float of `out` holds before the call (default: those of -1.0f)."""
    import torch

    h, w, _ = image.shape
    image_dev = torch.from_numpy(np.ascontiguousarray(image).view(np.uint8).reshape(-1).copy()).cuda()
    out = torch.full((h * w * 3,), -1.0, dtype=torch.float32, device="cuda")
    if out_bits is not None:
        out = torch.full((h * w * 3,), out_bits, dtype=torch.int32, device="cuda").view(torch.float32)
    p = develop.glare_params(**params)
    stream = torch.cuda.current_stream()
    check(lib().pyr_image_glare_device(C.c_void_p(image_dev.data_ptr()), w, h, C.byref(p), C.c_void_p(out.data_ptr()), 0, C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    return out.cpu().numpy().reshape(h, w, 3)


def random_image(width, height, seed):
    """Log-uniform over 1e-3 .. 1e3, with a few pixels NaN, inf, -inf, 1e30 and negative."""
    rng = np.random.default_rng(seed)
    n = width * height
    image = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (height, width, 3))).astype(f32)
    if n >= 10:
        for value in (np.nan, np.inf, -np.inf, 1e30, -2.5):
            image.reshape(-1)[rng.integers(0, 3 * n, max(1, n // 60))] = value
    return image


# The tail kernel (kernels/glare.hip, kTailSlots) takes the first level m >= 1 whose lower levels m+1 .. L hold at most 4,096 pixels
# together. With 12 levels 256 x 188 has 4,033 pixels below level 1 and the tail starts there; 256 x 192 has 4,097, one too many, and
# goes through one more plain down and up. With one level there is nothing below level 1 and the tail does not run at all.
SIZES = [(1, 1), (1, 5), (2, 2), (13, 7), (17, 33), (64, 36), (130, 67), (256, 188), (256, 192)]
CASES = [dict(levels=levels, threshold=threshold, falloff=falloff, strength=strength)
         for levels in (1, 2, 3, 12) for threshold in (0.0, 1.0) for falloff in (1.0, 2.0) for strength in (0.1, 1.0)]
WANTED = {}  # (size, case index) -> the restatement's image: computed once, shared by the two forms, never written to


def wanted(size, index, image):
    if (size, index) not in WANTED:
        WANTED[size, index] = R.glare(image, **CASES[index])
        WANTED[size, index].flags.writeable = False
    return WANTED[size, index]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_glare_is_the_restatement_bit_for_bit(size, form, gpu_lib):
    width, height = size
    image = random_image(width, height, seed=100 * width + height)
    kept = np.isfinite(image).all(axis=-1)
    for index, params in enumerate(CASES):
        got = develop.glare(image, **params)
        assert_same_image(got, wanted(size, index, image), "%dx%d %s %r" % (width, height, form, params))
        assert_same_image(got[~kept], image[~kept], "pixels that are not kept")
        assert np.isfinite(got[kept]).all()
        assert width * height == 1 or params["threshold"] > 0 or (got.view(np.uint32) != image.view(np.uint32)).any()
    assert_same_image(glare_on_device(image, **params), got, "the device entry against the host entry")
    assert_same_image(develop.glare(image, **params), got, "two calls")


def test_both_forms_over_many_tiles(form, gpu_lib):
    """256 x 144: 144 tiles in the compose, several workgroups in the downs and ups of levels 1 and 2, the tail below them."""
    image = random_image(256, 144, seed=9)
    for params in (dict(), dict(levels=11, threshold=0.5, falloff=0.5)):
        assert_same_image(develop.glare(image, **params), R.glare(image, **params), "256x144 %s %r" % (form, params))


# ------------------------------------------------------------------------------------------------------------------------ the session
def test_a_session_glares_its_own_frame_and_keeps_its_film(gpu_lib):
    world, cam, r, _ = scenes.build(scenes.c2_cornell(64, 64, 16), seed=5)
    r.pixel_samples = 24  # the session's budget: 16 for the frame, 8 for the pass that follows
    with r.session((64, 64), cam, world) as s:
        s.render(16)
        film = s.film()
        linear = s.linear()
        got = s.glared()
        assert_same_image(got, develop.glare(linear), "the session entry against its parts")
        assert_same_image(got, R.glare(linear), "the session entry against the restatement")
        assert film.grains.tobytes() == s.film().grains.tobytes(), "the session's film changed under the glare"
        assert_same_image(s.glared(), got, "two calls")
        other = dict(strength=0.5, levels=3, threshold=0.8, falloff=2.0)
        assert_same_image(s.glared(**other), develop.glare(linear, **other), "other parameters")
        features = s.features()
        lamp_materials = [i for i, m in enumerate(world.desc.materials[:world.desc.num_materials]) if m.num_emissive > 0]
        lamp = (features.coverage > 0) & np.isin(features.material, lamp_materials)
        kept = np.isfinite(linear).all(axis=-1)
        near = np.zeros_like(lamp)
        ys, xs = np.nonzero(lamp)
        for dy in range(-4, 5):
            for dx in range(-4, 5):
                near[np.clip(ys + dy, 0, 63), np.clip(xs + dx, 0, 63)] = True
        ring = near & ~lamp & kept
        lamp &= kept
        mean = lambda a, where: float(a[where].astype(np.float64).mean())  # noqa: E731
        print("cornell 64 x 64, 16 samples: %d lamp pixels, mean %.4f -> %.4f; %d ring pixels within 4, mean %.4f -> %.4f"
              % (int(lamp.sum()), mean(linear, lamp), mean(got, lamp), int(ring.sum()), mean(linear, ring), mean(got, ring)))
        assert lamp.sum() > 20 and ring.sum() > 20
        assert mean(got, lamp) < mean(linear, lamp)
        assert mean(got, ring) > mean(linear, ring)
        s.render(8)  # a pass may follow
        s.sync()
        assert s.samples_done == 24 and film.grains.tobytes() != s.film().grains.tobytes()
    world.close()


# ------------------------------------------------------------------------------------------------------------------------ the command line
def read_pfm(path):
    data = open(path, "rb").read()
    magic, size, scale, pixels = data.split(b"\n", 3)
    w, h = (int(x) for x in size.split())
    assert magic == b"PF" and float(scale) < 0
    return np.frombuffer(pixels, dtype="<f4").reshape(h, w, 3)[::-1].astype(f32)


def test_the_command_line_glares_the_final_image(gpu_lib, tmp_path):
    """tests/golden/projects/materials.lua is the module of materials that gallery.lua requires, not a project of its own: it is
    rendered through gallery.lua."""
    from pyrite_amd import lua_project
    from pyrite_amd.__main__ import main

    project_file = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    common = [project_file, "--seed", "7", "--spp", "4", "--size", "32x32"]
    plain, glared, pfm = str(tmp_path / "plain.png"), str(tmp_path / "glared.png"), str(tmp_path / "glared.pfm")
    assert main(common + ["-o", plain]) == 0
    assert main(common + ["-o", glared, "--glare", "--hdr", pfm]) == 0

    project, base_dir = lua_project.load_project(project_file)
    project.setdefault("image", {}).update(width=32, height=32)
    project["renderer"] = project["renderer"].with_(pixel_samples=4)
    world, cam, r, film = scenes.build(project, seed=7, base_dir=base_dir)
    r.render(film, cam, world)
    image = project.get("image") or {}
    expected = str(tmp_path / "expected.png")
    develop.save_png(expected, develop.develop(film, filter=image.get("filter"), white=image.get("white")))
    assert open(plain, "rb").read() == open(expected, "rb").read(), "without --glare the PNG changed"
    linear = develop.develop_linear(film, "srgb", filter=image.get("filter"), white=image.get("white"))
    want = develop.glare(linear)
    assert_same_image(read_pfm(pfm), want, "the --hdr file against develop.glare of the linear image")
    develop.save_png(expected, develop.tonemap(want))
    assert open(glared, "rb").read() == open(expected, "rb").read()
    assert open(glared, "rb").read() != open(plain, "rb").read()
    assert main(common + ["-o", glared, "--glare", "0.5", "--glare-levels", "3", "--glare-threshold", "0.25", "--exposure", "auto", "--hdr", pfm]) == 0
    assert_same_image(read_pfm(pfm), develop.glare(linear, strength=0.5, levels=3, threshold=0.25), "the three flags")
    world.close()
