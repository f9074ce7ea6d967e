"""The guided upsampling on the GPU (include/pyrite_gpu.h "upsample") -- run with `-m gpu` on an MI355X.

The kernel is held against the numpy restatement (tests/upsample_restatement.py) bit for bit: the header spells every f32 operation
and its order out, contraction is off on both sides, and the compiler's division rounds as numpy's does. Where the rule makes a float
a NaN both sides must have a NaN there; its sign and payload are the one thing the header leaves open. Then the session entry and the
command line are held against the plain entry, and the whole is held against what it is for: a low render upsampled under its guides
is nearer a full-size reference than the same render upsampled without them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upsample_restatement as R  # noqa: E402

from pyrite_amd import develop, scenes  # noqa: E402
from pyrite_amd._lib import check, lib  # noqa: E402
from pyrite_amd.features import RECORD  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_same_image(got, want, what):
    """The same bits, but for a NaN, where a NaN of any sign and payload is wanted."""
    differs = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))
    assert len(differs) == 0, "%s: out differs in %d of %d floats, first %s: GPU %r, expected %r" % (
        what, len(differs), got.size, tuple(differs[0]), got[tuple(differs[0])], want[tuple(differs[0])])


def upsample_on_device(low, scale, albedo=None, pixels=None, low_albedo=None, low_pixels=None, out_bits=None, **params):
    """`out_bits`: the 32 bits every float of `out` holds before the call (default: those of -1.0f)."""
    import torch

    h, w, _ = low.shape
    keep = [None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda() for a in (low, low_albedo, low_pixels, albedo, pixels)]
    at = [None if t is None else C.c_void_p(t.data_ptr()) for t in keep]
    out = torch.full((h * scale * w * scale * 3,), -1.0, dtype=torch.float32, device="cuda")
    if out_bits is not None:
        out = torch.full((h * scale * w * scale * 3,), out_bits, dtype=torch.int32, device="cuda").view(torch.float32)
    p = develop.upsample_params(**params)
    stream = torch.cuda.current_stream()
    check(lib().pyr_image_upsample_device(at[0], at[1], at[2], w, h, scale, at[3], at[4], C.byref(p), C.c_void_p(out.data_ptr()), 0, C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    return out.cpu().numpy().reshape(h * scale, w * scale, 3)


# ------------------------------------------------------------------------------------------------------------------------ the inputs
NORMALS = np.array([(0, 0, 1), (1, 0, 0), (0, 0.6, 0.8), (0.05, 0, 0.99875)], dtype=f32)  # the last within sigma_normal of the first
DEPTHS = np.array([2.0, 2.02, 5.0, 2.0], dtype=f32)                                       # the second within sigma_depth of the first
MATERIALS = np.array([3, 7, 7, 12], dtype=np.uint32)


def random_inputs(width, height, scale, seed):
    """low: log-uniform over 1e-3 .. 1e3 with a few pixels NaN, inf, -inf, 1e30 and negative, as the glare's random_image. Albedos
    in [0, 1] with exact zeros (a sixth of the low ones, a tenth of the full-size ones). Records: four surfaces -- distinct normals,
    depths and material ids, two pairs of them near each other in one guide -- laid out in blocks of 3 x 2 low pixels; the full-size
    records repeat the low ones, a pixel in nine is moved to a neighbouring block's surface (accepted and rejected taps) and one in
    eight is a surface no low pixel has (the fallback); a few depths and normals are NaN."""
    rng = np.random.default_rng(seed)
    n = width * height
    low = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (height, width, 3))).astype(f32)
    if n >= 10:
        for value in (np.nan, np.inf, -np.inf, 1e30, -2.5):
            low.reshape(-1)[rng.integers(0, 3 * n, max(1, n // 60))] = value
    H, W = height * scale, width * scale
    low_albedo = rng.uniform(0, 1, (height, width, 3)).astype(f32)
    low_albedo[rng.random((height, width)) < 1 / 6] = 0
    albedo = rng.uniform(0, 1, (H, W, 3)).astype(f32)
    albedo[rng.random((H, W)) < 0.1] = 0
    ys, xs = np.mgrid[0:height, 0:width]
    surface = ((xs // 3) + 2 * (ys // 2) + rng.integers(0, 4)) % 4
    high_surface = np.repeat(np.repeat(surface, scale, axis=0), scale, axis=1)
    moved = rng.random((H, W)) < 1 / 9
    high_surface = np.where(moved, (high_surface + 1) % 4, high_surface)

    def records_of(surface):
        out = np.zeros(surface.shape, dtype=RECORD)
        out["normal"], out["depth"], out["material"] = NORMALS[surface], DEPTHS[surface], MATERIALS[surface]
        out["coverage"], out["shape"] = 1.0, surface
        return out

    low_pixels, pixels = records_of(surface), records_of(high_surface)
    alone = rng.random((H, W)) < 1 / 8
    pixels["normal"][alone], pixels["depth"][alone], pixels["material"][alone] = (0, -1, 0), 50.0, 99
    if n >= 10:
        at = rng.integers(0, n, max(1, n // 40))
        low_pixels["depth"][at // width, at % width] = np.nan
        at = rng.integers(0, 3 * H * W, max(1, H * W // 80))
        pixels["normal"][at // (3 * W), at // 3 % W, at % 3] = np.nan
    return dict(low=low, albedo=albedo, pixels=pixels, low_albedo=low_albedo, low_pixels=low_pixels)


LOW_SIZES = [(1, 1), (1, 3), (2, 2), (5, 3), (9, 17), (17, 9), (33, 20)]
SCALES, RADII = (2, 3, 4, 8), (1, 2, 3)
# the four combinations of the pairs, PYR_UPSAMPLE_MATCH_MATERIAL on and off where records are read
COMBINATIONS = [((), True), (("albedo",), True), (("records",), True), (("records",), False), (("albedo", "records"), True), (("albedo", "records"), False)]


def arguments(inputs, pairs):
    chosen = {}
    if "albedo" in pairs:
        chosen.update(albedo=inputs["albedo"], low_albedo=inputs["low_albedo"])
    if "records" in pairs:
        chosen.update(pixels=inputs["pixels"], low_pixels=inputs["low_pixels"])
    return chosen


def seed_of(width, height, scale):
    return 1000 * width + 10 * height + scale


@pytest.mark.parametrize("size", LOW_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_upsample_is_the_restatement_bit_for_bit(size, gpu_lib):
    width, height = size
    for scale in SCALES:
        inputs = random_inputs(width, height, scale, seed_of(width, height, scale))
        for radius in RADII:
            for pairs, match in COMBINATIONS:
                given = arguments(inputs, pairs)
                want = R.upsample(inputs["low"], scale, radius=radius, flags=R.MATCH_MATERIAL if match else 0, **given)
                got = develop.upsample(inputs["low"], scale, radius=radius, match_material=match, **given)
                assert_same_image(got, want, "%dx%d scale %d radius %d %r match %r" % (width, height, scale, radius, pairs, match))
            # the last combination: the device entry, and a second call
            assert_same_image(upsample_on_device(inputs["low"], scale, radius=radius, match_material=match, **given), want, "the device entry, scale %d radius %d" % (scale, radius))
            again = develop.upsample(inputs["low"], scale, radius=radius, match_material=match, **given)
            assert got.tobytes() == again.tobytes(), "two calls, scale %d radius %d" % (scale, radius)


@pytest.mark.parametrize("scale", SCALES)
def test_the_inputs_take_every_path(scale):
    """A condition on the inputs, from the restatement alone: in the 33 x 20 case the guided sum, the fallback and the clamped gain
    each own at least 5 % of the pixels, at every scale and radius, with the material rule and without it."""
    inputs = random_inputs(33, 20, scale, seed_of(33, 20, scale))
    for radius in RADII:
        for match in (True, False):
            _, guided, clamped = R.upsample(inputs["low"], scale, radius=radius, flags=R.MATCH_MATERIAL if match else 0, paths=True, **arguments(inputs, ("albedo", "records")))
            shares = guided.mean(), (~guided).mean(), clamped.mean()
            print("33x20 scale %d radius %d match %r: guided %.3f, fallback %.3f, a gain clamped %.3f" % ((scale, radius, match) + shares))
            assert min(shares) >= 0.05, shares


def test_a_wide_image_crosses_many_tiles(gpu_lib):
    """70 x 5 low pixels at scale 8: 560 x 40, eighteen tiles a row and five rows of them, and a low image wider than one patch."""
    inputs = random_inputs(70, 5, 8, seed=11)
    for radius in (1, 3):
        given = arguments(inputs, ("albedo", "records"))
        assert_same_image(develop.upsample(inputs["low"], 8, radius=radius, **given), R.upsample(inputs["low"], 8, radius=radius, **given), "70x5 scale 8 radius %d" % radius)


def test_albedos_below_0_and_nan_albedos_count_as_0(gpu_lib):
    """Beside the inputs above, whose albedos lie in [0, 1]: a developed albedo can be negative, and the rule takes it, and a NaN, as 0."""
    inputs = random_inputs(17, 9, 3, seed=21)
    rng = np.random.default_rng(22)
    for value in (-0.01, -0.010000001, -0.5, np.nan, -np.inf, -0.0):
        inputs["low_albedo"].reshape(-1)[rng.integers(0, inputs["low_albedo"].size, 12)] = value
        inputs["albedo"].reshape(-1)[rng.integers(0, inputs["albedo"].size, 100)] = value
    for pairs in (("albedo",), ("albedo", "records")):
        given = arguments(inputs, pairs)
        assert_same_image(develop.upsample(inputs["low"], 3, radius=2, **given), R.upsample(inputs["low"], 3, radius=2, **given), "albedos below 0, %r" % (pairs,))


# ------------------------------------------------------------------------------------------------------------------------ the session
def guides_of(r, cam, world, size, scale, **develop_args):
    """The two feature passes and their developed albedos, as develop.upsample takes them."""
    low_f, high_f = r.features(size, cam, world), r.features((size[0] * scale, size[1] * scale), cam, world)
    return dict(albedo=develop.develop_linear(high_f.albedo, "srgb", **develop_args), pixels=high_f.records,
                low_albedo=develop.develop_linear(low_f.albedo, "srgb", **develop_args), low_pixels=low_f.records)


def test_a_session_upsamples_its_own_frame_and_keeps_its_films(gpu_lib):
    world, cam, r, _ = scenes.build(scenes.c2_cornell(32, 24, 16), seed=5)
    r.pixel_samples = 24  # the session's budget: 16 for the frame, 8 for the pass that follows
    with r.session((32, 24), cam, world, halves=True) as s:
        s.render(8)
        s.render(8)
        film, halves = s.film(), s.half_films()
        guides = guides_of(r, cam, world, (32, 24), 2)
        assert s.features().records.tobytes() == guides["low_pixels"].tobytes(), "the session's feature pass against the renderer's"
        linear = s.linear()
        got = s.upsampled(2)
        assert got.shape == (48, 64, 3)
        assert_same_image(got, develop.upsample(linear, 2, **guides), "the session entry against its parts")
        assert_same_image(s.upsampled(2), got, "two calls")
        assert_same_image(s.upsampled(2, guides=False, radius=2), develop.upsample(linear, 2, radius=2), "without guides")
        denoised = s.denoised()[0]
        assert_same_image(s.upsampled(2, denoise={}), develop.upsample(denoised, 2, **guides), "with the denoiser: the session entry against its parts")
        small = dict(radius=3)
        assert_same_image(s.upsampled(2, denoise=small, radius=2, match_material=False), develop.upsample(s.denoised(**small)[0], 2, radius=2, match_material=False, **guides),
                          "other parameters")
        guides3 = guides_of(r, cam, world, (32, 24), 3)
        assert_same_image(s.upsampled(3), develop.upsample(linear, 3, **guides3), "scale 3")
        assert film.grains.tobytes() == s.film().grains.tobytes(), "the session's film changed under the upsample"
        assert all(a.tobytes() == b.tobytes() for a, b in zip(halves, s.half_films())), "a half film changed under the upsample"
        s.render(8)  # a pass may follow
        s.sync()
        assert s.samples_done == 24 and film.grains.tobytes() != s.film().grains.tobytes()
    with r.session((32, 24), cam, world) as s:  # no halves: the denoiser's refusal, and the plain route still serves
        s.render(8)
        with pytest.raises(Exception) as refused:
            s.upsampled(2, denoise={})
        assert "PYR_SESSION_HALVES" in str(refused.value)
        assert_same_image(s.upsampled(2), develop.upsample(s.linear(), 2, **guides), "a session without halves")
    world.close()


# ------------------------------------------------------------------------------------------------------------------------ the command line
def read_pfm(path):
    data = open(path, "rb").read()
    magic, size, scale, pixels = data.split(b"\n", 3)
    w, h = (int(x) for x in size.split())
    assert magic == b"PF" and float(scale) < 0
    return np.frombuffer(pixels, dtype="<f4").reshape(h, w, 3)[::-1].astype(f32)


def read_png_size(path):
    data = open(path, "rb").read(24)
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
    return int.from_bytes(data[16:20], "big"), int.from_bytes(data[20:24], "big")


def test_the_command_line_upsamples_the_final_image(gpu_lib, tmp_path):
    from pyrite_amd import lua_project
    from pyrite_amd.__main__ import main

    project_file = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    project, base_dir = lua_project.load_project(project_file)
    full = int(project["image"]["width"]), int(project["image"]["height"])
    png = str(tmp_path / "project_size.png")
    if full[0] % 2 == 0 and full[1] % 2 == 0:  # the project's own size, rendered at half of it
        assert main([project_file, "--seed", "7", "--spp", "1", "--upsample", "2", "-o", png]) == 0
        assert read_png_size(png) == full
    common = [project_file, "--seed", "7", "--spp", "4", "--size", "32x32"]
    pfm = str(tmp_path / "upsampled.pfm")
    assert main(common + ["-o", png, "--upsample", "2", "--upsample-radius", "2", "--hdr", pfm]) == 0
    assert read_png_size(png) == (32, 32)

    project.setdefault("image", {}).update(width=16, height=16)
    project["renderer"] = project["renderer"].with_(pixel_samples=4)
    world, cam, r, film = scenes.build(project, seed=7, base_dir=base_dir)
    r.render(film, cam, world)
    image = project.get("image") or {}
    develop_args = dict(filter=image.get("filter"), white=image.get("white"))
    linear = develop.develop_linear(film, "srgb", **develop_args)
    want = develop.upsample(linear, 2, radius=2, **guides_of(r, cam, world, (16, 16), 2, **develop_args))
    assert_same_image(read_pfm(pfm), want, "the --hdr file against develop.upsample of the parts")
    expected = str(tmp_path / "expected.png")
    develop.save_png(expected, develop.tonemap(want))
    assert open(png, "rb").read() == open(expected, "rb").read()
    world.close()


# ------------------------------------------------------------------------------------------------------------------------ what it is for
def mse(a, b):
    finite = np.isfinite(a).all(axis=-1) & np.isfinite(b).all(axis=-1)
    return float(((a[finite].astype(np.float64) - b[finite].astype(np.float64)) ** 2).mean())


def low_and_reference(project_of, seed):
    """A 32 x 32 render at 256 samples, its guides for twice the size, and the 64 x 64 reference at 1024 samples under the same camera."""
    world, cam, r, film = scenes.build(project_of(32, 32, 256), seed=seed)
    r.render(film, cam, world)
    low = develop.develop_linear(film, "srgb")
    guides = guides_of(r, cam, world, (32, 32), 2)
    world.close()
    world, cam, r, film = scenes.build(project_of(64, 64, 1024), seed=seed + 1)
    r.render(film, cam, world)
    reference = develop.develop_linear(film, "srgb")
    world.close()
    return low, guides, reference


def test_the_guides_bring_the_cornell_box_nearer_its_reference(gpu_lib):
    low, guides, reference = low_and_reference(scenes.c2_cornell, seed=3)
    guided, plain = mse(develop.upsample(low, 2, **guides), reference), mse(develop.upsample(low, 2), reference)
    print("cornell 32 x 32 at 256 spp, twice: mse against 64 x 64 at 1024 spp guided %.6g, unguided %.6g, ratio %.3f" % (guided, plain, guided / plain))
    assert guided < plain


def test_the_guides_and_the_albedo_bring_the_textures_nearer_their_reference(gpu_lib):
    low, guides, reference = low_and_reference(scenes.textures_example, seed=4)
    guided, plain = mse(develop.upsample(low, 2, **guides), reference), mse(develop.upsample(low, 2), reference)
    records_only = mse(develop.upsample(low, 2, pixels=guides["pixels"], low_pixels=guides["low_pixels"]), reference)
    print("textures 32 x 32 at 256 spp, twice: mse against 64 x 64 at 1024 spp guided %.6g, records alone %.6g, unguided %.6g; ratios %.3f and %.3f"
          % (guided, records_only, plain, guided / plain, guided / records_only))
    assert guided < plain
    assert guided < records_only
