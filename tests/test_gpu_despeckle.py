"""The firefly clamp on the GPU (include/pyrite_gpu.h "despeckle") -- run with `-m gpu` on an MI355X.

The kernel is held against the numpy restatement (tests/despeckle_restatement.py) bit for bit, as uint32, with no tolerance and no
exception for a NaN: only luminance products and sums, fabsf, fmaxf, one IEEE division and three multiplies touch a value, medians
are selections, contraction is off on both sides, and the rule makes no NaN of its own -- a pixel that is not finite keeps its bits
and removed_out is 0.0f there. Then the host and the device entries are held against each other, the session entry against the
pipeline composed by hand, and the two command lines against each other with the flag and without it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import despeckle_restatement as R
from pyrite_amd import develop, scenes
from pyrite_amd import build as gpu_build
from pyrite_amd._lib import PyriteGpuError, check, lib
from pyrite_amd.film import Film
from test_gpu_session import read_png

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(37, 29), (33, 17), (16, 16), (5, 3), (2, 1), (1, 1)]  # two that straddle the 16 x 16 tiles, one tile, smaller than a window, n < 5, one pixel
RADII = (1, 2)


def bits(image):
    return np.ascontiguousarray(image, dtype=f32).view(np.uint32)


def assert_same_bits(got, want, what):
    differs = np.argwhere(bits(got) != bits(want))
    assert len(differs) == 0, "%s differs in %d of %d floats, first %s: GPU %r (%08x), expected %r (%08x)" % (
        what, len(differs), got.size, tuple(differs[0]), got[tuple(differs[0])], bits(got)[tuple(differs[0])], want[tuple(differs[0])], bits(want)[tuple(differs[0])])


def halves(width, height, seed):
    """Two half images of one picture: blocks of 4 x 4 pixels log-uniform over 1e-4 .. 1e3 with a hue each, under log-normal noise
    (sigma 0.3) independent per half; fireflies in alternating halves (times 50 to 5000), corners among them; one pixel bright in
    both halves; a flat zero block with one speck in it; channels that are -0.0, denormal and negative (out of gamut); a NaN with a
    payload, an infinity and a -infinity. What does not fit a small image is left out."""
    rng = np.random.default_rng(seed)
    blocks = np.exp(rng.uniform(np.log(1e-4), np.log(1e3), ((height + 3) // 4, (width + 3) // 4, 1))) * rng.uniform(0.3, 1.0, ((height + 3) // 4, (width + 3) // 4, 3))
    clean = np.repeat(np.repeat(blocks, 4, axis=0), 4, axis=1)[:height, :width]
    a, b = ((clean * np.exp(rng.normal(0, 0.3, (height, width, 1)))).astype(f32) for _ in range(2))
    n = width * height
    if n >= 15:
        a[0, 0], b[0, 0] = clean[0, 0] * 200, clean[0, 0]  # a corner each, the other half at the picture's own value there
        b[height - 1, width - 1], a[height - 1, width - 1] = clean[-1, -1] * 200, clean[-1, -1]
        for i in range(max(2, n // 40)):
            y, x = int(rng.integers(0, height)), int(rng.integers(0, width))
            (a, b)[i % 2][y, x] *= f32(np.exp(rng.uniform(np.log(50), np.log(5000))))
        y, x = height // 2, width // 2
        a[y, x] = b[y, x] = 4000.0  # bright in both halves
        a[1, 2, 1], b[1, 1, 0] = -0.0, -0.0
        a[2, 1, 2], b[2, 2, 1] = 1e-41, 3e-39  # denormal channels
        a[2, 3] = (0.9, -0.05, 0.4)  # out of gamut
    if width >= 16 and height >= 16:
        a[8:14, 3:10] = 0
        b[8:14, 3:10] = 0
        a[10, 6] = 2e-3  # a speck over black: the floor decides
        a[11, 4, 2] = -0.0
        a[3, 12] = (np.nan, 1.0, 2.0)
        a.view(np.uint32)[3, 12, 0] = 0xFFC12345
        b[5, 13] = (1.0, np.inf, 0.5)
        a[12, 12] = (-np.inf, 1.0, 1.0)
        b[12, 12] = (np.inf, -np.inf, 1.0)
    return a, b


def despeckle_on_device(a, b, **params):
    import torch

    h, w, _ = a.shape
    keep = [None if image is None else torch.from_numpy(np.ascontiguousarray(image).view(np.uint8).reshape(-1).copy()).cuda() for image in (a, b)]
    outs = [torch.full((h * w * 3,), -1.0, dtype=torch.float32, device="cuda") if needed else None for needed in (True, b is not None, True)]
    counts = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    at = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    p = develop.despeckle_params(**params)
    stream = torch.cuda.current_stream()
    check(lib().pyr_image_despeckle_device(at(keep[0]), at(keep[1]), w, h, C.byref(p), at(outs[0]), at(outs[1]), at(outs[2]), at(counts), 0, C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    images = [None if t is None else t.cpu().numpy().reshape(h, w, 3) for t in outs]
    return images[0], images[1], images[2], tuple(int(c) for c in counts.cpu().numpy())


@pytest.fixture(scope="module")
def expected():
    """(size, radius, with b) -> the inputs and what the restatement makes of them: computed once, shared, never written to."""
    table = {}
    for width, height in SIZES:
        a, b = halves(width, height, seed=1000 * width + height)
        for radius in RADII:
            for with_b in (True, False):
                table[(width, height), radius, with_b] = (a, b if with_b else None, R.despeckle(a, b if with_b else None, radius=radius))
    return table


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_despeckle_is_the_restatement_bit_for_bit(size, expected, gpu_lib):
    for radius in RADII:
        for with_b in (True, False):
            a, b, (a_want, b_want, removed_want, counts_want) = expected[size, radius, with_b]
            what = "%dx%d radius %d %s" % (size + (radius, "with b" if with_b else "one image"))
            got = develop.despeckle(a, b, radius=radius)
            a_got, b_got, removed_got, counts_got = got if with_b else (got[0], None, got[1], got[2])
            print("%s: %r clamped" % (what, counts_got))
            assert_same_bits(a_got, a_want, what + ": a_out")
            if with_b:
                assert_same_bits(b_got, b_want, what + ": b_out")
            assert_same_bits(removed_got, removed_want, what + ": removed_out")
            assert counts_got == counts_want, what
            for turn in range(2):  # the device entry writes the same bytes, twice
                device = despeckle_on_device(a, b, radius=radius)
                assert device[0].tobytes() == a_got.tobytes() and device[2].tobytes() == removed_got.tobytes() and device[3] == counts_got, what + ": the device entry"
                assert (device[1] is None) == (not with_b) and (not with_b or device[1].tobytes() == b_got.tobytes()), what + ": the device entry"
            again = develop.despeckle(a, b, radius=radius)
            assert all(x.tobytes() == y.tobytes() if isinstance(x, np.ndarray) else x == y for x, y in zip(got, again)), what + ": two calls"


def test_the_inputs_take_every_path(expected):
    """A condition on the inputs, from the restatement alone: in the two ragged cases both halves lose pixels at either radius, the
    pixel bright in both halves, the NaN and the infinities keep their bits, the speck over black and a corner are clamped, and the small cases
    (n < 5 everywhere) are returned untouched."""
    for size in ((37, 29), (33, 17)):
        for radius in RADII:
            a, b, (a_out, b_out, removed, counts) = expected[size, radius, True]
            assert min(counts) >= 2, (size, radius, counts)
            y, x = size[1] // 2, size[0] // 2
            assert bits(a_out[y, x]).tolist() == bits(a[y, x]).tolist() and bits(b_out[y, x]).tolist() == bits(b[y, x]).tolist()
            for half, out, at in ((a, a_out, (3, 12)), (b, b_out, (5, 13)), (a, a_out, (12, 12)), (b, b_out, (12, 12))):  # what is not finite
                assert bits(out[at]).tolist() == bits(half[at]).tolist()
            assert not removed[12, 12].any() and np.isfinite(removed).all()
            assert a_out[10, 6, 0] < a[10, 6, 0]
            assert bits(a_out[0, 0]).tolist() != bits(a[0, 0]).tolist(), "a firefly in a corner of the image, where the window is a quarter of itself"
            assert expected[size, radius, False][2][3][0] > 0 and expected[size, radius, False][2][3][1] == 0
    for size in ((2, 1), (1, 1)):
        for radius in RADII:
            a, b, (a_out, b_out, removed, counts) = expected[size, radius, True]
            assert counts == (0, 0) and a_out.tobytes() == a.tobytes() and b_out.tobytes() == b.tobytes()


def test_a_wide_image_crosses_many_tiles(gpu_lib):
    """300 x 20: nineteen tiles a row and two rows of them, more than one workgroup a row of tiles."""
    a, b = halves(300, 20, seed=9)
    want = R.despeckle(a, b)
    got = develop.despeckle(a, b)
    for g, w, name in zip(got[:3], want[:3], ("a_out", "b_out", "removed_out")):
        assert_same_bits(g, w, "300x20: " + name)
    assert got[3] == want[3] and min(got[3]) > 0


# ------------------------------------------------------------------------------------------------------------------------ the session
def test_a_session_despeckles_as_the_pipeline_composed_by_hand(gpu_lib):
    from pyrite_amd import lua_project

    project, base_dir = lua_project.load_project(os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua"))
    project.setdefault("image", {}).update(width=32, height=32)
    project["renderer"] = project["renderer"].with_(pixel_samples=8)
    world, cam, r, film = scenes.build(project, seed=7, base_dir=base_dir)
    image = project.get("image") or {}
    develop_args = dict(filter=image.get("filter"), white=image.get("white"))
    span = (film.wavelength_start, film.wavelength_start + film.wavelength_width)
    with r.session((32, 32), cam, world, halves=True) as s:
        s.render(4)
        with pytest.raises(PyriteGpuError, match="two passes"):
            s.despeckled(**develop_args)
        s.render(4)
        before = [grains.copy() for grains in s.half_films()]
        developed = []
        for grains in before:
            half = Film(32, 32, film.bins, span)
            half.grains[...] = grains
            developed.append(develop.develop_linear(half, "srgb", **develop_args))
        for params in (dict(), dict(k=2.0, radius=1)):  # the defaults, and a k low enough that the noise itself is clamped
            a_out, b_out, removed, counts = develop.despeckle(developed[0], developed[1], **params)
            print("gallery 32 x 32 at 4 + 4 spp, %r: %r clamped" % (params, counts))
            got = s.despeckled(**develop_args, **params)
            assert got[0].tobytes() == ((a_out + b_out) * f32(0.5)).tobytes(), "the mean of the cleaned halves"
            assert got[1].tobytes() == (np.abs(a_out - b_out) * f32(0.5)).tobytes(), "half their difference"
            assert got[2].tobytes() == removed.tobytes() and got[3] == counts
            features = s.features()
            albedo = develop.develop_linear(features.albedo, "srgb", **develop_args)
            by_hand = develop.denoise(a_out, b_out, albedo=albedo, pixels=features.records, radius=3)
            got = s.despeckled(denoise=dict(radius=3), **develop_args, **params)
            assert got[0].tobytes() == by_hand[0].tobytes() and got[1].tobytes() == by_hand[1].tobytes(), "with the denoiser: the session entry against its parts"
            assert got[2].tobytes() == removed.tobytes() and got[3] == counts
            unguided = s.despeckled(denoise=dict(radius=2), guides=False, **develop_args, **params)
            assert unguided[0].tobytes() == develop.denoise(a_out, b_out, radius=2)[0].tobytes(), "without guides"
        assert sum(counts) > 0, "k = 2 clamps some of the noise: the session's test reads a cleaned image"
        assert all(x.tobytes() == y.tobytes() for x, y in zip(before, s.half_films())), "a half film changed under the despeckle"
    with r.session((32, 32), cam, world) as s:
        s.render(4)
        s.render(4)
        with pytest.raises(PyriteGpuError, match="PYR_SESSION_HALVES"):
            s.despeckled(**develop_args)
    world.close()


# ------------------------------------------------------------------------------------------------------------------------ the command lines
def test_both_command_lines_write_the_same_despeckled_image(gpu_lib, tmp_path):
    project = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--spp", "8", "--size", "32x32"]
    names = ("py", "cpp", "py_denoised", "cpp_denoised", "py_plain", "cpp_plain", "py_passes", "cpp_passes")
    paths = {name: str(tmp_path / (name + ".png")) for name in names}

    def py(out, *flags):
        return subprocess.run([sys.executable, "-m", "pyrite_amd", project, "--seed", "7", "-o", out] + common + list(flags), check=True, cwd=ROOT, env=env, timeout=600,
                              capture_output=True, text=True).stdout

    def cpp(out, *flags):
        return subprocess.run([gpu_build.HOST_TOOL, "render-project", project, "-", "7", out] + common + list(flags), check=True, cwd=ROOT, timeout=600, capture_output=True,
                              text=True).stdout

    flags = ("--despeckle", "2", "--despeckle-radius", "1")
    lines = [[line for line in run(paths[name], *flags).splitlines() if line.startswith("despeckle: ")] for run, name in ((py, "py"), (cpp, "cpp"))]
    assert len(lines[0]) == 1 and lines[0] == lines[1], lines  # one line with the two counts, the same from both
    py(paths["py_denoised"], "--despeckle", "--denoise", "--denoise-radius", "2")
    cpp(paths["cpp_denoised"], "--despeckle", "--denoise", "--denoise-radius", "2")
    py(paths["py_plain"])
    cpp(paths["cpp_plain"])
    py(paths["py_passes"], "--pass-samples", "4")  # what a run without the flag wrote before it existed: the session's film, hard clamp
    cpp(paths["cpp_passes"], "--pass-samples", "4")
    # the two tools pack their PNGs differently: the image bytes are what must agree
    image = {name: read_png(path).tobytes() for name, path in paths.items()}
    assert image["py"] == image["cpp"] and image["py_denoised"] == image["cpp_denoised"]
    assert image["py_plain"] == image["cpp_plain"] == image["py_passes"] == image["cpp_passes"]
    assert open(paths["py_plain"], "rb").read() == open(paths["py_passes"], "rb").read()
    assert image["py"] != image["py_plain"] and image["py_denoised"] != image["py"]  # and the flags do something
