"""The denoise kernels (pyrite_amd/csrc/kernels/denoise.hip) against the numpy restatement of include/pyrite_gpu.h's text
(tests/denoise_restatement.py), the host and the device entry against each other, a session's denoised image against the same
pipeline composed by hand, and the two command lines.

Parity bound: 1e-5 of the largest finite magnitude of either half in the pixel's window. Only expf differs from
the restatement, a few ulp on a weight, and the output is a weighted mean of the window. The largest observed ratio is printed and,
when PYRITE_OBSERVED_DIR names a directory, written to denoise_parity.txt there (kept as profiles/r09_denoise_parity.txt)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_restatement as R
from pyrite_amd import abi, develop, scenes
from pyrite_amd import build as gpu_build
from pyrite_amd._lib import PyriteGpuError, lib
from pyrite_amd.features import RECORD
from pyrite_amd.film import Film
from test_gpu_session import read_png

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
TOL = 1e-5
OBSERVED = {}

SIZES = [(37, 29), (16, 16), (5, 3), (1, 1)]  # ragged against the 16 x 16 tiles both ways; one tile; smaller than every window; one pixel
WINDOWS = [(1, 0), (3, 1), (10, 3)]
GUIDES = ["none", "albedo", "normal", "depth", "all"]


@pytest.fixture(scope="module", autouse=True)
def record_the_observed_parity():
    """After the module's tests: what the parity cases measured, written to the directory PYRITE_OBSERVED_DIR names, if any."""
    yield
    out_dir = os.environ.get("PYRITE_OBSERVED_DIR", "")
    if OBSERVED and os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "denoise_parity.txt"), "w") as f:
            f.write("largest |gpu - restatement| / (largest finite magnitude in the pixel's window); bound %g\n" % TOL)
            f.write("overall %.3g over %d comparisons\n" % (max(OBSERVED.values()), len(OBSERVED)))
            for what, worst in sorted(OBSERVED.items()):
                f.write("%-28s %.3g\n" % (what, worst))


def hdr_halves(width, height, seed):
    """Seeded HDR content over 1e-4 .. 1e3 with an edge, a flat zero block (V = 0), and -- where the image has room -- a NaN and an inf;
    an albedo, normals and depths that change where the content does or where it does not."""
    rng = np.random.default_rng(seed)
    level = np.exp(rng.uniform(np.log(1e-4), np.log(1e3), size=(height, width, 1))).astype(f32)
    level[:, width // 2:] = f32(2.0) + level[:, width // 2:] * f32(1e-3)  # a smooth half, where the filter really averages
    truth = (level * rng.uniform(0.5, 1.0, size=(1, 1, 3))).astype(f32)
    a = (truth * (1 + 0.3 * rng.standard_normal(truth.shape))).astype(f32)
    b = (truth * (1 + 0.3 * rng.standard_normal(truth.shape))).astype(f32)
    if width >= 5:
        a[height // 2:, :2] = 0
        b[height // 2:, :2] = 0
    if width >= 16:
        a[3, 4, 1] = np.nan
        b[height - 3, width - 2] = np.inf
    albedo = rng.uniform(0.1, 0.9, size=(1, 1, 3)).astype(f32) * np.ones((height, width, 3), dtype=f32)
    albedo[: height // 2] *= f32(0.97)
    albedo += (0.004 * rng.standard_normal(albedo.shape)).astype(f32)
    records = np.zeros((height, width), dtype=RECORD)
    normal = np.array([0.0, 0.6, 0.8], dtype=f32) + (0.03 * rng.standard_normal((height, width, 3))).astype(f32)
    records["normal"] = normal
    records["depth"] = (f32(5.0) + np.arange(width, dtype=f32)[None, :] * f32(0.02) + (0.01 * rng.standard_normal((height, width))).astype(f32))
    records["coverage"] = 1
    if width >= 5:  # a patch the camera sees nothing in: normal 0, depth 0
        records["normal"][:2, :2] = 0
        records["depth"][:2, :2] = 0
        records["coverage"][:2, :2] = 0
    return a, b, albedo, records


def gpu_denoise(a, b, albedo, records, params, want_error=True, device_entry=False, out_bits=None):
    """pyr_image_denoise / pyr_image_denoise_device through ctypes: (out, error or None). `out_bits`: the 32 bits every float of the
    device entry's outputs holds before the call (default: zeros)."""
    h, w, _ = a.shape
    p = develop.denoise_params(**params)
    out, error = np.full(a.shape, -7, dtype=f32), np.full(a.shape, -7, dtype=f32) if want_error else None
    if not device_entry:
        rc = lib().pyr_image_denoise(a.ctypes.data, b.ctypes.data, albedo.ctypes.data if albedo is not None else None, records.ctypes.data if records is not None else None,
                                     w, h, C.byref(p), out.ctypes.data, error.ctypes.data if want_error else None, 0)
        assert rc == abi.PYR_OK, lib().pyr_last_error()
        return out, error
    import torch

    def up(x):
        return None if x is None else torch.from_numpy(np.frombuffer(np.ascontiguousarray(x).tobytes(), dtype=np.uint8).copy()).cuda()

    ta, tb, talb, trec = up(a), up(b), up(albedo), up(records)
    tout, terr = torch.zeros(a.size * 4, dtype=torch.uint8, device="cuda"), torch.zeros(a.size * 4, dtype=torch.uint8, device="cuda")
    if out_bits is not None:
        tout, terr = (torch.full((a.size,), out_bits, dtype=torch.int32, device="cuda").view(torch.uint8) for _ in range(2))
    stream = torch.cuda.current_stream()
    rc = lib().pyr_image_denoise_device(C.c_void_p(ta.data_ptr()), C.c_void_p(tb.data_ptr()), C.c_void_p(talb.data_ptr()) if talb is not None else None,
                                        C.c_void_p(trec.data_ptr()) if trec is not None else None, w, h, C.byref(p), C.c_void_p(tout.data_ptr()),
                                        C.c_void_p(terr.data_ptr()) if want_error else None, 0, C.c_void_p(stream.cuda_stream))
    assert rc == abi.PYR_OK, lib().pyr_last_error()
    stream.synchronize()
    back = lambda t: np.frombuffer(t.cpu().numpy().tobytes(), dtype=f32).reshape(a.shape)  # noqa: E731
    return back(tout), back(terr) if want_error else None


def window_scale(a, b, radius):
    """The largest finite magnitude of either half in every pixel's window."""
    h, w, _ = a.shape
    m = np.maximum(np.where(np.isfinite(a), np.abs(a), 0).max(-1), np.where(np.isfinite(b), np.abs(b), 0).max(-1))
    padded = np.zeros((h + 2 * radius, w + 2 * radius), dtype=f32)
    padded[radius:radius + h, radius:radius + w] = m
    return np.lib.stride_tricks.sliding_window_view(padded, (2 * radius + 1, 2 * radius + 1)).max(axis=(2, 3))


def assert_close(got, expected, scale, what):
    finite = np.isfinite(expected)
    assert np.array_equal(np.isnan(got), np.isnan(expected)), what + ": NaNs elsewhere"
    assert np.array_equal(got[~finite & ~np.isnan(expected)], expected[~finite & ~np.isnan(expected)]), what + ": infinities differ"
    ratio = np.where(finite, np.abs(np.where(finite, got, 0) - np.where(finite, expected, 0)), 0) / np.maximum(scale, f32(1e-30))[..., None]
    worst = float(ratio.max())
    OBSERVED[what] = worst
    print("%s: largest |gpu - restatement| / window scale %.3g" % (what, worst))
    assert worst <= TOL, what


@pytest.mark.parametrize("radius,patch", WINDOWS, ids=["r%dp%d" % w for w in WINDOWS])
@pytest.mark.parametrize("width,height", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_the_kernels_match_the_restatement(width, height, radius, patch, gpu_lib):
    a, b, albedo, records = hdr_halves(width, height, seed=100 * width + radius)
    normal, depth = np.ascontiguousarray(records["normal"]), np.ascontiguousarray(records["depth"])
    v = R.variance(a, b)
    distances = (R.colour_distance(b, v, radius, patch, R.DEFAULTS["k"], R.DEFAULTS["epsilon"]), R.colour_distance(a, v, radius, patch, R.DEFAULTS["k"], R.DEFAULTS["epsilon"]))
    scale = window_scale(a, b, radius)
    off = dict(sigma_albedo=0.0, sigma_normal=0.0, sigma_depth=0.0)
    for i, guides in enumerate(GUIDES):
        params = dict(radius=radius, patch=patch)
        if guides != "all":
            params.update({k: v_ for k, v_ in off.items() if k != "sigma_" + guides})
        use_albedo, use_records = guides in ("albedo", "all"), guides in ("normal", "depth", "all")
        expected, expected_error = R.denoise(a, b, albedo if use_albedo else None, normal if guides in ("normal", "all") else None,
                                             depth if guides in ("depth", "all") else None, distances=distances, **params)
        # a buffer that is given with its sigma off must change nothing: the guides that are off are still passed on odd rounds
        pass_all = i % 2 == 1
        out, error = gpu_denoise(a, b, albedo if use_albedo or pass_all else None, records if use_records or pass_all else None, params)
        what = "%dx%d r%d p%d %s" % (width, height, radius, patch, guides)
        assert_close(out, expected, scale, what)
        assert_close(error, expected_error, scale, what + " error")
        alone, none = gpu_denoise(a, b, albedo if use_albedo else None, records if use_records else None, params, want_error=False)
        assert none is None and alone.tobytes() == out.tobytes(), what + ": the image depends on whether the error is asked for"
    if width > 1:  # the planted values stay where they are
        assert np.array_equal(~np.isfinite(out).all(-1), ~(np.isfinite(a).all(-1) & np.isfinite(b).all(-1)))


def test_the_filter_really_filters_on_the_gpu(gpu_lib):
    """Against parity with a restatement that does nothing: the smooth half of the image comes back much closer to its truth."""
    a, b, _, _ = hdr_halves(37, 29, seed=3)
    out, _ = develop.denoise(a, b)
    region = (slice(8, 20), slice(24, 34))

    def spread(x):  # the relative scatter of a flat region, channel by channel
        return float(np.mean([np.std(x[region][..., c]) / np.mean(x[region][..., c]) for c in range(3)]))

    spread_in, spread_out = spread((a + b) * f32(0.5)), spread(out)
    print("relative spread of a flat region: %.3f before, %.3f after" % (spread_in, spread_out))
    assert spread_out < 0.5 * spread_in


def test_the_host_and_the_device_entry_write_the_same_bytes_twice(gpu_lib):
    a, b, albedo, records = hdr_halves(37, 29, seed=11)
    params = dict(radius=3, patch=1)
    host = gpu_denoise(a, b, albedo, records, params)
    again = gpu_denoise(a, b, albedo, records, params)
    device = gpu_denoise(a, b, albedo, records, params, device_entry=True)
    for x, y in zip(host, again):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(host, device):
        assert x.tobytes() == y.tobytes()
    assert gpu_denoise(a, b, None, None, params, want_error=False, device_entry=True)[0].tobytes() == gpu_denoise(a, b, None, None, params)[0].tobytes()
    image, error = develop.denoise(a, b, albedo=albedo, pixels=records, **params)  # and the Python surface is that entry
    assert image.tobytes() == host[0].tobytes() and error.tobytes() == host[1].tobytes()


def test_a_session_denoises_as_the_pipeline_composed_by_hand(gpu_lib):
    world, cam, r, film = scenes.build(scenes.c2_cornell(48, 40, 16), seed=5)
    whole = r.new_film(48, 40)
    r.render(whole, cam, world)
    span = (film.wavelength_start, film.wavelength_start + film.wavelength_width)
    with r.session((48, 40), cam, world, halves=True) as s:
        s.render(8)
        with pytest.raises(PyriteGpuError, match="two passes") as one_pass:
            s.denoised()
        assert one_pass.value.status == abi.PYR_ERR_INVALID_ARGUMENT
        s.render(8)
        image, error = s.denoised()
        unguided, _ = s.denoised(guides=False, radius=3)
        halves = []
        for grains in s.half_films():
            half = Film(48, 40, film.bins, span)
            half.grains[...] = grains
            halves.append(develop.develop_linear(half, "srgb"))
        features = s.features()
        albedo = develop.develop_linear(features.albedo, "srgb")
        by_hand, by_hand_error = develop.denoise(halves[0], halves[1], albedo=albedo, pixels=features.records)
        assert image.tobytes() == by_hand.tobytes() and error.tobytes() == by_hand_error.tobytes()
        assert unguided.tobytes() == develop.denoise(halves[0], halves[1], radius=3)[0].tobytes()
        assert np.isfinite(image).all() and not np.array_equal(image, (halves[0] + halves[1]) * f32(0.5))
        assert np.array_equal(s.film().grains[..., 1], whole.grains[..., 1])  # the films were not touched
    with r.session((48, 40), cam, world, halves=True) as s:  # a pass rendered after a denoise still adds up to the one-shot film
        s.render(4)
        s.render(4)
        s.denoised()
        s.render(8)
        after = s.film()
        assert np.array_equal(after.grains[..., 1], whole.grains[..., 1])
        x, y = after.develop(), whole.develop()
        assert (np.sqrt(((x - y) ** 2).sum(-1)) / (np.sqrt((y ** 2).sum(-1)) + 1e-6)).max() <= TOL
    with r.session((48, 40), cam, world, halves=False) as s:
        s.render(8)
        s.render(8)
        with pytest.raises(PyriteGpuError, match="PYR_SESSION_HALVES") as no_halves:
            s.denoised()
        assert no_halves.value.status == abi.PYR_ERR_INVALID_ARGUMENT
    world.close()


def test_both_command_lines_write_the_same_denoised_image(gpu_lib, tmp_path):
    project = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--spp", "8", "--size", "48x32"]
    paths = {name: str(tmp_path / (name + ".png")) for name in ("py", "py_plain", "py_again", "cpp", "cpp_plain", "cpp_again")}
    hdr_py, hdr_cpp = str(tmp_path / "py.hdr"), str(tmp_path / "cpp.hdr")

    def py(out, *flags):
        subprocess.run([sys.executable, "-m", "pyrite_amd", project, "--seed", "7", "-o", out] + common + list(flags), check=True, cwd=ROOT, env=env, timeout=600,
                       capture_output=True)

    def cpp(out, *flags):
        subprocess.run([gpu_build.HOST_TOOL, "render-project", project, "-", "7", out] + common + list(flags), check=True, cwd=ROOT, timeout=600, capture_output=True)

    py(paths["py"], "--denoise", "--hdr", hdr_py)
    cpp(paths["cpp"], "--denoise", "--hdr", hdr_cpp)
    py(paths["py_plain"])
    py(paths["py_again"], "--pass-samples", "4")  # what a plain run wrote before this flag existed: the session's film, hard clamp
    cpp(paths["cpp_plain"])
    cpp(paths["cpp_again"], "--pass-samples", "4")
    data = {name: open(path, "rb").read() for name, path in paths.items()}
    assert data["py"] == open(paths["py"], "rb").read()
    # the two tools pack their PNGs differently (zlib level 6 against stored blocks): the image bytes are what must agree
    assert read_png(paths["py"]).tobytes() == read_png(paths["cpp"]).tobytes()
    assert open(hdr_py, "rb").read() == open(hdr_cpp, "rb").read()
    assert data["py_plain"] == data["py_again"] and data["cpp_plain"] == data["cpp_again"]
    assert read_png(paths["py_plain"]).tobytes() == read_png(paths["cpp_plain"]).tobytes()
    assert read_png(paths["py"]).tobytes() != read_png(paths["py_plain"]).tobytes()  # and the flag does something
