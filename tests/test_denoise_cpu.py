"""The denoiser without a GPU: what the semantics of include/pyrite_gpu.h ("denoising a linear image from two halves") achieve,
measured on their numpy restatement (tests/denoise_restatement.py; tests/test_gpu_denoise.py holds the kernels against it), the
argument checks of pyr_image_denoise, the flags of the two command lines, and the stand-alone address walk of the kernel's tile
addressing under AddressSanitizer and UBSan.

The thresholds of the quality tests are properties of the semantics, not of a kernel: each is the restatement's own value on the
seeds 0..3, written beside it, with a margin for other seeds."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_restatement as R
from pyrite_amd import abi, develop
from pyrite_amd import build as gpu_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
H, W = 40, 48


def noisy_halves(seed, sigma=0.3):
    """A 48 x 40 image with a 1 : 1.3 vertical edge and a 1 : 20 horizontal one, two halves under multiplicative Gaussian noise, and
    an albedo that carries the 1.3 edge alone."""
    rng = np.random.default_rng(seed)
    truth = np.ones((H, W, 3), dtype=f32) * np.array([0.8, 0.5, 0.3], dtype=f32)
    truth[:, W // 2:] *= f32(1.3)
    truth[H // 2:] *= f32(20.0)
    a = (truth * (1 + sigma * rng.standard_normal(truth.shape))).astype(f32)
    b = (truth * (1 + sigma * rng.standard_normal(truth.shape))).astype(f32)
    albedo = np.ones((H, W, 3), dtype=f32) * f32(0.5)
    albedo[:, W // 2:] *= f32(1.3)
    return truth, a, b, albedo


def rel_rmse(x, truth):
    return float(np.sqrt(np.mean(((x - truth) / truth) ** 2)))


def edge_step(x, truth):
    """The mean step across the 1.3 edge in units of the level left of it: three columns on either side. 0.3 in the truth."""
    n = x / truth[:, :1]
    return float(np.mean(n[:, W // 2:W // 2 + 3]) - np.mean(n[:, W // 2 - 3:W // 2]))


@pytest.fixture(scope="module")
def filtered():
    truth, a, b, albedo = noisy_halves(0)
    return truth, a, b, R.denoise(a, b), R.denoise(a, b, albedo=albedo)


def test_the_filter_removes_most_of_the_noise(filtered):
    """Relative RMSE against the truth, as a fraction of that of (a + b) / 2. Observed without guides at the defaults: 0.200, 0.184,
    0.187, 0.179 on the seeds 0..3 (and 0.203, 0.173, 0.189, 0.180 at sigma 0.05); the bound is the largest with a quarter on top."""
    truth, a, b, (out, error), _ = filtered
    ratio = rel_rmse(out, truth) / rel_rmse((a + b) * f32(0.5), truth)
    print("relative RMSE ratio %.4f" % ratio)
    assert ratio <= 0.25
    # the error image is the filter's own estimate of what is left: the same order as the true error, far below the input's noise
    assert 0.25 * rel_rmse(out, truth) <= float(np.sqrt(np.mean((error / truth) ** 2))) <= 4 * rel_rmse(out, truth)


def test_low_noise_is_filtered_as_well():
    """Observed 0.203 on seed 0 at sigma 0.05: the variance estimate scales the distance, the ratio does not depend on the level."""
    truth, a, b, _ = noisy_halves(0, sigma=0.05)
    ratio = rel_rmse(R.denoise(a, b)[0], truth) / rel_rmse((a + b) * f32(0.5), truth)
    print("relative RMSE ratio at sigma 0.05 %.4f" % ratio)
    assert ratio <= 0.25


def test_an_albedo_guide_keeps_the_edge_it_carries(filtered):
    """The mean step across the 1.3 edge. Observed: 0.320, 0.307, 0.302, 0.314 with the guide against 0.199, 0.190, 0.187, 0.191
    without on the seeds 0..3 (0.3 in the truth): a noisy 1.3 : 1 edge is within the noise of the colour distance and blurs; the
    guide forbids the averaging across it."""
    truth, a, b, (plain, _), (guided, _) = filtered
    step_plain, step_guided = edge_step(plain, truth), edge_step(guided, truth)
    print("step across the edge: %.4f guided, %.4f unguided" % (step_guided, step_plain))
    assert abs(step_guided - 0.3) < abs(step_plain - 0.3)
    assert abs(step_guided - 0.3) <= 0.04 and step_plain <= 0.25
    assert rel_rmse(guided, truth) < rel_rmse(plain, truth)  # observed 0.178 against 0.200 of the input's error


def test_a_noise_free_edge_comes_back_untouched():
    """a == b: V = 0 everywhere, the distance across the step is its square over epsilon, every cross-edge weight underflows to 0."""
    image = np.full((20, 24, 3), 0.25, dtype=f32)
    image[:, 12:] = f32(4.0)
    image[10:, :, 1] *= f32(3.0)
    out, error = R.denoise(image, image.copy())
    assert np.max(np.abs(out - image) / image) <= 1e-6
    assert np.max(error) == 0.0


def test_a_nan_pixel_stays_one_pixel():
    truth, a, b, _ = noisy_halves(1)
    a[17, 20, 1] = np.nan
    b[30, 5] = np.inf
    out, error = R.denoise(a, b)
    bad = ~np.isfinite(out).all(axis=-1)
    assert sorted(map(tuple, np.argwhere(bad))) == [(17, 20), (30, 5)]
    # around it the filter steps aside: within patch + 1 = 2 pixels the output is the plain mean of the halves
    near = np.zeros((H, W), dtype=bool)
    near[15:20, 18:23] = True
    near[17, 20] = False
    assert np.array_equal(out[near], ((a + b) * f32(0.5))[near])
    clean = R.denoise(*noisy_halves(1)[1:3])[0]
    far = np.ones((H, W), dtype=bool)
    far[17 - 7:17 + 8, 20 - 7:20 + 8] = False
    far[30 - 7:30 + 8, 0:5 + 8] = False
    assert np.array_equal(out[far], clean[far])  # radius + patch + 1 away nothing has changed


def test_the_variance_is_half_the_mean_squared_difference():
    rng = np.random.default_rng(5)
    a, b = rng.random((3, 4, 3)).astype(f32), rng.random((3, 4, 3)).astype(f32)
    v = R.variance(a, b)
    s = (a - b) ** 2
    assert v[0, 0, 0] == f32(0.5) * (((s[0, 0, 0] + s[0, 1, 0]) + s[1, 0, 0]) + s[1, 1, 0]) / f32(4)
    assert np.allclose(v[1, 1], 0.5 * s[0:3, 0:3].mean(axis=(0, 1)), rtol=1e-6)
    one = R.variance(a[:1, :1], b[:1, :1])
    assert one[0, 0, 2] == f32(0.5) * s[0, 0, 2]


# ------------------------------------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    gpu_build.build()
    return abi.bind(C.CDLL(gpu_build.OUT))


def test_the_parameter_block_is_the_header_s(lib):
    assert C.sizeof(abi.PyrDenoiseParams) == 32
    p = develop.denoise_params()
    assert (p.radius, p.patch, p.reserved) == (5, 1, 0)
    assert (f32(p.k), f32(p.epsilon), f32(p.sigma_albedo), f32(p.sigma_normal), f32(p.sigma_depth)) == (f32(0.45), f32(1e-10), f32(0.02), f32(0.1), f32(0.02))
    header = open(os.path.join(ROOT, "include", "pyrite_gpu.h")).read()
    for name, value in [("RADIUS", "5u"), ("PATCH", "1u"), ("K", "0.45f"), ("EPSILON", "1e-10f"), ("SIGMA_ALBEDO", "0.02f"), ("SIGMA_NORMAL", "0.1f"),
                        ("SIGMA_DEPTH", "0.02f")]:
        assert "#define PYR_DENOISE_%s %s\n" % (name, value) in header
    assert set(R.DEFAULTS.items()) == {("radius", 5), ("patch", 1), ("k", 0.45), ("epsilon", 1e-10), ("sigma_albedo", 0.02), ("sigma_normal", 0.1), ("sigma_depth", 0.02)}
    assert lib.pyr_abi_version() == 5


def call(lib, a=True, b=True, width=4, height=3, params=True, out=True, device=0, entry="pyr_image_denoise", **fields):
    image = np.zeros((3, 4, 3), dtype=f32)
    result = np.zeros((3, 4, 3), dtype=f32)
    p = develop.denoise_params()
    for name, value in fields.items():
        setattr(p, name, value)
    args = [image.ctypes.data if a else None, image.ctypes.data if b else None, None, None, width, height, C.byref(p) if params else None,
            result.ctypes.data if out else None, None, device]
    if entry.endswith("_device"):
        args.append(None)
    rc = getattr(lib, entry)(*args)
    return rc, lib.pyr_last_error().decode()


REFUSED = [
    (dict(a=False), "a"), (dict(b=False), "b"), (dict(params=False), "params"), (dict(out=False), "out"),
    (dict(width=0), "width"), (dict(height=0), "height"),
    (dict(radius=0), "radius"), (dict(radius=11), "radius"), (dict(patch=4), "patch"),
    (dict(k=0.0), "k"), (dict(k=-1.0), "k"), (dict(k=float("nan")), "k"),
    (dict(epsilon=0.0), "epsilon"), (dict(epsilon=float("nan")), "epsilon"),
    (dict(reserved=1), "reserved"),
]


@pytest.mark.parametrize("entry", ["pyr_image_denoise", "pyr_image_denoise_device"])
@pytest.mark.parametrize("change,name", REFUSED)
def test_bad_arguments_are_refused_by_name_before_a_device_is_looked_for(change, name, entry, lib):
    rc, message = call(lib, entry=entry, device=99, **change)  # no such device: the argument is still what is reported
    assert rc == abi.PYR_ERR_INVALID_ARGUMENT
    assert name in message.replace("params->", " ").replace(":", " ").split(), message


@pytest.mark.parametrize("entry", ["pyr_image_denoise", "pyr_image_denoise_device"])
def test_size_then_device(entry, lib):
    rc, message = call(lib, entry=entry, width=65536, height=65536, device=99)
    assert rc == abi.PYR_ERR_UNSUPPORTED and "2^32" in message
    rc, message = call(lib, entry=entry, device=99)
    assert rc == abi.PYR_ERR_DEVICE
    if lib.pyr_device_count() <= 0:  # valid arguments where there is no GPU
        assert call(lib, entry=entry)[0] == abi.PYR_ERR_DEVICE
    assert call(lib, entry=entry, sigma_albedo=0.0, sigma_normal=-1.0, sigma_depth=0.0, device=99)[0] == abi.PYR_ERR_DEVICE  # a guide turned off is no error
    assert lib.pyr_session_denoised(None, None, None, None, None, None) == abi.PYR_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------------------------------ the flags
BAD_FLAGS = [
    (["--denoise", "--spp", "7"], "--denoise needs an even number of samples per pixel: the two half films must be equal"),
    (["--denoise", "--spp", "8", "--pass-samples", "3"], "--denoise needs an even number of equal passes: the samples per pixel must be a multiple of twice --pass-samples"),
    (["--denoise-radius", "3"], "--denoise-radius needs --denoise"),
    (["--denoise", "--denoise-radius", "11"], "--denoise-radius must be 1 to 10"),
]


def test_flag_rules():
    assert develop.denoise_flag_problem(False, None) is None and develop.denoise_flag_problem(True, 10, 64, 16) is None
    assert develop.denoise_flag_problem(False, None, 7) is None  # an odd budget is fine without --denoise
    assert develop.denoise_flag_problem(True, None, 7) == BAD_FLAGS[0][1]
    assert develop.denoise_flag_problem(True, None, 8, 3) == BAD_FLAGS[1][1] and develop.denoise_flag_problem(True, None, 8, 2) is None
    assert develop.denoise_flag_problem(False, 3) == BAD_FLAGS[2][1] and develop.denoise_flag_problem(True, 0) == BAD_FLAGS[3][1]


@pytest.mark.parametrize("flags,message", BAD_FLAGS)
def test_both_front_ends_reject_the_same_flags_in_the_same_words(flags, message, lib):
    project = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    py = subprocess.run([sys.executable, "-m", "pyrite_amd", project] + flags, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", project, "-", "1", os.devnull] + flags, cwd=ROOT, capture_output=True, text=True)
    assert py.returncode == 2 and cpp.returncode == 2
    assert py.stderr.strip() == cpp.stderr.strip() == "error: " + message


def test_both_front_ends_parse_the_flags(lib, tmp_path):
    """Well-formed flags get past the parser: what stops the run here is the missing GPU (or nothing, on a GPU box)."""
    project = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    flags = ["--denoise", "--denoise-radius", "2", "--spp", "2", "--size", "16x16"]
    py = subprocess.run([sys.executable, "-m", "pyrite_amd", project, "-o", str(tmp_path / "a.png")] + flags, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                        capture_output=True, text=True)
    cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", project, "-", "1", str(tmp_path / "b.png")] + flags, cwd=ROOT, capture_output=True, text=True)
    for run in (py, cpp):
        assert "unrecognized" not in run.stderr and "unknown flag" not in run.stderr and "must" not in run.stderr and "needs" not in run.stderr, run.stderr
        assert run.returncode == 0 or "HIP device" in run.stderr, run.stderr


# ------------------------------------------------------------------------------------------------------------------------ the addresses
def test_the_tile_addressing_stays_in_range_under_the_sanitizers(tmp_path):
    """tests/probes/denoise_address_check.cpp: a program of its own with the kernel's addressing function, run as a child process;
    nothing is loaded into this interpreter."""
    exe = tmp_path / "denoise_address_check"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-o", str(exe),
                           os.path.join(ROOT, "tests", "probes", "denoise_address_check.cpp")])
    run = subprocess.run([str(exe)], capture_output=True, text=True)  # the runtimes are linked statically: the environment stays as it is
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok: ")
