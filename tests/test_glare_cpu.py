"""The glare without a GPU (include/pyrite_gpu.h "glare"): the new names of the ABI in the header, abi.py and
the library, every argument check before a device is looked for, the C++ wrappers through a stand-alone program, the flags of the two
command lines, and the numpy restatement (tests/glare_restatement.py, which tests/test_gpu_glare.py holds the kernels against) on
properties of the rule itself."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import glare_restatement as R
from pyrite_amd import abi, develop
from pyrite_amd import build as gpu_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pyrite_gpu.h")
f32 = np.float32
IMAGE_ENTRIES = ["pyr_image_glare", "pyr_image_glare_device"]
NEW_ENTRIES = IMAGE_ENTRIES + ["pyr_session_glared"]


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
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "%s"' % HEADER, "int main(void){", 'printf("size %zu\\n", sizeof(PyrGlareParams));']
    for field, _ in abi.PyrGlareParams._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(PyrGlareParams, %s));' % (field, field))
    lines += ['printf("floats %.9g %.9g %.9g\\n", (double)PYR_GLARE_STRENGTH, (double)PYR_GLARE_THRESHOLD, (double)PYR_GLARE_FALLOFF);',
              'printf("ints %u %u\\n", PYR_GLARE_LEVELS, PYR_GLARE_MOST_LEVELS);', "return 0;}"]
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines))
    subprocess.check_call(["gcc", "-o", exe, src])
    seen = dict(line.split(None, 1) for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(seen["size"]) == C.sizeof(abi.PyrGlareParams) == 32
    for field, _ in abi.PyrGlareParams._fields_:
        assert int(seen[field]) == getattr(abi.PyrGlareParams, field).offset, field
    assert [f32(float(v)) for v in seen["floats"].split()] == [f32(abi.PYR_GLARE_STRENGTH), f32(abi.PYR_GLARE_THRESHOLD), f32(abi.PYR_GLARE_FALLOFF)]
    assert [int(v) for v in seen["ints"].split()] == [abi.PYR_GLARE_LEVELS, abi.PYR_GLARE_MOST_LEVELS] == [6, 12] and R.MOST_LEVELS == 12
    assert "#define PYR_ABI_VERSION 5\n" in header and abi.PYR_ABI_VERSION == 5 and lib.pyr_abi_version() == 5  # additions only


def test_the_python_defaults_are_the_header_s():
    p = develop.glare_params()
    assert (f32(p.strength), p.levels, f32(p.threshold), f32(p.falloff)) == (f32(abi.PYR_GLARE_STRENGTH), abi.PYR_GLARE_LEVELS, f32(abi.PYR_GLARE_THRESHOLD), f32(abi.PYR_GLARE_FALLOFF))
    assert (f32(p.strength), p.levels, p.threshold, p.falloff, list(p.reserved)) == (f32(0.1), 6, 0.0, 1.0, [0, 0, 0, 0])
    defaults = {k: v.default for k, v in inspect.signature(R.glare).parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(strength=0.1, levels=6, threshold=0.0, falloff=1.0)  # the restatement's too


# ------------------------------------------------------------------------------------------------------------------------ the argument checks
def glare_call(lib, entry="pyr_image_glare", missing=(), params=True, width=4, height=3, device=99, overlap=None, **fields):
    """One call with 4 x 3 buffers of zeros; `missing` names the pointers passed as NULL, `overlap` = "first" or "last": out starts
    on the last pixel of image, or image on the last pixel of out. A larger image gets addresses that are far apart and never read."""
    store = np.zeros(2 * 12 * 12 + 64, dtype=np.uint8)
    at = {"image": store.ctypes.data, "out": store.ctypes.data + 12 * 12 + 32}
    if width * height > 12:  # never read: an image this large is refused, and its two buffers must still lie apart
        at = {"image": 1 << 12, "out": 1 << 60}
    if overlap == "last":
        at["out"] = at["image"] + 11 * 12
    if overlap == "first":
        at["image"] = at["out"] + 11 * 12
    p = develop.glare_params()
    for name, value in fields.items():
        if name == "reserved":
            p.reserved[value] = 1
        else:
            setattr(p, name, value)
    ptr = lambda name: None if name in missing else at[name]  # noqa: E731
    args = [ptr("image"), width, height, C.byref(p) if params else None, ptr("out"), device]
    if entry.endswith("_device"):
        args.append(None)
    rc = getattr(lib, entry)(*args)
    return rc, lib.pyr_last_error().decode()


NAN, INF = float("nan"), float("inf")
REFUSED = [
    (dict(missing=("image",)), "image"), (dict(params=False), "params"), (dict(missing=("out",)), "out"),
    (dict(width=0), "width"), (dict(height=0), "height"),
    (dict(strength=0.0), "strength"), (dict(strength=-0.1), "strength"), (dict(strength=1.5), "strength"), (dict(strength=NAN), "strength"), (dict(strength=INF), "strength"),
    (dict(levels=0), "levels"), (dict(levels=13), "levels"), (dict(levels=0xFFFFFFFF), "levels"),
    (dict(threshold=-1.0), "threshold"), (dict(threshold=NAN), "threshold"), (dict(threshold=INF), "threshold"),
    (dict(falloff=0.0), "falloff"), (dict(falloff=-1.0), "falloff"), (dict(falloff=4.5), "falloff"), (dict(falloff=NAN), "falloff"), (dict(falloff=INF), "falloff"),
    (dict(reserved=0), "reserved"), (dict(reserved=1), "reserved"), (dict(reserved=2), "reserved"), (dict(reserved=3), "reserved"),
]


def names_in(message):
    return message.replace("params->", " ").replace(":", " ").replace(",", " ").split()


@pytest.mark.parametrize("entry", IMAGE_ENTRIES)
@pytest.mark.parametrize("change,name", REFUSED)
def test_the_glare_refuses_bad_arguments_by_name_before_a_device_is_looked_for(change, name, entry, lib):
    rc, message = glare_call(lib, entry=entry, **change)  # no device 99: the argument is still what is reported
    assert rc == abi.PYR_ERR_INVALID_ARGUMENT
    assert name in names_in(message), message


def test_the_device_form_refuses_an_out_that_overlaps_the_image(lib):
    for overlap in ("first", "last"):
        rc, message = glare_call(lib, entry="pyr_image_glare_device", overlap=overlap)
        assert rc == abi.PYR_ERR_INVALID_ARGUMENT and message.split() == ["out_device", "overlaps", "image_device"], message
        assert glare_call(lib, entry="pyr_image_glare", overlap=overlap)[0] == abi.PYR_ERR_DEVICE  # host buffers are copied: no such rule
    assert glare_call(lib, entry="pyr_image_glare_device", overlap="last", levels=0)[1].split()[0] == "params->levels"  # what both entries refuse comes first


@pytest.mark.parametrize("entry", IMAGE_ENTRIES)
def test_size_then_device(entry, lib):
    rc, message = glare_call(lib, entry=entry, width=65536, height=65536)
    assert rc == abi.PYR_ERR_UNSUPPORTED and "2^32" in message
    assert glare_call(lib, entry=entry, width=65536, height=65536, levels=13)[0] == abi.PYR_ERR_INVALID_ARGUMENT  # a parameter before the size
    assert glare_call(lib, entry=entry)[0] == abi.PYR_ERR_DEVICE
    assert glare_call(lib, entry=entry, strength=1.0, levels=12, threshold=0.0, falloff=4.0)[0] == abi.PYR_ERR_DEVICE  # the edges are inside
    assert glare_call(lib, entry=entry, strength=1e-6, levels=1, threshold=1e30, falloff=1e-6)[0] == abi.PYR_ERR_DEVICE
    assert glare_call(lib, entry=entry, width=1, height=1)[0] == abi.PYR_ERR_DEVICE
    if lib.pyr_device_count() <= 0:  # valid arguments where there is no GPU
        assert glare_call(lib, entry=entry, device=0)[0] == abi.PYR_ERR_DEVICE


def test_the_session_entry_names_what_is_missing(lib):
    p, d, out = develop.glare_params(), abi.PyrDevelopParams(), np.zeros(3, dtype=f32)
    session = C.c_void_p(1)  # never read: every check below comes before the session is looked at
    for args, name in (((None, C.byref(d), C.byref(p), out.ctypes.data), "session"), ((session, None, C.byref(p), out.ctypes.data), "develop_params"),
                       ((session, C.byref(d), C.byref(p), None), "out"), ((session, C.byref(d), None, out.ctypes.data), "glare_params")):
        assert lib.pyr_session_glared(*args) == abi.PYR_ERR_INVALID_ARGUMENT
        assert lib.pyr_last_error().decode().split()[-1] == name
    p.levels = 13
    assert lib.pyr_session_glared(session, C.byref(d), C.byref(p), out.ctypes.data) == abi.PYR_ERR_INVALID_ARGUMENT
    assert lib.pyr_last_error().decode().startswith("glare_params->levels")


def test_the_python_wrapper_checks_its_image(lib):
    with pytest.raises(AssertionError):
        develop.glare(np.zeros((3, 4), dtype=f32), device=99)
    with pytest.raises(TypeError):
        develop.glare(np.zeros((3, 4, 3), dtype=f32), shutter=0.5, device=99)
    with pytest.raises(Exception) as refused:  # good arguments reach the library, which finds no device 99
        develop.glare(np.zeros((3, 4, 3), dtype=f32), strength=0.5, levels=3, threshold=1.0, falloff=2.0, device=99)
    assert not isinstance(refused.value, (AssertionError, ValueError, TypeError))


# ------------------------------------------------------------------------------------------------------------------------ the C++ wrappers
def test_the_cpp_wrappers(lib, tmp_path):
    """pyrite::glare, glare_params and glare_from_flags from a stand-alone program (tests/glare_driver.cpp) linked against
    libpyrite_host.so: the ProjectError for a buffer of the wrong size, the GpuError and its status for a parameter out of range, and
    with good arguments PYR_ERR_DEVICE here -- or, where there is a GPU, a constant image that stays constant and a 1 x 1 image's bits."""
    exe = str(tmp_path / "glare_driver")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "glare_driver.cpp"), "-L" + gpu_build.HOST_DIR, "-lpyrite_host", "-L" + gpu_build.CSRC, "-lpyrite_gpu",
                           "-Wl,-rpath," + gpu_build.HOST_DIR, "-Wl,-rpath," + gpu_build.CSRC])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-2000:]
    assert run.stdout.split()[0] == "ok"


# ------------------------------------------------------------------------------------------------------------------------ the flags
BAD_FLAGS = [
    (["--glare-levels", "3"], "--glare-levels needs --glare"),
    (["--glare-threshold", "1"], "--glare-threshold needs --glare"),
    (["--glare", "0"], "--glare must be a strength above 0 and at most 1"),
    (["--glare", "1.5"], "--glare must be a strength above 0 and at most 1"),
    (["--glare", "much"], "--glare must be a strength above 0 and at most 1"),
    (["--glare", "nan"], "--glare must be a strength above 0 and at most 1"),
    (["--glare", "--glare-levels", "0"], "--glare-levels must be 1 to 12"),
    (["--glare", "0.2", "--glare-levels", "13"], "--glare-levels must be 1 to 12"),
    (["--glare", "--glare-threshold", "-1"], "--glare-threshold must be a finite number that is not negative"),
    (["--glare", "--glare-threshold", "inf"], "--glare-threshold must be a finite number that is not negative"),
]


def test_flag_rules():
    assert develop.glare_flag_problem(None, None, None) is None and develop.glare_from_flags(None, None, None) is None
    assert develop.glare_flag_problem("0.1", None, None) is None and develop.glare_flag_problem("1", 12, 0.0) is None and develop.glare_flag_problem(0.5, 1, 3.0) is None
    assert develop.glare_flag_problem(None, 3, None) == BAD_FLAGS[0][1] and develop.glare_flag_problem(None, None, 1.0) == BAD_FLAGS[1][1]
    assert develop.glare_flag_problem("0", None, None) == develop.glare_flag_problem("x", None, None) == develop.glare_flag_problem("-1", None, None) == BAD_FLAGS[2][1]
    assert develop.glare_flag_problem("0.1", 0, None) == BAD_FLAGS[6][1] and develop.glare_flag_problem("0.1", None, NAN) == BAD_FLAGS[8][1]
    assert develop.glare_from_flags("0.1", None, None) == dict(strength=0.1)
    assert develop.glare_from_flags("0.5", 3, 0.25) == dict(strength=0.5, levels=3, threshold=0.25)


@pytest.mark.parametrize("flags,message", BAD_FLAGS, ids=lambda v: "_".join(v).strip("-") if isinstance(v, list) else None)
def test_both_front_ends_reject_the_same_flags_in_the_same_words(flags, message, lib):
    project = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    py = subprocess.run([sys.executable, "-m", "pyrite_amd", project] + flags, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", project, "-", "1", os.devnull] + flags, cwd=ROOT, capture_output=True, text=True)
    assert py.returncode == 2 and cpp.returncode == 2, py.stderr + cpp.stderr
    assert py.stderr.strip() == cpp.stderr.strip() == "error: " + message


def test_both_front_ends_parse_the_flags(lib, tmp_path):
    """Well-formed flags get past the parser: what stops the run here is the missing GPU (or nothing, on a GPU box)."""
    project = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    for flags in (["--glare"], ["--glare", "0.3", "--glare-levels", "4", "--glare-threshold", "0.5", "--tone", "reinhard"]):
        flags = flags + ["--spp", "2", "--size", "16x16"]
        py = subprocess.run([sys.executable, "-m", "pyrite_amd", project, "-o", str(tmp_path / "a.png")] + flags, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                            capture_output=True, text=True)
        cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", project, "-", "1", str(tmp_path / "b.png")] + flags, cwd=ROOT, capture_output=True, text=True)
        for run in (py, cpp):
            assert "unrecognized" not in run.stderr and "unknown flag" not in run.stderr and "must" not in run.stderr and "needs" not in run.stderr, run.stderr
            assert run.returncode == 0 or "HIP device" in run.stderr, run.stderr


# ------------------------------------------------------------------------------------------------------------------------ the rule itself
def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=f32).view(np.uint32), np.asarray(b, dtype=f32).view(np.uint32))


def impulse(levels):
    image = np.zeros((257, 257, 3), dtype=f32)
    image[128, 128] = f32(1000)
    return image, R.glare(image, strength=0.1, levels=levels)


def test_level_sizes():
    assert R.level_sizes(1920, 1080, 6) == [(1920, 1080), (960, 540), (480, 270), (240, 135), (120, 68), (60, 34), (30, 17)]
    assert R.level_sizes(1, 5, 12) == [(1, 5), (1, 3), (1, 2), (1, 1)] and R.level_sizes(1, 1, 6) == [(1, 1)]
    assert len(R.level_sizes(1920, 1080, 12)) - 1 == 11


def test_a_single_pixel_comes_back_bit_for_bit():
    for pixel in ([0.25, 7.0, 1e30], [np.nan, 1.0, 2.0], [0.0, -0.0, 5.0]):
        image = np.array([[pixel]], dtype=f32)
        for params in (dict(), dict(strength=1.0, levels=12, threshold=0.5, falloff=2.0)):
            assert same_bits(R.glare(image, **params), image)


@pytest.mark.parametrize("size", [(64, 64), (67, 130), (1, 5), (13, 7)], ids=lambda s: "%dx%d" % s)
def test_a_constant_image_stays_constant(size):
    """Every stage's weights sum to 1, so only rounding moves a constant: 4 ulp bounds the L downs, L ups, the 1/G and the blend of a
    value whose partial sums are exact in the weights' binary fractions more often than not. Observed: 0, 0, 0 and 1 ulp."""
    width, height = size
    for value, params in ((3.7, dict()), (0.3, dict(levels=12, strength=1.0, falloff=2.0))):
        image = np.full((height, width, 3), f32(value), dtype=f32)
        out = R.glare(image, **params)
        ulps = int(np.abs(out.view(np.int32).astype(np.int64) - image.view(np.int32).astype(np.int64)).max())
        print("constant %g at %dx%d %r: %d ulp" % (value, width, height, params, ulps))
        assert ulps <= 4


def test_an_interior_impulse_keeps_its_light():
    image, out = impulse(6)
    before, after = image.astype(np.float64).sum(), out.astype(np.float64).sum()
    print("impulse of 1000 at 257 x 257, 6 levels: sum changes by %.3g relative" % abs(after / before - 1))
    assert abs(after / before - 1) <= 1e-5
    assert (out >= 0).all()


def test_the_impulse_response_falls_with_distance_and_reaches_as_far_as_its_levels():
    image, six = impulse(6)
    row = six[128, 128:, 0]
    print("impulse response at r = 1, 2, 4, 8, 16, 32: " + ", ".join("%.4g" % row[r] for r in (1, 2, 4, 8, 16, 32)))
    assert (np.diff(row[1:].astype(np.float64)) <= 0).all()  # from r = 1 outward it does not increase
    assert row[32] > 0
    _, three = impulse(3)
    assert three[128, 128 + 32, 0] == 0 and three[128, 128 + 4, 0] > 0
    assert six[128, 128, 0] < 1000 and same_bits(six[..., 0], six[..., 1])


def test_nothing_is_negative_for_an_image_that_is_not():
    rng = np.random.default_rng(3)
    image = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (37, 41, 3))).astype(f32)
    image[rng.random((37, 41)) < 0.2] = 0
    for params in (dict(), dict(strength=1.0, levels=12), dict(threshold=2.0, falloff=0.5), dict(strength=1.0, threshold=5.0, levels=3)):
        assert (R.glare(image, **params) >= 0).all(), params


def test_a_pixel_that_is_not_finite_keeps_its_bits_and_adds_nothing():
    rng = np.random.default_rng(4)
    image = rng.uniform(0, 4, (21, 34, 3)).astype(f32)
    zeroed = image.copy()
    holes = {(5, 7): [np.nan, 1.0, 2.0], (0, 0): [1.0, np.inf, 2.0], (20, 33): [-np.inf, 0.5, 0.5], (11, 12): [np.nan, np.nan, np.nan]}
    for at, value in holes.items():
        image[at], zeroed[at] = value, 0
    for params in (dict(), dict(levels=12, threshold=1.0, strength=1.0)):
        out, want = R.glare(image, **params), R.glare(zeroed, **params)
        for at in holes:
            assert same_bits(out[at], image[at])
            out[at] = want[at]
        assert same_bits(out, want)


def test_a_threshold_above_the_image_changes_nothing_where_nothing_arrives():
    rng = np.random.default_rng(5)
    image = rng.uniform(0, 4, (21, 34, 3)).astype(f32)
    luminance = (R.LUMA[0] * image[..., 0] + R.LUMA[1] * image[..., 1]) + R.LUMA[2] * image[..., 2]
    out = R.glare(image, threshold=float(luminance.max()) * 1.01, strength=1.0)
    B = R.blurred(image, threshold=float(luminance.max()) * 1.01)
    assert (B == 0).all() and same_bits(out, image)
    image[10, 17] = f32(50)  # one pixel above the threshold: the bits stay wherever its light does not reach
    out, B = R.glare(image, threshold=8.0, levels=2), R.blurred(image, threshold=8.0, levels=2)
    untouched = (B == 0).all(axis=-1)
    assert untouched.any() and not untouched.all()
    assert same_bits(out[untouched], image[untouched]) and not same_bits(out[~untouched], image[~untouched])


def test_levels_above_what_the_image_has_count_as_all_it_has():
    rng = np.random.default_rng(6)
    image = rng.uniform(0, 4, (13, 7, 3)).astype(f32)  # 13 rows, 7 columns: 7 x 13 -> 4 x 7 -> 2 x 4 -> 1 x 2 -> 1 x 1
    assert len(R.level_sizes(7, 13, 12)) - 1 == 4
    assert same_bits(R.glare(image, levels=12), R.glare(image, levels=4)) and same_bits(R.glare(image, levels=5, falloff=2.0), R.glare(image, levels=4, falloff=2.0))
    assert not same_bits(R.glare(image, levels=3), R.glare(image, levels=4))


def test_the_weights_are_f32_and_summed_from_the_left():
    g, inv = R.weights(4, 0.3)
    assert [type(v) for v in g[1:]] == [f32] * 4 and g[1] == 1 and g[3] == f32(f32(f32(1) * f32(0.3)) * f32(0.3))
    assert inv == f32(1) / f32(f32(f32(g[1] + g[2]) + g[3]) + g[4])
