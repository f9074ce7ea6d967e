"""The guided upsampling without a GPU (include/pyrite_gpu.h "upsample"): the new names of the ABI in the
header, abi.py and the library, every argument check before a device is looked for, the C++ wrappers through a stand-alone program,
the flags of the two command lines, and the numpy restatement (tests/upsample_restatement.py, which tests/test_gpu_upsample.py holds
the kernel against) on properties of the rule itself."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import upsample_restatement as R
from pyrite_amd import abi, develop
from pyrite_amd import build as gpu_build
from pyrite_amd.features import RECORD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pyrite_gpu.h")
f32 = np.float32
IMAGE_ENTRIES = ["pyr_image_upsample", "pyr_image_upsample_device"]
NEW_ENTRIES = IMAGE_ENTRIES + ["pyr_session_upsampled"]
NAN, INF = float("nan"), float("inf")


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
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "%s"' % HEADER, "int main(void){", 'printf("size %zu\\n", sizeof(PyrUpsampleParams));']
    for field, _ in abi.PyrUpsampleParams._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(PyrUpsampleParams, %s));' % (field, field))
    lines += ['printf("floats %.9g %.9g %.9g %.9g\\n", (double)PYR_UPSAMPLE_SIGMA_NORMAL, (double)PYR_UPSAMPLE_SIGMA_DEPTH, (double)PYR_UPSAMPLE_ALBEDO_FLOOR, (double)PYR_UPSAMPLE_MAX_GAIN);',
              'printf("ints %u %u %u %u\\n", PYR_UPSAMPLE_RADIUS, PYR_UPSAMPLE_MOST_RADIUS, PYR_UPSAMPLE_MOST_SCALE, PYR_UPSAMPLE_MATCH_MATERIAL);',
              'printf("sigmas %d\\n", PYR_UPSAMPLE_SIGMA_NORMAL == PYR_DENOISE_SIGMA_NORMAL && PYR_UPSAMPLE_SIGMA_DEPTH == PYR_DENOISE_SIGMA_DEPTH);', "return 0;}"]
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines))
    subprocess.check_call(["gcc", "-o", exe, src])
    seen = dict(line.split(None, 1) for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(seen["size"]) == C.sizeof(abi.PyrUpsampleParams) == 32
    for field, _ in abi.PyrUpsampleParams._fields_:
        assert int(seen[field]) == getattr(abi.PyrUpsampleParams, field).offset, field
    assert [f32(float(v)) for v in seen["floats"].split()] == [f32(abi.PYR_UPSAMPLE_SIGMA_NORMAL), f32(abi.PYR_UPSAMPLE_SIGMA_DEPTH), f32(abi.PYR_UPSAMPLE_ALBEDO_FLOOR),
                                                               f32(abi.PYR_UPSAMPLE_MAX_GAIN)]
    assert [int(v) for v in seen["ints"].split()] == [abi.PYR_UPSAMPLE_RADIUS, abi.PYR_UPSAMPLE_MOST_RADIUS, abi.PYR_UPSAMPLE_MOST_SCALE, abi.PYR_UPSAMPLE_MATCH_MATERIAL] == [1, 3, 8, 1]
    assert (R.MOST_RADIUS, R.MOST_SCALE, R.MATCH_MATERIAL) == (3, 8, 1) and seen["sigmas"] == "1"
    assert "#define PYR_ABI_VERSION 5\n" in header and abi.PYR_ABI_VERSION == 5 and lib.pyr_abi_version() == 5  # additions only


def test_the_python_defaults_are_the_header_s():
    p = develop.upsample_params()
    assert (p.radius, p.flags, f32(p.sigma_normal), f32(p.sigma_depth), f32(p.albedo_floor), f32(p.max_gain), list(p.reserved)) == (
        1, abi.PYR_UPSAMPLE_MATCH_MATERIAL, f32(0.1), f32(0.02), f32(0.01), f32(4.0), [0, 0])
    assert develop.upsample_params(match_material=False).flags == 0 and develop.upsample_params(flags=6).flags == 6 and develop.upsample_params(radius=3).radius == 3
    defaults = {k: v.default for k, v in inspect.signature(R.upsample).parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(albedo=None, pixels=None, low_albedo=None, low_pixels=None, radius=1, flags=1, sigma_normal=0.1, sigma_depth=0.02, albedo_floor=0.01,
                            max_gain=4.0, paths=False)  # the restatement's too


# ------------------------------------------------------------------------------------------------------------------------ the argument checks
def upsample_call(lib, entry="pyr_image_upsample", missing=(), pairs=("albedo", "records"), params=True, width=4, height=3, scale=2, device=99, misaligned=None, **fields):
    """One call with 4 x 3 low buffers of zeros; `missing` names the pointers passed as NULL beyond those of the pairs left out of
    `pairs`; `misaligned` names a records pointer moved by 8 bytes. Images that are refused for their size get addresses never read."""
    names = ["low", "low_albedo", "low_pixels", "albedo", "pixels", "out"]
    small = width * height <= 12 and scale <= 8
    store = np.zeros(6 * 12 * 64 * 32 + 64, dtype=np.uint8)
    base = (store.ctypes.data + 31) & ~31
    at = {name: (base + k * 12 * 64 * 32) if small else ((k + 1) << 40) for k, name in enumerate(names)}
    if "albedo" not in pairs:
        missing = tuple(missing) + ("low_albedo", "albedo")
    if "records" not in pairs:
        missing = tuple(missing) + ("low_pixels", "pixels")
    if misaligned:
        at[misaligned] += 8
    p = develop.upsample_params()
    for name, value in fields.items():
        if name == "reserved":
            p.reserved[value] = 1
        else:
            setattr(p, name, value)
    ptr = lambda name: None if name in missing else at[name]  # noqa: E731
    args = [ptr("low"), ptr("low_albedo"), ptr("low_pixels"), width, height, scale, ptr("albedo"), ptr("pixels"), C.byref(p) if params else None, ptr("out"), device]
    if entry.endswith("_device"):
        args.append(None)
    rc = getattr(lib, entry)(*args)
    return rc, lib.pyr_last_error().decode()


REFUSED = [
    (dict(missing=("low",)), "low"), (dict(params=False), "params"), (dict(missing=("out",)), "out"),
    (dict(missing=("low_albedo",)), "albedo"), (dict(missing=("albedo",)), "low_albedo"), (dict(missing=("low_pixels",)), "pixels"), (dict(missing=("pixels",)), "low_pixels"),
    (dict(width=0), "low_width"), (dict(height=0), "low_height"),
    (dict(scale=0), "scale"), (dict(scale=1), "scale"), (dict(scale=9), "scale"), (dict(scale=0xFFFFFFFF), "scale"),
    (dict(radius=0), "radius"), (dict(radius=4), "radius"), (dict(radius=0xFFFFFFFF), "radius"),
    (dict(flags=2), "flags"), (dict(flags=3), "flags"), (dict(flags=0x80000000), "flags"),
    (dict(albedo_floor=0.0), "albedo_floor"), (dict(albedo_floor=-1.0), "albedo_floor"), (dict(albedo_floor=NAN), "albedo_floor"),
    (dict(max_gain=0.5), "max_gain"), (dict(max_gain=-INF), "max_gain"), (dict(max_gain=NAN), "max_gain"),
    (dict(reserved=0), "reserved"), (dict(reserved=1), "reserved"),
]


def names_in(message):
    return message.replace("params->", " ").replace(":", " ").replace(",", " ").split()


@pytest.mark.parametrize("entry", IMAGE_ENTRIES)
@pytest.mark.parametrize("change,name", REFUSED)
def test_the_upsample_refuses_bad_arguments_by_name_before_a_device_is_looked_for(change, name, entry, lib):
    rc, message = upsample_call(lib, entry=entry, **change)  # no device 99: the argument is still what is reported
    assert rc == abi.PYR_ERR_INVALID_ARGUMENT
    assert name in names_in(message), message


@pytest.mark.parametrize("entry", IMAGE_ENTRIES)
def test_the_floor_and_the_gain_are_read_only_with_the_albedo_pair(entry, lib):
    for fields in (dict(albedo_floor=0.0), dict(max_gain=NAN)):
        assert upsample_call(lib, entry=entry, pairs=("records",), **fields)[0] == abi.PYR_ERR_DEVICE
        assert upsample_call(lib, entry=entry, pairs=(), **fields)[0] == abi.PYR_ERR_DEVICE


def test_the_device_form_refuses_records_that_are_not_aligned(lib):
    for name in ("low_pixels", "pixels"):
        rc, message = upsample_call(lib, entry="pyr_image_upsample_device", misaligned=name)
        assert rc == abi.PYR_ERR_INVALID_ARGUMENT and "16-byte aligned" in message and "pixels_device" in message, message
        assert upsample_call(lib, entry="pyr_image_upsample", misaligned=name)[0] == abi.PYR_ERR_DEVICE  # host buffers are copied: no such rule
    assert upsample_call(lib, entry="pyr_image_upsample_device", misaligned="pixels", radius=0)[1].startswith("params->radius")  # what both entries refuse comes first


@pytest.mark.parametrize("entry", IMAGE_ENTRIES)
def test_size_then_device(entry, lib):
    rc, message = upsample_call(lib, entry=entry, width=32768, height=32768, scale=2)  # 2^32 pixels
    assert rc == abi.PYR_ERR_UNSUPPORTED and "2^32" in message
    rc, message = upsample_call(lib, entry=entry, width=(1 << 23) + 1, height=1, scale=2)  # a side the f32 coordinates do not count
    assert rc == abi.PYR_ERR_UNSUPPORTED and "2^24" in message
    assert upsample_call(lib, entry=entry, width=32768, height=32768, scale=9)[0] == abi.PYR_ERR_INVALID_ARGUMENT  # the scale before the size
    assert upsample_call(lib, entry=entry, width=32768, height=32768, radius=4)[0] == abi.PYR_ERR_INVALID_ARGUMENT  # a parameter too
    assert upsample_call(lib, entry=entry)[0] == abi.PYR_ERR_DEVICE
    for pairs in ((), ("albedo",), ("records",)):
        assert upsample_call(lib, entry=entry, pairs=pairs)[0] == abi.PYR_ERR_DEVICE
    assert upsample_call(lib, entry=entry, scale=8, radius=3, flags=0, sigma_normal=-1.0, sigma_depth=NAN, albedo_floor=1e-30, max_gain=1.0)[0] == abi.PYR_ERR_DEVICE  # the edges are inside
    assert upsample_call(lib, entry=entry, width=1, height=1, max_gain=INF)[0] == abi.PYR_ERR_DEVICE
    if lib.pyr_device_count() <= 0:  # valid arguments where there is no GPU
        assert upsample_call(lib, entry=entry, device=0)[0] == abi.PYR_ERR_DEVICE


def test_the_session_entry_names_what_is_missing(lib):
    p, d, out = develop.upsample_params(), abi.PyrDevelopParams(), np.zeros(3, dtype=f32)
    session = C.c_void_p(1)  # never read: every check below comes before the session is looked at
    call = lambda s, scale, dev, up, o: lib.pyr_session_upsampled(s, scale, dev, None, None, up, o)  # noqa: E731
    for args, name in (((None, 2, C.byref(d), C.byref(p), out.ctypes.data), "session"), ((session, 2, None, C.byref(p), out.ctypes.data), "develop_params"),
                       ((session, 2, C.byref(d), C.byref(p), None), "out"), ((session, 2, C.byref(d), None, out.ctypes.data), "upsample_params")):
        assert call(*args) == abi.PYR_ERR_INVALID_ARGUMENT
        assert lib.pyr_last_error().decode().split()[-1] == name
    for scale in (0, 1, 9):
        assert call(session, scale, C.byref(d), C.byref(p), out.ctypes.data) == abi.PYR_ERR_INVALID_ARGUMENT and "scale" in lib.pyr_last_error().decode()
    p.radius = 4
    assert call(session, 2, C.byref(d), C.byref(p), out.ctypes.data) == abi.PYR_ERR_INVALID_ARGUMENT
    assert lib.pyr_last_error().decode().startswith("upsample_params->radius")


def test_the_python_wrapper_checks_its_images(lib):
    low = np.zeros((3, 4, 3), dtype=f32)
    with pytest.raises(AssertionError):
        develop.upsample(np.zeros((3, 4), dtype=f32), 2, device=99)
    with pytest.raises(TypeError):
        develop.upsample(low, 2, strength=0.5, device=99)
    with pytest.raises(ValueError):
        develop.upsample(low, 2, albedo=np.zeros((6, 8, 3), dtype=f32), device=99)
    with pytest.raises(ValueError):
        develop.upsample(low, 2, low_pixels=np.zeros((3, 4), dtype=RECORD), device=99)
    with pytest.raises(AssertionError):
        develop.upsample(low, 2, albedo=np.zeros((3, 4, 3), dtype=f32), low_albedo=low, device=99)  # the full-size albedo has the low size
    with pytest.raises(AssertionError):
        develop.upsample(low, 2, pixels=np.zeros((3, 4), dtype=RECORD), low_pixels=np.zeros((3, 4), dtype=RECORD), device=99)
    for scale, name in ((1, "scale"), (9, "scale")):
        with pytest.raises(Exception) as refused:
            develop.upsample(low, scale, device=99)
        assert name in str(refused.value)
    with pytest.raises(Exception) as refused:  # good arguments reach the library, which finds no device 99
        develop.upsample(low, 2, albedo=np.zeros((6, 8, 3), dtype=f32), pixels=np.zeros((6, 8), dtype=RECORD), low_albedo=low, low_pixels=np.zeros((3, 4), dtype=RECORD),
                         radius=2, match_material=False, device=99)
    assert not isinstance(refused.value, (AssertionError, ValueError, TypeError))


# ------------------------------------------------------------------------------------------------------------------------ the C++ wrappers
def test_the_cpp_wrappers(lib, tmp_path):
    """pyrite::upsample, upsample_params, upsample_flag_problem and upsample_from_flags from a stand-alone program
    (tests/upsample_driver.cpp) linked against libpyrite_host.so: the ProjectError for a buffer of the wrong size or half a pair, the
    GpuError and its status for a scale or a parameter out of range, and with good arguments PYR_ERR_DEVICE here -- or, where there is
    a GPU, a constant image that stays constant."""
    exe = str(tmp_path / "upsample_driver")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "upsample_driver.cpp"), "-L" + gpu_build.HOST_DIR, "-lpyrite_host", "-L" + gpu_build.CSRC, "-lpyrite_gpu",
                           "-Wl,-rpath," + gpu_build.HOST_DIR, "-Wl,-rpath," + gpu_build.CSRC])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-2000:]
    assert run.stdout.split()[0] == "ok"


# ------------------------------------------------------------------------------------------------------------------------ the flags
PROJECT = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
BAD_FLAGS = [
    (["--upsample-radius", "2"], "--upsample-radius needs --upsample"),
    (["--upsample", "1"], "--upsample must be 2 to 8"),
    (["--upsample", "9"], "--upsample must be 2 to 8"),
    (["--upsample", "2", "--upsample-radius", "0"], "--upsample-radius must be 1 to 3"),
    (["--upsample", "2", "--upsample-radius", "4"], "--upsample-radius must be 1 to 3"),
    (["--upsample", "3", "--size", "32x32"], "--upsample 3 does not divide the image size 32x32"),  # both numbers, before anything renders
    (["--upsample", "4", "--size", "32x30"], "--upsample 4 does not divide the image size 32x30"),
    (["--upsample", "5", "--size", "30x32"], "--upsample 5 does not divide the image size 30x32"),
]


def test_flag_rules():
    assert develop.upsample_flag_problem(None, None) is None and develop.upsample_from_flags(None, None) is None
    assert develop.upsample_flag_problem(2, None) is None and develop.upsample_flag_problem(8, 3, (64, 8)) is None
    assert develop.upsample_flag_problem(None, 2) == BAD_FLAGS[0][1] and develop.upsample_flag_problem(1, None) == BAD_FLAGS[1][1]
    assert develop.upsample_flag_problem(2, 0) == BAD_FLAGS[3][1] and develop.upsample_flag_problem(3, None, (32, 32)) == BAD_FLAGS[5][1]
    assert develop.upsample_from_flags(2, None) == {} and develop.upsample_from_flags(4, 3) == dict(radius=3)


@pytest.mark.parametrize("flags,message", BAD_FLAGS, ids=lambda v: "_".join(v).strip("-") if isinstance(v, list) else None)
def test_both_front_ends_reject_the_same_flags_in_the_same_words(flags, message, lib):
    py = subprocess.run([sys.executable, "-m", "pyrite_amd", PROJECT] + flags, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", PROJECT, "-", "1", os.devnull] + flags, cwd=ROOT, capture_output=True, text=True)
    assert py.returncode == 2 and cpp.returncode == 2, py.stderr + cpp.stderr
    assert py.stderr.strip() == cpp.stderr.strip() == "error: " + message
    assert "Rendering" not in py.stdout + cpp.stdout and "The scene contains" not in py.stdout + cpp.stdout  # before anything renders


def test_both_front_ends_parse_the_flags(lib, tmp_path):
    """Well-formed flags get past the parser: what stops the run here is the missing GPU (or nothing, on a GPU box)."""
    for flags in (["--upsample", "2"], ["--upsample", "4", "--upsample-radius", "2", "--glare", "--tone", "reinhard"]):
        flags = flags + ["--spp", "2", "--size", "16x16"]
        py = subprocess.run([sys.executable, "-m", "pyrite_amd", PROJECT, "-o", str(tmp_path / "a.png")] + flags, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                            capture_output=True, text=True)
        cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", PROJECT, "-", "1", str(tmp_path / "b.png")] + flags, cwd=ROOT, capture_output=True, text=True)
        for run in (py, cpp):
            assert "unrecognized" not in run.stderr and "unknown flag" not in run.stderr and "must" not in run.stderr and "needs" not in run.stderr and "divide" not in run.stderr, run.stderr
            assert run.returncode == 0 or "HIP device" in run.stderr, run.stderr


# ------------------------------------------------------------------------------------------------------------------------ the rule itself
def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=f32).view(np.uint32), np.asarray(b, dtype=f32).view(np.uint32))


def ulps(a, b):
    return int(np.abs(np.asarray(a, dtype=f32).view(np.int32).astype(np.int64) - np.asarray(b, dtype=f32).view(np.int32).astype(np.int64)).max())


def records(height, width, normal=(0.0, 0.0, 1.0), depth=2.0, material=3):
    out = np.zeros((height, width), dtype=RECORD)
    out["normal"], out["depth"], out["coverage"], out["material"] = normal, depth, 1.0, material
    return out


def bilinear(low, scale):
    """Bilinear interpolation written directly, for the pixels whose four neighbours are inside: the four products summed in raster
    order over the sum of the four weights, in f32."""
    h, w, _ = low.shape
    out = np.full((h * scale, w * scale, 3), np.nan, dtype=f32)
    for Y in range(h * scale):
        ly = (f32(Y) + f32(0.5)) / f32(scale) - f32(0.5)
        y0 = int(np.floor(ly))
        for X in range(w * scale):
            lx = (f32(X) + f32(0.5)) / f32(scale) - f32(0.5)
            x0 = int(np.floor(lx))
            if x0 < 0 or y0 < 0 or x0 + 1 >= w or y0 + 1 >= h:
                continue
            total, acc = f32(0), np.zeros(3, dtype=f32)
            for qy in (y0, y0 + 1):
                wy = f32(1) - abs(f32(qy) - ly)
                for qx in (x0, x0 + 1):
                    wx = f32(1) - abs(f32(qx) - lx)
                    weight = f32(wy * wx)
                    if weight == 0:
                        continue
                    total = f32(total + weight)
                    acc = (acc + weight * low[qy, qx]).astype(f32)
            out[Y, X] = acc / total
    return out


@pytest.mark.parametrize("scale", [2, 3, 4, 8])
def test_without_pairs_and_radius_1_the_interior_is_bilinear(scale):
    rng = np.random.default_rng(scale)
    low = rng.uniform(0, 4, (5, 7, 3)).astype(f32)
    out, want = R.upsample(low, scale), bilinear(low, scale)
    interior = np.isfinite(want).all(axis=-1)
    assert interior.sum() == (4 * scale) * (6 * scale)
    assert same_bits(out[interior], want[interior])
    assert np.isfinite(out).all() and out.min() >= low.min() * (1 - 1e-6) and out.max() <= low.max() * (1 + 1e-6)  # the edges are clamped by renormalisation: convex up to rounding
    assert ulps(out[0, 0], low[0, 0]) <= 1  # one tap: w * v / w


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("scale", [2, 3, 4, 8])
def test_a_constant_image_with_constant_guides_stays_constant(scale, radius):
    """Within 2 ulp at the default radius, whatever the scale and the pairs. The sums are f32 and run tap by tap, so the distance
    grows with the number of taps n = (2 radius)^2: W_ is off by at most (n - 1) u relative (u = 2^-24, non-negative terms), A by n u
    (a product more), the quotient adds one, and an ulp of 3.7 is 1.08 u of it: at most (2 n) / 1.08 ulp -- 30 at radius 2, 67 at
    radius 3, the bounds held here. Seen: 0 to 2 ulp at radius 1, up to 3 at radius 2 and 5 at radius 3."""
    value = f32(3.7)
    low = np.full((4, 5, 3), value, dtype=f32)
    guides = dict(pixels=records(4 * scale, 5 * scale), low_pixels=records(4, 5))
    albedos = dict(albedo=np.full((4 * scale, 5 * scale, 3), f32(0.5)), low_albedo=np.full((4, 5, 3), f32(0.5)))
    assert f32(f32(0.5) + f32(0.01)) * (f32(1) / f32(f32(0.5) + f32(0.01))) == 1  # the gain of these albedos is exactly 1
    taps = (2 * radius) ** 2
    bound = 2 if radius == 1 else int(2 * taps / 1.08)
    for name, pairs in (("no pair", {}), ("records", guides), ("both pairs", dict(guides, **albedos))):
        out = R.upsample(low, scale, radius=radius, **pairs)
        distance = ulps(out, np.full_like(out, value))
        print("constant, scale %d radius %d, %s: %d ulp (bound %d)" % (scale, radius, name, distance, bound))
        assert distance <= bound


STEP_GUIDES = {
    "normals": lambda r, right: r["normal"].__setitem__(right, (1.0, 0.0, 0.0)),
    "depths": lambda r, right: r["depth"].__setitem__(right, 3.0),
    "materials": lambda r, right: r["material"].__setitem__(right, 9),
}


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("guide", sorted(STEP_GUIDES))
@pytest.mark.parametrize("scale", [2, 3, 4])
def test_a_step_comes_back_two_valued_under_a_guide_that_steps_with_it(scale, guide, radius):
    h, w, column = 6, 8, 3  # low columns 0..2 hold 1, 3..7 hold 5
    low = np.full((h, w, 3), f32(1), dtype=f32)
    low[:, column:] = f32(5)
    low_r, high_r = records(h, w), records(h * scale, w * scale)
    STEP_GUIDES[guide](low_r, (slice(None), slice(column, None)))
    STEP_GUIDES[guide](high_r, (slice(None), slice(column * scale, None)))
    out = R.upsample(low, scale, radius=radius, pixels=high_r, low_pixels=low_r)
    left, right = out[:, :column * scale], out[:, column * scale:]
    assert ulps(left, np.full_like(left, f32(1))) <= 2 and ulps(right, np.full_like(right, f32(5))) <= 2
    plain = R.upsample(low, scale, radius=radius)
    between = (plain > f32(1.001)) & (plain < f32(4.999))
    assert between.any(), "without the records pair the step is blurred"


def test_demodulation_brings_a_checkerboard_back():
    """low = E * low_albedo with a smooth E, the full-size albedo a one-pixel checkerboard whose 2 x 2 block means are low_albedo. With
    f the floor, a tap's value is E(q) * a_low * (a + f) / (a_low + f); the taps' E(q) are within the variation of E over the tent,
    delta, of E(P), so the output lies within  E * (a + f) * [a_low / (a_low + f)] * (1 +- delta)  of E * (a + f): the relative
    bound is  f / (a_low + f) + delta  (+ rounding, 1e-5). No gain reaches max_gain: (0.8 + f) / (0.5 + f) < 4."""
    scale, h, w, floor = 2, 12, 16, 0.01
    a_low = f32(0.5)
    ys, xs = np.mgrid[0:h, 0:w].astype(f32)
    E = (f32(2) + f32(0.02) * xs + f32(0.01) * ys).astype(f32)  # smooth: 1 % a low pixel at the most
    low_albedo = np.full((h, w, 3), a_low, dtype=f32)
    low = (E[..., None] * low_albedo).astype(f32)
    Y, X = np.mgrid[0:h * scale, 0:w * scale]
    albedo = np.where((X + Y) % 2 == 0, f32(0.8), f32(0.2)).astype(f32)[..., None].repeat(3, axis=-1)
    assert np.allclose(albedo.reshape(h, scale, w, scale, 3).mean(axis=(1, 3)), low_albedo)
    out = R.upsample(low, scale, albedo=albedo, low_albedo=low_albedo, albedo_floor=floor)
    E_high = np.repeat(np.repeat(E, scale, axis=0), scale, axis=1)[..., None]
    want = E_high * (albedo + f32(floor))
    delta = 0.02 * 1.0 / 2.0 + 0.01 * 1.0 / 2.0  # E moves by 0.03 over the one low pixel a radius-1 tent reaches, against E >= 2
    bound = floor / (float(a_low) + floor) + delta + 1e-5
    worst = float(np.abs(out / want - 1).max())
    print("checkerboard: worst relative distance from E * (albedo + floor) %.4f, bound %.4f" % (worst, bound))
    assert worst <= bound
    contrast = lambda image: float(np.abs(image[:, 1:] - image[:, :-1]).mean() / image.mean())  # noqa: E731
    plain = R.upsample(low, scale)
    print("checkerboard: contrast between neighbours %.3f demodulated, %.4f not" % (contrast(out), contrast(plain)))
    assert contrast(out) > 0.5 and contrast(plain) < 0.02  # (0.81 - 0.21) / 0.51 against a smooth ramp


def test_a_pixel_every_guide_rejects_is_the_raw_tent():
    h, w, scale = 4, 5, 2
    rng = np.random.default_rng(7)
    low = rng.uniform(0.5, 4, (h, w, 3)).astype(f32)
    low_r, high_r = records(h, w, material=3), records(h * scale, w * scale, material=3)
    alone = [(2, 3), (5, 4), (0, 0), (7, 9)]
    for at in alone:
        high_r["material"][at] = 77  # no low pixel has it
    low_albedo = np.full((h, w, 3), f32(0.5), dtype=f32)
    albedo = np.full((h * scale, w * scale, 3), f32(0.5), dtype=f32)
    low_albedo[1, 1] = 0  # under (2, 3): its division is 1 / floor, the gain clamped
    albedo[2, 3] = 1
    for radius in (1, 2, 3):
        out, guided, _ = R.upsample(low, scale, radius=radius, pixels=high_r, low_pixels=low_r, albedo=albedo, low_albedo=low_albedo, paths=True)
        tent = R.upsample(low, scale, radius=radius)
        for at in alone:
            assert not guided[at] and same_bits(out[at], tent[at]) and np.isfinite(out[at]).all()
        assert guided.sum() == guided.size - len(alone) and np.isfinite(out).all()
        assert out.max() <= 4 * 4.0 * 1.0001  # no pixel explodes: max_gain times the largest low value
    flagless = R.upsample(low, scale, pixels=high_r, low_pixels=low_r, flags=0)  # without the flag the material is not read at all
    assert same_bits(flagless, R.upsample(low, scale, pixels=records(h * scale, w * scale), low_pixels=low_r, flags=0))


def test_a_nan_tap_of_weight_0_leaves_its_neighbours_finite():
    h, w, scale = 5, 6, 2
    low = np.full((h, w, 3), f32(2), dtype=f32)
    low[2, 3] = (np.nan, np.inf, -np.inf)
    low_r, high_r = records(h, w), records(h * scale, w * scale)
    low_r["material"][2, 3] = 50  # a surface of its own: no full-size pixel but its own four sees it
    high_r["material"][4:6, 6:8] = 50
    for radius in (1, 2, 3):
        out = R.upsample(low, scale, radius=radius, pixels=high_r, low_pixels=low_r)
        bad = ~np.isfinite(out).all(axis=-1)
        assert bad[4:6, 6:8].all() and bad.sum() == 4, "only the pixels that own the tap are lost"
        assert ulps(out[~bad], np.full_like(out[~bad], f32(2))) <= 2
        plain = ~np.isfinite(R.upsample(low, scale, radius=radius)).all(axis=-1)
        assert plain.sum() > 4  # without the guide it leaks into every pixel whose tent reaches it
    nan_depth = records(h, w)
    nan_depth["depth"][1, 1] = np.nan  # a NaN term makes the weight 0 explicitly: fmaxf alone would have ignored it
    low2 = np.full((h, w, 3), f32(2), dtype=f32)
    low2[1, 1] = 1000
    out = R.upsample(low2, scale, pixels=records(h * scale, w * scale), low_pixels=nan_depth, flags=0)
    assert ulps(out, np.full_like(out, f32(2))) <= 2, "the tap whose depth is a NaN weighs nothing"
    assert np.isfinite(out[2:4, 2:4]).all()  # the pixels inside low pixel (1, 1) live on their other taps


def test_no_albedo_makes_a_gain_below_0_or_above_max_gain():
    """A developed albedo can be negative (a saturated colour lies outside linear sRGB) or, in a broken input, a NaN: both count as 0,
    so that low_albedo + floor never crosses 0. Then 0 <= k <= max_gain, and the output of a positive image lies within
    [0, max_gain * its largest value] (times 1 + 1e-6 for the sums' rounding)."""
    h, w, scale, floor = 5, 6, 2, 0.01
    rng = np.random.default_rng(9)
    low = rng.uniform(0.5, 4, (h, w, 3)).astype(f32)
    low_albedo = rng.uniform(0, 1, (h, w, 3)).astype(f32)
    albedo = rng.uniform(0, 1, (h * scale, w * scale, 3)).astype(f32)
    for value in (-floor, -floor * (1 + 1e-6), -floor * (1 - 1e-6), -0.5, np.nan, -np.inf):
        low_albedo.reshape(-1)[rng.integers(0, low_albedo.size, 4)] = value
        albedo.reshape(-1)[rng.integers(0, albedo.size, 8)] = value
    for radius in (1, 2, 3):
        out = R.upsample(low, scale, radius=radius, albedo=albedo, low_albedo=low_albedo, albedo_floor=floor)
        assert np.isfinite(out).all() and out.min() >= 0 and out.max() <= 4.0 * float(low.max()) * (1 + 1e-6)
    cleaned = R.upsample(low, scale, albedo=np.fmax(albedo, f32(0)), low_albedo=np.fmax(low_albedo, f32(0)), albedo_floor=floor)
    assert same_bits(R.upsample(low, scale, albedo=albedo, low_albedo=low_albedo, albedo_floor=floor), cleaned)
