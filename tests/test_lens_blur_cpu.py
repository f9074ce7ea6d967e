"""Lens blur over the feature records without a GPU (include/pyrite_gpu.h "lens blur over the feature records", DESIGN.md section
9o): the new names of the ABI in the header, abi.py and the library, every argument check before a device is looked for, the C++
wrappers through a stand-alone program, the figures of the kernel's build, and the numpy restatement
(tests/lens_blur_restatement.py, which tests/test_gpu_lens_blur.py holds the kernel against) on properties of the rule itself."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import closed_forms as forms
import lens_blur_restatement as R
from pyrite_amd import abi, develop, features
from pyrite_amd import build as gpu_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pyrite_gpu.h")
f32 = np.float32
U = 2.0 ** -24  # half an ulp of 1: the relative error of one f32 rounding
NEW_ENTRIES = ["pyr_image_lens_blur", "pyr_image_lens_blur_device", "pyr_session_lens_blurred"]


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
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "%s"' % HEADER, "int main(void){", 'printf("size %zu\\n", sizeof(PyrLensBlurParams));']
    for field, _ in abi.PyrLensBlurParams._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(PyrLensBlurParams, %s));' % (field, field))
    lines += ['printf("tolerance_default %.9g\\n", (double)PYR_REPROJECT_DEPTH_TOLERANCE);', 'printf("ints %u %u\\n", PYR_LENS_BLUR_MAX_RADIUS, PYR_LENS_BLUR_MOST_RADIUS);',
              "return 0;}"]
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines))
    subprocess.check_call(["gcc", "-o", exe, src])
    seen = dict(line.split(None, 1) for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(seen["size"]) == C.sizeof(abi.PyrLensBlurParams) == 32
    for field, _ in abi.PyrLensBlurParams._fields_:
        assert int(seen[field]) == getattr(abi.PyrLensBlurParams, field).offset, field
    assert [int(v) for v in seen["ints"].split()] == [abi.PYR_LENS_BLUR_MAX_RADIUS, abi.PYR_LENS_BLUR_MOST_RADIUS] == [8, 16]
    defaults = develop.lens_blur_params(focus_distance=2.0, aperture=0.5, view_plane=3.0)
    assert (defaults.focus_distance, defaults.aperture, defaults.view_plane, defaults.max_radius) == (2.0, 0.5, 3.0, 8) and not any(defaults.reserved)
    assert f32(defaults.depth_tolerance) == f32(float(seen["tolerance_default"])) == f32(abi.PYR_REPROJECT_DEPTH_TOLERANCE)
    assert R.RECORD == features.RECORD and R.RECORD.itemsize == C.sizeof(abi.PyrFeaturePixel)
    assert "#define PYR_ABI_VERSION 5\n" in header and abi.PYR_ABI_VERSION == 5 and lib.pyr_abi_version() == 5  # additions only


def test_the_python_parameters_read_a_camera():
    camera = abi.PyrCamera()
    camera.view_plane, camera.focus_distance, camera.aperture = 2.5, 7.0, 0.04
    from pyrite_amd.renderer import Camera

    for given in (camera, Camera(camera)):
        p = develop.lens_blur_params(given, max_radius=5)
        assert (p.view_plane, p.focus_distance, f32(p.aperture), p.max_radius) == (2.5, 7.0, f32(0.04), 5)
    assert develop.lens_blur_params(camera, aperture=0.0).aperture == 0.0 and develop.lens_blur_params(camera, focus_distance=2.0).focus_distance == 2.0
    with pytest.raises(ValueError, match="view_plane"):
        develop.lens_blur_params(focus_distance=1.0, aperture=0.1)
    assert develop.lens_blur_flag_problem(False, None) is None and develop.lens_blur_flag_problem(True, None) is None and develop.lens_blur_flag_problem(True, 16) is None
    assert "needs --lens-blur" in develop.lens_blur_flag_problem(False, 4)
    assert "1 to 16" in develop.lens_blur_flag_problem(True, 0) and "1 to 16" in develop.lens_blur_flag_problem(True, 17)


# ------------------------------------------------------------------------------------------------------------------------ the argument checks
def blur_call(lib, entry="pyr_image_lens_blur", image=True, records=True, params=True, out=True, width=4, height=3, device=99, misalign=False, overlap=None, **fields):
    pixels = np.zeros((3, 4, 3), dtype=f32)
    store = np.zeros(3 * 4 * 32 + 16, dtype=np.uint8)
    start = store.ctypes.data + (-store.ctypes.data) % 16 + (4 if misalign else 0)
    p = abi.PyrLensBlurParams(2.0, 0.01, 2.4, abi.PYR_LENS_BLUR_MAX_RADIUS, abi.PYR_REPROJECT_DEPTH_TOLERANCE)
    for name, value in fields.items():
        if name == "reserved":
            p.reserved[value] = 1
        else:
            setattr(p, name, value)
    result = np.zeros((3, 4, 3), dtype=f32)
    target = {None: result.ctypes.data, "image": pixels.ctypes.data + 12 * 11, "pixels": start + 32 * 11 + 16}[overlap]  # the last pixel of either input
    args = [pixels.ctypes.data if image else None, start if records else None, width, height, C.byref(p) if params else None, target if out else None, device]
    if entry.endswith("_device"):
        args.append(None)
    rc = getattr(lib, entry)(*args)
    return rc, lib.pyr_last_error().decode()


NAN, INF = float("nan"), float("inf")
BLUR_REFUSED = [
    (dict(image=False), "image"), (dict(records=False), "pixels"), (dict(params=False), "params"), (dict(out=False), "out"), (dict(width=0), "width"), (dict(height=0), "height"),
    (dict(focus_distance=0.0), "focus_distance"), (dict(focus_distance=-1.0), "focus_distance"), (dict(focus_distance=NAN), "focus_distance"), (dict(focus_distance=INF), "focus_distance"),
    (dict(aperture=-0.001), "aperture"), (dict(aperture=NAN), "aperture"), (dict(aperture=INF), "aperture"),
    (dict(view_plane=0.0), "view_plane"), (dict(view_plane=-2.0), "view_plane"), (dict(view_plane=NAN), "view_plane"), (dict(view_plane=INF), "view_plane"),
    (dict(max_radius=0), "max_radius"), (dict(max_radius=17), "max_radius"),
    (dict(depth_tolerance=-0.01), "depth_tolerance"), (dict(depth_tolerance=1.0), "depth_tolerance"), (dict(depth_tolerance=NAN), "depth_tolerance"), (dict(depth_tolerance=INF), "depth_tolerance"),
    (dict(reserved=0), "reserved"), (dict(reserved=1), "reserved"), (dict(reserved=2), "reserved"),
]


def names_in(message):
    return message.replace("params->", " ").replace(":", " ").replace(",", " ").split()


@pytest.mark.parametrize("entry", ["pyr_image_lens_blur", "pyr_image_lens_blur_device"])
@pytest.mark.parametrize("change,name", BLUR_REFUSED)
def test_lens_blur_refuses_bad_arguments_by_name_before_a_device_is_looked_for(change, name, entry, lib):
    rc, message = blur_call(lib, entry=entry, **change)  # no device 99: the argument is still what is reported
    assert rc == abi.PYR_ERR_INVALID_ARGUMENT
    assert name in names_in(message), message


def test_the_device_form_refuses_misaligned_records_and_an_overlapping_out(lib):
    rc, message = blur_call(lib, entry="pyr_image_lens_blur_device", misalign=True)
    assert rc == abi.PYR_ERR_INVALID_ARGUMENT and "pixels_device" in message and "16-byte" in message
    for which in ("image", "pixels"):
        rc, message = blur_call(lib, entry="pyr_image_lens_blur_device", overlap=which)
        assert rc == abi.PYR_ERR_INVALID_ARGUMENT and "out_device overlaps %s_device" % which in message, message
    assert blur_call(lib, entry="pyr_image_lens_blur", misalign=True)[0] == abi.PYR_ERR_DEVICE  # host buffers are staged: any alignment


@pytest.mark.parametrize("entry", ["pyr_image_lens_blur", "pyr_image_lens_blur_device"])
def test_lens_blur_size_then_device(entry, lib):
    rc, message = blur_call(lib, entry=entry, width=65536, height=65536)
    assert rc == abi.PYR_ERR_UNSUPPORTED and "2^32" in message
    assert blur_call(lib, entry=entry)[0] == abi.PYR_ERR_DEVICE
    assert blur_call(lib, entry=entry, aperture=0.0, max_radius=16, depth_tolerance=0.0, focus_distance=1e-38)[0] == abi.PYR_ERR_DEVICE  # the edges of the ranges are inside
    assert blur_call(lib, entry=entry, max_radius=1, depth_tolerance=float(np.nextafter(f32(1), f32(0))), view_plane=1e-38, aperture=3e38)[0] == abi.PYR_ERR_DEVICE
    if lib.pyr_device_count() <= 0:  # valid arguments where there is no GPU
        assert blur_call(lib, entry=entry, device=0)[0] == abi.PYR_ERR_DEVICE


def test_the_session_entry_refuses_by_name_before_a_device_is_looked_for(lib):
    stand_in = (C.c_char * 4096)()
    session = C.addressof(stand_in)
    develop_p, out = abi.PyrDevelopParams(), np.zeros(3, dtype=f32)
    fp = abi.PyrFeatureParams(1, 1)
    good = abi.PyrLensBlurParams(2.0, 0.01, 2.4, 8, 0.02)
    call = lib.pyr_session_lens_blurred
    invalid = abi.PYR_ERR_INVALID_ARGUMENT
    assert call(None, None, None, C.byref(good), out.ctypes.data) == invalid and b"session" in lib.pyr_last_error()
    assert call(session, None, C.byref(fp), C.byref(good), out.ctypes.data) == invalid and b"develop_params" in lib.pyr_last_error()
    assert call(session, C.byref(develop_p), None, C.byref(good), out.ctypes.data) == invalid and b"feature_params" in lib.pyr_last_error()
    assert call(session, C.byref(develop_p), C.byref(fp), C.byref(good), None) == invalid and b"out" in lib.pyr_last_error()
    assert call(session, C.byref(develop_p), C.byref(fp), None, out.ctypes.data) == invalid and b"blur_params" in lib.pyr_last_error()
    for field, value in [("focus_distance", 0.0), ("aperture", -1.0), ("view_plane", NAN), ("max_radius", 17), ("depth_tolerance", 1.0)]:
        bad = abi.PyrLensBlurParams(2.0, 0.01, 2.4, 8, 0.02)
        setattr(bad, field, value)
        assert call(session, C.byref(develop_p), C.byref(fp), C.byref(bad), out.ctypes.data) == invalid and ("blur_params->" + field).encode() in lib.pyr_last_error()
    bad = abi.PyrLensBlurParams(2.0, 0.01, 2.4, 8, 0.02)
    bad.reserved[1] = 1
    assert call(session, C.byref(develop_p), C.byref(fp), C.byref(bad), out.ctypes.data) == invalid and b"blur_params->reserved" in lib.pyr_last_error()
    assert call(session, C.byref(develop_p), C.byref(abi.PyrFeatureParams(9, 1)), C.byref(good), out.ctypes.data) == invalid and b"grid" in lib.pyr_last_error()


# ------------------------------------------------------------------------------------------------------------------------ the C++ wrappers
def test_the_cpp_wrappers(lib, tmp_path):
    """pyrite::lens_blur, pyrite::lens_blur_params and pyrite::lens_blur_flag_problem from a stand-alone program
    (tests/lens_blur_driver.cpp) linked against libpyrite_host.so: the ProjectError for buffers of the wrong size, the GpuError and
    its status for a parameter out of range, and with good arguments PYR_ERR_DEVICE here -- or, where there is a GPU, the input's
    bits for an aperture of 0."""
    exe = str(tmp_path / "lens_blur_driver")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "lens_blur_driver.cpp"), "-L" + gpu_build.HOST_DIR, "-lpyrite_host", "-L" + gpu_build.CSRC, "-lpyrite_gpu",
                           "-Wl,-rpath," + gpu_build.HOST_DIR, "-Wl,-rpath," + gpu_build.CSRC])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-2000:]
    assert run.stdout.split()[0] == "ok"


# ------------------------------------------------------------------------------------------------------------------------ the build
@pytest.mark.timeout(600)
def test_the_kernel_needs_no_scratch_and_its_tile_fits_the_lds(tmp_path):
    """kernels/lens_blur.hip cross-compiled for gfx950 with the build's flags: the kernel's descriptor, as tests/test_kernel_isa.py
    reads it."""
    flags = [f for f in gpu_build.FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "lens_blur.s"
    subprocess.check_call([gpu_build.HIPCC] + flags + ["--cuda-device-only", "-S", "kernels/lens_blur.hip", "-o", str(out)], cwd=gpu_build.CSRC, stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = text[text.index(".amdhsa_kernel", text.index("lens_blur_kernel")):]
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1))
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1))
    vgprs = int(re.search(r"; NumVgprs: (\d+)", meta).group(1))
    print("lens_blur_kernel: %d VGPRs, %d B of LDS, %d B of scratch" % (vgprs, lds, scratch))
    assert scratch == 0
    assert 0 < lds <= 64 * 1024
    assert text.count(".amdhsa_kernel") == 1  # one kernel: the figures above are its


# ------------------------------------------------------------------------------------------------------------------------ the rule itself
FAR_PLANE = float(2 ** 20)  # a view plane so far off that 1 + t rounds to 1 at every pixel: z is the record's depth, bit for bit


def records(width, height, depth=2.0, coverage=1.0):
    rec = np.zeros((height, width), dtype=R.RECORD)
    rec["depth"], rec["coverage"] = f32(depth), f32(coverage)
    rec["normal"][..., 2] = 1
    rec["shape"], rec["material"] = 7, 1
    return rec


def aperture_for(A, width, height, focus_distance, view_plane):
    """The aperture whose scale is A pixels per unit of |1 - f/z| (float64; the caller reads the f32 result back from R.scale)."""
    return (A * focus_distance / (view_plane * max(width, height) * 0.5)) ** 2


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=f32).view(np.uint32), np.asarray(b, dtype=f32).view(np.uint32))


def test_no_aperture_and_a_frame_in_focus_return_the_input_s_bits():
    rng = np.random.default_rng(28)
    width, height = 21, 9
    image = rng.random((height, width, 3), dtype=f32)
    image[3, 4], image[0, 0], image[8, 20] = (np.nan, -0.0, np.inf), (-np.inf, 1, 2), (0.5, np.nan, 0.25)
    rec = records(width, height)
    rec["depth"] = rng.uniform(0.5, 20, (height, width)).astype(f32)
    rec["coverage"][rng.random((height, width)) < 0.2] = 0
    rec["depth"][2, 2], rec["depth"][5, 7], rec["depth"][6, 1] = np.nan, np.inf, 0
    for radius in (1, 8, 16):
        assert same_bits(R.lens_blur(image, rec, 3.0, 0.0, 2.4, max_radius=radius), image)
    c, inv, z = R.circles(rec, 3.0, 0.0, 2.4, 16)
    assert not c.any() and (inv == 1).all() and (z[rec["coverage"] == 0] == R.FLT_MAX).all() and z[2, 2] == z[5, 7] == z[6, 1] == R.FLT_MAX
    focused = records(width, height, depth=3.0)  # every record at the focus distance, which under the far view plane is its z
    c, inv, z = R.circles(focused, 3.0, 0.5, FAR_PLANE, 16)
    assert (z == 3).all() and not c.any()
    assert same_bits(R.lens_blur(image, focused, 3.0, 0.5, FAR_PLANE, max_radius=16), image)
    assert not same_bits(R.lens_blur(image, records(width, height, depth=4.0), 3.0, 0.5, FAR_PLANE, max_radius=16), image)  # and out of focus it does blur


def test_the_circle_of_confusion_is_the_thin_lens_s():
    """A camera of tests/closed_forms.py above floors at several heights: the pinhole ray of a pixel's centre and the ray from the
    rim of the lens towards the same point of the focus plane (closed_forms.rays, float64) meet the floor s apart. Seen from the
    lens that is s * f/z on the focus plane, and one unit there is view_plane/f * max(W,H)/2 pixels: c64 = s * view_plane/z * max/2,
    which is sqrt(aperture)*|1 - f/z| * view_plane/f * max(W,H)/2. The record's depth is the pinhole ray's length to the floor.
      The bound, u = 2^-24 per rounding, first order: A takes 4 operations and its three inputs are rounded to f32 (the aperture's
    under the root): <= 7u. px, py: (x - W/2) is exact, / m, 1/m, + : <= 3u each; their squares <= 7u, the sum <= 8u, / (vp*vp, 3u)
    <= 12u on t; 1 + t <= 13u, its root <= 7.5u, the record's depth 1u, the division 1u: z <= 10u. f/z: f's rounding and the division:
    <= 12u, an absolute 12u * f/z on 1 - f/z, which is rounded once more, and the product with A once: |c - c64| <=
    (12 * f/z * A + 9 * c64) u. Taken as (13 * f/z * A + 10 * c64) u for the terms of second order."""
    width, height, f, aperture = 48, 32, 5.0, 0.04
    cam = forms.Camera((0, 0, 5), (0, 0, 0), fov=40, focus_distance=f, aperture=aperture)
    py, px = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    worst = 0.0
    for floor_z in (-3.0, 0.0, 1.0, 2.5, 4.0):
        o, d = forms.rays(cam, width, height, px, py, 0.5, 0.5)
        depth = (floor_z - o[..., 2]) / d[..., 2]
        hit = o + d * depth[..., None]
        lo, ld = forms.rays(cam, width, height, px, py, 0.5, 0.5, lens=(np.sqrt(aperture), 0.0))
        lens_hit = lo + ld * ((floor_z - lo[..., 2]) / ld[..., 2])[..., None]
        s = np.linalg.norm(lens_hit - hit, axis=-1)
        z = 5.0 - floor_z
        c64 = s * cam.view_plane / z * max(width, height) * 0.5
        assert np.allclose(c64, np.sqrt(aperture) * abs(1 - f / z) * cam.view_plane / f * max(width, height) * 0.5, rtol=1e-9, atol=1e-9)  # the issue's form
        rec = records(width, height)
        rec["depth"] = depth.astype(f32)
        c, inv, z32 = R.circles(rec, f, aperture, cam.view_plane, 16)
        A = float(R.scale(width, height, f, aperture, cam.view_plane)[1])
        bound = (13 * f / z * A + 10 * c64) * U
        assert (c64 < 16).all()  # no clamp in this comparison
        ratio = float((np.abs(c.astype(np.float64) - c64) / bound).max())
        worst = max(worst, ratio)
        assert np.abs(z32.astype(np.float64) - z).max() <= 10 * U * z
        assert np.allclose(inv, 1 / np.maximum(np.pi * (c64 + 0.5) ** 2, 1), rtol=1e-5)
    print("circle of confusion against the thin lens in float64: at most %.2f of the bound" % worst)
    assert worst <= 1.0
    clamped = R.circles(records(4, 4, depth=0.25), f, aperture, cam.view_plane, 3)[0]
    assert (clamped == 3).all()  # far out of focus: the clamp
    assert (R.circles(records(4, 4, coverage=0.0), f, aperture, cam.view_plane, 16)[0] == R.scale(4, 4, f, aperture, cam.view_plane)[1]).all()  # the sky: |1 - f/inf| = 1


@pytest.mark.parametrize("radius", [1, 4])
def test_a_constant_image_stays_constant(radius):
    """out = a F + (1 - a) B with F = S_f / W_f, B = S_b / W_b. A sum of N = (2 radius + 1)^2 terms at the most: each of W's terms
    passes through at most N additions, each of S's through one multiplication more, so with weights of one sign S / W = colour
    (1 + e), |e| <= (2N + 1) u, and the division rounds once more: (2N + 2) u (tests/test_motion_blur_cpu.py has the same sum). The
    mix multiplies each by its share (1u each, and 1u for 1 - a) and adds (1u): a convex combination of two values within
    (2N + 2 + 2) u, rounded once more: (2N + 5) u, taken as (2N + 7) u for the terms of second order."""
    rng = np.random.default_rng(radius)
    width, height = 33, 17
    rec = records(width, height)
    rec["depth"] = rng.choice(np.array([1.0, 2.0, 2.03, 3.0, 8.0], dtype=f32), (height, width))
    rec["coverage"][rng.random((height, width)) < 0.2] = 0
    colour = np.array([0.37, 1.0, 7.25], dtype=f32)
    image = np.broadcast_to(colour, (height, width, 3)).copy()
    out = R.lens_blur(image, rec, 2.0, 0.01, 2.4, max_radius=radius)
    n = (2 * radius + 1) ** 2
    bound = (2 * n + 7) * U
    worst = float((np.abs(out.astype(np.float64) - colour) / colour).max())
    print("constant image, radius %d: at most %.3g relative, bound %.3g; %d pixels changed" % (radius, worst, bound, int((out != image).any(axis=-1).sum())))
    assert (out != image).any() and worst <= bound


def test_one_bright_pixel_in_a_field_of_equal_circles():
    """Every record a miss: c = A = 2.5 and z = FLT_MAX everywhere, so no tap is in front and every pixel away from the border has
    the same W. The bright pixel shows exactly where d < c + 1, and what it spreads sums to what it held: out(q) = V w(d_q) / W and
    the w(d_q) over the offsets are W's own terms. Each out(q) is within (2N + 3) u of that quotient (the sum of the test above
    without the mix; N = 81 offsets), all of one sign, so the sum, taken in float64, is within (2N + 3) u of V."""
    width, height, radius = 31, 25, 4
    rec = records(width, height, coverage=0.0)
    f, vp = 3.0, 2.4
    aperture = aperture_for(2.5, width, height, f, vp)
    c, inv, z = R.circles(rec, f, aperture, vp, radius)
    assert (np.abs(c - 2.5) <= 4 * 2.5 * U).all() and (z == R.FLT_MAX).all()
    image = np.zeros((height, width, 3), dtype=f32)
    image[12, 15] = (60.0, 6.0, 0.75)
    out = R.lens_blur(image, rec, f, aperture, vp, max_radius=radius)
    yy, xx = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    d = np.sqrt((yy - 12.0) ** 2 + (xx - 15.0) ** 2)
    assert np.array_equal((out > 0).all(axis=-1), d < 2.5 + 1) and np.array_equal((out > 0).any(axis=-1), d < 2.5 + 1)
    n = (2 * radius + 1) ** 2
    total = out.astype(np.float64).sum(axis=(0, 1))
    worst = float((np.abs(total - image[12, 15]) / image[12, 15]).max())
    print("one bright pixel: its sum moved by %.3g relative, bound %.3g; peak %.4g of 60" % (worst, (2 * n + 3) * U, out[12, 15, 0]))
    assert worst <= (2 * n + 3) * U
    assert out[12, 15, 0] < 60 * 0.05  # spread over a disc of pi 3^2 pixels


FOREGROUND, BACKGROUND = np.array([1, 0, 0], dtype=f32), np.array([0, 0, 1], dtype=f32)


def two_layers(square_depth, ground_depth, focus, A=5.0, radius=8):
    """A 6 x 6 square over a ground in a 40 x 30 image under the far view plane: (image, records, out, rows, cols, c)."""
    width, height = 40, 30
    rec = records(width, height, depth=ground_depth)
    image = np.broadcast_to(BACKGROUND, (height, width, 3)).copy()
    rows, cols = slice(12, 18), slice(17, 23)
    rec["depth"][rows, cols] = square_depth
    image[rows, cols] = FOREGROUND
    aperture = aperture_for(A, width, height, focus, FAR_PLANE)
    out = R.lens_blur(image, rec, focus, aperture, FAR_PLANE, max_radius=radius)
    return image, rec, out, rows, cols, R.circles(rec, focus, aperture, FAR_PLANE, radius)[0]


def test_a_sharp_foreground_over_a_blurred_background():
    image, rec, out, rows, cols, c = two_layers(square_depth=2.0, ground_depth=10.0, focus=2.0)
    assert not c[rows, cols].any() and abs(float(c[0, 0]) - 5.0 * 0.8) < 1e-4  # |1 - 2/10| = 0.8
    assert same_bits(out[rows, cols], image[rows, cols])  # no background colour inside the square: it is seen through its own circle, 0
    outside = np.ones(c.shape, dtype=bool)
    outside[rows, cols] = False
    assert not out[outside][:, 0].any()  # none of the square outside it: a front tap spreads by its own circle, 0
    assert (out[outside][:, 2] > 0.999).all() and np.isfinite(out).all()  # blue blurred into blue


def test_a_blurred_foreground_over_a_sharp_background():
    """The ground in focus, the square nearer with c = 5 |1 - 10/2| clamped to 8. A hole of one ground pixel in the middle of the
    square lies wholly under its blur: every other tap of its window within d < 9 is a front tap of weight clamp01(9 - d) / (pi 8.5^2).
    With a = fminf(W_f, 1) the hole shows a F + (1 - a) B, F the square's colour and B its own."""
    width, height = 40, 30
    image, rec, out, rows, cols, c = two_layers(square_depth=2.0, ground_depth=10.0, focus=10.0)
    assert (c[rows, cols] == 8).all() and not c[0, 0]
    assert np.allclose(out[rows, cols], FOREGROUND, atol=1e-5)  # one layer a pixel: the square sees the ground behind it through the ground's circle, 0, and stays opaque
    reached = out[..., 0] > 0
    yy, xx = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    nearest = np.hypot(np.clip(yy, 12, 17) - yy, np.clip(xx, 17, 22) - xx)  # distance to the square
    assert np.array_equal(reached, nearest < 9)  # the foreground bleeds over the sharp ground as far as its circle reaches, and no further
    rec = records(width, height, depth=2.0)  # now the whole frame is foreground but one pixel of ground
    rec["depth"][15, 20] = 10.0
    image = np.broadcast_to(FOREGROUND, (height, width, 3)).copy()
    image[15, 20] = BACKGROUND
    aperture = aperture_for(5.0, width, height, 10.0, FAR_PLANE)
    out = R.lens_blur(image, rec, 10.0, aperture, FAR_PLANE, max_radius=8)
    offsets = np.hypot(*np.meshgrid(np.arange(-8, 9), np.arange(-8, 9)))
    share = (np.clip(9 - offsets, 0, 1).sum() - 1) / max(np.pi * 8.5 ** 2, 1)  # W_f: every tap of the window but the hole itself
    a = min(share, 1.0)
    print("a ground pixel under a blurred foreground: W_f = %.4f, it shows %.4f of the foreground" % (share, out[15, 20, 0]))
    assert a > 0.95
    assert np.allclose(out[15, 20], a * FOREGROUND + (1 - a) * BACKGROUND, atol=1e-5)


def test_a_tap_that_is_not_finite_is_skipped_and_poisons_nothing():
    rng = np.random.default_rng(11)
    width, height = 24, 16
    image = rng.random((height, width, 3), dtype=f32)
    rec = records(width, height)
    rec["depth"] = rng.uniform(1, 6, (height, width)).astype(f32)
    clean = R.lens_blur(image, rec, 2.0, 0.02, 2.4, max_radius=5)
    assert np.isfinite(clean).all() and not same_bits(clean, image)
    dirty = image.copy()
    dirty[7, 11, 1], dirty[9, 3, 0] = np.nan, np.inf
    out = R.lens_blur(dirty, rec, 2.0, 0.02, 2.4, max_radius=5)
    bad = np.zeros((height, width), dtype=bool)
    bad[7, 11] = bad[9, 3] = True
    assert same_bits(out[bad], dirty[bad])  # a pixel that is not finite itself keeps its bits
    assert np.isfinite(out[~bad]).all()
    assert (out[~bad] != clean[~bad]).any()  # its neighbours went without it


def test_depths_exactly_at_the_tolerance_fall_on_the_stated_side():
    """front = (z_p - z_q) > depth_tolerance * z_p, strictly. p in focus at z = 4 (c_p = 0) beside q at z = 3 with tolerance 0.25:
    4 - 3 = 0.25 * 4, so q is not in front and is seen through p's circle, 0: p keeps its bits. One ulp nearer, q is in front,
    spreads by its own circle and changes p."""
    width, height = 9, 5
    aperture = aperture_for(6.0, width, height, 4.0, FAR_PLANE)
    image = np.full((height, width, 3), 0.25, dtype=f32)
    image[2, 5] = (4, 2, 1)
    for z_q, moved in [(f32(3), False), (np.nextafter(f32(3), f32(0)), True), (np.nextafter(f32(3), f32(4)), False)]:
        rec = records(width, height, depth=4.0)
        rec["depth"][2, 5] = z_q
        c, inv, z = R.circles(rec, 4.0, aperture, FAR_PLANE, 8)
        assert z[2, 5] == z_q and z[2, 4] == 4 and c[2, 4] == 0 and abs(float(c[2, 5]) - 2.0) < 1e-5
        out = R.lens_blur(image, rec, 4.0, aperture, FAR_PLANE, max_radius=8, depth_tolerance=0.25)
        assert (not same_bits(out[2, 4], image[2, 4])) == moved, z_q
        assert same_bits(out[2, 5], image[2, 5])  # q itself sees the ground behind it only through the ground's circle, 0
