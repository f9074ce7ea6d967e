"""Linear images and tone mapping without a GPU: the new entries of the C ABI (still version 5) and the layouts of their two structs
against gcc, the argument checks that come before a device is looked for, pyr_tone_resolve on hand-built histograms, the Radiance
RGBE and PFM writers read back by readers written here, the same bytes from the Python and the C++ writer, and the --hdr /
--exposure / --tone flags of both command lines.

The RGBE round trip is held to one mantissa step of the pixel's shared exponent, |c' - c| <= 2^(e - 8), against the value the
format can hold: a channel that is not positive (negative, NaN) is 0, and one above the format's largest value 255 * 2^119 =
1.69e38 (3e38, and +inf by way of FLT_MAX) is that value -- its exponent byte would be 256 otherwise. A pixel whose largest
channel is below the 1e-32 cut is four zero bytes."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from pyrite_amd import abi
from pyrite_amd import build as gpu_build
from pyrite_amd import develop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pyrite_gpu.h")
f32 = np.float32
TONE_ENTRIES = ["pyr_film_develop_linear", "pyr_film_develop_linear_device", "pyr_image_stats", "pyr_image_stats_device", "pyr_tone_resolve", "pyr_image_tonemap",
                "pyr_image_tonemap_device", "pyr_session_linear", "pyr_session_preview_tone"]


@pytest.fixture(scope="module")
def lib():
    return abi.bind(C.CDLL(gpu_build.build()))


@pytest.fixture(scope="module")
def host(lib):
    h = C.CDLL(gpu_build.HOST_OUT)
    h.pyrh_test_linear_image.restype = C.c_int
    h.pyrh_test_linear_image.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
    return h


# ------------------------------------------------------------------------------------------------------------------------ ABI
def test_library_exports_the_tone_entries_and_stays_at_abi_5(lib):
    header = open(HEADER).read()
    for name in TONE_ENTRIES:
        assert hasattr(lib, name), "libpyrite_gpu.so does not export %s" % name
        assert name in abi.ENTRY_POINTS
        assert re.search(r"\b%s\(" % name, header)
    assert lib.pyr_abi_version() == abi.PYR_ABI_VERSION == 5
    assert re.search(r"#define PYR_ABI_VERSION 5\b", header)


def test_tone_struct_layouts_and_constants_match_the_header():
    structs = ["PyrImageStats", "PyrToneParams"]
    constants = ["PYR_LINEAR_XYZ", "PYR_LINEAR_SRGB", "PYR_TONE_CLIP", "PYR_TONE_REINHARD"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "%s"' % HEADER, "int main(void){"]
    for s in structs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for field, _ in getattr(abi, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, field, s, field))
    for c in constants:
        lines.append('printf("%s %%u\\n", (unsigned)%s);' % (c, c))
    lines.append('printf("defaults %.17g %.17g %.17g\\n", (double)PYR_TONE_KEY, (double)PYR_TONE_PERCENTILE, (double)PYR_TONE_WHITE_PERCENTILE);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-o", exe, src])
        out = [l.split() for l in subprocess.check_output([exe]).decode().split("\n") if l]
    expect = {l[0]: l[1:] for l in out}
    for s in structs:
        cls = getattr(abi, s)
        assert int(expect[s][0]) == C.sizeof(cls), s
        for field, _ in cls._fields_:
            assert int(expect["%s.%s" % (s, field)][0]) == getattr(cls, field).offset, "%s.%s" % (s, field)
    assert C.sizeof(abi.PyrImageStats) == 1040 and C.sizeof(abi.PyrToneParams) == 24
    for c in constants:
        assert int(expect[c][0]) == getattr(abi, c), c
    assert [float(x) for x in expect["defaults"]] == [float(f32(abi.PYR_TONE_KEY)), float(f32(abi.PYR_TONE_PERCENTILE)), float(f32(abi.PYR_TONE_WHITE_PERCENTILE))]


def test_python_surface():
    from pyrite_amd.renderer import Session

    for name in ("develop_linear", "image_stats", "tonemap", "tone_params", "tone_resolve", "save_hdr", "save_pfm", "encode_hdr", "encode_pfm"):
        assert callable(getattr(develop, name)), name
    assert callable(Session.linear) and "tone" in Session.preview.__code__.co_varnames
    t = develop.tone_params("reinhard")
    assert (t.op, t.exposure, t.white) == (abi.PYR_TONE_REINHARD, 0.0, 0.0)
    assert (t.key, t.percentile, t.white_percentile) == (f32(0.18), f32(0.5), f32(0.99))


def test_entries_check_their_arguments_before_they_look_for_a_device(lib):
    """Null pointers, an unknown space or operator, unresolved tone parameters: PYR_ERR_INVALID_ARGUMENT; more than 2^32 - 1 pixels:
    PYR_ERR_UNSUPPORTED; and only then the missing device."""
    tb_xyz = np.zeros((4, 3), dtype=f32)
    p = abi.PyrDevelopParams(2.0, 3.444, 201, None, None, None, tb_xyz.ctypes.data_as(C.POINTER(C.c_float)), 4, 380.0, 780.0)
    film = abi.PyrFilmDesc(4, 2, 8, 380.0, 400.0)
    grains, out = np.zeros((2, 4, 8, 2), dtype=f32), np.zeros((2, 4, 3), dtype=f32)
    rgb8, stats = np.zeros((2, 4, 3), dtype=np.uint8), abi.PyrImageStats()
    INVALID, UNSUPPORTED, DEVICE = abi.PYR_ERR_INVALID_ARGUMENT, abi.PYR_ERR_UNSUPPORTED, abi.PYR_ERR_DEVICE
    no_gpu = lib.pyr_device_count() == 0

    def linear(film=film, grains=grains.ctypes.data, p=p, space=abi.PYR_LINEAR_SRGB, out=out.ctypes.data, device=0):
        return lib.pyr_film_develop_linear(C.byref(film) if film else None, grains, None, C.byref(p) if p else None, space, out, device)

    def linear_device(film=film, grains=grains.ctypes.data, p=p, space=abi.PYR_LINEAR_SRGB, out=out.ctypes.data, device=0):
        return lib.pyr_film_develop_linear_device(C.byref(film) if film else None, grains, None, C.byref(p) if p else None, space, out, device, None)

    for call in (linear, linear_device):
        for missing in ("film", "grains", "p", "out"):
            assert call(**{missing: None}) == INVALID and b"null argument" in lib.pyr_last_error(), missing
        assert call(space=2) == INVALID and b"unknown space" in lib.pyr_last_error()
        assert call(p=abi.PyrDevelopParams(0.0, 3.444, 201, None, None, None, p.xyz_table, 4, 380.0, 780.0)) == INVALID
        assert call(film=abi.PyrFilmDesc(1 << 16, 1 << 16, 8, 380.0, 400.0)) == UNSUPPORTED and b"2^32 - 1 pixels" in lib.pyr_last_error()
        assert call(device=-1) == DEVICE
        if no_gpu:
            assert call() == DEVICE and b"HIP device" in lib.pyr_last_error()

    for call in (lambda *a: lib.pyr_image_stats(*a, 0), lambda *a: lib.pyr_image_stats_device(*a, 0, None)):
        assert call(None, 4, 2, C.byref(stats)) == INVALID
        assert call(out.ctypes.data, 4, 2, None) == INVALID
        assert call(out.ctypes.data, 1 << 16, 1 << 16, C.byref(stats)) == UNSUPPORTED
        if no_gpu:
            assert call(out.ctypes.data, 4, 2, C.byref(stats)) == DEVICE

    good = abi.PyrToneParams(abi.PYR_TONE_REINHARD, 1.0, 2.0, 0.18, 0.5, 0.99)
    for call in (lambda *a: lib.pyr_image_tonemap(*a, 0), lambda *a: lib.pyr_image_tonemap_device(*a, 0, None)):
        assert call(None, 4, 2, C.byref(good), rgb8.ctypes.data) == INVALID
        assert call(out.ctypes.data, 4, 2, None, rgb8.ctypes.data) == INVALID
        assert call(out.ctypes.data, 4, 2, C.byref(good), None) == INVALID
        assert call(out.ctypes.data, 4, 2, C.byref(abi.PyrToneParams(2, 1.0, 2.0, 0.18, 0.5, 0.99)), rgb8.ctypes.data) == INVALID and b"unknown tone operator" in lib.pyr_last_error()
        assert call(out.ctypes.data, 4, 2, C.byref(abi.PyrToneParams(abi.PYR_TONE_CLIP, 0.0, 0.0, 0.18, 0.5, 0.99)), rgb8.ctypes.data) == INVALID and b"unresolved" in lib.pyr_last_error()
        assert call(out.ctypes.data, 4, 2, C.byref(abi.PyrToneParams(abi.PYR_TONE_REINHARD, 1.0, 0.0, 0.18, 0.5, 0.99)), rgb8.ctypes.data) == INVALID
        assert call(out.ctypes.data, 1 << 16, 1 << 16, C.byref(good), rgb8.ctypes.data) == UNSUPPORTED
        if no_gpu:
            assert call(out.ctypes.data, 4, 2, C.byref(good), rgb8.ctypes.data) == DEVICE

    assert lib.pyr_session_linear(None, C.byref(p), abi.PYR_LINEAR_SRGB, out.ctypes.data) == INVALID
    assert lib.pyr_session_preview_tone(None, C.byref(p), C.byref(good), rgb8.ctypes.data, None) == INVALID
    session = C.create_string_buffer(1 << 12)  # stands in for a PyrSession: the checks below come before anything but its film description is read
    assert lib.pyr_session_linear(session, None, abi.PYR_LINEAR_SRGB, out.ctypes.data) == INVALID
    assert lib.pyr_session_linear(session, C.byref(p), abi.PYR_LINEAR_SRGB, None) == INVALID
    assert lib.pyr_session_linear(session, C.byref(p), 7, out.ctypes.data) == INVALID and b"unknown space" in lib.pyr_last_error()
    assert lib.pyr_session_preview_tone(session, C.byref(p), None, rgb8.ctypes.data, None) == INVALID
    assert lib.pyr_session_preview_tone(session, C.byref(p), C.byref(good), None, None) == INVALID
    assert lib.pyr_session_preview_tone(session, C.byref(p), C.byref(abi.PyrToneParams(9, 1.0, 2.0, 0.18, 0.5, 0.99)), rgb8.ctypes.data, None) == INVALID and b"unknown tone operator" in lib.pyr_last_error()
    assert lib.pyr_session_preview_tone(session, C.byref(p), C.byref(abi.PyrToneParams(0, 0.0, 0.0, 0.18, 0.0, 0.99)), rgb8.ctypes.data, None) == INVALID and b"percentile" in lib.pyr_last_error()


# ------------------------------------------------------------------------------------------------------------------------ the rule
def upper_edge(k):
    return np.array([(k + 889) << 20], dtype=np.uint32).view(f32)[0]


def histogram(counts):
    s = abi.PyrImageStats()
    for k, n in counts.items():
        s.histogram[k] = n
    s.lit = sum(counts.values())
    return s


def resolve(lib, stats, tone):
    exposure, white = C.c_float(-1), C.c_float(-1)
    rc = lib.pyr_tone_resolve(C.byref(stats) if stats is not None else None, C.byref(tone), C.byref(exposure), C.byref(white))
    return rc, f32(exposure.value), f32(white.value)


def test_the_histogram_edges():
    assert upper_edge(-1) == f32(2.0 ** -16) and upper_edge(255) == f32(2.0 ** 16)  # bin 0 starts at 2^-16, bin 255 ends at 2^16
    assert upper_edge(7) == f32(2.0 ** -15) and upper_edge(0) == f32(2.0 ** -16 * 1.125)  # 8 bins per octave, linear in the mantissa


def test_tone_resolve_on_hand_built_histograms(lib):
    key = f32(0.18)
    auto = abi.PyrToneParams(abi.PYR_TONE_REINHARD, 0.0, 0.0, 0.18, 0.5, 0.99)
    # everything in one bin
    rc, exposure, white = resolve(lib, histogram({100: 1000}), auto)
    assert rc == 0 and exposure == f32(key / upper_edge(100)) and white == f32(exposure * upper_edge(100))
    # nothing lit
    rc, exposure, white = resolve(lib, histogram({}), auto)
    assert (rc, exposure, white) == (0, 1.0, 1.0)
    # the percentile lands exactly on a cumulative boundary: 50 of 100 are reached by the first bin; one more pixel needs the second
    two = histogram({10: 50, 20: 50})
    rc, exposure, white = resolve(lib, two, auto)
    assert rc == 0 and exposure == f32(key / upper_edge(10)) and white == f32(exposure * upper_edge(20))
    rc, exposure, _ = resolve(lib, two, abi.PyrToneParams(abi.PYR_TONE_REINHARD, 0.0, 0.0, 0.18, 0.51, 0.5))
    assert rc == 0 and exposure == f32(key / upper_edge(20))
    rc, exposure, white = resolve(lib, two, abi.PyrToneParams(abi.PYR_TONE_REINHARD, 0.0, 0.0, 0.18, 0.51, 0.5))
    assert white == f32(exposure * upper_edge(10))  # the white point's own percentile, on the boundary too
    rc, exposure, _ = resolve(lib, two, abi.PyrToneParams(abi.PYR_TONE_CLIP, 0.0, 0.0, 0.18, 1.0, 0.99))
    assert rc == 0 and exposure == f32(key / upper_edge(20))  # percentile 1: the last lit pixel
    rc, exposure, _ = resolve(lib, two, abi.PyrToneParams(abi.PYR_TONE_CLIP, 0.0, 0.0, 0.18, 1e-9, 0.99))
    assert rc == 0 and exposure == f32(key / upper_edge(10))  # a target below one pixel is the first lit pixel
    # bin 0 and bin 255
    ends = histogram({0: 3, 255: 1})
    rc, exposure, white = resolve(lib, ends, auto)
    assert rc == 0 and exposure == f32(key / upper_edge(0)) and white == f32(exposure * f32(65536.0))
    rc, exposure, _ = resolve(lib, histogram({255: 5}), auto)
    assert rc == 0 and exposure == f32(key / f32(65536.0))
    # what is given is kept; the clip reads no white point
    rc, exposure, white = resolve(lib, ends, abi.PyrToneParams(abi.PYR_TONE_REINHARD, 4.0, 0.0, 0.18, 0.5, 0.99))
    assert (rc, exposure, white) == (0, 4.0, f32(4.0) * f32(65536.0))
    rc, exposure, white = resolve(lib, None, abi.PyrToneParams(abi.PYR_TONE_REINHARD, 0.25, 3.0, 0.18, 0.5, 0.99))
    assert (rc, exposure, white) == (0, 0.25, 3.0)
    rc, exposure, white = resolve(lib, None, abi.PyrToneParams(abi.PYR_TONE_CLIP, 2.0, 0.0, 0.18, 0.5, 0.99))
    assert (rc, exposure, white) == (0, 2.0, 1.0)
    # the Python wrapper is the same call
    assert develop.tone_resolve(two, auto) == (float(f32(key / upper_edge(10))), float(f32(f32(key / upper_edge(10)) * upper_edge(20))))


def test_tone_resolve_refuses_nonsense(lib):
    INVALID = abi.PYR_ERR_INVALID_ARGUMENT
    some = histogram({5: 1})
    for percentile in (0.0, -0.5, 1.5, float("nan")):
        assert resolve(lib, some, abi.PyrToneParams(abi.PYR_TONE_CLIP, 0.0, 0.0, 0.18, percentile, 0.99))[0] == INVALID, percentile
        assert resolve(lib, some, abi.PyrToneParams(abi.PYR_TONE_REINHARD, 0.0, 0.0, 0.18, 0.5, percentile))[0] == INVALID, percentile
        assert b"percentile" in lib.pyr_last_error()
    assert resolve(lib, some, abi.PyrToneParams(2, 0.0, 0.0, 0.18, 0.5, 0.99))[0] == INVALID and b"unknown tone operator" in lib.pyr_last_error()
    assert resolve(lib, some, abi.PyrToneParams(abi.PYR_TONE_CLIP, 0.0, 0.0, 0.0, 0.5, 0.99))[0] == INVALID and b"key" in lib.pyr_last_error()
    assert resolve(lib, None, abi.PyrToneParams(abi.PYR_TONE_CLIP, 0.0, 0.0, 0.18, 0.5, 0.99))[0] == INVALID and b"statistics" in lib.pyr_last_error()
    assert resolve(lib, None, abi.PyrToneParams(abi.PYR_TONE_REINHARD, 1.0, 0.0, 0.18, 0.5, 0.99))[0] == INVALID
    tone = abi.PyrToneParams(abi.PYR_TONE_CLIP, 1.0, 0.0, 0.18, 0.5, 0.99)
    out = C.c_float()
    assert lib.pyr_tone_resolve(C.byref(some), None, C.byref(out), C.byref(out)) == INVALID
    assert lib.pyr_tone_resolve(C.byref(some), C.byref(tone), None, C.byref(out)) == INVALID
    assert lib.pyr_tone_resolve(C.byref(some), C.byref(tone), C.byref(out), None) == INVALID


# ------------------------------------------------------------------------------------------------------------------------ the writers
RGBE_MAX = f32(255.0 * 2.0 ** 119)


def hand_made_image():
    """7 x 3 pixels: zero, a negative value and NaN; +inf; 1e-40 and 1e-33 below the 1e-32 cut and 1e-31 above it; 1, 0.5, 255.999 and
    3e38; a pixel whose channels differ by 2^20; the rest ordinary colours."""
    inf, nan = float("inf"), float("nan")
    rows = [
        [[0, 0, 0], [-1.0, 0.25, 0.5], [nan, 2.0, nan], [inf, 1.0, 3.0], [1e-40, 0, 1e-41], [1e-33, 5e-34, 0], [1e-31, 2e-32, 1e-33]],
        [[1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [255.999, 1.0, 0.001], [3e38, 1e38, 1e30], [1048576.0, 1.0, 0.5], [2.0 ** -20, 1.0, 3.0], [0.18, 0.18, 0.18]],
        [[0.999999, 0.5000001, 0.2499999], [inf, inf, -inf], [nan, nan, nan], [1e-32, 0, 0], [3.4028235e38, 7.0, 0.1], [12.5, 700.25, 0.0625], [-0.0, 1e-5, 3e-5]],
    ]
    return np.asarray(rows, dtype=f32)


def read_pfm(data):
    magic, size, scale, rest = data.split(b"\n", 3)
    assert magic == b"PF" and scale == b"-1.0"
    w, h = (int(x) for x in size.split())
    assert len(rest) == w * h * 12
    return np.frombuffer(rest, dtype="<f4").reshape(h, w, 3)[::-1]


def read_hdr(data):
    """(float64 [h, w, 3] decoded as byte * 2^(E - 136), the exponent bytes [h, w])"""
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n"
    assert data.startswith(head)
    size, rest = data[len(head):].split(b"\n", 1)
    m = re.fullmatch(rb"-Y (\d+) \+X (\d+)", size)
    h, w = int(m.group(1)), int(m.group(2))
    assert len(rest) == w * h * 4  # flat scanlines
    px = np.frombuffer(rest, dtype=np.uint8).reshape(h, w, 4)
    e = px[..., 3].astype(np.int64)
    value = np.where(e[..., None] == 0, 0.0, px[..., :3].astype(np.float64) * np.exp2((e - 136).astype(np.float64))[..., None])
    assert not px[e == 0].any()  # a zero exponent byte goes with zero mantissas
    return value, e


def storable(image):
    """What the RGBE format can hold of a pixel: non-positive and NaN channels as 0, anything above the largest value as that value."""
    with np.errstate(invalid="ignore"):
        return np.minimum(np.where(image > 0, image, f32(0)), RGBE_MAX).astype(np.float64)


def check_hdr_round_trip(image, data):
    value, e = read_hdr(data)
    want = storable(image)
    assert value.shape == want.shape
    flushed = e == 0
    assert (want[flushed].max(axis=-1) < 1e-32).all() if flushed.any() else True
    assert (want[~flushed].max(axis=-1) >= 1e-32).all()
    step = np.exp2((e - 128 - 8).astype(np.float64))[..., None]  # one mantissa step of the shared exponent
    assert (np.abs(value - want)[~flushed] <= np.broadcast_to(step, want.shape)[~flushed]).all()
    # the shared exponent is the largest channel's: its mantissa byte has the top bit set
    assert (value[~flushed].max(axis=-1) >= 128 * step[~flushed][:, 0]).all()
    return value


def test_pfm_round_trip_is_exact():
    image = hand_made_image()
    data = develop.encode_pfm(image)
    assert data.startswith(b"PF\n7 3\n-1.0\n")
    back = read_pfm(data)
    assert back.dtype == np.dtype("<f4") and back.tobytes() == image.tobytes()  # NaN payloads, -0.0 and the infinities too
    assert data[-7 * 12:] == image[0].tobytes()  # rows bottom to top: the file ends with the image's first row


def test_hdr_round_trip_is_within_one_mantissa_step():
    image = hand_made_image()
    data = develop.encode_hdr(image)
    assert data.startswith(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 3 +X 7\n")
    value = check_hdr_round_trip(image, data)
    pixels = np.frombuffer(data[-7 * 3 * 4:], dtype=np.uint8).reshape(3, 7, 4)
    assert pixels[1, 0].tolist() == [128, 128, 128, 129] and pixels[1, 1].tolist() == [128, 128, 128, 128]  # 1.0 = 0.5 * 2^1, 0.5 = 0.5 * 2^0
    assert pixels[0, 0].tolist() == [0, 0, 0, 0] and pixels[0, 4].tolist() == [0, 0, 0, 0] and pixels[0, 5].tolist() == [0, 0, 0, 0]  # zero, and below the cut
    assert pixels[0, 6, 3] != 0 and pixels[2, 3, 3] != 0  # 1e-31 and 1e-32 itself are kept
    assert pixels[0, 1].tolist() == [0, 64, 128, 128] and pixels[0, 2].tolist() == [0, 128, 0, 130]  # the negative channel and the NaNs are 0
    assert pixels[0, 3].tolist() == [255, 0, 0, 255] and pixels[1, 3, 3] == 255 and pixels[2, 4].tolist() == [255, 0, 0, 255]  # +inf, 3e38, FLT_MAX: the format's largest value
    assert pixels[1, 4].tolist() == [128, 0, 0, 149]  # channels 2^20 apart: the small ones vanish, inside the bound all the same
    assert pixels[1, 2].tolist() == [255, 1, 0, 136]  # 255.999 = 0.99999 * 2^8: one mantissa step is 1.0
    assert value[1, 2, 0] == 255.0


def test_both_front_ends_write_the_same_bytes(host, tmp_path):
    image = hand_made_image()
    for pfm, encode in ((0, develop.encode_hdr), (1, develop.encode_pfm)):
        path = tmp_path / ("image.pfm" if pfm else "image.hdr")
        assert host.pyrh_test_linear_image(str(path).encode(), image.ctypes.data, 7, 3, pfm) == 0
        assert path.read_bytes() == encode(image)
    # and a larger image of ordinary values, the mantissa roundings of 4096 pixels
    rng = np.random.default_rng(7)
    big = np.exp2(rng.uniform(-30, 30, size=(64, 64, 3))).astype(f32)
    path = tmp_path / "big.hdr"
    assert host.pyrh_test_linear_image(str(path).encode(), big.ctypes.data, 64, 64, 0) == 0
    assert path.read_bytes() == develop.encode_hdr(big)
    check_hdr_round_trip(big, path.read_bytes())
    py = tmp_path / "py.hdr"
    develop.save_hdr(str(py), big)
    assert py.read_bytes() == path.read_bytes()
    develop.save_pfm(str(py), big)
    assert read_pfm(py.read_bytes()).tobytes() == big.tobytes()


# ------------------------------------------------------------------------------------------------------------------------ the flags
BAD_FLAGS = [
    (["--hdr", "out.exr"], "--hdr must end in .hdr or .pfm"),
    (["--hdr", "hdr"], "--hdr must end in .hdr or .pfm"),
    (["--tone", "filmic"], "--tone must be clip or reinhard"),
    (["--exposure", "bright"], "--exposure must be a number of stops or auto"),
]


def test_flag_rules():
    assert develop.tone_flag_problem(None, None, None) is None and develop.tone_flag_problem("a.hdr", "auto", "reinhard") is None
    assert develop.tone_flag_problem("A.PFM", "-1.5", "clip") is None
    assert develop.tone_flag_problem("a.png", None, None) == BAD_FLAGS[0][1] and develop.tone_flag_problem(None, None, "Reinhard") == BAD_FLAGS[2][1]
    assert develop.tone_flag_problem(None, "nan", None) == BAD_FLAGS[3][1]
    assert develop.tone_from_flags(None, None) is None
    t = develop.tone_from_flags("1.5", None)
    assert (t.op, t.exposure, t.white) == (abi.PYR_TONE_CLIP, f32(2.0 ** 1.5), 0.0)  # stops
    t = develop.tone_from_flags(None, "reinhard")
    assert (t.op, t.exposure) == (abi.PYR_TONE_REINHARD, 0.0)  # reinhard alone: automatic exposure
    t = develop.tone_from_flags(None, "clip")
    assert (t.op, t.exposure) == (abi.PYR_TONE_CLIP, 1.0)
    t = develop.tone_from_flags("auto", "clip")
    assert (t.op, t.exposure) == (abi.PYR_TONE_CLIP, 0.0)
    assert math.isclose(develop.tone_from_flags("-2", "reinhard").exposure, 0.25)


@pytest.mark.parametrize("flags,message", BAD_FLAGS)
def test_both_front_ends_reject_nonsense_in_the_same_words(flags, message, lib):
    project = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    py = subprocess.run([sys.executable, "-m", "pyrite_amd", project] + flags, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", project, "-", "1", os.devnull] + flags, cwd=ROOT, capture_output=True, text=True)
    assert py.returncode == 2 and cpp.returncode == 2
    assert py.stderr.strip() == cpp.stderr.strip() == "error: " + message


def test_both_front_ends_parse_the_flags():
    """Well-formed flags get past the parser: what stops the run here is the missing GPU (or nothing, on a GPU box)."""
    project = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    with tempfile.TemporaryDirectory() as d:
        flags = ["--hdr", os.path.join(d, "f.hdr"), "--exposure", "-1", "--tone", "reinhard", "--spp", "1", "--size", "16x16"]
        py = subprocess.run([sys.executable, "-m", "pyrite_amd", project, "-o", os.path.join(d, "a.png")] + flags, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                            capture_output=True, text=True)
        cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", project, "-", "1", os.path.join(d, "b.png")] + flags, cwd=ROOT, capture_output=True, text=True)
    for run in (py, cpp):
        assert "unrecognized" not in run.stderr and "unknown flag" not in run.stderr and "must" not in run.stderr and "needs" not in run.stderr, run.stderr
        assert run.returncode == 0 or "HIP device" in run.stderr, run.stderr
