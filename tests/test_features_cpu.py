"""The first-hit feature pass without a GPU: the three new entries of the C ABI (still version 5), the layouts of their two structs
against gcc, the argument checks that come before a device is looked for, the --features flags of both command lines, and the
8-bit encodings of the normal and depth images, which must be the same bytes from Python and from pyrite_host_tool."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from pyrite_amd import abi
from pyrite_amd import build as gpu_build
from pyrite_amd.features import RECORD, Features, encode_depth, encode_normal, features_flag_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pyrite_gpu.h")
FEATURE_ENTRIES = ["pyr_render_features", "pyr_render_features_device", "pyr_session_features"]


@pytest.fixture(scope="module")
def lib():
    return abi.bind(C.CDLL(gpu_build.build()))


def test_library_exports_the_feature_entries_and_stays_at_abi_5(lib):
    for name in FEATURE_ENTRIES:
        assert hasattr(lib, name), "libpyrite_gpu.so does not export %s" % name
        assert name in abi.ENTRY_POINTS
        assert re.search(r"\b%s\(" % name, open(HEADER).read())
    assert lib.pyr_abi_version() == abi.PYR_ABI_VERSION == 5


def test_feature_struct_layouts_match_the_header():
    structs = ["PyrFeatureParams", "PyrFeaturePixel"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "%s"' % HEADER, "int main(void){"]
    for s in structs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for field, _ in getattr(abi, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, field, s, field))
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-o", exe, src])
        expect = dict(l.split() for l in subprocess.check_output([exe]).decode().split("\n") if l)
    for s in structs:
        cls = getattr(abi, s)
        assert int(expect[s]) == C.sizeof(cls), s
        for field, _ in cls._fields_:
            assert int(expect["%s.%s" % (s, field)]) == getattr(cls, field).offset, "%s.%s" % (s, field)
    assert C.sizeof(abi.PyrFeatureParams) == 16 and C.sizeof(abi.PyrFeaturePixel) == 32 == RECORD.itemsize
    assert [RECORD.fields[name][1] for name in RECORD.names] == [getattr(abi.PyrFeaturePixel, name).offset for name, _ in abi.PyrFeaturePixel._fields_]


def test_feature_entries_check_their_arguments_before_they_look_for_a_device(lib):
    camera, film, fp = abi.PyrCamera(), abi.PyrFilmDesc(8, 8, 64, 380.0, 400.0), abi.PyrFeatureParams(2, 16)
    scene = C.create_string_buffer(1 << 16)  # stands in for a PyrScene: the checks below come before anything reads it
    albedo, pixels = (abi.PyrGrain * (8 * 8 * 64))(), (abi.PyrFeaturePixel * 64)()

    def host(scene=scene, camera=camera, film=film, fp=fp, albedo=albedo, pixels=pixels):
        return lib.pyr_render_features(scene, C.byref(camera) if camera else None, C.byref(film) if film else None, C.byref(fp) if fp else None, albedo, pixels)

    def device(scene=scene, camera=camera, film=film, fp=fp, albedo=albedo, pixels=pixels):
        return lib.pyr_render_features_device(scene, C.byref(camera) if camera else None, C.byref(film) if film else None, C.byref(fp) if fp else None, albedo, pixels, None)

    for call in (host, device):
        for missing in ("scene", "camera", "film", "fp"):
            assert call(**{missing: None}) == abi.PYR_ERR_INVALID_ARGUMENT, missing
            assert b"null argument: " + missing.encode() in lib.pyr_last_error()
        assert call(albedo=None, pixels=None) == abi.PYR_ERR_INVALID_ARGUMENT and b"both null" in lib.pyr_last_error()
        for grid in (0, 9):
            fp.grid = grid
            assert call() == abi.PYR_ERR_INVALID_ARGUMENT and b"fp->grid must be 1..8" in lib.pyr_last_error()
        fp.grid = 2
        for bins in (0, 65):
            fp.albedo_bins = bins
            assert call() == abi.PYR_ERR_INVALID_ARGUMENT and b"fp->albedo_bins must be 1..64" in lib.pyr_last_error()
            if lib.pyr_device_count() == 0:
                assert call(albedo=None) == abi.PYR_ERR_DEVICE  # the bins are not read without an albedo buffer
        fp.albedo_bins = 16
        film.width = 0
        assert call() == abi.PYR_ERR_INVALID_ARGUMENT and b"film: zero-sized image" in lib.pyr_last_error()
        film.width, film.height = 1 << 16, 1 << 16
        assert call() == abi.PYR_ERR_INVALID_ARGUMENT and b"film: 2^32 pixels or more" in lib.pyr_last_error()
        film.width, film.height = 8, 8
        film.wl_width = 0.0
        assert call() == abi.PYR_ERR_INVALID_ARGUMENT and b"wavelength span" in lib.pyr_last_error()
        film.wl_width = 400.0
        if lib.pyr_device_count() == 0:
            assert call() == abi.PYR_ERR_DEVICE and b"no HIP device" in lib.pyr_last_error()
    assert lib.pyr_session_features(None, C.byref(fp), albedo, pixels) == abi.PYR_ERR_INVALID_ARGUMENT and b"null argument: session" in lib.pyr_last_error()


def test_python_surface():
    from pyrite_amd.renderer import Renderer, Session

    assert callable(Renderer.features) and callable(Session.features)
    f = Features(3, 2, 5)
    assert f.albedo.grains.shape == (2, 3, 5, 2) and f.normal.shape == (2, 3, 3) and f.depth.shape == f.coverage.shape == f.shape.shape == f.material.shape == (2, 3)
    f.records["depth"][1, 2] = 4.0
    assert f.depth[1, 2] == 4.0  # views of the records


BAD_FLAGS = [
    (["--features", "p", "--features-grid", "0"], "--features-grid must be 1 to 8"),
    (["--features", "p", "--features-grid", "9"], "--features-grid must be 1 to 8"),
    (["--features-grid", "2"], "--features-grid needs --features"),
]


def test_flag_rules():
    assert features_flag_problem(None, None) is None and features_flag_problem("p", None) is None and features_flag_problem("p", 8) is None
    assert features_flag_problem("p", 0) == BAD_FLAGS[0][1] and features_flag_problem(None, 2) == BAD_FLAGS[2][1]


@pytest.mark.parametrize("flags,message", BAD_FLAGS)
def test_both_front_ends_reject_nonsense_in_the_same_words(flags, message, lib):
    project = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    py = subprocess.run([sys.executable, "-m", "pyrite_amd", project] + flags, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", project, "-", "1", os.devnull] + flags, cwd=ROOT, capture_output=True, text=True)
    assert py.returncode == 2 and cpp.returncode == 2
    assert py.stderr.strip() == cpp.stderr.strip() == "error: " + message


def hand_made_records():
    """3 x 2 pixels: two depths' ends, values on both sides of a rounding step, a normal beyond the unit cube, and one miss."""
    rec = np.zeros((2, 3), dtype=RECORD)
    rec["normal"] = [[[0.0, 0.0, 1.0], [-1.0, 0.25, 0.5], [0.3, -0.7, 0.648]], [[1.5, -1.5, 0.001], [0.0, 0.0, 0.0], [0.57735, 0.57735, -0.57735]]]
    rec["depth"] = [[2.0, 3.5, 10.0], [7.25, 0.0, 2.0000002]]
    rec["coverage"] = [[1.0, 0.5, 1.0], [0.25, 0.0, 1.0]]
    rec["shape"][1, 1] = abi.HIT_NONE
    return rec


def test_both_front_ends_encode_the_same_bytes(lib, tmp_path):
    rec = hand_made_records()
    normal, depth = encode_normal(rec["normal"], rec["coverage"]), encode_depth(rec["depth"], rec["coverage"])
    # the encodings themselves, by hand
    assert normal.shape == depth.shape == (2, 3, 3) and normal.dtype == depth.dtype == np.uint8
    assert normal[0, 0].tolist() == [128, 128, 255] and normal[0, 1].tolist() == [0, 159, 191] and normal[1, 0].tolist() == [255, 0, 128]
    assert not normal[1, 1].any() and not depth[1, 1].any()  # the miss is black
    assert depth[0, 0].tolist() == [255, 255, 255] and depth[0, 2].tolist() == [0, 0, 0]  # near is white, far is black
    assert depth[0, 1].tolist() == [207] * 3 and (depth[..., 0] == depth[..., 1]).all() and (depth[..., 1] == depth[..., 2]).all()
    one = np.zeros((1, 2), dtype=RECORD)
    one["depth"], one["coverage"] = [[3.0, 3.0]], [[1.0, 0.0]]
    assert encode_depth(one["depth"], one["coverage"])[0].tolist() == [[255] * 3, [0] * 3]  # one depth only: covered is white
    # the C++ front end writes the same bytes
    records, out_n, out_d = tmp_path / "records.bin", tmp_path / "normal.rgb", tmp_path / "depth.rgb"
    records.write_bytes(rec.tobytes())
    subprocess.check_call([gpu_build.HOST_TOOL, "encode-features", str(records), str(out_n), str(out_d)])
    assert out_n.read_bytes() == normal.tobytes()
    assert out_d.read_bytes() == depth.tobytes()


def test_both_front_ends_parse_the_flags():
    """Well-formed flags get past the parser: what stops the run here is the missing GPU (or nothing, on a GPU box)."""
    project = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    with tempfile.TemporaryDirectory() as d:
        flags = ["--features", os.path.join(d, "f"), "--features-grid", "2", "--spp", "1", "--size", "16x16"]
        py = subprocess.run([sys.executable, "-m", "pyrite_amd", project, "-o", os.path.join(d, "a.png")] + flags, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                            capture_output=True, text=True)
        cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", project, "-", "1", os.path.join(d, "b.png")] + flags, cwd=ROOT, capture_output=True, text=True)
    for run in (py, cpp):
        assert "unrecognized" not in run.stderr and "unknown flag" not in run.stderr and "must" not in run.stderr and "needs" not in run.stderr, run.stderr
        assert run.returncode == 0 or "no HIP device" in run.stderr, run.stderr
