"""Progressive sessions without a GPU: the grown ABI (version 5: PyrRenderParams::sample_begin, the pyr_session_* entries and
pyr_render_simple_progressive), their argument checks, and the command-line flags of both front ends."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import pytest

from pyrite_amd import abi
from pyrite_amd import build as gpu_build
from pyrite_amd.__main__ import progressive_flag_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pyrite_gpu.h")
SESSION_ENTRIES = ["pyr_session_create", "pyr_session_destroy", "pyr_session_render", "pyr_session_sync", "pyr_session_samples_done", "pyr_session_preview",
                   "pyr_session_film", "pyr_session_film_device", "pyr_session_halves", "pyr_session_noise", "pyr_render_simple_progressive"]


@pytest.fixture(scope="module")
def lib():
    return abi.bind(C.CDLL(gpu_build.build()))


def test_library_exports_the_session_entries_at_abi_5(lib):
    for name in SESSION_ENTRIES:
        assert hasattr(lib, name), "libpyrite_gpu.so does not export %s" % name
        assert name in abi.ENTRY_POINTS
    assert lib.pyr_abi_version() == abi.PYR_ABI_VERSION == 5
    assert int(re.search(r"#define PYR_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 5
    assert re.search(r"#define PYR_SESSION_HALVES (\d+)u", open(HEADER).read()).group(1) == str(abi.PYR_SESSION_HALVES)


def test_grown_render_params_layout_matches_the_header():
    """sizeof / offsetof as gcc lays the header out against the ctypes mirror (the way tests/test_abi.py does it), for the struct
    that grew and the ones a session takes."""
    structs = ["PyrRenderParams", "PyrDevelopParams", "PyrFilmDesc", "PyrCamera", "PyrGrain"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "%s"' % HEADER, "int main(void){"]
    for s in structs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for field, _ in getattr(abi, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, field, s, field))
    lines.append('printf("preview_fn %zu\\n", sizeof(PyrPreviewFn));')
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
    assert abi.PyrRenderParams._fields_[-1][0] == "sample_begin" and abi.PyrRenderParams.sample_begin.offset == 56 and C.sizeof(abi.PyrRenderParams) == 64
    assert int(expect["preview_fn"]) == C.sizeof(abi.PyrPreviewFn)


def test_python_params_carry_the_window():
    from pyrite_amd.renderer import Renderer

    r = Renderer(16)
    assert r.params().sample_begin == 0 and r.params(sample_begin=8).sample_begin == 8


def good_arguments():
    camera, film, params = abi.PyrCamera(), abi.PyrFilmDesc(8, 8, 64, 380.0, 400.0), abi.PyrRenderParams()
    params.bounces, params.pixel_samples, params.light_samples, params.spectrum_samples, params.tile_size = 2, 4, 1, 10, 32
    develop = abi.PyrDevelopParams()
    table = (C.c_float * 6)()
    develop.step_size, develop.xyz_scale, develop.sample_count, develop.xyz_count, develop.xyz_min, develop.xyz_max = 30.0, 3.444, 15, 2, 360.0, 830.0
    develop.xyz_table = C.cast(table, C.POINTER(C.c_float))
    return camera, film, params, develop, table


def test_session_entries_refuse_null_arguments(lib):
    out = (C.c_uint8 * 4096)()
    n = C.c_uint32(7)
    _, _, _, develop, _table = good_arguments()
    for call in (lambda: lib.pyr_session_render(None, 4),
                 lambda: lib.pyr_session_sync(None),
                 lambda: lib.pyr_session_samples_done(None, C.byref(n)),
                 lambda: lib.pyr_session_preview(None, C.byref(develop), out),
                 lambda: lib.pyr_session_film(None, out),
                 lambda: lib.pyr_session_film_device(None, out),
                 lambda: lib.pyr_session_halves(None, out, out),
                 lambda: lib.pyr_session_noise(None, out)):
        assert call() == abi.PYR_ERR_INVALID_ARGUMENT
        assert b"null" in lib.pyr_last_error()
    lib.pyr_session_destroy(None)  # a no-op


def test_session_create_checks_its_arguments_before_it_looks_for_a_device(lib):
    camera, film, params, develop, _table = good_arguments()
    scene = C.create_string_buffer(1 << 16)  # stands in for a PyrScene: the checks below come before anything reads it
    handle = C.c_void_p(1)

    def create(scene=scene, camera=camera, film=film, params=params, flags=0, out=handle):
        return lib.pyr_session_create(scene, C.byref(camera) if camera else None, C.byref(film) if film else None, C.byref(params) if params else None, flags, None,
                                      C.byref(out) if out is not None else None)

    assert create(out=None) == abi.PYR_ERR_INVALID_ARGUMENT
    for missing in ("scene", "camera", "film", "params"):
        assert create(**{missing: None}) == abi.PYR_ERR_INVALID_ARGUMENT, missing
        assert b"null" in lib.pyr_last_error() and not handle
    for field, target in (("width", film), ("height", film), ("bins", film), ("tile_size", params), ("spectrum_samples", params), ("pixel_samples", params)):
        keep = getattr(target, field)
        setattr(target, field, 0)
        assert create() == abi.PYR_ERR_INVALID_ARGUMENT, field
        assert b"zero" in lib.pyr_last_error()
        setattr(target, field, keep)
    params.sample_begin = 3
    assert create() == abi.PYR_ERR_INVALID_ARGUMENT and b"sample_begin" in lib.pyr_last_error()
    params.sample_begin = 0
    params.film_layout = abi.PYR_FILM_TILE_BLOCKS
    assert create() == abi.PYR_ERR_INVALID_ARGUMENT
    params.film_layout = abi.PYR_FILM_ROWS
    if lib.pyr_device_count() == 0:
        assert create() == abi.PYR_ERR_DEVICE and b"no HIP device" in lib.pyr_last_error() and not handle


def test_progressive_render_checks_its_arguments_before_it_looks_for_a_device(lib):
    camera, film, params, develop, _table = good_arguments()
    scene = C.create_string_buffer(1 << 16)
    grains = (abi.PyrGrain * (8 * 8 * 64))()
    no_status, no_preview = C.cast(None, abi.PyrProgressFn), C.cast(None, abi.PyrPreviewFn)
    preview = abi.PyrPreviewFn(lambda user, rgb, width, height, done: None)

    def run(scene=scene, camera=camera, film=film, params=params, grains=grains, pass_samples=4, on_preview=no_preview, interval=0.0, develop=develop):
        return lib.pyr_render_simple_progressive(scene, C.byref(camera) if camera else None, C.byref(film) if film else None, C.byref(params) if params else None,
                                                 grains, pass_samples, no_status, on_preview, interval, C.byref(develop) if develop else None, None)

    for missing in ("scene", "camera", "film", "params", "grains"):
        assert run(**{missing: None}) == abi.PYR_ERR_INVALID_ARGUMENT, missing
        assert b"null" in lib.pyr_last_error()
    assert run(on_preview=preview, develop=None) == abi.PYR_ERR_INVALID_ARGUMENT  # a preview needs its development parameters
    assert run(pass_samples=0) == abi.PYR_ERR_INVALID_ARGUMENT and b"pass_samples" in lib.pyr_last_error()
    assert run(interval=-1.0) == abi.PYR_ERR_INVALID_ARGUMENT and b"interval" in lib.pyr_last_error()
    assert run(interval=float("nan")) == abi.PYR_ERR_INVALID_ARGUMENT
    film.width = 0
    assert run() == abi.PYR_ERR_INVALID_ARGUMENT and b"zero" in lib.pyr_last_error()
    film.width = 8
    if lib.pyr_device_count() == 0:
        assert run() == abi.PYR_ERR_DEVICE and b"no HIP device" in lib.pyr_last_error()
        assert run(on_preview=preview) == abi.PYR_ERR_DEVICE


def test_plain_renders_refuse_a_window_without_a_device_like_any_render(lib):
    """sample_begin rides in PyrRenderParams of every render entry: the null / zero checks come first, as before."""
    camera, film, params, _, _table = good_arguments()
    params.sample_begin = 8
    assert lib.pyr_render_simple(None, C.byref(camera), C.byref(film), C.byref(params), None, C.cast(None, abi.PyrProgressFn), None) == abi.PYR_ERR_INVALID_ARGUMENT


BAD_FLAGS = [
    (["--pass-samples", "0"], "--pass-samples must be at least 1"),
    (["--pass-samples", "-3"], "--pass-samples must be at least 1"),
    (["--preview", "p.png", "--preview-every", "-1"], "--preview-every must not be negative"),
    (["--noise"], "--noise needs --preview"),
]


def test_flag_rules():
    assert progressive_flag_problem(None, None, 20.0, False) is None
    assert progressive_flag_problem(4, "p.png", 0.0, True) is None
    assert progressive_flag_problem(0, None, 20.0, False) == BAD_FLAGS[0][1]
    assert progressive_flag_problem(1, "p.png", float("nan"), False) == BAD_FLAGS[2][1]
    assert progressive_flag_problem(None, None, 20.0, True) == BAD_FLAGS[3][1]


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
        flags = ["--pass-samples", "2", "--preview", os.path.join(d, "p.png"), "--preview-every", "0.5", "--noise"]
        py = subprocess.run([sys.executable, "-m", "pyrite_amd", project, "--spp", "4", "--size", "16x16", "-o", os.path.join(d, "a.png")] + flags, cwd=ROOT,
                            env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
        cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", project, "-", "1", os.path.join(d, "b.png")] + flags, cwd=ROOT, capture_output=True, text=True)
    for run in (py, cpp):
        assert "unrecognized" not in run.stderr and "unknown flag" not in run.stderr and "must" not in run.stderr and "needs" not in run.stderr, run.stderr
        assert run.returncode == 0 or "no HIP device" in run.stderr, run.stderr
    unknown = subprocess.run([gpu_build.HOST_TOOL, "render-project", project, "-", "1", os.devnull, "--pass-sample", "2"], cwd=ROOT, capture_output=True, text=True)
    assert unknown.returncode != 0 and "unknown flag" in unknown.stderr
