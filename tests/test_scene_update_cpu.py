"""pyr_scene_update without a GPU: the two new structs of the ABI, the argument checks that come before any
device is looked for, and the host rehearsal of the refit -- refit_bvh / refit_wide (pyrite_amd/csrc/bvh.cpp) on the rules of
bvh_level.h that kernels/refit.hip compiles too -- through tests/probes/refit_check.cpp, a program of its own built with
-fsanitize=address,undefined and run as a child process."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_build_inputs as inputs  # noqa: E402

from pyrite_amd import abi  # noqa: E402
from pyrite_amd import build as gpu_build  # noqa: E402

HEADER = os.path.join(ROOT, "include", "pyrite_gpu.h")
STRUCTS = ["PyrGeometryUpdate", "PyrUpdateInfo"]


def test_header_and_ctypes_agree_on_the_update_structs():
    """sizeof / offsetof as gcc lays the header out, against the ctypes mirrors (tests/test_abi.py's check, for the new structs)."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "%s"' % HEADER, "int main(void){"]
    for s in STRUCTS:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for field, _ in getattr(abi, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, field, s, field))
    lines.append('printf("REFIT %u REBUILD %u\\n", PYR_UPDATE_REFIT, PYR_UPDATE_REBUILD);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    expect = dict(l.split() for l in out if l and not l.startswith("REFIT"))
    for s in STRUCTS:
        cls = getattr(abi, s)
        assert int(expect[s]) == C.sizeof(cls), s
        for field, _ in cls._fields_:
            assert int(expect["%s.%s" % (s, field)]) == getattr(cls, field).offset, "%s.%s" % (s, field)
    assert "REFIT %d REBUILD %d" % (abi.PYR_UPDATE_REFIT, abi.PYR_UPDATE_REBUILD) in out
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+PYR_ABI_VERSION\s+5\b", text) and abi.PYR_ABI_VERSION == 5  # additions only


@pytest.fixture(scope="module")
def lib():
    return abi.bind(C.CDLL(gpu_build.build()))


def test_bad_arguments_are_refused_before_any_device_is_looked_for(lib):
    """No GPU here: anything that reached the device would be PYR_ERR_DEVICE. pyr_last_error names the argument."""
    positions = np.zeros((1, 9), dtype=np.float32)
    good = abi.PyrGeometryUpdate(mode=abi.PYR_UPDATE_REFIT)
    cases = [
        ("null scene", None, good, b"null scene"),
        ("null update", None, None, b"null update"),
        ("unknown mode", None, abi.PyrGeometryUpdate(mode=7), b"mode"),
        ("wrong counts: triangles given for a count of zero", None, abi.PyrGeometryUpdate(mode=abi.PYR_UPDATE_REBUILD, num_triangles=0, tri_positions=positions.ctypes.data),
         b"num_triangles"),
        ("wrong counts: spheres given for a count of zero", None, abi.PyrGeometryUpdate(mode=abi.PYR_UPDATE_REFIT, num_spheres=0, spheres=positions.ctypes.data), b"num_spheres"),
        ("reserved word", None, abi.PyrGeometryUpdate(mode=abi.PYR_UPDATE_REFIT, reserved=(C.c_uint32 * 4)(0, 0, 1, 0)), b"reserved"),
    ]
    for what, scene, update, word in cases:
        for call in (lambda: lib.pyr_scene_update(scene, C.byref(update) if update is not None else None),
                     lambda: lib.pyr_scene_update_device(scene, C.byref(update) if update is not None else None, None)):
            assert call() == abi.PYR_ERR_INVALID_ARGUMENT, what
            assert word in lib.pyr_last_error(), (what, lib.pyr_last_error())
    assert lib.pyr_scene_update_info(None, None) == abi.PYR_ERR_INVALID_ARGUMENT
    info = abi.PyrUpdateInfo()
    assert lib.pyr_scene_update_info(None, C.byref(info)) == abi.PYR_ERR_INVALID_ARGUMENT


def test_the_python_layer_names_its_modes():
    from pyrite_amd.renderer import World

    assert World.UPDATE_MODES == {"refit": abi.PYR_UPDATE_REFIT, "rebuild": abi.PYR_UPDATE_REBUILD}
    assert callable(World.update) and callable(World.update_info)


def write_input(path, spheres, tris):
    with open(path, "wb") as f:
        f.write(np.array([len(spheres), len(tris)], dtype=np.uint32).tobytes())
        f.write(np.ascontiguousarray(spheres, dtype=np.float32).tobytes())
        f.write(np.ascontiguousarray(tris, dtype=np.float32).tobytes())


def test_the_host_rehearsal_of_the_refit_under_sanitizers(tmp_path):
    """tests/probes/refit_check.cpp on every tie-free input (the LDS-sized ones, `mixed`, and `sliver_mesh` with its 4,612 triangles)
    and the fallback ones, both collapses each: an identity refit leaves the Node64 and Node128 arrays byte for byte; after a rigid
    move and a random displacement every stored box contains what lies beneath it; the area ratios are printed, 1 for the identity."""
    exe = tmp_path / "refit_check"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", str(exe), os.path.join(ROOT, "tests", "probes", "refit_check.cpp"),
                           os.path.join(ROOT, "pyrite_amd", "csrc", "bvh.cpp")])
    files = []
    for name, make in list(inputs.TIE_FREE.items()) + list(inputs.FALLBACK.items()):
        spheres, tris = make()
        files.append(str(tmp_path / name))
        write_input(files[-1], spheres, tris)
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "OK: 0 failure(s)" in run.stdout
    ratios = {tuple(l.split()[:2]): float(l.split()[3]) for l in run.stdout.splitlines() if " area_ratio " in l}
    for name in list(inputs.TIE_FREE) + list(inputs.FALLBACK):
        assert ratios[name, "identity"] == 1.0
        assert np.isfinite(ratios[name, "rigid"]) and ratios[name, "rigid"] > 0.0 and np.isfinite(ratios[name, "shaken"]) and ratios[name, "shaken"] > 0.0
