"""The device BVH builder's rehearsal on the CPU: build_bvh_levelwise (pyrite_amd/csrc/bvh.cpp) builds level
by level with the per-reference and per-node functions of bvh_level.h -- the ones kernels/build.hip compiles -- through
tools/bvh_quality.cpp's `level` mode. No GPU.

Where the recursive builder needs no median fallback, the level-wise tree is its tree: equal digests, equal node numbering.
All builders decide by the same functions, so a wrong edit there moves them together: tests/golden/bvh_digests.json pins the trees.
Where it does (or the depth bound is lowered to 8), the tree keeps the tool's invariants: every primitive named once by a leaf
whose box holds it, depth and stack bounds, the same closest hits and blocked shadow rays as brute force, the same bytes twice.
The argument checks of pyr_scene_create_with come before any device is looked for."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_quality  # noqa: E402

import bvh_build_inputs as inputs  # noqa: E402

from pyrite_amd import abi  # noqa: E402
from pyrite_amd import build as gpu_build  # noqa: E402

SOURCES = [os.path.join(ROOT, "tools", "bvh_quality.cpp"), os.path.join(ROOT, "pyrite_amd", "csrc", "bvh.cpp")]
with open(os.path.join(ROOT, "tests", "golden", "bvh_digests.json")) as f:
    PINS = json.load(f)


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bvh_level") / "bvh_quality")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", out] + SOURCES)
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (PRIMS path, RAYS path) of every input."""
    d = tmp_path_factory.mktemp("bvh_level_inputs")
    out = {}
    for name, make in list(inputs.TIE_FREE.items()) + list(inputs.FALLBACK.items()) + list(inputs.TOO_LARGE.items()):
        spheres, tris = make()
        prims, rays = str(d / (name + ".prims")), str(d / (name + ".rays"))
        bvh_quality.write_prims(prims, spheres, tris)
        bvh_quality.write_rays(rays, *inputs.rays_for(spheres, tris))
        out[name] = (prims, rays)
    return out


@functools.lru_cache(maxsize=None)
def run_level(tool, prims, rays, *extra):
    run = subprocess.run([tool, "level", prims, rays] + list(extra), capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    recursive, levelwise = lines[0].split(), lines[1].split()
    assert recursive[0] == "recursive" and levelwise[0] == "levelwise" and lines[2].startswith("OK"), run.stdout
    return {"recursive": recursive[1], "recursive_medians": int(recursive[3]), "levelwise": levelwise[1], "medians": int(levelwise[3]),
            "levels": int(levelwise[5]), "ok": lines[2]}


def test_the_sliver_mesh_is_the_one_of_the_builder_tests():
    assert len(inputs.sliver_mesh()) == 4612


@pytest.mark.parametrize("name", sorted(inputs.TIE_FREE))
def test_tie_free_inputs_give_the_recursive_builders_tree(tool, files, name):
    r = run_level(tool, *files[name])
    assert r["recursive_medians"] == 0, "%s needs the median fallback: it belongs to FALLBACK" % name
    assert r["medians"] == 0
    assert r["levelwise"] == r["recursive"]  # (the tool also compared the node numbering and checked the invariants)


@pytest.mark.parametrize("name", sorted(inputs.FALLBACK) + sorted(inputs.TOO_LARGE))
def test_fallback_inputs_keep_the_invariants(tool, files, name):
    r = run_level(tool, *files[name])  # exit status 0: coverage, real primitives, depth and stack, brute force, the same bytes twice
    assert r["recursive_medians"] > 0 and r["medians"] > 0


def test_every_input_is_pinned():
    assert sorted(PINS["level_tie_free"]) == sorted(inputs.TIE_FREE)
    assert sorted(PINS["level_fallback"]) == sorted(list(inputs.FALLBACK) + list(inputs.TOO_LARGE))


@pytest.mark.parametrize("name", sorted(inputs.TIE_FREE))
def test_tie_free_inputs_give_the_pinned_trees(tool, files, name):
    r = run_level(tool, *files[name])
    assert {"recursive": r["recursive"], "levelwise": r["levelwise"]} == PINS["level_tie_free"][name]


@pytest.mark.parametrize("name", sorted(inputs.FALLBACK) + sorted(inputs.TOO_LARGE))
def test_fallback_inputs_give_the_pinned_level_wise_trees(tool, files, name):
    """(the recursive builder's tree of these depends on the C++ library's nth_element and is not pinned)"""
    assert run_level(tool, *files[name])["levelwise"] == PINS["level_fallback"][name]["levelwise"]


def test_the_c3_mesh_gives_the_pinned_tree_with_both_builders(tool, tmp_path):
    """819,212 triangles, no rays: the tree DESIGN.md section 9e and profiles/r10_build.txt report, a few seconds."""
    tris = bvh_quality.c3_triangles()
    assert len(tris) == PINS["level_c3_mesh"]["triangles"]
    prims = str(tmp_path / "c3.prims")
    bvh_quality.write_prims(prims, inputs.NO_SPHERES, tris)
    r = run_level(tool, prims, "-")
    assert r["recursive_medians"] == 0 and r["medians"] == 0
    assert (r["recursive"], r["levelwise"]) == (PINS["level_c3_mesh"]["recursive"], PINS["level_c3_mesh"]["levelwise"])


@pytest.mark.parametrize("name", ["sliver_mesh", "mixed", "tri257"])
def test_a_depth_bound_of_8_forces_medians_and_keeps_the_invariants(tool, files, name):
    r = run_level(tool, *files[name], "8")
    assert r["medians"] > 0 and r["levelwise"] != r["recursive"]
    assert r["levels"] <= 41


def test_the_rays_exercise_the_trees(tool, files):
    ok = run_level(tool, *files["sliver_mesh"])["ok"]
    hits = int(ok.split("(")[1].split()[0])
    blocked = int(ok.split(",")[-1].split()[0])
    assert hits > 500 and 100 < blocked < 1400


def test_the_level_wise_builder_is_clean_under_the_sanitizers(tmp_path, files):
    """tests/probes/bvh_level_check.cpp: a program of its own, run as a child process; nothing is loaded into this interpreter."""
    exe = tmp_path / "bvh_level_check"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", str(exe), os.path.join(ROOT, "tests", "probes", "bvh_level_check.cpp"), SOURCES[1]])
    run = subprocess.run([str(exe)] + [files[name][0] for name in sorted(files)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok: ")


# ------------------------------------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    library = C.CDLL(gpu_build.build())
    abi.bind(library)
    return library


def test_a_bad_builder_or_dirty_reserved_words_are_refused_before_any_device(lib):
    assert abi.PYR_ABI_VERSION == 5 and lib.pyr_abi_version() == 5
    handle = C.c_void_p()
    params = abi.PyrBuildParams(builder=2)
    # a null description: were anything looked at before the build parameters, the message would name it instead
    assert lib.pyr_scene_create_with(None, 0, C.byref(params), C.byref(handle)) == abi.PYR_ERR_INVALID_ARGUMENT
    assert b"builder" in lib.pyr_last_error() and not handle.value
    for word in range(7):
        params = abi.PyrBuildParams(builder=abi.PYR_BUILD_DEVICE)
        params.reserved[word] = 1
        assert lib.pyr_scene_create_with(None, 0, C.byref(params), C.byref(handle)) == abi.PYR_ERR_INVALID_ARGUMENT
        assert b"reserved" in lib.pyr_last_error() and not handle.value
    # well-formed parameters reach the description's own checks
    params = abi.PyrBuildParams(builder=abi.PYR_BUILD_DEVICE)
    assert lib.pyr_scene_create_with(None, 0, C.byref(params), C.byref(handle)) == abi.PYR_ERR_INVALID_ARGUMENT
    assert b"builder" not in lib.pyr_last_error() and b"reserved" not in lib.pyr_last_error()
    assert lib.pyr_scene_build_info(None, None) == abi.PYR_ERR_INVALID_ARGUMENT


def test_the_build_structs_match_the_header(tmp_path):
    """sizeof / offsetof as gcc lays the header out, against the ctypes mirrors (tests/test_abi.py does this for the older structs)."""
    header = os.path.join(ROOT, "include", "pyrite_gpu.h")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "%s"' % header, "int main(void){"]
    for s in ("PyrBuildParams", "PyrBuildInfo"):
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for field, _ in getattr(abi, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, field, s, field))
    lines.append("return 0;}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    expect = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines() if line)
    for s in ("PyrBuildParams", "PyrBuildInfo"):
        cls = getattr(abi, s)
        assert int(expect[s]) == C.sizeof(cls), s
        for field, _ in cls._fields_:
            assert int(expect["%s.%s" % (s, field)]) == getattr(cls, field).offset, "%s.%s" % (s, field)


def test_both_command_lines_refuse_an_unknown_builder():
    project = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    py = subprocess.run([sys.executable, "-m", "pyrite_amd", project, "--build", "both"], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert py.returncode == 2 and "--build" in py.stderr
    gpu_build.build()
    cpp = subprocess.run([gpu_build.HOST_TOOL, "render-project", project, "-", "1", os.devnull, "--build", "both"], cwd=ROOT, capture_output=True, text=True)
    assert cpp.returncode == 2 and "--build takes host or device" in cpp.stderr
