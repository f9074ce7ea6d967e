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
    for name, make in list(inputs.TIE_FREE.items()) + list(inputs.FALLBACK.items()) + list(inputs.TOO_LARGE.items()) + list(inputs.DEPTH_RULE.items()):
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
    recursive, levelwise, paths = lines[0].split(), lines[1].split(), lines[3].split()
    assert recursive[0] == "recursive" and levelwise[0] == "levelwise" and lines[2].startswith("OK") and paths[0] == "paths", run.stdout
    r = {"recursive": recursive[1], "recursive_medians": int(recursive[3]), "levelwise": levelwise[1], "medians": int(levelwise[3]),
         "levels": int(levelwise[5]), "depth": int(levelwise[11]), "ok": lines[2], "stack": int(lines[2].split("stack ")[1].split(",")[0])}
    r.update({paths[i]: int(paths[i + 1]) for i in range(1, 17, 2)})  # LevelBuildStats: which paths of the device builder the input takes
    assert paths[17] == "root_centroid_extent"
    r["root_centroid_extent"] = [float.fromhex(x) for x in paths[18:21]]
    return r


# chain3000's four-wide tree needs a deeper stack than the kernels have: the tool reports that only when told to
DEEP = {"chain3000": ("-", "deep")}


def level_of(tool, files, name):
    return run_level(tool, *files[name], *DEEP.get(name, ()))


def test_the_sliver_mesh_is_the_one_of_the_builder_tests():
    assert len(inputs.sliver_mesh()) == 4612


@pytest.mark.parametrize("name", sorted(inputs.TIE_FREE))
def test_tie_free_inputs_give_the_recursive_builders_tree(tool, files, name):
    r = run_level(tool, *files[name])
    assert r["recursive_medians"] == 0, "%s needs the median fallback: it belongs to FALLBACK" % name
    assert r["medians"] == 0
    assert r["levelwise"] == r["recursive"]  # (the tool also compared the node numbering and checked the invariants)


@pytest.mark.parametrize("name", sorted(inputs.FALLBACK) + sorted(inputs.TOO_LARGE) + sorted(inputs.DEPTH_RULE))
def test_fallback_inputs_keep_the_invariants(tool, files, name):
    r = level_of(tool, files, name)  # exit status 0: coverage, real primitives, depth and stack, brute force, the same bytes twice
    assert r["recursive_medians"] > 0 and r["medians"] > 0


def test_every_input_is_pinned():
    assert sorted(PINS["level_tie_free"]) == sorted(inputs.TIE_FREE)
    assert sorted(PINS["level_fallback"]) == sorted(list(inputs.FALLBACK) + list(inputs.TOO_LARGE))
    assert sorted(PINS["level_depth_rule"]) == sorted(inputs.DEPTH_RULE)
    assert sorted(PINS["level_counts"]) == sorted(list(inputs.TIE_FREE) + list(inputs.FALLBACK) + list(inputs.TOO_LARGE) + list(inputs.DEPTH_RULE))


@pytest.mark.parametrize("name", sorted(inputs.TIE_FREE))
def test_tie_free_inputs_give_the_pinned_trees(tool, files, name):
    r = run_level(tool, *files[name])
    assert {"recursive": r["recursive"], "levelwise": r["levelwise"]} == PINS["level_tie_free"][name]


@pytest.mark.parametrize("name", sorted(inputs.FALLBACK) + sorted(inputs.TOO_LARGE))
def test_fallback_inputs_give_the_pinned_level_wise_trees(tool, files, name):
    """(the recursive builder's tree of these depends on the C++ library's nth_element and is not pinned)"""
    assert run_level(tool, *files[name])["levelwise"] == PINS["level_fallback"][name]["levelwise"]


@pytest.mark.parametrize("name", sorted(inputs.DEPTH_RULE))
def test_depth_rule_inputs_give_the_pinned_level_wise_trees(tool, files, name):
    r = level_of(tool, files, name)
    assert r["levelwise"] == PINS["level_depth_rule"][name]["levelwise"]


@pytest.mark.parametrize("name", sorted(inputs.TIE_FREE) + sorted(inputs.FALLBACK) + sorted(inputs.TOO_LARGE) + sorted(inputs.DEPTH_RULE))
def test_the_pinned_medians_and_levels_are_the_rehearsals(tool, files, name):
    """What tests/test_gpu_bvh_build.py holds the device's PyrBuildInfo to: both count the iterations of the level loop (none for a
    scene that is a single leaf)."""
    r = level_of(tool, files, name)
    assert {"medians": r["medians"], "levels": r["levels"]} == PINS["level_counts"][name]


# ------------------------------------------------------------------- which path of the device builder an input reaches
# kernels/build.hip: a node of more than 64 references is "large" (bin_large / choose_large / partition_large or median_large, in
# chunks of 2,048), a smaller one is one wave's (small_kernel); a median over more than 2,048 ends the device build.
def test_tri40000_has_more_large_nodes_in_a_level_than_one_workgroup_of_the_choose_kernel(tool, files):
    assert level_of(tool, files, "tri40000")["most_large_nodes"] > 64


@pytest.mark.parametrize("name,chunks", [("tri66", 1), ("tri2047", 1), ("tri2048", 1), ("tri2049", 2), ("tri4096", 2), ("tri4097", 3)])
def test_the_roots_at_the_chunk_edges_have_that_many_chunks(tool, files, name, chunks):
    spheres, tris = inputs.TIE_FREE[name]()
    assert len(tris) == int(name[3:]) and level_of(tool, files, name)["most_chunks"] == chunks


def test_a_root_of_a_waves_worth_is_no_large_node(tool, files):
    assert len(inputs.TIE_FREE["tri64"]()[1]) == 64 and level_of(tool, files, "tri64")["most_large_nodes"] == 0
    assert level_of(tool, files, "mixed2600")["most_chunks"] == 2  # spheres and triangles past one chunk


@pytest.mark.parametrize("name", ["chain300", "chain300_r4"])
def test_the_depth_rule_forces_a_median_over_distinct_centroids_in_the_median_kernel(tool, files, name):
    r = level_of(tool, files, name)
    assert 64 < r["largest_forced_median"] <= 2048
    assert r["medians_positive_large"] > 0 and r["medians_positive_small"] > 0  # distinct centroids: the comparison decides, not the shape code
    assert r["depth"] == 39
    assert r["stack"] <= 64  # the scene keeps its four-wide tree


def test_chain3000_forces_a_median_too_large_for_the_device_and_loses_its_wide_tree(tool, files):
    r = level_of(tool, files, "chain3000")
    assert r["largest_forced_median"] > 2048 and r["depth"] == 39
    assert r["stack"] > 64
    # without the new argument the tool stops where it always did
    run = subprocess.run([tool, "level", *files["chain3000"]], capture_output=True, text=True)
    assert run.returncode == 1 and "FAIL stack need" in run.stdout


def test_tiny_xyz_ranks_distinct_centroids_whose_extent_is_subnormal(tool, files):
    import numpy as np

    r = level_of(tool, files, "tiny_xyz")
    assert r["medians_positive_small"] > 0 and r["medians_positive_large"] > 0
    assert r["medians_infinite_scale"] == r["medians_positive_small"] + r["medians_positive_large"] == r["medians"]
    with np.errstate(over="ignore"):
        for extent in r["root_centroid_extent"]:
            assert 0.0 < extent < float(np.finfo(np.float32).tiny) and np.isinf(np.float32(16.0) / np.float32(extent))


@pytest.mark.parametrize("name,axes", [("tiny_x", (0,)), ("tiny_xy", (0, 1))])
def test_the_tiny_inputs_have_subnormal_extents_on_their_axes_only(tool, files, name, axes):
    import numpy as np

    extent = level_of(tool, files, name)["root_centroid_extent"]
    for a in range(3):
        assert (0.0 < extent[a] < float(np.finfo(np.float32).tiny)) == (a in axes) and (a in axes or extent[a] > 1.0)


def test_grid_z0_splits_large_nodes_with_a_degenerate_axis_and_needs_no_median(tool, files):
    r = level_of(tool, files, "grid_z0")
    assert r["medians"] == 0 and r["largest_median"] == 0
    assert r["root_centroid_extent"][2] == 0.0 and min(r["root_centroid_extent"][:2]) > 0.0
    assert r["degenerate_axis_splits"] > 0 and r["most_chunks"] == 2


def test_spheres_on_triangles_is_one_median_of_200(tool, files):
    spheres, tris = inputs.FALLBACK["spheres_on_triangles"]()
    assert len(spheres) == len(tris) == 100
    r = level_of(tool, files, "spheres_on_triangles")
    assert r["largest_median"] == 200 and r["medians_positive_small"] == r["medians_positive_large"] == 0 and r["levels"] > 1


def test_fives1000_ends_every_cluster_in_a_median_of_one_wave(tool, files):
    r = level_of(tool, files, "fives1000")
    assert r["largest_median"] == 5 and r["medians"] == 1000 and r["medians_positive_small"] == 0


def test_signed_zeros_and_near_limit_hold_what_their_names_say():
    import numpy as np

    t = inputs.TIE_FREE["signed_zeros"]()[1]
    zeros = t[t == 0.0]
    assert np.signbit(zeros).sum() > 50 and (~np.signbit(zeros)).sum() > 50  # about 150 of 4,500 coordinates are zero, either sign as often
    big = np.abs(inputs.TIE_FREE["near_limit"]()[1]).max()
    assert 5.0e13 < big < 1.0e15  # (a scene holds coordinates up to 1e15: scene_internal.h kMaxCoordinate)
    for name in inputs.DEPTH_RULE:
        assert np.abs(inputs.DEPTH_RULE[name]()[1]).max() < 1.0e15


NEW_HITTABLE = sorted(n for n in inputs.EDGES if n not in inputs.UNHITTABLE)


@pytest.mark.parametrize("name", NEW_HITTABLE)
def test_the_oracle_alone_hits_the_floor_the_gpu_tests_ask_for(name):
    """tests/test_gpu_bvh_build.py asserts at least 1,000 hits of these 20,000 rays: it must hold for the reference by itself."""
    import oracle
    from test_gpu_bvh_build import world_of

    spheres, tris = inputs.group_of(name)[name]()
    hits, _ = oracle.OracleScene(world_of(spheres, tris)).intersect(inputs.rays_of(name, spheres, tris))
    assert (hits["shape"] != 0xFFFFFFFF).sum() >= 1000


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
    # (all but tri40000: the probe's depth bound of 8 ranks its 40,000 references against each other at the root, two minutes under
    # the sanitizers, and what that input is for -- a level of many large nodes -- is the device's own affair; tri4097 stands for it here)
    run = subprocess.run([str(exe)] + [files[name][0] for name in sorted(files) if name != "tri40000"], capture_output=True, text=True)
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
