"""The mesh BVH's builder on the CPU (pyrite_amd/csrc/bvh.cpp through tools/bvh_quality.cpp): the cost-driven collapse and
the spatial-split build of the four-child pair tree. No GPU: the tool walks the trees with the kernels' semantics.

On a small sliver mesh (a coarse torus knot, scenes.torus_knot_mesh, in a box of large walls) every tree: covers each triangle
with the leaf boxes that name it, names only real triangles, keeps the depth and stack bounds, builds to the same bytes twice,
and finds the same closest hits and the same blocked shadow rays as brute force. PYRITE_SPATIAL_SPLITS / PYRITE_WIDE_COLLAPSE
select the trees they say, and the three trees of the sliver mesh are the ones tests/golden/bvh_digests.json pins."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bvh_quality  # noqa: E402

from pyrite_amd import scenes  # noqa: E402


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bvh_quality") / "bvh_quality")
    src = [os.path.join(ROOT, "tools", "bvh_quality.cpp"), os.path.join(ROOT, "pyrite_amd", "csrc", "bvh.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", out] + src)
    return out


def sliver_mesh():
    positions, _ = scenes.torus_knot_mesh(segments=96, sides=24, fit_min=(-8.0, -8.0, 1.0), fit_max=(8.0, 8.0, 9.0))
    tris = np.asarray(positions, dtype=np.float32).reshape(-1, 9)
    # two walls of two big triangles each, across the whole knot: what spatial splits clip first
    walls = np.array([[-10, -10, 0, 10, -10, 0, 10, 10, 0], [-10, -10, 0, 10, 10, 0, -10, 10, 0],
                      [-10, 10, 0, 10, 10, 0, 10, 10, 10], [-10, 10, 0, 10, 10, 10, -10, 10, 10]], dtype=np.float32)
    return np.concatenate([walls, tris])


@pytest.fixture(scope="module")
def mesh_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh")
    tris = sliver_mesh()
    tri_path, ray_path = str(d / "tris.bin"), str(d / "rays.bin")
    bvh_quality.write_triangles(tri_path, tris)
    rng = np.random.RandomState(5)
    n = 3000
    o = rng.uniform([-9, -9, 0.5], [9, 9, 9.5], size=(n, 3))
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    # shadow rays between two random points: blocked where something lies in between
    a = rng.uniform([-9, -9, 0.5], [9, 9, 9.5], size=(n, 3))
    b = rng.uniform([-9, -9, 0.5], [9, 9, 9.5], size=(n, 3))
    to_b = b - a
    dist = np.linalg.norm(to_b, axis=1)
    origins = np.concatenate([o, a])
    directions = np.concatenate([dirs, to_b / dist[:, None]])
    limits = np.concatenate([np.full(n, -1.0), dist * dist - 1e-4])
    bvh_quality.write_rays(ray_path, origins, directions, limits)
    return tri_path, ray_path, len(tris)


@pytest.mark.parametrize("splits", ["object", "spatial"])
def test_tree_covers_every_triangle_and_walks_like_brute_force(tool, mesh_files, splits):
    tri_path, ray_path, n = mesh_files
    run = subprocess.run([tool, "check", tri_path, ray_path, splits], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("OK"), run.stdout
    fields = run.stdout.split()
    references = int(fields[fields.index("references,") - 1])
    if splits == "spatial":
        assert n < references <= 1.4 * n + 1  # splits happened, within the duplication budget
    else:
        assert references == n
    hits = int(run.stdout.split("(")[1].split()[0])
    blocked = int(run.stdout.split(",")[-1].split()[0])
    assert hits > 1000 and 100 < blocked < 2900  # the rays exercise the tree: many hit something, shadow rays go both ways


def hashes(tool, tri_path, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("PYRITE_SPATIAL_SPLITS", "PYRITE_WIDE_COLLAPSE")}
    e.update(env)
    out = subprocess.check_output([tool, "hash", tri_path], env=e, text=True)
    return dict(line.split() for line in out.splitlines())


def test_builds_are_deterministic_and_the_switches_select_the_trees(tool, mesh_files):
    tri_path = mesh_files[0]
    default = hashes(tool, tri_path)
    assert hashes(tool, tri_path) == default  # the same bytes in another process
    assert len({default["old"], default["cost"], default["spatial"]}) == 3
    assert default["selected"] == default["cost"]
    assert hashes(tool, tri_path, PYRITE_SPATIAL_SPLITS="0")["selected"] == default["cost"]
    assert hashes(tool, tri_path, PYRITE_WIDE_COLLAPSE="greedy")["selected"] == default["old"]
    assert hashes(tool, tri_path, PYRITE_SPATIAL_SPLITS="1")["selected"] == default["spatial"]


def test_the_three_trees_of_the_sliver_mesh_are_the_pinned_ones(tool, mesh_files):
    with open(os.path.join(ROOT, "tests", "golden", "bvh_digests.json")) as f:
        pinned = json.load(f)["hash_sliver_mesh"]
    built = hashes(tool, mesh_files[0])
    assert {k: built[k] for k in ("old", "cost", "spatial")} == pinned
