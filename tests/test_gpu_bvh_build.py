"""The BVH built on the device (pyr_scene_create_with, PYR_BUILD_DEVICE) against the host builder's -- run
with `-m gpu` on an MI355X. The inputs are those of tests/test_bvh_device_cpu.py (tests/bvh_build_inputs.py).

Tie-free inputs: the device builds the host's tree -- equal digest (the one tests/golden/bvh_digests.json pins), equal PyrBvhInfo, hits equal bit for bit, equal traversal
counts. Fallback inputs (a node needs the median rule, where the two builders may break ties differently): equal hit distances bit
for bit, and equal shapes except where the oracle's own intersection routine says both primitives are hit at that very distance.
The command lines compare PNG files byte for byte: the 8-bit image of a fixed seed does not move with the order of the film's
float atomics in any test of this suite (tests/test_gpu_session.py compares the same way), and here the trees are equal too."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_build_inputs as inputs  # noqa: E402
from test_gpu_parity import TOL, primitive_distance, rel_l2  # noqa: E402

from pyrite_amd import abi, scenes  # noqa: E402
from pyrite_amd import build as gpu_build  # noqa: E402
from pyrite_amd.compiler import FlatScene  # noqa: E402
from pyrite_amd.project import material, shape, vector  # noqa: E402
from pyrite_amd.renderer import World  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "bvh_digests.json")) as f:
    PINS = json.load(f)


def world_of(spheres, tris):
    flat = FlatScene()
    grey = {"surface": material.diffuse(color=0.8)}
    flat.add_world({"objects": [shape.sphere(position=vector(float(s[0]), float(s[1]), float(s[2])), radius=float(s[3]), material=grey) for s in spheres]})
    if len(tris):
        mat, _ = flat.add_material(grey)
        t = tris.reshape(-1, 3, 3)
        n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
        flat.add_triangles(t, np.repeat(n[:, None, :], 3, axis=1), mat)
    return World(flat)


def rays_into(spheres, tris, n, seed=9):
    o, d, _ = inputs.rays_for(spheres, tris, n=n, seed=seed)
    return np.concatenate([o[:n], d[:n]], axis=1).astype(np.float32)


def built_pair(name, group):
    spheres, tris = group[name]()
    host, device = world_of(spheres, tris), world_of(spheres, tris)
    host.scene(0, build="host")
    device.scene(0, build="device")
    return spheres, tris, host, device


@pytest.mark.parametrize("name", sorted(inputs.TIE_FREE))
def test_tie_free_inputs_get_the_host_builders_tree(gpu_lib, name):
    """"spheres", "tri1" .. "tri65" live in LDS; "sliver_mesh" (4,612 triangles) is shared by several workgroups at the top and
    handled one node per wave below: both paths of the builder."""
    spheres, tris, host, device = built_pair(name, inputs.TIE_FREE)
    h, d = host.build_info(), device.build_info()
    assert h["builder_asked"] == h["builder_used"] == abi.PYR_BUILD_HOST and h["fallback_reason"] == 0 and h["median_splits"] == 0
    assert d["builder_asked"] == d["builder_used"] == abi.PYR_BUILD_DEVICE and d["fallback_reason"] == 0 and d["median_splits"] == 0
    assert d["tree_digest"] == h["tree_digest"]
    assert "%016x" % d["tree_digest"] == PINS["level_tie_free"][name]["levelwise"]
    assert device.bvh_info() == host.bvh_info()
    rays = rays_into(spheres, tris, 20000)
    hh, _, hc = host.intersect(rays, want_counters=True)
    dh, _, dc = device.intersect(rays, want_counters=True)
    for field in ("distance", "shape", "u", "v"):
        assert np.array_equal(hh[field].view(np.uint32), dh[field].view(np.uint32)), field
    assert (hc["box_tests"], hc["triangle_tests"], hc["sphere_tests"]) == (dc["box_tests"], dc["triangle_tests"], dc["sphere_tests"])
    if name in ("sliver_mesh", "spheres", "mixed"):
        assert (hh["shape"] != 0xFFFFFFFF).sum() > 1000  # the rays exercise the tree


@pytest.mark.parametrize("name", sorted(inputs.FALLBACK))
def test_fallback_inputs_get_a_tree_with_the_same_hits(gpu_lib, name):
    spheres, tris, host, device = built_pair(name, inputs.FALLBACK)
    d = device.build_info()
    assert d["builder_used"] == abi.PYR_BUILD_DEVICE and d["fallback_reason"] == 0
    assert d["median_splits"] > 0 and host.build_info()["median_splits"] > 0
    rays = rays_into(spheres, tris, 20000)
    hh, _, _ = host.intersect(rays)
    dh, _, _ = device.intersect(rays)
    assert np.array_equal(hh["distance"].view(np.uint32), dh["distance"].view(np.uint32))
    assert (hh["shape"] != 0xFFFFFFFF).sum() > 100
    assert_shapes_equal_up_to_ties(host, hh, dh, rays)


def assert_shapes_equal_up_to_ties(world, hh, dh, rays):
    """Every ray whose two shapes differ is a tie by the oracle's own routine: both primitives are hit at exactly the reported distance."""
    for i in np.nonzero(hh["shape"] != dh["shape"])[0]:
        for hits in (hh, dh):
            hit, dist, _, _ = primitive_distance(world, hits["shape"][i], rays[i])
            assert hit and dist == hits["distance"][i], "ray %d: shapes differ without a tie" % i
    same = hh["shape"] == dh["shape"]
    assert np.array_equal(hh["u"][same].view(np.uint32), dh["u"][same].view(np.uint32)) and np.array_equal(hh["v"][same].view(np.uint32), dh["v"][same].view(np.uint32))


def test_the_median_rule_of_a_large_node_runs_in_its_own_kernel(gpu_lib):
    """300 coincident triangles: nodes of 300, 150 and 75 references are split by the median rule one workgroup each (the bins cannot
    separate them and they are more than a wave's worth); every split of this input is a median split. The scene's creation
    validates that the leaves name every primitive once."""
    _, _, host, device = built_pair("coincident300", inputs.FALLBACK)
    d = device.build_info()
    assert d["builder_used"] == abi.PYR_BUILD_DEVICE and d["fallback_reason"] == 0
    assert d["median_splits"] == device.bvh_info()["num_nodes"] == host.bvh_info()["num_nodes"]  # the root node included
    assert device.bvh_info() == host.bvh_info()  # the same shape: halves of halves


def test_a_median_node_too_large_for_the_device_is_built_on_the_host(gpu_lib):
    spheres, tris, host, device = built_pair("coincident3000", inputs.TOO_LARGE)
    h, d = host.build_info(), device.build_info()
    assert d["builder_asked"] == abi.PYR_BUILD_DEVICE and d["builder_used"] == abi.PYR_BUILD_HOST
    assert d["fallback_reason"] == abi.PYR_BUILD_FALLBACK_MEDIAN_TOO_LARGE and d["levels"] == 0
    assert d["tree_digest"] == h["tree_digest"] and d["median_splits"] == h["median_splits"] > 0  # the host builder's tree
    assert device.bvh_info() == host.bvh_info()
    rays = rays_into(spheres, tris, 20000)
    hh, _, _ = host.intersect(rays)
    dh, _, _ = device.intersect(rays)
    assert hh.tobytes() == dh.tobytes() and (hh["shape"] != 0xFFFFFFFF).sum() > 100


def test_a_render_on_a_device_built_scene_is_the_host_built_scenes(gpu_lib):
    films = {}
    for build in ("host", "device"):
        world, cam, r, film = scenes.build(scenes.c2_cornell(64, 48, 8), seed=5)
        world.scene(0, build=build)
        assert world.build_info()["builder_used"] == (abi.PYR_BUILD_DEVICE if build == "device" else abi.PYR_BUILD_HOST)
        r.render(film, cam, world)
        films[build] = film
    assert np.array_equal(films["device"].grains[..., 1], films["host"].grains[..., 1]), "film weights differ"
    assert films["host"].grains[..., 1].sum() > 0
    worst = float(rel_l2(films["device"], films["host"]).max())
    assert worst <= TOL, "relL2 max %.3g" % worst


def test_two_device_builds_in_one_process_are_the_same(gpu_lib):
    spheres, tris = inputs.TIE_FREE["sliver_mesh"]()
    rays = rays_into(spheres, tris, 20000)
    seen = []
    for _ in range(2):
        world = world_of(spheres, tris)
        world.scene(0, build="device")
        info = world.build_info()
        assert info["builder_used"] == abi.PYR_BUILD_DEVICE
        hits, _, _ = world.intersect(rays)
        seen.append((info["tree_digest"], info["levels"], world.bvh_info(), hits.tobytes()))
        world.close()
    assert seen[0] == seen[1]


CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import bvh_build_inputs as inputs
from test_gpu_bvh_build import world_of
world = world_of(*inputs.TIE_FREE["sliver_mesh"]())
world.scene(0, build="device")
b = world.build_info()
print("INFO", b["builder_asked"], b["builder_used"], b["fallback_reason"], world.bvh_info()["num_primitives"])
"""


def test_spatial_splits_are_built_on_the_host_and_the_info_says_so(gpu_lib):
    """PYRITE_SPATIAL_SPLITS is read at scene creation: a fresh child process, so that nothing else in this one sees it."""
    run = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=dict(os.environ, PYRITE_SPATIAL_SPLITS="1", PYTHONPATH=ROOT),
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    fields = [line.split() for line in run.stdout.splitlines() if line.startswith("INFO")][0]
    assert [int(x) for x in fields[1:4]] == [abi.PYR_BUILD_DEVICE, abi.PYR_BUILD_HOST, abi.PYR_BUILD_FALLBACK_SPATIAL_SPLITS]
    assert int(fields[4]) == 4612


def test_both_command_lines_write_the_same_png_with_either_builder(gpu_lib, tmp_path):
    project = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    env = dict(os.environ, PYTHONPATH=ROOT)
    png = {}
    for build in ("host", "device"):
        out = str(tmp_path / ("py_%s.png" % build))
        run = subprocess.run([sys.executable, "-m", "pyrite_amd", project, "--seed", "7", "--spp", "8", "--size", "96x64", "-o", out, "--build", build], cwd=ROOT, env=env,
                             capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stdout + run.stderr
        assert "build: asked %s, used %s" % (build, build) in run.stderr
        png["py", build] = open(out, "rb").read()
        out = str(tmp_path / ("cpp_%s.png" % build))
        run = subprocess.run([gpu_build.HOST_TOOL, "render-project", project, "-", "7", out, "--spp", "8", "--size", "96x64", "--build", build], cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stdout + run.stderr
        assert "build: asked %s, used %s" % (build, build) in run.stderr
        png["cpp", build] = open(out, "rb").read()
    assert png["py", "device"] == png["py", "host"] and png["cpp", "device"] == png["cpp", "host"]
    assert len(png["py", "host"]) > 1000
