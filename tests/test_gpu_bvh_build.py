"""The BVH built on the device (pyr_scene_create_with, PYR_BUILD_DEVICE) against the host builder's -- run
with `-m gpu` on an MI355X. The inputs are those of tests/test_bvh_device_cpu.py (tests/bvh_build_inputs.py).

Every tree the device builds is the rehearsal's (build_bvh_levelwise), medians included: its digest, median splits and levels are
the ones tests/golden/bvh_digests.json pins, and tests/test_bvh_device_cpu.py proves on the CPU which path of the builder each
input reaches (the median over distinct centroids in either kernel, the depth rule, chunk and wave edges, a level of more large
nodes than one workgroup chooses, degenerate axes, signed zeros, huge and subnormal coordinates).
Tie-free inputs: that is the host's tree too -- equal PyrBvhInfo, hits equal bit for bit, equal traversal
counts. Fallback inputs (a node needs the median rule, where the two builders may break ties differently): equal hit distances bit
for bit, and equal shapes except where the oracle's own intersection routine says both primitives are hit at that very distance.
The inputs at the builder's edges are held to the oracle's hits as well, and the deep trees of the depth rule to the oracle's
films, with the traversal stack spilled past its LDS part by real depth.
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
import oracle  # noqa: E402
from test_gpu_parity import TOL, assert_parity, assert_same_hits, primitive_distance, rel_l2  # noqa: E402

from pyrite_amd import abi, scenes  # noqa: E402
from pyrite_amd import build as gpu_build  # noqa: E402
from pyrite_amd.compiler import FlatScene  # noqa: E402
from pyrite_amd.project import material, shape, vector  # noqa: E402
from pyrite_amd.renderer import World  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "bvh_digests.json")) as f:
    PINS = json.load(f)


def world_of(spheres, tris, sky=None):
    flat = FlatScene()
    grey = {"surface": material.diffuse(color=0.8)}
    flat.add_world({"sky": sky, "objects": [shape.sphere(position=vector(float(s[0]), float(s[1]), float(s[2])), radius=float(s[3]), material=grey) for s in spheres]})
    if len(tris):
        mat, _ = flat.add_material(grey)
        t = tris.reshape(-1, 3, 3)
        e = t.astype(np.float64)  # (the cross product of a triangle of 1e-30 underflows in float32)
        n = np.cross(e[:, 1] - e[:, 0], e[:, 2] - e[:, 0])
        n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
        flat.add_triangles(t, np.repeat(n[:, None, :], 3, axis=1).astype(np.float32), mat)
    return World(flat)


rays_into = inputs.rays_into


def assert_the_rehearsals_tree(info, name):
    """The device built it, and it is build_bvh_levelwise's tree: the pinned digest, median splits and levels (both builders count the
    iterations of their level loop; none for a scene that is a single leaf)."""
    group = "level_tie_free" if name in inputs.TIE_FREE else "level_fallback" if name in inputs.FALLBACK else "level_depth_rule"
    assert info["builder_asked"] == info["builder_used"] == abi.PYR_BUILD_DEVICE and info["fallback_reason"] == 0
    assert "%016x" % info["tree_digest"] == PINS[group][name]["levelwise"]
    assert {"medians": info["median_splits"], "levels": info["levels"]} == PINS["level_counts"][name]


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
    assert_the_rehearsals_tree(d, name)
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
    assert_the_rehearsals_tree(d, name)  # both rank by median_before: the rehearsal's tree, digest for digest
    rays = rays_into(spheres, tris, 20000)
    hh, _, _ = host.intersect(rays)
    dh, _, _ = device.intersect(rays)
    assert np.array_equal(hh["distance"].view(np.uint32), dh["distance"].view(np.uint32))
    assert (hh["shape"] != 0xFFFFFFFF).sum() > 100 or name in inputs.UNHITTABLE
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


# ------------------------------------------------------------------------------------------------- the builder's edges
@pytest.mark.parametrize("name", [n for n in inputs.EDGES if n not in inputs.DEPTH_RULE and n != "tri40000"])
def test_edge_inputs_answer_like_the_oracle_on_a_device_built_scene(gpu_lib, name):
    """The host-built scene is not the only witness: closest hits of 20,000 rays against the oracle's, ties proven."""
    spheres, tris = inputs.group_of(name)[name]()
    world = world_of(spheres, tris)
    world.scene(0, build="device")
    assert_the_rehearsals_tree(world.build_info(), name)
    rays = inputs.rays_of(name, spheres, tris)
    ohits, _ = oracle.OracleScene(world).intersect(rays)
    ghits, _, _ = world.intersect(rays)
    ties = assert_same_hits(ohits, ghits, world, rays)
    print("%s: %d of %d rays hit, %d ties" % (name, (ohits["shape"] != 0xFFFFFFFF).sum(), len(rays), ties))
    assert (ghits["shape"] != 0xFFFFFFFF).sum() >= 1000 or name in inputs.UNHITTABLE
    world.close()


def test_forty_thousand_triangles_are_chosen_by_more_than_one_workgroup(gpu_lib):
    """tri40000 has levels of several hundred large nodes (choose_large_kernel decides 64 per workgroup) and a root of 20 chunks:
    the rehearsal's tree, and the host-built scene's hits and traversal counts on rays that hit."""
    spheres, tris, host, device = built_pair("tri40000", inputs.TIE_FREE)
    assert_the_rehearsals_tree(device.build_info(), "tri40000")
    assert device.bvh_info() == host.bvh_info()
    rays = inputs.rays_of("tri40000", spheres, tris)
    hh, _, hc = host.intersect(rays, want_counters=True)
    dh, _, dc = device.intersect(rays, want_counters=True)
    assert hh.tobytes() == dh.tobytes() and (hh["shape"] != 0xFFFFFFFF).sum() >= 1000
    assert (hc["box_tests"], hc["triangle_tests"], hc["sphere_tests"]) == (dc["box_tests"], dc["triangle_tests"], dc["sphere_tests"])


# ------------------------------------------------------------------------------------------------- the depth rule
def chain_world(name, build, sky=None):
    spheres, tris = inputs.DEPTH_RULE[name]()
    world = world_of(spheres, tris, sky=sky)
    world.scene(0, build=build)
    return spheres, tris, world


def assert_chain_tree(world, name):
    """chain300, chain300_r4: the device's median kernel ranked distinct centroids at the depth rule's node; the scene walks its
    four-wide tree. chain3000: that node is larger than the kernel ranks, the host built, and the four-wide tree, whose stack need
    is beyond the kernels', is dropped for the binary one."""
    info, bvh = world.build_info(), world.bvh_info()
    assert bvh["max_depth"] == 39
    if name == "chain3000":
        assert info["builder_asked"] == abi.PYR_BUILD_DEVICE and info["builder_used"] == abi.PYR_BUILD_HOST
        assert info["fallback_reason"] == abi.PYR_BUILD_FALLBACK_MEDIAN_TOO_LARGE and info["levels"] == 0
        assert bvh["num_wide_nodes"] == bvh["num_pair_records"] == 0 and bvh["wide_node_bytes"] == 0 and bvh["num_nodes"] > 1000
    else:
        assert_the_rehearsals_tree(info, name)
        assert bvh["num_wide_nodes"] > 0
    return info


@pytest.mark.parametrize("name", sorted(inputs.DEPTH_RULE))
def test_deep_trees_answer_like_the_oracle_whatever_part_of_the_stack_is_in_lds(gpu_lib, name, monkeypatch):
    """20,000 rays aimed at the triangles a ray can hit and 2,000 through the small end, which every padded box of the chain holds:
    a walk 39 levels down pushes past the LDS part of its stack with real depth. One LDS level, and the default: the same bits."""
    spheres, tris, world = chain_world(name, "device")
    info = assert_chain_tree(world, name)
    rays = inputs.rays_of(name, spheres, tris)
    assert len(rays) == 22000
    ohits, _ = oracle.OracleScene(world).intersect(rays)
    ghits, _, _ = world.intersect(rays)
    ties = assert_same_hits(ohits, ghits, world, rays)
    print("%s: %d of %d rays hit, %d ties, build_info %r" % (name, (ohits["shape"] != 0xFFFFFFFF).sum(), len(rays), ties, info))
    assert (ghits["shape"] != 0xFFFFFFFF).sum() >= 1000
    monkeypatch.setenv("PYRITE_LDS_STACK", "1")
    short, _, _ = world.intersect(rays)
    assert short.tobytes() == ghits.tobytes()
    monkeypatch.delenv("PYRITE_LDS_STACK")
    host = world_of(spheres, tris)
    host.scene(0, build="host")
    assert host.build_info()["tree_digest"] == info["tree_digest"]  # distinct centroids: nth_element has no tie to break its own way
    hh, _, _ = host.intersect(rays)
    assert hh.tobytes() == ghits.tobytes()
    host.close(), world.close()


def chain_view(tris):
    """Straight at the chain's triangle of a size nearest 100, from 1.5 sizes off its plane: it fills a good part of the view, the
    sky the rest, and every ray runs inside the padded boxes of all the smaller links and of the cluster (the padding, 16 ulps of
    the chain's top, is 2e6)."""
    from pyrite_amd.project import camera, transform
    from pyrite_amd.renderer import Camera

    t = tris.reshape(-1, 3, 3).astype(np.float64)
    size = np.linalg.norm(t.max(axis=1) - t.min(axis=1), axis=1)
    k = int(np.argmin(np.abs(np.log(size / 100.0))))
    n = np.cross(t[k, 1] - t[k, 0], t[k, 2] - t[k, 0])
    centre, eye = t[k].mean(axis=0), t[k].mean(axis=0) + 1.5 * size[k] * n / np.linalg.norm(n)
    up = np.cross(n, [1.0, 0.3, 0.2])
    return Camera.from_project(camera.perspective(fov=40.0, transform=transform.look_at(**{"from": vector(*eye), "to": vector(*centre), "up": vector(*(up / np.linalg.norm(up)))})))


@pytest.mark.parametrize("name", sorted(inputs.DEPTH_RULE))
def test_a_render_of_a_deep_tree_matches_the_oracles_film(gpu_lib, name):
    from pyrite_amd.project import renderer as project_renderer
    from pyrite_amd.renderer import Renderer

    _, tris, world = chain_world(name, "device", sky=1.0)
    assert_chain_tree(world, name)
    r, cam = Renderer.from_project(project_renderer.simple(pixel_samples=4), seed=3), chain_view(tris)
    gfilm, cfilm = r.new_film(32, 24), r.new_film(32, 24)
    ccount = oracle.OracleScene(world).render(r, cam, cfilm, threads=8)
    gcount = r.render(gfilm, cam, world, counters=True)
    assert_parity(gfilm, cfilm)
    for key in ("samples", "extension_rays", "shadow_rays", "shaded_hits", "exposures"):
        assert gcount[key] == ccount[key], key
    assert 100 < ccount["shaded_hits"] and ccount["samples"] == 32 * 24 * 4  # paths bounce off the chain under the sky
    world.close()


def test_feature_and_motion_passes_of_a_deep_tree_are_the_host_built_scenes(gpu_lib):
    """features_kernel and motion_kernel carry scratch stacks of their own."""
    from pyrite_amd.project import renderer as project_renderer
    from pyrite_amd.renderer import Renderer

    r, cam = Renderer.from_project(project_renderer.simple(pixel_samples=4), seed=3), chain_view(inputs.DEPTH_RULE["chain300"]()[1])
    seen = {}
    for build in ("host", "device"):
        _, _, world = chain_world("chain300", build, sky=1.0)
        f = r.features((32, 24), cam, world)
        seen[build] = (f.albedo.grains.tobytes(), f.records.tobytes(), r.motion((32, 24), cam, world).tobytes())
        if build == "device":
            assert_chain_tree(world, "chain300")
            assert 0 < (f.records["shape"] != 0xFFFFFFFF).sum() < f.records["shape"].size  # the view holds triangles and sky
        world.close()
    assert seen["host"] == seen["device"]


def test_an_identity_refit_of_the_binary_tree_of_chain3000_changes_nothing(gpu_lib):
    from test_gpu_scene_update import counts_of, same_bits, update_world

    spheres, tris, world = chain_world("chain3000", "device")
    assert_chain_tree(world, "chain3000")
    rays = inputs.rays_of("chain3000", spheres, tris)
    h0, _, c0 = world.intersect(rays, want_counters=True)
    update_world(world, spheres, tris)
    h1, _, c1 = world.intersect(rays, want_counters=True)
    assert same_bits(h0, h1) and counts_of(c0) == counts_of(c1) and (h0["shape"] != 0xFFFFFFFF).sum() >= 1000
    assert world.update_info()["mode_used"] == abi.PYR_UPDATE_REFIT and world.update_info()["area_ratio"] == 1.0
    world.close()


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
