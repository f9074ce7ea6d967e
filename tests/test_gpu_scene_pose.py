"""Posing a live scene's objects on the GPU (pyr_scene_set_objects / pyr_scene_pose / pyr_scene_geometry) --
run with `-m gpu` on an MI355X.

The geometry a pose leaves equals the numpy restatement (tests/pose_restatement.py) bit for bit: both sides are the same IEEE f32
operations with contraction off, and sqrt32 / rcp32 are bit-exact in the ranges used, so equality is the criterion. A posed scene
answers like a scene pyr_scene_update moved to those arrays; identity poses change nothing a ray can see; a rebuild pose IS the
scene created from the posed arrays; films of posed lamps match the oracle; refused poses leave the scene alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle  # noqa: E402
import pose_cases as cases  # noqa: E402
import pose_restatement as restatement  # noqa: E402
from test_gpu_bvh_build import assert_shapes_equal_up_to_ties  # noqa: E402
from test_gpu_parity import assert_parity  # noqa: E402
from test_gpu_scene_update import aimed_rays, counts_of, same_bits  # noqa: E402

from pyrite_amd import abi  # noqa: E402
from pyrite_amd._lib import PyriteGpuError, lib  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("positions", "normals", "frames", "spheres")
MOVING = [name for name in cases.ORDER if name != "identity"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_geometry_bits(got, want, what):
    for key in KEYS:
        if want[key] is None:
            assert got[key] is None, (what, key)
            continue
        differ = int((bits(got[key]) != bits(want[key])).sum())
        assert differ == 0, "%s: %d of %d words of %s differ from the restatement" % (what, differ, want[key].size, key)


def rays_at(arrays, n=20000):
    return aimed_rays(arrays["spheres"], arrays["positions"], n)


def update_to(world, arrays, mode="refit"):
    """pyr_scene_update, host form, with every array the description has."""
    given = {key: arrays[key] for key in KEYS if arrays[key] is not None and len(arrays[key])}
    world.update(mode=mode, **given)


# ---------------------------------------------------------------------------------------------------------------- 1. the arrays
@pytest.mark.parametrize("pose", cases.ORDER)
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_the_posed_geometry_is_the_restatements_bit_for_bit(gpu_lib, shape, pose):
    world, _, _, _, ranges = cases.build(shape)
    rest = cases.rest_of(world)
    poses = cases.poses_for(pose, len(ranges))
    world.pose(poses)
    want = restatement.pose_arrays(rest, ranges, poses)
    assert_geometry_bits(world.geometry(), want, "%s %s" % (shape, pose))
    if pose == "identity":
        assert_geometry_bits(world.geometry(), rest, "%s identity against rest" % shape)
    else:
        assert any(rest[k] is not None and rest[k].size and not np.array_equal(bits(rest[k]), bits(want[k])) for k in ("positions", "spheres"))
    info = world.update_info()
    assert info["mode_used"] == abi.PYR_UPDATE_REFIT and info["updates"] == 1
    assert_geometry_bits(cases.rest_of(world), rest, "World.flat stays the rest pose")
    world.close()


# ---------------------------------------------------------------------------------------------------------------- 2. identity
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_identity_poses_change_nothing_a_ray_can_see(gpu_lib, shape):
    world, _, _, _, ranges = cases.build(shape)
    rays = rays_at(cases.rest_of(world))
    h0, _, c0 = world.intersect(rays, want_counters=True)
    world.pose(cases.poses_for("identity", len(ranges)))
    h1, _, c1 = world.intersect(rays, want_counters=True)
    assert same_bits(h0, h1) and counts_of(c0) == counts_of(c1)
    assert (h0["shape"] != 0xFFFFFFFF).sum() > 1000
    assert world.update_info()["area_ratio"] == 1.0
    world.close()


# ---------------------------------------------------------------------------------------------------------------- 3. like an update
@pytest.mark.parametrize("pose", MOVING)
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_a_posed_scene_answers_like_a_scene_updated_to_the_restatements_arrays(gpu_lib, shape, pose):
    a, _, _, _, ranges = cases.build(shape)
    b, _, _, _, _ = cases.build(shape)
    rest = cases.rest_of(a)
    old_rays = rays_at(rest)
    h_old, _, c_old = a.intersect(old_rays, want_counters=True)
    poses = cases.poses_for(pose, len(ranges))
    want = restatement.pose_arrays(rest, ranges, poses)
    before = a.bvh_info()
    a.pose(poses)
    update_to(b, want)
    assert a.bvh_info() == before == b.bvh_info()
    rays = rays_at(want)
    ha, _, ca = a.intersect(rays, want_counters=True)
    hb, _, cb = b.intersect(rays, want_counters=True)
    assert np.array_equal(ha["distance"].view(np.uint32), hb["distance"].view(np.uint32))
    assert (hb["shape"] != 0xFFFFFFFF).sum() > 1000
    assert_shapes_equal_up_to_ties(b, hb, ha, rays)
    assert counts_of(ca) == counts_of(cb)
    assert a.update_info()["area_ratio"] == b.update_info()["area_ratio"]
    a.pose(cases.poses_for("identity", len(ranges)))  # and back: the first answers
    h_back, _, c_back = a.intersect(old_rays, want_counters=True)
    assert same_bits(h_old, h_back) and counts_of(c_old) == counts_of(c_back)
    assert a.update_info()["area_ratio"] == 1.0 and a.update_info()["updates"] == 2
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 4. from rest
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_poses_are_from_rest_never_from_the_previous_pose(gpu_lib, shape):
    a, _, _, _, ranges = cases.build(shape)
    b, _, _, _, _ = cases.build(shape)
    first, second = cases.poses_for("scaled_and_rotated", len(ranges)), cases.poses_for("rotated_and_translated", len(ranges))
    a.pose(first)
    a.pose(second)
    b.pose(second)
    assert_geometry_bits(a.geometry(), b.geometry(), "%s: pose(A) then pose(B) against pose(B)" % shape)
    a.pose({0: second[0]})  # objects a pose does not name keep the identity
    want = restatement.pose_arrays(cases.rest_of(a), ranges, {0: second[0]})
    assert_geometry_bits(a.geometry(), want, "%s: one object named" % shape)
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 5. rebuild
@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_a_rebuild_pose_is_the_scene_created_from_the_restatements_arrays(gpu_lib, shape, build):
    a, _, _, _, ranges = cases.build(shape)
    b, _, _, _, _ = cases.build(shape)
    rest = cases.rest_of(a)
    poses = cases.poses_for("rotated_and_translated", len(ranges))
    want = restatement.pose_arrays(rest, ranges, poses)
    for key, attr in (("positions", "tri_positions"), ("normals", "tri_normals"), ("frames", "tri_frames"), ("spheres", "spheres")):
        if want[key] is not None and len(want[key]):
            setattr(b.flat, attr, [want[key].copy()])
    b._desc = b.flat.desc()
    a.scene(0, build=build), b.scene(0, build=build)
    a.pose(poses, mode="rebuild")
    ia, ib = a.build_info(), b.build_info()
    for key in ("builder_asked", "builder_used", "fallback_reason", "levels", "median_splits", "tree_digest"):
        assert ia[key] == ib[key], key
    assert a.bvh_info() == b.bvh_info()
    rays = rays_at(want)
    ha, _, ca = a.intersect(rays, want_counters=True)
    hb, _, cb = b.intersect(rays, want_counters=True)
    assert same_bits(ha, hb) and counts_of(ca) == counts_of(cb)
    assert (hb["shape"] != 0xFFFFFFFF).sum() > 1000
    info = a.update_info()
    assert info["mode_used"] == abi.PYR_UPDATE_REBUILD and info["updates"] == 0 and info["area_ratio"] == 1.0
    assert_geometry_bits(a.geometry(), want, "%s rebuild" % shape)
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 6. lamps
def translation(x, y, z):
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = (x, y, z)
    return m


def about(centre, axis, angle):
    """The rotation about `centre`: T(c) R T(-c) as one float32 matrix."""
    r = cases.rotation4(axis, angle).astype(np.float64)
    c = np.asarray(centre, dtype=np.float64)
    r[:3, 3] = c - r[:3, :3] @ c
    return r.astype(np.float32)


def cornell_light_lowered(world):
    lamps = [index for _, index in cases.shape_lamps(world)]
    assert lamps == [32, 33]
    return [cases.triangles(32, 2)], {0: (translation(0.0, 0.0, -1.25), 1.0)}


def lamp_sphere_scaled(world):
    assert cases.shape_lamps(world) == [(abi.SHAPE_SPHERE, 7)]
    centre = cases.rest_of(world)["spheres"][7, :3].astype(np.float64)
    return [cases.sphere(7)], {0: (translation(*(-0.5 * centre)), 1.5)}  # grown by half where it hangs: its area changes


def cube_rotated(world):
    assert world.flat.uses_normal_maps
    objects = world.objects
    which = [k for k, o in enumerate(objects) if o["num_triangles"]]
    assert len(which) == 1
    o = objects[which[0]]
    centre = cases.rest_of(world)["positions"][o["first_triangle"]:o["first_triangle"] + o["num_triangles"]].reshape(-1, 3).astype(np.float64).mean(axis=0)
    return objects, {which[0]: (about(centre, (0.2, 0.3, 1.0), 0.4), 1.0)}


FILM_CASES = {
    "cornell_light_lowered": ("cornell", cornell_light_lowered),
    "lamp_sphere_scaled": ("three_spheres", lamp_sphere_scaled),
    "textures_cube_rotated": ("textures", cube_rotated),
}


@pytest.mark.parametrize("name", sorted(FILM_CASES))
def test_films_of_posed_lamps_match_the_oracle(gpu_lib, name):
    """The oracle renders a world created from the restatement's arrays; the GPU renders the scene created from the rest pose and
    posed, lamp records written on the device. Weights exact, every pixel within TOL, path counters equal."""
    shape, case = FILM_CASES[name]
    world, cam, r, gfilm, _ = cases.build(shape)
    ranges, poses = case(world)
    world.set_objects(ranges)
    rest = cases.rest_of(world)
    want = restatement.pose_arrays(rest, ranges, poses)
    fresh, _, _, _, _ = cases.build(shape)  # the posed description, never on the GPU
    for key, attr in (("positions", "tri_positions"), ("normals", "tri_normals"), ("frames", "tri_frames"), ("spheres", "spheres")):
        if want[key] is not None and len(want[key]):
            setattr(fresh.flat, attr, [want[key].copy()])
    fresh._desc = fresh.flat.desc()
    cfilm = r.new_film(gfilm.width, gfilm.height)
    ccount = oracle.OracleScene(fresh).render(r, cam, cfilm, threads=8)
    world.pose(poses)
    assert_geometry_bits(world.geometry(), want, name)
    gcount = r.render(gfilm, cam, world, counters=True)
    assert_parity(gfilm, cfilm)
    for key in ("samples", "extension_rays", "shadow_rays", "shaded_hits", "exposures"):
        assert gcount[key] == ccount[key], key
    assert cfilm.grains[..., 1].sum() > 0
    world.close()


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_a_pose_beyond_the_coordinate_range_is_refused_and_the_scene_stays(gpu_lib, mode):
    world, _, _, _, ranges = cases.build("knot")
    rest = cases.rest_of(world)
    rays = rays_at(rest)
    moved = cases.poses_for("rotated_and_translated", len(ranges))
    world.pose(moved)  # the scene is in a pose when the bad one arrives
    want = restatement.pose_arrays(rest, ranges, moved)
    h0, _, c0 = world.intersect(rays, want_counters=True)
    build, updates = world.build_info(), world.update_info()["updates"]
    with pytest.raises(PyriteGpuError) as err:
        world.pose({0: moved[0], 1: (translation(1e16, 0.0, 0.0), 1.0)}, mode=mode)
    assert err.value.status == abi.PYR_ERR_UNSUPPORTED and "1e15" in str(err.value)
    h1, _, c1 = world.intersect(rays, want_counters=True)
    assert same_bits(h0, h1) and counts_of(c0) == counts_of(c1)
    assert world.build_info() == build and world.update_info()["updates"] == updates
    assert_geometry_bits(world.geometry(), want, "the geometry did not move either")
    world.pose(cases.poses_for("identity", len(ranges)), mode=mode)  # and the scene still takes a good pose
    assert_geometry_bits(world.geometry(), rest, "back at rest")
    world.close()


def test_a_pose_under_a_live_session_is_refused(gpu_lib):
    world, cam, r, _, ranges = cases.build("cornell")
    with r.session((48, 48), cam, world) as session:
        session.render(2)
        for mode in ("refit", "rebuild"):
            with pytest.raises(PyriteGpuError) as err:
                world.pose(cases.poses_for("rotated_and_translated", len(ranges)), mode=mode)
            assert err.value.status == abi.PYR_ERR_INVALID_ARGUMENT and "PyrSession" in str(err.value)
        session.sync()
    world.pose(cases.poses_for("rotated_and_translated", len(ranges)))  # the session is gone: the pose goes through now
    world.close()


def test_objects_that_are_missing_overlap_or_reach_past_the_counts_are_refused(gpu_lib):
    world, _, _, _, ranges = cases.build("knot")
    world.scene(0)
    for bad, word in (([cases.triangles(0, 100), cases.triangles(99, 10)], "overlap"), ([cases.triangles(600, 53)], "past"), ([cases.sphere(0)], "past"),
                      ([cases.triangles(0xFFFFFFFF, 2)], "past")):
        with pytest.raises(PyriteGpuError) as err:
            world.set_objects(bad)
        assert err.value.status == abi.PYR_ERR_INVALID_ARGUMENT and word in str(err.value), bad
    assert world.objects == ranges  # a refused call leaves the objects
    world.pose(cases.poses_for("non_uniform", len(ranges)))
    world.set_objects([])  # forgets them
    with pytest.raises(PyriteGpuError) as err:
        world.pose({})
    assert err.value.status == abi.PYR_ERR_INVALID_ARGUMENT and "no objects" in str(err.value)
    world.close()


def test_the_argument_checks_that_need_a_scene(gpu_lib):
    """In pyrite_gpu.h's order: an unknown mode, a reserved word (update, then pose), the object count, NULL poses, an entry that is
    not finite, a last row that is not 0,0,0,1."""
    world, _, _, _, ranges = cases.build("knot")
    scene = world.scene(0)
    identity = (C.c_float * 16)(*[float(x) for x in restatement.IDENTITY])

    def records(n=2):
        r = (abi.PyrObjectPose * n)()
        for k in range(n):
            r[k].transform, r[k].scale = identity, 1.0
        return r

    good = records()
    reserved_pose, infinite, scale_nan, row = records(), records(), records(), records()
    reserved_pose[1].reserved[2] = 1
    infinite[1].transform[13] = float("inf")
    scale_nan[0].scale = float("nan")
    row[1].transform[7] = 0.5
    cases_ = [
        (abi.PyrPoseUpdate(mode=7, num_objects=2, poses=good), "mode"),
        (abi.PyrPoseUpdate(mode=abi.PYR_UPDATE_REFIT, num_objects=2, poses=good, reserved=(C.c_uint32 * 4)(0, 1, 0, 0)), "PyrPoseUpdate.reserved"),
        (abi.PyrPoseUpdate(mode=abi.PYR_UPDATE_REFIT, num_objects=2, poses=reserved_pose), "PyrObjectPose.reserved"),
        (abi.PyrPoseUpdate(mode=abi.PYR_UPDATE_REFIT, num_objects=3, poses=records(3)), "num_objects"),
        (abi.PyrPoseUpdate(mode=abi.PYR_UPDATE_REFIT, num_objects=2), "poses"),
        (abi.PyrPoseUpdate(mode=abi.PYR_UPDATE_REBUILD, num_objects=2, poses=infinite), "not finite"),
        (abi.PyrPoseUpdate(mode=abi.PYR_UPDATE_REBUILD, num_objects=2, poses=scale_nan), "scale"),
        (abi.PyrPoseUpdate(mode=abi.PYR_UPDATE_REFIT, num_objects=2, poses=row), "last row"),
    ]
    before = world.geometry()
    for update, word in cases_:
        assert lib().pyr_scene_pose(scene, C.byref(update), None) == abi.PYR_ERR_INVALID_ARGUMENT, word
        assert word in lib().pyr_last_error().decode(), (word, lib().pyr_last_error())
    assert lib().pyr_scene_pose(scene, C.byref(abi.PyrPoseUpdate(mode=abi.PYR_UPDATE_REFIT, num_objects=2, poses=good)), None) == abi.PYR_OK
    assert_geometry_bits(world.geometry(), before, "refused poses and an identity pose")
    world.close()


def test_an_update_with_arrays_forgets_the_objects(gpu_lib):
    world, _, _, _, ranges = cases.build("knot")
    rest = cases.rest_of(world)
    poses = cases.poses_for("rotated_and_translated", len(ranges))
    world.pose(poses)
    posed = world.geometry()
    world.update(mode="refit")  # no array: the geometry stays (the description is fetched from the device), and so do the objects
    assert_geometry_bits(world.geometry(), posed, "an update without arrays")
    world.pose(poses)
    world.update(positions=rest["positions"], mode="refit")  # new arrays are a new geometry, not a pose of the old one
    with pytest.raises(PyriteGpuError) as err:
        world.pose(poses)
    assert err.value.status == abi.PYR_ERR_INVALID_ARGUMENT and "no objects" in str(err.value)
    got = world.geometry()
    assert np.array_equal(bits(got["positions"]), bits(rest["positions"])) and np.array_equal(bits(got["normals"]), bits(posed["normals"]))  # what the update left out stayed
    world.set_objects(ranges)  # named again: the rest pose is the geometry as it is now
    world.pose(poses)
    now = {"positions": rest["positions"], "normals": posed["normals"], "frames": None, "spheres": rest["spheres"]}
    assert_geometry_bits(world.geometry(), restatement.pose_arrays(now, ranges, poses), "posed from the newly captured rest pose")
    world.close()


@pytest.mark.parametrize("shape", ["knot", "textures"])
def test_a_walk_through_every_way_to_move_a_scene(gpu_lib, shape):
    """One world through poses, updates from the host and from the device, rebuilds and set_objects in a row: after every step
    World.geometry() is the numpy expectation bit for bit, and at the end the scene answers like one created from the final arrays."""
    import torch

    world, _, _, _, ranges = cases.build(shape)
    rest = cases.rest_of(world)
    p1, p2 = cases.poses_for("rotated_and_translated", len(ranges)), cases.poses_for("scaled_and_rotated", len(ranges))

    def at(step, want, mode, updates):
        assert_geometry_bits(world.geometry(), want, "%s step %d" % (shape, step))
        info = world.update_info()
        assert (info["mode_used"], info["updates"]) == (mode, updates), (step, info)

    def the_objects_are_forgotten():
        with pytest.raises(PyriteGpuError) as err:
            world.pose(p1)
        assert err.value.status == abi.PYR_ERR_INVALID_ARGUMENT and "no objects" in str(err.value)

    world.pose(p1)  # 1
    g1 = restatement.pose_arrays(rest, ranges, p1)
    at(1, g1, abi.PYR_UPDATE_REFIT, 1)
    world.update(mode="rebuild")  # 2: no array -- the geometry and the objects stay, the tree is new
    at(2, g1, abi.PYR_UPDATE_REBUILD, 0)
    world.pose(p2)  # 3: from rest, on the rebuilt tree (its schedule is made again)
    g3 = restatement.pose_arrays(rest, ranges, p2)
    at(3, g3, abi.PYR_UPDATE_REFIT, 1)
    normals = restatement.pose_arrays(rest, ranges, cases.poses_for("non_uniform", len(ranges)))["normals"]
    world.update(normals=normals, mode="refit")  # 4: from the host -- the positions the pose left stay
    g4 = dict(g3, normals=normals)
    at(4, g4, abi.PYR_UPDATE_REFIT, 2)
    the_objects_are_forgotten()
    world.update(mode="refit")  # 5: no array -- the positions are staged from the description
    at(5, g4, abi.PYR_UPDATE_REFIT, 3)
    world.set_objects(ranges)  # 6: the rest pose is the geometry as it is now
    world.pose(p1, mode="rebuild")
    g6 = restatement.pose_arrays(g4, ranges, p1)
    at(6, g6, abi.PYR_UPDATE_REBUILD, 0)
    positions = restatement.pose_arrays(g6, ranges, p2)["positions"]
    world.update(positions=torch.from_numpy(positions).to("cuda:0"), mode="refit")  # 7: the device form
    final = dict(g6, positions=positions)
    at(7, final, abi.PYR_UPDATE_REFIT, 1)
    the_objects_are_forgotten()
    world.set_objects([])  # 8
    at(8, final, abi.PYR_UPDATE_REFIT, 1)

    fresh, _, _, _, _ = cases.build(shape)
    for key, attr in (("positions", "tri_positions"), ("normals", "tri_normals"), ("frames", "tri_frames"), ("spheres", "spheres")):
        if final[key] is not None and len(final[key]):
            setattr(fresh.flat, attr, [final[key].copy()])
    fresh._desc = fresh.flat.desc()
    rays = rays_at(final)
    hf = fresh.intersect(rays)[0]
    hits = int((hf["shape"] != 0xFFFFFFFF).sum())
    print("%s: %d of %d rays hit the scene created from the final arrays" % (shape, hits, len(rays)))
    assert hits > 1000
    hw = world.intersect(rays)[0]
    assert np.array_equal(hw["distance"].view(np.uint32), hf["distance"].view(np.uint32))
    assert int((hw["shape"] != 0xFFFFFFFF).sum()) == hits
    assert_shapes_equal_up_to_ties(fresh, hf, hw, rays)
    world.close(), fresh.close()


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_the_cpp_world_poses_like_the_restatement(gpu_lib, tmp_path, mode):
    """pyrite::World::pose and geometry() through pyrite_host_tool on the textures scene (frames, spheres, a lamp sphere)."""
    from test_host_cpp import HOST_TOOL, SCENES, data_dir_for
    from pyrite_amd.compiler import DATA_DIR, FlatScene
    from pyrite_amd.renderer import World

    world = World(FlatScene().add_world(SCENES["textures"]()["world"], DATA_DIR))
    rest, ranges = cases.rest_of(world), world.objects
    poses = cases.poses_for("scaled_and_rotated", len(ranges))
    records = np.concatenate([np.concatenate([restatement.column_major(poses[k][0]), np.float32([poses[k][1]])]) for k in range(len(ranges))]).astype("<f4")
    source, result = str(tmp_path / "poses.f32"), str(tmp_path / "geometry.f32")
    records.tofile(source)
    subprocess.check_call([HOST_TOOL, "pose", "textures", data_dir_for("textures", tmp_path), source, result, mode], stdout=subprocess.DEVNULL)
    want = restatement.pose_arrays(rest, ranges, poses)
    got = np.fromfile(result, dtype="<f4")
    expected = np.concatenate([want[key].reshape(-1) for key in KEYS])
    assert got.size == expected.size and np.array_equal(got.view(np.uint32), expected.view(np.uint32))


CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import pose_cases as cases, pose_restatement as restatement
from test_gpu_scene_update import aimed_rays, same_bits
from pyrite_amd import scenes
from pyrite_amd._lib import PyriteGpuError
def make():
    world, _, _, _ = scenes.build(scenes.c3_mesh_in_box(64, 36, 8, segments=96, sides=24), seed=5)
    world.set_objects([cases.triangles(12, 2 * 96 * 24)])
    return world
a, b = make(), make()
poses = {0: cases.POSES["rotated_and_translated"]}
want = restatement.pose_arrays(cases.rest_of(a), a.objects, poses)
b.flat.tri_positions, b.flat.tri_normals = [want["positions"].copy()], [want["normals"].copy()]
b._desc = b.flat.desc()
a.scene(0), b.scene(0)
try:
    a.pose(poses, mode="refit")
    print("REFIT went through")
except PyriteGpuError as e:
    print("REFIT", e.status)
a.pose(poses, mode="rebuild")
rays = aimed_rays(want["spheres"], want["positions"], 20000)
ha, hb = a.intersect(rays)[0], b.intersect(rays)[0]
print("REBUILD", int(a.build_info()["tree_digest"] == b.build_info()["tree_digest"]), int(a.bvh_info() == b.bvh_info()), int(same_bits(ha, hb)), int((hb["shape"] != 0xFFFFFFFF).sum()))
"""


def test_a_tree_with_spatial_splits_refuses_the_refit_pose_and_takes_the_rebuild_pose(gpu_lib):
    """PYRITE_SPATIAL_SPLITS is read when a tree is built: a fresh child process, so that nothing else in this one sees it (the way
    tests/test_gpu_scene_update.py sets it). A knot of 4,608 triangles: large enough for the pair tree, which is the one that splits."""
    run = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=dict(os.environ, PYRITE_SPATIAL_SPLITS="1", PYTHONPATH=ROOT),
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert "REFIT %d" % abi.PYR_ERR_UNSUPPORTED in lines, run.stdout
    rebuilt = [l.split() for l in lines if l.startswith("REBUILD")][0]
    assert rebuilt[1:4] == ["1", "1", "1"] and int(rebuilt[4]) > 1000, run.stdout
