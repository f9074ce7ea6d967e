"""Skinning a live scene's meshes on the GPU (pyr_scene_set_skins / pyr_scene_skin) -- run with `-m gpu` on an
MI355X.

The geometry a frame leaves equals the numpy restatement (tests/skin_restatement.py) bit for bit: both sides are the same IEEE f32
operations with contraction off, and sqrt32 / rcp32 are bit-exact in the ranges used, so equality is the criterion. A skinned scene
answers like a scene pyr_scene_update moved to those arrays; a frame is from rest, never from the previous one; a rebuild frame IS
the scene created from the skinned arrays; films of bent lamps and bent normal maps match the oracle; refused calls leave the scene
and its skins alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle  # noqa: E402
import pose_cases as cases  # noqa: E402
import pose_restatement  # noqa: E402
import skin_cases  # noqa: E402
import skin_restatement as restatement  # noqa: E402
from test_gpu_bvh_build import assert_shapes_equal_up_to_ties  # noqa: E402
from test_gpu_parity import assert_parity  # noqa: E402
from test_gpu_scene_pose import about, assert_geometry_bits, bits, rays_at, translation, update_to  # noqa: E402
from test_gpu_scene_update import counts_of, same_bits  # noqa: E402

from pyrite_amd import abi  # noqa: E402
from pyrite_amd._lib import PyriteGpuError, lib  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("positions", "normals", "frames", "spheres")
THREE = skin_cases.THREE
OTHER = THREE[::-1].copy()  # another frame of the same three joints


def the_skin(skins):
    (index, skin), = skins.items()
    return index, skin


def into_description(world, arrays):
    for key, attr in (("positions", "tri_positions"), ("normals", "tri_normals"), ("frames", "tri_frames"), ("spheres", "spheres")):
        if arrays[key] is not None and len(arrays[key]):
            setattr(world.flat, attr, [arrays[key].copy()])
    world._desc = world.flat.desc()


# ---------------------------------------------------------------------------------------------------------------- 1. the arrays
@pytest.mark.parametrize("pose", ["identity", "rotated_and_translated"])
@pytest.mark.parametrize("binding", skin_cases.BINDINGS)
@pytest.mark.parametrize("shape", skin_cases.SHAPES)
def test_the_skinned_geometry_is_the_restatements_bit_for_bit(gpu_lib, shape, binding, pose):
    world, _, _, _, ranges, rest, skins = skin_cases.build(shape, binding)
    index, _ = the_skin(skins)
    joints, poses = {index: THREE}, skin_cases.object_poses(pose, len(ranges))
    world.skin(joints, poses=poses)
    want = restatement.skin_arrays(rest, ranges, skins, joints, poses)
    what = "%s %s %s" % (shape, binding, pose)
    assert_geometry_bits(world.geometry(), want, what)
    assert not np.array_equal(bits(rest["positions"]), bits(want["positions"]))
    info = world.update_info()
    assert info["mode_used"] == abi.PYR_UPDATE_REFIT and info["updates"] == 1
    if binding == "one_hot" and pose == "identity":  # B is J[0] exactly: the rigid pose by J[0], through the pose kernel of a second world
        rigid, _, _, _, _ = cases.build(shape)
        rigid.pose({index: (THREE[0], 1.0)})
        assert_geometry_bits(world.geometry(), rigid.geometry(), what + " against World.pose")
        rigid.close()
    world.skin({}, poses={})  # the identity table, every pose the identity
    assert_geometry_bits(world.geometry(), rest, what + ": the identity table against rest")
    assert_geometry_bits(cases.rest_of(world), rest, "World.flat stays the rest pose")
    world.close()


# ---------------------------------------------------------------------------------------------------------------- 2. like an update
@pytest.mark.parametrize("shape", skin_cases.SHAPES)
def test_a_skinned_scene_answers_like_a_scene_updated_to_the_restatements_arrays(gpu_lib, shape):
    a, _, _, _, ranges, rest, skins = skin_cases.build(shape)
    b, _, _, _, _ = cases.build(shape)
    index, _ = the_skin(skins)
    old_rays = rays_at(rest)
    h_old, _, c_old = a.intersect(old_rays, want_counters=True)
    joints, poses = {index: THREE}, skin_cases.object_poses("scaled_and_rotated", len(ranges))
    want = restatement.skin_arrays(rest, ranges, skins, joints, poses)
    before = a.bvh_info()
    a.skin(joints, poses=poses)
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
    a.skin({}, poses={})  # and back: the first answers
    h_back, _, c_back = a.intersect(old_rays, want_counters=True)
    assert same_bits(h_old, h_back) and counts_of(c_old) == counts_of(c_back)
    assert a.update_info()["area_ratio"] == 1.0 and a.update_info()["updates"] == 2
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 3. from rest
@pytest.mark.parametrize("shape", skin_cases.SHAPES)
def test_frames_are_from_rest_and_poses_and_joints_keep_each_other(gpu_lib, shape):
    a, _, _, _, ranges, rest, skins = skin_cases.build(shape)
    b, _, _, _, _, _, _ = skin_cases.build(shape)
    index, _ = the_skin(skins)
    a.skin({index: THREE})
    a.skin({index: OTHER})
    b.skin({index: OTHER})
    assert_geometry_bits(a.geometry(), b.geometry(), "%s: skin(A) then skin(B) against skin(B)" % shape)
    assert_geometry_bits(a.geometry(), restatement.skin_arrays(rest, ranges, skins, {index: OTHER}), "%s: skin(B)" % shape)
    poses = cases.poses_for("rotated_and_translated", len(ranges))
    a.pose(poses)  # keeps the joints
    assert_geometry_bits(a.geometry(), restatement.skin_arrays(rest, ranges, skins, {index: OTHER}, poses), "%s: pose() after skin()" % shape)
    a.skin({index: THREE})  # poses=None keeps the poses
    assert_geometry_bits(a.geometry(), restatement.skin_arrays(rest, ranges, skins, {index: THREE}, poses), "%s: skin() after pose()" % shape)
    assert a.update_info()["updates"] == 4
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 4. rebuild
@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("shape", skin_cases.SHAPES)
def test_a_rebuild_frame_is_the_scene_created_from_the_restatements_arrays(gpu_lib, shape, build):
    a, _, _, _, ranges, rest, skins = skin_cases.build(shape)
    b, _, _, _, _ = cases.build(shape)
    index, _ = the_skin(skins)
    joints, poses = {index: THREE}, skin_cases.object_poses("rotated_and_translated", len(ranges))
    want = restatement.skin_arrays(rest, ranges, skins, joints, poses)
    into_description(b, want)
    a.scene(0, build=build), b.scene(0, build=build)
    a.skin(joints, poses=poses, mode="rebuild")
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


# ---------------------------------------------------------------------------------------------------------------- 5. films
def bending_joints(rest, o):
    """Three rotations of at most 0.4 rad about the object's centroid: the object bends and stays in the frame."""
    centre = skin_cases.vertices_of(rest, o).astype(np.float64).mean(axis=0)
    return np.stack([about(centre, (0.2, 0.3, 1.0), -0.3), about(centre, (1.0, 0.1, 0.2), 0.15), about(centre, (0.3, 1.0, 0.2), 0.4)]).astype(np.float32)


@pytest.mark.parametrize("shape", ["cornell", "textures"])
def test_films_of_bent_meshes_match_the_oracle(gpu_lib, shape):
    """The oracle renders a world created from the restatement's arrays; the GPU renders the scene created from the rest pose and
    skinned. cornell: the lamp triangles 32 and 33 lie inside the skinned object, so the lamp records come from skinned arrays.
    textures: the cube's frames bend under its normal map. Weights exact, every pixel within TOL, path counters equal."""
    world, cam, r, gfilm, ranges, rest, skins = skin_cases.build(shape)
    index, _ = the_skin(skins)
    if shape == "cornell":
        assert [at for _, at in cases.shape_lamps(world)] == [32, 33] and ranges[index]["first_triangle"] <= 32 < 33 < ranges[index]["first_triangle"] + ranges[index]["num_triangles"]
    else:
        assert world.flat.uses_normal_maps and rest["frames"] is not None
    joints = {index: bending_joints(rest, ranges[index])}
    want = restatement.skin_arrays(rest, ranges, skins, joints)
    fresh, _, _, _, _ = cases.build(shape)  # the skinned description, never on the GPU
    into_description(fresh, want)
    cfilm = r.new_film(gfilm.width, gfilm.height)
    ccount = oracle.OracleScene(fresh).render(r, cam, cfilm, threads=8)
    world.skin(joints)
    assert_geometry_bits(world.geometry(), want, shape)
    gcount = r.render(gfilm, cam, world, counters=True)
    assert_parity(gfilm, cfilm)
    for key in ("samples", "extension_rays", "shadow_rays", "shaded_hits", "exposures"):
        assert gcount[key] == ccount[key], key
    assert cfilm.grains[..., 1].sum() > 0
    world.close()


# ---------------------------------------------------------------------------------------------------------------- 6. refusals, lifetime
def refused(status_and_word, status):
    code, word = status_and_word
    assert code == status, (word, code, lib().pyr_last_error())
    assert word in lib().pyr_last_error().decode(), (word, lib().pyr_last_error())


def test_set_skins_refuses_what_the_header_lists_and_keeps_the_old_skins(gpu_lib):
    """The textures example: objects 0, 1 and 3 are spheres, object 2 the cube of two triangles."""
    world, _, _, _, ranges, rest, skins = skin_cases.build("textures")
    index, skin = the_skin(skins)
    assert index == 2 and ranges[0]["num_triangles"] == 0
    scene = world.scene(0)
    j, w = skin["joints"], skin["weights"]

    def record(object=index, num_joints=3, joints=j, weights=w, reserved=(0, 0, 0, 0)):
        return abi.PyrSkin(object=object, num_joints=num_joints, joints=None if joints is None else joints.ctypes.data, weights=None if weights is None else weights.ctypes.data,
                           reserved=(C.c_uint32 * 4)(*reserved))

    high = j.copy()
    high[1, 2, 3] = 3  # under a zero weight
    nan, negative, heavy = w.copy(), w.copy(), w.copy()
    nan[0, 1, 3] = np.nan
    negative[1, 0, :] = (1.5, -0.5, 0.0, 0.0)
    heavy[1, 2, 3] += np.float32(2e-3)
    bad = [
        ([record(reserved=(0, 0, 1, 0))], "PyrSkin.reserved"),
        ([record(object=4)], "PyrSkin.object"),
        ([record(object=0)], "no triangles"),
        ([record(), record()], "two skins"),
        ([record(num_joints=0)], "num_joints"),
        ([record(num_joints=65537)], "num_joints"),
        ([record(joints=None)], "PyrSkin.joints is null"),
        ([record(weights=None)], "PyrSkin.weights is null"),
        ([record(joints=high)], "joint index"),
        ([record(weights=nan)], "not finite"),
        ([record(weights=negative)], "negative"),
        ([record(weights=heavy)], "sum to 1"),
    ]
    for records, word in bad:
        array = (abi.PyrSkin * len(records))(*records)
        refused((lib().pyr_scene_set_skins(scene, array, len(records)), word), abi.PYR_ERR_INVALID_ARGUMENT)
    light = w.copy()
    light[1, 2, 3] += np.float32(5e-4)  # within 1e-3 of 1: taken, and not renormalised
    world.skin({index: THREE})  # the refused calls left the old skin in place
    assert_geometry_bits(world.geometry(), restatement.skin_arrays(rest, ranges, skins, {index: THREE}), "after the refusals")
    lighter = {index: dict(skin, weights=light)}
    world.set_skins(lighter)
    assert_geometry_bits(world.geometry(), restatement.skin_arrays(rest, ranges, skins, {index: THREE}), "set_skins moves nothing")
    world.skin({index: THREE})
    assert_geometry_bits(world.geometry(), restatement.skin_arrays(rest, ranges, lighter, {index: THREE}), "weights are not renormalised")
    world.set_objects([])
    array = (abi.PyrSkin * 1)(record())
    refused((lib().pyr_scene_set_skins(scene, array, 1), "no objects"), abi.PYR_ERR_INVALID_ARGUMENT)
    world.close()


def test_the_argument_checks_of_a_frame_that_need_a_scene(gpu_lib):
    """pyr_scene_pose's, in its order, then: no skins set, num_joints that is not the scene's, NULL joints, an entry that is not
    finite, a last row that is not 0,0,0,1."""
    world, _, _, _, ranges, rest, skins = skin_cases.build("knot")
    scene = world.scene(0)
    identity = (C.c_float * 16)(*[float(x) for x in pose_restatement.IDENTITY])
    table = np.ascontiguousarray(np.tile(pose_restatement.IDENTITY, (3, 1)), dtype=np.float32)
    infinite, row = table.copy(), table.copy()
    infinite[2, 13] = np.inf
    row[1, 11] = 0.25

    def records(n=2):
        r = (abi.PyrObjectPose * n)()
        for k in range(n):
            r[k].transform, r[k].scale = identity, 1.0
        return r

    def update(mode=abi.PYR_UPDATE_REFIT, num_objects=2, poses=None, joints=table, num_joints=3, reserved=(0, 0, 0, 0)):
        return abi.PyrSkinUpdate(mode=mode, num_objects=num_objects, poses=poses, joints=None if joints is None else joints.ctypes.data, num_joints=num_joints,
                                 reserved=(C.c_uint32 * 4)(*reserved))

    reserved_pose, scale_nan = records(), records()
    reserved_pose[1].reserved[2] = 1
    scale_nan[0].scale = float("nan")
    bad = [
        (update(mode=7), "mode"),
        (update(reserved=(0, 1, 0, 0)), "PyrSkinUpdate.reserved"),
        (update(poses=reserved_pose), "PyrObjectPose.reserved"),
        (update(num_objects=3, poses=records(3)), "num_objects"),
        (update(poses=scale_nan), "scale"),
        (update(num_joints=4), "num_joints"),
        (update(joints=None), "joints is null"),
        (update(joints=infinite, mode=abi.PYR_UPDATE_REBUILD), "not finite"),
        (update(joints=row), "last row"),
    ]
    before = world.geometry()
    for u, word in bad:
        refused((lib().pyr_scene_skin(scene, C.byref(u), None), word), abi.PYR_ERR_INVALID_ARGUMENT)
    good = update(poses=records())
    assert lib().pyr_scene_skin(scene, C.byref(good), None) == abi.PYR_OK
    assert_geometry_bits(world.geometry(), before, "refused frames and an identity frame")
    world.set_skins({})  # forgets the skins
    refused((lib().pyr_scene_skin(scene, C.byref(update()), None), "no skins"), abi.PYR_ERR_INVALID_ARGUMENT)
    world.close()


def test_a_frame_under_a_live_session_is_refused(gpu_lib):
    world, cam, r, _, ranges, rest, skins = skin_cases.build("cornell")
    index, _ = the_skin(skins)
    with r.session((48, 48), cam, world) as session:
        session.render(2)
        for mode in ("refit", "rebuild"):
            with pytest.raises(PyriteGpuError) as err:
                world.skin({index: THREE}, mode=mode)
            assert err.value.status == abi.PYR_ERR_INVALID_ARGUMENT and "PyrSession" in str(err.value)
        session.sync()
    world.skin({index: THREE})  # the session is gone: the frame goes through now
    assert_geometry_bits(world.geometry(), restatement.skin_arrays(rest, ranges, skins, {index: THREE}), "after the session")
    world.close()


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_a_joint_beyond_the_coordinate_range_is_refused_and_the_scene_stays(gpu_lib, mode):
    world, _, _, _, ranges, rest, skins = skin_cases.build("knot")
    index, _ = the_skin(skins)
    rays = rays_at(rest)
    poses = cases.poses_for("rotated_and_translated", len(ranges))
    world.skin({index: THREE}, poses=poses)  # the scene is in a frame when the bad one arrives
    want = restatement.skin_arrays(rest, ranges, skins, {index: THREE}, poses)
    h0, _, c0 = world.intersect(rays, want_counters=True)
    build, updates = world.build_info(), world.update_info()["updates"]
    far = OTHER.copy()
    far[1] = translation(1e16, 0.0, 0.0)
    with pytest.raises(PyriteGpuError) as err:
        world.skin({index: far}, mode=mode)
    assert err.value.status == abi.PYR_ERR_UNSUPPORTED and "1e15" in str(err.value)
    h1, _, c1 = world.intersect(rays, want_counters=True)
    assert same_bits(h0, h1) and counts_of(c0) == counts_of(c1)
    assert world.build_info() == build and world.update_info()["updates"] == updates
    assert_geometry_bits(world.geometry(), want, "the geometry did not move either")
    world.skin({index: OTHER}, mode=mode)  # and the scene still takes a good frame, on the poses it kept
    assert_geometry_bits(world.geometry(), restatement.skin_arrays(rest, ranges, skins, {index: OTHER}, poses), "a good frame afterwards")
    world.close()


def test_set_objects_and_an_update_with_arrays_forget_the_skins(gpu_lib):
    world, _, _, _, ranges, rest, skins = skin_cases.build("knot")
    index, _ = the_skin(skins)
    scene = world.scene(0)
    table = np.ascontiguousarray(THREE.transpose(0, 2, 1), dtype=np.float32)
    frame = abi.PyrSkinUpdate(mode=abi.PYR_UPDATE_REFIT, num_objects=2, joints=table.ctypes.data, num_joints=3)
    assert lib().pyr_scene_skin(scene, C.byref(frame), None) == abi.PYR_OK
    skinned = restatement.skin_arrays(rest, ranges, skins, {index: THREE})
    assert_geometry_bits(world.geometry(), skinned, "the frame through the C ABI")
    world.skin({index: THREE})  # (the same frame again, so that the world knows of it)
    world.update(mode="refit")  # no array: the geometry, the objects and the skins stay
    assert lib().pyr_scene_skin(scene, C.byref(frame), None) == abi.PYR_OK
    world.set_objects(ranges)  # the rest pose is the geometry as it is now; the skins are gone
    refused((lib().pyr_scene_skin(scene, C.byref(frame), None), "no skins"), abi.PYR_ERR_INVALID_ARGUMENT)
    with pytest.raises(ValueError):
        world.skin({index: THREE})  # the world forgot them too
    world.set_skins(skins)
    world.skin({index: OTHER})
    assert_geometry_bits(world.geometry(), restatement.skin_arrays(skinned, ranges, skins, {index: OTHER}), "skinned from the newly captured rest pose")
    world.update(positions=rest["positions"], mode="refit")  # new arrays are a new geometry: objects and skins are forgotten
    refused((lib().pyr_scene_skin(scene, C.byref(frame), None), "no objects"), abi.PYR_ERR_INVALID_ARGUMENT)
    array = (abi.PyrSkin * 1)(abi.PyrSkin(object=index, num_joints=3, joints=skins[index]["joints"].ctypes.data, weights=skins[index]["weights"].ctypes.data))
    refused((lib().pyr_scene_set_skins(scene, array, 1), "no objects"), abi.PYR_ERR_INVALID_ARGUMENT)
    world.close()


def test_a_world_builds_a_later_scene_for_the_frame_it_is_in(gpu_lib):
    """The world remembers skins, joints and poses: a scene it makes after a frame (here: after the first was closed) is in it."""
    world, _, _, _, ranges, rest, skins = skin_cases.build("knot")
    index, _ = the_skin(skins)
    poses = cases.poses_for("non_uniform", len(ranges))
    world.skin({index: THREE}, poses=poses)
    want = restatement.skin_arrays(rest, ranges, skins, {index: THREE}, poses)
    world.close()
    assert_geometry_bits(world.geometry(), want, "the scene made after the frame")
    world.skin({index: OTHER})
    assert_geometry_bits(world.geometry(), restatement.skin_arrays(rest, ranges, skins, {index: OTHER}, poses), "and the next frame on it")
    world.close()


# ---------------------------------------------------------------------------------------------------------------- 7. the C++ front end
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_the_cpp_world_skins_like_the_restatement(gpu_lib, tmp_path, mode):
    """pyrite::World::set_skins, skin and geometry() through pyrite_host_tool on the textures scene (frames, spheres that stay)."""
    from test_host_cpp import HOST_TOOL, SCENES, data_dir_for
    from pyrite_amd.compiler import DATA_DIR, FlatScene
    from pyrite_amd.renderer import World

    world = World(FlatScene().add_world(SCENES["textures"]()["world"], DATA_DIR))
    rest, ranges = cases.rest_of(world), world.objects
    index = skin_cases.skinned_object(world)
    skins = {index: skin_cases.bend(rest, ranges[index])}
    bindings, table, result = str(tmp_path / "bindings.bin"), str(tmp_path / "joints.f32"), str(tmp_path / "geometry.f32")
    with open(bindings, "wb") as f:
        f.write(np.array([index, 3], dtype="<u4").tobytes())
        f.write(np.ascontiguousarray(skins[index]["joints"], dtype="<u2").tobytes())
        f.write(np.ascontiguousarray(skins[index]["weights"], dtype="<f4").tobytes())
    restatement.joint_table(THREE, 3).astype("<f4").tofile(table)
    subprocess.check_call([HOST_TOOL, "skin", "textures", data_dir_for("textures", tmp_path), bindings, table, result, mode], stdout=subprocess.DEVNULL)
    want = restatement.skin_arrays(rest, ranges, skins, {index: THREE})
    got = np.fromfile(result, dtype="<f4")
    expected = np.concatenate([want[key].reshape(-1) for key in KEYS])
    assert got.size == expected.size and np.array_equal(got.view(np.uint32), expected.view(np.uint32))


CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import pose_cases as cases, skin_cases, skin_restatement as restatement
from test_gpu_scene_update import aimed_rays, same_bits
from pyrite_amd import scenes
from pyrite_amd._lib import PyriteGpuError
def make():
    world, _, _, _ = scenes.build(scenes.c3_mesh_in_box(64, 36, 8, segments=96, sides=24), seed=5)
    world.set_objects([cases.triangles(12, 2 * 96 * 24)])
    return world
a, b = make(), make()
rest = cases.rest_of(a)
skins = {0: skin_cases.bend(rest, a.objects[0])}
a.set_skins(skins)
joints = {0: skin_cases.THREE}
want = restatement.skin_arrays(rest, a.objects, skins, joints)
b.flat.tri_positions, b.flat.tri_normals = [want["positions"].copy()], [want["normals"].copy()]
b._desc = b.flat.desc()
a.scene(0), b.scene(0)
try:
    a.skin(joints, mode="refit")
    print("REFIT went through")
except PyriteGpuError as e:
    print("REFIT", e.status)
a.skin(joints, mode="rebuild")
rays = aimed_rays(want["spheres"], want["positions"], 20000)
ha, hb = a.intersect(rays)[0], b.intersect(rays)[0]
print("REBUILD", int(a.build_info()["tree_digest"] == b.build_info()["tree_digest"]), int(a.bvh_info() == b.bvh_info()), int(same_bits(ha, hb)), int((hb["shape"] != 0xFFFFFFFF).sum()))
"""


def test_a_tree_with_spatial_splits_refuses_the_refit_frame_and_takes_the_rebuild_frame(gpu_lib):
    """PYRITE_SPATIAL_SPLITS is read when a tree is built: a fresh child process, so that nothing else in this one sees it (the way
    tests/test_gpu_scene_pose.py sets it). A knot of 4,608 triangles: large enough for the pair tree, which is the one that splits."""
    run = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=dict(os.environ, PYRITE_SPATIAL_SPLITS="1", PYTHONPATH=ROOT),
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert "REFIT %d" % abi.PYR_ERR_UNSUPPORTED in lines, run.stdout
    rebuilt = [l.split() for l in lines if l.startswith("REBUILD")][0]
    assert rebuilt[1:4] == ["1", "1", "1"] and int(rebuilt[4]) > 1000, run.stdout
