"""Dual quaternion skinning of a live scene's meshes on the GPU (pyr_scene_set_skin_blend) -- run with `-m gpu` on
an MI355X.

The geometry a frame leaves equals the numpy restatement (tests/dq_skin_restatement.py) bit for bit: both sides are the same IEEE f32
operations with contraction off, the joints' dual quaternions are made on the host, and sqrt32 / rcp32 are bit-exact in the ranges
used, so equality is the criterion. Everything after the vertex's matrix is what a linear skin has: the object's pose, smoothing,
refit and rebuild, keep_previous. Linear skins are held against tests/skin_restatement.py, the yardstick from before this blend
existed, alone and next to a dual-quaternion skin in one call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dq_skin_cases  # noqa: E402
import dq_skin_restatement as restatement  # noqa: E402
import pose_cases as cases  # noqa: E402
import pose_restatement  # noqa: E402
import skin_cases  # noqa: E402
import skin_restatement  # noqa: E402
import smooth_restatement  # noqa: E402
from test_gpu_bvh_build import assert_shapes_equal_up_to_ties  # noqa: E402
from test_gpu_motion import check_moved  # noqa: E402
from test_gpu_scene_pose import assert_geometry_bits, bits, rays_at, update_to  # noqa: E402
from test_gpu_scene_skin import into_description  # noqa: E402
from test_gpu_scene_update import counts_of, same_bits  # noqa: E402

from pyrite_amd import abi  # noqa: E402
from pyrite_amd._lib import PyriteGpuError, lib  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("positions", "normals", "frames", "spheres")
RIGID, OTHER = dq_skin_cases.RIGID, dq_skin_cases.OTHER


def the_skin(skins):
    (index, skin), = skins.items()
    return index, skin


# ---------------------------------------------------------------------------------------------------------------- 1. the arrays
@pytest.mark.parametrize("pose", ["identity", "rotated_and_translated"])
@pytest.mark.parametrize("binding", dq_skin_cases.BINDINGS)
@pytest.mark.parametrize("shape", dq_skin_cases.SHAPES)
def test_the_dual_quaternion_geometry_is_the_restatements_bit_for_bit(gpu_lib, shape, binding, pose):
    world, _, _, _, ranges, rest, skins = dq_skin_cases.build(shape, binding)
    index, _ = the_skin(skins)
    joints, poses = {index: RIGID}, skin_cases.object_poses(pose, len(ranges))
    world.skin(joints, poses=poses)
    want = restatement.dq_skin_arrays(rest, ranges, skins, joints, poses)
    what = "%s %s %s" % (shape, binding, pose)
    assert_geometry_bits(world.geometry(), want, what)
    assert not np.array_equal(bits(rest["positions"]), bits(want["positions"]))
    assert not np.array_equal(bits(want["positions"]), bits(skin_restatement.skin_arrays(rest, ranges, skins, joints, poses)["positions"]))  # another blend
    info = world.update_info()
    assert info["mode_used"] == abi.PYR_UPDATE_REFIT and info["updates"] == 1
    world.skin({index: OTHER})  # a frame is from rest, never from the previous one; poses=None keeps the poses
    assert_geometry_bits(world.geometry(), restatement.dq_skin_arrays(rest, ranges, skins, {index: OTHER}, poses), what + ": the next frame")
    world.skin({}, poses={})  # the identity table, every pose the identity
    assert_geometry_bits(world.geometry(), rest, what + ": the identity table against rest")
    world.close()


@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("shape", dq_skin_cases.SHAPES)
def test_a_rebuild_frame_is_the_scene_created_from_the_restatements_arrays(gpu_lib, shape, build):
    a, _, _, _, ranges, rest, skins = dq_skin_cases.build(shape)
    b, _, _, _, _ = cases.build(shape)
    index, _ = the_skin(skins)
    joints, poses = {index: RIGID}, skin_cases.object_poses("rotated_and_translated", len(ranges))
    want = restatement.dq_skin_arrays(rest, ranges, skins, joints, poses)
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
    info = a.update_info()
    assert info["mode_used"] == abi.PYR_UPDATE_REBUILD and info["updates"] == 0
    assert_geometry_bits(a.geometry(), want, "%s rebuild" % shape)
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 2. both blends in one call
def two_skins(rest, ranges, kinds):
    """The knot's two objects, each with the bend binding and the blend `kinds` names."""
    return {k: dict(skin_cases.bend(rest, ranges[k]), blend=kinds[k]) for k in (0, 1)}


@pytest.mark.parametrize("kinds", [("linear", "dual_quaternion"), ("dual_quaternion", "linear")])
def test_a_linear_and_a_dual_quaternion_skin_in_one_call_are_each_their_own_restatement(gpu_lib, kinds):
    """The knot: lanes 0..287 belong to one skin and 288..639 to the other, so each kernel's workgroup 1 holds lanes of both."""
    world, _, _, _, ranges = cases.build("knot")
    rest = cases.rest_of(world)
    skins = two_skins(rest, ranges, kinds)
    world.set_skins(skins)
    tables = {"linear": skin_cases.THREE, "dual_quaternion": RIGID}
    joints = {k: tables[kinds[k]] for k in (0, 1)}
    poses = skin_cases.object_poses("rotated_and_translated", len(ranges))
    world.skin(joints, poses=poses)
    got = world.geometry()
    assert_geometry_bits(got, restatement.dq_skin_arrays(rest, ranges, skins, joints, poses), "both skins %r" % (kinds,))
    for k in (0, 1):  # and each object alone, against the yardstick of its own blend
        alone = {k: skins[k]}
        want = (skin_restatement.skin_arrays if kinds[k] == "linear" else restatement.dq_skin_arrays)(rest, ranges, alone, {k: joints[k]}, poses)
        cut = slice(ranges[k]["first_triangle"], ranges[k]["first_triangle"] + ranges[k]["num_triangles"])
        for key in ("positions", "normals"):
            assert np.array_equal(bits(got[key][cut]), bits(want[key][cut])), (kinds, k, key)
    world.close()


@pytest.mark.parametrize("shape", dq_skin_cases.SHAPES)
def test_a_linear_only_scene_is_what_it_was_before_this_blend_existed(gpu_lib, shape):
    """blend="linear" spelled out: the geometry is skin_restatement's, the yardstick of tests/test_gpu_scene_skin.py."""
    world, _, _, _, ranges, rest, skins = skin_cases.build(shape)
    index, skin = the_skin(skins)
    world.set_skins({index: dict(skin, blend="linear")})
    joints, poses = {index: skin_cases.THREE}, skin_cases.object_poses("rotated_and_translated", len(ranges))
    world.skin(joints, poses=poses)
    assert_geometry_bits(world.geometry(), skin_restatement.skin_arrays(rest, ranges, skins, joints, poses), shape)
    world.close()


# ---------------------------------------------------------------------------------------------------------------- 3. like an update
@pytest.mark.parametrize("shape", dq_skin_cases.SHAPES)
def test_a_dual_quaternion_scene_answers_like_a_scene_updated_to_the_restatements_arrays(gpu_lib, shape):
    a, _, _, _, ranges, rest, skins = dq_skin_cases.build(shape)
    b, _, _, _, _ = cases.build(shape)
    index, _ = the_skin(skins)
    joints, poses = {index: RIGID}, skin_cases.object_poses("scaled_and_rotated", len(ranges))
    want = restatement.dq_skin_arrays(rest, ranges, skins, joints, poses)
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
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 4. what comes after B
def test_keep_previous_and_the_motion_pass_on_a_dual_quaternion_frame(gpu_lib):
    world, cam, r, _, ranges, rest, skins = dq_skin_cases.build("cornell", "bend")
    index, _ = the_skin(skins)
    world.skin({index: RIGID})
    previous = world.geometry()
    assert_geometry_bits(previous, restatement.dq_skin_arrays(rest, ranges, skins, {index: RIGID}), "the frame that is kept")
    world.keep_previous()
    world.skin({index: OTHER})
    assert_geometry_bits(world.geometry(), restatement.dq_skin_arrays(rest, ranges, skins, {index: OTHER}), "the frame after it")
    check_moved(world, cam, r, (64, 64), previous, "cornell under a dual-quaternion skin, two joint tables", expect_moved=False)
    world.close()


@pytest.mark.parametrize("shape", ["cornell", "textures", "knot"])
def test_smoothing_on_top_is_n_of_the_restatement(gpu_lib, shape):
    world, _, _, _, ranges, rest, skins = dq_skin_cases.build(shape)
    index, _ = the_skin(skins)
    t0, n = ranges[index]["first_triangle"], ranges[index]["num_triangles"]
    smoothing = {index: smooth_restatement.weld(rest["positions"][t0:t0 + n], rest["normals"][t0:t0 + n])}
    world.set_smoothing(smoothing)
    joints, poses = {index: RIGID}, skin_cases.object_poses("rotated_and_translated", len(ranges))
    world.skin(joints, poses=poses)
    want, flag, _ = smooth_restatement.smoothed(restatement.dq_skin_arrays(rest, ranges, skins, joints, poses), rest, ranges, smoothing)
    assert flag == 0
    assert_geometry_bits(world.geometry(), want, shape + ": smoothed")
    world.close()


def test_the_twisted_cylinder_keeps_its_radius_on_the_device_and_loses_it_under_the_linear_blend(gpu_lib):
    """The closed form of tests/test_scene_dq_skin_cpu.py on the kernels: 1e-5 relative on every vertex's distance from the axis and
    on its z under the dual quaternion blend; the ring at z = 0.5 below 0.1 under the linear one."""
    for blend in ("dual_quaternion", "linear"):
        world, ranges, rest, skins = dq_skin_cases.twist_world(blend)
        index, _ = the_skin(skins)
        joints = {index: dq_skin_cases.TWIST}
        world.skin(joints)
        got = world.geometry()
        assert_geometry_bits(got, restatement.dq_skin_arrays(rest, ranges, skins, joints), "twist " + blend)
        radius, z, rest_radius, rest_z = dq_skin_cases.twist_radii(got, ranges[index], rest)
        if blend == "dual_quaternion":
            assert np.abs(radius - rest_radius).max() <= 1e-5 * rest_radius.max() and np.abs(z - rest_z).max() <= 1e-5
        else:
            assert (rest_z == 0.5).sum() == 6 * dq_skin_cases.TWIST_SEGMENTS and radius[rest_z == 0.5].max() < 0.1
        world.close()


# ---------------------------------------------------------------------------------------------------------------- 5. refusals, lifetime
def refused(status_and_word, status):
    code, word = status_and_word
    assert code == status, (word, code, lib().pyr_last_error())
    assert word in lib().pyr_last_error().decode(), (word, lib().pyr_last_error())


def test_set_skin_blend_refuses_what_the_header_lists_in_its_order_and_keeps_the_modes(gpu_lib):
    world, _, _, _, ranges, rest, skins = dq_skin_cases.build("knot")
    index, skin = the_skin(skins)
    scene = world.scene(0)
    dual, unknown, two = (C.c_uint32 * 1)(abi.PYR_SKIN_DUAL_QUATERNION), (C.c_uint32 * 1)(2), (C.c_uint32 * 2)(1, 7)
    blend = lib().pyr_scene_set_skin_blend
    refused((blend(scene, None, 1), "null modes"), abi.PYR_ERR_INVALID_ARGUMENT)
    refused((blend(None, None, 1), "null modes"), abi.PYR_ERR_INVALID_ARGUMENT)  # NULL modes before a NULL scene
    refused((blend(None, dual, 1), "null scene"), abi.PYR_ERR_INVALID_ARGUMENT)
    refused((blend(scene, two, 2), "num_skins"), abi.PYR_ERR_INVALID_ARGUMENT)  # the count before the unknown mode in the table
    refused((blend(scene, unknown, 1), "neither PYR_SKIN_LINEAR nor PYR_SKIN_DUAL_QUATERNION"), abi.PYR_ERR_INVALID_ARGUMENT)
    world.skin({index: RIGID})  # the refused calls left the mode in place
    assert_geometry_bits(world.geometry(), restatement.dq_skin_arrays(rest, ranges, skins, {index: RIGID}), "after the refusals")
    # pyr_scene_set_skin_blend sets every joint to the identity and moves nothing
    assert blend(scene, dual, 1) == abi.PYR_OK
    assert_geometry_bits(world.geometry(), restatement.dq_skin_arrays(rest, ranges, skins, {index: RIGID}), "set_skin_blend moves nothing")
    frame = abi.PyrPoseUpdate(mode=abi.PYR_UPDATE_REFIT, num_objects=len(ranges), poses=world._pose_records({}))
    assert lib().pyr_scene_pose(scene, C.byref(frame), None) == abi.PYR_OK  # keeps the joints the scene is in: the identity now
    assert_geometry_bits(world.geometry(), rest, "the joints are the identity after set_skin_blend")
    world.set_skins({})
    refused((blend(scene, dual, 1), "no skins"), abi.PYR_ERR_INVALID_ARGUMENT)
    refused((blend(scene, two, 2), "no skins"), abi.PYR_ERR_INVALID_ARGUMENT)  # no skins before the count
    world.close()


def test_a_joint_of_a_dual_quaternion_skin_that_is_no_rotation_is_refused_after_the_last_row(gpu_lib):
    world, _, _, _, ranges, rest, skins = dq_skin_cases.build("knot")
    index, _ = the_skin(skins)
    scene = world.scene(0)
    world.skin({index: RIGID})
    table = skin_restatement.joint_table(RIGID, 3)
    scaled, row_and_scaled = table.copy(), table.copy()
    scaled[2, 0:3] *= np.float32(1.01)
    row_and_scaled[2, 0:3] *= np.float32(1.01)
    row_and_scaled[0, 11] = 0.25
    uniform = skin_restatement.joint_table(skin_cases.THREE, 3)  # its third matrix is non-uniform

    def skin_update(joints):
        return abi.PyrSkinUpdate(mode=abi.PYR_UPDATE_REFIT, num_objects=len(ranges), joints=joints.ctypes.data, num_joints=3)

    def morph_update(joints):
        return abi.PyrMorphUpdate(mode=abi.PYR_UPDATE_REFIT, num_objects=len(ranges), joints=joints.ctypes.data, num_joints=3)

    for bad in (scaled, uniform):
        code = lib().pyr_scene_skin(scene, C.byref(skin_update(bad)), None)
        refused((code, "PyrSkinUpdate.joints"), abi.PYR_ERR_INVALID_ARGUMENT)
        refused((code, "rotation"), abi.PYR_ERR_INVALID_ARGUMENT)
    refused((lib().pyr_scene_skin(scene, C.byref(skin_update(row_and_scaled)), None), "last row"), abi.PYR_ERR_INVALID_ARGUMENT)  # the last row comes first
    assert_geometry_bits(world.geometry(), restatement.dq_skin_arrays(rest, ranges, skins, {index: RIGID}), "the refused frames moved nothing")
    from morph_cases import targets
    morphs = {index: targets(rest, ranges[index], with_normals=False)}
    world.set_morphs(morphs)
    code = lib().pyr_scene_morph(scene, C.byref(morph_update(scaled)), None)
    refused((code, "PyrMorphUpdate.joints"), abi.PYR_ERR_INVALID_ARGUMENT)
    refused((code, "rotation"), abi.PYR_ERR_INVALID_ARGUMENT)
    world.set_skins({index: dict(skins[index], blend="linear")})  # a linear skin takes any matrix
    assert lib().pyr_scene_skin(scene, C.byref(skin_update(uniform)), None) == abi.PYR_OK
    world.close()


def test_set_skins_set_objects_and_an_update_with_arrays_reset_or_forget_the_modes(gpu_lib):
    world, _, _, _, ranges, rest, skins = dq_skin_cases.build("knot")
    index, skin = the_skin(skins)
    scene = world.scene(0)
    dual = (C.c_uint32 * 1)(abi.PYR_SKIN_DUAL_QUATERNION)
    world.skin({index: RIGID})
    assert_geometry_bits(world.geometry(), restatement.dq_skin_arrays(rest, ranges, skins, {index: RIGID}), "dual quaternion")
    # pyr_scene_set_skins makes every skin linear again
    record = (abi.PyrSkin * 1)(abi.PyrSkin(object=index, num_joints=3, joints=skin["joints"].ctypes.data, weights=skin["weights"].ctypes.data))
    assert lib().pyr_scene_set_skins(scene, record, 1) == abi.PYR_OK
    table = skin_restatement.joint_table(RIGID, 3)
    frame = abi.PyrSkinUpdate(mode=abi.PYR_UPDATE_REFIT, num_objects=len(ranges), joints=table.ctypes.data, num_joints=3)
    assert lib().pyr_scene_skin(scene, C.byref(frame), None) == abi.PYR_OK
    assert_geometry_bits(world.geometry(), skin_restatement.skin_arrays(rest, ranges, skins, {index: RIGID}), "linear again after pyr_scene_set_skins")
    # the world's set_skins without a blend does the same
    world.set_skins({index: {k: v for k, v in skin.items() if k != "blend"}})
    world.skin({index: RIGID})
    assert_geometry_bits(world.geometry(), skin_restatement.skin_arrays(rest, ranges, skins, {index: RIGID}), "World.set_skins without a blend")
    world.set_skins(skins)
    world.skin({}, poses={})
    # whatever forgets the skins forgets the modes
    world.set_objects(ranges)
    refused((lib().pyr_scene_set_skin_blend(scene, dual, 1), "no skins"), abi.PYR_ERR_INVALID_ARGUMENT)
    world.set_skins({index: {k: v for k, v in skin.items() if k != "blend"}})
    world.skin({index: RIGID})
    assert_geometry_bits(world.geometry(), skin_restatement.skin_arrays(rest, ranges, skins, {index: RIGID}), "linear after set_objects and set_skins")
    world.set_skins(skins)
    world.update(positions=rest["positions"], mode="refit")  # new arrays are a new geometry: objects, skins and modes are forgotten
    refused((lib().pyr_scene_set_skin_blend(scene, dual, 1), "no skins"), abi.PYR_ERR_INVALID_ARGUMENT)
    world.close()


def test_a_world_builds_a_later_scene_with_its_blend(gpu_lib):
    world, _, _, _, ranges, rest, skins = dq_skin_cases.build("knot")
    index, _ = the_skin(skins)
    world.skin({index: RIGID})
    want = restatement.dq_skin_arrays(rest, ranges, skins, {index: RIGID})
    world.close()
    assert_geometry_bits(world.geometry(), want, "the scene made after the frame")
    world.close()


# ---------------------------------------------------------------------------------------------------------------- 6. the C++ front end
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_the_cpp_world_blends_dual_quaternions_like_the_restatement(gpu_lib, tmp_path, mode):
    """pyrite::World::set_skins with Skin::blend, skin and geometry() through pyrite_host_tool on the textures scene."""
    from test_host_cpp import HOST_TOOL, SCENES, data_dir_for
    from pyrite_amd.compiler import DATA_DIR, FlatScene
    from pyrite_amd.renderer import World

    world = World(FlatScene().add_world(SCENES["textures"]()["world"], DATA_DIR))
    rest, ranges = cases.rest_of(world), world.objects
    index = skin_cases.skinned_object(world)
    skins = {index: dq_skin_cases.binding("bend", rest, ranges[index])}
    bindings, table, result = str(tmp_path / "bindings.bin"), str(tmp_path / "joints.f32"), str(tmp_path / "geometry.f32")
    with open(bindings, "wb") as f:
        f.write(np.array([index, 3], dtype="<u4").tobytes())
        f.write(np.ascontiguousarray(skins[index]["joints"], dtype="<u2").tobytes())
        f.write(np.ascontiguousarray(skins[index]["weights"], dtype="<f4").tobytes())
    skin_restatement.joint_table(RIGID, 3).astype("<f4").tofile(table)
    subprocess.check_call([HOST_TOOL, "skin", "textures", data_dir_for("textures", tmp_path), bindings, table, result, mode, "dual_quaternion"], stdout=subprocess.DEVNULL)
    want = restatement.dq_skin_arrays(rest, ranges, skins, {index: RIGID})
    got = np.fromfile(result, dtype="<f4")
    expected = np.concatenate([want[key].reshape(-1) for key in KEYS])
    assert got.size == expected.size and np.array_equal(got.view(np.uint32), expected.view(np.uint32))
    linear = skin_restatement.skin_arrays(rest, ranges, skins, {index: RIGID})
    assert not np.array_equal(got.view(np.uint32), np.concatenate([linear[key].reshape(-1) for key in KEYS]).view(np.uint32))
