"""Morph targets for a live scene's meshes on the GPU (pyr_scene_set_morphs / pyr_scene_morph) -- run with
`-m gpu` on an MI355X.

The geometry a frame leaves equals the numpy restatement (tests/morph_restatement.py) bit for bit: both sides are the same IEEE f32
operations with contraction off, and sqrt32 / rcp32 are bit-exact in the ranges the rule's own check keeps them in, so equality is
the criterion. A morphed scene answers like a scene pyr_scene_update moved to those arrays; a frame is from rest, never from the
previous one; a rebuild frame IS the scene created from the morphed arrays; films of bulged lamps and bulged normal maps match the
oracle; refused calls leave the scene, its morphs and its weights alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_cases  # noqa: E402
import morph_restatement as restatement  # noqa: E402
import oracle  # noqa: E402
import pose_cases as cases  # noqa: E402
import pose_restatement  # noqa: E402
import skin_cases  # noqa: E402
from test_gpu_bvh_build import assert_shapes_equal_up_to_ties  # noqa: E402
from test_gpu_parity import TOL, assert_parity, rel_l2  # noqa: E402
from test_gpu_scene_pose import assert_geometry_bits, bits, rays_at, update_to  # noqa: E402
from test_gpu_scene_update import counts_of, same_bits  # noqa: E402

from pyrite_amd import abi  # noqa: E402
from pyrite_amd._lib import PyriteGpuError, lib  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("positions", "normals", "frames", "spheres")
WEIGHTS, OTHER, BULGE, ZERO = morph_cases.WEIGHTS, morph_cases.OTHER, morph_cases.BULGE, morph_cases.ZERO
f32 = np.float32


def into_description(world, arrays):
    for key, attr in (("positions", "tri_positions"), ("normals", "tri_normals"), ("frames", "tri_frames"), ("spheres", "spheres")):
        if arrays[key] is not None and len(arrays[key]):
            setattr(world.flat, attr, [arrays[key].copy()])
    world._desc = world.flat.desc()


def expected(shape, rest, ranges, morphs, skins, w=WEIGHTS):
    """(weights, joints, poses, the restatement's arrays) of the frame of morph_cases.frame_for."""
    weights, joints, poses = morph_cases.frame_for(shape, morphs, skins, ranges, w)
    return weights, joints, poses, restatement.morph_arrays(rest, ranges, morphs, weights, skins, joints, poses)


def run_frame(world, weights, joints, poses, mode="refit"):
    world.morph(weights, joints=joints or None, poses=poses, mode=mode)


# ---------------------------------------------------------------------------------------------------------------- 1. the arrays
@pytest.mark.parametrize("shape", morph_cases.SHAPES)
def test_the_morphed_geometry_is_the_restatements_bit_for_bit(gpu_lib, shape):
    """The knot runs morph+skin (object 0) and morph+pose (object 1) in the one call, the box's twelve triangles left alone."""
    world, _, _, _, ranges, rest, morphs, skins = morph_cases.build(shape)
    weights, joints, poses, want = expected(shape, rest, ranges, morphs, skins)
    run_frame(world, weights, joints, poses)
    assert_geometry_bits(world.geometry(), want, shape)
    assert not np.array_equal(bits(rest["positions"]), bits(want["positions"])) and not np.array_equal(bits(rest["normals"]), bits(want["normals"]))
    if shape == "knot":
        assert np.array_equal(bits(want["positions"][:12]), bits(rest["positions"][:12]))
    info = world.update_info()
    assert info["mode_used"] == abi.PYR_UPDATE_REFIT and info["updates"] == 1
    assert_geometry_bits(cases.rest_of(world), rest, "World.flat stays the rest pose")
    world.close()


@pytest.mark.parametrize("shape", morph_cases.SHAPES)
def test_a_morph_without_normal_deltas_keeps_rests_normals_and_frames(gpu_lib, shape):
    world, _, _, _, ranges, rest, morphs, _ = morph_cases.build(shape, with_normals=False)
    if shape == "knot":
        world.set_skins({})  # the morph alone
    weights = morph_cases.table(morphs, WEIGHTS)
    world.morph(weights)
    got = world.geometry()
    assert_geometry_bits(got, restatement.morph_arrays(rest, ranges, morphs, weights), shape)
    assert np.array_equal(bits(got["normals"]), bits(rest["normals"])) and not np.array_equal(bits(got["positions"]), bits(rest["positions"]))
    assert rest["frames"] is None or np.array_equal(bits(got["frames"]), bits(rest["frames"]))
    world.close()


@pytest.mark.parametrize("shape", morph_cases.SHAPES)
def test_zero_weights_give_rest_and_poison_under_weight_zero_changes_nothing(gpu_lib, shape):
    world, _, _, _, ranges, rest, morphs, skins = morph_cases.build(shape)
    world.morph(morph_cases.table(morphs, WEIGHTS))
    world.morph(morph_cases.table(morphs, [0.0, -0.0, 0.0]))  # both zeros are inactive
    assert_geometry_bits(world.geometry(), rest, shape + ": zero weights against rest")
    clean = {index: dict(positions=m["positions"][:2], normals=m["normals"][:2]) for index, m in morphs.items()}  # the same morphs without their poison
    other, _, _, _, _ = cases.build(shape)
    other.set_morphs(clean)
    world.morph(morph_cases.table(morphs, WEIGHTS))
    other.morph(morph_cases.table(clean, WEIGHTS[:2]))
    assert_geometry_bits(world.geometry(), other.geometry(), shape + ": with the poison target against without")
    assert all(np.isfinite(a).all() for a in world.geometry().values() if a is not None)
    world.close(), other.close()


# ---------------------------------------------------------------------------------------------------------------- 2. from rest
@pytest.mark.parametrize("shape", morph_cases.SHAPES)
def test_frames_are_from_rest_and_weights_joints_and_poses_keep_each_other(gpu_lib, shape):
    a, _, _, _, ranges, rest, morphs, skins = morph_cases.build(shape)
    b, _, _, _, _, _, _, _ = morph_cases.build(shape)
    a.morph(morph_cases.table(morphs, WEIGHTS))
    a.morph(morph_cases.table(morphs, OTHER))
    b.morph(morph_cases.table(morphs, OTHER))
    other = morph_cases.table(morphs, OTHER)
    assert_geometry_bits(a.geometry(), b.geometry(), "%s: morph(A) then morph(B) against morph(B)" % shape)
    assert_geometry_bits(a.geometry(), restatement.morph_arrays(rest, ranges, morphs, other, skins), "%s: morph(B)" % shape)
    poses = cases.poses_for("rotated_and_translated", len(ranges))
    a.pose(poses)  # keeps the weights
    assert_geometry_bits(a.geometry(), restatement.morph_arrays(rest, ranges, morphs, other, skins, {}, poses), "%s: pose() after morph()" % shape)
    joints = {}
    if skins:
        joints = {index: skin_cases.THREE for index in skins}
        a.skin(joints)  # keeps the weights and the poses
        assert_geometry_bits(a.geometry(), restatement.morph_arrays(rest, ranges, morphs, other, skins, joints, poses), "%s: skin() after morph()" % shape)
    first = sorted(morphs)[0]
    a.morph({first: WEIGHTS})  # joints=None and poses=None keep both; a morph that is not named keeps its weights
    kept = dict(other)
    kept[first] = WEIGHTS
    assert_geometry_bits(a.geometry(), restatement.morph_arrays(rest, ranges, morphs, kept, skins, joints, poses), "%s: morph() after pose() and skin()" % shape)
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 3. like an update
@pytest.mark.parametrize("shape", morph_cases.SHAPES)
def test_a_morphed_scene_answers_like_a_scene_updated_to_the_restatements_arrays(gpu_lib, shape):
    a, _, _, _, ranges, rest, morphs, skins = morph_cases.build(shape)
    b, _, _, _, _ = cases.build(shape)
    old_rays = rays_at(rest)
    h_old, _, c_old = a.intersect(old_rays, want_counters=True)
    weights, joints, poses, want = expected(shape, rest, ranges, morphs, skins)
    before = a.bvh_info()
    run_frame(a, weights, joints, poses)
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
    a.morph(morph_cases.table(morphs, ZERO), joints={} if skins else None, poses={})  # and back: the first answers
    h_back, _, c_back = a.intersect(old_rays, want_counters=True)
    assert same_bits(h_old, h_back) and counts_of(c_old) == counts_of(c_back)
    assert a.update_info()["area_ratio"] == 1.0 and a.update_info()["updates"] == 2
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 4. rebuild
@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("shape", morph_cases.SHAPES)
def test_a_rebuild_frame_is_the_scene_created_from_the_restatements_arrays(gpu_lib, shape, build):
    a, _, _, _, ranges, rest, morphs, skins = morph_cases.build(shape)
    b, _, _, _, _ = cases.build(shape)
    weights, joints, poses, want = expected(shape, rest, ranges, morphs, skins)
    into_description(b, want)
    a.scene(0, build=build), b.scene(0, build=build)
    run_frame(a, weights, joints, poses, mode="rebuild")
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


def test_a_world_builds_a_later_scene_for_the_frame_it_is_in(gpu_lib):
    """The world remembers morphs, weights, skins, joints and poses: a scene it makes after a frame is in that frame."""
    world, _, _, _, ranges, rest, morphs, skins = morph_cases.build("knot")
    weights, joints, poses, want = expected("knot", rest, ranges, morphs, skins)
    run_frame(world, weights, joints, poses)
    world.close()
    assert_geometry_bits(world.geometry(), want, "the scene made after the frame")
    world.morph(morph_cases.table(morphs, OTHER))
    assert_geometry_bits(world.geometry(), restatement.morph_arrays(rest, ranges, morphs, morph_cases.table(morphs, OTHER), skins, joints, poses), "and the next frame on it")
    world.close()


# ---------------------------------------------------------------------------------------------------------------- 5. films
@pytest.mark.parametrize("shape", ["cornell", "textures"])
def test_films_of_bulged_meshes_match_the_oracle(gpu_lib, shape):
    """The oracle renders a world created from the restatement's arrays; the GPU renders the scene created from the rest pose and
    morphed. cornell: the lamp triangles 32 and 33 lie inside the morphed object, so the lamp records come from morphed arrays.
    textures: the cube's frames follow the bulged normals under its normal map. Weights exact, every pixel within TOL, path
    counters equal."""
    world, cam, r, gfilm, ranges, rest, morphs, _ = morph_cases.build(shape)
    (index, _), = morphs.items()
    if shape == "cornell":
        assert [at for _, at in cases.shape_lamps(world)] == [32, 33] and ranges[index]["first_triangle"] <= 32 < 33 < ranges[index]["first_triangle"] + ranges[index]["num_triangles"]
    else:
        assert world.flat.uses_normal_maps and rest["frames"] is not None
    weights = morph_cases.table(morphs, BULGE)
    want = restatement.morph_arrays(rest, ranges, morphs, weights)
    assert not np.array_equal(bits(want["normals"]), bits(rest["normals"]))
    fresh, _, _, _, _ = cases.build(shape)  # the morphed description, never on the GPU
    into_description(fresh, want)
    cfilm = r.new_film(gfilm.width, gfilm.height)
    ccount = oracle.OracleScene(fresh).render(r, cam, cfilm, threads=8)
    world.morph(weights)
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


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_both_flag_refusals_leave_geometry_and_films_as_before(gpu_lib, mode):
    """Targets 3 and 4 of a five-target morph of the Cornell box: dn = -n (at weight 1 the morphed normal is exactly zero: bit 1 of
    the flag word) and a position delta of 1e16 (beyond the coordinate range: bit 0). Both are argument refusals on valid memory:
    PYR_ERR_UNSUPPORTED, and the scene renders as before, under the weights it was in."""
    world, cam, r, film, ranges = cases.build("cornell")
    rest = cases.rest_of(world)
    index = skin_cases.skinned_object(world)
    t0, n = ranges[index]["first_triangle"], ranges[index]["num_triangles"]
    base = morph_cases.targets(rest, ranges[index])
    collapse_n = (-rest["normals"][t0:t0 + n]).reshape(1, n, 3, 3).astype(f32)
    far_p = np.zeros((1, n, 3, 3), dtype=f32)
    far_p[0, 5, 1, 0] = 1e16
    zeros = np.zeros((1, n, 3, 3), dtype=f32)
    morphs = {index: dict(positions=np.concatenate([base["positions"], zeros, far_p]), normals=np.concatenate([base["normals"], collapse_n, zeros]))}
    world.set_morphs(morphs)
    held = {index: np.array([0.75, -0.5, 0.0, 0.0, 0.0], dtype=f32)}
    world.morph(held)  # the scene is in a frame when the bad ones arrive
    want = restatement.morph_arrays(rest, ranges, morphs, held)
    first = r.new_film(film.width, film.height)
    r.render(first, cam, world)
    build, updates = world.build_info(), world.update_info()["updates"]
    for bad, word in (([0.0, 0.0, 0.0, 1.0, 0.0], "morphed normal"), ([0.0, 0.0, 0.0, 0.0, 1.0], "1e15"), ([0.0, 0.0, 0.0, 1.0, 1.0], "1e15")):
        assert restatement.morph_flag(rest, ranges, morphs, {index: bad}) == (2 if bad[3] else 0)
        with pytest.raises(PyriteGpuError) as err:
            world.morph({index: np.array(bad, dtype=f32)}, mode=mode)
        assert err.value.status == abi.PYR_ERR_UNSUPPORTED and word in str(err.value), (bad, str(err.value))
        assert_geometry_bits(world.geometry(), want, "the geometry did not move")
        assert world.build_info() == build and world.update_info()["updates"] == updates
    again = r.new_film(film.width, film.height)
    r.render(again, cam, world)
    assert np.array_equal(first.grains[..., 1], again.grains[..., 1]) and first.grains[..., 1].sum() > 0
    assert float(rel_l2(again, first).max()) <= TOL
    world.morph({index: np.array([0.25, 1.25, 0.0, 0.0, 0.0], dtype=f32)}, mode=mode)  # and the scene still takes a good frame
    assert_geometry_bits(world.geometry(), restatement.morph_arrays(rest, ranges, morphs, {index: [0.25, 1.25, 0.0, 0.0, 0.0]}), "a good frame afterwards")
    world.close()


def test_set_morphs_refuses_what_the_header_lists_and_keeps_the_old_morphs(gpu_lib):
    """The textures example: objects 0, 1 and 3 are spheres, object 2 the cube of two triangles."""
    world, _, _, _, ranges, rest, morphs, _ = morph_cases.build("textures")
    (index, morph), = morphs.items()
    assert index == 2 and ranges[0]["num_triangles"] == 0
    scene = world.scene(0)
    dp, dn = morph["positions"], morph["normals"]

    def record(object=index, num_targets=3, positions=dp, normals=dn, reserved=(0, 0, 0, 0)):
        return abi.PyrMorph(object=object, num_targets=num_targets, position_deltas=None if positions is None else positions.ctypes.data,
                            normal_deltas=None if normals is None else normals.ctypes.data, reserved=(C.c_uint32 * 4)(*reserved))

    nan, infinite = dp.copy(), dn.copy()
    nan[1, 1, 2, 0] = np.nan
    infinite[2, 0, 1, 2] = np.inf
    bad = [
        ([record(reserved=(0, 0, 1, 0))], "PyrMorph.reserved"),
        ([record(object=4)], "PyrMorph.object"),
        ([record(object=0)], "no triangles"),
        ([record(), record()], "two morphs"),
        ([record(num_targets=0)], "num_targets"),
        ([record(num_targets=257)], "num_targets"),
        ([record(positions=None)], "position_deltas is null"),
        ([record(positions=nan)], "not finite"),
        ([record(normals=infinite)], "not finite"),
    ]
    for records, word in bad:
        array = (abi.PyrMorph * len(records))(*records)
        refused((lib().pyr_scene_set_morphs(scene, array, len(records)), word), abi.PYR_ERR_INVALID_ARGUMENT)
    refused((lib().pyr_scene_set_morphs(scene, None, 1), "null morphs"), abi.PYR_ERR_INVALID_ARGUMENT)
    weights = morph_cases.table(morphs, WEIGHTS)
    world.morph(weights)  # the refused calls left the old morph in place
    moved = restatement.morph_arrays(rest, ranges, morphs, weights)
    assert_geometry_bits(world.geometry(), moved, "after the refusals")
    world.set_morphs(morphs)
    assert_geometry_bits(world.geometry(), moved, "set_morphs moves nothing")
    world.pose({})  # and every weight is zero afterwards
    assert_geometry_bits(world.geometry(), rest, "the weights are zero after set_morphs")
    world.set_objects([])
    array = (abi.PyrMorph * 1)(record())
    refused((lib().pyr_scene_set_morphs(scene, array, 1), "no objects"), abi.PYR_ERR_INVALID_ARGUMENT)
    world.close()


def test_the_argument_checks_of_a_frame_that_need_a_scene(gpu_lib):
    """pyr_scene_pose's, in its order, then: no morphs set, joints given on a scene without skins, the joint table's checks, num_weights
    that is not the scene's, a weight that is not finite."""
    world, _, _, _, ranges, rest, morphs, skins = morph_cases.build("knot")
    scene = world.scene(0)
    identity = (C.c_float * 16)(*[float(x) for x in pose_restatement.IDENTITY])
    table = np.ascontiguousarray(np.tile(pose_restatement.IDENTITY, (3, 1)), dtype=np.float32)
    infinite, row = table.copy(), table.copy()
    infinite[2, 13] = np.inf
    row[1, 11] = 0.25
    zero = np.zeros(6, dtype=np.float32)
    nan = zero.copy()
    nan[4] = np.nan

    def records(n=2):
        r = (abi.PyrObjectPose * n)()
        for k in range(n):
            r[k].transform, r[k].scale = identity, 1.0
        return r

    def update(mode=abi.PYR_UPDATE_REFIT, num_objects=2, poses=None, joints=None, num_joints=0, weights=zero, num_weights=6, reserved=(0, 0, 0, 0)):
        return abi.PyrMorphUpdate(mode=mode, num_objects=num_objects, poses=poses, joints=None if joints is None else joints.ctypes.data, num_joints=num_joints,
                                  weights=None if weights is None else weights.ctypes.data, num_weights=num_weights, reserved=(C.c_uint32 * 4)(*reserved))

    reserved_pose, scale_nan = records(), records()
    reserved_pose[1].reserved[2] = 1
    scale_nan[0].scale = float("nan")
    bad = [
        (update(mode=7), "mode"),
        (update(reserved=(0, 1, 0, 0)), "PyrMorphUpdate.reserved"),
        (update(poses=reserved_pose), "PyrObjectPose.reserved"),
        (update(num_objects=3, poses=records(3)), "num_objects"),
        (update(poses=scale_nan), "scale"),
        (update(joints=table, num_joints=4), "num_joints"),
        (update(joints=infinite, num_joints=3, mode=abi.PYR_UPDATE_REBUILD), "not finite"),
        (update(joints=row, num_joints=3), "last row"),
        (update(num_weights=5), "num_weights"),
        (update(weights=nan), "weights has a weight that is not finite"),
    ]
    before = world.geometry()
    for u, word in bad:
        refused((lib().pyr_scene_morph(scene, C.byref(u), None), word), abi.PYR_ERR_INVALID_ARGUMENT)
    for good in (update(poses=records()), update(weights=None, num_weights=77), update(joints=table, num_joints=3)):  # NULL weights: num_weights is not read
        assert lib().pyr_scene_morph(scene, C.byref(good), None) == abi.PYR_OK
    assert_geometry_bits(world.geometry(), before, "refused frames and frames at rest")
    world.set_skins({})  # the morphs stay, the skins go
    refused((lib().pyr_scene_morph(scene, C.byref(update(joints=table, num_joints=3)), None), "no skins"), abi.PYR_ERR_INVALID_ARGUMENT)
    assert lib().pyr_scene_morph(scene, C.byref(update()), None) == abi.PYR_OK
    world.set_morphs({})  # forgets the morphs
    refused((lib().pyr_scene_morph(scene, C.byref(update()), None), "no morphs"), abi.PYR_ERR_INVALID_ARGUMENT)
    world.close()


def test_a_frame_under_a_live_session_is_refused(gpu_lib):
    world, cam, r, _, ranges, rest, morphs, _ = morph_cases.build("cornell")
    weights = morph_cases.table(morphs, WEIGHTS)
    with r.session((48, 48), cam, world) as session:
        session.render(2)
        for mode in ("refit", "rebuild"):
            with pytest.raises(PyriteGpuError) as err:
                world.morph(weights, mode=mode)
            assert err.value.status == abi.PYR_ERR_INVALID_ARGUMENT and "PyrSession" in str(err.value)
        session.sync()
    world.morph(weights)  # the session is gone: the frame goes through now
    assert_geometry_bits(world.geometry(), restatement.morph_arrays(rest, ranges, morphs, weights), "after the session")
    world.close()


def test_set_objects_and_an_update_with_arrays_forget_the_morphs_and_set_skins_does_not(gpu_lib):
    world, _, _, _, ranges, rest, morphs, skins = morph_cases.build("knot")
    scene = world.scene(0)
    table = np.ascontiguousarray(np.concatenate([WEIGHTS, OTHER]), dtype=np.float32)
    frame = abi.PyrMorphUpdate(mode=abi.PYR_UPDATE_REFIT, num_objects=2, weights=table.ctypes.data, num_weights=6)
    assert lib().pyr_scene_morph(scene, C.byref(frame), None) == abi.PYR_OK
    weights = {0: WEIGHTS, 1: OTHER}
    moved = restatement.morph_arrays(rest, ranges, morphs, weights, skins)
    assert_geometry_bits(world.geometry(), moved, "the frame through the C ABI")
    world.morph(weights)  # (the same frame again, so that the world knows of it)
    world.set_skins({})  # the morphs and their weights stay
    world.pose({})
    assert_geometry_bits(world.geometry(), moved, "set_skins leaves the morphs and the weights")
    world.set_skins(skins)
    joints = {0: skin_cases.THREE}
    world.skin(joints)
    assert_geometry_bits(world.geometry(), restatement.morph_arrays(rest, ranges, morphs, weights, skins, joints), "a skin bound after the morphs")
    world.update(mode="refit")  # no array: the geometry, the objects, the skins and the morphs stay
    assert lib().pyr_scene_morph(scene, C.byref(frame), None) == abi.PYR_OK
    world.morph(weights, joints={})  # (so that the world knows: the identity table)
    world.set_objects(ranges)  # the rest pose is the geometry as it is now; the morphs are gone
    refused((lib().pyr_scene_morph(scene, C.byref(frame), None), "no morphs"), abi.PYR_ERR_INVALID_ARGUMENT)
    with pytest.raises(ValueError):
        world.morph(weights)  # the world forgot them too
    world.set_morphs(morphs)
    world.morph({0: OTHER})
    assert_geometry_bits(world.geometry(), restatement.morph_arrays(moved, ranges, morphs, {0: OTHER}), "morphed from the newly captured rest pose")
    world.update(positions=rest["positions"], mode="refit")  # new arrays are a new geometry: objects and morphs are forgotten
    refused((lib().pyr_scene_morph(scene, C.byref(frame), None), "no objects"), abi.PYR_ERR_INVALID_ARGUMENT)
    array = (abi.PyrMorph * 1)(abi.PyrMorph(object=0, num_targets=3, position_deltas=morphs[0]["positions"].ctypes.data))
    refused((lib().pyr_scene_set_morphs(scene, array, 1), "no objects"), abi.PYR_ERR_INVALID_ARGUMENT)
    world.close()


# ---------------------------------------------------------------------------------------------------------------- 7. the C++ front end
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_the_cpp_world_morphs_like_the_restatement(gpu_lib, tmp_path, mode):
    """pyrite::World::set_morphs, morph and geometry() through pyrite_host_tool on the textures scene (frames, spheres that stay)."""
    from test_host_cpp import HOST_TOOL, SCENES, data_dir_for
    from pyrite_amd.compiler import DATA_DIR, FlatScene
    from pyrite_amd.renderer import World

    world = World(FlatScene().add_world(SCENES["textures"]()["world"], DATA_DIR))
    rest, ranges = cases.rest_of(world), world.objects
    index = skin_cases.skinned_object(world)
    morphs = {index: morph_cases.targets(rest, ranges[index])}
    targets, table, result = str(tmp_path / "targets.bin"), str(tmp_path / "weights.f32"), str(tmp_path / "geometry.f32")
    with open(targets, "wb") as f:
        f.write(np.array([index, 3, 1], dtype="<u4").tobytes())
        f.write(np.ascontiguousarray(morphs[index]["positions"], dtype="<f4").tobytes())
        f.write(np.ascontiguousarray(morphs[index]["normals"], dtype="<f4").tobytes())
    WEIGHTS.astype("<f4").tofile(table)
    subprocess.check_call([HOST_TOOL, "morph", "textures", data_dir_for("textures", tmp_path), targets, table, result, mode], stdout=subprocess.DEVNULL)
    want = restatement.morph_arrays(rest, ranges, morphs, {index: WEIGHTS})
    got = np.fromfile(result, dtype="<f4")
    expected_words = np.concatenate([want[key].reshape(-1) for key in KEYS])
    assert got.size == expected_words.size and np.array_equal(got.view(np.uint32), expected_words.view(np.uint32))
