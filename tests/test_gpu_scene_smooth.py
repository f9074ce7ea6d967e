"""Smooth normals for a live scene's meshes on the GPU (pyr_scene_set_smoothing) -- run with `-m gpu` on an
MI355X.

The geometry a frame leaves equals the numpy restatement (tests/smooth_restatement.py) bit for bit: both sides are the same IEEE
f32 operations with contraction off, sums in the same fixed order, and sqrt32 / rcp32 are bit-exact in the range the rule's own
check keeps them in, so equality is the criterion. A smoothed object is recomputed under the identity too; an unsmoothed one next to
it keeps what the calls gave it before; a smoothed scene answers like a scene pyr_scene_update moved to those arrays; a rebuild
frame IS the scene created from them; films of bulged meshes match the oracle; refused calls leave the scene and its smoothing
alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_cases  # noqa: E402
import oracle  # noqa: E402
import pose_cases as cases  # noqa: E402
import pose_restatement  # noqa: E402
import skin_cases  # noqa: E402
import smooth_cases  # noqa: E402
import smooth_restatement as restatement  # noqa: E402
from test_gpu_bvh_build import assert_shapes_equal_up_to_ties  # noqa: E402
from test_gpu_parity import TOL, assert_parity, rel_l2  # noqa: E402
from test_gpu_scene_pose import assert_geometry_bits, bits, rays_at, update_to  # noqa: E402
from test_gpu_scene_update import counts_of, same_bits  # noqa: E402

from pyrite_amd import abi  # noqa: E402
from pyrite_amd._lib import PyriteGpuError, lib  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("positions", "normals", "frames", "spheres")
WEIGHTS, BULGE = morph_cases.WEIGHTS, morph_cases.BULGE
f32 = np.float32


def into_description(world, arrays):
    for key, attr in (("positions", "tri_positions"), ("normals", "tri_normals"), ("frames", "tri_frames"), ("spheres", "spheres")):
        if arrays[key] is not None and len(arrays[key]):
            setattr(world.flat, attr, [arrays[key].copy()])
    world._desc = world.flat.desc()


def full_frame(shape, world, rest, ranges):
    """(morphs, skins, weights, joints, poses): everything at once -- a morph without normal deltas on every smoothed object; in the
    knots the skin of object 0; the last object under a pose."""
    morphs = smooth_cases.morphs_for(shape, world, rest, ranges)
    skins = smooth_cases.skins_for(shape, rest, ranges)
    weights = morph_cases.table(morphs, WEIGHTS)
    joints = {index: skin_cases.THREE for index in skins}
    poses = {len(ranges) - 1: cases.POSES["rotated_and_translated"]}
    return morphs, skins, weights, joints, poses


# ---------------------------------------------------------------------------------------------------------------- 1. the arrays
@pytest.mark.parametrize("pose", ["identity", "non_uniform", "rotated_and_translated"])
@pytest.mark.parametrize("shape", smooth_cases.SHAPES)
def test_a_posed_smoothed_geometry_is_the_restatements_bit_for_bit(gpu_lib, shape, pose):
    """The identity too: positions are rest's in every word, normals (and frames) the recomputed ones."""
    world, _, _, _, ranges, rest, smoothing = smooth_cases.build(shape)
    poses = cases.poses_for(pose, len(ranges))
    want = restatement.smooth_arrays(rest, ranges, smoothing, poses=poses)
    before = world.geometry()
    assert_geometry_bits(before, rest, "set_smoothing moves nothing")
    world.pose(poses)
    got = world.geometry()
    assert_geometry_bits(got, want, (shape, pose))
    assert not np.array_equal(bits(want["normals"]), bits(pose_restatement.pose_arrays(rest, ranges, poses)["normals"]))
    if pose == "identity":
        assert np.array_equal(bits(got["positions"]), bits(rest["positions"]))
    info = world.update_info()
    assert info["mode_used"] == abi.PYR_UPDATE_REFIT and info["updates"] == 1
    assert_geometry_bits(cases.rest_of(world), rest, "World.flat stays the rest pose")
    world.close()


@pytest.mark.parametrize("shape", smooth_cases.SHAPES)
def test_morph_skin_pose_and_smoothing_in_one_call(gpu_lib, shape):
    """The split knot runs morph+skin+smoothing (object 0) and morph+pose+smoothing (object 1) in the one call, the box's twelve
    triangles left alone; then a morph at rest and an identity skin still give recomputed normals."""
    world, _, _, _, ranges, rest, smoothing = smooth_cases.build(shape)
    morphs, skins, weights, joints, poses = full_frame(shape, world, rest, ranges)
    if skins:
        world.set_skins(skins)
    world.set_morphs(morphs)
    world.morph(weights, joints=joints or None, poses=poses)
    want = restatement.smooth_arrays(rest, ranges, smoothing, morphs, weights, skins, joints, poses)
    assert_geometry_bits(world.geometry(), want, shape)
    if shape.startswith("knot"):
        assert np.array_equal(bits(want["positions"][:12]), bits(rest["positions"][:12])) and np.array_equal(bits(want["normals"][:12]), bits(rest["normals"][:12]))
    world.morph(morph_cases.table(morphs, morph_cases.ZERO), joints={} if skins else None, poses={})
    at_rest = restatement.smooth_arrays(rest, ranges, smoothing)
    assert_geometry_bits(world.geometry(), at_rest, shape + ": a morph at rest, an identity skin, identity poses")
    assert np.array_equal(bits(at_rest["positions"]), bits(rest["positions"])) and not np.array_equal(bits(at_rest["normals"]), bits(rest["normals"]))
    if skins:
        world.skin(joints)
        assert_geometry_bits(world.geometry(), restatement.smooth_arrays(rest, ranges, smoothing, morphs, {}, skins, joints, {}), shape + ": skin() alone")
    world.close()


def test_an_unsmoothed_object_next_to_a_smoothed_one_keeps_every_word(gpu_lib):
    """The split knot with object 1 smoothed alone: object 0 and the box are what the same call leaves on a world without any
    smoothing, in every word; object 1's normals are the recomputed ones."""
    a, _, _, _, ranges, rest, smoothing = smooth_cases.build("knot")
    b, _, _, _, _ = cases.build("knot")
    a.set_smoothing({1: smoothing[1]})
    poses = cases.poses_for("non_uniform", len(ranges))
    a.pose(poses), b.pose(poses)
    ga, gb = a.geometry(), b.geometry()
    t1 = ranges[1]["first_triangle"]
    for key in ("positions", "normals"):
        assert np.array_equal(bits(ga[key][:t1]), bits(gb[key][:t1])), key
    assert np.array_equal(bits(ga["positions"]), bits(gb["positions"])) and not np.array_equal(bits(ga["normals"][t1:]), bits(gb["normals"][t1:]))
    assert_geometry_bits(ga, restatement.smooth_arrays(rest, ranges, {1: smoothing[1]}, poses=poses), "object 1 alone")
    a.close(), b.close()


def test_none_welds_by_the_rest_pose_and_a_later_scene_is_in_the_frame(gpu_lib):
    """World.set_smoothing({object: None}); the world remembers the smoothing: a scene it makes after a frame -- an identity frame
    too -- holds the recomputed normals."""
    world, _, _, _, ranges = smooth_cases.make("knot_one")
    rest = cases.rest_of(world)
    world.set_smoothing({0: None})
    smoothing = smooth_cases.labels_for("knot_one", world, rest, ranges)
    world.pose({})
    want = restatement.smooth_arrays(rest, ranges, smoothing)
    assert_geometry_bits(world.geometry(), want, "welded by None")
    world.close()
    assert_geometry_bits(world.geometry(), want, "the scene made after the identity frame")
    poses = cases.poses_for("non_uniform", 1)
    world.pose(poses)
    world.close()
    assert_geometry_bits(world.geometry(), restatement.smooth_arrays(rest, ranges, smoothing, poses=poses), "the scene made after a posed frame")
    world.close()


# ---------------------------------------------------------------------------------------------------------------- 2. like an update
@pytest.mark.parametrize("shape", smooth_cases.SHAPES)
def test_a_smoothed_scene_answers_like_a_scene_updated_to_the_restatements_arrays(gpu_lib, shape):
    a, _, _, _, ranges, rest, smoothing = smooth_cases.build(shape)
    b, _, _, _, _ = smooth_cases.make(shape)
    poses = cases.poses_for("non_uniform", len(ranges))
    want = restatement.smooth_arrays(rest, ranges, smoothing, poses=poses)
    before = a.bvh_info()
    a.pose(poses)
    update_to(b, want)
    assert a.bvh_info() == before == b.bvh_info()
    rays = rays_at(want)
    ha, na, ca = a.intersect(rays, want_counters=True)
    hb, nb, cb = b.intersect(rays, want_counters=True)
    assert np.array_equal(ha["distance"].view(np.uint32), hb["distance"].view(np.uint32))
    assert (hb["shape"] != 0xFFFFFFFF).sum() > 1000
    assert_shapes_equal_up_to_ties(b, hb, ha, rays)
    assert counts_of(ca) == counts_of(cb)
    assert a.update_info()["area_ratio"] == b.update_info()["area_ratio"]
    a.close(), b.close()


@pytest.mark.parametrize("build", ["host", "device"])
@pytest.mark.parametrize("shape", ["cornell", "knot"])
def test_a_rebuild_frame_is_the_scene_created_from_the_restatements_arrays(gpu_lib, shape, build):
    a, _, _, _, ranges, rest, smoothing = smooth_cases.build(shape)
    b, _, _, _, _ = smooth_cases.make(shape)
    poses = cases.poses_for("non_uniform", len(ranges))
    want = restatement.smooth_arrays(rest, ranges, smoothing, poses=poses)
    into_description(b, want)
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
    info = a.update_info()
    assert info["mode_used"] == abi.PYR_UPDATE_REBUILD and info["updates"] == 0
    assert_geometry_bits(a.geometry(), want, "%s rebuild" % shape)
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 3. films
@pytest.mark.parametrize("shape", ["cornell", "textures"])
def test_films_of_bulged_smoothed_meshes_match_the_oracle(gpu_lib, shape):
    """The oracle renders a world created from the restatement's arrays; the GPU renders the scene created from the rest pose,
    morphed without normal deltas and smoothed. cornell: the lamp triangles 32 and 33 lie inside the object, so the lamp records
    take recomputed normals. textures: the cube's frames are rebuilt against the recomputed normals under its normal map.
    Weights exact, every pixel within TOL, path counters equal."""
    world, cam, r, gfilm, ranges, rest, smoothing = smooth_cases.build(shape)
    (index, _), = smoothing.items()
    if shape == "cornell":
        assert [at for _, at in cases.shape_lamps(world)] == [32, 33] and ranges[index]["first_triangle"] <= 32 < 33 < ranges[index]["first_triangle"] + ranges[index]["num_triangles"]
    else:
        assert world.flat.uses_normal_maps and rest["frames"] is not None
    morphs = smooth_cases.morphs_for(shape, world, rest, ranges)
    weights = morph_cases.table(morphs, BULGE)
    want = restatement.smooth_arrays(rest, ranges, smoothing, morphs, weights)
    assert not np.array_equal(bits(want["normals"]), bits(rest["normals"]))
    fresh, _, _, _, _ = smooth_cases.make(shape)  # the smoothed description, never on the GPU
    into_description(fresh, want)
    cfilm = r.new_film(gfilm.width, gfilm.height)
    ccount = oracle.OracleScene(fresh).render(r, cam, cfilm, threads=8)
    world.set_morphs(morphs)
    world.morph(weights)
    assert_geometry_bits(world.geometry(), want, shape)
    gcount = r.render(gfilm, cam, world, counters=True)
    assert_parity(gfilm, cfilm)
    for key in ("samples", "extension_rays", "shadow_rays", "shaded_hits", "exposures"):
        assert gcount[key] == ccount[key], key
    assert cfilm.grains[..., 1].sum() > 0
    world.close()


# ---------------------------------------------------------------------------------------------------------------- 4. refusals, lifetime
def refused(status_and_word, status):
    code, word = status_and_word
    assert code == status, (word, code, lib().pyr_last_error())
    assert word in lib().pyr_last_error().decode(), (word, lib().pyr_last_error())


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_the_bit_2_refusal_leaves_geometry_and_films_as_before(gpu_lib, mode):
    """A pose of scale 0 puts every vertex of the Cornell box on the translation: every face vector is exactly zero, no bound is out of
    range. PYR_ERR_UNSUPPORTED naming a recomputed normal, and the scene renders as before, in the pose it was in. A position
    delta of 1e16 still answers with the coordinate range's message."""
    world, cam, r, film, ranges, rest, smoothing = smooth_cases.build("cornell")
    index = next(iter(smoothing))
    held = {index: cases.POSES["rotated_and_translated"]}
    world.pose(held)  # the scene is in a frame when the bad one arrives
    want = restatement.smooth_arrays(rest, ranges, smoothing, poses=held)
    first = r.new_film(film.width, film.height)
    r.render(first, cam, world)
    build, updates = world.build_info(), world.update_info()["updates"]
    collapse = {index: (cases.POSES["rotated_and_translated"][0], 0.0)}
    assert restatement.smooth_flag(rest, ranges, smoothing, poses=collapse) == 4
    with pytest.raises(PyriteGpuError) as err:
        world.pose(collapse, mode=mode)
    assert err.value.status == abi.PYR_ERR_UNSUPPORTED and "recomputed normal" in str(err.value), str(err.value)
    assert_geometry_bits(world.geometry(), want, "the geometry did not move")
    assert world.build_info() == build and world.update_info()["updates"] == updates
    n = ranges[index]["num_triangles"]
    far = np.zeros((1, n, 3, 3), dtype=f32)
    far[0, 5, 1, 0] = 1e16
    world.set_morphs({index: dict(positions=far, normals=None)})
    with pytest.raises(PyriteGpuError) as err:
        world.morph({index: [1.0]}, mode=mode)
    assert err.value.status == abi.PYR_ERR_UNSUPPORTED and "1e15" in str(err.value), str(err.value)
    assert_geometry_bits(world.geometry(), want, "the geometry did not move")
    again = r.new_film(film.width, film.height)
    r.render(again, cam, world)
    assert np.array_equal(first.grains[..., 1], again.grains[..., 1]) and first.grains[..., 1].sum() > 0
    assert float(rel_l2(again, first).max()) <= TOL
    other = {index: cases.POSES["non_uniform"]}
    world.pose(other, mode=mode)  # and the scene still takes a good frame
    assert_geometry_bits(world.geometry(), restatement.smooth_arrays(rest, ranges, smoothing, poses=other), "a good frame afterwards")
    world.close()


def test_set_smoothing_refuses_what_the_header_lists_and_keeps_the_old_smoothing(gpu_lib):
    """The textures example: objects 0, 1 and 3 are spheres, object 2 the cube of two triangles."""
    world, _, _, _, ranges, rest, smoothing = smooth_cases.build("textures")
    (index, ids), = smoothing.items()
    assert index == 2 and ranges[0]["num_triangles"] == 0
    scene = world.scene(0)

    def record(object=index, labels=ids, reserved0=0, reserved=(0, 0, 0, 0)):
        return abi.PyrSmoothing(object=object, reserved0=reserved0, vertex_ids=None if labels is None else labels.ctypes.data, reserved=(C.c_uint32 * 4)(*reserved))

    bad = [
        ([record(reserved=(0, 0, 1, 0))], "PyrSmoothing.reserved"),
        ([record(reserved0=1)], "PyrSmoothing.reserved"),
        ([record(object=4)], "PyrSmoothing.object"),
        ([record(object=0)], "no triangles"),
        ([record(), record()], "two smoothings"),
        ([record(labels=None)], "vertex_ids is null"),
        ([record(object=4, labels=None, reserved=(1, 0, 0, 0))], "PyrSmoothing.reserved"),  # in the header's order
        ([record(object=0, labels=None)], "no triangles"),
    ]
    for records, word in bad:
        array = (abi.PyrSmoothing * len(records))(*records)
        refused((lib().pyr_scene_set_smoothing(scene, array, len(records)), word), abi.PYR_ERR_INVALID_ARGUMENT)
    refused((lib().pyr_scene_set_smoothing(scene, None, 1), "null smoothings"), abi.PYR_ERR_INVALID_ARGUMENT)
    poses = cases.poses_for("non_uniform", len(ranges))
    world.pose(poses)  # the refused calls left the old smoothing in place
    moved = restatement.smooth_arrays(rest, ranges, smoothing, poses=poses)
    assert_geometry_bits(world.geometry(), moved, "after the refusals")
    world.set_smoothing(smoothing)
    assert_geometry_bits(world.geometry(), moved, "set_smoothing moves nothing")
    world.set_smoothing({})  # forgets it: the next frame is the parent's
    assert_geometry_bits(world.geometry(), moved, "forgetting moves nothing")
    world.pose(poses)
    assert_geometry_bits(world.geometry(), pose_restatement.pose_arrays(rest, ranges, poses), "a frame without the smoothing")
    world.set_objects([])
    array = (abi.PyrSmoothing * 1)(record())
    refused((lib().pyr_scene_set_smoothing(scene, array, 1), "no objects"), abi.PYR_ERR_INVALID_ARGUMENT)
    world.close()


def test_set_objects_and_an_update_with_arrays_forget_the_smoothing_and_set_skins_and_set_morphs_do_not(gpu_lib):
    world, _, _, _, ranges, rest, smoothing = smooth_cases.build("knot")
    morphs, skins, weights, joints, poses = full_frame("knot", world, rest, ranges)
    world.set_skins(skins), world.set_morphs(morphs)  # after the smoothing: it stays
    world.morph(weights, joints=joints, poses=poses)
    assert_geometry_bits(world.geometry(), restatement.smooth_arrays(rest, ranges, smoothing, morphs, weights, skins, joints, poses), "skins and morphs set after the smoothing")
    world.set_skins({}), world.set_morphs({})  # forgetting them leaves it too
    world.pose(poses)
    moved = restatement.smooth_arrays(rest, ranges, smoothing, poses=poses)
    assert_geometry_bits(world.geometry(), moved, "set_skins({}) and set_morphs({}) leave the smoothing")
    world.update(mode="refit")  # no array: the geometry, the objects and the smoothing stay
    world.pose({})
    assert_geometry_bits(world.geometry(), restatement.smooth_arrays(rest, ranges, smoothing), "an update without arrays leaves the smoothing")
    world.pose(poses)
    world.set_objects(ranges)  # the rest pose is the geometry as it is now; the smoothing is gone
    assert world._smoothing == {}
    world.pose(poses)
    assert_geometry_bits(world.geometry(), pose_restatement.pose_arrays(moved, ranges, poses), "posed from the newly captured rest pose, nothing recomputed")
    world.set_smoothing({1: smoothing[1]})
    world.update(positions=rest["positions"], mode="refit")  # new arrays are a new geometry: objects and smoothing are forgotten
    assert world._smoothing == {}
    array = (abi.PyrSmoothing * 1)(abi.PyrSmoothing(object=1, vertex_ids=smoothing[1].ctypes.data))
    refused((lib().pyr_scene_set_smoothing(world.scene(0), array, 1), "no objects"), abi.PYR_ERR_INVALID_ARGUMENT)
    world.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the C++ front end
@pytest.mark.parametrize("labels", ["given", "welded"])
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_the_cpp_world_smooths_like_the_restatement(gpu_lib, tmp_path, mode, labels):
    """pyrite::World::set_smoothing (with labels, and welding by pyrite::weld), pose and geometry() through pyrite_host_tool on the
    textures scene (frames, spheres that stay)."""
    from test_host_cpp import HOST_TOOL, SCENES, data_dir_for
    from pyrite_amd.compiler import DATA_DIR, FlatScene
    from pyrite_amd.renderer import World

    world = World(FlatScene().add_world(SCENES["textures"]()["world"], DATA_DIR))
    rest, ranges = cases.rest_of(world), world.objects
    index = skin_cases.skinned_object(world)
    smoothing = smooth_cases.labels_for("textures", world, rest, ranges)
    pose = cases.POSES["non_uniform"]
    ids, posed, result = str(tmp_path / "labels.bin"), str(tmp_path / "pose.f32"), str(tmp_path / "geometry.f32")
    with open(ids, "wb") as f:
        f.write(np.array([index, 1 if labels == "given" else 0], dtype="<u4").tobytes())
        if labels == "given":
            f.write(np.ascontiguousarray(smoothing[index] + 1000, dtype="<u4").tobytes())  # labels are arbitrary: only equality counts
    with open(posed, "wb") as f:
        f.write(pose_restatement.column_major(pose[0]).astype("<f4").tobytes())
        f.write(np.float32(pose[1]).tobytes())
    subprocess.check_call([HOST_TOOL, "smooth", "textures", data_dir_for("textures", tmp_path), ids, posed, result, mode], stdout=subprocess.DEVNULL)
    want = restatement.smooth_arrays(rest, ranges, smoothing, poses={index: pose})
    got = np.fromfile(result, dtype="<f4")
    expected_words = np.concatenate([want[key].reshape(-1) for key in KEYS])
    assert got.size == expected_words.size and np.array_equal(got.view(np.uint32), expected_words.view(np.uint32))
