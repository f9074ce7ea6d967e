"""Dual quaternion skinning without a GPU (pyr_scene_set_skin_blend): the additions to the ABI, the refusals that
need no scene, the world's bookkeeping, the closed form on a twisting cylinder -- the linear blend's collapse and its cure -- and the
host rehearsal of the two skin kernels: pose_rules.h, the header kernels/pose.hip compiles, through tests/probes/dq_skin_check.cpp, a
program of its own built with -fsanitize=address,undefined and run as a child process, compared as bits with the numpy restatement
(tests/dq_skin_restatement.py). The refusals that need a scene -- and a scene needs a device -- are in
tests/test_gpu_scene_dq_skin.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dq_skin_cases  # noqa: E402
import dq_skin_restatement as restatement  # noqa: E402
import pose_cases as cases  # noqa: E402
import pose_restatement  # noqa: E402
import skin_cases  # noqa: E402
import skin_restatement  # noqa: E402

from pyrite_amd import abi  # noqa: E402
from pyrite_amd import build as gpu_build  # noqa: E402

HEADER = os.path.join(ROOT, "include", "pyrite_gpu.h")
KEYS = ("positions", "normals", "frames")
RIGID = dq_skin_cases.RIGID


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- (a) the ABI
def test_the_abi_gains_one_entry_and_two_constants_and_keeps_its_version():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+PYR_ABI_VERSION\s+5\b", text) and abi.PYR_ABI_VERSION == 5
    assert re.search(r"\bint\s+pyr_scene_set_skin_blend\s*\(\s*PyrScene\s*\*\s*,\s*const\s+uint32_t\s*\*\s*modes\s*,\s*uint32_t\s+num_skins\s*\)", text)
    assert "pyr_scene_set_skin_blend" in abi.ENTRY_POINTS
    for name, value in (("PYR_SKIN_LINEAR", 0), ("PYR_SKIN_DUAL_QUATERNION", 1)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, value), text) and getattr(abi, name) == value
    # PyrSkin keeps its layout and its four reserved words
    fields = [name for name, _ in abi.PyrSkin._fields_]
    assert fields == ["object", "num_joints", "joints", "weights", "reserved"] and C.sizeof(abi.PyrSkin) == 40
    assert dict(abi.PyrSkin._fields_)["reserved"]._length_ == 4
    body = re.search(r"typedef struct PyrSkin \{(.*?)\} PyrSkin;", text, flags=re.S).group(1)
    assert [w for w in re.findall(r"(\w+)(?:\[4\])?;", body)] == fields


# ---------------------------------------------------------------------------------------------------------------- (b) refusals
@pytest.fixture(scope="module")
def lib():
    return abi.bind(C.CDLL(gpu_build.build()))


def test_set_skin_blend_refuses_null_modes_then_a_null_scene_before_any_device_is_looked_for(lib):
    """No GPU here: anything that reached the device would be PYR_ERR_DEVICE. NULL modes come first, a NULL scene second; the three
    refusals after them need a scene (tests/test_gpu_scene_dq_skin.py)."""
    modes = (C.c_uint32 * 1)(abi.PYR_SKIN_DUAL_QUATERNION)
    assert lib.pyr_scene_set_skin_blend(None, None, 1) == abi.PYR_ERR_INVALID_ARGUMENT and b"null modes" in lib.pyr_last_error()
    assert lib.pyr_scene_set_skin_blend(None, None, 0) == abi.PYR_ERR_INVALID_ARGUMENT and b"null modes" in lib.pyr_last_error()
    assert lib.pyr_scene_set_skin_blend(None, modes, 1) == abi.PYR_ERR_INVALID_ARGUMENT and b"null scene" in lib.pyr_last_error()


# ---------------------------------------------------------------------------------------------------------------- (c) the world
def test_the_world_takes_a_blend_per_skin_and_refuses_an_unknown_one():
    world, _, _, _, ranges, rest, skins = skin_cases.build("knot")
    (index, skin), = skins.items()
    assert world._skins[index]["blend"] == "linear"  # the default
    world.set_skins({index: dict(skin, blend="dual_quaternion")})
    assert world._skins[index]["blend"] == "dual_quaternion"
    with pytest.raises(ValueError):
        world.set_skins({index: dict(skin, blend="spherical")})
    assert world._skins[index]["blend"] == "dual_quaternion"  # a refused call leaves the skins as they were
    world.set_skins({index: skin})
    assert world._skins[index]["blend"] == "linear"
    assert not world._scenes  # nothing above made a scene


def test_the_joints_of_the_cases_are_rigid_and_the_sign_flip_is_taken_by_some_vertices_of_every_shape():
    for table in (RIGID, dq_skin_cases.OTHER, dq_skin_cases.TWIST):
        for m in skin_restatement.joint_table(table, len(table)):
            assert restatement.is_rotation(m) and np.array_equal(m[[3, 7, 11, 15]], np.float32([0, 0, 0, 1]))
    assert not restatement.is_rotation(skin_restatement.joint_table(skin_cases.THREE, 3)[2])  # the non-uniform matrix of skin_cases
    quats = restatement.joint_dual_quaternions(skin_restatement.joint_table(RIGID, 3))
    assert restatement.dot4(quats[0:1, :4], quats[1:2, :4])[0] < 0 and quats[1, 0] < 0  # 200 degrees about z against the pivot
    for shape in dq_skin_cases.SHAPES:
        world, _, _, _, ranges = cases.build(shape)
        rest, index = cases.rest_of(world), skin_cases.skinned_object(world)
        taken = dq_skin_cases.flipped(dq_skin_cases.binding("bend", rest, ranges[index]), RIGID)
        assert taken.any() and not taken.all(), shape


# ---------------------------------------------------------------------------------------------------------------- (d) the closed form
def test_the_linear_blend_collapses_the_twisted_cylinder_and_the_dual_quaternion_blend_keeps_it():
    """Joints 170 degrees apart about the cylinder's axis. Under the dual quaternion blend every vertex is rest turned about z by a
    unit quaternion: its distance from the axis and its z are rest's within 1e-5 relative (a quaternion normalised in f32 moves them
    by a few ulp of 6e-8; this is about a hundred times that). Under the linear blend the ring at z = 0.5 is rest scaled by
    cos 85 degrees = 0.087."""
    rest, ranges = dq_skin_cases.twist_rest()
    assert len(rest["positions"]) == 256
    joints = {0: dq_skin_cases.TWIST}
    dual = restatement.dq_skin_arrays(rest, ranges, {0: dq_skin_cases.twist_binding(rest, "dual_quaternion")}, joints)
    radius, z, rest_radius, rest_z = dq_skin_cases.twist_radii(dual, ranges[0], rest)
    assert np.abs(rest_radius - 1.0).max() < 1e-6
    assert np.abs(radius - rest_radius).max() <= 1e-5 * rest_radius.max()
    assert np.abs(z - rest_z).max() <= 1e-5
    assert not np.array_equal(bits(dual["positions"]), bits(rest["positions"]))
    linear = skin_restatement.skin_arrays(rest, ranges, {0: dq_skin_cases.twist_binding(rest, "linear")}, joints)
    radius, z, _, rest_z = dq_skin_cases.twist_radii(linear, ranges[0], rest)
    middle = rest_z == 0.5
    assert middle.sum() == 6 * dq_skin_cases.TWIST_SEGMENTS  # the ring's sixteen vertices, each a corner of six triangles
    assert radius[middle].max() < 0.1 and radius[middle].min() > 0.08
    # and the restatement's linear path is skin_restatement's
    same = restatement.dq_skin_arrays(rest, ranges, {0: dq_skin_cases.twist_binding(rest, "linear")}, joints)
    assert all(np.array_equal(bits(same[key]), bits(linear[key])) for key in ("positions", "normals"))


# ---------------------------------------------------------------------------------------------------------------- (e) the rehearsal
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("dq_skin_check")), "dq_skin_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "probes", "dq_skin_check.cpp")])
    return exe


MODES = {"linear": 0, "dual_quaternion": 1}


def rehearse(exe, tmp_path, name, rest, ranges, skins, joints, poses={}, status=0):
    source, result = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
    with open(source, "wb") as f:
        f.write(np.array([len(rest["positions"]), 0 if rest["frames"] is None else 1, len(ranges), len(skins)], dtype=np.uint32).tobytes())
        for key in KEYS:
            if rest[key] is not None:
                f.write(np.ascontiguousarray(rest[key], dtype=np.float32).tobytes())
        for k, r in enumerate(ranges):
            matrix, scale = poses.get(k, (None, 1.0))
            f.write(np.array([r["first_triangle"], r["num_triangles"]], dtype=np.uint32).tobytes())
            f.write(pose_restatement.column_major(matrix).tobytes())
            f.write(np.float32(scale).tobytes())
        for index in sorted(skins):
            skin = skins[index]
            f.write(np.array([index, skin["num_joints"], MODES[restatement.blend_of(skin)]], dtype=np.uint32).tobytes())
            f.write(skin_restatement.joint_table(joints.get(index), skin["num_joints"]).tobytes())
            f.write(np.ascontiguousarray(skin["weights"], dtype=np.float32).tobytes())
            f.write(np.ascontiguousarray(skin["joints"], dtype=np.uint16).tobytes())
    run = subprocess.run([exe, source, result], capture_output=True, text=True, timeout=120)
    assert run.returncode == status, run.stdout + run.stderr
    if status:
        return None
    data = np.fromfile(result, dtype=np.float32)
    out, at = {}, 0
    for key in KEYS:
        if rest[key] is None:
            out[key] = None
            continue
        out[key] = data[at:at + rest[key].size].reshape(rest[key].shape)
        at += rest[key].size
    assert at + 1 == len(data)
    out["flag"] = int(data[at:].view(np.uint32)[0])
    return out


@pytest.fixture(scope="module")
def rehearsal_inputs():
    """name -> (rest, ranges, skinned object): the Cornell box, the textures example with its frames, the knot with a rigid object
    beside the skin (288 lanes: more than one workgroup on the device)."""
    out = {}
    for shape in dq_skin_cases.SHAPES:
        world, _, _, _, ranges = cases.build(shape)
        out[shape] = (cases.rest_of(world), ranges, skin_cases.skinned_object(world))
    return out


def assert_same(got, want, rest, what):
    for key in KEYS:
        if rest[key] is None:
            continue
        assert np.array_equal(bits(got[key]), bits(want[key])), (what, key, int((bits(got[key]) != bits(want[key])).sum()))
        assert np.isfinite(got[key]).all(), (what, key)


@pytest.mark.parametrize("pose", ["identity", "rotated_and_translated"])
@pytest.mark.parametrize("binding", dq_skin_cases.BINDINGS)
def test_the_host_rehearsal_of_the_dual_quaternion_kernel_under_sanitizers(probe, rehearsal_inputs, tmp_path, binding, pose):
    """pose_rules.h on the CPU against the restatement, as bits: positions, normals and frames of every shape, with and without an
    object pose on top. one_hot: B is J[0] re-made from its dual quaternion, so the skin is the rigid pose by that matrix."""
    for name, (rest, ranges, index) in rehearsal_inputs.items():
        skins = {index: dq_skin_cases.binding(binding, rest, ranges[index])}
        joints = {index: RIGID}
        poses = skin_cases.object_poses(pose, len(ranges))
        got = rehearse(probe, tmp_path, name, rest, ranges, skins, joints, poses)
        want = restatement.dq_skin_arrays(rest, ranges, skins, joints, poses)
        assert_same(got, want, rest, (name, binding, pose))
        assert not np.array_equal(bits(got["positions"]), bits(rest["positions"])), (name, binding)
        assert got["flag"] == 0
        linear = skin_restatement.skin_arrays(rest, ranges, skins, joints, poses)
        assert not np.array_equal(bits(got["positions"]), bits(linear["positions"])), (name, binding)  # it is another blend
        if binding == "one_hot" and pose == "identity":
            quats = restatement.joint_dual_quaternions(skin_restatement.joint_table(RIGID, 3))
            remade, bad = restatement.blend_dual_quaternions(quats, [[0, 0, 0, 0]], [[1, 0, 0, 0]])
            assert not bad.any()
            rigid = pose_restatement.pose_arrays(rest, ranges, {index: (remade[:, 0].copy(), 1.0)})
            assert_same(got, rigid, rest, (name, "the rigid pose by J[0] re-made"))
            # (and that matrix is J[0] up to rounding: some thirty f32 operations on values below 1, half an ulp of 6e-8 each)
            assert np.abs(remade[:, 0] - skin_restatement.joint_table(RIGID, 3)[0]).max() < 2e-6


def test_all_identity_joints_copy_rests_bits(probe, rehearsal_inputs, tmp_path):
    for name, (rest, ranges, index) in rehearsal_inputs.items():
        skins = {index: dq_skin_cases.binding("bend", rest, ranges[index])}
        got = rehearse(probe, tmp_path, name, rest, ranges, skins, {})
        assert_same(got, rest, rest, name)
        assert got["flag"] == 0


def test_a_skin_with_every_mode_linear_is_the_linear_restatement(probe, rehearsal_inputs, tmp_path):
    for name, (rest, ranges, index) in rehearsal_inputs.items():
        skins = {index: skin_cases.binding("bend", rest, ranges[index])}
        joints = {index: skin_cases.THREE}
        poses = skin_cases.object_poses("rotated_and_translated", len(ranges))
        got = rehearse(probe, tmp_path, name, rest, ranges, skins, joints, poses)
        assert_same(got, skin_restatement.skin_arrays(rest, ranges, skins, joints, poses), rest, name)
        assert_same(got, restatement.dq_skin_arrays(rest, ranges, skins, joints, poses), rest, name)
        assert got["flag"] == 0


def test_the_rehearsal_keeps_the_twisted_cylinder(probe, tmp_path):
    rest, ranges = dq_skin_cases.twist_rest()
    skins, joints = {0: dq_skin_cases.twist_binding(rest, "dual_quaternion")}, {0: dq_skin_cases.TWIST}
    got = rehearse(probe, tmp_path, "twist", rest, ranges, skins, joints)
    assert_same(got, restatement.dq_skin_arrays(rest, ranges, skins, joints), rest, "twist")
    radius, z, rest_radius, rest_z = dq_skin_cases.twist_radii(got, ranges[0], rest)
    assert np.abs(radius - rest_radius).max() <= 1e-5 * rest_radius.max() and np.abs(z - rest_z).max() <= 1e-5 and got["flag"] == 0


def test_a_joint_that_is_no_rotation_is_what_the_rule_says_it_is(probe, rehearsal_inputs, tmp_path):
    """The rehearsal ends with status 4 where pyr_scene_skin refuses (pose_rules.h joint_is_rotation, which both call): a scaled
    column, a sheared pair, a mirrored matrix -- each just outside 1e-3 -- and takes what is just inside."""
    rest, ranges, index = rehearsal_inputs["cornell"]
    skins = {index: dq_skin_cases.binding("bend", rest, ranges[index])}

    def table(change):
        t = RIGID.copy()  # [3,4,4] as on paper
        t[1, :3, :3] = (t[1, :3, :3].astype(np.float64) @ change).astype(np.float32)
        return t

    scaled, sheared, mirrored = np.diag([1.002, 1.0, 1.0]), np.eye(3), np.diag([1.0, 1.0, -1.0])
    sheared[0, 1] = 0.002
    inside = np.diag([1.0002, 1.0, 1.0])
    for name, change, status in (("scaled", scaled, 4), ("sheared", sheared, 4), ("mirrored", mirrored, 4), ("inside", inside, 0)):
        t = table(change)
        assert restatement.is_rotation(skin_restatement.joint_table(t, 3)[1]) == (status == 0), name
        rehearse(probe, tmp_path, name, rest, ranges, skins, {index: t}, status=status)
    linear = {index: skin_cases.binding("bend", rest, ranges[index])}
    rehearse(probe, tmp_path, "linear", rest, ranges, linear, {index: table(mirrored)})  # a linear skin takes any matrix


def test_antipodal_rotations_under_equal_weights_raise_bit_3_and_nothing_else_does(probe, tmp_path):
    """The raw mode: a table of (r, d) taken as it is. Joints 1 and 2 are q and -q; the pivot, joint 0, is at a right angle to both
    (a dot of zero does not negate), so weights (0, .5, .5, 0) cancel the blend: bit 3, value 8. Every other vertex equals the
    restatement's blend applied to its point, and a joint index at the count uses joint 0 and raises bit 0."""
    q = np.float32([np.cos(0.4), 0.0, 0.0, np.sin(0.4)])
    table = np.zeros((3, 8), dtype=np.float32)
    table[0, :4], table[1, :4], table[2, :4] = (0, 1, 0, 0), q, -q
    table[1, 4:], table[2, 4:] = (0.1, 0.2, -0.3, 0.05), (0.1, 0.2, -0.3, 0.05)
    weights = np.float32([[0, 0.5, 0.5, 0], [0, 1, 0, 0], [0.25, 0.75, 0, 0], [0, 0.25, 0.75, 0], [1, 0, 0, 0], [0.5, 0.5, 0, 0]])
    indices = np.array([[0, 1, 2, 0], [0, 1, 2, 0], [0, 1, 2, 0], [0, 1, 2, 0], [0, 1, 2, 0], [1, 3, 0, 0]], dtype=np.uint16)
    points = np.float32([[1, 2, 3]] * len(weights))
    source, result = str(tmp_path / "raw.in"), str(tmp_path / "raw.out")
    with open(source, "wb") as f:
        f.write(np.array([len(table), len(weights)], dtype=np.uint32).tobytes())
        f.write(table.tobytes() + weights.tobytes() + indices.tobytes() + points.tobytes())
    run = subprocess.run([probe, "raw", source, result], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    data = np.fromfile(result, dtype=np.float32)
    moved, flags = data[:3 * len(weights)].reshape(-1, 3), data[3 * len(weights):].view(np.uint32)
    assert list(flags) == [8, 0, 0, 0, 0, 1]
    inside = indices.copy()
    inside[5, 1] = 0
    b, bad = restatement.blend_dual_quaternions(table, inside, weights)
    assert list(bad) == [True, False, False, False, False, False]
    want = pose_restatement.transform_point(b, points)
    assert np.array_equal(bits(moved[1:]), bits(want[1:]))
    assert restatement.signed_weights(table, indices[:5], weights[:5])[3, 2] == 0.75  # q and -q against the pivot at a right angle: no flip
