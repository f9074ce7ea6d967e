"""pyr_scene_set_skins / pyr_scene_skin without a GPU: the two new structs of the ABI, the argument checks that
need no scene, the world's bookkeeping, and the host rehearsal of the skin kernel -- pose_rules.h, the header kernels/pose.hip
compiles, through tests/probes/deform_check.cpp, a program of its own built with -fsanitize=address,undefined and run as a child
process -- compared as bits with the numpy restatement (tests/skin_restatement.py)."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_build_inputs as inputs  # noqa: E402
import deform_probe  # noqa: E402
import pose_cases as cases  # noqa: E402
import pose_restatement  # noqa: E402
import skin_cases  # noqa: E402
import skin_restatement as restatement  # noqa: E402

from pyrite_amd import abi  # noqa: E402
from pyrite_amd import build as gpu_build  # noqa: E402

HEADER = os.path.join(ROOT, "include", "pyrite_gpu.h")
STRUCTS = ["PyrSkin", "PyrSkinUpdate"]
KEYS = ("positions", "normals", "frames", "spheres")


# ---------------------------------------------------------------------------------------------------------------- (a) the ABI
def test_header_and_ctypes_agree_on_the_skin_structs():
    """sizeof / offsetof as gcc lays the header out, against the ctypes mirrors; additions only, so the ABI version stays."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "%s"' % HEADER, "int main(void){"]
    for s in STRUCTS:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for field, _ in getattr(abi, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, field, s, field))
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    expect = dict(l.split() for l in out if l)
    for s in STRUCTS:
        cls = getattr(abi, s)
        assert int(expect[s]) == C.sizeof(cls), s
        for field, _ in cls._fields_:
            assert int(expect["%s.%s" % (s, field)]) == getattr(cls, field).offset, "%s.%s" % (s, field)
        assert dict(cls._fields_)["reserved"]._length_ == 4
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+PYR_ABI_VERSION\s+5\b", text) and abi.PYR_ABI_VERSION == 5
    for name in ("pyr_scene_set_skins", "pyr_scene_skin"):
        assert name in abi.ENTRY_POINTS and re.search(r"\bint\s+%s\s*\(" % name, text)


# ---------------------------------------------------------------------------------------------------------------- (b) refusals
@pytest.fixture(scope="module")
def lib():
    return abi.bind(C.CDLL(gpu_build.build()))


def test_bad_arguments_are_refused_before_any_device_is_looked_for(lib):
    """No GPU here: anything that reached the device would be PYR_ERR_DEVICE. pyr_last_error names the argument. Every other
    refusal of these calls needs a scene (tests/test_gpu_scene_skin.py)."""
    good = abi.PyrSkinUpdate(mode=abi.PYR_UPDATE_REFIT)
    assert lib.pyr_scene_skin(None, None, None) == abi.PYR_ERR_INVALID_ARGUMENT and b"null update" in lib.pyr_last_error()
    assert lib.pyr_scene_skin(None, C.byref(good), None) == abi.PYR_ERR_INVALID_ARGUMENT and b"null scene" in lib.pyr_last_error()
    skins = (abi.PyrSkin * 1)(abi.PyrSkin(object=0, num_joints=1))
    assert lib.pyr_scene_set_skins(None, skins, 1) == abi.PYR_ERR_INVALID_ARGUMENT and b"null scene" in lib.pyr_last_error()
    assert lib.pyr_scene_set_skins(None, None, 0) == abi.PYR_ERR_INVALID_ARGUMENT and b"null scene" in lib.pyr_last_error()
    assert lib.pyr_scene_set_skins(None, None, 2) == abi.PYR_ERR_INVALID_ARGUMENT and b"skins" in lib.pyr_last_error()


# ---------------------------------------------------------------------------------------------------------------- (d) the world
def test_the_world_checks_skins_and_joints_before_any_scene_is_made():
    from pyrite_amd.renderer import World

    world, _, _, _, ranges, rest, skins = skin_cases.build("knot")
    assert callable(World.skin) and callable(World.set_skins)
    with pytest.raises(ValueError):
        world.skin({1: skin_cases.THREE})  # object 1 has no skin
    with pytest.raises(ValueError):
        world.skin({7: skin_cases.THREE})  # no such object
    with pytest.raises(ValueError):
        world.skin({0: skin_cases.THREE}, poses={2: (None, 1.0)})  # no such object to pose
    with pytest.raises(ValueError):
        world.skin({0: skin_cases.THREE[:2]})  # two matrices for three joints
    with pytest.raises(ValueError):
        world.skin({0: skin_cases.THREE}, mode="bend")
    good = skins[0]
    for joints, weights in ((good["joints"][:-1], good["weights"]), (good["joints"], good["weights"][:, :, :3]), (good["joints"].reshape(-1, 4), good["weights"].reshape(-1, 4))):
        with pytest.raises(ValueError):
            world.set_skins({0: dict(joints=joints, weights=weights, num_joints=3)})
    with pytest.raises(ValueError):
        world.set_skins({2: good})  # no such object
    assert not world._scenes  # nothing above made a scene


def test_the_bindings_of_the_cases_are_what_the_tests_take_them_for():
    """Weights that are finite, not negative and sum to 1 within f32 rounding; joints below the count; `three` with last rows 0,0,0,1."""
    for shape in skin_cases.SHAPES:
        for name in skin_cases.BINDINGS:
            _, _, _, _, ranges, rest, skins = skin_cases.build(shape, name)
            (index, skin), = skins.items()
            w = skin["weights"].reshape(-1, 4)
            assert skin["weights"].shape == skin["joints"].shape == (ranges[index]["num_triangles"], 3, 4)
            assert np.isfinite(w).all() and (w >= 0).all() and skin["joints"].max() < skin["num_joints"]
            total = ((w[:, 0] + w[:, 1]).astype(np.float32) + w[:, 2]).astype(np.float32) + w[:, 3]
            assert np.abs(total - np.float32(1.0)).max() <= 1e-6, (shape, name)
    assert np.array_equal(skin_cases.THREE[:, 3], np.tile(np.float32([0, 0, 0, 1]), (3, 1)))


# ---------------------------------------------------------------------------------------------------------------- (c) the rehearsal
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def skin_check(tmp_path_factory):
    return deform_probe.build(tmp_path_factory.mktemp("deform_check"))


@pytest.fixture(scope="module")
def rehearsal_inputs():
    """name -> (rest, ranges, lamps, skinned object): the Cornell box (its lamp triangles inside the skin), the textures example with
    its frames, the knot with a rigid object beside the skin, and the smallest tie-free mesh of tests/bvh_build_inputs.py (one
    triangle; flat normals; taken as a lamp for the area)."""
    out = {}
    for shape in skin_cases.SHAPES:
        world, _, _, _, ranges = cases.build(shape)
        out[shape] = (cases.rest_of(world), ranges, cases.shape_lamps(world), skin_cases.skinned_object(world))
    smallest = min(inputs.TIE_FREE, key=lambda name: len(inputs.TIE_FREE[name]()[1]) if len(inputs.TIE_FREE[name]()[1]) else 1 << 30)
    _, tris = inputs.TIE_FREE[smallest]()
    t = tris.reshape(-1, 3, 3)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    rest = {"positions": tris.astype(np.float32), "normals": np.repeat(n[:, None, :], 3, axis=1).reshape(-1, 9), "frames": None, "spheres": np.zeros((0, 4), dtype=np.float32)}
    out[smallest] = (rest, [cases.triangles(0, len(tris))], [(1, 0)], 0)
    return out


def rehearse(skin_check, tmp_path, name, rest, ranges, poses, lamps, skins, joints):
    return deform_probe.rehearse(skin_check, tmp_path, name, rest, ranges, lamps, poses=poses, skins=skins, joints=joints)


@pytest.mark.parametrize("pose", ["identity", "rotated_and_translated"])
@pytest.mark.parametrize("binding", skin_cases.BINDINGS)
def test_the_host_rehearsal_of_the_skin_kernel_under_sanitizers(skin_check, rehearsal_inputs, tmp_path, binding, pose):
    """pose_rules.h on the CPU against the restatement, as bits: positions, normals and frames of every input, with and without an
    object pose on top; the lamp records are the skinned arrays' and their areas pack_lamp's formula restated in numpy."""
    for name, (rest, ranges, lamps, index) in rehearsal_inputs.items():
        skins = {index: skin_cases.binding(binding, rest, ranges[index])}
        joints = {index: skin_cases.THREE}
        poses = skin_cases.object_poses(pose, len(ranges))
        got = rehearse(skin_check, tmp_path, name, rest, ranges, poses, lamps, skins, joints)
        want = restatement.skin_arrays(rest, ranges, skins, joints, poses)
        for key in KEYS:
            if rest[key] is None:
                continue
            assert np.array_equal(bits(got[key]), bits(want[key])), (name, binding, pose, key, int((bits(got[key]) != bits(want[key])).sum()))
            assert np.isfinite(got[key]).all()
        assert not np.array_equal(bits(got["positions"]), bits(rest["positions"])), (name, binding)
        assert got["flag"] == 0
        if binding == "one_hot" and pose == "identity":  # B is J[0] exactly: the rigid pose by J[0]
            rigid = pose_restatement.pose_arrays(rest, ranges, {index: (skin_cases.THREE[0], 1.0)})
            assert all(np.array_equal(bits(got[key]), bits(rigid[key])) for key in KEYS if rest[key] is not None), name
        areas = pose_restatement.lamp_areas(want, lamps)
        for k, (kind, at) in enumerate(lamps):
            record = got["lamps"][k]
            assert bits(record[22:23])[0] == bits(areas[k:k + 1])[0], (name, binding, pose, k)
            if kind == 0:
                assert np.array_equal(bits(record[0:4]), bits(want["spheres"][at]))
            else:
                assert np.array_equal(bits(record[4:13]), bits(want["positions"][at])) and np.array_equal(bits(record[13:22]), bits(want["normals"][at]))


def test_the_identity_table_gives_rest_bit_for_bit(skin_check, rehearsal_inputs, tmp_path):
    for name, (rest, ranges, lamps, index) in rehearsal_inputs.items():
        skins = {index: skin_cases.binding("bend", rest, ranges[index])}
        got = rehearse(skin_check, tmp_path, name, rest, ranges, {}, lamps, skins, {})
        assert all(np.array_equal(bits(got[key]), bits(rest[key])) for key in KEYS if rest[key] is not None), name
        assert got["flag"] == 0


def test_the_rehearsal_raises_the_flag_beyond_the_coordinate_range(skin_check, rehearsal_inputs, tmp_path):
    rest, ranges, lamps, index = rehearsal_inputs["knot"]
    skins = {index: skin_cases.binding("bend", rest, ranges[index])}
    far = skin_cases.THREE.copy()
    far[1, 0, 3] = 1e16  # joint 1 translated out of the coordinate range
    got = rehearse(skin_check, tmp_path, "far", rest, ranges, {}, lamps, skins, {index: far})
    assert got["flag"] == 1


def test_a_joint_index_at_the_skins_count_uses_joint_0_and_raises_bit_0(skin_check, rehearsal_inputs, tmp_path):
    """The guard the skin kernel and the rehearsal share (pose_rules.h skin_vertex): a binding pyr_scene_set_skins would have refused.
    One index equal to num_joints: the rehearsal ends clean under the sanitizers, bit 0 is set, and that vertex has the bits the
    restatement gives with the index replaced by 0; every other word is the unbroken binding's."""
    rest, ranges, lamps, index = rehearsal_inputs["knot"]
    good = skin_cases.binding("bend", rest, ranges[index])
    slot = 1  # (bend names joints 0, 1, 2, 0): the first vertex on which joint 1 weighs anything
    triangle, vertex = (int(x) for x in np.argwhere(np.asarray(good["weights"], dtype=np.float32).reshape(-1, 3, 4)[:, :, slot] > 0.25)[0])
    broken, replaced = (dict(good, joints=np.array(good["joints"], dtype=np.uint16).reshape(-1, 3, 4).copy()) for _ in range(2))
    broken["joints"][triangle, vertex, slot] = good["num_joints"]
    replaced["joints"][triangle, vertex, slot] = 0
    joints = {index: skin_cases.THREE}
    got = rehearse(skin_check, tmp_path, "beyond", rest, ranges, {}, lamps, {index: broken}, joints)
    assert got["flag"] & 1
    want = restatement.skin_arrays(rest, ranges, {index: replaced}, joints, {})
    for key in KEYS:
        if rest[key] is not None:
            assert np.array_equal(bits(got[key]), bits(want[key])), key
    unbroken = restatement.skin_arrays(rest, ranges, {index: good}, joints, {})
    at = ranges[index]["first_triangle"] + triangle
    assert not np.array_equal(bits(want["positions"][at]), bits(unbroken["positions"][at]))  # the replacement moved the vertex
    others = np.arange(len(rest["positions"])) != at
    assert np.array_equal(bits(got["positions"][others]), bits(unbroken["positions"][others]))
