"""pyr_scene_set_morphs / pyr_scene_morph without a GPU: the two new structs of the ABI, the argument checks
that need no scene, the world's bookkeeping, what the cases are, and the host rehearsal of the morph kernel -- pose_rules.h, the
header kernels/pose.hip compiles, through tests/probes/deform_check.cpp, a program of its own built with
-fsanitize=address,undefined and run as a child process -- compared as bits with the numpy restatement
(tests/morph_restatement.py)."""
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
import morph_cases  # noqa: E402
import morph_restatement as restatement  # noqa: E402
import pose_cases as cases  # noqa: E402
import pose_restatement  # noqa: E402
import skin_cases  # noqa: E402
import skin_restatement  # noqa: E402

from pyrite_amd import abi  # noqa: E402
from pyrite_amd import build as gpu_build  # noqa: E402

HEADER = os.path.join(ROOT, "include", "pyrite_gpu.h")
STRUCTS = ["PyrMorph", "PyrMorphUpdate"]
KEYS = ("positions", "normals", "frames", "spheres")
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- (a) the ABI
def test_header_and_ctypes_agree_on_the_morph_structs():
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
    for name in ("pyr_scene_set_morphs", "pyr_scene_morph"):
        assert name in abi.ENTRY_POINTS and re.search(r"\bint\s+%s\s*\(" % name, text)


# ---------------------------------------------------------------------------------------------------------------- (b) refusals
@pytest.fixture(scope="module")
def lib():
    return abi.bind(C.CDLL(gpu_build.build()))


def test_bad_arguments_are_refused_before_any_device_is_looked_for(lib):
    """No GPU here: anything that reached the device would be PYR_ERR_DEVICE. pyr_last_error names the argument. Every other
    refusal of these calls needs a scene (tests/test_gpu_scene_morph.py)."""
    good = abi.PyrMorphUpdate(mode=abi.PYR_UPDATE_REFIT)
    assert lib.pyr_scene_morph(None, None, None) == abi.PYR_ERR_INVALID_ARGUMENT and b"null update" in lib.pyr_last_error()
    assert lib.pyr_scene_morph(None, C.byref(good), None) == abi.PYR_ERR_INVALID_ARGUMENT and b"null scene" in lib.pyr_last_error()
    morphs = (abi.PyrMorph * 1)(abi.PyrMorph(object=0, num_targets=1))
    assert lib.pyr_scene_set_morphs(None, morphs, 1) == abi.PYR_ERR_INVALID_ARGUMENT and b"null scene" in lib.pyr_last_error()
    assert lib.pyr_scene_set_morphs(None, None, 0) == abi.PYR_ERR_INVALID_ARGUMENT and b"null scene" in lib.pyr_last_error()
    assert lib.pyr_scene_set_morphs(None, None, 2) == abi.PYR_ERR_INVALID_ARGUMENT and b"morphs" in lib.pyr_last_error()


# ---------------------------------------------------------------------------------------------------------------- (c) the world
def test_the_world_checks_morphs_and_weights_before_any_scene_is_made():
    from pyrite_amd.renderer import World

    world, _, _, _, ranges, rest, morphs, skins = morph_cases.build("knot")
    assert callable(World.morph) and callable(World.set_morphs)
    good = morphs[0]
    with pytest.raises(ValueError):
        world.morph({7: morph_cases.WEIGHTS})  # no such object
    with pytest.raises(ValueError):
        world.morph({0: morph_cases.WEIGHTS[:2]})  # two weights for three targets
    with pytest.raises(ValueError):
        world.morph({0: morph_cases.WEIGHTS}, poses={2: (None, 1.0)})  # no such object to pose
    with pytest.raises(ValueError):
        world.morph({0: morph_cases.WEIGHTS}, joints={1: skin_cases.THREE})  # object 1 has no skin
    with pytest.raises(ValueError):
        world.morph({0: morph_cases.WEIGHTS}, mode="bulge")
    for positions, normals in ((good["positions"][:, :-1], None), (good["positions"].reshape(3, -1, 9), None), (good["positions"], good["normals"][:2]),
                               (good["positions"][:0], None), (np.zeros((257,) + good["positions"].shape[1:], dtype=f32), None)):
        with pytest.raises(ValueError):
            world.set_morphs({0: dict(positions=positions, normals=normals)})
    with pytest.raises(ValueError):
        world.set_morphs({2: good})  # no such object
    assert sorted(world._morphs) == [0, 1] and sorted(world._skins) == [0] and world._weights == {}  # the refused calls changed nothing
    world.set_skins(skins)  # binding skins again leaves the morphs
    assert sorted(world._morphs) == [0, 1]
    world.set_morphs({1: morphs[1]})  # and new morphs leave the skins
    assert sorted(world._morphs) == [1] and sorted(world._skins) == [0]
    with pytest.raises(ValueError):
        world.morph({0: morph_cases.WEIGHTS})  # object 0 has no morph now
    world.set_objects(ranges)  # morphs hang on objects
    assert world._morphs == {} and world._weights == {} and world._skins == {}
    with pytest.raises(ValueError):
        world.morph({})  # no morphs
    assert not world._scenes  # nothing above made a scene


def test_the_targets_of_the_cases_are_what_the_tests_take_them_for():
    """Every delta finite, `poison` 1e30 throughout, every weight table's last entry exactly 0, and -- on the restatement, so that
    the reference alone stays off the flag -- every morphed normal's squared length inside [1e-30, 1e30] under the case weights."""
    for w in (morph_cases.WEIGHTS, morph_cases.OTHER, morph_cases.BULGE, morph_cases.ZERO):
        assert w.dtype == f32 and w.shape == (3,) and w[-1] == 0.0
    assert morph_cases.TARGETS[-1] == "poison"
    for shape in morph_cases.SHAPES:
        world, _, _, _, ranges, rest, morphs, skins = morph_cases.build(shape)
        assert sorted(morphs) == morph_cases.morphed_objects(shape, world)
        for index, morph in morphs.items():
            n = ranges[index]["num_triangles"]
            assert n > 0 and morph["positions"].shape == morph["normals"].shape == (3, n, 3, 3)
            assert np.isfinite(morph["positions"]).all() and np.isfinite(morph["normals"]).all()
            assert (morph["positions"][2] == f32(1e30)).all() and (morph["normals"][2] == f32(1e30)).all()
            assert np.abs(morph["positions"][:2]).max() > 0 and np.abs(morph["normals"][:2]).max() > 0
            for w in (morph_cases.WEIGHTS, morph_cases.OTHER, morph_cases.BULGE):
                start = rest["normals"][ranges[index]["first_triangle"]:ranges[index]["first_triangle"] + n].reshape(-1, 3)
                m = restatement.accumulated(start, morph["normals"], w)
                s = restatement.dot(m, m)
                assert (s >= f32(1e-30)).all() and (s <= f32(1e30)).all() and s.min() > 0.01, (shape, index)
        for w in (morph_cases.WEIGHTS, morph_cases.OTHER, morph_cases.BULGE):
            arrays, flag = restatement.morphed(rest, ranges, morphs, morph_cases.table(morphs, w))
            assert flag == 0 and all(np.isfinite(arrays[k]).all() for k in KEYS if arrays[k] is not None), shape
    world, _, _, _, ranges, _, morphs, skins = morph_cases.build("knot")
    assert ranges[0]["num_triangles"] == 288 and ranges[1]["num_triangles"] == 352 and sorted(skins) == [0]


# ---------------------------------------------------------------------------------------------------------------- (d) the rehearsal
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def morph_check(tmp_path_factory):
    return deform_probe.build(tmp_path_factory.mktemp("deform_check"))


@pytest.fixture(scope="module")
def rehearsal_inputs():
    """name -> (rest, ranges, lamps, morphed objects, skinned objects): the three shapes (the Cornell box's lamp triangles inside the
    morph; the textures example with its frames; the knot with a skinned and a rigid morphed object) and the smallest tie-free
    mesh of tests/bvh_build_inputs.py (flat normals; taken as a lamp for the area)."""
    out = {}
    for shape in morph_cases.SHAPES:
        world, _, _, _, ranges = cases.build(shape)
        morphed = morph_cases.morphed_objects(shape, world)
        out[shape] = (cases.rest_of(world), ranges, cases.shape_lamps(world), morphed, morphed[:1])
    smallest = min(inputs.TIE_FREE, key=lambda name: len(inputs.TIE_FREE[name]()[1]) if len(inputs.TIE_FREE[name]()[1]) else 1 << 30)
    _, tris = inputs.TIE_FREE[smallest]()
    t = tris.reshape(-1, 3, 3)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    rest = {"positions": tris.astype(np.float32), "normals": np.repeat(n[:, None, :], 3, axis=1).reshape(-1, 9), "frames": None, "spheres": np.zeros((0, 4), dtype=np.float32)}
    out[smallest] = (rest, [cases.triangles(0, len(tris))], [(1, 0)], [0], [0])
    return out


def rehearse(morph_check, tmp_path, name, rest, ranges, poses, lamps, skins, joints, morphs, weights):
    return deform_probe.rehearse(morph_check, tmp_path, name, rest, ranges, lamps, poses=poses, skins=skins, joints=joints, morphs=morphs, weights=weights)


def targets_of(rest, ranges, morphed, with_normals=True):
    return {index: morph_cases.targets(rest, ranges[index], with_normals) for index in morphed}


def assert_same_bits(got, want, rest, what):
    for key in KEYS:
        if rest[key] is not None:
            assert np.array_equal(bits(got[key]), bits(want[key])), (what, key, int((bits(got[key]) != bits(want[key])).sum()))


@pytest.mark.parametrize("pose", ["identity", "rotated_and_translated"])
@pytest.mark.parametrize("skinned", [False, True])
@pytest.mark.parametrize("with_normals", [True, False])
def test_the_host_rehearsal_of_the_morph_kernel_under_sanitizers(morph_check, rehearsal_inputs, tmp_path, with_normals, skinned, pose):
    """pose_rules.h on the CPU against the restatement, as bits: positions, normals and frames of every input, with and without
    normal deltas, a skin and an object pose on top; the lamp records are the morphed arrays' and their areas pack_lamp's formula
    restated in numpy."""
    for name, (rest, ranges, lamps, morphed, skinnable) in rehearsal_inputs.items():
        morphs = targets_of(rest, ranges, morphed, with_normals)
        weights = morph_cases.table(morphs, morph_cases.WEIGHTS)
        skins = {index: skin_cases.bend(rest, ranges[index]) for index in skinnable} if skinned else {}
        joints = {index: skin_cases.THREE for index in skins}
        poses = skin_cases.object_poses(pose, len(ranges))
        got = rehearse(morph_check, tmp_path, name, rest, ranges, poses, lamps, skins, joints, morphs, weights)
        want = restatement.morph_arrays(rest, ranges, morphs, weights, skins, joints, poses)
        what = (name, with_normals, skinned, pose)
        assert_same_bits(got, want, rest, what)
        assert all(np.isfinite(got[key]).all() for key in KEYS if rest[key] is not None), what
        assert not np.array_equal(bits(got["positions"]), bits(rest["positions"])), what
        assert got["flag"] == 0, what
        if not with_normals and not skinned and pose == "identity":  # normals and frames stay rest's in every word
            assert np.array_equal(bits(got["normals"]), bits(rest["normals"])), what
            assert rest["frames"] is None or np.array_equal(bits(got["frames"]), bits(rest["frames"])), what
        areas = pose_restatement.lamp_areas(want, lamps)
        for k, (kind, at) in enumerate(lamps):
            record = got["lamps"][k]
            assert bits(record[22:23])[0] == bits(areas[k:k + 1])[0], (what, k)
            if kind == 0:
                assert np.array_equal(bits(record[0:4]), bits(want["spheres"][at]))
            else:
                assert np.array_equal(bits(record[4:13]), bits(want["positions"][at])) and np.array_equal(bits(record[13:22]), bits(want["normals"][at]))


def test_zero_weights_give_rest_and_poison_under_weight_zero_changes_no_bit(morph_check, rehearsal_inputs, tmp_path):
    for name, (rest, ranges, lamps, morphed, _) in rehearsal_inputs.items():
        morphs = targets_of(rest, ranges, morphed)
        for zero in (0.0, -0.0):  # both zeros are inactive
            got = rehearse(morph_check, tmp_path, name, rest, ranges, {}, lamps, {}, {}, morphs, morph_cases.table(morphs, [zero, zero, zero]))
            assert_same_bits(got, rest, rest, (name, "zero weights"))
            assert got["flag"] == 0
        clean = {index: dict(positions=m["positions"][:2], normals=m["normals"][:2]) for index, m in morphs.items()}  # the same morph without its poison
        with_poison = rehearse(morph_check, tmp_path, name, rest, ranges, {}, lamps, {}, {}, morphs, morph_cases.table(morphs, morph_cases.WEIGHTS))
        without = rehearse(morph_check, tmp_path, name + "_clean", rest, ranges, {}, lamps, {}, {}, clean, morph_cases.table(clean, morph_cases.WEIGHTS[:2]))
        assert_same_bits(with_poison, without, rest, (name, "poison"))
        assert np.array_equal(bits(with_poison["lamps"]), bits(without["lamps"])) and with_poison["flag"] == without["flag"] == 0


def test_the_rehearsal_raises_the_two_flag_bits(morph_check, rehearsal_inputs, tmp_path):
    """Bit 1 (value 2) for a target with dn = -n at weight 1: the morphed normal is exactly zero. Bit 0 (value 1) for a position
    delta of 1e16 at weight 1: beyond the coordinate range. The restatement says the same of the first."""
    rest, ranges, lamps, morphed, _ = rehearsal_inputs["knot"]
    index = morphed[0]
    t0, n = ranges[index]["first_triangle"], ranges[index]["num_triangles"]
    collapse = {index: dict(positions=np.zeros((1, n, 3, 3), dtype=f32), normals=(-rest["normals"][t0:t0 + n]).reshape(1, n, 3, 3).astype(f32))}
    got = rehearse(morph_check, tmp_path, "collapse", rest, ranges, {}, lamps, {}, {}, collapse, {index: [1.0]})
    assert got["flag"] == 2
    assert restatement.morph_flag(rest, ranges, collapse, {index: [1.0]}) == 2
    far = np.zeros((1, n, 3, 3), dtype=f32)
    far[0, 5, 1, 0] = 1e16
    away = {index: dict(positions=far, normals=None)}
    got = rehearse(morph_check, tmp_path, "far", rest, ranges, {}, lamps, {}, {}, away, {index: [1.0]})
    assert got["flag"] == 1
