"""pyr_scene_set_smoothing without a GPU: the new struct of the ABI, the argument checks that need no scene,
the world's bookkeeping and `weld`, what the cases are, the host rehearsal of the smoothing kernel -- pose_rules.h, the header
kernels/pose.hip compiles, through tests/probes/deform_check.cpp, a program of its own built with -fsanitize=address,undefined and
run as a child process -- compared as bits with the numpy restatement (tests/smooth_restatement.py), and what the recomputed
normals are worth against the float64 truth of an affine deformation."""
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
import deform_probe  # noqa: E402
import morph_cases  # noqa: E402
import morph_restatement  # noqa: E402
import pose_cases as cases  # noqa: E402
import pose_restatement  # noqa: E402
import skin_cases  # noqa: E402
import skin_restatement  # noqa: E402
import smooth_cases  # noqa: E402
import smooth_restatement as restatement  # noqa: E402

from pyrite_amd import abi  # noqa: E402
from pyrite_amd import build as gpu_build  # noqa: E402

HEADER = os.path.join(ROOT, "include", "pyrite_gpu.h")
KEYS = ("positions", "normals", "frames", "spheres")
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- (a) the ABI
def test_header_and_ctypes_agree_on_the_smoothing_struct():
    """sizeof / offsetof as gcc lays the header out, against the ctypes mirror; additions only, so the ABI version stays."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "%s"' % HEADER, "int main(void){"]
    lines.append('printf("PyrSmoothing %zu\\n", sizeof(PyrSmoothing));')
    for field, _ in abi.PyrSmoothing._fields_:
        lines.append('printf("PyrSmoothing.%s %%zu\\n", offsetof(PyrSmoothing, %s));' % (field, field))
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-o", exe, src])
        out = subprocess.check_output([exe]).decode().split("\n")
    expect = dict(l.split() for l in out if l)
    assert int(expect["PyrSmoothing"]) == C.sizeof(abi.PyrSmoothing) == 32
    for field, _ in abi.PyrSmoothing._fields_:
        assert int(expect["PyrSmoothing.%s" % field]) == getattr(abi.PyrSmoothing, field).offset, field
    assert dict(abi.PyrSmoothing._fields_)["reserved"]._length_ == 4
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+PYR_ABI_VERSION\s+5\b", text) and abi.PYR_ABI_VERSION == 5
    assert "pyr_scene_set_smoothing" in abi.ENTRY_POINTS and re.search(r"\bint\s+pyr_scene_set_smoothing\s*\(", text)


# ---------------------------------------------------------------------------------------------------------------- (b) refusals
@pytest.fixture(scope="module")
def lib():
    return abi.bind(C.CDLL(gpu_build.build()))


def test_bad_arguments_are_refused_before_any_device_is_looked_for(lib):
    """No GPU here: anything that reached the device would be PYR_ERR_DEVICE. pyr_last_error names the argument. Every other
    refusal of this call needs a scene (tests/test_gpu_scene_smooth.py)."""
    one = (abi.PyrSmoothing * 1)(abi.PyrSmoothing(object=0))
    assert lib.pyr_scene_set_smoothing(None, None, 2) == abi.PYR_ERR_INVALID_ARGUMENT and b"null smoothings" in lib.pyr_last_error()
    assert lib.pyr_scene_set_smoothing(None, one, 1) == abi.PYR_ERR_INVALID_ARGUMENT and b"null scene" in lib.pyr_last_error()
    assert lib.pyr_scene_set_smoothing(None, None, 0) == abi.PYR_ERR_INVALID_ARGUMENT and b"null scene" in lib.pyr_last_error()


def test_a_scene_without_smoothing_launches_no_new_kernel():
    """The launch of the smoothing kernel is behind the scene's group count on the host, and behind the context's in the launcher:
    read off the two units, since nothing here can run a kernel."""
    host = open(os.path.join(ROOT, "pyrite_amd", "csrc", "live_scene.cpp")).read()
    unit = open(os.path.join(ROOT, "pyrite_amd", "csrc", "kernels", "pose.hip")).read()
    assert host.count("launch_smooth(") == 1
    state = open(os.path.join(ROOT, "pyrite_amd", "csrc", "scene_internal.h")).read()
    assert re.search(r"if \(live\.smooth\.groups\) \{\s*const hipError_t es = devpose::launch_smooth\(", host)
    assert re.search(r"forget_smoothing\(\) \{\s*smooth\.clear\(\);", host)
    assert re.search(r"struct Smooth \{.*?void clear\(\) \{[^}]*groups = corners = 0;", state, re.S)
    assert re.search(r"launch_smooth\(const SmoothCtx& c, hipStream_t stream\) \{\s*if \(c\.num_groups\) hipLaunchKernelGGL\(smooth_normals_kernel,", unit)
    assert unit.count("smooth_normals_kernel") == 2  # its definition and that one launch


# ---------------------------------------------------------------------------------------------------------------- (c) the world
def test_weld_groups_corners_by_the_bits_of_position_and_normal():
    from pyrite_amd.renderer import weld

    p = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1, 0, 0], [1, 1, 0], [0, 1, 0]], [[0, 0, 0], [0, 1, 0], [0, 0, 1]]], dtype=f32)
    n = np.zeros_like(p)
    n[:2, :, 2] = 1.0
    n[2, :, 0] = -1.0  # the third triangle meets the first along an edge, with another normal: a crease
    ids = weld(p, n)
    assert ids.dtype == np.uint32 and ids.shape == (3, 3)
    assert ids.tolist() == [[0, 1, 2], [1, 4, 2], [6, 7, 8]]  # a label is its group's first corner
    assert np.array_equal(weld(p.reshape(-1, 9), n.reshape(-1, 9)), ids)
    minus = p.copy()
    minus[1, 0, 1] = -0.0  # the bits differ: +0 and -0 are two vertices
    assert weld(minus, n)[1, 0] == 3
    assert weld(np.zeros((0, 3, 3), dtype=f32), np.zeros((0, 3, 3), dtype=f32)).shape == (0, 3)
    with pytest.raises(ValueError):
        weld(p, n[:2])
    for shape in smooth_cases.SHAPES:  # and on the cases it is the restatement's grouping
        world, _, _, _, ranges = smooth_cases.make(shape)
        rest = cases.rest_of(world)
        for index, ids in smooth_cases.labels_for(shape, world, rest, ranges).items():
            t0, count = ranges[index]["first_triangle"], ranges[index]["num_triangles"]
            assert np.array_equal(restatement.groups_of(weld(rest["positions"][t0:t0 + count], rest["normals"][t0:t0 + count]))[0], restatement.groups_of(ids)[0])


def test_the_world_checks_a_smoothing_before_any_scene_is_made():
    from pyrite_amd.renderer import World

    world, _, _, _, ranges, rest, smoothing = smooth_cases.build("knot")
    assert callable(World.set_smoothing) and sorted(world._smoothing) == [0, 1] and not world._smooth_frame
    good = smoothing[0]
    for bad in (good[:-1], good.reshape(-1), good.astype(np.float32), good.astype(np.int64) - 1, np.full(good.shape, 1 << 32, dtype=np.int64)):
        with pytest.raises(ValueError):
            world.set_smoothing({0: bad})
    with pytest.raises(ValueError):
        world.set_smoothing({2: good})  # no such object
    assert sorted(world._smoothing) == [0, 1]  # the refused calls changed nothing
    world.set_smoothing({1: None})  # welded by the rest pose's own bits
    assert sorted(world._smoothing) == [1] and world._smoothing[1].dtype == np.uint32
    assert np.array_equal(restatement.groups_of(world._smoothing[1])[0], restatement.groups_of(smoothing[1])[0])
    skins = {0: skin_cases.bend(rest, ranges[0])}
    morphs = smooth_cases.morphs_for("knot", world, rest, ranges)
    world.set_skins(skins), world.set_morphs(morphs)  # each leaves the others' state alone
    assert sorted(world._smoothing) == [1] and sorted(world._skins) == [0] and sorted(world._morphs) == [0, 1]
    world.set_smoothing({})
    assert world._smoothing == {} and sorted(world._skins) == [0] and sorted(world._morphs) == [0, 1]
    world.set_smoothing(smoothing)
    world.set_objects(ranges)  # the smoothing hangs on objects
    assert world._smoothing == {} and world._skins == {} and world._morphs == {}
    spheres, _, _, _, _ = cases.build("three_spheres")
    with pytest.raises(ValueError):
        spheres.set_smoothing({0: None})  # an object without triangles
    assert not world._scenes and not spheres._scenes  # nothing above made a scene


def test_the_cases_are_what_the_tests_take_them_for():
    """Group counts, valences and negated triangles of every shape; welded as it is, the one-object knot's recomputed rest normals
    are its stored ones to within 1e-7 in cosine; and -- on the restatement, so that the reference alone stays off the flag --
    every squared length that is normalised lies inside [1e-30, 1e30] under every frame the other tests run."""
    valences, flipped = {}, {}
    for shape in smooth_cases.SHAPES:
        world, _, _, _, ranges, rest, smoothing = smooth_cases.build(shape)
        assert sorted(smoothing) == smooth_cases.smoothed_objects(shape, world)
        counts = []
        for index in sorted(smoothing):
            t0, n = ranges[index]["first_triangle"], ranges[index]["num_triangles"]
            _, order, begin = restatement.groups_of(smoothing[index])
            counts.append(len(begin) - 1)
            valences[shape, index] = sorted(set(np.diff(begin).tolist()))
            flipped[shape, index] = int(restatement.negated(rest["positions"][t0:t0 + n], rest["normals"][t0:t0 + n]).sum())
            assert sorted(order.tolist()) == list(range(3 * n))
        assert counts == smooth_cases.GROUPS[shape], shape
        for frame in frames_of(shape, world, rest, ranges):
            arrays = moved(rest, ranges, frame)
            out, flag, s = restatement.smoothed(arrays, rest, ranges, smoothing)
            assert flag == 0 and (s >= f32(1e-30)).all() and (s <= f32(1e30)).all() and s.min() > 1e-3, (shape, frame["name"])
            assert all(np.isfinite(out[k]).all() for k in KEYS if out[k] is not None), (shape, frame["name"])
    assert valences["knot_one", 0] == [6] and valences["cornell", 0] == [1, 2] and flipped["cornell", 0] == 8
    assert ranges[0]["num_triangles"] == 640  # knot_one: 320 lanes, two workgroups, the second a partial one
    out = restatement.smoothed(rest, rest, ranges, smoothing)[0]
    a, b = out["normals"][12:].reshape(-1, 3).astype(np.float64), rest["normals"][12:].reshape(-1, 3).astype(np.float64)
    cosine = (a * b).sum(axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))  # (an f32 unit vector's length is 1 only to 6e-8)
    assert cosine.min() > 1 - 1e-7
    assert np.array_equal(bits(out["normals"][:12]), bits(rest["normals"][:12]))  # the box is no smoothed object


# ---------------------------------------------------------------------------------------------------------------- (d) the rehearsal
def frames_of(shape, world, rest, ranges):
    """The frames every shape is held to: a morph without normal deltas under WEIGHTS; the two poses; in the knots the skin too,
    and everything in one call."""
    morphs = smooth_cases.morphs_for(shape, world, rest, ranges)
    skins = smooth_cases.skins_for(shape, rest, ranges)
    joints = {index: skin_cases.THREE for index in skins}
    weights = morph_cases.table(morphs, morph_cases.WEIGHTS)
    out = [dict(name="rest"), dict(name="morph", morphs=morphs, weights=weights)]
    for pose in ("non_uniform", "rotated_and_translated"):
        out.append(dict(name=pose, poses=cases.poses_for(pose, len(ranges))))
    if skins:
        out.append(dict(name="skin", skins=skins, joints=joints))
        out.append(dict(name="all", morphs=morphs, weights=weights, skins=skins, joints=joints, poses={len(ranges) - 1: cases.POSES["rotated_and_translated"]}))
    return out


def moved(rest, ranges, frame):
    arrays, _ = morph_restatement.morphed(rest, ranges, frame.get("morphs", {}), frame.get("weights", {}))
    return skin_restatement.skin_arrays(arrays, ranges, frame.get("skins", {}), frame.get("joints", {}), frame.get("poses", {}))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def smooth_check(tmp_path_factory):
    return deform_probe.build(tmp_path_factory.mktemp("deform_check"))


@pytest.fixture(scope="module")
def rehearsal_inputs():
    """name -> (world, rest, ranges, lamps, smoothing): the four shapes, and the textures example once more without its frames."""
    out = {}
    for shape in smooth_cases.SHAPES:
        world, _, _, _, ranges, rest, smoothing = smooth_cases.build(shape)
        out[shape] = (world, rest, ranges, cases.shape_lamps(world), smoothing)
    world, rest, ranges, lamps, smoothing = out["textures"]
    assert rest["frames"] is not None
    out["textures_without_frames"] = (world, dict(rest, frames=None), ranges, lamps, smoothing)
    return out


def rehearse(smooth_check, tmp_path, name, rest, ranges, lamps, smoothing, frame):
    return deform_probe.rehearse(smooth_check, tmp_path, name, rest, ranges, lamps, smoothing=smoothing, **{k: v for k, v in frame.items() if k != "name"})


def test_the_host_rehearsal_of_the_smoothing_kernel_under_sanitizers(smooth_check, rehearsal_inputs, tmp_path):
    """pose_rules.h on the CPU against the restatement, as bits: positions, normals and frames of every shape under every frame;
    an unsmoothed object's words are those of the frame without any smoothing; the lamp records are the smoothed arrays'."""
    for name, (world, rest, ranges, lamps, smoothing) in rehearsal_inputs.items():
        shape = name.replace("_without_frames", "")
        for frame in frames_of(shape, world, rest, ranges):
            what = (name, frame["name"])
            got = rehearse(smooth_check, tmp_path, name + "_" + frame["name"], rest, ranges, lamps, smoothing, frame)
            plain = moved(rest, ranges, frame)
            want, flag, _ = restatement.smoothed(plain, rest, ranges, smoothing)
            assert got["flag"] == flag == 0, what
            for key in KEYS:
                if rest[key] is not None:
                    assert np.array_equal(bits(got[key]), bits(want[key])), (what, key, int((bits(got[key]) != bits(want[key])).sum()))
            assert np.array_equal(bits(got["positions"]), bits(plain["positions"])), what  # the smoothing moves no vertex
            untouched = np.ones(len(rest["positions"]), dtype=bool)
            for index in smoothing:
                untouched[ranges[index]["first_triangle"]:ranges[index]["first_triangle"] + ranges[index]["num_triangles"]] = False
            assert np.array_equal(bits(got["normals"][untouched]), bits(plain["normals"][untouched])), what
            if frame["name"] != "rest":
                assert not np.array_equal(bits(got["normals"]), bits(plain["normals"])), what
            for k, (kind, at) in enumerate(lamps):
                if kind == 1:
                    assert np.array_equal(bits(got["lamps"][k][13:22]), bits(want["normals"][at])), (what, k)


def test_the_rehearsal_raises_bit_2_and_bit_0_still_wins(smooth_check, rehearsal_inputs, tmp_path):
    """4 for a pose of scale 0 (every position becomes the translation exactly, so every face vector is exactly 0); 4 for a target
    dp = -p at weight 1; and a position delta of 1e16 still raises bit 0, which comes first."""
    world, rest, ranges, lamps, smoothing = rehearsal_inputs["knot_one"]
    matrix, _ = cases.POSES["rotated_and_translated"]
    collapse = dict(name="scale0", poses={0: (matrix, 0.0)})
    got = rehearse(smooth_check, tmp_path, "scale0", rest, ranges, lamps, smoothing, collapse)
    assert got["flag"] == 4
    assert restatement.smoothed(moved(rest, ranges, collapse), rest, ranges, smoothing)[1] == 4
    assert (got["positions"][12:].reshape(-1, 3) == np.asarray(matrix, dtype=f32)[:3, 3]).all()
    t0, n = ranges[0]["first_triangle"], ranges[0]["num_triangles"]
    away = {0: dict(positions=(-rest["positions"][t0:t0 + n]).reshape(1, n, 3, 3).astype(f32), normals=None)}
    vanish = dict(name="vanish", morphs=away, weights={0: [1.0]})
    got = rehearse(smooth_check, tmp_path, "vanish", rest, ranges, lamps, smoothing, vanish)
    assert got["flag"] == 4 and not got["positions"][12:].any()
    assert restatement.smoothed(moved(rest, ranges, vanish), rest, ranges, smoothing)[1] == 4
    far = np.zeros((1, n, 3, 3), dtype=f32)
    far[0, 5, 1, 0] = 1e16
    got = rehearse(smooth_check, tmp_path, "far", rest, ranges, lamps, smoothing, dict(name="far", morphs={0: dict(positions=far, normals=None)}, weights={0: [1.0]}))
    assert got["flag"] & 1


# ---------------------------------------------------------------------------------------------------------------- (e) quality
def angles(a, b):
    """Degrees between unit-ish vectors, float64, by atan2 (small angles keep their digits)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(axis=1)))


@pytest.mark.parametrize("case", ["non_uniform", "shear"])
def test_recomputed_normals_are_nearer_the_truth_at_every_corner(case):
    """The one-object knot under an affine deformation A, on the restatement: the true normal is normalize(A^-T n_rest) in
    float64. At EVERY corner the recomputed normal's angle to it is smaller than the unsmoothed normal's -- normalize(M3 n) under the
    pose, rest's own normal under the morph without normal deltas."""
    world, _, _, _, ranges, rest, smoothing = smooth_cases.build("knot_one")
    t0, n = ranges[0]["first_triangle"], ranges[0]["num_triangles"]
    if case == "non_uniform":
        frame = dict(poses={0: cases.POSES["non_uniform"]})
        a = np.asarray(cases.POSES["non_uniform"][0], dtype=np.float64)[:3, :3]
    else:
        morphs = smooth_cases.morphs_for("knot_one", world, rest, ranges)
        frame = dict(morphs=morphs, weights={0: [0.0, 1.0, 0.0]})
        _, _, axis, second = morph_cases.axes_of(skin_cases.vertices_of(rest, ranges[0]))
        a = np.eye(3)
        a[second, axis] = np.float64(f32(0.2))
    plain = moved(rest, ranges, frame)
    got = restatement.smoothed(plain, rest, ranges, smoothing)[0]
    truth = rest["normals"][t0:t0 + n].reshape(-1, 3).astype(np.float64) @ np.linalg.inv(a)  # rows: (A^-T n)^T = n^T A^-1
    truth /= np.linalg.norm(truth, axis=1, keepdims=True)
    before = angles(plain["normals"][t0:t0 + n].reshape(-1, 3), truth)
    after = angles(got["normals"][t0:t0 + n].reshape(-1, 3), truth)
    print("%s: unsmoothed median %.3g max %.3g degrees; recomputed median %.3g max %.3g degrees; corners that violate: %d of %d"
          % (case, np.median(before), before.max(), np.median(after), after.max(), int((after >= before).sum()), len(after)))
    assert len(after) == 1920 and (after < before).all()
