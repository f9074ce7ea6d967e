"""pyr_scene_pose without a GPU: the three new structs of the ABI, the argument checks that need no scene,
the objects the description records, and the host rehearsal of the pose kernels -- pose_rules.h, the header kernels/pose.hip
compiles, through tests/probes/deform_check.cpp, a program of its own built with -fsanitize=address,undefined and run as a child
process -- compared as bits with the numpy restatement (tests/pose_restatement.py)."""
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
import pose_restatement as restatement  # noqa: E402

from pyrite_amd import abi  # noqa: E402
from pyrite_amd import build as gpu_build  # noqa: E402

HEADER = os.path.join(ROOT, "include", "pyrite_gpu.h")
STRUCTS = ["PyrObjectRange", "PyrObjectPose", "PyrPoseUpdate"]


def test_header_and_ctypes_agree_on_the_pose_structs():
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
    assert C.sizeof(abi.PyrObjectPose) == 80 and C.sizeof(abi.PyrObjectRange) == 16  # "80 bytes per object"
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+PYR_ABI_VERSION\s+5\b", text) and abi.PYR_ABI_VERSION == 5
    for name in ("pyr_scene_set_objects", "pyr_scene_pose", "pyr_scene_geometry"):
        assert name in abi.ENTRY_POINTS and re.search(r"\bint\s+%s\s*\(" % name, text)


@pytest.fixture(scope="module")
def lib():
    return abi.bind(C.CDLL(gpu_build.build()))


def test_bad_arguments_are_refused_before_any_device_is_looked_for(lib):
    """No GPU here: anything that reached the device would be PYR_ERR_DEVICE. pyr_last_error names the argument. Every other
    refusal of these calls needs a scene (tests/test_gpu_scene_pose.py)."""
    good = abi.PyrPoseUpdate(mode=abi.PYR_UPDATE_REFIT)
    assert lib.pyr_scene_pose(None, None, None) == abi.PYR_ERR_INVALID_ARGUMENT and b"null update" in lib.pyr_last_error()
    assert lib.pyr_scene_pose(None, C.byref(good), None) == abi.PYR_ERR_INVALID_ARGUMENT and b"null scene" in lib.pyr_last_error()
    ranges = (abi.PyrObjectRange * 1)(abi.PyrObjectRange(0, 1, 0, 0))
    assert lib.pyr_scene_set_objects(None, ranges, 1) == abi.PYR_ERR_INVALID_ARGUMENT and b"null scene" in lib.pyr_last_error()
    assert lib.pyr_scene_set_objects(None, None, 0) == abi.PYR_ERR_INVALID_ARGUMENT and b"null scene" in lib.pyr_last_error()
    assert lib.pyr_scene_set_objects(None, None, 3) == abi.PYR_ERR_INVALID_ARGUMENT and b"ranges" in lib.pyr_last_error()
    assert lib.pyr_scene_geometry(None, None, None, None, None) == abi.PYR_ERR_INVALID_ARGUMENT and b"null scene" in lib.pyr_last_error()


def test_the_description_records_what_moves_together():
    """One object per project object that has geometry and per add_triangles call; lamps without geometry have none."""
    from pyrite_amd.renderer import World

    world, _, _, _, objects = cases.build("cornell")
    assert objects == [dict(name="objects[0]", first_triangle=0, num_triangles=36, first_sphere=0, num_spheres=0)]
    world, _, _, _, objects = cases.build("textures")
    assert [(o["num_triangles"], o["num_spheres"]) for o in objects] == [(0, 1), (0, 1), (2, 0), (0, 1)]  # the point light (objects[0]) has none
    assert [o["name"] for o in objects] == ["objects[1]", "objects[2]", "objects[3]", "objects[4]"]
    world, _, _, _, _ = cases.build("knot")
    assert [(o["name"], o["first_triangle"], o["num_triangles"]) for o in world.flat.objects] == [("objects[0]", 0, 12), ("triangles[12]", 12, 640)]
    assert [(o["first_triangle"], o["num_triangles"]) for o in world.objects] == [(12, 288), (300, 352)]  # set_objects named other ranges
    assert callable(World.pose) and callable(World.geometry) and callable(World.set_objects)
    with pytest.raises(ValueError):
        world.pose({2: (None, 1.0)})  # no such object: refused before any scene is made
    for name, (matrix, scale) in cases.POSES.items():
        if matrix is not None:
            entries = np.abs(matrix[matrix != 0])
            assert entries.min() >= 1e-3 and entries.max() <= 1e3, name
            assert np.array_equal(matrix[3], np.float32([0, 0, 0, 1]))


def test_the_cpp_front_end_records_the_same_objects(tmp_path):
    """pyrite::World::objects() of every scene of pyrite_host_tool against World.objects of the same scene written in Python."""
    from test_host_cpp import SCENES, data_dir_for
    from pyrite_amd import scenes
    from pyrite_amd.compiler import DATA_DIR, FlatScene

    gpu_build.build_host()
    for name in sorted(SCENES):
        flat = FlatScene().add_world(SCENES[name]()["world"], DATA_DIR)
        want = ["%s %d %d %d %d" % (o["name"], o["first_triangle"], o["num_triangles"], o["first_sphere"], o["num_spheres"]) for o in flat.objects]
        got = subprocess.check_output([gpu_build.HOST_TOOL, "objects", name, data_dir_for(name, tmp_path)], text=True).splitlines()
        assert got == want and (want or name == "lamps"), name
    assert scenes  # (SCENES' makers)


# ---------------------------------------------------------------------------------------------------------------- the rehearsal
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pose_check(tmp_path_factory):
    return deform_probe.build(tmp_path_factory.mktemp("deform_check"))


def rehearsal_inputs():
    """name -> (rest, ranges, lamps): the Cornell box, the textures example with its frames, three spheres of which one is a lamp,
    and the smallest tie-free mesh of tests/bvh_build_inputs.py (one triangle; flat normals, no lamp)."""
    out = {}
    for shape in ("cornell", "textures", "three_spheres"):
        world, _, _, _, ranges = cases.build(shape)
        out[shape] = (cases.rest_of(world), ranges, cases.shape_lamps(world))
    smallest = min(inputs.TIE_FREE, key=lambda name: len(inputs.TIE_FREE[name]()[1]) if len(inputs.TIE_FREE[name]()[1]) else 1 << 30)
    _, tris = inputs.TIE_FREE[smallest]()
    t = tris.reshape(-1, 3, 3)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    rest = {"positions": tris.astype(np.float32), "normals": np.repeat(n[:, None, :], 3, axis=1).reshape(-1, 9), "frames": None, "spheres": np.zeros((0, 4), dtype=np.float32)}
    out[smallest] = (rest, [cases.triangles(0, len(tris))], [(1, 0)])  # (its one triangle taken as a lamp, for the area)
    return out


@pytest.mark.parametrize("pose", cases.ORDER)
def test_the_host_rehearsal_of_the_pose_kernels_under_sanitizers(pose_check, tmp_path, pose):
    """pose_rules.h on the CPU against the restatement, as bits: positions, normals, frames and spheres of every input; the lamp
    records' vertices, normals, centres and radii are the posed arrays' and their areas pack_lamp's formula restated in numpy."""
    for name, (rest, ranges, lamps) in rehearsal_inputs().items():
        poses = cases.poses_for(pose, len(ranges))
        got = deform_probe.rehearse(pose_check, tmp_path, name, rest, ranges, lamps, poses=poses)
        want = restatement.pose_arrays(rest, ranges, poses)
        for key in ("positions", "normals", "frames", "spheres"):
            if rest[key] is None:
                continue
            assert np.array_equal(bits(got[key]), bits(want[key])), (name, pose, key, int((bits(got[key]) != bits(want[key])).sum()))
            assert np.isfinite(got[key]).all()
        if pose == "identity":
            assert all(np.array_equal(bits(got[key]), bits(rest[key])) for key in ("positions", "normals", "frames", "spheres") if rest[key] is not None)
        else:
            moved = [key for key in ("positions", "spheres") if rest[key] is not None and rest[key].size and not np.array_equal(bits(got[key]), bits(rest[key]))]
            assert moved, (name, pose)
        assert got["flag"] == 0
        areas = restatement.lamp_areas(want, lamps)
        for k, (kind, index) in enumerate(lamps):
            record = got["lamps"][k]
            assert bits(record[22:23])[0] == bits(areas[k:k + 1])[0], (name, pose, k)
            if kind == 0:
                assert np.array_equal(bits(record[0:4]), bits(want["spheres"][index]))
            else:
                assert np.array_equal(bits(record[4:13]), bits(want["positions"][index])) and np.array_equal(bits(record[13:22]), bits(want["normals"][index]))


def test_the_rehearsal_raises_the_flag_beyond_the_coordinate_range(pose_check, tmp_path):
    rest, ranges, lamps = rehearsal_inputs()["three_spheres"]
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 1e16
    assert deform_probe.rehearse(pose_check, tmp_path, "far", rest, ranges, lamps, poses={1: (far, 1.0)})["flag"] == 1
