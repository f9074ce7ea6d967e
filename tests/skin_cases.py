"""Shapes, bindings and joint tables of the pyr_scene_skin tests (tests/test_scene_skin_cpu.py on the host rehearsal,
tests/test_gpu_scene_skin.py on the kernels): the shapes of tests/pose_cases.py, each with the one object that is skinned.

In `knot` object 0 (288 triangles) is skinned and object 1 (352) is rigid: 640 lanes with the box's twelve triangles left alone,
so one call carries a skinned object and a posed object side by side, and the skin's 288 lanes fill more than one workgroup."""
import numpy as np

import pose_cases as cases

f32 = np.float32

SHAPES = ("cornell", "textures", "knot")
BINDINGS = ("bend", "one_hot")
# three joints: the matrices (not the scales) of three poses of tests/pose_cases.py
THREE = np.stack([cases.POSES[name][0] for name in ("rotated_and_translated", "scaled_and_rotated", "non_uniform")]).astype(f32)


def skinned_object(world):
    """The index of the first object that has triangles."""
    return next(k for k, o in enumerate(world.objects) if o["num_triangles"])


def vertices_of(rest, o):
    return rest["positions"][o["first_triangle"]:o["first_triangle"] + o["num_triangles"]].reshape(-1, 3).astype(f32)


def bend(rest, o):
    """u: the vertex's coordinate along the object's longest axis, scaled to [0,1]. Joints (0,1,2,0); w0 = clip(1-2u, 0, 1),
    w2 = clip(2u-1, 0, 1), w1 = 1 - w0 - w2, w3 = 0, all in f32."""
    p = vertices_of(rest, o)
    lo, hi = p.min(axis=0), p.max(axis=0)
    axis = int(np.argmax(hi - lo))
    u = ((p[:, axis] - lo[axis]) / (hi[axis] - lo[axis])).astype(f32)
    w0 = np.clip(f32(1.0) - f32(2.0) * u, f32(0.0), f32(1.0)).astype(f32)
    w2 = np.clip(f32(2.0) * u - f32(1.0), f32(0.0), f32(1.0)).astype(f32)
    w1 = (f32(1.0) - w0 - w2).astype(f32)
    weights = np.stack([w0, w1, w2, np.zeros_like(u)], axis=1).astype(f32)
    joints = np.tile(np.array([0, 1, 2, 0], dtype=np.uint16), (len(p), 1))
    return dict(joints=joints.reshape(-1, 3, 4), weights=weights.reshape(-1, 3, 4), num_joints=3)


def one_hot(rest, o):
    """Every vertex on joint 0 alone: B equals J[0] exactly, so the skin is the rigid pose by J[0]."""
    n = 3 * o["num_triangles"]
    weights = np.tile(np.array([1, 0, 0, 0], dtype=f32), (n, 1))
    return dict(joints=np.zeros((n, 4), dtype=np.uint16).reshape(-1, 3, 4), weights=weights.reshape(-1, 3, 4), num_joints=3)


def binding(name, rest, o):
    return {"bend": bend, "one_hot": one_hot}[name](rest, o)


def build(shape, name="bend", seed=5):
    """(world, camera, renderer, film, ranges, rest, skins) of a shape with its one skin set; nothing touches a GPU before a scene
    is asked for."""
    world, cam, r, film, ranges = cases.build(shape, seed=seed)
    rest = cases.rest_of(world)
    index = skinned_object(world)
    skins = {index: binding(name, rest, ranges[index])}
    world.set_skins(skins)
    return world, cam, r, film, ranges, rest, skins


def object_poses(name, num_objects):
    """The poses on top of the skin: every object at the identity, or every object moved (tests/pose_cases.py poses_for)."""
    return {} if name == "identity" else cases.poses_for(name, num_objects)
