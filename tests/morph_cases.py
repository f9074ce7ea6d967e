"""Shapes, targets and weight tables of the pyr_scene_morph tests (tests/test_scene_morph_cpu.py on the host rehearsal,
tests/test_gpu_scene_morph.py on the kernel): the shapes of tests/pose_cases.py, each morphed object with three targets --
`bulge`, `shear`, `poison` -- and weight tables whose last entry is exactly 0, so `poison` (every delta 1e30) is never read.

In `knot` object 0 (288 triangles: more than one workgroup, the second a partial one) carries a morph and the skin of
tests/skin_cases.py, and object 1 (352) a morph and only a pose: one call runs morph+skin and morph+pose side by side, with the
box's twelve triangles left alone."""
import numpy as np

import pose_cases as cases
import skin_cases

f32 = np.float32

SHAPES = ("cornell", "textures", "knot")
TARGETS = ("bulge", "shear", "poison")
WEIGHTS = np.array([0.75, -0.5, 0.0], dtype=f32)  # a blend with an extrapolating (negative) weight; poison inactive
OTHER = np.array([0.25, 1.25, 0.0], dtype=f32)    # another frame, one weight above 1
BULGE = np.array([1.0, 0.0, 0.0], dtype=f32)      # the bulge alone
ZERO = np.zeros(3, dtype=f32)


def morphed_objects(shape, world):
    """The indices of the objects that carry a morph."""
    return [0, 1] if shape == "knot" else [skin_cases.skinned_object(world)]


def axes_of(p):
    lo, hi = p.min(axis=0), p.max(axis=0)
    order = np.argsort(hi - lo)
    return lo, hi, int(order[2]), int(order[1])  # the longest axis and the next


def bulge(rest, o):
    """u: the vertex's coordinate along the object's longest axis, scaled to [0,1]. dp = n * (0.05 * extent) * sin(pi u), and the
    normal tilts against the slope: dn = -0.3 cos(pi u) along that axis. All in f32."""
    p = skin_cases.vertices_of(rest, o)
    n = rest["normals"][o["first_triangle"]:o["first_triangle"] + o["num_triangles"]].reshape(-1, 3).astype(f32)
    lo, hi, axis, _ = axes_of(p)
    extent = f32(hi[axis] - lo[axis])
    u = ((p[:, axis] - lo[axis]) / extent).astype(f32)
    height = (f32(0.05) * extent * np.sin(f32(np.pi) * u)).astype(f32)
    dp = (n * height[:, None]).astype(f32)
    dn = np.zeros_like(n)
    dn[:, axis] = (f32(-0.3) * np.cos(f32(np.pi) * u)).astype(f32)
    return dp, dn


def shear(rest, o):
    """Positions slide along the second axis by 0.2 of their height on the longest; normals take the inverse transpose's part:
    dn = -0.2 * n[second] along the longest axis."""
    p = skin_cases.vertices_of(rest, o)
    n = rest["normals"][o["first_triangle"]:o["first_triangle"] + o["num_triangles"]].reshape(-1, 3).astype(f32)
    lo, _, axis, second = axes_of(p)
    dp, dn = np.zeros_like(p), np.zeros_like(n)
    dp[:, second] = (f32(0.2) * (p[:, axis] - lo[axis])).astype(f32)
    dn[:, axis] = (f32(-0.2) * n[:, second]).astype(f32)
    return dp, dn


def poison(rest, o):
    d = np.full((3 * o["num_triangles"], 3), 1e30, dtype=f32)
    return d, d.copy()


def targets(rest, o, with_normals=True):
    """dict(positions [3,n,3,3], normals [3,n,3,3] | None) of the three targets."""
    made = [{"bulge": bulge, "shear": shear, "poison": poison}[name](rest, o) for name in TARGETS]
    shape = (len(TARGETS), o["num_triangles"], 3, 3)
    positions = np.stack([dp for dp, _ in made]).reshape(shape).astype(f32)
    normals = np.stack([dn for _, dn in made]).reshape(shape).astype(f32) if with_normals else None
    return dict(positions=np.ascontiguousarray(positions), normals=None if normals is None else np.ascontiguousarray(normals))


def morphs_for(shape, world, rest, ranges, with_normals=True):
    return {index: targets(rest, ranges[index], with_normals) for index in morphed_objects(shape, world)}


def build(shape, with_normals=True, seed=5):
    """(world, camera, renderer, film, ranges, rest, morphs, skins) of a shape with its morphs set (and, in the knot, the skin of
    object 0); nothing touches a GPU before a scene is asked for."""
    world, cam, r, film, ranges = cases.build(shape, seed=seed)
    rest = cases.rest_of(world)
    morphs = morphs_for(shape, world, rest, ranges, with_normals)
    skins = {0: skin_cases.bend(rest, ranges[0])} if shape == "knot" else {}
    if skins:
        world.set_skins(skins)
    world.set_morphs(morphs)
    return world, cam, r, film, ranges, rest, morphs, skins


def table(morphs, w):
    """The weight table `w` for every morph."""
    return {index: np.array(w, dtype=f32) for index in morphs}


def frame_for(shape, morphs, skins, ranges, w=WEIGHTS):
    """(weights, joints, poses) of the frame the tests run: every morph under `w`; in the knot the skin under skin_cases.THREE
    and object 1 under a pose, object 0 at the identity."""
    weights = table(morphs, w)
    joints = {index: skin_cases.THREE for index in skins}
    poses = {1: cases.POSES["rotated_and_translated"]} if shape == "knot" else {}
    return weights, joints, poses
