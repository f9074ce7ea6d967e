"""Shapes and poses of the pyr_scene_pose tests (tests/test_scene_pose_cpu.py on the host rehearsal, tests/test_gpu_scene_pose.py on
the kernels): small scenes of the project with the primitive ranges that move together, and four poses.

A shape is (project, ranges): `ranges` None takes the objects the description records (World.objects)."""
import numpy as np

from pyrite_amd import scenes

f32 = np.float32


def rotation4(axis, angle, translation=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    """A 4x4 matrix as on paper, float32: rotation about `axis` by `angle` times diag(scale), then the translation."""
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    r = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)
    m = np.eye(4)
    m[:3, :3] = r @ np.diag(scale)
    m[:3, 3] = translation
    return m.astype(f32)


# (matrix, scale); every matrix entry is zero or within [1e-3, 1e3] in magnitude, the range rcp32 is verified for with room to spare
POSES = {
    "identity": (None, 1.0),
    "rotated_and_translated": (rotation4((1, 2, 3), 0.3, translation=(0.5, -0.25, 0.75)), 1.0),
    "scaled_and_rotated": (rotation4((2, -1, 0.5), 0.5), 1.5),
    "non_uniform": (rotation4((0, 0, 1), 0.0, scale=(2.0, 1.0, 0.5)), 1.0),
}
ORDER = list(POSES)


def poses_for(name, num_objects):
    """Object 0, 2, ... get the pose `name`, the others the next one of the list (the identity case: all identity), so that
    neighbouring ranges of one launch carry different matrices."""
    if name == "identity":
        return {k: POSES["identity"] for k in range(num_objects)}
    other = ORDER[1 + (ORDER.index(name) % (len(ORDER) - 1))]
    return {k: POSES[name if k % 2 == 0 else other] for k in range(num_objects)}


def triangles(first, count):
    return dict(first_triangle=first, num_triangles=count, first_sphere=0, num_spheres=0)


def sphere(index):
    return dict(first_triangle=0, num_triangles=0, first_sphere=index, num_spheres=1)


KNOT_TRIANGLES = 2 * 16 * 20  # 640: with the twelve of the box, lanes 0..287 and 288..639 -- three workgroups, the object boundary inside the second

SHAPES = {
    # the Cornell box, 36 triangles of one mesh object, two of them the emissive light
    "cornell": (lambda: scenes.c2_cornell(64, 64, 16), None),
    # the textures example: two triangles with normal maps (so the scene keeps frames and tri_tex) and three spheres, one a lamp
    "textures": (lambda: scenes.textures_example(64, 48, 8), None),
    # the three small spheres of the sphere box, the last one emissive; the five wall spheres are in no range and never move
    "three_spheres": (lambda: scenes.c1_spheres(64, 64, 16), [sphere(5), sphere(6), sphere(7)]),
    # a knot of 640 triangles in the open box, split into two objects at triangle 300; the box stays
    "knot": (lambda: scenes.c3_mesh_in_box(64, 36, 8, segments=20, sides=16), [triangles(12, 288), triangles(300, 12 + KNOT_TRIANGLES - 300)]),
}


def build(shape, seed=5):
    """(world, camera, renderer, film, ranges) of a shape; nothing touches a GPU before a scene is asked for."""
    make, ranges = SHAPES[shape]
    world, cam, r, film = scenes.build(make(), seed=seed)
    if ranges is not None:
        world.set_objects(ranges)
    return world, cam, r, film, world.objects


def rest_of(world):
    """The description's arrays as float32 [n,9], [n,9], [n,12] | None, [m,4]."""
    f = world.flat
    cat = lambda rows, width: np.concatenate([np.asarray(r, dtype=f32).reshape(-1, width) for r in rows]) if len(rows) else np.zeros((0, width), dtype=f32)  # noqa: E731
    return {"positions": cat(f.tri_positions, 9), "normals": cat(f.tri_normals, 9), "frames": cat(f.tri_frames, 12) if f.uses_normal_maps and len(f.tri_material) else None,
            "spheres": cat(f.spheres, 4)}


def shape_lamps(world):
    """(shape_kind, shape_index) of every shape lamp, in lamp order."""
    from pyrite_amd import abi

    return [(l["shape_kind"], l["shape_index"]) for l in world.flat.lamps if l["kind"] == abi.LAMP_SHAPE]
