"""Inputs of the level-wise BVH builders' tests (tests/test_bvh_device_cpu.py on the host rehearsal, tests/test_gpu_bvh_build.py
on the device builder): name -> (spheres [n,4], triangles [m,9]), float32. TIE_FREE: the recursive builder needs no median
fallback on them, so every builder must give its tree; FALLBACK: it does (coincident or collinear centroids); TOO_LARGE: it does at a node larger than the device builder ranks."""
import numpy as np

from pyrite_amd import scenes


def sliver_mesh():
    """tests/test_bvh_build.py's mesh: a coarse torus knot in a box of large walls, 4,612 triangles."""
    positions, _ = scenes.torus_knot_mesh(segments=96, sides=24, fit_min=(-8.0, -8.0, 1.0), fit_max=(8.0, 8.0, 9.0))
    tris = np.asarray(positions, dtype=np.float32).reshape(-1, 9)
    walls = np.array([[-10, -10, 0, 10, -10, 0, 10, 10, 0], [-10, -10, 0, 10, 10, 0, -10, 10, 0],
                      [-10, 10, 0, 10, 10, 0, 10, 10, 10], [-10, 10, 0, 10, 10, 10, -10, 10, 10]], dtype=np.float32)
    return np.concatenate([walls, tris])


def random_triangles(n, seed):
    rng = np.random.RandomState(seed)
    centre = rng.uniform(-8, 8, size=(n, 1, 3))
    return (centre + rng.uniform(-0.7, 0.7, size=(n, 3, 3))).astype(np.float32).reshape(n, 9)


def sphere_scene():
    """The spheres of scenes.c1_spheres: five walls of radius 100 around three small ones."""
    R = 100.0
    x0, x1, y1, z0, z1 = -5.56, 0.0, 5.592, 0.0, 5.488
    cx, cy, cz = (x0 + x1) / 2, y1 / 2, (z0 + z1) / 2
    return np.array([[x0 - R, cy, cz, R], [x1 + R, cy, cz, R], [cx, y1 + R, cz, R], [cx, cy, z0 - R, R], [cx, cy, z1 + R, R],
                     [-3.7, 3.3, 0.9, 0.9], [-1.6, 1.7, 0.8, 0.8], [-2.78, 2.795, 4.9, 0.5]], dtype=np.float32)


def random_spheres(n, seed):
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.uniform(-8, 8, size=(n, 3)), rng.uniform(0.1, 0.9, size=(n, 1))], axis=1).astype(np.float32)


NO_SPHERES = np.zeros((0, 4), dtype=np.float32)
NO_TRIANGLES = np.zeros((0, 9), dtype=np.float32)

TIE_FREE = {
    "sliver_mesh": lambda: (NO_SPHERES, sliver_mesh()),
    "spheres": lambda: (sphere_scene(), NO_TRIANGLES),
    "mixed": lambda: (random_spheres(37, 11), random_triangles(300, 12)),
    "tri1": lambda: (NO_SPHERES, random_triangles(1, 21)),
    "tri4": lambda: (NO_SPHERES, random_triangles(4, 22)),
    "tri5": lambda: (NO_SPHERES, random_triangles(5, 23)),
    "tri6": lambda: (NO_SPHERES, random_triangles(6, 24)),
    "tri65": lambda: (NO_SPHERES, random_triangles(65, 25)),
    "tri257": lambda: (NO_SPHERES, random_triangles(257, 26)),
}


def _line_triangles():
    """40 triangles whose centroids lie on one line: equal boxes shifted along x in steps that 16 bins cannot separate at the end."""
    t = np.zeros((40, 9), dtype=np.float32)
    base = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0], dtype=np.float32)
    for i in range(40):
        t[i] = base
        t[i, 0::3] += np.float32(0.25 * (i // 8))  # five clusters of eight coincident centroids
    return t


FALLBACK = {
    "nine_copies": lambda: (NO_SPHERES, np.repeat(random_triangles(1, 31), 9, axis=0)),
    "concentric_spheres": lambda: (np.array([[1.0, 2.0, 3.0, 0.5 + 0.25 * i] for i in range(12)], dtype=np.float32), NO_TRIANGLES),
    "line40": lambda: (NO_SPHERES, _line_triangles()),
    # more than a wave's worth of coincident centroids: on the device the median rule runs in its own kernel, one workgroup per
    # node (300 -> 150 -> 75 references), before the halves are small enough for one wave
    "coincident300": lambda: (NO_SPHERES, np.repeat(random_triangles(1, 32), 300, axis=0)),
}

# A median node beyond what one workgroup of the device builder ranks (2,048 references): the device builder steps aside and the
# host builds. The rehearsal on the CPU has no such limit.
TOO_LARGE = {
    "coincident3000": lambda: (NO_SPHERES, np.repeat(random_triangles(1, 33), 3000, axis=0)),
}


def rays_for(spheres, tris, n=1500, seed=5):
    """(origins, directions, limits): n closest-hit rays and n shadow rays between random points, inside the primitives' bounds."""
    pts = np.concatenate([tris.reshape(-1, 3), spheres[:, :3] - spheres[:, 3:], spheres[:, :3] + spheres[:, 3:]]).astype(np.float64)
    lo, hi = np.maximum(pts.min(axis=0), -12.0) - 0.5, np.minimum(pts.max(axis=0), 12.0) + 0.5
    rng = np.random.RandomState(seed)
    o = rng.uniform(lo, hi, size=(n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    a, b = rng.uniform(lo, hi, size=(n, 3)), rng.uniform(lo, hi, size=(n, 3))
    dist = np.linalg.norm(b - a, axis=1)
    return np.concatenate([o, a]), np.concatenate([d, (b - a) / dist[:, None]]), np.concatenate([np.full(n, -1.0), dist * dist - 1e-4])
