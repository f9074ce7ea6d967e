"""Inputs of the level-wise BVH builders' tests (tests/test_bvh_device_cpu.py on the host rehearsal, tests/test_gpu_bvh_build.py
on the device builder): name -> (spheres [n,4], triangles [m,9]), float32. TIE_FREE: the recursive builder needs no median
fallback on them, so every builder must give its tree; FALLBACK: it does (coincident or collinear centroids); TOO_LARGE: it does at a node larger than the device builder ranks;
DEPTH_RULE: trees so deep that the depth rule forces median splits over distinct centroids. tests/test_bvh_device_cpu.py proves, from
the rehearsal's own account, which path of the device builder each input reaches."""
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


def grid_z0():
    """A 40 x 30 grid of squares in the plane z = 0, two triangles each: every centroid extent on z is zero, at the root already."""
    i, j = np.meshgrid(np.arange(40), np.arange(30), indexing="ij")
    x0, y0 = (i.reshape(-1) * 0.5 - 10.0), (j.reshape(-1) * 0.5 - 7.5)
    z = np.zeros_like(x0)
    a, b, c, d = (np.stack(v, axis=1) for v in ((x0, y0, z), (x0 + 0.5, y0, z), (x0 + 0.5, y0 + 0.5, z), (x0, y0 + 0.5, z)))
    return np.concatenate([np.concatenate([a, b, c], axis=1), np.concatenate([a, c, d], axis=1)]).astype(np.float32)


TINY = 1.0e-42  # a float32 subnormal: 16 / (a few hundred of these) is infinite in float32


def tiny_triangles(n, seed, axes):
    """Random triangles flattened on `axes` to subnormal coordinates: triangle k lies within TINY of (a multiple of TINY below n * TINY)
    there, so the centroid extent on those axes is positive and so small that bin_scale is infinite. On the other axes: random_triangles."""
    rng = np.random.RandomState(seed)
    t = random_triangles(n, seed + 1000).reshape(n, 3, 3).astype(np.float64)
    for a in axes:
        t[:, :, a] = (rng.permutation(n)[:, None] + rng.randint(0, 2, size=(n, 3))) * TINY
    return t.astype(np.float32).reshape(n, 9)


def tiny_tiles(seed):
    """300 triangles in the slab 0 <= x <= 300 * TINY, one per cell of a 20 x 15 grid in y and z (no two overlap, so a ray hits
    one at most: the triangles of tiny_triangles(.., (0,)) would all but share a plane and tie wherever they overlap). Triangle
    k's x coordinates are subnormal multiples of TINY as in tiny_triangles; its centre is jittered inside its cell."""
    rng = np.random.RandomState(seed)
    cell = rng.permutation(300)
    centre = np.stack([np.zeros(300), cell // 15 - 9.5 + rng.uniform(-0.2, 0.2, size=300), cell % 15 - 7.0 + rng.uniform(-0.2, 0.2, size=300)], axis=1)
    t = centre[:, None, :] + rng.uniform(-0.25, 0.25, size=(300, 3, 3))
    t[:, :, 0] = (rng.permutation(300)[:, None] + rng.randint(0, 2, size=(300, 3))) * TINY
    return t.astype(np.float32).reshape(300, 9)


def signed_zeros(n, seed):
    """Random triangles rounded to halves (many coordinates are zero, many bounds coincide), every zero signed at random."""
    rng = np.random.RandomState(seed)
    t = np.round(random_triangles(n, seed + 1000).astype(np.float64) * 2.0) / 2.0
    t = np.where(t == 0.0, np.where(rng.randint(0, 2, size=t.shape) == 1, -0.0, 0.0), t)
    return t.astype(np.float32)


def near_limit(n, seed):
    """Triangles of a size of 1e11 around centres up to 8e13, under the 1e15 a scene may hold. (Triangles of 1e13 would be there
    too, but no float32 intersection routine hits them: edge x edge x distance overflows.)"""
    rng = np.random.RandomState(seed)
    centre = rng.uniform(-8.0e13, 8.0e13, size=(n, 1, 3))
    return (centre + rng.uniform(-0.7e11, 0.7e11, size=(n, 3, 3))).astype(np.float32).reshape(n, 9)


TIE_FREE.update({
    # a root of kSmallNode - 1 .. + 2 references, and of 1, 1, 2, 2 and 3 chunks of kChunk
    "tri64": lambda: (NO_SPHERES, random_triangles(64, 41)),
    "tri66": lambda: (NO_SPHERES, random_triangles(66, 42)),
    "tri2047": lambda: (NO_SPHERES, random_triangles(2047, 43)),
    "tri2048": lambda: (NO_SPHERES, random_triangles(2048, 44)),
    "tri2049": lambda: (NO_SPHERES, random_triangles(2049, 45)),
    "tri4096": lambda: (NO_SPHERES, random_triangles(4096, 46)),
    "tri4097": lambda: (NO_SPHERES, random_triangles(4097, 47)),
    # more than 64 large nodes in one level: choose_large_kernel past its first workgroup
    "tri40000": lambda: (NO_SPHERES, random_triangles(40000, 48)),
    "grid_z0": lambda: (NO_SPHERES, grid_z0()),
    "tiny_x": lambda: (NO_SPHERES, tiny_tiles(49)),
    "tiny_xy": lambda: (NO_SPHERES, tiny_triangles(3000, 50, (0, 1))),
    "signed_zeros": lambda: (NO_SPHERES, signed_zeros(500, 51)),
    "near_limit": lambda: (NO_SPHERES, near_limit(500, 52)),
    "mixed2600": lambda: (random_spheres(500, 53), random_triangles(2100, 54)),
})


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


def spheres_on_triangles():
    """100 copies of one triangle and 100 concentric spheres on the centre of its box: one median node of 200 coincident centroids,
    ranked by shape codes of two kinds. (Every coordinate is a small dyadic number, so both kinds' centroids are exactly (1, 1, 0).)"""
    tri = np.array([[0, 0, 0, 2, 0, 0, 0, 2, 0]], dtype=np.float32)
    spheres = np.array([[1.0, 1.0, 0.0, 0.25 + 0.125 * i] for i in range(100)], dtype=np.float32)
    return spheres, np.repeat(tri, 100, axis=0)


FALLBACK.update({
    # subnormal centroid extents on every axis: every reference falls into bin 0, so the median rule ranks DISTINCT centroids
    "tiny_xyz": lambda: (NO_SPHERES, tiny_triangles(300, 55, (0, 1, 2))),
    "spheres_on_triangles": spheres_on_triangles,
    # 1,000 distinct triangles, each five times: SAH splits all the way down, and every cluster ends in a median over equal
    # centroids in one wave (two copies, or four, would be a leaf: kLeafMax is 4)
    "fives1000": lambda: (NO_SPHERES, np.repeat(random_triangles(1000, 56), 5, axis=0)),
})

# A median node beyond what one workgroup of the device builder ranks (2,048 references): the device builder steps aside and the
# host builds. The rehearsal on the CPU has no such limit.
TOO_LARGE = {
    "coincident3000": lambda: (NO_SPHERES, np.repeat(random_triangles(1, 33), 3000, axis=0)),
}


def chain(steps, ratio, cluster, seed):
    """A geometric chain: `steps` triangles of size s around (s, s/2, s/4), s from 2^40 down by `ratio` (all far below the 1e15 a
    scene may hold), vertices within 5 % of s of the centre; then `cluster` triangles of the last size around the small end. The SAH
    peels the chain off a few triangles per level, so the depth rule (kDepthMax 40) meets a node that still holds the cluster."""
    rng = np.random.RandomState(seed)
    s = 2.0 ** 40 / float(ratio) ** np.arange(steps)
    centre = np.stack([s, s / 2, s / 4], axis=1)
    tris = [centre[:, None, :] + 0.05 * s[:, None, None] * rng.uniform(-1, 1, size=(steps, 3, 3))]
    tris.append(centre[-1] + s[-1] * (rng.uniform(-1, 1, size=(cluster, 1, 3)) + 0.05 * rng.uniform(-1, 1, size=(cluster, 3, 3))))
    return np.concatenate(tris).astype(np.float32).reshape(-1, 9)


# The depth rule's medians. chain300 / chain300_r4: at a node of more than a wave's worth and at most 2,048 references (the device
# builder's median kernel, over distinct centroids). chain3000: at a node of more than 2,048, which ends the device build, and its
# four-wide tree needs a deeper stack than the kernels have, so the scene keeps the binary tree.
DEPTH_RULE = {
    "chain300": lambda: (NO_SPHERES, chain(140, 2, 300, 61)),
    "chain300_r4": lambda: (NO_SPHERES, chain(70, 4, 300, 62)),
    "chain3000": lambda: (NO_SPHERES, chain(140, 2, 3000, 63)),
}

# the inputs at the device builder's edges (every entry above that the first thirteen GPU inputs and coincident3000 are not)
EDGES = ("tri64", "tri66", "tri2047", "tri2048", "tri2049", "tri4096", "tri4097", "tri40000", "grid_z0", "tiny_x", "tiny_xy", "signed_zeros", "near_limit",
         "mixed2600", "tiny_xyz", "spheres_on_triangles", "fives1000") + tuple(sorted(DEPTH_RULE))

# inputs no ray can hit (subnormal triangles, or slivers of subnormal width): the tests that ask for a floor of hits leave them out
UNHITTABLE = ("tiny_xy", "tiny_xyz")


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


def rays_into(spheres, tris, n, seed=9):
    """[n, 6] float32: the closest-hit rays of rays_for."""
    o, d, _ = rays_for(spheres, tris, n=n, seed=seed)
    return np.concatenate([o[:n], d[:n]], axis=1).astype(np.float32)


def aimed_rays(spheres, tris, n, seed=3):
    """rays_for's set and as many rays aimed at primitives from points around them, so that small inputs are hit often too."""
    centres = np.concatenate([tris.reshape(-1, 3, 3).mean(axis=1), spheres[:, :3]]).astype(np.float64)
    rng = np.random.RandomState(seed)
    target = centres[rng.randint(len(centres), size=n // 2)]
    origin = target + rng.normal(size=target.shape) * 6.0
    d = target - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([rays_into(spheres, tris, n - n // 2), np.concatenate([origin, d], axis=1).astype(np.float32)])


def aimed_rays_at_scale(spheres, tris, n, seed=3, through=0):
    """For inputs rays_for's +-12 box barely hits (coordinates of 1e13, sizes from 1e-30 to 1e12): every ray is aimed at a point of
    a primitive of a size a ray can hit (at least 0.01), from three to six of that primitive's sizes away. `through`: as many
    rays more from 1e2 .. 1e3 away that pass the smallest primitive at a distance of 10 -- inside every padded box of a chain (the
    padding, 16 ulps of its top, is 2e6), clear of the links too small for a float32 ray from that far to hit or miss reliably."""
    t = tris.reshape(-1, 3, 3).astype(np.float64)
    centres = np.concatenate([t.mean(axis=1), spheres[:, :3].astype(np.float64)])
    sizes = np.concatenate([np.linalg.norm(t.max(axis=1) - t.min(axis=1), axis=1), 2.0 * spheres[:, 3].astype(np.float64)])
    rng = np.random.RandomState(seed)
    big = np.nonzero(sizes >= 0.01)[0]
    pick = big[rng.randint(len(big), size=n)]
    away = rng.normal(size=(n, 3))
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    target = centres[pick] + 0.1 * sizes[pick, None] * rng.uniform(-1, 1, size=(n, 3))
    origin = centres[pick] + away * (sizes[pick] * rng.uniform(3, 6, size=n))[:, None]
    if through:
        away = rng.normal(size=(through, 3))
        away /= np.linalg.norm(away, axis=1, keepdims=True)
        beside = rng.normal(size=(through, 3))
        beside = centres[np.argmin(sizes)] + 10.0 * beside / np.linalg.norm(beside, axis=1, keepdims=True)
        origin = np.concatenate([origin, beside + away * (10.0 ** rng.uniform(2, 3, size=through))[:, None]])
        target = np.concatenate([target, beside])
    d = target - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([origin, d], axis=1).astype(np.float32)


AT_SCALE = ("near_limit",) + tuple(sorted(DEPTH_RULE))


def rays_of(name, spheres, tris, n=20000):
    """The [n, 6] closest-hit rays the tests send into input `name`."""
    if name in DEPTH_RULE:
        return aimed_rays_at_scale(spheres, tris, n, through=n // 10)
    return aimed_rays_at_scale(spheres, tris, n) if name in AT_SCALE else aimed_rays(spheres, tris, n)


def group_of(name):
    return next(g for g in (TIE_FREE, FALLBACK, TOO_LARGE, DEPTH_RULE) if name in g)
