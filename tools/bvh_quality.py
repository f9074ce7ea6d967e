"""Tree quality of the C3 mesh's four-child pair tree, old against new, on the CPU (tools/bvh_quality.cpp).

Writes C3's triangles and the three ray sets of tests/test_gpu_parity.py's full-mesh check -- bench.py's `traversal_roofline`
rays, camera rays, floor-to-lamp shadow rays with their blocking distance -- builds the tool with the host compiler and prints
its table: references, nodes, build time, bytes, SAH cost, and per ray set the node visits, box tests and pair steps per ray.

    python tools/bvh_quality.py [--rays-scale 1.0] > profiles/r05_bvh_quality.txt
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BUILD_DIR = os.path.join(ROOT, "tools", "_build")
TOOL = os.path.join(BUILD_DIR, "bvh_quality")


def build_tool():
    os.makedirs(BUILD_DIR, exist_ok=True)
    src = [os.path.join(ROOT, "tools", "bvh_quality.cpp"), os.path.join(ROOT, "pyrite_amd", "csrc", "bvh.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", TOOL] + src)
    return TOOL


def write_triangles(path, tris):
    tris = np.ascontiguousarray(tris, dtype="<f4").reshape(-1, 9)
    with open(path, "wb") as f:
        f.write(np.uint32(len(tris)).tobytes())
        f.write(tris.tobytes())


def write_prims(path, spheres, tris):
    """PRIMS of the tool's `level` mode: spheres [n,4] (centre, radius) first, then triangles [m,9], as pyr_scene_create orders them."""
    spheres = np.asarray(spheres, dtype="<f4").reshape(-1, 4)
    tris = np.asarray(tris, dtype="<f4").reshape(-1, 9)
    rec = np.zeros((len(spheres) + len(tris), 10), dtype="<f4")
    rec[:len(spheres), 1:5] = spheres
    rec[len(spheres):, 0] = 1.0
    rec[len(spheres):, 1:] = tris
    with open(path, "wb") as f:
        f.write(np.uint32(len(rec)).tobytes())
        f.write(rec.tobytes())


def write_rays(path, origins, dirs, limits=None):
    n = len(origins)
    rec = np.zeros((n, 8), dtype="<f4")
    rec[:, 0:3], rec[:, 3:6] = origins, dirs
    rec[:, 6] = -1.0 if limits is None else limits
    with open(path, "wb") as f:
        f.write(np.uint32(n).tobytes())
        f.write(rec.tobytes())


def c3_triangles():
    from pyrite_amd import scenes

    flat = scenes.c3_flat()
    return np.concatenate([np.asarray(t, dtype=np.float32).reshape(-1, 9) for t in flat.tri_positions])


def c3_ray_sets(scale=1.0):
    """(name, origins, directions, squared blocking distance or None) as test_closest_hit_on_the_full_c3_mesh draws them."""
    from pyrite_amd import scenes
    from pyrite_amd.compiler import camera_from_project

    n_bench, n_cam, n_shadow = int(250000 * scale), int(150000 * scale), int(50000 * scale)
    rng = np.random.RandomState(1)  # c3_bench_rays
    o = rng.uniform([-55, 1, 1], [-1, 55, 54], size=(n_bench, 3))
    d = rng.normal(size=(n_bench, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sets = [("bench", o.astype(np.float32), d.astype(np.float32), None)]

    c = camera_from_project(scenes.cornell_camera(scale=10.0))  # camera_rays
    m = np.array(list(c.cam_to_world), dtype=np.float64).reshape(4, 4).T
    rng = np.random.RandomState(2)
    aspect = 1080.0 / 1920.0
    x, y = rng.uniform(-1, 1, n_cam), rng.uniform(-aspect, aspect, n_cam)
    target = np.stack([x / c.view_plane * c.focus_distance, -y / c.view_plane * c.focus_distance, np.full(n_cam, -c.focus_distance)], axis=1)
    d = target / np.linalg.norm(target, axis=1, keepdims=True)
    d = d @ m[:3, :3].T
    sets.append(("camera", np.broadcast_to(m[:3, 3], (n_cam, 3)).astype(np.float32), d.astype(np.float32), None))

    rng = np.random.RandomState(4)
    floor = rng.uniform([-55, 1, 0.01], [-1, 55, 0.01], size=(n_shadow, 3))
    lamp = rng.uniform([-34.3, 22.7, 54.79], [-21.3, 33.2, 54.79], size=(n_shadow, 3))
    to_lamp = lamp - floor
    dist = np.linalg.norm(to_lamp, axis=1)
    limit = (dist * dist - 1e-4).astype(np.float32)  # squared distance to the lamp minus DIST_EPSILON, as the kernels block
    sets.append(("shadow", floor.astype(np.float32), (to_lamp / dist[:, None]).astype(np.float32), limit))
    return sets


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rays-scale", type=float, default=1.0, help="fraction of the test's 450 k rays")
    args = ap.parse_args()
    tool = build_tool()
    with tempfile.TemporaryDirectory() as tmp:
        tri_path = os.path.join(tmp, "tris.bin")
        write_triangles(tri_path, c3_triangles())
        argv = [tool, "report", tri_path]
        for name, o, d, limit in c3_ray_sets(args.rays_scale):
            path = os.path.join(tmp, name + ".bin")
            write_rays(path, o, d, limit)
            argv.append("%s:%s" % (name, path))
        sys.stdout.write("C3 mesh (scenes.c3_flat), four-child pair tree: old and new builds and their walks\n")
        sys.stdout.flush()
        subprocess.check_call(argv)


if __name__ == "__main__":
    main()
