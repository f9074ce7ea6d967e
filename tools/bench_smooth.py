#!/usr/bin/env python3
"""Developer tool (GPU box): what recomputing a morphing mesh's normals on the GPU costs per frame, against the
same frame without it (section 9p) and against uploading arrays whose normals the host computed (section 9f).

    python tools/bench_smooth.py [repeats] > profiles/r30_smooth.txt

One process, one GPU. Two meshes: C3's (scenes.c3_flat) and the 160 x 160 torus knot in the same box. The knot carries 8 targets of
position deltas without normal deltas (target k pushes every vertex along its rest normal by a wave of k + 1 periods along the mesh's
longest axis), one of them active. One warm-up and `repeats` (default 7) rounds; in a round the active weight takes a value that
changes from round to round, in three ways on three live scenes, alternating:
  smooth     World.morph on a world with World.set_smoothing({knot: None}): the triangles morphed and their normals recomputed on
             the device (pyr_scene_morph, refit)
  morph      the same call on a world without a smoothing: the normals stay rest's
  update     World.update(mode="refit") from host arrays (pyr_scene_update): positions and the normals the host recomputed
The arrays of the last are computed by the numpy restatements (tests/morph_restatement.py, tests/smooth_restatement.py) before the
clock starts; what the host spends on that is printed and is on no bill. Reported per way: the median, smallest and largest of
PyrUpdateInfo's upload_ms, prims_ms, refit_ms and total_ms (smooth and morph enqueue: their prims_ms and refit_ms are the time to
enqueue; upload_ms holds the morph, pose and smoothing kernels and the read-back of the flag word), of the wall clock of the World
call with its kernels waited for, and the bytes that cross the bus per frame in each way."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import morph_restatement  # noqa: E402
import smooth_restatement  # noqa: E402

from pyrite_amd import scenes  # noqa: E402
from pyrite_amd.renderer import World, weld  # noqa: E402

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STAGES = ("upload_ms", "prims_ms", "refit_ms", "total_ms", "wall_ms")
MESHES = [("C3 mesh (scenes.c3_flat)", dict(segments=640, sides=640)), ("160 x 160 knot mesh", dict(segments=160, sides=160))]
BOX_TRIANGLES = 12  # the Cornell box without its two blocks comes first in scenes.c3_flat
TARGETS = 8
f32 = np.float32


def rest_of(world):
    cat = lambda rows: np.concatenate([np.asarray(r, dtype=np.float32).reshape(-1, 9) for r in rows])  # noqa: E731
    return {"positions": cat(world.flat.tri_positions), "normals": cat(world.flat.tri_normals), "frames": None, "spheres": np.zeros((0, 4), dtype=np.float32)}


def knot_targets(rest, o):
    """dict(positions [8,n,3,3], normals None): waves along the longest axis, pushed along the rest normals."""
    t0, n = o["first_triangle"], o["num_triangles"]
    p = rest["positions"][t0:t0 + n].reshape(-1, 3)
    normal = rest["normals"][t0:t0 + n].reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    axis = int(np.argmax(hi - lo))
    u = ((p[:, axis] - lo[axis]) / (hi[axis] - lo[axis])).astype(f32)
    positions = np.zeros((TARGETS, len(p), 3), dtype=f32)
    for k in range(TARGETS):
        positions[k] = normal * (f32(0.02) * (hi[axis] - lo[axis]) * np.sin(f32(np.pi * (k + 1)) * u))[:, None]
    return dict(positions=positions.reshape(TARGETS, n, 3, 3), normals=None)


def report(title, runs):
    print("  %s" % title)
    for stage in STAGES:
        t = sorted(r[stage] for r in runs)
        print("    %-10s median %9.3f ms  (min %9.3f max %9.3f, %d runs)" % (stage, statistics.median(t), t[0], t[-1], len(t)))


def timings(title, mesh):
    import torch

    live = {way: World(scenes.c3_flat(**mesh)) for way in ("smooth", "morph", "update")}
    rest = rest_of(live["smooth"])
    ranges = live["smooth"].objects
    knot = [k for k, o in enumerate(ranges) if o["first_triangle"] == BOX_TRIANGLES]
    assert len(knot) == 1 and ranges[knot[0]]["num_triangles"] == len(rest["positions"]) - BOX_TRIANGLES == 2 * mesh["segments"] * mesh["sides"]
    index = knot[0]
    t0, n = ranges[index]["first_triangle"], ranges[index]["num_triangles"]
    morphs = {index: knot_targets(rest, ranges[index])}
    ids = weld(rest["positions"][t0:t0 + n], rest["normals"][t0:t0 + n])
    groups = len(np.unique(ids))
    print("%s: %d triangles, %d groups over %d corners; the groups are %.1f MB on the device once (4 bytes a corner and 4 a group), the position deltas "
          "%.1f MB once; a frame of smooth or morph is %d bytes of arguments (8 weights and %d poses), a frame of update %.1f MB of positions and normals"
          % (title, len(rest["positions"]), groups, ids.size, (4 * ids.size + 4 * (groups + 1)) / 1e6, morphs[index]["positions"].nbytes / 1e6,
             4 * TARGETS + 80 * len(ranges), len(ranges), (rest["positions"].nbytes + rest["normals"].nbytes) / 1e6), flush=True)
    for world in live.values():
        world.scene(0, build="device")
    live["smooth"].set_morphs(morphs), live["morph"].set_morphs(morphs)
    live["smooth"].set_smoothing({index: ids})
    runs = {way: [] for way in live}
    host_ms = []
    for i in range(REPEATS + 1):
        w = np.zeros(TARGETS, dtype=f32)
        w[0] = f32(0.15 * (i + 1))
        weights = {index: w}
        t_host = time.perf_counter()
        plain = morph_restatement.morph_arrays(rest, ranges, morphs, weights)
        want = smooth_restatement.smoothed(plain, rest, ranges, {index: ids})[0]
        host_ms.append((time.perf_counter() - t_host) * 1e3)
        p, normals = want["positions"], want["normals"]
        row = {}
        for way, call in (("smooth", lambda: live["smooth"].morph(weights)), ("morph", lambda: live["morph"].morph(weights)),
                          ("update", lambda: live["update"].update(positions=p, normals=normals, mode="refit"))):
            torch.cuda.synchronize()
            t_call = time.perf_counter()
            call()
            torch.cuda.synchronize()
            row[way] = dict(live[way].update_info(), wall_ms=(time.perf_counter() - t_call) * 1e3)
        if i > 0:  # the first round is the warm-up
            for way in runs:
                runs[way].append(row[way])
    report("smooth     (World.morph with a smoothing, refit; upload_ms = the morph, pose and smoothing kernels and the read-back of the flag)", runs["smooth"])
    report("morph      (World.morph without a smoothing, refit)", runs["morph"])
    report("update     (World.update mode=refit, host arrays with host-computed normals)", runs["update"])
    print("    the host's restatement of the frame for the update path (numpy, on no bill): median %.3f ms" % statistics.median(host_ms[1:]))
    med = {way: statistics.median(r["total_ms"] for r in runs[way]) for way in runs}
    up = {way: statistics.median(r["upload_ms"] for r in runs[way]) for way in runs}
    print("    total_ms medians: smooth - morph = %.3f ms (upload_ms medians: %.3f ms), update / smooth = %.1f" % (med["smooth"] - med["morph"], up["smooth"] - up["morph"], med["update"] / med["smooth"]))
    got = live["smooth"].geometry()
    differ = sum(int((got[key].view(np.uint32) != want[key].view(np.uint32)).sum()) for key in ("positions", "normals"))
    print("    words of the smoothed positions and normals that differ from the restatement's: %d" % differ, flush=True)
    for world in live.values():
        world.close()


if __name__ == "__main__":
    for title, mesh in MESHES:
        timings(title, mesh)
