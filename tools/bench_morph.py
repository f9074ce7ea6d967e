#!/usr/bin/env python3
"""Developer tool (GPU box): what a frame of a morphing mesh costs when its targets are blended on the GPU,
against uploading whole new arrays (section 9f).

    python tools/bench_morph.py [repeats] > profiles/r29_morph.txt

One process, one GPU. Two meshes: C3's (scenes.c3_flat) and the 160 x 160 torus knot in the same box. The knot carries 8 targets with
position and normal deltas: target k pushes every vertex along its normal by a wave of k + 1 periods along the mesh's longest axis and
tilts the normal against the wave's slope. Per mesh and per number of active targets (1, 2 and 8 of the 8; the others at weight 0)
one warm-up and `repeats` (default 7) rounds; in a round the active weights take values that change from round to round, in three
ways on three live scenes, alternating:
  morph      World.morph: 8 weights, the triangles computed on the device (pyr_scene_morph, refit)
  update     World.update(mode="refit") from host arrays (pyr_scene_update) of the same deformed geometry
  update-dev World.update(mode="refit") from torch tensors on the device (pyr_scene_update_device), uploaded beforehand
The arrays of the last two are computed by the numpy restatement of the morph rule (tests/morph_restatement.py) before the clock
starts; what the host spends on that is printed and is on no bill. Reported per way: the median, smallest and largest of
PyrUpdateInfo's upload_ms, prims_ms, refit_ms and total_ms (morph and update-dev enqueue: their prims_ms and refit_ms are the time to
enqueue), of the wall clock of the World call with its kernels waited for, and of area_ratio after the call; for morph, the share of
total_ms that is upload_ms -- the morph, pose and skin kernels and the read-back of the flag word."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import morph_restatement as restatement  # noqa: E402

from pyrite_amd import scenes  # noqa: E402
from pyrite_amd.renderer import World  # noqa: E402

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STAGES = ("upload_ms", "prims_ms", "refit_ms", "total_ms", "wall_ms", "area_ratio")
MESHES = [("C3 mesh (scenes.c3_flat)", dict(segments=640, sides=640)), ("160 x 160 knot mesh", dict(segments=160, sides=160))]
BOX_TRIANGLES = 12  # the Cornell box without its two blocks comes first in scenes.c3_flat
TARGETS = 8
ACTIVE = (1, 2, 8)
f32 = np.float32


def rest_of(world):
    cat = lambda rows: np.concatenate([np.asarray(r, dtype=np.float32).reshape(-1, 9) for r in rows])  # noqa: E731
    return {"positions": cat(world.flat.tri_positions), "normals": cat(world.flat.tri_normals), "frames": None, "spheres": np.zeros((0, 4), dtype=np.float32)}


def knot_targets(rest, o):
    """dict(positions [8,n,3,3], normals [8,n,3,3]): waves along the longest axis, pushed along the normals."""
    t0, n = o["first_triangle"], o["num_triangles"]
    p = rest["positions"][t0:t0 + n].reshape(-1, 3)
    normal = rest["normals"][t0:t0 + n].reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    axis = int(np.argmax(hi - lo))
    u = ((p[:, axis] - lo[axis]) / (hi[axis] - lo[axis])).astype(f32)
    positions, normals = np.zeros((TARGETS, len(p), 3), dtype=f32), np.zeros((TARGETS, len(p), 3), dtype=f32)
    for k in range(TARGETS):
        phase = f32(np.pi * (k + 1)) * u
        positions[k] = normal * (f32(0.02) * (hi[axis] - lo[axis]) * np.sin(phase))[:, None]
        normals[k, :, axis] = f32(-0.1) * np.cos(phase)
    return dict(positions=positions.reshape(TARGETS, n, 3, 3), normals=normals.reshape(TARGETS, n, 3, 3))


def frame(round_index, active):
    w = np.zeros(TARGETS, dtype=f32)
    for k in range(active):
        w[k] = f32(0.15 * (round_index + 1) * (-1.0) ** k / (1 + k // 2))
    return w


def report(title, runs):
    print("  %s" % title)
    for stage in STAGES:
        t = sorted(r[stage] for r in runs)
        unit = "" if stage == "area_ratio" else " ms"
        print("    %-10s median %9.3f%s  (min %9.3f max %9.3f, %d runs)" % (stage, statistics.median(t), unit, t[0], t[-1], len(t)))


def timings(title, mesh):
    import torch

    live = {way: World(scenes.c3_flat(**mesh)) for way in ("morph", "update", "update-dev")}
    rest = rest_of(live["morph"])
    ranges = live["morph"].objects
    knot = [k for k, o in enumerate(ranges) if o["first_triangle"] == BOX_TRIANGLES]
    assert len(knot) == 1 and ranges[knot[0]]["num_triangles"] == len(rest["positions"]) - BOX_TRIANGLES == 2 * mesh["segments"] * mesh["sides"]
    morphs = {knot[0]: knot_targets(rest, ranges[knot[0]])}
    once = morphs[knot[0]]["positions"].nbytes + morphs[knot[0]]["normals"].nbytes
    print("%s: %d triangles, %d targets with normal deltas; a frame is %d bytes (8 weights and %d poses; the table of active pairs and the morph records the call "
          "writes to the device: at most %d), the deltas %.1f MB once, the arrays of an update %.1f MB"
          % (title, len(rest["positions"]), TARGETS, 4 * TARGETS + 80 * len(ranges), len(ranges), 8 * TARGETS + 48 + 96 * len(ranges), once / 1e6,
             (rest["positions"].nbytes + rest["normals"].nbytes) / 1e6), flush=True)
    for world in live.values():
        world.scene(0, build="device")
    live["morph"].set_morphs(morphs)
    for active in ACTIVE:
        runs = {way: [] for way in live}
        host_ms = []
        for i in range(REPEATS + 1):
            weights = {knot[0]: frame(i, active)}
            t0 = time.perf_counter()
            want = restatement.morph_arrays(rest, ranges, morphs, weights)
            host_ms.append((time.perf_counter() - t0) * 1e3)
            p, n = want["positions"], want["normals"]
            tp, tn = torch.from_numpy(p).to("cuda:0"), torch.from_numpy(n).to("cuda:0")
            row = {}
            for way, call in (("morph", lambda: live["morph"].morph(weights)),
                              ("update", lambda: live["update"].update(positions=p, normals=n, mode="refit")),
                              ("update-dev", lambda: live["update-dev"].update(positions=tp, normals=tn, mode="refit"))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                row[way] = dict(live[way].update_info(), wall_ms=wall)
            if i > 0:  # the first round is the warm-up
                for way in runs:
                    runs[way].append(row[way])
        print(" %d of %d targets active" % (active, TARGETS))
        report("morph      (World.morph, refit; upload_ms = the morph, pose and skin kernels and the read-back of the flag)", runs["morph"])
        report("update     (World.update mode=refit, host arrays)", runs["update"])
        report("update-dev (World.update mode=refit, device tensors)", runs["update-dev"])
        print("    the host's restatement of the frame for the two update paths (numpy, on no bill): median %.3f ms" % statistics.median(host_ms[1:]))
        med = {way: statistics.median(r["total_ms"] for r in runs[way]) for way in runs}
        wall = {way: statistics.median(r["wall_ms"] for r in runs[way]) for way in runs}
        share = statistics.median(r["upload_ms"] / r["total_ms"] for r in runs["morph"])
        print("    morph: upload_ms / total_ms median %.2f; total_ms medians: update / morph = %.1f, update-dev / morph = %.1f; wall_ms medians: update / morph = %.1f, update-dev / morph = %.1f"
              % (share, med["update"] / med["morph"], med["update-dev"] / med["morph"], wall["update"] / wall["morph"], wall["update-dev"] / wall["morph"]))
        got = live["morph"].geometry()
        differ = sum(int((got[key].view(np.uint32) != want[key].view(np.uint32)).sum()) for key in ("positions", "normals"))
        print("    words of the morphed positions and normals that differ from the restatement's: %d" % differ, flush=True)
    for world in live.values():
        world.close()


if __name__ == "__main__":
    for title, mesh in MESHES:
        timings(title, mesh)
