#!/usr/bin/env python3
"""Developer tool (GPU box): what a frame of a bending mesh costs when it is skinned on the GPU, against
uploading whole new arrays (section 9f).

    python tools/bench_skin.py [repeats] > profiles/r16_skin.txt

One process, one GPU. Two meshes: C3's (scenes.c3_flat) and the 160 x 160 torus knot in the same box. The knot is skinned to 64
joints placed along its parameter (the closed curve the tube follows): a vertex of segment s lies between joints floor(64 s / S)
and the next one, and its two weights fall linearly between them. Per mesh one warm-up and `repeats` (default 7) rounds; in a round
every joint turns about the vertical axis through the knot's centre and rises or sinks, by amounts that vary along the knot and grow
from round to round, in four ways on four live scenes, alternating:
  skin       World.skin: 64 matrices, the triangles computed on the device (pyr_scene_skin, refit)
  skin-dq    the same frame with the skin dual-quaternion (pyr_scene_set_skin_blend); its row comes last
  update     World.update(mode="refit") from host arrays (pyr_scene_update) of the same deformed geometry
  update-dev World.update(mode="refit") from torch tensors on the device (pyr_scene_update_device), uploaded beforehand
The arrays of the last two are computed by the numpy restatement of the skin rule (tests/skin_restatement.py) before the clock starts;
what the host spends on that is printed once per mesh and is on no bill. Reported per way: the median, smallest and largest of
PyrUpdateInfo's upload_ms, prims_ms, refit_ms and total_ms (skin and update-dev enqueue: their prims_ms and refit_ms are the time to
enqueue), of the wall clock of the World call with its kernels waited for, and of area_ratio after the call."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dq_skin_restatement  # noqa: E402
import skin_restatement as restatement  # noqa: E402

from pyrite_amd import scenes  # noqa: E402
from pyrite_amd.renderer import World  # noqa: E402

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STAGES = ("upload_ms", "prims_ms", "refit_ms", "total_ms", "wall_ms", "area_ratio")
MESHES = [("C3 mesh (scenes.c3_flat)", dict(segments=640, sides=640)), ("160 x 160 knot mesh", dict(segments=160, sides=160))]
BOX_TRIANGLES = 12  # the Cornell box without its two blocks comes first in scenes.c3_flat
JOINTS = 64


def rest_of(world):
    cat = lambda rows: np.concatenate([np.asarray(r, dtype=np.float32).reshape(-1, 9) for r in rows])  # noqa: E731
    return {"positions": cat(world.flat.tri_positions), "normals": cat(world.flat.tri_normals), "frames": None, "spheres": np.zeros((0, 4), dtype=np.float32)}


def knot_bindings(segments, sides):
    """joints uint16 [T,3,4] and weights float32 [T,3,4] of scenes.torus_knot_mesh's triangles: its faces, in its order, by the
    segment each vertex belongs to."""
    i, j = np.arange(segments)[:, None], np.arange(sides)[None, :]
    i1 = (i + 1) % segments
    quad = np.stack([i + 0 * j, i1 + 0 * j, i1 + 0 * j, i + 0 * j], axis=-1).reshape(-1, 4)  # the segment of each corner of each quad
    segment = np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]], axis=0).reshape(-1)
    x = segment.astype(np.float64) * JOINTS / segments
    first = np.floor(x).astype(np.int64) % JOINTS
    w1 = (x - np.floor(x)).astype(np.float32)
    joints = np.stack([first, (first + 1) % JOINTS, np.zeros_like(first), np.zeros_like(first)], axis=1).astype(np.uint16)
    weights = np.stack([np.float32(1.0) - w1, w1, np.zeros_like(w1), np.zeros_like(w1)], axis=1).astype(np.float32)
    return dict(joints=joints.reshape(-1, 3, 4), weights=weights.reshape(-1, 3, 4), num_joints=JOINTS)


def frame(round_index, centre):
    """The 64 joint matrices of a round, [64,4,4] as on paper, float32: a turn about the vertical axis through `centre` and a lift,
    both varying once around the knot."""
    out = np.zeros((JOINTS, 4, 4))
    for k in range(JOINTS):
        phase = 2.0 * np.pi * k / JOINTS
        a = np.radians(1.5 * (round_index + 1)) * np.sin(phase)
        m = np.eye(4)
        m[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
        m[:3, 3] = centre - m[:3, :3] @ centre
        m[2, 3] += 0.2 * (round_index + 1) * np.cos(phase)
        out[k] = m
    return out.astype(np.float32)


def report(title, runs):
    print("  %s" % title)
    for stage in STAGES:
        t = sorted(r[stage] for r in runs)
        unit = "" if stage == "area_ratio" else " ms"
        print("    %-10s median %9.3f%s  (min %9.3f max %9.3f, %d runs)" % (stage, statistics.median(t), unit, t[0], t[-1], len(t)))


def timings(title, mesh):
    import torch

    live = {way: World(scenes.c3_flat(**mesh)) for way in ("skin", "update", "update-dev", "skin-dq")}
    rest = rest_of(live["skin"])
    ranges = live["skin"].objects
    knot = [k for k, o in enumerate(ranges) if o["first_triangle"] == BOX_TRIANGLES]
    assert len(knot) == 1 and ranges[knot[0]]["num_triangles"] == len(rest["positions"]) - BOX_TRIANGLES == 2 * mesh["segments"] * mesh["sides"]
    skins = {knot[0]: knot_bindings(mesh["segments"], mesh["sides"])}
    centre = rest["positions"][BOX_TRIANGLES:].reshape(-1, 3).astype(np.float64).mean(axis=0)
    print("%s: %d triangles; a frame is %d bytes, the bindings %.1f MB once, the arrays of an update %.1f MB"
          % (title, len(rest["positions"]), 64 * JOINTS + 80 * len(ranges), 72 * ranges[knot[0]]["num_triangles"] / 1e6, (rest["positions"].nbytes + rest["normals"].nbytes) / 1e6), flush=True)
    for world in live.values():
        world.scene(0, build="device")
    live["skin"].set_skins(skins)
    dual = {index: dict(skin, blend="dual_quaternion") for index, skin in skins.items()}
    live["skin-dq"].set_skins(dual)
    runs = {way: [] for way in live}
    host_ms = []
    for i in range(REPEATS + 1):
        joints = {knot[0]: frame(i, centre)}
        t0 = time.perf_counter()
        want = restatement.skin_arrays(rest, ranges, skins, joints)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        p, n = want["positions"], want["normals"]
        tp, tn = torch.from_numpy(p).to("cuda:0"), torch.from_numpy(n).to("cuda:0")
        row = {}
        for way, call in (("skin", lambda: live["skin"].skin(joints)),
                          ("update", lambda: live["update"].update(positions=p, normals=n, mode="refit")),
                          ("update-dev", lambda: live["update-dev"].update(positions=tp, normals=tn, mode="refit")),
                          ("skin-dq", lambda: live["skin-dq"].skin(joints))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            row[way] = dict(live[way].update_info(), wall_ms=wall)
        if i > 0:  # the first round is the warm-up
            for way in runs:
                runs[way].append(row[way])
    report("skin       (World.skin, refit; upload_ms = the pose and skin kernels and the read-back of the flag)", runs["skin"])
    report("update     (World.update mode=refit, host arrays)", runs["update"])
    report("update-dev (World.update mode=refit, device tensors)", runs["update-dev"])
    print("    the host's restatement of the frame for the two update paths (numpy, on no bill): median %.3f ms" % statistics.median(host_ms[1:]))
    med = {way: statistics.median(r["total_ms"] for r in runs[way]) for way in runs}
    wall = {way: statistics.median(r["wall_ms"] for r in runs[way]) for way in runs}
    print("    total_ms medians: update / skin = %.1f, update-dev / skin = %.1f; wall_ms medians: update / skin = %.1f, update-dev / skin = %.1f"
          % (med["update"] / med["skin"], med["update-dev"] / med["skin"], wall["update"] / wall["skin"], wall["update-dev"] / wall["skin"]))
    got = live["skin"].geometry()
    differ = sum(int((got[key].view(np.uint32) != want[key].view(np.uint32)).sum()) for key in ("positions", "normals"))
    print("    words of the skinned positions and normals that differ from the restatement's: %d" % differ, flush=True)
    report("skin-dq    (World.skin with the skin dual-quaternion, refit)", runs["skin-dq"])
    print("    total_ms medians: skin-dq / skin = %.2f; wall_ms medians: skin-dq / skin = %.2f"
          % (statistics.median(r["total_ms"] for r in runs["skin-dq"]) / med["skin"], statistics.median(r["wall_ms"] for r in runs["skin-dq"]) / wall["skin"]))
    got, want = live["skin-dq"].geometry(), dq_skin_restatement.dq_skin_arrays(rest, ranges, dual, joints)
    differ = sum(int((got[key].view(np.uint32) != want[key].view(np.uint32)).sum()) for key in ("positions", "normals"))
    print("    words of its positions and normals that differ from the dual quaternion restatement's: %d" % differ, flush=True)
    for world in live.values():
        world.close()


if __name__ == "__main__":
    for title, mesh in MESHES:
        timings(title, mesh)
