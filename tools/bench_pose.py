#!/usr/bin/env python3
"""Developer tool (GPU box): what a turntable frame costs when the object is posed on the GPU, against
uploading whole new arrays (section 9f).

    python tools/bench_pose.py [repeats] > profiles/r13_pose.txt

One process, one GPU. Two meshes: C3's (scenes.c3_flat) and the 160 x 160 torus knot in the same box. Per mesh one warm-up and
`repeats` (default 7) rounds; a round turns the knot two degrees further about the vertical axis through its centre, in three ways
on three live scenes, alternating:
  pose       World.pose: one matrix for the knot's object, the triangles computed on the device (pyr_scene_pose, refit)
  update     World.update(mode="refit") from host arrays (pyr_scene_update), the arrays computed beforehand
  update-dev World.update(mode="refit") from torch tensors on the device (pyr_scene_update_device), uploaded beforehand
The last two are the paths that existed before poses, run here in the same process. Reported per way: the median, smallest and
largest of PyrUpdateInfo's upload_ms, prims_ms, refit_ms and total_ms (pose and update-dev enqueue: their prims_ms and refit_ms are
the time to enqueue), and of the wall clock of the World call with its kernels waited for (the Python layer's own bookkeeping
included: World.update keeps `flat` and the description in step). What the host spends computing the arrays of
the update paths (a rotation of every vertex and normal in numpy) is printed once per mesh and is on neither bill."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyrite_amd import scenes  # noqa: E402
from pyrite_amd.renderer import World  # noqa: E402

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STAGES = ("upload_ms", "prims_ms", "refit_ms", "total_ms", "wall_ms")
MESHES = [("C3 mesh (scenes.c3_flat)", dict(segments=640, sides=640)), ("160 x 160 knot mesh", dict(segments=160, sides=160))]
BOX_TRIANGLES = 12  # the Cornell box without its two blocks comes first in scenes.c3_flat


def arrays_of(world):
    cat = lambda rows: np.concatenate([np.asarray(r, dtype=np.float32).reshape(-1, 9) for r in rows])  # noqa: E731
    return cat(world.flat.tri_positions), cat(world.flat.tri_normals)


def turn(degrees, centre):
    """The rotation about the vertical axis through `centre`, 4x4 as on paper, float64."""
    a = np.radians(degrees)
    m = np.eye(4)
    m[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    m[:3, 3] = centre - m[:3, :3] @ centre
    return m


def knot_turned(positions, normals, m):
    p, n = positions.reshape(-1, 3, 3).astype(np.float64), normals.reshape(-1, 3, 3).astype(np.float64)
    p[BOX_TRIANGLES:] = p[BOX_TRIANGLES:] @ m[:3, :3].T + m[:3, 3]
    n[BOX_TRIANGLES:] = n[BOX_TRIANGLES:] @ m[:3, :3].T
    return p.astype(np.float32).reshape(-1, 9), n.astype(np.float32).reshape(-1, 9)


def report(title, runs):
    print("  %s" % title)
    for stage in STAGES:
        t = sorted(r[stage] for r in runs)
        print("    %-10s median %9.3f ms  (min %9.3f max %9.3f, %d runs)" % (stage, statistics.median(t), t[0], t[-1], len(t)))


def timings(title, mesh):
    import torch

    live = {way: World(scenes.c3_flat(**mesh)) for way in ("pose", "update", "update-dev")}
    positions, normals = arrays_of(live["pose"])
    knot = [k for k, o in enumerate(live["pose"].objects) if o["first_triangle"] == BOX_TRIANGLES]
    assert len(knot) == 1 and live["pose"].objects[knot[0]]["num_triangles"] == len(positions) - BOX_TRIANGLES
    centre = positions[BOX_TRIANGLES:].reshape(-1, 3).astype(np.float64).mean(axis=0)
    print("%s: %d triangles; a pose is %d bytes, the arrays of an update %.1f MB" % (title, len(positions), 80 * len(live["pose"].objects), (positions.nbytes + normals.nbytes) / 1e6),
          flush=True)
    for world in live.values():
        world.scene(0, build="device")
    runs = {way: [] for way in live}
    host_ms = []
    for i in range(REPEATS + 1):
        m = turn(2.0 * (i + 1), centre)
        t0 = time.perf_counter()
        p, n = knot_turned(positions, normals, m)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        tp, tn = torch.from_numpy(p).to("cuda:0"), torch.from_numpy(n).to("cuda:0")
        row = {}
        for way, call in (("pose", lambda: live["pose"].pose({knot[0]: (m.astype(np.float32), 1.0)})),
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
    report("pose       (World.pose, refit; upload_ms = the pose kernels and the read-back of the flag)", runs["pose"])
    report("update     (World.update mode=refit, host arrays)", runs["update"])
    report("update-dev (World.update mode=refit, device tensors)", runs["update-dev"])
    print("    the host's rotation of the arrays for the two update paths (numpy, on neither bill): median %.3f ms" % statistics.median(host_ms[1:]))
    med = {way: statistics.median(r["total_ms"] for r in runs[way]) for way in runs}
    wall = {way: statistics.median(r["wall_ms"] for r in runs[way]) for way in runs}
    print("    total_ms medians: update / pose = %.1f, update-dev / pose = %.1f; wall_ms medians: update / pose = %.1f, update-dev / pose = %.1f"
          % (med["update"] / med["pose"], med["update-dev"] / med["pose"], wall["update"] / wall["pose"], wall["update-dev"] / wall["pose"]))
    # the three scenes end in the same place: the posed geometry next to the arrays the update paths were given (f32 on the device
    # against f64 rounded once on the host: close, not equal)
    got = live["pose"].geometry()
    print("    largest difference between the posed positions and the host's arrays: %.3g" % float(np.abs(got["positions"] - p).max()), flush=True)
    for world in live.values():
        world.close()


if __name__ == "__main__":
    for title, mesh in MESHES:
        timings(title, mesh)
