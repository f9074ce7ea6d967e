#!/usr/bin/env python3
"""Developer tool (GPU box): what scene creation costs with the BVH built on the host and on the device.

    python tools/bench_build.py [repeats] > profiles/r10_build.txt

One process. Two meshes: C3's (scenes.c3_flat, 819,212 triangles) and the 160 x 160 torus knot in the same box that the tone and
denoise benches render. Per mesh one warm-up and `repeats` (default 7) scene creations per builder, host and device alternating;
every scene is destroyed before the next is created. Reported per builder: the median, smallest and largest of each stage time of
PyrBuildInfo (host wall clock, milliseconds) and the tree's digest; then whether the two digests and PyrBvhInfo are equal."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyrite_amd import scenes  # noqa: E402
from pyrite_amd.renderer import World  # noqa: E402

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STAGES = ("bounds_ms", "tree_ms", "finish_ms", "collapse_ms", "pack_upload_ms", "total_ms")
MESHES = [("C3 mesh (scenes.c3_flat)", dict(segments=640, sides=640)), ("160 x 160 knot mesh", dict(segments=160, sides=160))]


def create(world, build):
    world.scene(0, build=build)
    info, bvh = world.build_info(), world.bvh_info()
    world.close()
    return info, bvh


for title, mesh in MESHES:
    world = World(scenes.c3_flat(**mesh))
    print("%s: %d triangles" % (title, world.desc.num_triangles), flush=True)
    runs = {"host": [], "device": []}
    for i in range(REPEATS + 1):
        for build in ("host", "device"):
            info, bvh = create(world, build)
            if i > 0:  # the first of each is the warm-up
                runs[build].append((info, bvh))
    for build in ("host", "device"):
        info, bvh = runs[build][0]
        used = "device" if info["builder_used"] == 1 else "host"
        print("  asked %-6s used %-6s fallback %d  levels %2d  median splits %d  digest %016x  nodes %d  leaves %d  depth %d  wide nodes %d  pair records %d"
              % (build, used, info["fallback_reason"], info["levels"], info["median_splits"], info["tree_digest"], bvh["num_nodes"], bvh["num_leaves"], bvh["max_depth"],
                 bvh["num_wide_nodes"], bvh["num_pair_records"]))
        for stage in STAGES:
            t = sorted(r[0][stage] for r in runs[build])
            print("    %-15s median %9.2f ms  (min %9.2f max %9.2f, %d runs)" % (stage, statistics.median(t), t[0], t[-1], len(t)))
        assert len({r[0]["tree_digest"] for r in runs[build]}) == 1, "the %s builder's digest moved between runs" % build
    same = runs["host"][0][0]["tree_digest"] == runs["device"][0][0]["tree_digest"] and runs["host"][0][1] == runs["device"][0][1]
    ratio = statistics.median(r[0]["tree_ms"] for r in runs["host"]) / max(1e-9, statistics.median(r[0]["tree_ms"] + r[0]["finish_ms"] for r in runs["device"]))
    print("  digests and PyrBvhInfo equal: %s;  host tree_ms / device (tree_ms + finish_ms): %.1fx" % ("yes" if same else "NO", ratio), flush=True)
    world.close()
