#!/usr/bin/env python3
"""Developer tool (GPU box): what the glare costs.

    python tools/bench_glare.py [--no-session] [--level-bytes 12]

In one process, HIP events around the enqueue on the current stream, one warm-up and seven timed repetitions per row, the rows turn
by turn, median and spread:
  - pyr_image_glare_device at 1920 x 1080 on C3's developed image (8 samples a pixel, linear sRGB), 6 and 11 levels, in the plain
    form (one launch a step, PYRITE_GLARE_TAIL=0) and in the tail form (the small levels in one workgroup, PYRITE_GLARE_TAIL=1),
    each against the floor of the bytes the rule must move -- the image read twice, out written once, every level written once
    and read twice -- at the 3.0 TB/s reproject_kernel reached;
  - the two forms' outputs compared byte for byte at the size they are timed at;
  - unless --no-session: one frame through the session entry (development, glare, the copy to the host; wall clock) beside
    Session.linear."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pyrite_amd import develop, scenes  # noqa: E402
from pyrite_amd._lib import check, lib  # noqa: E402

REPEATS = 7
W, H, SPP = 1920, 1080, 8
# a pixel of a level in working memory (kernels/glare.hip, kPixelFloats): 12 for a build with -DPYR_GLARE_PIXEL_FLOATS=3 (PYRITE_GPU_LIB)
LEVEL_BYTES = int(sys.argv[sys.argv.index("--level-bytes") + 1]) if "--level-bytes" in sys.argv else 16
FLOOR_RATE = 3.0e12  # bytes a second: what reproject_kernel reached
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def level_pixels(width, height, levels):
    sizes = [(width, height)]
    while len(sizes) - 1 < levels and sizes[-1] != (1, 1):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return [w * h for w, h in sizes[1:]]


world, cam, r, host_film = scenes.build(scenes.c3_mesh_in_box(W, H, SPP), seed=1)
del host_film
with r.session((W, H), cam, world) as s:
    s.render(SPP)
    image_host = s.linear()
image = torch.from_numpy(image_host).to(dev)
out = torch.zeros_like(image)
luminance = image_host @ np.array([0.2126, 0.7152, 0.0722], dtype=np.float32)
print("c3 %dx%d, %d samples a pixel, linear sRGB: luminance median %.4f, 99.9th percentile %.3f, largest %.2f; %d pixels not finite" % (
    W, H, SPP, float(np.median(luminance)), float(np.percentile(luminance, 99.9)), float(luminance.max()), int((~np.isfinite(image_host).all(axis=-1)).sum())), flush=True)


def glare(levels, tail):
    p = develop.glare_params(levels=levels)

    def run():
        os.environ["PYRITE_GLARE_TAIL"] = "1" if tail else "0"  # read at every call
        check(lib().pyr_image_glare_device(C.c_void_p(image.data_ptr()), W, H, C.byref(p), C.c_void_p(out.data_ptr()), 0, C.c_void_p(stream.cuda_stream)))
    return run


runs = {}
for levels in (6, 11):
    for tail in (False, True):
        runs["%2d levels, %s" % (levels, "tail" if tail else "plain")] = (glare(levels, tail), levels)
times = {name: [] for name in runs}
for turn in range(REPEATS + 1):  # the first turn warms up; the rows alternate
    for name, (run, _) in runs.items():
        ms = timed(run)
        if turn:
            times[name].append(ms)
for name, (run, levels) in runs.items():
    t = sorted(times[name])
    median = statistics.median(t)
    moved = W * H * 36 + 3 * LEVEL_BYTES * sum(level_pixels(W, H, levels))
    floor_ms = moved / FLOOR_RATE * 1e3
    print("%dx%d glare %-18s median %7.3f ms  (min %7.3f max %7.3f, %d runs)  %5.1f MB to move: floor %.3f ms at 3.0 TB/s, %.1f x the floor, %5.0f GB/s" % (
        W, H, name, median, t[0], t[-1], len(t), moved / 1e6, floor_ms, median / floor_ms, moved / median / 1e6), flush=True)
for levels in (6, 11):
    results = []
    for tail in (False, True):
        out.fill_(-1.0)
        glare(levels, tail)()
        torch.cuda.synchronize(dev)
        results.append(out.cpu().numpy().tobytes())
    print("  %2d levels: the two forms write %s" % (levels, "the same bytes" if results[0] == results[1] else "DIFFERENT bytes"), flush=True)
os.environ.pop("PYRITE_GLARE_TAIL", None)

if "--no-session" not in sys.argv:
    linear_ms, glared_ms = [], []
    with r.session((W, H), cam, world) as s:
        s.render(SPP)
        s.sync()
        for turn in range(REPEATS + 1):
            t0 = time.perf_counter()
            s.linear()
            t1 = time.perf_counter()
            s.glared()
            t2 = time.perf_counter()
            if turn:
                linear_ms.append(1e3 * (t1 - t0)), glared_ms.append(1e3 * (t2 - t1))
    print("session %dx%d, wall clock, median of %d: Session.linear (development + 24.9 MB to the host) %.2f ms; Session.glared (development, glare, 24.9 MB to the host) %.2f ms" % (
        W, H, len(linear_ms), statistics.median(linear_ms), statistics.median(glared_ms)), flush=True)
world.close()
