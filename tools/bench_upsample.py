#!/usr/bin/env python3
"""Developer tool (GPU box): what the guided upsampling costs.

    python tools/bench_upsample.py [--no-session]

In one process, HIP events around the enqueue on the current stream, one warm-up and seven timed repetitions per row, the rows turn
by turn, median and spread:
  - pyr_image_upsample_device to 1920 x 1080 from C3 rendered at 960 x 540 (scale 2) and at 480 x 270 (scale 4), 8 samples a pixel,
    under C3's own feature passes at both sizes, at radius 1 and 2, with neither pair, with the albedo pair, with the records pair and
    with both, each against the floor of the bytes the rule must move -- per output pixel 12 B written, 12 B of albedo and 20 B of a
    record (16 B and the material word) read, the same per low pixel for the low image and its guides -- at the 3.0 TB/s
    reproject_kernel reached;
  - unless --no-session: one frame through the session entry at scale 2 (development, both feature passes, the upsample, the copy to
    the host; wall clock) beside Session.linear."""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyrite_amd import develop, scenes  # noqa: E402
from pyrite_amd._lib import check, lib  # noqa: E402

REPEATS = 7
W, H, SPP = 1920, 1080, 8
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


def on_device(array):
    return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).to(dev)


world, cam, r, host_film = scenes.build(scenes.c3_mesh_in_box(W, H, SPP), seed=1)
del host_film
full = r.features((W, H), cam, world)
albedo, pixels = on_device(develop.develop_linear(full.albedo, "srgb")), on_device(full.records)
out = torch.zeros(W * H * 3, dtype=torch.float32, device=dev)
runs = {}
for scale in (2, 4):
    w, h = W // scale, H // scale
    with r.session((w, h), cam, world) as s:
        s.render(SPP)
        low = on_device(s.linear())
    guides = r.features((w, h), cam, world)
    low_albedo, low_pixels = on_device(develop.develop_linear(guides.albedo, "srgb")), on_device(guides.records)
    for radius in (1, 2):
        for name, with_albedo, with_records in (("neither pair", False, False), ("albedo pair", True, False), ("records pair", False, True), ("both pairs", True, True)):
            def run(scale=scale, w=w, h=h, low=low, low_albedo=low_albedo, low_pixels=low_pixels, with_albedo=with_albedo, with_records=with_records,
                    p=develop.upsample_params(radius=radius)):
                at = lambda t, given: C.c_void_p(t.data_ptr()) if given else None  # noqa: E731
                check(lib().pyr_image_upsample_device(at(low, True), at(low_albedo, with_albedo), at(low_pixels, with_records), w, h, scale, at(albedo, with_albedo),
                                                      at(pixels, with_records), C.byref(p), C.c_void_p(out.data_ptr()), 0, C.c_void_p(stream.cuda_stream)))
            per_pixel = 12 + 12 * with_albedo + 20 * with_records
            runs["from %4dx%-4d radius %d, %-12s" % (w, h, radius, name)] = (run, per_pixel * (W * H + w * h))
times = {name: [] for name in runs}
for turn in range(REPEATS + 1):  # the first turn warms up; the rows alternate
    for name, (run, _) in runs.items():
        ms = timed(run)
        if turn:
            times[name].append(ms)
for name, (run, moved) in runs.items():
    t = sorted(times[name])
    median = statistics.median(t)
    floor_ms = moved / FLOOR_RATE * 1e3
    print("%dx%d upsample %s median %7.3f ms  (min %7.3f max %7.3f, %d runs)  %5.1f MB to move: floor %.3f ms at 3.0 TB/s, %.1f x the floor, %5.0f GB/s" % (
        W, H, name, median, t[0], t[-1], len(t), moved / 1e6, floor_ms, median / floor_ms, moved / median / 1e6), flush=True)

if "--no-session" not in sys.argv:
    linear_ms, upsampled_ms = [], []
    with r.session((W // 2, H // 2), cam, world) as s:
        s.render(SPP)
        s.sync()
        for turn in range(REPEATS + 1):
            t0 = time.perf_counter()
            s.linear()
            t1 = time.perf_counter()
            s.upsampled(2)
            t2 = time.perf_counter()
            if turn:
                linear_ms.append(1e3 * (t1 - t0)), upsampled_ms.append(1e3 * (t2 - t1))
    print("session %dx%d, wall clock, median of %d: Session.linear (development + 6.2 MB to the host) %.2f ms; Session.upsampled(2) (development, two feature passes, "
          "two albedo developments, upsample, 24.9 MB to the host) %.2f ms" % (W // 2, H // 2, len(linear_ms), statistics.median(linear_ms), statistics.median(upsampled_ms)), flush=True)
world.close()
