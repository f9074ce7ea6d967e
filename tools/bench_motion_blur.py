#!/usr/bin/env python3
"""Developer tool (GPU box): what the motion blur over the motion records costs.

    python tools/bench_motion_blur.py [--only static|pan|posed]

In one process, HIP events around the enqueue on the current stream, one warm-up and seven timed repetitions per row, median and
spread, all at 1920 x 1080 on C3's full mesh with the default parameters (15 taps, tiles of 16, shutter 0.5):
  - the static frame: records of a camera and a scene that did not move, so every tile takes the copy path; beside it the bytes
    that must move;
  - a camera pan that moves every pixel by more than the clamp: every pixel gathers 15 taps of length 16, the worst case;
  - only the mesh posed (turned by two degrees about its axis, the box at rest): most tiles copy, some gather;
  - one frame through the session entry (development, motion pass, blur, the copy to the host; wall clock) beside the frame's render.
The event window of a row holds what the device entry enqueues: the stream-ordered allocation of the working memory (33 MB), the three
kernels and the free, enqueued on an empty stream: what the host spends between the launches falls into the window too, and it is
several times the kernels' own time (profiles/r19_motion_blur.txt). For the kernels by themselves run one row under a profiler:
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_motion_blur.py --only pan`."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pyrite_amd import abi, develop, scenes  # noqa: E402
from pyrite_amd._lib import check, lib  # noqa: E402
from pyrite_amd.renderer import Camera  # noqa: E402

REPEATS = 7
ONLY = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
W, H = 1920, 1080
PIXELS = W * H
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def report(what, times, extra=""):
    t = sorted(times)
    print("%-58s median %8.3f ms  (min %8.3f max %8.3f, %d runs)  %8.1f Mpixels/s%s" % (what, statistics.median(t), t[0], t[-1], len(t), PIXELS / statistics.median(t) / 1e3, extra),
          flush=True)
    return statistics.median(t)


def turned_camera(cam, angle):
    """`cam` turned about its own y axis by `angle`."""
    c = abi.PyrCamera.from_buffer_copy(cam.c)
    m = np.array(c.cam_to_world[:], dtype=np.float64).reshape(4, 4).T
    turn = np.eye(4)
    turn[0, 0] = turn[2, 2] = np.cos(angle)
    turn[0, 2], turn[2, 0] = np.sin(angle), -np.sin(angle)
    c.cam_to_world = (C.c_float * 16)(*[float(v) for v in (m @ turn).astype(np.float32).T.reshape(-1)])
    return Camera(c)


world, cam, r, host_film = scenes.build(scenes.c3_mesh_in_box(W, H, 1), seed=1)
del host_film
desc = abi.PyrFilmDesc(W, H, r.spectrum_bins, r.spectrum_span[0], r.spectrum_span[1] - r.spectrum_span[0])
scene = world.scene(0)
image = torch.rand((H, W, 3), dtype=torch.float32, device=dev)
out = torch.zeros_like(image)
params = develop.motion_blur_params()


def records_against(previous):
    records = torch.zeros((H, W, 8), dtype=torch.int32, device=dev)
    check(lib().pyr_render_motion_device(scene, C.byref(cam.c), C.byref(previous.c), C.byref(desc), C.c_void_p(records.data_ptr()), C.c_void_p(stream.cuda_stream)))
    torch.cuda.synchronize(dev)
    return records


def blur_row(what, records):
    times = []
    for turn in range(REPEATS + 1):  # the first turn warms up
        ms = timed(lambda: check(lib().pyr_image_motion_blur_device(C.c_void_p(image.data_ptr()), C.c_void_p(records.data_ptr()), W, H, C.byref(params), C.c_void_p(out.data_ptr()), 0,
                                                                    C.c_void_p(stream.cuda_stream))))
        if turn:
            times.append(ms)
    copied = float((out == image).all(dim=-1).float().mean())
    prev = records.view(torch.float32)[..., :2]
    x, y = torch.arange(W, device=dev, dtype=torch.float32) + 0.5, torch.arange(H, device=dev, dtype=torch.float32) + 0.5
    moved = torch.sqrt((x[None, :] - prev[..., 0]) ** 2 + (y[:, None] - prev[..., 1]) ** 2)
    return report(what, times, "  %.1f %% of the pixels keep their bits; motion median %.1f, max %.1f pixels a frame" % (100 * copied, float(moved.median()), float(moved.max())))


# ------------------------------------------------------------------------------------------------ the static frame
world.keep_previous()
if ONLY in (None, "static"):
    median = blur_row("blur %dx%d, static frame (every tile copies)" % (W, H), records_against(cam))
if ONLY is None:
    tiles = ((W + params.max_radius - 1) // params.max_radius) * ((H + params.max_radius - 1) // params.max_radius)
    must = PIXELS * (12 + 12)  # the image read and written
    velocity = PIXELS * (32 + 16) + tiles * 16 * 3  # the records read, the compact velocity image written, the tile arrays
    print("  bytes that must move: %.1f MB image in and out + %.1f MB velocity step (+ 16 B of neighbour maximum a pixel through the cache) -> %.0f GB/s at the median" % (
        must / 1e6, velocity / 1e6, (must + velocity) / median / 1e6), flush=True)

# ------------------------------------------------------------------------------------------------ the pan: every pixel gathers
angle = 80.0 / (cam.c.view_plane * max(W, H) / 2)  # about 80 pixels a frame at the image's centre: a half velocity of 20 at shutter 0.5, clamped to 16
if ONLY in (None, "pan"):
    median = blur_row("blur %dx%d, camera pan, 15 taps of length 16" % (W, H), records_against(turned_camera(cam, angle)))
    taps = PIXELS * 15 * (16 + 12)
    print("  through the cache: %.2f GB of taps (16 + 12 B each) -> %.0f GB/s at the median" % (taps / 1e9, taps / median / 1e6), flush=True)

# ------------------------------------------------------------------------------------------------ only the mesh posed
knot = max(range(len(world.objects)), key=lambda k: world.objects[k]["num_triangles"])
first, count = world.objects[knot]["first_triangle"], world.objects[knot]["num_triangles"]
centre = world.geometry()["positions"].reshape(-1, 3, 3)[first:first + count].reshape(-1, 3).astype(np.float64).mean(axis=0)
a = np.radians(2.0)
m = np.eye(4)
m[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
m[:3, 3] = centre - m[:3, :3] @ centre
if ONLY in (None, "posed"):
    world.keep_previous()
    world.pose({knot: (m.astype(np.float32), 1.0)})
    blur_row("blur %dx%d, the mesh turned by 2 degrees, the box at rest" % (W, H), records_against(cam))
    world.pose({})
world.keep_previous(False)
del image, out
if ONLY is not None:
    world.close()
    sys.exit(0)

# ------------------------------------------------------------------------------------------------ a frame through the session entry
SPP = 32
r.pixel_samples = SPP
previous = turned_camera(cam, angle / 10)
render_ms, blur_ms, linear_ms = [], [], []
for turn in range(REPEATS + 1):
    with r.session((W, H), cam, world) as s:
        t0 = time.perf_counter()
        s.render(SPP)
        s.sync()
        t1 = time.perf_counter()
        s.linear()
        t2 = time.perf_counter()
        s.motion_blurred(previous)
        t3 = time.perf_counter()
    if turn:
        render_ms.append(1e3 * (t1 - t0)), linear_ms.append(1e3 * (t2 - t1)), blur_ms.append(1e3 * (t3 - t2))
print("session %dx%d, %d samples a pixel, wall clock, median of %d: render %.2f ms; Session.linear (development + 24.9 MB to the host) %.2f ms; "
      "Session.motion_blurred (development, motion pass, blur, 24.9 MB to the host) %.2f ms" % (W, H, SPP, len(render_ms), statistics.median(render_ms), statistics.median(linear_ms),
                                                                                                 statistics.median(blur_ms)), flush=True)
world.close()
