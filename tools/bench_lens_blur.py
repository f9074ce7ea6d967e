#!/usr/bin/env python3
"""Developer tool (GPU box): what the lens blur over the feature records costs.

    python tools/bench_lens_blur.py [--only sharp|r8|r16|motion]

In one process, HIP events around the enqueue on the current stream, one warm-up and seven timed repetitions per row, median and
range, all at 1920 x 1080 on C3's full mesh, the records those of its feature pass:
  - the all-sharp frame: an aperture of 0, so every tile's reach is 0 and it copies its input; beside it the bytes that must move;
  - max_radius 8 and 16 with the focus on the mesh and an aperture under which c spans 0 .. the clamp, then one twenty times as
    wide a lens, under which every circle but the few in focus is the clamp; beside each the share of tiles that took the copy
    path and the mean reach of the others, computed from the restatement's circles;
  - pyr_image_motion_blur under a camera pan on the same box, for scale.
The lens blur enqueues one kernel and allocates nothing, so its event window is the kernel."""
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import lens_blur_restatement as R  # noqa: E402

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


world, cam, r, host_film = scenes.build(scenes.c3_mesh_in_box(W, H, 1), seed=1)
del host_film
desc = abi.PyrFilmDesc(W, H, r.spectrum_bins, r.spectrum_span[0], r.spectrum_span[1] - r.spectrum_span[0])
scene = world.scene(0)
image = torch.rand((H, W, 3), dtype=torch.float32, device=dev)
out = torch.zeros_like(image)
records = torch.zeros((H, W, 8), dtype=torch.int32, device=dev)
fp = abi.PyrFeatureParams(1, 1)
check(lib().pyr_render_features_device(scene, C.byref(cam.c), C.byref(desc), C.byref(fp), None, C.c_void_p(records.data_ptr()), C.c_void_p(stream.cuda_stream)))
torch.cuda.synchronize(dev)
host_records = records.cpu().numpy().view(R.RECORD).reshape(H, W)
z = R.circles(host_records, 1.0, 0.0, cam.c.view_plane, 1)[2]
hit = host_records["coverage"] > 0
focus = float(np.median(z[hit]))
print("records of %dx%d: %.1f %% hits, axial depth %.3g .. %.3g, the focus at the median %.3g" % (W, H, 100 * hit.mean(), float(z[hit].min()), float(z[hit].max()), focus), flush=True)


def tiles_of(c, radius):
    """(share of the 16 x 16 tiles whose staged slots hold no c above 0, mean reach of the others)."""
    t = torch.from_numpy(np.ascontiguousarray(c))[None, None]
    most = torch.nn.functional.max_pool2d(t, kernel_size=16 + 2 * radius, stride=16, padding=radius, ceil_mode=True)[0, 0]
    # max_pool2d pads by at most half the kernel: radius <= 8 + radius holds; windows are the tile and its ring
    reach = torch.ceil(most).clamp(max=radius)
    copies = reach == 0
    return float(copies.float().mean()), float(reach[~copies].mean()) if (~copies).any() else 0.0


def blur_row(what, radius, aperture):
    params = develop.lens_blur_params(cam, focus_distance=focus, aperture=aperture, max_radius=radius)
    times = []
    for turn in range(REPEATS + 1):  # the first turn warms up
        ms = timed(lambda: check(lib().pyr_image_lens_blur_device(C.c_void_p(image.data_ptr()), C.c_void_p(records.data_ptr()), W, H, C.byref(params), C.c_void_p(out.data_ptr()), 0,
                                                                  C.c_void_p(stream.cuda_stream))))
        if turn:
            times.append(ms)
    kept = float((out == image).all(dim=-1).float().mean())
    c = R.circles(host_records, focus, aperture, cam.c.view_plane, radius)[0]
    share, reach = tiles_of(c, radius)
    return report(what, times, "  c %.2f .. %.2f, median %.2f; %.1f %% of the tiles copy, mean reach of the others %.1f; %.1f %% of the pixels keep their bits"
                  % (float(c.min()), float(c.max()), float(np.median(c)), 100 * share, reach, 100 * kept))


if ONLY in (None, "sharp"):
    median = blur_row("lens blur %dx%d, aperture 0 (every tile copies), radius 8" % (W, H), 8, 0.0)
    must = PIXELS * (12 + 12 + 32)  # the image read and written, the records read
    print("  bytes that must move: %.1f MB (image in and out, records) -> %.0f GB/s at the median; the rings are read again through the cache" % (must / 1e6, must / median / 1e6), flush=True)
    blur_row("lens blur %dx%d, aperture 0 (every tile copies), radius 16" % (W, H), 16, 0.0)

# an aperture under which the surface most out of focus reaches 1.5 times the widest clamp: c spans 0 .. 8 and 0 .. 16
most = max(abs(1 - focus / float(z[hit].min())), abs(1 - focus / float(z[hit].max())))
aperture = (24.0 / most * focus / (cam.c.view_plane * max(W, H) * 0.5)) ** 2
if ONLY in (None, "r8"):
    blur_row("lens blur %dx%d, radius 8" % (W, H), 8, aperture)
if ONLY in (None, "r16"):
    blur_row("lens blur %dx%d, radius 16" % (W, H), 16, aperture)
# and one so wide that every pixel but the few in focus sits at the clamp: the most a frame can cost
if ONLY in (None, "r8"):
    blur_row("lens blur %dx%d, radius 8, every circle at the clamp" % (W, H), 8, 400 * aperture)
if ONLY in (None, "r16"):
    blur_row("lens blur %dx%d, radius 16, every circle at the clamp" % (W, H), 16, 400 * aperture)

if ONLY in (None, "motion"):  # for scale: the motion blur of a pan that moves every pixel beyond its clamp, 15 taps of length 16
    angle = 80.0 / (cam.c.view_plane * max(W, H) / 2)
    c = abi.PyrCamera.from_buffer_copy(cam.c)
    m = np.array(c.cam_to_world[:], dtype=np.float64).reshape(4, 4).T
    turn = np.eye(4)
    turn[0, 0] = turn[2, 2] = np.cos(angle)
    turn[0, 2], turn[2, 0] = np.sin(angle), -np.sin(angle)
    c.cam_to_world = (C.c_float * 16)(*[float(v) for v in (m @ turn).astype(np.float32).T.reshape(-1)])
    world.keep_previous()
    motion = torch.zeros((H, W, 8), dtype=torch.int32, device=dev)
    check(lib().pyr_render_motion_device(scene, C.byref(cam.c), C.byref(Camera(c).c), C.byref(desc), C.c_void_p(motion.data_ptr()), C.c_void_p(stream.cuda_stream)))
    torch.cuda.synchronize(dev)
    mp = develop.motion_blur_params()
    times = []
    for turn_ in range(REPEATS + 1):
        ms = timed(lambda: check(lib().pyr_image_motion_blur_device(C.c_void_p(image.data_ptr()), C.c_void_p(motion.data_ptr()), W, H, C.byref(mp), C.c_void_p(out.data_ptr()), 0,
                                                                    C.c_void_p(stream.cuda_stream))))
        if turn_:
            times.append(ms)
    report("motion blur %dx%d, camera pan, 15 taps of length 16" % (W, H), times, "  (three kernels and a stream-ordered allocation in the window)")
    world.keep_previous(False)
world.close()
