#!/usr/bin/env python3
"""Developer tool (GPU box): what the motion pass and the accumulation over frames cost and buy.

    python tools/bench_motion.py

In one process, HIP events around the enqueue on the current stream, one warm-up and seven timed repetitions per row, median and
spread:
  - C3's full mesh at 1920 x 1080: pyr_render_motion_device (previous camera turned a little, a snapshot kept) and, turn by turn
    beside it, pyr_render_features_device with grid 1 and the records alone -- the same rays through the same traversal;
  - pyr_image_reproject_device at 1920 x 1080 on the records of that pass and a full history, with the bytes it has to move;
  - 16 frames of the Cornell box with one box sliding, 8 samples a pixel each: every frame denoised from its half films
    (Session.denoised) and then accumulated along its motion records; the RMSE of the last frame against 4096 samples a pixel of
    that pose with and without the accumulation, and what a frame's pass and reprojection cost next to its render and denoising
    (host entries, wall clock: uploads and downloads included on both sides)."""
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
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def report(what, times, pixels, extra=""):
    t = sorted(times)
    print("%-58s median %8.3f ms  (min %8.3f max %8.3f, %d runs)  %8.1f Mpixels/s%s" % (what, statistics.median(t), t[0], t[-1], len(t), pixels / statistics.median(t) / 1e3, extra),
          flush=True)
    return statistics.median(t)


def moved_camera(cam, dx):
    """`cam` moved by dx along its own x axis."""
    c = abi.PyrCamera.from_buffer_copy(cam.c)
    m = np.array(c.cam_to_world[:], dtype=np.float32).reshape(4, 4).T.copy()
    m[:3, 3] += m[:3, 0] * np.float32(dx)
    c.cam_to_world = (C.c_float * 16)(*[float(v) for v in m.T.reshape(-1)])
    return Camera(c)


# ------------------------------------------------------------------------------------------------ the pass beside the feature pass
W, H = 1920, 1080
world, cam, r, host_film = scenes.build(scenes.c3_mesh_in_box(W, H, 1), seed=1)
del host_film
desc = abi.PyrFilmDesc(W, H, r.spectrum_bins, r.spectrum_span[0], r.spectrum_span[1] - r.spectrum_span[0])
scene = world.scene(0)
world.keep_previous()
previous = moved_camera(cam, 0.05)
motion_records = torch.zeros((H, W, 8), dtype=torch.int32, device=dev)
feature_records = torch.zeros((H, W, 8), dtype=torch.int32, device=dev)
fp = abi.PyrFeatureParams(1, 0)
runs = {
    "motion": lambda: check(lib().pyr_render_motion_device(scene, C.byref(cam.c), C.byref(previous.c), C.byref(desc), C.c_void_p(motion_records.data_ptr()), C.c_void_p(stream.cuda_stream))),
    "features grid 1, records only": lambda: check(lib().pyr_render_features_device(scene, C.byref(cam.c), C.byref(desc), C.byref(fp), None, C.c_void_p(feature_records.data_ptr()),
                                                                                     C.c_void_p(stream.cuda_stream))),
}
times = {name: [] for name in runs}
for turn in range(REPEATS + 1):  # the first turn warms up; the two alternate
    for name, run in runs.items():
        ms = timed(run)
        if turn:
            times[name].append(ms)
for name in runs:
    report("C3 %dx%d %s" % (W, H, name), times[name], W * H)
same = torch.equal(motion_records[..., 4], feature_records[..., 5]) and torch.equal(motion_records[..., 3], feature_records[..., 3])
print("shape and depth of the two passes are the same bits: %s" % bool(same), flush=True)

# ------------------------------------------------------------------------------------------------ the reprojection
pixels = W * H
current = torch.rand((H, W, 3), dtype=torch.float32, device=dev)
history = torch.rand((H, W, 3), dtype=torch.float32, device=dev)
count = torch.full((H, W), 4.0, dtype=torch.float32, device=dev)
out, count_out = torch.zeros_like(current), torch.zeros_like(count)
static_records = torch.zeros_like(motion_records)
check(lib().pyr_render_motion_device(scene, C.byref(cam.c), C.byref(cam.c), C.byref(desc), C.c_void_p(static_records.data_ptr()), C.c_void_p(stream.cuda_stream)))
torch.cuda.synchronize(dev)
p = abi.PyrReprojectParams(abi.PYR_REPROJECT_DEPTH_TOLERANCE, abi.PYR_REPROJECT_MAX_HISTORY)
times = []
for turn in range(REPEATS + 1):
    ms = timed(lambda: check(lib().pyr_image_reproject_device(C.c_void_p(current.data_ptr()), C.c_void_p(motion_records.data_ptr()), C.c_void_p(history.data_ptr()),
                                                              C.c_void_p(static_records.data_ptr()), C.c_void_p(count.data_ptr()), W, H, C.byref(p), C.c_void_p(out.data_ptr()),
                                                              C.c_void_p(count_out.data_ptr()), 0, C.c_void_p(stream.cuda_stream))))
    if turn:
        times.append(ms)
# every input read once and every output written once: 12 + 32 (this frame) + 12 + 32 + 4 (the history) + 12 + 4 (written) bytes a pixel
moved = pixels * (12 + 32 + 12 + 32 + 4 + 12 + 4)
median = report("reproject %dx%d, full history" % (W, H), times, pixels)
print("  bytes that must move: %.1f MB -> %.0f GB/s at the median; %.1f %% of the pixels found history" % (moved / 1e6, moved / median / 1e6, 100.0 * float((count_out > 1).float().mean())),
      flush=True)
world.close()
del motion_records, feature_records, static_records, current, history, out

# ------------------------------------------------------------------------------------------------ sixteen frames of a sliding box
SIZE, FRAMES, SPP, REFERENCE_SPP = (256, 256), 16, 8, 4096
world, cam, r, host_film = scenes.build(scenes.c2_cornell(SIZE[0], SIZE[1], SPP), seed=3)
del host_film
world.set_objects([dict(first_triangle=0, num_triangles=12, first_sphere=0, num_spheres=0), dict(first_triangle=12, num_triangles=12, first_sphere=0, num_spheres=0)])  # the tall box, the short box
world.scene(0)


def pose_of(frame):
    m = np.eye(4, dtype=np.float32)
    m[0, 3] = 0.05 * frame  # the tall box slides along x, about two pixels a frame
    return {0: (m, 1.0)}


def frame_image(spp, seed, halves):
    r.pixel_samples, r.seed = spp, seed
    with r.session(SIZE, cam, world, halves=halves) as s:
        for _ in range(2):
            s.render(spp // 2)
        image = s.denoised()[0] if halves else s.linear()
    return image


accumulated = None
render_ms, temporal_ms = [], []
for frame in range(FRAMES):
    world.pose(pose_of(frame))
    t0 = time.perf_counter()
    image = frame_image(SPP, 100 + frame, True)
    t1 = time.perf_counter()
    records = r.motion(SIZE, cam, world)
    if accumulated is None:
        accumulated = develop.reproject(image, records) + (records,)
    else:
        accumulated = develop.reproject(image, records, accumulated[0], accumulated[2], accumulated[1]) + (records,)
    t2 = time.perf_counter()
    world.keep_previous()
    if frame:  # the first frame pays for allocations on both sides
        render_ms.append(1e3 * (t1 - t0)), temporal_ms.append(1e3 * (t2 - t1))
reference = frame_image(REFERENCE_SPP, 7, False)


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


print("c2 %dx%d, %d frames of %d samples a pixel, one box sliding 0.05 a frame; against %d samples a pixel of the last pose:" % (SIZE + (FRAMES, SPP, REFERENCE_SPP)), flush=True)
print("  RMSE of the last frame denoised alone %.5f, accumulated %.5f (mean history %.2f frames, %.1f %% of the pixels at 1)" % (
    rmse(image, reference), rmse(accumulated[0], reference), float(accumulated[1].mean()), 100.0 * float((accumulated[1] == 1).mean())), flush=True)
# the lamp's pixels are two orders of magnitude above the rest and carry the whole-image figure: the surfaces by themselves, and the raw frame
raw = frame_image(SPP, 100 + FRAMES - 1, False)
surfaces = (reference < 1.0).all(axis=-1)
print("  over the %.1f %% of the pixels below 1.0 in the reference: denoised alone %.5f, accumulated %.5f; the frame not denoised %.5f there, %.5f over all" % (
    100.0 * float(surfaces.mean()), rmse(image[surfaces], reference[surfaces]), rmse(accumulated[0][surfaces], reference[surfaces]), rmse(raw[surfaces], reference[surfaces]),
    rmse(raw, reference)), flush=True)
print("  per frame, host entries, median of %d: render + denoise %.2f ms, motion pass + reprojection %.2f ms" % (len(render_ms), statistics.median(render_ms), statistics.median(temporal_ms)),
      flush=True)
world.close()
