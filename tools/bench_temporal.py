#!/usr/bin/env python3
"""Developer tool (GPU box): what the temporal resolve costs and buys.

    python tools/bench_temporal.py

In one process, HIP events around the enqueue on the current stream, one warm-up and seven timed repetitions per row, median and
spread:
  - pyr_image_temporal_resolve_device at 1920 x 1080 on the records of C3's motion pass (previous camera moved a little, a
    snapshot kept) and a full history, with and without a noise image, radius 1 and 3, turn by turn with
    pyr_image_reproject_device on the same buffers, each with the bytes it has to move;
  - section 9i's sequence -- 16 frames of the Cornell box at 256 x 256 with the tall box sliding, 8 samples a pixel each, every
    frame denoised from its half films (Session.denoised) with its error image -- accumulated once by develop.reproject and once
    by develop.resolve; the RMSE of the last frame against 4,096 samples a pixel of that pose over the pixels the box's shadow
    crossed (static records in every frame, true luminance of the first and the last pose more than 20 % apart) and over the
    rest of the static pixels, each also without the pixels that reach 1.0 in either reference (the lamp, fireflies)."""
import ctypes as C
import os
import statistics
import sys

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


def report(what, times, pixels, moved):
    t = sorted(times)
    median = statistics.median(t)
    print("%-46s median %7.3f ms  (min %7.3f max %7.3f, %d runs)  %7.1f Mpixels/s  %5.1f MB to move -> %5.0f GB/s" % (
        what, median, t[0], t[-1], len(t), pixels / median / 1e3, moved / 1e6, moved / median / 1e6), flush=True)
    return median


def moved_camera(cam, dx):
    """`cam` moved by dx along its own x axis."""
    c = abi.PyrCamera.from_buffer_copy(cam.c)
    m = np.array(c.cam_to_world[:], dtype=np.float32).reshape(4, 4).T.copy()
    m[:3, 3] += m[:3, 0] * np.float32(dx)
    c.cam_to_world = (C.c_float * 16)(*[float(v) for v in m.T.reshape(-1)])
    return Camera(c)


# ------------------------------------------------------------------------------------------------ the kernel beside the reprojection
W, H = 1920, 1080
world, cam, r, host_film = scenes.build(scenes.c3_mesh_in_box(W, H, 1), seed=1)
del host_film
desc = abi.PyrFilmDesc(W, H, r.spectrum_bins, r.spectrum_span[0], r.spectrum_span[1] - r.spectrum_span[0])
scene = world.scene(0)
world.keep_previous()
previous = moved_camera(cam, 0.05)
motion_records = torch.zeros((H, W, 8), dtype=torch.int32, device=dev)
static_records = torch.zeros_like(motion_records)
check(lib().pyr_render_motion_device(scene, C.byref(cam.c), C.byref(previous.c), C.byref(desc), C.c_void_p(motion_records.data_ptr()), C.c_void_p(stream.cuda_stream)))
check(lib().pyr_render_motion_device(scene, C.byref(cam.c), C.byref(cam.c), C.byref(desc), C.c_void_p(static_records.data_ptr()), C.c_void_p(stream.cuda_stream)))
torch.cuda.synchronize(dev)
world.close()

pixels = W * H
current = torch.rand((H, W, 3), dtype=torch.float32, device=dev)
history = (current + 0.3 * (torch.rand((H, W, 3), dtype=torch.float32, device=dev) - 0.5)).contiguous()
noise = 0.05 * torch.rand((H, W, 3), dtype=torch.float32, device=dev)
count = torch.full((H, W), 4.0, dtype=torch.float32, device=dev)
out, count_out, clip_out = torch.zeros_like(current), torch.zeros_like(count), torch.zeros_like(count)
ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
rp = abi.PyrReprojectParams(abi.PYR_REPROJECT_DEPTH_TOLERANCE, abi.PYR_REPROJECT_MAX_HISTORY)


def reproject():
    check(lib().pyr_image_reproject_device(ptr(current), ptr(motion_records), ptr(history), ptr(static_records), ptr(count), W, H, C.byref(rp), ptr(out), ptr(count_out), 0,
                                           C.c_void_p(stream.cuda_stream)))


def resolve(radius, with_noise, with_clip=True):
    p = develop.temporal_params(radius=radius)
    return lambda: check(lib().pyr_image_temporal_resolve_device(ptr(current), ptr(motion_records), ptr(noise if with_noise else None), ptr(history), ptr(static_records),
                                                                 ptr(count), W, H, C.byref(p), ptr(out), ptr(count_out), ptr(clip_out if with_clip else None), 0,
                                                                 C.c_void_p(stream.cuda_stream)))


# every input read once and every output written once: 12 + 32 (this frame) + 12 + 32 + 4 (the history) + 12 + 4 (written) = 108 bytes
# a pixel, 12 more with a noise image, 4 more with clip_out
runs = {"reproject": (reproject, 108)}
for radius in (1, 3):
    runs["resolve radius %d" % radius] = (resolve(radius, False), 108 + 4)
    runs["resolve radius %d, noise image" % radius] = (resolve(radius, True), 108 + 12 + 4)
runs["resolve radius 1, noise image, no clip_out"] = (resolve(1, True, False), 108 + 12)
times = {name: [] for name in runs}
for turn in range(REPEATS + 1):  # the first turn warms up; the rows alternate
    for name, (run, _) in runs.items():
        ms = timed(run)
        if turn:
            times[name].append(ms)
medians = {name: report("%dx%d %s" % (W, H, name), times[name], pixels, pixels * runs[name][1]) for name in runs}
for name in runs:
    if name != "reproject":
        print("  %-44s %.2f x the reprojection" % (name, medians[name] / medians["reproject"]), flush=True)
resolve(1, True)()
torch.cuda.synchronize(dev)
print("  at radius 1 with the noise image %.1f %% of the pixels found history, %.1f %% of those were clipped" % (
    100.0 * float(((count_out > 1) | (clip_out > 0)).float().mean()), 100.0 * float((clip_out > 0).float().sum() / ((count_out > 1) | (clip_out > 0)).float().sum())), flush=True)
del motion_records, static_records, current, history, noise, out

# ------------------------------------------------------------------------------------------------ sixteen frames of a sliding box
SIZE, FRAMES, SPP, REFERENCE_SPP = (256, 256), 16, 8, 4096
world, cam, r, host_film = scenes.build(scenes.c2_cornell(SIZE[0], SIZE[1], SPP), seed=3)
del host_film
world.set_objects([dict(first_triangle=0, num_triangles=12, first_sphere=0, num_spheres=0), dict(first_triangle=12, num_triangles=12, first_sphere=0, num_spheres=0)])  # the tall box, the short box
world.scene(0)


def pose(frame):
    m = np.eye(4, dtype=np.float32)
    m[0, 3] = 0.05 * frame  # the tall box slides along x, about two pixels a frame
    world.pose({0: (m, 1.0)})


def frame_image(spp, seed, halves):
    r.pixel_samples, r.seed = spp, seed
    with r.session(SIZE, cam, world, halves=halves) as s:
        for _ in range(2):
            s.render(spp // 2)
        return s.denoised() if halves else s.linear()


x, y = np.meshgrid(np.arange(SIZE[0], dtype=np.float32) + np.float32(0.5), np.arange(SIZE[1], dtype=np.float32) + np.float32(0.5))
static = np.ones((SIZE[1], SIZE[0]), dtype=bool)
plain = resolved = before = None
for frame in range(FRAMES):
    pose(frame)
    image, error = frame_image(SPP, 100 + frame, True)
    records = r.motion(SIZE, cam, world)
    static &= ((records["flags"] & abi.PYR_MOTION_HIT) != 0) & (np.abs(records["prev_x"] - x) <= 1e-3) & (np.abs(records["prev_y"] - y) <= 1e-3)
    if before is None:
        plain, resolved = develop.reproject(image, records), develop.resolve(image, records, noise=error)
    else:
        static &= records["shape"] == before["shape"]
        plain = develop.reproject(image, records, plain[0], before, plain[1])
        resolved = develop.resolve(image, records, resolved[0], before, resolved[1], noise=error)
    before = records
    world.keep_previous()
truth_last = frame_image(REFERENCE_SPP, 7, False)
pose(0)
truth_first = frame_image(REFERENCE_SPP, 8, False)
world.close()


def luminance(rgb):
    return rgb.astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])


def rmse(a, where):
    return float(np.sqrt(np.mean((a[where].astype(np.float64) - truth_last[where].astype(np.float64)) ** 2)))


first, last = luminance(truth_first), luminance(truth_last)
change = np.abs(first - last) / np.maximum(np.maximum(first, last), 1e-12)
crossed, rest = static & (change > 0.20), static & ~(change > 0.20)
print("c2 %dx%d, %d frames of %d samples a pixel, the tall box sliding 0.05 a frame; against %d samples a pixel of the last pose:" % (SIZE + (FRAMES, SPP, REFERENCE_SPP)), flush=True)
# the lamp's pixels and the fireflies that 4,096 samples still hold are two orders of magnitude above the rest and carry both figures
# (tools/bench_motion.py): each region again over its pixels below 1.0 in both references
surfaces = (truth_last < 1.0).all(axis=-1) & (truth_first < 1.0).all(axis=-1)
for name, where in (("where the shadow crossed", crossed), ("the other static pixels", rest), ("  of those, below 1.0", crossed & surfaces), ("  of those, below 1.0", rest & surfaces)):
    print("  %-26s %6d pixels: RMSE of the last frame denoised alone %.5f, reprojected %.5f, resolved %.5f (%.2f of the reprojection's); mean count %.2f against %.2f" % (
        name, int(where.sum()), rmse(image, where), rmse(plain[0], where), rmse(resolved[0], where), rmse(resolved[0], where) / rmse(plain[0], where),
        float(resolved[1][where].mean()), float(plain[1][where].mean())), flush=True)
print("  history clipped in %.1f %% of the pixels of the last frame" % (100.0 * float((resolved[2] > 0).mean())), flush=True)
