#!/usr/bin/env python3
"""Developer tool (GPU box): what a progressive session costs on C3 at its contract size (1920 x 1080 x 64 bins).

    python tools/bench_session.py [spp] [parent-library.so]

  1. develop: develop_wave_kernel (kernels/film.hip) against develop_kernel (kernels/main.hip) on a film that holds a real render,
     at steps 30 and 2, alternating, HIP events around pyr_film_develop_device; GB/s = film bytes / time.
  2. passes: the render one-shot (pyr_render_simple_device) and as a session in passes of 256, 64, 16 and 4 samples per pixel, wall
     time from the first enqueue to the end of pyr_session_sync, Msamples/s; two rounds.
  3. with a second argument, a build of the parent commit's library: plain pyr_render_simple_device on both, alternating."""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pyrite_amd import abi, scenes  # noqa: E402
from pyrite_amd._lib import check, lib  # noqa: E402
from pyrite_amd.develop import develop_params  # noqa: E402

spp = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
parent_path = sys.argv[2] if len(sys.argv) > 2 else None
W, H = 1920, 1080
world, cam, r, host_film = scenes.build(scenes.c3_mesh_in_box(W, H, spp), seed=1)
del host_film.grains
world.scene(0)
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)
film = torch.zeros((H, W, r.spectrum_bins, 2), dtype=torch.float32, device=dev)
desc = abi.PyrFilmDesc(W, H, r.spectrum_bins, r.spectrum_span[0], r.spectrum_span[1] - r.spectrum_span[0])
film_bytes = film.numel() * 4


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def plain_render(library, samples):
    params = r.params()
    params.pixel_samples = samples
    check(library.pyr_render_simple_device(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(params), C.c_void_p(film.data_ptr()), C.c_void_p(stream.cuda_stream)))


# ---- 1. develop -------------------------------------------------------------------------------------------------------------
timed(lambda: plain_render(lib(), 8))  # a real film: 8 samples per pixel
rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
images = {}
for step in (30.0, 2.0):
    p, keep = develop_params(host_film, step)
    times = {"pixel": [], "wave": []}
    for turn in range(7):
        for kernel in ("pixel", "wave"):
            os.environ["PYRITE_DEVELOP_KERNEL"] = kernel
            ms = timed(lambda: check(lib().pyr_film_develop_device(C.byref(desc), C.c_void_p(film.data_ptr()), C.byref(p), C.c_void_p(rgb.data_ptr()), 0,
                                                                   C.c_void_p(stream.cuda_stream))))
            if turn:  # the first turn warms up
                times[kernel].append(ms)
            images[(step, kernel)] = rgb.clone()
    for kernel in ("pixel", "wave"):
        t = sorted(times[kernel])
        print("develop step %4.0f %-5s  median %7.3f ms  (min %7.3f max %7.3f, %d runs)  %7.1f GB/s" % (step, kernel, statistics.median(t), t[0], t[-1], len(t),
                                                                                                      film_bytes / statistics.median(t) / 1e6), flush=True)
    print("develop step %4.0f: the two kernels wrote the same bytes: %s" % (step, bool(torch.equal(images[(step, "pixel")], images[(step, "wave")]))), flush=True)
os.environ.pop("PYRITE_DEVELOP_KERNEL", None)
del rgb, images

# ---- 2. passes --------------------------------------------------------------------------------------------------------------
r.pixel_samples = spp
for round_ in (1, 2):
    film.zero_()
    ms = timed(lambda: plain_render(lib(), spp))
    print("round %d  one shot              %9.1f ms  %7.1f Msamples/s" % (round_, ms, W * H * spp / ms / 1e3), flush=True)
    for per_pass in (256, 64, 16, 4):
        if per_pass > spp:
            continue
        with r.session((W, H), cam, world) as s:
            t = time.perf_counter()
            while s.samples_done < spp:
                s.render(per_pass)
            s.sync()
            ms = (time.perf_counter() - t) * 1e3
        print("round %d  passes of %4d (%4d)  %9.1f ms  %7.1f Msamples/s" % (round_, per_pass, -(-spp // per_pass), ms, W * H * spp / ms / 1e3), flush=True)

# ---- 3. plain render against the parent commit's library ----------------------------------------------------------------------
if parent_path:
    parent = C.CDLL(parent_path)
    for name in ("pyr_scene_create", "pyr_scene_destroy", "pyr_render_simple_device", "pyr_last_error"):
        getattr(parent, name).restype, getattr(parent, name).argtypes = abi.ENTRY_POINTS[name]
    handle = C.c_void_p()
    assert parent.pyr_scene_create(C.byref(world.desc), 0, C.byref(handle)) == 0, parent.pyr_last_error()
    ab_spp = min(spp, 256)

    def parent_render():
        params = r.params()  # the parent reads the first 56 bytes: everything but sample_begin
        params.pixel_samples = ab_spp
        assert parent.pyr_render_simple_device(handle, C.byref(cam.c), C.byref(desc), C.byref(params), C.c_void_p(film.data_ptr()), C.c_void_p(stream.cuda_stream)) == 0

    runs = {"parent": [], "this": []}
    for turn in range(5):
        for which in ("parent", "this"):
            film.zero_()
            ms = timed(parent_render if which == "parent" else (lambda: plain_render(lib(), ab_spp)))
            if turn:
                runs[which].append(W * H * ab_spp / ms / 1e3)
    for which in ("parent", "this"):
        print("plain render at %d spp, %-6s  Msamples/s %s  median %.1f" % (ab_spp, which, " ".join("%.1f" % x for x in runs[which]), statistics.median(runs[which])), flush=True)
    parent.pyr_scene_destroy(handle)
