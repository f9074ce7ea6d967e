#!/usr/bin/env python3
"""Developer tool (GPU box): what the first-hit feature pass costs.

    python tools/bench_features.py [row-major-library.so]

On C3 at 1920 x 1080 and on textures_example (interpreter programs, textures, normal maps) at 1024 x 512, in one process, HIP
events around the enqueue on the current stream, one warm-up and seven timed repetitions per row, median and spread:
  - pyr_render_features_device at grid 1 and 2, albedo_bins 16, both outputs, with the 8 x 8-square item order of the library;
  - the same from a build with -DPYR_FEATURES_ROW_MAJOR (python -m pyrite_amd.build --variant features_rows -DPYR_FEATURES_ROW_MAJOR),
    given as the argument: the two libraries alternate, and the bytes they write are compared;
  - beside them one pyr_render_simple_device call of 1 sample per pixel of the same scene, as a scale."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pyrite_amd import abi, scenes  # noqa: E402
from pyrite_amd._lib import check, lib  # noqa: E402

rows_path = sys.argv[1] if len(sys.argv) > 1 else None
REPEATS = 7
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)
libraries = {"squares": lib()}
if rows_path:
    libraries["rows"] = abi.bind(C.CDLL(rows_path))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def report(what, times, pixels):
    t = sorted(times)
    print("%-46s median %8.3f ms  (min %8.3f max %8.3f, %d runs)  %8.1f Mpixels/s" % (what, statistics.median(t), t[0], t[-1], len(t), pixels / statistics.median(t) / 1e3), flush=True)


for name, project, (W, H) in (("C3", scenes.c3_mesh_in_box, (1920, 1080)), ("textures_example", scenes.textures_example, (1024, 512))):
    world, cam, r, host_film = scenes.build(project(W, H, 1), seed=1)
    del host_film
    bins = 16
    desc = abi.PyrFilmDesc(W, H, r.spectrum_bins, r.spectrum_span[0], r.spectrum_span[1] - r.spectrum_span[0])
    handles = {}
    for which, library in libraries.items():
        handles[which] = C.c_void_p()
        assert library.pyr_scene_create(C.byref(world.desc), 0, C.byref(handles[which])) == 0, library.pyr_last_error()
    albedo = torch.zeros((H, W, bins, 2), dtype=torch.float32, device=dev)
    records = torch.zeros((H, W, 8), dtype=torch.int32, device=dev)
    film = torch.zeros((H, W, r.spectrum_bins, 2), dtype=torch.float32, device=dev)
    for grid in (1, 2):
        fp = abi.PyrFeatureParams(grid, bins)
        times, images = {which: [] for which in libraries}, {}
        for turn in range(REPEATS + 1):  # the first turn warms up
            for which, library in libraries.items():
                albedo.zero_()
                ms = timed(lambda: check(library.pyr_render_features_device(handles[which], C.byref(cam.c), C.byref(desc), C.byref(fp), C.c_void_p(albedo.data_ptr()),
                                                                            C.c_void_p(records.data_ptr()), C.c_void_p(stream.cuda_stream))))
                if turn:
                    times[which].append(ms)
                images[which] = (albedo.clone(), records.clone())
        for which in libraries:
            report("%s %dx%d features grid %d bins %d, %s" % (name, W, H, grid, bins, which), times[which], W * H)
        if rows_path:
            print("%s grid %d: both item orders wrote the same bytes: %s" % (name, grid, bool(torch.equal(images["squares"][0], images["rows"][0]) and torch.equal(images["squares"][1], images["rows"][1]))),
                  flush=True)
    params = r.params()
    params.pixel_samples = 1
    times = []
    for turn in range(REPEATS + 1):
        film.zero_()
        ms = timed(lambda: check(lib().pyr_render_simple_device(handles["squares"], C.byref(cam.c), C.byref(desc), C.byref(params), C.c_void_p(film.data_ptr()), C.c_void_p(stream.cuda_stream))))
        if turn:
            times.append(ms)
    report("%s %dx%d render, 1 sample per pixel (scale)" % (name, W, H), times, W * H)
    for which, library in libraries.items():
        library.pyr_scene_destroy(handles[which])
    del albedo, records, film
