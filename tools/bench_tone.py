#!/usr/bin/env python3
"""Developer tool (GPU box): what the linear image and its tone mapping cost on a C3-sized film (1920 x 1080 x 64 bins).

    python tools/bench_tone.py [spp] [mesh segments]

One process, HIP events, one warm-up and seven repetitions each, on a film that holds a real render of C3 (`spp` samples per
pixel, default 8; a smaller torus-knot mesh than the contract's 640 builds faster and leaves the film's size as it is):
  1. develop_linear_kernel (kernels/tone.hip) against develop_wave_kernel (kernels/film.hip) at step 2, alternating: the same walk
     with 9 more bytes written per pixel; GB/s = film bytes / time.
  2. image_stats_kernel and tonemap_kernel (clip and Reinhard): ms, and GB/s of the 24.9 MB linear image.
  3. a step-30 pyr_session_preview_tone (Reinhard, everything automatic) against pyr_session_preview: wall time of the blocking
     calls, image download included."""
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
from pyrite_amd.develop import develop_params, tone_params  # noqa: E402

spp = int(sys.argv[1]) if len(sys.argv) > 1 else 8
mesh = int(sys.argv[2]) if len(sys.argv) > 2 else 640
W, H = 1920, 1080
REPEATS = 7
world, cam, r, host_film = scenes.build(scenes.c3_mesh_in_box(W, H, spp, segments=mesh, sides=mesh), seed=1)
del host_film.grains
world.scene(0)
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)
film = torch.zeros((H, W, r.spectrum_bins, 2), dtype=torch.float32, device=dev)
desc = abi.PyrFilmDesc(W, H, r.spectrum_bins, r.spectrum_span[0], r.spectrum_span[1] - r.spectrum_span[0])
film_bytes, image_bytes = film.numel() * 4, W * H * 3 * 4
print("C3 %d x %d x %d bins, mesh %d x %d, %d samples per pixel; film %.1f MB, linear image %.1f MB" % (W, H, r.spectrum_bins, mesh, mesh, spp, film_bytes / 1e6, image_bytes / 1e6), flush=True)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def report(name, times, nbytes):
    t = sorted(times)
    print("%-34s median %7.3f ms  (min %7.3f max %7.3f, %d runs)  %7.1f GB/s" % (name, statistics.median(t), t[0], t[-1], len(t), nbytes / statistics.median(t) / 1e6), flush=True)
    return statistics.median(t), t[-1] - t[0]


params = r.params()
check(lib().pyr_render_simple_device(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(params), C.c_void_p(film.data_ptr()), C.c_void_p(stream.cuda_stream)))
torch.cuda.synchronize(dev)

# ---- 1. linear development against the 8-bit wave kernel -----------------------------------------------------------------------
os.environ["PYRITE_DEVELOP_KERNEL"] = "wave"
rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
linear = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
p, keep = develop_params(host_film, 2.0)
calls = {
    "develop_wave_kernel (8 bit)": lambda: check(lib().pyr_film_develop_device(C.byref(desc), C.c_void_p(film.data_ptr()), C.byref(p), C.c_void_p(rgb.data_ptr()), 0, C.c_void_p(stream.cuda_stream))),
    "develop_linear_kernel (sRGB)": lambda: check(lib().pyr_film_develop_linear_device(C.byref(desc), C.c_void_p(film.data_ptr()), None, C.byref(p), abi.PYR_LINEAR_SRGB,
                                                                                      C.c_void_p(linear.data_ptr()), 0, C.c_void_p(stream.cuda_stream))),
}
times = {name: [] for name in calls}
for turn in range(REPEATS + 1):
    for name, call in calls.items():
        ms = timed(call)
        if turn:  # the first turn warms up
            times[name].append(ms)
results = {name: report("step 2  " + name, times[name], film_bytes) for name in calls}
(wave, wave_spread), (lin, lin_spread) = results["develop_wave_kernel (8 bit)"], results["develop_linear_kernel (sRGB)"]
print("linear / 8 bit = %.3f; the run's own spread (max - min): %.3f ms and %.3f ms" % (lin / wave, wave_spread, lin_spread), flush=True)
os.environ.pop("PYRITE_DEVELOP_KERNEL", None)

# ---- 2. statistics and tone mapping of the linear image ----------------------------------------------------------------------------
stats = torch.zeros(C.sizeof(abi.PyrImageStats) // 4, dtype=torch.int32, device=dev)
times = []
for turn in range(REPEATS + 1):
    ms = timed(lambda: check(lib().pyr_image_stats_device(C.c_void_p(linear.data_ptr()), W, H, C.c_void_p(stats.data_ptr()), 0, C.c_void_p(stream.cuda_stream))))
    if turn:
        times.append(ms)
report("image_stats_kernel (+ memset, finish)", times, image_bytes)
host_stats = abi.PyrImageStats.from_buffer_copy(stats.cpu().numpy().tobytes())
print("  lit %d, dark %d, luminance %.4g .. %.4g" % (host_stats.lit, host_stats.dark, host_stats.min_lit, host_stats.max_lit), flush=True)
for name, tone in (("tonemap_kernel clip, exposure 1", abi.PyrToneParams(abi.PYR_TONE_CLIP, 1.0, 1.0, 0.18, 0.5, 0.99)), ("tonemap_kernel reinhard", abi.PyrToneParams(abi.PYR_TONE_REINHARD, 1.0, 4.0, 0.18, 0.5, 0.99))):
    times = []
    for turn in range(REPEATS + 1):
        ms = timed(lambda: check(lib().pyr_image_tonemap_device(C.c_void_p(linear.data_ptr()), W, H, C.byref(tone), C.c_void_p(rgb.data_ptr()), 0, C.c_void_p(stream.cuda_stream))))
        if turn:
            times.append(ms)
    report(name, times, image_bytes + W * H * 3)
del rgb, linear, film

# ---- 3. a session's previews ---------------------------------------------------------------------------------------------------------
with r.session((W, H), cam, world) as s:
    s.render(min(spp, 4))
    s.sync()
    tone = tone_params("reinhard")
    previews = {"pyr_session_preview": lambda: s.preview(30.0), "pyr_session_preview_tone": lambda: s.preview(30.0, tone=tone)}
    times = {name: [] for name in previews}
    for turn in range(REPEATS + 1):
        for name, call in previews.items():
            t = time.perf_counter()
            call()
            if turn:
                times[name].append((time.perf_counter() - t) * 1e3)
    for name in previews:
        t = sorted(times[name])
        print("step 30 %-26s wall median %7.3f ms  (min %7.3f max %7.3f, %d runs)" % (name, statistics.median(t), t[0], t[-1], len(t)), flush=True)
del keep
