#!/usr/bin/env python3
"""Developer tool (GPU box): what denoising a 1920 x 1080 linear image costs.

    python tools/bench_denoise.py [spp] [mesh segments]

One process, HIP events, one warm-up and seven repetitions each. The two halves are developed from a real low-sample render of C3
(`spp` samples per pixel in all, default 8: the sample windows [0, spp/2) and [spp/2, spp) into two films; mesh 160 x 160 by
default, which builds fast and leaves the image's size as it is), the guides from the feature pass of the same scene. Timed:
pyr_image_denoise_device -- the variance kernel, the two filter launches, the combine and the stream-ordered working memory -- at
(radius, patch) = (5, 1) and (10, 3), with and without guides, and one pyr_film_develop_linear_device of a half beside them as a scale."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pyrite_amd import abi, scenes  # noqa: E402
from pyrite_amd._lib import check, lib  # noqa: E402
from pyrite_amd.develop import denoise_params, develop_params  # noqa: E402

spp = int(sys.argv[1]) if len(sys.argv) > 1 else 8
mesh = int(sys.argv[2]) if len(sys.argv) > 2 else 160
assert spp >= 2 and spp % 2 == 0, "two equal halves need an even number of samples"
W, H = 1920, 1080
REPEATS = 7
ALBEDO_BINS = 16
world, cam, r, host_film = scenes.build(scenes.c3_mesh_in_box(W, H, spp // 2, segments=mesh, sides=mesh), seed=1)
del host_film.grains
world.scene(0)
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)
sp = C.c_void_p(stream.cuda_stream)
desc = abi.PyrFilmDesc(W, H, r.spectrum_bins, r.spectrum_span[0], r.spectrum_span[1] - r.spectrum_span[0])
print("C3 %d x %d, mesh %d x %d, two halves of %d samples per pixel; linear image %.1f MB" % (W, H, mesh, mesh, spp // 2, W * H * 12 / 1e6), flush=True)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def measure(name, fn):
    timed(fn)  # warm-up
    times = sorted(timed(fn) for _ in range(REPEATS))
    print("%-44s median %9.3f ms  (min %9.3f max %9.3f, %d runs)" % (name, statistics.median(times), times[0], times[-1], len(times)), flush=True)


# ---- the inputs: two half films, their linear images, the guides -----------------------------------------------------------------
p, keep = develop_params(host_film, 2.0)
halves = []
film = torch.zeros((H, W, r.spectrum_bins, 2), dtype=torch.float32, device=dev)
for k in range(2):
    film.zero_()
    params = r.params(sample_begin=k * (spp // 2))
    check(lib().pyr_render_simple_device(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(params), ptr(film), sp))
    linear = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    check(lib().pyr_film_develop_linear_device(C.byref(desc), ptr(film), None, C.byref(p), abi.PYR_LINEAR_SRGB, ptr(linear), 0, sp))
    torch.cuda.synchronize(dev)
    halves.append(linear)
measure("develop_linear_kernel (one half, step 2)",
        lambda: check(lib().pyr_film_develop_linear_device(C.byref(desc), ptr(film), None, C.byref(p), abi.PYR_LINEAR_SRGB, ptr(linear), 0, sp)))
del film
albedo_film = torch.zeros((H, W, ALBEDO_BINS, 2), dtype=torch.float32, device=dev)
records = torch.zeros((H, W, 8), dtype=torch.float32, device=dev)  # PyrFeaturePixel is 32 bytes
fp = abi.PyrFeatureParams(1, ALBEDO_BINS)
check(lib().pyr_render_features_device(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(fp), ptr(albedo_film), ptr(records), sp))
albedo_desc = abi.PyrFilmDesc(W, H, ALBEDO_BINS, desc.wl_start, desc.wl_width)
albedo = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
check(lib().pyr_film_develop_linear_device(C.byref(albedo_desc), ptr(albedo_film), None, C.byref(p), abi.PYR_LINEAR_SRGB, ptr(albedo), 0, sp))
torch.cuda.synchronize(dev)
difference = float(((halves[0] - halves[1]).abs().mean() / (0.5 * (halves[0] + halves[1])).abs().mean()).item())
print("mean |a - b| / mean |(a + b) / 2| of the halves: %.3f" % difference, flush=True)

# ---- the filter ------------------------------------------------------------------------------------------------------------------
out, error = torch.zeros((H, W, 3), dtype=torch.float32, device=dev), torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
for radius, patch in ((5, 1), (10, 3)):
    dp = denoise_params(radius=radius, patch=patch)
    for guides in (False, True):
        measure("denoise radius %2d patch %d %s" % (radius, patch, "albedo, normal, depth" if guides else "no guides"),
                lambda: check(lib().pyr_image_denoise_device(ptr(halves[0]), ptr(halves[1]), ptr(albedo) if guides else None, ptr(records) if guides else None, W, H,
                                                             C.byref(dp), ptr(out), ptr(error), 0, sp)))
    left = float((error.mean() / out.abs().mean()).item())
    print("    mean error_out / mean |out| with guides: %.4f" % left, flush=True)
del keep
