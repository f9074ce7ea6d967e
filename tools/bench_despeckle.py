#!/usr/bin/env python3
"""Developer tool (GPU box): what the firefly clamp costs and what it clamps on a real render.

    python tools/bench_despeckle.py [spp]

One process, HIP events, one warm-up and seven repetitions each. The two halves are developed from a real render of C5 (the
dispersive diamonds, `spp` samples per pixel in all, default 8: the sample windows [0, spp/2) and [spp/2, spp) into two films) at
1920 x 1080. Timed: pyr_image_despeckle_device at radius 1 and at radius 2, with both halves and with one, each against the floor of
the bytes the rule must move -- every given half read once, every output written once -- at the 3.0 TB/s reproject_kernel reached
(DESIGN.md section 9k), and one pyr_film_develop_linear_device of a half beside them as a scale. Then the counts and the share of
pixels clamped at k = 4, 6 and 8 at both radii."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pyrite_amd import abi, scenes  # noqa: E402
from pyrite_amd._lib import check, lib  # noqa: E402
from pyrite_amd.develop import despeckle_params, develop_params  # noqa: E402

spp = int(sys.argv[1]) if len(sys.argv) > 1 else 8
assert spp >= 2 and spp % 2 == 0, "two equal halves need an even number of samples"
W, H = 1920, 1080
REPEATS = 7
FLOOR_RATE = 3.0e12  # bytes a second: what reproject_kernel reached
world, cam, r, host_film = scenes.build(scenes.diamonds_example(W, H, spp // 2), seed=1)
del host_film.grains
world.scene(0)
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)
sp = C.c_void_p(stream.cuda_stream)
desc = abi.PyrFilmDesc(W, H, r.spectrum_bins, r.spectrum_span[0], r.spectrum_span[1] - r.spectrum_span[0])
print("C5 (diamonds) %d x %d, two halves of %d samples per pixel; linear image %.1f MB" % (W, H, spp // 2, W * H * 12 / 1e6), flush=True)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def measure(name, fn, moved=None):
    timed(fn)  # warm-up
    times = sorted(timed(fn) for _ in range(REPEATS))
    median = statistics.median(times)
    line = "%-44s median %9.3f ms  (min %9.3f max %9.3f, %d runs)" % (name, median, times[0], times[-1], len(times))
    if moved:
        floor_ms = moved / FLOOR_RATE * 1e3
        line += "  %5.1f MB to move: floor %.3f ms at 3.0 TB/s, %.1f x the floor" % (moved / 1e6, floor_ms, median / floor_ms)
    print(line, flush=True)


# ---- the inputs: two half films and their linear images ---------------------------------------------------------------------------
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
weights = torch.tensor([0.2126, 0.7152, 0.0722], dtype=torch.float32, device=dev)
for name, half in zip("ab", halves):
    y = (half * weights).sum(dim=-1).flatten()
    y = y[torch.isfinite(y)]
    print("half %s: luminance median %.4f, 99.9th percentile %.3f, largest %.2f; %d pixels not finite" % (
        name, float(y.median()), float(torch.quantile(y[:: max(1, y.numel() // 1000000)], 0.999)), float(y.max()), W * H - y.numel()), flush=True)

# ---- the clamp -------------------------------------------------------------------------------------------------------------------
a_out, b_out, removed = (torch.zeros((H, W, 3), dtype=torch.float32, device=dev) for _ in range(3))
counts = torch.zeros(2, dtype=torch.int32, device=dev)


def despeckle(radius, k, both):
    dp = despeckle_params(radius=radius, k=k)
    return lambda: check(lib().pyr_image_despeckle_device(ptr(halves[0]), ptr(halves[1]) if both else None, W, H, C.byref(dp), ptr(a_out), ptr(b_out) if both else None,
                                                          ptr(removed), ptr(counts), 0, sp))


for radius in (1, 2):
    for both in (True, False):
        moved = W * H * 12 * ((4 if both else 2) + 1)  # the halves read, their outputs and removed_out written
        measure("despeckle radius %d, %s" % (radius, "both halves" if both else "one image"), despeckle(radius, abi.PYR_DESPECKLE_K, both), moved)
print("| radius | k | clamped in a | clamped in b | share of the pixels of both halves | clamped in a alone |", flush=True)
print("|---|---|---|---|---|---|", flush=True)
for radius in (1, 2):
    for k in (4.0, 6.0, 8.0):
        despeckle(radius, k, True)()
        torch.cuda.synchronize(dev)
        with_b = [int(c) for c in counts.cpu().numpy()]
        despeckle(radius, k, False)()
        torch.cuda.synchronize(dev)
        alone = int(counts.cpu().numpy()[0])
        print("| %d | %g | %d | %d | %.4f %% | %d (%.4f %%) |" % (radius, k, with_b[0], with_b[1], 100.0 * sum(with_b) / (2 * W * H), alone, 100.0 * alone / (W * H)), flush=True)
despeckle(2, abi.PYR_DESPECKLE_K, True)()
torch.cuda.synchronize(dev)
mean_before = 0.5 * (halves[0] + halves[1])
lost = removed.sum(dim=(0, 1)) / mean_before.nan_to_num(0.0, 0.0, 0.0).sum(dim=(0, 1))
print("defaults: the mean of the halves lost %.3f %% / %.3f %% / %.3f %% of its R / G / B" % tuple(100.0 * float(v) for v in lost), flush=True)
del keep
world.close()
