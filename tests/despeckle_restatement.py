"""The despeckle rule of include/pyrite_gpu.h ("despeckle") restated in numpy, operation by operation in f32:
what tests/test_gpu_despeckle.py holds kernels/despeckle.hip against bit for bit, and what tests/test_despeckle_cpu.py checks the
properties of the rule on. Nothing here is shared with the library: the medians come from numpy's sort."""
import numpy as np

f32 = np.float32
MOST_RADIUS, LEAST_SAMPLES = 2, 5
RADIUS, K, RELATIVE, FLOOR = 2, 6.0, 0.1, 1e-4


def luminance(image):
    """Y = ((0.2126f*R + 0.7152f*G) + 0.0722f*B) + 0.0f, one rounding per operation."""
    image = np.asarray(image, dtype=f32)
    with np.errstate(all="ignore"):
        y = (f32(0.2126) * image[..., 0] + f32(0.7152) * image[..., 1]).astype(f32)
        y = (y + f32(0.0722) * image[..., 2]).astype(f32)
        return (y + f32(0.0)).astype(f32)


def limits(halves, radius, k, relative, floor):
    """(limit, n) per pixel: the median of the finite luminances of the window in every given half, the centre left out, plus k
    spreads; n counts the sample set."""
    h, w = halves[0].shape
    ys = []
    for y in halves:
        padded = np.full((h + 2 * radius, w + 2 * radius), np.inf, dtype=f32)
        padded[radius:radius + h, radius:radius + w] = np.where(np.isfinite(y), y, f32(np.inf))  # what is not finite is no sample
        for oy in range(2 * radius + 1):
            for ox in range(2 * radius + 1):
                if (ox, oy) != (radius, radius):
                    ys.append(padded[oy:oy + h, ox:ox + w])
    ys = np.sort(np.stack(ys), axis=0)  # ascending, the empty slots (+inf) last
    n = np.isfinite(ys).sum(axis=0)
    rank = (np.maximum(n, 1) - 1) // 2
    with np.errstate(all="ignore"):
        m = np.take_along_axis(ys, rank[None], axis=0)[0]
        deviations = np.sort(np.abs((ys - m[None]).astype(f32)), axis=0)  # inf - m stays inf; with n == 0 a NaN, which nothing reads
        s = np.take_along_axis(deviations, rank[None], axis=0)[0]
        spread = np.maximum(np.maximum((s * f32(1.4826)).astype(f32), (f32(relative) * m).astype(f32)), f32(floor))
        limit = (m + (f32(k) * spread).astype(f32)).astype(f32)
    return limit, n


def despeckle(a, b=None, radius=RADIUS, k=K, relative=RELATIVE, floor=FLOOR):
    """(a_out, b_out or None, removed, counts): counts is a pair of ints, the pixels clamped in a and in b."""
    assert 1 <= radius <= MOST_RADIUS
    images = [np.ascontiguousarray(a, dtype=f32)] + ([np.ascontiguousarray(b, dtype=f32)] if b is not None else [])
    ys = [luminance(image) for image in images]
    limit, n = limits(ys, radius, k, relative, floor)
    with np.errstate(all="ignore"):
        above = [np.isfinite(y) & (y > limit) for y in ys]
        outs, lost, counts = [], [], [0, 0]
        for which, (image, y) in enumerate(zip(images, ys)):
            firefly = (n >= LEAST_SAMPLES) & above[which]
            if len(images) == 2:
                firefly &= ~above[1 - which]
            g = (limit / y).astype(f32)
            out = np.where(firefly[..., None], (image * g[..., None]).astype(f32), image)
            lost.append(np.where(firefly[..., None], (image - out).astype(f32), f32(0)))  # d_H: 0.0f where H was not clamped
            outs.append(out)
            counts[which] = int(firefly.sum())
        removed = ((lost[0] + lost[1]).astype(f32) * f32(0.5)).astype(f32) if len(images) == 2 else lost[0]
    return outs[0], (outs[1] if len(outs) == 2 else None), removed, tuple(counts)
