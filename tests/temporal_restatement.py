"""include/pyrite_gpu.h "temporal resolve" restated in numpy float32, one rounding per operation in the order the header writes.
Nothing here calls the library and nothing is taken from another restatement: the history fetch is written out again from the
header's "accumulation over frames" -- here over whole arrays, a tap at a time, where motion_restatement.reproject goes pixel by
pixel -- so that tests/test_temporal_cpu.py can hold the two against each other as two statements of one rule.
tests/test_gpu_temporal.py compares the kernels with this file bit for bit.
  Every array operation below is one f32 operation per element, and a sum "over the kept pixels in raster order" is a walk over
the (dy, dx) offsets in that order which adds where the neighbour is kept and leaves the sum alone where it is not."""
import numpy as np

f32 = np.float32
MOTION_HIT, MOTION_IN_FRONT, MOTION_INSIDE = 1, 2, 4
RECORD = np.dtype([("prev_x", "<f4"), ("prev_y", "<f4"), ("prev_depth", "<f4"), ("depth", "<f4"), ("shape", "<u4"), ("flags", "<u4"), ("reserved", "<u4", (2,))])
HALF, ONE, ZERO = f32(0.5), f32(1), f32(0)
TINY, HUGE = f32(1e-30), f32(1e30)


def usable_pixels(current, noise=None):
    """bool [h, w]: step 1."""
    ok = np.isfinite(current).all(axis=-1)
    if noise is not None:
        ok &= np.isfinite(noise).all(axis=-1)
    return ok


@np.errstate(all="ignore")
def fetch(motion, history, history_motion, history_count, depth_tolerance):
    """(Wt [h, w], Hc [h, w, 3], N [h, w]): step 3's sums over the counting taps, in tap order from 0.0f. Wt is 0 where the rule says
    "no history" before a tap is read."""
    height, width = motion.shape
    fw, fh, tol = f32(width), f32(height), f32(depth_tolerance)
    flags = motion["flags"]
    start = ((flags & MOTION_IN_FRONT) != 0) & np.isfinite(motion["prev_x"]) & np.isfinite(motion["prev_y"])
    gx, gy = motion["prev_x"] - HALF, motion["prev_y"] - HALF
    x0, y0 = np.floor(gx), np.floor(gy)
    fx, fy = gx - x0, gy - y0
    x1, y1 = x0 + ONE, y0 + ONE
    taps = [(x0, y0, (ONE - fx) * (ONE - fy)), (x1, y0, fx * (ONE - fy)), (x0, y1, (ONE - fx) * fy), (x1, y1, fx * fy)]
    Wt, Hc, N = np.zeros((height, width), dtype=f32), np.zeros((height, width, 3), dtype=f32), np.zeros((height, width), dtype=f32)
    for tx, ty, w in taps:
        counts = start & (tx >= ZERO) & (tx < fw) & (ty >= ZERO) & (ty < fh)  # decided on the floats, before any cast
        ix, iy = np.where(counts, tx, ZERO).astype(np.int64), np.where(counts, ty, ZERO).astype(np.int64)
        counts &= (ix < width) & (iy < height)
        ix, iy = np.minimum(ix, width - 1), np.minimum(iy, height - 1)
        theirs, colour, frames = history_motion[iy, ix], history[iy, ix], history_count[iy, ix]
        counts &= theirs["shape"] == motion["shape"]
        near = np.abs(theirs["depth"] - motion["prev_depth"]) <= tol * np.fmax(theirs["depth"], motion["prev_depth"])
        counts &= near | ((flags & MOTION_HIT) == 0)
        counts &= frames > ZERO
        counts &= np.isfinite(colour).all(axis=-1)
        Wt = np.where(counts, Wt + w, Wt)
        Hc = np.where(counts[..., None], Hc + w[..., None] * colour, Hc)
        N = np.where(counts, N + w * frames, N)
    return Wt, Hc, N


def neighbours(image, usable, radius):
    """The kept neighbours of every pixel in raster order, dy outer, dx inner: pairs (values [h, w, ...], kept [h, w])."""
    height, width = usable.shape
    padded = np.zeros((height + 2 * radius, width + 2 * radius) + image.shape[2:], dtype=image.dtype)
    padded[radius:radius + height, radius:radius + width] = image
    flag = np.zeros((height + 2 * radius, width + 2 * radius), dtype=bool)
    flag[radius:radius + height, radius:radius + width] = usable
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            yield padded[dy:dy + height, dx:dx + width], flag[dy:dy + height, dx:dx + width]


@np.errstate(all="ignore")
def moments(current, noise, usable, radius):
    """(mean, sigma, nbar, k): step 2 for every pixel; what it gives a pixel that is not usable is never read."""
    height, width = usable.shape
    k, total = np.zeros((height, width), dtype=f32), np.zeros((height, width, 3), dtype=f32)
    for value, kept in neighbours(current, usable, radius):
        total = np.where(kept[..., None], total + value, total)
        k = np.where(kept, k + ONE, k)
    mean = total / k[..., None]
    squares = np.zeros((height, width, 3), dtype=f32)
    for value, kept in neighbours(current, usable, radius):
        d = value - mean
        squares = np.where(kept[..., None], squares + d * d, squares)
    sigma = np.sqrt(squares / k[..., None])
    nbar = np.zeros((height, width, 3), dtype=f32)
    if noise is not None:
        total = np.zeros((height, width, 3), dtype=f32)
        for value, kept in neighbours(np.abs(noise), usable, radius):
            total = np.where(kept[..., None], total + value, total)
        nbar = total / k[..., None]
    return mean, sigma, nbar, k


def resolve(current, motion, history=None, history_motion=None, history_count=None, noise=None, depth_tolerance=0.02, max_history=32.0, radius=1, gamma=1.0,
            noise_scale=1.0, response=1.0):
    """(out [h, w, 3], count [h, w], clip [h, w]) of pyr_image_temporal_resolve."""
    current = np.asarray(current, dtype=f32)
    height, width, _ = current.shape
    out, count, clip = current.copy(), np.ones((height, width), dtype=f32), np.zeros((height, width), dtype=f32)
    if history is None:
        return out, count, clip
    history, history_count = np.asarray(history, dtype=f32), np.asarray(history_count, dtype=f32)
    noise = None if noise is None else np.asarray(noise, dtype=f32)
    with np.errstate(all="ignore"):
        usable = usable_pixels(current, noise)
        Wt, Hc, N = fetch(motion, history, history_motion, history_count, depth_tolerance)
        blended = usable & (Wt > ZERO)
        mean, sigma, nbar, _ = moments(current, noise, usable, radius)
        H = Hc / Wt[..., None]
        n = np.fmin(N / Wt, f32(max_history))
        e = f32(gamma) * sigma + f32(noise_scale) * nbar
        lo, hi = mean - e, mean + e
        clipped = np.fmin(np.fmax(H, lo), hi)
        q = np.abs(H - clipped) / np.fmax(e, TINY)
        r = np.fmin(np.fmax(np.fmax(q[..., 0], q[..., 1]), q[..., 2]), HUGE)
        n2 = n / (ONE + f32(response) * r)
        result = clipped + (current - clipped) / (n2 + ONE)[..., None]
    assert all(a.dtype == f32 for a in (Wt, Hc, N, mean, sigma, nbar, H, n, e, clipped, q, r, n2, result))  # nothing was promoted on the way
    out[blended], count[blended], clip[blended] = result[blended], (n2 + ONE)[blended], r[blended]
    return out, count, clip
