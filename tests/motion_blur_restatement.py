"""include/pyrite_gpu.h "motion blur over the motion records" restated in numpy float32, one rounding per operation in the order
the header writes: the half velocity and depth of a pixel, the tile maxima, the neighbour maxima and the gather. Every step runs
over all pixels at once and the taps in order, which rounds like the header's pixel-by-pixel statement does. Nothing here calls
the library; of the product it reads constants of abi alone."""
import numpy as np

from pyrite_amd import abi

f32 = np.float32
u32 = np.uint32
MOTION_HIT, MOTION_IN_FRONT = abi.PYR_MOTION_HIT, abi.PYR_MOTION_IN_FRONT
RECORD = np.dtype([("prev_x", "<f4"), ("prev_y", "<f4"), ("prev_depth", "<f4"), ("depth", "<f4"), ("shape", "<u4"), ("flags", "<u4"), ("reserved", "<u4", (2,))])
HALF, ONE, ZERO, TWO, THREE = f32(0.5), f32(1), f32(0), f32(2), f32(3)
FLT_MAX = np.finfo(f32).max
DEFAULTS = dict(shutter=abi.PYR_MOTION_BLUR_SHUTTER, samples=abi.PYR_MOTION_BLUR_SAMPLES, max_radius=abi.PYR_MOTION_BLUR_MAX_RADIUS,
                depth_softness=abi.PYR_MOTION_BLUR_DEPTH_SOFTNESS, seed=0)


def clamp01(v):
    return np.fmin(np.fmax(v, ZERO), ONE)  # fmaxf, fminf: a NaN becomes 0


def velocities(motion, shutter, max_radius):
    """(hx, hy, len, z), float32 [height, width] each."""
    height, width = motion.shape
    radius = f32(max_radius)
    x, y = np.meshgrid(np.arange(width).astype(f32), np.arange(height).astype(f32))
    with np.errstate(all="ignore"):
        dx, dy = (x + HALF) - motion["prev_x"], (y + HALF) - motion["prev_y"]
        s = HALF * f32(shutter)
        hx, hy = dx * s, dy * s
        length = np.sqrt(hx * hx + hy * hy)
        still = ((motion["flags"] & MOTION_IN_FRONT) == 0) | ~np.isfinite(motion["prev_x"]) | ~np.isfinite(motion["prev_y"]) | ~np.isfinite(length)
        over = ~still & (length > radius)
        k = radius / length
        hx, hy, length = np.where(over, hx * k, hx), np.where(over, hy * k, hy), np.where(over, radius, length)
        hx, hy, length = np.where(still, ZERO, hx), np.where(still, ZERO, hy), np.where(still, ZERO, length)
    z = np.where((motion["flags"] & MOTION_HIT) != 0, motion["depth"], FLT_MAX).astype(f32)
    return hx.astype(f32), hy.astype(f32), length.astype(f32), z


def tile_maxima(hx, hy, length, max_radius):
    """float32 [tiles_y, tiles_x, 3]: (hx, hy, len) of each tile's pixel of largest len, the smallest row-major index among equals."""
    height, width = length.shape
    edge = int(max_radius)
    tiles_x, tiles_y = (width + edge - 1) // edge, (height + edge - 1) // edge
    out = np.zeros((tiles_y, tiles_x, 3), dtype=f32)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            rows, cols = slice(ty * edge, min((ty + 1) * edge, height)), slice(tx * edge, min((tx + 1) * edge, width))
            block = length[rows, cols]
            r, c = np.unravel_index(np.argmax(block), block.shape)  # the first of equal maxima in row-major order
            out[ty, tx] = hx[rows, cols][r, c], hy[rows, cols][r, c], block[r, c]
    return out


def neighbour_maxima(tiles):
    """float32 [tiles_y, tiles_x, 3]: per tile, the tile maximum of largest len in its 3 x 3 block, the smallest tile index among equals."""
    tiles_y, tiles_x, _ = tiles.shape
    out = np.zeros_like(tiles)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            best = None
            for y in range(max(ty - 1, 0), min(ty + 1, tiles_y - 1) + 1):
                for x in range(max(tx - 1, 0), min(tx + 1, tiles_x - 1) + 1):
                    if best is None or tiles[y, x, 2] > best[2]:
                        best = tiles[y, x]
            out[ty, tx] = best
    return out


def jitter(width, height, seed):
    """float32 [height, width] in [-0.5, 0.5): the header's integer hash of (pixel index, seed), its top 24 bits as the float."""
    with np.errstate(over="ignore"):
        k = np.arange(width * height, dtype=np.uint64).astype(u32).reshape(height, width) + u32(seed & 0xFFFFFFFF) * u32(0x9E3779B1)
        k = k ^ (k >> u32(16))
        k = k * u32(0x7FEB352D)
        k = k ^ (k >> u32(15))
        k = k * u32(0x846CA68B)
        k = k ^ (k >> u32(16))
    return (k >> u32(8)).astype(f32) * f32(2.0 ** -24) - HALF


def cone(d, l):
    return clamp01(ONE - d / l)


def cylinder(d, l):
    lo, hi = f32(0.95) * l, f32(1.05) * l
    u = clamp01((d - lo) / (hi - lo))
    return ONE - (u * u) * (THREE - TWO * u)


def front(a, b, e):
    return clamp01(ONE - (a - b) / e)


def neighbour_of_pixels(neighbours, width, height, max_radius):
    """float32 [height, width, 3]: each pixel's tile's neighbour maximum."""
    edge = int(max_radius)
    return neighbours[np.arange(height)[:, None] // edge, np.arange(width)[None, :] // edge]


def motion_blur(image, motion, shutter=DEFAULTS["shutter"], samples=DEFAULTS["samples"], max_radius=DEFAULTS["max_radius"], depth_softness=DEFAULTS["depth_softness"],
                seed=0, taps_out=None):
    """out [height, width, 3] of pyr_image_motion_blur. `taps_out`, a list, receives (ax, ay, counted) of every tap in order: the
    tap positions as floats [height, width] and which pixels counted that tap."""
    image = np.asarray(image, dtype=f32)
    height, width, _ = image.shape
    hx, hy, length, z = velocities(motion, shutter, max_radius)
    per_pixel = neighbour_of_pixels(neighbour_maxima(tile_maxima(hx, hy, length, max_radius)), width, height, max_radius)
    nx, ny, ln = per_pixel[..., 0], per_pixel[..., 1], per_pixel[..., 2]
    copies = (ln < HALF) | ~np.isfinite(image).all(axis=-1)
    x, y = np.meshgrid(np.arange(width).astype(f32), np.arange(height).astype(f32))
    cx, cy = x + HALF, y + HALF
    fw, fh, n, soft = f32(width), f32(height), f32(samples), f32(depth_softness)
    j = jitter(width, height, seed)
    with np.errstate(all="ignore"):
        l_x = np.fmax(length, HALF)
        w0 = ONE / l_x
        weight = w0.copy()
        total = (w0[..., None] * image).astype(f32)
        for i in range(int(samples)):
            t = (((f32(i) + HALF) + j) / n) * TWO - ONE
            ox, oy = nx * t, ny * t
            ax, ay = np.floor(cx + ox), np.floor(cy + oy)
            inside = (ax >= 0) & (ax < fw) & (ay >= 0) & (ay < fh)
            ix, iy = np.where(inside, ax, ZERO).astype(np.int64), np.where(inside, ay, ZERO).astype(np.int64)
            inside &= (ix < width) & (iy < height)
            ix, iy = np.minimum(ix, width - 1), np.minimum(iy, height - 1)
            theirs = image[iy, ix]
            counted = inside & np.isfinite(theirs).all(axis=-1) & ~copies
            dist = np.sqrt(ox * ox + oy * oy)
            l_y, z_y = np.fmax(length[iy, ix], HALF), z[iy, ix]
            e = soft * np.fmax(z, z_y)
            w = (front(z_y, z, e) * cone(dist, l_y) + front(z, z_y, e) * cone(dist, l_x)) + (cylinder(dist, l_y) * cylinder(dist, l_x)) * TWO
            weight = np.where(counted, weight + w, weight).astype(f32)
            total = np.where(counted[..., None], total + w[..., None] * np.where(counted[..., None], theirs, ZERO), total).astype(f32)
            if taps_out is not None:
                taps_out.append((ax, ay, counted))
        out = (total / weight[..., None]).astype(f32)
    return np.where(copies[..., None], image, out).astype(f32)
