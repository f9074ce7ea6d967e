"""include/pyrite_gpu.h "lens blur over the feature records" restated in numpy float32, one rounding per operation in the order the
header writes: the circle of confusion, disc weight and axial depth of every pixel, and the gather. The offsets of the window run
in the header's order and every step runs over all pixels at once, which rounds like the header's pixel-by-pixel statement does.
Every offset of the (2*max_radius+1)^2 window is visited: nothing here knows of tiles or of a reach. Nothing here calls the
library; of the product it reads constants of abi alone."""
import numpy as np

from pyrite_amd import abi

f32 = np.float32
RECORD = np.dtype([("normal", "<f4", (3,)), ("depth", "<f4"), ("coverage", "<f4"), ("shape", "<u4"), ("material", "<u4"), ("reserved", "<u4")])
HALF, ONE, ZERO = f32(0.5), f32(1), f32(0)
FLT_MAX = np.finfo(f32).max
PI_F = f32(3.14159265)
DEFAULTS = dict(max_radius=abi.PYR_LENS_BLUR_MAX_RADIUS, depth_tolerance=abi.PYR_REPROJECT_DEPTH_TOLERANCE)


def clamp01(v):
    return np.fmin(np.fmax(v, ZERO), ONE)  # fmaxf, fminf: a NaN becomes 0


def scale(width, height, focus_distance, aperture, view_plane):
    """(m, A): half the longer side, and the pixels of blur per unit of |1 - f/z|."""
    with np.errstate(all="ignore"):
        m = f32(max(width, height)) * HALF
        A = (np.sqrt(f32(aperture)) * (f32(view_plane) / f32(focus_distance))) * m
    return m, f32(A)


def circles(pixels, focus_distance, aperture, view_plane, max_radius):
    """(c, inv, z), float32 [height, width] each: the circle of confusion in pixels, one over its disc's area, the axial depth."""
    height, width = pixels.shape
    f, vp, R = f32(focus_distance), f32(view_plane), f32(max_radius)
    m, A = scale(width, height, focus_distance, aperture, view_plane)
    x, y = np.meshgrid(np.arange(width).astype(f32), np.arange(height).astype(f32))
    depth, coverage = pixels["depth"], pixels["coverage"]
    with np.errstate(all="ignore"):
        miss = (coverage == 0) | ~np.isfinite(depth) | (depth <= 0)
        half_size = (ONE / m) * HALF
        px, py = (x + -(f32(width) * HALF)) / m + half_size, (y + -(f32(height) * HALF)) / m + half_size
        t = (px * px + py * py) / (vp * vp)
        z = depth / np.sqrt(ONE + t)
        c = np.fmin(A * np.abs(ONE - f / z), R)
        z = np.where(miss, FLT_MAX, z).astype(f32)
        c = np.where(miss, np.fmin(A, R), c).astype(f32)
        inv = ONE / np.fmax(PI_F * ((c + HALF) * (c + HALF)), ONE)
    return c, inv.astype(f32), z


def lens_blur(image, pixels, focus_distance, aperture, view_plane, max_radius=DEFAULTS["max_radius"], depth_tolerance=DEFAULTS["depth_tolerance"]):
    """out [height, width, 3] of pyr_image_lens_blur."""
    image = np.asarray(image, dtype=f32)
    height, width, _ = image.shape
    radius, tol = int(max_radius), f32(depth_tolerance)
    c_p, inv_p, z_p = circles(pixels, focus_distance, aperture, view_plane, max_radius)
    usable = np.isfinite(image).all(axis=-1)
    weight_f, weight_b = np.zeros((height, width), dtype=f32), np.zeros((height, width), dtype=f32)
    sum_f, sum_b = np.zeros((height, width, 3), dtype=f32), np.zeros((height, width, 3), dtype=f32)
    others = np.zeros((height, width), dtype=bool)
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    with np.errstate(all="ignore"):
        limit = tol * z_p
        for oy in range(-radius, radius + 1):
            for ox in range(-radius, radius + 1):
                qy, qx = ys + oy, xs + ox
                inside = (qy >= 0) & (qy < height) & (qx >= 0) & (qx < width)
                qy, qx = np.clip(qy, 0, height - 1), np.clip(qx, 0, width - 1)
                counted = inside & usable[qy, qx]
                c_q, inv_q, z_q, colour = c_p[qy, qx], inv_p[qy, qx], z_p[qy, qx], image[qy, qx]
                d = np.sqrt(f32(ox * ox + oy * oy))
                front = (z_p - z_q) > limit
                c_e = np.where(front, c_q, np.fmin(c_q, c_p))
                inv_e = np.where(front | (c_q < c_p), inv_q, inv_p)
                w = (clamp01((c_e - d) + ONE) * inv_e).astype(f32)
                counted &= w > 0  # a tap with w == 0 adds nothing
                to_f, to_b = counted & front, counted & ~front
                colour = np.where(counted[..., None], colour, ZERO)  # nothing of a tap that is not counted reaches a product
                weight_f = np.where(to_f, weight_f + w, weight_f).astype(f32)
                weight_b = np.where(to_b, weight_b + w, weight_b).astype(f32)
                sum_f = np.where(to_f[..., None], sum_f + w[..., None] * colour, sum_f).astype(f32)
                sum_b = np.where(to_b[..., None], sum_b + w[..., None] * colour, sum_b).astype(f32)
                if ox != 0 or oy != 0:
                    others |= counted
        B = sum_b / weight_b[..., None]
        a = np.fmin(weight_f, ONE)[..., None]
        F = sum_f / weight_f[..., None]
        mixed = a * F + (ONE - a) * B
        out = np.where((weight_f == 0)[..., None], B, mixed).astype(f32)
    keeps = ~usable | ~others
    return np.where(keeps[..., None], image, out).astype(f32)
