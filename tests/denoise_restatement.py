"""The denoiser of include/pyrite_gpu.h ("denoising a linear image from two halves") restated in numpy f32: vectorised over the
image, looping over the offsets in the order the header fixes, one rounding per operation. It shares no code with the kernels;
of everything below only np.exp may differ from what the GPU computes (expf)."""
import numpy as np

f32 = np.float32

DEFAULTS = dict(radius=5, patch=1, k=0.45, epsilon=1e-10, sigma_albedo=0.02, sigma_normal=0.1, sigma_depth=0.02)


def variance(a, b):
    """V_c(p) = 0.5f * (sum of (a - b)^2 over the clipped 3 x 3 neighbourhood, raster order, / the pixels summed); NaN where that is +inf."""
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    h, w, _ = a.shape
    with np.errstate(all="ignore"):
        d = a - b
        s = np.zeros((h + 2, w + 2, 3), dtype=f32)
        s[1:-1, 1:-1] = d * d
        inside = np.zeros((h + 2, w + 2), dtype=bool)
        inside[1:-1, 1:-1] = True
        total, count = np.zeros((h, w, 3), dtype=f32), np.zeros((h, w), dtype=f32)
        for dy in range(3):
            for dx in range(3):
                keep = inside[dy:dy + h, dx:dx + w]
                total = np.where(keep[..., None], total + s[dy:dy + h, dx:dx + w], total)  # a skipped neighbour adds nothing
                count = count + keep.astype(f32)
        v = f32(0.5) * (total / count[..., None])
        return np.where(np.isposinf(v), f32(np.nan), v)


def _padded(image, pad):
    h, w = image.shape[:2]
    out = np.zeros((h + 2 * pad, w + 2 * pad) + image.shape[2:], dtype=image.dtype)
    out[pad:pad + h, pad:pad + w] = image
    return out


def _windows(padded, pad, radius, ty, tx, h, w):
    """view[oy + radius, ox + radius, y, x] = padded image at pixel (y + oy + ty, x + ox + tx)"""
    base = padded[pad - radius + ty:pad + radius + ty + h, pad - radius + tx:pad + radius + tx + w]
    return np.lib.stride_tricks.sliding_window_view(base, (h, w), axis=(0, 1))


def colour_distance(half, v, radius, patch, k, epsilon):
    """(S / (3.0f * n)) for every window offset and pixel, shape [2r+1, 2r+1, h, w]: NaN where it is NaN, before fmaxf(., 0)."""
    half, v = np.asarray(half, dtype=f32), np.asarray(v, dtype=f32)
    h, w, _ = half.shape
    pad = radius + patch
    hp, vp, inside = _padded(half, pad), _padded(v, pad), _padded(np.ones((h, w), dtype=bool), pad)
    side = 2 * radius + 1
    s, n = np.zeros((side, side, h, w), dtype=f32), np.zeros((side, side, h, w), dtype=f32)
    kk, eps = f32(k) * f32(k), f32(epsilon)
    with np.errstate(all="ignore"):
        for dy in range(-patch, patch + 1):
            for dx in range(-patch, patch + 1):
                keep = inside[pad + dy:pad + dy + h, pad + dx:pad + dx + w][None, None] & _windows(inside, pad, radius, dy, dx, h, w)
                n = n + keep.astype(f32)
                for c in range(3):
                    h_p, v_p = hp[pad + dy:pad + dy + h, pad + dx:pad + dx + w, c][None, None], vp[pad + dy:pad + dy + h, pad + dx:pad + dx + w, c][None, None]
                    h_q, v_q = _windows(hp[..., c], pad, radius, dy, dx, h, w), _windows(vp[..., c], pad, radius, dy, dx, h, w)
                    d = h_p - h_q
                    term = (d * d - (v_p + np.fmin(v_p, v_q))) / (eps + kk * (v_p + v_q))
                    s = np.where(keep, s + term, s)
        return s / (f32(3.0) * n)  # n = 0 only where q is outside the image: never read


def _guide_term(values, radius, sigma):
    """sum_c (g_c(p) - g_c(q))^2 / (2.0f * (sigma * sigma)), shape [2r+1, 2r+1, h, w]"""
    h, w, channels = values.shape
    gp = _padded(values, radius)
    total = np.zeros((2 * radius + 1, 2 * radius + 1, h, w), dtype=f32)
    for c in range(channels):
        d = values[..., c][None, None] - _windows(gp[..., c], radius, radius, 0, 0, h, w)
        total = total + d * d
    return total / (f32(2.0) * (f32(sigma) * f32(sigma)))


def weights(half, v, albedo=None, normal=None, depth=None, radius=5, patch=1, k=0.45, epsilon=1e-10, sigma_albedo=0.02, sigma_normal=0.1, sigma_depth=0.02,
            distance=None):
    """w(p, p + o), shape [2r+1, 2r+1, h, w]; 0 where q is outside the image. `distance`: colour_distance's result, when at hand."""
    h, w, _ = half.shape
    with np.errstate(all="ignore"):
        d = colour_distance(half, v, radius, patch, k, epsilon) if distance is None else distance
        nan = np.isnan(d)
        d = np.fmax(d, f32(0.0))
        terms = []
        if albedo is not None and sigma_albedo > 0:
            terms.append(_guide_term(np.asarray(albedo, dtype=f32), radius, sigma_albedo))
        if normal is not None and sigma_normal > 0:
            terms.append(_guide_term(np.asarray(normal, dtype=f32), radius, sigma_normal))
        if depth is not None and sigma_depth > 0:
            z = np.asarray(depth, dtype=f32)
            z_p, z_q = z[None, None], _windows(_padded(z, radius), radius, radius, 0, 0, h, w)
            m = np.fmax(np.fmax(z_p, z_q), f32(1e-30))
            r = (z_p - z_q) / m
            terms.append((r * r) / (f32(2.0) * (f32(sigma_depth) * f32(sigma_depth))))
        for g in terms:
            nan = nan | np.isnan(g)
            d = np.fmax(d, g)
        out = np.where(nan, f32(0.0), np.exp(-d).astype(f32))
        out[radius, radius] = f32(1.0)  # o = 0 by definition
        return np.where(_windows(_padded(np.ones((h, w), dtype=bool), radius), radius, radius, 0, 0, h, w), out, f32(0.0))


def cross_filter(wts, image, radius):
    """(sum_o w * image(p + o)) / (sum_o w), o in raster order; an offset of weight 0 adds nothing."""
    image = np.asarray(image, dtype=f32)
    h, w, _ = image.shape
    ip = _padded(image, radius)
    num, den = np.zeros((h, w, 3), dtype=f32), np.zeros((h, w), dtype=f32)
    with np.errstate(all="ignore"):
        for oy in range(2 * radius + 1):
            for ox in range(2 * radius + 1):
                wt = wts[oy, ox]
                use = wt > 0
                num = np.where(use[..., None], num + wt[..., None] * ip[oy:oy + h, ox:ox + w], num)
                den = np.where(use, den + wt, den)
        return num / den[..., None]


def denoise(a, b, albedo=None, normal=None, depth=None, distances=None, **params):
    """(out, error) of the header's semantics. `distances`: (colour_distance of b, colour_distance of a), when at hand."""
    p = dict(DEFAULTS, **params)
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    v = variance(a, b)
    d_b, d_a = distances if distances is not None else (None, None)
    fa = cross_filter(weights(b, v, albedo, normal, depth, distance=d_b, **p), a, p["radius"])
    fb = cross_filter(weights(a, v, albedo, normal, depth, distance=d_a, **p), b, p["radius"])
    with np.errstate(all="ignore"):
        return (fa + fb) * f32(0.5), np.abs(fa - fb) * f32(0.5)
