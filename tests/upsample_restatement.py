"""The guided upsampling of include/pyrite_gpu.h ("upsample") restated in numpy: float32 throughout, one operation a line, in the
header's order, written from the header's text and not from the kernel. tests/test_upsample_cpu.py holds it against properties of
the rule, tests/test_gpu_upsample.py holds the kernel against it bit for bit.

Every output pixel is computed at once, tap by tap: the sums of a pixel run in tap order (j outer) as the header says. `paths`
returns, beside the image, which rule gave each pixel -- the guided sum or the fallback -- and whether a gain was clamped there."""
import numpy as np

f32 = np.float32
MATCH_MATERIAL = 1
MOST_RADIUS, MOST_SCALE = 3, 8


def record_fields(pixels, height, width):
    """(normal [h, w, 3], depth [h, w], material [h, w]) of PyrFeaturePixel records given as any array of 32 bytes a pixel."""
    words = np.ascontiguousarray(pixels).view(np.uint8).reshape(height, width, 32)
    floats = words[..., :16].copy().view(f32).reshape(height, width, 4)
    material = words[..., 24:28].copy().view(np.uint32).reshape(height, width)
    return floats[..., :3], floats[..., 3], material


def upsample(low, scale, albedo=None, pixels=None, low_albedo=None, low_pixels=None, radius=1, flags=MATCH_MATERIAL, sigma_normal=0.1, sigma_depth=0.02,
             albedo_floor=0.01, max_gain=4.0, paths=False):
    low = np.asarray(low, dtype=f32)
    h, w, _ = low.shape
    H, W = h * scale, w * scale
    assert 2 <= scale <= MOST_SCALE and 1 <= radius <= MOST_RADIUS and (albedo is None) == (low_albedo is None) and (pixels is None) == (low_pixels is None)
    sigma_normal, sigma_depth, albedo_floor, max_gain = f32(sigma_normal), f32(sigma_depth), f32(albedo_floor), f32(max_gain)
    one, half, zero = f32(1), f32(0.5), f32(0)
    with np.errstate(all="ignore"):
        lx = (np.arange(W, dtype=np.uint32).astype(f32) + half)
        lx = lx / f32(scale)
        lx = lx - half
        ly = (np.arange(H, dtype=np.uint32).astype(f32) + half)
        ly = ly / f32(scale)
        ly = ly - half
        x0, y0 = np.floor(lx).astype(np.int64), np.floor(ly).astype(np.int64)
        if albedo is not None:
            d = np.fmax(np.asarray(low_albedo, dtype=f32), zero)  # fmaxf: a NaN albedo counts as 0
            d = d + albedo_floor
            d = one / d  # per low pixel and channel, once
            own = np.fmax(np.asarray(albedo, dtype=f32), zero)
            own = own + albedo_floor
        if pixels is not None:
            n_low, z_low, m_low = record_fields(low_pixels, h, w)
            n_own, z_own, m_own = record_fields(pixels, H, W)
            normal_div = sigma_normal * sigma_normal
            normal_div = f32(2) * normal_div
            depth_div = sigma_depth * sigma_depth
            depth_div = f32(2) * depth_div
        Wt, S = np.zeros((H, W), dtype=f32), np.zeros((H, W), dtype=f32)
        A, B = np.zeros((H, W, 3), dtype=f32), np.zeros((H, W, 3), dtype=f32)
        clamped = np.zeros((H, W), dtype=bool)
        for j in range(2 * radius):
            qy = y0 - (radius - 1) + j
            sy = np.abs(qy.astype(f32) - ly)
            sy = sy / f32(radius)
            sy = np.maximum(one - sy, zero)
            for i in range(2 * radius):
                qx = x0 - (radius - 1) + i
                sx = np.abs(qx.astype(f32) - lx)
                sx = sx / f32(radius)
                sx = np.maximum(one - sx, zero)
                sp = sy[:, None] * sx[None, :]
                inside = ((qy >= 0) & (qy < h))[:, None] & ((qx >= 0) & (qx < w))[None, :]
                kept = inside & (sp != 0)
                cy, cx = np.clip(qy, 0, h - 1)[:, None], np.clip(qx, 0, w - 1)[None, :]  # read somewhere; `kept` decides what counts
                tap = low[cy, cx]
                gw = np.ones((H, W), dtype=f32)
                if pixels is not None:
                    D = np.zeros((H, W), dtype=f32)
                    nan = np.zeros((H, W), dtype=bool)
                    if sigma_normal > 0:
                        e = n_own - n_low[cy, cx]
                        g = zero + e[..., 0] * e[..., 0]
                        g = g + e[..., 1] * e[..., 1]
                        g = g + e[..., 2] * e[..., 2]
                        g = g / normal_div
                        nan |= np.isnan(g)
                        D = np.where(np.isnan(g), D, np.maximum(D, g))
                    if sigma_depth > 0:
                        z_q = z_low[cy, cx]
                        m = np.fmax(np.fmax(z_own, z_q), f32(1e-30))  # fmaxf: a NaN operand is ignored
                        r = z_own - z_q
                        r = r / m
                        g = r * r
                        g = g / depth_div
                        nan |= np.isnan(g)
                        D = np.where(np.isnan(g), D, np.maximum(D, g))
                    t = one - D
                    gw = np.where(t > 0, t * t, zero)
                    gw = np.where(nan, zero, gw)
                    if flags & MATCH_MATERIAL:
                        gw = np.where(m_own != m_low[cy, cx], zero, gw)
                wgt = sp * gw
                S = np.where(kept, S + sp, S)
                B = np.where(kept[..., None], B + sp[..., None] * tap, B)
                counts = kept & (wgt > 0)
                v = tap
                if albedo is not None:
                    k = own * d[cy, cx]
                    over = ~(k < max_gain)  # fminf(k, max_gain), a NaN k counting as max_gain
                    k = np.where(over, max_gain, k)
                    clamped |= counts & over.any(axis=-1)
                    v = tap * k
                Wt = np.where(counts, Wt + wgt, Wt)
                A = np.where(counts[..., None], A + wgt[..., None] * v, A)
        guided = Wt > 0
        out = np.where(guided[..., None], A / Wt[..., None], B / S[..., None]).astype(f32)
    if paths:
        return out, guided, clamped
    return out
