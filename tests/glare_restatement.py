"""include/pyrite_gpu.h "glare" restated in numpy float32, one rounding per operation in the order the header writes. Nothing here
calls the library and nothing is taken from the kernels: every step is an operation over a whole level, written from the header's
text. tests/test_glare_cpu.py checks the rule's own properties on this file, tests/test_gpu_glare.py compares the kernels with it
bit for bit.
  Every array operation below is one f32 operation per element; the constants are np.float32 scalars, so nothing is promoted."""
import numpy as np

f32 = np.float32
ZERO, ONE, TINY = f32(0), f32(1), f32(1e-30)
EIGHTH, THREE_EIGHTHS, QUARTER, THREE_QUARTERS = f32(0.125), f32(0.375), f32(0.25), f32(0.75)
LUMA = (f32(0.2126), f32(0.7152), f32(0.0722))
MOST_LEVELS = 12


def clamp01(v):
    """fminf(fmaxf(v, 0.0f), 1.0f): a NaN becomes 0."""
    return np.fmin(np.fmax(v, ZERO), ONE)


def kept_pixels(image):
    """bool [h, w]: the pixels whose three floats are all finite."""
    return np.isfinite(image).all(axis=-1)


@np.errstate(all="ignore")
def source(image, threshold):
    """S0 [h, w, 3]: 0 at a pixel that is not kept; the image's own bits with threshold == 0; else image * k."""
    kept = kept_pixels(image)
    if f32(threshold) == ZERO:
        s = image.copy()
    else:
        r, g, b = image[..., 0], image[..., 1], image[..., 2]
        y = (LUMA[0] * r + LUMA[1] * g) + LUMA[2] * b
        k = clamp01((y - f32(threshold)) / np.fmax(y, TINY))
        s = image * k[..., None]
    s[~kept] = ZERO
    return s


def level_sizes(width, height, levels):
    """[(w_0, h_0), ..., (w_L, h_L)]: L = min(levels, the steps until a level is 1 x 1)."""
    sizes = [(width, height)]
    while len(sizes) - 1 < levels and sizes[-1] != (1, 1):
        w, h = sizes[-1]
        sizes.append(((w + 1) // 2, (h + 1) // 2))
    return sizes


def _down_axis(s, axis):
    n = s.shape[axis]
    x = np.arange((n + 1) // 2)
    a, b, c, d = (np.take(s, np.clip(2 * x + k, 0, n - 1), axis=axis) for k in (-1, 0, 1, 2))
    return (a + d) * EIGHTH + (b + c) * THREE_EIGHTHS


@np.errstate(all="ignore")
def down(s):
    """S_{l+1} [(h+1)//2, (w+1)//2, 3] from S_l [h, w, 3]: rows first (along x), then columns on the f32 row results."""
    return _down_axis(_down_axis(s, 1), 0)


def _up_axis(t, axis, n):
    m = t.shape[axis]
    x = np.arange(n)
    i = x >> 1
    other = np.where(x & 1, np.minimum(i + 1, m - 1), np.maximum(i - 1, 0))
    return np.take(t, i, axis=axis) * THREE_QUARTERS + np.take(t, other, axis=axis) * QUARTER


@np.errstate(all="ignore")
def up(t, width, height):
    """Up(T) [height, width, 3] from T of the level below: rows first (along x), then columns."""
    return _up_axis(_up_axis(t, 1, width), 0, height)


def weights(levels, falloff):
    """(g [L + 1] with g[0] unused, inv): g_1 = 1, g_{l+1} = g_l * falloff, G summed from the left, inv = 1 / G -- all f32."""
    g = [None, ONE]
    for _ in range(2, levels + 1):
        g.append(f32(g[-1] * f32(falloff)))
    total = g[1]
    for l in range(2, levels + 1):
        total = f32(total + g[l])
    with np.errstate(all="ignore"):
        return g, f32(ONE / total)


@np.errstate(all="ignore")
def blurred(image, levels=6, threshold=0.0, falloff=1.0):
    """B [h, w, 3] = Up(T_1) * inv, or None for a 1 x 1 image (L = 0)."""
    image = np.ascontiguousarray(image, dtype=f32)
    height, width, _ = image.shape
    sizes = level_sizes(width, height, levels)
    L = len(sizes) - 1
    if L == 0:
        return None
    S = [source(image, threshold)]
    for _ in range(L):
        S.append(down(S[-1]))
    g, inv = weights(L, falloff)
    T = S[L] * g[L]
    for l in range(L - 1, 0, -1):
        T = S[l] * g[l] + up(T, sizes[l][0], sizes[l][1])
    return up(T, width, height) * inv


@np.errstate(all="ignore")
def glare(image, strength=0.1, levels=6, threshold=0.0, falloff=1.0):
    """out [h, w, 3]: the header's rule; a pixel that is not kept keeps its bits."""
    image = np.ascontiguousarray(image, dtype=f32)
    B = blurred(image, levels, threshold, falloff)
    if B is None:
        return image.copy()
    s0 = source(image, threshold)
    out = (image - f32(strength) * s0) + f32(strength) * B
    kept = kept_pixels(image)
    out.view(np.uint32)[~kept] = image.view(np.uint32)[~kept]
    return out
