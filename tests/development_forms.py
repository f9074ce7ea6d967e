"""What the reference computes between a film and its picture, restated in float64 numpy: the companion of tests/closed_forms.py and
tests/surface_forms.py for film development -- grains to quotients, the step-function spectrum, the trapezoid walk against the CIE
observer, `filter` and `white`, XYZ to linear sRGB and the 8-bit encoding. Nothing here comes from pyrite_amd or from the oracle:
the tables are read from the reference's own data files (tests/golden/colour/*.csv, byte-for-byte copies), the cases are plain
arrays and tuples that the callers turn into Films and project expressions. Every statement cites the reference line
(pyrite/src/..., pyrite/build.rs) it restates.

The reference walks its wavelengths in f32 (`wl_min + step_size`) and finds a bin by an f32 quotient. A float64 form can only say
what that does where both are exact, so `sample_points` REFUSES a span and step whose sample wavelengths are not all f32 numbers,
and the assignment of samples to bins is done in exact rationals (`fractions`). Where a sample falls exactly on a bin edge and the
f32 quotient (w - min) / (max - min) is not exact, the reference may land in either bin: `uncertain_edges` names those pairs of
bins and `left_out` the pixels in which the two bins differ. tests/test_development_forms_cpu.py holds the caps on what may be left
out, on this module alone.

Bounds: the kernels and the oracle work in f32. The bound of each statement class is FOUR TIMES the largest |oracle - form| measured
on the CPU over every case (MEASURED below, profiles/r26_development_forms.txt) -- never a figure taken from the kernels."""
import csv
import math
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colour")
XYZ_SCALE = 3.444  # main.rs:368 "Scale up to better match D65 light source data"

# Largest |oracle - form| per statement class over all cases, measured on the CPU by
# tests/test_development_forms_cpu.py::test_measured_figures_are_the_ones_the_bounds_come_from, and the bound: four times that.
# "xyz" and "linear srgb" are relative to the pixel's largest |XYZ| of the form; "bytes" is the distance between the two values of
# 255 e (the number that is rounded to the byte), in bytes: the half-width of the band around k + 0.5 in which either byte passes.
MEASURED = {
    "xyz": 1.1e-6,  # 1.069e-6: one hot, 64 bins, step 30, filter and white
    "linear srgb": 3.1e-6,  # 3.014e-6: the same case
    "bytes": 6.3e-4,  # 6.236e-4: random, 67x5x5, 400-701
}
BOUNDS = {k: (np.inf if v is None else 4.0 * v) for k, v in MEASURED.items()}
MOST_IN_BAND = 0.02  # of a case's bytes
MOST_LEFT_OUT = 0.25  # of a case's pixels


def f32(x):
    """The float32 nearest to x, as a Python float: how the reference holds a number it parsed or wrote as f32."""
    return float(np.float32(x))


def is_f32(x):
    """x: a Fraction. Whether it is a float32 number."""
    return Fraction(f32(float(x))) == x


# ------------------------------------------------------------------------------------------------
# the tables (build.rs)
# ------------------------------------------------------------------------------------------------
def read_csv(name):
    """(header, rows of strings) of tests/golden/colour/<name>."""
    with open(os.path.join(GOLDEN, name), newline="") as f:
        rows = [r for r in csv.reader(f) if r]
    return rows[0], rows[1:]


def load_tables():
    """The spectra build.rs generates, every number the f32 the reference's csv + serde parser makes of the text:
    observer  build.rs:68-121  x, y, z over [min, max] of the file's wavelength column (360 .. 830)
    d65, a    build.rs:131-187 ONE range for both lamps, the extremes of both files (300 .. 830); a is `intensity / 100.0` in f32 (:157)
    rgb       build.rs:18-59   min 360, max = 360 + len (sic: one past the data, 831)"""
    _, xyz = read_csv("ciexyz65_1.csv")
    _, d65 = read_csv("d65.csv")
    _, a = read_csv("a.csv")
    _, rgb = read_csv("srgb_cie1931.csv")
    lamp_w = [f32(r[0]) for r in d65] + [f32(r[0]) for r in a]
    return {
        "xyz": np.array([[f32(v) for v in r[1:4]] for r in xyz]),
        "xyz_min": min(f32(r[0]) for r in xyz),
        "xyz_max": max(f32(r[0]) for r in xyz),
        "d65": np.array([f32(r[1]) for r in d65]),
        "a": np.array([float(np.float32(r[1]) / np.float32(100.0)) for r in a]),
        "light_min": min(lamp_w),
        "light_max": max(lamp_w),
        "rgb_basis": np.array([[f32(v) for v in r] for r in rgb]),
        "rgb_min": 360.0,
        "rgb_max": f32(360.0 + len(rgb)),
    }


TABLES = load_tables()


# ------------------------------------------------------------------------------------------------
# spectra and the expressions of `filter` and `white`
# ------------------------------------------------------------------------------------------------
def array_get(points, lo, hi, w):
    """Spectrum::Array::get (project/spectra.rs:32-55): the END VALUES at and outside [min, max] (:38-39), linear interpolation
    between the two neighbouring points inside (:41-52). points: [n] or [n, c]."""
    points = np.asarray(points, dtype=np.float64)
    if w <= lo:
        return points[0]
    if w >= hi:
        return points[-1]
    index = (w - lo) / (hi - lo) * (len(points) - 1.0)
    i0 = int(math.floor(index))  # trunc of a positive number
    mix = index - i0
    return points[i0] * (1.0 - mix) + points[i0 + 1] * mix


def curve_get(points, w):
    """Interpolated::get (math.rs:22-72): ZERO at and outside the first and last knots (:37-45 return Default), linear between
    the two knots around w; a knot's own value at a knot."""
    if len(points) == 0 or points[0][0] >= w or points[-1][0] <= w:
        return 0.0
    for (x0, y0), (x1, y1) in zip(points[:-1], points[1:]):
        if x0 <= w <= x1:
            return y0 + (y1 - y0) * ((w - x0) / (x1 - x0))
    raise ValueError("knots out of order")


def blackbody(w, temperature):
    """math.rs:177-182: Planck's law with the reference's constants, w in nm."""
    metres = w * 1.0e-9
    return 3.74183e-16 * metres ** -5 / (math.exp(1.4388e-2 / (metres * temperature)) - 1.0)


def observer(w):
    """[x, y, z] of xyz::response::{X, Y, Z} (build.rs:100-114) at w."""
    return array_get(TABLES["xyz"], TABLES["xyz_min"], TABLES["xyz_max"], w)


def d65(w):
    """light_source::D65 (build.rs:171-175) at w."""
    return float(array_get(TABLES["d65"], TABLES["light_min"], TABLES["light_max"], w))


def evaluate(expression, w):
    """An expression of the image settings at wavelength w. A number; ("curve", [(x, y), ...]); ("array", min, max, [y, ...]);
    ("blackbody", kelvin); ("d65",); ("a",)."""
    if isinstance(expression, (int, float)):
        return float(expression)
    kind = expression[0]
    if kind == "curve":
        return curve_get(expression[1], w)
    if kind == "array":
        return float(array_get(expression[3], expression[1], expression[2], w))
    if kind == "blackbody":
        return blackbody(w, expression[1])
    if kind == "d65":
        return d65(w)
    if kind == "a":
        return float(array_get(TABLES["a"], TABLES["light_min"], TABLES["light_max"], w))
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------
# the film's spectrum (film.rs)
# ------------------------------------------------------------------------------------------------
def quotients(grains, grains_b=None):
    """Grain::develop (film.rs:132-143) of every grain: acc / weight, 0 when weight <= 0. grains: float32 [..., bins, 2] ->
    float64 [..., bins]. Two half films develop as their sum film, (accA + accB) / (wA + wB): film_sum adds accs and weights grain
    by grain before the quotient."""
    acc, weight = grains[..., 0].astype(np.float64), grains[..., 1].astype(np.float64)
    if grains_b is not None:
        acc, weight = acc + grains_b[..., 0], weight + grains_b[..., 1]
    out = np.zeros_like(acc)
    np.divide(acc, weight, out=out, where=weight > 0)
    return out


def exact_span(span):
    lo, hi = Fraction(span[0]), Fraction(span[1])
    if not (is_f32(lo) and is_f32(hi) and is_f32(hi - lo) and hi > lo):
        raise ValueError("span %r: min, max and max - min must be float32 numbers" % (span,))
    return lo, hi


def bin_of(span, bins, w):
    """Spectrum::get's grain index (film.rs:322-337) in exact rationals: None strictly outside [min, max] (:327-328);
    floor((w - min) / (max - min) * bins) (:330-332), so a sample exactly on an edge belongs to the UPPER bin; clamped to the last
    bin (:332), which is where w == max lands."""
    lo, hi = exact_span(span)
    w = Fraction(w)
    if w < lo or w > hi:
        return None
    return min(math.floor((w - lo) / (hi - lo) * bins), bins - 1)


def sample_points(span, step):
    """The wavelengths spectrum_to_tristimulus visits (main.rs:392-411), as Fractions: min, then + step while the previous one is
    below max -- so the last may overshoot max. Raises unless every one is a float32 number: the reference adds in f32."""
    lo, hi = exact_span(span)
    step = Fraction(step)
    if step <= 0 or not is_f32(step):
        raise ValueError("step %r is not a positive float32 number" % (step,))
    points = [lo]
    while points[-1] < hi:
        points.append(points[-1] + step)
    for w in points:
        if not is_f32(w):
            raise ValueError("sample wavelength %s of span %r, step %s is not a float32 number" % (w, span, step))
    return points


def uncertain_edges(span, bins, step):
    """[(lower bin, upper bin)] of the samples that fall exactly on an inner bin edge while the f32 quotient
    (w - min) / (max - min) of film.rs:330 is not exact: floor() of the rounded product may give either bin. Raises when a sample
    that is NOT on an edge comes closer to one than f32 could tell apart (2^-18 of the bin count)."""
    lo, hi = exact_span(span)
    out = []
    for w in sample_points(span, step):
        if w <= lo or w >= hi:
            continue  # w == min: index 0 exactly; w == max: the quotient is 1 exactly, clamped; beyond: no bin
        normalized = (w - lo) / (hi - lo)
        index = normalized * bins
        if index.denominator == 1:
            if not is_f32(normalized):
                out.append((int(index) - 1, int(index)))
        elif abs(index - round(index)) < Fraction(bins, 2 ** 18):
            raise ValueError("sample %s is too close to a bin edge for f32" % w)
    return out


def left_out(q, edges):
    """bool [pixels]: the pixels whose quotients differ between the two bins of an uncertain edge. q: [pixels, bins]."""
    mask = np.zeros(len(q), dtype=bool)
    for lower, upper in edges:
        mask |= q[:, lower] != q[:, upper]
    return mask


# ------------------------------------------------------------------------------------------------
# filter and white (main.rs:197-238)
# ------------------------------------------------------------------------------------------------
def white_maxima(span, white):
    """main.rs:206-214: the maxima of `white` and of D65 over min, min + 1, ... while below max -- a scan of its own, at 1 nm, NOT
    at the sample wavelengths. Both start from 0."""
    lo, hi = exact_span(span)
    w, most, most_d65 = lo, 0.0, 0.0
    while w < hi:
        if not is_f32(w):
            raise ValueError("white scan wavelength %s is not a float32 number" % w)
        most, most_d65 = max(most, evaluate(white, float(w))), max(most_d65, d65(float(w)))
        w += 1
    return most, most_d65


def gains(span, step, filter=None, white=None):
    """float64 [samples]: what multiplies the film's value at each sample wavelength (main.rs:224-238). filter (:197-202):
    intensity * filter(w). white (:216-221): intensity / max(white(w) / max_white, 0.000001) * (D65(w) / max_d65). Both are applied
    to the overshooting sample too, where the film's value is 0."""
    points = [float(w) for w in sample_points(span, step)]
    g = np.ones(len(points))
    if filter is not None:
        g *= [evaluate(filter, w) for w in points]
    if white is not None:
        most, most_d65 = white_maxima(span, white)
        g *= [1.0 / max(evaluate(white, w) / most, 0.000001) * (d65(w) / most_d65) for w in points]
    return g


# ------------------------------------------------------------------------------------------------
# the trapezoid walk (main.rs:352-418)
# ------------------------------------------------------------------------------------------------
def walk(q, span, step, filter=None, white=None):
    """XYZ of ONE pixel, q: [bins], sample by sample as spectrum_to_tristimulus does it (main.rs:389-417): each step adds
    (start * s_min + end * s_max) * 0.5 * (wl_max - wl_min) and its width to the weight; the sum is divided by the weight --
    n * step, which is more than the span when the last step overshoots -- and spectrum_to_xyz multiplies by 3.444 (:368)."""
    points = sample_points(span, step)
    g = gains(span, step, filter, white)
    bins = len(q)

    def sample(k):
        index = bin_of(span, bins, points[k])
        return (0.0 if index is None else q[index]) * g[k]

    total, weight = np.zeros(3), 0.0
    low, start = sample(0), observer(float(points[0]))
    for k in range(1, len(points)):
        high, end = sample(k), observer(float(points[k]))
        width = float(points[k] - points[k - 1])
        total += (start * low + end * high) * 0.5 * width
        weight += width
        low, start = high, end
    return (total if weight == 0.0 else total / weight) * XYZ_SCALE


def linear_map(span, bins, step, filter=None, white=None):
    """A, float64 [3, bins], with XYZ = A q: the film's spectrum is a step function, so the walk is linear in the quotients. The
    trapezoid rule over n equal steps weighs the first and last sample 1/2 and the others 1, times step; over the weight n * step
    that is c_k / n. Sample k adds c_k / n * 3.444 * observer(w_k) * gain_k to the column of the bin it falls in (exact rationals),
    nothing when it lies outside the span."""
    points = sample_points(span, step)
    g = gains(span, step, filter, white)
    n = len(points) - 1
    a = np.zeros((3, bins))
    for k, w in enumerate(points):
        index = bin_of(span, bins, w)
        if index is not None:
            a[:, index] += (0.5 if k in (0, n) else 1.0) / n * XYZ_SCALE * observer(float(w)) * g[k]
    return a


# ------------------------------------------------------------------------------------------------
# XYZ -> linear sRGB -> bytes
# ------------------------------------------------------------------------------------------------
PRIMARIES = ((0.64, 0.33), (0.30, 0.60), (0.15, 0.06))  # IEC 61966-2-1, xy of red, green, blue
WHITE_POINT = (0.95047, 1.0, 1.08883)  # [3P] palette 0.7.2 white_point::D65


def xyz_to_rgb_matrix():
    """[3P] palette 0.7.2 (`LinSrgb::from_color(Xyz)`, main.rs:323) derives the matrix from the primaries and the white point:
    the columns of RGB -> XYZ are the primaries' XYZ at Y = 1, each scaled so that (1, 1, 1) maps to the white point; XYZ -> RGB
    is its inverse."""
    p = np.array([[x / y, 1.0, (1.0 - x - y) / y] for x, y in PRIMARIES]).T
    scale = np.linalg.solve(p, np.array(WHITE_POINT))
    return np.linalg.inv(p * scale)


def encode255(rgb):
    """255 e: the clamp to [0, 1] (palette's FromColor clamps), the piecewise sRGB curve (IEC 61966-2-1: 12.92 v up to 0.0031308,
    1.055 v^(1/2.4) - 0.055 above), times 255. The byte is round(255 e) = floor(255 e + 0.5)."""
    v = np.clip(np.asarray(rgb, dtype=np.float64), 0.0, 1.0)
    e = np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(v, 1.0 / 2.4) - 0.055)
    return 255.0 * np.clip(e, 0.0, 1.0)


def develop(grains, span, step=2.0, filter=None, white=None, grains_b=None):
    """The picture of a film. grains: float32 [height, width, bins, 2]. -> dict of float64 [height * width, ...] arrays: "q" the
    quotients, "xyz", "rgb" (linear sRGB), "e255" and "bytes" (uint8), "scale" the pixel's largest |XYZ|, "left_out" (bool). The
    film's LAST pixel is never developed (film.rs:299: DevelopedPixels::next needs `end < len`) and stays black."""
    bins = grains.shape[-2]
    q = quotients(grains, grains_b).reshape(-1, bins)
    xyz = q @ linear_map(span, bins, step, filter, white).T
    xyz[-1] = 0.0
    rgb = xyz @ xyz_to_rgb_matrix().T
    e255 = encode255(rgb)
    return {"q": q, "xyz": xyz, "rgb": rgb, "e255": e255, "bytes": np.floor(e255 + 0.5).astype(np.uint8), "scale": np.abs(xyz).max(axis=1),
            "left_out": left_out(q, uncertain_edges(span, bins, step))}


# ------------------------------------------------------------------------------------------------
# the assertions, shared by the CPU and the GPU tests
# ------------------------------------------------------------------------------------------------
def linear_error(got, want, scale):
    """float64 [pixels]: the largest |got - want| of each pixel's three channels over the pixel's largest |XYZ| of the form (pixels
    whose form is all zero: the absolute difference)."""
    difference = np.abs(np.asarray(got, dtype=np.float64).reshape(-1, 3) - want).max(axis=1)
    return difference / np.where(scale > 0, scale, 1.0)


def in_band(e255, band):
    """bool like e255: 255 e lies within `band` of a rounding boundary k + 0.5, where either neighbouring byte passes."""
    return np.abs(e255 - np.floor(e255) - 0.5) <= band


def wrong_bytes(got, form, band):
    """bool [pixels, 3]: got's byte is not the form's, nor -- within the band around a rounding boundary -- the boundary's other
    byte. Left-out pixels are the caller's to mask."""
    got = np.asarray(got).reshape(-1, 3).astype(np.int64)
    want = form["bytes"].astype(np.int64)
    other = np.where(form["e255"] - np.floor(form["e255"]) >= 0.5, want - 1, want + 1)  # the byte across the nearest boundary
    return (got != want) & ~(in_band(form["e255"], band) & (got == other))


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
DEFAULT_SPAN = (380.0, 780.0)
# knots on sample wavelengths (450, 500, 600) and between them (455.5, 651): zero at and outside the end knots
CURVE = ("curve", [(450.0, 0.0), (455.5, 0.25), (500.0, 1.0), (600.0, 0.75), (651.0, 0.0)])
WARM = ("blackbody", 4000.0)
# a white that is 0 from 502 to 520 nm: there the balance divides by its floor (main.rs:219), a gain of a million over bins 20-21
# and, in part, 19 and 22
GAP = ("curve", [(379.0, 1.0), (500.0, 1.0), (502.0, 0.0), (520.0, 0.0), (522.0, 1.0), (781.0, 1.0)])


def one_hot(bins, dim=()):
    """Pixel p lights only bin p mod bins, with a value that depends on the pixel: the picture shows A column by column, and a
    quotient read from the wrong place shows at full size. 130 pixels or 2 bins + 3, whichever is more (more than two runs of 64, an
    odd count). The value grows with the bin count so that the pictures stay in the range of the bytes; of the unlit grains those
    in even bins have no weight and those in odd bins a weight and no light. The bins named in `dim` are lit a million times
    weaker: where a white balance divides by its floor of 0.000001."""
    pixels = max(130, 2 * bins + 3)
    grains = np.zeros((1, pixels, bins, 2), dtype=np.float32)
    grains[0, :, 1::2, 1] = 1.0
    p = np.arange(pixels)
    weight = (1 + p % 7).astype(np.float32)
    value = (bins * 0.25 * (0.3 + 0.6 * ((37 * p) % 101) / 101.0)).astype(np.float32)
    value[np.isin(p % bins, dim)] *= np.float32(2.0 ** -20)
    grains[0, p, p % bins, 0] = value * weight
    grains[0, p, p % bins, 1] = weight
    return grains


def random_film(width, height, bins, seed, most=1.0):
    """Seeded grains: weights are sample counts, about a tenth of them zero and one in fifty negative (no light: film.rs:138);
    |acc / weight| spans three decades up to `most`, about a tenth of the quotients negative."""
    rng = np.random.default_rng(seed)
    shape = (height, width, bins)
    weight = rng.integers(1, 65, size=shape).astype(np.float32)
    weight[rng.random(shape) < 0.1] = 0
    weight[rng.random(shape) < 0.02] *= -1
    value = (most * np.power(10.0, rng.uniform(-3, 0, size=shape)) * np.where(rng.random(shape) < 0.1, -1.0, 1.0)).astype(np.float32)
    grains = np.zeros(shape + (2,), dtype=np.float32)
    grains[..., 0], grains[..., 1] = weight * value, weight
    return grains


def long_film(runs):
    """`runs` runs of 64 pixels at one bin; the value depends on the pixel."""
    p = np.arange(runs * 64, dtype=np.uint64)
    grains = np.zeros((64, runs, 1, 2), dtype=np.float32)
    weight = (1 + p % 5).astype(np.float32)
    value = (0.05 + 1.2 * ((p * np.uint64(2654435761)) % np.uint64(1 << 20)).astype(np.float64) / (1 << 20)).astype(np.float32)
    grains[..., 0, 0], grains[..., 0, 1] = (value * weight).reshape(64, runs), weight.reshape(64, runs)
    return grains


class Case:
    def __init__(self, name, make, span=DEFAULT_SPAN, step=2.0, filter=None, white=None, halves=False, forms=("pixel", "wave")):
        self.name, self.make, self.span, self.step, self.filter, self.white, self.halves, self.forms = name, make, span, step, filter, white, halves, forms
        self._grains = self._form = None

    def grains(self):
        """float32 [height, width, bins, 2] -- of the first half film when the case has halves."""
        if self._grains is None:
            self._grains = self.make()
        return self._grains

    def grains_b(self):
        """The second half film: the first one's grains in another order along the row, so that no half alone gives the picture."""
        return np.ascontiguousarray(self.grains()[:, ::-1]) if self.halves else None

    def settings(self):
        return {"step": self.step, "filter": self.filter, "white": self.white}

    def form(self):
        """develop() of the case, computed once and shared; nothing may write to it."""
        if self._form is None:
            self._form = develop(self.grains(), self.span, self.step, self.filter, self.white, self.grains_b())
            for v in self._form.values():
                v.setflags(write=False)
        return self._form


WAVE_GRID = 256 * 32  # develop_wave_kernel's most workgroups, one run of 64 pixels each
PIXEL_GRID = 256 * 16 * 256  # develop_kernel's most threads, one pixel each

CASES = [Case("one hot, %d bins" % b, lambda b=b: one_hot(b), forms=("pixel", "wave") if b <= 255 else ("pixel",)) for b in (1, 2, 3, 64, 127, 128, 129, 255, 256)] + [
    Case("one hot, 64 bins, step 30", lambda: one_hot(64), step=30.0),  # 14 steps of 30 nm: 420 nm of weight over a span of 400
    Case("one hot, 64 bins, filter", lambda: one_hot(64), filter=CURVE),
    Case("one hot, 64 bins, white", lambda: one_hot(64), white=WARM),
    Case("one hot, 64 bins, a white with a gap", lambda: one_hot(64, dim=(19, 20, 21, 22)), white=GAP),
    Case("one hot, 64 bins, filter and white", lambda: one_hot(64), filter=CURVE, white=WARM),
    Case("one hot, 64 bins, step 30, filter and white", lambda: one_hot(64), step=30.0, filter=CURVE, white=WARM),
    Case("one hot, 129 bins, two halves", lambda: one_hot(129), halves=True),
    Case("one hot, 7 bins, 400-700", lambda: one_hot(7), span=(400.0, 700.0)),  # no sample on an inner edge
    # the two lowest bins lie below the observer table's 360 nm: lit by its END VALUE alone (quarters of the span: exact)
    Case("one hot, 4 bins, 328-392", lambda: one_hot(4), span=(328.0, 392.0)),
    Case("one hot, 4 bins, 500-510, step 30", lambda: one_hot(4), span=(500.0, 510.0), step=30.0),  # a span narrower than one step
    Case("one hot, 16 bins, 500-516, step 0.5", lambda: one_hot(16), span=(500.0, 516.0), step=0.5),  # every other sample on an edge, k/32: exact
    # 5 bins put every inner edge at a fifth of the span, which no f32 quotient states exactly; 400-701 at step 2 keeps the
    # samples off them (edges at 400 + 60.2 m) and ends on an overshooting sample
    Case("random, 67x5x5, 400-701", lambda: random_film(67, 5, 5, 21), span=(400.0, 701.0)),
    Case("random, 130x3x64", lambda: random_film(130, 3, 64, 22)),
    Case("random, 130x3x64, step 30", lambda: random_film(130, 3, 64, 23), step=30.0),
    Case("random, 130x3x64, filter and white", lambda: random_film(130, 3, 64, 24), filter=CURVE, white=WARM),
    Case("random, 130x3x64, two halves", lambda: random_film(130, 3, 64, 25), halves=True),
    Case("random, 1x1x64", lambda: random_film(1, 1, 64, 26)),  # the film whose only pixel is the last: black
    # 8193 runs: one more than develop_wave_kernel's grid, so its run loop takes a second trip
    Case("long, 8193 runs of 64 pixels, 1 bin, step 30", lambda: long_film(WAVE_GRID + 1), step=30.0),
    # one run more than develop_kernel's threads (its grid stride takes a second trip): 16385 runs, a third trip of the wave form's
    Case("long, 16385 runs of 64 pixels, 1 bin, step 30", lambda: long_film(PIXEL_GRID // 64 + 1), step=30.0),
]
