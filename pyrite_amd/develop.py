"""Film development, the step after the hot path: developed pixel spectra -> CIE XYZ ->
sRGB, as pyrite/src/main.rs:190-238 (filter / white balance) and :315-418 (spectrum_to_xyz) do it, on the GPU through
`pyr_film_develop`. The image-settings programs (`filter`, `white`: project/mod.rs:111-118) only depend on the wavelength
(SpectrumSamplingInput, main.rs:470-476) and are evaluated here, once per sampling wavelength, in f32."""
from __future__ import annotations

import ctypes as C
import struct
import zlib

import numpy as np

from . import abi
from ._lib import check, lib
from .compiler import ProjectError, is_number, tables
from .film import Film

f32 = np.float32


def _array_get(data, mn, mx, w):
    """Spectrum::Array::get (project/spectra.rs:32-55) for one f32 wavelength."""
    n = len(data)
    if w <= mn:
        return f32(data[0])
    if w >= mx:
        return f32(data[-1])
    normalized = f32(f32(w - mn) / f32(mx - mn))
    fi = f32(normalized * f32(f32(n) - f32(1)))
    i0 = int(np.trunc(fi))
    mix = f32(fi - f32(np.trunc(fi)))
    return f32(f32(f32(data[i0]) * f32(f32(1) - mix)) + f32(f32(data[i0 + 1]) * mix))


def _curve_get(points, w):
    """Interpolated::get (math.rs:22-72): zero at and outside the end points."""
    pts = np.asarray(points, dtype=f32).reshape(-1, 2)
    if len(pts) == 0 or pts[0, 0] >= w or pts[-1, 0] <= w:
        return f32(0)
    lo, hi = 0, len(pts) - 1
    while hi > lo + 1:
        mid = (lo + hi) // 2
        if pts[mid, 0] == w:
            return f32(pts[mid, 1])
        if pts[mid, 0] > w:
            hi = mid
        else:
            lo = mid
    (x0, y0), (x1, y1) = pts[lo], pts[hi]
    return f32(y0 + f32(f32(y1 - y0) * f32(f32(w - x0) / f32(x1 - x0))))


def evaluate_at(expression, wavelength):
    """Value of a number expression at one wavelength, with the VM's f32 arithmetic (program/execution_context.rs:69-283).
    Only wavelength-dependent expressions are allowed here, as in the reference (main.rs:478-518)."""
    w = f32(wavelength)
    e = expression
    if is_number(e):
        return f32(e)
    t = e.type
    with np.errstate(all="ignore"):
        if t == "spectrum":
            name = e.get("name")
            if name is not None:
                tb = tables()
                return _array_get(tb[name], f32(tb["light_min"]), f32(tb["light_max"]), w)
            if e.get("format") == "array":
                return _array_get(np.asarray(e.points, dtype=f32), f32(e.min), f32(e.max), w)
            return _curve_get(e.points, w)
        if t == "blackbody":  # math.rs:177-182
            temperature = evaluate_at(e.temperature, w)
            wl = f32(w * f32(1.0e-9))
            a2 = f32(wl * wl)
            a4 = f32(a2 * a2)
            power = f32(f32(3.74183e-16) * f32(f32(1) / f32(wl * a4)))
            return f32(power / f32(f32(np.exp(np.float64(f32(f32(1.4388e-2) / f32(wl * temperature))))) - f32(1)))
        if t == "binary":
            l, r = evaluate_at(e.lhs, w), evaluate_at(e.rhs, w)
            return f32({"add": l + r, "sub": l - r, "mul": l * r, "div": l / r}[e.operator])
        if t == "mix":
            amount = min(max(evaluate_at(e.amount, w), f32(0)), f32(1))
            return f32(f32(evaluate_at(e.lhs, w) * f32(f32(1) - amount)) + f32(evaluate_at(e.rhs, w) * amount))
        if t == "clamp":
            return f32(max(min(evaluate_at(e.value, w), evaluate_at(e.max, w)), evaluate_at(e.min, w)))
    if t == "fresnel":
        raise ProjectError("the surface normal cannot be used while sampling a constant spectrum")
    raise ProjectError("cannot sample a %s expression as a spectrum" % t)


def sampling_wavelengths(film: Film, step_size):
    """wl_i of spectrum_to_tristimulus (main.rs:393-411): start at the span's minimum, add `step_size` in f32 while below the
    maximum; one more sample than steps."""
    lo, hi = f32(film.wavelength_start), f32(film.wavelength_start + film.wavelength_width)
    out = [lo]
    while out[-1] < hi:
        out.append(f32(out[-1] + f32(step_size)))
    return np.asarray(out, dtype=f32)


def develop_params(film: Film, step_size=2.0, filter=None, white=None):
    """PyrDevelopParams for `film` (+ the numpy arrays it borrows)."""
    tb = tables()
    wl = sampling_wavelengths(film, step_size)
    keep = {"xyz": np.ascontiguousarray(tb["xyz"], dtype=f32)}
    p = abi.PyrDevelopParams()
    p.step_size, p.xyz_scale, p.sample_count = float(step_size), 3.444, len(wl)
    p.xyz_table = keep["xyz"].ctypes.data_as(C.POINTER(C.c_float))
    p.xyz_count, p.xyz_min, p.xyz_max = len(keep["xyz"]), float(tb["xyz_min"]), float(tb["xyz_max"])
    if filter is not None:  # main.rs:197-202
        keep["filter"] = np.asarray([evaluate_at(filter, w) for w in wl], dtype=f32)
        p.filter = keep["filter"].ctypes.data_as(C.POINTER(C.c_float))
    if white is not None:  # main.rs:204-222
        w, hi = f32(film.wavelength_start), f32(film.wavelength_start + film.wavelength_width)
        mx, d65_mx = f32(0), f32(0)
        while w < hi:
            mx = max(mx, evaluate_at(white, w))
            d65_mx = max(d65_mx, _array_get(tb["d65"], f32(tb["light_min"]), f32(tb["light_max"]), w))
            w = f32(w + f32(1.0))
        keep["white_div"] = np.asarray([max(f32(evaluate_at(white, x) / mx), f32(0.000001)) for x in wl], dtype=f32)
        keep["white_mul"] = np.asarray([f32(_array_get(tb["d65"], f32(tb["light_min"]), f32(tb["light_max"]), x) / d65_mx) for x in wl], dtype=f32)
        p.white_div = keep["white_div"].ctypes.data_as(C.POINTER(C.c_float))
        p.white_mul = keep["white_mul"].ctypes.data_as(C.POINTER(C.c_float))
    return p, keep


def develop(film: Film, step_size=2.0, filter=None, white=None, device=0):
    """uint8 [height, width, 3] sRGB image of `film`, developed on the GPU."""
    p, keep = develop_params(film, step_size, filter, white)
    desc = film.desc()
    grains = np.ascontiguousarray(film.grains)
    out = np.zeros((film.height, film.width, 3), dtype=np.uint8)
    check(lib().pyr_film_develop(C.byref(desc), grains.ctypes.data, C.byref(p), out.ctypes.data, int(device)))
    del keep
    return out


def save_png(path, rgb):
    """Minimal PNG writer (8-bit RGB, no interlace) -- the image::save of main.rs:327."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w, _ = rgb.shape
    raw = b"".join(b"\x00" + rgb[y].tobytes() for y in range(h))

    def chunk(tag, data):
        body = tag + data
        return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


# ---------------------------------------------------------------------------------------------- linear images and tone mapping
SPACES = {"xyz": abi.PYR_LINEAR_XYZ, "srgb": abi.PYR_LINEAR_SRGB}
TONE_OPS = {"clip": abi.PYR_TONE_CLIP, "reinhard": abi.PYR_TONE_REINHARD}


def develop_linear(film: Film, space="srgb", film_b: Film = None, step_size=2.0, filter=None, white=None, device=0):
    """float32 [height, width, 3]: `film` (plus `film_b`, grain by grain, when given) developed on the GPU to CIE XYZ or to the
    linear sRGB triple that `develop` clamps and encodes (pyr_film_develop_linear)."""
    p, keep = develop_params(film, step_size, filter, white)
    desc = film.desc()
    grains = np.ascontiguousarray(film.grains)
    grains_b = None
    if film_b is not None:
        assert film_b.grains.shape == film.grains.shape
        grains_b = np.ascontiguousarray(film_b.grains)
    out = np.zeros((film.height, film.width, 3), dtype=np.float32)
    check(lib().pyr_film_develop_linear(C.byref(desc), grains.ctypes.data, grains_b.ctypes.data if grains_b is not None else None, C.byref(p),
                                        SPACES[space], out.ctypes.data, int(device)))
    del keep
    return out


def _linear_image(rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    assert rgb.ndim == 3 and rgb.shape[2] == 3
    return rgb


def image_stats(rgb, device=0):
    """abi.PyrImageStats of a linear sRGB image: the luminance histogram (8 bins per octave over 2^-16 .. 2^16), the lit and dark
    pixel counts, the extremes of the lit luminance (pyr_image_stats). Integer counters: the same bits on every call."""
    rgb = _linear_image(rgb)
    out = abi.PyrImageStats()
    check(lib().pyr_image_stats(rgb.ctypes.data, rgb.shape[1], rgb.shape[0], C.byref(out), int(device)))
    return out


def tone_params(op="clip", exposure=None, white=None, key=abi.PYR_TONE_KEY, percentile=abi.PYR_TONE_PERCENTILE, white_percentile=abi.PYR_TONE_WHITE_PERCENTILE):
    """abi.PyrToneParams: `exposure` is a factor on the linear values, `white` the exposed luminance that Reinhard's curve takes to
    1; None or "auto" leaves either to the image's statistics."""
    automatic = (None, "auto")
    return abi.PyrToneParams(TONE_OPS[op] if isinstance(op, str) else int(op), 0.0 if exposure in automatic else float(exposure),
                             0.0 if white in automatic else float(white), float(key), float(percentile), float(white_percentile))


def tone_resolve(stats, tone):
    """(exposure, white) that `tone` stands for on an image with these statistics (pyr_tone_resolve: host arithmetic, no device)."""
    exposure, white = C.c_float(0), C.c_float(0)
    check(lib().pyr_tone_resolve(C.byref(stats) if stats is not None else None, C.byref(tone), C.byref(exposure), C.byref(white)))
    return float(exposure.value), float(white.value)


def tonemap(rgb, tone=None, stats=None, device=0):
    """uint8 [height, width, 3] sRGB of a linear sRGB image under `tone` (tone_params; default: the clip at exposure 1, which is
    `develop`'s image). What `tone` leaves automatic is resolved from `stats`, taken on the GPU here when not given."""
    rgb = _linear_image(rgb)
    tone = tone_params(exposure=1.0) if tone is None else tone
    needs_stats = not tone.exposure > 0 or (tone.op == abi.PYR_TONE_REINHARD and not tone.white > 0)
    if needs_stats and stats is None:
        stats = image_stats(rgb, device)
    exposure, white = tone_resolve(stats, tone)
    resolved = abi.PyrToneParams(tone.op, exposure, white, tone.key, tone.percentile, tone.white_percentile)
    out = np.zeros(rgb.shape, dtype=np.uint8)
    check(lib().pyr_image_tonemap(rgb.ctypes.data, rgb.shape[1], rgb.shape[0], C.byref(resolved), out.ctypes.data, int(device)))
    return out


# ---------------------------------------------------------------------------------------------- denoising
def denoise_params(radius=abi.PYR_DENOISE_RADIUS, patch=abi.PYR_DENOISE_PATCH, k=abi.PYR_DENOISE_K, epsilon=abi.PYR_DENOISE_EPSILON,
                   sigma_albedo=abi.PYR_DENOISE_SIGMA_ALBEDO, sigma_normal=abi.PYR_DENOISE_SIGMA_NORMAL, sigma_depth=abi.PYR_DENOISE_SIGMA_DEPTH):
    """abi.PyrDenoiseParams: the window is (2*radius+1)^2 pixels, the patch (2*patch+1)^2; a sigma <= 0 turns that guide off."""
    return abi.PyrDenoiseParams(int(radius), int(patch), float(k), float(epsilon), float(sigma_albedo), float(sigma_normal), float(sigma_depth), 0)


def denoise(a, b, albedo=None, pixels=None, device=0, **params):
    """(image, error), float32 [height, width, 3] each: the two half images `a` and `b` (linear light, independent samples of one
    picture) cross filtered on the GPU (pyr_image_denoise; include/pyrite_gpu.h has the arithmetic) and the noise that is left.
    Guides: `albedo`, a linear image, and `pixels`, the records of the feature pass (Features.records). `params`: denoise_params."""
    a, b = _linear_image(a), _linear_image(b)
    assert a.shape == b.shape
    h, w, _ = a.shape
    if albedo is not None:
        albedo = _linear_image(albedo)
        assert albedo.shape == a.shape
    if pixels is not None:
        pixels = np.ascontiguousarray(pixels)
        assert pixels.nbytes == h * w * C.sizeof(abi.PyrFeaturePixel)
    p = denoise_params(**params)
    out, error = np.zeros(a.shape, dtype=np.float32), np.zeros(a.shape, dtype=np.float32)
    check(lib().pyr_image_denoise(a.ctypes.data, b.ctypes.data, _ptr(albedo), _ptr(pixels), w, h, C.byref(p), out.ctypes.data, error.ctypes.data, int(device)))
    return out, error


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _frame_and_history(current, motion, history, history_motion, history_count):
    """What reproject and resolve are given, as the library reads it: (current, motion, history, history_motion, history_count,
    height, width), contiguous, of the right types and sizes, the history all None or all given."""
    current = _linear_image(current)
    h, w, _ = current.shape
    records = C.sizeof(abi.PyrMotionPixel) * h * w
    motion = np.ascontiguousarray(motion)
    assert motion.nbytes == records
    given = [x is not None for x in (history, history_motion, history_count)]
    if any(given):
        if not all(given):
            raise ValueError("history, history_motion and history_count go together")
        history, history_motion = _linear_image(history), np.ascontiguousarray(history_motion)
        history_count = np.ascontiguousarray(history_count, dtype=np.float32)
        assert history.shape == current.shape and history_motion.nbytes == records and history_count.shape == (h, w)
    return current, motion, history, history_motion, history_count, h, w


def reproject(current, motion, history=None, history_motion=None, history_count=None, depth_tolerance=abi.PYR_REPROJECT_DEPTH_TOLERANCE,
              max_history=abi.PYR_REPROJECT_MAX_HISTORY, device=0):
    """(out, count): the running mean of linear images over frames of a moving scene (pyr_image_reproject; include/pyrite_gpu.h has
    the arithmetic). `current`: this frame, float32 [height, width, 3]; `motion`: its records (Renderer.motion, motion.RECORD
    [height, width]). `history`, `history_motion`, `history_count`: the previous call's `out`, the records of that frame and its
    `count` -- all None for a first frame. `count` [height, width] float32 is the number of frames a pixel's mean holds; a pixel
    whose surface was hidden a frame ago starts again at 1."""
    current, motion, history, history_motion, history_count, h, w = _frame_and_history(current, motion, history, history_motion, history_count)
    p = abi.PyrReprojectParams(float(depth_tolerance), float(max_history))
    out, count = np.zeros(current.shape, dtype=np.float32), np.zeros((h, w), dtype=np.float32)
    check(lib().pyr_image_reproject(current.ctypes.data, motion.ctypes.data, _ptr(history), _ptr(history_motion), _ptr(history_count), w, h, C.byref(p), out.ctypes.data,
                                    count.ctypes.data, int(device)))
    return out, count


def temporal_params(depth_tolerance=abi.PYR_REPROJECT_DEPTH_TOLERANCE, max_history=abi.PYR_REPROJECT_MAX_HISTORY, radius=abi.PYR_TEMPORAL_RADIUS,
                    gamma=abi.PYR_TEMPORAL_GAMMA, noise_scale=abi.PYR_TEMPORAL_NOISE_SCALE, response=abi.PYR_TEMPORAL_RESPONSE):
    """abi.PyrTemporalParams: the reprojection's `depth_tolerance` and `max_history`; the history is clipped to mean +- (`gamma`
    standard deviations + `noise_scale` times the noise image) of the (2 radius + 1)^2 neighbourhood of the current frame, and a
    pixel clipped by r half-widths of that box keeps 1 / (1 + `response` r) of its count."""
    return abi.PyrTemporalParams(float(depth_tolerance), float(max_history), int(radius), float(gamma), float(noise_scale), float(response))


def resolve(current, motion, history=None, history_motion=None, history_count=None, noise=None, device=0, **params):
    """(image, count, clip): reproject's running mean with the fetched history clipped to the neighbourhood of `current`, so that
    light which changes on a surface that stays -- a shadow that moves on -- leaves no trail (pyr_image_temporal_resolve;
    include/pyrite_gpu.h has the arithmetic). The arguments are reproject's; `noise`, optional, is the error image of `denoise` for
    the frame `current` shows and widens the clip box. `params`: temporal_params. `clip` [height, width] float32 says how far
    outside the box each pixel's history lay, 0 where it was kept as it was: there `image` and `count` are reproject's."""
    current, motion, history, history_motion, history_count, h, w = _frame_and_history(current, motion, history, history_motion, history_count)
    if noise is not None:
        noise = _linear_image(noise)
        assert noise.shape == current.shape
    p = temporal_params(**params)
    out, count, clip = np.zeros(current.shape, dtype=np.float32), np.zeros((h, w), dtype=np.float32), np.zeros((h, w), dtype=np.float32)
    check(lib().pyr_image_temporal_resolve(current.ctypes.data, motion.ctypes.data, _ptr(noise), _ptr(history), _ptr(history_motion), _ptr(history_count), w, h, C.byref(p),
                                           out.ctypes.data, count.ctypes.data, clip.ctypes.data, int(device)))
    return out, count, clip


def motion_blur_params(shutter=abi.PYR_MOTION_BLUR_SHUTTER, samples=abi.PYR_MOTION_BLUR_SAMPLES, max_radius=abi.PYR_MOTION_BLUR_MAX_RADIUS,
                       depth_softness=abi.PYR_MOTION_BLUR_DEPTH_SOFTNESS, seed=0):
    """abi.PyrMotionBlurParams: the shutter is open for `shutter` of the frame interval, a moving pixel takes `samples` taps along a
    blur of at most `max_radius` pixels to either side, depths within `depth_softness` (relative) count as one surface."""
    return abi.PyrMotionBlurParams(float(shutter), int(samples), int(max_radius), float(depth_softness), int(seed) & 0xFFFFFFFF)


def motion_blur(image, motion, device=0, **params):
    """float32 [height, width, 3]: the linear image `image` blurred along its motion records (pyr_image_motion_blur;
    include/pyrite_gpu.h has the arithmetic). `motion`: the records of the frame the image shows (Renderer.motion, motion.RECORD
    [height, width]) against the previous frame. `params`: motion_blur_params. Pixels that nothing moves near keep their bits."""
    image = _linear_image(image)
    h, w, _ = image.shape
    motion = np.ascontiguousarray(motion)
    assert motion.nbytes == C.sizeof(abi.PyrMotionPixel) * h * w
    p = motion_blur_params(**params)
    out = np.zeros(image.shape, dtype=np.float32)
    check(lib().pyr_image_motion_blur(image.ctypes.data, motion.ctypes.data, w, h, C.byref(p), out.ctypes.data, int(device)))
    return out


def lens_blur_params(camera=None, focus_distance=None, aperture=None, view_plane=None, max_radius=abi.PYR_LENS_BLUR_MAX_RADIUS,
                     depth_tolerance=abi.PYR_REPROJECT_DEPTH_TOLERANCE):
    """abi.PyrLensBlurParams: a thin lens of `aperture` (the lens disc's radius squared, as the project file has it) focused at
    `focus_distance` before a camera of `view_plane`; circles of confusion are clamped to `max_radius` pixels, and depths within
    `depth_tolerance` (relative) count as one layer. With `camera` (a renderer.Camera or an abi.PyrCamera) the three lens numbers
    are read from it, each unless given; without one all three must be given."""
    c = getattr(camera, "c", camera)
    given = {"focus_distance": focus_distance, "aperture": aperture, "view_plane": view_plane}
    for name, value in given.items():
        if value is None:
            if c is None:
                raise ValueError("lens_blur_params: %s is needed without a camera" % name)
            given[name] = getattr(c, name)
    return abi.PyrLensBlurParams(float(given["focus_distance"]), float(given["aperture"]), float(given["view_plane"]), int(max_radius), float(depth_tolerance))


def lens_blur(image, pixels, device=0, **params):
    """float32 [height, width, 3]: the linear image `image`, rendered through a pinhole, blurred as a thin lens would blur it
    (pyr_image_lens_blur; include/pyrite_gpu.h has the arithmetic). `pixels`: the feature records of the same camera at the same
    size (Features.records). `params`: lens_blur_params. Pixels in focus that no neighbour's blur reaches keep their bits."""
    image = _linear_image(image)
    h, w, _ = image.shape
    pixels = np.ascontiguousarray(pixels)
    assert pixels.nbytes == C.sizeof(abi.PyrFeaturePixel) * h * w
    p = lens_blur_params(**params)
    out = np.zeros(image.shape, dtype=np.float32)
    check(lib().pyr_image_lens_blur(image.ctypes.data, pixels.ctypes.data, w, h, C.byref(p), out.ctypes.data, int(device)))
    return out


def lens_blur_flag_problem(lens_blur, lens_blur_radius):
    """What is wrong with --lens-blur / --lens-blur-radius R, in the words pyrite_host_tool uses too, or None."""
    if not lens_blur:
        return "--lens-blur-radius needs --lens-blur" if lens_blur_radius is not None else None
    if lens_blur_radius is not None and not 1 <= lens_blur_radius <= abi.PYR_LENS_BLUR_MOST_RADIUS:
        return "--lens-blur-radius must be 1 to %d" % abi.PYR_LENS_BLUR_MOST_RADIUS
    return None


def glare_params(strength=abi.PYR_GLARE_STRENGTH, levels=abi.PYR_GLARE_LEVELS, threshold=abi.PYR_GLARE_THRESHOLD, falloff=abi.PYR_GLARE_FALLOFF):
    """abi.PyrGlareParams: `strength` of every pixel's light (of what lies above the luminance `threshold`, when that is not 0) is
    spread over `levels` blurs, each twice as wide as the one before and weighted `falloff` times as much."""
    return abi.PyrGlareParams(float(strength), int(levels), float(threshold), float(falloff))


def glare(image, device=0, **params):
    """float32 [height, width, 3]: the linear image `image` with the glare of a lens or an eye added -- a long-tailed point spread
    that moves light from the bright pixels to their surroundings (pyr_image_glare; include/pyrite_gpu.h has the arithmetic).
    `params`: glare_params. A pixel that is not finite keeps its bits and spreads nothing."""
    image = _linear_image(image)
    h, w, _ = image.shape
    p = glare_params(**params)
    out = np.zeros(image.shape, dtype=np.float32)
    check(lib().pyr_image_glare(image.ctypes.data, w, h, C.byref(p), out.ctypes.data, int(device)))
    return out


def glare_flag_problem(glare, glare_levels, glare_threshold):
    """What is wrong with --glare / --glare-levels / --glare-threshold, in the words pyrite_host_tool uses too, or None. `glare`:
    the strength as given (a string or a number), or None without --glare."""
    if glare is None:
        if glare_levels is not None:
            return "--glare-levels needs --glare"
        if glare_threshold is not None:
            return "--glare-threshold needs --glare"
        return None
    try:
        strength = float(glare)
    except ValueError:
        strength = float("nan")
    if not 0.0 < strength <= 1.0:
        return "--glare must be a strength above 0 and at most 1"
    if glare_levels is not None and not 1 <= glare_levels <= abi.PYR_GLARE_MOST_LEVELS:
        return "--glare-levels must be 1 to %d" % abi.PYR_GLARE_MOST_LEVELS
    if glare_threshold is not None and not (np.isfinite(glare_threshold) and glare_threshold >= 0.0):
        return "--glare-threshold must be a finite number that is not negative"
    return None


def glare_from_flags(glare, glare_levels, glare_threshold):
    """The glare_params keywords of --glare [STRENGTH] --glare-levels N --glare-threshold T, or None without --glare."""
    if glare is None:
        return None
    params = {"strength": float(glare)}
    if glare_levels is not None:
        params["levels"] = glare_levels
    if glare_threshold is not None:
        params["threshold"] = glare_threshold
    return params


def upsample_params(radius=abi.PYR_UPSAMPLE_RADIUS, match_material=True, sigma_normal=abi.PYR_UPSAMPLE_SIGMA_NORMAL, sigma_depth=abi.PYR_UPSAMPLE_SIGMA_DEPTH,
                    albedo_floor=abi.PYR_UPSAMPLE_ALBEDO_FLOOR, max_gain=abi.PYR_UPSAMPLE_MAX_GAIN, flags=None):
    """abi.PyrUpsampleParams: (2*radius)^2 taps under a tent of that radius; a sigma <= 0 turns that guide off; `match_material`
    sets PYR_UPSAMPLE_MATCH_MATERIAL (`flags`, when given, is the whole flag word instead)."""
    word = (abi.PYR_UPSAMPLE_MATCH_MATERIAL if match_material else 0) if flags is None else int(flags)
    return abi.PyrUpsampleParams(int(radius), word, float(sigma_normal), float(sigma_depth), float(albedo_floor), float(max_gain))


def upsample(low, scale, albedo=None, pixels=None, low_albedo=None, low_pixels=None, device=0, **params):
    """float32 [scale*height, scale*width, 3]: the linear image `low`, [height, width, 3], upsampled on the GPU under the guidance
    of full-size feature images (pyr_image_upsample; include/pyrite_gpu.h has the arithmetic). The albedo pair -- `low_albedo` of
    low's size, `albedo` of the result's, linear images -- demodulates, so that texture detail comes back at full size; the records
    pair -- `low_pixels`, `pixels`, the records of the two feature passes (Features.records) -- keeps the taps on the pixel's own
    surface. Each pair is given whole or not at all. `params`: upsample_params."""
    low = _linear_image(low)
    h, w, _ = low.shape
    scale = int(scale)
    if (albedo is None) != (low_albedo is None):
        raise ValueError("albedo and low_albedo go together")
    if (pixels is None) != (low_pixels is None):
        raise ValueError("pixels and low_pixels go together")
    if albedo is not None:
        albedo, low_albedo = _linear_image(albedo), _linear_image(low_albedo)
        assert low_albedo.shape == low.shape and albedo.shape == (h * scale, w * scale, 3)
    if pixels is not None:
        pixels, low_pixels = np.ascontiguousarray(pixels), np.ascontiguousarray(low_pixels)
        assert low_pixels.nbytes == h * w * C.sizeof(abi.PyrFeaturePixel) and pixels.nbytes == low_pixels.nbytes * scale * scale
    p = upsample_params(**params)
    sized = min(max(scale, 1), abi.PYR_UPSAMPLE_MOST_SCALE)  # a scale the library refuses never writes
    out = np.zeros((h * sized, w * sized, 3), dtype=np.float32)
    check(lib().pyr_image_upsample(low.ctypes.data, _ptr(low_albedo), _ptr(low_pixels), w, h, scale, _ptr(albedo), _ptr(pixels), C.byref(p), out.ctypes.data, int(device)))
    return out


def upsample_flag_problem(upsample, upsample_radius, size=None):
    """What is wrong with --upsample N / --upsample-radius R, in the words pyrite_host_tool uses too, or None. `size`: the image's
    (width, height) once the project is loaded -- N must divide both."""
    if upsample is None:
        return "--upsample-radius needs --upsample" if upsample_radius is not None else None
    if not 2 <= upsample <= abi.PYR_UPSAMPLE_MOST_SCALE:
        return "--upsample must be 2 to %d" % abi.PYR_UPSAMPLE_MOST_SCALE
    if upsample_radius is not None and not 1 <= upsample_radius <= abi.PYR_UPSAMPLE_MOST_RADIUS:
        return "--upsample-radius must be 1 to %d" % abi.PYR_UPSAMPLE_MOST_RADIUS
    if size is not None and (size[0] % upsample or size[1] % upsample):
        return "--upsample %d does not divide the image size %dx%d" % (upsample, size[0], size[1])
    return None


def upsample_from_flags(upsample, upsample_radius):
    """The upsample_params keywords of --upsample N --upsample-radius R, or None without --upsample."""
    if upsample is None:
        return None
    return {"radius": upsample_radius} if upsample_radius is not None else {}


def despeckle_params(radius=abi.PYR_DESPECKLE_RADIUS, k=abi.PYR_DESPECKLE_K, relative=abi.PYR_DESPECKLE_RELATIVE, floor=abi.PYR_DESPECKLE_FLOOR, flags=0):
    """abi.PyrDespeckleParams: a pixel is a firefly when it lies more than `k` spreads above the median of its (2*radius+1)^2
    window; the spread is the scaled median deviation, at least `relative` times the median and at least `floor`."""
    return abi.PyrDespeckleParams(int(radius), float(k), float(relative), float(floor), int(flags))


def despeckle(a, b=None, device=0, **params):
    """(a_out, b_out, removed, counts) -- or (a_out, removed, counts) without `b` -- the half images `a` and `b` (linear light,
    independent samples of one picture) with their fireflies clamped on the GPU (pyr_image_despeckle; include/pyrite_gpu.h has the
    arithmetic): a pixel far above the median of its neighbourhood in one half and not in the other lands on the limit, its hue
    kept; everything else keeps its bits. `removed`: float32 [height, width, 3], what the mean of the halves lost; `counts`: the
    pixels clamped in a and in b. Without `b` one image is filtered and bright edges lose pixels too. `params`: despeckle_params."""
    a = _linear_image(a)
    h, w, _ = a.shape
    if b is not None:
        b = _linear_image(b)
        assert b.shape == a.shape
    p = despeckle_params(**params)
    a_out, removed = np.zeros(a.shape, dtype=np.float32), np.zeros(a.shape, dtype=np.float32)
    b_out = np.zeros(a.shape, dtype=np.float32) if b is not None else None
    counts = np.zeros(2, dtype=np.uint32)
    check(lib().pyr_image_despeckle(a.ctypes.data, _ptr(b), w, h, C.byref(p), a_out.ctypes.data, _ptr(b_out), removed.ctypes.data, counts.ctypes.data, int(device)))
    counts = (int(counts[0]), int(counts[1]))
    return (a_out, b_out, removed, counts) if b is not None else (a_out, removed, counts)


def despeckle_flag_problem(despeckle, despeckle_radius, pixel_samples=None, pass_samples=None):
    """What is wrong with --despeckle [K] / --despeckle-radius R, in the words pyrite_host_tool uses too, or None. `despeckle`: K as
    it was given (a string or a number), or None without --despeckle; `pixel_samples`: the render's budget once the project is
    loaded; `pass_samples`: --pass-samples, when given."""
    if despeckle is None:
        return "--despeckle-radius needs --despeckle" if despeckle_radius is not None else None
    try:
        k = float(despeckle)
    except ValueError:
        k = float("nan")
    if not (np.isfinite(k) and k > 0.0):
        return "--despeckle must be a finite number above 0"
    if despeckle_radius is not None and not 1 <= despeckle_radius <= abi.PYR_DESPECKLE_MOST_RADIUS:
        return "--despeckle-radius must be 1 to %d" % abi.PYR_DESPECKLE_MOST_RADIUS
    if pixel_samples is not None and pixel_samples % 2:
        return "--despeckle needs an even number of samples per pixel: the two half films must be equal"
    if pixel_samples is not None and pass_samples and pixel_samples % (2 * pass_samples):
        return "--despeckle needs an even number of equal passes: the samples per pixel must be a multiple of twice --pass-samples"
    return None


def despeckle_from_flags(despeckle, despeckle_radius):
    """The despeckle_params keywords of --despeckle [K] --despeckle-radius R, or None without --despeckle."""
    if despeckle is None:
        return None
    params = {"k": float(despeckle)}
    if despeckle_radius is not None:
        params["radius"] = despeckle_radius
    return params


def denoise_flag_problem(denoise, denoise_radius, pixel_samples=None, pass_samples=None):
    """What is wrong with --denoise / --denoise-radius, in the words pyrite_host_tool uses too, or None. `pixel_samples`: the
    render's budget once the project is loaded; `pass_samples`: --pass-samples, when given."""
    if denoise_radius is not None and not denoise:
        return "--denoise-radius needs --denoise"
    if denoise_radius is not None and not 1 <= denoise_radius <= abi.PYR_DENOISE_MAX_RADIUS:
        return "--denoise-radius must be 1 to %d" % abi.PYR_DENOISE_MAX_RADIUS
    if denoise and pixel_samples is not None and pixel_samples % 2:
        return "--denoise needs an even number of samples per pixel: the two half films must be equal"
    if denoise and pixel_samples is not None and pass_samples and pixel_samples % (2 * pass_samples):
        return "--denoise needs an even number of equal passes: the samples per pixel must be a multiple of twice --pass-samples"
    return None


RGBE_MAX = 255.0 * 2.0 ** 119  # the largest value a Radiance pixel holds: mantissa 255, exponent byte 255


def encode_hdr(rgb):
    """The bytes of a Radiance picture of a linear image: flat scanlines of RGBE pixels, no run-length coding. Ward's mapping, in
    f64 (pyrite_host.hpp encode_hdr writes the same bytes): a channel that is not positive (negative, NaN) is 0, one above RGBE_MAX
    (+inf too) is RGBE_MAX; m = the largest channel; m < 1e-32: four zero bytes; else m = f * 2^e with f in [0.5, 1), the mantissa
    bytes are (uint8)(c * (f * 256 / m)) and the exponent byte is e + 128."""
    rgb = _linear_image(rgb)
    h, w, _ = rgb.shape
    with np.errstate(all="ignore"):
        c = np.where(rgb > 0, rgb, np.float32(0)).astype(np.float64)
        c = np.minimum(c, RGBE_MAX)
        m = c.max(axis=2)
        some = m >= 1e-32
        f, e = np.frexp(np.where(some, m, 1.0))
        scale = f * 256.0 / np.where(some, m, 1.0)
        pixels = np.zeros((h, w, 4), dtype=np.uint8)
        pixels[..., :3] = np.where(some[..., None], c * scale[..., None], 0.0).astype(np.uint8)
        pixels[..., 3] = np.where(some, e + 128, 0).astype(np.uint8)
    return b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w) + pixels.tobytes()


def encode_pfm(rgb):
    """The bytes of a colour PFM file: little-endian f32 as they are, rows bottom to top."""
    rgb = _linear_image(rgb)
    h, w, _ = rgb.shape
    return b"PF\n%d %d\n-1.0\n" % (w, h) + rgb[::-1].astype("<f4").tobytes()


def save_hdr(path, rgb):
    with open(path, "wb") as f:
        f.write(encode_hdr(rgb))


def save_pfm(path, rgb):
    with open(path, "wb") as f:
        f.write(encode_pfm(rgb))


def tone_flag_problem(hdr, exposure, tone):
    """What is wrong with --hdr / --exposure / --tone, in the words pyrite_host_tool uses too, or None."""
    if hdr is not None and not hdr.lower().endswith((".hdr", ".pfm")):
        return "--hdr must end in .hdr or .pfm"
    if exposure is not None and exposure != "auto":
        try:
            ok = np.isfinite(float(exposure))
        except ValueError:
            ok = False
        if not ok:
            return "--exposure must be a number of stops or auto"
    if tone is not None and tone not in TONE_OPS:
        return "--tone must be clip or reinhard"
    return None


def tone_from_flags(exposure, tone):
    """The PyrToneParams of --exposure EV|auto and --tone clip|reinhard, or None when neither is given: EV is stops (a factor of
    2^EV), --tone reinhard alone means --exposure auto, --exposure alone means --tone clip."""
    if exposure is None and tone is None:
        return None
    op = tone or "clip"
    if exposure is None:
        exposure = "auto" if op == "reinhard" else "0"
    return tone_params(op, None if exposure == "auto" else f32(2.0 ** float(exposure)))


def save_linear(path, rgb):
    """--hdr PATH: .hdr or .pfm by the extension."""
    (save_pfm if path.lower().endswith(".pfm") else save_hdr)(path, rgb)
