"""Linear images and tone mapping on the GPU (include/pyrite_gpu.h "linear images and tone mapping"): the linear sRGB image is what
the 8-bit development encodes, byte for byte; XYZ and linear sRGB against a numpy f32 restatement of the trapezoid walk; two half
films develop as their sum; the luminance statistics are exact; Reinhard's curve against its f32 restatement; a real picture that
the 8-bit path clips; the _device forms on tensors and a stream of the caller's against the host forms, byte for byte; and the
argument checks, none of which reaches a kernel."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from pyrite_amd import abi, scenes
from pyrite_amd._lib import check, lib
from pyrite_amd.compiler import tables
from pyrite_amd.develop import (_array_get, develop, develop_linear, develop_params, encode_hdr, image_stats, tone_params, tone_resolve, tonemap)
from pyrite_amd.film import Film
from pyrite_amd.project import blackbody, spectrum
from test_tone_cpu import check_hdr_round_trip

pytestmark = pytest.mark.gpu

f32 = np.float32
TOL = 1e-5  # DESIGN.md section 4, the project's parity tolerance: here relative to the pixel's largest channel magnitude
OBSERVED = {}

# (width, height, bins): odd bins and an odd pixel count (the lone last grain, a ragged last run); more than one full run at the
# contract's 64 bins; more bins than the wave form's LDS rows hold (the thread-per-pixel form); the film whose only pixel is the last
FILMS = [(67, 5, 5), (130, 3, 64), (9, 2, 300), (1, 1, 64)]
SETTINGS = [
    {"step_size": 2.0},
    {"step_size": 30.0},
    {"step_size": 2.0, "filter": spectrum(format="curve", points=[(450, 0), (500, 1), (600, 1), (650, 0)]), "white": blackbody(4000)},
    {"step_size": 30.0, "filter": spectrum(format="curve", points=[(450, 0), (500, 1), (600, 1), (650, 0)]), "white": blackbody(4000)},
]


def random_film(width, height, bins, seed):
    """Seeded grains: weights are sample counts, about one in ten zero; acc / weight spans 1e-4 .. 1e3."""
    rng = np.random.default_rng(seed)
    film = Film(width, height, bins)
    weight = rng.integers(1, 65, size=(height, width, bins)).astype(f32)
    weight[rng.random((height, width, bins)) < 0.1] = 0
    film.grains[..., 1] = weight
    film.grains[..., 0] = weight * np.power(10.0, rng.uniform(-4, 3, size=(height, width, bins))).astype(f32)
    return film


def restate_linear(film, step_size=2.0, filter=None, white=None):
    """(xyz, rgb) float32 [height, width, 3]: develop_kernel's trapezoid walk for every pixel at once, numpy f32, one rounding per
    operation."""
    p, keep = develop_params(film, step_size, filter, white)
    tb = tables()
    observer, xyz_min, xyz_max = np.asarray(tb["xyz"], dtype=f32), f32(tb["xyz_min"]), f32(tb["xyz_max"])
    spectra = film.develop().reshape(-1, film.bins)
    lo = f32(film.wavelength_start)
    hi = f32(lo + f32(film.wavelength_width))
    step, count, bins = f32(step_size), int(p.sample_count), film.bins

    def xyz_get(w):
        return [_array_get(observer[:, c], xyz_min, xyz_max, w) for c in range(3)]

    def sample(w, i):
        if w < lo or w > hi:
            intensity = np.zeros(len(spectra), dtype=f32)
        else:
            normalized = f32(f32(w - lo) / f32(hi - lo))
            index = int(min(np.floor(f32(normalized * f32(bins))), f32(bins - 1)))
            intensity = spectra[:, index]
        if "filter" in keep:
            intensity = intensity * keep["filter"][i]
        if "white_div" in keep:
            intensity = (intensity / keep["white_div"][i]) * keep["white_mul"][i]
        return intensity

    with np.errstate(all="ignore"):
        total = [np.zeros(len(spectra), dtype=f32) for _ in range(3)]
        weight, wl_min, i = f32(0), lo, 0
        spectrum_min, start = sample(wl_min, 0), xyz_get(wl_min)
        while wl_min < hi:
            wl_max = f32(wl_min + step)
            i += 1
            spectrum_max, end = sample(wl_max, min(i, count - 1)), xyz_get(wl_max)
            w = f32(wl_max - wl_min)
            for c in range(3):
                total[c] = total[c] + ((start[c] * spectrum_min + end[c] * spectrum_max) * f32(0.5)) * w
            weight = f32(weight + w)
            wl_min, spectrum_min, start = wl_max, spectrum_max, end
        x, y, z = [(t if weight == 0 else t / weight) * f32(p.xyz_scale) for t in total]
        rgb = [f32(3.2404542) * x + f32(-1.5371385) * y + f32(-0.4985314) * z,
               f32(-0.9692660) * x + f32(1.8760108) * y + f32(0.0415560) * z,
               f32(0.0556434) * x + f32(-0.2040259) * y + f32(1.0572252) * z]
    xyz, rgb = np.stack([x, y, z], axis=-1), np.stack(rgb, axis=-1)
    xyz[-1], rgb[-1] = 0, 0  # the film's last pixel is never developed (film.rs:299)
    assert xyz.dtype == rgb.dtype == f32
    shape = (film.height, film.width, 3)
    return xyz.reshape(shape), rgb.reshape(shape)


def case_name(setting):
    return "step %g%s" % (setting["step_size"], ", filter + white" if "filter" in setting else "")


# ------------------------------------------------------------------------------------------------ 1. linear is what the 8-bit path encodes
@pytest.mark.parametrize("shape", FILMS, ids=lambda s: "%dx%dx%d" % s)
def test_clipping_the_linear_image_gives_the_developed_bytes(shape, gpu_lib):
    film = random_film(*shape, seed=11)
    clip = tone_params("clip", exposure=1.0)
    for setting in SETTINGS:
        linear = develop_linear(film, "srgb", **setting)
        assert linear.shape == (film.height, film.width, 3) and linear.dtype == f32
        assert np.array_equal(tonemap(linear, clip), develop(film, **setting)), case_name(setting)
        assert np.array_equal(tonemap(linear), develop(film, **setting))  # the default tone is that clip
        assert (linear[-1, -1] == 0).all()
        if shape != (1, 1, 64):
            assert linear.max() > 1.0 and np.isfinite(linear).all()  # the film is brighter than 8 bits hold


# ------------------------------------------------------------------------------------------------ 2. against the restatement
@pytest.mark.parametrize("shape", FILMS, ids=lambda s: "%dx%dx%d" % s)
def test_linear_values_match_the_restatement(shape, gpu_lib):
    film = random_film(*shape, seed=12)
    for setting in SETTINGS:
        want = dict(zip(("xyz", "srgb"), restate_linear(film, **setting)))
        for space in ("xyz", "srgb"):
            got = develop_linear(film, space, **setting)
            scale = np.abs(want[space]).max(axis=-1, keepdims=True)
            error = np.abs(got.astype(np.float64) - want[space]) / np.where(scale > 0, scale, 1)
            worst = float(error.max())
            OBSERVED["%dx%dx%d, %s, %s" % (shape + (case_name(setting), space))] = (worst, bool(np.array_equal(got, want[space])))
            print("%s %s %s: max error relative to the pixel's largest channel %.3g, equal bits: %s" % (shape, case_name(setting), space, worst, np.array_equal(got, want[space])))
            assert worst <= TOL, (case_name(setting), space)
            assert (got[-1, -1] == 0).all()
    report = os.environ.get("PYRITE_TONE_PARITY_REPORT")  # a file to keep the measurement behind the bound in (profiles/r08_tone_parity.txt); nothing reads it back
    if report:
        with open(report, "w") as f:
            f.write("develop_linear against the numpy f32 restatement: max |difference| / the pixel's largest channel magnitude (bound %g)\n" % TOL)
            for name, (worst, equal) in sorted(OBSERVED.items()):
                f.write("%-52s %.3g%s\n" % (name, worst, "  (equal bits)" if equal else ""))


# ------------------------------------------------------------------------------------------------ 3. halves
@pytest.mark.parametrize("shape", FILMS[:3], ids=lambda s: "%dx%dx%d" % s)
def test_two_half_films_develop_as_their_sum(shape, gpu_lib):
    a, b = random_film(*shape, seed=21), random_film(*shape, seed=22)
    both = Film(*shape)
    both.grains[...] = a.grains + b.grains  # accs added, weights added, in f32
    for setting in (SETTINGS[0], SETTINGS[3]):
        for space in ("xyz", "srgb"):
            assert develop_linear(a, space, film_b=b, **setting).tobytes() == develop_linear(both, space, **setting).tobytes(), (case_name(setting), space)


def c2_session_case():
    world, cam, r, film = scenes.build(scenes.c2_cornell(40, 24, 12), seed=5)
    return world, cam, r


def test_session_linear_is_the_linear_image_of_its_film(gpu_lib):
    world, cam, r = c2_session_case()
    with r.session((40, 24), cam, world, halves=True) as s:
        for _ in range(3):  # two passes in A, one in B
            s.render(4)
        film = s.film()
        a, b = s.half_films()
        assert a[..., 1].sum() == 2 * b[..., 1].sum() > 0
        for setting in (SETTINGS[0], SETTINGS[3]):
            kwargs = {"filter": setting.get("filter"), "white": setting.get("white")}
            for space in ("xyz", "srgb"):
                got = s.linear(setting["step_size"], space, **kwargs)
                assert got.shape == (24, 40, 3) and got.dtype == f32
                assert got.tobytes() == develop_linear(film, space, step_size=setting["step_size"], **kwargs).tobytes(), (case_name(setting), space)
        assert s.linear().max() > 1.0  # the lamp
    world.close()


def test_session_preview_resolves_its_tone_from_its_own_statistics(gpu_lib):
    world, cam, r = c2_session_case()
    with r.session((40, 24), cam, world, halves=True) as s:
        s.render(4)
        s.render(4)
        linear = s.linear(30.0)
        plain = s.preview(30.0)
        assert np.array_equal(s.preview(30.0, tone=tone_params("clip", exposure=1.0)), plain)  # the clip at exposure 1 is the plain preview
        for tone in (tone_params("reinhard"), tone_params("clip"), tone_params("reinhard", exposure=2.0), tone_params("reinhard", white=4.0),
                     tone_params("reinhard", percentile=0.25, white_percentile=1.0)):
            stats = abi.PyrImageStats()
            shown = s.preview(30.0, tone=tone, stats=stats)
            assert bytes(stats) == bytes(image_stats(linear))
            assert stats.lit + stats.dark == 40 * 24 and stats.lit > 0
            exposure, white = tone_resolve(stats, tone)
            if not tone.exposure > 0:
                assert exposure == float(f32(f32(tone.key) / upper_edge(percentile_bin(stats, tone.percentile))))
            resolved = abi.PyrToneParams(tone.op, exposure, white, tone.key, tone.percentile, tone.white_percentile)
            assert np.array_equal(shown, tonemap(linear, resolved)), (tone.op, tone.exposure, tone.white)
            assert np.array_equal(shown, tonemap(linear, tone))  # the host wrapper resolves the same way
            assert np.array_equal(shown, s.preview(30.0, tone=tone))  # and the statistics need not be asked for
        assert not np.array_equal(s.preview(30.0, tone=tone_params("reinhard")), plain)
    world.close()


# ------------------------------------------------------------------------------------------------ 4. statistics
def upper_edge(k):
    return np.array([(k + 889) << 20], dtype=np.uint32).view(f32)[0]


def percentile_bin(stats, percentile):
    target = min(max(int(math.ceil(float(f32(percentile)) * stats.lit)), 1), stats.lit)
    return int(np.searchsorted(np.cumsum(np.asarray(stats.histogram[:], dtype=np.int64)), target))


def restate_stats(image):
    rgb = image.reshape(-1, 3)
    with np.errstate(all="ignore"):
        y = (f32(0.2126) * rgb[:, 0] + f32(0.7152) * rgb[:, 1]) + f32(0.0722) * rgb[:, 2]
        lit = y > 0
    bits = y[lit].view(np.uint32)
    bins = np.clip((bits >> 20).astype(np.int64) - 888, 0, 255)
    return {"histogram": np.bincount(bins, minlength=256).tolist(), "lit": int(lit.sum()), "dark": int((~lit).sum()),
            "min_lit": float(bits.min().view(f32)) if lit.any() else 0.0, "max_lit": float(bits.max().view(f32)) if lit.any() else 0.0}


def stats_image(width, height, seed):
    """Grey-ish pixels of log-uniform luminance over 2^-20 .. 2^20, with planted pixels: luminances exactly on bin edges and one ulp
    below them, zero, a negative value, NaN, +inf and a denormal (the one-pixel image is one lit pixel)."""
    rng = np.random.default_rng(seed)
    n = width * height
    image = (np.exp2(rng.uniform(-20, 20, size=(n, 1))) * rng.uniform(0.5, 1.5, size=(n, 3))).astype(f32)
    planted = []
    for k in (888, 889, 896, 1000, 1015, 1016, 1143, 1144, 880, 1200):  # k << 20 is an edge; 888 the first bin's, 1144 the end of the last
        edge = np.array([k << 20, (k << 20) - 1], dtype=np.uint32).view(f32)
        planted += [[0, edge[0] / f32(0.7152), 0], [0, edge[1] / f32(0.7152), 0]]  # near the edge through the rounding of one product
        planted += [[edge[0], edge[0], edge[0]], [edge[1], edge[1], edge[1]]]
    planted += [[0, 0, 0], [-1, -1, -1], [float("nan"), 1, 1], [float("inf"), 1, 1], [1e-40, 1e-40, 1e-40], [-0.0, 0, 0], [1, -5, 1], [float("inf"), float("-inf"), 0]]
    planted = np.asarray(planted if n > 1 else [[0.25, 0.5, 0.125]], dtype=f32)
    assert len(planted) <= n
    image[rng.permutation(n)[: len(planted)]] = planted
    return image.reshape(height, width, 3)


@pytest.mark.parametrize("size", [(1, 1), (63, 1), (65, 3), (257, 5)], ids=lambda s: "%dx%d" % s)
def test_statistics_are_exact(size, gpu_lib):
    image = stats_image(*size, seed=31)
    want = restate_stats(image)
    got, again = image_stats(image), image_stats(image)
    assert bytes(got) == bytes(again)  # integer sums: the same struct on every call
    assert got.as_dict()["histogram"] == want["histogram"]
    assert (got.lit, got.dark) == (want["lit"], want["dark"]) and got.lit + got.dark == size[0] * size[1]
    assert np.array([got.min_lit, got.max_lit], dtype=f32).tobytes() == np.array([want["min_lit"], want["max_lit"]], dtype=f32).tobytes()
    if size[0] * size[1] > 60:
        assert want["histogram"][0] > 0 and want["histogram"][255] > 0 and want["dark"] >= 5 and math.isinf(want["max_lit"])


def test_statistics_of_a_dark_image(gpu_lib):
    got = image_stats(np.zeros((3, 5, 3), dtype=f32))
    assert (got.lit, got.dark, got.min_lit, got.max_lit) == (0, 15, 0.0, 0.0) and not any(got.histogram)
    assert tone_resolve(got, tone_params("reinhard")) == (1.0, 1.0)


# ------------------------------------------------------------------------------------------------ 5. Reinhard
def restate_tonemap(image, op, exposure, white, power=None):
    """uint8 image: the header's f32 operations, the encoder's pow in f64 (numpy's, or `power` element by element)."""
    exposure, white = f32(exposure), f32(white)
    with np.errstate(all="ignore"):
        v = exposure * image
        lit = np.ones(image.shape[:2], dtype=bool)
        if op == abi.PYR_TONE_REINHARD:
            y = (f32(0.2126) * image[..., 0] + f32(0.7152) * image[..., 1]) + f32(0.0722) * image[..., 2]
            lit = y > 0
            l = exposure * y
            ld = (l * (f32(1) + l / (white * white))) / (f32(1) + l)
            v = v * (ld / l)[..., None]
        v = np.fmin(np.fmax(v, f32(0)), f32(1))  # fmaxf / fminf: a NaN gives way to the number
        if power is None:
            curve = np.power(v.astype(np.float64), 1.0 / 2.4)
        else:
            curve = np.asarray([power(float(x), 1.0 / 2.4) for x in v.reshape(-1)], dtype=np.float64).reshape(v.shape)
        e = np.where(v <= f32(0.0031308), f32(12.92) * v, f32(1.055) * curve.astype(f32) - f32(0.055))
        e = np.fmin(np.fmax(e, f32(0)), f32(1))
        assert e.dtype == f32
        out = (e * f32(255) + f32(0.5)).astype(np.uint8)
    out[~lit] = 0
    return out


def within_the_cap(a, b):
    """No byte more than one code apart, at most 0.1 % of the bytes apart at all: the last bit of pow before it is rounded to f32."""
    d = np.abs(a.astype(int) - b.astype(int))
    return int(d.max()) <= 1 and float((d != 0).mean()) <= 0.001


def tone_image(seed=41):
    """65 x 33 (four-pixel groups and a tail): coloured pixels of log-uniform luminance over 2^-10 .. 2^10, and pixels that are not lit
    or not finite."""
    rng = np.random.default_rng(seed)
    n = 65 * 33
    image = (np.exp2(rng.uniform(-10, 10, size=(n, 1))) * rng.uniform(0.2, 1.8, size=(n, 3))).astype(f32)
    image[rng.permutation(n)[:8]] = np.asarray([[0, 0, 0], [-1, -2, -3], [float("nan"), 1, 1], [float("inf"), 1, 1], [1e-40, 1e-40, 1e-40], [3, -0.5, 0.1],
                                                 [1e30, 1e30, 1e30], [0.0031308, 0.0031309, 0.0031307]], dtype=f32)
    return image.reshape(33, 65, 3)


TONES = [(abi.PYR_TONE_REINHARD, 1.0, 4.0), (abi.PYR_TONE_REINHARD, 0.37, 1.5), (abi.PYR_TONE_REINHARD, 8.0, 1000.0), (abi.PYR_TONE_CLIP, 0.6, 1.0), (abi.PYR_TONE_CLIP, 3.0, 1.0)]


def test_the_restatement_agrees_with_itself_through_a_second_pow():
    """The cap is wide enough for the one admitted difference on this very image: numpy's pow against math.pow. (No GPU in this
    one; it stands here because it vouches for the image the next test uses.)"""
    image = tone_image()
    for op, exposure, white in TONES:
        assert within_the_cap(restate_tonemap(image, op, exposure, white), restate_tonemap(image, op, exposure, white, power=math.pow)), (op, exposure, white)


def test_tone_mapping_matches_the_restatement(gpu_lib):
    image = tone_image()
    for op, exposure, white in TONES:
        got = tonemap(image, abi.PyrToneParams(op, exposure, white, 0.18, 0.5, 0.99))
        want = restate_tonemap(image, op, exposure, white)
        d = np.abs(got.astype(int) - want.astype(int))
        print("op %d exposure %g white %g: %d of %d bytes differ, by at most %d" % (op, exposure, white, int((d != 0).sum()), d.size, int(d.max())))
        assert within_the_cap(got, want), (op, exposure, white)
        assert got.min() == 0 and got.max() == 255
    # automatic: the image's own statistics
    auto = tone_params("reinhard")
    exposure, white = tone_resolve(image_stats(image), auto)
    assert within_the_cap(tonemap(image, auto), restate_tonemap(image, abi.PYR_TONE_REINHARD, exposure, white))
    # one pixel, and fewer pixels than a four-pixel group
    for n in (1, 3):
        small = np.ascontiguousarray(image[:1, :n])
        assert within_the_cap(tonemap(small, abi.PyrToneParams(abi.PYR_TONE_REINHARD, 1.0, 4.0, 0.18, 0.5, 0.99)), restate_tonemap(small, abi.PYR_TONE_REINHARD, 1.0, 4.0))


# ------------------------------------------------------------------------------------------------ 6. a real picture
def test_a_picture_the_8_bit_path_clips(gpu_lib, tmp_path):
    from pyrite_amd.develop import save_hdr

    project = scenes.lamps_example(48, 32, 16)
    world, cam, r, film = scenes.build(project, seed=5)
    r.render(film, cam, world)
    image = project.get("image") or {}
    kwargs = {"filter": image.get("filter"), "white": image.get("white")}
    png, linear = develop(film, **kwargs), develop_linear(film, "srgb", **kwargs)
    clipped = (png == 255).any(axis=-1)
    assert clipped.any()  # the sky and the lamps saturate the 8-bit image
    assert linear[clipped].max() > 1.0 and float(linear.max()) > 1.0
    path = tmp_path / "lamps.hdr"
    save_hdr(str(path), linear)
    assert path.read_bytes() == encode_hdr(linear)
    check_hdr_round_trip(linear, path.read_bytes())
    shown = tonemap(linear, tone_params("reinhard"))
    assert shown.shape == png.shape and shown.dtype == np.uint8 and shown.max() > 0
    world.close()


# ------------------------------------------------------------------------------------------------ 7. the _device forms
def on_device(entry, *args):
    """The bytes `entry`, a _device form, writes on device 0 and a stream of its own: every numpy array among `args` goes as a device
    copy, the last of them is the output."""
    import torch

    side = torch.cuda.Stream()
    held = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() if isinstance(a, np.ndarray) else a for a in args]
    side.wait_stream(torch.cuda.current_stream())  # the copies above
    check(getattr(lib(), entry)(*[C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in held], 0, C.c_void_p(side.cuda_stream)))
    side.synchronize()
    return [a for a in held if isinstance(a, torch.Tensor)][-1].cpu().numpy().tobytes()


@pytest.mark.parametrize("shape", [FILMS[0], FILMS[3]], ids=lambda s: "%dx%dx%d" % s)
def test_the_device_forms_write_the_bytes_the_host_forms_return(shape, gpu_lib):
    """pyr_film_develop_device, pyr_film_develop_linear_device (one film and two), pyr_image_stats_device, pyr_image_tonemap_device:
    the host forms run through the same enqueues, so on tensors and a stream of the caller's the bytes are the same, none excepted."""
    film, film_b = random_film(*shape, seed=61), random_film(*shape, seed=62)
    width, height, _ = shape
    desc, grains, grains_b = film.desc(), np.ascontiguousarray(film.grains), np.ascontiguousarray(film_b.grains)
    for step_size in (2.0, 30.0):  # the wave kernel, the thread-per-pixel kernel
        p, keep = develop_params(film, step_size)
        rgb8 = on_device("pyr_film_develop_device", C.byref(desc), grains, C.byref(p), np.zeros((height, width, 3), dtype=np.uint8))
        assert rgb8 == develop(film, step_size).tobytes(), step_size
        for halves in (None, film_b):
            linear = on_device("pyr_film_develop_linear_device", C.byref(desc), grains, grains_b if halves is not None else None, C.byref(p), abi.PYR_LINEAR_SRGB,
                               np.zeros((height, width, 3), dtype=f32))
            image = develop_linear(film, "srgb", film_b=halves, step_size=step_size)
            assert linear == image.tobytes(), (step_size, halves is not None)
        del keep
        stats = on_device("pyr_image_stats_device", image, width, height, np.zeros(C.sizeof(abi.PyrImageStats), dtype=np.uint8))
        assert stats == bytes(image_stats(image)), step_size
        tone = abi.PyrToneParams(abi.PYR_TONE_REINHARD, 0.37, 1.5, abi.PYR_TONE_KEY, abi.PYR_TONE_PERCENTILE, abi.PYR_TONE_WHITE_PERCENTILE)
        mapped = on_device("pyr_image_tonemap_device", image, width, height, C.byref(tone), np.zeros((height, width, 3), dtype=np.uint8))
        assert mapped == tonemap(image, tone).tobytes(), step_size


# ------------------------------------------------------------------------------------------------ 8. errors
def test_invalid_arguments_are_refused_before_any_kernel(gpu_lib):
    L = lib()
    INVALID, UNSUPPORTED, DEVICE = abi.PYR_ERR_INVALID_ARGUMENT, abi.PYR_ERR_UNSUPPORTED, abi.PYR_ERR_DEVICE
    film = random_film(6, 4, 8, seed=51)
    p, keep = develop_params(film)
    desc = film.desc()
    grains = np.ascontiguousarray(film.grains)
    out = np.full((4, 6, 3), 7.0, dtype=f32)
    rgb8 = np.full((4, 6, 3), 9, dtype=np.uint8)
    stats = abi.PyrImageStats()
    stats.lit = 123

    def linear(desc=desc, grains=grains.ctypes.data, p=p, space=abi.PYR_LINEAR_SRGB, out=out.ctypes.data, device=0):
        return L.pyr_film_develop_linear(C.byref(desc) if desc else None, grains, None, C.byref(p) if p else None, space, out, device)

    for missing in ("desc", "grains", "p", "out"):
        assert linear(**{missing: None}) == INVALID, missing
    assert linear(space=2) == INVALID and linear(space=0xFFFFFFFF) == INVALID
    bad = abi.PyrDevelopParams(-1.0, p.xyz_scale, p.sample_count, None, None, None, p.xyz_table, p.xyz_count, p.xyz_min, p.xyz_max)
    assert linear(p=bad) == INVALID
    assert linear(desc=abi.PyrFilmDesc(1 << 16, 1 << 16, 8, 380.0, 400.0)) == UNSUPPORTED
    assert linear(device=99) == DEVICE and linear(device=-1) == DEVICE
    assert (out == 7.0).all()

    image = np.ones((4, 6, 3), dtype=f32)
    assert L.pyr_image_stats(None, 6, 4, C.byref(stats), 0) == INVALID and L.pyr_image_stats(image.ctypes.data, 6, 4, None, 0) == INVALID
    assert L.pyr_image_stats(image.ctypes.data, 1 << 16, 1 << 16, C.byref(stats), 0) == UNSUPPORTED
    assert L.pyr_image_stats(image.ctypes.data, 6, 4, C.byref(stats), 99) == DEVICE
    assert stats.lit == 123

    def tone(image=image.ctypes.data, width=6, height=4, t=abi.PyrToneParams(abi.PYR_TONE_REINHARD, 1.0, 2.0, 0.18, 0.5, 0.99), rgb=rgb8.ctypes.data, device=0):
        return L.pyr_image_tonemap(image, width, height, C.byref(t) if t else None, rgb, device)

    for missing in ("image", "t", "rgb"):
        assert tone(**{missing: None}) == INVALID, missing
    assert tone(t=abi.PyrToneParams(2, 1.0, 2.0, 0.18, 0.5, 0.99)) == INVALID
    assert tone(t=abi.PyrToneParams(abi.PYR_TONE_CLIP, 0.0, 0.0, 0.18, 0.5, 0.99)) == INVALID  # unresolved
    assert tone(t=abi.PyrToneParams(abi.PYR_TONE_REINHARD, 1.0, -1.0, 0.18, 0.5, 0.99)) == INVALID
    assert tone(width=1 << 16, height=1 << 16) == UNSUPPORTED
    assert tone(device=99) == DEVICE
    assert (rgb8 == 9).all()

    world, cam, r = c2_session_case()
    with r.session((6, 4), cam, world) as s:
        s.render(1)
        good = abi.PyrToneParams(abi.PYR_TONE_REINHARD, 0.0, 0.0, 0.18, 0.5, 0.99)
        assert L.pyr_session_linear(s.handle, None, abi.PYR_LINEAR_SRGB, out.ctypes.data) == INVALID
        assert L.pyr_session_linear(s.handle, C.byref(p), 5, out.ctypes.data) == INVALID
        assert L.pyr_session_linear(s.handle, C.byref(p), abi.PYR_LINEAR_XYZ, None) == INVALID
        assert L.pyr_session_preview_tone(s.handle, C.byref(p), None, rgb8.ctypes.data, None) == INVALID
        assert L.pyr_session_preview_tone(s.handle, None, C.byref(good), rgb8.ctypes.data, None) == INVALID
        assert L.pyr_session_preview_tone(s.handle, C.byref(p), C.byref(good), None, None) == INVALID
        for percentile in (0.0, 1.5, -1.0, float("nan")):
            assert L.pyr_session_preview_tone(s.handle, C.byref(p), C.byref(abi.PyrToneParams(abi.PYR_TONE_CLIP, 0.0, 0.0, 0.18, percentile, 0.99)), rgb8.ctypes.data, None) == INVALID
            assert L.pyr_session_preview_tone(s.handle, C.byref(p), C.byref(abi.PyrToneParams(abi.PYR_TONE_CLIP, 1.0, 0.0, 0.18, 0.5, percentile)), rgb8.ctypes.data, None) == INVALID
        assert L.pyr_session_preview_tone(s.handle, C.byref(p), C.byref(abi.PyrToneParams(3, 1.0, 1.0, 0.18, 0.5, 0.99)), rgb8.ctypes.data, None) == INVALID
        assert L.pyr_session_preview_tone(s.handle, C.byref(p), C.byref(abi.PyrToneParams(abi.PYR_TONE_CLIP, 0.0, 0.0, 0.0, 0.5, 0.99)), rgb8.ctypes.data, None) == INVALID
        assert (out == 7.0).all() and (rgb8 == 9).all()
        assert L.pyr_session_preview_tone(s.handle, C.byref(p), C.byref(good), rgb8.ctypes.data, None) == 0 and not (rgb8 == 9).all()  # and the session still works
    world.close()
    del keep
