"""Every image kernel past its launch cap and off its aligned path -- run with `-m gpu` on an MI355X.

The kernels that cap their grid walk `for (t = blockIdx.x; t < tiles; t += gridDim.x)`, stage a tile in LDS and stage it again for
the next, and some carry state from one trip to the next; the small images of their own test modules end in the first trip. Here
each kernel family runs once at the smallest narrow image that takes the second trip with a ragged last row and column
(tests/launch_caps.py derives the sizes from the kernel sources; tests/test_launch_caps_cpu.py holds the conditions on the inputs),
through its _device entry, into an output that holds a sentinel no result can equal, against the numpy restatement of the same
operation and with the very assertion its small-size test uses. A failing comparison names the trip and the tile of the first
differing pixel. Then the three fallbacks of kernels/tone.hip for buffers that are not aligned, which no other test passes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_caps as lc  # noqa: E402

from pyrite_amd import abi, scenes  # noqa: E402
from pyrite_amd._lib import check, lib  # noqa: E402

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
SENTINEL = lc.SENTINEL


# ------------------------------------------------------------------------------------------------------------------------ helpers
def differing(got, want):
    """The first place where the bits differ and not both are NaN; else the first where the bits differ at all; else None."""
    bits = got.view(u32) != want.view(u32)
    for mask in (bits & ~(np.isnan(got) & np.isnan(want)), bits):
        at = np.argwhere(mask)
        if len(at):
            return tuple(int(i) for i in at[0])
    return None


def held(assertion, got, want, what, where, differing=differing):
    """`assertion(got, want, what)`, the comparison of the kernel's own small-size test, over arrays [height, width, ...] or tuples of
    them; before it, no float of `got` may still be the sentinel. A failure says in which trip and tile its first pixel lies:
    `differing(got, want)` finds it, by bits unless the comparison is another. (A pixel takes from its neighbours: the first one
    that differs may lie a tile before the trip that went wrong.)"""
    gots, wants = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    try:
        for g in gots:
            unwritten = np.argwhere(g.view(u32) == u32(SENTINEL))
            assert len(unwritten) == 0, "%s: %d of %d floats were never written, the first at %s" % (what, len(unwritten), g.size, tuple(unwritten[0]))
        assertion(got, want, what)
    except AssertionError as failure:
        for g, w in zip(gots, wants):
            unwritten = np.argwhere(g.view(u32) == u32(SENTINEL))
            at = tuple(int(i) for i in unwritten[0]) if len(unwritten) else differing(g, w)
            if at is not None:
                raise AssertionError("%s\n%s" % (failure, where(at[1], at[0]))) from None
        raise


def tiled_where(kernel, size):
    return lambda x, y: kernel.where(size[0], size[1], x, y)


def flat_where(kernel, size, items_per_pixel=1):
    return lambda x, y: kernel.where(size[0] * size[1] * items_per_pixel, (y * size[0] + x) * items_per_pixel)


def call_device(entry, *args):
    """`entry`, a _device form, on device 0 and the current stream. A numpy array among `args` goes as a device copy; a pair (array,
    offset) as a copy that starts `offset` bytes into an allocation of torch's, which is 256-byte aligned: its address is the
    offset modulo 16. Returns the bytes of the last array, the output."""
    import torch

    def placed(a):
        array, offset = a if isinstance(a, tuple) else (a, 0)
        room = torch.zeros(array.nbytes + 16, dtype=torch.uint8, device="cuda")
        assert room.data_ptr() % 16 == 0
        part = room[offset:offset + array.nbytes]
        part.copy_(torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()))
        return part

    is_buffer = lambda a: isinstance(a, np.ndarray) or (isinstance(a, tuple) and isinstance(a[0], np.ndarray))  # noqa: E731
    placed_args = [placed(a) if is_buffer(a) else a for a in args]
    stream = torch.cuda.current_stream()
    check(getattr(lib(), entry)(*[C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in placed_args], 0, C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    return [a for a in placed_args if isinstance(a, torch.Tensor)][-1].cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------------------------------ the tile kernels
@pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "no noise"])
def test_temporal_past_its_cap(with_noise, gpu_lib):
    """temporal_kernel<NOISE>, radius 1: three tile columns, the second trip the last 256 tiles."""
    import test_gpu_temporal as T

    frame = lc.temporal_frame()
    got = T.resolve_on_device(*frame[:5], frame[5] if with_noise else None, out_bits=SENTINEL, radius=1)
    held(T.assert_same, got, lc.temporal_wanted(with_noise), "temporal %dx%d" % lc.TEMPORAL_SIZE, tiled_where(lc.TEMPORAL, lc.TEMPORAL_SIZE))


@pytest.mark.parametrize("max_radius", [1, 2])
def test_lens_blur_past_its_cap(max_radius, gpu_lib):
    """lens_blur_kernel: the first tile of every workgroup that takes a second lies in focus and copies, the second is out of focus,
    so the largest c and the rows' reach it kept in LDS are wrong for it; at max_radius 2 the reach differs between the two."""
    import test_gpu_lens_blur as T

    image, rec = lc.lens_blur_frame()
    got = T.blur_on_device(image, rec, out_bits=SENTINEL, **lc.lens_blur_params(max_radius))
    held(T.assert_same_image, got, lc.lens_blur_wanted(max_radius), "lens blur %dx%d radius %d" % (lc.LENS_BLUR_SIZE + (max_radius,)), tiled_where(lc.LENS_BLUR, lc.LENS_BLUR_SIZE))


@pytest.mark.parametrize("radius", [1, 3])
def test_upsample_past_its_cap(radius, gpu_lib):
    """upsample_kernel<R, true, true>, scale 2, the material rule on: the cells of the LDS patch that lie outside the low image are
    never written, and on a second trip they hold the tile before; at radius 3 the patch is the widest."""
    import test_gpu_upsample as T

    inputs = lc.upsample_inputs()
    size = (lc.UPSAMPLE_LOW_SIZE[0] * lc.UPSAMPLE_SCALE, lc.UPSAMPLE_LOW_SIZE[1] * lc.UPSAMPLE_SCALE)
    got = T.upsample_on_device(inputs["low"], lc.UPSAMPLE_SCALE, albedo=inputs["albedo"], pixels=inputs["pixels"], low_albedo=inputs["low_albedo"], low_pixels=inputs["low_pixels"],
                               out_bits=SENTINEL, radius=radius, match_material=True)
    held(T.assert_same_image, got, lc.upsample_wanted(radius)[0], "upsample to %dx%d radius %d" % (size + (radius,)), tiled_where(lc.UPSAMPLE, size))


@pytest.fixture(params=("plain", "tail"))
def form(request, monkeypatch):
    monkeypatch.setenv("PYRITE_GLARE_TAIL", "1" if request.param == "tail" else "0")
    return request.param


@pytest.mark.parametrize("levels", [3, 12])
@pytest.mark.parametrize("deep", [False, True], ids=["tall", "deep"])
def test_glare_past_its_caps(deep, levels, form, gpu_lib):
    """tall: the compose (glare_up_kernel<true>) takes a third trip, the down to level 1 (glare_down_kernel<true>) and the up from
    level 2 (glare_up_kernel<false>) a second. deep: a 17-wide image so tall that level 2 exceeds the cap too, which
    glare_down_kernel<false> writes. The trip a failure names is the compose's; a wrong lower level shows over the pixels above it."""
    import test_gpu_glare as T

    size = lc.GLARE_DEEP_SIZE if deep else lc.GLARE_SIZE
    image = lc.glare_image(deep)
    got = T.glare_on_device(image, out_bits=SENTINEL, levels=levels, **lc.GLARE_PARAMS)
    held(T.assert_same_image, got, lc.glare_wanted(levels, deep), "glare %dx%d %s, %d levels" % (size + (form, levels)), tiled_where(lc.GLARE, size))


def test_motion_blur_past_its_cap(gpu_lib):
    """motion_blur_velocity_kernel at max_radius 1: a tile is a pixel, and the last 1,024 of them are the second trip."""
    import test_gpu_motion_blur as T

    image, rec = lc.motion_blur_frame()
    got = T.blur_on_device(image, rec, out_bits=SENTINEL, **lc.MOTION_BLUR_PARAMS)
    held(T.assert_same_image, got, lc.motion_blur_wanted(), "motion blur %dx%d" % lc.MOTION_BLUR_SIZE, tiled_where(lc.VELOCITY, lc.MOTION_BLUR_SIZE))


# ------------------------------------------------------------------------------------------------------------------------ the flat kernels
def same_images(got, want, what):
    """tests/test_gpu_motion.py test_reproject_is_the_restatement_bit_for_bit: the bits of `out`, the bytes of `count_out`."""
    for name, g, w in zip(("out", "count_out"), got, want):
        differs = np.argwhere(g.view(u32) != w.view(u32))
        assert len(differs) == 0, "%s: %s differs in %d floats, first %s: GPU %r, restatement %r" % (what, name, len(differs), tuple(differs[0]), g[tuple(differs[0])], w[tuple(differs[0])])


def test_reproject_past_its_cap(gpu_lib):
    """reproject_kernel: the last 1,024 pixels are the second trip and carry full records; so do the first 2,048 and a twentieth of the
    rest (tests/launch_caps.py reproject_frame)."""
    import test_gpu_motion as T

    frame = lc.reproject_frame()
    got = T.reproject_on_device(*frame[:5], out_bits=SENTINEL)
    held(same_images, got, lc.reproject_wanted(), "reproject %dx%d" % lc.REPROJECT_SIZE, flat_where(lc.REPROJECT, lc.REPROJECT_SIZE))


def test_denoise_past_its_caps(gpu_lib):
    """denoise_variance_kernel over pixels and denoise_combine_kernel over floats in one run: radius 1, patch 0, no guides."""
    import test_gpu_denoise as T

    a, b, _, _ = lc.denoise_halves()
    params = dict(lc.DENOISE_PARAMS)
    out, error = T.gpu_denoise(a, b, None, None, params, device_entry=True, out_bits=SENTINEL)
    want, want_error = lc.denoise_wanted()
    scale = T.window_scale(a, b, params["radius"])
    what = "denoise %dx%d r%d p%d" % (lc.DENOISE_SIZE + (params["radius"], params["patch"]))
    close = lambda got, expected, name: T.assert_close(got, expected, scale, name)  # noqa: E731

    def beyond(got, expected):  # the first float T.assert_close objects to
        with np.errstate(all="ignore"):
            finite = np.isfinite(expected)
            bad = (np.isnan(got) != np.isnan(expected)) | (~finite & (got != expected) & ~np.isnan(expected))
            bad |= np.where(finite, np.abs(np.where(finite, got, 0) - np.where(finite, expected, 0)), 0) / np.maximum(scale, f32(1e-30))[..., None] > T.TOL
        at = np.argwhere(bad)
        return tuple(int(i) for i in at[0]) if len(at) else None

    width, height = lc.DENOISE_SIZE
    where = lambda x, y: "%s\n%s" % (lc.VARIANCE.where(width * height, y * width + x), lc.COMBINE.where(3 * width * height, 3 * (y * width + x)))  # noqa: E731
    held(close, out, want, what, where, differing=beyond)
    held(close, error, want_error, what + " error", where, differing=beyond)


def stats_struct(want):
    s = abi.PyrImageStats()
    s.histogram[:] = want["histogram"]
    s.lit, s.dark = want["lit"], want["dark"]
    C.memmove(C.byref(s, abi.PyrImageStats.min_lit.offset), np.array([want["min_lit"], want["max_lit"]], dtype=f32).tobytes(), 8)
    return bytes(s)


def test_statistics_past_their_cap_and_off_their_alignment(gpu_lib):
    """image_stats_kernel: more pixels than 2,048 workgroups of 256 threads take four at a time, then the same image 4 bytes off a
    16-byte boundary, where the kernel takes no group of four at all. Integer sums: the struct's bytes, every time."""
    import test_gpu_tone as T

    image = lc.stats_case()
    width, height = lc.STATS_SIZE
    want = T.restate_stats(image)
    assert want["lit"] + want["dark"] == width * height and want["histogram"][0] > 0 and want["histogram"][255] > 0
    before = np.full(C.sizeof(abi.PyrImageStats), 0xA5, dtype=np.uint8)
    aligned = call_device("pyr_image_stats_device", image, width, height, before)
    got = abi.PyrImageStats.from_buffer_copy(aligned)
    assert aligned == stats_struct(want), "statistics of %dx%d: GPU %r against %r" % (width, height, {k: v for k, v in got.as_dict().items() if k != "histogram"},
                                                                                      {k: v for k, v in want.items() if k != "histogram"})
    shifted = call_device("pyr_image_stats_device", (image, 4), width, height, before)
    assert shifted == aligned, "the image 4 bytes off: %r" % ({k: v for k, v in abi.PyrImageStats.from_buffer_copy(shifted).as_dict().items() if k != "histogram"},)


TONES_BY_OPERATOR = {}


def one_tone_per_operator():
    import test_gpu_tone as T

    for tone in T.TONES:
        TONES_BY_OPERATOR.setdefault(tone[0], tone)
    return sorted(TONES_BY_OPERATOR.values())


def test_tone_mapping_past_its_cap(gpu_lib):
    """tonemap_kernel: test_gpu_tone's image tiled to more pixels than 4,096 workgroups of 256 threads take four at a time."""
    import test_gpu_tone as T

    image = lc.tonemap_case()
    width, height = lc.TONEMAP_SIZE
    trips = lc.TONEMAP.trips(width * height)
    for op, exposure, white in one_tone_per_operator():
        tone = abi.PyrToneParams(op, exposure, white, abi.PYR_TONE_KEY, abi.PYR_TONE_PERCENTILE, abi.PYR_TONE_WHITE_PERCENTILE)
        got = np.frombuffer(call_device("pyr_image_tonemap_device", image, width, height, C.byref(tone), np.full((height, width, 3), 0xA5, dtype=np.uint8)), dtype=np.uint8)
        want = T.restate_tonemap(image, op, exposure, white).reshape(-1)
        d = np.abs(got.astype(int) - want.astype(int))
        far = np.flatnonzero(d > 1)
        where = lc.TONEMAP.where(width * height, int(far[0]) // 3) if len(far) else "no byte more than one code apart"
        print("op %d exposure %g white %g: %d of %d bytes differ, by at most %d; %s" % (op, exposure, white, int((d != 0).sum()), d.size, int(d.max()), where))
        for trip in range(int(trips.max()) + 1):  # within the cap in every trip, not on the average of them
            part = np.repeat(trips == trip, 3)
            assert T.within_the_cap(got[part], want[part]), (op, exposure, white, "trip %d" % trip, where)
        assert T.within_the_cap(got, want), (op, exposure, white, where)


@pytest.mark.parametrize("offsets", [(4, 0), (0, 1), (4, 1)], ids=["image+4", "rgb_out+1", "both"])
def test_tone_mapping_off_its_alignment(offsets, gpu_lib):
    """tonemap_kernel's byte path: an image off 16 bytes, an rgb_out off 4, and both, must write the aligned call's bytes."""
    import test_gpu_tone as T

    image = T.tone_image()
    height, width, _ = image.shape
    before = np.full((height, width, 3), 0xA5, dtype=np.uint8)
    for op, exposure, white in one_tone_per_operator():
        tone = abi.PyrToneParams(op, exposure, white, abi.PYR_TONE_KEY, abi.PYR_TONE_PERCENTILE, abi.PYR_TONE_WHITE_PERCENTILE)
        aligned = call_device("pyr_image_tonemap_device", image, width, height, C.byref(tone), before)
        assert T.within_the_cap(np.frombuffer(aligned, dtype=np.uint8), T.restate_tonemap(image, op, exposure, white).reshape(-1))
        shifted = call_device("pyr_image_tonemap_device", (image, offsets[0]), width, height, C.byref(tone), (before, offsets[1]))
        differs = np.flatnonzero(np.frombuffer(shifted, dtype=np.uint8) != np.frombuffer(aligned, dtype=np.uint8))
        assert len(differs) == 0, "op %d, image + %d, rgb_out + %d: %d bytes differ from the aligned call's, the first in pixel %d" % ((op,) + offsets + (len(differs), differs[0] // 3))


@pytest.mark.parametrize("shape", [0, 1], ids=lambda i: "FILMS[%d]" % i)
def test_linear_development_off_its_alignment(shape, gpu_lib):
    """develop_linear_kernel's dword path: `out` 4 bytes off a 16-byte boundary must hold the aligned call's bytes -- one film and two
    halves, step 2 and step 30."""
    import test_gpu_tone as T
    from pyrite_amd.develop import develop_params

    width, height, bins = T.FILMS[shape]
    film, film_b = T.random_film(width, height, bins, seed=61), T.random_film(width, height, bins, seed=62)
    desc, grains, grains_b = film.desc(), np.ascontiguousarray(film.grains), np.ascontiguousarray(film_b.grains)
    before = np.full((height, width, 3), SENTINEL, dtype=u32)
    for step_size in (2.0, 30.0):
        p, keep = develop_params(film, step_size)
        for halves in (None, grains_b):
            aligned = call_device("pyr_film_develop_linear_device", C.byref(desc), grains, halves, C.byref(p), abi.PYR_LINEAR_SRGB, before)
            shifted = call_device("pyr_film_develop_linear_device", C.byref(desc), grains, halves, C.byref(p), abi.PYR_LINEAR_SRGB, (before, 4))
            a, s = np.frombuffer(aligned, dtype=u32), np.frombuffer(shifted, dtype=u32)
            assert not (a == SENTINEL).any() and np.isfinite(a.view(f32)).all() and a.view(f32).any()
            differs = np.flatnonzero(a != s)
            assert len(differs) == 0, "step %g, %s: %d floats differ from the aligned call's, the first in pixel %d (run %d): %r against %r" % (
                step_size, "two halves" if halves is not None else "one film", len(differs), differs[0] // 3, differs[0] // 3 // 64, s.view(f32)[differs[0]], a.view(f32)[differs[0]])
        del keep


# ------------------------------------------------------------------------------------------------------------------------ the films
def test_a_session_s_film_is_the_sum_of_its_halves_past_the_cap(gpu_lib):
    """film_sum_kernel: Session.film() of a session with halves, more grains than 8,192 workgroups of 256 threads take."""
    case = lc.FILM_SUM_CASE
    world, cam, r, _ = scenes.build(scenes.c2_cornell(case["width"], case["height"], 2), seed=9)
    assert r.spectrum_bins == case["bins"]
    with r.session((case["width"], case["height"]), cam, world, halves=True) as s:
        for _ in range(2):
            s.render(1)
        film = s.film().grains
        a, b = s.half_films()
    world.close()
    assert a.dtype == f32 and a.size // 2 >= lc.FILM_SUM.cap + lc.FLAT_MARGIN
    want = a + b
    assert a[..., 1].any() and b[..., 1].any() and (a != b).any()
    differs = np.flatnonzero((film.view(u32) != want.view(u32)).reshape(-1, 2).any(axis=-1))
    assert len(differs) == 0, "%d grains differ from a + b, the first: %s" % (len(differs), lc.FILM_SUM.where(a.size // 2, int(differs[0])))


def test_block_assembly_past_its_caps(gpu_lib):
    """assemble_interior_kernel and assemble_ring_kernel: a block set of more grains than 8,192 workgroups of 256 threads take, in the
    interior and in the ring, against the torch form as test_gpu_parity.py test_blocks_assembly_kernel_equals_the_torch_form has it.
    (Its full-size multi-device tests cross both caps too, but a render exposes next to nothing in the rings.)"""
    import torch

    from pyrite_amd import distributed as pdist

    dev = torch.device("cuda", 0)
    ts, bins, width = 16, 64, 75  # five tile columns, the last 11 wide
    tiles_y = -(-(lc.ASSEMBLE.cap + lc.FLAT_MARGIN) // (4 * (ts + 1) * bins * 5))  # the ring is the smaller count: 4 (ts + 1) pixels a tile
    height = tiles_y * ts - 7
    share = pdist.plan(width, height, ts, 1, "tiles")[0]
    assert 4 * (ts + 1) * bins * share.tile_count >= lc.ASSEMBLE.cap + lc.FLAT_MARGIN and ts * ts * bins * share.tile_count >= lc.ASSEMBLE.cap + lc.FLAT_MARGIN
    gen = torch.Generator(device="cpu").manual_seed(5)
    blocks = torch.rand((share.pixels(width), bins, 2), generator=gen)
    expect = pdist.assemble_blocks_torch(torch.ones((height, width, bins, 2)), blocks, share, ts)
    got = pdist.assemble(torch.ones((height, width, bins, 2), device=dev), blocks.to(dev), share, ts).cpu()
    far = torch.nonzero(~torch.isclose(got, expect, rtol=1e-6, atol=0))
    assert len(far) == 0, "%d grains differ, the first at (y, x, bin, part) %s: %r against %r" % (len(far), tuple(far[0].tolist()), float(got[tuple(far[0])]), float(expect[tuple(far[0])]))
    assert torch.allclose(got, expect, rtol=1e-6, atol=0)
