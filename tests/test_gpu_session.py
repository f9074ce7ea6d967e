"""Progressive sessions on the GPU (include/pyrite_gpu.h "progressive sessions"): sample windows add up to the one-shot film and
to the oracle's, a session equals one shot, the preview is the developed film byte for byte, the wave-shaped develop kernel writes
develop_kernel's bytes, the noise estimate is its formula, and the blocking convenience reports as main.rs:243-305 does."""
import ctypes as C
import os
import struct
import subprocess
import sys
import threading
import zlib

import numpy as np
import pytest

import oracle
from pyrite_amd import abi, scenes
from pyrite_amd._lib import PyriteGpuError, check, lib
from pyrite_amd.develop import develop, develop_params
from pyrite_amd.distributed import Share, assemble_blocks_torch
from pyrite_amd.film import Film
from pyrite_amd.project import blackbody, spectrum
from pyrite_amd.renderer import Camera, Renderer, World

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5  # per-pixel relative L2 of the developed spectra


def rel_l2(film, reference):
    a, b = film.develop(), reference.develop()
    return (np.sqrt(((a - b) ** 2).sum(-1)) / (np.sqrt((b ** 2).sum(-1)) + 1e-6)).reshape(-1)


def assert_same_film(film, reference, what):
    e = rel_l2(film, reference)
    worst = float(e.max()) if e.size else 0.0
    print("%s: relL2 median %.3g max %.3g (pixel %d), weights equal: %s" % (what, np.median(e), worst, int(e.argmax()),
                                                                            np.array_equal(film.grains[..., 1], reference.grains[..., 1])))
    assert np.array_equal(film.grains[..., 1], reference.grains[..., 1]), what + ": film weights differ"
    assert worst <= TOL, what
    assert not np.isnan(film.grains).any()


def c2_case():
    world, cam, r, film = scenes.build(scenes.c2_cornell(64, 64, 16), seed=5)  # test_gpu_parity.py CASES, seed of test_render_matches_the_oracle
    return world, cam, r


def c3_case():
    project = scenes.c3_mesh_in_box(width=64, height=36, pixel_samples=16)  # test_c3_shaped_scene_at_scale_50: tiles of 32, the bottom row 4 pixels high
    world = World(scenes.c3_flat(segments=96, sides=48))
    return world, Camera.from_project(project["camera"]), Renderer.from_project(project["renderer"], seed=6)


def textures_case():
    world, cam, r, film = scenes.build(scenes.textures_example(72, 48, 16), seed=5)  # interpreter programs, textures, the hit tape
    return world, cam, r


CASES = {"c2_cornell": c2_case, "c3_shaped": c3_case, "textures_example": textures_case}


def one_shot(r, cam, world, width, height):
    film = r.new_film(width, height)
    r.render(film, cam, world)
    return film


def size_of(name):
    return {"c2_cornell": (64, 64), "c3_shaped": (64, 36), "textures_example": (72, 48)}[name]


def windows_film(r, cam, world, width, height, windows, layout=abi.PYR_FILM_ROWS):
    """The windows [a, b) rendered by one pyr_render_simple call each into ONE film."""
    total = r.pixel_samples
    film = r.new_film(width, height)
    try:
        if layout == abi.PYR_FILM_ROWS:
            for a, b in windows:
                r.pixel_samples = b - a
                r.render(film, cam, world, sample_begin=a)
        else:
            import torch

            share = Share(0, r.num_tiles(width, height), 1, abi.PYR_FILM_TILE_BLOCKS, tile_size=r.tile_size)
            blocks = np.zeros((share.pixels(width), film.bins, 2), dtype=np.float32)
            for a, b in windows:
                r.pixel_samples = b - a
                r.render(film, cam, world, window=blocks, share=share, sample_begin=a)
            whole = assemble_blocks_torch(torch.zeros(height, width, film.bins, 2), torch.from_numpy(blocks), share, r.tile_size)
            film.grains[...] = whole.numpy()
    finally:
        r.pixel_samples = total
    return film


@pytest.mark.parametrize("windows", [((0, 8), (8, 16)), ((0, 3), (3, 16))], ids=["even", "uneven"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_sample_windows_add_up_to_the_one_shot_film_and_the_oracle(name, windows, gpu_lib):
    world, cam, r = CASES[name]()
    width, height = size_of(name)
    assert r.pixel_samples == 16
    info = r.path_info(world)
    assert info["stage_scheduler"] == (0 if name == "c2_cornell" else 1) and (info["tape"] == 2) == (name == "textures_example"), info
    whole = one_shot(r, cam, world, width, height)
    cpu = r.new_film(width, height)
    oracle.OracleScene(world).render(r, cam, cpu, threads=8)
    layouts = [abi.PYR_FILM_ROWS] + ([abi.PYR_FILM_TILE_BLOCKS] if name == "c3_shaped" else [])
    for layout in layouts:
        film = windows_film(r, cam, world, width, height, windows, layout)
        assert_same_film(film, whole, "%s %r layout %d against one shot" % (name, windows, layout))
        assert_same_film(film, cpu, "%s %r layout %d against the oracle" % (name, windows, layout))
    world.close()


def test_a_window_is_not_the_first_samples_again(gpu_lib):
    world, cam, r = c2_case()
    r.pixel_samples = 4
    first, second = r.new_film(64, 64), r.new_film(64, 64)
    r.render(first, cam, world)
    r.render(second, cam, world, sample_begin=4)
    assert first.total_weight() == second.total_weight() and not np.array_equal(first.grains, second.grains)
    world.close()


def test_windows_beyond_the_chunk_bound_are_refused(gpu_lib):
    world, cam, r = c2_case()
    film = r.new_film(64, 64)
    r.pixel_samples = 1
    with pytest.raises(PyriteGpuError, match="sample window") as e:
        r.render(film, cam, world, sample_begin=0xFFFFFFFF)
    assert e.value.status == abi.PYR_ERR_UNSUPPORTED and film.total_weight() == 0
    world.close()


@pytest.mark.parametrize("halves", [False, True], ids=["one_film", "halves"])
@pytest.mark.parametrize("name", ["c2_cornell", "c3_shaped"])
def test_session_in_passes_equals_one_shot(name, halves, gpu_lib):
    world, cam, r = CASES[name]()
    width, height = size_of(name)
    whole = one_shot(r, cam, world, width, height)
    with r.session((width, height), cam, world, halves=halves) as s:
        assert s.samples_done == 0
        seen = []
        for _ in range(4):
            s.render(4)
            seen.append(s.samples_done)
        assert seen == [4, 8, 12, 16]
        s.sync()
        film = s.film()
        assert_same_film(film, whole, "%s session halves=%s" % (name, halves))
        if halves:
            a, b = s.half_films()
            assert np.array_equal(a[..., 1] + b[..., 1], whole.grains[..., 1])
            assert a[..., 1].sum(dtype=np.float64) == b[..., 1].sum(dtype=np.float64) > 0  # two passes each
            assert np.array_equal(a + b, film.grains)
        else:
            with pytest.raises(PyriteGpuError, match="PYR_SESSION_HALVES"):
                s.half_films()
        s.render(4)  # the budget is spent: nothing happens
        s.sync()
        assert s.samples_done == 16 and np.array_equal(s.film().grains, film.grains)
    with r.session((width, height), cam, world, halves=halves) as s:  # a pass that overshoots is clipped
        s.render(12)
        s.render(12)
        assert s.samples_done == 16
        assert_same_film(s.film(), whole, "%s session 12 + 12 clipped, halves=%s" % (name, halves))
    world.close()


def test_session_continues_from_a_host_film(gpu_lib):
    world, cam, r = c2_case()
    start = one_shot(r, cam, world, 64, 64)
    twice = r.new_film(64, 64)
    twice.grains[...] = start.grains
    r.render(twice, cam, world)
    with r.session((64, 64), cam, world, film=start) as s:
        s.render(16)
        film = s.film()
    assert_same_film(film, twice, "session on top of a film")
    world.close()


def test_session_arguments(gpu_lib):
    world, cam, r = c2_case()
    desc, params = r.new_film(64, 64).desc(), r.params(sample_begin=1)
    handle = C.c_void_p()
    rc = lib().pyr_session_create(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(params), 0, None, C.byref(handle))
    assert rc == abi.PYR_ERR_INVALID_ARGUMENT and b"sample_begin" in lib().pyr_last_error() and not handle
    params = r.params()
    assert lib().pyr_session_create(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(params), 2, None, C.byref(handle)) == abi.PYR_ERR_INVALID_ARGUMENT
    with r.session((64, 64), cam, world) as s:
        assert lib().pyr_session_render(s.handle, 0) == abi.PYR_ERR_INVALID_ARGUMENT
    world.close()


DEVELOP_CASES = [
    {"step": 30.0},
    {"step": 2.0},
    {"step": 30.0, "white": blackbody(4000)},
    {"step": 2.0, "filter": spectrum(format="curve", points=[(450, 0), (500, 1), (600, 1), (650, 0)]), "white": blackbody(4000)},
]


@pytest.mark.parametrize("halves", [False, True], ids=["one_film", "halves"])
@pytest.mark.parametrize("bins", [64, 50])
def test_preview_is_the_developed_film(bins, halves, gpu_lib):
    world, cam, r = c2_case()
    r.spectrum_bins = bins
    width, height = 61, 37  # ragged against the tiles and against the kernel's runs of 64 pixels
    with r.session((width, height), cam, world, halves=halves) as s:
        for done in (4, 8, 12):  # mid-render, with the halves unequal (two passes in A, one in B) at the end
            s.render(4)
            film = s.film()  # the film downloaded at the same moment
            assert film.total_weight() == width * height * done * r.spectrum_samples
            for kwargs in DEVELOP_CASES:
                shown = s.preview(kwargs["step"], filter=kwargs.get("filter"), white=kwargs.get("white"))
                expect = develop(film, step_size=kwargs["step"], filter=kwargs.get("filter"), white=kwargs.get("white"))
                assert shown.shape == (height, width, 3) and shown.dtype == np.uint8
                assert np.array_equal(shown, expect), (done, kwargs)
                assert (shown[-1, -1] == 0).all() and shown.reshape(-1, 3)[:-1].max() > 50
    world.close()


def develop_with(kernel, film, monkeypatch, **kwargs):
    monkeypatch.setenv("PYRITE_DEVELOP_KERNEL", kernel)
    return develop(film, **kwargs)


def test_wave_develop_kernel_writes_the_pixel_kernels_bytes(gpu_lib, monkeypatch):
    """develop_wave_kernel (kernels/film.hip) against develop_kernel (kernels/main.hip) on the films tests/test_develop.py develops
    and on a rendered C2 film; and both against the oracle, so that neither can drift."""
    world, cam, r, film = scenes.build(scenes.c2_cornell(96, 64, 16), seed=3)
    r.render(film, cam, world)
    world.close()
    rng = np.random.RandomState(4)
    noise = Film(33, 17, 50, (400.0, 700.0))
    noise.grains[..., 0] = rng.gamma(0.5, 1.0, size=noise.grains.shape[:-1])
    noise.grains[..., 1] = rng.randint(0, 3, size=noise.grains.shape[:-1])
    odd = Film(9, 7, 3, (400.0, 700.0))  # odd bins, an odd number of pixels: the lone last grain of a run
    odd.grains[..., 0] = rng.gamma(0.5, 1.0, size=odd.grains.shape[:-1])
    odd.grains[..., 1] = rng.randint(0, 3, size=odd.grains.shape[:-1])
    wide = Film(5, 3, 300)  # more bins than the wave kernel's rows hold: both names run develop_kernel
    wide.grains[..., 0] = rng.gamma(0.5, 1.0, size=wide.grains.shape[:-1])
    wide.grains[..., 1] = 1.0
    flat = Film(4, 3, 64)
    flat.grains[..., 0], flat.grains[..., 1] = 0.6, 2.0
    empty = Film(3, 2, 64)
    for name, f in (("c2", film), ("noise", noise), ("odd", odd), ("wide", wide), ("flat", flat), ("empty", empty)):
        for kwargs in ({}, {"step_size": 30.0}, {"white": blackbody(4000)}, {"filter": spectrum(format="curve", points=[(450, 0), (500, 1), (600, 1), (650, 0)])}):
            pixel = develop_with("pixel", f, monkeypatch, **kwargs)
            wave = develop_with("wave", f, monkeypatch, **kwargs)
            assert np.array_equal(pixel, wave), (name, kwargs)
            assert np.array_equal(wave, oracle.film_develop(f, **kwargs)), (name, kwargs)
    assert develop_with("wave", film, monkeypatch).reshape(-1, 3)[:-1].max() > 100


def noise_formula(a, b, tile_size):
    """pyr_session_noise in numpy: f32 quotients, f64 sums, per tile of the make_tiles grid."""
    def quotient(g):
        out = np.zeros(g.shape[:-1], dtype=np.float32)
        np.divide(g[..., 0], g[..., 1], out=out, where=g[..., 1] > 0)
        return out.astype(np.float64)

    qa, qb = quotient(a), quotient(b)
    height, width = qa.shape[:2]
    ty, tx = (height + tile_size - 1) // tile_size, (width + tile_size - 1) // tile_size
    out = np.zeros((ty, tx), dtype=np.float64)
    for j in range(ty):
        for i in range(tx):
            ta = qa[j * tile_size:(j + 1) * tile_size, i * tile_size:(i + 1) * tile_size]
            tb = qb[j * tile_size:(j + 1) * tile_size, i * tile_size:(i + 1) * tile_size]
            num, den = ((ta - tb) ** 2).sum(), (((ta + tb) / 2) ** 2).sum()
            out[j, i] = np.sqrt(num / den) if den != 0 else 0.0
    return out


def test_noise_is_its_formula_and_falls_with_samples(gpu_lib):
    world, cam, r = c2_case()
    r.pixel_samples = 256
    width, height = 80, 72  # tiles of 32: ragged right column and bottom row
    with r.session((width, height), cam, world) as s:
        s.render(8)
        s.render(8)
        with pytest.raises(PyriteGpuError, match="PYR_SESSION_HALVES") as e:
            s.noise()
        assert e.value.status == abi.PYR_ERR_INVALID_ARGUMENT
    with r.session((width, height), cam, world, halves=True) as s:
        s.render(8)
        with pytest.raises(PyriteGpuError, match="two passes"):
            s.noise()
        s.render(8)
        early = s.noise()
        again = s.noise()
        assert early.shape == (3, 3) and early.dtype == np.float32
        assert np.array_equal(early.view(np.uint32), again.view(np.uint32))  # no atomics: the same bits
        a, b = s.half_films()
        expect = noise_formula(a, b, r.tile_size)
        rel = np.abs(early.astype(np.float64) - expect) / np.maximum(expect, 1e-30)
        print("noise at 16 spp:", early.reshape(-1), "largest relative difference to the formula %.3g" % rel.max())
        assert (expect > 0).all() and rel.max() <= 1e-6
        while s.samples_done < 256:
            s.render(8)
        late = s.noise()
        a, b = s.half_films()
        expect = noise_formula(a, b, r.tile_size)
        assert (np.abs(late.astype(np.float64) - expect) / np.maximum(expect, 1e-30)).max() <= 1e-6
        print("noise at 256 spp:", late.reshape(-1))
        lit = early > 0
        assert lit.any() and (late[lit] < early[lit]).all()
    world.close()


def test_blocking_convenience_reports_previews_and_returns_the_one_shot_film(gpu_lib):
    world, cam, r = c2_case()
    whole = one_shot(r, cam, world, 64, 64)
    film = r.new_film(64, 64)
    desc, params = film.desc(), r.params()
    dp, keep = develop_params(film, 30.0)
    status, previews, threads = [], [], set()

    def on_status(user, percent, message):
        status.append((int(percent), message.decode()))
        threads.add(threading.get_ident())

    def on_preview(user, rgb, width, height, samples_done):
        threads.add(threading.get_ident())
        previews.append((int(samples_done), np.ctypeslib.as_array(rgb, shape=(height, width, 3)).copy()))

    scb, pcb = abi.PyrProgressFn(on_status), abi.PyrPreviewFn(on_preview)
    check(lib().pyr_render_simple_progressive(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(params), film.grains.ctypes.data, 4, scb, pcb, 0.0,
                                              C.byref(dp), None))
    percents = [p for p, _ in status]
    assert percents == sorted(percents) and percents[0] == 0 and percents[-1] == 100 and percents[1:] == [25, 50, 75, 100]
    assert all(m == "Rendering" for _, m in status)
    assert threads == {threading.get_ident()}
    assert [n for n, _ in previews] == [4, 8, 12, 16]  # interval 0: one preview per pass
    assert_same_film(film, whole, "pyr_render_simple_progressive")
    assert np.array_equal(previews[-1][1], develop(film, step_size=30.0))
    # a long interval: no preview at all; and the film is added to, as pyr_render_simple does
    previews.clear()
    check(lib().pyr_render_simple_progressive(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(params), film.grains.ctypes.data, 5, scb, pcb, 3600.0,
                                              C.byref(dp), None))
    assert previews == [] and np.array_equal(film.grains[..., 1], 2 * whole.grains[..., 1])
    rc = lib().pyr_render_simple_progressive(world.scene(0), C.byref(cam.c), C.byref(desc), C.byref(params), film.grains.ctypes.data, 0, scb, pcb, 0.0,
                                             C.byref(dp), None)
    assert rc == abi.PYR_ERR_INVALID_ARGUMENT
    del keep
    world.close()


def read_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    width, height = struct.unpack(">II", data[16:24])
    i = data.index(b"IDAT")
    n = struct.unpack(">I", data[i - 4:i])[0]
    rows = np.frombuffer(zlib.decompress(data[i + 4:i + 4 + n]), dtype=np.uint8).reshape(height, 1 + width * 3)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(height, width, 3)


def test_command_line_writes_previews_and_the_same_final_image(gpu_lib, tmp_path):
    project = os.path.join(ROOT, "tests", "golden", "projects", "gallery.lua")
    common = [sys.executable, "-m", "pyrite_amd", project, "--seed", "7", "--spp", "8", "--size", "96x64"]
    plain, passes, preview = str(tmp_path / "plain.png"), str(tmp_path / "passes.png"), str(tmp_path / "preview.png")
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run(common + ["-o", plain], check=True, cwd=ROOT, env=env, timeout=600)
    out = subprocess.run(common + ["-o", passes, "--pass-samples", "2", "--preview", preview, "--preview-every", "0", "--noise"], check=True, cwd=ROOT, env=env,
                         timeout=600, capture_output=True, text=True).stdout
    assert read_png(preview).shape == (64, 96, 3)
    assert "noise" in out
    assert open(plain, "rb").read() == open(passes, "rb").read()


LDS_REFUSAL = "spectrum_samples + BVH depth need more than 160 KB of LDS per workgroup"


def test_a_launcher_refusal_reaches_both_callers_with_its_own_words(gpu_lib, monkeypatch):
    """The one refusal of a launcher that a caller reaches without anything being launched: the synchronous walk of a scene that
    lives in LDS keeps 3 * spectrum_samples rows of 1 KB next to its stack, so 64 wavelengths need more than a workgroup's
    160 KB and launch_render says so. The code and the text arrive through pyr_render_simple and through a session's pass alike,
    nothing is rendered, and the scene renders afterwards."""
    monkeypatch.delenv("PYRITE_SCHEDULER", raising=False)
    world, cam, r, film = scenes.build(scenes.c1_spheres(8, 8, 4), seed=5)
    r.spectrum_samples = 64
    info = r.path_info(world)
    assert info["scene_in_lds"] == 1 and info["stage_scheduler"] == 0, info
    refused = "pyrite_gpu error %d: %s" % (abi.PYR_ERR_UNSUPPORTED, LDS_REFUSAL)
    with pytest.raises(PyriteGpuError) as e:
        r.render(film, cam, world)
    print("pyr_render_simple: %s" % e.value)
    assert e.value.status == abi.PYR_ERR_UNSUPPORTED and str(e.value) == refused
    assert film.total_weight() == 0
    with r.session((8, 8), cam, world) as s:
        with pytest.raises(PyriteGpuError) as e:
            s.render(4)
        print("pyr_session_render: %s" % e.value)
        assert e.value.status == abi.PYR_ERR_UNSUPPORTED and str(e.value) == refused
        assert s.samples_done == 0
    r.spectrum_samples = 4
    r.render(film, cam, world)
    assert film.total_weight() > 0 and not np.isnan(film.grains).any()
    world.close()
