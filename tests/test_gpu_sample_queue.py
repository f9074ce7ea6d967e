"""The stage scheduler's queue of ready sample starts (kernels.hip Walker::expose_and_restart) -- run with `-m gpu`.

The tape builds without interpreter programs start their samples 64 at a time: a wave computes the starts of a whole chunk at full
width, appends those that exist to a ring in global memory, and a lane that needs a sample pops one. A sample's start is a function
of (seed, tile, iteration) alone and the film is a sum of atomics, so nothing a caller can see may change: every case renders a
C3-shaped scene that is walked from HBM (768 triangles: the kernel the queue lives in runs) and compares with the CPU oracle --
per-pixel relL2 <= 1e-5 (the suite's tolerance: only the order of the float atomics differs), film weights and the path counters
exactly. The sizes are the ones at which the queue's bookkeeping takes another path: tiles and chunks that are no multiple of 64,
launches of less than, exactly and one more than a fill, waves that never get a chunk, chunk windows, sample windows, strided tiles."""
import numpy as np
import pytest

import oracle
from pyrite_amd import scenes

pytestmark = pytest.mark.gpu
TOL = 1e-5
PATH_COUNTERS = ("samples", "extension_rays", "shadow_rays", "shaded_hits", "exposures")


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


def mesh_scene(width, height, spp, seed=1, spectrum_samples=None, **kw):
    """(world, camera, renderer) of the small C3: the x10 Cornell box with a 768-triangle knot, walked from HBM by the stage scheduler."""
    world, cam, r, _ = scenes.build(scenes.c3_mesh_in_box(width, height, spp, segments=24, sides=16, **kw), seed=seed)
    if spectrum_samples is not None:
        r.spectrum_samples = spectrum_samples
    info = r.path_info(world)
    assert info["stage_scheduler"] == 1 and info["tape"] == 1 and info["interpreter"] == 0 and info["scene_in_lds"] == 0, info
    assert r.tile_size == 32
    return world, cam, r


def oracle_film(world, cam, r, width, height):
    film = r.new_film(width, height)
    return film, oracle.OracleScene(world).render(r, cam, film, threads=8)


def assert_matches_the_oracle(world, cam, r, width, height, what):
    """One render with counters against the oracle: film, weights, path counters. Returns (gpu film, oracle film)."""
    cpu, ccount = oracle_film(world, cam, r, width, height)
    gpu = r.new_film(width, height)
    gcount = r.render(gpu, cam, world, counters=True)
    print("%s: counters %r" % (what, {k: (gcount[k], ccount[k]) for k in PATH_COUNTERS}))
    assert_same_film(gpu, cpu, what)
    for key in PATH_COUNTERS:
        assert gcount[key] == ccount[key], (what, key, gcount[key], ccount[key])
    return gpu, cpu


@pytest.mark.parametrize("seed", [1, 3])
def test_ragged_tiles_and_partial_chunks(seed, gpu_lib):
    """41 x 23 at 3 spp in tiles of 32: a 32 x 23 and a 9 x 23 tile, 2208 and 621 iterations -- neither a multiple of 64, so both end
    in a partial fill, and the cut tile leaves chunk numbers with no iteration at all (fills that append nothing)."""
    world, cam, r = mesh_scene(41, 23, 3, seed=seed)
    assert (32 * 23 * 3, 9 * 23 * 3) == (2208, 621)
    gpu, _ = assert_matches_the_oracle(world, cam, r, 41, 23, "41x23x3 seed %d" % seed)
    assert gpu.total_weight() > 0
    world.close()


@pytest.mark.parametrize("width,height,spp", [(1, 1, 1), (7, 9, 1), (8, 8, 1), (5, 13, 1), (8, 8, 2), (3, 43, 1)],
                         ids=["1", "63", "64", "65", "128", "129"])
def test_fill_boundaries(width, height, spp, gpu_lib):
    """1, 63, 64, 65, 128 and 129 samples in all: less than one fill, exactly one, one more than one, two, and (3 x 43: two tiles of
    96 and 33 iterations) partial fills in a row -- in launches where most waves of the grid get no chunk and end at once."""
    world, cam, r = mesh_scene(width, height, spp, seed=2)
    gpu, _ = assert_matches_the_oracle(world, cam, r, width, height, "%dx%dx%d" % (width, height, spp))
    assert gpu.grains[..., 1].sum(dtype=np.float64) <= width * height * spp * r.spectrum_samples
    world.close()


def test_tile_ranges_add_up_to_the_whole(gpu_lib):
    world, cam, r = mesh_scene(70, 40, 3, seed=4)  # 3 x 2 tiles, both edges cut
    whole, _ = assert_matches_the_oracle(world, cam, r, 70, 40, "70x40x3 whole")
    parts = r.new_film(70, 40)
    for lo, hi in ((0, 2), (2, 3), (3, 6)):
        r.render(parts, cam, world, tile_range=(lo, hi))
    assert np.array_equal(whole.grains[..., 1], parts.grains[..., 1])
    assert np.allclose(whole.grains, parts.grains, rtol=1e-5)
    world.close()


def test_chunk_windows_of_a_progress_callback_equal_one_launch(gpu_lib):
    """With a progress callback the chunk range is cut into one launch per 4096 chunks at least: 128 x 128 x 48 is 12288 chunks of
    768 per tile, so the two cuts fall inside tiles -- every launch starts and ends with empty queues, and no sample is lost or
    started twice at a cut. (The largest case of this file: 786 k samples, the fewest that make a wave of the full grid take three chunks.)"""
    world, cam, r = mesh_scene(128, 128, 48, seed=5)
    # one launch: three chunks a wave of the full grid, so every ring of 128 entries wraps and is filled over entries already popped
    plain, _ = assert_matches_the_oracle(world, cam, r, 128, 128, "128x128x48 one launch")
    sliced = r.new_film(128, 128)
    seen = []
    r.render(sliced, cam, world, on_status=lambda percent, message: seen.append(percent))
    assert seen == [0, 33, 66, 100], seen  # three launches
    assert_same_film(sliced, plain, "three chunk windows against one launch")
    world.close()


def test_sample_windows_of_a_session_equal_one_render_of_the_sum(gpu_lib):
    world, cam, r = mesh_scene(41, 23, 8, seed=6)
    whole, cpu = assert_matches_the_oracle(world, cam, r, 41, 23, "41x23x8 one shot")
    with r.session((41, 23), cam, world) as s:
        s.render(3)  # samples [0, 3)
        s.render(5)  # samples [3, 8): sample_begin = 3
        assert s.samples_done == 8
        s.sync()
        film = s.film()
    assert_same_film(film, whole, "session 3 + 5 against one shot")
    assert_same_film(film, cpu, "session 3 + 5 against the oracle")
    windows = r.new_film(41, 23)
    r.pixel_samples = 3
    r.render(windows, cam, world)
    r.pixel_samples = 5
    r.render(windows, cam, world, sample_begin=3)
    r.pixel_samples = 8
    assert_same_film(windows, cpu, "windows [0, 3) + [3, 8) against the oracle")
    world.close()


def test_shares_of_three_ranks_equal_the_single_device_film(gpu_lib):
    """The native multi-device entry with one GPU standing in for three ranks: every rank one launch over its strided tiles
    (tile_stride 3) into ringed tile blocks. (The entry returns no counters: films and weights.)"""
    world, cam, r = mesh_scene(48, 40, 4, seed=7)
    r.tile_size = 16  # 3 x 3 tiles, the bottom row cut: three tiles a rank
    whole, cpu = assert_matches_the_oracle(world, cam, r, 48, 40, "48x40x4 one device")
    multi = r.new_film(48, 40)
    r.render_multi(multi, cam, world, devices=[0, 0, 0])
    assert np.array_equal(multi.grains[..., 1], whole.grains[..., 1])
    assert np.allclose(multi.grains, whole.grains, rtol=1e-5)
    assert_same_film(multi, cpu, "three ranks against the oracle")
    world.close()


def test_dispersed_paths(gpu_lib):
    """The mesh made of dispersive glass, 6 bounces: the companions travel through the queue with every start, and a path that
    disperses exposes its hero wavelength only."""
    world, cam, r = mesh_scene(33, 17, 4, seed=8, glass=True, bounces=6)
    gpu, _ = assert_matches_the_oracle(world, cam, r, 33, 17, "glass 33x17x4")
    samples = 33 * 17 * 4
    assert samples <= gpu.grains[..., 1].sum(dtype=np.float64) < samples * r.spectrum_samples  # some paths dispersed
    world.close()


@pytest.mark.parametrize("spectrum_samples", [1, 7])
def test_other_wavelength_counts(spectrum_samples, gpu_lib):
    """An entry of the queue is 11 + S words: one wavelength (no companions at all) and seven."""
    world, cam, r = mesh_scene(24, 24, 4, seed=9, spectrum_samples=spectrum_samples)
    gpu, _ = assert_matches_the_oracle(world, cam, r, 24, 24, "S = %d" % spectrum_samples)
    weight, most = gpu.grains[..., 1].sum(dtype=np.float64), 24 * 24 * 4 * spectrum_samples
    assert 0.999 * most <= weight <= most  # a diffuse scene: every sample exposes its S wavelengths (bar one outside the film's span)
    world.close()
