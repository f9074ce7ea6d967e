"""The tape replay of the stage scheduler's builds without interpreter programs, two wavelengths per lane (kernels.hip replay_tapes,
device_scene.h tape_pairs) -- run with `-m gpu`.

An item of the replay is a path and the halves k and k + P of its S wavelengths, P = (S + 1) / 2; each half makes the single form's f32
operations in its order, so nothing a caller can see may change. Every case renders a small C3 (the x10 Cornell box with a knot of a few
hundred triangles, walked from HBM: render_kernel_sm<.., false, false, true> runs) through the ABI and compares with the CPU oracle:
per-pixel relL2 <= 1e-5 (the suite's tolerance: only the order of the film's float atomics differs), film weights and path counters
exactly. The sizes are the ones at which the pairing takes another path: odd S (a path's last item has one half), S = 1 (the hero alone,
P = 1), S = 2 (the hero in the second half of the only item), dispersed paths (one item, its hero in the first half) among full ones,
hero-only records, passes of fewer than, exactly and more than 64 items, tapes that are no multiple of the batch of four records, a
clipped tape. A scene is replayed in pairs while it has at most four spectrum-reading programs (pairs then cost no LDS the single rows
would not take: device_scene.h tape_replays_pairs); the last test holds the scenes past that: five programs (the first replayed one
wavelength per item over packed single rows), fifteen (the last row a record can name) and sixteen (looked up record by record).
The number of programs is what decides, so every scene's count of distinct spectra is asserted."""
import numpy as np
import pytest

import oracle
from pyrite_amd import abi, scenes
from pyrite_amd.project import material, shape, spectrum

pytestmark = pytest.mark.gpu
TOL = 1e-5
PATH_COUNTERS = ("samples", "extension_rays", "shadow_rays", "shaded_hits", "exposures")


@pytest.fixture(autouse=True)
def stage_scheduler(monkeypatch):
    monkeypatch.setenv("PYRITE_SCHEDULER", "sm")


def rel_l2(film, reference):
    a, b = film.develop(), reference.develop()
    return (np.sqrt(((a - b) ** 2).sum(-1)) / (np.sqrt((b ** 2).sum(-1)) + 1e-6)).reshape(-1)


def small_c3(width, height, spp, seed=1, flat=None, **renderer_fields):
    """(world, camera, renderer) of the small C3; `flat` builds another scene of its shape, `renderer_fields` set spectrum_samples, bounces, ..."""
    project = scenes.c3_mesh_in_box(width, height, spp, segments=24, sides=16)
    if flat is not None:
        project["flat"] = flat
    world, cam, r, _ = scenes.build(project, seed=seed)
    for key, value in renderer_fields.items():
        assert hasattr(r, key), key
        setattr(r, key, value)
    info = r.path_info(world)
    assert info["stage_scheduler"] == 1 and info["tape"] == 1 and info["interpreter"] == 0 and info["scene_in_lds"] == 0, info
    return world, cam, r


def assert_matches_the_oracle(world, cam, r, width, height, what):
    """One render with counters against the oracle: film, weights, path counters. Returns the GPU film."""
    cpu = r.new_film(width, height)
    ccount = oracle.OracleScene(world).render(r, cam, cpu, threads=8)
    gpu = r.new_film(width, height)
    gcount = r.render(gpu, cam, world, counters=True)
    e = rel_l2(gpu, cpu)
    worst = float(e.max()) if e.size else 0.0
    print("%s: relL2 median %.3g max %.3g, weight %d, counters %r" % (what, np.median(e), worst, gpu.grains[..., 1].sum(dtype=np.float64),
                                                                         {k: (gcount[k], ccount[k]) for k in PATH_COUNTERS}))
    assert not np.isnan(gpu.grains).any(), what
    assert np.array_equal(gpu.grains[..., 1], cpu.grains[..., 1]), what + ": film weights differ"
    assert worst <= TOL, (what, worst)
    for key in PATH_COUNTERS:
        assert gcount[key] == ccount[key], (what, key, gcount[key], ccount[key])
    return gpu


def knot_flat(mesh_material=None, spectra_in_front=0, glass=False, lamp_probability=None, one_wall_colour=False):
    """scenes.c3_flat with a knot of 768 triangles, and: `spectra_in_front` unused diffuse materials of distinct array spectra compiled
    BEFORE the box's (their programs take the first value slots of the replay, the scene's own the ones behind them); `lamp_probability`,
    an expression the lamp's emissive component gets as its probability program (one that reads the wavelength makes the lamp's light
    samples hero-only records); `one_wall_colour` paints the green wall red (one spectrum-reading program less)."""
    from pyrite_amd.compiler import FlatScene

    def build():
        flat = FlatScene()
        rng = np.random.default_rng(1)
        for k in range(spectra_in_front):
            points = [float(x) for x in rng.uniform(0.1, 0.9, 5 + k)]
            flat.add_material({"surface": material.diffuse(color=spectrum(format="array", min=400.0, max=700.0, points=points))})
        m = scenes.cornell_materials()
        if one_wall_colour:
            m["green"] = m["red"]
        box = scenes._box_mesh(drop=("tall", "short"))
        flat.add_world({"objects": [shape.mesh(file=box, scale=10.0, materials=scenes._box_materials(m, [o["name"] for o in box["objects"]]))]})
        if glass:
            surface = material.refractive(ior=1.5, dispersion=0.01371, color=1)
        else:
            surface = mesh_material if mesh_material is not None else material.diffuse(color=0.8)
        mat, _ = flat.add_material({"surface": surface})
        positions, normals = scenes.torus_knot_mesh(segments=24, sides=16)
        flat.add_triangles(positions, normals, mat)
        if lamp_probability is not None:
            program = flat.compile(lamp_probability)
            lamps = [c for c in flat.components if c["bsdf"] == abi.BSDF_EMISSIVE]
            assert lamps
            for c in lamps:
                c["probability"] = program
        return flat

    return build


@pytest.mark.parametrize("spectrum_samples,seed", [(1, 1), (2, 2), (3, 3), (4, 1), (7, 2), (10, 3)])
def test_wavelength_counts(spectrum_samples, seed, gpu_lib):
    """S = 1: P = 1, the hero alone, no second half. 2: one item, the hero its second half. 3: P = 2, the hero in the first half of the
    second item, whose second half is no wavelength. 4: P = 2, the hero the second half of the last item. 7 and 10: the same two
    shapes with several items a path. 64 x 36 at 4 spp: 2,304 paths a tile, so most replays hold 16 paths or more."""
    world, cam, r = small_c3(64, 36, 4, seed=seed, spectrum_samples=spectrum_samples)
    gpu = assert_matches_the_oracle(world, cam, r, 64, 36, "S = %d" % spectrum_samples)
    weight, most = gpu.grains[..., 1].sum(dtype=np.float64), 64 * 36 * 4 * spectrum_samples
    assert 0.999 * most <= weight <= most  # a diffuse scene: every sample exposes its S wavelengths (bar one outside the film's span)
    world.close()


@pytest.mark.parametrize("spectrum_samples", [3, 10])
def test_dispersed_paths_among_full_ones(spectrum_samples, gpu_lib):
    """The knot of dispersive glass in the diffuse box, 6 bounces: a path that dispersed is ONE item whose only half is the hero, listed
    behind the items of the paths that kept their companions -- both kinds in one pass. The weight bound is the benchmark's for C5."""
    world, cam, r = small_c3(64, 36, 4, seed=2, flat=knot_flat(glass=True), bounces=6, spectrum_samples=spectrum_samples)
    gpu = assert_matches_the_oracle(world, cam, r, 64, 36, "glass, S = %d" % spectrum_samples)
    samples = 64 * 36 * 4
    weight = gpu.grains[..., 1].sum(dtype=np.float64)
    assert samples * (1 - 1e-5) <= weight < samples * spectrum_samples  # some paths dispersed (hero only), none exposed more than S
    world.close()


@pytest.mark.parametrize("spectrum_samples", [4, 7])
def test_hero_only_records(spectrum_samples, gpu_lib):
    """The lamp's emissive component under a probability program that reads the wavelength (a plain spectrum: no interpreter): its
    light samples are recorded for the hero alone, and each half of an item skips them unless it is the hero -- in the second half
    of a path's last item (S = 4) and in the first (S = 7)."""
    probability = spectrum(format="array", min=400.0, max=700.0, points=[0.9, 0.6, 0.8, 0.5, 0.7])
    flat = knot_flat(lamp_probability=probability, one_wall_colour=True)
    built = flat()
    assert any(c["bsdf"] == abi.BSDF_EMISSIVE and c["probability"] >= 0 for c in built.components)
    assert len(built.spectra) == 4  # lamp, white, red and the probability: four programs, replayed in pairs
    world, cam, r = small_c3(64, 36, 4, seed=3, flat=flat, spectrum_samples=spectrum_samples)
    assert_matches_the_oracle(world, cam, r, 64, 36, "hero-only lamp, S = %d" % spectrum_samples)
    world.close()


@pytest.mark.parametrize("expose_lanes", ["12", "13", "64"])
def test_items_across_the_pass_boundary(expose_lanes, monkeypatch, gpu_lib):
    """S = 10, P = 5: a replay of 12 finished lanes is 60 items, of 13 is 65 -- one item into a second pass, its path's other items in
    the first -- and with a quorum of 64 lanes up to 320 items, five full passes."""
    monkeypatch.setenv("PYRITE_SM_EXPOSE_LANES", expose_lanes)
    world, cam, r = small_c3(64, 36, 4, seed=1)
    assert r.spectrum_samples == 10
    assert_matches_the_oracle(world, cam, r, 64, 36, "expose quorum " + expose_lanes)
    world.close()


@pytest.mark.parametrize("width,height,spp,spectrum_samples", [(1, 1, 1, 10), (1, 1, 1, 3), (3, 2, 2, 7)], ids=["1x5", "1x2", "12x4"])
def test_fewer_items_than_one_pass(width, height, spp, spectrum_samples, gpu_lib):
    """One path (5 items, or 2 of which one has one half) and twelve (48 items): every pass is partly empty."""
    world, cam, r = small_c3(width, height, spp, seed=2, spectrum_samples=spectrum_samples)
    assert_matches_the_oracle(world, cam, r, width, height, "%d paths, S = %d" % (width * height * spp, spectrum_samples))
    world.close()


@pytest.mark.parametrize("bounces,light_samples", [(1, 1), (3, 2), (8, 4)])
def test_tape_lengths_around_the_batch(bounces, light_samples, gpu_lib):
    """A tape holds at most 2 bounces + 2 light_samples + 1 records: 5 (one batch of four and one record), 11 and 25, and every
    shorter length a path ends with -- rows past a tape's end replay the identity record in both halves."""
    world, cam, r = small_c3(64, 36, 4, seed=1, bounces=bounces, light_samples=light_samples)
    assert_matches_the_oracle(world, cam, r, 64, 36, "%d bounces, %d light samples" % (bounces, light_samples))
    world.close()


def test_a_clipped_tape_raises_and_the_next_render_is_whole(monkeypatch, gpu_lib):
    """PYRITE_TEST_TAPE_OPS = 3: paths want more records than the tape holds; the replay walks the three it has and the render fails
    with the overflow word's error. The switch gone, the same objects render the oracle's film."""
    from pyrite_amd._lib import PyriteGpuError

    world, cam, r = small_c3(64, 36, 4, seed=2)
    monkeypatch.setenv("PYRITE_TEST_TAPE_OPS", "3")
    with pytest.raises(PyriteGpuError, match="spectral tape"):
        r.render(r.new_film(64, 36), cam, world)
    monkeypatch.delenv("PYRITE_TEST_TAPE_OPS")
    assert_matches_the_oracle(world, cam, r, 64, 36, "after the clipped tape")
    world.close()


def test_the_scenes_replayed_in_pairs_have_four_spectra(gpu_lib):
    """What the cases above rest on: the box's lamp, white, red and green are the scene's spectrum-reading programs, and glass adds none."""
    assert len(scenes.c3_flat(segments=24, sides=16).spectra) == 4
    assert len(knot_flat(glass=True)().spectra) == 4


@pytest.mark.parametrize("spectra_in_front,what", [(0, "five programs: single rows"), (10, "the last value row"), (11, "one program too many: record by record")])
def test_value_rows_up_to_the_last_and_past_it(spectra_in_front, what, gpu_lib):
    """The box has four spectrum-reading programs (lamp, white, red, green) and the knot here a fifth: pairs would take more LDS than
    single rows, so the scene is replayed one wavelength per item over packed single rows (1.0 in row 2). With 10 more in front of them
    the knot's is slot 14, row 15 of 16, the last one. With 11 the scene needs a seventeenth row: the replay looks values up record by
    record."""
    colour = spectrum(format="array", min=420.0, max=680.0, points=[0.7, 0.2, 0.5, 0.9, 0.3, 0.6])
    flat = knot_flat(mesh_material=material.diffuse(color=colour), spectra_in_front=spectra_in_front)
    assert len(flat().spectra) == 5 + spectra_in_front
    world, cam, r = small_c3(64, 36, 4, seed=3, flat=flat, spectrum_samples=7)
    assert_matches_the_oracle(world, cam, r, 64, 36, what)
    world.close()
