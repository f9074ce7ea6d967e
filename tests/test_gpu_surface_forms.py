"""The HIP path against tests/surface_forms.py -- no oracle anywhere in this file. Texture lookup (widths 1 to 16, both load paths
of `texture_get`, wrap-around, texel boundaries), linearisation and the RGB basis, the texture coordinates and tangent frames of
triangles, planes and spheres (seam and pole), normal maps, and triangle lamps (chance hits, next-event estimation, the lamp pick,
|cos_in|, a texture read at the sampled point), each under both schedulers on 40 x 24 images with 16-pixel tiles.

Exact cases go through the first-hit feature pass at grid 1, a pure function of the pixel-centre ray, against a float64 form of the
same ray; their bounds are four times the largest |oracle - form| measured on the CPU (surface_forms.BOUNDS, never a figure from
the kernels). Stochastic cases are rendered films under closed_forms.py's fixed rule, 5 sigma1 / sqrt(N) + 1e-4, with sample counts
at which that is just under 1 % of the expectation. tests/test_surface_forms_cpu.py holds the same statements against the oracle, so
a failure here is a difference between the kernels and the oracle, not a wrong derivation."""
import json
import os

import numpy as np
import pytest

import closed_forms as cf
import surface_forms as sf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tables():
    with np.load(os.path.join(ROOT, "pyrite_amd", "data", "tables.npz")) as z:
        return {k: z[k] for k in z.files}


TABLES = tables()
EXACT = sf.exact_cases(TABLES)
STOCHASTIC = sf.stochastic_cases(TABLES)
SCHEDULERS = ["sync", "sm"]


@pytest.fixture(scope="module")
def gpu_lib():
    from pyrite_amd import _lib

    lib = _lib.lib()
    if lib.pyr_device_count() < 1:
        pytest.fail("no HIP device: the surface-form tests need a GPU and pyrite_amd has no CPU path")
    return lib


@pytest.fixture(scope="module")
def observed():
    """Every assertion's observed deviation and bound; written as surface_forms_observed.json into the directory
    PYRITE_OBSERVED_DIR names, where that is set and exists. Nothing reads the file back."""
    records = []
    yield records
    out = os.environ.get("PYRITE_OBSERVED_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "surface_forms_observed.json"), "w") as f:
            json.dump(records, f, indent=1)


def features_of(case):
    """(Features, texture offsets of the scene) of an exact case: one feature pass at grid 1."""
    from pyrite_amd import project as P
    from pyrite_amd import scenes

    world, cam, r, _ = scenes.build(case.project(P), seed=1)
    got = r.features((case.width, case.height), cam, world, grid=1, albedo_bins=case.bins)
    offsets = [int(world.desc.textures[k].offset) for k in range(world.desc.num_textures)]
    world.close()
    return got, offsets


@pytest.mark.parametrize("scheduler", SCHEDULERS)
@pytest.mark.parametrize("case", EXACT, ids=[c.name for c in EXACT])
def test_feature_pass_meets_the_exact_form(case, scheduler, gpu_lib, observed, monkeypatch):
    monkeypatch.setenv("PYRITE_SCHEDULER", scheduler)
    got, _ = features_of(case)
    checks = case.checks(got.albedo.grains, got.normal, got.depth, got.coverage)
    observed.extend(dict(c.record(), case=case.name, scheduler=scheduler) for c in checks)
    cf.assert_checks(checks)


@pytest.mark.parametrize("scheduler", SCHEDULERS)
def test_both_load_paths_of_the_lookup_give_the_same_film(scheduler, gpu_lib, monkeypatch):
    """The same colour texture once at texel offset 0 (16-byte aligned: `texture_get`'s float4 path) and once at offset 9, behind a
    3 x 3 mono texture (`offset & 3` != 0: the generic path). The offsets are read from the scene description, so both paths are
    known to be taken; the two albedo films must be equal bit for bit (each meets the form in the test above)."""
    monkeypatch.setenv("PYRITE_SCHEDULER", scheduler)
    aligned, offset = (next(c for c in EXACT if c.name == name) for name in sf.LOAD_PATH_PAIR)
    (a, offsets_a), (b, offsets_b) = features_of(aligned), features_of(offset)
    assert offsets_a == [0] and offsets_b == [0, 9] and offsets_a[0] % 4 == 0 and offsets_b[1] % 4 != 0
    assert np.array_equal(a.albedo.grains, b.albedo.grains) and a.albedo.grains[..., 0].any()
    assert np.array_equal(a.normal, b.normal) and np.array_equal(a.depth, b.depth)


def test_the_wide_case_needs_the_wide_interpreter_build(gpu_lib):
    """surface_forms.WIDE_BUILD is the case whose texture values go through `wide::features_kernel`: its programs must be refused
    by the in-register build, and every other exact case must fit it."""
    from pyrite_amd import project as P
    from pyrite_amd import scenes

    for case in EXACT:
        world, _, r, _ = scenes.build(case.project(P), seed=1)
        assert r.program_info(world)["wide"] == (1 if case.name == sf.WIDE_BUILD else 0), case.name
        world.close()


def render(case, hit_tape=None, monkeypatch=None):
    from pyrite_amd import project as P
    from pyrite_amd import scenes

    if hit_tape is not None:
        monkeypatch.setenv("PYRITE_HIT_TAPE", hit_tape)  # read when the scene is created
    else:
        monkeypatch.delenv("PYRITE_HIT_TAPE", raising=False)
    world, cam, r, film = scenes.build(cf.build_projects(case, P, None)["main"], seed=1)
    info = r.path_info(world)
    r.render(film, cam, world)
    assert film.total_weight() > 0
    world.close()
    return film.grains, r.spectrum_samples, info


@pytest.mark.parametrize("scheduler", SCHEDULERS)
@pytest.mark.parametrize("case", STOCHASTIC, ids=[c.name for c in STOCHASTIC])
def test_kernels_meet_the_stochastic_form(case, scheduler, gpu_lib, observed, monkeypatch):
    monkeypatch.setenv("PYRITE_SCHEDULER", scheduler)
    grains, S, info = render(case, None, monkeypatch)
    if "textured" in case.name:  # a texture needs the interpreter, which lives in the stage scheduler whatever PYRITE_SCHEDULER says
        assert info["interpreter"] == 1 and info["stage_scheduler"] == 1, info
    if case.name == "emissive_textured_quad":  # spectrum x constant x texture is a PRODUCT, and four wavelengths record a hit tape
        assert info["tape"] == 2, info
    checks = case.checks({"main": grains}, S)
    observed.extend(dict(c.record(), case=case.name, scheduler=scheduler, tape=info["tape"]) for c in checks)
    cf.assert_checks(checks, resolution=case.resolution)


@pytest.mark.parametrize("scheduler", SCHEDULERS)
def test_the_online_interpreter_meets_the_emissive_texture_too(scheduler, gpu_lib, observed, monkeypatch):
    """`d65 * k * texture` is a PRODUCT on the hit tape (`tape` 2, asserted in the test above); with PYRITE_HIT_TAPE=0 the same
    scene keeps every wavelength online (`tape` 0) and must meet the same form."""
    monkeypatch.setenv("PYRITE_SCHEDULER", scheduler)
    case = STOCHASTIC[0]
    assert case.name == "emissive_textured_quad"
    grains, S, info = render(case, "0", monkeypatch)
    assert info["interpreter"] == 1 and info["tape"] == 0, info
    checks = case.checks({"main": grains}, S)
    observed.extend(dict(c.record(), case=case.name + "_online", scheduler=scheduler, tape=info["tape"]) for c in checks)
    cf.assert_checks(checks, resolution=case.resolution)
