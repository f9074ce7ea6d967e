"""The HIP path against tests/closed_forms.py -- no oracle anywhere in this file. Point, directional and sphere lamps, planes,
the refractive BSDF's branch probabilities and weights, dispersion per wavelength bin, `mix` / `fresnel` component
probabilities, the pixel-to-ray mapping on a non-square image and the thin lens, each under both schedulers, on 40 x 24 images
with 16-pixel tiles (cut tiles in both directions). tests/test_closed_forms_cpu.py holds the same statements against the oracle
on the CPU, so a failure here is a difference between the kernels and the oracle, not a wrong derivation.

Sphere lamp with next-event estimation: the reference rejects a light sample when the shadow ray's re-intersection of the lamp
comes out nearer than the sampled point by more than DIST_EPSILON in squared distance (tracer.rs:381-389), a float32 accident
that grows with distance. At (1.5, 0, 1), r = 0.25 the oracle's deficit is 0.052 % / 0.055 % (1 / 4 light
samples, 16384 samples per pixel on the CPU); those two cases get an extra allowance of twice that, 0.104 % / 0.110 % of the
expectation (closed_forms.NEE_ALLOWANCE)."""
import json
import os

import pytest

import closed_forms as cf

pytestmark = pytest.mark.gpu

CASES = cf.cases()


@pytest.fixture(scope="module")
def gpu_lib():
    from pyrite_amd import _lib

    lib = _lib.lib()
    if lib.pyr_device_count() < 1:
        pytest.fail("no HIP device: the closed-form tests need a GPU and pyrite_amd has no CPU path")
    return lib


@pytest.fixture(scope="module")
def observed():
    """Every assertion's observed deviation and bound; written as closed_forms_observed.json into the directory
    PYRITE_OBSERVED_DIR names, where that is set and exists. Nothing reads the file back."""
    records = []
    yield records
    out = os.environ.get("PYRITE_OBSERVED_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "closed_forms_observed.json"), "w") as f:
            json.dump(records, f, indent=1)


@pytest.mark.parametrize("scheduler", ["sync", "sm"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernels_meet_the_closed_form(case, scheduler, gpu_lib, observed, monkeypatch):
    from pyrite_amd import project as P
    from pyrite_amd import scenes

    monkeypatch.setenv("PYRITE_SCHEDULER", scheduler)
    films, S = {}, None
    for name, project in cf.build_projects(case, P, scenes._mesh_dict_from_arrays).items():
        world, cam, r, film = scenes.build(project, seed=1)
        r.render(film, cam, world)
        films[name], S = film.grains, r.spectrum_samples
        assert film.total_weight() > 0
        world.close()
    checks = case.checks(films, S)
    observed.extend(dict(c.record(), case=case.name, scheduler=scheduler) for c in checks)
    cf.assert_checks(checks, resolution=case.resolution)
