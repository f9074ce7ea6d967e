"""tests/closed_forms.py held on the CPU, from both sides. (a) The algebra: every closed form against a brute-force float64
evaluation of the same quantity that does not use it. (b) The oracle: every scene of the GPU test rendered by
oracle/oracle.cpp at a sixteenth of the GPU test's samples and checked by the same `assert_checks`, with N from the film.
A red tests/test_gpu_closed_forms.py then means kernel != oracle, not a wrong derivation."""
import itertools

import numpy as np
import pytest

import closed_forms as cf

CASES = cf.cases()


# ------------------------------------------------------------------------------------------------
# (a) the algebra
# ------------------------------------------------------------------------------------------------
def cap_quadrature(f, cos_gamma, cos_alpha, nodes=96, turns=512):
    """Integral over the cap of half-angle alpha of f(n.w) d(omega), by Gauss-Legendre in cos(theta) and the (spectrally exact)
    periodic trapezoid rule in the azimuth, with n.w from explicit vectors: the axis is z, n lies in the xz plane."""
    t, wt = np.polynomial.legendre.leggauss(nodes)
    c = 0.5 * (1.0 - cos_alpha) * t + 0.5 * (1.0 + cos_alpha)
    wt = wt * 0.5 * (1.0 - cos_alpha)
    phi = (np.arange(turns) + 0.5) * 2.0 * np.pi / turns
    s = np.sqrt(1.0 - c * c)
    w = np.stack([s[:, None] * np.cos(phi), s[:, None] * np.sin(phi), c[:, None] + 0.0 * phi], axis=-1)
    n = np.array([np.sqrt(1.0 - cos_gamma ** 2), 0.0, cos_gamma])
    return (f(np.maximum(w @ n, 0.0)) * wt[:, None]).sum() * 2.0 * np.pi / turns


@pytest.mark.parametrize("centre,radius,x", [((1.5, 0, 1), 0.25, (0, 0, 0)), ((1.5, 0, 1), 0.25, (-0.8, 0.5, 0)), ((3, 0, 2), 0.5, (0.3, -0.2, 0)), ((0, 0, 1), 0.9, (0, 0, 0))])
def test_sphere_lamp_radiance_is_the_cosine_weighted_integral_over_the_sphere(centre, radius, x):
    """rho / pi times the integral of L cos over the directions that meet the sphere, the sphere wholly above the horizon."""
    v = np.array(centre, dtype=np.float64) - np.array(x, dtype=np.float64)
    d = np.linalg.norm(v)
    cos_g, cos_a = v[2] / d, np.sqrt(1.0 - (radius / d) ** 2)
    brute = 0.5 / np.pi * cap_quadrature(lambda c: c, cos_g, cos_a)
    assert cf.sphere_lamp_radiance(0.5, 1.0, radius, d, cos_g) == pytest.approx(brute, rel=1e-6)
    omega = 2.0 * np.pi * (1.0 - cos_a)
    m1, m2 = cf.cap_moments(cos_g, cos_a)
    assert m1 == pytest.approx(cap_quadrature(lambda c: c, cos_g, cos_a) / omega, rel=1e-6)
    assert m2 == pytest.approx(cap_quadrature(lambda c: c * c, cos_g, cos_a) / omega, rel=1e-6)


@pytest.mark.parametrize("width_deg", [20.0, 5.0, 50.0])
def test_cone_mean_of_the_cosine_for_the_directional_lamp(width_deg):
    """The directional lamp of width cos(20 deg) about (0.6, 0, 0.8): mean and mean square of max(n.w, 0) over the cone."""
    cos_a = np.cos(np.radians(width_deg))
    omega = 2.0 * np.pi * (1.0 - cos_a)
    m1, m2 = cf.cap_moments(cf.SUN[2], cos_a)
    assert m1 == pytest.approx(cap_quadrature(lambda c: c, cf.SUN[2], cos_a) / omega, rel=1e-6)
    assert m2 == pytest.approx(cap_quadrature(lambda c: c * c, cf.SUN[2], cos_a) / omega, rel=1e-6)


def test_thin_lens_edge_profile_against_a_lens_and_pixel_monte_carlo():
    """10^6 numpy samples of (pixel jitter, lens point) per pixel traced through closed_forms.rays to the quad's plane: the share
    that lands on the quad is the pixel's expectation, within 5 of the Monte Carlo's own standard errors."""
    w, h, quad_z, half, aperture = 40, 24, 2.5, np.array([0.4, 0.3]), 0.04
    cam = cf.Camera((0, 0, 5), (0, 0, 0), fov=40, focus_distance=5.0, aperture=aperture)
    pin = cf.Camera((0, 0, 5), (0, 0, 0), fov=40)
    blur = np.sqrt(aperture) * 0.5
    rng = np.random.RandomState(7)
    n = 10 ** 6
    for px, py, axis in ((10, 12, 0), (11, 9, 0), (29, 14, 0), (12, 11, 0), (20, 5, 1), (17, 18, 1)):
        u, v = rng.uniform(size=n), rng.uniform(size=n)
        radius, psi = np.sqrt(aperture * rng.uniform(size=n)), 2.0 * np.pi * rng.uniform(size=n)  # cameras.rs:84-87
        p = cf.plane_hit(*cf.rays(cam, w, h, px, py, u, v, lens=(radius * np.cos(psi), radius * np.sin(psi))), quad_z)
        seen = (np.abs(p[:, 0]) <= half[0]) & (np.abs(p[:, 1]) <= half[1])
        t = (np.arange(cf.MIDPOINTS) + 0.5) / cf.MIDPOINTS
        vv, uu = np.meshgrid(t, t, indexing="ij")
        x = cf.plane_hit(*cf.rays(pin, w, h, px, py, uu, vv), quad_z)
        expected = cf.disc_segment((half[axis] - np.abs(x[..., axis])) / blur).mean()
        assert 0.02 < expected < 0.999
        assert abs(seen.mean() - expected) <= 5.0 * np.sqrt(expected * (1.0 - expected) / n) + 1e-4, (px, py, seen.mean(), expected)


@pytest.mark.parametrize("cos_theta", [1.0, 0.7, 0.196, 0.05])
def test_refraction_moments_by_enumeration_of_the_branches(cos_theta):
    """refractive.rs:80-90 written out branch by branch: the half-space (reflected light 1, transmitted light 0), the glass sphere
    (every path up to the cut enumerated with its probability and weight) and the three mixes."""
    re = cf.schlick(cos_theta, 1.5)
    p = 0.25 + 0.5 * re
    branches = [(p, re / p * 1.0), (1.0 - p, (1.0 - re) / (1.0 - p) * 0.0)]
    m1, m2 = cf.refract_moments(re)
    assert m1 == pytest.approx(sum(q * v for q, v in branches), rel=1e-12) and m2 == pytest.approx(sum(q * v * v for q, v in branches), rel=1e-12)
    segments = 9
    paths = [(p, re / p)]
    for k in range(segments - 2):  # enter, k inner reflections, leave: k + 3 segments
        paths.append(((1.0 - p) * p ** k * (1.0 - p), ((1.0 - re) / (1.0 - p)) ** 2 * (re / p) ** k))
    g1, g2 = cf.glass_sphere_moments(re, segments)
    assert g1 == pytest.approx(sum(q * v for q, v in paths), rel=1e-12) and g2 == pytest.approx(sum(q * v * v for q, v in paths), rel=1e-12)
    assert cf.glass_sphere_moments(re, 64)[0] == pytest.approx(1.0 - (1.0 - re) * re ** 62, rel=1e-12)  # the furnace: nothing is lost but the cut's tail
    # the fresnel mix: mirror (1/2, weight 2 F), diffuse (1/2, weight 2 (1 - F) 0.5 2 c, c uniform: 4096 midpoints)
    f = cf.reference_fresnel(cos_theta, 1.5)
    c = (np.arange(4096) + 0.5) / 4096
    e1 = 0.5 * 2 * f + 0.5 * (2 * (1 - f) * 0.5 * 2 * c).mean()
    e2 = 0.5 * (2 * f) ** 2 + 0.5 * ((2 * (1 - f) * 0.5 * 2 * c) ** 2).mean()
    assert f + (1 - f) * 0.5 == pytest.approx(e1, rel=1e-6) and 2 * f * f + 2 * (1 - f) ** 2 / 3 == pytest.approx(e2, rel=1e-6)


def test_pixel_to_ray_mapping_is_its_own_inverse():
    """closed_forms.rays against film.rs:233-247: the ray of a film point, pushed back through view_plane and to_pixel's
    longer-side rule, lands in the pixel it came from, on a landscape and on a portrait image."""
    for w, h in ((40, 24), (24, 40)):
        cam = cf.Camera((1, 2, 3), (0.5, -1, 0), fov=35, up=(0, 0, 1))
        for px, py in itertools.product((0, w // 3, w - 1), (0, h // 2, h - 1)):
            o, d = cf.rays(cam, w, h, px, py, 0.25, 0.75)
            local = cam.basis @ d
            x, y = local[0] / -local[2] * cam.view_plane, -local[1] / -local[2] * cam.view_plane
            size, ratio = max(w, h), min(w, h) / max(w, h)
            fx, fy = ((x + 1.0, y + ratio) if w >= h else (x + ratio, y + 1.0))
            assert (int(size * fx * 0.5), int(size * fy * 0.5)) == (px, py)
            assert np.allclose(o, cam.from_)


# ------------------------------------------------------------------------------------------------
# (b) the oracle against the closed forms
# ------------------------------------------------------------------------------------------------
def render_case(case, render, divide=1):
    """{render name: grains} and the spectrum sample count; `render(world, cam, renderer, film)` fills the film."""
    from pyrite_amd import project as P
    from pyrite_amd import scenes

    films, S = {}, None
    for name, project in cf.build_projects(case, P, scenes._mesh_dict_from_arrays).items():
        if divide != 1:
            project["renderer"] = project["renderer"].with_(pixel_samples=max(16, project["renderer"].pixel_samples // divide))
        world, cam, r, film = scenes.build(project, seed=1)
        render(world, cam, r, film)
        films[name], S = film.grains, r.spectrum_samples
        world.close()
    return films, S


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_oracle_meets_the_closed_form(case):
    import oracle

    films, S = render_case(case, lambda world, cam, r, film: oracle.OracleScene(world).render(r, cam, film, threads=4), divide=16)
    checks = cf.assert_checks(case.checks(films, S))
    # the GPU test's sample count resolves every stochastic statement: 5 sigma1 / sqrt(N) <= 1 % (2 % for the dispersion bins)
    from pyrite_amd import project as P
    from pyrite_amd import scenes

    spp = cf.build_projects(case, P, scenes._mesh_dict_from_arrays)["main"]["renderer"].pixel_samples
    for c in checks:
        if c.nominal is not None:
            assert c.nominal(spp) <= case.resolution * c.expected, (c.label, c.nominal(spp) / c.expected)
