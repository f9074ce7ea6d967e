"""tests/surface_forms.py held on the CPU, from both sides. (a) The algebra: every piece against a brute-force float64 evaluation
that does not use it. (b) The oracle: oracle.texture_get, OracleScene.surface_data and oracle films (at a sixteenth of the GPU
test's samples) against the forms, which is also where the bounds of the exact statements are MEASURED: the largest
|oracle - form| per statement class, times four (surface_forms.MEASURED / BOUNDS). (c) The caps on what an exact case may leave
out, checked on the form alone. A red tests/test_gpu_surface_forms.py then means kernel != oracle, not a wrong derivation."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import closed_forms as cf
import surface_forms as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def tables():
    with np.load(os.path.join(ROOT, "pyrite_amd", "data", "tables.npz")) as z:
        return {k: z[k] for k in z.files}


EXACT = sf.exact_cases(tables())
STOCHASTIC = sf.stochastic_cases(tables())


# ------------------------------------------------------------------------------------------------
# (a) the algebra
# ------------------------------------------------------------------------------------------------
def test_the_cubic_is_the_polynomial_through_its_four_conditions():
    """p(0) = v2, p(1) = v3, p'(0) = v3 - v1 (the FULL central difference: c is not halved), p'(1) = v4 - v2 -- solved as a linear
    system for numpy.polynomial's coefficients."""
    rng = np.random.default_rng(1)
    conditions = np.array([[1, 0, 0, 0], [1, 1, 1, 1], [0, 1, 0, 0], [0, 1, 2, 3]], dtype=np.float64)  # p(0), p(1), p'(0), p'(1) on (c0, c1, c2, c3)
    for _ in range(50):
        v1, v2, v3, v4 = rng.normal(size=4)
        coefficients = np.linalg.solve(conditions, [v2, v3, v3 - v1, v4 - v2])
        pos = rng.uniform(size=16)
        assert np.allclose(sf.cubic(v1, v2, v3, v4, pos), np.polynomial.polynomial.polyval(pos, coefficients), rtol=0, atol=1e-12)
    assert sf.cubic(1.0, 2.0, 4.0, 8.0, 0.25) == pytest.approx(2 + (3 + (-6 + 1.25) * 0.25) * 0.25)  # the hand evaluation of test_textures.py
    assert sf.cubic(0.0, 1.0, 2.0, 3.0, 0.5) == pytest.approx(1.5)  # a ramp of slope 1 per texel has c = 2 and still comes out linear
    assert sf.cubic(0.0, 0.0, 1.0, 1.0, 0.25) == pytest.approx(0.25)  # with c halved it would be 0.125


@pytest.mark.parametrize("width,height", sf.QUAD_SIZES + ((7, 2), (2, 1)))
def test_the_lookup_against_a_tiled_image_without_wrapping(width, height):
    """get_color against a scalar evaluation on the image tiled over thirteen periods, where no index wraps: the centre of texel
    (i, j) lies at ((i + 0.5) / w, 1 - (j + 0.5) / h), rows are interpolated first."""
    rng = np.random.default_rng(width * 31 + height)
    texels = rng.uniform(size=(height, width, 2))
    tiled = np.tile(texels, (13, 13, 1))
    px, py = rng.uniform(-3.5, 3.5, 200), rng.uniform(-3.5, 3.5, 200)
    got = sf.get_color(texels, px, py)
    for k in range(len(px)):
        x, y = px[k] * width - 0.5 + 6 * width, (1.0 - py[k]) * height - 0.5 + 6 * height
        i, j = int(np.floor(x)), int(np.floor(y))
        rows = [sf.cubic(*[tiled[j + b, i + a] for a in (-1, 0, 1, 2)], x - i) for b in (-1, 0, 1, 2)]
        assert np.allclose(got[k], sf.cubic(*rows, y - j), rtol=0, atol=1e-12)
    for j in range(height):  # texel centres return the texel; a period further out too
        for i in range(width):
            assert np.allclose(sf.get_color(texels, (i + 0.5) / width - 2.0, 1.0 - (j + 0.5) / height + 1.0), texels[j, i], rtol=0, atol=1e-12)


def test_linearisation_pixel_by_pixel():
    """linearise against the conversions written out per pixel; the luma weights against the Y row of the RGB -> XYZ matrix
    derived from the sRGB primaries and the D65 white point."""
    rng = np.random.default_rng(2)

    def decode(c):
        return c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4

    primaries = np.array([[0.64, 0.33], [0.30, 0.60], [0.15, 0.06]])
    xyz = np.array([[x / y, 1.0, (1.0 - x - y) / y] for x, y in primaries]).T
    white = np.array([0.95047, 1.0, 1.08883])  # palette's D65
    luma = (xyz * np.linalg.solve(xyz, white))[1]
    assert np.allclose(luma, sf.LUMA, rtol=0, atol=2e-6)
    for dtype, top in ((np.uint8, 255), (np.uint16, 65535)):
        rgba = rng.integers(0, top + 1, (3, 4, 4)).astype(dtype)
        for linear in (False, True):
            colour, mono = sf.linearise(rgba, linear, False), sf.linearise(rgba, linear, True)
            assert colour.shape == (3, 4, 4) and mono.shape == (3, 4)
            for j in range(3):
                for i in range(4):
                    c = [int(v) / top for v in rgba[j, i]]
                    lin = c[:3] if linear else [decode(v) for v in c[:3]]
                    assert np.allclose(colour[j, i], lin + [c[3]], rtol=0, atol=1e-15)  # alpha stays linear
                    assert mono[j, i] == pytest.approx(sum(a * b for a, b in zip(lin, luma)), abs=2e-6)
        grey = rng.integers(0, top + 1, (3, 4)).astype(dtype)
        assert np.allclose(sf.linearise(grey, True, True), grey / top, rtol=0, atol=1e-15)
        assert np.allclose(sf.linearise(grey, False, False)[..., :3], np.vectorize(decode)(grey / top)[..., None], rtol=0, atol=1e-15)
        assert (sf.linearise(grey, False, False)[..., 3] == 1.0).all()
        grey_alpha = rng.integers(0, top + 1, (3, 4, 2)).astype(dtype)
        assert np.allclose(sf.linearise(grey_alpha, False, False)[..., 3], grey_alpha[..., 1] / top, rtol=0, atol=1e-15)


def test_the_project_linearises_as_the_form_does():
    """pyrite_amd.images.linearise, which fills the texels the kernels read, against the form: within float32 rounding."""
    from pyrite_amd import images

    rng = np.random.default_rng(3)
    for dtype, top in ((np.uint8, 255), (np.uint16, 65535)):
        for channels in (1, 2, 3, 4):
            image = rng.integers(0, top + 1, (5, 6, channels)).astype(dtype)
            for linear in (False, True):
                for mono in (False, True):
                    got, expected = images.linearise(image, linear, mono), sf.linearise(image, linear, mono)
                    assert got.shape == expected.shape and np.abs(got - expected).max() <= 2.0 ** -23, (dtype, channels, linear, mono)


def rotation_matrix(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


def test_quaternions_against_rotation_matrices():
    """quat_from_cols of a rotation matrix's columns is the unit quaternion of that rotation, in all four branches of the
    conversion; its conjugate is the transposed matrix; plane_frame's columns are an orthonormal right-handed basis ending in the
    normal."""
    rng = np.random.default_rng(4)
    branches = set()
    for _ in range(200):
        m = rotation_matrix(rng)
        q = sf.quat_from_cols(m[:, 0], m[:, 1], m[:, 2])
        branches.add("trace" if np.trace(m) >= 0 else int(np.argmax(np.diag(m))))
        v = rng.normal(size=(5, 3))
        assert np.linalg.norm(q) == pytest.approx(1.0, abs=1e-12)
        assert np.allclose(sf.quat_rotate(q, v), v @ m.T, rtol=0, atol=1e-12)
        assert np.allclose(sf.quat_rotate(sf.quat_conjugate(q), v), v @ m, rtol=0, atol=1e-12)
    assert branches == {"trace", 0, 1, 2}
    for normal in ([0.3, -0.2, 1.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [-0.5, 0.5, -0.7]):
        n = sf.unit(normal)
        q = sf.plane_frame(n)
        x, y, z = (sf.quat_rotate(q, e) for e in np.eye(3))
        assert np.allclose(z, n, atol=1e-12) and abs(x @ y) < 1e-12 and abs(x @ n) < 1e-12 and np.allclose(np.cross(x, y), n, atol=1e-12)
        b, t = sf.basis(n)
        assert np.allclose(x, b, atol=1e-12) and np.allclose(y, t, atol=1e-12)


def test_triangle_frames_follow_the_uv_deltas():
    """With an orthonormal result the frame maps the tangent-space x axis onto the direction in which u grows and y onto the
    direction in which v grows, whatever the triangle's orientation in space and in uv."""
    rng = np.random.default_rng(5)
    for _ in range(20):
        m = rotation_matrix(rng)
        spin = rng.uniform(0, 2 * np.pi)
        uv = np.array([[0.2, -0.3], [0.2 + np.cos(spin), -0.3 + np.sin(spin)], [0.2 - np.sin(spin), -0.3 + np.cos(spin)]])  # an isometric uv map
        p = np.array([1.0, 2.0, 3.0]) + np.array([[0, 0, 0], m[:, 0], m[:, 1]])
        # position = p0 + (uv - uv0) mapped by the rotation [[cos, sin], [-sin, cos]] into the (m0, m1) plane
        du = np.cos(spin) * m[:, 0] - np.sin(spin) * m[:, 1]
        dv = np.sin(spin) * m[:, 0] + np.cos(spin) * m[:, 1]
        _, frames = sf.triangle_frames(p, uv, [m[:, 2]] * 3)
        for q in frames:
            assert np.allclose(sf.quat_rotate(q, [1, 0, 0]), du, atol=1e-12) and np.allclose(sf.quat_rotate(q, [0, 1, 0]), dv, atol=1e-12)
            assert np.allclose(sf.quat_rotate(q, [0, 0, 1]), m[:, 2], atol=1e-12)


def test_the_spheres_rotation_against_the_two_tangents():
    """from_angle_y(lon) from_angle_x(lat - pi/2): z -> the normal, x -> dP/dlon normalised, y -> -dP/dlat (towards the pole
    n.y = 1, where the texture's second coordinate 1 - lat / pi grows), by central differences of
    P(lat, lon) = (sin lat sin lon, cos lat, sin lat cos lon) -- the inverse of lat = acos(n.y), lon = atan2(n.x, n.z)."""
    point = lambda lat, lon: np.array([np.sin(lat) * np.sin(lon), np.cos(lat), np.sin(lat) * np.cos(lon)])  # noqa: E731
    rng = np.random.default_rng(6)
    h = 1e-6
    for _ in range(50):
        lat, lon = rng.uniform(0.1, np.pi - 0.1), rng.uniform(-np.pi, np.pi)
        n = point(lat, lon)
        assert np.arccos(n[1]) == pytest.approx(lat) and np.arctan2(n[0], n[2]) == pytest.approx(lon)
        m = sf.sphere_rotation(lat, lon)
        d_lon = (point(lat, lon + h) - point(lat, lon - h)) / (2 * h)
        d_lat = (point(lat + h, lon) - point(lat - h, lon)) / (2 * h)
        assert np.allclose(m @ [0, 0, 1], n, atol=1e-12)
        assert np.allclose(m @ [1, 0, 0], sf.unit(d_lon), atol=1e-8) and np.allclose(m @ [0, 1, 0], -sf.unit(d_lat), atol=1e-8)
        assert np.allclose(m @ m.T, np.eye(3), atol=1e-12) and np.linalg.det(m) == pytest.approx(1.0)
    s = sf.sphere_surface().evaluate(np.array([0.0, 0.0, -3.0]), np.array([0.0, 0.0, 1.0]))  # the seam: n = (0, 0, -1)
    assert abs(abs(s["longitude"]) - np.pi) < 1e-12 and s["ty"] == pytest.approx(0.5 / 0.25)


def test_plane_coordinates_are_the_position_in_the_frame():
    """into_space as the transposed matrix of the frame's columns, on the tilted plane of the cases."""
    plane = sf.plane_surface()
    binormal, tangent = sf.basis(plane.normal)
    o, d = cf.rays(sf.TILTED, sf.W, sf.H, np.array([3.0, 20.0, 37.0]), np.array([2.0, 12.0, 22.0]), 0.5, 0.5)
    s = plane.evaluate(o, d)
    position = o + d * s["t"][:, None]
    assert np.allclose((position - plane.origin) @ plane.normal, 0.0, atol=1e-12)
    assert np.allclose(s["tx"], position @ binormal / 2.0, atol=1e-12) and np.allclose(s["ty"], position @ tangent / 0.25, atol=1e-12)


def test_rgb_basis_and_stratified_wavelengths():
    t = tables()
    wl = np.array([355.0, 360.0, 401.3, 555.5, 830.9, 840.0])
    grid = np.linspace(float(t["rgb_min"]), float(t["rgb_max"]), len(t["rgb_basis"]))
    rgb = np.array([[0.2, 0.5, 0.9, 0.3], [1.0, 0.0, 0.0, 1.0]])
    expected = sum(rgb[:, c, None] * np.interp(wl, grid, t["rgb_basis"][:, c].astype(np.float64))[None, :] for c in range(3))
    assert np.allclose(sf.rgb_to_number(rgb, wl, t), expected, rtol=0, atol=1e-12)
    rng = np.random.default_rng(7)
    f = lambda lam: 1.0 + np.sin(lam / 40.0) ** 2  # noqa: E731
    for strata in (1, 4):
        lam = cf.SPAN[0] + (np.arange(strata) + rng.uniform(size=(400000, strata))) / strata * (cf.SPAN[1] - cf.SPAN[0])
        mean_of_path = f(lam).mean(-1)
        m1, m2 = sf.stratified_moments(f, strata)
        assert mean_of_path.mean() == pytest.approx(m1, rel=2e-3) and (mean_of_path ** 2).mean() == pytest.approx(m2, rel=2e-3)


@pytest.mark.parametrize("point", [(0.0, 0.0, 0.0), (-0.8, 0.5, 0.0), (0.85, -0.5, 0.0)])
@pytest.mark.parametrize("lamp", ["triangle", "tilted", "quad"])
def test_lamberts_formula_against_an_area_quadrature(lamp, point):
    """E = L integral of cos_in cos_out / d^2 dA over the emitter, by a midpoint rule over 10^6 sub-triangles of each triangle."""
    if lamp == "quad":
        polygon, triangles = sf.LAMP_QUAD, [sf.LAMP_QUAD[[0, 1, 2]], sf.LAMP_QUAD[[0, 2, 3]]]
    else:
        polygon = sf.LAMP_TRIANGLE if lamp == "triangle" else sf.rotate_about_y(sf.LAMP_TRIANGLE, sf.LAMP_TRIANGLE.mean(0), 60.0)
        triangles = [polygon]
    x, n = np.array(point, dtype=np.float64), np.array([0.0, 0.0, 1.0])
    u, v = sf.triangle_points(1000)
    assert len(u) == 10 ** 6
    brute = sum(sf.triangle_area(t) * sf.geometry_term(x[None, :], n, t, u, v).mean() for t in triangles)
    assert sf.lambert_irradiance(x, n, polygon, radiance=1.0) == pytest.approx(brute, rel=1e-6)
    assert sum(sf.lambert_irradiance(x, n, t) for t in triangles) == pytest.approx(brute, rel=1e-6)  # the quad is the sum of its triangles


def test_the_fold_is_uniform_over_the_triangle_and_the_estimators_moments_by_simulation():
    """Lamp::sample for a triangle written out sample by sample in numpy (the fold, the point, |cos_in| area / d^2, the uniform lamp
    pick, probability 1 / (n 2 pi p), the Lambert factor 2 cos_out) and averaged over 4 x 10^5 paths, against triangle_lamp_moments;
    and the chance-hit estimator by uniform hemisphere directions against the same."""
    rng = np.random.default_rng(8)
    triangles = [sf.LAMP_QUAD[[0, 1, 2]], sf.LAMP_QUAD[[0, 2, 3]]]
    x, n, rho, radiance, paths = np.array([-0.3, 0.2, 0.0]), np.array([0.0, 0.0, 1.0]), 0.5, 4.0, 400000
    u, v = sf.fold(rng.uniform(size=paths), rng.uniform(size=paths))
    assert (u + v <= 1.0).all() and u.mean() == pytest.approx(1 / 3, abs=2e-3) and (u * v).mean() == pytest.approx(1 / 12, abs=1e-3)  # uniform: E[uv] = 1/12
    for light_samples in (1, 4):
        pick = rng.integers(0, 2, paths)
        value = np.zeros(paths)
        for _ in range(light_samples):
            u, v = sf.fold(rng.uniform(size=paths), rng.uniform(size=paths))
            for k, tri in enumerate(triangles):
                a, b = tri[1] - tri[0], tri[2] - tri[0]
                y = tri[0] + u[:, None] * a + v[:, None] * b
                direction = y - x
                d2 = (direction * direction).sum(-1)
                direction /= np.sqrt(d2)[:, None]
                weight = np.abs(sf.unit(np.cross(a, b)) @ -direction.T) * sf.triangle_area(tri) / d2
                sample = weight / (light_samples * 2 * np.pi * 0.5) * rho * 2 * np.maximum(direction @ n, 0) * radiance
                value += np.where(pick == k, sample, 0.0)
        m1, m2 = sf.triangle_lamp_moments(x[None, :], n, triangles, rho, radiance, light_samples)
        sigma = np.sqrt(m2[0] - m1[0] ** 2)
        assert abs(value.mean() - m1[0]) <= 5 * sigma / np.sqrt(paths) and (value ** 2).mean() == pytest.approx(m2[0], rel=0.02)
        assert m1[0] == pytest.approx(rho / np.pi * sf.lambert_irradiance(x, n, sf.LAMP_QUAD, radiance), rel=1e-4)
    m1, m2 = sf.triangle_lamp_moments(x[None, :], n, triangles, rho, radiance, 0)
    assert m1[0] == pytest.approx(rho / np.pi * sf.lambert_irradiance(x, n, sf.LAMP_QUAD, radiance), rel=1e-4)
    paths = 4 * 10 ** 6
    z, phi = rng.uniform(size=paths), 2 * np.pi * rng.uniform(size=paths)  # uniform on the hemisphere: cos theta uniform
    w = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], -1)
    t = (1.0 - x[2]) / w[:, 2]  # the lamp lies in the plane z = 1
    y = x + w * t[:, None]
    hit = np.zeros(paths, dtype=bool)
    for tri in triangles:
        e = np.linalg.solve(np.array([tri[1] - tri[0], tri[2] - tri[0]])[:, :2].T, (y - tri[0])[:, :2].T)
        hit |= (e[0] >= 0) & (e[1] >= 0) & (e[0] + e[1] <= 1)
    value = np.where(hit, rho * 2 * z * radiance, 0.0)
    sigma = np.sqrt(m2[0] - m1[0] ** 2)
    assert abs(value.mean() - m1[0]) <= 5 * sigma / np.sqrt(paths) and (value ** 2).mean() == pytest.approx(m2[0], rel=0.02)


# ------------------------------------------------------------------------------------------------
# (b) the oracle against the forms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", sf.QUAD_SIZES)
def test_oracle_texture_get_meets_the_lookup(width, height):
    """oracle.texture_get on random positions, some of them many periods out, mono and colour: within float32's rounding of the
    position (|position| width ulps of a texel, times the cubic's slope) of the float64 lookup."""
    import oracle

    rng = np.random.default_rng(width + 100 * height)
    for texels in (rng.uniform(0.1, 0.9, (height, width)).astype(np.float32), rng.uniform(0.1, 0.9, (height, width, 4)).astype(np.float32)):
        worst = 0.0
        for _ in range(300):
            px, py = (float(np.float32(v)) for v in rng.uniform(-2.5, 3.5, 2))
            got = oracle.texture_get(texels, px, py)
            expected = np.atleast_1d(sf.get_color(texels, px, py))
            worst = max(worst, float(np.abs(got - expected).max()))
        # float32: the position px w - 0.5 carries half an ulp of |px| w <= 56, 3.8e-6 texel, the cubic's slope is at most ~3 per
        # texel for values in [0.1, 0.9], and its own arithmetic adds a few ulps of 1: 2e-5 covers both
        assert worst <= 2e-5, worst


def oracle_rays(cam, width, height):
    """float32 [h, w, 6]: the pixel-centre rays as the oracle makes them (oracle_to_view_area, oracle_ray_towards), aperture 0."""
    import oracle
    from pyrite_amd import abi

    lib = oracle.lib()
    pinhole = abi.PyrCamera.from_buffer_copy(cam.c)
    pinhole.aperture = 0.0
    rays = np.zeros((height, width, 6), dtype=np.float32)
    area, ray, state = (C.c_float * 4)(), oracle.F6(), oracle.U4(1, 2, 3, 4)
    for y in range(height):
        for x in range(width):
            lib.oracle_to_view_area(x, y, 1, 1, width, height, area)
            lib.oracle_ray_towards(C.byref(pinhole), state, np.float32(area[0] + np.float32(area[2] * np.float32(0.5))), np.float32(area[1] + np.float32(area[3] * np.float32(0.5))), ray)
            rays[y, x] = ray[:]
    return rays


@functools.lru_cache(maxsize=None)
def oracle_features(index):
    """What the feature pass computes at grid 1, composed from the oracle's entry points: (albedo grains, normal, depth, coverage,
    texture coordinates) of exact case `index`, and the texture offsets of its scene."""
    import oracle
    from pyrite_amd import abi, scenes
    from pyrite_amd import project as P

    case = EXACT[index]
    world, cam, r, _ = scenes.build(case.project(P), seed=1)
    scene = oracle.OracleScene(world)
    desc = world.desc
    w, h = case.width, case.height
    rays = oracle_rays(cam, w, h)
    hits, _ = scene.intersect(rays.reshape(-1, 6))
    hits = hits.reshape(h, w)
    grains = np.zeros((h, w, case.bins, 2), dtype=np.float32)
    grains[..., 1] = 1.0
    normal, depth, coverage, coords = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w), dtype=np.float32), np.zeros((h, w), dtype=np.float32), np.zeros((h, w, 2))
    middle = float(np.float32(cf.SPAN[0]) + np.float32(np.float32(cf.SPAN[1] - cf.SPAN[0]) * np.float32(0.5)))
    wavelengths = [float(np.float32(cf.SPAN[0]) + np.float32(np.float32(np.float32(b) + np.float32(0.5)) * np.float32(np.float32(cf.SPAN[1] - cf.SPAN[0]) / np.float32(case.bins)))) for b in range(case.bins)]
    for y, x in zip(*np.nonzero(hits["shape"] != abi.HIT_NONE)):
        kind, item = int(hits["shape"][y, x]) >> 30, int(hits["shape"][y, x]) & 0x3FFFFFFF
        material = desc.materials[int({abi.SHAPE_TRIANGLE: desc.tri_material, abi.SHAPE_SPHERE: desc.sphere_material, abi.SHAPE_PLANE: desc.plane_material}[kind][item])]
        assert material.num_components == 1
        _, t, _, shading = scene.surface_data(rays[y, x], wavelength=middle)
        program = desc.components[material.first_component].color_program
        for b, wl in enumerate(wavelengths):
            grains[y, x, b, 0] = scene.run_program(program, wl, shading, rays[y, x, 3:], t)[0]
        normal[y, x], depth[y, x], coverage[y, x], coords[y, x] = shading, hits["distance"][y, x], 1.0, t
    offsets = [int(desc.textures[k].offset) for k in range(desc.num_textures)]
    scene.close()
    world.close()
    return grains, normal, depth, coverage, coords, offsets


def unbounded():
    return {k: np.inf for k in sf.BOUNDS}


def test_measured_figures_are_the_ones_the_bounds_come_from(capsys):
    """Per statement class the largest |oracle - form| over every kept probe of every exact case. surface_forms.MEASURED records
    these figures (rounded up to two digits) and BOUNDS is four times them; a run on another machine may differ in the last
    digits (libm), so the recorded figure must cover this run's and not exceed twice it."""
    figures, lines = {k: 0.0 for k in sf.BOUNDS}, []
    for index, case in enumerate(EXACT):
        grains, normal, depth, coverage, coords, _ = oracle_features(index)
        p = case.predict()
        checks = case.checks(grains, normal, depth, coverage)
        for c in checks[1:4]:
            key = case.lookup if c.label.startswith("albedo") else ("shading normal" if c.label.startswith("normal") else "depth")
            figures[key] = max(figures[key], c.deviation)
        drift = np.abs(coords - np.stack([p.tx, p.ty], -1))[p.keep].max()
        lines.append("%-28s kept %3d of %3d hit (left out %4.1f %%: %d straddle, %d pole, %d conditioning)  albedo %.3g  normal %.3g  depth %.3g  coordinates %.3g" % (
            case.name, p.keep.sum(), p.hit.sum(), 100 * p.left_out, (p.hit & ~p.inside).sum(), (p.inside & p.pole).sum(), (p.inside & ~p.pole & p.sensitive).sum(),
            checks[1].deviation, checks[2].deviation, checks[3].deviation, drift))
    with capsys.disabled():
        print()
        for line in lines:
            print("surface_forms oracle-form " + line)
        for key, figure in figures.items():
            print("surface_forms figure %-20s measured %.3g recorded %r bound %.3g" % (key, figure, sf.MEASURED[key], sf.BOUNDS[key]))
    for key, figure in figures.items():
        assert sf.MEASURED[key] is not None, "no figure recorded for " + key
        assert figure <= sf.MEASURED[key] <= 2.0 * figure, (key, figure, sf.MEASURED[key])


@pytest.mark.parametrize("index", range(len(EXACT)), ids=[c.name for c in EXACT])
def test_oracle_meets_the_exact_form(index):
    grains, normal, depth, coverage, _, _ = oracle_features(index)
    cf.assert_checks(EXACT[index].checks(grains, normal, depth, coverage))


def test_both_load_paths_are_set_up_and_agree():
    """The same colour texture at a texel offset divisible by 4 and at offset 9 (behind a 3 x 3 mono texture): the two albedo films
    are equal bit for bit in the oracle, which has one path; the GPU test asserts the same of texture_get's two."""
    a, b = (next(i for i, c in enumerate(EXACT) if c.name == name) for name in sf.LOAD_PATH_PAIR)
    first, second = oracle_features(a), oracle_features(b)
    assert first[5] == [0] and second[5] == [0, 9]
    assert np.array_equal(first[0], second[0]) and first[0][..., 0].any()


# ------------------------------------------------------------------------------------------------
# (c) the caps, on the form alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EXACT, ids=[c.name for c in EXACT])
def test_no_exact_case_leaves_out_more_than_a_quarter(case):
    p = case.predict()
    assert p.hit.sum() >= 400 and p.left_out <= sf.MOST_LEFT_OUT, (p.hit.sum(), p.left_out)
    if case.name == "sphere_seam" or case.name.endswith("_sphere"):
        lon = p.surface["longitude"]
        east, west = p.keep & (lon > np.pi - sf.SEAM_BAND), p.keep & (lon < -np.pi + sf.SEAM_BAND)
        assert east.sum() >= 20 and west.sum() >= 20, (east.sum(), west.sum())
    if case.name == "sphere_pole":
        assert p.pole.any() and (p.keep & (np.abs(p.surface["n"][..., 1]) > np.cos(np.radians(12.0)))).sum() >= 20  # the pole is in view and kept pixels ring it
    if case.name == "quad_mono_boundary_16x8":
        x, _ = sf.texel_position(case.texels, p.tx, p.ty)
        near = p.keep & (np.abs(x - np.round(x)) < 1e-3)
        assert near.sum() >= 10, near.sum()


def test_the_quad_cases_take_the_coordinates_the_issue_names():
    """Texture coordinates negative, beyond one period and non-integer at the corners; widths 1-3 repeat columns, 4 and 5 straddle
    the contiguous-row branch; the quad of the normal-map cases has three different frames per triangle."""
    q = sf.quad()
    assert q.uvs.min() == -1.25 and q.uvs.max() == 2.5
    p = EXACT[0].predict()
    assert p.tx[p.keep].min() < -1.0 and p.tx[p.keep].max() > 2.0 and p.ty[p.keep].min() < -0.5 and p.ty[p.keep].max() > 1.5
    assert [w for w, _ in sf.QUAD_SIZES] == [1, 2, 3, 4, 5, 16]
    bent = sf.quad(normals=sf.QUAD_NORMALS)
    for tri in bent.triangles:
        _, frames = sf.triangle_frames(bent.positions[list(tri)], bent.uvs[list(tri)], bent.vertex_normals(tri))
        assert min(np.abs(frames[i] - frames[j]).max() for i, j in ((0, 1), (0, 2), (1, 2))) > 0.01


# ------------------------------------------------------------------------------------------------
# the oracle's films against the stochastic forms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STOCHASTIC, ids=[c.name for c in STOCHASTIC])
def test_oracle_meets_the_stochastic_form(case):
    import oracle
    from pyrite_amd import project as P
    from pyrite_amd import scenes

    project = cf.build_projects(case, P, None)["main"]
    spp = project["renderer"].pixel_samples
    project["renderer"] = project["renderer"].with_(pixel_samples=max(16, spp // 16))
    world, cam, r, film = scenes.build(project, seed=1)
    oracle.OracleScene(world).render(r, cam, film, threads=4)
    world.close()
    checks = cf.assert_checks(case.checks({"main": film.grains}, r.spectrum_samples))
    for c in checks:  # the GPU test's sample count resolves every statement to 1 %, and hardly more than that needs
        assert c.nominal(spp) <= case.resolution * c.expected, (c.label, c.nominal(spp) / c.expected)
    assert max(c.nominal(spp) / c.expected for c in checks) > 0.9 * case.resolution, "more samples than 1 % needs"
