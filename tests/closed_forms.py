"""Closed forms of what the reference's `simple` renderer computes for nine small scenes: float64 numpy only. Nothing here
comes from pyrite_amd or from the oracle, so a misreading the kernels and oracle/oracle.cpp share does not reach these numbers.
Every formula follows the reference source (pyrite/src/...), cited line by line; where the reference departs from physics the
closed form follows the reference and says so.

A `Case` is one scene: its project (built from the `pyrite_amd.project` module the caller hands in -- this file imports
none of it), the renders it needs, and `checks(films, spectrum_samples)`, which turns the rendered films into `Check`
records: an observed deviation and its bound. `assert_checks` is the one assertion both the CPU test (oracle films) and the
GPU test (kernel films) run.

Two kinds of statement (the tolerances are fixed here, before any render):
  exact       a pixel whose value has no variance: |got - expected| <= 1e-6 |expected| (0 means exactly 0).
  stochastic  a mean over a region of N independent paths: |got - expected| <= 5 sigma1 / sqrt(N) + 1e-4 expected, where
              sigma1 is the single-sample standard deviation derived next to the expectation. The renderer draws its samples
              uniformly over a tile (algorithm.rs:113-119), so the samples of a region are independent draws over the region:
              sigma1^2 = mean over the region of E[v^2 | point] - (mean over the region of E[v | point])^2. The S wavelengths
              of one path share the path (simple.rs:91-139), so N = film weight / S; a dispersed path exposes its main
              wavelength alone (simple.rs:123-139) and then N = film weight."""
import numpy as np

DIST_EPSILON = 1e-4  # math.rs:4
EXACT = 1e-6
SIGMAS = 5.0
FLOOR = 1e-4
SPAN = (380.0, 780.0)  # renderer/mod.rs:16


# ------------------------------------------------------------------------------------------------
# pixel footprint -> ray (cameras.rs:57-97, film.rs:203-247, algorithm.rs:113-119, project/mod.rs:250-266)
# ------------------------------------------------------------------------------------------------
class Camera:
    """camera.perspective: `fov` in degrees across the LONGER image side, look_at(from, to, up)."""

    def __init__(self, from_, to, fov, up=(0.0, 1.0, 0.0), focus_distance=1.0, aperture=0.0):
        self.from_, self.to, self.up = (np.asarray(v, dtype=np.float64) for v in (from_, to, up))
        self.fov, self.focus_distance, self.aperture = float(fov), float(focus_distance), float(aperture)
        half = np.radians(self.fov * 0.5)
        self.view_plane = np.cos(half) / np.sin(half)  # cameras.rs:43-45: cot(fov / 2)
        f = self.to - self.from_
        f /= np.linalg.norm(f)
        s = np.cross(f, self.up)
        s /= np.linalg.norm(s)
        self.basis = np.stack([s, np.cross(s, f), -f])  # cgmath look_at inverted: camera x, y, z axes in world space

    def to_world(self, v):
        return v @ self.basis


def view_point(width, height, px, py, u, v):
    """The film point of offset (u, v) in [0, 1]^2 inside pixel (px, py). to_view_area (cameras.rs:57-68) divides by HALF THE
    LONGER side, so x spans [-1, 1] on a landscape image and y only [-h/w, h/w]; Film::to_pixel (film.rs:233-247) inverts it."""
    half = max(width, height) * 0.5  # cameras.rs:62-65
    return (px + u - width * 0.5) / half, (py + v - height * 0.5) / half


def rays(cam, width, height, px, py, u, v, lens=None):
    """Camera::ray_towards (cameras.rs:70-97) in float64. `lens` = (lx, ly), a point on the lens in camera space, or None for the
    pinhole. Returns world-space (origin, unit direction); arrays broadcast."""
    x, y = view_point(width, height, px, py, u, v)
    fd = cam.focus_distance
    target = np.stack(np.broadcast_arrays(x / cam.view_plane * fd, -(y / cam.view_plane * fd), -fd + 0.0 * x), axis=-1)  # :78-81
    if lens is None:
        origin = np.zeros_like(target)  # :91
    else:
        lx, ly = np.broadcast_arrays(lens[0] + 0.0 * x, lens[1] + 0.0 * x)
        origin = np.stack([lx, ly, 0.0 * lx], axis=-1)  # :84-89: radius sqrt(aperture * U), uniform on the disc of radius sqrt(aperture)
    d = target - origin
    d /= np.linalg.norm(d, axis=-1, keepdims=True)  # :94
    return cam.from_ + cam.to_world(origin), cam.to_world(d)


def footprints(cam, width, height, n, closed, lens=None):
    """Rays of an n x n grid in every pixel's footprint, shape [h, w, n, n, 3]: the midpoints of n x n cells (a midpoint rule for
    the pixel's mean), or with `closed` the grid that includes the footprint's border (for inside / outside decisions)."""
    t = np.arange(n) / (n - 1.0) if closed else (np.arange(n) + 0.5) / n
    py, px, v, u = np.meshgrid(np.arange(height), np.arange(width), t, t, indexing="ij")
    return rays(cam, width, height, px, py, u, v, lens)


MIDPOINTS, BORDER = 8, 9


def classify(signed, margin):
    """signed: [h, w, n, n] of a function that is positive inside a convex region, over the closed grid of every footprint.
    -> (inside, outside, straddling) pixel masks. A pixel counts as inside (outside) only if every grid point is inside (outside)
    by more than `margin`; the margin covers the arc that may bulge between two grid points and float32 rounding in the code
    under test."""
    inside = (signed > margin).all(axis=(-1, -2))
    outside = (signed < -margin).all(axis=(-1, -2))
    return inside, outside, ~(inside | outside)


def plane_hit(o, d, z0=0.0):
    t = (z0 - o[..., 2]) / d[..., 2]
    return o + d * t[..., None]


def sphere_hit(o, d, centre, radius):
    """-> (hit mask, cos of the incidence angle -d.n at the first hit)."""
    l = np.asarray(centre, dtype=np.float64) - o
    tca = (l * d).sum(-1)
    d2 = (l * l).sum(-1) - tca * tca
    hit = (tca > 0) & (d2 < radius * radius)
    thc = np.sqrt(np.maximum(radius * radius - d2, 0.0))
    p = o + d * (tca - thc)[..., None]
    n = (p - centre) / radius
    return hit, -(d * n).sum(-1)


# ------------------------------------------------------------------------------------------------
# pieces of algebra (each is held against a brute-force evaluation in test_closed_forms_cpu.py)
# ------------------------------------------------------------------------------------------------
def cap_moments(cos_gamma, cos_alpha):
    """Mean and mean square of n.w for w uniform IN SOLID ANGLE on the cap of half-angle alpha about an axis with n.axis =
    cos gamma, the cap wholly above n's horizon. sample_cone (math.rs:125-137) draws cos theta uniformly in [cos alpha, 1] and the
    azimuth uniformly, which is that distribution. With n.w = cos g cos t + sin g sin t cos phi:
    E[n.w] = cos g (1 + c) / 2,  E[(n.w)^2] = cos^2 g E[cos^2 t] + sin^2 g (1 - E[cos^2 t]) / 2,  E[cos^2 t] = (1 + c + c^2) / 3."""
    c = cos_alpha
    ec2 = (1.0 + c + c * c) / 3.0
    return cos_gamma * (1.0 + c) * 0.5, cos_gamma ** 2 * ec2 + (1.0 - cos_gamma ** 2) * (1.0 - ec2) * 0.5


def sphere_lamp_radiance(rho, emission, radius, distance, cos_gamma):
    """Radiance leaving a Lambertian surface of albedo rho lit by a sphere of radiance `emission` wholly above its horizon:
    irradiance = pi L (r/d)^2 cos gamma (the classic result), times rho / pi."""
    return rho * emission * (radius / distance) ** 2 * cos_gamma


def schlick(cos_theta, ior, env_ior=1.0):
    """refractive.rs:75-80 for a ray entering the denser medium (`into`): c = 1 + ddn = 1 - cos theta."""
    r0 = ((ior - env_ior) / (ior + env_ior)) ** 2
    return r0 + (1.0 - r0) * (1.0 - cos_theta) ** 5


def refract_moments(re):
    """refractive.rs:80-90 when only the reflected branch returns light L = 1 (the transmitted one ends on a black surface):
    reflect with probability p = 1/4 + Re/2 and weight rp = Re/p, else transmit with weight tp = Tr/(1-p).
    E = p rp = Re;  E[v^2] = p rp^2 = Re^2 / p."""
    p = 0.25 + 0.5 * re
    return re, re * re / p


def glass_sphere_moments(re, segments):
    """A glass sphere in a uniform sky L = 1, the path cut after `segments` ray segments (tracer.rs:221). Inside a sphere every
    chord meets the surface at the refraction angle of the entry, and refractive.rs:78 takes c = 1 - tdir.normal on the way out,
    which is 1 - cos(theta outside) again: Re, p, rp, tp are the same at every event of one path. The path is: reflect at once
    (prob p, weight rp), or enter (1-p, tp), reflect inside k times (p, rp each) and leave (1-p, tp); the leaving ray is
    segment k + 3, so k <= segments - 3.
    E = Re + Tr^2 sum Re^k -> 1;  E[v^2] = Re^2/p + Tr^4/(1-p)^2 sum (Re^2/p)^k."""
    re = np.asarray(re, dtype=np.float64)
    tr = 1.0 - re
    p = 0.25 + 0.5 * re
    k = np.arange(max(segments - 2, 0)).reshape((-1,) + (1,) * re.ndim)
    m1 = re + tr * tr * (re ** k).sum(0)
    m2 = re * re / p + tr ** 4 / (1.0 - p) ** 2 * ((re * re / p) ** k).sum(0)
    return m1, m2


def reference_fresnel(cos_theta, ior, env_ior=1.0):
    """math.rs:167-175 for a ray that meets the surface from outside (incident.normal < 0): schlick(env_ior, ior, normal,
    incident), math.rs:75-96 with ref_index1 = env_ior < ref_index2 = ior, so no total reflection branch."""
    r0 = (env_ior - ior) / (env_ior + ior)
    return r0 * r0 + (1.0 - r0 * r0) * (1.0 - cos_theta) ** 5


def disc_segment(s):
    """Share of a disc's area on the inner side of a straight edge, s = signed distance of the disc's centre from the edge in
    radii (positive inside): (acos(-s) + s sqrt(1 - s^2)) / pi."""
    s = np.clip(s, -1.0, 1.0)
    return (np.arccos(-s) + s * np.sqrt(1.0 - s * s)) / np.pi


def dispersed_ior(ior, dispersion, wavelength_nm):
    wl = wavelength_nm * 0.001  # refractive.rs:16-17
    return ior + dispersion / (wl * wl)


# ------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------
class Check:
    def __init__(self, label, deviation, bound, expected=None, got=None, n=None, noise=None, pixels=None, nominal=None):
        self.label, self.deviation, self.bound = label, float(deviation), float(bound)
        self.expected, self.got, self.n, self.noise, self.pixels, self.nominal = expected, got, n, noise, pixels, nominal

    def record(self):
        return {k: (None if v is None else float(v)) if k != "label" else v for k, v in self.__dict__.items() if k != "nominal"}


def values(grains):
    g = np.asarray(grains, dtype=np.float64)
    return g[..., 0].sum(-1) / np.maximum(g[..., 1].sum(-1), 1.0)


def exact_check(label, grains, mask, expected, tol=EXACT):
    """Every pixel of `mask` equals `expected` (scalar or per-pixel array) to `tol` relative. The record is the worst pixel."""
    got = values(grains)[mask]
    exp = np.broadcast_to(np.asarray(expected, dtype=np.float64), mask.shape)[mask]
    assert mask.any(), label + ": no pixel to check"
    assert (np.asarray(grains)[..., 1].sum(-1)[mask] > 0).all(), label + ": a pixel without samples"
    dev = np.abs(got - exp) - tol * np.abs(exp)
    k = int(np.argmax(dev))
    return Check(label, abs(got[k] - exp[k]), tol * abs(exp[k]), expected=exp[k], got=got[k], pixels=int(mask.sum()))


def region_check(label, grains, mask, m1, m2, paths_per_weight, bins=None):
    """The mean over the pixels of `mask` (and the bins of `bins`) against the mean of the per-pixel expectation m1, with sigma1
    from the per-pixel second moment m2. paths_per_weight = 1 / S, or 1 for dispersed paths."""
    g = np.asarray(grains, dtype=np.float64)[mask]
    if bins is not None:
        g = g[:, bins]
    weight = g[..., 1].sum()
    got = g[..., 0].sum() / weight
    m1 = np.broadcast_to(np.asarray(m1, dtype=np.float64), mask.shape)[mask]
    m2 = np.broadcast_to(np.asarray(m2, dtype=np.float64), mask.shape)[mask]
    expected = m1.mean()
    sigma1 = np.sqrt(max(m2.mean() - expected * expected, 0.0))
    n = weight * paths_per_weight
    noise = SIGMAS * sigma1 / np.sqrt(n)
    share = 1.0 if bins is None else len(range(*bins.indices(np.asarray(grains).shape[2]))) / np.asarray(grains).shape[2]
    nominal = lambda pixel_samples: SIGMAS * sigma1 / np.sqrt(mask.sum() * pixel_samples * share)  # noqa: E731
    return Check(label, abs(got - expected), noise + FLOOR * expected, expected=expected, got=got, n=n, noise=noise, pixels=int(mask.sum()), nominal=nominal)


def assert_checks(checks, resolution=None):
    """The one assertion of the CPU and the GPU test. With `resolution` (0.01: the GPU test) every stochastic check must first
    resolve its expectation: 5 sigma1 / sqrt(N) <= resolution * expected."""
    assert checks
    for c in checks:
        if resolution is not None and c.noise is not None:
            assert c.noise <= resolution * c.expected, "%s: 5 sigma1/sqrt(N) = %.3g does not resolve %.3g of %.6g (N = %.0f)" % (c.label, c.noise, resolution, c.expected, c.n)
        assert c.deviation <= c.bound, "%s: got %r, expected %r: off by %.3g, bound %.3g (N = %r)" % (c.label, c.got, c.expected, c.deviation, c.bound, c.n)
    return checks


class Case:
    """name; width x height; `renders`: {render name: project builder (P, mesh_dict) -> project}; checks({render name: grains}, S)
    -> [Check].
    `resolution` is what the stochastic checks must resolve at the GPU test's sample count."""

    def __init__(self, name, renders, checks, width=40, height=24, resolution=0.01):
        self.name, self.renders, self.checks, self.width, self.height, self.resolution = name, renders, checks, width, height, resolution


def renderer_args(pixel_samples, bounces, light_samples, spectrum_samples=4, bins=None):
    return dict(pixel_samples=pixel_samples, bounces=bounces, light_samples=light_samples, spectrum_samples=spectrum_samples, tile_size=16,
                spectrum_resolution=bins)


def project_camera(P, cam):
    return P.camera.perspective(fov=cam.fov, focus_distance=cam.focus_distance, aperture=cam.aperture,
                                transform=P.transform.look_at(**{"from": P.vector(*cam.from_), "to": P.vector(*cam.to), "up": P.vector(*cam.up)}))


RHO = 0.5
DOWN = Camera((0, 0, 5), (0, 0, 0), fov=20)  # looking down the z axis at the plane z = 0; camera x, y = world x, y


def floor(P, rho=RHO, z=0.0):
    return P.shape.plane(origin=P.vector(0, 0, z), normal=P.vector(z=1), material={"surface": P.material.diffuse(color=rho)})


# ------------------------------------------------------------------------------------------------
# 1. point lamp over a plane
# ------------------------------------------------------------------------------------------------
def point_lamp(occluder_radius=None, pixel_samples=64):
    """Camera ray -> plane point X (diffuse rho, one component: probability 1, materials/mod.rs:213-247). trace_direct
    (tracer.rs:347-442) with one lamp: pick_lamp gives p_lamp = 1 / lights.len() = 1 (world.rs:301-305), probability =
    1 / (samples 2 pi p_lamp) (:365); Lamp::Point gives weight 4 pi / d^2 (lamp.rs:43-52); the Lambert factor is 2 |n.o|
    (diffuse.rs:27-29). scale = 4 pi / d^2 / (2 pi) 2 cos = 4 cos / d^2 (:423), times the path's reflectance rho
    (algorithm.rs:57, :83): value = rho 4 cos(theta) / d^2, with no randomness but the pixel jitter. The bounce ray leaves upwards
    and meets nothing; it reads the sky, 0, with the directional lamps masked (tracer.rs:258, :323-328).

    With `occluder_radius` a BLACK diffuse sphere (albedo 0) at (1.5, 0, 1) shadows the plane: the shadow ray is blocked when it
    hits anything nearer than the lamp (tracer.rs:381-389). The sphere is black so that the plane's bounce ray, when it lands on
    the sphere, carries nothing back (algorithm.rs:57: reflectance *= 0): every pixel stays a function of the plane point alone.
    The sphere lies outside the view (it projects to x = 1.875 on the plane, the view ends at 0.88)."""
    lamp, centre, w, h = np.array([3.0, 0.0, 2.0]), np.array([1.5, 0.0, 1.0]), 40, 24

    def project(P, mesh_dict=None):
        objects = [floor(P), P.light.point(position=P.vector(*lamp), color=1)]
        if occluder_radius is not None:
            objects.append(P.shape.sphere(position=P.vector(*centre), radius=occluder_radius, material={"surface": P.material.diffuse(color=0)}))
        return {"image": {"width": w, "height": h}, "renderer": P.renderer.simple(**renderer_args(pixel_samples, 2, 1)), "camera": project_camera(P, DOWN),
                "world": {"sky": 0, "objects": objects}}

    def radiance(o, d):
        x = plane_hit(o, d)
        v = lamp - x
        d2 = (v * v).sum(-1)
        return RHO * 4.0 * (v[..., 2] / np.sqrt(d2)) / d2, x

    def checks(films, S):
        grains = films["main"]
        mean = radiance(*footprints(DOWN, w, h, MIDPOINTS, False))[0].mean(axis=(-1, -2))
        border, x = radiance(*footprints(DOWN, w, h, BORDER, True))
        spread = border.max(axis=(-1, -2)) - border.min(axis=(-1, -2))
        n = np.asarray(grains, dtype=np.float64)[..., 1].sum(-1) / S
        got = values(grains)
        out = []
        if occluder_radius is None:
            lit = np.ones((h, w), dtype=bool)
        else:
            # X is shadowed iff the segment X -> lamp meets the sphere: the distance of the centre from that line is below the radius
            # (the lamp and the plane are both outside the sphere and on opposite sides of it)
            u = lamp - x
            u /= np.linalg.norm(u, axis=-1, keepdims=True)
            c = centre - x
            dist = np.linalg.norm(c - (c * u).sum(-1)[..., None] * u, axis=-1)
            dark, lit, edge = classify(occluder_radius - dist, 1e-4)
            out.append(Check("straddling share", edge.mean(), 0.10, pixels=int(edge.sum())))
            if dark.any():
                out.append(exact_check("shadowed pixels are 0", grains, dark, 0.0))
        assert (n[lit] > 0).all()
        bound = SIGMAS * spread / np.sqrt(12.0 * np.maximum(n, 1)) + 1e-5 * mean  # a uniform jitter over a near-linear field
        if lit.any():
            excess = np.where(lit, np.abs(got - mean) - bound, -np.inf)
            j, i = np.unravel_index(int(np.argmax(excess)), excess.shape)
            out.append(Check("lit pixels equal rho 4 cos / d^2", abs(got[j, i] - mean[j, i]), bound[j, i], expected=mean[j, i], got=got[j, i], n=n[j, i], pixels=int(lit.sum())))
        if occluder_radius is None:  # orientation: the lamp is at +x, so the image's right edge is the bright one, and the four corners differ
            corners = [got[0, 0], got[0, -1], got[-1, 0], got[-1, -1]]
            assert min(corners[1], corners[3]) > 2.0 * max(corners[0], corners[2]), corners
        return out

    return Case("point_lamp" if occluder_radius is None else "point_lamp_shadow_r%g" % occluder_radius, {"main": project}, checks)


# ------------------------------------------------------------------------------------------------
# 2. directional lamp
# ------------------------------------------------------------------------------------------------
SUN = np.array([0.6, 0.0, 0.8])  # TOWARDS the lamp: Lamp::Directional hands `direction` out as the shadow ray's direction (lamp.rs:25-41)


def directional_lamp(width_cos, pixel_samples=16):
    """Plane under a directional lamp. lamp.rs:25-42: direction = sample_cone(direction, width) when width > 0, else the
    direction itself; weight = 1 (NOT the cone's solid angle); no distance, so any hit blocks (tracer.rs:385-389) -- the plane
    itself is nearer than DIST_EPSILON and does not count (world.rs:279). scale = 1 / (2 pi) 2 n.w (tracer.rs:365, :423):
    value = rho (n.w) / pi. Width 0: rho 0.8 / pi in every pixel, to 1e-5 relative. Width cos 20 deg: the mean of n.w over the cone, cap_moments."""
    w, h = 40, 24

    def project(P, mesh_dict=None):
        return {"image": {"width": w, "height": h}, "renderer": P.renderer.simple(**renderer_args(pixel_samples, 2, 1)), "camera": project_camera(P, DOWN),
                "world": {"sky": 0, "objects": [floor(P), P.light.directional(direction=P.vector(*SUN), width=width_cos, color=1)]}}

    def checks(films, S):
        everywhere = np.ones((h, w), dtype=bool)
        if width_cos <= 0:
            return [exact_check("every pixel is rho cos / pi", films["main"], everywhere, RHO * SUN[2] / np.pi, tol=1e-5)]
        a, b = cap_moments(SUN[2], width_cos)
        return [region_check("image mean is rho / pi times the cone mean of n.w", films["main"], everywhere, RHO / np.pi * a, (RHO / np.pi) ** 2 * b, 1.0 / S)]

    return Case("directional_lamp_width_%.3f" % width_cos, {"main": project}, checks)


def directional_disc(width_cos=np.cos(np.radians(12.0)), pixel_samples=16):
    """No objects: every camera ray misses, and trace_directional (tracer.rs:444-459) shows the lamp's colour where
    direction.ray >= width, the sky elsewhere (:323-328). The camera looks along the lamp's direction, fov 60: the disc of
    half-angle 12 deg is a circle of radius 7.4 pixels about the image centre."""
    w, h, sky = 40, 24, 0.25
    cam = Camera((0, 0, 0), SUN, fov=60)

    def project(P, mesh_dict=None):
        return {"image": {"width": w, "height": h}, "renderer": P.renderer.simple(**renderer_args(pixel_samples, 2, 1)), "camera": project_camera(P, cam),
                "world": {"sky": sky, "objects": [P.light.directional(direction=P.vector(*SUN), width=float(width_cos), color=1)]}}

    def checks(films, S):
        _, d = footprints(cam, w, h, BORDER, True)
        lamp, away, edge = classify((d * SUN).sum(-1) - width_cos, 1e-5)
        return [Check("straddling share", edge.mean(), 0.10, pixels=int(edge.sum())),
                exact_check("pixels inside the disc show the lamp", films["main"], lamp, 1.0),
                exact_check("pixels outside the disc show the sky", films["main"], away, sky)]

    return Case("directional_disc", {"main": project}, checks)


# ------------------------------------------------------------------------------------------------
# 3. sphere lamp over a plane
# ------------------------------------------------------------------------------------------------
def sphere_lamp(light_samples, pixel_samples, centre=(1.5, 0.0, 1.0), radius=0.25, allowance=0.0):
    """An emissive sphere (radiance 1) over the diffuse plane; the sphere is outside the view.
    light_samples = 0: the plane's bounce ray (uniform hemisphere, density 1 / 2 pi, weight rho 2 n.o) finds the sphere by chance
    and reads its emission (tracer.rs:303-318 with sample_light = true): value = rho 2 (n.o) on a hit, mean rho (r/d)^2 cos g
    (sphere_lamp_radiance), E[v^2] = rho^2 4 / (2 pi) integral of (n.o)^2 over the sphere's cap = rho^2 4 (1 - c) E_cap[(n.o)^2].
    light_samples > 0: sample_towards (shapes/mod.rs:209-251) samples the cone of the sphere of radius r - DIST_EPSILON (:216) --
    the reference's choice, followed here -- uniformly in solid angle, and solid_angle_towards (:253-271) weighs by the solid angle
    of the FULL radius: each of the L samples is rho Omega(r) / (L 2 pi) 2 (n.w) (tracer.rs:365, :423), so the mean is
    rho Omega(r) / pi E_cap(r - eps)[n.w] = rho (1 - c_r)(1 + c_r') cos g and the variance that of n.w over the cap, over L.
    The bounce ray that then hits the sphere is not counted (sample_light = false, tracer.rs:258, :304).
    `allowance` (relative) is added to the bound: the reference's own next-event deficit, see the test's docstring."""
    centre, w, h = np.asarray(centre, dtype=np.float64), 40, 24

    def project(P, mesh_dict=None):
        lamp = P.shape.sphere(position=P.vector(*centre), radius=radius, material={"surface": P.material.emissive(color=1)})
        return {"image": {"width": w, "height": h}, "renderer": P.renderer.simple(**renderer_args(pixel_samples, 2, light_samples)), "camera": project_camera(P, DOWN),
                "world": {"sky": 0, "objects": [floor(P), lamp]}}

    def moments():
        x = plane_hit(*footprints(DOWN, w, h, MIDPOINTS, False))
        v = centre - x
        d2 = (v * v).sum(-1)
        cos_g = v[..., 2] / np.sqrt(d2)
        c_full = np.sqrt(1.0 - radius * radius / d2)
        if light_samples == 0:
            m1 = sphere_lamp_radiance(RHO, 1.0, radius, np.sqrt(d2), cos_g)
            m2 = RHO ** 2 * 4.0 * (1.0 - c_full) * cap_moments(cos_g, c_full)[1]
        else:
            c_sampled = np.sqrt(1.0 - (radius - DIST_EPSILON) ** 2 / d2)
            a, b = cap_moments(cos_g, c_sampled)
            k = RHO * 2.0 * (1.0 - c_full)  # rho Omega(r) / pi
            m1 = k * a
            m2 = m1 * m1 + k * k * (b - a * a) / light_samples
        return m1.mean(axis=(-1, -2)), m2.mean(axis=(-1, -2))

    def checks(films, S):
        m1, m2 = moments()
        c = region_check("image mean is rho (r/d)^2 cos", films["main"], np.ones((h, w), dtype=bool), m1, m2, 1.0 / S)
        c.bound += allowance * c.expected
        return [c]

    return Case("sphere_lamp_L%d_r%g_at_%g_%g_%g" % ((light_samples, radius) + tuple(centre)), {"main": project}, checks)


# ------------------------------------------------------------------------------------------------
# 4, 5. Schlick half-space, without and with dispersion
# ------------------------------------------------------------------------------------------------
GRAZING = Camera((0, -5, 1), (0, 0, 0), fov=10, up=(0, 0, 1))
LEVEL = Camera((0, -5, 1), (0, 0, 1), fov=10, up=(0, 0, 1))  # looks along the horizon: the upper rows see the sky alone


def schlick_half_space(dispersion=0.0, pixel_samples=10400, bins=64, camera=GRAZING):
    """A refractive plane z = 0 (ior 1.5, colour 1) over a black diffuse plane z = -1, sky 1, no lamps, light_samples = 0. A
    camera ray that meets the glass at cos theta reflects with probability p = 1/4 + Re/2 and weight Re / p into the sky, or refracts with weight Tr / (1 - p) onto the black plane, where the path's
    reflectance becomes 0 (refractive.rs:46-91, refract_moments). Re = schlick(cos theta, ior). Rays above the horizon read the
    sky, exactly 1. The GRAZING camera (11.3 deg below the horizon, +-3 deg of rows) has no such row; the LEVEL camera looks along
    the horizon, so its upper rows are sky, its lower rows meet the glass at under 3 deg (Re 0.87 and more), and the two rows that
    touch the horizon are left out.
    With dispersion the path's ior is ior + dispersion / (lambda / 1000)^2 (refractive.rs:15-19) and only the main wavelength is
    exposed (simple.rs:123-139): bin b holds the mean of Re over the bin's wavelength interval [start + b width / bins, ...)
    (film.rs:85-87; the main wavelength is uniform over the span: a stratum picked uniformly, simple.rs:105-106, and uniform
    inside it, film.rs:68-83)."""
    w, h, ior = 40, 24, 1.5

    def project(P, mesh_dict=None):
        glass = P.shape.plane(origin=P.vector(0, 0, 0), normal=P.vector(z=1), material={"surface": P.material.refractive(color=1, ior=ior, dispersion=dispersion or None)})
        return {"image": {"width": w, "height": h}, "renderer": P.renderer.simple(**renderer_args(pixel_samples, 4, 0, bins=bins)), "camera": project_camera(P, camera),
                "world": {"sky": 1, "objects": [glass, floor(P, rho=0, z=-1.0)]}}

    def checks(films, S):
        grains = films["main"]
        o, d = footprints(camera, w, h, MIDPOINTS, False)
        _, db = footprints(camera, w, h, BORDER, True)
        below, above, _ = classify(-db[..., 2], 1e-6)
        cos_t = -d[..., 2]
        out = []
        if above.any():
            out.append(exact_check("rows above the horizon show the sky", grains, above, 1.0))
        if not dispersion:
            m1, m2 = (m.mean(axis=(-1, -2)) for m in refract_moments(schlick(cos_t, ior)))
            for row in range(h):
                mask = np.zeros((h, w), dtype=bool)
                mask[row] = below[row]
                if mask.any():
                    out.append(region_check("row %d mean is Re(theta)" % row, grains, mask, m1, m2, 1.0 / S))
            return out
        nb, group = np.asarray(grains).shape[2], 8
        quarter = {}
        for b0 in range(0, nb, group):
            lam = SPAN[0] + (b0 + (np.arange(group * 16) + 0.5) / 16.0) * (SPAN[1] - SPAN[0]) / nb  # 16 midpoints per bin
            re = schlick(cos_t[..., None], dispersed_ior(ior, dispersion, lam))
            m1, m2 = (m.mean(axis=(-1, -2, -3)) for m in refract_moments(re))
            out.append(region_check("bins %d-%d mean is Re(theta, ior(lambda))" % (b0, b0 + group - 1), grains, below, m1, m2, 1.0, bins=slice(b0, b0 + group)))
        g = np.asarray(grains, dtype=np.float64)[below]
        first, last = (g[:, s, 0].sum() / g[:, s, 1].sum() for s in (slice(0, nb // 4), slice(nb - nb // 4, nb)))
        blue, red = out[-nb // group].expected, out[-1].expected  # shorter wavelengths have the higher ior and reflect more
        assert blue > red and first > last, "the first quarter of bins (%.5f) must lie above the last (%.5f)" % (first, last)
        return out

    name = "schlick_half_space" + ("_dispersion_%g" % dispersion if dispersion else "") + ("_level" if camera is LEVEL else "")
    return Case(name, {"main": project}, checks, resolution=0.02 if dispersion else 0.01)


# ------------------------------------------------------------------------------------------------
# 6, 7. a sphere in a uniform sky: glass furnace and mixes
# ------------------------------------------------------------------------------------------------
BALL = Camera((0, 0, 10), (0, 0, 0), fov=20)  # unit sphere at the origin: a disc of radius 11.4 pixels


def on_ball(cam, w, h, min_cos=0.0):
    """(pixels wholly on the unit sphere, pixels wholly off it, straddlers, cos of incidence at the 8 x 8 midpoints). A pixel is on
    the sphere if the whole footprint hits it with cos(incidence) > min_cos."""
    hit, cos_b = sphere_hit(*footprints(cam, w, h, BORDER, True), np.zeros(3), 1.0)
    inside, _, _ = classify(np.where(hit, cos_b - min_cos, -1.0), 1e-4)
    o, d = footprints(cam, w, h, BORDER, True)
    l = -o
    miss = np.sqrt(np.maximum((l * l).sum(-1) - (l * d).sum(-1) ** 2, 0.0)) - 1.0  # distance of the ray from the sphere's surface
    outside = (miss > 1e-4).all(axis=(-1, -2))
    _, cos_m = sphere_hit(*footprints(cam, w, h, MIDPOINTS, False), np.zeros(3), 1.0)
    return inside, outside, ~(inside | outside), cos_m


def glass_furnace(dispersion=0.0, pixel_samples=640, sky=0.75, bounces=32):
    """A glass sphere (ior 1.5, colour 1) in a sky of 0.75: every weight of refractive.rs:80-90 has expectation 1 over its branch
    choice and a sphere cannot trap a ray by total internal reflection, so the mean is the sky (glass_sphere_moments, which also
    gives sigma1 and the 1e-12 the 32-segment cut removes). Pixels off the sphere are exactly the sky. The rim where
    cos(incidence) < 0.1 is left out of the region: towards grazing Re^2 / p passes 1 and the variance is unbounded. With
    dispersion each path has the ior of its main wavelength and exposes it alone."""
    w, h, ior = 40, 24, 1.5

    def project(P, mesh_dict=None):
        ball = P.shape.sphere(position=P.vector(0, 0, 0), radius=1.0, material={"surface": P.material.refractive(color=1, ior=ior, dispersion=dispersion or None)})
        return {"image": {"width": w, "height": h}, "renderer": P.renderer.simple(**renderer_args(pixel_samples, bounces, 0)), "camera": project_camera(P, BALL),
                "world": {"sky": sky, "objects": [ball]}}

    def checks(films, S):
        inside, outside, _, cos_m = on_ball(BALL, w, h, min_cos=0.1)
        cos_m = np.where(inside[..., None, None], cos_m, 1.0)
        if dispersion:
            lam = SPAN[0] + (np.arange(16) + 0.5) / 16.0 * (SPAN[1] - SPAN[0])
            re = schlick(cos_m[..., None], dispersed_ior(ior, dispersion, lam))
            m1, m2 = (m.mean(axis=(-1, -2, -3)) for m in glass_sphere_moments(re, bounces))
        else:
            m1, m2 = (m.mean(axis=(-1, -2)) for m in glass_sphere_moments(schlick(cos_m, ior), bounces))
        return [exact_check("pixels off the sphere show the sky", films["main"], outside, sky),
                region_check("mean over the sphere is the sky", films["main"], inside, sky * m1, sky * sky * m2, 1.0 if dispersion else 1.0 / S)]

    return Case("glass_furnace" + ("_dispersion_%g" % dispersion if dispersion else ""), {"main": project}, checks)


def mixes(kind, pixel_samples=1024):
    """A sphere under sky 1, light_samples = 0; every bounce ray leaves the convex sphere and reads the sky. A diffuse event is
    rho 2 cos with cos uniform in [0, 1] (sample_hemisphere, math.rs:155-164: z = |cos| of a uniform sphere point):
    E = rho, E[v^2] = 4 rho^2 / 3.
    material: mix(diffuse 0.2, diffuse 0.8, 0.25). SurfaceMaterial::from_project (materials/mod.rs:176-195) gives the LHS the
        probability `amount` and the rhs 1 - amount; a component is picked uniformly (1/2) and compensated by the component
        count 2 (:48-54, :213-247): value = 2 a 0.2 2 cos or 2 (1 - a) 0.8 2 cos, mean 0.25 0.2 + 0.75 0.8 = 0.65.
    colour: diffuse(mix(0.2, 0.8, 0.25)). lib.lua:104-118 only names the operands lhs, rhs, amount; the instruction
        (program/execution_context.rs:195-211) computes lhs (1 - amount) + rhs amount: here the amount weighs the RHS, 0.35.
    fresnel: mix(mirror 1, diffuse 0.5, fresnel(1.5)): amount = F(theta) = reference_fresnel: value 2 F (mirror, probability 1/2) or
        2 (1 - F) 0.5 2 cos: mean F + (1 - F) / 2, E[v^2] = 2 F^2 + 2 (1 - F)^2 / 3."""
    w, h = 40, 24

    def project(P, mesh_dict=None):
        m = {"material": lambda: P.mix(P.material.diffuse(color=0.2), P.material.diffuse(color=0.8), 0.25),
             "colour": lambda: P.material.diffuse(color=P.mix(0.2, 0.8, 0.25)),
             "fresnel": lambda: P.mix(P.material.mirror(color=1), P.material.diffuse(color=0.5), P.fresnel(1.5))}[kind]()
        ball = P.shape.sphere(position=P.vector(0, 0, 0), radius=1.0, material={"surface": m})
        return {"image": {"width": w, "height": h}, "renderer": P.renderer.simple(**renderer_args(pixel_samples, 4, 0)), "camera": project_camera(P, BALL),
                "world": {"sky": 1, "objects": [ball]}}

    def checks(films, S):
        inside, outside, _, cos_m = on_ball(BALL, w, h)
        if kind == "material":
            a = 0.25
            m1, m2 = a * 0.2 + (1 - a) * 0.8, 0.5 * (2 * a * 0.2) ** 2 * 4 / 3 + 0.5 * (2 * (1 - a) * 0.8) ** 2 * 4 / 3
        elif kind == "colour":
            rho = 0.2 * (1 - 0.25) + 0.8 * 0.25
            m1, m2 = rho, 4 * rho * rho / 3
        else:
            f = reference_fresnel(np.where(inside[..., None, None], cos_m, 1.0), 1.5)
            m1, m2 = (f + (1 - f) * 0.5).mean(axis=(-1, -2)), (2 * f * f + 2 * (1 - f) ** 2 / 3).mean(axis=(-1, -2))
        return [exact_check("pixels off the sphere show the sky", films["main"], outside, 1.0),
                region_check("mean over the sphere (%s mix)" % kind, films["main"], inside, m1, m2, 1.0 / S)]

    return Case("mix_" + kind, {"main": project}, checks)


# ------------------------------------------------------------------------------------------------
# 8. pinhole mapping
# ------------------------------------------------------------------------------------------------
def pinhole_mapping(pixel_samples=16):
    """An emissive unit sphere at depth 10, off the axis by (1.5, 0.8), fov 30, bounces 1: a pixel is 1 where its rays meet the
    sphere and 0 elsewhere. The silhouette is the cone of half-angle asin(r / |c|) about the direction to the centre, seen through
    view_plane = cot(fov / 2) over HALF THE LONGER side (cameras.rs:43-45, :57-68) with the image's y pointing down (:81)."""
    w, h = 40, 24
    cam, centre = Camera((0, 0, 10), (0, 0, 0), fov=30), np.array([1.5, 0.8, 0.0])

    def project(P, mesh_dict=None):
        ball = P.shape.sphere(position=P.vector(*centre), radius=1.0, material={"surface": P.material.emissive(color=1)})
        return {"image": {"width": w, "height": h}, "renderer": P.renderer.simple(**renderer_args(pixel_samples, 1, 0)), "camera": project_camera(P, cam),
                "world": {"sky": 0, "objects": [ball]}}

    def checks(films, S):
        _, d = footprints(cam, w, h, BORDER, True)
        c = centre - cam.from_
        dist = np.linalg.norm(c)
        on, off, edge = classify((d * (c / dist)).sum(-1) - np.sqrt(1.0 - 1.0 / (dist * dist)), 1e-5)
        assert on.sum() > 50 and on[:, : w // 2].sum() == 0 and on[h // 2 + 4:].sum() == 0  # right of the centre, in the upper half
        return [Check("straddling share", edge.mean(), 0.10, pixels=int(edge.sum())),
                exact_check("pixels inside the silhouette are 1", films["main"], on, 1.0),
                exact_check("pixels outside the silhouette are 0", films["main"], off, 0.0)]

    return Case("pinhole_mapping", {"main": project}, checks)


# ------------------------------------------------------------------------------------------------
# 9. thin lens
# ------------------------------------------------------------------------------------------------
def thin_lens(quad_z, pixel_samples, half=(0.4, 0.3), aperture=0.04, fov=40):
    """An emissive quad +-(0.4, 0.3) at height quad_z under the camera at (0, 0, 5), focus_distance 5, aperture 0.04: the lens is
    the disc of radius sqrt(aperture) = 0.2 (cameras.rs:84: sqrt(aperture U)), every lens ray goes through the pinhole ray's point
    in the focal plane (:78-89). A lens ray from l through the focal point T meets the quad's plane, at distance z below the lens,
    at l (1 - z/f) + T z/f: the pinhole's point blurred by a disc of radius R |1 - z/f| -- in pixels
    R |1/f - 1/z| view_plane max_dim / 2 (2.2 at fov 40, width 40; the fov is 40 so that the quad at z = 2.5, its blur and a margin
    fit into the 24 rows).
    quad_z = 0 (the focal plane): the disc has radius 0. The film equals the pinhole render's, weights and values, wherever the
        footprint does not straddle the quad's edge: the sample's film position is drawn before the lens (simple.rs:87-89) and a pixel's
        weight does not depend on the ray (the wavelengths, drawn after the lens, fall into other bins: the pixel's weight is the
        sum over its bins).
    quad_z = 2.5: pixels further than the blur radius from every edge are exactly 1 or 0; elsewhere a sample sees the quad with
        probability disc_segment(s) (one straight edge inside the disc: the quad's half sizes exceed the disc's diameter), a
        Bernoulli value, so E = P and E[v^2] = P. Column means across the edges x = +-0.4 are taken over the rows whose blur
        discs stay inside the quad in y, row means across y = +-0.3 likewise; columns whose expectation is below 0.25 are left
        out, because 1 % of so small an expectation is out of reach of any sample count a quick test can use."""
    w, h = 40, 24
    half = np.asarray(half, dtype=np.float64)
    cam = Camera((0, 0, 5), (0, 0, 0), fov=fov, focus_distance=5.0, aperture=aperture)
    pin = Camera((0, 0, 5), (0, 0, 0), fov=fov)
    blur = np.sqrt(aperture) * abs(1.0 - (5.0 - quad_z) / 5.0)

    def project_with(camera):
        def project(P, mesh_dict):
            x, y = half
            corners = np.array([[-x, -y, quad_z], [x, -y, quad_z], [x, y, quad_z], [-x, y, quad_z]], dtype=np.float32)
            positions = np.array([corners[[0, 1, 2]], corners[[0, 2, 3]]], dtype=np.float32)
            normals = np.tile(np.array([0, 0, 1], dtype=np.float32), (2, 3, 1))
            quad = P.shape.mesh(file=mesh_dict("quad", positions, normals), materials={"quad": {"surface": P.material.emissive(color=1)}})
            return {"image": {"width": w, "height": h}, "renderer": P.renderer.simple(**renderer_args(pixel_samples, 1, 0)), "camera": project_camera(P, camera),
                    "world": {"sky": 0, "objects": [quad]}}
        return project

    def checks(films, S):
        grains = films["main"]
        xb = plane_hit(*footprints(pin, w, h, BORDER, True), quad_z)[..., :2]
        depth = half - np.abs(xb)  # signed distance inside each pair of edges, [h, w, n, n, 2]
        inside, _, _ = classify(depth.min(-1) - blur, 1e-5)
        outside = ((-depth - blur) > 1e-5).all(axis=(-2, -3)).any(-1)  # the whole footprint beyond one edge by more than the blur
        out = [exact_check("pixels inside the quad are 1", grains, inside, 1.0), exact_check("pixels outside the quad are 0", grains, outside, 0.0)]
        if blur == 0:
            sharp = inside | outside
            a, b = np.asarray(grains), np.asarray(films["pinhole"])
            out.append(Check("pixel weights equal the pinhole render's", np.abs(a[..., 1].sum(-1, dtype=np.float64) - b[..., 1].sum(-1, dtype=np.float64)).max(), 0.0))
            out.append(Check("values equal the pinhole render's off the edge", np.abs(values(a) - values(b))[sharp].max(), 0.0, pixels=int(sharp.sum())))
            assert sharp.mean() > 0.9
            return out
        xm = plane_hit(*footprints(pin, w, h, MIDPOINTS, False), quad_z)[..., :2]
        for axis, name in ((0, "column"), (1, "row")):
            other = 1 - axis
            clear = ((depth[..., other] - blur) > 1e-5).all(axis=(-1, -2))  # the disc stays inside the quad across the other axis
            p = disc_segment((half[axis] - np.abs(xm[..., axis])) / blur).mean(axis=(-1, -2))
            for k in range(w if axis == 0 else h):
                mask = np.zeros((h, w), dtype=bool)
                if axis == 0:
                    mask[:, k] = clear[:, k]
                else:
                    mask[k, :] = clear[k, :]
                mask &= ~(inside | outside)
                if mask.any() and p[mask].mean() >= 0.25:
                    out.append(region_check("%s %d follows the disc-segment profile" % (name, k), grains, mask, p, p, 1.0 / S))
        assert sum(c.noise is not None for c in out) >= 8, "the profile must be sampled on both sides of both axes"
        return out

    renders = {"main": project_with(cam)}
    if blur == 0:
        renders["pinhole"] = project_with(pin)
    return Case("thin_lens_quad_z_%g" % quad_z, renders, checks)


# ------------------------------------------------------------------------------------------------
# the cases, at the sample counts of the GPU test
# ------------------------------------------------------------------------------------------------
# Next-event estimation towards a sphere lamp loses the samples whose shadow ray, re-intersecting the lamp, comes out nearer than
# the sampled point by more than DIST_EPSILON in SQUARED distance (tracer.rs:381-389 against lamp.rs:54-62; DESIGN section 6 has
# the table): the reference's own bias. The oracle's deficit at (1.5, 0, 1), r = 0.25, measured on the CPU with 16384 samples per
# pixel (16 x the test's), was 0.0522 % (1 light sample) and 0.0548 % (4), each +- 0.017 %; the allowance is twice that.
NEE_ALLOWANCE = {1: 2 * 0.000522, 4: 2 * 0.000548}


def cases():
    return [
        point_lamp(), point_lamp(occluder_radius=0.3), point_lamp(occluder_radius=0.1),
        directional_lamp(0.0), directional_lamp(float(np.cos(np.radians(20.0)))), directional_disc(),
        sphere_lamp(0, 28000), sphere_lamp(1, 1024, allowance=NEE_ALLOWANCE[1]), sphere_lamp(4, 1024, allowance=NEE_ALLOWANCE[4]),
        schlick_half_space(), schlick_half_space(camera=LEVEL), schlick_half_space(dispersion=0.05, pixel_samples=1024),
        glass_furnace(), glass_furnace(dispersion=0.02),
        mixes("material"), mixes("colour"), mixes("fresnel"),
        pinhole_mapping(),
        thin_lens(0.0, 64), thin_lens(2.5, 76000),
    ]


def build_projects(case, P, mesh_dict, pixel_samples=None):
    """{render name: project} of a case; `P` is the pyrite_amd.project module, `mesh_dict` scenes._mesh_dict_from_arrays.
    `pixel_samples` overrides the case's sample count (the CPU test renders fewer)."""
    out = {}
    for name, build in case.renders.items():
        project = build(P, mesh_dict)
        if pixel_samples is not None:
            project["renderer"] = project["renderer"].with_(pixel_samples=int(pixel_samples))
        out[name] = project
    return out
