"""Random ABI-level material programs (tests/program_gen.py) through every GPU program form on an MI355X.

A. Every instruction, bit for bit, through the feature pass: with grid 1 and a material of one diffuse component the albedo grain of a
   pixel is (0 + 1 * colour) / 1, the colour program's value at the bin's centre wavelength and the pixel's normal, incident
   direction and texture coordinates (kernels/features.hip feature_shade). The independent evaluator
   (tests/program_restatement.py), run on the oracle's first-hit surface data, gives the expected bit pattern of every grain; inf and
   NaN included. The in-register build and the wide build both run (features_kernel<true>, wide::features_kernel<true>).
B. Every program form through the render kernels: scenes whose colour programs are all of one family, so that
   pyr_scene_path_info's `tape` tells what scene_pack.cpp's pack_program / split_product made of them, rendered with and without the hit
   tape at 1, 4 and 7 wavelengths a path, staged in LDS and on a mesh walked from memory, against the oracle's film as
   tests/test_gpu_parity.py states parity.

Which programs may colour a surface is decided on the CPU (tests/test_program_forms_cpu.py: the filter and its quotas). The tests
print one line per scene ("program forms A ..." / "program forms B ..."), collected in profiles/r10_program_forms.txt.
PYRITE_FORMS_SEEDS=N runs N corpora instead of the fixed one, PYRITE_FORMS_BASE=B starts them at another seed."""
import functools
import os

import numpy as np
import pytest

import oracle
import program_restatement as R
from program_gen import Case, Gen, const, near_miss_names, writes_number
from pyrite_amd import abi, scenes
from pyrite_amd.project import camera, light, light_source, material, mix, shape, transform, vector
from pyrite_amd.renderer import Camera, Renderer, World
from test_gpu_features import TOL, camera_rays, material_of
from test_gpu_parity import assert_parity, rel_l2
from test_gpu_program_registers import assert_same_counters
from test_program_forms_cpu import SEED, allocate, append_programs, corpus, fits, renderable, tables, tables_flat

pytestmark = pytest.mark.gpu
f32 = np.float32
SEEDS = [SEED + int(os.environ.get("PYRITE_FORMS_BASE", "0")) + k for k in range(int(os.environ.get("PYRITE_FORMS_SEEDS", "1")))]
PER_SCENE = 8


# ------------------------------------------------------------------------------------------------ the scenes
SPHERES = [((-2.1, 0.0, 0.7), 0.65), ((-0.7, 0.0, 0.7), 0.65), ((0.7, 0.0, 0.7), 0.65), ((2.1, 0.0, 0.7), 0.65),
           ((-1.4, 1.8, 1.9), 0.6), ((0.0, 1.8, 1.9), 0.6), ((1.4, 1.8, 1.9), 0.6)]
CAMERA = camera.perspective(fov=55, transform=transform.look_at(**{"from": vector(0.3, -7, 2.5), "to": vector(0, 0, 1), "up": vector(z=1)}))


def knot(material_):
    tri, nrm = scenes.torus_knot_mesh(segments=40, sides=10, noise_seed=3, fit_min=(-0.9, 1.2, 1.3), fit_max=(0.9, 2.4, 2.5))
    n = len(tri)
    uv = (tri.reshape(-1, 3)[:, :2] * f32(0.7) + tri.reshape(-1, 3)[:, 2:3] * f32(0.3)).astype(f32)
    corner = np.arange(3 * n).reshape(n, 3)
    mesh = {"position": tri.reshape(-1, 3), "texture": uv, "normal": nrm.reshape(-1, 3),
            "objects": [{"name": "knot", "polys": [[(int(a), int(a), int(a)), (int(b), int(b), int(b)), (int(c), int(c), int(c))] for a, b, c in corner]}]}
    return shape.mesh(file=mesh, materials={"knot": material_})


def sphere(k, surface):
    position, radius = SPHERES[k]
    return shape.sphere(position=vector(*position), radius=radius, material={"surface": surface}, texture_scale=vector(0.5, 0.5))


def plane(surface):
    return shape.plane(origin=vector(0, 0, 0), normal=vector(0, 0, 1), material={"surface": surface}, texture_scale=vector(2, 2))


def grey():
    return material.diffuse(color=0.5)


# ------------------------------------------------------------------------------------------------ A. the feature pass, bit for bit
A_SIZE = (32, 20)


def feature_flat(cases, normal_maps=()):
    """A plane and seven spheres, one diffuse component each: object k is coloured by cases[k] (grey where there is none) and bent
    by normal_maps[k]. Cases past the eighth are programs of the scene that colour nothing (tests/test_scene_pack_cpu.py packs the
    whole corpus that way). Returns the FlatScene."""
    flat = tables_flat()
    assert not flat.components and not flat.materials
    flat.add_world({"objects": [plane(grey())] + [sphere(k, grey()) for k in range(len(SPHERES))]})
    assert len(flat.components) == len(flat.materials) == 1 + len(SPHERES)
    ids = append_programs(flat, list(cases) + list(normal_maps))
    for k in range(min(len(cases), len(flat.components))):
        flat.components[k]["color"] = ids[k]
    for k in range(len(normal_maps)):
        m = flat.materials[k]
        flat.materials[k] = (m[0], m[1], m[2], m[3], ids[len(cases) + k])
    return flat


def feature_world(cases, normal_maps=()):
    return World(feature_flat(cases, normal_maps))


def feature_renderer():
    return Renderer(pixel_samples=1, spectrum_samples=4, seed=1)


def first_hits(world):
    """The oracle's first hit of every pixel's centre ray: (rays [h, w, 6], shape, shading normal, texture coordinates, material)."""
    width, height = A_SIZE
    r = feature_renderer()
    span = r.spectrum_span
    normal_wl = f32(f32(span[0]) + f32(f32(span[1] - span[0]) * f32(0.5)))
    rays = camera_rays(Camera.from_project(CAMERA), width, height, 1).reshape(height, width, 6)
    scene = oracle.OracleScene(world)
    hits, _ = scene.intersect(rays.reshape(-1, 6))
    n = width * height
    normal, texture, mat = np.zeros((n, 3), f32), np.zeros((n, 2), f32), np.full(n, 0xFFFFFFFF, np.uint32)
    for i in np.nonzero(hits["shape"] != abi.HIT_NONE)[0]:
        _, t, _, shading = scene.surface_data(rays.reshape(-1, 6)[i], wavelength=float(normal_wl))
        normal[i], texture[i], mat[i] = shading, t, material_of(world.desc, hits["shape"][i])
    scene.close()
    return rays, hits["shape"].reshape(height, width), normal.reshape(height, width, 3), texture.reshape(height, width, 2), mat.reshape(height, width)


@functools.lru_cache(maxsize=None)
def plain_first_hits():
    """Without normal maps the first hits depend on the geometry alone: computed once for every scene of section A."""
    return first_hits(feature_world([]))


def bin_wavelengths(r, bins):
    start, width = f32(r.spectrum_span[0]), f32(r.spectrum_span[1] - r.spectrum_span[0])
    bin_width = f32(width / f32(bins))
    return np.array([f32(start + f32(f32(f32(b) + f32(0.5)) * bin_width)) for b in range(bins)], f32)


def expected_albedo(cases, hits, r, bins):
    """[h, w, bins] float32: 0 + the program's value, per pixel and bin, by the evaluator."""
    rays, _, normal, texture, mat = hits
    height, width = mat.shape
    out = np.zeros((height, width, bins), f32)
    wavelengths = bin_wavelengths(r, bins)
    for k in range(1 + len(SPHERES)):
        where = mat == k
        count = int(where.sum())
        if count == 0:
            continue
        if k >= len(cases):
            out[where] = f32(0.5)
            continue
        value = R.evaluate(tables(), cases[k].instrs, cases[k].p, np.tile(wavelengths, count), np.repeat(normal[where], bins, 0), np.repeat(rays[where][:, 3:], bins, 0),
                           np.repeat(texture[where], bins, 0))
        out[where] = R.add(f32(0.0), value).reshape(count, bins)  # the grain's 0 + x: a -0 becomes +0, nothing else changes
    return out


A_FAMILIES = ("general", "hit_value", "lambda", "fast", "hit_rgb", "product", "near_miss", "allocated")


def interleave(groups):
    """Round robin over the lists of `groups`, in their order, until all are empty."""
    groups, out = [list(g) for g in groups], []
    while any(groups):
        for g in groups:
            if g:
                out.append(g.pop(0))
    return out


def by_kind(cases):
    """The cases grouped by kind in order of first appearance (the special_* programs of a family form one group), interleaved."""
    groups = {}
    for c in cases:
        groups.setdefault("special" if c.kind.startswith("special_") else c.kind, []).append(c)
    return interleave(groups.values())


A_SCENES = 3


def feature_cases(seed, family, index, wide):
    """Eight number programs of the family, raw ones (inf, NaN, negative values) included, every kind of the family in turn: one,
    two and three factors, every fast shape and neighbour, every near miss, specials beside raw and closed programs, declared beside
    allocated. The in-register scenes take those that fit the in-register file once allocated; the wide scenes take those that need
    the wide build of their own first and put a program that certainly needs it in the last place."""
    pool = [c for c in corpus(seed) if c.family == family and c.p.output_kind == abi.OUTPUT_NUMBER and c.kind != "wide_forcer"]
    if wide:
        forcer = [c for c in corpus(seed) if c.kind == "wide_forcer"][0]
        pool = [c for c in pool if not c.fits] + by_kind([c for c in pool if c.fits])
        return pool[index * (PER_SCENE - 1):(index + 1) * (PER_SCENE - 1)] + [forcer]
    pool = by_kind([c for c in pool if c.fits])
    return pool[index * PER_SCENE:(index + 1) * PER_SCENE]


@pytest.mark.parametrize("build", ["registers", "wide"])
@pytest.mark.parametrize("index", range(A_SCENES))
@pytest.mark.parametrize("family", A_FAMILIES)
@pytest.mark.parametrize("seed", SEEDS)
def test_every_grain_of_the_albedo_is_the_evaluators_bit_pattern(seed, family, index, build, gpu_lib):
    """Observed on an MI355X: zero differing grains in every scene (profiles/r10_program_forms.txt)."""
    cases = feature_cases(seed, family, index, build == "wide")
    assert len(cases) == PER_SCENE, "the corpus holds too few %s programs for scene %d" % (family, index)
    world, r = feature_world(cases), feature_renderer()
    assert r.program_info(world)["wide"] == (1 if build == "wide" else 0)
    hits = plain_first_hits()
    cam = Camera.from_project(CAMERA)
    for bins in (5, 16):
        got = r.features(A_SIZE, cam, world, grid=1, albedo_bins=bins)
        assert np.array_equal(got.shape, hits[1]) and np.array_equal(got.material, hits[4]), "the pass and the oracle hit different things"
        grains = got.albedo.grains
        assert np.array_equal(grains[..., 1], np.ones_like(grains[..., 1])), "a grain's weight is not 1"
        want = expected_albedo(cases, hits, r, bins)
        same = R.same_bits(grains[..., 0], want)
        special = int((~np.isfinite(want)).sum())
        print("program forms A %s seed %d scene %d %s bins %d: %d grains compared, %d inf or NaN, %d differ" % (
            family, seed, index, build, bins, same.size, special, int((~same).sum())))
        if not same.all():
            y, x, b = [int(v) for v in np.argwhere(~same)[0]]
            k = int(hits[4][y, x])
            raise AssertionError("%d grains differ; first: pixel (%d, %d) bin %d, program %s: GPU %r (%#010x), evaluator %r (%#010x)" % (
                int((~same).sum()), x, y, b, cases[k].name, grains[y, x, b, 0], int(grains[y, x, b, 0].view(np.uint32)), want[y, x, b], int(want[y, x, b].view(np.uint32))))
    world.close()


@pytest.mark.parametrize("index", [0, 1, 2])
@pytest.mark.parametrize("seed", SEEDS)
def test_normal_map_programs_bend_the_normal_as_the_oracle_does(seed, index, gpu_lib):
    """Eight generated normal maps on the eight objects: the record's normal against oracle_surface_data's shading normal within 1e-5
    (tests/test_gpu_features.py TOL). Of the programs' raw vectors the CPU test holds the x component bitwise (oracle_run_program
    returns no more); y and z are held here alone, through the shading normal."""
    maps = renderable(seed)["normal_map"][index * PER_SCENE:(index + 1) * PER_SCENE]
    assert len(maps) == PER_SCENE
    world, r = feature_world([], maps), feature_renderer()
    assert r.program_info(world)["wide"] == 0
    rays, shapes, normal, _, mat = first_hits(world)
    got = r.features(A_SIZE, Camera.from_project(CAMERA), world, grid=1, albedo_bins=5)
    assert np.array_equal(got.shape, shapes) and np.array_equal(got.material, mat)
    error = float(np.abs(got.normal - normal).max())
    plain = float(np.abs(plain_first_hits()[2] - normal).max())
    print("program forms A normal_map seed %d scene %d: normal max abs %.3g (the maps move it by up to %.3g), bit-equal %s" % (
        seed, index, error, plain, got.normal.tobytes() == normal.tobytes()))
    assert plain > 0.05, "the normal maps do nothing"
    assert error <= TOL and not np.isnan(got.normal).any()
    world.close()


# ------------------------------------------------------------------------------------------------ B. the render kernels
B_SIZE = (24, 16)
WAVELENGTH_ONLY = ("lambda", "fast")


def one_minus(case):
    """The program 1 - case (the other side of a `mix` whose probability is `case`)."""
    n = case.p.num_numbers
    deps = [ins.deps for ins in case.instrs if ins.output == case.p.output_reg][-1]
    one = abi.PyrInstr(op=abi.OP_NUMBER, deps=0, output=n, x=const(1.0)[0])
    minus = abi.PyrInstr(op=abi.OP_BINARY, value_type=abi.VT_NUMBER, operator_=abi.BIN_SUB, deps=deps, output=n + 1, a=n, b=case.p.output_reg)
    p = abi.PyrProgram.from_buffer_copy(case.p)
    p.num_instrs, p.num_numbers, p.output_reg = p.num_instrs + 2, n + 2, n + 1
    return Case(case.family, case.kind + "_one_minus", list(case.instrs) + [one, minus], p)


def render_world(family, cases, mesh):
    """A plane, six spheres (the fifth a knot mesh with `mesh`), a ball lamp and a point lamp under a sky. The generated programs
    colour, in this order: the plane (diffuse), a mirror, a refractive sphere, the diffuse and the mirror side of a `mix`, an
    emissive component -- and then, for the families that read the wavelength alone, the point lamp and the sky; for the others two
    more diffuse spheres. A hit_value program is also the probability of the `mix`; normal_map programs bend the normals of the
    objects instead (colours are constants and fast shapes then). Everything else is a constant or a fast shape."""
    flat = tables_flat()
    lit = material.diffuse(color=0.5) + material.emissive(color=light_source.d65 * 0.2)
    mixed = mix(material.diffuse(color=0.5), material.mirror(color=0.5), 0.5)
    fifth = knot({"surface": grey()}) if mesh else sphere(5, grey())
    objects = [plane(grey()), sphere(0, material.mirror(color=0.5)), sphere(1, material.refractive(ior=1.5, color=0.5)), sphere(2, mixed), sphere(3, lit), sphere(4, grey()), fifth,
               shape.sphere(position=vector(0.5, -1.5, 4.5), radius=0.4, material={"surface": material.emissive(color=light_source.d65 * 8)}),
               light.point(position=vector(0, -3, 4), color=light_source.a * 12)]
    flat.add_world({"sky": light_source.d65 * 0.1, "objects": objects})
    comps = flat.components
    kinds = [c["bsdf"] for c in comps]
    # plane, mirror, refractive, the mix's two sides (pushed on a stack: the right side first), diffuse + emissive and the emissive list's copy, ...
    assert kinds[:4] == [abi.BSDF_DIFFUSE, abi.BSDF_MIRROR, abi.BSDF_REFRACTIVE, abi.BSDF_MIRROR] and kinds[4] == abi.BSDF_DIFFUSE, kinds
    mix_mirror, mix_diffuse = 3, 4
    emissive = [k for k, c in enumerate(comps) if c["bsdf"] == abi.BSDF_EMISSIVE][:2]  # the component and the emissive list's copy of it
    rest = [k for k, c in enumerate(comps) if c["bsdf"] == abi.BSDF_DIFFUSE and k > max(emissive)][:2]  # the sixth object's and the fifth's / the knot's
    assert len(emissive) == 2 and len(rest) == 2, kinds
    if family == "normal_map":
        ids = append_programs(flat, cases)
        assert len(cases) <= len(flat.materials)
        for k, program in enumerate(ids):  # materials in object order; the eighth is the ball lamp's
            m = flat.materials[k]
            flat.materials[k] = (m[0], m[1], m[2], m[3], program)
        flat.uses_normal_maps = True
        return World(flat)
    extra = [one_minus(cases[0])] if family == "hit_value" else []
    ids = append_programs(flat, list(cases) + extra)
    slots = [0, 1, 2, mix_diffuse, mix_mirror]
    for slot, program in zip(slots, ids):
        comps[slot]["color"] = program
    if len(cases) > 5:
        for k in emissive:
            comps[k]["color"] = ids[5]
    if family in WAVELENGTH_ONLY:
        if len(cases) > 6:
            [l for l in flat.lamps if l["kind"] == abi.LAMP_POINT][0]["color"] = ids[6]
        if len(cases) > 7:
            flat.sky_program = ids[7]
    else:
        for k, program in zip(rest, ids[6:8]):
            comps[k]["color"] = program
    if family == "hit_value":  # the mix: the diffuse side with probability cases[0], the mirror side with 1 - cases[0]
        comps[mix_diffuse]["probability"], comps[mix_mirror]["probability"] = ids[0], ids[len(cases)]
    return World(flat)


ALLOCATED_WITH_A_FORM = ("hit_value", "lambda", "hit_rgb", "product")


def allocated_version(case):
    return case if fits(case.p) else allocate(case)


def product_keeps_its_wavelength_factor(case):
    """Of an over-declared product, once allocated: is the register of l, the factor that depends on the wavelength alone, left alone
    after l's writer? The allocation pass gives every hit factor and every constant the wavelength side reads a register of its own
    (they are read by instructions that depend on the wavelength), so this is the one condition of split_product that the renumbering
    can turn: where l's register serves a later value, the program keeps the online form, and rightly."""
    instrs = allocated_version(case).instrs
    hit = abi.DEP_NORMAL | abi.DEP_INCIDENT | abi.DEP_TEXTURE
    writer = max(k for k, ins in enumerate(instrs) if ins.deps & abi.DEP_WAVELENGTH and not ins.deps & hit)
    return not any(writes_number(ins) and ins.output == instrs[writer].output for ins in instrs[writer + 1:])


def render_cases(seed, family, index):
    r = renderable(seed)
    if family == "general":
        pool = [c for c in r["general"] if c.kind == "number_closed" and c.fits]
    elif family == "wide":  # programs that need the wide build, a near miss that names register 16 among them, and others beside them
        wide = [c for c in r["general"] + r["near_miss"] if c.wide]
        pool = wide[index::2][:2] + [c for c in r["general"] if c.kind == "number_closed"][index * 6:(index + 1) * 6]
        return pool
    elif family == "product":  # one, two and three factors in every scene
        pool = interleave([c for c in r["product"] if c.kind == f] for f in "123")
    elif family == "near_miss":  # by name: every near miss at least twice over the scenes, no name twice in a scene
        pool = interleave([c for c in r["near_miss"] if c.kind == name and not c.wide] for name in near_miss_names())
    elif family == "fast":  # every kind in every scene
        pool = interleave([c for c in r["fast"] if c.kind == kind] for kind in Gen.FAST_KINDS)
    elif family == "allocated":  # every scene: each kind with a tape form as declared and as allocated (registers used again)
        kinds = [kind + version for kind in ALLOCATED_WITH_A_FORM for version in ("", "_after")]
        groups = [[c for c in r["allocated"] if c.kind == kind and c.fits] for kind in kinds]
        # the products that stay products once allocated first (scenes 0 to 3 record a tape), the others after them (scene 4 does not)
        pool = interleave(sorted(g, key=lambda c: not product_keeps_its_wavelength_factor(c)) if g[0].kind.startswith("product") else g for g in groups)
    elif family == "allocated_general":
        pool = interleave([c for c in r["allocated"] if c.kind == kind and c.fits] for kind in ("general", "general_after"))
    else:
        pool = [c for c in r[family] if c.fits]
    return pool[index * PER_SCENE:(index + 1) * PER_SCENE]


B_SCENES = [(family, index) for family in ("general", "hit_value", "lambda", "fast", "hit_rgb", "product", "allocated", "normal_map") for index in range(3)]
B_SCENES += [("near_miss", index) for index in range(7)] + [("wide", 0), ("wide", 1), ("allocated", 3), ("allocated", 4), ("allocated_general", 0)]
MESH_SCENE = {"near_miss": 3, "wide": 1, "allocated_general": None}  # the scene of a family that lies on the knot mesh (the others': 2)
EXPECTED_TAPE = {"hit_value": 2, "lambda": 2, "fast": 2, "hit_rgb": 2, "product": 2, "near_miss": 0, "wide": 0}  # general, allocated_general, normal_map: no claim


def expected_tape(family, cases):
    """What pyr_scene_path_info must report at four wavelengths or more; None for no claim."""
    if family == "allocated":  # every kind here has a tape form; an allocated product keeps it where l's register is left alone
        return 2 if all(product_keeps_its_wavelength_factor(c) for c in cases if c.kind.startswith("product")) else 0
    return EXPECTED_TAPE.get(family)


def renderer(spectrum_samples, seed):
    return Renderer(pixel_samples=2, bounces=3, light_samples=1, spectrum_samples=spectrum_samples, tile_size=8, seed=seed)


@pytest.mark.parametrize("family,index", B_SCENES)
@pytest.mark.parametrize("seed", SEEDS)
def test_a_scene_of_one_family_renders_the_oracles_film(seed, family, index, gpu_lib, monkeypatch):
    """One scene in all its runs: 1, 4 and 7 wavelengths a path, with the hit tape and with PYRITE_HIT_TAPE=0. One scene of every
    family (MESH_SCENE) lies on a knot mesh that is not staged in LDS."""
    cases = render_cases(seed, family, index)
    last = max(i for f, i in B_SCENES if f == family)
    mesh = index == MESH_SCENE.get(family, 2)
    assert len(cases) >= (2 if (family, index) == ("near_miss", last) or family == "wide" else PER_SCENE), "too few %s programs for scene %d" % (family, index)
    if family == "near_miss":
        assert len({c.kind for c in cases}) == len(cases)
    want = expected_tape(family, cases)
    cam = Camera.from_project(CAMERA)
    worst, tapes = 0.0, []
    for spectrum_samples in (1, 4, 7):
        r = renderer(spectrum_samples, seed + index)
        reference = render_world(family, cases, mesh)
        cfilm = r.new_film(*B_SIZE)
        ccount = oracle.OracleScene(reference).render(r, cam, cfilm, threads=8)
        for hit_tape in ("1", "0"):
            monkeypatch.setenv("PYRITE_HIT_TAPE", hit_tape)
            world = render_world(family, cases, mesh)
            info, programs = r.path_info(world), r.program_info(world)
            assert programs["wide"] == (1 if family == "wide" else 0)
            assert info["scene_in_lds"] == (0 if mesh else 1)
            if hit_tape == "1":
                tapes.append(info["tape"])
                if spectrum_samples >= 4 and want is not None:
                    assert info["tape"] == want, "%s scene %d at %d wavelengths: tape %d" % (family, index, spectrum_samples, info["tape"])
            else:
                assert info["tape"] == 0
            if spectrum_samples == 1:
                assert info["tape"] == 0  # the hero alone: nothing to replay
            gfilm = r.new_film(*B_SIZE)
            gcount = r.render(gfilm, cam, world, counters=True)
            worst = max(worst, float(rel_l2(gfilm, cfilm).max()))
            assert_parity(gfilm, cfilm)
            assert_same_counters(gcount, ccount)
            world.close()
        reference.close()
    print("program forms B %s seed %d scene %d (%s): %d programs, tape at 1/4/7 wavelengths %s, relL2 max %.3g" % (
        family, seed, index, "mesh" if mesh else "lds", len(cases), "/".join(str(t) for t in tapes), worst))


def single_program_world(case):
    flat = tables_flat()
    flat.add_world({"sky": light_source.d65 * 0.1, "objects": [plane(grey()), sphere(1, grey()), light.point(position=vector(0, -3, 4), color=light_source.a * 12)]})
    flat.components[0]["color"] = append_programs(flat, [case])[0]
    return World(flat)


@pytest.mark.parametrize("name", near_miss_names())
def test_each_near_miss_alone_is_refused_a_tape(name, gpu_lib):
    """The scenes above hold eight near misses each, and one refusal is enough for `tape` 0: here each stands alone, beside constants
    and fast shapes. The same scene with a product in its place records a tape."""
    r = renderer(4, 1)
    control = single_program_world(renderable()["product"][0])
    assert r.path_info(control)["tape"] == 2
    control.close()
    cases = [c for c in renderable()["near_miss"] if c.kind == name]
    assert len(cases) >= 2
    for case in cases:
        world = single_program_world(case)
        info = r.path_info(world)
        assert info["interpreter"] == 1 and info["tape"] == 0, (case.name, info)
        assert r.program_info(world)["wide"] == (1 if case.wide else 0)
        world.close()


@pytest.mark.parametrize("total", [124, 140])
def test_more_programs_than_a_hit_tape_takes(total, gpu_lib):
    """pyr_scene_create's "a hit tape takes at most 128 programs": with 124 programs of the caller's, of which three are products, the
    first two are split (126, 128 programs) and the third is not; with 140 none is. Either way the scene keeps the online form and
    equals the oracle."""
    products = renderable()["product"][:3]
    fast = renderable()["fast"][:3]

    def build():
        flat = tables_flat()
        flat.add_world({"sky": light_source.d65 * 0.1, "objects": [plane(grey()), sphere(0, grey()), sphere(2, grey()), sphere(5, material.mirror(color=0.5)),
                                                                    light.point(position=vector(0, -3, 4), color=light_source.a * 12)]})
        ids = append_programs(flat, products)
        for k, program in enumerate(ids):
            flat.components[k]["color"] = program
        while len(flat.programs) < total:
            append_programs(flat, [fast[len(flat.programs) % 3]])
        assert len(flat.programs) == total
        return World(flat)

    cam, r = Camera.from_project(CAMERA), renderer(4, 3)
    world = build()
    info = r.path_info(world)
    assert info["interpreter"] == 1 and info["tape"] == 0, info
    cfilm, gfilm = r.new_film(*B_SIZE), r.new_film(*B_SIZE)
    ccount = oracle.OracleScene(world).render(r, cam, cfilm, threads=8)
    gcount = r.render(gfilm, cam, world, counters=True)
    print("program forms B cap %d programs: tape %d, relL2 max %.3g" % (total, info["tape"], float(rel_l2(gfilm, cfilm).max())))
    assert_parity(gfilm, cfilm)
    assert_same_counters(gcount, ccount)
    world.close()


def test_a_shape_lamps_unused_colour_program_does_not_cost_the_tape(gpu_lib):
    """Found by the scenes above: PyrLamp::color_program belongs to directional and point lamps, and a shape lamp shines with its
    material's emissive components. pyr_scene_create nevertheless asked the program a shape lamp's field happens to name (here program
    0, the tables' own sum of textures and spectra, which has no tape form) for a tape form, and the scene lost its tape. Every
    colour that is read has one: the scene records a tape, and equals the oracle."""
    case = renderable()["lambda"][0]
    flat = tables_flat()
    flat.add_world({"sky": light_source.d65 * 0.1, "objects": [plane(grey()), sphere(1, grey()),
                                                                shape.sphere(position=vector(0.5, -1.5, 4.5), radius=0.4, material={"surface": material.emissive(color=light_source.d65 * 8)})]})
    flat.components[0]["color"] = append_programs(flat, [case])[0]
    shape_lamps = [l for l in flat.lamps if l["kind"] == abi.LAMP_SHAPE]
    assert shape_lamps and all(l.get("color", 0) == 0 for l in shape_lamps) and flat.programs[0]["kind"] == abi.PROGRAM_INSTRUCTIONS
    world = World(flat)
    cam, r = Camera.from_project(CAMERA), renderer(4, 2)
    assert r.path_info(world)["tape"] == 2
    cfilm, gfilm = r.new_film(*B_SIZE), r.new_film(*B_SIZE)
    ccount = oracle.OracleScene(world).render(r, cam, cfilm, threads=8)
    gcount = r.render(gfilm, cam, world, counters=True)
    assert_parity(gfilm, cfilm)
    assert_same_counters(gcount, ccount)
    world.close()
