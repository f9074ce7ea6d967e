"""Scenes whose material programs declare more registers than the interpreter's in-register file, against the CPU oracle on an
MI355X: those that fit after pyr_scene_create's register allocation run the usual interpreter builds (with and without the hit
tape), those that do not run the wide interpreter build. Parity as tests/test_gpu_parity.py states it."""
import os

import numpy as np
import pytest

from pyrite_amd import abi, lua_project, scenes
from pyrite_amd.compiler import FlatScene
from pyrite_amd.project import camera, fresnel, light, light_source, material, mix, renderer, rgb, shape, spectrum, texture, transform, vector
from pyrite_amd.renderer import World
from test_gpu_parity import assert_parity, render_both

pytestmark = pytest.mark.gpu
PROJECTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "projects")
PATH_KEYS = ("samples", "extension_rays", "shadow_rays", "shaded_hits", "exposures")
f32 = np.float32


def assert_same_counters(gcount, ccount):
    for key in PATH_KEYS:
        assert gcount[key] == ccount[key], key


def registers_project(width=48, height=32, spp=4):
    project, _ = lua_project.load_project(os.path.join(PROJECTS, "registers.lua"))
    project["image"] = {"width": width, "height": height}
    project["renderer"] = renderer.simple(pixel_samples=spp, spectrum_samples=6, bounces=4, light_samples=1, tile_size=16)
    return project


def render_project(project, seed, gpu_lib):
    cwd = os.getcwd()
    os.chdir(PROJECTS)  # registers.lua names its textures relative to itself
    try:
        return render_both(project, seed, gpu_lib)
    finally:
        os.chdir(cwd)


def program_info(project):
    cwd = os.getcwd()
    os.chdir(PROJECTS)
    try:
        world, _, r, _ = scenes.build(project, seed=1)
    finally:
        os.chdir(cwd)
    return r.program_info(world), r.path_info(world)


# ------------------------------------------------------------------------------------------------ 5. fits after allocation
@pytest.mark.parametrize("hit_tape", ["1", "0"])
def test_over_declared_scene_runs_the_in_register_build(hit_tape, gpu_lib, monkeypatch):
    monkeypatch.setenv("PYRITE_HIT_TAPE", hit_tape)
    project = registers_project()
    info, _ = program_info(project)
    assert (info["declared_numbers"], info["declared_vectors"], info["declared_rgbs"]) == (19, 13, 11)
    assert info["allocated_numbers"] <= abi.MAX_NUMBER_REGISTERS and info["allocated_vectors"] <= abi.MAX_VECTOR_REGISTERS
    assert info["allocated_rgbs"] <= abi.MAX_RGB_REGISTERS and info["wide"] == 0
    gfilm, cfilm, gcount, ccount = render_project(project, 7, gpu_lib)
    assert_parity(gfilm, cfilm)
    assert_same_counters(gcount, ccount)


def test_programs_sharing_a_range_render_like_the_oracle(gpu_lib):
    """The blend's program and a second program naming the same instructions colour two spheres: each is allocated from the caller's
    instructions (the one renumbered first must not change what the other reads)."""
    project = registers_project()
    cwd = os.getcwd()
    os.chdir(PROJECTS)
    try:
        world, cam, r, gfilm = scenes.build(project, seed=9)
        flat = world.flat
    finally:
        os.chdir(cwd)
    blend = [i for i, p in enumerate(flat.programs) if p["kind"] == abi.PROGRAM_INSTRUCTIONS and p["rgbs"] == 11]
    assert len(blend) == 1
    flat.programs.append(dict(flat.programs[blend[0]]))
    diffuse = [c for c in flat.components if c["bsdf"] == abi.BSDF_DIFFUSE and c["color"] != blend[0]]
    assert diffuse
    diffuse[0]["color"] = len(flat.programs) - 1
    world = World(flat)
    assert r.program_info(world)["allocated_rgbs"] <= abi.MAX_RGB_REGISTERS
    import oracle

    cfilm = r.new_film(gfilm.width, gfilm.height)
    ccount = oracle.OracleScene(world).render(r, cam, cfilm, threads=8)
    gcount = r.render(gfilm, cam, world, counters=True)
    assert_parity(gfilm, cfilm)
    assert_same_counters(gcount, ccount)


# ------------------------------------------------------------------------------------------------ 6. the wide build
@pytest.mark.parametrize("mesh", [False, True], ids=["lds_scene", "mesh"])
def test_scene_that_needs_the_wide_build(mesh, gpu_lib):
    project = scenes.wide_program_project(mesh)
    info, path = program_info(project)
    assert info["wide"] == 1 and info["allocated_rgbs"] > abi.MAX_RGB_REGISTERS and info["allocated_vectors"] > abi.MAX_VECTOR_REGISTERS
    assert info["allocated_rgbs"] <= abi.WIDE_RGB_REGISTERS and info["allocated_vectors"] <= abi.WIDE_VECTOR_REGISTERS
    assert path["interpreter"] == 1 and path["tape"] == 0 and path["scene_in_lds"] == (0 if mesh else 1)
    gfilm, cfilm, gcount, ccount = render_both(project, 3, gpu_lib)
    assert_parity(gfilm, cfilm)
    assert_same_counters(gcount, ccount)


# ------------------------------------------------------------------------------------------------ 7. the split's closed check
def test_a_hit_side_write_between_a_constant_and_its_wavelength_side_read(gpu_lib):
    """[c = 2 -> r0; clamp(0.25) -> r0; spectrum -> r1; r1 * r0 -> r2; 0.5 -> r3; r2 * r3 -> r4]: the wavelength side reads r0 after
    the clamp overwrote the constant. Splitting the product with the constant on the wavelength side computes spectrum * 2 * 0.5
    instead of spectrum * 0.25 * 0.5; the split must be refused and the film must equal the oracle's."""
    project = scenes.spheres_example(width=40, height=24, pixel_samples=4)
    project["renderer"] = renderer.simple(pixel_samples=4, bounces=4, light_samples=1, spectrum_samples=6, tile_size=16)
    world_desc = project["world"]
    flat = FlatScene().add_world(world_desc)
    assert flat.spectra, "the scene needs a spectrum to read"

    def op(op_, output, **kw):
        d = dict(op=op_, value_type=abi.VT_NUMBER, operator=0, deps=0, output=output, a=0, b=0, x=None, y=None, z=None, w=None)
        d.update(kw)
        return d

    def const(v):
        return (abi.OPERAND_CONSTANT, int(f32(v).view(np.uint32)))

    wl = (abi.OPERAND_INPUT, abi.INPUT_WAVELENGTH)
    program = [op(abi.OP_NUMBER, 0, x=const(2.0)), op(abi.OP_CLAMP, 0, x=const(0.25), y=const(0.0), z=const(1.0)),
               op(abi.OP_SPECTRUM, 1, x=wl, a=0, deps=abi.DEP_WAVELENGTH),
               op(abi.OP_BINARY, 2, operator=abi.BIN_MUL, a=1, b=0, deps=abi.DEP_WAVELENGTH), op(abi.OP_NUMBER, 3, x=const(0.5)),
               op(abi.OP_BINARY, 4, operator=abi.BIN_MUL, a=2, b=3, deps=abi.DEP_WAVELENGTH)]
    first = len(flat.instrs)
    flat.instrs.extend(program)
    flat.programs.append(dict(kind=abi.PROGRAM_INSTRUCTIONS, constant=0.0, first=first, n=len(program), output_kind=abi.OUTPUT_NUMBER, output_reg=4,
                              numbers=5, vectors=0, rgbs=0))
    diffuse = [c for c in flat.components if c["bsdf"] == abi.BSDF_DIFFUSE]
    assert diffuse
    for c in diffuse:
        c["color"] = len(flat.programs) - 1
    world = World(flat)
    _, cam, r, gfilm = scenes.build(project, seed=5)
    import oracle

    cfilm = r.new_film(gfilm.width, gfilm.height)
    ccount = oracle.OracleScene(world).render(r, cam, cfilm, threads=8)
    gcount = r.render(gfilm, cam, world, counters=True)
    assert_parity(gfilm, cfilm)
    assert_same_counters(gcount, ccount)


# ------------------------------------------------------------------------------------------------ 8. too large for the wide file
def test_too_large_for_the_wide_file_is_refused(gpu_lib):
    project = scenes.wide_program_project(False, textures=40)
    world, _, r, _ = scenes.build(project, seed=1)
    with pytest.raises(Exception) as error:
        world.scene(0)
    assert "RGB" in str(error.value) and str(abi.WIDE_RGB_REGISTERS) in str(error.value)


# ------------------------------------------------------------------------------------------------ 9. random scenes
def random_project(seed):
    """Spheres (or a torus knot) under materials whose colours are sums of 3-14 textured / spectral / RGB terms: most declare more
    registers than the in-register file; some fit after allocation, some need the wide build."""
    rng = np.random.default_rng(seed)
    tex = scenes._generated_textures(seed=seed, size=8)

    def term():
        kind = rng.integers(0, 5)
        s = spectrum(format="array", min=400.0, max=700.0, points=[float(x) for x in rng.uniform(0.1, 0.9, 4)])
        if kind == 0:
            return texture(tex["checker"]) * s
        if kind == 1:
            return texture(tex["mono"], "mono") * s
        if kind == 2:
            return rgb(*[float(x) for x in rng.uniform(0.1, 0.9, 3)]) * float(rng.uniform(0.2, 1.0))
        if kind == 3:
            return texture(tex["rgba"]) * float(rng.uniform(0.2, 1.0))
        return s * fresnel(float(rng.uniform(1.2, 1.8)))

    def colour():
        n = int(rng.integers(3, 15))
        e = term()
        for _ in range(n - 1):
            e = term() + e if rng.random() < 0.5 else e + term()
        return e * (1.0 / n)

    def surface():
        kind = rng.integers(0, 4)
        if kind == 0:
            return material.diffuse(color=colour())
        if kind == 1:
            return mix(material.diffuse(color=colour()), material.mirror(color=colour()), fresnel(float(rng.uniform(1.2, 1.7))))
        if kind == 2:
            return material.refractive(ior=float(rng.uniform(1.3, 1.9)), color=colour())
        return material.diffuse(color=colour()) + material.emissive(color=light_source.d65 * float(rng.uniform(0.1, 0.5)))

    def mat():
        m = {"surface": surface()}
        if rng.random() < 0.3:
            m["normal_map"] = scenes.layered_normal_map(seed) if rng.random() < 0.5 else texture(tex["normal_map"], "linear") * vector(1, -1, 1)
        return m

    objects = [shape.plane(origin=vector(0, 0, 0), normal=vector(0, 0, 1), material=mat(), texture_scale=vector(2, 2))]
    if rng.random() < 0.25:
        tri, nrm = scenes.torus_knot_mesh(segments=int(rng.integers(40, 70)), sides=int(rng.integers(10, 16)), noise_seed=int(seed), fit_min=(-2.5, -2.0, 0.2),
                                          fit_max=(2.5, 2.0, 3.2))
        n = len(tri)
        uv = (tri.reshape(-1, 3)[:, :2] * f32(0.7) + tri.reshape(-1, 3)[:, 2:3] * f32(0.3)).astype(f32)
        corner = np.arange(3 * n).reshape(n, 3)
        knot = {"position": tri.reshape(-1, 3), "texture": uv, "normal": nrm.reshape(-1, 3),
                "objects": [{"name": "knot", "polys": [[(int(a), int(a), int(a)), (int(b), int(b), int(b)), (int(c), int(c), int(c))] for a, b, c in corner]}]}
        objects.append(shape.mesh(file=knot, materials={"knot": mat()}))
    else:
        for _ in range(int(rng.integers(1, 4))):
            r = float(rng.uniform(0.3, 1.0))
            objects.append(shape.sphere(position=vector(float(rng.uniform(-2, 2)), float(rng.uniform(-1.5, 1.5)), r + float(rng.uniform(0, 1))), radius=r,
                                        material=mat(), texture_scale=vector(0.5, 0.5)))
    objects.append(shape.sphere(position=vector(float(rng.uniform(-2, 2)), 1.5, 3.5), radius=0.4, material={"surface": material.emissive(color=light_source.d65 * 8)}))
    objects.append(light.point(position=vector(0, -3, 4), color=light_source.a * float(rng.uniform(5, 20))))
    return {
        "image": {"width": int(rng.integers(20, 40)), "height": int(rng.integers(12, 28))},
        "renderer": renderer.simple(pixel_samples=int(rng.integers(1, 4)), bounces=int(rng.integers(1, 8)), light_samples=int(rng.integers(0, 3)),
                                    spectrum_samples=int(rng.integers(1, 9)), tile_size=16),
        "camera": camera.perspective(fov=55, transform=transform.look_at(**{"from": vector(0.3, -7, 2.5), "to": vector(0, 0, 1), "up": vector(z=1)})),
        "world": {"sky": light_source.d65 * 0.1, "objects": objects},
    }


SEEDS = list(range(1, 31))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_over_declared_scene_matches_the_oracle(seed, gpu_lib):
    project = random_project(seed)
    gfilm, cfilm, gcount, ccount = render_both(project, seed, gpu_lib)
    assert_parity(gfilm, cfilm)
    assert_same_counters(gcount, ccount)


def test_the_random_scenes_cover_both_forms(gpu_lib):
    wide = fits = 0
    for seed in SEEDS:
        info, _ = program_info(random_project(seed))
        over = max(info["declared_numbers"] - abi.MAX_NUMBER_REGISTERS, info["declared_vectors"] - abi.MAX_VECTOR_REGISTERS,
                   info["declared_rgbs"] - abi.MAX_RGB_REGISTERS) > 0
        wide += info["wide"]
        fits += 1 if over and not info["wide"] else 0
    assert wide >= 5 and fits >= 5, (wide, fits)
