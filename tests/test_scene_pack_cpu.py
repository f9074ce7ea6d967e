"""Scene creation's deciding half (pyrite_amd/csrc/scene_pack.cpp) on the CPU: tests/probes/pack_check.cpp, built with the address
and undefined-behaviour sanitizers, packs a dumped description (tests/scene_dump.py) as pyr_scene_create does -- validate, register
allocation, the tables step, the build-plan step, the host tree, the records step -- and prints every packed table's size and
digest and every scalar of DevScene, PyrBvhInfo and PyrProgramInfo, or the refusal's code and message.

The expected lines (tests/golden/scene_pack_pins.json) were NOT made by this code. They come from the commit before the packing
unit existed: a scratch build of that commit's api.cpp whose DeviceBuffer methods were malloc / memcpy / free plus a line that
printed each upload's size and digest, with the device lookup cut out of pyr_scene_create_with, loaded lazily and given the same
descriptions under the same switches. Its 23 uploads come in a fixed order; the scalars were printed from the scene it made; a
refusal's code and pyr_last_error() were taken as returned. A change that moves any decision of the packer fails here, on a machine
without a device.

Every scene is small and chosen for a branch (CASES below); the corpus scenes hold every Case of tests/program_gen.py, so the pinned
DevProgram tables hold each decision of pack_program and split_product the corpus aims at."""
import json
import os
import subprocess

import numpy as np
import pytest

import scene_dump
from pyrite_amd import abi, scenes
from pyrite_amd.compiler import FlatScene
from pyrite_amd.project import light_source, material, shape, vector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyrite_amd", "csrc")
PINS = os.path.join(ROOT, "tests", "golden", "scene_pack_pins.json")
SWITCHES = ("PYRITE_WIDE_BVH", "PYRITE_PAIR_PRIMS", "PYRITE_SPATIAL_SPLITS", "PYRITE_WIDE_COLLAPSE", "PYRITE_HIT_TAPE")


# ------------------------------------------------------------------------------------------------ the scenes
def project_flat(project):
    return FlatScene().add_world(project["world"])


def mesh_588():
    return scenes.c3_flat(segments=24, sides=12)


def mesh_and_a_sphere():
    """The 588-triangle mesh with one sphere: too big for LDS, so the wide tree; not triangles only, so no pair records."""
    flat = mesh_588()
    flat.add_world({"objects": [shape.sphere(position=vector(0, 0, 1), radius=0.5, material={"surface": material.diffuse(color=0.5)})]})
    return flat


def triangle_lamp_with_uvs():
    """A small emissive mesh with texture coordinates under a diffuse plane: every triangle is a shape lamp whose record takes
    its uvs."""
    tri, nrm = scenes.torus_knot_mesh(segments=6, sides=4, noise_seed=3, fit_min=(-0.9, 1.2, 1.3), fit_max=(0.9, 2.4, 2.5))
    n = len(tri)
    uv = (tri.reshape(-1, 3)[:, :2] * np.float32(0.7) + tri.reshape(-1, 3)[:, 2:3] * np.float32(0.3)).astype(np.float32)
    corner = np.arange(3 * n).reshape(n, 3)
    mesh = {"position": tri.reshape(-1, 3), "texture": uv, "normal": nrm.reshape(-1, 3),
            "objects": [{"name": "knot", "polys": [[(int(a), int(a), int(a)), (int(b), int(b), int(b)), (int(c), int(c), int(c))] for a, b, c in corner]}]}
    lit = {"surface": material.emissive(color=light_source.d65 * 4)}
    floor = shape.plane(origin=vector(0, 0, 0), normal=vector(0, 0, 1), material={"surface": material.diffuse(color=0.5)})
    flat = FlatScene().add_world({"objects": [floor, shape.mesh(file=mesh, materials={"knot": lit})]})
    assert any(l["kind"] == abi.LAMP_SHAPE and l.get("shape_kind") == abi.SHAPE_TRIANGLE for l in flat.lamps) and len(flat.tri_uvs)
    return flat


CORPUS_CHUNK = 40  # programs of the caller's in a chunk scene: with two more for every product, well under the 128 a hit tape takes


def corpus_cases():
    from test_program_forms_cpu import corpus  # (draws the corpus: a second or two, once)

    return list(corpus())


def corpus_flat(chunk=None):
    """The scene tests/test_gpu_program_forms.py section A renders, with every Case of the corpus as a program (chunk None): the
    pinned DevProgram table holds what pack_program makes of each. That scene holds hundreds of programs and wide ones among them,
    and split_product runs only in a scene of at most 128 programs that fits the in-register file: chunk k is the same scene with
    the k-th CORPUS_CHUNK of the cases that fit -- there the products are split and the near misses are not."""
    from test_gpu_program_forms import feature_flat

    cases = corpus_cases()
    if chunk is not None:
        cases = [c for c in cases if c.fits][chunk * CORPUS_CHUNK:(chunk + 1) * CORPUS_CHUNK]
        assert cases
    return feature_flat(cases)


def corpus_chunks():
    return (sum(1 for c in corpus_cases() if c.fits) + CORPUS_CHUNK - 1) // CORPUS_CHUNK


# ------------------------------------------------------------------------------------------------ the refusals
def refusal(base, change):
    def make():
        flat = base()
        desc = flat.desc()
        change(flat, desc)
        desc._flat = flat  # the description borrows its arrays
        return desc

    return make


def vertex_far_away(flat, desc):
    flat._keep["tp"][3, 4] = 2.0e15


def set_field(name, value):
    def change(flat, desc):
        setattr(desc, name, value)

    return change


def in_record(array, index, field, value):
    def change(flat, desc):
        setattr(flat._keep[array][index], field, value)

    return change


def in_array(array, index, value):
    def change(flat, desc):
        flat._keep[array].reshape(-1)[index] = value

    return change


def lamp_program_out_of_range(flat, desc):
    k = [i for i in range(desc.num_lamps) if desc.lamps[i].kind != abi.LAMP_SHAPE][0]
    desc.lamps[k].color_program = 10 ** 6


def too_many_registers(flat, desc):
    k = [i for i in range(desc.num_programs) if desc.programs[i].kind == abi.PROGRAM_INSTRUCTIONS][0]
    desc.programs[k].num_numbers = abi.MAX_DECLARED_REGISTERS + 1


def textures_flat():
    return project_flat(scenes.textures_example())


def lamps_flat():
    return project_flat(scenes.lamps_example())


# one branch of each loop of validate (and of what stands before the loops), by the message it ends in
REFUSALS = {
    "refuse_vertex_at_2e15": refusal(mesh_588, vertex_far_away),
    "refuse_sky_program": refusal(lamps_flat, set_field("sky_program", 10 ** 6)),
    "refuse_null_geometry": refusal(mesh_588, set_field("tri_normals", None)),
    "refuse_null_table": refusal(lamps_flat, set_field("spectra", None)),
    "refuse_instr_opcode": refusal(textures_flat, in_record("instrs", 0, "op", abi.OP_CLAMP + 1)),
    "refuse_spectrum_range": refusal(lamps_flat, in_record("spectra", 0, "count", 10 ** 6)),
    "refuse_texture_range": refusal(textures_flat, in_record("texrec", 0, "width", 10 ** 4)),
    "refuse_program_range": refusal(textures_flat, set_field("num_instrs", 1)),
    "refuse_material_components": refusal(lamps_flat, in_record("mats", 0, "num_components", 0)),
    "refuse_component_bsdf": refusal(lamps_flat, in_record("comps", 0, "bsdf", abi.BSDF_REFRACTIVE + 1)),
    "refuse_triangle_material": refusal(mesh_588, in_array("tm", 5, 10 ** 6)),
    "refuse_sphere_material": refusal(lamps_flat, in_array("sm", 0, 10 ** 6)),
    "refuse_plane_material": refusal(lamps_flat, in_array("pm", 0, 10 ** 6)),
    "refuse_lamp_program": refusal(lamps_flat, lamp_program_out_of_range),
    "refuse_declared_registers": refusal(textures_flat, too_many_registers),
}


# name -> (a function that makes the FlatScene, or the description itself; the switches it is packed under)
CASES = {
    "c1_spheres": (lambda: project_flat(scenes.c1_spheres()), {}),
    "c2_cornell": (lambda: project_flat(scenes.c2_cornell()), {}),
    "mesh_588": (mesh_588, {}),
    "mesh_588_and_a_sphere": (mesh_and_a_sphere, {}),
    "textures_example": (textures_flat, {}),
    "lamps_example": (lamps_flat, {}),
    "triangle_lamp_with_uvs": (triangle_lamp_with_uvs, {}),
    "mesh_588_no_wide": (mesh_588, {"PYRITE_WIDE_BVH": "0"}),
    "mesh_588_no_pairs": (mesh_588, {"PYRITE_PAIR_PRIMS": "0"}),
    "mesh_588_spatial": (mesh_588, {"PYRITE_SPATIAL_SPLITS": "1"}),
    "mesh_588_greedy": (mesh_588, {"PYRITE_WIDE_COLLAPSE": "greedy"}),
    "textures_example_no_hit_tape": (textures_flat, {"PYRITE_HIT_TAPE": "0"}),
    "corpus": (corpus_flat, {}),
    "corpus_no_hit_tape": (corpus_flat, {"PYRITE_HIT_TAPE": "0"}),
    "corpus_chunk_6_no_hit_tape": (lambda: corpus_flat(6), {"PYRITE_HIT_TAPE": "0"}),  # (a chunk whose eight colours all have a tape form)
}
CASES.update({name: (make, {}) for name, make in REFUSALS.items()})


def chunk_cases():
    """The chunk scenes of the corpus (their number follows from the corpus, which is drawn when a test runs, not when it is collected)."""
    return {"corpus_chunk_%d" % k: ((lambda k=k: corpus_flat(k)), {}) for k in range(corpus_chunks())}


def description(make):
    made = make()
    if isinstance(made, FlatScene):
        desc = made.desc()
        desc._flat = made
        return desc
    return made


def environment(switches):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    return env


# ------------------------------------------------------------------------------------------------ the probe
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pack_check") / "pack_check")
    sources = [os.path.join(ROOT, "tests", "probes", "pack_check.cpp")] + [os.path.join(CSRC, f) for f in ("scene_pack.cpp", "bvh.cpp", "program_regs.cpp", "error.cpp")]
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe] + sources)
    return exe


@pytest.fixture(scope="module")
def pins():
    with open(PINS) as f:
        return json.load(f)


def test_the_packing_unit_includes_no_hip_header():
    for name in ("scene_pack.cpp", "scene_pack.h", "error.cpp", "error.h"):
        with open(os.path.join(CSRC, name)) as f:
            assert "hip_runtime" not in f.read(), name


def test_every_case_is_pinned(pins):
    assert sorted(pins) == sorted(list(CASES) + list(chunk_cases()))


def assert_pinned(name, make, switches, probe, pins, tmp_path):
    path = str(tmp_path / (name + ".scene"))
    scene_dump.write(path, description(make))
    run = subprocess.run([probe, path], capture_output=True, text=True, timeout=120, env=environment(switches))
    assert run.returncode == 0, run.stdout + run.stderr
    got, want = run.stdout.splitlines(), pins[name]
    assert got[0].startswith("refused ") == name.startswith("refuse_"), got[0]
    differ = [(g, w) for g, w in zip(got, want) if g != w]
    assert not differ and len(got) == len(want), "%s: %d of %d lines differ (%d pinned); first: %r" % (name, len(differ), len(got), len(want), differ[:1])


@pytest.mark.parametrize("name", list(CASES))
def test_the_packed_scene_is_the_parent_commits(name, probe, pins, tmp_path):
    """Every line the probe prints -- 23 tables and the scalars, or the refusal -- equals the line pinned from the commit before."""
    assert_pinned(name, *CASES[name], probe, pins, tmp_path)


def test_the_packed_corpus_chunks_are_the_parent_commits(probe, pins, tmp_path):
    for name, (make, switches) in chunk_cases().items():
        assert_pinned(name, make, switches, probe, pins, tmp_path)


def test_the_corpus_scenes_reach_the_product_split(probe, pins):
    """What the pins hold, so that they cannot go stale in silence: the whole-corpus scene is wide and splits nothing (its program
    table has the caller's programs alone); the chunks split products (programs are added); PYRITE_HIT_TAPE=0 takes a tape away from scenes that had one."""
    def scalars(name):
        return {line.split()[1]: line.split()[2] for line in pins[name] if line.startswith("scalar ")}

    whole = scalars("corpus")
    assert whole["program.wide"] == "1" and whole["dev.num_programs"] == whole["scene.caller_programs"] and int(whole["dev.num_programs"]) > 128 and whole["dev.hit_tape"] == "0"
    chunks = [scalars(n) for n in pins if n.startswith("corpus_chunk_") and not n.endswith("no_hit_tape")]
    assert all(c["program.wide"] == "0" for c in chunks)
    assert any(int(c["dev.num_programs"]) > int(c["scene.caller_programs"]) for c in chunks), "no chunk split a product"
    assert any(int(c["dev.tape_value_rows"]) > 8 for c in chunks), "no chunk needs more value rows than eight"
    assert scalars("corpus_chunk_6")["dev.hit_tape"] == "1" and scalars("corpus_chunk_6_no_hit_tape")["dev.hit_tape"] == "0"
    assert scalars("textures_example")["dev.product_records"] == "1" and scalars("textures_example_no_hit_tape")["dev.product_records"] == "0"
