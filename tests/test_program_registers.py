"""Register allocation of material programs that declare more registers than the interpreter's in-register file
(pyr_program_allocate_registers, the pass pyr_scene_create applies), on the CPU: the front ends accept such projects, the pass
keeps every value a run of the program -- full, or memoised as the kernels re-run it -- reads, the oracle agrees on the original and
the allocated descriptions, and the wide interpreter build keeps the resources DESIGN.md section 3.2 records."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from pyrite_amd import abi, build as gpu_build, lua_project, scenes
from pyrite_amd.compiler import FlatScene, ProjectError
from pyrite_amd.project import blackbody, material, renderer, rgb, shape, spectrum, texture, vector
from program_gen import Gen
from test_host_cpp import check_project_file, host  # noqa: F401 (fixture)

PROJECTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "projects")
REGISTERS = os.path.join(PROJECTS, "registers.lua")
WL = abi.DEP_WAVELENGTH


@pytest.fixture(scope="module")
def lib():
    return abi.bind(C.CDLL(gpu_build.build()))


def allocate(lib, instrs, program):
    """pyr_program_allocate_registers on one program; `instrs` indexed like PyrSceneDesc::instrs."""
    n = len(instrs)
    src = (abi.PyrInstr * max(1, n))(*instrs)
    dst = (abi.PyrInstr * max(1, n))()
    out = abi.PyrProgram()
    assert lib.pyr_program_allocate_registers(src, C.byref(program), dst, C.byref(out)) == abi.PYR_OK
    return list(dst)[:n], out


def raw(x):
    return bytes(x)


def allocated_desc(lib, desc):
    """A copy of `desc` whose programs went through the pass (the arrays are kept alive on the returned object)."""
    instrs = (abi.PyrInstr * max(1, desc.num_instrs))(*[desc.instrs[k] for k in range(desc.num_instrs)])
    progs = (abi.PyrProgram * desc.num_programs)()
    for i in range(desc.num_programs):
        out = abi.PyrProgram()
        assert lib.pyr_program_allocate_registers(instrs, C.byref(desc.programs[i]), instrs, C.byref(out)) == abi.PYR_OK
        progs[i] = out
    d = abi.PyrSceneDesc.from_buffer_copy(desc)
    d.instrs, d.programs = instrs, progs
    d._keep = (instrs, progs)
    return d


class _World:
    def __init__(self, desc):
        self.desc = desc


def registers_project():
    project, base_dir = lua_project.load_project(REGISTERS)
    return project, FlatScene().add_world(project["world"], base_dir)


# ------------------------------------------------------------------------------------------------ 1. the front ends accept them
def test_over_declared_projects_load_in_both_front_ends(host, tmp_path):  # noqa: F811
    _, flat = registers_project()
    over = [p for p in flat.programs if p["kind"] == abi.PROGRAM_INSTRUCTIONS and
            (p["numbers"] > abi.MAX_NUMBER_REGISTERS or p["vectors"] > abi.MAX_VECTOR_REGISTERS or p["rgbs"] > abi.MAX_RGB_REGISTERS)]
    assert any(p["rgbs"] == 11 for p in over), "the three-colour blend declares 11 RGB registers"
    assert any(p["numbers"] > abi.MAX_NUMBER_REGISTERS for p in over), "the nested mix passes 16 number registers"
    assert any(p["vectors"] > abi.MAX_VECTOR_REGISTERS for p in over), "the normal map passes 8 vector registers"
    check_project_file(host, REGISTERS, tmp_path)


def test_the_front_ends_keep_a_sanity_bound():
    flat = FlatScene()
    e = rgb(0.5, 0.5, 0.5)
    for k in range(40):
        e = e * (0.5 + k * 1e-3)
    flat.compile(e)  # 80 RGB registers: accepted by the front end (pyr_scene_create decides)
    import pyrite_amd.compiler as compiler

    bound, compiler.PROGRAM_REGISTER_BOUND = compiler.PROGRAM_REGISTER_BOUND, 64
    try:
        with pytest.raises(ProjectError):
            FlatScene().compile(e)
    finally:
        compiler.PROGRAM_REGISTER_BOUND = bound


# ------------------------------------------------------------------------------------------------ 2. the pass on random programs
def memoised_runs(instrs, p, wavelengths, texture=(0.3, 0.7)):
    """A small interpreter with the kernels' memoised re-run: a full run at wavelengths[0], then only the PYR_DEP_WAVELENGTH
    instructions at each further wavelength; the register files persist (filled with a marker first). Returns the outputs' bits."""
    f = np.float32
    num = [f(np.nan)] * max(1, p.num_numbers)
    vec = [np.full(4, np.float32(-7.25))] * max(1, p.num_vectors)
    col = [np.full(4, np.float32(-9.5))] * max(1, p.num_rgbs)
    normal, incident = np.array([0.0, 0.8, 0.6, 0], f), np.array([0.6, -0.8, 0.0, 0], f)

    def value(o, wl):
        if o.kind == abi.OPERAND_CONSTANT:
            return np.array([o.bits], np.uint32).view(f)[0]
        if o.kind == abi.OPERAND_INPUT:
            return f(wl)
        return num[o.bits]

    def files(vt):
        return num if vt == abi.VT_NUMBER else (vec if vt == abi.VT_VECTOR else col)

    def binop(op, a, b):
        with np.errstate(all="ignore"):
            return [a + b, a - b, a * b, a / b][op]

    outs = []
    for pass_, wl in enumerate(wavelengths):
        for ins in instrs:
            if pass_ > 0 and not (ins.deps & WL):
                continue
            o, op = ins.output, ins.op
            with np.errstate(all="ignore"):
                if op == abi.OP_NUMBER:
                    num[o] = np.array([ins.x.bits], np.uint32).view(f)[0]
                elif op == abi.OP_VECTOR:
                    vec[o] = np.array([value(ins.x, wl), value(ins.y, wl), value(ins.z, wl), value(ins.w, wl)], f)
                elif op == abi.OP_RGB:
                    col[o] = np.array([value(ins.x, wl), value(ins.y, wl), value(ins.z, wl), 1.0], f)
                elif op == abi.OP_SPECTRUM:
                    num[o] = f(np.sin(f(value(ins.x, wl)) * f(0.01) + f(ins.a)))
                elif op == abi.OP_COLOR_TEXTURE:
                    col[o] = np.array([texture[0] + ins.a, texture[1], texture[0] * texture[1], 1.0], f)
                elif op == abi.OP_MONO_TEXTURE:
                    num[o] = f(texture[0] * f(ins.a + 1))
                elif op == abi.OP_RGB_SPECTRUM:
                    w = f(value(ins.x, wl))
                    c = col[ins.a]
                    num[o] = f(c[0] * f(w * f(1e-3)) + c[1] * f(0.5) + c[2] * f(w * f(2e-3)))
                elif op == abi.OP_FRESNEL:
                    num[o] = f(value(ins.x, wl) * normal[1] - value(ins.y, wl) * incident[0])
                elif op == abi.OP_BLACKBODY:
                    num[o] = f(value(ins.x, wl) * f(1e-3) + value(ins.y, wl) * f(1e-4))
                elif op == abi.OP_RGB_TO_VECTOR:
                    vec[o] = (col[ins.a] * f(2.0) - f(1.0)).astype(f)
                elif op == abi.OP_MIX:
                    amount = f(min(max(value(ins.x, wl), f(0.0)), f(1.0)))
                    F = files(ins.value_type)
                    F[o] = (F[ins.a] * (f(1.0) - amount) + F[ins.b] * amount) if ins.value_type == abi.VT_NUMBER else (F[ins.a] + (F[ins.b] - F[ins.a]) * amount).astype(f)
                elif op == abi.OP_BINARY:
                    F = files(ins.value_type)
                    F[o] = f(binop(ins.operator_, F[ins.a], F[ins.b])) if ins.value_type == abi.VT_NUMBER else binop(ins.operator_, F[ins.a], F[ins.b]).astype(f)
                elif op == abi.OP_CLAMP:
                    v, lo, hi = value(ins.x, wl), value(ins.y, wl), value(ins.z, wl)
                    num[o] = f(max(min(v, hi), lo)) if not (np.isnan(v) or np.isnan(lo) or np.isnan(hi)) else f(np.nan)
        r = num[p.output_reg] if p.output_kind == abi.OUTPUT_NUMBER else vec[p.output_reg]
        outs.append(np.array(r, f).tobytes())
    return outs


def operand_shape(ins):
    """Everything of an instruction but register indices."""
    keep = [ins.op, ins.value_type, ins.operator_, ins.deps, ins.reserved]
    for name in "xyzw":
        o = getattr(ins, name)
        keep += [o.kind, None if o.kind == abi.OPERAND_REGISTER and ins.op != abi.OP_NUMBER else o.bits]
    if ins.op in (abi.OP_SPECTRUM, abi.OP_COLOR_TEXTURE, abi.OP_MONO_TEXTURE, abi.OP_FRESNEL):
        keep += [ins.a, ins.b]
    return keep


def fits(p):
    return p.num_numbers <= abi.MAX_NUMBER_REGISTERS and p.num_vectors <= abi.MAX_VECTOR_REGISTERS and p.num_rgbs <= abi.MAX_RGB_REGISTERS


def test_the_pass_on_random_programs(lib):
    rng = np.random.default_rng(20261016)
    gen = Gen(rng, num_spectra=3, colour_textures=[0, 1], mono_textures=[2])
    over = unchanged = 0
    for case in range(3000):
        output = "vector" if case % 5 == 4 else "number"
        instrs, p = gen.program(allow_wavelength=output == "number", output=output)
        got, q = allocate(lib, instrs, p)
        again, q2 = allocate(lib, instrs, p)
        assert [raw(i) for i in got] == [raw(i) for i in again] and raw(q) == raw(q2), "not deterministic"
        if fits(p):
            unchanged += 1
            assert [raw(i) for i in got] == [raw(i) for i in instrs] and raw(q) == raw(p), "a program that fits was changed"
            continue
        over += 1
        assert [operand_shape(i) for i in got] == [operand_shape(i) for i in instrs]
        assert (q.kind, q.first_instr, q.num_instrs, q.output_kind, raw(C.c_float(q.constant))) == (p.kind, p.first_instr, p.num_instrs, p.output_kind, raw(C.c_float(p.constant)))
        assert q.num_numbers <= p.num_numbers and q.num_vectors <= p.num_vectors and q.num_rgbs <= p.num_rgbs
        wls = [412.5, 533.0, 611.25, 702.0] if output == "number" else [500.0]
        assert memoised_runs(got, q, wls) == memoised_runs(instrs, p, wls), "case %d: the allocated program computes something else" % case
    assert over > 1000 and unchanged > 100, (over, unchanged)


def test_the_pass_leaves_what_it_cannot_follow(lib):
    """A register written twice, or read before any write: copied unchanged (and so judged by its declared counts)."""
    ins = [abi.PyrInstr(op=abi.OP_NUMBER, output=k, x=abi.PyrOperand(abi.OPERAND_CONSTANT, 0x3F800000)) for k in range(20)]
    ins.append(abi.PyrInstr(op=abi.OP_BINARY, value_type=abi.VT_NUMBER, operator_=abi.BIN_ADD, a=3, b=4, output=3))  # a second write of 3
    p = abi.PyrProgram(abi.PROGRAM_INSTRUCTIONS, 0.0, 0, len(ins), abi.OUTPUT_NUMBER, 3, 20, 0, 0)
    got, q = allocate(lib, ins, p)
    assert [raw(i) for i in got] == [raw(i) for i in ins] and raw(q) == raw(p)
    ins[-1].output = 19
    ins[-2].op = abi.OP_CLAMP  # reads registers through constants only: still single assignment
    got, q = allocate(lib, ins, abi.PyrProgram(abi.PROGRAM_INSTRUCTIONS, 0.0, 0, len(ins) - 1, abi.OUTPUT_NUMBER, 18, 20, 0, 0))
    assert q.num_numbers == 2 and q.output_reg == 0  # the output keeps register 0 (it does not depend on the wavelength); 19 dead values share 1


def test_pinned_values_survive_the_rerun(lib):
    """A texture value read by a wavelength-dependent product keeps its register although it is dead in a single run."""
    instrs = []

    def mk(**kw):
        i = abi.PyrInstr()
        for k, v in kw.items():
            setattr(i, k, v)
        instrs.append(i)

    wl = abi.PyrOperand(abi.OPERAND_INPUT, abi.INPUT_WAVELENGTH)
    for k in range(10):  # ten colour textures, each times a spectrum, summed: ten RGB values live through every companion pass
        mk(op=abi.OP_COLOR_TEXTURE, a=0, b=abi.INPUT_TEXTURE, deps=abi.DEP_TEXTURE, output=k)
    for k in range(10):
        mk(op=abi.OP_SPECTRUM, x=wl, a=0, deps=WL, output=2 * k)
        mk(op=abi.OP_RGB_SPECTRUM, x=wl, a=k, deps=WL | abi.DEP_TEXTURE, output=2 * k + 1)
    acc = 20
    mk(op=abi.OP_BINARY, value_type=abi.VT_NUMBER, operator_=abi.BIN_MUL, a=0, b=1, deps=WL | abi.DEP_TEXTURE, output=acc)
    for k in range(1, 10):
        mk(op=abi.OP_BINARY, value_type=abi.VT_NUMBER, operator_=abi.BIN_MUL, a=2 * k, b=2 * k + 1, deps=WL | abi.DEP_TEXTURE, output=acc + 1)
        mk(op=abi.OP_BINARY, value_type=abi.VT_NUMBER, operator_=abi.BIN_ADD, a=acc, b=acc + 1, deps=WL | abi.DEP_TEXTURE, output=acc + 2)
        acc += 2
    p = abi.PyrProgram(abi.PROGRAM_INSTRUCTIONS, 0.0, 0, len(instrs), abi.OUTPUT_NUMBER, acc, acc + 1, 0, 10)
    got, q = allocate(lib, instrs, p)
    assert q.num_rgbs == 10, "every texture value is read by a wavelength-dependent instruction: none may share a register"
    assert q.num_numbers < p.num_numbers
    wls = [420.0, 480.0, 560.0, 680.0]
    assert memoised_runs(got, q, wls) == memoised_runs(instrs, p, wls)


def oracle_base():
    """A small scene whose tables hold what the random programs name: three spectra, two colour textures and a mono one, the RGB basis."""
    tex = scenes._generated_textures(seed=11, size=8)
    spectra = [spectrum(format="array", min=400.0, max=700.0, points=[0.1 * (k + 1), 0.5, 0.9 - 0.2 * k, 0.3]) for k in range(3)]
    world = {"objects": [
        shape.sphere(position=vector(0, 0, 0), radius=1.0, material={"surface": material.diffuse(
            color=texture(tex["checker"]) * spectra[0] + texture(tex["rgba"]) * spectra[1] + texture(tex["mono"], "mono") * spectra[2] + rgb(0.2, 0.3, 0.4))}),
        shape.sphere(position=vector(0, 3, 0), radius=0.5, material={"surface": material.emissive(color=blackbody(4000) * 1e-12)}),
    ]}
    flat = FlatScene().add_world(world)
    kinds = [t[0] for t in flat.textures]
    return flat, [k for k, t in enumerate(kinds) if t == abi.TEXTURE_COLOR], [k for k, t in enumerate(kinds) if t == abi.TEXTURE_MONO]


def test_the_oracle_agrees_on_both_descriptions(lib):
    flat, colour, mono = oracle_base()
    base = flat.desc()
    assert base.num_spectra >= 3 and colour and mono and base.rgb_basis
    rng = np.random.default_rng(77)
    gen = Gen(rng, base.num_spectra, colour, mono)
    programs, originals, allocated = [], [], []
    while len(programs) < 150:
        instrs, p = gen.program()
        if fits(p):
            continue
        programs.append((instrs, p))
    for which in ("original", "allocated"):
        all_instrs = [base.instrs[k] for k in range(base.num_instrs)]
        all_progs = [base.programs[k] for k in range(base.num_programs)]
        for instrs, p in programs:
            if which == "allocated":
                instrs, p = allocate(lib, instrs, p)
            p = abi.PyrProgram.from_buffer_copy(p)
            p.first_instr = len(all_instrs)
            all_instrs += instrs
            all_progs.append(p)
        d = abi.PyrSceneDesc.from_buffer_copy(base)
        I, P = (abi.PyrInstr * len(all_instrs))(*all_instrs), (abi.PyrProgram * len(all_progs))(*all_progs)
        d.instrs, d.num_instrs, d.programs, d.num_programs = I, len(all_instrs), P, len(all_progs)
        scene = oracle.OracleScene(_World(d))
        values = []
        for k in range(len(programs)):
            for wl, tex in ((431.0, (0.2, 0.8)), (587.5, (0.65, 0.1))):
                values.append(scene.run_program(base.num_programs + k, wl, normal=(0, 0.8, 0.6), incident=(0.6, -0.8, 0), texture=tex)[0])
        (originals if which == "original" else allocated).extend(values)
        scene.close()
    assert np.array_equal(np.array(originals, np.float32).view(np.uint32), np.array(allocated, np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. oracle films
def test_oracle_films_match_for_the_allocated_description(lib):
    project, flat = registers_project()
    desc = flat.desc()
    d2 = allocated_desc(lib, desc)
    changed = sum(raw(desc.programs[i]) != raw(d2.programs[i]) for i in range(desc.num_programs))
    assert changed >= 3
    r = renderer.simple(pixel_samples=2, spectrum_samples=6, bounces=4, light_samples=1, tile_size=16)
    _, cam, rend, _ = scenes.build(dict(project, image={"width": 32, "height": 24}, renderer=r), base_dir=PROJECTS)
    films = []
    for d in (desc, d2):
        f = rend.new_film(32, 24)
        oracle.OracleScene(_World(d)).render(rend, cam, f, threads=4)
        films.append(f.grains.copy())
    assert films[0][..., 1].sum() > 0
    assert np.array_equal(films[0].view(np.uint32), films[1].view(np.uint32))


# ------------------------------------------------------------------------------------------------ the scene-level refusal (no device needed)
def test_too_large_even_for_the_wide_file_is_refused_before_anything_runs(lib):
    """65 number values all read by the last instruction: 65 live at once, more than PYR_WIDE_NUMBER_REGISTERS. pyr_scene_create
    refuses the scene with PYR_ERR_UNSUPPORTED and the counts it needs, before it looks for a device."""
    flat = FlatScene()
    world = {"objects": [shape.sphere(position=vector(0, 0, 0), radius=1.0, material={"surface": material.diffuse(color=0.5)})]}
    flat.add_world(world)
    instrs = [dict(op=abi.OP_NUMBER, value_type=0, operator=0, deps=0, output=k, a=0, b=0,
                   x=(abi.OPERAND_CONSTANT, int(np.float32(0.01 * (k + 1)).view(np.uint32))), y=None, z=None, w=None) for k in range(65)]
    # a clamp chain that reads every constant only at the end would need 65 live values; a binary sum tree reads them late too
    regs, nxt = list(range(65)), 65
    while len(regs) > 1:
        a, b = regs.pop(), regs.pop()
        instrs.append(dict(op=abi.OP_BINARY, value_type=abi.VT_NUMBER, operator=abi.BIN_ADD, deps=0, output=nxt, a=a, b=b, x=None, y=None, z=None, w=None))
        regs.insert(0, nxt)
        nxt += 1
    first = len(flat.instrs)
    flat.instrs.extend(instrs)
    flat.programs.append(dict(kind=abi.PROGRAM_INSTRUCTIONS, constant=0.0, first=first, n=len(instrs), output_kind=abi.OUTPUT_NUMBER, output_reg=regs[0],
                              numbers=nxt, vectors=0, rgbs=0))
    flat.components[0]["color"] = len(flat.programs) - 1
    desc = flat.desc()
    handle = C.c_void_p()
    rc = lib.pyr_scene_create(C.byref(desc), 0, C.byref(handle))
    assert rc == abi.PYR_ERR_UNSUPPORTED, (rc, lib.pyr_last_error())
    assert b"number" in lib.pyr_last_error() and b"64" in lib.pyr_last_error()


def test_program_info_layout_matches_the_header(tmp_path):
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pyrite_gpu.h")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "%s"' % header, "int main(void){", 'printf("%zu\\n", sizeof(PyrProgramInfo));']
    lines += ['printf("%%zu\\n", offsetof(PyrProgramInfo, %s));' % f for f, _ in abi.PyrProgramInfo._fields_]
    lines += ['printf("%d %d %d\\n", PYR_WIDE_NUMBER_REGISTERS, PYR_WIDE_VECTOR_REGISTERS, PYR_WIDE_RGB_REGISTERS);', "return 0;}"]
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    assert int(out[0]) == C.sizeof(abi.PyrProgramInfo)
    assert [int(x) for x in out[1:1 + len(abi.PyrProgramInfo._fields_)]] == [getattr(abi.PyrProgramInfo, f).offset for f, _ in abi.PyrProgramInfo._fields_]
    assert out[1 + len(abi.PyrProgramInfo._fields_)].split() == [str(abi.WIDE_NUMBER_REGISTERS), str(abi.WIDE_VECTOR_REGISTERS), str(abi.WIDE_RGB_REGISTERS)]


def sum_chain_scene(values, programs_on_the_range=1):
    """A sphere whose diffuse colour is a sum chain over `values` constants (2 values live at a time, `values` declared), named by
    `programs_on_the_range` programs that share ONE instruction range (the first colours the sphere, the others the sky and so on)."""
    flat = FlatScene()
    flat.add_world({"objects": [shape.sphere(position=vector(0, 0, 0), radius=1.0, material={"surface": material.diffuse(color=0.5)})], "sky": 0.25})
    instrs = [dict(op=abi.OP_NUMBER, value_type=0, operator=0, deps=0, output=0, a=0, b=0, x=(abi.OPERAND_CONSTANT, int(np.float32(0.01).view(np.uint32))),
                   y=None, z=None, w=None)]
    for k in range(1, values):
        instrs.append(dict(op=abi.OP_NUMBER, value_type=0, operator=0, deps=0, output=2 * k - 1, a=0, b=0,
                           x=(abi.OPERAND_CONSTANT, int(np.float32(0.01 * (k + 1)).view(np.uint32))), y=None, z=None, w=None))
        instrs.append(dict(op=abi.OP_BINARY, value_type=abi.VT_NUMBER, operator=abi.BIN_ADD, deps=0, output=2 * k, a=2 * k - 2, b=2 * k - 1, x=None, y=None, z=None, w=None))
    first = len(flat.instrs)
    flat.instrs.extend(instrs)
    ids = []
    for _ in range(programs_on_the_range):
        flat.programs.append(dict(kind=abi.PROGRAM_INSTRUCTIONS, constant=0.0, first=first, n=len(instrs), output_kind=abi.OUTPUT_NUMBER, output_reg=2 * values - 2,
                                  numbers=2 * values - 1, vectors=0, rgbs=0))
        ids.append(len(flat.programs) - 1)
    flat.components[0]["color"] = ids[0]
    if len(ids) > 1:
        flat.sky_program = ids[1]
    return flat, ids


def create_status(lib, desc):
    """pyr_scene_create's status (the scene, where a device made one, is destroyed again) and pyr_last_error()."""
    handle = C.c_void_p()
    rc = lib.pyr_scene_create(C.byref(desc), 0, C.byref(handle))
    message = lib.pyr_last_error()
    if rc == abi.PYR_OK:
        lib.pyr_scene_destroy(handle)
    return rc, message


def test_programs_sharing_one_range_are_each_allocated_from_the_original(lib):
    """Two programs name one instruction range of 141 number values (more than the wide file declared, three live). Each must be allocated
    from the caller's instructions: had the second read the first's renumbered copy, it would see a register written twice, stay as
    declared and be refused. Neither is: the scene is refused for no register reason (without a device: PYR_ERR_DEVICE)."""
    flat, ids = sum_chain_scene(71, programs_on_the_range=2)
    desc = flat.desc()
    assert desc.programs[ids[0]].first_instr == desc.programs[ids[1]].first_instr and desc.sky_program == ids[1]
    rc, message = create_status(lib, desc)
    assert rc in (abi.PYR_OK, abi.PYR_ERR_DEVICE), (rc, message)
    # the pass itself, on the shared range: the same result both times, and the caller's instructions untouched
    before = [raw(desc.instrs[k]) for k in range(desc.num_instrs)]
    results = [allocate(lib, [desc.instrs[k] for k in range(desc.num_instrs)], desc.programs[i]) for i in ids]
    assert [raw(i) for i in results[0][0]] == [raw(i) for i in results[1][0]] and raw(results[0][1]) == raw(results[1][1])
    assert results[0][1].num_numbers == 3 and [raw(desc.instrs[k]) for k in range(desc.num_instrs)] == before


def test_absurd_declared_counts_are_refused_not_allocated(lib):
    """A program declaring 0xF0000000 numbers: PYR_ERR_UNSUPPORTED from the pass and from pyr_scene_create, no attempt to size tables by it."""
    flat, ids = sum_chain_scene(20)
    flat.programs[ids[0]]["numbers"] = 0xF0000000
    desc = flat.desc()
    out = abi.PyrProgram()
    instrs = (abi.PyrInstr * desc.num_instrs)(*[desc.instrs[k] for k in range(desc.num_instrs)])
    assert lib.pyr_program_allocate_registers(instrs, C.byref(desc.programs[ids[0]]), instrs, C.byref(out)) == abi.PYR_ERR_UNSUPPORTED
    rc, message = create_status(lib, desc)
    assert rc == abi.PYR_ERR_UNSUPPORTED and b"65536" in message, (rc, message)
    flat.programs[ids[0]]["numbers"] = abi.MAX_DECLARED_REGISTERS  # at the bound: allocated (to 3 registers: the output keeps one of its own)
    rc, message = create_status(lib, flat.desc())
    assert rc in (abi.PYR_OK, abi.PYR_ERR_DEVICE), (rc, message)


def test_both_front_ends_and_the_header_share_one_bound(tmp_path):
    """compiler.py's bound is abi.MAX_DECLARED_REGISTERS, which must be the header's PYR_MAX_DECLARED_REGISTERS; pyrite_host.cpp tests its
    counts against that macro."""
    import pyrite_amd.compiler as compiler

    assert compiler.PROGRAM_REGISTER_BOUND == abi.MAX_DECLARED_REGISTERS == 65536
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pyrite_gpu.h")
    src, exe = tmp_path / "b.c", tmp_path / "b"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(void){printf("%%d\\n", PYR_MAX_DECLARED_REGISTERS);return 0;}\n' % header)
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    assert int(subprocess.check_output([str(exe)])) == abi.MAX_DECLARED_REGISTERS
    cpp = open(os.path.join(gpu_build.HOST_DIR, "pyrite_host.cpp")).read()
    bound = re.search(r"constexpr uint32_t kProgramRegisterBound = (\w+);", cpp)
    assert bound and bound.group(1) == "PYR_MAX_DECLARED_REGISTERS"
    assert "counts[RN] > kProgramRegisterBound || counts[RV] > kProgramRegisterBound || counts[RC] > kProgramRegisterBound" in cpp


# ------------------------------------------------------------------------------------------------ 4. the wide build's resources
# DESIGN.md section 3.2 records them: every wide kernel at 168 VGPRs (the interpreter builds' own count) and so 3 waves per SIMD (sm_waves), its
# scratch 960 B above the matching in-register build (the files: 64 x 4 + 32 x 16 + 32 x 16 = 1,280 B against 16 x 4 + 8 x 16 + 8 x 16 = 320 B).
WIDE_VGPRS, WIDE_WAVES = 168, 3
WIDE_SCRATCH = {  # render_kernel_sm<COUNT, true, LDS_SCENE, LDS_TABLES>: bytes of scratch per lane
    (False, True, False): 1432, (False, False, True): 1680, (False, False, False): 1696,
    (True, True, False): 1488, (True, False, True): 1744, (True, False, False): 1760,
}


@pytest.mark.timeout(900)
def test_the_wide_build_keeps_its_resources(tmp_path):
    flags = [f for f in gpu_build.FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / "wide.s"
    subprocess.check_call([gpu_build.HIPCC] + flags + ["--cuda-device-only", "-S", "kernels/wide.hip", "-o", str(out)], cwd=gpu_build.CSRC,
                          stderr=subprocess.DEVNULL)
    text = out.read_text()
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    assert len(kernels) == 6 and all(k.startswith("_ZN3pyr4wide16render_kernel_sm") for k in kernels), kernels
    found = {}
    for name in kernels:
        args = re.match(r"_ZN3pyr4wide16render_kernel_smILb([01])ELb1ELb([01])ELb([01])ELb0ELb0EE", name)
        assert args, name
        meta = text[text.index(".amdhsa_kernel " + name):]
        meta = meta[:meta.index(".end_amdhsa_kernel")]
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1))
        found[tuple(a == "1" for a in args.groups())] = (vgprs, min(8, 512 // (((vgprs + 7) // 8) * 8)), scratch)  # launch_render's residency rule
    assert found == {key: (WIDE_VGPRS, WIDE_WAVES, scratch) for key, scratch in WIDE_SCRATCH.items()}
