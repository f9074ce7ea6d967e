"""Random ABI-level material programs (tests/program_gen.py) on the CPU: the independent evaluator (tests/program_restatement.py)
against the oracle's interpreter bit for bit, the full run against the memoised run, and the quotas that tests/test_gpu_program_forms.py
relies on -- how many programs of each family are physical enough to colour a surface. No device is needed.

The corpus, the tables its programs name and the filter are shared with the GPU tests, which import them from here."""
import ctypes as C
import functools

import numpy as np

import oracle
import program_restatement as R
from program_gen import Case, Gen, near_miss_names
from pyrite_amd import abi, build as gpu_build, scenes
from pyrite_amd.compiler import FlatScene
from pyrite_amd.project import rgb, spectrum, texture

f32 = np.float32
SEED = 20261018
NUM_SPECTRA = 3  # the generated programs read the first three spectra of the tables: arrays over [400, 700] with values in (0, 1)


# ------------------------------------------------------------------------------------------------ the tables and the probe grid
def tables_flat():
    """A FlatScene that holds what the generated programs name and nothing else yet: three array spectra, the colour textures
    (checker, rgba, a normal map read as linear colour), a mono texture and the RGB basis. Worlds are added on top of it, so every
    scene of these tests has the same tables in the same places."""
    flat = FlatScene()
    tex = scenes._generated_textures(seed=11, size=8)
    spectra = [spectrum(format="array", min=400.0, max=700.0, points=[0.1 * (k + 1), 0.5, 0.9 - 0.2 * k, 0.3]) for k in range(NUM_SPECTRA)]
    flat.compile(texture(tex["checker"]) * spectra[0] + texture(tex["rgba"]) * spectra[1] + texture(tex["mono"], "mono") * spectra[2] +
                 texture(tex["normal_map"], "linear") * 0.5 + rgb(0.2, 0.3, 0.4))
    assert flat.uses_rgb_basis and len(flat.spectra) == NUM_SPECTRA
    return flat


def texture_ids(flat):
    kinds = [t[0] for t in flat.textures]
    return [k for k, t in enumerate(kinds) if t == abi.TEXTURE_COLOR], [k for k, t in enumerate(kinds) if t == abi.TEXTURE_MONO]


def make_gen(wide=False, seed=SEED):
    colour, mono = texture_ids(tables_flat())
    return Gen(np.random.default_rng([seed, 1 if wide else 0]), NUM_SPECTRA, colour, mono, wide=wide, seed=seed)


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.sqrt((v * v).sum())).astype(f32)


WAVELENGTHS = [380.0, 431.0, 587.5, 745.0]  # below, inside (twice) and above the spectra's range
TEXTURES = [(0.2, 0.8), (0.65, 0.1), (0.0, 0.0), (1.37, -0.45)]  # the last outside the unit square
DIRECTIONS = [((0, 0, 1), (0, 0, -1)),  # normal incidence
              ((0, 0, 1), _unit((0.99995, 0.0, -0.01))),  # grazing
              (_unit((0.0, 0.6, 0.8)), _unit((0.0, 0.6, 0.8)))]  # the back side: the ray leaves along the normal


def probe_grid():
    """(wavelength [N], normal [N, 3], incident [N, 3], texture [N, 2]) over 4 x 4 x 3 probes."""
    rows = [(w, n, i, t) for w in WAVELENGTHS for t in TEXTURES for n, i in DIRECTIONS]
    return (np.array([r[0] for r in rows], f32), np.array([r[1] for r in rows], f32), np.array([r[2] for r in rows], f32), np.array([r[3] for r in rows], f32))


@functools.lru_cache(maxsize=None)
def tables():
    flat = tables_flat()
    return R.Tables(flat.desc())


@functools.lru_cache(maxsize=None)
def gpu_library():
    return abi.bind(C.CDLL(gpu_build.build()))


def allocate(case):
    """The case as pyr_program_allocate_registers leaves it (what pyr_scene_create runs)."""
    n = len(case.instrs)
    src, dst, out = (abi.PyrInstr * max(1, n))(*case.instrs), (abi.PyrInstr * max(1, n))(), abi.PyrProgram()
    assert gpu_library().pyr_program_allocate_registers(src, C.byref(case.p), dst, C.byref(out)) == abi.PYR_OK
    return Case(case.family, case.kind + "_after", list(dst)[:n], out, tape=case.tape, wide=case.wide)


def fits(p):
    return p.num_numbers <= abi.MAX_NUMBER_REGISTERS and p.num_vectors <= abi.MAX_VECTOR_REGISTERS and p.num_rgbs <= abi.MAX_RGB_REGISTERS


# ------------------------------------------------------------------------------------------------ the corpus
def draw_corpus(seed=SEED, scale=1):
    """Every family's programs for one seed, in a fixed order. `scale` multiplies the counts (a wider campaign)."""
    g, gw = make_gen(False, seed), make_gen(True, seed)
    n = lambda k: k * scale  # noqa: E731
    cases = []
    cases += [g.general("number") for _ in range(n(24))] + [g.general("vector") for _ in range(n(10))] + [gw.general("number") for _ in range(n(8))]
    cases += [g.general("number", close=True) for _ in range(n(44))]
    cases += [g.special(kind, hit=True) for kind in g.SPECIALS] + [g.hit_value(close=False) for _ in range(n(8))] + [g.hit_value() for _ in range(n(44))]
    cases += [g.special(kind) for kind in g.SPECIALS] + [g.lambda_(close=False) for _ in range(n(12))] + [g.lambda_() for _ in range(n(40))]
    cases += [g.fast(kind) for kind in g.FAST_KINDS for _ in range(n(5))]
    cases += [g.hit_rgb() for _ in range(n(70))]
    cases += [g.product(factors) for factors in (1, 2, 3) for _ in range(n(14))]
    cases += [g.near_miss(name) for name in near_miss_names() for _ in range(n(3))]
    over = [g.allocated(kind) for kind in g.ALLOCATED_KINDS for _ in range(n(10))]
    cases += over + [allocate(c) for c in over]
    cases += [g.normal_map() for _ in range(n(40))]
    cases += [g.wide_forcer() for _ in range(n(2))]
    return cases


def physical(case, values):
    """May the program colour a surface (or be a normal map)? Decided by the evaluator alone, over the probe grid: every value
    finite and a reflectance in [0, 1] -- which is also inside [0, 10], the range of an emissive, lamp or sky colour; a normal
    map's vector finite and on the surface's own side."""
    if not np.isfinite(values).all():
        return False
    if case.p.output_kind == abi.OUTPUT_VECTOR:
        return bool((values[:, 2] >= 0.05).all())
    return bool((values >= 0.0).all() and (values <= 1.0).all())


@functools.lru_cache(maxsize=None)
def corpus(seed=SEED, scale=1):
    """The corpus with every case's values on the probe grid (`case.values`), whether it may be rendered (`case.physical`) and
    whether it fits the in-register file once allocated (`case.fits`)."""
    cases = draw_corpus(seed, scale)
    grid = probe_grid()
    for case in cases:
        case.values = R.evaluate(tables(), case.instrs, case.p, *grid)
        case.physical = physical(case, case.values)
        case.fits = fits(case.p) or fits(allocate(case).p)
    return cases


def renderable(seed=SEED, scale=1):
    """family -> the cases a GPU scene may use as colours: physical, and running the build the family is about."""
    out = {}
    for case in corpus(seed, scale):
        if case.physical and (case.fits or case.wide):
            out.setdefault(case.family, []).append(case)
    return out


def append_programs(flat, cases):
    """Appends the cases' instructions and programs to a FlatScene (as tests/test_gpu_program_registers.py section 7 does);
    returns their program indices."""
    ids = []
    for case in cases:
        first = len(flat.instrs)
        for ins in case.instrs:
            flat.instrs.append(dict(op=ins.op, value_type=ins.value_type, operator=ins.operator_, deps=ins.deps, output=ins.output, a=ins.a, b=ins.b,
                                    x=(ins.x.kind, ins.x.bits), y=(ins.y.kind, ins.y.bits), z=(ins.z.kind, ins.z.bits), w=(ins.w.kind, ins.w.bits)))
        p = case.p
        flat.programs.append(dict(kind=p.kind, constant=p.constant, first=first, n=p.num_instrs, output_kind=p.output_kind, output_reg=p.output_reg,
                                  numbers=p.num_numbers, vectors=p.num_vectors, rgbs=p.num_rgbs))
        ids.append(len(flat.programs) - 1)
    return ids


class _World:
    def __init__(self, desc):
        self.desc = desc


# ------------------------------------------------------------------------------------------------ the tests
def test_the_evaluator_equals_the_oracle_bit_for_bit():
    """Every program of the corpus, every probe: the evaluator's bits are oracle_run_program's, NaN where it has NaN. Of a vector
    program the oracle's entry returns the x component alone, and no instruction carries a vector's component into a number: the
    evaluator's y, z and w (of Vector, RgbToVector, vector Binary and Mix) are compared with nothing here. They run the same
    component-wise code as x; on the GPU the vector programs are held through the oracle's shading normal within 1e-5
    (tests/test_gpu_program_forms.py), not bitwise."""
    cases = corpus()
    assert len(cases) >= 300 and {c.family for c in cases} == set(Gen.FAMILIES)
    flat = tables_flat()
    ids = append_programs(flat, cases)
    scene = oracle.OracleScene(_World(flat.desc()))
    wavelength, normal, incident, tex = probe_grid()
    assert len(wavelength) >= 48
    compared = special = 0
    for case, index in zip(cases, ids):
        got = np.array([scene.run_program(index, float(w), normal=[float(v) for v in n], incident=[float(v) for v in i], texture=[float(v) for v in t])[0]
                        for w, n, i, t in zip(wavelength, normal, incident, tex)], f32)
        want = case.values if case.p.output_kind == abi.OUTPUT_NUMBER else case.values[:, 0]
        same = R.same_bits(want, got)
        assert same.all(), "%s: probe %d: evaluator %r, oracle %r" % (case.name, int(np.argmin(same)), want[np.argmin(same)], got[np.argmin(same)])
        compared += len(got)
        special += int((~np.isfinite(got)).sum())
    scene.close()
    print("program forms cpu: %d programs, %d values compared bitwise, %d of them inf or NaN" % (len(cases), compared, special))
    assert special > 0, "no inf or NaN anywhere: Div by zero and its kin are not reached"


def test_full_run_equals_memoised_run():
    """The kernels re-run only the PYR_DEP_WAVELENGTH instructions for a path's further wavelengths, the reference those and the
    instructions without dependencies: every generated program, as declared and as allocated, gives the full run's bits either way."""
    wavelength, normal, incident, tex = probe_grid()
    # one probe per (texture, directions) pair, the four wavelengths in two orders as the columns of a memoised run
    first = np.arange(len(TEXTURES) * len(DIRECTIONS))
    per_wavelength = len(first)
    for order in ([0, 1, 2, 3], [2, 3, 0, 1]):
        columns = np.stack([wavelength[first + k * per_wavelength] for k in order], 1)
        for case in corpus():
            for version in ([case] if fits(case.p) else [case, allocate(case)]):
                full = np.stack([R.evaluate(tables(), version.instrs, version.p, columns[:, k], normal[first], incident[first], tex[first]) for k in range(4)], 1)
                for rerun_constants in (False, True):
                    memo = R.evaluate_memoised(tables(), version.instrs, version.p, columns, normal[first], incident[first], tex[first], rerun_constants)
                    assert R.same_bits(full, memo).all(), "%s: the memoised run (constants re-run: %s) differs from the full run" % (version.name, rerun_constants)
                if version is not case:
                    declared = np.stack([case.values[first + k * per_wavelength] for k in order], 1)
                    assert R.same_bits(full, declared).all(), "%s: the allocated program computes something else" % case.name


QUOTA = 24


def test_the_families_fill_their_quotas():
    """What tests/test_gpu_program_forms.py renders: at least 24 programs a family pass the filter (product: 8 for each of one, two
    and three factors; every near miss: 2; every fast kind: 3)."""
    r = renderable()
    lines = []
    for family in Gen.FAMILIES:
        generated = [c for c in corpus() if c.family == family]
        passed = r.get(family, [])
        lines.append("program forms quota %s: %d generated, %d pass" % (family, len(generated), len(passed)))
    print("\n".join(lines))
    closed_general = [c for c in r["general"] if c.kind == "number_closed"]
    assert len(closed_general) >= QUOTA, len(closed_general)
    for family in ("hit_value", "lambda", "fast", "hit_rgb", "allocated", "normal_map"):
        assert len(r.get(family, [])) >= QUOTA, (family, len(r.get(family, [])))
    for factors in "123":
        assert sum(c.kind == factors for c in r["product"]) >= 8, factors
    for name in near_miss_names():
        assert sum(c.kind == name for c in r["near_miss"]) >= 2, name
    for kind in Gen.FAST_KINDS:
        assert sum(c.kind == kind for c in r["fast"]) >= 3, kind
    assert any(c.wide for c in r["general"]), "no program that needs the wide build"
    # the families that claim a tape form fit the in-register file (a wide scene records no tape)
    for family in ("hit_value", "lambda", "fast", "hit_rgb", "product"):
        assert all(c.fits for c in r[family]), family


def test_the_families_are_what_they_claim():
    """The structural claims of the generator, checked on the instructions: dependencies are transitive and true; hit_value and
    normal_map read no wavelength; lambda is number-only without hit inputs; hit_rgb has exactly one dependent instruction, its
    last; every near miss is named after a condition of scene_pack.cpp."""
    hit = abi.DEP_NORMAL | abi.DEP_INCIDENT | abi.DEP_TEXTURE
    for case in corpus():
        deps_of = {"n": {}, "v": {}, "c": {}}
        for ins in case.instrs:
            reads, file = _reads(ins)
            want = {abi.OP_COLOR_TEXTURE: abi.DEP_TEXTURE, abi.OP_MONO_TEXTURE: abi.DEP_TEXTURE, abi.OP_FRESNEL: abi.DEP_NORMAL | abi.DEP_INCIDENT}.get(ins.op, 0)
            for f, r in reads:
                want |= abi.DEP_WAVELENGTH if f == "w" else deps_of[f][r]
            assert ins.deps == want, "%s: an instruction with op %d carries deps %#x, its operands give %#x" % (case.name, ins.op, ins.deps, want)
            deps_of[file][ins.output] = want
        all_deps = 0
        for ins in case.instrs:
            all_deps |= ins.deps
        if case.family in ("hit_value", "normal_map"):
            assert not all_deps & abi.DEP_WAVELENGTH, case.name
        if case.family == "lambda":
            assert not all_deps & hit and all_deps & abi.DEP_WAVELENGTH, case.name
            assert all(ins.op in (abi.OP_NUMBER, abi.OP_SPECTRUM, abi.OP_BLACKBODY, abi.OP_CLAMP) or
                       (ins.op in (abi.OP_BINARY, abi.OP_MIX) and ins.value_type == abi.VT_NUMBER) for ins in case.instrs), case.name
        if case.family == "hit_rgb":
            assert [bool(ins.deps & abi.DEP_WAVELENGTH) for ins in case.instrs] == [False] * (len(case.instrs) - 1) + [True], case.name
            assert case.instrs[-1].op == abi.OP_RGB_SPECTRUM and case.instrs[-1].output == case.p.output_reg
    lam = [c for c in corpus() if c.family == "lambda"]
    operators = {ins.operator_ for c in lam for ins in c.instrs if ins.op == abi.OP_BINARY}
    assert operators == {abi.BIN_ADD, abi.BIN_SUB, abi.BIN_MUL, abi.BIN_DIV}
    assert any(ins.op == abi.OP_SPECTRUM and ins.x.kind == abi.OPERAND_REGISTER for c in lam for ins in c.instrs)
    constant = lambda o: np.array([o.bits], np.uint32).view(f32)[0]  # noqa: E731
    assert any(ins.op == abi.OP_CLAMP and ins.y.kind == ins.z.kind == abi.OPERAND_CONSTANT and constant(ins.y) > constant(ins.z) for c in lam for ins in c.instrs)
    assert any(ins.op == abi.OP_MIX and ins.x.kind == abi.OPERAND_CONSTANT and not 0.0 <= constant(ins.x) <= 1.0 for c in lam for ins in c.instrs)


def _reads(ins):
    """([(file, register) | ("w", None)], output file) of an instruction, by the header's opcode table."""
    def operands(*names):
        out = []
        for name in names:
            o = getattr(ins, name)
            if o.kind == abi.OPERAND_REGISTER:
                out.append(("n", o.bits))
            elif o.kind == abi.OPERAND_INPUT:
                out.append(("w", None))
        return out

    typed = {abi.VT_NUMBER: "n", abi.VT_VECTOR: "v", abi.VT_RGB: "c"}
    op = ins.op
    if op == abi.OP_NUMBER:
        return [], "n"
    if op == abi.OP_VECTOR:
        return operands("x", "y", "z", "w"), "v"
    if op == abi.OP_RGB:
        return operands("x", "y", "z"), "c"
    if op == abi.OP_SPECTRUM:
        return operands("x"), "n"
    if op == abi.OP_COLOR_TEXTURE:
        return [], "c"
    if op == abi.OP_MONO_TEXTURE:
        return [], "n"
    if op == abi.OP_RGB_SPECTRUM:
        return operands("x") + [("c", ins.a)], "n"
    if op in (abi.OP_FRESNEL, abi.OP_BLACKBODY):
        return operands("x", "y"), "n"
    if op == abi.OP_RGB_TO_VECTOR:
        return [("c", ins.a)], "v"
    if op == abi.OP_CLAMP:
        return operands("x", "y", "z"), "n"
    f = typed[ins.value_type]
    return (operands("x") if op == abi.OP_MIX else []) + [(f, ins.a), (f, ins.b)], f
