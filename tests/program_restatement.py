"""A numpy restatement of ExecutionContext::run (program/execution_context.rs:69-283) over the flattened programs of
include/pyrite_gpu.h: the independent evaluator the program-form tests hold the oracle and the GPU interpreters against. Test
infrastructure only. Written from the header's opcode table and execution_context.rs, not from kernels.hip or oracle.cpp.

Every arithmetic step is one f32 operation: the operands are widened to float64, combined, and rounded once to float32 (for + - * /
of two f32 operands that is the correctly rounded f32 result), so what comes out is a bit pattern, not a value with a tolerance. The
leaf functions -- spectrum lookup, texture lookup, fresnel, blackbody -- are the oracle's single-function entries, which have
known-answer tests of their own (tests/test_oracle_kat.py, tests/test_textures.py); the RGB basis lookup of RgbSpectrumValue is
restated here (execution_context.rs:140-152 over spectra.rs:32-55).

All inputs are arrays over N probes; register files are arrays [N] (numbers) and [N, 4] (vectors, RGB with alpha last)."""
import ctypes as C

import numpy as np

import oracle
from pyrite_amd import abi

f32, f64 = np.float32, np.float64
WL = abi.DEP_WAVELENGTH


def _op(operator, a, b):
    a, b = np.asarray(a, f32).astype(f64), np.asarray(b, f32).astype(f64)
    with np.errstate(all="ignore"):
        if operator == abi.BIN_ADD:
            return (a + b).astype(f32)
        if operator == abi.BIN_SUB:
            return (a - b).astype(f32)
        if operator == abi.BIN_MUL:
            return (a * b).astype(f32)
        return (a / b).astype(f32)


def add(a, b):
    return _op(abi.BIN_ADD, a, b)


def sub(a, b):
    return _op(abi.BIN_SUB, a, b)


def mul(a, b):
    return _op(abi.BIN_MUL, a, b)


def div(a, b):
    return _op(abi.BIN_DIV, a, b)


def rust_min(a, b):
    """f32::min: the other operand when one is NaN."""
    return np.fmin(np.asarray(a, f32), np.asarray(b, f32)).astype(f32)


def rust_max(a, b):
    return np.fmax(np.asarray(a, f32), np.asarray(b, f32)).astype(f32)


def same_bits(a, b):
    """Elementwise: equal bit patterns, or NaN on both sides."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


class Tables:
    """What the programs of a PyrSceneDesc name: spectra, textures, the RGB basis (copied out of the description)."""

    def __init__(self, desc):
        data = np.array(np.ctypeslib.as_array(desc.spectrum_data, (max(1, desc.num_spectrum_floats),)), f32) if desc.num_spectrum_floats else np.zeros(1, f32)
        self.spectra = []
        for k in range(desc.num_spectra):
            s = desc.spectra[k]
            floats = s.count * (2 if s.format == abi.SPECTRUM_CURVE else 1)
            self.spectra.append((s.format, s.min, s.max, np.ascontiguousarray(data[s.offset:s.offset + floats]), s.count))
        self.textures = []
        if desc.num_textures:
            texels = np.array(np.ctypeslib.as_array(desc.texture_data, (desc.num_texture_floats,)), f32)
            for k in range(desc.num_textures):
                t = desc.textures[k]
                channels = 4 if t.format == abi.TEXTURE_COLOR else 1
                self.textures.append((channels, t.width, t.height, np.ascontiguousarray(texels[t.offset:t.offset + t.width * t.height * channels])))
        self.rgb_basis = None
        if desc.rgb_basis and desc.rgb_basis_count:
            self.rgb_basis = np.array(np.ctypeslib.as_array(desc.rgb_basis, (3 * desc.rgb_basis_count,)), f32).reshape(-1, 3)
            self.rgb_min, self.rgb_max = f32(desc.rgb_basis_min), f32(desc.rgb_basis_max)

    # ---- leaves: the oracle's single-function entries, once per distinct argument
    def spectrum(self, index, wavelength):
        fmt, mn, mx, data, count = self.spectra[index]
        L = oracle.lib()
        values, inverse = np.unique(np.asarray(wavelength, f32).view(np.uint32), return_inverse=True)
        out = np.array([L.oracle_spectrum_get(fmt, mn, mx, data.ctypes.data, count, float(v)) for v in values.view(f32)], f32)
        return out[inverse]

    def blackbody(self, wavelength, temperature):
        L = oracle.lib()
        pairs = np.stack([np.asarray(wavelength, f32), np.asarray(temperature, f32)], -1)
        values, inverse = np.unique(pairs.view(np.uint32), axis=0, return_inverse=True)
        out = np.array([L.oracle_blackbody(float(w), float(t)) for w, t in values.view(f32)], f32)
        return out[np.asarray(inverse).reshape(-1)]

    def texture(self, index, coordinates):
        channels, width, height, texels = self.textures[index]
        L = oracle.lib()
        values, inverse = np.unique(np.ascontiguousarray(coordinates, f32).view(np.uint32), axis=0, return_inverse=True)
        out = np.zeros((len(values), channels), f32)
        for k, (x, y) in enumerate(values.view(f32)):
            L.oracle_texture_get(channels, width, height, texels.ctypes.data, float(x), float(y), out[k].ctypes.data)
        return out[np.asarray(inverse).reshape(-1)]

    def fresnel(self, ior, env_ior, normal, incident):
        L = oracle.lib()
        return np.array([L.oracle_fresnel(float(a), float(b), oracle.F3(*[float(v) for v in n]), oracle.F3(*[float(v) for v in i]))
                         for a, b, n, i in zip(ior, env_ior, normal, incident)], f32)

    def rgb_response(self, wavelength):
        """crate::rgb::response::RGB.get(wavelength): Spectrum::Array<LinSrgb>::get (spectra.rs:32-55), [N, 3]."""
        d, mn, mx = self.rgb_basis, self.rgb_min, self.rgb_max
        w = np.asarray(wavelength, f32)
        count = len(d)
        normalized = div(sub(w, mn), sub(mx, mn))
        float_index = mul(normalized, sub(f32(count), f32(1.0)))
        with np.errstate(all="ignore"):
            low = np.trunc(float_index).astype(f32)
        inside = (w > mn) & (w < mx)
        i0 = np.where(inside, low, 0).astype(np.int64).clip(0, count - 2)
        mix = sub(float_index, low)
        value = add(mul(d[i0], sub(f32(1.0), mix)[:, None]), mul(d[i0 + 1], mix[:, None]))
        value = np.where((w <= mn)[:, None], d[0][None, :], value)
        value = np.where((w >= mx)[:, None], d[-1][None, :], value)
        return value.astype(f32)


class Machine:
    """The register files of one ExecutionContext over N probes, and run_instructions."""

    def __init__(self, tables, n, p):
        self.tables, self.n = tables, n
        self.number = np.zeros((max(1, p.num_numbers), n), f32)  # registers.rs: reserved with zeros
        self.vector = np.zeros((max(1, p.num_vectors), n, 4), f32)
        self.rgb = np.zeros((max(1, p.num_rgbs), n, 4), f32)

    def operand(self, o, wavelength):
        if o.kind == abi.OPERAND_CONSTANT:
            return np.full(self.n, np.array([o.bits], np.uint32).view(f32)[0], f32)
        if o.kind == abi.OPERAND_INPUT:
            return np.asarray(wavelength, f32)
        return self.number[o.bits]

    def file(self, value_type):
        return self.number if value_type == abi.VT_NUMBER else (self.vector if value_type == abi.VT_VECTOR else self.rgb)

    def run(self, instrs, wavelength, normal, incident, texture, only=None):
        """One pass over `instrs`; with `only`, a predicate on the instruction, the pass of a memoised re-run."""
        T, one, two = self.tables, f32(1.0), f32(2.0)
        for ins in instrs:
            if only is not None and not only(ins):
                continue
            op, o = ins.op, ins.output
            if op == abi.OP_NUMBER:  # :82-84 -- the constant whatever the operand's kind says
                self.number[o] = np.array([ins.x.bits], np.uint32).view(f32)[0]
            elif op == abi.OP_VECTOR:  # :85-92 -- w from its operand
                self.vector[o] = np.stack([self.operand(getattr(ins, c), wavelength) for c in "xyzw"], -1)
            elif op == abi.OP_RGB:  # :93-104 -- alpha 1
                self.rgb[o] = np.stack([self.operand(ins.x, wavelength), self.operand(ins.y, wavelength), self.operand(ins.z, wavelength), np.full(self.n, one)], -1)
            elif op == abi.OP_SPECTRUM:  # :105-113
                self.number[o] = T.spectrum(ins.a, self.operand(ins.x, wavelength))
            elif op == abi.OP_COLOR_TEXTURE:  # :114-126
                self.rgb[o] = T.texture(ins.a, texture)
            elif op == abi.OP_MONO_TEXTURE:  # :127-139
                self.number[o] = T.texture(ins.a, texture)[:, 0]
            elif op == abi.OP_RGB_SPECTRUM:  # :140-152 -- rgb * response, then (red + green) + blue
                response = mul(self.rgb[ins.a][:, :3], T.rgb_response(self.operand(ins.x, wavelength)))
                self.number[o] = add(add(response[:, 0], response[:, 1]), response[:, 2])
            elif op == abi.OP_FRESNEL:  # :153-170
                vectors = {abi.INPUT_NORMAL: normal, abi.INPUT_INCIDENT: incident}
                self.number[o] = T.fresnel(self.operand(ins.x, wavelength), self.operand(ins.y, wavelength), vectors[ins.a], vectors[ins.b])
            elif op == abi.OP_BLACKBODY:  # :171-181
                self.number[o] = T.blackbody(self.operand(ins.x, wavelength), self.operand(ins.y, wavelength))
            elif op == abi.OP_RGB_TO_VECTOR:  # :182-194 -- (c * 2) - 1, alpha too
                self.vector[o] = sub(mul(self.rgb[ins.a], two), one)
            elif op == abi.OP_MIX:  # :195-227
                amount = rust_max(rust_min(self.operand(ins.x, wavelength), one), f32(0.0))  # amount.min(1.0).max(0.0)
                F = self.file(ins.value_type)
                if ins.value_type == abi.VT_NUMBER:  # lhs * (1 - amount) + rhs * amount
                    F[o] = add(mul(F[ins.a], sub(one, amount)), mul(F[ins.b], amount))
                else:  # cgmath lerp / palette mix: lhs + (rhs - lhs) * amount, all four components
                    F[o] = add(F[ins.a], mul(sub(F[ins.b], F[ins.a]), amount[:, None]))
            elif op == abi.OP_BINARY:  # :228-268 -- componentwise, all four components
                F = self.file(ins.value_type)
                F[o] = _op(ins.operator_, F[ins.a], F[ins.b])
            elif op == abi.OP_CLAMP:  # :269-280 -- value.min(max).max(min)
                value, lo, hi = self.operand(ins.x, wavelength), self.operand(ins.y, wavelength), self.operand(ins.z, wavelength)
                self.number[o] = rust_max(rust_min(value, hi), lo)
            else:
                raise ValueError("unknown opcode %d" % op)

    def output(self, p):
        return (self.number[p.output_reg] if p.output_kind == abi.OUTPUT_NUMBER else self.vector[p.output_reg]).copy()


def _inputs(wavelength, normal, incident, texture):
    wavelength = np.atleast_1d(np.asarray(wavelength, f32))
    n = wavelength.shape[0]
    return wavelength, np.broadcast_to(np.asarray(normal, f32), (n, 3)), np.broadcast_to(np.asarray(incident, f32), (n, 3)), np.broadcast_to(np.asarray(texture, f32), (n, 2))


def evaluate(tables, instrs, p, wavelength, normal, incident, texture):
    """A full run per probe: float32 [N] (number output) or [N, 4] (vector output). `instrs` are the program's own instructions."""
    if p.kind == abi.PROGRAM_CONSTANT:
        return np.full(np.atleast_1d(wavelength).shape[0], f32(p.constant), f32)
    wavelength, normal, incident, texture = _inputs(wavelength, normal, incident, texture)
    m = Machine(tables, len(wavelength), p)
    m.run(instrs, wavelength, normal, incident, texture)
    return m.output(p)


def evaluate_memoised(tables, instrs, p, wavelengths, normal, incident, texture, rerun_constants=False):
    """The memoised run: `wavelengths` is [N, K]; a full run at [:, 0], then only the PYR_DEP_WAVELENGTH instructions at each further
    column, the files persisting. With `rerun_constants` the instructions without dependencies run again too, as
    execution_context.rs:76 has it. Returns [N, K] (or [N, K, 4])."""
    wavelengths = np.asarray(wavelengths, f32)
    first, normal, incident, texture = _inputs(wavelengths[:, 0], normal, incident, texture)
    m = Machine(tables, len(first), p)
    outs = []
    for k in range(wavelengths.shape[1]):
        only = None if k == 0 else ((lambda ins: ins.deps == 0 or bool(ins.deps & WL)) if rerun_constants else (lambda ins: bool(ins.deps & WL)))
        m.run(instrs, wavelengths[:, k], normal, incident, texture, only)
        outs.append(m.output(p))
    return np.stack(outs, 1)


def program_instrs(desc, index):
    p = desc.programs[index]
    return [desc.instrs[p.first_instr + k] for k in range(p.num_instrs)], p
