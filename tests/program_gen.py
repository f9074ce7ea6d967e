"""Generators of well-typed straight-line material programs at the level of the ABI (include/pyrite_gpu.h PyrInstr / PyrProgram):
what a caller of pyr_scene_create may hand over, not only what compiler.py and lua_project.py happen to emit. Test infrastructure.

`Gen.program()` is the generator tests/test_program_registers.py has always used (its draws are unchanged). The families on top of
it each draw from a random stream of their own and aim at one decision of scene_pack.cpp's pack_program / split_product or at one corner
of the interpreters (kernels.hip Vm::step, lambda_eval, the tape replay, the wide build). Every instruction carries its transitive
dependencies. No family emits a program whose memoised re-run differs from its full run (include/pyrite_gpu.h, PyrInstr::deps)."""
import zlib

import numpy as np

from pyrite_amd import abi

WL = abi.DEP_WAVELENGTH
HIT = abi.DEP_NORMAL | abi.DEP_INCIDENT | abi.DEP_TEXTURE
f32 = np.float32


def bits(v):
    return int(np.float32(v).view(np.uint32))


def const(v):
    return abi.PyrOperand(abi.OPERAND_CONSTANT, bits(v)), 0


WAVELENGTH = (abi.PyrOperand(abi.OPERAND_INPUT, abi.INPUT_WAVELENGTH), WL)


class Case:
    """One generated program: `family`, `kind` (the sub-case: a near miss's name, a product's factor count ...), its instructions
    (register numbers as the program declares them, first_instr 0) and what the classifier must make of a scene that holds it
    (`tape`: 2, 0 or None for no claim)."""

    def __init__(self, family, kind, instrs, p, tape=None, wide=False):
        self.family, self.kind, self.instrs, self.p, self.tape, self.wide = family, kind, instrs, p, tape, wide

    @property
    def name(self):
        return "%s/%s" % (self.family, self.kind)

    def over_declared(self):
        p = self.p
        return p.num_numbers > abi.MAX_NUMBER_REGISTERS or p.num_vectors > abi.MAX_VECTOR_REGISTERS or p.num_rgbs > abi.MAX_RGB_REGISTERS


class Builder:
    """Emits instructions into one program, numbers registers and tracks every register's transitive dependencies."""

    def __init__(self):
        self.instrs = []
        self.counts = {"n": 0, "v": 0, "c": 0}
        self.deps = {"n": {}, "v": {}, "c": {}}

    def emit(self, file, deps, output=None, **kw):
        ins = abi.PyrInstr()
        for k, v in kw.items():
            setattr(ins, k, v)
        ins.deps = deps
        ins.output = self.counts[file] if output is None else output
        self.counts[file] = max(self.counts[file], ins.output + 1)
        self.instrs.append(ins)
        self.deps[file][ins.output] = deps
        return ins.output

    def reg(self, r):
        return abi.PyrOperand(abi.OPERAND_REGISTER, r), self.deps["n"][r]

    def number(self, v, output=None):
        return self.emit("n", 0, output, op=abi.OP_NUMBER, x=const(v)[0])

    def spectrum(self, a, x=WAVELENGTH, output=None):
        return self.emit("n", x[1], output, op=abi.OP_SPECTRUM, x=x[0], a=a)

    def blackbody(self, temperature, x=WAVELENGTH, output=None):
        return self.emit("n", x[1] | temperature[1], output, op=abi.OP_BLACKBODY, x=x[0], y=temperature[0])

    def clamp(self, x, y, z, output=None):
        return self.emit("n", x[1] | y[1] | z[1], output, op=abi.OP_CLAMP, x=x[0], y=y[0], z=z[0])

    def mono(self, texture, output=None):
        return self.emit("n", abi.DEP_TEXTURE, output, op=abi.OP_MONO_TEXTURE, a=texture, b=abi.INPUT_TEXTURE)

    def colour(self, texture, output=None):
        return self.emit("c", abi.DEP_TEXTURE, output, op=abi.OP_COLOR_TEXTURE, a=texture, b=abi.INPUT_TEXTURE)

    def fresnel(self, ior, env_ior, output=None):
        return self.emit("n", ior[1] | env_ior[1] | abi.DEP_NORMAL | abi.DEP_INCIDENT, output, op=abi.OP_FRESNEL, x=ior[0], y=env_ior[0], a=abi.INPUT_NORMAL,
                         b=abi.INPUT_INCIDENT)

    def rgb(self, x, y, z, output=None):
        return self.emit("c", x[1] | y[1] | z[1], output, op=abi.OP_RGB, x=x[0], y=y[0], z=z[0])

    def vector(self, x, y, z, w, output=None):
        return self.emit("v", x[1] | y[1] | z[1] | w[1], output, op=abi.OP_VECTOR, x=x[0], y=y[0], z=z[0], w=w[0])

    def rgb_spectrum(self, source, x=WAVELENGTH, output=None):
        return self.emit("n", self.deps["c"][source] | x[1], output, op=abi.OP_RGB_SPECTRUM, x=x[0], a=source)

    def rgb_to_vector(self, source, output=None):
        return self.emit("v", self.deps["c"][source], output, op=abi.OP_RGB_TO_VECTOR, a=source)

    def mix(self, file, a, b, amount, output=None):
        vt = {"n": abi.VT_NUMBER, "v": abi.VT_VECTOR, "c": abi.VT_RGB}[file]
        return self.emit(file, self.deps[file][a] | self.deps[file][b] | amount[1], output, op=abi.OP_MIX, value_type=vt, a=a, b=b, x=amount[0])

    def binary(self, file, operator, a, b, output=None):
        vt = {"n": abi.VT_NUMBER, "v": abi.VT_VECTOR, "c": abi.VT_RGB}[file]
        return self.emit(file, self.deps[file][a] | self.deps[file][b], output, op=abi.OP_BINARY, value_type=vt, operator_=operator, a=a, b=b)

    def mul(self, a, b, output=None):
        return self.binary("n", abi.BIN_MUL, a, b, output)

    def program(self, reg, output="number"):
        return self.instrs, abi.PyrProgram(abi.PROGRAM_INSTRUCTIONS, 0.0, 0, len(self.instrs), abi.OUTPUT_NUMBER if output == "number" else abi.OUTPUT_VECTOR, reg,
                                           self.counts["n"], self.counts["v"], self.counts["c"])


class Gen:
    """Well-typed single-assignment programs over every opcode, with shared subexpressions and every kind of dependency."""

    def __init__(self, rng, num_spectra, colour_textures, mono_textures, wide=False, seed=0, spectrum_range=(400.0, 700.0)):
        self.rng, self.num_spectra, self.colour_textures, self.mono_textures = rng, num_spectra, colour_textures, mono_textures
        self.wide = wide
        self.seed, self.spectrum_range, self._streams = seed, spectrum_range, {}  # the families below: one stream each, none of them self.rng

    def program(self, allow_wavelength=True, output="number"):
        rng = self.rng
        instrs, vals = [], {"n": [], "v": [], "c": []}  # (register, deps)
        counts = {"n": 0, "v": 0, "c": 0}

        def emit(file, deps, **kw):
            ins = abi.PyrInstr()
            for k, v in kw.items():
                setattr(ins, k, v)
            ins.deps, ins.output = deps, counts[file]
            counts[file] += 1
            instrs.append(ins)
            vals[file].append((ins.output, deps))
            return ins.output, deps

        def number_operand():
            r = rng.random()
            if r < 0.25 or not vals["n"]:
                if allow_wavelength and r < 0.12:
                    return abi.PyrOperand(abi.OPERAND_INPUT, abi.INPUT_WAVELENGTH), WL
                return abi.PyrOperand(abi.OPERAND_CONSTANT, int(np.float32(rng.uniform(0.05, 2.0)).view(np.uint32))), 0
            reg, deps = vals["n"][rng.integers(len(vals["n"]))]
            return abi.PyrOperand(abi.OPERAND_REGISTER, reg), deps

        def pick(file):
            return vals[file][rng.integers(len(vals[file]))]

        def f32bits(v):
            return abi.PyrOperand(abi.OPERAND_CONSTANT, int(np.float32(v).view(np.uint32)))

        length = int(rng.integers(12, 90 if self.wide else 60))
        for _ in range(length):
            choice = rng.integers(0, 14)
            if choice == 0 or not vals["n"]:
                emit("n", 0, op=abi.OP_NUMBER, x=f32bits(rng.uniform(0.1, 1.5)))
            elif choice == 1 and allow_wavelength:
                x, d = number_operand()
                if x.kind == abi.OPERAND_CONSTANT:
                    x, d = abi.PyrOperand(abi.OPERAND_INPUT, abi.INPUT_WAVELENGTH), WL
                emit("n", d, op=abi.OP_SPECTRUM, x=x, a=int(rng.integers(self.num_spectra)))
            elif choice == 2 and allow_wavelength:
                emit("n", WL, op=abi.OP_BLACKBODY, x=abi.PyrOperand(abi.OPERAND_INPUT, abi.INPUT_WAVELENGTH), y=f32bits(rng.uniform(2000, 8000)))
            elif choice == 3:
                (x, dx), (y, dy), (z, dz) = number_operand(), number_operand(), number_operand()
                emit("n", dx | dy | dz, op=abi.OP_CLAMP, x=x, y=y, z=z)
            elif choice == 4:
                emit("n", abi.DEP_TEXTURE, op=abi.OP_MONO_TEXTURE, a=self.mono_textures[rng.integers(len(self.mono_textures))], b=abi.INPUT_TEXTURE)
            elif choice == 5:
                emit("c", abi.DEP_TEXTURE, op=abi.OP_COLOR_TEXTURE, a=self.colour_textures[rng.integers(len(self.colour_textures))], b=abi.INPUT_TEXTURE)
            elif choice == 6:
                (x, dx), (y, dy) = number_operand(), number_operand()
                emit("n", dx | dy | abi.DEP_NORMAL | abi.DEP_INCIDENT, op=abi.OP_FRESNEL, x=x, y=y, a=abi.INPUT_NORMAL, b=abi.INPUT_INCIDENT)
            elif choice == 7:
                (x, dx), (y, dy), (z, dz) = number_operand(), number_operand(), number_operand()
                emit("c", dx | dy | dz, op=abi.OP_RGB, x=x, y=y, z=z)
            elif choice == 8:
                ops = [number_operand() for _ in range(4)]
                emit("v", ops[0][1] | ops[1][1] | ops[2][1] | ops[3][1], op=abi.OP_VECTOR, x=ops[0][0], y=ops[1][0], z=ops[2][0], w=ops[3][0])
            elif choice == 9 and vals["c"] and allow_wavelength:
                reg, d = pick("c")
                emit("n", d | WL, op=abi.OP_RGB_SPECTRUM, x=abi.PyrOperand(abi.OPERAND_INPUT, abi.INPUT_WAVELENGTH), a=reg)
            elif choice == 10 and vals["c"]:
                reg, d = pick("c")
                emit("v", d, op=abi.OP_RGB_TO_VECTOR, a=reg)
            else:
                file = ["n", "v", "c"][rng.integers(3)]
                if not vals[file]:
                    file = "n"
                (ra, da), (rb, db) = pick(file), pick(file)
                vt = {"n": abi.VT_NUMBER, "v": abi.VT_VECTOR, "c": abi.VT_RGB}[file]
                if rng.random() < 0.3:
                    x, dx = number_operand()
                    emit(file, da | db | dx, op=abi.OP_MIX, value_type=vt, a=ra, b=rb, x=x)
                else:
                    emit(file, da | db, op=abi.OP_BINARY, value_type=vt, operator_=int(rng.integers(4)), a=ra, b=rb)
        out_file = "n" if output == "number" else "v"
        if output == "vector" and not vals["v"]:
            emit("v", 0, op=abi.OP_VECTOR, x=f32bits(0.0), y=f32bits(0.0), z=f32bits(1.0), w=f32bits(0.0))
        # the output: the last value of its file, most of the time a late one
        reg = vals[out_file][-1][0] if rng.random() < 0.8 else pick(out_file)[0]
        p = abi.PyrProgram(abi.PROGRAM_INSTRUCTIONS, 0.0, 0, len(instrs), abi.OUTPUT_NUMBER if output == "number" else abi.OUTPUT_VECTOR, reg,
                           counts["n"], counts["v"], counts["c"])
        return instrs, p

    # ================================================================================== the families (each on a stream of its own)
    FAMILIES = ("general", "hit_value", "lambda", "fast", "hit_rgb", "product", "near_miss", "allocated", "normal_map")
    FAST_KINDS = ("spectrum", "spectrum_mul", "mul_spectrum", "shared_output", "output_names_spectrum", "crossed", "fourth_instruction")
    LO, HI = 0.02, 0.98  # the closing clamp of a program that is to colour a surface

    def stream(self, name):
        if name not in self._streams:
            self._streams[name] = np.random.default_rng([self.seed, zlib.crc32(name.encode())])
        return self._streams[name]

    def _with_stream(self, name, **kw):
        saved, self.rng = self.rng, self.stream(name)
        try:
            return self.program(**kw)
        finally:
            self.rng = saved

    def _spectrum_id(self, rng):
        return int(rng.integers(self.num_spectra))

    def _mono_id(self, rng):
        return int(self.mono_textures[rng.integers(len(self.mono_textures))])

    def _colour_id(self, rng):
        return int(self.colour_textures[rng.integers(len(self.colour_textures))])

    # ---- general: today's program(), number and vector output (pack_program: any form, or none)
    def general(self, output="number", close=False):
        instrs, p = self._with_stream("general_" + output, allow_wavelength=output == "number", output=output)
        if close and output == "number":
            instrs, p = close_number(instrs, p, self.LO, self.HI)
        return Case("general", ("wide_" if self.wide else "") + output + ("_closed" if close else ""), instrs, p)

    # ---- hit_value: no instruction reads the wavelength (pack_program: dependent == 0 -> TAPE_FORM_HIT_VALUE)
    def hit_value(self, close=True):
        instrs, p = self._with_stream("hit_value", allow_wavelength=False, output="number")
        if close:
            instrs, p = close_number(instrs, p, self.LO, self.HI)
        return Case("hit_value", "closed" if close else "raw", instrs, p, tape=2)

    # ---- lambda: number-only opcodes, no hit inputs (pack_program: `lambda` -> TAPE_FORM_LAMBDA, kernels.hip lambda_eval)
    def _lambda_fragment(self, b, rng, length, shared=(), pure=False):
        """Emits `length` number-only instructions without hit inputs; returns a register that depends on the wavelength. `pure`:
        every instruction that is not a NumberValue depends on the wavelength (what split_product's closed check asks of a
        product's wavelength side)."""
        vals = list(shared)
        lo, hi = self.spectrum_range

        def pick():
            return vals[rng.integers(len(vals))]

        def dependent():
            ws = [v for v in vals if b.deps["n"][v] & WL]
            if not ws:
                vals.append(b.spectrum(self._spectrum_id(rng)))
                return vals[-1]
            return ws[rng.integers(len(ws))]

        def operand():
            r = rng.random()
            if r < 0.2:
                return WAVELENGTH
            if r < 0.5 or not vals:
                return const(rng.uniform(-0.5, 1.5))  # Mix amounts outside [0, 1]; Clamp bounds in either order
            return b.reg(pick())

        for _ in range(length):
            c = rng.integers(0, 9)
            if c == 0 or len(vals) < 2:
                vals.append(b.number(0.0 if rng.random() < 0.15 else rng.uniform(0.05, 1.5)))  # a zero now and then: x / 0 is inf, 0 / 0 and inf - inf are NaN
            elif c == 1:
                vals.append(b.spectrum(self._spectrum_id(rng)))
            elif c == 2:  # a Spectrum read at a register value below, inside and above the spectrum's range
                if pure or rng.random() < 0.4:
                    at = b.mul(dependent(), b.number([300.0, 600.0, 900.0][rng.integers(3)]))
                else:
                    at = b.number([lo - 50.0, lo, 0.5 * (lo + hi) + 12.5, hi, hi + 45.0, 1e-3][rng.integers(6)])
                vals.append(b.spectrum(self._spectrum_id(rng), b.reg(at)))
            elif c == 3:
                t = const(rng.uniform(2500.0, 6500.0))
                if rng.random() < 0.3:
                    t = b.reg(b.number(rng.uniform(2500.0, 6500.0)))
                vals.append(b.mul(b.blackbody(t), b.number(2e-14)))
            elif c == 4:
                x = (WAVELENGTH if rng.random() < 0.3 else b.reg(dependent())) if pure else operand()
                vals.append(b.clamp(x, operand(), operand()))  # min > max half of the time
            elif c in (5, 6):
                a, other = (dependent() if pure else pick()), pick()
                if rng.random() < 0.5:
                    a, other = other, a
                vals.append(b.binary("n", int(rng.integers(4)), a, other))
            else:
                a, other = (dependent() if pure else pick()), pick()
                if rng.random() < 0.5:
                    a, other = other, a
                vals.append(b.mix("n", a, other, operand()))
        out = vals[-1]
        if not b.deps["n"][out] & WL:
            s = b.spectrum(self._spectrum_id(rng))
            out = b.mul(s, out) if rng.random() < 0.5 else b.mul(out, s)
        return out

    def lambda_(self, close=True, length=None):
        rng = self.stream("lambda")
        b = Builder()
        out = self._lambda_fragment(b, rng, int(rng.integers(3, 12)) if length is None else length)
        if close:
            out = b.clamp(b.reg(out), const(self.LO), const(self.HI))
        return Case("lambda", "closed" if close else "raw", *b.program(out), tape=2)

    # ---- specials: inf, -inf, NaN and -0 made from a spectrum (lambda) or a mono texel (hit_value), and what Clamp and Mix make of a NaN
    # (f32::min / f32::max return the other operand: three of these are reflectances again, and are rendered)
    SPECIALS = ("inf", "minus_inf", "nan", "clamp_of_nan", "clamp_to_nan", "mix_by_nan", "mix_with_inf", "minus_zero", "negative")

    def special(self, kind, hit=False):
        rng = self.stream("special")
        b = Builder()
        leaf = (lambda: b.mono(self._mono_id(rng))) if hit else (lambda: b.spectrum(self._spectrum_id(rng)))
        s, t = leaf(), leaf()
        zero = b.binary("n", abi.BIN_SUB, s, s)
        minus = b.binary("n", abi.BIN_SUB, zero, s)
        nan = b.binary("n", abi.BIN_DIV, zero, zero)
        inf = b.binary("n", abi.BIN_DIV, s, zero)
        if kind == "inf":
            out = inf
        elif kind == "minus_inf":
            out = b.binary("n", abi.BIN_DIV, minus, zero)
        elif kind == "nan":
            out = nan
        elif kind == "clamp_of_nan":  # NaN.min(0.8).max(0.2) is 0.8
            out = b.clamp(b.reg(nan), const(0.2), const(0.8))
        elif kind == "clamp_to_nan":  # s.min(0.8).max(NaN) is s.min(0.8)
            out = b.clamp(b.reg(s), b.reg(nan), const(0.8))
        elif kind == "mix_by_nan":  # NaN.min(1).max(0) is 1: the right-hand side
            out = b.mix("n", s, t, b.reg(nan))
        elif kind == "mix_with_inf":  # s * 1 + inf * 0 is NaN
            out = b.mix("n", s, inf, const(0.0))
        elif kind == "minus_zero":
            out = b.mul(minus, zero)
        elif kind == "negative":
            out = b.binary("n", abi.BIN_SUB, b.mul(s, b.number(0.5)), t)
        else:
            raise ValueError(kind)
        return Case("hit_value" if hit else "lambda", "special_" + kind, *b.program(out), tape=2)

    # ---- fast shapes: the three shapes pack_program short-cuts (FAST_SPECTRUM, FAST_SPECTRUM_MUL, FAST_MUL_SPECTRUM) and their one-off
    # neighbours, which it must not (they are LAMBDA forms: the interpreter's value, not the short cut's)
    def fast(self, kind):
        rng = self.stream("fast")
        b = Builder()
        s, c = self._spectrum_id(rng), rng.uniform(0.1, 0.95)
        if kind == "spectrum":  # num_instrs == 1 && is_spectrum(I[0]) && output_reg == I[0].output
            out = b.spectrum(s)
        elif kind == "spectrum_mul":  # [Spectrum -> r, Number -> q, r * q]
            r, q = b.spectrum(s), b.number(c)
            out = b.mul(r, q)
        elif kind == "mul_spectrum":  # [Number -> q, Spectrum -> r, q * r]
            q, r = b.number(c), b.spectrum(s)
            out = b.mul(q, r)
        elif kind == "shared_output":  # the two leading instructions share an output register: I[0].output != I[1].output fails
            if rng.random() < 0.5:
                b.spectrum(s, output=0), b.number(c, output=0)  # the product is c * c
            else:
                b.number(c, output=0), b.spectrum(s, output=0)  # the product is spectrum * spectrum
            out = b.mul(0, 0)
        elif kind == "output_names_spectrum":  # output_reg names the spectrum, not the product: output_reg == I[2].output fails
            r, q = (b.spectrum(s), b.number(c)) if rng.random() < 0.5 else (b.number(c), b.spectrum(s))[::-1]
            b.mul(r, q) if rng.random() < 0.5 else b.mul(q, r)
            out = r
        elif kind == "crossed":  # the multiply's a / b crossed against the pattern: I[2].a == I[0].output fails
            first, second = (b.spectrum(s), b.number(c)) if rng.random() < 0.5 else (b.number(c), b.spectrum(s))
            out = b.mul(second, first)
        elif kind == "fourth_instruction":  # num_instrs == 3 fails
            r, q = (b.spectrum(s), b.number(c)) if rng.random() < 0.5 else (b.number(c), b.spectrum(s))
            out = b.mul(r, q)
            b.number(rng.uniform(0.1, 0.9))
        else:
            raise ValueError(kind)
        return Case("fast", kind, *b.program(out), tape=2)

    # ---- hit_rgb: a wavelength-free RGB-valued prefix closed by one RgbSpectrum on the wavelength input (pack_program: dependent == 1
    # && last.op == RGB_SPECTRUM && operand_is_wavelength(last.x) && last.output == output_reg -> TAPE_FORM_HIT_RGB)
    def _rgb_fragment(self, b, rng, length):
        nums, cols = [], []

        def number_operand(lo=0.05, hi=0.95):
            if rng.random() < 0.5 or not nums:
                return const(rng.uniform(lo, hi))
            return b.reg(nums[rng.integers(len(nums))])

        def pick():
            return cols[rng.integers(len(cols))]

        for _ in range(length):
            c = rng.integers(0, 9)
            if c == 0 or not cols:
                cols.append(b.colour(self._colour_id(rng)) if rng.random() < 0.6 else b.rgb(number_operand(), number_operand(), number_operand()))
            elif c == 1:
                nums.append(b.mono(self._mono_id(rng)))
            elif c == 2:
                nums.append(b.fresnel(const(rng.uniform(1.2, 1.9)), const(1.0)))
            elif c == 3:
                cols.append(b.rgb(number_operand(), number_operand(), number_operand()))
            elif c in (4, 5, 6):
                operator = [abi.BIN_MUL, abi.BIN_MUL, abi.BIN_ADD, abi.BIN_SUB, abi.BIN_DIV][rng.integers(5)]
                lhs, rhs = pick(), pick()
                if operator == abi.BIN_SUB:  # a small constant colour: the difference stays a reflectance at most hits
                    rhs = b.rgb(const(rng.uniform(0.0, 0.1)), const(rng.uniform(0.0, 0.1)), const(rng.uniform(0.0, 0.1)))
                elif operator == abi.BIN_DIV:  # by a constant colour, never by a texel (a zero texel between the probes would be an inf in the film)
                    rhs = b.rgb(const(rng.uniform(1.0, 2.5)), const(rng.uniform(1.0, 2.5)), const(rng.uniform(1.0, 2.5)))
                cols.append(b.binary("c", operator, lhs, rhs))
            else:
                cols.append(b.mix("c", pick(), pick(), number_operand(-0.5, 1.5)))
        return cols[-1]

    def hit_rgb(self, length=None):
        rng = self.stream("hit_rgb")
        b = Builder()
        source = self._rgb_fragment(b, rng, int(rng.integers(2, 9)) if length is None else length)
        return Case("hit_rgb", "prefix", *b.program(b.rgb_spectrum(source)), tape=2)

    # ---- product: ((l * h1) * h2) ... (split_product -> TAPE_FORM_PRODUCT): l a fast-shape spectrum or a lambda fragment, every h a
    # hit_value fragment; both operand orders at every level; constants before l's writer serve both sides
    def _hit_fragment(self, b, rng, length, shared=()):
        """Wavelength-free number instructions over the hit's inputs, closed by a clamp to [LO, HI]; returns its register."""
        vals = list(shared)

        def pick():
            return vals[rng.integers(len(vals))]

        def operand():
            if rng.random() < 0.5 or not vals:
                return const(rng.uniform(0.0, 1.0))
            return b.reg(pick())

        for _ in range(length):
            c = rng.integers(0, 9)
            if c == 0:
                vals.append(b.number(0.0 if rng.random() < 0.15 else rng.uniform(0.05, 1.0)))
            elif c == 1 or not vals:
                vals.append(b.mono(self._mono_id(rng)))
            elif c == 2:
                vals.append(b.fresnel(const(rng.uniform(1.2, 1.9)) if rng.random() < 0.7 else b.reg(b.number(rng.uniform(1.2, 1.9))), const(1.0)))
            elif c == 3:
                vals.append(b.clamp(operand(), operand(), operand()))
            elif c == 4:  # an RgbSpectrum at a constant wavelength is a hit value
                vals.append(b.rgb_spectrum(b.colour(self._colour_id(rng)), const(rng.uniform(400.0, 700.0))))
            elif c == 5:  # a Spectrum read at a value of the hit
                at = b.mul(b.mono(self._mono_id(rng)), b.number(rng.uniform(500.0, 900.0)))
                vals.append(b.spectrum(self._spectrum_id(rng), b.reg(at)))
            elif c in (6, 7):
                vals.append(b.binary("n", int(rng.integers(4)), pick(), pick()))
            else:
                vals.append(b.mix("n", pick(), pick(), operand()))
        out = vals[-1] if vals else b.mono(self._mono_id(rng))
        if not b.deps["n"][out] & HIT:
            m = b.mono(self._mono_id(rng))
            out = b.mul(out, m) if rng.random() < 0.5 else b.mul(m, out)
        return b.clamp(b.reg(out), const(self.LO), const(self.HI))

    def _fast_l(self, b, rng):
        """One of the three fast shapes, inline."""
        s, c, kind = self._spectrum_id(rng), rng.uniform(0.2, 0.95), rng.integers(3)
        if kind == 0:
            return b.spectrum(s)
        if kind == 1:
            r, q = b.spectrum(s), b.number(c)
            return b.mul(r, q)
        q, r = b.number(c), b.spectrum(s)
        return b.mul(q, r)

    def product(self, factors, over=False):
        rng = self.stream("product_over" if over else "product")
        while True:
            b = Builder()
            shared = [b.number(rng.uniform(0.1, 0.9)) for _ in range(int(rng.integers(0, 3)))]
            before = [rng.random() < 0.5 for _ in range(factors)]
            h = [None] * factors
            size = (4, 9) if over else (1, 4)
            for i in range(factors):
                if before[i]:
                    h[i] = self._hit_fragment(b, rng, int(rng.integers(*size)), shared)
            if rng.random() < 0.4:
                l = self._fast_l(b, rng)
            else:
                l = self._lambda_fragment(b, rng, int(rng.integers(*((5, 10) if over else (2, 6)))), shared, pure=True)
                l = b.clamp(b.reg(l), const(self.LO), const(self.HI))
            for i in range(factors):
                if not before[i]:
                    h[i] = self._hit_fragment(b, rng, int(rng.integers(*size)), shared)
            cur = l
            for i in range(factors):
                cur = b.mul(cur, h[i]) if rng.random() < 0.5 else b.mul(h[i], cur)
            if (b.counts["n"] > abi.MAX_NUMBER_REGISTERS or b.counts["c"] > abi.MAX_RGB_REGISTERS) == over:
                return Case("product", str(factors), *b.program(cur), tape=None if over else 2)

    # ---- near misses: one per rejecting condition of pack_program's form choice and of split_product. Each is a scene that must NOT
    # record a tape (TAPE_FORM_NONE, no split), and must still equal the oracle. Conditions no well-typed program of a caller reaches,
    # and which therefore have no case: split_product's `wa < 0 || wb < 0` (a register read before any write),
    # `hit_list.empty() || lambda_list.empty()` (the chain's hit factor and l's writer are always there) and pyr_scene_create's second look
    # at the two halves (a hit side is wavelength-free, a wavelength side number-only, by construction). `output_kind != NUMBER` is the
    # normal_map family's, `kind != INSTRUCTIONS` every scene's constants', and the closing product missing or not the output
    # (`!is_number_mul(last) || output != output_reg`) is fresnel_in_lambda's and rgb_spectrum_is_not_the_output's.
    def near_miss(self, name):
        rng = self.stream("near_miss_" + name)
        b = Builder()
        out = getattr(self, "_miss_" + name)(b, rng)
        return Case("near_miss", name, *b.program(out), tape=0, wide=b.counts["n"] > abi.MAX_NUMBER_REGISTERS)

    def _l(self, b, rng, output=None):
        return b.spectrum(self._spectrum_id(rng), output=output)

    def _h(self, b, rng, output=None):
        if rng.random() < 0.5:
            return b.mono(self._mono_id(rng), output=output)
        return b.fresnel(const(rng.uniform(1.2, 1.9)), const(1.0), output=output)

    def _soft_colour(self, b, rng):
        """A texel pulled towards grey: its RgbSpectrum stays a reflectance at every wavelength."""
        grey = b.rgb(const(rng.uniform(0.3, 0.6)), const(rng.uniform(0.3, 0.6)), const(rng.uniform(0.3, 0.6)))
        return b.mix("c", b.colour(self._colour_id(rng)), grey, const(rng.uniform(0.6, 0.8)))

    def _miss_four_hit_factors(self, b, rng):  # split_product: outer_first.size() == 3 at the fourth level
        cur = self._l(b, rng)
        for _ in range(4):
            h = self._h(b, rng)
            cur = b.mul(cur, h) if rng.random() < 0.5 else b.mul(h, cur)
        return cur

    def _miss_mul_same_operands(self, b, rng):  # split_product: mul.a == mul.b
        p = b.mul(self._l(b, rng), self._h(b, rng))
        return b.mul(p, p)

    def _miss_both_factors_wavelength(self, b, rng):  # split_product: la == lb, both dependent
        p = b.mul(self._l(b, rng), self._h(b, rng))
        other = self._l(b, rng)
        return b.mul(p, other) if rng.random() < 0.5 else b.mul(other, p)

    def _miss_both_factors_wavelength_free(self, b, rng):  # split_product: la == lb, neither dependent (a dead Spectrum keeps HIT_VALUE away)
        self._l(b, rng)
        return b.mul(self._h(b, rng), self._h(b, rng))

    def _miss_hit_register_rewritten(self, b, rng):  # split_product: written_once_more(hit_reg, hw) -- the same value again, so both runs agree
        l, texture = self._l(b, rng), self._mono_id(rng)
        h = b.mono(texture)
        p = b.mul(l, h) if rng.random() < 0.5 else b.mul(h, l)
        b.mono(texture, output=h)
        return b.mul(p, self._h(b, rng))

    def _miss_lambda_register_rewritten(self, b, rng):  # split_product: written_once_more(l's register, lambda_writer)
        l = self._l(b, rng)
        p = b.mul(l, self._h(b, rng))
        self._l(b, rng, output=l)
        return b.mul(p, self._h(b, rng))

    def _miss_wavelength_after_lambda(self, b, rng):  # split_product: a dependent instruction at k > lambda_writer
        p = b.mul(self._l(b, rng), self._h(b, rng))
        self._l(b, rng)
        return b.mul(self._h(b, rng), p)

    def _miss_unfolded_constant(self, b, rng):  # split_product's closed check: 2 * 3 left unfolded stands on the hit side, the wavelength side reads it
        k = b.mul(b.number(rng.uniform(0.5, 0.9)), b.number(rng.uniform(0.5, 1.0)))
        l = b.mul(self._l(b, rng), k)
        return b.mul(l, self._h(b, rng))

    def _miss_clamp_overwrite(self, b, rng):  # split_product's closed check: a hit-side write between a constant and its wavelength-side read
        b.number(2.0, output=0)
        b.clamp(const(rng.uniform(0.2, 0.9)), const(0.0), const(1.0), output=0)
        l = b.mul(self._l(b, rng), 0)
        return b.mul(l, self._h(b, rng))

    # split_product's `>= PYR_MAX_NUMBER_REGISTERS` rejections are NOT reached by this or any case: only a program the allocation pass
    # leaves as declared (a register written twice) still names register 16, a scene with such a program runs the wide build, and a wide
    # scene is never split. The case holds that much: wide build, no tape, the oracle's film.
    def _miss_register_16(self, b, rng):
        l = self._l(b, rng)
        b.number(0.5, output=1), b.number(0.25, output=1)
        h = self._h(b, rng, output=16)
        return b.mul(l, h)

    def _miss_rgb_spectrum_at_a_register(self, b, rng):  # pack_program HIT_RGB: operand_is_wavelength(last.x) fails (and, with true dependencies, dependent == 2)
        c = self._soft_colour(b, rng)
        at = b.clamp(WAVELENGTH, const(400.0), const(700.0))
        return b.rgb_spectrum(c, b.reg(at))

    def _miss_rgb_spectrum_is_not_the_output(self, b, rng):  # pack_program HIT_RGB: last.output == output_reg fails
        h = self._h(b, rng)
        b.rgb_spectrum(self._soft_colour(b, rng))
        return h

    def _miss_two_dependent_in_hit_rgb(self, b, rng):  # pack_program HIT_RGB: dependent == 1 fails
        c = self._soft_colour(b, rng)
        self._l(b, rng)
        return b.rgb_spectrum(c)

    def _miss_fresnel_in_lambda(self, b, rng):  # pack_program LAMBDA: a hit input among number-only instructions; split_product: the last is no product
        t = b.binary("n", abi.BIN_ADD, self._l(b, rng), b.fresnel(const(rng.uniform(1.2, 1.9)), const(1.0)))
        return b.clamp(b.reg(t), const(self.LO), const(self.HI))

    def _miss_mix_under_product(self, b, rng):  # split_product: the wavelength side has hit inputs and is not a product (!is_number_mul(lw))
        t = b.mix("n", self._l(b, rng), self._h(b, rng), const(rng.uniform(0.2, 0.8)))
        return b.mul(t, self._h(b, rng))

    def _miss_rgb_on_the_wavelength_side(self, b, rng):  # split_product: a dependent instruction that is no number op (!number_op)
        l = b.rgb_spectrum(b.rgb(const(rng.uniform(0.1, 0.5)), const(rng.uniform(0.1, 0.5)), const(rng.uniform(0.1, 0.5))))
        return b.mul(l, self._h(b, rng))

    def _miss_dead_mixed_instruction(self, b, rng):  # split_product: a dependent instruction off the chain that reads the hit too (hit_deps(ins))
        l, h = self._l(b, rng), self._h(b, rng)
        b.mix("n", l, h, const(0.3))
        return b.mul(b.mul(l, h), self._h(b, rng))

    def _miss_two_instructions(self, b, rng):  # split_product: num_instrs < 3
        h = b.mono(self._mono_id(rng))
        self._l(b, rng)
        return h

    # ---- allocated: programs of the families above that declare more than 16 / 8 / 8 registers (pyr_program_allocate_registers gives
    # them registers that are used again)
    ALLOCATED_KINDS = ("general", "hit_value", "lambda", "hit_rgb", "product")

    def allocated(self, kind):
        rng = self.stream("allocated")
        for _ in range(1000):
            if kind == "general":
                case = self.general(close=True)
            elif kind == "hit_value":
                case = self.hit_value()
            elif kind == "lambda":
                case = self.lambda_(length=int(rng.integers(16, 30)))
            elif kind == "hit_rgb":
                case = self.hit_rgb(length=int(rng.integers(14, 24)))
            else:
                case = self.product(int(rng.integers(1, 4)), over=True)
            if case.over_declared():
                return Case("allocated", kind, case.instrs, case.p, tape=None)
        raise AssertionError("no over-declared %s program in 1000 draws" % kind)

    # ---- normal_map: vector output, wavelength-free: Vector, RgbToVector, vector Binary / Mix, ColorTexture
    def normal_map(self):
        rng = self.stream("normal_map")
        b = Builder()
        vecs = []

        def constant_vector(lo, hi, w=0.0):
            return b.vector(const(rng.uniform(lo, hi)), const(rng.uniform(lo, hi)), const(rng.uniform(lo, hi)), const(w))

        def pick():
            return vecs[rng.integers(len(vecs))]

        for _ in range(int(rng.integers(2, 8))):
            c = rng.integers(0, 6)
            if c == 0 or not vecs:
                vecs.append(b.rgb_to_vector(b.colour(self._colour_id(rng))))
            elif c == 1:
                vecs.append(constant_vector(-1.0, 1.0))
            elif c in (2, 3):
                operator = int(rng.integers(4))
                rhs = pick() if operator != abi.BIN_DIV else constant_vector(1.0, 2.0, 1.0)
                vecs.append(b.binary("v", operator, pick(), rhs))
            elif c == 4:
                vecs.append(b.mix("v", pick(), pick(), const(rng.uniform(-0.5, 1.5)) if rng.random() < 0.5 else b.reg(b.mono(self._mono_id(rng)))))
            else:
                vecs.append(b.binary("v", abi.BIN_MUL, pick(), b.vector(const(1.0), const(-1.0), const(1.0), const(1.0))))
        up = b.vector(const(0.0), const(0.0), const(rng.uniform(2.0, 4.0)), const(0.0))  # keeps the result on the surface's own side
        out = b.mix("v", vecs[-1], up, const(rng.uniform(0.6, 0.9)))
        return Case("normal_map", "vector", *b.program(out, output="vector"), tape=None)

    def wide_forcer(self):
        """Ten RGB values live at once: no allocation fits them into 8 registers, the scene runs the wide interpreter build."""
        rng = self.stream("wide_forcer")
        b = Builder()
        cols = [b.colour(self._colour_id(rng)) if k % 3 == 0 else b.rgb(const(rng.uniform(0.0, 0.1)), const(rng.uniform(0.0, 0.1)), const(rng.uniform(0.0, 0.1))) for k in range(10)]
        acc = b.binary("c", abi.BIN_MUL, cols[0], b.rgb(const(0.5), const(0.5), const(0.5)))
        for c in cols[1:]:
            acc = b.binary("c", abi.BIN_ADD, acc, c)
        out = b.clamp(b.reg(b.rgb_spectrum(acc)), const(self.LO), const(self.HI))
        return Case("general", "wide_forcer", *b.program(out), tape=0, wide=True)


NUMBER_WRITERS = (abi.OP_NUMBER, abi.OP_SPECTRUM, abi.OP_MONO_TEXTURE, abi.OP_RGB_SPECTRUM, abi.OP_FRESNEL, abi.OP_BLACKBODY, abi.OP_CLAMP)


def writes_number(ins):
    return ins.op in NUMBER_WRITERS or (ins.op in (abi.OP_BINARY, abi.OP_MIX) and ins.value_type == abi.VT_NUMBER)


def close_number(instrs, p, lo, hi):
    """The program with `Clamp(output, lo, hi)` appended as its new output (a new register): a reflectance whatever came before."""
    deps = 0
    for ins in instrs:
        if writes_number(ins) and ins.output == p.output_reg:
            deps = ins.deps
    clamp = abi.PyrInstr(op=abi.OP_CLAMP, deps=deps, output=p.num_numbers, x=abi.PyrOperand(abi.OPERAND_REGISTER, p.output_reg), y=const(lo)[0], z=const(hi)[0])
    q = abi.PyrProgram.from_buffer_copy(p)
    q.num_instrs, q.output_reg, q.num_numbers = p.num_instrs + 1, p.num_numbers, p.num_numbers + 1
    return list(instrs) + [clamp], q

def near_miss_names():
    return sorted(name[len("_miss_"):] for name in dir(Gen) if name.startswith("_miss_"))
