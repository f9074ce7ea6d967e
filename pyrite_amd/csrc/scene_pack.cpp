// scene_pack.cpp -- scene_pack.h: validation, register allocation, and the three packing steps of scene creation. Built with
// -ffp-contract=off like everything that has to round as the reference does.
#include "scene_pack.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include "program_regs.h"

namespace pyr {

int validate(const PyrSceneDesc* d) {
    if (!d) return fail(PYR_ERR_INVALID_ARGUMENT, "null scene description");
    if (d->num_programs == 0 || d->sky_program >= d->num_programs) return fail(PYR_ERR_INVALID_ARGUMENT, "sky program out of range");
    if ((d->num_triangles && (!d->tri_positions || !d->tri_normals || !d->tri_material)) || (d->num_spheres && (!d->spheres || !d->sphere_material)) ||
        (d->num_planes && (!d->planes || !d->plane_material)))
        return fail(PYR_ERR_INVALID_ARGUMENT, "null geometry array");
    // a leaf code packs (first_primitive << 3 | count) into 31 bits (bvh.h): the primitives together must stay below 2^28
    if ((uint64_t)d->num_triangles + d->num_spheres >= (1ull << 28)) return fail(PYR_ERR_INVALID_ARGUMENT, "too many primitives");
    if ((d->num_programs && !d->programs) || (d->num_instrs && !d->instrs) || (d->num_materials && !d->materials) || (d->num_components && !d->components) ||
        (d->num_lamps && !d->lamps) || (d->num_spectra && !d->spectra) || (d->num_spectrum_floats && !d->spectrum_data))
        return fail(PYR_ERR_INVALID_ARGUMENT, "null table with a non-zero count");
    for (uint32_t i = 0; i < d->num_instrs; ++i) {
        const PyrInstr& ins = d->instrs[i];
        if (ins.op == PYR_OP_COLOR_TEXTURE || ins.op == PYR_OP_MONO_TEXTURE) {
            if (ins.a >= d->num_textures || !d->textures) return fail(PYR_ERR_INVALID_ARGUMENT, "texture id out of range");
            if (d->textures[ins.a].format != (ins.op == PYR_OP_COLOR_TEXTURE ? PYR_TEXTURE_COLOR : PYR_TEXTURE_MONO))
                return fail(PYR_ERR_INVALID_ARGUMENT, "texture format does not match the opcode");
        }
        if (ins.op > PYR_OP_CLAMP) return fail(PYR_ERR_INVALID_ARGUMENT, "unknown opcode");
        if (ins.op == PYR_OP_SPECTRUM && ins.a >= d->num_spectra) return fail(PYR_ERR_INVALID_ARGUMENT, "spectrum id out of range");
        if (ins.op == PYR_OP_RGB_SPECTRUM && !d->rgb_basis) return fail(PYR_ERR_INVALID_ARGUMENT, "RgbSpectrumValue needs rgb_basis");
    }
    for (uint32_t i = 0; i < d->num_spectra; ++i) {
        const PyrSpectrum& s = d->spectra[i];
        uint64_t floats = s.format == PYR_SPECTRUM_CURVE ? 2ull * s.count : s.count;
        if (s.offset + floats > d->num_spectrum_floats) return fail(PYR_ERR_INVALID_ARGUMENT, "spectrum data out of range");
        // Spectrum::get interpolates between samples i and i + 1 for min < w < max (project/spectra.rs:44-54): with one sample
        // the reference indexes out of bounds and panics; here the description is refused
        if (s.format == PYR_SPECTRUM_ARRAY && s.count == 1 && s.min < s.max) return fail(PYR_ERR_INVALID_ARGUMENT, "array spectrum with one sample over a non-empty span");
        if (s.format > PYR_SPECTRUM_CURVE) return fail(PYR_ERR_INVALID_ARGUMENT, "unknown spectrum format");
    }
    for (uint32_t i = 0; i < d->num_textures; ++i) {
        const PyrTexture& t = d->textures[i];
        uint64_t floats = (uint64_t)t.width * t.height * (t.format == PYR_TEXTURE_COLOR ? 4u : 1u);
        if (t.width == 0 || t.height == 0 || t.format > PYR_TEXTURE_MONO || !d->texture_data || t.offset + floats > d->num_texture_floats)
            return fail(PYR_ERR_INVALID_ARGUMENT, "texture data out of range");
    }
    for (uint32_t i = 0; i < d->num_programs; ++i) {
        const PyrProgram& p = d->programs[i];
        if (p.kind == PYR_PROGRAM_INSTRUCTIONS) {
            if ((uint64_t)p.first_instr + p.num_instrs > d->num_instrs) return fail(PYR_ERR_INVALID_ARGUMENT, "program instruction range out of bounds");
        }
    }
    for (uint32_t i = 0; i < d->num_materials; ++i) {
        const PyrMaterial& m = d->materials[i];
        if (m.normal_map_program >= 0 && (uint32_t)m.normal_map_program >= d->num_programs)
            return fail(PYR_ERR_INVALID_ARGUMENT, "normal map program out of range");
        if (m.num_components == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "material without components");
        if ((uint64_t)m.first_component + m.num_components > d->num_components || (uint64_t)m.first_emissive + m.num_emissive > d->num_components)
            return fail(PYR_ERR_INVALID_ARGUMENT, "material component range out of bounds");
    }
    for (uint32_t i = 0; i < d->num_components; ++i) {
        const PyrComponent& c = d->components[i];
        if (c.bsdf > PYR_BSDF_REFRACTIVE) return fail(PYR_ERR_INVALID_ARGUMENT, "unknown bsdf");
        if (c.color_program >= d->num_programs || (c.probability_program >= 0 && (uint32_t)c.probability_program >= d->num_programs))
            return fail(PYR_ERR_INVALID_ARGUMENT, "component program out of range");
    }
    for (uint32_t i = 0; i < d->num_triangles; ++i)
        if (d->tri_material[i] >= d->num_materials) return fail(PYR_ERR_INVALID_ARGUMENT, "triangle material out of range");
    for (uint32_t i = 0; i < d->num_spheres; ++i)
        if (d->sphere_material[i] >= d->num_materials) return fail(PYR_ERR_INVALID_ARGUMENT, "sphere material out of range");
    for (uint32_t i = 0; i < d->num_planes; ++i)
        if (d->plane_material[i] >= d->num_materials) return fail(PYR_ERR_INVALID_ARGUMENT, "plane material out of range");
    for (uint32_t i = 0; i < d->num_lamps; ++i) {
        const PyrLamp& l = d->lamps[i];
        if (l.kind == PYR_LAMP_SHAPE) {
            uint32_t limit = l.shape_kind == PYR_SHAPE_SPHERE ? d->num_spheres : (l.shape_kind == PYR_SHAPE_TRIANGLE ? d->num_triangles : 0);
            if (l.shape_index >= limit) return fail(PYR_ERR_INVALID_ARGUMENT, "lamp shape out of range");
            uint32_t mat = l.shape_kind == PYR_SHAPE_SPHERE ? d->sphere_material[l.shape_index] : d->tri_material[l.shape_index];
            if (d->materials[mat].num_emissive == 0) return fail(PYR_ERR_INVALID_ARGUMENT, "lamp shape has no emissive component");
        } else if (l.kind > PYR_LAMP_SHAPE || l.color_program >= d->num_programs) {
            return fail(PYR_ERR_INVALID_ARGUMENT, "lamp program out of range");
        }
    }
    return PYR_OK;
}

namespace {

float bits_to_float(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
float shape_bits(uint32_t shape) { return bits_to_float(shape); }

bool operand_is_wavelength(const PyrOperand& o) { return o.kind == PYR_OPERAND_INPUT && o.bits == PYR_INPUT_WAVELENGTH; }

} // namespace

// Which operand slots an opcode evaluates (execution_context.rs:81-281): decides ProbabilityInput::wavelength_used.
bool instr_reads_wavelength(const PyrInstr& ins) {
    switch (ins.op) {
    case PYR_OP_VECTOR: return operand_is_wavelength(ins.x) || operand_is_wavelength(ins.y) || operand_is_wavelength(ins.z) || operand_is_wavelength(ins.w);
    case PYR_OP_RGB:
    case PYR_OP_CLAMP: return operand_is_wavelength(ins.x) || operand_is_wavelength(ins.y) || operand_is_wavelength(ins.z);
    case PYR_OP_SPECTRUM:
    case PYR_OP_RGB_SPECTRUM:
    case PYR_OP_MIX: return operand_is_wavelength(ins.x);
    case PYR_OP_FRESNEL:
    case PYR_OP_BLACKBODY: return operand_is_wavelength(ins.x) || operand_is_wavelength(ins.y);
    default: return false;
    }
}

DevProgram pack_program(const PyrInstr* instrs, const PyrProgram& p) {
    DevProgram o{};
    o.kind = p.kind;
    o.constant = p.constant;
    o.first_instr = p.first_instr;
    o.num_instrs = p.num_instrs;
    o.output_kind = p.output_kind;
    o.output_reg = p.output_reg;
    o.fast = FAST_NONE;
    o.tape_form = TAPE_FORM_DIRECT;
    if (p.kind != PYR_PROGRAM_INSTRUCTIONS) return o;
    const PyrInstr* I = instrs + p.first_instr;
    for (uint32_t k = 0; k < p.num_instrs; ++k)
        if (instr_reads_wavelength(I[k])) o.reads_wavelength = 1;
    // the tape form of a program the interpreter has to run (device_scene.h TapeForm); a fast shape found below is DIRECT again
    {
        auto depends_on_wavelength = [&](const PyrInstr& ins) { return (ins.deps & PYR_DEP_WAVELENGTH) != 0u || instr_reads_wavelength(ins); };
        uint32_t dependent = 0;
        for (uint32_t k = 0; k < p.num_instrs; ++k) dependent += depends_on_wavelength(I[k]) ? 1u : 0u;
        o.tape_form = TAPE_FORM_NONE;
        if (p.output_kind == PYR_OUTPUT_NUMBER && p.num_instrs != 0) {
            const PyrInstr& last = I[p.num_instrs - 1];
            // a function of the wavelength alone, numbers only: the subset kernels.hip lambda_eval interprets
            bool lambda = true;
            for (uint32_t k = 0; k < p.num_instrs; ++k) {
                const PyrInstr& ins = I[k];
                const bool number_op = ins.op == PYR_OP_NUMBER || ins.op == PYR_OP_SPECTRUM || ins.op == PYR_OP_BLACKBODY || ins.op == PYR_OP_CLAMP ||
                                       ((ins.op == PYR_OP_BINARY || ins.op == PYR_OP_MIX) && ins.value_type == PYR_VT_NUMBER);
                if (!number_op || (ins.deps & (PYR_DEP_NORMAL | PYR_DEP_INCIDENT | PYR_DEP_TEXTURE)) != 0u) lambda = false;
            }
            if (dependent == 0)
                o.tape_form = TAPE_FORM_HIT_VALUE;
            else if (lambda)
                o.tape_form = TAPE_FORM_LAMBDA;
            else if (dependent == 1 && last.op == PYR_OP_RGB_SPECTRUM && operand_is_wavelength(last.x) && last.output == p.output_reg) {
                o.tape_form = TAPE_FORM_HIT_RGB;
                o.tape_rgb_reg = last.a;
            }
        }
    }
    auto is_spectrum = [&](const PyrInstr& ins) { return ins.op == PYR_OP_SPECTRUM && operand_is_wavelength(ins.x); };
    auto is_mul = [&](const PyrInstr& ins) { return ins.op == PYR_OP_BINARY && ins.value_type == PYR_VT_NUMBER && ins.operator_ == PYR_BIN_MUL; };
    if (p.output_kind != PYR_OUTPUT_NUMBER) return o;
    if (p.num_instrs == 1 && is_spectrum(I[0]) && p.output_reg == I[0].output) {
        o.fast = FAST_SPECTRUM;
        o.fast_spectrum = I[0].a;
    } else if (p.num_instrs == 3 && is_mul(I[2]) && p.output_reg == I[2].output) {
        // [Spectrum -> r, Number c -> q, r * q] or [Number c -> q, Spectrum -> r, q * r] (compiler.rs convert_operands order)
        if (is_spectrum(I[0]) && I[1].op == PYR_OP_NUMBER && I[2].a == I[0].output && I[2].b == I[1].output && I[0].output != I[1].output) {
            o.fast = FAST_SPECTRUM_MUL;
            o.fast_spectrum = I[0].a;
            o.fast_scale = bits_to_float(I[1].x.bits);
        } else if (I[0].op == PYR_OP_NUMBER && is_spectrum(I[1]) && I[2].a == I[0].output && I[2].b == I[1].output && I[0].output != I[1].output) {
            o.fast = FAST_MUL_SPECTRUM;
            o.fast_spectrum = I[1].a;
            o.fast_scale = bits_to_float(I[0].x.bits);
        }
    }
    if (o.fast != FAST_NONE) o.tape_form = TAPE_FORM_DIRECT;
    return o;
}

static bool instr_depends_on_wavelength(const PyrInstr& ins) { return (ins.deps & PYR_DEP_WAVELENGTH) != 0u || instr_reads_wavelength(ins); }

// TAPE_FORM_PRODUCT (device_scene.h): a number program without a tape form of its own whose value is a chain of products
// ((lambda * h1) * h2) ... -- ONE factor made by number-only instructions that depend on the wavelength and on nothing else, every other
// factor made by instructions that do not depend on the wavelength -- is split into those two instruction lists, appended to `instrs`
// as two programs (the hit side first; registers keep their numbers). `chain` receives the hit side's registers in the order the
// products are formed, innermost first (at most three). Returns false when the program does not factor that way.
bool split_product(std::vector<PyrInstr>& instrs, const PyrProgram& p, PyrProgram& hit, PyrProgram& lambda, std::vector<uint32_t>& chain) {
    if (p.kind != PYR_PROGRAM_INSTRUCTIONS || p.output_kind != PYR_OUTPUT_NUMBER || p.num_instrs < 3) return false;
    const size_t first = p.first_instr, end = first + p.num_instrs;
    auto writes_number = [](const PyrInstr& ins) {
        return ins.op == PYR_OP_NUMBER || ins.op == PYR_OP_SPECTRUM || ins.op == PYR_OP_BLACKBODY || ins.op == PYR_OP_CLAMP || ins.op == PYR_OP_FRESNEL ||
               ins.op == PYR_OP_MONO_TEXTURE || ins.op == PYR_OP_RGB_SPECTRUM || ((ins.op == PYR_OP_BINARY || ins.op == PYR_OP_MIX) && ins.value_type == PYR_VT_NUMBER);
    };
    auto is_number_mul = [](const PyrInstr& ins) { return ins.op == PYR_OP_BINARY && ins.value_type == PYR_VT_NUMBER && ins.operator_ == PYR_BIN_MUL; };
    auto hit_deps = [](const PyrInstr& ins) { return (ins.deps & (PYR_DEP_NORMAL | PYR_DEP_INCIDENT | PYR_DEP_TEXTURE)) != 0u; };
    auto writer_before = [&](uint32_t reg, size_t before) { // the instruction whose result a read of number register `reg` at `before` sees
        for (size_t k = before; k-- > first;)
            if (writes_number(instrs[k]) && instrs[k].output == reg) return (long)k;
        return -1L;
    };
    auto written_once_more = [&](uint32_t reg, size_t after) { // ... and nobody writes it again (the split programs read registers at their ends)
        for (size_t k = after + 1; k < end; ++k)
            if (writes_number(instrs[k]) && instrs[k].output == reg) return true;
        return false;
    };
    // from the closing product down to the factor that depends on the wavelength alone
    std::vector<bool> on_chain(p.num_instrs, false);
    size_t cur = end - 1;
    if (!is_number_mul(instrs[cur]) || instrs[cur].output != p.output_reg) return false;
    std::vector<uint32_t> outer_first;
    long lambda_writer = -1;
    for (;;) {
        const PyrInstr mul = instrs[cur];
        if (mul.a == mul.b) return false;
        const long wa = writer_before(mul.a, cur), wb = writer_before(mul.b, cur);
        if (wa < 0 || wb < 0) return false;
        const bool la = instr_depends_on_wavelength(instrs[(size_t)wa]), lb = instr_depends_on_wavelength(instrs[(size_t)wb]);
        if (la == lb) return false;
        const long lw = la ? wa : wb, hw = la ? wb : wa;
        const uint32_t hit_reg = la ? mul.b : mul.a;
        if (written_once_more(hit_reg, (size_t)hw) || outer_first.size() == 3) return false;
        outer_first.push_back(hit_reg);
        on_chain[cur - first] = true;
        if (hit_deps(instrs[(size_t)lw])) { // the wavelength side is itself a product with something of the hit in it: one level down
            if (!is_number_mul(instrs[(size_t)lw])) return false;
            cur = (size_t)lw;
            continue;
        }
        lambda_writer = lw;
        break;
    }
    if (written_once_more(instrs[(size_t)lambda_writer].output, (size_t)lambda_writer)) return false;
    std::vector<PyrInstr> hit_list, lambda_list;
    std::vector<bool> on_lambda(p.num_instrs, false); // the instructions of lambda_list, by position in the program
    for (size_t k = first; k < end; ++k) {
        const PyrInstr& ins = instrs[k];
        if (on_chain[k - first]) continue;
        if (instr_depends_on_wavelength(ins)) {
            const bool number_op = ins.op == PYR_OP_SPECTRUM || ins.op == PYR_OP_BLACKBODY || ins.op == PYR_OP_CLAMP || ((ins.op == PYR_OP_BINARY || ins.op == PYR_OP_MIX) && ins.value_type == PYR_VT_NUMBER);
            if (!number_op || hit_deps(ins) || k > (size_t)lambda_writer) return false; // a second factor that reads the wavelength, or one that reads the hit too
            lambda_list.push_back(ins);
            on_lambda[k - first] = true;
        } else {
            hit_list.push_back(ins);
            if (ins.op == PYR_OP_NUMBER && k < (size_t)lambda_writer) lambda_list.push_back(ins), on_lambda[k - first] = true; // a constant either side may read
        }
    }
    if (hit_list.empty() || lambda_list.empty()) return false;
    // the wavelength side must be closed: the value every number register it reads holds there in the whole program was written by one
    // of its own instructions -- the LAST writer before the read, in program order (a hit-side instruction may write a register between
    // a constant's write and the read: the registers of an allocated program are reused). A constant that is not a NumberValue -- 2 * 3
    // left unfolded -- stands on the hit side only, and the program keeps the online form.
    {
        bool closed = true;
        for (size_t k = first; k < end && closed; ++k) {
            if (!on_lambda[k - first]) continue;
            const PyrInstr& ins = instrs[k];
            auto reads_register = [&](uint32_t r) {
                const long w = writer_before(r, k);
                if (!(r < PYR_MAX_NUMBER_REGISTERS && w >= 0 && on_lambda[(size_t)w - first])) closed = false;
            };
            auto reads = [&](const PyrOperand& o) {
                if (o.kind == PYR_OPERAND_REGISTER) reads_register(o.bits);
            };
            switch (ins.op) {
            case PYR_OP_SPECTRUM: reads(ins.x); break;
            case PYR_OP_BLACKBODY: reads(ins.x), reads(ins.y); break;
            case PYR_OP_CLAMP: reads(ins.x), reads(ins.y), reads(ins.z); break;
            case PYR_OP_BINARY: reads_register(ins.a), reads_register(ins.b); break;
            case PYR_OP_MIX: reads(ins.x), reads_register(ins.a), reads_register(ins.b); break;
            default: break; // NumberValue
            }
            if (ins.output >= PYR_MAX_NUMBER_REGISTERS) closed = false;
        }
        if (!closed) return false;
    }
    chain.assign(outer_first.rbegin(), outer_first.rend());
    for (uint32_t reg : chain)
        if (reg >= PYR_MAX_NUMBER_REGISTERS) return false;
    hit = lambda = p;
    hit.first_instr = (uint32_t)instrs.size();
    hit.num_instrs = (uint32_t)hit_list.size();
    hit.output_reg = chain[0];
    instrs.insert(instrs.end(), hit_list.begin(), hit_list.end());
    lambda.first_instr = (uint32_t)instrs.size();
    lambda.num_instrs = (uint32_t)lambda_list.size();
    lambda.output_reg = instrs[(size_t)lambda_writer].output;
    instrs.insert(instrs.end(), lambda_list.begin(), lambda_list.end());
    return true;
}

// world.rs:88-100 for a caller that did not pass plane_frames: basis(normal) (math.rs:98-123) and
// Matrix3::from_cols(binormal, tangent, normal).into() -- the f32 operations of oracle.cpp's ortho / normalize / cross /
// quat_from_cols in the same order (this file is built with -ffp-contract=off).
void plane_frame_from_normal(const float n[3], float q[4]) {
    auto cross = [](const float a[3], const float b[3], float o[3]) {
        o[0] = a[1] * b[2] - a[2] * b[1];
        o[1] = a[2] * b[0] - a[0] * b[2];
        o[2] = a[0] * b[1] - a[1] * b[0];
    };
    auto normalize = [](float v[3]) {
        float m = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        float k = 1.0f / m;
        v[0] *= k, v[1] *= k, v[2] *= k;
    };
    float unit[3] = {-n[1], n[0], 0.0f};
    if (std::fabs(n[0]) < 1.0e-4f)
        unit[0] = 1.0f, unit[1] = 0.0f, unit[2] = 0.0f;
    else if (std::fabs(n[1]) < 1.0e-4f)
        unit[0] = 0.0f, unit[1] = 1.0f, unit[2] = 0.0f;
    else if (std::fabs(n[2]) < 1.0e-4f)
        unit[0] = 0.0f, unit[1] = 0.0f, unit[2] = 1.0f;
    float z[3], y[3];
    cross(n, unit, z);
    normalize(z);
    cross(z, n, y);
    normalize(y);
    const float m00 = y[0], m01 = y[1], m02 = y[2], m10 = z[0], m11 = z[1], m12 = z[2], m20 = n[0], m21 = n[1], m22 = n[2];
    const float trace = m00 + m11 + m22;
    if (trace >= 0.0f) {
        float s = std::sqrt(1.0f + trace), w = 0.5f * s;
        s = 0.5f / s;
        q[0] = w, q[1] = (m12 - m21) * s, q[2] = (m20 - m02) * s, q[3] = (m01 - m10) * s;
    } else if (m00 > m11 && m00 > m22) {
        float s = std::sqrt((m00 - m11 - m22) + 1.0f), x = 0.5f * s;
        s = 0.5f / s;
        q[0] = (m12 - m21) * s, q[1] = x, q[2] = (m10 + m01) * s, q[3] = (m02 + m20) * s;
    } else if (m11 > m22) {
        float s = std::sqrt((m11 - m00 - m22) + 1.0f), yy = 0.5f * s;
        s = 0.5f / s;
        q[0] = (m20 - m02) * s, q[1] = (m10 + m01) * s, q[2] = yy, q[3] = (m21 + m12) * s;
    } else {
        float s = std::sqrt((m22 - m00 - m11) + 1.0f), zz = 0.5f * s;
        s = 0.5f / s;
        q[0] = (m01 - m10) * s, q[1] = (m02 + m20) * s, q[2] = (m21 + m12) * s, q[3] = zz;
    }
}

double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

const char* const kCoordinateRangeMessage =
    "a primitive lies beyond 1e15 units from the origin (or is not finite): outside the range the kernels' arithmetic is verified for";

// One DevLamp from the description: a shape lamp gathers its shape's vertices, normals, area and material (Lamp::sample touches
// nothing else). Scene creation and pyr_scene_update both pack lamps here, so a moved lamp gets creation's arithmetic.
DevLamp pack_lamp(const PyrSceneDesc* d, uint32_t i) {
    DevLamp o;
    const PyrLamp& l = d->lamps[i];
    std::memset(&o, 0, sizeof(o));
    o.kind = l.kind;
    o.shape_kind = l.shape_kind;
    o.shape_index = l.shape_index;
    o.color_program = l.color_program;
    for (int a = 0; a < 3; ++a) o.v[a] = l.v[a];
    o.width = l.width;
    if (l.kind == PYR_LAMP_SHAPE && l.shape_kind == PYR_SHAPE_SPHERE) {
        const float* p = d->spheres + 4 * (size_t)l.shape_index;
        for (int a = 0; a < 3; ++a) o.v[a] = p[a];
        o.width = p[3];
        o.area = p[3] * p[3] * 4.0f * 3.14159265358979323846f; // Shape::surface_area, shapes/mod.rs:275
        o.material = d->sphere_material[l.shape_index];
        o.t1[0] = d->sphere_tex_scale ? d->sphere_tex_scale[2 * (size_t)l.shape_index] : 1.0f;
        o.t1[1] = d->sphere_tex_scale ? d->sphere_tex_scale[2 * (size_t)l.shape_index + 1] : 1.0f;
    } else if (l.kind == PYR_LAMP_SHAPE) {
        const float* p = d->tri_positions + 9 * (size_t)l.shape_index;
        const float* n = d->tri_normals + 9 * (size_t)l.shape_index;
        for (int a = 0; a < 3; ++a) {
            o.p1[a] = p[a];
            o.p2[a] = p[3 + a];
            o.p3[a] = p[6 + a];
            o.n1[a] = n[a];
            o.n2[a] = n[3 + a];
            o.n3[a] = n[6 + a];
        }
        // 0.5 * |a x b| (shapes/mod.rs:276-285), evaluated in f32 without fusing
        volatile float ax = p[3] - p[0], ay = p[4] - p[1], az = p[5] - p[2];
        volatile float bx = p[6] - p[0], by = p[7] - p[1], bz = p[8] - p[2];
        volatile float m1 = ay * bz, m2 = az * by, m3 = az * bx, m4 = ax * bz, m5 = ax * by, m6 = ay * bx;
        volatile float cx = m1 - m2, cy = m3 - m4, cz = m5 - m6;
        volatile float xx = cx * cx, yy = cy * cy, zz = cz * cz;
        volatile float s1 = xx + yy;
        volatile float s2 = s1 + zz;
        o.area = 0.5f * std::sqrt(s2);
        o.material = d->tri_material[l.shape_index];
        if (d->tri_uvs) {
            const float* uv = d->tri_uvs + 6 * (size_t)l.shape_index;
            o.t1[0] = uv[0], o.t1[1] = uv[1], o.t2[0] = uv[2], o.t2[1] = uv[3], o.t3[0] = uv[4], o.t3[1] = uv[5];
        }
    }
    return o;
}

int pack_tables(const PyrSceneDesc* d, const PyrProgramInfo& info, PackedTables& out) {
    const bool wide_vm = info.wide != 0;
    for (uint32_t i = 0; i < d->num_programs; ++i) // (the allocated description: the kernels read every range from the uploaded array)
        if (d->programs[i].kind == PYR_PROGRAM_INSTRUCTIONS && (uint64_t)d->programs[i].first_instr + d->programs[i].num_instrs > d->num_instrs)
            return fail(PYR_ERR_INVALID_ARGUMENT, "program instruction range out of bounds after register allocation");
    out = PackedTables{};
    std::vector<DevProgram>& programs = out.programs;
    programs.resize(d->num_programs);
    for (uint32_t i = 0; i < d->num_programs; ++i) programs[i] = pack_program(d->instrs, d->programs[i]);
    // programs without a tape form that factor into a hit side and a wavelength side get both as programs of their own, behind the
    // caller's (TAPE_FORM_PRODUCT); the instruction array grows by their instructions
    std::vector<PyrInstr>& instrs = out.instrs;
    instrs.assign(d->instrs, d->instrs + d->num_instrs);
    for (uint32_t i = 0; i < d->num_programs && !wide_vm; ++i) { // (the wide build has no tape)
        if (programs[i].kind != PYR_PROGRAM_INSTRUCTIONS || programs[i].tape_form != TAPE_FORM_NONE || programs.size() + 2 > 128) continue; // (a hit tape takes at most 128 programs)
        const size_t instrs_before = instrs.size();
        PyrProgram hit, lambda;
        std::vector<uint32_t> chain;
        if (!split_product(instrs, d->programs[i], hit, lambda, chain)) continue;
        const DevProgram dev_hit = pack_program(instrs.data(), hit), dev_lambda = pack_program(instrs.data(), lambda);
        if (dev_hit.tape_form != TAPE_FORM_HIT_VALUE || !(dev_lambda.tape_form == TAPE_FORM_LAMBDA || dev_lambda.fast != FAST_NONE)) {
            instrs.resize(instrs_before);
            continue;
        }
        programs[i].tape_form = TAPE_FORM_PRODUCT;
        uint32_t packed = (uint32_t)programs.size() | (((uint32_t)programs.size() + 1u) << 8) | ((uint32_t)chain.size() << 16); // device_scene.h DevProgram::tape_rgb_reg
        for (size_t c = 0; c < chain.size(); ++c) packed |= chain[c] << (20u + 4u * (uint32_t)c); // PYR_MAX_NUMBER_REGISTERS == 16
        programs[i].tape_rgb_reg = packed;
        programs.push_back(dev_hit);
        programs.push_back(dev_lambda);
    }

    bool needs_interpreter = false, uses_textures = false;
    for (const DevProgram& pr : programs)
        if (pr.kind == PYR_PROGRAM_INSTRUCTIONS && pr.fast == FAST_NONE) needs_interpreter = true;
    for (uint32_t i = 0; i < d->num_instrs; ++i)
        if (d->instrs[i].op == PYR_OP_COLOR_TEXTURE || d->instrs[i].op == PYR_OP_MONO_TEXTURE) uses_textures = true;
    for (uint32_t i = 0; i < d->num_materials; ++i)
        if (d->materials[i].normal_map_program >= 0) uses_textures = needs_interpreter = true;
    std::vector<float>&sphere_scale = out.sphere_scale, &plane_frames = out.plane_frames;
    std::vector<DevTexture>& textures = out.textures;
    textures.resize(d->num_textures);
    if (needs_interpreter) {
        sphere_scale.assign(2 * (size_t)d->num_spheres, 1.0f);
        if (d->sphere_tex_scale) sphere_scale.assign(d->sphere_tex_scale, d->sphere_tex_scale + 2 * (size_t)d->num_spheres);
        plane_frames.resize(4 * (size_t)d->num_planes);
        for (uint32_t i = 0; i < d->num_planes; ++i) {
            if (d->plane_frames) {
                for (int a = 0; a < 4; ++a) plane_frames[4 * (size_t)i + a] = d->plane_frames[4 * (size_t)i + a];
            } else {
                plane_frame_from_normal(d->planes + 8 * (size_t)i + 3, &plane_frames[4 * (size_t)i]);
            }
        }
    }
    for (uint32_t i = 0; i < d->num_textures; ++i)
        textures[i] = DevTexture{d->textures[i].format == PYR_TEXTURE_COLOR ? 4u : 1u, d->textures[i].width, d->textures[i].height, 0u, d->textures[i].offset};

    out.texture_data = View(d->texture_data, d->num_textures ? (size_t)d->num_texture_floats * 4 : 0);
    out.sphere_material = View(d->sphere_material, (size_t)d->num_spheres * 4);
    out.planes = View(d->planes, (size_t)d->num_planes * 32);
    out.plane_material = View(d->plane_material, (size_t)d->num_planes * 4);
    out.materials = View(d->materials, (size_t)d->num_materials * sizeof(PyrMaterial));
    out.components = View(d->components, (size_t)d->num_components * sizeof(PyrComponent));
    out.spectra = View(d->spectra, (size_t)d->num_spectra * sizeof(PyrSpectrum));
    out.spectrum_data = View(d->spectrum_data, (size_t)d->num_spectrum_floats * 4);
    out.rgb_basis = View(d->rgb_basis, d->rgb_basis ? (size_t)d->rgb_basis_count * 12 : 0);
    // the small tables the kernels stage into LDS, in floats (pack_records decides whether the scene is big enough to stage them)
    out.table_floats = (uint64_t)d->num_spectra * (sizeof(PyrSpectrum) / 4) + d->num_spectrum_floats + (uint64_t)d->num_materials * (sizeof(PyrMaterial) / 4) +
                       (uint64_t)d->num_components * (sizeof(PyrComponent) / 4) + (uint64_t)programs.size() * (sizeof(DevProgram) / 4) +
                       (uint64_t)d->num_lamps * (sizeof(DevLamp) / 4);

    DevScene& v = out.scene;
    v.num_planes = d->num_planes;
    v.num_lamps = d->num_lamps;
    v.rgb_count = d->rgb_basis ? d->rgb_basis_count : 0;
    v.rgb_min = d->rgb_basis_min;
    v.rgb_max = d->rgb_basis_max;
    v.sky_program = d->sky_program;
    v.num_spectra = d->num_spectra;
    v.num_programs = (uint32_t)programs.size();
    v.num_spectrum_floats = d->num_spectrum_floats;
    v.num_materials = d->num_materials;
    v.num_components = d->num_components;
    v.needs_interpreter = needs_interpreter ? 1u : 0u;
    v.uses_textures = uses_textures ? 1u : 0u;
    // Round 4: the spectral tape for scenes WITH interpreter programs (device_scene.h TapeForm). Every colour program -- of a
    // component, of a lamp, the sky -- must have a tape form; the value slots the replay keeps in LDS (kTapeEagerSlots = 8: one
    // holds 1.0, three the RGB basis when a HIT_RGB program exists) must hold every spectrum-reading fast program (counted here
    // without the sharing the kernel finds, so never fewer), and the prepared programs must fit their LDS table (128).
    v.hit_tape = v.rgb_records = v.micro_records = v.product_records = 0;
    // value slots of the replay: one per LAMBDA program and one per DISTINCT fast shape -- programs of the same shape, factor and
    // spectrum share a slot (kernels.hip prepare_tape_tables `alike`: C3's three white walls are three programs over one spectrum)
    uint32_t fast_programs = 0;
    {
        for (size_t i = 0; i < programs.size(); ++i) {
            const DevProgram& pr = programs[i];
            if (pr.kind != PYR_PROGRAM_INSTRUCTIONS) continue;
            if (pr.tape_form == TAPE_FORM_LAMBDA) {
                fast_programs += 1u;
            } else if (pr.fast != FAST_NONE) {
                bool seen = false;
                for (size_t j = 0; j < i && !seen; ++j) {
                    const DevProgram& q = programs[j];
                    seen = q.kind == PYR_PROGRAM_INSTRUCTIONS && q.fast == pr.fast && q.fast_spectrum == pr.fast_spectrum && std::memcmp(&q.fast_scale, &pr.fast_scale, sizeof(float)) == 0;
                }
                fast_programs += seen ? 0u : 1u;
            }
        }
    }
    // the eager replay's value rows for these programs (device_scene.h), asked before and after a scene is refused its hit tape: rgb_records is 0 again then
    auto rows_needed = [&] { return tape_rows_needed(fast_programs, v.rgb_records != 0); };
    if (needs_interpreter) {
        bool ok = programs.size() <= 128;
        auto colour = [&](uint32_t id) {
            if (id >= programs.size()) return;
            const DevProgram& pr = programs[id];
            if (pr.kind != PYR_PROGRAM_INSTRUCTIONS) return;
            if (pr.tape_form == TAPE_FORM_NONE) ok = false;
            if (pr.tape_form == TAPE_FORM_HIT_RGB) v.rgb_records = 1u;
            if (pr.tape_form == TAPE_FORM_HIT_RGB || pr.tape_form == TAPE_FORM_PRODUCT) v.micro_records = 1u;
            if (pr.tape_form == TAPE_FORM_PRODUCT) v.product_records = 1u;
        };
        for (uint32_t i = 0; i < d->num_components; ++i) colour(d->components[i].color_program);
        // (a shape lamp shines with its material's emissive components, counted above: its color_program is not read)
        for (uint32_t i = 0; i < d->num_lamps; ++i)
            if (d->lamps[i].kind != PYR_LAMP_SHAPE) colour(d->lamps[i].color_program);
        colour(d->sky_program);
        if (rows_needed() > kTapeMaxValueRows) ok = false; // (counted here without LAMBDA's hit-tape condition: never fewer than the kernel finds)
        const char* off = std::getenv("PYRITE_HIT_TAPE"); // A/B and tests: PYRITE_HIT_TAPE=0 keeps the online form (read at scene creation)
        if (off && off[0] == '0') ok = false;
        if (wide_vm) ok = false; // the wide interpreter build keeps every wavelength online (kernels/wide.hip pick_wide_kernel)
        v.hit_tape = ok ? 1u : 0u;
        if (!ok) v.rgb_records = v.micro_records = v.product_records = 0u;
    }
    // eight, or what the scene's programs need; past sixteen the replay looks values up record by record
    const uint32_t rows = rows_needed();
    v.tape_value_rows = rows <= kTapeMaxValueRows ? rows : kTapeValueRows;
    // builds that replay two wavelengths per lane: packed pairs of rows where pairs pay, packed single rows where they would cost LDS
    if (tape_pairs(needs_interpreter)) v.tape_value_rows = tape_pair_build_rows(fast_programs);
    v.shadow_margin = d->num_spheres != 0 ? 1.01f : 1.001f; // device_scene.h
    v.hero_only_records = 0;
    for (uint32_t i = 0; i < d->num_materials; ++i)
        for (uint32_t k = 0; k < d->materials[i].num_emissive; ++k) {
            const int probability = d->components[d->materials[i].first_emissive + k].probability_program;
            if (probability >= 0 && programs[(size_t)probability].reads_wavelength) v.hero_only_records = 1u;
        }
    return PYR_OK;
}

// ---- the build-plan step
// Leaves are tested in pairs only by the four-child pair tree: a triangle-only scene too big to live in LDS with neither tree
// switched off. Asked before the tree exists, so by the primitives alone: their records outgrow the 8 KB the LDS-resident walk allows.
static bool predicts_pair_tree(const PyrSceneDesc* d, const BuildPlan& plan) {
    return d->num_spheres == 0 && plan.bounds.size() * 48 > 8 * 1024 && plan.wide_allowed && plan.pairs_allowed;
}

static bool switched_off(const char* name) { // A/B switches, read at every creation and rebuild
    const char* value = std::getenv(name);
    return value && value[0] == '0';
}

int plan_build(const PyrSceneDesc* d, BuildPlan& plan) {
    plan = BuildPlan{};
    std::vector<PrimBounds>& bounds = plan.bounds;
    bounds.reserve((size_t)d->num_spheres + d->num_triangles);
    for (uint32_t i = 0; i < d->num_spheres; ++i) { // Bounded::aabb, shapes/mod.rs:411-416
        PrimBounds b;
        lvl::sphere_bounds(d->spheres + 4 * (size_t)i, b.lo, b.hi);
        b.shape = ((uint32_t)PYR_SHAPE_SPHERE << 30) | i;
        bounds.push_back(b);
    }
    for (uint32_t i = 0; i < d->num_triangles; ++i) { // shapes/mod.rs:417-428
        PrimBounds b;
        lvl::triangle_bounds(d->tri_positions + 9 * (size_t)i, b.lo, b.hi);
        b.shape = ((uint32_t)PYR_SHAPE_TRIANGLE << 30) | i;
        bounds.push_back(b);
    }
    // exact_math.h: `normalize` multiplies by rcp32(sqrt32(|v|^2)), which is the correctly rounded IEEE result (what the reference
    // computes) only while lengths and squared lengths stay normal f32 numbers. Coordinates are the user's units, so a scene whose
    // extent leaves the verified range is refused instead of rendered differently from the reference (pyrite_gpu.h "Coordinates").
    for (const PrimBounds& b : bounds)
        if (!within_coordinate_range(b)) return fail(PYR_ERR_UNSUPPORTED, kCoordinateRangeMessage);
    plan.wide_allowed = !switched_off("PYRITE_WIDE_BVH");
    plan.pairs_allowed = !switched_off("PYRITE_PAIR_PRIMS");
    plan.pair_tree_expected = predicts_pair_tree(d, plan);
    // The pair tree may also split space (PYRITE_SPATIAL_SPLITS, bvh.h) and is collapsed by cost (PYRITE_WIDE_COLLAPSE); every
    // other tree is built and collapsed as before, byte for byte.
    plan.spatial = plan.pair_tree_expected && spatial_splits_wanted();
    plan.cost_driven_collapse = plan.pair_tree_expected && cost_driven_collapse_wanted();
    return PYR_OK;
}

BuiltBvh build_planned_tree(const PyrSceneDesc* d, const BuildPlan& plan, uint32_t& median_splits) {
    median_splits = 0;
    if (!plan.spatial) return build_bvh(plan.bounds, plan.pair_tree_expected, &median_splits);
    SpatialSplits spatial_params;
    spatial_params.tri_positions = d->tri_positions;
    return build_bvh_spatial(plan.bounds, spatial_params);
}

// ---- the records step
int pack_records(const PyrSceneDesc* d, const BuiltBvh& bvh, const BuildPlan& plan, bool needs_interpreter, uint64_t table_floats, PackedRecords& out) {
    if (bvh.max_depth > 96) return fail(PYR_ERR_UNSUPPORTED, "BVH deeper than the LDS traversal stack allows");
    // spatial splits repeat triangles in prim_order (and so in `prims` and the pair records): a leaf code keeps `first` in 28 bits
    if (bvh.prim_order.size() >= (1ull << 28)) return fail(PYR_ERR_UNSUPPORTED, "scene too large: 2^28 primitive references or more");
    // the traversal addresses a node by a 32-bit byte offset from the tree's base (one SGPR pair + one VGPR per load): 4 GB of 64-byte
    // binary nodes, 4 GB of 128-byte wide nodes -- about 200 M triangles, beyond which the call says so instead of wrapping around
    if (bvh.nodes.size() >= (1ull << 26)) return fail(PYR_ERR_UNSUPPORTED, "scene too large: the acceleration structure has 2^26 nodes or more (4 GB)");

    out = PackedRecords{};
    std::vector<DevPrim>& prims = out.prims;
    std::vector<DevTriShade>& shade = out.shade;
    std::vector<DevLamp>& lamps = out.lamps;
    std::vector<DevTriTex>& tri_tex = out.tri_tex;
    prims.resize(bvh.prim_order.size());
    for (size_t k = 0; k < prims.size(); ++k) {
        uint32_t shape = bvh.prim_order[k], index = shape & 0x3FFFFFFFu;
        DevPrim& o = prims[k];
        std::memset(&o, 0, sizeof(o));
        if ((shape >> 30) == PYR_SHAPE_TRIANGLE) {
            const float* p = d->tri_positions + 9 * (size_t)index;
            for (int a = 0; a < 3; ++a) {
                o.a[a] = p[a];
                o.b[a] = p[3 + a] - p[a]; // edge1 = v2 - v1, edge2 = v3 - v1 (world.rs:330-331, shapes/mod.rs:338-339)
                o.c[a] = p[6 + a] - p[a];
            }
        } else {
            const float* p = d->spheres + 4 * (size_t)index;
            for (int a = 0; a < 3; ++a) o.a[a] = p[a];
            o.b[0] = p[3];
        }
        o.a[3] = shape_bits(shape);
    }
    shade.resize(d->num_triangles);
    for (uint32_t i = 0; i < d->num_triangles; ++i) {
        const float* n = d->tri_normals + 9 * (size_t)i;
        DevTriShade& o = shade[i];
        std::memset(&o, 0, sizeof(o));
        for (int a = 0; a < 3; ++a) {
            o.n1[a] = n[a];
            o.n2[a] = n[3 + a];
            o.n3[a] = n[6 + a];
        }
        o.n1[3] = bits_to_float(d->tri_material[i]);
    }
    lamps.resize(d->num_lamps);
    for (uint32_t i = 0; i < d->num_lamps; ++i) lamps[i] = pack_lamp(d, i);
    // texture space: only the interpreter builds of the kernels read it
    if (needs_interpreter) {
        tri_tex.resize(d->num_triangles);
        for (uint32_t i = 0; i < d->num_triangles; ++i) {
            DevTriTex& o = tri_tex[i];
            std::memset(&o, 0, sizeof(o));
            if (d->tri_uvs) {
                const float* uv = d->tri_uvs + 6 * (size_t)i;
                for (int a = 0; a < 4; ++a) o.uv12[a] = uv[a];
                o.uv3[0] = uv[4], o.uv3[1] = uv[5];
            }
            o.f1[0] = o.f2[0] = o.f3[0] = 1.0f; // identity
            if (d->tri_frames) {
                const float* f = d->tri_frames + 12 * (size_t)i;
                for (int a = 0; a < 4; ++a) o.f1[a] = f[a], o.f2[a] = f[4 + a], o.f3[a] = f[8 + a];
            }
        }
    }
    out.spheres = View(d->spheres, (size_t)d->num_spheres * 16);
    // scenes that do not live in LDS also get the 4-wide tree for the resumable traversal (latency bound there);
    // PYRITE_WIDE_BVH=0 keeps the binary tree (A/B)
    WideBvh& wide = out.wide;
    const bool big_scene = outgrows_lds(bvh.nodes.size(), prims.size());
    if (big_scene && plan.wide_allowed) {
        const auto t_collapse = std::chrono::steady_clock::now();
        wide = plan.cost_driven_collapse ? collapse_to_wide_sah(bvh) : collapse_to_wide(bvh);
        out.collapse_ms = ms_between(t_collapse, std::chrono::steady_clock::now());
        if (wide.stack_need > kMaxStackDepth || wide.nodes.size() >= (1ull << 25)) wide = WideBvh{}; // too deep, or past 4 GB: the binary tree
    }
    // Triangle pairs for the wide tree's leaves (device_scene.h DevPrimPair): every leaf gets ceil(n / 2) records of its own and
    // its code in the wide nodes is rewritten to count in records. PYRITE_PAIR_PRIMS=0 keeps the one-primitive records (A/B).
    std::vector<DevPrimPair>& pairs = out.pairs;
    std::vector<Node128>& pair_nodes = out.pair_nodes;
    if (!wide.nodes.empty() && d->num_spheres == 0 && plan.pairs_allowed) {
        pair_nodes = wide.nodes;
        for (Node128& node : pair_nodes)
            for (int k = 0; k < 4; ++k) {
                const int32_t code = node.child[k];
                if (code >= 0 || code == kEmptyChild) continue;
                const uint32_t first = (uint32_t)(-1 - code) >> 3, count = (uint32_t)(-1 - code) & 7u;
                node.child[k] = encode_leaf((uint32_t)pairs.size(), count);
                if (count == 0) { // an empty leaf still names a record (trav_step_lean loads it before it looks at the count): one no triangle passes
                    DevPrimPair none;
                    std::memset(&none, 0, sizeof(none));
                    none.q[1][2] = none.q[1][3] = shape_bits(PYR_HIT_NONE);
                    pairs.push_back(none);
                }
                for (uint32_t j = 0; j < count; j += 2) {
                    DevPrimPair pr;
                    std::memset(&pr, 0, sizeof(pr));
                    for (uint32_t h = 0; h < 2; ++h) {
                        if (j + h >= count) {
                            pr.q[1][2 + h] = shape_bits(PYR_HIT_NONE);
                            continue;
                        }
                        const DevPrim& t = prims[first + j + h];
                        pr.q[0][0 + h] = t.a[0], pr.q[0][2 + h] = t.a[1], pr.q[1][0 + h] = t.a[2], pr.q[1][2 + h] = t.a[3];
                        pr.q[2][0 + h] = t.b[0], pr.q[2][2 + h] = t.b[1], pr.q[3][0 + h] = t.b[2];
                        pr.q[3][2 + h] = t.c[0], pr.q[4][0 + h] = t.c[1], pr.q[4][2 + h] = t.c[2];
                    }
                    pairs.push_back(pr);
                }
            }
    }
    out.wide_stack_depth = std::max(1u, wide.stack_need);
    out.stack_depth = std::max(1u, bvh.max_depth);
    out.num_nodes = (uint32_t)bvh.nodes.size();
    out.num_prims = (uint32_t)prims.size();
    // the small tables the kernels stage into LDS (kernels.hip stage_tables): spectra + the material / component / program /
    // lamp records. <= 16 KB, and only for scenes too big to live in LDS themselves: a small scene leaves L1 to the tables
    // (C2: staging the spectra costs a workgroup per CU and is 0.9x), a big one evicts them all the time (C3: 1.33x)
    out.lds_table_floats = (table_floats <= 4096 && big_scene) ? (uint32_t)table_floats : 0;
    PyrBvhInfo& info = out.info;
    info.num_nodes = (uint32_t)bvh.nodes.size();
    info.num_leaves = bvh.num_leaves;
    info.max_depth = bvh.max_depth;
    info.num_primitives = (uint32_t)plan.bounds.size(); // the scene's primitives; `prims` and the pair records may repeat some (spatial splits)
    info.node_bytes = bvh.nodes.size() * sizeof(Node64);
    info.primitive_bytes = prims.size() * sizeof(DevPrim);
    info.num_wide_nodes = (uint32_t)wide.nodes.size();
    info.num_pair_records = (uint32_t)pairs.size();
    info.wide_node_bytes = wide.nodes.size() * sizeof(Node128);
    info.pair_record_bytes = pairs.size() * sizeof(DevPrimPair);
    return PYR_OK;
}

// pyr_scene_create's register allocation (program_regs.h) of every program that declares more than the in-register file. Each program
// is read from the caller's instructions, never from a copy an earlier program's allocation rewrote -- two programs may name the same
// or overlapping ranges -- and a program the pass renumbered gets its instructions of its own, appended to `instrs` (which starts as
// the caller's array, so every other program keeps its range). Fails with PYR_ERR_UNSUPPORTED for a program that declares more than
// PYR_MAX_DECLARED_REGISTERS registers of a file or still needs more than the wide interpreter build's file after allocation.
int allocate_scene_registers(const PyrSceneDesc* desc, std::vector<PyrProgram>& programs, std::vector<PyrInstr>& instrs, PyrProgramInfo& info) {
    try {
        programs.assign(desc->programs, desc->programs + desc->num_programs);
        instrs.assign(desc->instrs, desc->instrs + desc->num_instrs);
        info = PyrProgramInfo{};
        std::vector<PyrInstr> code;
        for (uint32_t i = 0; i < desc->num_programs; ++i) {
            const PyrProgram& p = desc->programs[i];
            if (p.kind != PYR_PROGRAM_INSTRUCTIONS) continue;
            PyrProgram& q = programs[i];
            if (!program_fits_registers(p)) {
                code.resize(p.num_instrs);
                if (allocate_program_registers(desc->instrs + p.first_instr, p, code.data(), q) != PYR_OK)
                    return fail(PYR_ERR_UNSUPPORTED, "program " + std::to_string(i) + " declares more than " + std::to_string(PYR_MAX_DECLARED_REGISTERS) +
                                                         " registers of one kind");
                if (std::memcmp(&q, &p, sizeof(PyrProgram)) != 0) { // renumbered: its own copy of the instructions
                    if ((uint64_t)instrs.size() + code.size() >= 0xFFFFFFFFull) return fail(PYR_ERR_UNSUPPORTED, "too many program instructions");
                    q.first_instr = (uint32_t)instrs.size();
                    instrs.insert(instrs.end(), code.begin(), code.end());
                }
            }
            info.declared_numbers = std::max(info.declared_numbers, p.num_numbers);
            info.declared_vectors = std::max(info.declared_vectors, p.num_vectors);
            info.declared_rgbs = std::max(info.declared_rgbs, p.num_rgbs);
            info.allocated_numbers = std::max(info.allocated_numbers, q.num_numbers);
            info.allocated_vectors = std::max(info.allocated_vectors, q.num_vectors);
            info.allocated_rgbs = std::max(info.allocated_rgbs, q.num_rgbs);
            if (!program_fits_wide_registers(q))
                return fail(PYR_ERR_UNSUPPORTED, "program " + std::to_string(i) + " needs " + std::to_string(q.num_numbers) + " number, " + std::to_string(q.num_vectors) +
                                                     " vector and " + std::to_string(q.num_rgbs) + " RGB registers after register allocation; the wide interpreter build holds " +
                                                     std::to_string(PYR_WIDE_NUMBER_REGISTERS) + ", " + std::to_string(PYR_WIDE_VECTOR_REGISTERS) + " and " +
                                                     std::to_string(PYR_WIDE_RGB_REGISTERS));
            if (!program_fits_registers(q)) info.wide = 1u;
        }
    } catch (const std::bad_alloc&) {
        return fail(PYR_ERR_OUT_OF_MEMORY, "out of host memory while allocating program registers");
    }
    return PYR_OK;
}

} // namespace pyr
