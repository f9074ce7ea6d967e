// program_regs.cpp -- linear-scan register allocation for over-sized material programs (program_regs.h).
#include "program_regs.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

namespace pyr {
namespace {

enum File { NUM = 0, VEC = 1, RGB = 2, NONE = -1 };

// One register an instruction reads: its file and the field that names it.
struct Read {
    int file;
    uint32_t* reg;
};

// The registers instruction `ins` reads and the file it writes, as kernels.hip Vm::step evaluates them: only the operand
// slots an opcode evaluates count (a NumberValue's x is its constant whatever its kind says). False for an opcode or value
// type the interpreter does not know.
bool registers_of(PyrInstr& ins, Read reads[4], int& num_reads, int& out_file) {
    num_reads = 0;
    auto operand = [&](PyrOperand& o) {
        if (o.kind == PYR_OPERAND_REGISTER) reads[num_reads++] = Read{NUM, &o.bits};
    };
    auto typed = [&](uint32_t value_type) { return value_type == PYR_VT_NUMBER ? NUM : (value_type == PYR_VT_VECTOR ? VEC : RGB); };
    switch (ins.op) {
    case PYR_OP_NUMBER: out_file = NUM; return true;
    case PYR_OP_VECTOR: operand(ins.x), operand(ins.y), operand(ins.z), operand(ins.w), out_file = VEC; return true;
    case PYR_OP_RGB: operand(ins.x), operand(ins.y), operand(ins.z), out_file = RGB; return true;
    case PYR_OP_SPECTRUM: operand(ins.x), out_file = NUM; return true;
    case PYR_OP_COLOR_TEXTURE: out_file = RGB; return true;
    case PYR_OP_MONO_TEXTURE: out_file = NUM; return true;
    case PYR_OP_RGB_SPECTRUM: operand(ins.x), reads[num_reads++] = Read{RGB, &ins.a}, out_file = NUM; return true;
    case PYR_OP_FRESNEL:
    case PYR_OP_BLACKBODY: operand(ins.x), operand(ins.y), out_file = NUM; return true;
    case PYR_OP_RGB_TO_VECTOR: reads[num_reads++] = Read{RGB, &ins.a}, out_file = VEC; return true;
    case PYR_OP_MIX:
    case PYR_OP_BINARY:
        if (ins.value_type > PYR_VT_RGB) return false;
        if (ins.op == PYR_OP_MIX) operand(ins.x);
        reads[num_reads++] = Read{typed(ins.value_type), &ins.a};
        reads[num_reads++] = Read{typed(ins.value_type), &ins.b};
        out_file = typed(ins.value_type);
        return true;
    case PYR_OP_CLAMP: operand(ins.x), operand(ins.y), operand(ins.z), out_file = NUM; return true;
    default: return false;
    }
}

} // namespace

bool program_fits_registers(const PyrProgram& p) {
    return p.num_numbers <= PYR_MAX_NUMBER_REGISTERS && p.num_vectors <= PYR_MAX_VECTOR_REGISTERS && p.num_rgbs <= PYR_MAX_RGB_REGISTERS;
}

bool program_fits_wide_registers(const PyrProgram& p) {
    return p.num_numbers <= PYR_WIDE_NUMBER_REGISTERS && p.num_vectors <= PYR_WIDE_VECTOR_REGISTERS && p.num_rgbs <= PYR_WIDE_RGB_REGISTERS;
}

int allocate_program_registers(const PyrInstr* instrs, const PyrProgram& p, PyrInstr* instrs_out, PyrProgram& out) {
    const uint32_t n = p.num_instrs;
    if (p.kind == PYR_PROGRAM_INSTRUCTIONS &&
        (p.num_numbers > PYR_MAX_DECLARED_REGISTERS || p.num_vectors > PYR_MAX_DECLARED_REGISTERS || p.num_rgbs > PYR_MAX_DECLARED_REGISTERS))
        return PYR_ERR_UNSUPPORTED;
    std::vector<PyrInstr> code(instrs, instrs + (p.kind == PYR_PROGRAM_INSTRUCTIONS ? n : 0u));
    out = p;
    auto copy_back = [&] {
        if (!code.empty()) std::memmove(instrs_out, code.data(), code.size() * sizeof(PyrInstr));
        return PYR_OK;
    };
    if (p.kind != PYR_PROGRAM_INSTRUCTIONS || program_fits_registers(p)) return copy_back();
    const std::vector<PyrInstr> original = code;

    // The values of the program: one per writing instruction. def[file][reg] = the instruction that writes it (single assignment).
    const uint32_t declared[3] = {p.num_numbers, p.num_vectors, p.num_rgbs};
    std::vector<long> def[3];
    for (int f = 0; f < 3; ++f) def[f].assign(declared[f], -1L);
    std::vector<int> out_file(n, NONE);
    std::vector<uint32_t> last_use(n, 0);
    std::vector<bool> pinned(n, false);
    const auto depends_on_wavelength = [&](uint32_t k) { return (code[k].deps & PYR_DEP_WAVELENGTH) != 0u; };
    for (uint32_t k = 0; k < n; ++k) {
        Read reads[4];
        int num_reads = 0;
        if (!registers_of(code[k], reads, num_reads, out_file[k])) return copy_back();
        for (int r = 0; r < num_reads; ++r) {
            const uint32_t reg = *reads[r].reg;
            if (reg >= declared[reads[r].file] || def[reads[r].file][reg] < 0) return copy_back(); // read beyond the file or before any write
            const uint32_t v = (uint32_t)def[reads[r].file][reg];
            last_use[v] = k;
            // the memoised re-run: a value the re-run does not recompute but reads must survive every later (re-run) write
            if (depends_on_wavelength(k) && !depends_on_wavelength(v)) pinned[v] = true;
        }
        const uint32_t reg = code[k].output;
        if (reg >= declared[out_file[k]] || def[out_file[k]][reg] >= 0) return copy_back(); // beyond the file, or a second write
        def[out_file[k]][reg] = k;
        last_use[k] = k;
    }
    const int result_file = p.output_kind == PYR_OUTPUT_NUMBER ? NUM : VEC;
    if (p.output_reg >= declared[result_file] || def[result_file][p.output_reg] < 0) return copy_back();
    const uint32_t result = (uint32_t)def[result_file][p.output_reg];
    last_use[result] = n; // read after the last instruction, after every pass
    if (!depends_on_wavelength(result)) pinned[result] = true;

    // Pinned values first, registers 0, 1, ... in program order; then linear scan over the rest, lowest free register first. A value
    // whose last read is instruction k frees its register for k's own result (Vm::step reads every operand before it writes).
    std::vector<uint32_t> assigned(n, 0);
    uint32_t pinned_count[3] = {0, 0, 0}, used[3] = {0, 0, 0};
    for (uint32_t k = 0; k < n; ++k)
        if (pinned[k]) assigned[k] = pinned_count[out_file[k]]++;
    std::vector<long> holder[3]; // holder[file][reg]: the value in a register of the scan, -1 when free
    for (uint32_t k = 0; k < n; ++k) {
        for (int f = 0; f < 3; ++f)
            for (long& h : holder[f])
                if (h >= 0 && last_use[(size_t)h] <= k) h = -1;
        if (pinned[k]) continue;
        std::vector<long>& pool = holder[out_file[k]];
        size_t slot = 0;
        while (slot < pool.size() && pool[slot] >= 0) ++slot;
        if (slot == pool.size()) pool.push_back(-1);
        pool[slot] = (long)k;
        assigned[k] = pinned_count[out_file[k]] + (uint32_t)slot;
    }
    for (uint32_t k = 0; k < n; ++k) used[out_file[k]] = std::max(used[out_file[k]], assigned[k] + 1u);

    // rewrite: every read names the register its value got, every write its own
    for (uint32_t k = 0; k < n; ++k) {
        Read reads[4];
        int num_reads = 0, file = NONE;
        registers_of(code[k], reads, num_reads, file);
        Read before[4];
        int unused = 0;
        PyrInstr probe = original[k];
        registers_of(probe, before, unused, file);
        for (int r = 0; r < num_reads; ++r) *reads[r].reg = assigned[(size_t)def[reads[r].file][*before[r].reg]];
        code[k].output = assigned[k];
    }
    out.output_reg = assigned[result];
    out.num_numbers = used[NUM];
    out.num_vectors = used[VEC];
    out.num_rgbs = used[RGB];
    return copy_back();
}

} // namespace pyr

extern "C" int pyr_program_allocate_registers(const PyrInstr* instrs, const PyrProgram* program, PyrInstr* instrs_out, PyrProgram* program_out) {
    if (!program || !program_out || (program->kind == PYR_PROGRAM_INSTRUCTIONS && program->num_instrs != 0 && (!instrs || !instrs_out)))
        return PYR_ERR_INVALID_ARGUMENT;
    PyrProgram result;
    try {
        const size_t first = program->kind == PYR_PROGRAM_INSTRUCTIONS ? program->first_instr : 0u;
        const int rc = pyr::allocate_program_registers(instrs + first, *program, instrs_out + first, result);
        if (rc != PYR_OK) return rc;
    } catch (const std::bad_alloc&) {
        return PYR_ERR_OUT_OF_MEMORY;
    }
    *program_out = result;
    return PYR_OK;
}
