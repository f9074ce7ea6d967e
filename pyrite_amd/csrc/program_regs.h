// program_regs.h -- register allocation for material programs that declare more registers than the interpreter's in-register
// file holds (include/pyrite_gpu.h PYR_MAX_*_REGISTERS). Host only: no HIP.
//
// Both front ends give every value of a program a register of its own (compiler.rs next_reg), so a program of a few dozen
// instructions declares a few dozen registers although only a handful of values are ever live at once. This pass renumbers the
// registers of such a program by linear scan over its straight-line code, one pool per file (number, vector, RGB). Nothing but
// register indices and the three counts change: the same instructions in the same order, with the same ops, deps, constants
// and inputs.
//
// The kernels run a program in full for the hero wavelength and then, for every companion wavelength, re-run only the
// instructions whose deps carry PYR_DEP_WAVELENGTH (kernels.hip contribute_pending, the reference's memoised re-run). For the
// re-run to reproduce a full run, a value that does not depend on the wavelength but is read by an instruction that does -- and
// the program's output, when it does not depend on the wavelength -- keeps a register of its own for the whole program.
#pragma once
#include <cstdint>

#include "../../include/pyrite_gpu.h"

namespace pyr {

// Does `p` fit the in-register file (16 numbers, 8 vectors, 8 RGBs)? A program that fits is never renumbered.
bool program_fits_registers(const PyrProgram& p);
// ... or the wide interpreter build's file (PYR_WIDE_*_REGISTERS)?
bool program_fits_wide_registers(const PyrProgram& p);

// Reads the program's p.num_instrs instructions from `instrs` (its first instruction, not the scene's array), writes as many to
// `instrs_out` (which may be `instrs` itself) and `out` (a copy of p with output_reg and the counts renumbered). A program that fits the
// in-register file, a constant program, and one the pass cannot follow -- a register written twice, read before it is written or
// beyond its declared count, an unknown opcode or value type -- are copied unchanged. PYR_OK, or PYR_ERR_UNSUPPORTED (nothing
// written) when p declares more than PYR_MAX_DECLARED_REGISTERS registers of a file.
int allocate_program_registers(const PyrInstr* instrs, const PyrProgram& p, PyrInstr* instrs_out, PyrProgram& out);

} // namespace pyr
