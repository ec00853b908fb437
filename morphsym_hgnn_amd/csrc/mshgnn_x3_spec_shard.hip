// One shard of the split plan's compile-time programs (see mshgnn_spec_shard.hip): compiled with -DMSHGNN_SPEC_SHARD=k, this translation unit instantiates the split plan's
// 8-wave stack kernels over program k (MSHGNN_SPEC_X3_LIST_<k>, mshgnn_spec_tables.inc) and defines its selector x3_spec_shard<k>, which mshgnn_x3.hip asks for a plan's kernels.
#include "mshgnn_x3_stack.hpp"
#include "mshgnn_pick.hpp"
#ifndef MSHGNN_SPEC_SHARD
#error "compile with -DMSHGNN_SPEC_SHARD=<k>: the program list this unit instantiates (csrc/Makefile)"
#endif
#if MSHGNN_SPEC_SHARD == 99      // a program compiled for one plan after the build (morphsym_hgnn_amd/jit.py; see shard 99 of mshgnn_spec_shard.hip)
#include MSHGNN_JIT_TABLES
#endif
// the program's launch table, row i the kernel of pick::SpecFormX3 i
template <class SP> static constexpr StackKernelX3 X3_SPEC_TABLE[pick::SPEC_FORMS_X3] = {k_stack_step_x3<SP::ALIAS != 0, SP>, k_stack_fwd_x3_spec<SP::ALIAS != 0, SP>, k_stack_bwd_x3_spec<SP>};
#define MSHGNN_SPEC_TRY(SP) if (spec_matches_x3<SP>(hp)) { if (name) *name = #SP; return form >= 0 && form < pick::SPEC_FORMS_X3 ? X3_SPEC_TABLE<SP>[form] : nullptr; }
StackKernelX3 SPEC_CAT(x3_spec_shard, MSHGNN_SPEC_SHARD)(const HostPlan& hp, int form, const char** name) { SPEC_CAT(MSHGNN_SPEC_X3_LIST_, MSHGNN_SPEC_SHARD)(MSHGNN_SPEC_TRY) return nullptr; }
#if MSHGNN_SPEC_SHARD == 99
extern "C" StackKernelX3 mshgnn_jit_program_x3(const HostPlan& hp, int form, const char** name) { return x3_spec_shard99(hp, form, name); }
#endif
#undef MSHGNN_SPEC_TRY
