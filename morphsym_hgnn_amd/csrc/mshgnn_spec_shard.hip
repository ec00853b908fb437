// One shard of the bf16 plan's compile-time programs: compiled with -DMSHGNN_SPEC_SHARD=k (csrc/Makefile: k = 1..7), this translation unit instantiates the slab kernels
// over program k (MSHGNN_SPEC_LIST_<k>, mshgnn_spec_tables.inc) and defines its selector spec_shard<k>, which mshgnn.hip asks for a plan's kernels.
#include "mshgnn_slab.hpp"
#include "mshgnn_pick.hpp"
#ifndef MSHGNN_SPEC_SHARD
#error "compile with -DMSHGNN_SPEC_SHARD=<k>: the program list this unit instantiates (csrc/Makefile)"
#endif
#if MSHGNN_SPEC_SHARD == 99
// Shard 99 is not part of the library: it is this source compiled AFTER the build, for one plan's own tables (morphsym_hgnn_amd/jit.py renders them as MSHGNN_JIT_TABLES -- a
// struct spec::JIT_<hash> and MSHGNN_SPEC_LIST_99 -- and compiles a small shared library of the program's kernels), for topologies the build has no program for.  The library
// takes its selector through mshgnn_plan_attach_program and checks the tables like every shard does.
#include MSHGNN_JIT_TABLES
#endif
// the program's launch table, row i the kernel of pick::SpecForm i (which forms exist, and why: pick::spec_form, mshgnn_pick.hpp)
template <class SP> static constexpr StackKernel SPEC_TABLE[pick::SPEC_FORMS] = {
    k_slab_step<__bf16, SP::NM, SP::HB, SP, 0>, k_slab_step<__bf16, SP::NM, SP::HB, SP, 1>, k_slab_step<__bf16, SP::NM, SP::HB, SP, 0, false>,
    k_slab_fwd_spec<__bf16, SP::NM, SP::HB, SP, 0, 0>, k_slab_fwd_spec<__bf16, SP::NM, SP::HB, SP, 0, 0, false>,
    k_slab_fwd_spec<__bf16, SP::NM, SP::HB, SP, 1, 0>, k_slab_fwd_spec<__bf16, SP::NM, SP::HB, SP, 1, 1>,
    k_slab_bwd_spec<__bf16, SP::NM, SP::HB, SP, 0>, k_slab_bwd_spec<__bf16, SP::NM, SP::HB, SP, 1>};
#define MSHGNN_SPEC_TRY(SP) if (spec_matches<SP>(hp)) { if (name) *name = #SP; return form >= 0 && form < pick::SPEC_FORMS ? SPEC_TABLE<SP>[form] : nullptr; }
StackKernel SPEC_CAT(spec_shard, MSHGNN_SPEC_SHARD)(const HostPlan& hp, int form, const char** name) { SPEC_CAT(MSHGNN_SPEC_LIST_, MSHGNN_SPEC_SHARD)(MSHGNN_SPEC_TRY) return nullptr; }
#if MSHGNN_SPEC_SHARD == 99
extern "C" StackKernel mshgnn_jit_program(const HostPlan& hp, int form, const char** name) { return spec_shard99(hp, form, name); }
#endif
#undef MSHGNN_SPEC_TRY
