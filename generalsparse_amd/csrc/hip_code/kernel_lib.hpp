// hip_code/kernel_lib.hpp -- hand-written gfx950 (MI355X, CDNA4) SpMM kernel families.
//
// Replaces cuda_code/kernel_lib.hpp of the reference (Load()/__ldg helpers,
// kernel_lib.hpp:1006-1148) and the kernels its reduction tokens print
// (SURVEY.md §2.2 K1-K7).  C = A * B, B row-major K x N, C row-major M x N.
// Written for 64-lane waves: a wave is split into S = 64/X "slots" of X column
// lanes; every lane owns CF consecutive dense columns (one 16-byte load of a B
// row segment when CF*sizeof(VT) == 16).  A (cols/vals) is streamed once,
// vector-loaded; B rows are gathered through L1/L2 (B is small and shared).
// Accumulation is always fp32 (the reference accumulates fp16 in half).
//
// This file is the umbrella: the emitted programs include it and get every family.  Each
// family is defined in a header of its own, which the engine's launch files (kernels/*.hip)
// include directly.
//
// Families (selected by code_generator::compile from the reduction tokens):
//   gather.hpp:
//   k_thread_total   K1: X lanes per BMT row, rows sorted + col-padded (SCF-aligned)
//   k_warp_rows      K4: one wave per BMW, nnz split over S slots, xor-shuffle reduce
//                       (+ optional BMTB grouping = one workgroup per BMTB)
//   k_block_rows     K6: one 256-thread workgroup per BMTB, wave reduce + LDS reduce
//   k_bitmap_segment K2+K3: fixed 32-nnz BMTs, row segments from bitmaps, open
//                       head/tail partials combined per wave, then atomics
//   k_row_chunks     K5/K7: col-direction BMTs (chunks of one row), segmented
//                       slot tree + a row carry per wave
//   parts.hpp:
//   k_combine_parts, k_add_parts, k_finalize_rows  element-wise companions of the above
//   k_epilogue, k_tm_in, k_tm_out  the epilogue post-pass; the transposes around a plan's SpMM (gs_linear)
//   lds_rows.hpp:
//   k_lds_rows[_dma,_rs] K4 with B chunks staged in LDS, one workgroup per BMTB
//   mfma_rows.hpp:
//   k_mfma_rows      BMTB row blocks on the matrix cores, one workgroup per row block
//   mfma_ks.hpp:
//   k_mfma_ks[_group] the same with K split over workgroups
//   mfma_ks_tm.hpp:
//   k_mfma_ks_tm     a k_mfma_ks plan on token-major activations (gs_linear: Y = X * A^T)
//   sddmm.hpp:
//   k_sddmm_tm       the sampled product G^T * X at a plan's pattern, token-major operands (gs_sddmm)
//   set_values.hpp:
//   k_set_values     an uploaded k_mfma_ks plan's values rewritten in place from a device array (gs_plan_set_values)
//   nm_mfma.hpp:
//   k_nm_mfma        2:4 panels on the sparse matrix cores
//   merge_path.hpp:
//   k_merge_path     merge-path levels (+ k_permute_rows, k_merge_fixup)
//   experiments build only: k_mfma_kb, k_mfma_bm, k_mfma_bm2: mfma_bm_exp.hpp;
//                       k_nm_mfma_ks, k_nm_mfma4: nm_mfma_exp.hpp
// kernel_common.hpp: what the families share; host_layouts.hpp: the host-only gsk_host helpers
#pragma once

#include "kernel_common.hpp"

#include "gather.hpp"
#include "parts.hpp"
#include "lds_rows.hpp"
#include "mfma_rows.hpp"
#include "mfma_ks.hpp"
#include "mfma_ks_tm.hpp"
#include "sddmm.hpp"
#include "set_values.hpp"
#include "nm_mfma.hpp"
#include "merge_path.hpp"
#ifdef GS_EXPERIMENTS  // opt-in kernels measured slower than the default ones
#include "mfma_bm_exp.hpp"
#include "nm_mfma_exp.hpp"
#endif

#include "host_layouts.hpp"
