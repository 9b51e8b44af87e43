// LDS-resident limb NTT building blocks for gfx950 (design notes: lm_ntt.hip).
//
// v3 structure.  A transform of N = 2^logN coefficients runs in one workgroup of NT = N/16 threads
// (64 <= NT <= 1024), i.e. NW = NT/64 waves, 16 coefficients per lane, as a list of passes of
// R <= 4 butterfly stages; a work item keeps 2^R coefficients in VGPRs for the R stages of a pass.
//   * The CROSS-WAVE pass does log2(NW) stages (the ones whose butterflies span more than N/NW
//     coefficients): it is the first pass of the forward transform, which reads its coefficients
//     straight from global memory through a caller-supplied loader (fusing e.g. an RNS basis
//     extension into the load), and the last pass of the inverse.
//   * Every other stage only touches one block of N/NW = 1024 consecutive coefficients, and each
//     block is owned by ONE wave for the rest of the transform: work items are dealt so that wave j
//     handles block j in every pass.  Those passes exchange coefficients through LDS without
//     workgroup barriers (a wave's LDS operations execute in order), so a transform has ONE
//     s_barrier instead of one per pass and the waves of a CU drift apart -- which is what keeps
//     the VALU fed: a single wave can issue a VALU instruction only every ~8 cycles
//     (profiles/r01_ubench_mad_latency.txt), so each SIMD needs two of its four waves runnable.
//   * The forward transform's last pass hands runs of 8 finished coefficients to a
//     caller-supplied storer (final reduction, rescale combine, ... fused) that writes global memory.
// Multiplications by twiddles are Shoup multiplications written as explicit v_mad_u64_u32 chains
// with the quotient estimate truncated to three partial products: the result is in [0, 3q).
// Twiddles of stages whose block index is wave-uniform are fetched with scalar loads.
//
// This file is the umbrella; each header below holds one subject and compiles on its own.
#pragma once
#include "lm_ntt_plan.h"  // LDS layout, launch geometry, pass plan, ring degrees and dispatchers, launch, split table layout, modulus bound (host / constexpr only)
#include "lm_shoup.h"     // the hand-scheduled Shoup multiplication, lm_bfly_diff, lm_qc
#include "lm_ntt_bfly.h"  // twiddle sets, the lazy butterfly stages, work-item dealing
#include "lm_ntt_fwd.h"   // lm_ntt_forward, lm_lds_runs / lm_linear_out, lm_load_run / lm_store_run
#include "lm_ntt_w14.h"   // lm_ntt_forward_w14: N = 2^14 in registers, two workgroups per CU
#include "lm_ntt_inv.h"   // lm_ntt_inverse
#include "lm_ntt_split.h" // the split degrees: lm_half, the split transforms, lm_ntt_forward_half / lm_ntt_inverse_whole
