// fold_subopt_lds.hpp -- the second-best folds of fold_subopt.hpp / fold_cofold_subopt.hpp for sequences (or pairs, both strands
// together) of at most SUB_LDS_MAX nucleotides, with the three K = 2 tables of the workgroup in LDS instead of HBM/L2.
//
// The negative-design step (-nd on) folds every SOLVED candidate of an iteration once more, and design targets are short (the
// reference's examples are 35 - 36 nt, its two-strand ones 18 + 18): in the general kernels such a fold is ~35 - 70 diagonals of
// a few cells each, every operand a global load behind a barrier.  Here the same kbest_fill<NT, 2, CO> and kbest_exterior<2, CO>
// (same candidates, same order of minima, same wave_topk butterfly) get C, M and M2 as pointers into shared memory, so E2 and E12
// are the general kernels' bit for bit; only the 1-D arrays and the staged energy tables get a layout of their own, because
// MfeSmemCore<MAXN> sizes its arrays for 2046 nt.
//
// LDS per workgroup (pitch ld = n + 2 like the general kernels, rows 0 .. n - 1):
//   3 tables x TopK<2> x SUB_LDS_MAX x (SUB_LDS_MAX + 2) = 24 x 79 x 81 = 153,576 B
//   staged energy tables 7,680 B, fcA / fcB (one strand: F) 1,312 B, sequence codes and flag 88 B          -> 162,656 B
// of the CU's 163,840 B: one workgroup per CU (a batch of 64 solved candidates is 64 workgroups on 256 CUs).
#pragma once
#include "fold_cofold_subopt.hpp"

namespace drna {

constexpr int SUB_LDS_MAX = 79;                    // longest sequence / pair (both strands, no '&') of the LDS path
constexpr int SUB_LDS_BYTES = 160 * 1024;          // what one workgroup may declare on gfx950

// what kbest_fill / kbest_exterior and the loop energies use of SubSmem / CoSubSmem, sized for NLEN nucleotides
template <int NLEN>
struct SubLdsSmemT {
  int stack[64];
  int mmH[128], mmI[128], mm1n[128], mm23[128], mmM[128], mmExt[128];
  int int11[1024];
  int d5[32], d3[32];
  // two strands: as in CoSubSmem (nick-side decompositions during the sweep, then Fu / Fc); one strand: fcA is F, fcB unused
  TopK<2> fcA[NLEN + 3], fcB[NLEN + 3];
  TopK<2> C[NLEN * (NLEN + 2)], M[NLEN * (NLEN + 2)], M2[NLEN * (NLEN + 2)];
  unsigned char S[NLEN + 4];
  int flag;
};
using SubLdsSmem = SubLdsSmemT<SUB_LDS_MAX>;
static_assert(sizeof(SubLdsSmem) <= SUB_LDS_BYTES, "the second-best tables of SUB_LDS_MAX nucleotides must fit one workgroup's LDS");
static_assert(sizeof(SubLdsSmemT<SUB_LDS_MAX + 1>) > SUB_LDS_BYTES, "SUB_LDS_MAX is the longest sequence that fits");
static_assert(SUB_LDS_MAX >= 64, "every pair of the co-fold LDS path (CO_LDS_MAX, fold_cofold_lds.hpp) gets its second-best fold in LDS, too");

// CO = false: subopt_kernel, CO = true: cofold_subopt_kernel, with the tables in sm, for sequence r (A.L letters at seq).  The
// host launches this for A.L <= SUB_LDS_MAX with the pitch A.ld = A.L + 2 only; anything else leaves at once with the status
// of an internal error
template <int NT, bool CO>
__device__ __forceinline__ void second_best_lds(SubLdsSmem& sm, const SuboptArgs& A, int r, const char* seq) {
  const MfeTables& T = *A.T;
  const int n = A.L, ld = A.ld;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());
  if (n > SUB_LDS_MAX || ld != n + 2) {
    if (tid == 0) second_best_report(A, r, ST_TRACEBACK, 0, INF_DEV);
    return;
  }
  TopK<2>*C = sm.C, *M = sm.M, *M2 = sm.M2;

  stage_energy_tables<NT>(sm, T, tid);
  // the rows below the first diagonal of the sweep: no pair, no multiloop content
  TopK<2> none;
  tk_init(none);
  for (int d = 0; d <= (CO ? 0 : TURN) && d < n; d++)
    for (int k = tid; k < ld; k += NT) { C[d * ld + k] = none; M[d * ld + k] = none; M2[d * ld + k] = none; }
  if constexpr (CO)
    for (int k = tid; k <= n + 2; k += NT) { sm.fcA[k] = TopK<2>{{0, INF_DEV}}; sm.fcB[k] = TopK<2>{{0, INF_DEV}}; }   // empty / one-nt segments
  load_sequence<NT>(sm, seq, n, tid);
  if (sm.flag) {
    if (tid == 0) second_best_report(A, r, ST_BAD_CHAR, 0, INF_DEV);
    return;
  }
  kbest_fill<NT, 2, CO>(sm, A, C, M, M2, lane_id(), wave);
  if (wave != 0) return;
  kbest_exterior<2, CO>(sm, T, C, sm.fcA, CO ? sm.fcB : nullptr, n, CO ? A.cut : 0, ld);
  if (tid == 0) {
    TopK<2> f = sm.fcA[n];
    if constexpr (CO) tk_add_sum(f, sm.fcB[n], A.DuplexInit);
    second_best_report(A, r, ST_OK, f.v[0], f.v[1]);
  }
}

// RAGGED: the instance of the ragged launches; the uniform instance never looks at A.rg
template <int NT, bool RAGGED = false>
__global__ __launch_bounds__(NT) void subopt_lds_kernel(SuboptArgs A) {
  __shared__ SubLdsSmem sm;
  const int r = RAGGED ? A.rg.seq_of(blockIdx.x) : blockIdx.x;
  if (RAGGED && A.rg.len) { A.L = A.rg.len[r]; A.ld = A.L + 2; }     // the workgroup's own length and pitch
  second_best_lds<NT, false>(sm, A, r, A.seqs + (RAGGED ? A.rg.off_of(r, A.L) : (long long)r * A.L));
}

template <int NT>
__global__ __launch_bounds__(NT) void cofold_subopt_lds_kernel(SuboptArgs A) {
  __shared__ SubLdsSmem sm;
  second_best_lds<NT, true>(sm, A, blockIdx.x, A.seqs + (long long)blockIdx.x * A.L);
}

}  // namespace drna
