// fold_cofold_subopt.hpp -- energy of the second-best co-fold structure of one sequence pair per workgroup on gfx950.
// Replaces get_first_suboptimal_structure_and_energy(seq, fc, 1)[1] on the DIMER fold compound of the reference's
// two-strand -nd on path (utils/energy_scores.py:105-108, :453-488): the lowest energy over all co-fold structures other
// than one ground-state structure (0 if none lies within 49 kcal/mol of the co-fold MFE).
//
// The kernel is the two-strand instance of the K-best programme of fold_subopt.hpp with K = 2: kbest_fill<NT, 2, true> (the
// structure set and the nick rules are derived there) and kbest_exterior<2, true> (Fu / Fc), then E = top2(Fu[n] ; Fc[n] +
// DuplexInit).  C, M, M2 are TopK<2> lists in HBM/L2 (diagonal-major), fcA / fcB (and then Fu / Fc) TopK<2> lists in LDS.
#pragma once
#include "fold_subopt.hpp"

namespace drna {

using CoSubArgs = SuboptArgs;     // (the name this kernel's argument struct had before the family shared one)

struct CoSubSmem : MfeSmemCore<MAXN> {
  // during the sweep: fcA[x] of [x..cut] and fcB[y] of [cut+1..y]; afterwards wave 0 reuses them for Fu / Fc of the
  // exterior loop (the nick loops are all filled by then)
  TopK<2> fcA[MAXN + 3], fcB[MAXN + 3];
};

template <int NT>
__global__ __launch_bounds__(NT) void cofold_subopt_kernel(SuboptArgs A) {
  __shared__ CoSubSmem sm;
  const MfeTables& T = *A.T;
  const int r = blockIdx.x;
  const int n = A.L, cut = A.cut, ld = A.ld;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());
  TopK<2>*C, *M, *M2;
  kb_tables(A, r, C, M, M2);

  stage_energy_tables<NT>(sm, T, tid);
  // row 0 (single nucleotides): no pair, no multiloop content
  TopK<2> none;
  tk_init(none);
  for (int k = tid; k < ld; k += NT) { C[k] = none; M[k] = none; M2[k] = none; }
  for (int k = tid; k <= n + 2; k += NT) { sm.fcA[k] = TopK<2>{{0, INF_DEV}}; sm.fcB[k] = TopK<2>{{0, INF_DEV}}; }   // empty / one-nt segments
  load_sequence<NT>(sm, A.seqs + (long long)r * n, n, tid);
  if (sm.flag) {
    if (tid == 0) second_best_report(A, r, ST_BAD_CHAR, 0, INF_DEV);
    return;
  }
  kbest_fill<NT, 2, true>(sm, A, C, M, M2, lane_id(), wave);
  if (wave != 0) return;
  kbest_exterior<2, true>(sm, T, C, sm.fcA, sm.fcB, n, cut, ld);
  if (tid == 0) {
    TopK<2> f = sm.fcA[n];
    tk_add_sum(f, sm.fcB[n], A.DuplexInit);
    second_best_report(A, r, ST_OK, f.v[0], f.v[1]);
  }
}

}  // namespace drna
