// fold_edef_lds.hpp -- ensemble defect (-sf Edef) of short designs in ONE launch: the inside sweep (cofold_pf_body, fold_cofold.hpp)
// and the outside sweep, probabilities and defect (cofold_outside_body, fold_cofold_outside.hpp) of one sequence or sequence pair
// per workgroup on gfx950, on tables that never leave LDS.  Replaces, for designs of at most EDEF_LDS_MAX / CO_EDEF_LDS_MAX
// nucleotides, the two launches of the general kernels (pf_kernel + outside_kernel, cofold_pf_kernel + cofold_outside_kernel),
// whose tables live in a workspace slot: ~70 diagonals twice, every operand an L2 load behind a barrier.
//
// One kernel family serves both strand counts.  Two strands run the two bodies as the general kernels do, so edef and every
// probability are theirs bit for bit.  One strand is the instance with an empty second strand (cut = n): under the co-fold rules
// every neighbour test then holds and nothing joins, which IS the one-strand recursion (tests/test_edef_lds_emulated.py checks it
// against the oracle); the compile-time flag ONE of the outside body drops the tables and terms that could only repeat the full
// weights.  Its order of summation is this family's, not outside_kernel's: one-strand values differ from the general path in the
// last bits (both within EDEF_TOL = 1e-10 of the oracle).
//
// Layout CoTri: the cells (p, p + d), 1 <= d < n, packed by diagonal -- n (n - 1) / 2 entries and slot 0 for the empty segment,
// half of what the square pitch-(n + 2) tables of fold_cofold_lds.hpp take (they store the cells with i > j, too).
//
// LDS per workgroup (the static_asserts below decide the bounds):
//   two strands, CO_EDEF_LDS_MAX = 57: 11 fp64 tables + INFO x 1,597 entries = 142,133 B; staged energy tables 15,360 B; the
//     columns q5, qA3, qB5, q3, H, Hb 2,864 B; letters and flag  ->  160,424 B of the CU's 163,840 (58 nt: 165,544 B)
//   one strand, EDEF_LDS_MAX = 71: 7 fp64 tables + INFO x 2,486 entries = 141,702 B + 15,360 B + columns  ->  160,096 B
//     (72 nt: 164,184 B)
// Every example input of the reference is 35 or 36 nt (17 + 18 for two strands), so all of them take this path.
#pragma once
#include "fold_cofold_outside.hpp"

namespace drna {

__host__ __device__ constexpr int tri_cells(int n) { return 1 + n * (n - 1) / 2; }       // entries of one packed table

// the packed triangle of cofold_pf_body / cofold_outside_body: n nucleotides in all, the first strand cut long
struct CoTri {
  int n, cut;
  long long off;                                 // of the letters in the sequence buffer (uniform batch: r * n)
  static constexpr bool homodimer = false;
  __device__ __forceinline__ int at(int d, int p) const {
    return d <= 0 ? 0 : 1 + (d - 1) * n - ((d - 1) * d >> 1) + (p - 1);     // slot 0: the empty segment
  }
  __device__ __forceinline__ int cells(int d) const { return n - d; }
  __device__ __forceinline__ int zeros() const { return 1; }
  template <int NT, class SM>
  __device__ __forceinline__ void load(SM& sm, const char* seqs, int r, int tid) const {
    load_sequence<NT>(sm, seqs + off, n, tid);
  }
};

constexpr int CO_EDEF_LDS_MAX = 57;            // longest pair (both strands, no '&') of the fused kernel
constexpr int EDEF_LDS_MAX = 71;               // longest single sequence the kernel holds
// One strand competes with pf_kernel + outside_kernel, which split a diagonal's work over all waves instead of one wave per cell:
// measured on the MI355X at R = 64 the fused kernel wins up to 40 nt (36 nt: 0.619 against 0.719 ms, 40 nt: 0.771 against 0.804)
// and loses from 44 nt on (0.921 against 0.895; 71 nt: 2.32 against 1.53), so the host sends it sequences up to this length only.
// Pairs win over the whole range (18 + 18: 0.599 against 0.671 ms, 28 + 29: 1.506 against 1.720): their host bound is the kernel's.
constexpr int EDEF_LDS_HOST_MAX = 40;
static_assert(EDEF_LDS_HOST_MAX <= EDEF_LDS_MAX && EDEF_LDS_HOST_MAX >= 36, "the reference's 36-nt examples take the fused kernel");

template <int N, bool ONE>
struct EdefLdsSmem : CoPfSmemCore<N> {
  static constexpr int TABLES = ONE ? 7 : 11;  // QB, QM, QM1, OB, AT, OM, OM1 (+ OBU, ATU, OMU, OM1U)
  double q3[N + 3];
  double H[ONE ? 1 : N + 2], Hb[N + 2];
  double tab[TABLES][tri_cells(N)];
  unsigned char INFO[tri_cells(N)];
};
static_assert(sizeof(EdefLdsSmem<CO_EDEF_LDS_MAX, false>) <= 160 * 1024, "CO_EDEF_LDS_MAX: the tables of a pair no longer fit the CU's LDS");
static_assert(sizeof(EdefLdsSmem<CO_EDEF_LDS_MAX + 1, false>) > 160 * 1024, "CO_EDEF_LDS_MAX: one more nucleotide fits the CU's LDS");
static_assert(sizeof(EdefLdsSmem<EDEF_LDS_MAX, true>) <= 160 * 1024, "EDEF_LDS_MAX: the tables of a sequence no longer fit the CU's LDS");
static_assert(sizeof(EdefLdsSmem<EDEF_LDS_MAX + 1, true>) > 160 * 1024, "EDEF_LDS_MAX: one more nucleotide fits the CU's LDS");

// in: the inside sweep's arguments (wsp unused; F4: 4 doubles per sequence, meaningless for one strand; status_pf), out: the
// outside sweep's (wsp / wu unused; the same status_pf).  ONE: in.cut = in.L.
// One strand only: a ragged batch (drna_ensemble_defect_ragged) -- workgroup b folds sequence rg.idx[b] of its own length, its
// letters at rg.off, against its own structure (pair tables of drna_set_targets_ragged in out.pt, that of sequence r at
// pt_off[target_of[r]]); edef and the status word go to the sequence's position.  All null: the uniform batch.
struct EdefLdsArgs {
  CoArgs in;
  CoOutArgs out;
  Ragged rg;
  const int* target_of = nullptr;
  const int* pt_off = nullptr;
};

// the host launches this for lengths <= the bound only (one strand: <= EDEF_LDS_HOST_MAX); a longer one leaves at once with the status of an internal error
// RAGGED (one strand only): the instance of the ragged launches; the uniform instances never look at the descriptors
template <int NT, bool ONE, bool RAGGED = false>
__global__ __launch_bounds__(NT) void edef_lds_kernel(EdefLdsArgs A) {
  static_assert(ONE || !RAGGED, "no ragged pairs");
  constexpr int N = ONE ? EDEF_LDS_MAX : CO_EDEF_LDS_MAX;
  constexpr int TAB_U = ONE ? 0 : 7;             // the first of the four tables without joining pairs (one strand: none)
  __shared__ EdefLdsSmem<N, ONE> sm;
  const int r = RAGGED ? A.rg.seq_of(blockIdx.x) : blockIdx.x;
  const int n = RAGGED ? A.rg.len_of(r, A.in.L) : A.in.L, cut = ONE ? n : A.in.cut;
  if (n > N) {
    if (threadIdx.x == 0) { A.in.status_pf[r] = ST_TRACEBACK; A.out.edef[r] = 0.0; }
    return;
  }
  const CoTri lay{n, cut, RAGGED ? A.rg.off_of(r, n) : (long long)r * n};
  if (RAGGED && A.target_of) A.out.pt += A.pt_off[A.target_of[r]];
  cofold_pf_body<NT>(sm, A.in, r, sm.tab[0], sm.tab[1], sm.tab[2], sm.INFO, lay);
  __syncthreads();                               // wave 0 finished q5 and the status word; a bad letter left every wave early
  const CoOutTables tb{sm.tab[0], sm.tab[1], sm.tab[2], sm.INFO, sm.tab[3], sm.tab[4], sm.tab[5], sm.tab[6],
                       ONE ? nullptr : sm.tab[TAB_U], ONE ? nullptr : sm.tab[TAB_U + 1], ONE ? nullptr : sm.tab[TAB_U + 2],
                       ONE ? nullptr : sm.tab[TAB_U + 3], ONE ? nullptr : sm.H, sm.Hb};
  cofold_outside_body<NT, ONE, true>(sm, A.out, r, tb, lay);
}

}  // namespace drna
