// fold_self_dimer.hpp -- partition function of a sequence folded against a copy of itself (s & s) for one sequence per workgroup
// on gfx950.  Replaces RNA.fold_compound(s + "&" + s).pf_dimer() of the reference's -o on ("avoid" oligomerization,
// utils/energy_scores.py:412-419; utils/dimer_multichain_energy.py:36-50): FA, FcAA and FAA of every candidate.
//
// Both kernels call cofold_pf_body (fold_cofold.hpp) on n = 2 L nucleotides with the nick at cut = L: the cell, the column steps,
// the q5 sweep and the four free energies exist once, for pairs and self-dimers.  What is this file's own is the layout SdPacked,
// which leaves out the work and the storage that two equal strands make redundant:
//   * a cell (i, j) with both ends in the second copy sees the letters, the strand ends and the nick exactly as the cell
//     (i - L, j - L) of the first copy does, so it is never computed and never stored: sd_slot() maps it onto the first copy;
//   * what is left on diagonal d are the cells i = 1 .. min(L, 2 L - d): the monomer cells (j <= L) and the cells that span the
//     nick (i <= L < j), L (L - 1) / 2 + L^2 ~ 1.5 L^2 cells instead of the 2 L^2 of the square layout;
//   * a table is therefore 1 + L (L - 1) / 2 + L^2 entries: slot 0 (the empty segment, reads 0), the monomer triangle packed by
//     diagonal, the L x L block of nick-spanning cells by (i, j - L);
//   * the L letters are loaded once and doubled in LDS; the symmetry factor 0.5 needs no comparison of the strands.
// The INFO byte of a cell packs the neighbour letters S[i-1] and S[j+1]; the body uses them under the presence flags (h5 / h3 /
// adj_*) only, so a cell read through the map at a strand end never contributes a letter that is not there.  A cell holds the
// bits that cofold_pf_kernel computes for s & s (tests/test_self_dimer_emulated.py compares the bytes).
//
// LDS per workgroup of self_dimer_pf_lds_kernel at SD_LDS_MAX = 62 (the accounting of fold_cofold_lds.hpp):
//   3 fp64 tables + 1 byte table x 5,736 entries = 143,400 B; staged energy tables 15,360 B; q5, qA3, qB5 (2 L + 3 doubles
//   each) 3,048 B; letters and flag 128 B  ->  161,936 B of the CU's 163,840 (63 nt: 166.7 KB).  Packing the triangle is what
//   buys the last 9 nt: with a square monomer table (L^2 + L^2 entries) the bound is 53.
// Longer sequences keep the same tables in a workspace slot (self_dimer_pf_kernel).
#pragma once
#include "fold_cofold.hpp"

namespace drna {

__host__ __device__ constexpr int sd_cells(int L) { return 1 + L * (L - 1) / 2 + L * L; }       // entries of one table
// doubles of a workspace slot: QB, QM, QM1, then the INFO bytes
__host__ __device__ constexpr long long sd_ws_stride(int L) { return 3ll * sd_cells(L) + (sd_cells(L) + 7) / 8; }

// slot of the cell (p, p + d) of s & s, 1 <= p, p + d <= 2 L
__device__ __forceinline__ int sd_slot(int d, int p, int L) {
  if (d <= 0) return 0;                                   // the empty segment
  if (p > L) p -= L;                                      // both ends in the second copy: the first copy's cell
  const int q = p + d;
  if (q <= L) return 1 + (d - 1) * L - ((d - 1) * d >> 1) + (p - 1);
  return 1 + (L * (L - 1) >> 1) + (p - 1) * L + (q - L - 1);
}

// the packed layout of cofold_pf_body for s & s, s of L letters: n = 2 L, the nick at cut = L
struct SdPacked {
  int n, cut;
  static constexpr bool homodimer = true;
  __device__ __forceinline__ int at(int d, int p) const { return sd_slot(d, p, cut); }
  // monomer cells i <= L - d, then the cells that span the nick
  __device__ __forceinline__ int cells(int d) const { return cut < n - d ? cut : n - d; }
  __device__ __forceinline__ int zeros() const { return 1; }
  template <int NT, class SM>
  __device__ __forceinline__ void load(SM& sm, const char* seqs, int r, int tid) const {
    load_sequence<NT>(sm, seqs + (long long)r * cut, cut, tid);       // S[0] = S[L], S[L + 1] = S[1]
    for (int k = tid + 1; k <= cut; k += NT) sm.S[cut + k] = sm.S[k];   // the second copy; S[n + 1] = S[1]
    if (tid == 0) sm.S[n + 1] = sm.S[1];
    __syncthreads();
  }
};

constexpr int SD_LDS_MAX = 62;                 // longest sequence of the LDS path
struct SdLdsSmem : CoPfSmemCore<2 * SD_LDS_MAX> {
  double QB[sd_cells(SD_LDS_MAX)], QM[sd_cells(SD_LDS_MAX)], QM1[sd_cells(SD_LDS_MAX)];
  unsigned char INFO[sd_cells(SD_LDS_MAX)];
};
static_assert(sizeof(SdLdsSmem) <= 160 * 1024, "SD_LDS_MAX: the tables of the self-dimer no longer fit the CU's LDS");
static_assert(sizeof(SdLdsSmem) + 3 * 8 * (sd_cells(SD_LDS_MAX + 1) - sd_cells(SD_LDS_MAX)) > 160 * 1024,
              "SD_LDS_MAX: one more nucleotide fits the CU's LDS");

using SdSmem = CoPfSmemCore<2 * MAXN>;         // the workspace kernel: any length the engine takes

// Both kernels: partition function of s & s, s = sequence r (A.L letters), by one workgroup; A.cut is not read.  F4[r] = FA, FB,
// FcAA, FAA in drna_cofold_batch's layout.
// the host launches this for A.L <= SD_LDS_MAX only; a longer sequence leaves at once with the status of an internal error
template <int NT>
__global__ __launch_bounds__(NT) void self_dimer_pf_lds_kernel(CoArgs A) {
  __shared__ SdLdsSmem sm;
  const int r = blockIdx.x;
  if (A.L > SD_LDS_MAX) {
    if (threadIdx.x == 0) A.status_pf[r] = ST_TRACEBACK;
    return;
  }
  cofold_pf_body<NT>(sm, A, r, sm.QB, sm.QM, sm.QM1, sm.INFO, SdPacked{2 * A.L, A.L});
}

// any length: the tables in the sequence's workspace slot (A.wsp, A.wsp_stride >= sd_ws_stride(A.L) doubles)
template <int NT>
__global__ __launch_bounds__(NT) void self_dimer_pf_kernel(CoArgs A) {
  __shared__ SdSmem sm;
  const int r = blockIdx.x;
  double* base = A.wsp + (long long)r * A.wsp_stride;
  const long long tab = sd_cells(A.L);
  cofold_pf_body<NT>(sm, A, r, base, base + tab, base + 2 * tab, reinterpret_cast<unsigned char*>(base + 3 * tab), SdPacked{2 * A.L, A.L});
}

}  // namespace drna
