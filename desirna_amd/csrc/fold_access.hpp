// fold_access.hpp -- partition function with positions held unpaired (drna_pf_unpaired_batch): the free energy F[mask] of the
// ensemble in which every masked nucleotide stays unpaired.  Eopen = F[mask] - F is the opening energy of the masked region and
// exp(-Eopen / kT) the probability that the region is free.
//
// A fold is a (sequence, mask) pair: workgroup b folds pair g = fold0 + b, i.e. sequence g / M under mask g % M, and leaves
// its result in slot b.  The mask becomes pairing codes Sp (4 = must stay unpaired, the code of the MFE kernels' pseudoknot
// re-folds); only pairability reads them.  A masked nucleotide is still that nucleotide next to a pair: mismatches, dangles, the
// special hairpins and the small-loop tables keep reading the letters S.
//
// Two bodies: the general one is pf_kernel<NT, true> (fold_pf.hpp, tables in a workspace slot, any length); the one here keeps
// QB, QM, QM1 and INFO in LDS on the packed triangle CoTri, as the one-strand instance of edef_lds_kernel does (cut = n: the
// empty second strand, under which cofold_pf_body IS the one-strand recursion), for sequences of at most ACCESS_LDS_MAX nt.
#pragma once
#include "fold_edef_lds.hpp"
#include "fold_pf.hpp"

namespace drna {

// CoTri whose load() also writes the pairing codes sm.Sp[0 .. n + 1] from a mask of n bytes (both wrap ends 4)
struct CoTriMasked : CoTri {
  const unsigned char* mask;
  template <int NT, class SM>
  __device__ __forceinline__ void load(SM& sm, const char* seqs, int r, int tid) const {
    load_sequence<NT>(sm, seqs + off, n, tid);
    for (int k = tid; k <= n + 1; k += NT) sm.Sp[k] = k >= 1 && k <= n && !mask[k - 1] ? sm.S[k] : 4;
    __syncthreads();
  }
};

// longest sequence whose three fp64 tables and INFO (25 B per entry of the triangle) fit the CU's LDS beside the staged energy
// tables and the columns: 162,728 B of 163,840 at 108 nt, 165,456 B at 109
constexpr int ACCESS_LDS_MAX = 108;
// What the host sends to the LDS kernel (option "access_lds_max").  Its body is one wave per cell; pf_kernel<NT, true> splits a
// diagonal's work over all waves.  Measured on the MI355X at R = 64, M = 1, device events, medians of eight alternating rounds
// after a warm-up (spread of a figure: +-1 %), LDS kernel against general kernel, ms (profiles/access.json):
//   24 nt 0.124 / 0.193    36 nt 0.279 / 0.309    48 nt 0.500 / 0.434    64 nt 0.859 / 0.587    80 nt 1.359 / 0.746    108 nt 2.520 / 1.044
// It wins up to 36 nt and loses from 48 nt on; nothing was measured in between, so the bound is the last length at which it won.
constexpr int ACCESS_LDS_HOST_MAX = 36;
static_assert(ACCESS_LDS_HOST_MAX <= ACCESS_LDS_MAX, "the host bound is within the kernel's");

template <int N>
struct AccessLdsSmem : CoPfSmemCore<N> {
  unsigned char Sp[N + 4];
  double tab[3][tri_cells(N)];                 // QB, QM, QM1
  unsigned char INFO[tri_cells(N)];
};
static_assert(sizeof(AccessLdsSmem<ACCESS_LDS_MAX>) <= 160 * 1024, "ACCESS_LDS_MAX: the tables of a sequence no longer fit the CU's LDS");
static_assert(sizeof(AccessLdsSmem<ACCESS_LDS_MAX + 1>) > 160 * 1024, "ACCESS_LDS_MAX: one more nucleotide fits the CU's LDS");

// in: cofold_pf_body's arguments -- seqs: the letters of sequence seq0 first; status_pf by slot; F4: 4 doubles per slot, of which
// F4[0], the strand's own free energy (kcal/mol; from qA3[1], the whole sequence), is F[mask]; cut, ld and wsp are not read
struct AccessLdsArgs {
  CoArgs in;
  const unsigned char* nopair = nullptr;       // M x L bytes, non-zero = the position stays unpaired
  int M = 1;
  int fold0 = 0;                               // the (sequence, mask) pair of workgroup 0
  int seq0 = 0;                                // the sequence whose letters stand first in in.seqs
};

// a length above ACCESS_LDS_MAX leaves at once with the status of an internal error (the host never sends one)
template <int NT>
__global__ __launch_bounds__(NT) void access_lds_kernel(AccessLdsArgs A) {
  __shared__ AccessLdsSmem<ACCESS_LDS_MAX> sm;
  const int b = blockIdx.x, n = A.in.L;
  if (n > ACCESS_LDS_MAX) {
    if (threadIdx.x == 0) { A.in.status_pf[b] = ST_TRACEBACK; A.in.F4[(long long)b * 4] = 0.0; }
    return;
  }
  const int g = A.fold0 + b;
  CoTriMasked lay;
  lay.n = n; lay.cut = n; lay.off = (long long)(g / A.M - A.seq0) * n;
  lay.mask = A.nopair + (long long)(g % A.M) * n;
  A.in.cut = n;
  cofold_pf_body<NT, true>(sm, A.in, b, sm.tab[0], sm.tab[1], sm.tab[2], sm.INFO, lay);
}

}  // namespace drna
