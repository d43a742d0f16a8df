// fold_cofold_lds.hpp -- two interacting strands of at most CO_LDS_MAX nucleotides in all: the co-fold MFE (fill + traceback)
// and partition function of fold_cofold.hpp with every 2-D table of the workgroup in LDS instead of HBM/L2.
//
// Design pairs are short (the reference's two-strand examples are 18 + 18 nt), so the general kernels spend their diagonals
// waiting for L2: ~70 diagonals of a few cells each, every operand a global load behind a barrier.  Here cofold_mfe_body and
// cofold_pf_body are handed tables in LDS (the partition function in the square layout CoSquare with pitch n + 2), so the
// results are the general kernels' bit for bit.  The 1-D arrays and the staged energy tables are sized for CO_LDS_MAX
// (MfeSmemCore<CO_LDS_MAX>, CoPfSmemCore<CO_LDS_MAX>) instead of the 2046 nt of the general kernels' structs.
//
// LDS per workgroup at CO_LDS_MAX = 64 (pitch ld = n + 2 <= 66, n + 1 rows):
//   MFE  3 int32 tables x 66 x 66 = 52,272 B + staged tables and 1-D arrays  9,5 KB  ->  ~61 KB
//   PF   3 fp64 tables + 1 byte table x 66 x 66 = 108,900 B + staged tables 15.9 KB   -> ~125 KB of the CU's 160 KB
// so one partition-function workgroup per CU; a batch of 64 pairs is 128 workgroups on 256 CUs either way.
#pragma once
#include "fold_cofold.hpp"

namespace drna {

constexpr int CO_LDS_MAX = 64;                 // longest pair (both strands, no '&') of the LDS path
constexpr int CO_LDS_LD = CO_LDS_MAX + 2;      // largest pitch; a pair of n nucleotides uses pitch n + 2 like the general kernels

struct CoLdsMfeSmem : MfeSmemCore<CO_LDS_MAX> {
  int fcA[CO_LDS_MAX + 3], fcB[CO_LDS_MAX + 3];
  int32_t Wc[CO_LDS_LD * CO_LDS_LD], FML[CO_LDS_LD * CO_LDS_LD], EXT[CO_LDS_LD * CO_LDS_LD];
};

struct CoLdsPfSmem : CoPfSmemCore<CO_LDS_MAX> {
  double QB[CO_LDS_LD * CO_LDS_LD], QM[CO_LDS_LD * CO_LDS_LD], QM1[CO_LDS_LD * CO_LDS_LD];
  unsigned char INFO[CO_LDS_LD * CO_LDS_LD];
};

// the host launches these for A.L <= CO_LDS_MAX only; a longer pair leaves at once with the status of an internal error
template <int NT>
__global__ __launch_bounds__(NT) void cofold_mfe_lds_kernel(CoArgs A) {
  __shared__ CoLdsMfeSmem sm;
  const int r = blockIdx.x;
  if (A.L > CO_LDS_MAX) {
    if (threadIdx.x == 0) { A.status[r] = ST_TRACEBACK; A.Emfe[r] = 0; }
    return;
  }
  cofold_mfe_body<NT>(sm, A, r, sm.Wc, sm.FML, sm.EXT, A.L + 2);
}

template <int NT>
__global__ __launch_bounds__(NT) void cofold_pf_lds_kernel(CoArgs A) {
  __shared__ CoLdsPfSmem sm;
  const int r = blockIdx.x;
  if (A.L > CO_LDS_MAX) {
    if (threadIdx.x == 0) A.status_pf[r] = ST_TRACEBACK;
    return;
  }
  cofold_pf_body<NT>(sm, A, r, sm.QB, sm.QM, sm.QM1, sm.INFO, CoSquare{A.L, A.cut, A.L + 2});
}

}  // namespace drna
