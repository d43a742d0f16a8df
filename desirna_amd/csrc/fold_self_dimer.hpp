// fold_self_dimer.hpp -- partition function of a sequence folded against a copy of itself (s & s) for one sequence per workgroup
// on gfx950.  Replaces RNA.fold_compound(s + "&" + s).pf_dimer() of the reference's -o on ("avoid" oligomerization,
// utils/energy_scores.py:412-419; utils/dimer_multichain_energy.py:36-50): FA, FcAA and FAA of every candidate.
//
// It is cofold_pf_body (fold_cofold.hpp) on n = 2 L nucleotides with the nick at cut = L -- the same candidates, co_same rules,
// presence flags, per-lane assignment of loop shapes and split points and the same fixed-order wave sums, so a cell holds the
// general kernel's bits -- minus the work and the storage that the two equal strands make redundant:
//   * a cell (i, j) with both ends in the second copy sees the letters, the strand ends and the nick exactly as the cell
//     (i - L, j - L) of the first copy does, so it is never computed and never stored: sd_slot() maps it onto the first copy;
//   * what is left on diagonal d are the cells i = 1 .. min(L, 2 L - d): the monomer cells (j <= L) and the cells that span the
//     nick (i <= L < j), L (L - 1) / 2 + L^2 ~ 1.5 L^2 cells instead of the 2 L^2 of the general sweep;
//   * a table is therefore 1 + L (L - 1) / 2 + L^2 entries: slot 0 (the empty segment, reads 0), the monomer triangle packed by
//     diagonal, the L x L block of nick-spanning cells by (i, j - L).
// The INFO byte of a cell packs the neighbour letters S[i-1] and S[j+1]; every use of them stays under the presence flags
// (h5 / h3 / adj_*) as in the general body, so a cell read through the map at a strand end never contributes a letter that is
// not there.  qA3 / qB5 advance one entry per diagonal as in the general body (qB5[L + k] is the monomer's 5' array), the
// symmetry factor 0.5 is always on.
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

// what self_dimer_pf_body uses of its shared memory, for sequences of at most N nucleotides (1-D arrays over both copies)
template <int N>
struct SdSmemCore {
  double stack[64];
  double mmH[128], mmI[128], mm1n[128], mm23[128], mmM[128], mmExt[128];
  double int11[1024];
  double d5[32], d3[32];
  double q5[2 * N + 2];
  double qA3[2 * N + 3], qB5[2 * N + 3];
  unsigned char S[2 * N + 4];
  int flag;
};

constexpr int SD_LDS_MAX = 62;                 // longest sequence of the LDS path
struct SdLdsSmem : SdSmemCore<SD_LDS_MAX> {
  double QB[sd_cells(SD_LDS_MAX)], QM[sd_cells(SD_LDS_MAX)], QM1[sd_cells(SD_LDS_MAX)];
  unsigned char INFO[sd_cells(SD_LDS_MAX)];
};
static_assert(sizeof(SdLdsSmem) <= 160 * 1024, "SD_LDS_MAX: the tables of the self-dimer no longer fit the CU's LDS");
static_assert(sizeof(SdLdsSmem) + 3 * 8 * (sd_cells(SD_LDS_MAX + 1) - sd_cells(SD_LDS_MAX)) > 160 * 1024,
              "SD_LDS_MAX: one more nucleotide fits the CU's LDS");

using SdSmem = SdSmemCore<MAXN>;               // the workspace kernel: any length the engine takes

// partition function of s & s, s = sequence r (A.L letters), by the calling workgroup; QB, QM, QM1 (doubles) and INFO (bytes)
// of sd_cells(A.L) entries each live where the caller put them (LDS or a workspace slot); A.cut is not read.  F4[r] = FA, FB,
// FcAA, FAA in drna_cofold_batch's layout
template <int NT, class SM>
__device__ __forceinline__ void self_dimer_pf_body(SM& sm, const CoArgs& A, int r, double* QB, double* QM, double* QM1, unsigned char* INFO) {
  const PfTables& T = *A.F;
  const Plan& P = *A.plan;
  const int L = A.L, n = 2 * L, cut = L;
  const int tid = threadIdx.x, lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());
  int32_t* status = A.status_pf;
  auto at = [L](int d, int p) { return sd_slot(d, p, L); };

  stage_energy_tables<NT>(sm, T, tid);
  if (tid == 0) { QM[0] = 0.0; QM1[0] = 0.0; QB[0] = 0.0; INFO[0] = 0; }
  // empty segments, and the one-nucleotide segments next to the nick (the sweep advances these arrays from diagonal 1 on)
  for (int k = tid; k <= n + 2; k += NT) {
    sm.qA3[k] = k == cut ? A.scale[1] : 1.0;
    sm.qB5[k] = k == cut + 1 ? A.scale[1] : 1.0;
  }
  load_sequence<NT>(sm, A.seqs + (long long)r * L, L, tid);          // S[0] = S[L], S[L + 1] = S[1]
  if (sm.flag) {
    if (tid == 0) { status[r] = ST_BAD_CHAR; for (int k = 0; k < 4; k++) A.F4[r * 4 + k] = 0.0; }
    return;
  }
  for (int k = tid + 1; k <= L; k += NT) sm.S[L + k] = sm.S[k];      // the second copy; S[n + 1] = S[1]
  if (tid == 0) sm.S[n + 1] = sm.S[1];
  __syncthreads();
  PfArgs H;                        // for pf_hairpin()
  H.T = A.F; H.plan = A.plan; H.hp_w = A.hp_w; H.scale = A.scale; H.eMLb = A.eMLb; H.seqs = A.seqs; H.L = n; H.ld = 0;
  H.ws = nullptr; H.ws_stride = 0; H.Epf = nullptr; H.status = nullptr;
  const double b1 = A.eMLb[1], sc1 = A.scale[1], sc2 = A.scale[2];

  for (int d = 1; d < n; d++) {
    const int ncell = L < n - d ? L : n - d;          // monomer cells i <= L - d, then the cells that span the nick
    // one wave per cell: the lanes share the interior-loop shapes and the split points; fixed-order wave sums
    for (int i = wave + 1; i <= ncell; i += NT / WAVE) {
      const int j = i + d;
      const bool same = co_same(i, j, cut);
      const int t = (d > TURN || !same) ? pair_type(sm.S[i], sm.S[j]) : 0;
      const double tau = t > 2 ? T.TermAU : 1.0;
      const bool adj_i = co_same(i, i + 1, cut), adj_j = co_same(j - 1, j, cut);
      double qb = 0.0;
      int info = 0;
      if (t) {
        const int si1 = sm.S[i + 1], sj1 = sm.S[j - 1];
        if (same) qb = pf_hairpin(sm, H, i, j, t);
        else qb = sm.qA3[i + 1] * sm.qB5[j - 1] * sc2 * tau * co_pf_endstem(sm.mmExt, sm, rtype_of(t), adj_j, sj1, adj_i, si1);
        double acc = 0.0;
        for (int e = lane; e < NPLAN; e += WAVE) {
          const int u1 = P.tb_u1[e], u2 = P.tb_u2[e];
          const int dp = d - 2 - u1 - u2;
          if (dp < 1) continue;
          const int p = i + 1 + u1, q = j - 1 - u2;
          if (!co_same(i, p, cut) || !co_same(q, j, cut)) continue;
          const int x = at(dp, p);
          const int fi = INFO[x];
          if (!fi) continue;
          acc += QB[x] * co_pf_intloop(sm, T, A.scale, u1, u2, t, si1, sj1, fi);
        }
        double tmp = 0.0;
        if (adj_i && adj_j) {
          for (int k = i + 3 + lane; k <= j - 2; k += WAVE) {
            if (k - 1 == cut) continue;                               // k-1, k must be neighbours
            tmp += QM[at(k - i - 2, i + 1)] * QM1[at(j - 1 - k, k)];
          }
        }
        acc = wave_sum_f64(acc);
        tmp = wave_sum_f64(tmp);
        qb += acc + tmp * T.MLclosing * T.MLintern * tau * sm.mmM[rtype_of(t) * 16 + sj1 * 4 + si1] * sc2;
        info = (rtype_of(t) << 4) | (sm.S[j + 1] << 2) | sm.S[i - 1];
      }
      const bool h5 = i > 1 && co_same(i - 1, i, cut), h3 = j < n && co_same(j, j + 1, cut);
      double m1 = adj_j ? QM1[at(d - 1, i)] * b1 : 0.0;
      if (t) m1 += qb * T.MLintern * tau * co_pf_endstem(sm.mmM, sm, t, h5, sm.S[i - 1], h3, sm.S[j + 1]);
      double m = 0.0;
      for (int k = i + 1 + lane; k <= j - 1; k += WAVE) {
        double left = (k - 1 != cut) ? QM[at(k - 1 - i, i)] : 0.0;
        if (co_same(i, k, cut)) left += A.eMLb[k - i];
        m += left * QM1[at(j - k, k)];
      }
      m = m1 + wave_sum_f64(m);
      if (lane == 0) {
        const int x = at(d, i);
        QB[x] = qb;
        INFO[x] = (unsigned char)info;
        QM1[x] = m1;
        QM[x] = m;
      }
    }
    __syncthreads();
    if (d >= L) continue;                             // both strands' exterior arrays are complete
    if (wave == 0) {
      const int x = cut - d;
      double s = 0.0;
      for (int k = x + 1 + lane; k <= cut; k += WAVE) {
        const int c = at(k - x, x);
        const int fi = INFO[c];
        if (!fi) continue;
        const int t = rtype_of(fi >> 4);
        s += QB[c] * (t > 2 ? T.TermAU : 1.0) * co_pf_endstem(sm.mmExt, sm, t, x > 1, sm.S[x - 1], k < cut, sm.S[k + 1]) * sm.qA3[k + 1];
      }
      s = wave_sum_f64(s);
      sm.qA3[x] = sm.qA3[x + 1] * sc1 + s;
    }
    if (wave == (NT > WAVE ? 1 : 0)) {
      const int y = cut + 1 + d;
      double s = 0.0;
      for (int k = cut + 1 + lane; k < y; k += WAVE) {
        const int c = at(y - k, k);
        const int fi = INFO[c];
        if (!fi) continue;
        const int t = rtype_of(fi >> 4);
        s += sm.qB5[k - 1] * QB[c] * (t > 2 ? T.TermAU : 1.0) * co_pf_endstem(sm.mmExt, sm, t, k > cut + 1, sm.S[k - 1], y < n, sm.S[y + 1]);
      }
      s = wave_sum_f64(s);
      sm.qB5[y] = sm.qB5[y - 1] * sc1 + s;
    }
    __syncthreads();
  }
  if (wave != 0) return;
  sm.q5[0] = 1.0;
  for (int j = 1; j <= n; j++) {
    double s = 0.0;
    for (int i = lane + 1; i < j; i += WAVE) {
      const int c = at(j - i, i);
      const int fi = INFO[c];
      if (!fi) continue;
      const int t = rtype_of(fi >> 4);
      const bool h5 = i > 1 && co_same(i - 1, i, cut), h3 = j < n && co_same(j, j + 1, cut);
      s += sm.q5[i - 1] * QB[c] * (t > 2 ? T.TermAU : 1.0) * co_pf_endstem(sm.mmExt, sm, t, h5, sm.S[i - 1], h3, sm.S[j + 1]);
    }
    s = wave_sum_f64(s);
    sm.q5[j] = sm.q5[j - 1] * sc1 + s;
  }
  if (lane == 0) {
    const double kT = T.kT / 1000.0, lsc = log(T.pf_scale);
    const double Q0 = sm.q5[n];
    double* out = A.F4 + (long long)r * 4;
    if (!(Q0 > 0.0) || !(Q0 < 1.0e300)) {
      status[r] = ST_PF_RANGE;
      for (int k = 0; k < 4; k++) out[k] = 0.0;
    } else {
      // strand partition functions: scale^len when a strand cannot fold at all
      const double QA = sm.qA3[1], QB_ = sm.qB5[n];
      const double QAB = (Q0 - QA * QB_) * A.eDuplexInit * 0.5;        // rotational symmetry of a homodimer
      status[r] = ST_OK;
      out[0] = -kT * (log(QA) + cut * lsc);
      out[1] = -kT * (log(QB_) + (n - cut) * lsc);
      out[2] = QAB > 1e-17 ? -kT * (log(QAB) + n * lsc) : 999.0;
      out[3] = -kT * (log(QA * QB_ + QAB) + n * lsc);
    }
  }
}

// the host launches this for A.L <= SD_LDS_MAX only; a longer sequence leaves at once with the status of an internal error
template <int NT>
__global__ __launch_bounds__(NT) void self_dimer_pf_lds_kernel(CoArgs A) {
  __shared__ SdLdsSmem sm;
  const int r = blockIdx.x;
  if (A.L > SD_LDS_MAX) {
    if (threadIdx.x == 0) A.status_pf[r] = ST_TRACEBACK;
    return;
  }
  self_dimer_pf_body<NT>(sm, A, r, sm.QB, sm.QM, sm.QM1, sm.INFO);
}

// any length: the tables in the sequence's workspace slot (A.wsp, A.wsp_stride >= sd_ws_stride(A.L) doubles)
template <int NT>
__global__ __launch_bounds__(NT) void self_dimer_pf_kernel(CoArgs A) {
  __shared__ SdSmem sm;
  const int r = blockIdx.x;
  double* base = A.wsp + (long long)r * A.wsp_stride;
  const long long tab = sd_cells(A.L);
  self_dimer_pf_body<NT>(sm, A, r, base, base + tab, base + 2 * tab, reinterpret_cast<unsigned char*>(base + 3 * tab));
}

}  // namespace drna
