// fold_cofold_outside.hpp -- outside recursion, pair probabilities and ensemble defect of two interacting strands, one
// sequence pair per workgroup on gfx950: two-strand -sf Edef.  The reference calls get_ensemble_defect whatever
// the oligo_state (utils/energy_scores.py:93-94, :362-374) but pins no value for two strands; the definition is DESIGN 3.5's:
// the ensemble is cofold_pf_kernel's (fold_cofold.hpp), a structure weighs its Boltzmann factor times kappa if a pair joins the
// strands (kappa = expDuplexInit, halved for two equal strands), so that the weights sum to exp(-FAB / kT).
//
// Runs after cofold_pf_kernel on the tables that kernel left in the workspace (QB, QM, QM1, INFO, diagonal-major); the 1-D
// columns q5, qA3, qB5 are rebuilt here by that kernel's own column functions (four waves side by side, with the suffix column
// q3), so cofold_pf_kernel need not keep them.  Like outside_kernel (fold_outside.hpp) the weights are GATHERED: diagonals
// n-1 ... 1, a cell pulls from finished cells of larger span, every fp64 sum has one writer and a fixed order.  Like
// cofold_pf_kernel one wave works one cell, the lanes share the 496 interior-loop shapes and the split points.
// The sweep is cofold_outside_body, which takes its tables and their layout from the caller like cofold_pf_body:
// cofold_outside_kernel hands it the workspace slot (CoSquare), fold_edef_lds.hpp tables in LDS right after the inside sweep.
//
// Outside weights under the co-fold rules (x ~ y: x and y = x+1 are neighbours on one strand):
//   A[i,j]   = Om[i,j] + CL[i-1,j+1] (i-1 ~ i, j ~ j+1)            weight of the split products sum_k qm[i,k-1] qm1[k,j]
//   Om[i,j]  = sum_{j''>j} A[i,j''] qm1[j+1,j'']  (j ~ j+1, else 0)
//   Om1[i,j] = Om[i,j] + sum_{i'<i} ( A[i',j] qm[i',i-1] (i-1 ~ i) + Om[i',j] b^(i-i') (i'..i on one strand) )
//              + Om1[i,j+1] b (j ~ j+1)
//   Ob[i,j]  = Om1[i,j] MLstem(i,j) + q5[i-1] q3[j+1] Ext(i,j) + sum_{(p,q) encloses, stretches on one strand} Ob[p,q] IntLoop
//              + N[i,j]
//   CL[p,q]  = Ob[p,q] MLclosing MLstem(q,p) scale^2
// N is the loop that holds the nick, seen from a stem inside it.  A joining pair (p,q) closes the exterior-like segments
// [p+1..cut] and [cut+1..q-1] with the factor K(p,q) that cofold_pf_kernel puts on qA3[p+1] qB5[q-1].  For (i,j) on strand A
//   N[i,j] = H[i] Ext(i,j) qA3[j+1],   G[p] = sum_{q>cut} Ob[p,q] K(p,q) qB5[q-1],
//   H[x]   = G[x-1] + H[x-1] scale + sum_{k<x-1} H[k] qb[k,x-1] Ext(k,x-1)
// (H[x] = sum_p G[p] x partition function of the exterior-like prefix [p+1..x-1]); every (p,q) in H[x] lies on a diagonal
// >= cut-x+2, so H gains one entry per diagonal, the mirror image of how the inside sweep advances qA3.  Strand B: Hb[y] from
// Gb[q] = sum_{p<=cut} Ob[p,q] K(p,q) qA3[p+1], backwards.  H / Hb live in LDS like qA3 / qB5.
//
// kappa belongs to the connected structures only.  Cells inside a strand therefore carry a second set of weights (the *U
// tables) that leaves out every contribution of a joining pair: the one-strand outside weights of that strand times the other
// strand's partition function.  P = [kappa (W - Wu) + Wu] / Q inside a strand, kappa W / Q for a joining pair.
#pragma once
#include "fold_cofold.hpp"

namespace drna {

struct CoOutArgs {
  const PfTables* F = nullptr;
  const Plan* plan = nullptr;
  const double* scale = nullptr;
  const double* eMLb = nullptr;
  const char* seqs = nullptr;      // R x L ASCII, both strands, no '&'
  int L = 0, cut = 0, ld = 0;
  double eDuplexInit = 1.0;
  double* wsp = nullptr;           // per pair: QB, QM, QM1, INFO as cofold_pf_kernel left them, then OB, AT, OM, OM1 (ld*ld doubles each)
  long long wsp_stride = 0;
  double* wu = nullptr;            // per pair: OBU, ATU, OMU, OM1U (ld*ld doubles each): the weights without joining pairs
  long long wu_stride = 0;
  const short* pt = nullptr;       // pair table of the design target ('&' removed): L+2 shorts, 1-based, 0 = unpaired
  double* edef = nullptr;          // R
  double* bpp = nullptr;           // optional: R x (L+1) x (L+1), P[i,j] at [i*(L+1)+j], i < j, 1-based
  int32_t* status_pf = nullptr;    // R: written by cofold_pf_kernel; this kernel adds ST_PF_RANGE
};

// doubles per pair in wsp: the three inside tables, INFO (one byte per cell), four outside tables
inline long long cofold_outside_ws_stride(int ld) { const long long tab = (long long)ld * ld; return 7 * tab + (tab + 7) / 8; }

struct CoOutSmem : PfSmem {
  double q3[MAXN + 3], qA3[MAXN + 3], qB5[MAXN + 3];
};
static_assert(PART_ITEMS * WAVE >= MAXN, "H / Hb reuse PfSmem::partI / partK: indices up to n + 1 <= MAXN - 1");

// the factor cofold_pf_kernel puts on qA3[p+1] qB5[q-1] for the joining pair (p,q) whose INFO byte is fi
template <class SM>
__device__ __forceinline__ double co_nick_factor(const SM& sm, const PfTables& T, double sc2, int fi, int p, int q, int cut) {
  const int rt = fi >> 4;
  return sc2 * (rt > 2 ? T.TermAU : 1.0) *
         co_pf_endstem(sm.mmExt, sm, rt, co_same(q - 1, q, cut), sm.S[q - 1], co_same(p, p + 1, cut), sm.S[p + 1]);
}

// Where the tables of one pair live: the three inside tables and INFO as cofold_pf_body left them, the four outside tables, their
// twins without joining pairs, and the two columns of the nick loop (n + 2 doubles each).  Hb holds the per-position terms of the
// defect after the sweep.  The one-strand instance reads neither the *U tables nor H.
struct CoOutTables {
  const double *QB, *QM, *QM1;
  const unsigned char* INFO;
  double *OB, *AT, *OM, *OM1;
  double *OBU, *ATU, *OMU, *OM1U;
  double *H, *Hb;
};

// outside sweep, probabilities and defect of pair r by the calling workgroup; the cells of every table where the layout says
// (fold_cofold.hpp), sm with the members of CoPfSmemCore and the column q3.
//   ONE    the second strand is empty (cut = n): every cell lies inside the one strand, where the weights without joining pairs
//          ARE the weights (`same` always holds, nothing joins), so the *U tables, H / Hb / G and the nick terms are left out
//          and Z = q5[n].  What remains is the one-strand outside recursion in this file's order of summation.
//   RESUME the caller has just run cofold_pf_body on the same sm: the staged tables, the letters and the columns q5, qA3, qB5
//          are there already (the inside sweep builds them with the same steps, so they hold the same bits); only q3 is built.
template <int NT, bool ONE, bool RESUME, class SM, class LAY>
__device__ __forceinline__ void cofold_outside_body(SM& sm, const CoOutArgs& A, int r, const CoOutTables& tb, const LAY lay) {
  constexpr int NW = NT / WAVE;
  const PfTables& T = *A.F;
  const Plan& P = *A.plan;
  const int n = lay.n, cut = lay.cut;
  const int tid = threadIdx.x, lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());
  const double* QB = tb.QB;
  const double* QM = tb.QM;
  const double* QM1 = tb.QM1;
  const unsigned char* INFO = tb.INFO;
  double* OB = tb.OB;
  double* AT = tb.AT;
  double* OM = tb.OM;
  double* OM1 = tb.OM1;
  double* OBU = tb.OBU;
  double* ATU = tb.ATU;
  double* OMU = tb.OMU;
  double* OM1U = tb.OM1U;
  double* H = tb.H;                // H[1..cut]
  double* Hb = tb.Hb;              // Hb[cut..n]; after the sweep: the per-position terms of the defect

  if (!RESUME) {
    stage_energy_tables<NT>(sm, T, tid);
    for (int k = tid; k <= n + 2; k += NT) {
      sm.qA3[k] = k == cut ? A.scale[1] : 1.0;
      sm.qB5[k] = k == cut + 1 && k <= n ? A.scale[1] : 1.0;
    }
  }
  if (!ONE)
    for (int k = tid; k <= n + 1; k += NT) { H[k] = 0.0; Hb[k] = 0.0; }
  if (!RESUME) lay.template load<NT>(sm, A.seqs, r, tid);
  if (A.status_pf[r] != ST_OK) {          // bad character / partition function out of range: the host reports it
    if (tid == 0) A.edef[r] = 0.0;
    return;
  }
  const double b1 = A.eMLb[1], sc1 = A.scale[1], sc2 = A.scale[2];

  // ---- the 1-D columns, each by one wave with the inside sweep's own steps (fold_cofold.hpp): qA3 of [x..cut], qB5 of
  // [cut+1..y], q5 of [1..j] and the suffix column q3 of [i..n].  They read QB / INFO only, so the four run side by side.
  if (!RESUME) {
    if (!ONE && wave == 0)
      for (int x = cut - 1; x >= 1; x--) co_qA3_step(sm, lay, QB, INFO, x, T.TermAU, sc1, lane);
    if (!ONE && wave == 1 % NW)
      for (int y = cut + 2; y <= n; y++) co_qB5_step(sm, lay, QB, INFO, y, T.TermAU, sc1, lane);
    if (wave == 2 % NW) co_q5_column(sm, lay, QB, INFO, T.TermAU, sc1, lane);
  }
  if (wave == 3 % NW) co_q3_column(sm, lay, QB, INFO, T.TermAU, sc1, lane);
  __syncthreads();
  const double QAs = ONE ? 1.0 : sm.qA3[1], QBs = ONE ? 1.0 : sm.qB5[n];     // the strands' own partition functions

  for (int d = n - 1; d >= 1; d--) {
    const int ncell = n - d;
    for (int i = wave + 1; i <= ncell; i += NW) {
      const int j = i + d;
      const bool same = co_same(i, j, cut);
      const bool su = !ONE && same;               // the cell also carries the weights without joining pairs
      if (same && d <= TURN) continue;               // no pair, and nothing below reads these cells
      const int at = lay.at(d, i);
      const int info = INFO[at];
      const bool inA = j <= cut;
      const int lo = same && !inA ? cut + 1 : 1, hi = same && inA ? cut : n;   // the cell's strand (the *U sums stay inside it)
      // Om[i,j]
      double s1 = 0.0, s1u = 0.0;
      if (j != cut) {
        for (int jj = j + 1 + lane; jj <= n; jj += WAVE) {
          const double m1 = QM1[lay.at(jj - j - 1, j + 1)];
          const int aj = lay.at(jj - i, i);
          s1 += AT[aj] * m1;
          if (su && jj <= hi) s1u += ATU[aj] * m1;
        }
      }
      // what Om1[i,j] gathers from the cells to the left in its column
      double s2 = 0.0, s2u = 0.0;
      const bool nb = i - 1 != cut;
      for (int ii = lane + 1; ii < i; ii += WAVE) {
        const int aj = lay.at(j - ii, ii);
        const bool inu = su && ii >= lo;
        double term = 0.0, termu = 0.0;
        if (nb) {
          const double qm = QM[lay.at(i - 1 - ii, ii)];
          term = AT[aj] * qm;
          if (inu) termu = ATU[aj] * qm;
        }
        if (co_same(ii, i, cut)) {
          const double b = A.eMLb[i - ii];
          term += OM[aj] * b;
          if (inu) termu += OMU[aj] * b;
        }
        s2 += term;
        s2u += termu;
      }
      // interior loops that enclose (i,j); inside a strand they lie on that strand
      double si = 0.0, siu = 0.0;
      if (info) {
        for (int e = lane; e < NPLAN; e += WAVE) {
          const int u1 = P.tb_u1[e], u2 = P.tb_u2[e];
          const int p = i - 1 - u1, q = j + 1 + u2;
          if (p < 1 || q > n) continue;
          if (!co_same(p, i, cut) || !co_same(j, q, cut)) continue;
          const int t = pair_type(sm.S[p], sm.S[q]);
          if (!t) continue;
          const double f = co_pf_intloop(sm, T, A.scale, u1, u2, t, sm.S[p + 1], sm.S[q - 1], info);
          const int ap = lay.at(q - p, p);
          si += OB[ap] * f;
          if (su) siu += OBU[ap] * f;
        }
      }
      s1 = wave_sum_f64(s1);
      s2 = wave_sum_f64(s2);
      si = wave_sum_f64(si);
      if (su) {
        s1u = wave_sum_f64(s1u);
        s2u = wave_sum_f64(s2u);
        siu = wave_sum_f64(siu);
      }
      const bool h5 = i > 1 && co_same(i - 1, i, cut), h3 = j < n && co_same(j, j + 1, cut);
      double om1 = s1 + s2, om1u = s1u + s2u;
      if (h3) {
        om1 += OM1[lay.at(d + 1, i)] * b1;
        if (su) om1u += OM1U[lay.at(d + 1, i)] * b1;
      }
      double cl = 0.0, clu = 0.0;                    // the multiloop closed by (i-1, j+1)
      if (h5 && h3) {
        const int tp = pair_type(sm.S[i - 1], sm.S[j + 1]);
        if (tp) {
          const double c = T.MLclosing * T.MLintern * (tp > 2 ? T.TermAU : 1.0) * sm.mmM[rtype_of(tp) * 16 + sm.S[j] * 4 + sm.S[i]] * sc2;
          cl = OB[lay.at(d + 2, i - 1)] * c;
          if (su) clu = OBU[lay.at(d + 2, i - 1)] * c;
        }
      }
      double ob = 0.0, obu = 0.0;
      if (info) {
        const int t = rtype_of(info >> 4);
        const double tau = t > 2 ? T.TermAU : 1.0;
        const double ext = tau * co_pf_endstem(sm.mmExt, sm, t, h5, sm.S[i - 1], h3, sm.S[j + 1]);
        const double stm = T.MLintern * tau * co_pf_endstem(sm.mmM, sm, t, h5, sm.S[i - 1], h3, sm.S[j + 1]);
        ob = om1 * stm + sm.q5[i - 1] * sm.q3[j + 1] * ext + si;
        if (su && inA) {
          ob += H[i] * ext * sm.qA3[j + 1];
          obu = om1u * stm + sm.q5[i - 1] * sm.qA3[j + 1] * QBs * ext + siu;
        } else if (su) {
          ob += sm.qB5[i - 1] * ext * Hb[j];
          obu = om1u * stm + QAs * sm.qB5[i - 1] * sm.q3[j + 1] * ext + siu;
        }
      }
      if (lane == 0) {
        OB[at] = ob;
        AT[at] = s1 + cl;
        OM[at] = s1;
        OM1[at] = om1;
        if (su) {
          OBU[at] = obu;
          ATU[at] = s1u + clu;
          OMU[at] = s1u;
          OM1U[at] = om1u;
        }
      }
    }
    __syncthreads();
    if (ONE) continue;
    // the nick loop seen from inside: H[cut - d + 2] and Hb[cut + d - 1] (every joining pair they need is finished)
    if (wave == 0 && d >= 2 && d <= cut) {
      const int x = cut - d + 2, p = x - 1;
      double g = 0.0, s = 0.0;
      for (int q = cut + 1 + lane; q <= n; q += WAVE) {
        const int fi = INFO[lay.at(q - p, p)];
        if (!fi) continue;
        g += OB[lay.at(q - p, p)] * co_nick_factor(sm, T, sc2, fi, p, q, cut) * sm.qB5[q - 1];
      }
      for (int k = 1 + lane; k <= x - 2; k += WAVE) {
        const int fi = INFO[lay.at(p - k, k)];
        if (!fi) continue;
        const int t = rtype_of(fi >> 4);
        s += H[k] * QB[lay.at(p - k, k)] * (t > 2 ? T.TermAU : 1.0) *
             co_pf_endstem(sm.mmExt, sm, t, k > 1, sm.S[k - 1], p < cut, sm.S[p + 1]);
      }
      g = wave_sum_f64(g);
      s = wave_sum_f64(s);
      H[x] = g + H[p] * sc1 + s;
    }
    if (wave == (NT > WAVE ? 1 : 0) && d >= 2 && d <= n - cut) {
      const int y = cut + d - 1, q = y + 1;
      double g = 0.0, s = 0.0;
      for (int p = 1 + lane; p <= cut; p += WAVE) {
        const int fi = INFO[lay.at(q - p, p)];
        if (!fi) continue;
        g += OB[lay.at(q - p, p)] * co_nick_factor(sm, T, sc2, fi, p, q, cut) * sm.qA3[p + 1];
      }
      for (int k = q + 1 + lane; k <= n; k += WAVE) {
        const int fi = INFO[lay.at(k - q, q)];
        if (!fi) continue;
        const int t = rtype_of(fi >> 4);
        s += QB[lay.at(k - q, q)] * (t > 2 ? T.TermAU : 1.0) *
             co_pf_endstem(sm.mmExt, sm, t, q > cut + 1, sm.S[q - 1], k < n, sm.S[k + 1]) * Hb[k];
      }
      g = wave_sum_f64(g);
      s = wave_sum_f64(s);
      Hb[y] = g + Hb[q] * sc1 + s;
    }
    __syncthreads();
  }

  // ---- probabilities (in place of OB), kappa on the connected part only
  const double kap = ONE ? 1.0 : co_homodimer(sm, n, cut) ? 0.5 * A.eDuplexInit : A.eDuplexInit;   // rotational symmetry of a homodimer
  const double Z = ONE ? sm.q5[n] : (sm.q5[n] - QAs * QBs) * kap + QAs * QBs;
  for (int d = 1; d < n; d++) {
    for (int i = tid + 1; i <= n - d; i += NT) {
      const int at = lay.at(d, i);
      double p = 0.0;
      if (INFO[at]) {
        const double w = OB[at];
        if (!ONE && co_same(i, i + d, cut)) { const double wu = OBU[at]; p = (kap * (w - wu) + wu) * QB[at] / Z; }
        else p = kap * w * QB[at] / Z;
        p = p < 0.0 ? 0.0 : p > 1.0 ? 1.0 : p;       // rounding only: a probability stays one
      }
      OB[at] = p;
    }
  }
  __syncthreads();
  // ---- ensemble defect ('(' ')' pairs of the target only, as in outside_kernel)
  double* val = Hb;
  const short* pt = A.pt;
  for (int k = tid + 1; k <= n; k += NT) {
    const int m = pt[k];
    double v;
    if (m == 0) {
      v = 0.0;
      for (int i = 1; i < k; i++) v += OB[lay.at(k - i, i)];
      for (int j = k + 1; j <= n; j++) v += OB[lay.at(j - k, k)];
    } else {
      const int a = m < k ? m : k, c = m < k ? k : m;
      v = 1.0 - OB[lay.at(c - a, a)];
    }
    val[k] = v;
  }
  if (A.bpp) {
    double* B = A.bpp + (long long)r * (n + 1) * (n + 1);
    for (int d = 1; d < n; d++)
      for (int i = tid + 1; i <= n - d; i += NT) B[(long long)i * (n + 1) + i + d] = OB[lay.at(d, i)];
  }
  __syncthreads();
  if (tid == 0) {
    double ed = 0.0;
    for (int k = 1; k <= n; k++) ed += val[k];
    ed /= (double)n;
    if (!(Z > 0.0) || !(Z < 1.0e300) || !(ed >= 0.0) || !(ed < 1.0e300)) { A.status_pf[r] = ST_PF_RANGE; ed = 0.0; }
    A.edef[r] = ed;
  }
}

template <int NT>
__global__ __launch_bounds__(NT) void cofold_outside_kernel(CoOutArgs A) {
  __shared__ CoOutSmem sm;
  const int r = blockIdx.x;
  double* base = A.wsp + (long long)r * A.wsp_stride;
  const long long tab = (long long)A.ld * A.ld;
  double* OB = base + 3 * tab + (tab + 7) / 8;
  double* OBU = A.wu + (long long)r * A.wu_stride;
  const CoOutTables tb{base, base + tab, base + 2 * tab, reinterpret_cast<const unsigned char*>(base + 3 * tab),
                       OB, OB + tab, OB + 2 * tab, OB + 3 * tab, OBU, OBU + tab, OBU + 2 * tab, OBU + 3 * tab, sm.partI, sm.partK};
  cofold_outside_body<NT, false, false>(sm, A, r, tb, CoSquare{A.L, A.cut, A.ld});
}

}  // namespace drna
