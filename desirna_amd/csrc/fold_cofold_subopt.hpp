// fold_cofold_subopt.hpp -- energy of the second-best co-fold structure of one sequence pair per workgroup on gfx950.
// Replaces get_first_suboptimal_structure_and_energy(seq, fc, 1)[1] on the DIMER fold compound of the reference's
// two-strand -nd on path (utils/energy_scores.py:105-108, :453-488): the lowest energy over all co-fold structures other
// than one ground-state structure (0 if none lies within 49 kcal/mol of the co-fold MFE).
//
// The structures are those cofold_mfe_kernel minimises over (fold_cofold.hpp: canonical non-crossing pairs; hairpins,
// interior-loop stretches and multiloop backbones inside a strand; the loop whose backbone holds the nick is exterior-like;
// dangles only inside a strand; DuplexInit iff a pair joins the strands).  Two-best dynamic programme over the unambiguous
// decomposition of fold_subopt.hpp with the nick rules of cofold_mfe_kernel, term for term:
//   C[i,j]  = { hairpin (same strand) ; nick loop: E_ExtLoop + fcA[i+1] + fcB[j-1] (joining pair) ;
//               C[p,q] + interior (stretches inside a strand) ; M2[i+1,j-1] + closing (i,i+1 and j-1,j neighbours) }
//   M[i,j]  (>= 1 stem) = { M[i,j-1] + b (j-1,j neighbours) ; (k-i) b + C[k,j] + stem (i..k inside a strand) ;
//                           M[i,k-1] + C[k,j] + stem (k-1,k neighbours) }
//   M2[i,j] (>= 2 stems) = { M2[i,j-1] + b (j-1,j neighbours) ; M[i,k-1] + C[k,j] + stem (k-1,k neighbours) }
//   fcA[x] of [x..cut], fcB[y] of [cut+1..y]: exterior decompositions next to the nick, advanced one entry per diagonal.
// The exterior level is split into UNCONNECTED structures (Fu: no pair joins the strands) and CONNECTED ones (Fc: exactly one
// exterior-level pair joins them -- two could only cross), so every structure is counted once and DuplexInit goes to the
// connected half only: E = top2(Fu[n] ; Fc[n] + DuplexInit).  No symmetry reduction for two equal strands: a structure and
// its rotation by `cut` are two structures.
// One wave per cell (the lanes share the interior-loop shapes and the split points, wave_top2 folds them); C, M, M2 are
// (best, second) int32 pairs in HBM/L2 (diagonal-major), fcA / fcB (and then Fu / Fc) pairs in LDS.
#pragma once
#include "fold_cofold.hpp"
#include "fold_subopt.hpp"

namespace drna {

struct CoSubArgs {
  const MfeTables* T = nullptr;
  const Plan* plan = nullptr;
  const int* hp_len = nullptr;
  const char* seqs = nullptr;     // R x L ASCII, both strands, no '&'
  int L = 0, cut = 0, ld = 0;
  int DuplexInit = 0;
  int32_t* ws = nullptr;          // per pair: C, M, M2 as (best, second) int32 pairs: 6 ld*ld int32
  long long ws_stride = 0;
  int32_t* E2 = nullptr;          // R: the reference's subopt energy (dcal/mol; 0 = none within 4900)
  int32_t* E12 = nullptr;         // optional R x 2: the two lowest energies (second = INF_REF if there is one structure only)
  int32_t* status = nullptr;      // R
};

struct CoSubSmem : MfeSmemCore<MAXN> {
  // during the sweep: fcA[x] of [x..cut] and fcB[y] of [cut+1..y]; afterwards wave 0 reuses them for Fu / Fc of the
  // exterior loop (the nick loops are all filled by then)
  Top2 fcA[MAXN + 3], fcB[MAXN + 3];
};

template <int NT>
__global__ __launch_bounds__(NT) void cofold_subopt_kernel(CoSubArgs A) {
  __shared__ CoSubSmem sm;
  const MfeTables& T = *A.T;
  const Plan& P = *A.plan;
  const int r = blockIdx.x;
  const int n = A.L, cut = A.cut, ld = A.ld;
  const int tid = threadIdx.x, lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());
  const int INF = INF_DEV, HALF = INF_DEV / 2;
  int32_t* base = A.ws + (long long)r * A.ws_stride;
  const long long tab = (long long)ld * ld;
  Top2* C = reinterpret_cast<Top2*>(base);
  Top2* M = reinterpret_cast<Top2*>(base + 2 * tab);
  Top2* M2 = reinterpret_cast<Top2*>(base + 4 * tab);

  stage_energy_tables<NT>(sm, T, tid);
  // row 0 (single nucleotides): no pair, no multiloop content
  for (int k = tid; k < ld; k += NT) { C[k] = Top2{INF, INF}; M[k] = Top2{INF, INF}; M2[k] = Top2{INF, INF}; }
  for (int k = tid; k <= n + 2; k += NT) { sm.fcA[k] = Top2{0, INF}; sm.fcB[k] = Top2{0, INF}; }   // empty / one-nt segments
  load_sequence<NT>(sm, A.seqs + (long long)r * n, n, tid);
  if (sm.flag) {
    if (tid == 0) { A.status[r] = ST_BAD_CHAR; A.E2[r] = 0; if (A.E12) { A.E12[2 * r] = 0; A.E12[2 * r + 1] = INF_REF; } }
    return;
  }

  // pairs that join the strands exist at any distance: the sweep starts at diagonal 1
  for (int d = 1; d < n; d++) {
    const int ncell = n - d;
    for (int i = wave + 1; i <= ncell; i += NT / WAVE) {
      const int j = i + d;
      const bool same = co_same(i, j, cut);
      const int t = (d > TURN || !same) ? pair_type(sm.S[i], sm.S[j]) : 0;
      const int tau = t > 2 ? T.TermAU : 0;
      const bool adj_i = co_same(i, i + 1, cut), adj_j = co_same(j - 1, j, cut);
      Top2 c{INF, INF};
      if (t) {
        const int si1 = sm.S[i + 1], sj1 = sm.S[j - 1];
        for (int e = lane; e < NPLAN; e += WAVE) {
          const int u1 = P.u1[e], u2 = P.u2[e];
          const int dp = d - 2 - u1 - u2;
          if (dp < 1) continue;
          const int p = i + 1 + u1, q = j - 1 - u2;
          if (!co_same(i, p, cut) || !co_same(q, j, cut)) continue;
          const int t2 = pair_type(sm.S[p], sm.S[q]);
          if (!t2) continue;
          const Top2 cp = C[dp * ld + p];
          if (cp.a >= HALF) continue;
          const int info = (rtype_of(t2) << 4) | (sm.S[q + 1] << 2) | sm.S[p - 1];
          t2_add_sum(c, cp, mfe_intloop(sm, T, u1, u2, t, si1, sj1, info));
        }
        if (lane == 0) {
          if (same) t2_add(c, mfe_hairpin_e(sm, T, A.hp_len[d - 1], i, j, t));
          else t2_add_sum2(c, sm.fcA[i + 1], sm.fcB[j - 1], tau + co_endstem(sm.mmExt, sm, rtype_of(t), adj_j, sj1, adj_i, si1));
          if (adj_i && adj_j && d >= 2)
            t2_add_sum(c, M2[(d - 2) * ld + i + 1], T.MLclosing + T.MLintern + tau + sm.mmM[rtype_of(t) * 16 + sj1 * 4 + si1]);
        }
        c = wave_top2(c);
      }
      Top2 m{INF, INF}, m2{INF, INF};
      if (lane == 0 && adj_j) {
        t2_add_sum(m, M[(d - 1) * ld + i], T.MLbase);
        t2_add_sum(m2, M2[(d - 1) * ld + i], T.MLbase);
      }
      const bool h3 = j < n && co_same(j, j + 1, cut);
      for (int k = i + lane; k < j; k += WAVE) {
        const int tk = (j - k > TURN || !co_same(k, j, cut)) ? pair_type(sm.S[k], sm.S[j]) : 0;
        if (!tk) continue;
        const Top2 ck = k == i ? c : C[(j - k) * ld + k];
        if (ck.a >= HALF) continue;
        const bool h5 = k > 1 && co_same(k - 1, k, cut);
        const int st = T.MLintern + (tk > 2 ? T.TermAU : 0) + co_endstem(sm.mmM, sm, tk, h5, sm.S[k - 1], h3, sm.S[j + 1]);
        if (co_same(i, k, cut)) t2_add_sum(m, ck, (k - i) * T.MLbase + st);
        if (k > i && k - 1 != cut) {
          const Top2 mk = M[(k - 1 - i) * ld + i];
          t2_add_sum2(m, mk, ck, st);
          t2_add_sum2(m2, mk, ck, st);
        }
      }
      m = wave_top2(m);
      m2 = wave_top2(m2);
      if (lane == 0) { C[d * ld + i] = c; M[d * ld + i] = m; M2[d * ld + i] = m2; }
    }
    __syncthreads();
    // exterior decompositions next to the nick: fcA[cut - d] of [cut-d .. cut], fcB[cut + 1 + d] of [cut+1 .. cut+1+d]
    if (wave == 0 && cut - d >= 1) {
      const int x = cut - d;
      Top2 f{INF, INF};
      if (lane == 0) t2_add_sum(f, sm.fcA[x + 1], 0);
      for (int k = x + 1 + lane; k <= cut; k += WAVE) {
        const int t = pair_type(sm.S[x], sm.S[k]);
        if (!t) continue;
        const Top2 ck = C[(k - x) * ld + x];
        if (ck.a >= HALF) continue;
        const int ext = (t > 2 ? T.TermAU : 0) + co_endstem(sm.mmExt, sm, t, x > 1, sm.S[x - 1], k < cut, sm.S[k + 1]);
        t2_add_sum2(f, ck, sm.fcA[k + 1], ext);
      }
      f = wave_top2(f);
      sm.fcA[x] = f;                               // every lane stores the same value (here and below)
    }
    if (wave == (NT > WAVE ? 1 : 0) && cut + 1 + d <= n) {
      const int y = cut + 1 + d;
      Top2 f{INF, INF};
      if (lane == 0) t2_add_sum(f, sm.fcB[y - 1], 0);
      for (int k = cut + 1 + lane; k < y; k += WAVE) {
        const int t = pair_type(sm.S[k], sm.S[y]);
        if (!t) continue;
        const Top2 ck = C[(y - k) * ld + k];
        if (ck.a >= HALF) continue;
        const int ext = (t > 2 ? T.TermAU : 0) + co_endstem(sm.mmExt, sm, t, k > cut + 1, sm.S[k - 1], y < n, sm.S[y + 1]);
        t2_add_sum2(f, sm.fcB[k - 1], ck, ext);
      }
      f = wave_top2(f);
      sm.fcB[y] = f;
    }
    __syncthreads();
  }

  if (wave != 0) return;
  // ---- exterior loop over the concatenation, unconnected (Fu) and connected (Fc) prefixes kept apart
  Top2* Fu = sm.fcA;
  Top2* Fc = sm.fcB;
  Fu[0] = Top2{0, INF};
  Fc[0] = Top2{INF, INF};
  for (int j = 1; j <= n; j++) {
    Top2 fu{INF, INF}, fc{INF, INF};
    if (lane == 0) { t2_add_sum(fu, Fu[j - 1], 0); t2_add_sum(fc, Fc[j - 1], 0); }
    const bool h3 = j < n && co_same(j, j + 1, cut);
    for (int i = lane + 1; i < j; i += WAVE) {
      const bool same = co_same(i, j, cut);
      const int t = (j - i > TURN || !same) ? pair_type(sm.S[i], sm.S[j]) : 0;
      if (!t) continue;
      const Top2 cij = C[(j - i) * ld + i];
      if (cij.a >= HALF) continue;
      const bool h5 = i > 1 && co_same(i - 1, i, cut);
      const int ext = (t > 2 ? T.TermAU : 0) + co_endstem(sm.mmExt, sm, t, h5, sm.S[i - 1], h3, sm.S[j + 1]);
      if (same) {
        t2_add_sum2(fu, Fu[i - 1], cij, ext);
        t2_add_sum2(fc, Fc[i - 1], cij, ext);
      } else {
        t2_add_sum2(fc, Fu[i - 1], cij, ext);     // the one exterior-level pair that joins the strands
      }
    }
    fu = wave_top2(fu);
    fc = wave_top2(fc);
    Fu[j] = fu;
    Fc[j] = fc;
  }
  if (lane == 0) {
    Top2 f = Fu[n];
    t2_add_sum(f, Fc[n], A.DuplexInit);
    A.status[r] = ST_OK;
    A.E2[r] = (f.b >= HALF || f.b - f.a > 4900) ? 0 : f.b;
    if (A.E12) { A.E12[2 * r] = f.a; A.E12[2 * r + 1] = f.b >= HALF ? INF_REF : f.b; }
  }
}

}  // namespace drna
