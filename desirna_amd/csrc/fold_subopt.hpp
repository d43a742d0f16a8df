// fold_subopt.hpp -- the lowest-energy structures next to the ground state, one sequence (or sequence pair) per workgroup on
// gfx950.  Four kernels over one table fill (kbest_fill) and one exterior level (kbest_exterior):
//
//   subopt_kernel         energy of the second-best structure of one strand.  Replaces
//       get_first_suboptimal_structure_and_energy(seq, fc, 1)[1] of the reference's negative-design option (-nd on;
//       utils/energy_scores.py:105-107, :453-488): ViennaRNA's subopt enumeration (uniq_ML = 1) with a growing energy band
//       until it holds two structures, sorted by energy, second entry taken -- SURVEY 8(f)-4.  Only that entry's ENERGY is
//       used by the caller: the lowest energy over all structures other than one ground-state structure (0 if none lies
//       within 49 kcal/mol of the MFE).
//   cofold_subopt_kernel  the same for two strands: fold_cofold_subopt.hpp, over the CO = true instance of the fill below.
//   cofold_kbest_kernel   kbest_kernel (below) for two strands: fold_cofold_subopt.hpp, over the CO = true instances of the fill and
//       of the traceback's enumerator kb_enum.
//   kbest_kernel          K lowest-energy structures (energies AND dot-bracket strings) of one strand.  Replaces
//       get_first_suboptimal_structure_and_energy(seq, fc, k)[0] for k = 1 .. #alt structures, the call behind get_alt_mcc()
//       in the reference's final ranking of alternative-structure designs (utils/sequence_utils.py:766-793,
//       utils/energy_scores.py:453-488): entry k of ViennaRNA's energy-sorted subopt list (uniq_ML = 1).
//
// K-best dynamic programme over an unambiguous decomposition (every structure has one derivation, so the K smallest
// values of a table entry belong to K different structures):
//   F[j]    = { F[j-1] ; F[i-1] + C[i,j] + ext(i,j) }
//   C[i,j]  = { hairpin ; C[p,q] + interior ; M2[i+1,j-1] + closing }
//   M[i,j]  (>= 1 stem) = { M[i,j-1] + b ; (k-i) b + C[k,j] + stem ; M[i,k-1] + C[k,j] + stem }
//   M2[i,j] (>= 2 stems) = { M2[i,j-1] + b ; M[i,k-1] + C[k,j] + stem }
// One wave per cell: the lanes share the interior-loop shapes and the positions k, the K-lists are folded with a butterfly
// over disjoint lane groups.  Tables (K int32 per entry, diagonal-major) live in HBM/L2.
//
// Two strands (concatenated, cut = length of the first): the structures are those cofold_mfe_kernel minimises over
// (fold_cofold.hpp: canonical non-crossing pairs; hairpins, interior-loop stretches and multiloop backbones inside a strand;
// the loop whose backbone holds the nick is exterior-like; dangles only inside a strand; DuplexInit iff a pair joins the
// strands).  The same decomposition with the nick rules of cofold_mfe_kernel, term for term:
//   C[i,j]  = { hairpin (same strand) ; nick loop: E_ExtLoop + fcA[i+1] + fcB[j-1] (joining pair) ;
//               C[p,q] + interior (stretches inside a strand) ; M2[i+1,j-1] + closing (i,i+1 and j-1,j neighbours) }
//   M[i,j]  (>= 1 stem) = { M[i,j-1] + b (j-1,j neighbours) ; (k-i) b + C[k,j] + stem (i..k inside a strand) ;
//                           M[i,k-1] + C[k,j] + stem (k-1,k neighbours) }
//   M2[i,j] (>= 2 stems) = { M2[i,j-1] + b (j-1,j neighbours) ; M[i,k-1] + C[k,j] + stem (k-1,k neighbours) }
//   fcA[x] of [x..cut], fcB[y] of [cut+1..y]: exterior decompositions next to the nick, advanced one entry per diagonal.
// Pairs that join the strands exist at any distance, so the sweep starts at diagonal 1.  No symmetry reduction for two equal
// strands: a structure and its rotation by `cut` are two structures.
#pragma once
#include "fold_cofold.hpp"

namespace drna {

struct SuboptArgs {
  const MfeTables* T = nullptr;
  const Plan* plan = nullptr;
  const int* hp_len = nullptr;
  const char* seqs = nullptr;     // R x L ASCII (two strands: both, no '&')
  int L = 0, cut = 0, ld = 0;     // cut = length of the first strand, 0 = one strand
  int DuplexInit = 0;             // two strands only
  int32_t* ws = nullptr;          // per sequence: C, M, M2 as K-lists: 3 K ld*ld int32 (K = 2 in the second-best kernels)
  long long ws_stride = 0;
  // second-best kernels
  int32_t* E2 = nullptr;          // R: the reference's subopt energy (dcal/mol; 0 = none within 4900)
  int32_t* E12 = nullptr;         // optional R x 2: the two lowest energies (second = INF_REF if there is one structure only)
  // kbest_kernel
  int32_t* E = nullptr;           // R x K energies, ascending (INF_REF where the sequence has fewer structures)
  char* ss = nullptr;             // R x K x L dot-bracket strings (all dots where E = INF_REF)
  int32_t* status = nullptr;      // R
  // ragged batch (drna_subopt_energy_ragged; the one-strand second-best kernels only): lengths and letter offsets per sequence,
  // workgroup -> sequence.  A sequence of n nucleotides then folds at its OWN pitch n + 2 (ld is ignored) inside its workspace
  // slot of ws_stride words, so every table cell sits where the uniform call of that length puts it
  Ragged rg;
};
// the three kernels had an argument struct each; launch code written against those names keeps compiling
using SubArgs = SuboptArgs;
using KbArgs = SuboptArgs;

// the K smallest values seen, ascending, duplicates included
template <int K>
struct TopK { int v[K]; };

template <int K>
__device__ __forceinline__ void tk_init(TopK<K>& t) {
#pragma unroll
  for (int r = 0; r < K; r++) t.v[r] = INF_DEV;
}
template <int K>
__device__ __forceinline__ void tk_add(TopK<K>& t, int v) {
  if (v >= INF_DEV / 2) return;
#pragma unroll
  for (int r = 0; r < K; r++) { const int lo = min(v, t.v[r]); v = max(v, t.v[r]); t.v[r] = lo; }
}
template <int K>
__device__ __forceinline__ void tk_add_sum(TopK<K>& t, const TopK<K>& x, int e) {
#pragma unroll
  for (int r = 0; r < K; r++) if (x.v[r] < INF_DEV / 2) tk_add(t, x.v[r] + e);
}
template <int K>
__device__ __forceinline__ void tk_add_sum2(TopK<K>& t, const TopK<K>& x, const TopK<K>& y, int e) {
#pragma unroll
  for (int a = 0; a < K; a++)
#pragma unroll
    for (int b = 0; a + b < K; b++)       // the r-th best sum never needs ranks with a + b > r
      if (x.v[a] < INF_DEV / 2 && y.v[b] < INF_DEV / 2) tk_add(t, x.v[a] + y.v[b] + e);
}
// every lane ends with the K smallest values of the wave (the lane groups merged at each step are disjoint)
template <int K>
__device__ __forceinline__ TopK<K> wave_topk(TopK<K> t) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    TopK<K> x;
#pragma unroll
    for (int r = 0; r < K; r++) x.v[r] = __shfl_xor(t.v[r], o);
#pragma unroll
    for (int r = 0; r < K; r++) tk_add(t, x.v[r]);
  }
  return t;
}

// K = 2, the lists of the second-best kernels (every scoring step): the two-value form of the merge.  With the generic one
// above those kernels measured 4 - 14 % slower on an MI355X (profiles/subopt_family.json, generic_k2_build)
__device__ __forceinline__ TopK<2> wave_topk(TopK<2> t) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int oa = __shfl_xor(t.v[0], o), ob = __shfl_xor(t.v[1], o);
    const int lo = min(t.v[0], oa), hi = max(t.v[0], oa);
    t.v[1] = min(hi, min(t.v[1], ob));
    t.v[0] = lo;
  }
  return t;
}

// C, M, M2 of workgroup r
template <int K>
__device__ __forceinline__ void kb_tables(const SuboptArgs& A, int r, TopK<K>*& C, TopK<K>*& M, TopK<K>*& M2) {
  int32_t* base = A.ws + (long long)r * A.ws_stride;
  const long long tab = (long long)A.ld * A.ld * K;
  C = reinterpret_cast<TopK<K>*>(base);
  M = reinterpret_cast<TopK<K>*>(base + tab);
  M2 = reinterpret_cast<TopK<K>*>(base + 2 * tab);
}

// the diagonal sweep that writes C, M, M2 (all threads of the workgroup).  The caller has set the rows below the first
// diagonal of the sweep (TURN + 1; two strands: 1) and, for two strands (CO), sm.fcA / sm.fcB to the empty decomposition.
// With CO false every nick test below is a compile-time constant.  (The scalars come from A, lane and wave from the kernel:
// with n, ld, hp_len ... passed one by one the K = 8 instance takes 80 VGPRs instead of 76.)
template <int NT, int K, bool CO, class SM>
__device__ __forceinline__ void kbest_fill(SM& sm, const SuboptArgs& A, TopK<K>* C, TopK<K>* M, TopK<K>* M2, int lane, int wave) {
  const MfeTables& T = *A.T;
  const Plan& P = *A.plan;
  const int n = A.L, cut = A.cut, ld = A.ld;
  const int* hp_len = A.hp_len;
  const int HALF = INF_DEV / 2;
  constexpr int D0 = CO ? 1 : TURN + 1;               // first diagonal that can hold a pair
  TopK<K> none;
  tk_init(none);
  for (int d = D0; d < n; d++) {
    const int ncell = n - d;
    for (int i = wave + 1; i <= ncell; i += NT / WAVE) {
      const int j = i + d;
      const bool same = !CO || co_same(i, j, cut);
      const int t = (!CO || d > TURN || !same) ? pair_type(sm.S[i], sm.S[j]) : 0;
      const int tau = t > 2 ? T.TermAU : 0;
      const bool adj_i = !CO || co_same(i, i + 1, cut), adj_j = !CO || co_same(j - 1, j, cut);
      TopK<K> c = none;
      if (t) {
        const int si1 = sm.S[i + 1], sj1 = sm.S[j - 1];
        for (int e = lane; e < NPLAN; e += WAVE) {
          const int u1 = P.u1[e], u2 = P.u2[e];
          const int dp = d - 2 - u1 - u2;
          if (dp < D0) continue;
          const int p = i + 1 + u1, q = j - 1 - u2;
          if (CO && (!co_same(i, p, cut) || !co_same(q, j, cut))) continue;
          const int t2 = pair_type(sm.S[p], sm.S[q]);
          if (!t2) continue;
          const TopK<K> cp = C[dp * ld + p];
          if (cp.v[0] >= HALF) continue;
          const int info = (rtype_of(t2) << 4) | (sm.S[q + 1] << 2) | sm.S[p - 1];
          tk_add_sum(c, cp, mfe_intloop(sm, T, u1, u2, t, si1, sj1, info));
        }
        if (lane == 0) {
          if (same) tk_add(c, mfe_hairpin_e(sm, T, hp_len[d - 1], i, j, t));
          if constexpr (CO)
            if (!same) tk_add_sum2(c, sm.fcA[i + 1], sm.fcB[j - 1], tau + co_endstem(sm.mmExt, sm, rtype_of(t), adj_j, sj1, adj_i, si1));
          if (adj_i && adj_j && (!CO || d >= 2))
            tk_add_sum(c, M2[(d - 2) * ld + i + 1], T.MLclosing + T.MLintern + tau + sm.mmM[rtype_of(t) * 16 + sj1 * 4 + si1]);
        }
        c = wave_topk(c);
      }
      TopK<K> m = none, m2 = none;
      if (lane == 0 && adj_j) {
        tk_add_sum(m, M[(d - 1) * ld + i], T.MLbase);
        tk_add_sum(m2, M2[(d - 1) * ld + i], T.MLbase);
      }
      const bool h3 = j < n && co_same(j, j + 1, cut);  // (two strands)
      for (int k = i + lane; k <= j - D0; k += WAVE) {
        const int tk = (!CO || j - k > TURN || !co_same(k, j, cut)) ? pair_type(sm.S[k], sm.S[j]) : 0;
        if (!tk) continue;
        // the cell's own list at k = i.  K = 2 selects the values; the longer lists select the address (the chosen list then
        // goes through scratch): by value the K = 8 instance takes 83 VGPRs instead of 76, one wave less per SIMD
        TopK<K> ck = c;
        if constexpr (K == 2) { if (k != i) ck = C[(j - k) * ld + k]; }
        else ck = k == i ? c : C[(j - k) * ld + k];
        if (ck.v[0] >= HALF) continue;
        int st = T.MLintern + (tk > 2 ? T.TermAU : 0);
        if constexpr (CO) st += co_endstem(sm.mmM, sm, tk, k > 1 && co_same(k - 1, k, cut), sm.S[k - 1], h3, sm.S[j + 1]);
        else st += sm.mmM[tk * 16 + sm.S[k - 1] * 4 + sm.S[j + 1]];
        if (!CO || co_same(i, k, cut)) tk_add_sum(m, ck, (k - i) * T.MLbase + st);
        if (k > i && (!CO || k - 1 != cut)) {
          const TopK<K> mk = M[(k - 1 - i) * ld + i];
          tk_add_sum2(m, mk, ck, st);
          tk_add_sum2(m2, mk, ck, st);
        }
      }
      m = wave_topk(m);
      m2 = wave_topk(m2);
      if (lane == 0) { C[d * ld + i] = c; M[d * ld + i] = m; M2[d * ld + i] = m2; }
    }
    __syncthreads();
    if constexpr (CO) {
      // exterior decompositions next to the nick: fcA[cut - d] of [cut-d .. cut], fcB[cut + 1 + d] of [cut+1 .. cut+1+d]
      if (wave == 0 && cut - d >= 1) {
        const int x = cut - d;
        TopK<K> f = none;
        if (lane == 0) tk_add_sum(f, sm.fcA[x + 1], 0);
        for (int k = x + 1 + lane; k <= cut; k += WAVE) {
          const int t = pair_type(sm.S[x], sm.S[k]);
          if (!t) continue;
          const TopK<K> ck = C[(k - x) * ld + x];
          if (ck.v[0] >= HALF) continue;
          const int ext = (t > 2 ? T.TermAU : 0) + co_endstem(sm.mmExt, sm, t, x > 1, sm.S[x - 1], k < cut, sm.S[k + 1]);
          tk_add_sum2(f, ck, sm.fcA[k + 1], ext);
        }
        f = wave_topk(f);
        sm.fcA[x] = f;                               // every lane stores the same value (here and below)
      }
      if (wave == (NT > WAVE ? 1 : 0) && cut + 1 + d <= n) {
        const int y = cut + 1 + d;
        TopK<K> f = none;
        if (lane == 0) tk_add_sum(f, sm.fcB[y - 1], 0);
        for (int k = cut + 1 + lane; k < y; k += WAVE) {
          const int t = pair_type(sm.S[k], sm.S[y]);
          if (!t) continue;
          const TopK<K> ck = C[(y - k) * ld + k];
          if (ck.v[0] >= HALF) continue;
          const int ext = (t > 2 ? T.TermAU : 0) + co_endstem(sm.mmExt, sm, t, k > cut + 1, sm.S[k - 1], y < n, sm.S[y + 1]);
          tk_add_sum2(f, sm.fcB[k - 1], ck, ext);
        }
        f = wave_topk(f);
        sm.fcB[y] = f;
      }
      __syncthreads();
    }
  }
}

// exterior level over [1..n] from the filled C, one wave (every lane stores the same lists).  One strand: Fu = F above, Fc is
// not used.  Two strands: the level is split into UNCONNECTED structures (Fu: no pair joins the strands) and CONNECTED ones
// (Fc: exactly one exterior-level pair joins them -- two could only cross), so every structure is counted once and DuplexInit
// goes to the connected half only: E = topK(Fu[n] ; Fc[n] + DuplexInit).
template <int K, bool CO, class SM>
__device__ __forceinline__ void kbest_exterior(const SM& sm, const MfeTables& T, const TopK<K>* C, TopK<K>* Fu, TopK<K>* Fc, int n,
                                               int cut, int ld) {
  const int lane = lane_id(), HALF = INF_DEV / 2;
  constexpr int D0 = CO ? 1 : TURN + 1;
  TopK<K> none;
  tk_init(none);
  TopK<K> f0 = none;
  f0.v[0] = 0;
  Fu[0] = f0;
  if constexpr (CO) Fc[0] = none;
  for (int j = 1; j <= n; j++) {
    TopK<K> fu = none, fc = none;
    if (lane == 0) {
      tk_add_sum(fu, Fu[j - 1], 0);
      if constexpr (CO) tk_add_sum(fc, Fc[j - 1], 0);
    }
    const bool h3 = j < n && co_same(j, j + 1, cut);  // (two strands)
    for (int i = lane + 1; i <= j - D0; i += WAVE) {
      const bool same = !CO || co_same(i, j, cut);
      const int t = (!CO || j - i > TURN || !same) ? pair_type(sm.S[i], sm.S[j]) : 0;
      if (!t) continue;
      const TopK<K> cij = C[(j - i) * ld + i];
      if (cij.v[0] >= HALF) continue;
      int ext = t > 2 ? T.TermAU : 0;
      if constexpr (CO) ext += co_endstem(sm.mmExt, sm, t, i > 1 && co_same(i - 1, i, cut), sm.S[i - 1], h3, sm.S[j + 1]);
      else ext += mfe_extstem(sm, t, i, j, n);
      if (same) {
        tk_add_sum2(fu, Fu[i - 1], cij, ext);
        if constexpr (CO) tk_add_sum2(fc, Fc[i - 1], cij, ext);
      } else {
        tk_add_sum2(fc, Fu[i - 1], cij, ext);       // the one exterior-level pair that joins the strands
      }
    }
    fu = wave_topk(fu);
    Fu[j] = fu;
    if constexpr (CO) { fc = wave_topk(fc); Fc[j] = fc; }
  }
}

// status and the two energies of a second-best kernel (one lane)
__device__ __forceinline__ void second_best_report(const SuboptArgs& A, int r, int status, int e1, int e2) {
  const int HALF = INF_DEV / 2;
  A.status[r] = status;
  A.E2[r] = (e2 >= HALF || e2 - e1 > 4900) ? 0 : e2;
  if (A.E12) { A.E12[2 * r] = e1; A.E12[2 * r + 1] = e2 >= HALF ? INF_REF : e2; }
}

struct SubSmem : MfeSmemCore<MAXN> {
  TopK<2> F[MAXN + 2];
};

// RAGGED: the instance of the ragged launches; the uniform instance never looks at A.rg
template <int NT, bool RAGGED = false>
__global__ __launch_bounds__(NT) void subopt_kernel(SuboptArgs A) {
  __shared__ SubSmem sm;
  const MfeTables& T = *A.T;
  const int r = RAGGED ? A.rg.seq_of(blockIdx.x) : blockIdx.x;
  if (RAGGED && A.rg.len) { A.L = A.rg.len[r]; A.ld = A.L + 2; }
  const int n = A.L, ld = A.ld;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());
  TopK<2>*C, *M, *M2;
  kb_tables(A, r, C, M, M2);

  stage_energy_tables<NT>(sm, T, tid);
  // diagonals 0 .. TURN: no pair, no multiloop content
  TopK<2> none;
  tk_init(none);
  for (int d = 0; d <= TURN && d < n; d++)
    for (int k = tid; k < ld; k += NT) { C[d * ld + k] = none; M[d * ld + k] = none; M2[d * ld + k] = none; }
  load_sequence<NT>(sm, A.seqs + (RAGGED ? A.rg.off_of(r, n) : (long long)r * n), n, tid);
  if (sm.flag) {
    if (tid == 0) second_best_report(A, r, ST_BAD_CHAR, 0, INF_DEV);
    return;
  }
  kbest_fill<NT, 2, false>(sm, A, C, M, M2, lane_id(), wave);
  if (wave != 0) return;
  kbest_exterior<2, false>(sm, T, C, sm.F, nullptr, n, 0, ld);
  if (tid == 0) second_best_report(A, r, ST_OK, sm.F[n].v[0], sm.F[n].v[1]);
}


// ---------------------------------------------------------------------------------------------------------------------
// kbest_kernel: the fill above with K-lists, then one traceback per rank: a table entry's r-th value is expanded by
// re-enumerating the entry's candidates in a fixed order and taking, among those that reproduce the value, the one whose
// index equals the number of equal values ranked before r.  Different ranks of one entry thus expand to different
// derivations, i.e. different structures.  The order among structures of EQUAL energy is this enumeration order, not
// ViennaRNA's (which the reference pins nowhere).

template <int K>
struct KbSmem : MfeSmemCore<MAXN> {
  char db[K][MAXN + 2];
};

// kinds of a traceback item.  KB_F is the exterior level (two strands: Fu, the unconnected half); the last three exist for two
// strands only: Fc[j], fcA[x] and fcB[y] (x, y travel in the item's i).  Seven kinds: the packed word has three bits for them
enum { KB_F = 1, KB_C = 2, KB_M = 3, KB_M2 = 4, KB_FC = 5, KB_FA = 6, KB_FB = 7 };
__device__ __forceinline__ int kb_pack(int kind, int i, int j, int r) { return i | (j << 12) | (kind << 24) | (r << 27); }

template <int K, bool CO>
struct KbNick {};
template <int K>
struct KbNick<K, true> {           // two strands (F is Fu there)
  const TopK<K>*Fc, *fcA, *fcB;
  int cut;
};
template <int K, bool CO>
struct KbCtx : KbNick<K, CO> {
  const KbSmem<K>* sm;
  const MfeTables* T;
  const Plan* P;
  const int* hp_len;
  const TopK<K>*C, *M, *M2, *F;
  int n, ld;
};

// candidates of element e of a table entry whose value is v; returns how many of them reproduce v and, when sel >= 0,
// leaves the children of the sel-th such candidate in (ca, cb) (0 = no child).  The candidates are the terms of kbest_fill /
// kbest_exterior, with the same conditions; CO adds the nick rules and the levels next to the nick
template <int K, bool CO>
__device__ int kb_enum(const KbCtx<K, CO>& X, int kind, int i, int j, int v, int e, int sel, int& ca, int& cb) {
  const KbSmem<K>& sm = *X.sm;
  const MfeTables& T = *X.T;
  const int ld = X.ld, n = X.n, HALF = INF_DEV / 2;
  int cut = 0;
  if constexpr (CO) cut = X.cut;
  constexpr int D0 = CO ? 1 : TURN + 1;
  int cnt = 0;
#define KB_HIT(A_, B_) do { if (cnt == sel) { ca = (A_); cb = (B_); } cnt++; } while (0)
  if (kind == KB_F || (CO && kind == KB_FC)) {
    const bool conn = CO && kind == KB_FC;
    const TopK<K>* own = X.F;
    if constexpr (CO) { if (conn) own = X.Fc; }
    const int ok = conn ? KB_FC : KB_F;
    if (e == 0) {
      const TopK<K> f = own[j - 1];
      for (int a = 0; a < K; a++) if (f.v[a] < HALF && f.v[a] == v) KB_HIT(kb_pack(ok, 0, j - 1, a), 0);
    } else {
      const int p = e;
      const bool same = !CO || co_same(p, j, cut);
      const int t = (!CO || j - p > TURN || !same) ? pair_type(sm.S[p], sm.S[j]) : 0;
      if (t && (same || conn)) {
        // (two strands) the one exterior-level pair that joins the strands leads from Fc to Fu
        const TopK<K> c = X.C[(j - p) * ld + p], f = (same ? own : X.F)[p - 1];
        const int fk = same ? ok : KB_F;
        int x = t > 2 ? T.TermAU : 0;
        if constexpr (CO) x += co_endstem(sm.mmExt, sm, t, p > 1 && co_same(p - 1, p, cut), sm.S[p - 1], j < n && co_same(j, j + 1, cut), sm.S[j + 1]);
        else x += mfe_extstem(sm, t, p, j, n);
        for (int a = 0; a < K; a++)
          for (int b = 0; b < K; b++)
            if (f.v[a] < HALF && c.v[b] < HALF && f.v[a] + c.v[b] + x == v) KB_HIT(kb_pack(fk, 0, p - 1, a), kb_pack(KB_C, p, j, b));
      }
    }
  } else if (kind == KB_C) {
    const int d = j - i;
    const bool same = !CO || co_same(i, j, cut);
    const int t = (!CO || d > TURN || !same) ? pair_type(sm.S[i], sm.S[j]) : 0;
    const int si1 = sm.S[i + 1], sj1 = sm.S[j - 1];
    const int tau = t > 2 ? T.TermAU : 0;
    if (CO && !t) return 0;
    if (e == 0) {
      if (same && mfe_hairpin_e(sm, T, X.hp_len[d - 1], i, j, t) == v) KB_HIT(0, 0);
      const bool adj_i = !CO || co_same(i, i + 1, cut), adj_j = !CO || co_same(j - 1, j, cut);
      if constexpr (CO)
        if (!same) {
          const TopK<K> fa = X.fcA[i + 1], fb = X.fcB[j - 1];
          const int x = tau + co_endstem(sm.mmExt, sm, rtype_of(t), adj_j, sj1, adj_i, si1);
          for (int a = 0; a < K; a++)
            for (int b = 0; b < K; b++)
              if (fa.v[a] < HALF && fb.v[b] < HALF && fa.v[a] + fb.v[b] + x == v) KB_HIT(kb_pack(KB_FA, i + 1, 0, a), kb_pack(KB_FB, j - 1, 0, b));
        }
      if (adj_i && adj_j && (!CO || d >= 2)) {
        const TopK<K> m2 = X.M2[(d - 2) * ld + i + 1];
        const int x = T.MLclosing + T.MLintern + tau + sm.mmM[rtype_of(t) * 16 + sj1 * 4 + si1];
        for (int a = 0; a < K; a++) if (m2.v[a] < HALF && m2.v[a] + x == v) KB_HIT(kb_pack(KB_M2, i + 1, j - 1, a), 0);
      }
    } else {
      const int u1 = X.P->u1[e - 1], u2 = X.P->u2[e - 1];
      const int dp = d - 2 - u1 - u2;
      const int p = i + 1 + u1, q = j - 1 - u2;
      if (dp >= D0 && (!CO || (co_same(i, p, cut) && co_same(q, j, cut)))) {
        const int t2 = pair_type(sm.S[p], sm.S[q]);
        if (t2) {
          const TopK<K> c = X.C[dp * ld + p];
          const int info = (rtype_of(t2) << 4) | (sm.S[q + 1] << 2) | sm.S[p - 1];
          const int x = mfe_intloop(sm, T, u1, u2, t, si1, sj1, info);
          for (int a = 0; a < K; a++) if (c.v[a] < HALF && c.v[a] + x == v) KB_HIT(kb_pack(KB_C, p, q, a), 0);
        }
      }
    }
  } else if (!CO || kind == KB_M || kind == KB_M2) {
    const int d = j - i;
    const TopK<K>* own = kind == KB_M ? X.M : X.M2;
    if (e == 0) {
      if (!CO || co_same(j - 1, j, cut)) {
        const TopK<K> m = own[(d - 1) * ld + i];
        for (int a = 0; a < K; a++) if (m.v[a] < HALF && m.v[a] + T.MLbase == v) KB_HIT(kb_pack(kind, i, j - 1, a), 0);
      }
    } else {
      const int k = i + e - 1;
      const int tk = (!CO || j - k > TURN || !co_same(k, j, cut)) ? pair_type(sm.S[k], sm.S[j]) : 0;
      if (tk) {
        const TopK<K> c = X.C[(j - k) * ld + k];
        int st = T.MLintern + (tk > 2 ? T.TermAU : 0);
        if constexpr (CO) st += co_endstem(sm.mmM, sm, tk, k > 1 && co_same(k - 1, k, cut), sm.S[k - 1], j < n && co_same(j, j + 1, cut), sm.S[j + 1]);
        else st += sm.mmM[tk * 16 + sm.S[k - 1] * 4 + sm.S[j + 1]];
        if (kind == KB_M && (!CO || co_same(i, k, cut)))
          for (int a = 0; a < K; a++) if (c.v[a] < HALF && c.v[a] + (k - i) * T.MLbase + st == v) KB_HIT(kb_pack(KB_C, k, j, a), 0);
        if (k > i && (!CO || k - 1 != cut)) {
          const TopK<K> m = X.M[(k - 1 - i) * ld + i];
          for (int a = 0; a < K; a++)
            for (int b = 0; b < K; b++)
              if (m.v[a] < HALF && c.v[b] < HALF && m.v[a] + c.v[b] + st == v) KB_HIT(kb_pack(KB_M, i, k - 1, a), kb_pack(KB_C, k, j, b));
        }
      }
    }
  } else if constexpr (CO) {
    if (kind == KB_FA) {
      // fcA[x] of [x .. cut]: x unpaired, or x pairs with k <= cut and fcA[k + 1] follows
      const int x = i;
      if (e == 0) {
        const TopK<K> f = X.fcA[x + 1];
        for (int a = 0; a < K; a++) if (f.v[a] < HALF && f.v[a] == v) KB_HIT(kb_pack(KB_FA, x + 1, 0, a), 0);
      } else {
        const int k = x + e;
        const int t = pair_type(sm.S[x], sm.S[k]);
        if (t) {
          const TopK<K> c = X.C[(k - x) * ld + x], f = X.fcA[k + 1];
          const int ext = (t > 2 ? T.TermAU : 0) + co_endstem(sm.mmExt, sm, t, x > 1, sm.S[x - 1], k < cut, sm.S[k + 1]);
          for (int a = 0; a < K; a++)
            for (int b = 0; b < K; b++)
              if (c.v[a] < HALF && f.v[b] < HALF && c.v[a] + f.v[b] + ext == v) KB_HIT(kb_pack(KB_C, x, k, a), kb_pack(KB_FA, k + 1, 0, b));
        }
      }
    } else {
      // fcB[y] of [cut + 1 .. y]: y unpaired, or y pairs with k > cut and fcB[k - 1] precedes
      const int y = i;
      if (e == 0) {
        const TopK<K> f = X.fcB[y - 1];
        for (int a = 0; a < K; a++) if (f.v[a] < HALF && f.v[a] == v) KB_HIT(kb_pack(KB_FB, y - 1, 0, a), 0);
      } else {
        const int k = cut + e;
        const int t = pair_type(sm.S[k], sm.S[y]);
        if (t) {
          const TopK<K> f = X.fcB[k - 1], c = X.C[(y - k) * ld + k];
          const int ext = (t > 2 ? T.TermAU : 0) + co_endstem(sm.mmExt, sm, t, k > cut + 1, sm.S[k - 1], y < n, sm.S[y + 1]);
          for (int a = 0; a < K; a++)
            for (int b = 0; b < K; b++)
              if (f.v[a] < HALF && c.v[b] < HALF && f.v[a] + c.v[b] + ext == v) KB_HIT(kb_pack(KB_FB, k - 1, 0, a), kb_pack(KB_C, k, y, b));
        }
      }
    }
  }
#undef KB_HIT
  return cnt;
}

template <int NT, int K>
__global__ __launch_bounds__(NT) void kbest_kernel(SuboptArgs A) {
  __shared__ KbSmem<K> sm;
  const MfeTables& T = *A.T;
  const Plan& P = *A.plan;
  const int r = blockIdx.x;
  const int n = A.L, ld = A.ld;
  const int tid = threadIdx.x, lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());
  const int HALF = INF_DEV / 2;
  TopK<K>*C, *M, *M2;
  kb_tables(A, r, C, M, M2);
  TopK<K>* F = C;                                       // rows 0 .. TURN of C are never read: row 0 holds F[0 .. n]
  int32_t* stacks = reinterpret_cast<int32_t*>(M2);     // rows 0, 1 of M2 are never read: one traceback stack of ld ints per rank

  stage_energy_tables<NT>(sm, T, tid);
  // (the sequence load of load_sequence, written out: with the initial stores below moved ahead of it the K = 8 instance takes
  // 84 VGPRs instead of 76, one wave less per SIMD)
  if (tid == 0) sm.flag = 0;
  __syncthreads();
  const char* seq = A.seqs + (long long)r * n;
  for (int k = tid; k < n; k += NT) {
    const int c = enc_nt(seq[k]);
    if (c < 0) sm.flag = 1;
    sm.S[k + 1] = (unsigned char)(c < 0 ? 0 : c);
  }
  TopK<K> none;
  tk_init(none);
  for (int d = 0; d <= TURN && d < n; d++)
    for (int k = tid; k < ld; k += NT) { if (d) C[d * ld + k] = none; M[d * ld + k] = none; if (d > 1) M2[d * ld + k] = none; }
  for (int x = tid; x < K * n; x += NT) A.ss[(long long)r * K * n + x] = '.';
  __syncthreads();
  if (tid == 0) { sm.S[0] = sm.S[n]; sm.S[n + 1] = sm.S[1]; }
  __syncthreads();
  if (sm.flag) {
    if (tid == 0) { A.status[r] = ST_BAD_CHAR; for (int k = 0; k < K; k++) A.E[r * K + k] = INF_REF; }
    return;
  }
  kbest_fill<NT, K, false>(sm, A, C, M, M2, lane, wave);
  if (wave == 0) {
    kbest_exterior<K, false>(sm, T, C, F, nullptr, n, 0, ld);
    if (lane == 0) {
      A.status[r] = ST_OK;
      for (int k = 0; k < K; k++) A.E[r * K + k] = F[n].v[k] >= HALF ? INF_REF : F[n].v[k];
    }
  }
  __syncthreads();

  // ---- one traceback per rank; a wave works on one rank at a time, every lane holds the same state
  KbCtx<K, false> X;
  X.sm = &sm; X.T = &T; X.P = &P; X.hp_len = A.hp_len; X.C = C; X.M = M; X.M2 = M2; X.F = F; X.n = n; X.ld = ld;
  for (int rank = wave; rank < K; rank += NT / WAVE) {
    if (F[n].v[rank] >= HALF) continue;
    char* db = sm.db[rank];
    for (int x = lane; x <= n; x += WAVE) db[x] = '.';
    (void)__ballot(true);                            // the dots are in place before any lane writes a bracket
    int32_t* stk = stacks + (long long)rank * ld;
    int sp = 0;
    bool bad = false;
    stk[sp++] = kb_pack(KB_F, 0, n, rank);
    while (sp > 0 && !bad) {
      const int it = stk[--sp];
      const int i = it & 4095, j = (it >> 12) & 4095, kind = (it >> 24) & 7, rk = it >> 27;
      if (kind == KB_F && j == 0) continue;
      const TopK<K>* tabp = kind == KB_F ? F + j : kind == KB_C ? C + (j - i) * ld + i : kind == KB_M ? M + (j - i) * ld + i : M2 + (j - i) * ld + i;
      const int v = tabp->v[rk];
      int m = 0;
      for (int a = 0; a < rk; a++) m += tabp->v[a] == v;
      if (kind == KB_C) { db[i] = '('; db[j] = ')'; }
      const int nel = kind == KB_F ? 1 + max(j - TURN - 1, 0) : kind == KB_C ? 1 + NPLAN : 1 + max(j - TURN - i, 0);
      bool found = false;
      int ca = 0, cb = 0;
      for (int b0 = 0; b0 < nel && !found; b0 += WAVE) {
        const int e = b0 + lane;
        int da = 0, dbb = 0;
        const int cnt = e < nel ? kb_enum<K, false>(X, kind, i, j, v, e, -1, da, dbb) : 0;
        int pre = cnt;                               // inclusive prefix over the lanes (= over the elements, in order)
        for (int o = 1; o < WAVE; o <<= 1) {
          const int x = __shfl(pre, lane >= o ? lane - o : lane);
          if (lane >= o) pre += x;
        }
        const int total = __shfl(pre, WAVE - 1);
        if (m < total) {
          const unsigned long long mask = __ballot(pre > m);
          const int win = __ffsll((long long)mask) - 1;
          const int sel = m - (__shfl(pre, win) - __shfl(cnt, win));
          if (lane == win) kb_enum<K, false>(X, kind, i, j, v, e, sel, da, dbb);
          ca = __shfl(da, win); cb = __shfl(dbb, win);
          found = true;
        } else m -= total;
      }
      if (!found) { bad = true; break; }
      if (cb) stk[sp++] = cb;
      if (ca) stk[sp++] = ca;
    }
    (void)__ballot(true);
    if (bad) { if (lane == 0) A.status[r] = ST_TRACEBACK; continue; }
    for (int x = lane; x < n; x += WAVE) A.ss[((long long)r * K + rank) * n + x] = db[x + 1];
  }
}

}  // namespace drna
