// fold_cofold_subopt.hpp -- energy of the second-best co-fold structure of one sequence pair per workgroup on gfx950, and (second
// half of the file) its K lowest-energy co-fold structures with their strings.
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


// ---------------------------------------------------------------------------------------------------------------------
// cofold_kbest_kernel: the K lowest-energy co-fold structures (energies AND dot-bracket strings) of one sequence pair per
// workgroup.  Replaces get_first_suboptimal_structure_and_energy(seq, fc, k)[0] on the DIMER fold compound, the call behind
// get_alt_mcc() for a two-strand design with alternative structures (utils/sequence_utils.py:766-793).  kbest_fill<NT, K, true>
// and kbest_exterior<K, true> as above, E = topK(Fu[n] ; Fc[n] + DuplexInit), then one traceback per rank (cofold_kb_trace over
// kb_enum<K, true> of fold_subopt.hpp) through every level the fill wrote: Fu / Fc, C (with the nick loop), M, M2, fcA, fcB.
//
// The two-strand sweep starts at diagonal 1 and reads rows 0 of C, M and M2 as empty lists, and the traceback re-reads them, so
// nothing else may live there (kbest_kernel keeps F and its stacks in such rows).  All four 1-D lists stay live until the last
// rank is traced (the nick loop is traced through fcA / fcB), 4 x 64 KB at K = 8 and MAXN: they and the stacks lie behind the
// three tables in the pair's workspace slot, cofold_kbest_ws_extra(K, ld) int32, so any L up to MAXN is served.
__host__ __device__ inline long long cofold_kbest_ws_extra(int K, int ld) { return (long long)5 * K * (ld + 2); }

template <int K>
struct CoKbSmem : KbSmem<K> {
  TopK<K>*fcA, *fcB;              // ld + 2 lists each in the workspace slot (the fill only indexes them)
};

// one traceback by the calling wave (every lane holds the same state): expands the item `root` into db[1 .. n] ('.' on entry);
// the loop of kbest_kernel with the levels next to the nick, over the same kb_enum.  stk holds cap words.  False: a table value
// could not be reproduced, or the stack or the number of expansions passed its bound (8 n + 16: every step consumes a position,
// closes a pair or splits off a stem, fewer than 4 n + 8 in all) -- a status word for the caller, never a spinning wave
template <int K>
__device__ __forceinline__ bool cofold_kb_trace(const KbCtx<K, true>& X, char* db, int32_t* stk, int cap, int root, int lane) {
  // (copies: X itself is handed to kb_enum by address)
  const int n = X.n, ld = X.ld, cut = X.cut;
  const TopK<K>*F = X.F, *C = X.C, *M = X.M, *M2 = X.M2, *Fc = X.Fc, *fcA = X.fcA, *fcB = X.fcB;
  int sp = 0, pops = 8 * n + 16;
  stk[sp++] = root;
  while (sp > 0) {
    if (--pops < 0 || sp + 1 > cap) return false;     // (an expansion pops one word and pushes two at most)
    const int it = stk[--sp];
    const int i = it & 4095, j = (it >> 12) & 4095, kind = (it >> 24) & 7, rk = (it >> 27) & 7;
    if (kind == KB_F && j == 0) continue;
    if ((kind == KB_FA && i > cut) || (kind == KB_FB && i <= cut)) continue;       // the empty segment next to the nick
    const TopK<K>* tabp = kind == KB_F ? F + j : kind == KB_FC ? Fc + j : kind == KB_FA ? fcA + i : kind == KB_FB ? fcB + i
                          : (kind == KB_C ? C : kind == KB_M ? M : M2) + (j - i) * ld + i;
    const int v = tabp->v[rk];
    int m = 0;
    for (int a = 0; a < rk; a++) m += tabp->v[a] == v;
    if (kind == KB_C) { db[i] = '('; db[j] = ')'; }
    // elements: the "unpaired" / loop-closing one, then one per pairing partner (C: per interior-loop shape)
    const int nel = kind == KB_F || kind == KB_FC ? 1 + max(j - 1, 0) : kind == KB_C ? 1 + NPLAN
                    : kind == KB_FA ? 1 + max(cut - i, 0) : kind == KB_FB ? 1 + max(i - cut - 1, 0) : 1 + max(j - i, 0);
    bool found = false;
    int ca = 0, cb = 0;
    for (int b0 = 0; b0 < nel && !found; b0 += WAVE) {
      const int e = b0 + lane;
      int da = 0, dbb = 0;
      const int cnt = e < nel ? kb_enum<K, true>(X, kind, i, j, v, e, -1, da, dbb) : 0;
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
        if (lane == win) kb_enum<K, true>(X, kind, i, j, v, e, sel, da, dbb);
        ca = __shfl(da, win); cb = __shfl(dbb, win);
        found = true;
      } else m -= total;
    }
    if (!found) return false;
    if (cb) stk[sp++] = cb;
    if (ca) stk[sp++] = ca;
  }
  return true;
}

template <int NT, int K>
__global__ __launch_bounds__(NT) void cofold_kbest_kernel(SuboptArgs A) {
  __shared__ CoKbSmem<K> sm;
  const MfeTables& T = *A.T;
  const int r = blockIdx.x;
  const int n = A.L, cut = A.cut, ld = A.ld;
  const int tid = threadIdx.x, lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());
  const int HALF = INF_DEV / 2;
  TopK<K>*C, *M, *M2;
  kb_tables(A, r, C, M, M2);
  TopK<K>* lists = M2 + (long long)ld * ld;            // behind the three tables: fcA, fcB, Fu, Fc, then K stacks of ld + 2 words
  TopK<K>*fcA = lists, *fcB = lists + (ld + 2), *Fu = lists + 2 * (ld + 2), *Fc = lists + 3 * (ld + 2);
  int32_t* stacks = reinterpret_cast<int32_t*>(lists + 4 * (ld + 2));

  stage_energy_tables<NT>(sm, T, tid);
  // row 0 (single nucleotides): no pair, no multiloop content
  TopK<K> none, one;
  tk_init(none);
  one = none;
  one.v[0] = 0;
  for (int k = tid; k < ld; k += NT) { C[k] = none; M[k] = none; M2[k] = none; }
  for (int k = tid; k <= n + 2; k += NT) { fcA[k] = one; fcB[k] = one; }                 // empty / one-nt segments
  for (int x = tid; x < K * n; x += NT) A.ss[(long long)r * K * n + x] = '.';
  if (tid == 0) { sm.fcA = fcA; sm.fcB = fcB; A.status[r] = ST_OK; }
  load_sequence<NT>(sm, A.seqs + (long long)r * n, n, tid);
  if (sm.flag) {
    if (tid == 0) { A.status[r] = ST_BAD_CHAR; for (int k = 0; k < K; k++) A.E[r * K + k] = INF_REF; }
    return;
  }
  kbest_fill<NT, K, true>(sm, A, C, M, M2, lane, wave);
  if (wave == 0) kbest_exterior<K, true>(sm, T, C, Fu, Fc, n, cut, ld);
  __syncthreads();
  // the merged list, in every lane: Fu entries first among equal values
  TopK<K> fin = Fu[n];
  const TopK<K> fcn = Fc[n];
  tk_add_sum(fin, fcn, A.DuplexInit);
  if (tid == 0)
    for (int k = 0; k < K; k++) A.E[r * K + k] = fin.v[k] >= HALF ? INF_REF : fin.v[k];

  // ---- one traceback per rank; a wave works on one rank at a time, every lane holds the same state
  KbCtx<K, true> X;
  X.sm = &sm; X.T = &T; X.P = A.plan; X.hp_len = A.hp_len; X.C = C; X.M = M; X.M2 = M2; X.F = Fu; X.n = n; X.ld = ld;
  X.Fc = Fc; X.fcA = fcA; X.fcB = fcB; X.cut = cut;
  for (int rank = wave; rank < K; rank += NT / WAVE) {
    const int v = fin.v[rank];
    if (v >= HALF) continue;
    // rank of the merged list -> (Fu[n], a) or (Fc[n], b): the candidate whose index among those of value v equals the number
    // of equal values ranked before it
    int m = 0, root = 0;
    for (int a = 0; a < rank; a++) m += fin.v[a] == v;
    for (int a = 0; a < K; a++) if (Fu[n].v[a] < HALF && Fu[n].v[a] == v && m-- == 0) root = kb_pack(KB_F, 0, n, a);
    for (int b = 0; b < K; b++) if (fcn.v[b] < HALF && fcn.v[b] + A.DuplexInit == v && m-- == 0) root = kb_pack(KB_FC, 0, n, b);
    char* db = sm.db[rank];
    for (int x = lane; x <= n; x += WAVE) db[x] = '.';
    (void)__ballot(true);                            // the dots are in place before any lane writes a bracket
    const bool ok = root && cofold_kb_trace<K>(X, db, stacks + (long long)rank * (ld + 2), ld + 2, root, lane);
    (void)__ballot(true);
    if (!ok) { if (lane == 0) A.status[r] = ST_TRACEBACK; continue; }
    for (int x = lane; x < n; x += WAVE) A.ss[((long long)r * K + rank) * n + x] = db[x + 1];
  }
}

}  // namespace drna
