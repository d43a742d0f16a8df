// fold_mea.hpp -- the two structures that represent an ensemble, from its pair probabilities, on gfx950: the maximum-expected-
// accuracy (MEA) structure for a weight gamma and the centroid (ViennaRNA's fc.MEA(gamma), fc.centroid()).  Runs after the outside
// pass (fold_outside.hpp, fold_cofold_outside.hpp, fold_edef_lds.hpp) on the matrix that pass wrote: P(i,j), 1 <= i < j <= n, at
// bpp[i (n+1) + j].  The kernel reads the matrix only, so one kernel serves one strand and two (pair type, hairpin length and the
// nick are all in P > 0).  ONE WORKGROUP PER SEQUENCE.
//
//   q(i)     = 1 - sum_j P(min(i,j), max(i,j))                      summed in ascending j, not clamped
//   EA(s)    = sum_{i unpaired in s} q(i) + 2 gamma sum_{(i,j) in s} P(i,j)
//   M(i,i-1) = 0
//   M(i,j)   = max( M(i,j-1) + q(j),  max_{i <= k < j, P(k,j) > 0}  M(i,k-1) + M(k+1,j-1) + 2 gamma P(k,j) ),    value M(1,n)
// TIE RULE: "j unpaired" first, then k ascending; a later candidate replaces only if it is strictly greater.
//
// Prologue: q(.) and, per column j, the list of its candidates k (ascending) with w = (2 gamma) P(k,j).  A pair with
// 2 gamma P(k,j) < q(k) + q(j) is left out: M(i,j) >= M(i,j-1) + q(j) >= M(i,k-1) + q(k) + M(k+1,j-1) + q(j) (structures of two
// neighbouring segments concatenate), so such a pair is strictly worse than its two ends unpaired and never attains a maximum --
// the fill is O(n^2 c) for c candidates per column instead of O(n^3).  The lists live in LDS while they hold at most MEA_CAND_LDS
// pairs in all, else behind M in the sequence's slot of the outside workspace (free once bpp is written).
// Fill by diagonals (segment length 1 .. n): groups of MEA_GW lanes own cells, the lanes of a group split the column's candidates,
// and a fixed-order butterfly takes the maximum (greater value, then smaller k: the tie rule whatever the split).  M is a packed
// triangle, rows by segment length: in LDS up to MEA_LDS_MAX nucleotides, else at the start of the workspace slot -- the same
// template over the table's location, so both give the same bits.
// Traceback by one wave: mea_cell() again on the stored doubles -- the one expression the fill used -- gives the winning case.
// Then, same workgroup: the centroid {P > 0.5} and its distance sum_{c} (1 - P) + sum_{not c} P, and (E given) the energy of both
// structures by eval_loaded (eval_structure.hpp; cut and DuplexInit for two strands).  No multiplication feeds an addition
// anywhere here (w is stored before it is added), so there is nothing for the compiler to contract.
#pragma once
#include <math.h>

#include "eval_structure.hpp"

namespace drna {

constexpr int MEA_GW = 8;                      // lanes per cell of the fill
constexpr int MEA_CAND_LDS = 4096;             // candidate pairs (all columns) the LDS lists hold
constexpr int MEA_SEG = MAXN / 2 + 8;          // pending segments of the traceback: one per open pair
constexpr int MEA_LDS_BYTES = 160 * 1024;

struct MeaArgs {
  EvalArgs ev;                     // tables of the loop energies, seqs (R x L; unused when E is null), L, cut, DuplexInit
  const double* bpp = nullptr;     // R x (L+1) x (L+1)
  double* ws = nullptr;            // outside workspace: M (when not in LDS) and candidate lists that overflow LDS
  long long ws_stride = 0;         // doubles per sequence, at least 3 (L+2)^2
  double gamma = 1.0;
  char* mea_ss = nullptr;          // R x L
  double* mea_val = nullptr;       // R
  char* cen_ss = nullptr;          // R x L
  double* cen_dist = nullptr;      // R
  int32_t* E = nullptr;            // R x 2 (dcal/mol): MEA, centroid; or null
  int32_t* ncand = nullptr;        // R: candidates the pruning left, all columns; or null
};

template <int NMAX>
struct MeaSmemT {
  double M[(NMAX + 1) * (NMAX + 2) / 2];
  double q[MAXN + 2];
  double cw[MEA_CAND_LDS];
  double part[16];
  int cstart[MAXN + 2];            // candidates of column j: cstart[j] .. cstart[j+1] - 1
  int seg[MEA_SEG];                // i | j << 12
  short ck[MEA_CAND_LDS];
  EvalSmem ev;                     // codes and the pair table of the structure being written
};
constexpr int MEA_LDS_MAX = 146;               // longest sequence whose M stays in LDS
static_assert(sizeof(MeaSmemT<MEA_LDS_MAX>) <= MEA_LDS_BYTES, "MEA_LDS_MAX: the triangle no longer fits the CU's LDS");
static_assert(sizeof(MeaSmemT<MEA_LDS_MAX + 1>) > MEA_LDS_BYTES, "MEA_LDS_MAX: one more nucleotide fits the CU's LDS");
static_assert(MAXN <= 4096, "a traceback segment packs i and j into 12 bits each");
using MeaSmem = MeaSmemT<MEA_LDS_MAX>;

// M(i,j), 1 <= i <= n + 1, i - 1 <= j <= n: row = segment length j - i + 1 (n + 1 - len cells), then i
__device__ __forceinline__ int mea_at(int n, int i, int j) {
  const int len = j - i + 1;
  return len * (n + 1) - len * (len - 1) / 2 + i - 1;
}
__device__ __forceinline__ bool mea_keep(double p, double tg, double qk, double qj) { return p > 0.0 && !(tg * p < qk + qj); }

struct MeaCands {
  const int* cstart;
  const short* ck;
  const double* cw;
};
struct MeaBest {
  double v;
  int k;                           // 0: j unpaired
};

// The best case of cell (i,j), i <= j, by the group of MEA_GW lanes that `sub` counts; every lane of the group ends with the same
// answer.  All 64 lanes of a wave must come here together (live = false: a group without a cell).
__device__ __forceinline__ MeaBest mea_cell(const double* M, const double* q, const MeaCands& C, int n, int i, int j, int sub, bool live) {
  double best = -INFINITY;
  int bk = 0x7fffffff;
  if (live) {
    const int c1 = C.cstart[j + 1];
    for (int c = C.cstart[j] + sub; c < c1; c += MEA_GW) {
      const int k = C.ck[c];
      if (k < i) continue;
      const double v = M[mea_at(n, i, k - 1)] + M[mea_at(n, k + 1, j - 1)] + C.cw[c];
      if (v > best) { best = v; bk = k; }
    }
  }
#pragma unroll
  for (int o = MEA_GW / 2; o > 0; o >>= 1) {
    const double ov = __shfl_xor(best, o);
    const int ok = __shfl_xor(bk, o);
    if (ov > best || (ov == best && ok < bk)) { best = ov; bk = ok; }
  }
  MeaBest b{-INFINITY, 0};
  if (live) {
    b.v = M[mea_at(n, i, j - 1)] + q[j];
    if (best > b.v) { b.v = best; b.k = bk; }
  }
  return b;
}

// the structure in sm.ev.pt as n characters, and (E given) its energy, by one wave
template <class SM>
__device__ __forceinline__ void mea_emit(const SM& sm, const MeaArgs& A, int n, int lane, char* out, int32_t* E) {
  for (int x = lane; x < n; x += WAVE) {
    const int p = sm.ev.pt[x + 1];
    out[x] = p == 0 ? '.' : p > x + 1 ? '(' : ')';
  }
  if (E) {
    const int e = eval_loaded(sm.ev, A.ev, n, lane);
    if (lane == 0) *E = e;
  }
}

template <int NT, bool INLDS>
__global__ __launch_bounds__(NT) void mea_kernel(MeaArgs A) {
  static_assert(NT % WAVE == 0 && NT / WAVE <= 16 && WAVE % MEA_GW == 0, "whole waves, one partial sum each");
  __shared__ MeaSmem sm;
  const int r = blockIdx.x, n = A.ev.L, tid = threadIdx.x, lane = lane_id();
  const int wave = wave_id();
  const int ld = n + 2;
  const double* __restrict__ B = A.bpp + (long long)r * (n + 1) * (n + 1);
  double* slot = A.ws + (long long)r * A.ws_stride;
  double* M;
  if constexpr (INLDS) M = sm.M; else M = slot;
  double* wcw = slot + (long long)ld * ld;
  short* wck = reinterpret_cast<short*>(slot + 2ll * ld * ld);
  const double tg = 2.0 * A.gamma;

  // ---- prologue: q, the lists, the empty segments; codes for the energies
  for (int i = 1 + tid; i <= n; i += NT) {
    double s = 0.0;
    for (int j = 1; j < i; j++) s += B[j * (n + 1) + i];
    for (int j = i + 1; j <= n; j++) s += B[i * (n + 1) + j];
    sm.q[i] = 1.0 - s;
  }
  for (int x = tid; x < n + 2; x += NT) { sm.ev.pt[x] = 0; sm.ev.S[x] = 0; }
  for (int x = tid; x <= n; x += NT) M[x] = 0.0;                    // row 0: M(i, i-1), i = 1 .. n + 1
  __syncthreads();
  if (A.E) {
    const char* seq = A.ev.seqs + (long long)r * n;
    for (int x = tid; x < n; x += NT) {
      const int c = enc_nt(seq[x]);
      sm.ev.S[x + 1] = (unsigned char)(c < 0 ? 0 : c);
    }
    __syncthreads();
    if (tid == 0) { sm.ev.S[0] = sm.ev.S[n]; sm.ev.S[n + 1] = sm.ev.S[1]; }
  }
  for (int j = 1 + tid; j <= n; j += NT) {
    const double qj = sm.q[j];
    int cnt = 0;
#pragma unroll 4
    for (int k = 1; k < j; k++) cnt += mea_keep(B[k * (n + 1) + j], tg, sm.q[k], qj) ? 1 : 0;
    sm.cstart[j] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    int at = 0;
    for (int j = 1; j <= n; j++) { const int c = sm.cstart[j]; sm.cstart[j] = at; at += c; }
    sm.cstart[n + 1] = at;
    if (A.ncand) A.ncand[r] = at;
  }
  __syncthreads();
  const bool cl = sm.cstart[n + 1] <= MEA_CAND_LDS;
  for (int j = 1 + tid; j <= n; j += NT) {
    const double qj = sm.q[j];
    int at = sm.cstart[j];
#pragma unroll 4
    for (int k = 1; k < j; k++) {
      const double p = B[k * (n + 1) + j];
      if (mea_keep(p, tg, sm.q[k], qj)) {
        if (cl) { sm.ck[at] = (short)k; sm.cw[at] = tg * p; }
        else { wck[at] = (short)k; wcw[at] = tg * p; }
        at++;
      }
    }
  }
  __syncthreads();
  const MeaCands CL{sm.cstart, sm.ck, sm.cw}, CW{sm.cstart, wck, wcw};       // (a wave-uniform choice between two inlined bodies, not one pointer into either memory)

  // ---- fill
  const int sub = tid & (MEA_GW - 1), grp = tid / MEA_GW;
  constexpr int NG = NT / MEA_GW;
  for (int len = 1; len <= n; len++) {
    const int ncell = n - len + 1;
    for (int base = 0; base < ncell; base += NG) {
      const int i = base + grp + 1, j = i + len - 1;
      const bool live = base + grp < ncell;
      const MeaBest b = cl ? mea_cell(M, sm.q, CL, n, i, j, sub, live) : mea_cell(M, sm.q, CW, n, i, j, sub, live);
      if (live && sub == 0) M[mea_at(n, i, j)] = b.v;
    }
    __syncthreads();
  }

  // ---- traceback and the MEA structure's outputs
  if (wave == 0) {
    // every lane pushes and pops the same words: a lane reads back what it has stored itself
    int sp = 0;
    sm.seg[sp++] = 1 | (n << 12);
    while (sp > 0) {
      const int word = sm.seg[--sp];
      const int i = word & 4095;
      int j = word >> 12;
      while (j >= i) {
        const MeaBest b = cl ? mea_cell(M, sm.q, CL, n, i, j, sub, true) : mea_cell(M, sm.q, CW, n, i, j, sub, true);
        if (b.k == 0) { j--; continue; }
        if (lane == 0) { sm.ev.pt[b.k] = (short)j; sm.ev.pt[j] = (short)b.k; }
        if (b.k + 1 <= j - 1 && sp < MEA_SEG) sm.seg[sp++] = (b.k + 1) | ((j - 1) << 12);
        j = b.k - 1;
      }
    }
    wave_lds_sync();
    if (lane == 0) A.mea_val[r] = M[mea_at(n, 1, n)];
    mea_emit(sm, A, n, lane, A.mea_ss + (long long)r * n, A.E ? A.E + 2ll * r : nullptr);
  }
  __syncthreads();

  // ---- centroid
  for (int x = tid; x < n + 2; x += NT) sm.ev.pt[x] = 0;
  __syncthreads();
  double acc = 0.0;
  const int cells = (n + 1) * (n + 1);
  for (int x = tid; x < cells; x += NT) {
    const int i = x / (n + 1), j = x - i * (n + 1);
    if (i < 1 || j <= i) continue;
    const double p = B[x];
    if (p > 0.5) { sm.ev.pt[i] = (short)j; sm.ev.pt[j] = (short)i; acc += 1.0 - p; }
    else acc += p;
  }
  acc = wave_sum_f64(acc);
  if (lane == 0) sm.part[wave] = acc;
  __syncthreads();
  if (wave == 0) {
    if (lane == 0) {
      double d = 0.0;
      for (int w = 0; w < NT / WAVE; w++) d += sm.part[w];
      A.cen_dist[r] = d;
    }
    mea_emit(sm, A, n, lane, A.cen_ss + (long long)r * n, A.E ? A.E + 2ll * r + 1 : nullptr);
  }
}

}  // namespace drna
