// fold_sample.hpp -- stochastic traceback: structures drawn from the Boltzmann ensemble of a sequence on gfx950
// (ViennaRNA's pbacktrack, RNAsubopt -p).  Runs after pf_kernel (fold_pf.hpp) on the tables that kernel left in the workspace
// slot (QB, QBI, QM, QM1, QEXT, INFO; diagonal-major, pitch ld) and its q5[] column, as outside_kernel does; any 1 <= n <= max_L.
//
// ONE WAVE PER SAMPLE.  A launch is R x G workgroups; workgroup g of sequence r holds NW waves, and wave w of it takes the
// samples g NW + w, + G NW, ...  A sample is a walk over segments kept on a small stack in LDS:
//   EXT  [1..j]   q5[j]    = q5[j-1] scale + sum_i q5[i-1] QEXT[i,j]
//   PAIR (i,j)    qb[i,j]  = hairpin + sum over the loop plan (u1 + u2 <= 30) of qb[p,q] x loop + multiloop closing x sum_k qm[i+1,k-1] qm1[k,j-1]
//   QM   [i,j]    qm[i,j]  = qm1[i,j] + sum_k expMLbase^(k-i) qm1[k,j] + sum_k qm[i,k-1] qm1[k,j]
//   QM1  [i,j]    qm1[i,j] = sum_l qb[i,l] MLstem(i,l) expMLbase^(j-l)
// -- exactly the summands of pf_kernel's recurrences with their pf_scale powers.  A step is wave-uniform: the
// wave pops a segment, spreads its candidates over the lanes in a fixed order in chunks of 64 with a carried running sum, and takes
// the FIRST candidate whose cumulative weight exceeds u x (table value of the segment) by a wave prefix sum and a ballot; then it
// pushes the candidate's sub-segments.  The candidates are summed in another order than the fill used, so their sum can end a few
// ulp below the table value: if the threshold is never reached the LAST candidate of non-zero weight is taken.  Only cells the fill
// wrote are read (diagonals TURN + 1 .. n - 1, columns 1 .. n - d).
//
// Random numbers: u(seed_r, s, k) of sample_rng.hpp, k = index of the step within the sample -- sample s of a sequence depends on
// the sequence, its seed and s alone (not on S, R, the neighbours in the batch, the workgroup size or the grid).
// Output per sample: the structure as n bytes of ( ) . and its energy in dcal/mol by eval_structure.hpp's loop sum on the pair
// table the walk has built in LDS.  A sequence whose pf_kernel status is not OK writes nothing (the host reports it).
#pragma once
#include "eval_structure.hpp"
#include "fold_pf.hpp"
#include "sample_rng.hpp"

namespace drna {

// pending segments are disjoint intervals of at least TURN + 2 nucleotides
constexpr int SAMPLE_STACK = MAXN / 4 + 8;
enum : int { SG_EXT = 0, SG_PAIR = 1, SG_QM = 2, SG_QM1 = 3 };

struct SampleArgs {
  PfArgs pf;                    // what pf_kernel was launched with: tables, sequences, L, ld, workspace, status words, q5out / q5_stride
  EvalArgs ev;                  // T, hp_len, bulge_len, int_len (one strand)
  const uint64_t* seeds;        // R
  int S;                        // samples per sequence
  int G;                        // workgroups per sequence
  char* ss;                     // R x S x L
  int32_t* E;                   // R x S (dcal/mol) or null
};

struct SampleWaveSmem {
  EvalSmem ev;                  // codes and the pair table of the sample being drawn
  int seg[SAMPLE_STACK];        // kind | i << 2 | j << 14
};
template <int NW>
struct SampleSmem {
  double stack[64];
  double mmH[128], mmI[128], mm1n[128], mm23[128], mmM[128], mmExt[128];
  double int11[1024];
  double d5[32], d3[32];
  int plan_u[NPLAN];            // u1 | u2 << 8 | kind << 16
  double plan_W[NPLAN];
  unsigned char S[MAXN + 4];
  int flag;
  SampleWaveSmem w[NW];
};

// the tables of one sequence as the walk reads them
struct SampleTabs {
  const double *QB, *QBI, *QM, *QM1, *QEXT, *q5;
  const unsigned char* INFO;
  int n, ld, segG;
  double sc1, sc2;
};

template <class SM>
__device__ __forceinline__ double sample_endstem(const double* mm, const SM& sm, int t, int i, int j, int n) {   // = pf_endstem
  if (i > 1 && j < n) return mm[t * 16 + sm.S[i - 1] * 4 + sm.S[j + 1]];
  if (i > 1) return sm.d5[t * 4 + sm.S[i - 1]];
  if (j < n) return sm.d3[t * 4 + sm.S[j + 1]];
  return 1.0;
}

struct SamplePick {
  double thr, carry;
  int chosen, last;
};

// One chunk of 64 candidates: lane l holds candidate c0 + l with weight w (0: none).  True when the threshold is passed inside
// the chunk (p.chosen); else the running sum is carried on.  Every lane ends with the same p.
__device__ __forceinline__ bool sample_chunk(SamplePick& p, double w, int c0, int lane) {
  double cum = w;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {                     // inclusive prefix sum in a fixed order
    const double t = __shfl(cum, lane >= o ? lane - o : lane);
    if (lane >= o) cum += t;
  }
  cum += p.carry;
  const unsigned long long nz = __ballot(w > 0.0);
  const unsigned long long hit = __ballot(w > 0.0 && cum > p.thr);
  if (nz) p.last = c0 + 63 - __builtin_clzll(nz);
  if (hit) { p.chosen = c0 + __ffsll((long long)hit) - 1; return true; }
  p.carry = __shfl(cum, WAVE - 1);
  return false;
}

// candidate c of EXT [1..j]: 0 = j unpaired, i >= 1 = the pair (i,j)
__device__ __forceinline__ int sample_ext_count(int j) { return 1 + (j - TURN - 1 > 0 ? j - TURN - 1 : 0); }
__device__ __forceinline__ double sample_ext_weight(const SampleTabs& X, int j, int c) {
  if (c == 0) return X.q5[j - 1] * X.sc1;
  return X.q5[c - 1] * X.QEXT[j * X.ld + c];
}

// candidate c of PAIR (i,j): 0 = hairpin, 1 + e = entry e of the loop plan, 1 + NPLAN + m = multiloop with qm[i+1, i+1+tt],
// qm1[i+tt+2, j-1], tt = TURN + 1 + m
__device__ __forceinline__ int sample_pair_count(int d) { return 1 + NPLAN + (d - 2 * TURN - 4 > 0 ? d - 2 * TURN - 4 : 0); }
template <class SM>
__device__ __forceinline__ double sample_pair_weight(const SM& sm, const PfArgs& A, const SampleTabs& X, int i, int j, int c) {
  const PfTables& T = *A.T;
  const int d = j - i, ld = X.ld;
  const int t = pair_type(sm.S[i], sm.S[j]);
  if (!t) return 0.0;
  if (c == 0) return pf_hairpin(sm, A, i, j, t);
  const int si1 = sm.S[i + 1], sj1 = sm.S[j - 1];
  const double tau = t > 2 ? T.TermAU : 1.0;
  if (c <= NPLAN) {
    const int e = c - 1;
    const int pu = sm.plan_u[e];
    const int u1 = pu & 255, u2 = (pu >> 8) & 255;
    const int dp = d - 2 - u1 - u2;
    if (dp <= TURN) return 0.0;
    const int at = dp * ld + i + 1 + u1;
    const int ij = t * 16 + si1 * 4 + sj1;
    if (e >= X.segG) return X.QBI[at] * sm.plan_W[e] * sm.mmI[ij];
    const int info = X.INFO[at] & 127, t2 = info >> 4;
    double f;
    switch (pu >> 16) {
      case PK_STACK: f = sm.stack[t * 8 + t2]; break;
      case PK_BULGE1: f = sm.stack[t * 8 + t2]; break;
      case PK_BULGEN: f = tau * (t2 > 2 ? T.TermAU : 1.0); break;
      case PK_INT11: f = sm.int11[(t * 8 + t2) * 16 + si1 * 4 + sj1]; break;
      case PK_INT21: f = T.int21[(t * 8 + t2) * 64 + si1 * 16 + ((info >> 2) & 3) * 4 + sj1]; break;
      case PK_INT12: f = T.int21[(t2 * 8 + t) * 64 + ((info >> 2) & 3) * 16 + si1 * 4 + (info & 3)]; break;
      case PK_1XN: f = sm.mm1n[ij] * sm.mm1n[info]; break;
      case PK_INT22: f = T.int22[(t * 8 + t2) * 256 + si1 * 64 + (info & 3) * 16 + ((info >> 2) & 3) * 4 + sj1]; break;
      default: /* PK_INT23 */ f = sm.mm23[ij] * sm.mm23[info]; break;
    }
    return X.QB[at] * f * sm.plan_W[e];
  }
  const int tt = TURN + 1 + (c - NPLAN - 1), i1 = i + 1, d1 = d - 2;
  if (tt > d1 - TURN - 2) return 0.0;
  const double w = T.MLclosing * T.MLintern * tau * sm.mmM[rtype_of(t) * 16 + sj1 * 4 + si1] * X.sc2;
  return X.QM[tt * ld + i1] * X.QM1[(d1 - tt - 1) * ld + i1 + tt + 1] * w;
}

// candidate c of QM [i,j]: 0 = qm1[i,j]; 1 .. nU = unpaired prefix, qm1[i+c, j]; then the splits qm[i, k-1] qm1[k, j]
__device__ __forceinline__ int sample_qm_nU(int d) { return d - TURN - 1; }
__device__ __forceinline__ int sample_qm_count(int d) { return 1 + sample_qm_nU(d) + (d - 2 * TURN - 2 > 0 ? d - 2 * TURN - 2 : 0); }
__device__ __forceinline__ int sample_qm_split(int d, int c) { return c - sample_qm_nU(d) + TURN + 1; }       // k - i of split candidate c
__device__ __forceinline__ double sample_qm_weight(const PfArgs& A, const SampleTabs& X, int i, int j, int c) {
  const int d = j - i, ld = X.ld;
  if (c == 0) return X.QM1[d * ld + i];
  if (c <= sample_qm_nU(d)) return A.eMLb[c] * X.QM1[(d - c) * ld + i + c];
  const int k = sample_qm_split(d, c);
  return X.QM[(k - 1) * ld + i] * X.QM1[(d - k) * ld + i + k];
}

// candidate c of QM1 [i,j]: the pair (i, j - c), c unpaired bases behind it
__device__ __forceinline__ int sample_qm1_count(int d) { return d - TURN; }
template <class SM>
__device__ __forceinline__ double sample_qm1_weight(const SM& sm, const PfArgs& A, const SampleTabs& X, int i, int j, int c) {
  const PfTables& T = *A.T;
  const int l = j - c;
  const int t = pair_type(sm.S[i], sm.S[l]);
  if (!t) return 0.0;
  const double w = X.QB[(l - i) * X.ld + i] * T.MLintern * (t > 2 ? T.TermAU : 1.0) * sample_endstem(sm.mmM, sm, t, i, l, X.n);
  return c ? w * A.eMLb[c] : w;
}

__device__ __forceinline__ int sample_seg(int kind, int i, int j) { return kind | (i << 2) | (j << 14); }

// one sample by one wave: the pair table ends in W.ev.pt
template <class SM>
__device__ __forceinline__ void sample_walk(const SM& sm, SampleWaveSmem& W, const PfArgs& A, const SampleTabs& X, uint64_t key, int lane) {
  const int n = X.n, ld = X.ld;
  for (int x = lane; x < n + 2; x += WAVE) W.ev.pt[x] = 0;
  wave_lds_sync();
  // every lane pushes and pops the same words: a lane reads back what it has stored itself, no rendezvous needed
  int sp = 0;
  if (n > TURN + 1) W.seg[sp++] = sample_seg(SG_EXT, 1, n);
  for (int step = 0; sp > 0 && step < 4 * n + 8; step++) {
    const int word = __builtin_amdgcn_readfirstlane(W.seg[--sp]);
    const int kind = word & 3, i = (word >> 2) & 4095, j = word >> 14;
    const int d = j - i;
    int N;
    double tabv;
    if (kind == SG_EXT) { N = sample_ext_count(j); tabv = X.q5[j]; }
    else if (kind == SG_PAIR) { N = sample_pair_count(d); tabv = X.QB[d * ld + i]; }
    else if (kind == SG_QM) { N = sample_qm_count(d); tabv = X.QM[d * ld + i]; }
    else { N = sample_qm1_count(d); tabv = X.QM1[d * ld + i]; }
    if (kind == SG_PAIR && lane == 0) { W.ev.pt[i] = (short)j; W.ev.pt[j] = (short)i; }
    SamplePick p{sample_u_key(key, (uint64_t)step) * tabv, 0.0, -1, -1};
    // (issuing the next chunk's loads before this chunk's scan was measured: 9.40 against 7.26 ms at 64 x 200 x 1,024 -- most steps
    // end in their first chunk, and the extra chunk's scattered loads cost more than the overlap gains)
    for (int c0 = 0; c0 < N; c0 += WAVE) {
      const int c = c0 + lane;
      double w = 0.0;
      if (c < N) {
        if (kind == SG_EXT) w = sample_ext_weight(X, j, c);
        else if (kind == SG_PAIR) w = sample_pair_weight(sm, A, X, i, j, c);
        else if (kind == SG_QM) w = sample_qm_weight(A, X, i, j, c);
        else w = sample_qm1_weight(sm, A, X, i, j, c);
      }
      if (sample_chunk(p, w, c0, lane)) break;
    }
    const int c = p.chosen >= 0 ? p.chosen : p.last;
    if (c < 0 || sp + 2 > SAMPLE_STACK) break;              // (no candidate of non-zero weight: tables the fill did not leave)
    if (kind == SG_EXT) {
      const int rest = c == 0 ? j - 1 : c - 1;
      if (rest > TURN + 1) W.seg[sp++] = sample_seg(SG_EXT, 1, rest);
      if (c) W.seg[sp++] = sample_seg(SG_PAIR, c, j);
    } else if (kind == SG_PAIR) {
      if (c == 0) continue;
      if (c <= NPLAN) {
        const int pu = sm.plan_u[c - 1];
        W.seg[sp++] = sample_seg(SG_PAIR, i + 1 + (pu & 255), j - 1 - ((pu >> 8) & 255));
      } else {
        const int tt = TURN + 1 + (c - NPLAN - 1);
        W.seg[sp++] = sample_seg(SG_QM, i + 1, i + 1 + tt);
        W.seg[sp++] = sample_seg(SG_QM1, i + tt + 2, j - 1);
      }
    } else if (kind == SG_QM) {
      if (c <= sample_qm_nU(d)) W.seg[sp++] = sample_seg(SG_QM1, i + c, j);
      else {
        const int k = i + sample_qm_split(d, c);
        W.seg[sp++] = sample_seg(SG_QM, i, k - 1);
        W.seg[sp++] = sample_seg(SG_QM1, k, j);
      }
    } else {
      W.seg[sp++] = sample_seg(SG_PAIR, i, j - c);
    }
  }
  wave_lds_sync();
}

template <int NT>
__global__ __launch_bounds__(NT) void sample_kernel(SampleArgs A) {
  constexpr int NW = NT / WAVE;
  __shared__ SampleSmem<NW> sm;
  const PfArgs& P = A.pf;
  const int G = A.G;
  const int r = blockIdx.x / G, g = blockIdx.x - r * G;
  const int n = P.L, ld = P.ld;
  const int tid = threadIdx.x, lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());

  stage_energy_tables<NT>(sm, *P.T, tid);
  for (int e = tid; e < NPLAN; e += NT) {
    sm.plan_u[e] = P.plan->u1[e] | (P.plan->u2[e] << 8) | (P.plan->kind[e] << 16);
    sm.plan_W[e] = P.plan->W[e];
  }
  load_sequence<NT>(sm, P.seqs + (long long)r * n, n, tid);
  if (P.status[r] != ST_OK) return;       // bad character / PF out of range: the host reports it

  const double* base = P.ws + (long long)r * P.ws_stride;
  const long long tab = (long long)ld * ld;
  SampleTabs X;
  X.QB = base; X.QBI = base + tab; X.QM = base + 2 * tab; X.QM1 = base + 3 * tab; X.QEXT = base + 6 * tab;
  X.INFO = reinterpret_cast<const unsigned char*>(base + 7 * tab);
  X.q5 = P.q5out + (long long)r * P.q5_stride;
  X.n = n; X.ld = ld; X.segG = P.plan->seg[PK_GENERIC];
  X.sc1 = P.scale[1]; X.sc2 = P.scale[2];

  SampleWaveSmem& W = sm.w[wave];
  for (int x = lane; x < n + 2; x += WAVE) W.ev.S[x] = sm.S[x];
  const uint64_t seed = A.seeds[r];
  for (int s = g * NW + wave; s < A.S; s += G * NW) {
    sample_walk(sm, W, P, X, sample_key(seed, (uint64_t)s), lane);
    char* out = A.ss + ((long long)r * A.S + s) * n;
    for (int x = lane; x < n; x += WAVE) {
      const int q = W.ev.pt[x + 1];
      out[x] = q == 0 ? '.' : q > x + 1 ? '(' : ')';
    }
    if (A.E) {
      const int e = eval_loaded(W.ev, A.ev, n, lane);
      if (lane == 0) A.E[(long long)r * A.S + s] = e;
    }
    wave_lds_sync();                      // the next sample clears the pair table
  }
}

}  // namespace drna
