// emu_access.cpp -- TEST-ONLY: the two kernels of the partition function with positions held unpaired (pf_kernel<NT, true> of
// desirna_amd/csrc/fold_pf.hpp and access_lds_kernel of fold_access.hpp, unmodified) compiled against hip_emu.h for
// tests/test_access_emulated.py (CPU, no GPU needed).  A library of its own; the lanes of a workgroup run as fibers of one OS
// thread (emu_fibers.h).
#include "emu_fibers.h"

#include "../../desirna_amd/csrc/fold_access.hpp"

using namespace drna;

extern "C" {

int emu_access_lds_max() { return ACCESS_LDS_MAX; }

// R sequences of L nucleotides under each of M masks (M x L bytes): F and status hold R x M entries, fold g = r M + m.  The folds
// run one workgroup of |nt| threads at a time, in launches of `chunk` workgroups that begin at slot 0 again, as the engine's
// chunks do (fold0 = the launch's first fold, seq0 = its first sequence).  lds = 0: pf_kernel<NT, true>, nt = 64, 128 or 256, each
// slot with a workspace of its own; lds = 1: access_lds_kernel, nt = 64 or 128.  masked = 0 (lds = 0, M = 1 only): the unmasked
// pf_kernel<NT> on the same sequences, the instance the all-zero mask is held against.
int emu_access(const int32_t* blob, int n_int32, int R, int L, const char* seqs, int M, const unsigned char* nopair, int nt, int lds,
               int masked, int chunk, double* F, int32_t* status) {
  if (lds ? (nt != 64 && nt != 128) : (nt != 64 && nt != 128 && nt != 256)) return -2;
  if (!masked && (lds || M != 1)) return -2;
  if (chunk < 1) return -2;
  HostTables H;
  if (!build_tables(blob, n_int32, H).empty()) return -1;
  size_tables(H, L + 2);
  const int ld = L + 2, total = R * M;
  const size_t stride = (size_t)7 * ld * ld + ((size_t)ld * ld + 7) / 8;
  std::vector<double> ws(lds ? 1 : stride * (size_t)std::min(chunk, total), 0.0);
  std::vector<double> F4((size_t)4 * chunk, 0.0), Epf(chunk, 0.0);
  std::vector<int32_t> st(chunk, ST_OK);
  for (int g0 = 0; g0 < total; g0 += chunk) {
    const int m = std::min(chunk, total - g0), s0 = g0 / M;
    for (int b = 0; b < m; b++) st[b] = ST_OK;
    if (lds) {
      AccessLdsArgs a;
      a.in.F = &H.pf; a.in.plan = &H.plan; a.in.hp_w = H.hp_w.data(); a.in.scale = H.scale.data(); a.in.eMLb = H.eMLb.data();
      a.in.seqs = seqs + (size_t)s0 * L; a.in.L = L; a.in.cut = L; a.in.ld = 0;
      a.in.eDuplexInit = std::exp(-(double)H.DuplexInit * 10.0 / H.pf.kT);
      a.in.F4 = F4.data(); a.in.status_pf = st.data();
      a.nopair = nopair; a.M = M; a.fold0 = g0; a.seq0 = s0;
      for (int b = 0; b < m; b++) {
        if (nt == 64) fiber_launch(b, 64, [&]() { access_lds_kernel<64>(a); });
        else fiber_launch(b, 128, [&]() { access_lds_kernel<128>(a); });
        F[g0 + b] = F4[(size_t)4 * b]; status[g0 + b] = st[b];
      }
    } else {
      PfMaskArgs a;
      a.T = &H.pf; a.plan = &H.plan; a.hp_w = H.hp_w.data(); a.scale = H.scale.data(); a.eMLb = H.eMLb.data();
      a.seqs = seqs + (size_t)s0 * L; a.L = L; a.ld = ld;
      a.ws = ws.data(); a.ws_stride = (long long)stride;
      a.Epf = Epf.data(); a.status = st.data();
      a.nopair = nopair; a.M = M; a.fold0 = g0; a.seq0 = s0;
      const PfArgs& u = a;
      for (int b = 0; b < m; b++) {
        if (!masked) {
          if (nt == 64) fiber_launch(b, 64, [&]() { pf_kernel<64>(u); });
          else if (nt == 128) fiber_launch(b, 128, [&]() { pf_kernel<128>(u); });
          else fiber_launch(b, 256, [&]() { pf_kernel<256>(u); });
        } else if (nt == 64) fiber_launch(b, 64, [&]() { pf_kernel<64, true>(a); });
        else if (nt == 128) fiber_launch(b, 128, [&]() { pf_kernel<128, true>(a); });
        else fiber_launch(b, 256, [&]() { pf_kernel<256, true>(a); });
        F[g0 + b] = Epf[b]; status[g0 + b] = st[b];
      }
    }
  }
  return 0;
}
}
