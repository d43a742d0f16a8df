// emu_mea.cpp -- TEST-ONLY: mea_kernel (desirna_amd/csrc/fold_mea.hpp, unmodified) compiled against hip_emu.h for
// tests/test_mea_emulated.py (CPU, no GPU needed).  A library of its own; the lanes of a workgroup run as fibers of one OS thread
// (emu_fibers.h).
#include "emu_fibers.h"

#include "../../desirna_amd/csrc/fold_mea.hpp"

using namespace drna;

extern "C" {

int emu_mea_lds_max() { return MEA_LDS_MAX; }
int emu_mea_cand_lds() { return MEA_CAND_LDS; }

// R workgroups of nt threads, one after the other, on R matrices of (L+1) x (L+1); lds: M in LDS (needs L <= MEA_LDS_MAX).  The ONE
// workspace slot starts filled with the byte `fill` for every sequence (0xFF: NaN): whatever the kernel reads, it must have written.
// seqs / blob are needed for the energies only (E null: neither is read).
int emu_mea(const int32_t* blob, int n_int32, int nt, int lds, int R, int L, int cut, const char* seqs, const double* bpp, double gamma,
            int fill, char* mea_ss, double* mea_val, char* cen_ss, double* cen_dist, int32_t* E, int32_t* ncand) {
  if (nt != 64 && nt != 128) return -2;
  if (L < 1 || L > MAXN - 2 || cut < 0 || cut >= L || (lds && L > MEA_LDS_MAX) || (E && (!blob || !seqs))) return -3;
  HostTables H;
  if (E) {
    if (!build_tables(blob, n_int32, H).empty()) return -1;
    size_tables(H, L + 2);
  }
  const int ld = L + 2;
  const size_t stride = (size_t)4 * ld * ld + ld + 6;
  std::vector<double> ws(stride);
  for (int r = 0; r < R; r++) {
    MeaArgs a;
    if (E) {
      a.ev.T = &H.mfe; a.ev.hp_len = H.hp_len.data(); a.ev.bulge_len = H.bulge_len.data(); a.ev.int_len = H.int_len.data();
      a.ev.cut = cut; a.ev.DuplexInit = H.DuplexInit;
    }
    a.ev.seqs = seqs; a.ev.L = L;
    a.bpp = bpp; a.ws = ws.data() - (size_t)r * stride; a.ws_stride = (long long)stride; a.gamma = gamma;
    a.mea_ss = mea_ss; a.mea_val = mea_val; a.cen_ss = cen_ss; a.cen_dist = cen_dist; a.E = E; a.ncand = ncand;
    std::memset(ws.data(), fill, ws.size() * sizeof(double));
    if (nt == 64) {
      if (lds) fiber_launch(r, 64, [&]() { mea_kernel<64, true>(a); });
      else fiber_launch(r, 64, [&]() { mea_kernel<64, false>(a); });
    } else {
      if (lds) fiber_launch(r, 128, [&]() { mea_kernel<128, true>(a); });
      else fiber_launch(r, 128, [&]() { mea_kernel<128, false>(a); });
    }
  }
  return 0;
}
}
