// emu_self_dimer.cpp -- TEST-ONLY: the self-dimer partition function kernels (desirna_amd/csrc/fold_self_dimer.hpp, unmodified)
// compiled against hip_emu.h for tests/test_self_dimer_emulated.py (CPU, no GPU needed).  A library of its own beside libemu.so.
#include "hip_emu.h"

thread_local emu_dim3 threadIdx;
thread_local emu_dim3 blockIdx;
thread_local emu_group* emu_g = nullptr;

#include "../../desirna_amd/csrc/fold_self_dimer.hpp"

using namespace drna;

extern "C" {

int emu_self_dimer_lds_max(void) { return SD_LDS_MAX; }

// R sequences of L nucleotides through self_dimer_pf_lds_kernel (lds != 0) or self_dimer_pf_kernel (one workspace slot, used by
// one sequence after the other), one workgroup of nt threads at a time; status: R words
int emu_self_dimer(const int32_t* blob, int n_int32, int R, int L, const char* seqs, int nt, int lds, double* F4, int32_t* status) {
  HostTables H;
  if (!build_tables(blob, n_int32, H).empty()) return -1;
  size_tables(H, L + 2);                                   // sized for L, not 2 L, like the engine
  std::vector<double> ws(lds ? 1 : (size_t)sd_ws_stride(L));
  CoArgs a;
  a.T = &H.mfe; a.F = &H.pf; a.plan = &H.plan; a.hp_len = H.hp_len.data(); a.hp_w = H.hp_w.data();
  a.scale = H.scale.data(); a.eMLb = H.eMLb.data(); a.seqs = seqs; a.L = L; a.cut = L; a.ld = L + 2;
  a.DuplexInit = H.DuplexInit; a.eDuplexInit = std::exp(-(double)H.DuplexInit * 10.0 / H.pf.kT);
  a.wsp = ws.data(); a.wsp_stride = 0;
  a.F4 = F4; a.status_pf = status;
  for (int r = 0; r < R; r++) {
    if (lds) {
      if (nt == 64) emu_launch(r, 64, [&]() { self_dimer_pf_lds_kernel<64>(a); });
      else emu_launch(r, 128, [&]() { self_dimer_pf_lds_kernel<128>(a); });
    } else {
      if (nt == 64) emu_launch(r, 64, [&]() { self_dimer_pf_kernel<64>(a); });
      else emu_launch(r, 128, [&]() { self_dimer_pf_kernel<128>(a); });
    }
  }
  return 0;
}
}
