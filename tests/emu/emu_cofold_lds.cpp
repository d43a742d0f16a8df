// emu_cofold_lds.cpp -- TEST-ONLY: the short-pair co-fold kernels (desirna_amd/csrc/fold_cofold_lds.hpp, unmodified) compiled
// against hip_emu.h for tests/test_cofold_lds_emulated.py (CPU, no GPU needed).  A library of its own beside libemu.so.
#include "hip_emu.h"

thread_local emu_dim3 threadIdx;
thread_local emu_dim3 blockIdx;
thread_local emu_group* emu_g = nullptr;

#include "../../desirna_amd/csrc/fold_cofold_lds.hpp"

using namespace drna;

extern "C" {

int emu_cofold_lds_max(void) { return CO_LDS_MAX; }

// R pairs (L nucleotides each, the first strand cut long) through cofold_mfe_lds_kernel and cofold_pf_lds_kernel, one workgroup of
// nt threads at a time; status: R words of the MFE kernel, then R of the partition function
int emu_cofold_lds(const int32_t* blob, int n_int32, int R, int L, int cut, const char* seqs, int nt, int32_t* Emfe, char* ss,
                   double* F4, int32_t* status) {
  HostTables H;
  if (!build_tables(blob, n_int32, H).empty()) return -1;
  size_tables(H, L + 2);
  CoArgs a;
  a.T = &H.mfe; a.F = &H.pf; a.plan = &H.plan; a.hp_len = H.hp_len.data(); a.hp_w = H.hp_w.data();
  a.scale = H.scale.data(); a.eMLb = H.eMLb.data(); a.seqs = seqs; a.L = L; a.cut = cut; a.ld = L + 2;
  a.DuplexInit = H.DuplexInit; a.eDuplexInit = std::exp(-(double)H.DuplexInit * 10.0 / H.pf.kT);
  a.Emfe = Emfe; a.ss = ss; a.F4 = F4; a.status = status; a.status_pf = status + R;      // no workspace: the tables are in "LDS"
  for (int r = 0; r < R; r++) {
    if (nt == 64) { emu_launch(r, 64, [&]() { cofold_mfe_lds_kernel<64>(a); }); emu_launch(r, 64, [&]() { cofold_pf_lds_kernel<64>(a); }); }
    else { emu_launch(r, 128, [&]() { cofold_mfe_lds_kernel<128>(a); }); emu_launch(r, 128, [&]() { cofold_pf_lds_kernel<128>(a); }); }
  }
  return 0;
}
}
