// emu_edef_lds.cpp -- TEST-ONLY: the fused inside + outside kernel of short designs (desirna_amd/csrc/fold_edef_lds.hpp, unmodified)
// compiled against hip_emu.h for tests/test_edef_lds_emulated.py (CPU, no GPU needed).  A library of its own beside libemu.so.
#include "hip_emu.h"

thread_local emu_dim3 threadIdx;
thread_local emu_dim3 blockIdx;
thread_local emu_group* emu_g = nullptr;

#include "../../desirna_amd/csrc/fold_edef_lds.hpp"

using namespace drna;

extern "C" {

int emu_edef_lds_max(int one) { return one ? EDEF_LDS_MAX : CO_EDEF_LDS_MAX; }

// R sequences (cut = 0) or pairs (first strand cut long, 1 <= cut < L) of L nucleotides in all through edef_lds_kernel, one workgroup
// of nt threads at a time.  pt: L + 2 shorts; bpp: R x (L + 1) x (L + 1) or NULL, written where the kernel writes and nowhere else;
// F4: R x 4; status: R words
int emu_edef_lds(const int32_t* blob, int n_int32, int R, int L, int cut, const char* seqs, const short* pt, int nt, double* edef,
                 double* bpp, double* F4, int32_t* status) {
  if (nt != 64 && nt != 128) return -2;
  HostTables H;
  if (!build_tables(blob, n_int32, H).empty()) return -1;
  size_tables(H, L + 2);
  EdefLdsArgs a;
  a.in.F = &H.pf; a.in.plan = &H.plan; a.in.hp_w = H.hp_w.data(); a.in.scale = H.scale.data(); a.in.eMLb = H.eMLb.data();
  a.in.seqs = seqs; a.in.L = L; a.in.cut = cut ? cut : L; a.in.ld = 0;
  a.in.eDuplexInit = std::exp(-(double)H.DuplexInit * 10.0 / H.pf.kT);
  a.in.F4 = F4; a.in.status_pf = status;
  a.out.F = &H.pf; a.out.plan = &H.plan; a.out.scale = H.scale.data(); a.out.eMLb = H.eMLb.data();
  a.out.seqs = seqs; a.out.L = L; a.out.cut = a.in.cut; a.out.ld = 0; a.out.eDuplexInit = a.in.eDuplexInit;
  a.out.pt = pt; a.out.edef = edef; a.out.bpp = bpp; a.out.status_pf = status;
  for (int r = 0; r < R; r++) {
    status[r] = ST_OK;
    if (cut) {
      if (nt == 64) emu_launch(r, 64, [&]() { edef_lds_kernel<64, false>(a); });
      else emu_launch(r, 128, [&]() { edef_lds_kernel<128, false>(a); });
    } else {
      if (nt == 64) emu_launch(r, 64, [&]() { edef_lds_kernel<64, true>(a); });
      else emu_launch(r, 128, [&]() { edef_lds_kernel<128, true>(a); });
    }
  }
  return 0;
}
}
