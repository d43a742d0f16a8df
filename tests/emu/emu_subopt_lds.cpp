// emu_subopt_lds.cpp -- TEST-ONLY: the LDS-resident second-best kernels (desirna_amd/csrc/fold_subopt_lds.hpp, unmodified) and the
// general ones they must equal, compiled against hip_emu.h for tests/test_subopt_lds_emulated.py (CPU, no GPU needed).  A library of
// its own beside libemu.so.
#include "hip_emu.h"

thread_local emu_dim3 threadIdx;
thread_local emu_dim3 blockIdx;
thread_local emu_group* emu_g = nullptr;

#include "../../desirna_amd/csrc/fold_subopt_lds.hpp"

using namespace drna;

extern "C" {

int emu_subopt_lds_max(void) { return SUB_LDS_MAX; }
int emu_subopt_lds_bytes(void) { return (int)sizeof(SubLdsSmem); }

// R sequences of L nucleotides (cut > 0: pairs, the first strand cut long) through the second-best kernel, one workgroup of nt
// threads at a time.  lds = 1: subopt_lds_kernel / cofold_subopt_lds_kernel (no workspace: the tables are in "LDS");
// lds = 0: subopt_kernel / cofold_subopt_kernel with one workspace slot per sequence
int emu_subopt_lds(const int32_t* blob, int n_int32, int R, int L, int cut, const char* seqs, int nt, int lds, int32_t* E2,
                   int32_t* E12, int32_t* status) {
  if (nt != 64 && nt != 128) return -2;
  HostTables H;
  if (!build_tables(blob, n_int32, H).empty()) return -1;
  size_tables(H, L + 2);
  SuboptArgs a;
  a.T = &H.mfe; a.plan = &H.plan; a.hp_len = H.hp_len.data(); a.seqs = seqs; a.L = L; a.cut = cut; a.ld = L + 2;
  a.DuplexInit = H.DuplexInit; a.E2 = E2; a.E12 = E12; a.status = status;
  std::vector<int32_t> ws;
  if (!lds) {
    a.ws_stride = (long long)3 * 2 * (L + 2) * (L + 2);
    ws.assign((size_t)a.ws_stride * R, 0);
    a.ws = ws.data();
  }
  for (int r = 0; r < R; r++) {
    if (lds && cut) {
      if (nt == 64) emu_launch(r, 64, [&]() { cofold_subopt_lds_kernel<64>(a); });
      else emu_launch(r, 128, [&]() { cofold_subopt_lds_kernel<128>(a); });
    } else if (lds) {
      if (nt == 64) emu_launch(r, 64, [&]() { subopt_lds_kernel<64>(a); });
      else emu_launch(r, 128, [&]() { subopt_lds_kernel<128>(a); });
    } else if (cut) {
      if (nt == 64) emu_launch(r, 64, [&]() { cofold_subopt_kernel<64>(a); });
      else emu_launch(r, 128, [&]() { cofold_subopt_kernel<128>(a); });
    } else {
      if (nt == 64) emu_launch(r, 64, [&]() { subopt_kernel<64>(a); });
      else emu_launch(r, 128, [&]() { subopt_kernel<128>(a); });
    }
  }
  return 0;
}
}
