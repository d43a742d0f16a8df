// emu_cofold_subopt.cpp -- TEST-ONLY: compiles the unmodified fold_cofold_subopt.hpp against hip_emu.h and exposes the
// second-best co-fold kernel through a tiny C interface for tests/test_cofold_subopt_emulated.py (CPU, no GPU needed).
#include "hip_emu.h"

thread_local emu_dim3 threadIdx;
thread_local emu_dim3 blockIdx;
thread_local emu_group* emu_g = nullptr;

#include "../../desirna_amd/csrc/fold_cofold_subopt.hpp"

using namespace drna;

extern "C" {

// two-best co-fold energies (second-best structure) of R pairs of total length L, the first strand `cut` nucleotides long
int emu_cofold_subopt(const int32_t* blob, int n_int32, int R, int L, int cut, const char* seqs, int nt, int32_t* E2, int32_t* E12,
                      int32_t* status) {
  HostTables H;
  if (!build_tables(blob, n_int32, H).empty()) return -1;
  size_tables(H, L + 2);
  const int ld = L + 2;
  std::vector<int32_t> ws((size_t)6 * ld * ld, 0);
  for (int r = 0; r < R; r++) {
    CoSubArgs a;
    a.T = &H.mfe; a.plan = &H.plan; a.hp_len = H.hp_len.data(); a.seqs = seqs; a.L = L; a.cut = cut; a.ld = ld;
    a.DuplexInit = H.DuplexInit;
    a.ws = ws.data() - (size_t)r * 6 * ld * ld; a.ws_stride = (long long)6 * ld * ld;
    a.E2 = E2; a.E12 = E12; a.status = status;
    if (nt == 64) emu_launch(r, 64, [&]() { cofold_subopt_kernel<64>(a); });
    else if (nt == 128) emu_launch(r, 128, [&]() { cofold_subopt_kernel<128>(a); });
    else return -2;
  }
  return 0;
}
}
