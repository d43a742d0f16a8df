// emu_cofold_kbest.cpp -- TEST-ONLY: the K-best co-fold kernel (desirna_amd/csrc/fold_cofold_subopt.hpp, unmodified) and the
// one-strand K-best kernel that shares its enumerator and traceback (fold_subopt.hpp), compiled against hip_emu.h for
// tests/test_cofold_kbest_emulated.py (CPU, no GPU needed).  A library of its own beside libemu.so.
#include "hip_emu.h"

thread_local emu_dim3 threadIdx;
thread_local emu_dim3 blockIdx;
thread_local emu_group* emu_g = nullptr;

#include "../../desirna_amd/csrc/fold_cofold_subopt.hpp"

using namespace drna;

template <int K>
static void launch(int r, int nt, int cut, const SuboptArgs& a) {
  if (cut) {
    if (nt == 64) emu_launch(r, 64, [&]() { cofold_kbest_kernel<64, K>(a); });
    else emu_launch(r, 128, [&]() { cofold_kbest_kernel<128, K>(a); });
  } else {
    if (nt == 64) emu_launch(r, 64, [&]() { kbest_kernel<64, K>(a); });
    else emu_launch(r, 128, [&]() { kbest_kernel<128, K>(a); });
  }
}

extern "C" {

// R pairs of total length L (the first strand `cut` nucleotides long; cut = 0: single strands through kbest_kernel), one
// workgroup of nt threads at a time, one workspace slot per pair as on the device.  K = 4 or 8: E is R x K, ss R x K x L
int emu_cofold_kbest(const int32_t* blob, int n_int32, int R, int L, int cut, const char* seqs, int nt, int K, int32_t* E, char* ss,
                     int32_t* status) {
  if ((nt != 64 && nt != 128) || (K != 4 && K != 8)) return -2;
  HostTables H;
  if (!build_tables(blob, n_int32, H).empty()) return -1;
  size_tables(H, L + 2);
  const int ld = L + 2;
  SuboptArgs a;
  a.T = &H.mfe; a.plan = &H.plan; a.hp_len = H.hp_len.data(); a.seqs = seqs; a.L = L; a.cut = cut; a.ld = ld;
  a.DuplexInit = H.DuplexInit; a.E = E; a.ss = ss; a.status = status;
  a.ws_stride = (long long)3 * K * ld * ld + cofold_kbest_ws_extra(K, ld);
  std::vector<int32_t> ws((size_t)a.ws_stride * R, 0x55555555);      // (a word no table may take for a list value)
  a.ws = ws.data();
  for (int r = 0; r < R; r++) {
    if (K == 4) launch<4>(r, nt, cut, a);
    else launch<8>(r, nt, cut, a);
  }
  return 0;
}
}
