// emu_cofold_sampling.cpp -- TEST-ONLY: cofold_pf_kernel + cofold_columns_kernel + cofold_sample_kernel
// (desirna_amd/csrc/fold_cofold_sample.hpp, unmodified) compiled against hip_emu.h for tests/test_cofold_sampling_emulated.py
// (CPU, no GPU needed).  A library of its own; the lanes of a workgroup run as fibers of one OS thread (emu_fibers.h).
#include "emu_fibers.h"

#include "../../desirna_amd/csrc/fold_cofold_sample.hpp"

using namespace drna;

extern "C" {

// Workgroups b0 .. b1 - 1 of the launch of R x G workgroups of nt threads (workgroup b: pair b / G), one after the other.
// cofold_pf_kernel fills the ONE workspace slot and cofold_columns_kernel the one set of columns for a pair before its first
// workgroup runs; slot and columns start filled with the byte `fill` (0xFF: NaN): whatever the walk reads, a kernel must have written.
// ss (R x S x L) and E (R x S, may be null) keep what they held wherever these workgroups do not write; F4 (R x 4) / status get
// the fill's results of the pairs touched.
int emu_cofold_sample(const int32_t* blob, int n_int32, int nt, int R, int L, int cut, const char* seqs, const uint64_t* seeds,
                      int S, int G, int b0, int b1, int fill, char* ss, int32_t* E, double* F4, int32_t* status) {
  if (nt != 64 && nt != 128) return -2;
  if (G < 1 || b0 < 0 || b1 > R * G || cut < 1 || cut >= L) return -3;
  HostTables H;
  if (!build_tables(blob, n_int32, H).empty()) return -1;
  size_tables(H, L + 2);
  const int ld = L + 2;
  const size_t stride = (size_t)7 * ld * ld + ((size_t)ld * ld + 7) / 8, cstride = (size_t)ld;
  std::vector<double> ws(stride), cols(CO_COLS * cstride);
  int filled = -1;
  for (int b = b0; b < b1; b++) {
    const int r = b / G;
    CoSampleArgs a{};
    CoArgs& c = a.co;
    c.T = &H.mfe; c.F = &H.pf; c.plan = &H.plan; c.hp_len = H.hp_len.data(); c.hp_w = H.hp_w.data();
    c.scale = H.scale.data(); c.eMLb = H.eMLb.data(); c.seqs = seqs; c.L = L; c.cut = cut; c.ld = ld;
    c.DuplexInit = H.DuplexInit; c.eDuplexInit = std::exp(-(double)H.DuplexInit * 10.0 / H.pf.kT);
    c.wsp = ws.data() - (size_t)r * stride; c.wsp_stride = (long long)stride;
    c.F4 = F4; c.status_pf = status;
    a.ev.T = &H.mfe; a.ev.hp_len = H.hp_len.data(); a.ev.bulge_len = H.bulge_len.data(); a.ev.int_len = H.int_len.data();
    a.ev.cut = cut; a.ev.DuplexInit = H.DuplexInit;
    a.cols = cols.data() - (size_t)r * CO_COLS * cstride; a.col_stride = (long long)cstride;
    a.seeds = seeds; a.S = S; a.G = G; a.ss = ss; a.E = E;
    if (filled != r) {
      std::memset(ws.data(), fill, ws.size() * sizeof(double));
      std::memset(cols.data(), fill, cols.size() * sizeof(double));
      const CoArgs p = a.co;
      if (nt == 64) {
        fiber_launch(r, 64, [&]() { cofold_pf_kernel<64>(p); });
        fiber_launch(r, 64, [&]() { cofold_columns_kernel<64>(a); });
      } else {
        fiber_launch(r, 128, [&]() { cofold_pf_kernel<128>(p); });
        fiber_launch(r, 128, [&]() { cofold_columns_kernel<128>(a); });
      }
      filled = r;
    }
    if (nt == 64) fiber_launch(b, 64, [&]() { cofold_sample_kernel<64>(a); });
    else fiber_launch(b, 128, [&]() { cofold_sample_kernel<128>(a); });
  }
  return 0;
}
}
