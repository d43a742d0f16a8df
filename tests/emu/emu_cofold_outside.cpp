// emu_cofold_outside.cpp -- TEST-ONLY: compiles the unmodified fold_cofold_outside.hpp (and the cofold_pf_kernel it runs after)
// against hip_emu.h and exposes the two-strand ensemble defect through a tiny C interface for
// tests/test_cofold_edef_emulated.py (CPU, no GPU needed).
#include "hip_emu.h"

thread_local emu_dim3 threadIdx;
thread_local emu_dim3 blockIdx;
thread_local emu_group* emu_g = nullptr;

#include "../../desirna_amd/csrc/fold_cofold_outside.hpp"

using namespace drna;

extern "C" {

// pair probabilities and ensemble defect of R pairs of total length L, the first strand `cut` nucleotides long, against the
// pair table pt (L + 2 shorts); bpp (R x (L+1) x (L+1), zeroed by the caller) may be null; F4 = R x 4 free energies
int emu_cofold_edef(const int32_t* blob, int n_int32, int R, int L, int cut, const char* seqs, const short* pt, int nt, double* edef,
                    double* bpp, double* F4, int32_t* status) {
  HostTables H;
  if (!build_tables(blob, n_int32, H).empty()) return -1;
  size_tables(H, L + 2);
  const int ld = L + 2;
  const long long stride = cofold_outside_ws_stride(ld), ustride = (long long)4 * ld * ld;
  std::vector<double> ws((size_t)stride, 0.0), wu((size_t)ustride, 0.0);
  for (int r = 0; r < R; r++) {
    CoArgs a;
    a.F = &H.pf; a.plan = &H.plan; a.hp_w = H.hp_w.data(); a.scale = H.scale.data(); a.eMLb = H.eMLb.data();
    a.seqs = seqs; a.L = L; a.cut = cut; a.ld = ld;
    a.eDuplexInit = std::exp(-(double)H.DuplexInit * 10.0 / H.pf.kT);
    a.wsp = ws.data() - (size_t)r * stride; a.wsp_stride = stride;
    a.F4 = F4; a.status_pf = status;
    CoOutArgs o;
    o.F = &H.pf; o.plan = &H.plan; o.scale = H.scale.data(); o.eMLb = H.eMLb.data();
    o.seqs = seqs; o.L = L; o.cut = cut; o.ld = ld; o.eDuplexInit = a.eDuplexInit;
    o.wsp = a.wsp; o.wsp_stride = stride;
    o.wu = wu.data() - (size_t)r * ustride; o.wu_stride = ustride;
    o.pt = pt; o.edef = edef; o.bpp = bpp; o.status_pf = status;
    status[r] = ST_OK;
    if (nt == 64) {
      emu_launch(r, 64, [&]() { cofold_pf_kernel<64>(a); });
      emu_launch(r, 64, [&]() { cofold_outside_kernel<64>(o); });
    } else if (nt == 128) {
      emu_launch(r, 128, [&]() { cofold_pf_kernel<128>(a); });
      emu_launch(r, 128, [&]() { cofold_outside_kernel<128>(o); });
    } else return -2;
  }
  return 0;
}
}
