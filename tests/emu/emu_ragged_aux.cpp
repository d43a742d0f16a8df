// emu_ragged_aux.cpp -- TEST-ONLY: the four kernels of the auxiliary folds that take a ragged batch (edef_lds_kernel<NT, true>,
// pf_kernel + outside_kernel, subopt_lds_kernel, subopt_kernel; desirna_amd/csrc, unmodified) compiled against hip_emu.h for
// tests/test_ragged_aux_emulated.py (CPU, no GPU needed), in their uniform and their ragged form (the compile-time flag RAGGED of each).  A library of its own beside libemu.so.
#include "hip_emu.h"

thread_local emu_dim3 threadIdx;
thread_local emu_dim3 blockIdx;
thread_local emu_group* emu_g = nullptr;

#include "../../desirna_amd/csrc/fold_edef_lds.hpp"
#include "../../desirna_amd/csrc/fold_outside.hpp"
#include "../../desirna_amd/csrc/fold_subopt_lds.hpp"

using namespace drna;

extern "C" {

// kind 0: edef_lds_kernel<nt, true>; 1: pf_kernel + outside_kernel; 2: subopt_lds_kernel; 3: subopt_kernel.  Workgroups
// 0 .. nblocks - 1 of one launch, one after the other through ONE workspace slot (the base moved back by the sequence's position, as
// the engine moves a chunk's base), which starts filled with 0xFF bytes (NaN / -1): whatever a fold reads, it must have written.
//   ragged = 0  R sequences of L letters each (seqs R x L), one pair table pt (L + 2 shorts): the descriptors stay null
//   ragged = 1  sequence r has lens[r] letters at offs[r]; workgroup b folds sequence idx[b]; L = the longest length the "engine"
//               holds: the partition function's tables get the pitch L + 2 and every slot the size for L; pt holds all pair tables,
//               that of sequence r at pt_off[target_of[r]]
// edef R doubles, E2 R, E12 R x 2, status R words, all at the sequence's position.
int emu_ragged_aux(const int32_t* blob, int n_int32, int kind, int nt, int ragged, int R, int L, const int* lens, const int* offs,
                   const int* idx, const char* seqs, const short* pt, const int* pt_off, const int* target_of, int nblocks,
                   double* edef, int32_t* E2, int32_t* E12, int32_t* status) {
  if (nt != 64 && nt != 128) return -2;
  HostTables H;
  if (!build_tables(blob, n_int32, H).empty()) return -1;
  size_tables(H, L + 2);
  Ragged rg;
  if (ragged) { rg.idx = idx; rg.len = lens; rg.off = offs; }
  const int ld = L + 2;
  std::vector<double> F4((size_t)4 * R, 0.0), Epf(R, 0.0);
  // the one slot of every workspace, poisoned once: a later workgroup finds what its predecessors left
  const size_t stride = (size_t)7 * ld * ld + ((size_t)ld * ld + 7) / 8, ostride = (size_t)outside_ws_stride(ld);
  const size_t sstride = (size_t)3 * 2 * ld * ld;
  std::vector<double> ws(kind == 1 ? stride : 0), wo(kind == 1 ? ostride : 0);
  std::vector<int32_t> wsi(kind == 3 ? sstride : 0);
  if (!ws.empty()) std::memset(ws.data(), 0xFF, ws.size() * sizeof(double));
  if (!wo.empty()) std::memset(wo.data(), 0xFF, wo.size() * sizeof(double));
  if (!wsi.empty()) std::memset(wsi.data(), 0xFF, wsi.size() * sizeof(int32_t));
  for (int b = 0; b < nblocks; b++) {
    const int r = ragged ? idx[b] : b;
    if (kind == 0) {
      EdefLdsArgs a;
      a.in.F = &H.pf; a.in.plan = &H.plan; a.in.hp_w = H.hp_w.data(); a.in.scale = H.scale.data(); a.in.eMLb = H.eMLb.data();
      a.in.seqs = seqs; a.in.L = ragged ? 0 : L; a.in.cut = a.in.L; a.in.ld = 0;
      a.in.F4 = F4.data(); a.in.status_pf = status;
      a.out.F = &H.pf; a.out.plan = &H.plan; a.out.scale = H.scale.data(); a.out.eMLb = H.eMLb.data();
      a.out.seqs = seqs; a.out.L = a.in.L; a.out.cut = a.in.cut; a.out.ld = 0;
      a.out.pt = pt; a.out.edef = edef; a.out.status_pf = status;
      if (ragged) { a.rg = rg; a.target_of = target_of; a.pt_off = pt_off; }
      status[r] = ST_OK;
      if (ragged) {
        if (nt == 64) emu_launch(b, 64, [&]() { edef_lds_kernel<64, true, true>(a); });
        else emu_launch(b, 128, [&]() { edef_lds_kernel<128, true, true>(a); });
      } else {
        if (nt == 64) emu_launch(b, 64, [&]() { edef_lds_kernel<64, true>(a); });
        else emu_launch(b, 128, [&]() { edef_lds_kernel<128, true>(a); });
      }
    } else if (kind == 1) {
      PfArgs a;
      a.T = &H.pf; a.plan = &H.plan; a.hp_w = H.hp_w.data(); a.scale = H.scale.data(); a.eMLb = H.eMLb.data();
      a.seqs = seqs; a.L = ragged ? 0 : L; a.ld = ld;
      a.ws = ws.data() - (size_t)r * stride; a.ws_stride = (long long)stride;
      a.Epf = Epf.data(); a.status = status;
      a.q5out = wo.data() + (size_t)4 * ld * ld - (size_t)r * ostride; a.q5_stride = (long long)ostride;
      OutArgs o;
      o.T = &H.pf; o.plan = &H.plan; o.scale = H.scale.data(); o.eMLb = H.eMLb.data();
      o.seqs = seqs; o.L = a.L; o.ld = ld; o.ws = a.ws; o.ws_stride = a.ws_stride;
      o.wo = wo.data() - (size_t)r * ostride; o.wo_stride = (long long)ostride;
      o.pt = pt; o.edef = edef; o.pf_status = status;
      if (ragged) { a.rg = rg; o.rg = rg; o.target_of = target_of; o.pt_off = pt_off; }
      if (nt == 64) emu_launch(b, 64, [&]() { pf_kernel<64>(a); });
      else emu_launch(b, 128, [&]() { pf_kernel<128>(a); });
      if (ragged) {
        if (nt == 64) emu_launch(b, 64, [&]() { outside_kernel<64, true>(o); });
        else emu_launch(b, 128, [&]() { outside_kernel<128, true>(o); });
      } else {
        if (nt == 64) emu_launch(b, 64, [&]() { outside_kernel<64>(o); });
        else emu_launch(b, 128, [&]() { outside_kernel<128>(o); });
      }
    } else {
      SuboptArgs a;
      a.T = &H.mfe; a.plan = &H.plan; a.hp_len = H.hp_len.data(); a.seqs = seqs; a.L = ragged ? 0 : L; a.cut = 0; a.ld = ld;
      a.DuplexInit = H.DuplexInit; a.E2 = E2; a.E12 = E12; a.status = status;
      if (ragged) a.rg = rg;
      if (kind == 3) { a.ws_stride = (long long)sstride; a.ws = wsi.data() - (size_t)r * sstride; }
      if (kind == 2 && ragged) {
        if (nt == 64) emu_launch(b, 64, [&]() { subopt_lds_kernel<64, true>(a); });
        else emu_launch(b, 128, [&]() { subopt_lds_kernel<128, true>(a); });
      } else if (kind == 2) {
        if (nt == 64) emu_launch(b, 64, [&]() { subopt_lds_kernel<64>(a); });
        else emu_launch(b, 128, [&]() { subopt_lds_kernel<128>(a); });
      } else if (ragged) {
        if (nt == 64) emu_launch(b, 64, [&]() { subopt_kernel<64, true>(a); });
        else emu_launch(b, 128, [&]() { subopt_kernel<128, true>(a); });
      } else {
        if (nt == 64) emu_launch(b, 64, [&]() { subopt_kernel<64>(a); });
        else emu_launch(b, 128, [&]() { subopt_kernel<128>(a); });
      }
    }
  }
  return 0;
}
}
