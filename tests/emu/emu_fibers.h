// emu_fibers.h -- TEST-ONLY: the lanes of one emulated workgroup as FIBERS of one OS thread, for emu_cofold_sampling.cpp.  A copy of
// the scheduler in emu_sampling.cpp (which stays as it is): hip_emu.h's collectives rendezvous through pthread_barrier_wait(),
// redirected here to a round-robin hand-over between the fibers (a barrier is complete once every lane has passed the baton).
// Include it INSTEAD of hip_emu.h, once, in the one translation unit of a library.
#pragma once
#include <pthread.h>
#include <sched.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

extern "C" int emu_fiber_wait(pthread_barrier_t* b);
#define pthread_barrier_wait(b) emu_fiber_wait(b)
#include "hip_emu.h"

thread_local emu_dim3 threadIdx;
thread_local emu_dim3 blockIdx;
thread_local emu_group* emu_g = nullptr;

// ---- fibers
#if defined(__x86_64__)
// saves the callee-saved registers on the running stack, parks its stack pointer in *save and continues on the stack `load`
extern "C" void emu_ctx_switch(void** save, void* load);
asm(".text\n.globl emu_ctx_switch\n.hidden emu_ctx_switch\n.type emu_ctx_switch,@function\nemu_ctx_switch:\n"
    "  pushq %rbp\n  pushq %rbx\n  pushq %r12\n  pushq %r13\n  pushq %r14\n  pushq %r15\n"
    "  movq %rsp, (%rdi)\n  movq %rsi, %rsp\n"
    "  popq %r15\n  popq %r14\n  popq %r13\n  popq %r12\n  popq %rbx\n  popq %rbp\n  ret\n"
    ".size emu_ctx_switch,.-emu_ctx_switch\n");
struct emu_ctx { void* sp = nullptr; };
static void ctx_make(emu_ctx& c, char* stack, size_t bytes, void (*entry)()) {
  void** top = (void**)(((uintptr_t)stack + bytes) & ~(uintptr_t)15);
  *--top = nullptr;                 // keeps the stack as the ABI wants it at the entry of a function
  *--top = (void*)entry;            // where the first switch to this fiber returns to
  for (int k = 0; k < 6; k++) *--top = nullptr;
  c.sp = top;
}
static void ctx_switch(emu_ctx& from, emu_ctx& to) { emu_ctx_switch(&from.sp, to.sp); }
#else
#include <ucontext.h>
struct emu_ctx { ucontext_t u; };
static void ctx_make(emu_ctx& c, char* stack, size_t bytes, void (*entry)()) {
  getcontext(&c.u);
  c.u.uc_stack.ss_sp = stack; c.u.uc_stack.ss_size = bytes; c.u.uc_link = nullptr;
  makecontext(&c.u, entry, 0);
}
static void ctx_switch(emu_ctx& from, emu_ctx& to) { swapcontext(&from.u, &to.u); }
#endif

struct emu_fbar { int parties, count; unsigned gen; };     // lives in the storage of a pthread_barrier_t
static_assert(sizeof(emu_fbar) <= sizeof(pthread_barrier_t), "emu_fbar must fit a pthread_barrier_t");

constexpr size_t FIBER_STACK = 256 * 1024;
struct emu_fiber { emu_ctx ctx; bool done = false; };
static std::vector<emu_fiber> fibers;
static std::vector<char> fiber_stacks;
static emu_ctx main_ctx;
static volatile int fiber_cur = 0, fiber_live = 0;
static const std::function<void()>* fiber_fn = nullptr;

// hand the OS thread to the next lane that has not finished
static __attribute__((noinline)) void fiber_yield() {
  const int n = (int)fibers.size(), me = fiber_cur;
  int nx = me;
  do { nx = nx + 1 == n ? 0 : nx + 1; } while (fibers[nx].done && nx != me);
  if (nx == me) return;
  fiber_cur = nx;
  threadIdx.x = nx;
  ctx_switch(fibers[me].ctx, fibers[nx].ctx);
  threadIdx.x = fiber_cur;
}
static void fiber_entry() {
  (*fiber_fn)();
  const int me = fiber_cur;
  fibers[me].done = true;
  if (--fiber_live == 0) ctx_switch(fibers[me].ctx, main_ctx);
  else fiber_yield();
  abort();                          // a finished fiber is never resumed
}
extern "C" __attribute__((noinline)) int emu_fiber_wait(pthread_barrier_t* b) {
  volatile emu_fbar* B = reinterpret_cast<volatile emu_fbar*>(b);
  const unsigned g = B->gen;
  if (B->count + 1 == B->parties) { B->count = 0; B->gen = g + 1; return 0; }
  B->count = B->count + 1;
  while (B->gen == g) fiber_yield();
  return 0;
}
static void fbar_init(pthread_barrier_t* b, int parties) {
  std::memset(b, 0, sizeof *b);
  reinterpret_cast<emu_fbar*>(b)->parties = parties;
}
// one workgroup of nt lanes executing fn(), all on the calling OS thread
static void fiber_launch(int block, int nt, const std::function<void()>& fn) {
  emu_group g;
  g.waves.resize(nt / 64);
  fbar_init(&g.bar, nt);
  for (auto& w : g.waves) fbar_init(&w.bar, 64);
  emu_g = &g;
  blockIdx.x = block;
  fibers.assign(nt, emu_fiber());
  fiber_stacks.resize((size_t)nt * FIBER_STACK);
  for (int t = 0; t < nt; t++) ctx_make(fibers[t].ctx, fiber_stacks.data() + (size_t)t * FIBER_STACK, FIBER_STACK, fiber_entry);
  fiber_fn = &fn;
  fiber_live = nt;
  fiber_cur = 0;
  threadIdx.x = 0;
  ctx_switch(main_ctx, fibers[0].ctx);
  emu_g = nullptr;
}
