// A sum that crosses workgroups without float atomics and without anybody waiting (hk_dqn_td's loss, hk_optim_prepare's
// squared norm): every workgroup leaves its part in the workspace slot with its own index and draws a ticket; the
// workgroup whose ticket is the last adds the slots in index order, so the sum is the same bits on every launch.
//
// The part is stored with an agent-scope atomic store (write-through), the store has left the CU (s_waitcnt vmcnt(0))
// before the ticket is drawn with an agent-scope fetch_add.  The workgroup whose ticket is the last learns so from the
// value the add returned: by then every other workgroup's slot has drained.  Its lane runs an agent-scope acquire and
// waits for it, the workgroup passes a barrier, and every slot is read with an agent-scope atomic load (past L1, never a
// plain load, never through the scalar cache).  A per-XCD L2 is not coherent with the others and a CU's L1 is never
// refreshed by another CU's stores, so a plain store or load anywhere on that path could be stale.
#pragma once

#include "hk_common.h"

namespace hk {

constexpr int kTicketSlotOffset = 2;  // workspace words (8 bytes each) in front of the slots: the ticket, one spare

__device__ __forceinline__ double slot_load(const unsigned long long* p) {
  return __longlong_as_double((long long)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void slot_store(unsigned long long* p, double v) {
  __hip_atomic_store(p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ONE lane of the workgroup: draws a ticket of `tickets`; true for the last one, whose holder may read every slot
__device__ __forceinline__ bool ticket_draw(unsigned long long* ws, unsigned tickets) {
  // the slot has left this CU before the ticket says so (inline asm: the compiler may not drop or move it)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long old = __hip_atomic_fetch_add(ws, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool last = old == (unsigned long long)tickets - 1ull;
  if (last) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  return last;
}

// the whole workgroup of THREADS lanes, after the barrier that followed ticket_draw: the slots [0, slots) added in index
// order; the sum is lane 0's.  s_slot: THREADS doubles of LDS.
template <int THREADS>
__device__ __forceinline__ double ticket_sum(const unsigned long long* ws, unsigned slots, double* s_slot, int tid) {
  double total = 0.0;
  for (unsigned base = 0; base < slots; base += THREADS) {
    const unsigned i = base + (unsigned)tid;
    s_slot[tid] = i < slots ? slot_load(ws + kTicketSlotOffset + i) : 0.0;
    __syncthreads();
    if (tid == 0) {
      const unsigned n = slots - base < (unsigned)THREADS ? slots - base : (unsigned)THREADS;
      for (unsigned k = 0; k < n; ++k) total += s_slot[k];
    }
    __syncthreads();
  }
  return total;
}

// lane 0 of the last workgroup, when it is done: the ticket is zero for the next launch
__device__ __forceinline__ void ticket_reset(unsigned long long* ws) {
  __hip_atomic_store(ws, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace hk
