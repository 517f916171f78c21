// The per-workgroup LDS table keyed by domain id, of domtop.hip's
// domain_count and collapse.hip's domain_best: open addressing,
// IDTAB_SLOTS slots, linear probing, at most IDTAB_PROBES probes;
// atomicCAS claims a slot for an id. The values live in an array of the
// kernel's own (int adds in one, 64-bit maxima in the other), indexed by
// the slot. An id that finds no slot within the probes goes straight to
// global memory, and after the chunk the kernel flushes every occupied
// slot with one global atomic: both kernels combine with an operation
// that is exact in any order, so their results depend on neither the
// table size nor the hash.
#pragma once
#include "common.h"

#define IDTAB_SLOTS 2048   // a power of two
#define IDTAB_SLOT_BITS 11
#define IDTAB_PROBES 8
static_assert((1 << IDTAB_SLOT_BITS) == IDTAB_SLOTS, "power of two");

// Every slot free (s_key -1) and its value zero; a barrier follows
// before the first id_table_slot.
template <int THREADS, typename V>
DEVINL void id_table_init(int* s_key, V* s_val) {
  for (int i = threadIdx.x; i < IDTAB_SLOTS; i += THREADS) {
    s_key[i] = -1;
    s_val[i] = 0;
  }
}

// The slot of `id` (>= 0), claimed now or earlier; -1 when the probes
// found none.
DEVINL int id_table_slot(int* s_key, int id) {
  unsigned slot = ((unsigned)id * 2654435761u) >> (32 - IDTAB_SLOT_BITS);
  for (int p = 0; p < IDTAB_PROBES; ++p) {
    const int was = atomicCAS(&s_key[slot], -1, id);
    if (was == -1 || was == id) return (int)slot;
    slot = (slot + 1) & (IDTAB_SLOTS - 1);
  }
  return -1;
}
