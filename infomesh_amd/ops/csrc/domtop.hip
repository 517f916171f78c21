// Top domains by match count over a query row's WHOLE match set, with no
// list from the caller: domain_count tallies every matching document by
// its shard-local domain id, domain_select takes the first K domains of
// the tally. Replaces: domain_counter.most_common(20) over the LIMITed
// hit list in the reference's compute_facets (infomesh/search/facets.py).
//
// The match rule is the one in the header of facets.hip, and the grid,
// the row prologue and the streaming read that finds the matches are
// shared with it (match_queue.h). The shard keeps, per epoch, dom_keys
// [D] (the distinct w2 words of its rows, ascending as unsigned) and
// dom_id [N] (each row's index into dom_keys), so a domain is a dense id
// in [0, D) here and ids ascend with hashes.
//
// The order (the contract): count descending, then hash ascending as
// unsigned = id ascending: a strict total order, so every result is
// determined bit for bit.
//
// domain_count. Step 1 queues the chunk's matching documents in LDS.
// Step 2 takes one queued document per lane, loads its dom_id (4 bytes
// per match) and adds 1 under its id in the workgroup's LDS table
// (id_table.h), or straight to cnt[r, id] when the table has no slot for
// it. Lanes of a wave that hold the same id as the wave's first active
// lane are folded into that lane's add first, so a match set dominated
// by one site does not serialise 64 LDS atomics on one address per step.
// After the chunk every occupied slot is flushed with one global
// atomicAdd: with the LDS stage one address of cnt sees at most one
// atomic per chunk, plus whatever overflowed. Integer adds: exact in any
// order.
//
// domain_select. One workgroup per counted row. The key of domain id with
// count c > 0 is c << idbits | (D - 1 - id), idbits the width of D - 1:
// distinct per id, and descending key order is the contract's order.
// Zeros are skipped everywhere. key_select.h selects and sorts the K
// largest keys straight from the cnt row; they are written as (hash
// bits, count) pairs, (0, 0) past the last real one. Exact among ties as
// well: the id is part of the key. No host read-back, one launch.
#include "common.h"
#include "id_table.h"
#include "key_select.h"
#include "match_queue.h"

#define DOMTOP_THREADS MATCHQ_THREADS
#define DOMTOP_CHUNK MATCHQ_CHUNK
#define DOMTOP_K_MAX 65
#define DOMSEL_THREADS 1024
#define DOMSEL_CAND 2048        // LDS candidate keys of domain_select

namespace {

template <bool MASKED>
__global__ __launch_bounds__(DOMTOP_THREADS) void domain_count_kernel(
    const float* __restrict__ scores, const int* __restrict__ rows,
    const unsigned* __restrict__ bits, const int* __restrict__ row_pred,
    const int* __restrict__ dom_id, int* __restrict__ cnt, long N, long W,
    int B, int P, int D) {
  __shared__ int s_key[IDTAB_SLOTS];   // domain id, -1: free
  __shared__ int s_add[IDTAB_SLOTS];
  __shared__ unsigned short s_q[DOMTOP_CHUNK];
  __shared__ unsigned s_n;
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  int b;
  const unsigned* mrow;
  if (!match_row<MASKED>(rows, bits, row_pred, B, P, W, &b, &mrow)) return;
  id_table_init<DOMTOP_THREADS>(s_key, s_add);
  if (tid == 0) s_n = 0;
  __syncthreads();

  const long c0 = (long)blockIdx.y * DOMTOP_CHUNK;
  const long c1 = min(c0 + DOMTOP_CHUNK, N);
  match_queue_fill<MASKED>(scores + (long)b * N, mrow, c0, c1, N, s_q, &s_n);
  __syncthreads();
  const unsigned nq = min(s_n, (unsigned)DOMTOP_CHUNK);
  int* out = cnt + (long)r * D;
  for (unsigned i = tid; i < nq; i += DOMTOP_THREADS) {
    const int id = dom_id[c0 + s_q[i]];
    // fold the lanes that share the first active lane's id into it
    const unsigned long long act = __ballot(1);
    const int lead = __ffsll((long long)act) - 1;
    const int id0 = __shfl(id, lead, WAVE);
    const unsigned long long same = __ballot(id == id0);
    int add = 1;
    if (id == id0) add = (tid & (WAVE - 1)) == lead ? __popcll(same) : 0;
    if (add == 0 || id < 0 || id >= D) continue;
    const int slot = id_table_slot(s_key, id);
    if (slot >= 0)
      atomicAdd(&s_add[slot], add);
    else
      atomicAdd(&out[id], add);
  }
  __syncthreads();
  for (int i = tid; i < IDTAB_SLOTS; i += DOMTOP_THREADS) {
    const int id = s_key[i];
    if (id >= 0) atomicAdd(&out[id], s_add[i]);
  }
}

// f(id, count) for every id of the row with count > 0, four ids per lane
// and step (the row starts at a 4-byte boundary only: the unaligned
// dwordx4 loads of match_queue.h).
template <typename F>
DEVINL void for_nonzero(const int* __restrict__ row, int D, F f) {
  for (long i = (long)threadIdx.x * 4; i < D; i += DOMSEL_THREADS * 4) {
    if (i + 4 <= D) {
      const int4 v = *reinterpret_cast<const int4*>(row + i);
      if (v.x > 0) f((int)i, v.x);
      if (v.y > 0) f((int)i + 1, v.y);
      if (v.z > 0) f((int)i + 2, v.z);
      if (v.w > 0) f((int)i + 3, v.w);
    } else {
      for (long j = i; j < D; ++j)
        if (row[j] > 0) f((int)j, row[j]);
    }
  }
}

__global__ __launch_bounds__(DOMSEL_THREADS) void domain_select_kernel(
    const int* __restrict__ cnt, const int* __restrict__ dom_keys,
    int* __restrict__ out, int D, int K) {
  __shared__ KeySelectLds<DOMSEL_CAND> s_sel;
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  const int* row = cnt + (long)r * D;
  K = min(max(K, 1), DOMTOP_K_MAX);
  int idbits = 0;
  while (idbits < 32 && ((u64)(D - 1) >> idbits)) ++idbits;
  const u64 idmask = (1ull << idbits) - 1ull;
  const unsigned nc =
      key_select_sorted<DOMSEL_CAND, DOMSEL_THREADS, DOMTOP_K_MAX>(
          s_sel, K, [=](auto f) {
            for_nonzero(row, D, [&](int id, int c) {
              f(((u64)(unsigned)c << idbits) | (u64)(unsigned)(D - 1 - id));
            });
          });
  if (tid < K) {
    int2 o = make_int2(0, 0);
    const u64 k = (unsigned)tid < nc ? s_sel.cand[tid] : 0ull;
    if (k) {
      const int id = D - 1 - (int)(k & idmask);
      if (id >= 0 && id < D) o = make_int2(dom_keys[id], (int)(k >> idbits));
    }
    reinterpret_cast<int2*>(out)[(long)r * K + tid] = o;
  }
}

}  // namespace

extern "C" int infomesh_domtop_chunk_docs() { return DOMTOP_CHUNK; }
extern "C" int infomesh_domtop_lds_slots() { return IDTAB_SLOTS; }
extern "C" int infomesh_domtop_k_max() { return DOMTOP_K_MAX; }

// scores [B, N] f32; rows [R] i32 in [0, B); bits [P, W] u32 with
// W * 32 >= N and row_pred [B] i32 in [0, P), or both null (no mask);
// dom_id [N] i32 in [0, D); cnt [R, D] i32, zeroed by the caller. The
// caller guarantees all of that.
extern "C" void infomesh_domain_count(
    const void* scores, const void* rows, const void* bits,
    const void* row_pred, const void* dom_id, void* cnt, int B, int R,
    long N, long W, int P, int D, void* stream) {
  if (R <= 0 || N <= 0 || B <= 0 || D <= 0) return;
  auto s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)R,
                  (unsigned)((N + DOMTOP_CHUNK - 1) / DOMTOP_CHUNK));
  dispatch_masked(bits, row_pred, [&](auto masked) {
    hipLaunchKernelGGL(domain_count_kernel<decltype(masked)::value>, grid,
                       dim3(DOMTOP_THREADS), 0, s, (const float*)scores,
                       (const int*)rows, (const unsigned*)bits,
                       (const int*)row_pred, (const int*)dom_id, (int*)cnt,
                       N, W, B, P, D);
  });
}

// cnt [R, D] i32, counts >= 0; dom_keys [D] i32 (u32 bits); out [R, K, 2]
// i32, every element written; 1 <= K <= DOMTOP_K_MAX, D >= 1.
extern "C" void infomesh_domain_select(const void* cnt, const void* dom_keys,
                                       void* out, int R, int D, int K,
                                       void* stream) {
  if (R <= 0 || D <= 0 || K <= 0 || K > DOMTOP_K_MAX) return;
  auto s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(domain_select_kernel, dim3((unsigned)R),
                     dim3(DOMSEL_THREADS), 0, s, (const int*)cnt,
                     (const int*)dom_keys, (int*)out, D, K);
}
