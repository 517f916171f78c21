// At most m hits per domain, exact over a query row's WHOLE eligible set
// (field collapsing on the domain): domain_best finds, per domain id, the
// m best eligible documents of the row, collapse_select takes the first k
// of all of them. Replaces: quality.diversify / facets.cluster_by_domain
// over the LIMITed hit list in the reference, which can only thin that
// list out.
//
// Sibling of domtop.hip: the same per-epoch tables (dom_id [N], a dense
// id in [0, D) per document), the same grid and row prologue and, for the
// BM25 form, the same streaming read (match_queue.h).
//
// Eligible. POSITIVE (BM25 plane): the match rule in the header of
// facets.hip, mask bit and score > 0. Otherwise (dense plane): the mask
// bit alone; every document when there is no mask, whatever its score.
// Rows with NaN are outside the contract, as in topk.hip.
//
// The order (the contract): the 64-bit key
//     float_to_ordered(score) << 32 | (0xFFFFFFFF - d),
// d the shard-local column, descending: score descending (-0.0 below
// +0.0, by the bits as stored), then column ascending. A strict total
// order, so every result is determined bit for bit. No real document has
// key 0 (that would take column 2^32 - 1): 0 marks an empty entry.
//
// domain_best. Workspace best [m, R, D] u64, zeroed by the caller.
// Launched once per level j = 0 .. m-1, in stream order. Every eligible
// document of the chunk forms its key; at level j > 0 it takes part only
// if its key is strictly below best[j-1][r, id] (a zero entry there:
// nothing is left in the domain). The key is maxed (64-bit LDS atomicMax)
// under its id in the workgroup's LDS table (id_table.h), or straight
// into best[j][r, id] when the table has no slot for it. After the chunk
// every occupied slot is flushed with one global atomicMax. Max is exact
// in any order. After level j, best[j][r, id] is the (j+1)-th largest key
// of domain id: the m tables together are exactly the capped set.
//
// collapse_select. One workgroup per row; key_select.h selects and sorts
// the k largest non-zero keys of the row's m * D entries, straight from
// the tables. The first k are written as (score, column) decoded from
// the keys, -inf / -1 past the last one. No host read-back, one launch.
#include "common.h"
#include "id_table.h"
#include "key_select.h"
#include "match_queue.h"

#define COLLAPSE_THREADS MATCHQ_THREADS
#define COLLAPSE_CHUNK MATCHQ_CHUNK
#define COLLAPSE_M_MAX 4
#define COLLAPSE_K_MAX 1024
#define COLSEL_THREADS 1024
#define COLSEL_CAND 4096        // LDS candidate keys of collapse_select

namespace {

DEVINL u64 collapse_key(float score, long d) {
  return ((u64)float_to_ordered(score) << 32) |
         (u64)(0xFFFFFFFFu - (unsigned)d);
}

template <bool POSITIVE, bool MASKED>
__global__ __launch_bounds__(COLLAPSE_THREADS) void domain_best_kernel(
    const float* __restrict__ scores, const int* __restrict__ rows,
    const unsigned* __restrict__ bits, const int* __restrict__ row_pred,
    const int* __restrict__ dom_id, u64* __restrict__ best, long N, long W,
    int B, int P, int D, int R, int level) {
  __shared__ int s_key[IDTAB_SLOTS];   // domain id, -1: free
  __shared__ u64 s_best[IDTAB_SLOTS];
  __shared__ unsigned short s_q[POSITIVE ? COLLAPSE_CHUNK : 1];
  __shared__ unsigned s_n;
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  int b;
  const unsigned* mrow;
  if (!match_row<MASKED>(rows, bits, row_pred, B, P, W, &b, &mrow)) return;
  id_table_init<COLLAPSE_THREADS>(s_key, s_best);
  if (tid == 0) s_n = 0;
  __syncthreads();

  const long c0 = (long)blockIdx.y * COLLAPSE_CHUNK;
  const long c1 = min(c0 + COLLAPSE_CHUNK, N);
  const float* row = scores + (long)b * N;
  u64* out = best + ((long)level * R + r) * D;
  const u64* prev =
      level > 0 ? best + ((long)(level - 1) * R + r) * D : nullptr;
  // Max `key` into the LDS table under `id`, or into out[id] when no
  // slot is found within the probes.
  auto insert = [&](int id, u64 key) {
    if (id < 0 || id >= D) return;
    if (prev != nullptr) {
      const u64 p = prev[id];
      if (p == 0 || key >= p) return;
    }
    const int slot = id_table_slot(s_key, id);
    if (slot >= 0)
      atomicMax(&s_best[slot], key);
    else
      atomicMax(&out[id], key);
  };
  if constexpr (POSITIVE) {
    match_queue_fill<MASKED>(row, mrow, c0, c1, N, s_q, &s_n);
    __syncthreads();
    const unsigned nq = min(s_n, (unsigned)COLLAPSE_CHUNK);
    for (unsigned i = tid; i < nq; i += COLLAPSE_THREADS) {
      const long d = c0 + s_q[i];
      insert(dom_id[d], collapse_key(row[d], d));
    }
  } else {
    // the mask bit alone decides: one document per lane and step, the
    // mask word of 32 neighbours is one broadcast load
    for (long d = c0 + tid; d < c1; d += COLLAPSE_THREADS) {
      if constexpr (MASKED) {
        if (((mrow[d >> 5] >> (unsigned)(d & 31)) & 1u) == 0) continue;
      }
      insert(dom_id[d], collapse_key(row[d], d));
    }
  }
  __syncthreads();
  for (int i = tid; i < IDTAB_SLOTS; i += COLLAPSE_THREADS) {
    const int id = s_key[i];
    const u64 k = s_best[i];
    if (id >= 0 && k) atomicMax(&out[id], k);
  }
}

// f(key) for every non-zero entry of the row's m tables; table j's row
// starts at tabs + j * stride.
template <typename F>
DEVINL void for_entries(const u64* __restrict__ tabs, long stride, int m,
                        int D, F f) {
  for (int j = 0; j < m; ++j) {
    const u64* t = tabs + (long)j * stride;
    for (int i = threadIdx.x; i < D; i += COLSEL_THREADS) {
      const u64 k = t[i];
      if (k) f(k);
    }
  }
}

__global__ __launch_bounds__(COLSEL_THREADS) void collapse_select_kernel(
    const u64* __restrict__ best, float* __restrict__ vals,
    int* __restrict__ idx, int R, int D, int m, int K) {
  __shared__ KeySelectLds<COLSEL_CAND> s_sel;
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  const u64* tabs = best + (long)r * D;
  const long stride = (long)R * D;
  K = min(max(K, 1), COLLAPSE_K_MAX);
  const unsigned nc =
      key_select_sorted<COLSEL_CAND, COLSEL_THREADS, COLLAPSE_K_MAX>(
          s_sel, K, [=](auto f) { for_entries(tabs, stride, m, D, f); });
  for (int i = tid; i < K; i += COLSEL_THREADS) {
    const u64 k = (unsigned)i < nc ? s_sel.cand[i] : 0ull;
    float v = -INFINITY;
    int at = -1;
    if (k) {
      v = ordered_to_float((uint32_t)(k >> 32));
      at = (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull));
    }
    vals[(long)r * K + i] = v;
    idx[(long)r * K + i] = at;
  }
}

}  // namespace

extern "C" int infomesh_collapse_m_max() { return COLLAPSE_M_MAX; }
extern "C" int infomesh_collapse_k_max() { return COLLAPSE_K_MAX; }
extern "C" int infomesh_collapse_chunk_docs() { return COLLAPSE_CHUNK; }
extern "C" int infomesh_collapse_lds_slots() { return IDTAB_SLOTS; }

// scores [B, N] f32, N < 2^31; rows [R] i32 in [0, B); bits [P, W] u32
// with W * 32 >= N and row_pred [B] i32 in [0, P), or both null (no
// mask); dom_id [N] i32 in [0, D); best [m, R, D] u64, zeroed by the
// caller, 1 <= m <= COLLAPSE_M_MAX. positive != 0: the BM25 form. The
// caller guarantees all of that.
extern "C" void infomesh_domain_best(
    const void* scores, const void* rows, const void* bits,
    const void* row_pred, const void* dom_id, void* best, int B, int R,
    long N, long W, int P, int D, int m, int positive, void* stream) {
  if (R <= 0 || N <= 0 || B <= 0 || D <= 0 || m <= 0 || m > COLLAPSE_M_MAX)
    return;
  auto s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)R,
                  (unsigned)((N + COLLAPSE_CHUNK - 1) / COLLAPSE_CHUNK));
  for (int level = 0; level < m; ++level) {
    dispatch_bool(positive != 0, [&](auto pos) {
      dispatch_masked(bits, row_pred, [&](auto masked) {
        hipLaunchKernelGGL(
            (domain_best_kernel<decltype(pos)::value,
                                decltype(masked)::value>),
            grid, dim3(COLLAPSE_THREADS), 0, s, (const float*)scores,
            (const int*)rows, (const unsigned*)bits, (const int*)row_pred,
            (const int*)dom_id, (u64*)best, N, W, B, P, D, R, level);
      });
    });
  }
}

// best [m, R, D] u64 as domain_best left it; vals [R, K] f32 and idx
// [R, K] i32, every element written; 1 <= K <= COLLAPSE_K_MAX.
extern "C" void infomesh_collapse_select(const void* best, void* vals,
                                         void* idx, int R, int D, int m,
                                         int K, void* stream) {
  if (R <= 0 || D <= 0 || m <= 0 || m > COLLAPSE_M_MAX || K <= 0 ||
      K > COLLAPSE_K_MAX)
    return;
  auto s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(collapse_select_kernel, dim3((unsigned)R),
                     dim3(COLSEL_THREADS), 0, s, (const u64*)best,
                     (float*)vals, (int*)idx, R, D, m, K);
}
