// At most m hits per domain, exact over a query row's WHOLE eligible set
// (field collapsing on the domain): domain_best finds, per domain id, the
// m best eligible documents of the row, collapse_select takes the first k
// of all of them. Replaces: quality.diversify / facets.cluster_by_domain
// over the LIMITed hit list in the reference, which can only thin that
// list out.
//
// Sibling of domtop.hip: the same per-epoch tables (dom_id [N], a dense
// id in [0, D) per document), the same grid, rows / bits / row_pred, and
// for the BM25 form the same streaming read (match_queue.h).
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
// Launched once per level j = 0 .. m-1, in stream order; grid
// (R, ceil(N / COLLAPSE_CHUNK)). Every eligible document of the chunk
// forms its key; at level j > 0 it takes part only if its key is strictly
// below best[j-1][r, id] (a zero entry there: nothing is left in the
// domain). The key is maxed into a per-workgroup LDS table keyed by id:
// open addressing, COLLAPSE_SLOTS slots, linear probing, at most
// COLLAPSE_PROBES probes; atomicCAS claims the slot, a 64-bit LDS
// atomicMax holds the key. A key that finds no slot goes straight to a
// global 64-bit atomicMax. After the chunk every occupied slot is flushed
// with one global atomicMax. Max is exact in any order, so the result
// depends on neither the table size nor the hash. After level j,
// best[j][r, id] is the (j+1)-th largest key of domain id: the m tables
// together are exactly the capped set.
//
// collapse_select. One workgroup per row; the k largest non-zero keys of
// the row's m * D entries. A first read finds the largest key and the
// number of non-zero entries; then an MSB-first radix select, 8 bits a
// pass, straight from the tables, narrows down the bucket that holds the
// k-th key. As soon as the keys above the bucket plus the bucket fit the
// LDS candidate buffer they are gathered and sorted (bitonic), and the
// first k are written as (score, column) decoded from the keys, -inf / -1
// past the last one. Keys are distinct, so after all eight passes the
// bucket holds one key and fewer than k lie above it: the loop always
// ends with a set that fits. No host read-back, one launch.
#include "common.h"
#include "match_queue.h"

#define COLLAPSE_THREADS MATCHQ_THREADS
#define COLLAPSE_CHUNK MATCHQ_CHUNK
#define COLLAPSE_M_MAX 4
#define COLLAPSE_K_MAX 1024
#define COLLAPSE_SLOTS 2048     // LDS table of domain_best, a power of two
#define COLLAPSE_SLOT_BITS 11
#define COLLAPSE_PROBES 8
#define COLSEL_THREADS 1024
#define COLSEL_CAND 4096        // LDS candidate keys of collapse_select
static_assert((1 << COLLAPSE_SLOT_BITS) == COLLAPSE_SLOTS, "power of two");
static_assert(COLSEL_CAND >= COLLAPSE_K_MAX &&
                  (COLSEL_CAND & (COLSEL_CAND - 1)) == 0,
              "the candidates hold k keys and sort as a power of two");

namespace {

typedef unsigned long long u64;

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
  __shared__ int s_key[COLLAPSE_SLOTS];   // domain id, -1: free
  __shared__ u64 s_best[COLLAPSE_SLOTS];
  __shared__ unsigned short s_q[POSITIVE ? COLLAPSE_CHUNK : 1];
  __shared__ unsigned s_n;
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  // the caller checks rows and row_pred; the clamps keep a bad call
  // inside the arrays all the same (block-uniform)
  const int b = rows[r];
  if (b < 0 || b >= B) return;
  const unsigned* mrow = nullptr;
  if constexpr (MASKED) {
    const int p = row_pred[b];
    if (p < 0 || p >= P) return;
    mrow = bits + (long)p * W;
  }
  for (int i = tid; i < COLLAPSE_SLOTS; i += COLLAPSE_THREADS) {
    s_key[i] = -1;
    s_best[i] = 0;
  }
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
    unsigned slot =
        ((unsigned)id * 2654435761u) >> (32 - COLLAPSE_SLOT_BITS);
    for (int p = 0; p < COLLAPSE_PROBES; ++p) {
      const int was = atomicCAS(&s_key[slot], -1, id);
      if (was == -1 || was == id) {
        atomicMax(&s_best[slot], key);
        return;
      }
      slot = (slot + 1) & (COLLAPSE_SLOTS - 1);
    }
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
  for (int i = tid; i < COLLAPSE_SLOTS; i += COLLAPSE_THREADS) {
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
  __shared__ u64 s_cand[COLSEL_CAND];
  __shared__ unsigned s_hist[HIST8_U32];
  __shared__ unsigned s_bins[256];
  __shared__ u64 s_max;
  __shared__ unsigned s_nnz, s_nc;
  // the select's state, written by thread 0 between barriers
  __shared__ u64 s_prefix, s_det;   // the bucket: key & det == prefix
  __shared__ unsigned s_need, s_above, s_bucket;
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  const u64* tabs = best + (long)r * D;
  const long stride = (long)R * D;
  K = min(max(K, 1), COLLAPSE_K_MAX);
  if (tid == 0) {
    s_max = 0;
    s_nnz = 0;
    s_nc = 0;
  }
  __syncthreads();
  {
    u64 mx = 0;
    unsigned nz = 0;
    for_entries(tabs, stride, m, D, [&](u64 k) {
      mx = k > mx ? k : mx;
      ++nz;
    });
    for (int off = 32; off > 0; off >>= 1) {
      const u64 o = __shfl_xor(mx, off, WAVE);
      mx = o > mx ? o : mx;
      nz += __shfl_xor(nz, off, WAVE);
    }
    if ((tid & (WAVE - 1)) == 0 && nz) {
      atomicMax(&s_max, mx);
      atomicAdd(&s_nnz, nz);
    }
  }
  __syncthreads();
  if (tid == 0) {
    s_prefix = 0;
    s_det = 0;
    s_need = (unsigned)K;
    s_above = 0;
    s_bucket = s_nnz;
  }
  __syncthreads();
  // every key has no bit at or above `top`
  int top = 0;
  while (top < 64 && (s_max >> top)) ++top;
  // all reads of the state below are behind a barrier and block-uniform
  for (int shift = (top + 7) / 8 * 8 - 8;
       shift >= 0 && s_above + s_bucket > COLSEL_CAND; shift -= 8) {
    hist8_zero(s_hist);
    __syncthreads();
    const u64 prefix = s_prefix, det = s_det;
    unsigned* mine = hist8_mine(s_hist);
    for_entries(tabs, stride, m, D, [&](u64 k) {
      if ((k & det) == prefix)
        atomicAdd(&mine[(unsigned)(k >> shift) & 255u], 1u);
    });
    __syncthreads();
    if (tid < 256) {
      unsigned sum = 0;
#pragma unroll
      for (int c = 0; c < HIST8_COPIES; ++c)
        sum += s_hist[c * HIST8_STRIDE + tid];
      s_bins[tid] = sum;
    }
    __syncthreads();
    if (tid == 0) {
      // the bin of the need-th largest key of the bucket, from the top
      unsigned cum = 0;
      int bin = 255;
      for (; bin > 0; --bin) {
        if (cum + s_bins[bin] >= s_need) break;
        cum += s_bins[bin];
      }
      // the bucket holds at least `need` keys or all that are left: when
      // the scan runs out at bin 0 that bin is the rest either way
      s_above += cum;
      s_need -= min(cum, s_need - 1);
      s_bucket = s_bins[bin];
      s_prefix = prefix | ((u64)bin << shift);
      s_det = det | (255ull << shift);
    }
    __syncthreads();
  }
  // gather: every key whose determined bits are >= the prefix
  {
    const u64 prefix = s_prefix, det = s_det;
    for_entries(tabs, stride, m, D, [&](u64 k) {
      if ((k & det) >= prefix) {
        const unsigned at = atomicAdd(&s_nc, 1u);
        if (at < COLSEL_CAND) s_cand[at] = k;
      }
    });
  }
  __syncthreads();
  const unsigned nc = min(s_nc, (unsigned)COLSEL_CAND);
  unsigned n2 = 1;
  while (n2 < nc) n2 <<= 1;
  for (unsigned i = nc + tid; i < n2; i += COLSEL_THREADS) s_cand[i] = 0;
  __syncthreads();
  // bitonic sort, descending; every thread takes its pairs of a step
  for (unsigned size = 2; size <= n2; size <<= 1) {
    for (unsigned stride2 = size >> 1; stride2 > 0; stride2 >>= 1) {
      for (unsigned t = (unsigned)tid; t < (n2 >> 1); t += COLSEL_THREADS) {
        const unsigned lo = 2 * t - (t & (stride2 - 1));
        const unsigned hi = lo + stride2;
        const bool desc = (lo & size) == 0;
        const u64 a = s_cand[lo], c = s_cand[hi];
        if (desc ? a < c : a > c) {
          s_cand[lo] = c;
          s_cand[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < K; i += COLSEL_THREADS) {
    const u64 k = (unsigned)i < nc ? s_cand[i] : 0ull;
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

template <bool POSITIVE>
void launch_best(hipStream_t s, dim3 grid, const void* scores,
                 const void* rows, const void* bits, const void* row_pred,
                 const void* dom_id, void* best, long N, long W, int B,
                 int P, int D, int R, int level) {
  if (bits != nullptr && row_pred != nullptr) {
    hipLaunchKernelGGL((domain_best_kernel<POSITIVE, true>), grid,
                       dim3(COLLAPSE_THREADS), 0, s, (const float*)scores,
                       (const int*)rows, (const unsigned*)bits,
                       (const int*)row_pred, (const int*)dom_id, (u64*)best,
                       N, W, B, P, D, R, level);
  } else {
    hipLaunchKernelGGL((domain_best_kernel<POSITIVE, false>), grid,
                       dim3(COLLAPSE_THREADS), 0, s, (const float*)scores,
                       (const int*)rows, (const unsigned*)nullptr,
                       (const int*)nullptr, (const int*)dom_id, (u64*)best,
                       N, W, B, P, D, R, level);
  }
}

}  // namespace

extern "C" int infomesh_collapse_m_max() { return COLLAPSE_M_MAX; }
extern "C" int infomesh_collapse_k_max() { return COLLAPSE_K_MAX; }
extern "C" int infomesh_collapse_chunk_docs() { return COLLAPSE_CHUNK; }
extern "C" int infomesh_collapse_lds_slots() { return COLLAPSE_SLOTS; }

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
    if (positive)
      launch_best<true>(s, grid, scores, rows, bits, row_pred, dom_id, best,
                        N, W, B, P, D, R, level);
    else
      launch_best<false>(s, grid, scores, rows, bits, row_pred, dom_id,
                         best, N, W, B, P, D, R, level);
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
