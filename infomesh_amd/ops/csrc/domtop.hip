// Top domains by match count over a query row's WHOLE match set, with no
// list from the caller: domain_count tallies every matching document by
// its shard-local domain id, domain_select takes the first K domains of
// the tally. Replaces: domain_counter.most_common(20) over the LIMITed
// hit list in the reference's compute_facets (infomesh/search/facets.py).
//
// The match rule is the one in the header of facets.hip, and the
// streaming read that finds the matches is shared with it
// (match_queue.h). The shard keeps, per epoch, dom_keys [D] (the distinct
// w2 words of its rows, ascending as unsigned) and dom_id [N] (each row's
// index into dom_keys), so a domain is a dense id in [0, D) here and ids
// ascend with hashes.
//
// The order (the contract): count descending, then hash ascending as
// unsigned = id ascending: a strict total order, so every result is
// determined bit for bit.
//
// domain_count. Grid (R, ceil(N / DOMTOP_CHUNK)) as in facets.hip, same
// rows / bits / row_pred. Step 1 queues the chunk's matching documents in
// LDS. Step 2 takes one queued document per lane, loads its dom_id (4
// bytes per match) and adds 1 to a per-workgroup LDS table keyed by id:
// open addressing, DOMTOP_SLOTS slots, linear probing, at most
// DOMTOP_PROBES probes. A key that finds no slot within the probes adds
// straight to cnt[r, id] in global memory. Lanes of a wave that hold the
// same id as the wave's first active lane are folded into that lane's
// add first, so a match set dominated by one site does not serialise 64
// LDS atomics on one address per step. After the chunk every occupied
// slot is flushed with one global atomicAdd: with the LDS stage one
// address of cnt sees at most one atomic per chunk, plus whatever
// overflowed. Integer adds: exact in any order, whatever the table size
// and the hash.
//
// domain_select. One workgroup per counted row. The key of domain id with
// count c > 0 is c << idbits | (D - 1 - id), idbits the width of D - 1:
// distinct per id, and descending key order is the contract's order.
// Zeros are skipped everywhere. A first read finds the largest key and
// the number of non-zero counts; then an MSB-first radix select, 8 bits a
// pass, straight from the cnt row, narrows down the bucket that holds
// the K-th key. A (keys above the bucket, fewer than K) and S (the
// bucket) are kept as a prefix test; as soon as |A| + |S| fits the LDS
// candidate buffer the keys of both are gathered, sorted with a bitonic
// sort, and the first K are written as (hash bits, count) pairs, (0, 0)
// past the last real one. Exact among ties as well: the id is part of
// the key. No host read-back, one launch.
#include "common.h"
#include "match_queue.h"

#define DOMTOP_THREADS MATCHQ_THREADS
#define DOMTOP_CHUNK MATCHQ_CHUNK
#define DOMTOP_SLOTS 2048       // LDS table of domain_count, a power of two
#define DOMTOP_SLOT_BITS 11
#define DOMTOP_PROBES 8
#define DOMTOP_K_MAX 65
#define DOMSEL_THREADS 1024
#define DOMSEL_CAND 2048        // LDS candidate keys of domain_select
static_assert((1 << DOMTOP_SLOT_BITS) == DOMTOP_SLOTS, "power of two");
static_assert(DOMSEL_CAND >= DOMTOP_K_MAX &&
                  (DOMSEL_CAND & (DOMSEL_CAND - 1)) == 0 &&
                  DOMSEL_CAND <= 2 * DOMSEL_THREADS,
              "the sort takes one pair per thread and step");

namespace {

template <bool MASKED>
__global__ __launch_bounds__(DOMTOP_THREADS) void domain_count_kernel(
    const float* __restrict__ scores, const int* __restrict__ rows,
    const unsigned* __restrict__ bits, const int* __restrict__ row_pred,
    const int* __restrict__ dom_id, int* __restrict__ cnt, long N, long W,
    int B, int P, int D) {
  __shared__ int s_key[DOMTOP_SLOTS];   // domain id, -1: free
  __shared__ int s_add[DOMTOP_SLOTS];
  __shared__ unsigned short s_q[DOMTOP_CHUNK];
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
  for (int i = tid; i < DOMTOP_SLOTS; i += DOMTOP_THREADS) {
    s_key[i] = -1;
    s_add[i] = 0;
  }
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
    unsigned slot = ((unsigned)id * 2654435761u) >> (32 - DOMTOP_SLOT_BITS);
    bool placed = false;
    for (int p = 0; p < DOMTOP_PROBES; ++p) {
      const int prev = atomicCAS(&s_key[slot], -1, id);
      if (prev == -1 || prev == id) {
        atomicAdd(&s_add[slot], add);
        placed = true;
        break;
      }
      slot = (slot + 1) & (DOMTOP_SLOTS - 1);
    }
    if (!placed) atomicAdd(&out[id], add);
  }
  __syncthreads();
  for (int i = tid; i < DOMTOP_SLOTS; i += DOMTOP_THREADS) {
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
  __shared__ unsigned long long s_cand[DOMSEL_CAND];
  __shared__ unsigned s_hist[HIST8_U32];
  __shared__ unsigned s_bins[256];
  __shared__ unsigned long long s_max;
  __shared__ unsigned s_nnz, s_nc;
  // the select's state, written by thread 0 between barriers
  __shared__ unsigned long long s_prefix, s_det;  // S: key & det == prefix
  __shared__ unsigned s_need, s_above, s_bucket;
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  const int* row = cnt + (long)r * D;
  K = min(max(K, 1), DOMTOP_K_MAX);
  int idbits = 0;
  while (idbits < 32 && ((unsigned long long)(D - 1) >> idbits)) ++idbits;
  const unsigned long long idmask = (1ull << idbits) - 1ull;
  auto key_of = [=](int id, int c) {
    return ((unsigned long long)(unsigned)c << idbits) |
           (unsigned long long)(unsigned)(D - 1 - id);
  };
  if (tid == 0) {
    s_max = 0;
    s_nnz = 0;
    s_nc = 0;
  }
  __syncthreads();
  {
    unsigned long long mx = 0;
    unsigned nz = 0;
    for_nonzero(row, D, [&](int id, int c) {
      const unsigned long long k = key_of(id, c);
      mx = k > mx ? k : mx;
      ++nz;
    });
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(mx, off, WAVE);
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
       shift >= 0 && s_above + s_bucket > DOMSEL_CAND; shift -= 8) {
    hist8_zero(s_hist);
    __syncthreads();
    const unsigned long long prefix = s_prefix, det = s_det;
    unsigned* mine = hist8_mine(s_hist);
    for_nonzero(row, D, [&](int id, int c) {
      const unsigned long long k = key_of(id, c);
      if ((k & det) == prefix) atomicAdd(&mine[(k >> shift) & 255u], 1u);
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
      // the bucket of the need-th largest key of S, from the top
      unsigned cum = 0;
      int bin = 255;
      for (; bin > 0; --bin) {
        if (cum + s_bins[bin] >= s_need) break;
        cum += s_bins[bin];
      }
      // S holds at least `need` keys or all the non-zero ones: when the
      // scan runs out at bin 0 that bucket is the rest either way
      s_above += cum;
      s_need -= min(cum, s_need - 1);
      s_bucket = s_bins[bin];
      s_prefix = prefix | ((unsigned long long)bin << shift);
      s_det = det | (255ull << shift);
    }
    __syncthreads();
  }
  // gather A and S: every key whose determined bits are >= the prefix
  {
    const unsigned long long prefix = s_prefix, det = s_det;
    for_nonzero(row, D, [&](int id, int c) {
      const unsigned long long k = key_of(id, c);
      if ((k & det) >= prefix) {
        const unsigned at = atomicAdd(&s_nc, 1u);
        if (at < DOMSEL_CAND) s_cand[at] = k;
      }
    });
  }
  __syncthreads();
  const unsigned nc = min(s_nc, (unsigned)DOMSEL_CAND);
  unsigned n2 = 1;
  while (n2 < nc) n2 <<= 1;
  for (unsigned i = nc + tid; i < n2; i += DOMSEL_THREADS) s_cand[i] = 0;
  __syncthreads();
  // bitonic sort, descending; one pair per thread and step
  for (unsigned size = 2; size <= n2; size <<= 1) {
    for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
      const unsigned t = (unsigned)tid;
      if (t < (n2 >> 1)) {
        const unsigned lo = 2 * t - (t & (stride - 1));
        const unsigned hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long a = s_cand[lo], c = s_cand[hi];
        if (desc ? a < c : a > c) {
          s_cand[lo] = c;
          s_cand[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  if (tid < K) {
    int2 o = make_int2(0, 0);
    const unsigned long long k = (unsigned)tid < nc ? s_cand[tid] : 0ull;
    if (k) {
      const int id = D - 1 - (int)(k & idmask);
      if (id >= 0 && id < D) o = make_int2(dom_keys[id], (int)(k >> idbits));
    }
    reinterpret_cast<int2*>(out)[(long)r * K + tid] = o;
  }
}

}  // namespace

extern "C" int infomesh_domtop_chunk_docs() { return DOMTOP_CHUNK; }
extern "C" int infomesh_domtop_lds_slots() { return DOMTOP_SLOTS; }
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
  if (bits != nullptr && row_pred != nullptr) {
    hipLaunchKernelGGL(domain_count_kernel<true>, grid,
                       dim3(DOMTOP_THREADS), 0, s, (const float*)scores,
                       (const int*)rows, (const unsigned*)bits,
                       (const int*)row_pred, (const int*)dom_id, (int*)cnt,
                       N, W, B, P, D);
  } else {
    hipLaunchKernelGGL(domain_count_kernel<false>, grid,
                       dim3(DOMTOP_THREADS), 0, s, (const float*)scores,
                       (const int*)rows, (const unsigned*)nullptr,
                       (const int*)nullptr, (const int*)dom_id, (int*)cnt, N,
                       W, B, P, D);
  }
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
