// The K largest of a row's 64-bit keys, sorted, in one workgroup: the
// select of domtop.hip's domain_select and collapse.hip's
// collapse_select.
//
// The contract. The caller enumerates the row's keys; they are distinct
// and non-zero, and 0 is the empty key (it pads the result and is never
// enumerated). Descending key order is the caller's result order, so
// with distinct keys every result is determined bit for bit, ties in
// whatever the key encodes included.
//
// The algorithm. A first read finds the largest key and the number of
// keys; then an MSB-first radix select, 8 bits a pass, straight from the
// caller's enumeration, narrows down the bucket S (key & det == prefix)
// that holds the K-th largest key, with `above` keys above it (fewer
// than K) and `need` = K - above of S still wanted. As soon as
// above + |S| fits the LDS candidate buffer the keys of both, (key &
// det) >= prefix, are gathered, padded with zeros to a power of two and
// sorted descending with a bitonic sort. No pass runs when all keys fit
// at once. Keys are distinct, so once every bit is determined S holds
// one key and fewer than K <= CAND lie above it: the loop always ends
// with a set that fits, after at most eight passes.
//
// Barriers. Every thread of the THREADS-wide workgroup makes the call
// and reaches every barrier in it: all reads of the select's state are
// behind a barrier and block-uniform, so trip counts are too. The state
// is written by thread 0 between barriers. The call ends behind a
// barrier: s.cand is ready to read.
#pragma once
#include "common.h"

typedef unsigned long long u64;

template <int CAND>
struct KeySelectLds {
  static_assert((CAND & (CAND - 1)) == 0,
                "the candidates sort as a power of two");
  u64 cand[CAND];
  unsigned hist[HIST8_U32];
  unsigned bins[256];
  u64 max;
  u64 prefix, det;   // S: key & det == prefix
  unsigned nnz, nc;
  unsigned need, above, bucket;
};

// for_keys(f) calls f(key) for every key of this workgroup's row, each
// key by exactly one thread, the same set on every call. 1 <= K <= K_MAX,
// the calling kernel's cap. Returns nc; s.cand[0 .. nc) holds, sorted
// descending, every key >= the K-th largest (all keys when there are
// fewer than K), and zeros from there up to the next power of two.
template <int CAND, int THREADS, int K_MAX, typename ForKeys>
DEVINL unsigned key_select_sorted(KeySelectLds<CAND>& s, int K,
                                  ForKeys for_keys) {
  static_assert(CAND >= K_MAX, "the candidates hold K keys");
  const int tid = threadIdx.x;
  if (tid == 0) {
    s.max = 0;
    s.nnz = 0;
    s.nc = 0;
  }
  __syncthreads();
  {
    u64 mx = 0;
    unsigned nz = 0;
    for_keys([&](u64 k) {
      mx = k > mx ? k : mx;
      ++nz;
    });
    for (int off = 32; off > 0; off >>= 1) {
      const u64 o = __shfl_xor(mx, off, WAVE);
      mx = o > mx ? o : mx;
      nz += __shfl_xor(nz, off, WAVE);
    }
    if ((tid & (WAVE - 1)) == 0 && nz) {
      atomicMax(&s.max, mx);
      atomicAdd(&s.nnz, nz);
    }
  }
  __syncthreads();
  if (tid == 0) {
    s.prefix = 0;
    s.det = 0;
    s.need = (unsigned)K;
    s.above = 0;
    s.bucket = s.nnz;
  }
  __syncthreads();
  // every key has no bit at or above `top`
  int top = 0;
  while (top < 64 && (s.max >> top)) ++top;
  for (int shift = (top + 7) / 8 * 8 - 8;
       shift >= 0 && s.above + s.bucket > CAND; shift -= 8) {
    hist8_zero(s.hist);
    __syncthreads();
    const u64 prefix = s.prefix, det = s.det;
    unsigned* mine = hist8_mine(s.hist);
    for_keys([&](u64 k) {
      if ((k & det) == prefix)
        atomicAdd(&mine[(unsigned)(k >> shift) & 255u], 1u);
    });
    __syncthreads();
    if (tid < 256) {
      unsigned sum = 0;
#pragma unroll
      for (int c = 0; c < HIST8_COPIES; ++c)
        sum += s.hist[c * HIST8_STRIDE + tid];
      s.bins[tid] = sum;
    }
    __syncthreads();
    if (tid == 0) {
      // the bin of the need-th largest key of S, from the top
      unsigned cum = 0;
      int bin = 255;
      for (; bin > 0; --bin) {
        if (cum + s.bins[bin] >= s.need) break;
        cum += s.bins[bin];
      }
      // S holds at least `need` keys or all there are: when the scan
      // runs out at bin 0 that bin is the rest either way
      s.above += cum;
      s.need -= min(cum, s.need - 1);
      s.bucket = s.bins[bin];
      s.prefix = prefix | ((u64)bin << shift);
      s.det = det | (255ull << shift);
    }
    __syncthreads();
  }
  // gather the keys above S and S: determined bits >= the prefix
  {
    const u64 prefix = s.prefix, det = s.det;
    for_keys([&](u64 k) {
      if ((k & det) >= prefix) {
        const unsigned at = atomicAdd(&s.nc, 1u);
        if (at < CAND) s.cand[at] = k;
      }
    });
  }
  __syncthreads();
  const unsigned nc = min(s.nc, (unsigned)CAND);
  unsigned n2 = 1;
  while (n2 < nc) n2 <<= 1;
  for (unsigned i = nc + tid; i < n2; i += THREADS) s.cand[i] = 0;
  __syncthreads();
  // bitonic sort, descending; every thread takes its pairs of a step:
  // n2 <= CAND, so PAIRS trips cover them (one at CAND <= 2 * THREADS)
  constexpr unsigned PAIRS = (CAND / 2 + THREADS - 1) / THREADS;
  for (unsigned size = 2; size <= n2; size <<= 1) {
    for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
      for (unsigned u = 0; u < PAIRS; ++u) {
        const unsigned t = (unsigned)tid + u * THREADS;
        if (t >= (n2 >> 1)) break;
        const unsigned lo = 2 * t - (t & (stride - 1));
        const unsigned hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const u64 a = s.cand[lo], c = s.cand[hi];
        if (desc ? a < c : a > c) {
          s.cand[lo] = c;
          s.cand[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  return nc;
}
