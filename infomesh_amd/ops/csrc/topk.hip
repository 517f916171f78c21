// Per-row top-k selection over [B, N] f32 score arrays (N up to tens of
// millions, K <= 1024) via radix select (2 byte levels, 4 on rows that
// need them) + compaction + one-block bitonic sort. Replaces: ChromaDB
// HNSW top-k (reference infomesh/index/vector_store.py:216-220) and the
// FTS5 ORDER BY bm25() LIMIT path (index/local_store.py:316-332) on the
// GPU shards.
//
// Passes, one launch each (3 streaming reads of the score array, 2 when
// the producer supplies the pass-1 histogram):
//   1. hist1: 256-bin histogram of ordered-float top byte (LDS-staged);
//      skipped when the caller passes ext_hist1.
//   2. select1: find byte bin containing the Kth value.
//   3. hist2: 256-bin histogram of byte 2 within that bin.
//   4. select2: 16-bit threshold prefix. A row where more candidates
//      share that prefix than the tie region of the candidate buffer
//      holds is refined in the same kernel, by its one workgroup: bytes
//      3 and 4 of the threshold, two more reads of that row alone,
//      giving a full 32-bit threshold.
//   5. compact: gather (value, idx) — strictly-above candidates into a
//      reserved region (provably < K of them), threshold-equal
//      candidates until the cap. On an unrefined row all of them fit;
//      on a refined row they equal the threshold in all 32 bits, so the
//      excess dropped at the cap is interchangeable at rank K.
//   6. sort: one block per row bitonic-sorts candidates, emits top-K.
//
// Exact for every row without NaN: the values returned are the K
// largest, ordered by value, equal values by ascending index (+0.0 and
// -0.0 count as equal there). Which of several EQUAL values at rank K
// are returned is arbitrary.
//
// Masked variant (infomesh_topk_masked): the kernels that read scores
// (hist1, hist2, select2's refinement, compact) are templated on MASKED
// and read a per-document pass bit (docfilter.hip's [P, W] bitmask,
// row b using mask row row_pred[b]). A failing document
// is absent: not histogrammed, not compacted; rows with fewer than K
// passing documents pad with -inf / -1. One u32 of mask covers one
// 128-byte line of scores, and the mask word is loaded first (one loop
// iteration ahead of the scores it guards), so a zero word skips the
// line.
//
// Pruned variant (infomesh_topk_pruned, at the end of the file): for a
// producer that also wrote the maximum of every block of W consecutive
// columns. The K blocks with the largest maxima hold the top K, so one
// kernel, one workgroup per row, selects over the NB maxima and then over
// the K chosen blocks, never over [B, N]: 19.5k + 6.4k elements per row
// at 1.25M columns, W = 64, K = 100, instead of 3 x 1.25M. Its contract
// is stronger: ties at rank K go to the lowest columns. The steps, the
// contract and the argument for it stand above infomesh_topk_pruned.
// At 128 rows (device events, 7 rounds of 10 uncaptured calls, median):
// streaming 372 us, the earlier sixteen-launch composition 130 us, this
// kernel 38 us at 1.25M columns; 2612 / 151 / 69 us at 10M
// (docs/performance.md).
#include "common.h"

#define TOPK_CAP 8192

// Candidate layout per row (TOPK_CAP slots):
//   [0, HI_RES)        strictly-above-threshold candidates. Fewer than
//                      K <= 1024 exist (see compact_kernel), so the
//                      reserve is generous; its size also fixes where
//                      the tie region starts, i.e. how many ties
//                      survive and how large the sort gets on tied rows.
//   [HI_RES, TOPK_CAP) threshold-equal candidates, kept until the
//                      region fills. Where more candidates share the
//                      16-bit threshold prefix than fit here, the
//                      row's threshold is refined to all 32 bits
//                      (select2_kernel), and only candidates EQUAL to it
//                      land here. Those are interchangeable at rank K
//                      (any K of them is a valid top-k), so DROPPING
//                      the excess is sound: massively tied planes (BM25
//                      over tiny-vocab corpora) do not overflow.
//                      Candidates that share a prefix and differ below
//                      it are never dropped; the final bitonic sorts
//                      them by the full 32-bit ordered value.
#define HI_RES 4096

namespace {

// The masked kernels' extra argument. The streaming kernels take it as
// a parameter pack that is empty when !MASKED, so the unmasked
// instantiations keep the exact signature (and kernarg layout, hence
// code) they had before the mask existed.
struct MaskRef {
  const unsigned* bits;  // [P, W] u32, docfilter.hip
  const int* row_pred;   // [B] mask row of each batch row
  long W;
};
// Mask row of batch row b.
DEVINL const unsigned* mask_row(const MaskRef& m, int b) {
  return m.bits + (long)m.row_pred[b] * m.W;
}
// The 4 pass bits of columns 4i..4i+3: they never straddle a word.
DEVINL unsigned mask_nibble(const unsigned* __restrict__ mrow, long i) {
  return (mrow[i >> 3] >> ((unsigned)(i & 7) * 4)) & 15u;
}
// Pin a loaded float4 in registers: without it the compiler sinks the
// component loads into the per-bit branches of the masked loops,
// splitting one dwordx4 load into dependent partial loads with a wait
// each (measured: 0.46 -> 0.42 ms at 128 x 1.25M, all-pass mask).
DEVINL void keep_loaded(float4& v) {
  asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
}
DEVINL bool mask_bit(const unsigned* __restrict__ mrow, long col) {
  return (mrow[col >> 5] >> (unsigned)(col & 31)) & 1u;
}

// Walk a row's passing columns: f4(v, m, i) for every float4 group i
// whose pass nibble m is non-zero, then f1(value, col) for the passing
// columns of the scalar tail. The mask word is loaded before the scores
// it guards — one iteration ahead, so its latency hides behind the
// current group's score load instead of preceding it (0.42 -> 0.38 ms,
// unmasked 0.37) — and a zero nibble skips the score load.
template <typename F4, typename F1>
DEVINL void masked_stream(const float* __restrict__ row,
                          const unsigned* __restrict__ mrow, long N,
                          long start, long step, F4 f4, F1 f1) {
  const long n4 = N / 4;
  if (start < n4) {
    unsigned m = mask_nibble(mrow, start);
    for (long i = start; i < n4; i += step) {
      // clamped, so the prefetch needs no branch (the last one is unused)
      const unsigned mn = mask_nibble(mrow, min(i + step, n4 - 1));
      if (m != 0) {
        float4 v = reinterpret_cast<const float4*>(row)[i];
        keep_loaded(v);
        f4(v, m, i);
      }
      m = mn;
    }
  }
  for (long i = n4 * 4 + start; i < N; i += step)
    if (mask_bit(mrow, i)) f1(row[i], i);
}

template <bool MASKED, typename... M>
__global__ __launch_bounds__(256) void hist1_kernel(
    const float* __restrict__ scores, unsigned* __restrict__ hist,
    long N, M... mask) {
  __shared__ unsigned lh[HIST8_U32];
  const int b = blockIdx.y;
  hist8_zero(lh);
  __syncthreads();
  unsigned* my = hist8_mine(lh);
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long step = (long)gridDim.x * blockDim.x;
  const float* row = scores + (long)b * N;
  const long n4 = N / 4;
  if constexpr (MASKED) {
    auto count = [&](float f) {
      atomicAdd(&my[float_to_ordered(f) >> 24], 1u);
    };
    masked_stream(
        row, mask_row(mask..., b), N, start, step,
        [&](float4 v, unsigned m, long) {
          if (m & 1) count(v.x);
          if (m & 2) count(v.y);
          if (m & 4) count(v.z);
          if (m & 8) count(v.w);
        },
        [&](float f, long) { count(f); });
  } else {
    for (long i = start; i < n4; i += step) {
      const float4 v = reinterpret_cast<const float4*>(row)[i];
      atomicAdd(&my[float_to_ordered(v.x) >> 24], 1u);
      atomicAdd(&my[float_to_ordered(v.y) >> 24], 1u);
      atomicAdd(&my[float_to_ordered(v.z) >> 24], 1u);
      atomicAdd(&my[float_to_ordered(v.w) >> 24], 1u);
    }
    for (long i = n4 * 4 + start; i < N; i += step)
      atomicAdd(&my[float_to_ordered(row[i]) >> 24], 1u);
  }
  __syncthreads();
  hist8_merge(lh, hist + (long)b * 256);
}

// Scan a 256-bin histogram from the top: the highest bin at which the
// running count (starting at `cum`) reaches K, or bin 0 when it never
// does (N < K). On return `cum` is the count strictly above that bin.
DEVINL unsigned select_bin(const unsigned* __restrict__ h, unsigned& cum,
                           int K) {
  for (int i = 255;; --i) {
    const unsigned c = h[i];
    if (cum + c >= (unsigned)K || i == 0) return (unsigned)i;
    cum += c;
  }
}

__global__ void select1_kernel(const unsigned* __restrict__ hist,
                               unsigned* __restrict__ bin1,
                               unsigned* __restrict__ chi1, int K) {
  const int b = blockIdx.x;
  if (threadIdx.x != 0) return;
  unsigned cum = 0;
  bin1[b] = select_bin(hist + (long)b * 256, cum, K);
  chi1[b] = cum;
}

// count(value) for every (passing) column of batch row b, the columns
// dealt to threads from `start` in steps of `step`.
template <bool MASKED, typename F, typename... M>
DEVINL void for_each_score(const float* __restrict__ row, long N, int b,
                           long start, long step, F count, M... mask) {
  if constexpr (MASKED) {
    masked_stream(
        row, mask_row(mask..., b), N, start, step,
        [&](float4 v, unsigned m, long) {
          if (m & 1) count(v.x);
          if (m & 2) count(v.y);
          if (m & 4) count(v.z);
          if (m & 8) count(v.w);
        },
        [&](float f, long) { count(f); });
  } else {
    const long n4 = N / 4;
    for (long i = start; i < n4; i += step) {
      const float4 v = reinterpret_cast<const float4*>(row)[i];
      count(v.x); count(v.y); count(v.z); count(v.w);
    }
    for (long i = n4 * 4 + start; i < N; i += step) count(row[i]);
  }
}

template <bool MASKED, typename... M>
__global__ __launch_bounds__(256) void hist2_kernel(
    const float* __restrict__ scores, const unsigned* __restrict__ bin1,
    unsigned* __restrict__ hist2, long N, M... mask) {
  __shared__ unsigned lh[256];
  const int b = blockIdx.y;
  const unsigned b1 = bin1[b];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) lh[i] = 0;
  __syncthreads();
  for_each_score<MASKED>(
      scores + (long)b * N, N, b,
      (long)blockIdx.x * blockDim.x + threadIdx.x,
      (long)gridDim.x * blockDim.x,
      [&](float f) {
        const unsigned o = float_to_ordered(f);
        if ((o >> 24) == b1) atomicAdd(&lh[(o >> 16) & 255], 1u);
      },
      mask...);
  __syncthreads();
  for (int i = threadIdx.x; i < 256; i += blockDim.x)
    if (lh[i]) atomicAdd(&hist2[(long)b * 256 + i], lh[i]);
}

// One workgroup per row. Thread 0 finds the 16-bit threshold prefix.
// If every candidate sharing that prefix fits the tie region of the
// candidate buffer (all but degenerate rows), that is the row's
// threshold, shift[b] = 16 tells compact_kernel to compare the top 16
// bits, and the workgroup is done.
// Otherwise compact_kernel would have to drop candidates that differ
// below the prefix, so the workgroup refines the threshold to all 32
// bits here (shift[b] = 0): for bytes 3 and 4 in turn it streams the
// row, histograms that byte among the values matching the prefix so
// far, and extends the prefix by the bin holding the Kth value. Two
// more reads of the row by ONE workgroup: slow next to the grid-wide
// passes (a single CU's bandwidth), but it costs the rows that need no
// refinement nothing, not even a launch.
#define SELECT2_THREADS 1024
template <bool MASKED, typename... M>
__global__ __launch_bounds__(SELECT2_THREADS) void select2_kernel(
    const float* __restrict__ scores, const unsigned* __restrict__ hist2,
    const unsigned* __restrict__ bin1, const unsigned* __restrict__ chi1,
    unsigned* __restrict__ thresh, unsigned* __restrict__ shift, long N,
    int K, M... mask) {
  __shared__ unsigned lh[256];
  __shared__ unsigned s_pre, s_cum, s_refine;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) {
    const unsigned* h = hist2 + (long)b * 256;
    unsigned cum = chi1[b];
    const unsigned bin = select_bin(h, cum, K);
    s_pre = (bin1[b] << 8) | bin;
    s_cum = cum;
    s_refine = h[bin] > TOPK_CAP - HI_RES;
  }
  __syncthreads();
  if (!s_refine) {
    if (threadIdx.x == 0) { thresh[b] = s_pre; shift[b] = 16; }
    return;
  }
  for (int sh = 8; sh >= 0; sh -= 8) {
    const unsigned pre = s_pre;
    for (int i = threadIdx.x; i < 256; i += blockDim.x) lh[i] = 0;
    __syncthreads();
    for_each_score<MASKED>(
        scores + (long)b * N, N, b, (long)threadIdx.x, (long)blockDim.x,
        [&](float f) {
          const unsigned o = float_to_ordered(f);
          if ((o >> sh >> 8) == pre) atomicAdd(&lh[(o >> sh) & 255], 1u);
        },
        mask...);
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned cum = s_cum;
      s_pre = (pre << 8) | select_bin(lh, cum, K);
      s_cum = cum;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { thresh[b] = s_pre; shift[b] = 0; }
}

// The `pos < HI_RES` guard never trips here: every select level picks
// the highest bin at which the cumulative count reaches K, so the count
// strictly above the threshold is below K <= 1024 < HI_RES, and the
// bin-0 fall-through (N < K) counts fewer still. The tie-region guard
// trips only on a refined row, whose threshold has all 32 bits. Both
// guards stay as the memory-safety bound, also against a wrong producer
// histogram.
// MASKED: the argument holds as is, over the passing documents alone —
// the histograms counted exactly the documents this kernel emits.
template <bool MASKED, typename... M>
__global__ __launch_bounds__(256) void compact_kernel(
    const float* __restrict__ scores, const unsigned* __restrict__ thresh,
    const unsigned* __restrict__ shift,
    unsigned long long* __restrict__ cand, unsigned* __restrict__ cnt,
    unsigned* __restrict__ cnt_eq, long N, M... mask) {
  const int b = blockIdx.y;
  // the row's threshold: the top 16 bits (sh = 16), or all 32 (sh = 0)
  const unsigned t = thresh[b], sh = shift[b];
  const long start = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long step = (long)gridDim.x * blockDim.x;
  const float* row = scores + (long)b * N;
  unsigned long long* crow = cand + (long)b * TOPK_CAP;
  const long n4 = N / 4;
  auto emit = [&](float f, unsigned idx) {
    const unsigned o = float_to_ordered(f);
    const unsigned p = o >> sh;
    // Ascending sort key: ~ordered in high bits (desc value),
    // raw idx in low bits (ties -> smaller idx first).
    const unsigned long long key = ((unsigned long long)(~o) << 32) | idx;
    if (p > t) {
      const unsigned pos = atomicAdd(&cnt[b], 1u);
      if (pos < HI_RES) crow[pos] = key;
    } else if (p == t) {
      const unsigned pos = atomicAdd(&cnt_eq[b], 1u);
      if (pos < TOPK_CAP - HI_RES) crow[HI_RES + pos] = key;
    }
  };
  if constexpr (MASKED) {
    masked_stream(
        row, mask_row(mask..., b), N, start, step,
        [&](float4 v, unsigned m, long i) {
          const unsigned i4 = (unsigned)(i * 4);
          if (m & 1) emit(v.x, i4);
          if (m & 2) emit(v.y, i4 + 1);
          if (m & 4) emit(v.z, i4 + 2);
          if (m & 8) emit(v.w, i4 + 3);
        },
        [&](float f, long i) { emit(f, (unsigned)i); });
  } else {
    for (long i = start; i < n4; i += step) {
      const float4 v = reinterpret_cast<const float4*>(row)[i];
      const unsigned i4 = (unsigned)(i * 4);
      emit(v.x, i4); emit(v.y, i4 + 1); emit(v.z, i4 + 2); emit(v.w, i4 + 3);
    }
    for (long i = n4 * 4 + start; i < N; i += step) emit(row[i], (unsigned)i);
  }
}

__global__ __launch_bounds__(256) void sort_emit_kernel(
    unsigned long long* __restrict__ cand, const unsigned* __restrict__ cnt,
    const unsigned* __restrict__ cnt_eq,
    float* __restrict__ out_vals, int* __restrict__ out_idx, int K) {
  __shared__ unsigned long long d[TOPK_CAP];
  const int b = blockIdx.x;
  const int nhi = min(cnt[b], (unsigned)HI_RES);
  const int neq = min(cnt_eq[b], (unsigned)(TOPK_CAP - HI_RES));
  const int n = nhi + neq;
  // Bitonic network size: next pow2 of the actual candidate count —
  // typical rows carry ~K+epsilon candidates, so this cuts the sort
  // from CAP=8192 to 128/256 most of the time.
  int n2 = 64;
  while (n2 < n) n2 <<= 1;
  const unsigned long long* crow = cand + (long)b * TOPK_CAP;
  for (int i = threadIdx.x; i < n2; i += blockDim.x) {
    unsigned long long key = (i < nhi) ? crow[i]
                           : (i < n) ? crow[HI_RES + (i - nhi)]
                           : ~0ULL;  // pad = worst
    // -0.0 (high key word 0x80000000) takes +0.0's (0x7fffffff): the
    // two compare equal, so they order by index among themselves, and
    // the value emitted for either is +0.0. On purpose only here:
    // select and compact still rank -0.0 strictly below +0.0, which
    // only decides WHICH of the equal zeros are returned at rank K, and
    // that is arbitrary anyway.
    if ((unsigned)(key >> 32) == 0x80000000u) key -= 1ULL << 32;
    d[i] = key;
  }
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n2; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const bool up = ((i & k) == 0);
          const unsigned long long a = d[i], c = d[ixj];
          if ((a > c) == up) { d[i] = c; d[ixj] = a; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < K; i += blockDim.x) {
    if (i < n) {
      const unsigned long long v = d[i];
      out_vals[(long)b * K + i] = ordered_to_float(~(unsigned)(v >> 32));
      out_idx[(long)b * K + i] = (int)(v & 0xffffffffu);
    } else {
      out_vals[(long)b * K + i] = -INFINITY;
      out_idx[(long)b * K + i] = -1;
    }
  }
}

// Workspace layout, offsets in u32 units. The caller zeroes [0, cand)
// before every call (hist1, hist2, cnt and cnt_eq accumulate by atomics;
// the four select outputs ride along in the same fill).
struct TopkLayout {
  long hist1, hist2, bin1, chi1, thresh, shift, cnt, cnt_eq, cand, total;
  explicit TopkLayout(long B)
      : hist1(0), hist2(hist1 + B * 256), bin1(hist2 + B * 256),
        chi1(bin1 + B), thresh(chi1 + B), shift(thresh + B),
        cnt(shift + B), cnt_eq(cnt + B),
        cand((cnt_eq + B + 1) & ~1L),  // u64 candidates: 8-byte aligned
        total(cand + B * TOPK_CAP * 2) {}
};
// The candidate buffer of a whole workspace.
unsigned long long* cand_of(unsigned* ws, long B) {
  return reinterpret_cast<unsigned long long*>(ws + TopkLayout(B).cand);
}

// ---- pruned select from block maxima (infomesh_topk_pruned) ------------
// row_select_kernel, one workgroup of ROW_THREADS per row, everything in
// LDS, no global workspace. The steps are the ones listed above
// infomesh_topk_pruned; the pieces they share:
//
// Keys. Both levels rank by row_key: float_to_ordered with -0.0 folded
// onto +0.0, so the two zeros tie (and order by column) already in the
// selection, not only in the emitted order. A block maximum taken in
// float_to_ordered order maps to the maximum of its scores' keys, the
// fold being monotone. Key 0 is below -inf's and marks the columns >= N
// of the row's last block: no real score loses its place to padding.
//
// ROW_STAGE keys of LDS hold the row of maxima while the blocks are
// chosen, then the chosen blocks' scores. Scores that do not fit
// (K = 1024 at W = 64) are read from global memory in every pass.
// Maxima that do not fit (past 1.57M columns at W = 64) get one more
// level instead, because six passes of one workgroup over a 625 KB row
// measured 381 us at 128 x 10M: group_max_kernel, grid-wide, writes the
// maximum of every G consecutive block maxima (G = ceil(NB / ROW_STAGE))
// to the workspace, the row kernel chooses K1 of those groups by the same
// rule and then K1 blocks among their K1 * G children. That is the
// contract of this very selector applied to the maxima as scores with
// block width G, so the K1 blocks are the ones the direct choice takes.
// K1 * G must fit the stage too: G <= ROW_GROUP_MAX, 37.7M columns at
// W = 64.
#define ROW_THREADS 1024
#define ROW_WAVES (ROW_THREADS / WAVE)
#define ROW_STAGE 24576
// Keys a thread loads before it uses the first: a level read from global
// memory by one workgroup lives on the loads it keeps in flight.
#define ROW_U_LDS 4
#define ROW_U_MEM 16
#define ROW_GROUP_MAX (ROW_STAGE / 1024)

DEVINL unsigned row_key(float f) {
  const unsigned o = float_to_ordered(f);
  return o == 0x7fffffffu ? 0x80000000u : o;   // -0.0 -> +0.0
}

struct RowLds {
  unsigned stage[ROW_STAGE];       // staged keys of the current level
  unsigned hist[HIST8_U32];        // padded histogram copies (common.h)
  unsigned bins[256];              // the copies summed
  unsigned wave_gt[ROW_WAVES], wave_eq[ROW_WAVES];
  unsigned sel_bin, sel_cum;
  int blk[1024];                   // chosen block ids, ascending
  int grp[1024];                   // chosen groups of G blocks, ascending
  unsigned long long sort[1024];   // survivors: ~key << 32 | column
};

// This lane's rank among the set bits of a wave ballot.
DEVINL unsigned lane_rank(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                   __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
}

// The Kth largest of key_at(0 .. n-1), all 32 bits of it, one byte per
// pass from the top: histogram the byte among the keys that match the
// prefix so far, then wave 0 scans the 256 bins from the top (4 bins a
// lane, a shuffle prefix sum across lanes) for the bin where the running
// count reaches K. Returns the key; `above` is the count strictly above
// it. With fewer than K keys every pass falls through to bin 0, as
// select_bin does. All threads of the workgroup call it.
template <int U, typename KeyAt>
DEVINL unsigned row_radix_select(RowLds& l, long n, unsigned K,
                                 unsigned& above, KeyAt key_at) {
  const int lane = threadIdx.x & (WAVE - 1);
  unsigned prefix = 0, cum = 0;
  for (int sh = 24; sh >= 0; sh -= 8) {
    hist8_zero(l.hist);
    __syncthreads();
    unsigned* my = hist8_mine(l.hist);
    for (long base = threadIdx.x; base < n; base += ROW_THREADS * U) {
      unsigned o[U];   // all U loads in flight before the first use
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long i = base + (long)u * ROW_THREADS;
        o[u] = i < n ? key_at(i) : 0u;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // (o >> sh >> 8): the bytes above this one; sh + 8 may be 32
        if (base + (long)u * ROW_THREADS < n &&
            (sh == 24 || (o[u] >> sh >> 8) == prefix))
          atomicAdd(&my[(o[u] >> sh) & 255], 1u);
      }
    }
    __syncthreads();
    if (threadIdx.x < 256) {
      unsigned sum = 0;
#pragma unroll
      for (int c = 0; c < HIST8_COPIES; ++c)
        sum += l.hist[c * HIST8_STRIDE + threadIdx.x];
      l.bins[threadIdx.x] = sum;
    }
    __syncthreads();
    if (threadIdx.x < WAVE) {
      // lane L owns bins 255 - 4L .. 252 - 4L, highest first
      unsigned c[4], tot = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        c[j] = l.bins[255 - 4 * lane - j];
        tot += c[j];
      }
      unsigned inc = tot;   // inclusive prefix sum over lanes
#pragma unroll
      for (int off = 1; off < WAVE; off <<= 1) {
        const unsigned v = __shfl_up(inc, off, WAVE);
        if (lane >= off) inc += v;
      }
      unsigned run = cum + inc - tot;   // count above this lane's bins
      int hit = -1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (hit < 0) {
          if (run + c[j] >= K) hit = j; else run += c[j];
        }
      }
      const unsigned long long found = __ballot(hit >= 0);
      if (found == 0) {
        // never reaches K: bin 0, everything above it counted
        if (lane == WAVE - 1) { l.sel_bin = 0; l.sel_cum = run - c[3]; }
      } else if (lane == __ffsll((long long)found) - 1) {
        l.sel_bin = 255 - 4 * lane - hit;
        l.sel_cum = run;
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | l.sel_bin;
    cum = l.sel_cum;
  }
  above = cum;
  return prefix;
}

// Ordered compaction: of key_at(0 .. n-1), every key > t and the first
// `need_eq` keys == t, in ascending i. take(i, key, pos) runs once for
// each, pos being its rank among the taken, so positions ascend with i.
// Wave w owns one contiguous range and walks it 64 keys at a time, ranks
// from ballots: once to count, then, after a prefix over the waves, to
// place. A racing counter would give neither the first ties nor the
// order. All threads of the workgroup call it.
template <int U, typename KeyAt, typename Take>
DEVINL void row_ordered_take(RowLds& l, long n, unsigned t, unsigned need_eq,
                             KeyAt key_at, Take take) {
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const long per =   // keys per wave, a multiple of 64
      ((n + ROW_WAVES - 1) / ROW_WAVES + WAVE - 1) & ~(long)(WAVE - 1);
  const long lo = min(w * per, n), hi = min(lo + per, n);
  unsigned ng = 0, ne = 0;
  for (long base = lo; base < hi; base += WAVE * U) {
    unsigned o[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = base + u * WAVE + lane;
      o[u] = i < hi ? key_at(i) : 0u;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool in = base + u * WAVE + lane < hi;
      ng += __popcll(__ballot(in && o[u] > t));
      ne += __popcll(__ballot(in && o[u] == t));
    }
  }
  if (lane == 0) { l.wave_gt[w] = ng; l.wave_eq[w] = ne; }
  __syncthreads();
  unsigned og = 0, oe = 0;   // taken / tied keys before this wave's range
  for (int v = 0; v < w; ++v) { og += l.wave_gt[v]; oe += l.wave_eq[v]; }
  for (long base = lo; base < hi; base += WAVE * U) {
    unsigned o[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = base + u * WAVE + lane;
      o[u] = i < hi ? key_at(i) : 0u;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = base + u * WAVE + lane;
      const bool gt = i < hi && o[u] > t, eq = i < hi && o[u] == t;
      const unsigned long long mg = __ballot(gt), me = __ballot(eq);
      const unsigned rg = og + lane_rank(mg), re = oe + lane_rank(me);
      if (gt || (eq && re < need_eq)) take(i, o[u], rg + min(re, need_eq));
      og += __popcll(mg);
      oe += __popcll(me);
    }
  }
  __syncthreads();
}

// gmax[b][j] = the maximum, in row_key order, of bmax[b][j*G .. j*G+G-1]
// (the blocks < NB of the last group).
__global__ __launch_bounds__(256) void group_max_kernel(
    const float* __restrict__ bmax, float* __restrict__ gmax, long NB,
    long NG, int G) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= NG) return;
  const float* __restrict__ mrow = bmax + (long)blockIdx.y * NB;
  unsigned m = 0;
  for (long i = j * G; i < min(j * G + G, NB); ++i)
    m = max(m, row_key(mrow[i]));
  gmax[(long)blockIdx.y * NG + j] = ordered_to_float(m);
}

// gmax, NG, G: the group maxima, their count per row and the group size
// when NB > ROW_STAGE; otherwise G = 1 and they are not read.
__global__ __launch_bounds__(ROW_THREADS) void row_select_kernel(
    const float* __restrict__ scores, const float* __restrict__ bmax,
    const float* __restrict__ gmax, float* __restrict__ out_vals,
    int* __restrict__ out_idx, long N, long NB, long NG, unsigned G,
    unsigned W, int K1, int K) {
  __shared__ RowLds l;
  const int b = blockIdx.x;
  const float* __restrict__ mrow = bmax + (long)b * NB;
  const float* __restrict__ row = scores + (long)b * N;

  // 1. threshold of the maxima and the K1 blocks, ids ascending.
  // A row without NaN fills blk[0 .. K1); whatever a row fills, every
  // entry is a block of the row.
  for (int i = threadIdx.x; i < 1024; i += ROW_THREADS) l.blk[i] = 0;
  unsigned above, t;
  auto take_block = [&](long i, unsigned, unsigned pos) {
    if (pos < (unsigned)K1) l.blk[pos] = (int)i;   // always: memory bound
  };
  auto key_at = [&](long i) { return l.stage[i]; };
  if (G == 1) {   // host: NB <= ROW_STAGE
    for (long i = threadIdx.x; i < NB; i += ROW_THREADS)
      l.stage[i] = row_key(mrow[i]);
    t = row_radix_select<ROW_U_LDS>(l, NB, (unsigned)K1, above, key_at);
    row_ordered_take<ROW_U_LDS>(l, NB, t, (unsigned)K1 - above, key_at,
                                take_block);
  } else {        // host: NG <= ROW_STAGE, G <= ROW_GROUP_MAX
    const float* __restrict__ grow = gmax + (long)b * NG;
    const unsigned KG = (unsigned)min((long)K1, NG);
    for (int i = threadIdx.x; i < 1024; i += ROW_THREADS) l.grp[i] = 0;
    for (long i = threadIdx.x; i < NG; i += ROW_THREADS)
      l.stage[i] = row_key(grow[i]);
    t = row_radix_select<ROW_U_LDS>(l, NG, KG, above, key_at);
    row_ordered_take<ROW_U_LDS>(
        l, NG, t, KG - above, key_at, [&](long i, unsigned, unsigned pos) {
          if (pos < KG) l.grp[pos] = (int)i;
        });
    // the chosen groups' blocks, in id order; key 0 past the row's end
    const unsigned n1 = KG * G;
    auto blk_of = [&](unsigned e) { return (long)l.grp[e / G] * G + e % G; };
    for (unsigned e = threadIdx.x; e < n1; e += ROW_THREADS) {
      const long id = blk_of(e);
      l.stage[e] = id < NB ? row_key(mrow[id]) : 0u;
    }
    t = row_radix_select<ROW_U_LDS>(l, n1, (unsigned)K1, above, key_at);
    row_ordered_take<ROW_U_LDS>(
        l, n1, t, (unsigned)K1 - above, key_at,
        [&](long e, unsigned, unsigned pos) {
          const long id = blk_of((unsigned)e);
          if (pos < (unsigned)K1 && id < NB) l.blk[pos] = (int)id;
        });
  }

  // 2. threshold of the chosen blocks' scores and the survivors.
  // Position e of the K1 * W scores is column blk[e / W] * W + e % W;
  // the ids ascend, so e ascends with the column.
  const unsigned n2 = (unsigned)K1 * W;
  auto col_of = [&](unsigned e) { return (long)l.blk[e / W] * W + e % W; };
  auto take_score = [&](long e, unsigned o, unsigned pos) {
    const long col = col_of((unsigned)e);
    // a padding column is taken only where N < K; it is emitted as the
    // -inf / -1 every position past the survivors gets
    if (pos < (unsigned)K && col < N)
      l.sort[pos] = ((unsigned long long)(~o) << 32) | (unsigned)col;
  };
  for (int i = threadIdx.x; i < 1024; i += ROW_THREADS) l.sort[i] = ~0ULL;
  unsigned T;
  if (n2 <= ROW_STAGE) {
    for (unsigned e = threadIdx.x; e < n2; e += ROW_THREADS) {
      const long col = col_of(e);
      l.stage[e] = col < N ? row_key(row[col]) : 0u;
    }
    T = row_radix_select<ROW_U_LDS>(l, n2, (unsigned)K, above, key_at);
    row_ordered_take<ROW_U_LDS>(l, n2, T, (unsigned)K - above, key_at,
                                take_score);
  } else {
    auto mem_key_at = [&](long e) {
      const long col = col_of((unsigned)e);
      return col < N ? row_key(row[col]) : 0u;
    };
    T = row_radix_select<ROW_U_MEM>(l, n2, (unsigned)K, above, mem_key_at);
    row_ordered_take<ROW_U_MEM>(l, n2, T, (unsigned)K - above, mem_key_at,
                                take_score);
  }

  // 3. sort the survivors by (value descending, column ascending): the
  // empty slots hold the largest key and sort behind them
  int ns = 64;
  while (ns < K) ns <<= 1;
  for (int k = 2; k <= ns; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int i = threadIdx.x, ixj = i ^ j;
      if (i < ns && ixj > i) {
        const bool up = ((i & k) == 0);
        const unsigned long long a = l.sort[i], c = l.sort[ixj];
        if ((a > c) == up) { l.sort[i] = c; l.sort[ixj] = a; }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < K; i += ROW_THREADS) {
    const unsigned long long v = l.sort[i];
    const bool real = v != ~0ULL;
    out_vals[(long)b * K + i] =
        real ? ordered_to_float(~(unsigned)(v >> 32)) : -INFINITY;
    out_idx[(long)b * K + i] = real ? (int)(v & 0xffffffffu) : -1;
  }
}

// Blocks per group of group_max_kernel: 1 = the maxima fit the stage.
long row_group(long NB) {
  return NB <= ROW_STAGE ? 1 : (NB + ROW_STAGE - 1) / ROW_STAGE;
}

}  // namespace

extern "C" long infomesh_topk_workspace_u32(int B) {
  return TopkLayout(B).total;
}

// Length of the workspace prefix to zero before each infomesh_topk call.
extern "C" long infomesh_topk_zero_u32(int B) { return TopkLayout(B).cand; }

// Shared launcher: mask is one MaskRef for the masked entry, nothing for
// the unmasked one. ws is the zeroed prefix [0, L.cand) of a workspace,
// cand its candidate buffer (infomesh_topk_pruned keeps the two apart).
template <bool MASKED, typename... M>
static void topk_launch(const void* scores, unsigned* ws,
                        unsigned long long* cand, void* out_vals,
                        void* out_idx, int B, long N, int K,
                        const void* ext_hist1, hipStream_t s, M... mask) {
  static_assert(sizeof...(M) == (MASKED ? 1 : 0), "one MaskRef iff MASKED");
  const TopkLayout L(B);

  int chunks = (int)min((N + 256 * 64 - 1) / (256 * 64), (long)1024);
  if (chunks < 1) chunks = 1;
  dim3 g1(chunks, B), blk(256);
  const unsigned* h1 = (const unsigned*)ext_hist1;  // producer-fused pass 1
  if (!h1) {
    h1 = ws + L.hist1;
    hipLaunchKernelGGL((hist1_kernel<MASKED, M...>), g1, blk, 0, s,
                       (const float*)scores, ws + L.hist1, N, mask...);
  }
  hipLaunchKernelGGL(select1_kernel, dim3(B), dim3(64), 0, s,
                     h1, ws + L.bin1, ws + L.chi1, K);
  hipLaunchKernelGGL((hist2_kernel<MASKED, M...>), g1, blk, 0, s,
                     (const float*)scores, ws + L.bin1, ws + L.hist2, N,
                     mask...);
  hipLaunchKernelGGL((select2_kernel<MASKED, M...>), dim3(B),
                     dim3(SELECT2_THREADS), 0, s, (const float*)scores,
                     ws + L.hist2, ws + L.bin1, ws + L.chi1, ws + L.thresh,
                     ws + L.shift, N, K, mask...);
  hipLaunchKernelGGL((compact_kernel<MASKED, M...>), g1, blk, 0, s,
                     (const float*)scores, ws + L.thresh, ws + L.shift, cand,
                     ws + L.cnt, ws + L.cnt_eq, N, mask...);
  hipLaunchKernelGGL(sort_emit_kernel, dim3(B), blk, 0, s,
                     cand, ws + L.cnt, ws + L.cnt_eq, (float*)out_vals,
                     (int*)out_idx, K);
}

// ext_hist1: non-null = a producer-fused [B*256] top-byte histogram of
// the FULL score rows (exact counts, zeros included); pass 1 is skipped
// and select1 reads it directly.
extern "C" void infomesh_topk(const void* scores, void* workspace,
                              void* out_vals, void* out_idx,
                              int B, long N, int K,
                              const void* ext_hist1, void* stream) {
  unsigned* ws = reinterpret_cast<unsigned*>(workspace);
  topk_launch<false>(scores, ws, cand_of(ws, B), out_vals, out_idx, B, N, K,
                     ext_hist1, reinterpret_cast<hipStream_t>(stream));
}

// Top-k over the documents whose bit is set: bits [P, W] u32 with
// W >= ceil(N/32) (docfilter.hip writes W = ceil(N/64)*2), row_pred [B]
// i32 in [0, P). No ext_hist1: a producer histogram counts failing
// documents too.
extern "C" void infomesh_topk_masked(const void* scores, void* workspace,
                                     void* out_vals, void* out_idx,
                                     int B, long N, int K,
                                     const void* bits, const void* row_pred,
                                     long W, void* stream) {
  unsigned* ws = reinterpret_cast<unsigned*>(workspace);
  topk_launch<true>(scores, ws, cand_of(ws, B), out_vals, out_idx, B, N, K,
                    nullptr, reinterpret_cast<hipStream_t>(stream),
                    MaskRef{(const unsigned*)bits, (const int*)row_pred, W});
}

// Top-k for a producer that also wrote bmax [B, NB = ceil(N / W)], the
// maximum of every block of W consecutive columns of a row (valid
// columns only in the last block), taken in float_to_ordered order
// (gemm.hip's BMAX tiles, bm25.hip's BMAX writeout). One launch of
// row_select_kernel, one workgroup per row; it reads NB maxima and
// K1 * W scores per row, never [B, N]. 1 <= K <= 1024, K * W < 2^31.
// No fill, and no workspace up to ROW_STAGE block maxima per row; past
// that group_max_kernel runs first and writes the workspace (see above
// row_select_kernel). Returns 0, or 1 with nothing launched when the row
// has more than ROW_GROUP_MAX * ROW_STAGE blocks.
//
// Per row, K1 = min(K, NB):
//   1. t = the K1-th largest maximum (row_radix_select, 32 bits).
//   2. Take every block whose maximum is > t and, of the blocks whose
//      maximum equals t, the lowest ids until K1 are taken
//      (row_ordered_take: the ids come out ascending).
//   3. T = the Kth largest of the K1 * W scores of those blocks, columns
//      >= N ranking below -inf.
//   4. Keep every score > T and, of the scores equal to T, the lowest
//      columns until K are kept.
//   5. Sort the K survivors by (value descending, column ascending) and
//      emit values and global columns; -inf / -1 past the N-th.
//
// Contract: for every row without NaN the output is exactly the first K
// of a stable descending sort of the row, -0.0 counting as equal to
// +0.0 (and emitted as +0.0). Stronger than infomesh_topk's, which
// leaves open which of several equal values at rank K it returns.
//
// Why taking blocks this way gives it. At least K1 blocks have a maximum
// >= t, each holding a score >= t, so (K1 = K; the case K1 = NB takes
// every block) T >= t. Fewer than K1 blocks have a maximum > t.
//   - A score > T >= t lies in a block whose maximum is > t: taken.
//   - If T > t, so does a score equal to T.
//   - If T = t, a block left out has maximum t and a higher id than every
//     taken block with maximum t. Each of those holds a score equal to T
//     at a lower column than anything in the block left out, and there
//     are K - (blocks with maximum > t) of them, while at most
//     K - (scores > T) <= K - (blocks with maximum > t) scores equal to
//     T are needed. So the lowest-column ties needed all lie in taken
//     blocks, and nothing in a block left out is among them.
// Hence steps 3-5 over the taken blocks see every element of the stable
// top K, and select exactly those.
//
// A row with NaN: no promise about the result; the kernel still ends
// and stays in bounds (every LDS and output position is range-checked,
// columns are checked against N).
extern "C" int infomesh_topk_pruned(const void* scores, const void* bmax,
                                    int W, void* workspace, void* out_vals,
                                    void* out_idx, int B, long N, int K,
                                    void* stream) {
  if (B <= 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long NB = (N + W - 1) / W;
  const int K1 = (int)(K < NB ? K : NB);
  const long G = row_group(NB), NG = (NB + G - 1) / G;
  if (G > ROW_GROUP_MAX) return 1;
  if (G > 1)
    hipLaunchKernelGGL(group_max_kernel, dim3((unsigned)((NG + 255) / 256), B),
                       dim3(256), 0, s, (const float*)bmax, (float*)workspace,
                       NB, NG, (int)G);
  hipLaunchKernelGGL(row_select_kernel, dim3(B), dim3(ROW_THREADS), 0, s,
                     (const float*)scores, (const float*)bmax,
                     (const float*)workspace, (float*)out_vals, (int*)out_idx,
                     N, NB, NG, (unsigned)G, (unsigned)W, K1, K);
  return 0;
}

// Workspace of infomesh_topk_pruned in u32 units: the group maxima of a
// row of more than ROW_STAGE block maxima, else nothing. Never filled.
extern "C" long infomesh_topk_pruned_workspace_u32(int B, long N, int K,
                                                   int W) {
  const long NB = (N + W - 1) / W, G = row_group(NB);
  return G > 1 ? (long)B * ((NB + G - 1) / G) : 0;
}
