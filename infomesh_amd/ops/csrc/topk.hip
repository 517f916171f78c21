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
// columns. The K blocks with the largest maxima hold the top K, so the
// passes above run over the [B, NB] maxima and then over K gathered
// blocks per row, never over [B, N]: 19.5k + 6.4k elements per row at
// 1.25M columns, W = 64, K = 100, instead of 3 x 1.25M. Same contract.
// At 128 rows (device events, 7 rounds of 10 uncaptured calls, median):
// 372 -> 137 us at 1.25M columns, 2612 -> 163 us at 10M.
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
// gather_blocks_kernel, one workgroup per row: sort the row's K1 chosen
// block ids ascending (then position order in the gathered row IS global
// index order, which the tie rule needs), keep them in blk, and copy the
// K1 blocks of W scores side by side into gath [B, K1 * W]. Columns >= N
// of the row's last block take the bit pattern below: its ordered key is
// 0, under -inf's, so no real score ever loses its place to padding.
#define PRUNE_THREADS 1024
#define PRUNE_PAD 0xffffffffu
__global__ __launch_bounds__(PRUNE_THREADS) void gather_blocks_kernel(
    const float* __restrict__ scores, const int* __restrict__ ids,
    int* __restrict__ blk, float* __restrict__ gath, long N, long NB,
    int W, int K1) {
  __shared__ int d[1024];
  const int b = blockIdx.x;
  int n2 = 64;
  while (n2 < K1) n2 <<= 1;
  for (int i = threadIdx.x; i < n2; i += blockDim.x)
    d[i] = i < K1 ? ids[(long)b * K1 + i] : 0x7fffffff;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n2; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const bool up = ((i & k) == 0);
          const int a = d[i], c = d[ixj];
          if ((a > c) == up) { d[i] = c; d[ixj] = a; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < K1; i += blockDim.x)
    blk[(long)b * K1 + i] = d[i];
  const float* row = scores + (long)b * N;
  float* grow = gath + (long)b * K1 * W;
  for (int e = threadIdx.x; e < K1 * W; e += blockDim.x) {
    const long id = d[e / W];
    const long col = id * W + e % W;
    // id is a block of the row by construction (K1 <= NB, so the first
    // select pads nothing); the range check is the memory-safety bound
    grow[e] = (id >= 0 && id < NB && col < N) ? row[col]
                                              : __uint_as_float(PRUNE_PAD);
  }
}

// Positions in the gathered row -> global columns. A padding column
// (reached only when N < K) becomes the contract's -inf / -1.
__global__ __launch_bounds__(256) void remap_blocks_kernel(
    const int* __restrict__ blk, float* __restrict__ out_vals,
    int* __restrict__ out_idx, long N, int W, int K1, int K) {
  const int b = blockIdx.x;
  for (int i = threadIdx.x; i < K; i += blockDim.x) {
    const int p = out_idx[(long)b * K + i];
    if (p < 0) continue;
    const long col = (long)blk[(long)b * K1 + p / W] * W + p % W;
    if (col < N) {
      out_idx[(long)b * K + i] = (int)col;
    } else {
      out_vals[(long)b * K + i] = -INFINITY;
      out_idx[(long)b * K + i] = -1;
    }
  }
}

// Workspace of infomesh_topk_pruned, offsets in u32 units: the zeroed
// prefixes of its two selects first (one fill covers both), then the
// candidate buffer they share (the second select starts after the first
// has emitted), the first select's output and the gathered scores.
struct PrunedLayout {
  long K1, zero2, cand, vals1, idx1, blk, gath, total;
  PrunedLayout(long B, long NB, long K, long W)
      : K1(K < NB ? K : NB), zero2(TopkLayout(B).cand), cand(2 * zero2),
        vals1(cand + B * TOPK_CAP * 2), idx1(vals1 + B * K1),
        blk(idx1 + B * K1),
        gath((blk + B * K1 + 3) & ~3L),   // float4 reads: 16-byte aligned
        total(gath + B * K1 * W) {}
};

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

// Workspace length, and the prefix to zero before each call, of
// infomesh_topk_pruned. W > 0.
extern "C" long infomesh_topk_pruned_workspace_u32(int B, long N, int K,
                                                   int W) {
  return PrunedLayout(B, (N + W - 1) / W, K, W).total;
}
extern "C" long infomesh_topk_pruned_zero_u32(int B) {
  return 2 * TopkLayout(B).cand;
}

// infomesh_topk (same output contract) for a producer that also wrote
// bmax [B, NB = ceil(N / W)], the maximum of every block of W
// consecutive columns of a row (valid columns only in the last block),
// taken in float_to_ordered order (gemm.hip's BMAX tiles).
//
// Why it is exact: let t be a row's Kth largest block maximum. At least
// K scores are >= t (one per block), every score > t sits in a block
// whose maximum is > t, and fewer than K blocks have one. So the top K
// of the union of ANY K blocks with the largest maxima has the values of
// the true top K; scores equal to t in a block left out are
// interchangeable at rank K, which the contract leaves open.
//
// Steps: select the K1 = min(K, NB) largest maxima of each row; sort
// those block ids and gather the blocks (gather_blocks_kernel); select
// K among the K1 * W gathered scores; map positions back to columns.
// No pass over [B, N]: it reads NB + K1 * W scores per row.
extern "C" void infomesh_topk_pruned(const void* scores, const void* bmax,
                                     int W, void* workspace, void* out_vals,
                                     void* out_idx, int B, long N, int K,
                                     void* stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  unsigned* ws = reinterpret_cast<unsigned*>(workspace);
  const long NB = (N + W - 1) / W;
  const PrunedLayout L(B, NB, K, W);
  const int K1 = (int)L.K1;
  auto* cand = reinterpret_cast<unsigned long long*>(ws + L.cand);
  int* idx1 = reinterpret_cast<int*>(ws + L.idx1);
  int* blk = reinterpret_cast<int*>(ws + L.blk);
  float* gath = reinterpret_cast<float*>(ws + L.gath);
  topk_launch<false>(bmax, ws, cand, ws + L.vals1, idx1, B, NB, K1, nullptr,
                     s);
  hipLaunchKernelGGL(gather_blocks_kernel, dim3(B), dim3(PRUNE_THREADS), 0,
                     s, (const float*)scores, idx1, blk, gath, N, NB, W, K1);
  topk_launch<false>(gath, ws + L.zero2, cand, out_vals, out_idx, B,
                     (long)K1 * W, K, nullptr, s);
  hipLaunchKernelGGL(remap_blocks_kernel, dim3(B), dim3(256), 0, s, blk,
                     (float*)out_vals, (int*)out_idx, N, W, K1, K);
}
