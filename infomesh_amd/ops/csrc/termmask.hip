// Required and excluded query terms (+word / -word) -> pass bits for the
// masked top-k (topk.hip). Posting lists in, one bit per document out:
// the same [rows, W] bit rows docfilter.hip writes, so the selection does
// not care where a row's bits came from. Replaces on the GPU plane: FTS5
// `NOT` and the implicit AND of the reference's `MATCH`
// (infomesh/index/local_store.py search).
//
// THE layout (ops/kernels.py term_bitmask checks exactly this).
// An operand is a hashed BM25 term id with a kind: 0 = require (the term
// must occur in the document), 1 = exclude (it must not). A term row is a
// query row with at least one operand; there are R of them.
//   out       [R, W] u32, W = ceil(N/64)*2; bit d & 31 of word d >> 5 is
//             document d (docfilter.hip's layout). The caller fills row r
//             with the filter bits the row starts from; a launch only
//             CLEARS bits, and only of documents of its segment.
//   doc_ids   one posting segment's i32 ids, segment-local, ascending
//             inside every term's range (index/gpu_index.PostingSegment)
//   op_off    [R+1] i32, CSR: row r owns operands op_off[r] .. op_off[r+1];
//             at most TERM_OPS_MAX = 16 per row, both kinds together
//   op_begin  [T] i64 and
//   op_end    [T] i64: operand t's postings in THIS segment are
//             doc_ids[op_begin[t] .. op_end[t]); begin == end when the
//             segment lacks the term
//   op_kind   [T] i32, 0 = require, 1 = exclude
// One launch per segment, in stream order. A document keeps its bit iff
// every require operand of its row has a posting for it and no exclude
// operand has one. So a require term that is nowhere fails every document,
// and an id that is both required and excluded passes nothing.
//
// Grid (R, blocks): the GLOBAL document axis is cut into blocks of
// TERM_BLOCK documents at multiples of TERM_BLOCK, and a launch covers
// the blocks its segment [doc_base, doc_base + nseg) touches, each
// clipped to that range. TERM_BLOCK is a multiple of 32, so inside one
// launch every output word has exactly one owning workgroup and, in it,
// one owning lane: the writeback is a plain load / and / store, no global
// atomics. Segments start anywhere after appends, so a boundary word is
// touched by two launches; each clears only the bits of its own range and
// the stream orders them.
//
// TERM_BLOCK = 32768 documents: the two LDS bitmaps are 2 x 4 KB, so LDS
// never limits occupancy, while a workgroup's fixed work (the binary
// searches, up to 2 x 16 dependent chains of ~20 loads, and per require
// operand three barriers and a sweep of the bitmaps) is paid once per
// 32K documents. At B = 128 x 1.25M documents that is ~5k workgroups,
// about 20 per CU, enough to hide the searches' latency behind other
// workgroups. 8K-document blocks would quadruple the searches, and 8 KB
// of LDS is no limit to begin with; no other size was timed
// (docs/performance.md has the measured times).
#include "common.h"

#define TERM_BLOCK 32768
#define TERM_WORDS (TERM_BLOCK / 32)
#define TERM_OPS_MAX 16
#define TERM_THREADS 256

namespace {

// First index in [lo, hi) whose id is >= key (hi when none is).
__device__ __forceinline__ long lower_bound_ids(const int* __restrict__ ids,
                                                long lo, long hi, long key) {
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if ((long)ids[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(TERM_THREADS) void term_bitmask_kernel(
    const int* __restrict__ doc_ids, long npost,
    const int* __restrict__ op_off, const long* __restrict__ op_begin,
    const long* __restrict__ op_end, const int* __restrict__ op_kind, int T,
    unsigned* __restrict__ out, long W, long N, long doc_base, long nseg,
    long blk0) {
  __shared__ unsigned fail[TERM_WORDS];
  __shared__ unsigned seen[TERM_WORDS];
  __shared__ long s_edge[2 * TERM_OPS_MAX];  // [2t] first, [2t+1] past-last
  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const long g0 = (blk0 + blockIdx.y) * (long)TERM_BLOCK;  // block's doc 0
  // the block clipped to the segment (and to N, which the caller
  // guarantees anyway)
  const long lo = max(g0, doc_base);
  const long hi = min(min(g0 + TERM_BLOCK, doc_base + nseg), N);
  // the caller checks the table; the clamps keep a bad one inside the
  // arrays all the same
  const int o0 = min(max(op_off[r], 0), T);
  const int nops = min(min(max(op_off[r + 1] - o0, 0), TERM_OPS_MAX), T - o0);
  if (hi <= lo || nops == 0) return;  // block-uniform

  for (int w = tid; w < TERM_WORDS; w += TERM_THREADS) fail[w] = 0;
  // two lanes per operand, one per edge of its sub-range in this block
  if (tid < 2 * nops) {
    const int t = o0 + (tid >> 1);
    const long b = min(max(op_begin[t], 0L), npost);
    const long e = min(max(op_end[t], b), npost);
    const long key = ((tid & 1) ? hi : lo) - doc_base;  // segment-local
    s_edge[tid] = lower_bound_ids(doc_ids, b, e, key);
  }
  __syncthreads();

  const long loc0 = g0 - doc_base;  // segment-local id of the block's bit 0
  for (int j = 0; j < nops; ++j) {  // block-uniform trip count and kinds
    const long pb = s_edge[2 * j], pe = s_edge[2 * j + 1];
    if (op_kind[o0 + j] != 0) {
      // exclude: every posting fails its document
      for (long i = pb + tid; i < pe; i += TERM_THREADS) {
        const long d = (long)doc_ids[i] - loc0;
        if ((unsigned long)d < TERM_BLOCK)
          atomicOr(&fail[d >> 5], 1u << (d & 31));
      }
    } else {
      // require: every document WITHOUT a posting fails; an empty
      // sub-range therefore fails the whole block
      for (int w = tid; w < TERM_WORDS; w += TERM_THREADS) seen[w] = 0;
      __syncthreads();
      for (long i = pb + tid; i < pe; i += TERM_THREADS) {
        const long d = (long)doc_ids[i] - loc0;
        if ((unsigned long)d < TERM_BLOCK)
          atomicOr(&seen[d >> 5], 1u << (d & 31));
      }
      __syncthreads();  // also ends the atomics of earlier excludes
      for (int w = tid; w < TERM_WORDS; w += TERM_THREADS)
        fail[w] |= ~seen[w];
      __syncthreads();  // before a later exclude's atomics on fail
    }
  }
  __syncthreads();

  unsigned* row = out + (long)r * W;
  for (int w = tid; w < TERM_WORDS; w += TERM_THREADS) {
    const long gw = (g0 >> 5) + w;
    const long d0 = gw << 5;
    if (gw >= W || d0 + 32 <= lo || d0 >= hi) continue;
    const int a = (int)max(lo - d0, 0L), b = (int)min(hi - d0, 32L);
    const unsigned in_range =
        (b == 32 ? 0xffffffffu : (1u << b) - 1u) & ~((1u << a) - 1u);
    const unsigned f = fail[w] & in_range;
    if (f) row[gw] &= ~f;
  }
}

}  // namespace

// One segment's launch. The caller guarantees: out [R, W] holds the rows'
// base bits, 0 <= doc_base, doc_base + nseg <= N, op_off ascending inside
// [0, T] with at most 16 operands per row, every [begin, end) inside
// doc_ids[0 .. npost).
extern "C" void infomesh_term_bitmask(const void* doc_ids, long npost,
                                      const void* op_off,
                                      const void* op_begin,
                                      const void* op_end,
                                      const void* op_kind, int T, void* out,
                                      int R, long W, long N, long doc_base,
                                      long nseg, void* stream) {
  if (R <= 0 || T <= 0 || nseg <= 0 || N <= 0) return;
  auto s = reinterpret_cast<hipStream_t>(stream);
  const long blk0 = doc_base / TERM_BLOCK;
  const long nblk = (doc_base + nseg - 1) / TERM_BLOCK - blk0 + 1;
  hipLaunchKernelGGL(term_bitmask_kernel, dim3((unsigned)R, (unsigned)nblk),
                     dim3(TERM_THREADS), 0, s, (const int*)doc_ids, npost,
                     (const int*)op_off, (const long*)op_begin,
                     (const long*)op_end, (const int*)op_kind, T,
                     (unsigned*)out, W, N, doc_base, nseg, blk0);
}

extern "C" int infomesh_term_block_docs() { return TERM_BLOCK; }
