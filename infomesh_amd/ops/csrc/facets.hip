// Facet counts and total matches over a query row's WHOLE match set: one
// streaming read of the [B, N] BM25 score matrix the top-k selects from
// (topk.hip), with the pass bits of docfilter.hip / termmask.hip and the
// 16-byte attribute records of docfilter.hip. Replaces: the reference's
// facet counts over the LIMITed hit list (infomesh/search/facets.py).
//
// The match rule. Document d matches row b iff it passes the row's mask
// (bit d of bits[row_pred[b]]; every document passes when there is no
// mask) and scores[b, d] > 0, i.e. it holds at least one query term:
// BM25 scores are exact zeros elsewhere. -0.0 and negative scores do not
// match; the rule is specified for normal floats only.
//
// THE slot layout (ops/kernels.py reads it through infomesh_facet_slot /
// infomesh_facet_width, nothing else knows it). counts is [R, F] i32,
// F = 5 + E + L + Dw: E date edges, L listed languages, Dw the widest
// domain list of the batch. With w0, w1, w2 the attribute words, every
// matching document adds 1 in exactly these places:
//   TOTAL      = 0
//   DATE_ZERO  = 1              when w0 == 0, otherwise
//   DATE0      = 2 .. 2 + E     DATE0 + #{j : edges[j] <= w0}, unsigned;
//                               edges ascending, E <= 7: E + 1 buckets
//   LANG_ZERO  = 3 + E          when c == 0, c = w1 & 0xFFFF, otherwise
//   LANG0      = 4 + E ..       LANG0 + i when c == langs[i] (ascending,
//                               unique, L <= 32), otherwise
//   LANG_OTHER = 4 + E + L
//   DOM0       = 5 + E + L ..   DOM0 + i when w2 == doms[off + i], the
//                               row's list (unique, ascending as unsigned,
//                               n <= 64); a domain not listed counts
//                               nowhere
// So TOTAL equals the sum of the date slots and the sum of the language
// slots, and every domain slot is <= TOTAL.
//
// rows [R] i32 names the batch rows to count: count row r belongs to
// batch row rows[r]; padding rows and rows nobody asked about are simply
// not named (termmask.hip's src_row idea). The caller zeroes counts.
//
// Grid (R, ceil(N / FACET_CHUNK)), the row index fast: the workgroups of
// one chunk are dispatched together and share its mask words and
// attribute lines through L2. A workgroup stages edges, langs and its
// row's domain list in LDS with its counters, and works in two steps.
// Step 1 walks the chunk four documents per lane (one 32-bit mask word
// covers one 128-byte line of scores = 8 lanes; the word is read first
// and a lane whose four bits are 0 loads no scores) and queues the
// chunk-local numbers of the matching documents in LDS: __ballot +
// popcount place them, one LDS atomic per wave and step reserves the
// room. Step 2 hands the queue out one document per lane: only matching
// documents load an attribute record, all lanes are busy and 256 loads
// are in flight together; dates, languages and domains go through LDS
// integer atomics, and TOTAL is the queue's length. Each non-zero
// counter is flushed with one integer atomicAdd, exact in any order.
// Without a mask the kernel reads none: a facet request never pushes an
// unmasked batch onto the masked top-k.
//
// Why a queue (measured at R = B = 128, N = 1.25M, score density 4 %,
// unmasked, next to 108 us for topk.hip's unmasked hist1 over the same
// scores): classifying a match where it is found, in the lane that read
// its score, took 461 us. At that density a wave has ~2.5 matches per
// quarter step, so it ran the whole classification four times per step
// with ~4 % of its lanes, each time behind a dependent attribute load.
// docs/performance.md has the figures of both.
#include "common.h"
#include "match_queue.h"

#define FACET_THREADS MATCHQ_THREADS
#define FACET_CHUNK MATCHQ_CHUNK   // documents per workgroup
#define FACET_MAX_EDGES 7
#define FACET_MAX_LANGS 32
#define FACET_MAX_DOMS 64
#define FACET_F_MAX (5 + FACET_MAX_EDGES + FACET_MAX_LANGS + FACET_MAX_DOMS)
// The counters live in LDS in 8 copies, lane L adding to copy L & 7, as
// common.h's HIST8 histograms do: 136 >= FACET_F_MAX and 136 % 64 == 8,
// so the copies of a slot sit in 8 distinct banks and a wave whose
// matches all share a slot spreads its atomics over them.
#define FACET_COPIES 8
#define FACET_STRIDE 136
static_assert(FACET_STRIDE >= FACET_F_MAX, "a copy holds every slot");

#define FACET_TOTAL 0
#define FACET_DATE_ZERO 1
#define FACET_DATE0 2

namespace {

__host__ __device__ inline int facet_lang_zero(int E) { return 3 + E; }
__host__ __device__ inline int facet_lang0(int E) { return 4 + E; }
__host__ __device__ inline int facet_lang_other(int E, int L) {
  return 4 + E + L;
}
__host__ __device__ inline int facet_dom0(int E, int L) { return 5 + E + L; }

// Index of key among the n ascending (unsigned) values at s, -1 when it
// is not there. docfilter.hip's in_sorted: every lane runs the same
// ceil(log2 n) steps, whatever its key.
DEVINL int find_sorted(const unsigned* s, unsigned n, unsigned key) {
  if (n == 0) return -1;
  unsigned base = 0;
  for (unsigned len = n; len > 1;) {
    const unsigned half = len >> 1;
    base += s[base + half - 1] < key ? half : 0u;
    len -= half;
  }
  return s[base] == key ? (int)base : -1;
}

template <bool MASKED>
__global__ __launch_bounds__(FACET_THREADS) void facet_counts_kernel(
    const float* __restrict__ scores, const int* __restrict__ rows,
    const unsigned* __restrict__ bits, const int* __restrict__ row_pred,
    const uint4* __restrict__ attrs, const unsigned* __restrict__ edges,
    const unsigned* __restrict__ langs, const int2* __restrict__ dom_desc,
    const unsigned* __restrict__ doms, int* __restrict__ counts, long N,
    long W, int B, int P, int E, int L, int F, long ndoms) {
  __shared__ unsigned s_edges[FACET_MAX_EDGES + 1];
  __shared__ unsigned s_langs[FACET_MAX_LANGS];
  __shared__ unsigned s_doms[FACET_MAX_DOMS];
  __shared__ int s_cnt[FACET_COPIES * FACET_STRIDE];
  __shared__ unsigned short s_q[FACET_CHUNK];  // chunk-local matching docs
  __shared__ unsigned s_n;                     // how many are queued
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  int b;
  const unsigned* mrow;
  if (!match_row<MASKED>(rows, bits, row_pred, B, P, W, &b, &mrow)) return;
  // the caller checks the descriptors and the caps; the clamps keep a bad
  // call inside the arrays all the same (everything block-uniform)
  E = min(max(E, 0), FACET_MAX_EDGES);
  L = min(max(L, 0), FACET_MAX_LANGS);
  const int lang_zero = facet_lang_zero(E), lang0 = facet_lang0(E);
  const int lang_other = facet_lang_other(E, L), dom0 = facet_dom0(E, L);
  if (F < dom0 || F > FACET_F_MAX) return;
  const int2 ds = dom_desc[r];
  const long off = min(max((long)ds.x, 0L), ndoms);
  const int nd = (int)min((long)min(min(max(ds.y, 0), FACET_MAX_DOMS),
                                    F - dom0), ndoms - off);
  if (tid < E) s_edges[tid] = edges[tid];
  if (tid < L) s_langs[tid] = langs[tid];
  if (tid < nd) s_doms[tid] = doms[off + tid];
  for (int i = tid; i < FACET_COPIES * FACET_STRIDE; i += FACET_THREADS)
    s_cnt[i] = 0;
  if (tid == 0) s_n = 0;
  __syncthreads();

  const long c0 = (long)blockIdx.y * FACET_CHUNK;
  const long c1 = min(c0 + FACET_CHUNK, N);
  const float* row = scores + (long)b * N;
  // Step 1, the streaming read: queue the chunk's matching documents
  // (match_queue.h; domtop.hip starts the same way).
  match_queue_fill<MASKED>(row, mrow, c0, c1, N, s_q, &s_n);
  __syncthreads();
  // Step 2: one queued document per lane, so the attribute loads of 256
  // matches are in flight together whatever the score density.
  const unsigned nq = min(s_n, (unsigned)FACET_CHUNK);
  int* mine = s_cnt + (tid & (FACET_COPIES - 1)) * FACET_STRIDE;
  for (unsigned i = tid; i < nq; i += FACET_THREADS) {
    const uint4 a = attrs[c0 + s_q[i]];
    int nle = 0;
    for (int e = 0; e < E; ++e) nle += s_edges[e] <= a.x ? 1 : 0;
    atomicAdd(&mine[a.x == 0 ? FACET_DATE_ZERO : FACET_DATE0 + nle], 1);
    const unsigned c = a.y & 0xffffu;
    const int li = find_sorted(s_langs, (unsigned)L, c);
    atomicAdd(&mine[c == 0 ? lang_zero : li >= 0 ? lang0 + li : lang_other],
              1);
    const int di = find_sorted(s_doms, (unsigned)nd, a.z);
    if (di >= 0) atomicAdd(&mine[dom0 + di], 1);
  }
  __syncthreads();
  if (tid < F) {
    int sum = tid == FACET_TOTAL ? (int)nq : 0;
#pragma unroll
    for (int c = 0; c < FACET_COPIES; ++c) sum += s_cnt[c * FACET_STRIDE + tid];
    if (sum) atomicAdd(&counts[(long)r * F + tid], sum);
  }
}

}  // namespace

extern "C" int infomesh_facet_chunk_docs() { return FACET_CHUNK; }

// Row width F of counts for E edges, L languages and a widest domain
// list of Dw hashes.
extern "C" int infomesh_facet_width(int E, int L, int Dw) {
  return facet_dom0(E, L) + Dw;
}

// First slot of a group: which = 0 TOTAL, 1 DATE_ZERO, 2 DATE0,
// 3 LANG_ZERO, 4 LANG0, 5 LANG_OTHER, 6 DOM0; -1 for anything else.
extern "C" int infomesh_facet_slot(int which, int E, int L) {
  switch (which) {
    case 0: return FACET_TOTAL;
    case 1: return FACET_DATE_ZERO;
    case 2: return FACET_DATE0;
    case 3: return facet_lang_zero(E);
    case 4: return facet_lang0(E);
    case 5: return facet_lang_other(E, L);
    case 6: return facet_dom0(E, L);
    default: return -1;
  }
}

// scores [B, N] f32; rows [R] i32 in [0, B); bits [P, W] u32 with
// W * 32 >= N and row_pred [B] i32 in [0, P), or both null (no mask);
// attrs [N, 4] u32; edges [E] u32 ascending, E <= 7; langs [L] u32
// ascending and unique, L <= 32; dom_desc [R, 2] i32 (off, n) into doms
// [ndoms] u32, each list unique and ascending as unsigned, n <= 64;
// counts [R, F] i32, zeroed by the caller, F = infomesh_facet_width(E, L,
// Dw) with Dw >= every n. The caller guarantees all of that.
extern "C" void infomesh_facet_counts(
    const void* scores, const void* rows, const void* bits,
    const void* row_pred, const void* attrs, const void* edges,
    const void* langs, const void* dom_desc, const void* doms, long ndoms,
    void* counts, int B, int R, long N, long W, int P, int E, int L, int F,
    void* stream) {
  if (R <= 0 || N <= 0 || B <= 0) return;
  auto s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)R,
                  (unsigned)((N + FACET_CHUNK - 1) / FACET_CHUNK));
  dispatch_masked(bits, row_pred, [&](auto masked) {
    hipLaunchKernelGGL(facet_counts_kernel<decltype(masked)::value>, grid,
                       dim3(FACET_THREADS), 0, s, (const float*)scores,
                       (const int*)rows, (const unsigned*)bits,
                       (const int*)row_pred, (const uint4*)attrs,
                       (const unsigned*)edges, (const unsigned*)langs,
                       (const int2*)dom_desc, (const unsigned*)doms,
                       (int*)counts, N, W, B, P, E, L, F, ndoms);
  });
}
