// Per-document filter predicates -> pass/fail bitmasks for the masked
// top-k (topk.hip). Deletes (tombstones) and the site:/lang:/after:/
// before: query filters are one mechanism: a bit per document that the
// selection honours. Replaces: the reference's SQL WHERE clauses on the
// documents table (infomesh/index/local_store.py search filters) and its
// DELETE on the GPU-resident shard.
//
// THE layout (index/doc_attrs.py packs exactly this, nothing else does).
// One 16-byte record per document, four u32 words:
//   w0  crawled_at, whole seconds
//   w1  bits 0-15 language: ord(c0)<<8 | ord(c1) of the lower-cased
//       2-letter code, 0 = unknown; bit 16 = dead (tombstone)
//   w2  low 32 bits of hash64(domain), domain lower-cased
//   w3  reserved, 0
// One 16-byte predicate, four u32 words:
//   x   after, seconds (0 = none)
//   y   before, seconds (0xFFFFFFFF = none)
//   z   bits 0-15 language (0 = any); bit 16 = has_site
//   w   domain hash, compared when has_site
// A document passes iff it is not dead, x <= w0 <= y, the predicate's
// language is 0 or equals the document's, and has_site is clear or
// w2 == w.
//
// Domain lists (filter_bitmask_sets) extend the predicate, not its 16
// bytes. Bits 18 and 19 of z are has_allow and has_block (bit 17 is the
// query plane's in-transit mark); they tell a receiver that lists
// follow. The lists themselves travel beside the predicates:
//   doms  flat u32 domain hashes, each list unique and ascending AS
//         UNSIGNED
//   desc  [P, 4] i32 per predicate: allow_off, allow_n, block_off,
//         block_n, offsets into doms; allow_n + block_n <= 2048
// A document then passes iff it passes the predicate above, allow_n is 0
// or w2 is in the allow list, and w2 is not in the block list (so a
// domain in both is blocked). The kernel reads the counts, never the
// flag bits: allow_n == block_n == 0 gives filter_bitmask's bits.
//
// Same wave64 idiom as simhash.hip: one lane per document, and
// __ballot(pass) IS the 64 mask bits of the wave's documents.
#include "common.h"

#define ATTR_LANG_MASK 0xffffu
#define ATTR_DEAD_BIT 0x10000u
#define PRED_SITE_BIT 0x10000u

namespace {

// bits: [P, W] u32, W = ceil(N/64)*2; bit (d & 31) of word d >> 5 is
// document d. Every word of a row is written, positions >= N as 0.
__global__ __launch_bounds__(256) void filter_bitmask_kernel(
    const uint4* __restrict__ attrs, const uint4* __restrict__ preds,
    unsigned* __restrict__ bits, long N, long W) {
  const int p = blockIdx.y;
  const uint4 q = preds[p];  // block-uniform
  const long d = (long)blockIdx.x * blockDim.x + threadIdx.x;
  bool pass = false;
  if (d < N) {
    const uint4 a = attrs[d];
    const unsigned qlang = q.z & ATTR_LANG_MASK;
    pass = !(a.y & ATTR_DEAD_BIT) && q.x <= a.x && a.x <= q.y &&
           (qlang == 0 || qlang == (a.y & ATTR_LANG_MASK)) &&
           (!(q.z & PRED_SITE_BIT) || a.z == q.w);
  }
  const unsigned long long m = __ballot(pass);
  const long w0 = (d >> 6) * 2;  // wave-uniform; d is a multiple of 64 on lane 0
  if ((threadIdx.x & 63) == 0 && w0 < W) {
    unsigned* row = bits + (long)p * W;
    row[w0] = (unsigned)m;
    row[w0 + 1] = (unsigned)(m >> 32);
  }
}

#define SETS_MAX 2048        // hashes per predicate = 8 KB of LDS
#define SETS_CHUNK (8 * 256)  // documents per workgroup

// Is key among the n ascending (unsigned) values at s? Every lane of the
// workgroup runs the same ceil(log2 n) steps, whatever its key.
__device__ __forceinline__ bool in_sorted(const unsigned* s, unsigned n,
                                          unsigned key) {
  if (n == 0) return false;
  unsigned base = 0;
  for (unsigned len = n; len > 1;) {
    const unsigned half = len >> 1;
    base += s[base + half - 1] < key ? half : 0u;
    len -= half;
  }
  return s[base] == key;
}

// grid (ceil(N / SETS_CHUNK), P): the predicate and its lists are
// block-uniform. The lists go to LDS once and serve SETS_CHUNK
// documents; one 2048-entry list is 8 KB, as much as the attributes of
// 512 documents, so a 256-document workgroup would read more list than
// attributes. Output as filter_bitmask_kernel writes it.
__global__ __launch_bounds__(256) void filter_bitmask_sets_kernel(
    const uint4* __restrict__ attrs, const uint4* __restrict__ preds,
    const int4* __restrict__ desc, const unsigned* __restrict__ doms,
    unsigned* __restrict__ bits, long N, long W) {
  __shared__ unsigned lists[SETS_MAX];
  const int p = blockIdx.y;
  const uint4 q = preds[p];
  const int4 ds = desc[p];
  // the caller checks the descriptors; the clamps keep a bad one inside
  // the LDS array all the same
  const unsigned an = (unsigned)min(max(ds.y, 0), SETS_MAX);
  const unsigned bn = (unsigned)min(max(ds.w, 0), SETS_MAX - (int)an);
  for (unsigned i = threadIdx.x; i < an; i += blockDim.x)
    lists[i] = doms[(long)ds.x + i];
  for (unsigned i = threadIdx.x; i < bn; i += blockDim.x)
    lists[an + i] = doms[(long)ds.z + i];
  __syncthreads();
  const unsigned qlang = q.z & ATTR_LANG_MASK;
  unsigned* row = bits + (long)p * W;
  const long d0 = (long)blockIdx.x * SETS_CHUNK;
  for (int it = 0; it < SETS_CHUNK / 256 && d0 + it * 256 < N; ++it) {
    const long d = d0 + it * 256 + threadIdx.x;
    bool pass = false;
    if (d < N) {
      const uint4 a = attrs[d];
      pass = !(a.y & ATTR_DEAD_BIT) && q.x <= a.x && a.x <= q.y &&
             (qlang == 0 || qlang == (a.y & ATTR_LANG_MASK)) &&
             (!(q.z & PRED_SITE_BIT) || a.z == q.w);
      // evaluated for every document in range, so a wave never diverges
      // inside the search
      const bool allowed = an == 0 || in_sorted(lists, an, a.z);
      const bool blocked = in_sorted(lists + an, bn, a.z);
      pass = pass && allowed && !blocked;
    }
    const unsigned long long m = __ballot(pass);
    const long w0 = (d >> 6) * 2;  // wave-uniform, as above
    if ((threadIdx.x & 63) == 0 && w0 < W) {
      row[w0] = (unsigned)m;
      row[w0 + 1] = (unsigned)(m >> 32);
    }
  }
}

}  // namespace

extern "C" void infomesh_filter_bitmask(const void* attrs, const void* preds,
                                        void* bits, long N, int P,
                                        void* stream) {
  if (N <= 0 || P <= 0) return;
  auto s = reinterpret_cast<hipStream_t>(stream);
  const long W = (N + 63) / 64 * 2;
  hipLaunchKernelGGL(filter_bitmask_kernel,
                     dim3((unsigned)((N + 255) / 256), P), dim3(256), 0, s,
                     (const uint4*)attrs, (const uint4*)preds,
                     (unsigned*)bits, N, W);
}

// As infomesh_filter_bitmask, with per-predicate domain lists: desc
// [P, 4] i32 and doms u32 as in the header. The caller guarantees that
// every (off, n) lies inside doms and allow_n + block_n <= 2048.
extern "C" void infomesh_filter_bitmask_sets(const void* attrs,
                                             const void* preds,
                                             const void* desc,
                                             const void* doms, void* bits,
                                             long N, int P, void* stream) {
  if (N <= 0 || P <= 0) return;
  auto s = reinterpret_cast<hipStream_t>(stream);
  const long W = (N + 63) / 64 * 2;
  hipLaunchKernelGGL(filter_bitmask_sets_kernel,
                     dim3((unsigned)((N + SETS_CHUNK - 1) / SETS_CHUNK), P),
                     dim3(256), 0, s, (const uint4*)attrs,
                     (const uint4*)preds, (const int4*)desc,
                     (const unsigned*)doms, (unsigned*)bits, N, W);
}
