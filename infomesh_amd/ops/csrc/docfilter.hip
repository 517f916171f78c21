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
