// What the kernels over a query row's whole match set share (facets.hip,
// domtop.hip, collapse.hip): the grid (R, ceil(N / MATCHQ_CHUNK)), the
// row prologue and its mask dispatch, and the streaming read that
// queues, in LDS, the chunk-local numbers of a chunk's matching
// documents.
//
// The match rule is the one in the header of facets.hip: document d
// matches iff it passes the row's mask (bit d of mrow; every document
// passes when there is no mask) and row[d] > 0.
#pragma once
#include <type_traits>
#include "common.h"

#define MATCHQ_THREADS 256
#define MATCHQ_CHUNK 8192   // documents per workgroup: 8 steps of 1024
static_assert(MATCHQ_CHUNK <= 65536 &&
                  MATCHQ_CHUNK % (MATCHQ_THREADS * 4) == 0,
              "the queue holds chunk-local u16 document numbers");

// The row prologue: workgroup row r = blockIdx.x works on batch row
// *b = rows[r], under mask row *mrow = bits + row_pred[*b] * W (null
// when not MASKED). The caller checks rows and row_pred on the host; the
// clamps keep a bad call inside the arrays all the same: false (block-
// uniform) means the workgroup has nothing to do and returns.
template <bool MASKED>
DEVINL bool match_row(const int* __restrict__ rows,
                      const unsigned* __restrict__ bits,
                      const int* __restrict__ row_pred, int B, int P, long W,
                      int* b, const unsigned** mrow) {
  *mrow = nullptr;
  *b = rows[(int)blockIdx.x];
  if (*b < 0 || *b >= B) return false;
  if constexpr (MASKED) {
    const int p = row_pred[*b];
    if (p < 0 || p >= P) return false;
    *mrow = bits + (long)p * W;
  }
  return true;
}

// Host side: f(std::true_type{}) or f(std::false_type{}) as `on` says, so
// a launcher writes its launch once, with decltype(arg)::value as the
// kernel's template argument.
template <typename F>
inline void dispatch_bool(bool on, F f) {
  if (on)
    f(std::true_type{});
  else
    f(std::false_type{});
}
// The call has a mask when bits and row_pred are both given; the
// unmasked kernels read neither pointer.
template <typename F>
inline void dispatch_masked(const void* bits, const void* row_pred, F f) {
  dispatch_bool(bits != nullptr && row_pred != nullptr, f);
}

// Walks documents [c0, c1) of `row` (c1 <= N, c1 - c0 <= MATCHQ_CHUNK, c0
// a multiple of MATCHQ_CHUNK) four per lane: one 32-bit mask word covers
// one 128-byte line of scores = 8 lanes; the word is read first and a
// lane whose four bits are 0 loads no scores. __ballot + popcount place
// the matches in s_q [MATCHQ_CHUNK], one LDS atomic per wave and step
// reserves the room in *s_n, which the caller zeroes behind a barrier
// before the call and reads behind a barrier after it. Every lane of a
// MATCHQ_THREADS-wide workgroup must make the call: the trip count is
// block-uniform, so every lane reaches the ballots.
template <bool MASKED>
DEVINL void match_queue_fill(const float* __restrict__ row,
                             const unsigned* __restrict__ mrow, long c0,
                             long c1, long N, unsigned short* s_q,
                             unsigned* s_n) {
  const int tid = threadIdx.x;
  const unsigned long long below = (1ull << (tid & (WAVE - 1))) - 1ull;
  for (long base = c0; base < c1; base += MATCHQ_THREADS * 4) {
    const long d = base + tid * 4;
    unsigned m = 0;  // bit j: document d + j matches
    if (d < c1) {    // c1 <= N and d is a multiple of 4
      // bit j: document d + j exists (and passes)
      unsigned ok = d + 4 <= N ? 15u : (1u << (unsigned)(N - d)) - 1u;
      if constexpr (MASKED) ok &= mrow[d >> 5] >> (unsigned)(d & 31);
      if (ok) {
        if (d + 4 <= N) {
          // row = scores + b * N: with N % 4 != 0 and b > 0 this address
          // is 4-byte aligned only. It relies on the unaligned global
          // dwordx4 loads gfx950 does in hardware, as topk.hip's float4
          // reads of a row do; the tail branch is about the row's END
          // (fewer than four documents left), not about alignment.
          const float4 v = *reinterpret_cast<const float4*>(row + d);
          m = (v.x > 0.0f ? 1u : 0u) | (v.y > 0.0f ? 2u : 0u) |
              (v.z > 0.0f ? 4u : 0u) | (v.w > 0.0f ? 8u : 0u);
        } else {
          for (int j = 0; j < 3; ++j)
            if (d + j < N && row[d + j] > 0.0f) m |= 1u << j;
        }
        m &= ok;
      }
    }
    // one queue reservation per wave: ballots and popcounts place every
    // lane's matches, a single LDS atomic moves the tail
    const unsigned long long b0 = __ballot(m & 1u), b1 = __ballot(m & 2u);
    const unsigned long long b2 = __ballot(m & 4u), b3 = __ballot(m & 8u);
    const unsigned n0 = __popcll(b0), n1 = __popcll(b1), n2 = __popcll(b2);
    const unsigned nw = n0 + n1 + n2 + __popcll(b3);  // wave-uniform
    if (nw) {
      unsigned at = 0;
      if ((tid & (WAVE - 1)) == 0) at = atomicAdd(s_n, nw);
      at = __shfl(at, 0, WAVE);
      // a document is queued at most once, so the tail never passes
      // MATCHQ_CHUNK; d - c0 < MATCHQ_CHUNK <= 65536
      const unsigned loc = (unsigned)(d - c0);
      if (m & 1u) s_q[at + __popcll(b0 & below)] = (unsigned short)loc;
      at += n0;
      if (m & 2u) s_q[at + __popcll(b1 & below)] = (unsigned short)(loc + 1);
      at += n1;
      if (m & 4u) s_q[at + __popcll(b2 & below)] = (unsigned short)(loc + 2);
      at += n2;
      if (m & 8u) s_q[at + __popcll(b3 & below)] = (unsigned short)(loc + 3);
    }
  }
}
