// Pieces shared by the bf16 MFMA GEMM kernels (gemm.hip, gemm8.hip):
// the LDS swizzle, the 16-byte global->LDS copy and the epilogues.
// Everything here is DEVINL, so each kernel is the same code as if the
// piece were written out in its body.
#pragma once
#include "common.h"

// LDS swizzle on a [rows][64 bf16] row-major image (involution, 16 B
// granules), applied to the glds SOURCE address and the ds_read address
// (rule 21: the LDS destination stays lane-linear). BK=32 rows are 64 B
// and keep the linear image. Rows are 128 B so
// bank_start = 32*(row&1) + 4*chunk collapses rows r and r+2 onto the
// same banks; xoring the 16 B-chunk index (bits 4-6) with
// h(row) = (row ^ (row>>3)) & 7 (bits 7-12 of the offset) gives all 16
// rows of a quarter-wave MFMA operand read distinct 4-bank windows.
// Measured: the SQ_LDS_BANK_CONFLICT counter on the pipelined 64^2 tile
// (4.16e8, profiles/) is UNCHANGED by this — those conflicts come from
// the epilogue f32 staging (4-way ds_write folding, ~192 cycles/wave-
// tile), and wall time is glds-latency-bound either way; the swizzle is
// kept because conflict-free operand reads cost nothing. Key uses only
// bits >=7, which the xor never touches, so swz(swz(x)) == x and
// region bases (bit 13+) pass through unchanged.
DEVINL int swz(int byte_off) {
  return byte_off ^ ((((byte_off >> 7) ^ (byte_off >> 10)) & 7) << 4);
}

// One glds: every lane copies 16 B from its own global address to
// lds_base + lane*16 (lds_base is wave-uniform). CPOL is the
// cache-policy immediate: 0 = default, 2 = non-temporal.
// gemm8 streams A with CPOL=2: A (M up to ~512k rows) passes through
// exactly once while B (N*K*2 <= a few MB at the shapes that kernel
// serves) wants to stay in the XCD's 4 MB L2 across m-tiles. Marking
// the A loads non-temporal stops the A stream from evicting B —
// without it B thrashes and the kernel runs at the
// read-everything-from-HBM roofline (~700 GF/s at the reranker shapes;
// torch/rocBLAS was 2x faster purely on this reuse).
template <int CPOL>
DEVINL void glds16(const bf16* gsrc, void* lds_base) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)gsrc,
      (__attribute__((address_space(3))) unsigned int*)lds_base,
      16, 0, CPOL);
}

// A wave's accumulators are FM x FN fragments of 16x16 (mfma 16x16x32
// C layout: lane holds rows (lane>>4)*4 .. +3 of column lane&15). Both
// epilogues write act(alpha*acc + bias[n]) for the wave's block whose
// top-left element is (m_base, n_base); c_off is the element offset of
// this batch entry's C; lane is the caller's threadIdx.x & 63 (taking
// it as an argument, not recomputing it, keeps the compiler's output
// for the kernels what it was with the epilogue written in place).

// Guarded scalar stores: any M, N; row stride ldc; f32 or bf16 output.
template <bool OUT_F32, int FM, int FN>
DEVINL void store_frags_guarded(const f32x4 (&acc)[FM][FN], void* C,
                                long c_off, const float* bias,
                                int m_base, int n_base, int M, int N,
                                int ldc, int act, float alpha, int lane) {
  const int crow_base = (lane >> 4) * 4;
  const int ccol = lane & 15;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n_base + j * 16 + ccol;
      if (n >= N) continue;
      const float bv = bias ? bias[n] : 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m_base + i * 16 + crow_base + r;
        if (m >= M) continue;
        float v = apply_act(alpha * acc[i][j][r] + bv, act);
        if (OUT_F32)
          reinterpret_cast<float*>(C)[c_off + (long)m * ldc + n] = v;
        else
          reinterpret_cast<bf16*>(C)[c_off + (long)m * ldc + n] = f2bf(v);
      }
    }
  }
}

template <int CTRL>
DEVINL uint32_t max_dpp(uint32_t v) {   // max(v, v of the lane CTRL names)
  return max(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL,
                                                      0xf, 0xf, false));
}
// Maximum of o over each aligned group of G (8 or 16) lanes, returned in
// every lane of the group. DPP moves inside a 16-lane row — both quad
// swaps, then the half-row and (G = 16) row mirrors — so it costs four
// VALU ops and no LDS traffic, where __shfl_xor is a ds_bpermute each.
// Every lane of the wave must be active.
template <int G>
DEVINL uint32_t group_max_u32(uint32_t o) {
  static_assert(G == 8 || G == 16, "a half or a whole DPP row");
  o = max_dpp<0xB1>(o);                 // quad_perm [1,0,3,2]
  o = max_dpp<0x4E>(o);                 // quad_perm [2,3,0,1]
  o = max_dpp<0x141>(o);                // row_half_mirror
  if (G == 16) o = max_dpp<0x140>(o);   // row_mirror
  return o;
}

// f32 output of a FULL tile: stage the wave's [FM*16][FN*16] block
// through LDS (stage_f32, the wave's own region of the drained
// operand buffers) and emit 16-B dwordx4 stores, NONTEMPORAL — C is
// written once and next read by the streaming top-k, so allocating it
// in L2 only evicts the B rows being streamed. The caller has made
// sure nobody still reads or glds-writes the operand buffers.
// BMAX: also write the maximum of each row of the wave block (W = SEGN
// consecutive columns, block n_base / SEGN of the row) to
// bmax[m * NB + block], taken from the f32x4 each lane reads back —
// the values stored, so the maximum is of the scores bit for bit. The
// order is the top-k selector's (float_to_ordered: -0.0 < +0.0).
// The LPR lanes that read a row back reduce it among themselves, lane c
// of the group keeps the result of iteration c, and after the LPR
// iterations the wave's 64 lanes hold its 64 row maxima: one 4-byte
// store each. These are NOT nontemporal: the neighbouring n-tiles fill
// the rest of the line, which merges in L2.
template <int FM, int FN, bool BMAX = false>
DEVINL void store_frags_staged_f32(const f32x4 (&acc)[FM][FN],
                                   float* stage_f32, float* C, long c_off,
                                   const float* bias, int m_base,
                                   int n_base, int N, int act,
                                   float alpha, int lane,
                                   float* bmax = nullptr, long NB = 0) {
  constexpr int SEGN = FN * 16;                  // cols of the wave block
  const int crow_base = (lane >> 4) * 4;
  const int ccol = lane & 15;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lm = i * 16 + crow_base + r;      // wave-local row
        const int ln = j * 16 + ccol;               // wave-local col
        const float bv = bias ? bias[n_base + ln] : 0.0f;
        stage_f32[lm * SEGN + ln] =
            apply_act(alpha * acc[i][j][r] + bv, act);
      }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // LDS writes visible
  __builtin_amdgcn_wave_barrier();
  // each lane streams 16 B of a row segment
  constexpr int LPR = SEGN * 4 / 16;             // lanes per row
  constexpr int ROWS_PER_IT = 64 / LPR;
  static_assert(!BMAX || FM * 16 == LPR * ROWS_PER_IT,
                "BMAX: 64 rows per wave, one maximum per lane");
  const int srow = lane / LPR, scol4 = (lane % LPR) * 4;
  uint32_t mine = 0;       // ordered key of this lane's row maximum
#pragma unroll
  for (int base = 0; base < FM * 16; base += ROWS_PER_IT) {
    const int lm = base + srow;
    const int m = m_base + lm;
    const int n = n_base + scol4;
    f32x4 v = *reinterpret_cast<const f32x4*>(
        &stage_f32[lm * SEGN + scol4]);
    __builtin_nontemporal_store(
        v, reinterpret_cast<f32x4*>(C + c_off + (long)m * N + n));
    if constexpr (BMAX) {
      const uint32_t o = group_max_u32<LPR>(
          max(max(float_to_ordered(v[0]), float_to_ordered(v[1])),
              max(float_to_ordered(v[2]), float_to_ordered(v[3]))));
      if (lane % LPR == base / ROWS_PER_IT) mine = o;
    }
  }
  if constexpr (BMAX) {
    const int m = m_base + (lane % LPR) * ROWS_PER_IT + srow;
    bmax[(long)m * NB + n_base / SEGN] = ordered_to_float(mine);
  }
}

// The guarded f32 epilogue plus block maxima as above, for partial
// tiles: the maximum is over the block's valid columns (n < N) only, and
// a block with none (n_base >= N) or a row m >= M writes nothing. A row's
// 16 columns of a fragment sit in the 16 lanes of one DPP row; lane
// 4*i + r of it keeps the maximum of fragment row (i, r).
template <int FM, int FN>
DEVINL void store_frags_guarded_bmax(const f32x4 (&acc)[FM][FN], float* C,
                                     long c_off, const float* bias,
                                     int m_base, int n_base, int M, int N,
                                     int act, float alpha, int lane,
                                     float* bmax, long NB) {
  static_assert(FM == 4, "64 rows per wave, one maximum per lane");
  constexpr int SEGN = FN * 16;
  const int crow_base = (lane >> 4) * 4;
  const int ccol = lane & 15;
  uint32_t mine = 0;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    uint32_t o[4] = {0u, 0u, 0u, 0u};   // below every non-NaN key
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n_base + j * 16 + ccol;
      const bool valid = n < N;
      const float bv = (valid && bias) ? bias[n] : 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m_base + i * 16 + crow_base + r;
        const float v = apply_act(alpha * acc[i][j][r] + bv, act);
        if (valid) {
          o[r] = max(o[r], float_to_ordered(v));
          if (m < M) C[c_off + (long)m * N + n] = v;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t g = group_max_u32<16>(o[r]);
      if (ccol == i * 4 + r) mine = g;
    }
  }
  const int m = m_base + (ccol >> 2) * 16 + crow_base + (ccol & 3);
  if (m < M && n_base < N)
    bmax[(long)m * NB + n_base / SEGN] = ordered_to_float(mine);
}
