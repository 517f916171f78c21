// Batched-strided bf16 MFMA GEMM for gfx950: C[g] = act(A[g] @ B[g]^T + bias).
//
// Layout: A [M,K] row-major, B [N,K] row-major (both K-contiguous — "NT"),
// C [M,N]. f32 accumulation on mfma_f32_16x16x32_bf16; output bf16 or f32.
//
// Structure (guide cdna_hip_programming.md §5 "step-3"): 128x128 tile,
// BK∈{32,64}, 4 waves (2x2) each owning a 64x64 sub-tile as 4x4 fragments
// of 16x16, double-buffered LDS staged by __builtin_amdgcn_global_load_lds
// width 16 (lane-linear LDS image), one vmcnt(0)+barrier per K-step.
// Replaces: the reference's torch/sentence-transformers matmuls
// (infomesh/index/vector_store.py:120-157) and external-LLM HTTP calls
// (infomesh/summarizer/engine.py:111-318) — see SURVEY.md §2.9.
#include "gemm_common.h"
#include <cstdlib>

namespace {

// Blocks of W columns in a row of N.
__host__ DEVINL long bmax_blocks(int N, int W) { return ((long)N + W - 1) / W; }
// The one pointer of a BMAX kernel's parameter pack.
DEVINL float* bmax_of(float* p) { return p; }

// Tile configurations (4 waves each):
//   (128,128): 2x2 wave grid, 64x64 per wave (4x4 fragments) — default.
//   ( 64,128): 1x4 grid, 64x32 per wave — skinny-M (query scoring).
//   ( 64, 64): 2x2 grid, 32x32 per wave — latency-bound small-K shapes
//              (encoder projections) where 128^2 tiles underfill the
//              chip and the 6-step K loop's stage latency dominates.
//              Only K%64 != 0 lands here; K%64 == 0 takes
//              gemm_pipe64_kernel below.
// The BK=64 images are swizzled (swz); BK=32 rows are 64 B and keep
// the linear image.
// BMAX (f32 output only): the kernel also writes each row's maximum over
// every wave's column span W = BN / WN to bmax [batch, M, ceil(N / W)]:
// bmax[g][m][j] = max of C[g][m][j*W .. j*W+W-1] over the columns < N
// (gemm_common.h epilogues). The pointer is a parameter pack that is
// empty when !BMAX, so the plain instantiations keep the signature,
// the kernarg layout and hence the code they had without it (the
// MaskRef pack of topk.hip does the same).
template <int BM, int BN, int BK, bool OUT_F32, bool BMAX = false,
          typename... BmaxPtr>
__global__ __launch_bounds__(256) void gemm_bf16_nt_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ B,
    void* __restrict__ C, const float* __restrict__ bias,
    int M, int N, int K,
    long strideA, long strideB, long strideC,
    int act, float alpha, BmaxPtr... bmax) {
  static_assert(sizeof...(BmaxPtr) == (BMAX ? 1 : 0) && (OUT_F32 || !BMAX),
                "one float* iff BMAX, and BMAX is f32 only");
  // One __shared__ object only (glds pipeline rule, guide §5 item 4a).
  // Layout per buffer: A tile [BM*BK] then B tile [BN*BK].
  __shared__ bf16 smem[2][(BM + BN) * BK];

  const int tiles_n = (N + BN - 1) / BN;
  const int tiles_m = (M + BM - 1) / BM;
  const int tile = xcd_swizzle(blockIdx.x, tiles_m * tiles_n);
  const int tm = tile / tiles_n, tn = tile % tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int g = blockIdx.y;

  const bf16* Ag = A + (long)g * strideA;
  const bf16* Bg = B + (long)g * strideB;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;          // 4 waves
  constexpr int WM = (BM == 128 || BN == 64) ? 2 : 1;   // wave grid M
  constexpr int WN = 4 / WM;                // wave grid N
  constexpr int FM = (BM / WM) / 16;        // m-frags per wave
  constexpr int FN = (BN / WN) / 16;        // n-frags per wave
  const int wm = wid / WN, wn = wid % WN;

  // ---- glds staging geometry -------------------------------------------
  // One glds instruction: 64 lanes x 16 B = 1 KiB = 8 rows of BK=64 bf16
  // (or 16 rows of 64 B when BK=32).
  // A tile is BM*BK*2 bytes = BM*BK/512 KiB -> chunks of 1 KiB each.
  // Chunk count follows the larger (B) tile; A stages only its first
  // BM*BK*2/1024 chunks (guarded below) when BM < BN.
  constexpr int CHUNKS = ((BM > BN ? BM : BN) * BK * 2) / 1024;
  constexpr int CHUNKS_PER_WAVE = CHUNKS / 4;
  constexpr int ACHUNKS = (BM * BK * 2) / 1024;
  constexpr int BCHUNKS2 = (BN * BK * 2) / 1024;

  const int n_ksteps = K / BK;

  auto stage = [&](int buf, int kstep) {
    const long k0 = (long)kstep * BK;
#pragma unroll
    for (int c = 0; c < CHUNKS_PER_WAVE; ++c) {
      const int chunk = wid * CHUNKS_PER_WAVE + c;
      // region-relative source byte under the swizzle involution; the
      // LDS destination stays lane-linear (glds writes base + lane*16)
      const int lin = chunk * 1024 + lane * 16;
      const int src = (BK == 64) ? swz(lin) : lin;
      const int row = src / (BK * 2);
      const int colb = src % (BK * 2);
      if (chunk < BCHUNKS2) {
        int brow = n0 + row; brow = brow < N ? brow : N - 1;
        glds16<0>(Bg + (long)brow * K + k0 + colb / 2,
                  &smem[buf][BM * BK + chunk * 512]);
      }
      if (chunk < ACHUNKS) {
        int arow = m0 + row; arow = arow < M ? arow : M - 1;
        glds16<0>(Ag + (long)arow * K + k0 + colb / 2,
                  &smem[buf][chunk * 512]);
      }
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  __syncthreads();

  const int fr = lane & 15;          // fragment row (A) / col (B)
  const int fk = (lane >> 4) * 8;    // fragment k base

  int cur = 0;
  for (int t = 0; t < n_ksteps; ++t) {
    if (t + 1 < n_ksteps) stage(cur ^ 1, t + 1);
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      bf16x8 a[FM], b[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int row = wm * (BM / WM) + i * 16 + fr;
        const int off = (row * BK + ks * 32 + fk) * 2;
        a[i] = *reinterpret_cast<const bf16x8*>(
            (const char*)&smem[cur][0]
            + ((BK == 64) ? swz(off) : off));
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int row = wn * (BN / WN) + j * 16 + fr;
        const int off = (row * BK + ks * 32 + fk) * 2;
        b[j] = *reinterpret_cast<const bf16x8*>(
            (const char*)&smem[cur][BM * BK]
            + ((BK == 64) ? swz(off) : off));
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();   // drains the in-flight glds (vmcnt(0)) + barrier
    cur ^= 1;
  }

  // ---- epilogue ---------------------------------------------------------
  // Full f32 tiles (the dense scoring plane is huge-N f32) go out
  // through the LDS-staged nontemporal path; partial tiles and bf16
  // outputs keep the direct scalar path.
  const int m_base = m0 + wm * (BM / WM), n_base = n0 + wn * (BN / WN);
  // The f32 tile has to fit the operand buffers it is staged in: with
  // BK = 32 the 128-column tiles' do not (32 KB of smem for a 64 KB
  // tile), and staging them anyway lost the rows past the end of smem
  // (LDS writes out of range are dropped, the readback gave zeros).
  constexpr bool STAGE_FITS = BM * BN * 4 <= (int)sizeof(smem);
  if (OUT_F32 && STAGE_FITS && n0 + BN <= N && m0 + BM <= M) {
    // reuse the (drained) double buffer as an f32 staging tile:
    // per wave a [BM/WM][BN/WN] block = 64x64 (or 64x32/32x32) f32
    float* stage_f32 = reinterpret_cast<float*>(&smem[0][0])
        + wid * (BM / WM) * (BN / WN);
    __syncthreads();   // all MFMA reads of smem are done
    if constexpr (BMAX)
      store_frags_staged_f32<FM, FN, true>(
          acc, stage_f32, reinterpret_cast<float*>(C), (long)g * strideC,
          bias, m_base, n_base, N, act, alpha, lane,
          bmax_of(bmax...) + (long)g * M * bmax_blocks(N, BN / WN),
          bmax_blocks(N, BN / WN));
    else
      store_frags_staged_f32(acc, stage_f32, reinterpret_cast<float*>(C),
                             (long)g * strideC, bias, m_base, n_base, N,
                             act, alpha, lane);
    return;
  }
  if constexpr (BMAX)
    store_frags_guarded_bmax(
        acc, reinterpret_cast<float*>(C), (long)g * strideC, bias, m_base,
        n_base, M, N, act, alpha, lane,
        bmax_of(bmax...) + (long)g * M * bmax_blocks(N, BN / WN),
        bmax_blocks(N, BN / WN));
  else
    store_frags_guarded<OUT_F32>(acc, C, (long)g * strideC, bias,
                                 m_base, n_base, M, N, N, act, alpha, lane);
}

// ---- 3-buffer glds-span pipelined 64x64 tile ---------------------------
// For the latency-bound regime (encoder projections: M~4096, small N/K,
// few K-steps): the serial stage->vmcnt(0)->barrier->compute structure
// of the generic tile pays a full LDS-fill latency every K-step. Here
// stages t+1 AND t+2 stay in flight across RAW s_barriers with counted
// vmcnt waits (guide "pipelining across barriers": 3-buf span +83% over
// serial at 1-block/CU), and 16 KiB/buffer keeps 3 workgroups resident
// per CU on top. Round-1 BACKLOG item "counted-vmcnt small-tile
// pipeline (gemm8-style scheduling at 64^2)".
// (A 64x128 variant ran the full encoder in 1278 vs 990 us: 2 WGs/CU
// lose more than the wider MFMA blocks gain — see BACKLOG.)
template <bool OUT_F32>
__global__ __launch_bounds__(256) void gemm_pipe64_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ B,
    void* __restrict__ C, const float* __restrict__ bias,
    int M, int N, int K,
    long strideA, long strideB, long strideC,
    int act, float alpha) {
  constexpr int BM = 64, BN = 64, BK = 64;
  __shared__ bf16 smem[3][(BM + BN) * BK];   // 3 x 16 KiB

  const int tiles_n = (N + BN - 1) / BN;
  const int tiles_m = (M + BM - 1) / BM;
  const int tile = xcd_swizzle(blockIdx.x, tiles_m * tiles_n);
  const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
  const int g = blockIdx.y;
  const bf16* Ag = A + (long)g * strideA;
  const bf16* Bg = B + (long)g * strideB;

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wm = wid >> 1, wn = wid & 1;    // 2x2 waves, 32 x BN/2 each
  constexpr int FN = BN / 2 / 16;           // n-frags per wave
  const int n_ksteps = K / BK;

  // tile = (BM+BN)*BK*2 bytes in 1 KiB chunks (A chunks then B);
  // CPW glds per wave per stage
  constexpr int CPW = (BM + BN) * BK * 2 / 1024 / 4;
  auto stage = [&](int buf, int t) {
    const int ks = t < n_ksteps ? t : n_ksteps - 1;  // clamp (static cnt)
    const long k0 = (long)ks * BK;
#pragma unroll
    for (int c = 0; c < CPW; ++c) {
      const int chunk = wid * CPW + c;
      const int lin = chunk * 1024 + lane * 16;
      const int src = swz(lin);
      const int row = src / (BK * 2);
      const int colb = src % (BK * 2);
      const bool is_b = chunk >= (BM * BK * 2 / 1024);
      int grow = is_b ? (n0 + row - BM) : (m0 + row);
      const int lim = is_b ? N : M;
      grow = grow < lim ? grow : lim - 1;
      const bf16* gsrc = (is_b ? Bg : Ag) + (long)grow * K + k0 + colb / 2;
      // NT on the A loads was tried here (gemm8-style): encoder
      // 993 -> 1135 us. At these shapes BOTH operands fit the XCD L2
      // together (A 3.1 MB x 18-way n-reuse + B 0.9 MB), so the NT
      // hint only destroyed A's own reuse. Keep default caching.
      glds16<0>(gsrc, (char*)&smem[buf][0] + (long)chunk * 1024);
    }
  };

  const int fr = lane & 15;
  const int fk = (lane >> 4) * 8;
  f32x4 acc[2][FN];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  stage(1, 1);
  asm volatile("s_waitcnt vmcnt(%0)" :: "n"(CPW) : "memory");  // t0 in
  __builtin_amdgcn_s_barrier();

  for (int t = 0; t < n_ksteps; ++t) {
    const char* abase = (const char*)&smem[t % 3][0];
    const char* bbase = abase + BM * BK * 2;
    bf16x8 a[2][2], b[FN][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int row = wm * 32 + i * 16 + fr;
        a[i][ks] = *reinterpret_cast<const bf16x8*>(
            abase + swz((row * BK + ks * 32 + fk) * 2));
      }
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int brow = wn * (BN / 2) + j * 16 + fr;
        b[j][ks] = *reinterpret_cast<const bf16x8*>(
            bbase + swz((brow * BK + ks * 32 + fk) * 2));
      }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[i][ks], b[j][ks], acc[i][j], 0, 0, 0);
    stage((t + 2) % 3, t + 2);
    // own t+1 chunks landed (t+2's CPW stay in flight); cross-wave
    // visibility via the raw barrier — __syncthreads() would emit
    // vmcnt(0) and drain the span (guide pitfall)
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(CPW) : "memory");
    __builtin_amdgcn_s_barrier();
  }

  // drain the clamped tail prefetches before reusing smem
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  constexpr int SEGN = BN / 2;
  const int m_base = m0 + wm * 32, n_base = n0 + wn * SEGN;
  if (OUT_F32 && n0 + BN <= N && m0 + BM <= M) {
    float* stage_f32 = reinterpret_cast<float*>(&smem[0][0])
        + wid * 32 * SEGN;
    store_frags_staged_f32(acc, stage_f32, reinterpret_cast<float*>(C),
                           (long)g * strideC, bias, m_base, n_base, N,
                           act, alpha, lane);
    return;
  }
  store_frags_guarded<OUT_F32>(acc, C, (long)g * strideC, bias,
                               m_base, n_base, M, N, N, act, alpha, lane);
}

// ---- host side ---------------------------------------------------------
using GemmKernel = void (*)(const bf16*, const bf16*, void*, const float*,
                            int, int, int, long, long, long, int, float);

template <int BM, int BN, int BK>
GemmKernel generic_kernel(bool out_f32) {
  return out_f32 ? gemm_bf16_nt_kernel<BM, BN, BK, true>
                 : gemm_bf16_nt_kernel<BM, BN, BK, false>;
}

struct GemmTile {
  int bm, bn, bk;
  bool pipe;   // gemm_pipe64_kernel instead of the generic tile
};

// Tile heuristic. force is the INFOMESH_GEMM_TILE value (64 or 128
// forces that tile, anything else leaves the choice alone).
GemmTile pick_tile(int M, int N, int K, int batch, int force) {
  int bm = (M <= 64) ? 64 : 128, bn = 128;
  // Latency-bound regime: few K-steps and not enough 128^2 tiles to
  // fill the chip -> quarter tiles for 4x the block-level overlap.
  const long blocks128 =
      (long)((M + 127) / 128) * ((N + 127) / 128) * batch;
  if (bm == 128 && blocks128 < 512 && K <= 2048) bm = bn = 64;
  if (force == 64 && M > 64) bm = bn = 64;
  else if (force == 128) bm = bn = 128;
  // (BK=128 for the 64^2 tile was probe-tested and is ~60% SLOWER:
  // doubling LDS to 64 KB halves resident blocks per CU, which costs
  // more latency hiding than the halved K-step drains save.)
  const int bk = (K % 64 == 0) ? 64 : 32;
  // 64^2 with whole 64-deep K-steps: the 3-buffer glds-span pipeline
  return {bm, bn, bk, bm == 64 && bn == 64 && bk == 64};
}

GemmKernel tile_kernel(GemmTile t, bool out_f32) {
  if (t.pipe)
    return out_f32 ? gemm_pipe64_kernel<true> : gemm_pipe64_kernel<false>;
  if (t.bn == 64) return generic_kernel<64, 64, 32>(out_f32);
  if (t.bm == 64)
    return t.bk == 64 ? generic_kernel<64, 128, 64>(out_f32)
                      : generic_kernel<64, 128, 32>(out_f32);
  return t.bk == 64 ? generic_kernel<128, 128, 64>(out_f32)
                    : generic_kernel<128, 128, 32>(out_f32);
}

// Tuning override (read once): INFOMESH_GEMM_TILE=64|128 forces the
// tile; scripts/gemm_tile_probe.py uses it to validate the heuristic.
int tile_override() {
  static const int ov = [] {
    const char* e = getenv("INFOMESH_GEMM_TILE");
    return e ? atoi(e) : -1;
  }();
  return ov;
}

// The bmax variant always runs a generic tile with 128 columns, 64x128
// at M <= 64 and 128x128 above: pick_tile without its step down to the
// 64x64 tiles, which would need maxima instantiations of their own (and
// of the pipelined kernel) to serve planes of a few thousand documents,
// where the GEMM is microseconds either way. Every tile adds a score's
// K-steps in the same order, so the scores do not depend on the choice.
// bm == 0: not covered (the override forces 64x64).
GemmTile bmax_tile(int M, int K, int force) {
  if (force == 64 && M > 64) return {0, 0, 0, false};
  return {(M <= 64 && force != 128) ? 64 : 128, 128,
          (K % 64 == 0) ? 64 : 32, false};
}
// Columns per block maximum: the wave's column span BN / WN.
int bmax_width(GemmTile t) { return t.bm == 0 ? 0 : t.bm == 128 ? 64 : 32; }

template <int BM, int BK>
void launch_bmax(dim3 grid, hipStream_t s, const void* A, const void* B,
                 void* C, const void* bias, void* bmax, int M, int N, int K,
                 long strideA, long strideB, long strideC, int act,
                 float alpha) {
  hipLaunchKernelGGL((gemm_bf16_nt_kernel<BM, 128, BK, true, true, float*>),
                     grid, dim3(256), 0, s, (const bf16*)A, (const bf16*)B,
                     C, (const float*)bias, M, N, K, strideA, strideB,
                     strideC, act, alpha, (float*)bmax);
}

}  // namespace

// The tile infomesh_gemm_bf16_nt runs this shape on, packed as
// bm | bn << 8 | bk << 16 | pipe << 24 (tests pin their shapes to a
// kernel with it).
extern "C" int infomesh_gemm_tile(int M, int N, int K, int batch) {
  const GemmTile t = pick_tile(M, N, K, batch, tile_override());
  return t.bm | t.bn << 8 | t.bk << 16 | (int)t.pipe << 24;
}

extern "C" void infomesh_gemm_bf16_nt(
    const void* A, const void* B, void* C, const void* bias,
    int M, int N, int K, int batch,
    long strideA, long strideB, long strideC,
    int act, float alpha, int out_f32, void* stream) {
  const GemmTile t = pick_tile(M, N, K, batch, tile_override());
  const int tiles = ((M + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn);
  hipLaunchKernelGGL(tile_kernel(t, out_f32), dim3(tiles, batch), dim3(256),
                     0, reinterpret_cast<hipStream_t>(stream),
                     (const bf16*)A, (const bf16*)B, C, (const float*)bias,
                     M, N, K, strideA, strideB, strideC, act, alpha);
}

// Column span W of one block maximum of infomesh_gemm_bf16_nt_bmax at
// this shape (64 on the 128x128 tile, 32 on the 64x128 one), or 0 when
// the variant does not cover it. Callers size bmax by it:
// [batch, M, ceil(N / W)] f32.
extern "C" int infomesh_gemm_bmax_width(int M, int N, int K, int batch) {
  return bmax_width(bmax_tile(M, K, tile_override()));
}

// infomesh_gemm_bf16_nt with f32 output, plus the block maxima of every
// row (the BMAX instantiations, tile by bmax_tile). Same scores bit for
// bit. Returns 0, or 1 without launching when the width above is 0.
extern "C" int infomesh_gemm_bf16_nt_bmax(
    const void* A, const void* B, void* C, const void* bias, void* bmax,
    int M, int N, int K, int batch,
    long strideA, long strideB, long strideC,
    int act, float alpha, void* stream) {
  const GemmTile t = bmax_tile(M, K, tile_override());
  if (bmax_width(t) == 0) return 1;
  const dim3 grid(((M + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn), batch);
  auto* launch = t.bm == 128
      ? (t.bk == 64 ? launch_bmax<128, 64> : launch_bmax<128, 32>)
      : (t.bk == 64 ? launch_bmax<64, 64> : launch_bmax<64, 32>);
  launch(grid, reinterpret_cast<hipStream_t>(stream), A, B, C, bias, bmax,
         M, N, K, strideA, strideB, strideC, act, alpha);
  return 0;
}
