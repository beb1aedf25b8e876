// sim_rescore.h -- one row of A against rows of B with the similarity product's own contraction sequence: what score.hip's
// overflowing rows recompute with, and what screen.hip rescores its surviving candidates with.  The bits are sim_gemm_kernel's.
#pragma once
#include "common.h"
#include "topk_select.h"

namespace jmac {

// THE rescored value, in this order everywhere it is computed.  2 s is exact in fp32, so fma(2, s, -r1) and the unfused form round
// identically: the bits do not depend on the compiler's contraction choice.
__device__ __forceinline__ float csls_value(float s, float r1, float r2) { return 2.f * s - r1 - r2; }

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int SG_K = 16;                    // the product's k slab: the contraction order below is stated in it

// One 32 x 32 tile of the product with sim_gemm_kernel's contraction sequence per output element: four v_mfma_f32_32x32x2_f32 per
// (kt, q), planes k = 16 kt + 8 q + 4 h, clamped loads zeroed past d.  Lane (r = lane & 31, h = lane >> 5) supplies row r of
// both operands; ROW0: only tile row 0 carries A (one row of A against 32 rows of B), the rest is padding.
template <bool ROW0>
__device__ __forceinline__ f32x16 sim_tile_32x32(const float* __restrict__ arow, const float* __restrict__ brow, int d) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int nk = (d + SG_K - 1) / SG_K;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    for (int kt = 0; kt < nk; ++kt)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = kt * SG_K + 8 * q + 4 * h;
            float4 a4 = ld4(arow + min(k, d - 4)), b4 = ld4(brow + min(k, d - 4));
            if (k >= d) a4 = b4 = f4zero();
            if (ROW0 && r != 0) a4 = f4zero();
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
        }
    return acc;
}

// sim_tile_32x32<true>'s register 0 -- one row of A against 32 rows of B -- with the SAME MFMA sequence (step t = 2 kt + q, planes
// k = 8 t + 4 h, every step of every slab, zeros past d included), the loads of eight steps requested together: a caller with
// a handful of tiles per row (screen.hip's rescoring) waits for memory once per group instead of once per step.
__device__ __forceinline__ f32x16 sim_row_tile_grouped(const float* __restrict__ arow, const float* __restrict__ brow, int d) {
    constexpr int G = 8;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int steps = 2 * ((d + SG_K - 1) / SG_K);
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    for (int t0 = 0; t0 < steps; t0 += G) {
        float4 a4[G], b4[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int k = 8 * min(t0 + g, steps - 1) + 4 * h;
            a4[g] = ld4(arow + min(k, d - 4));
            b4[g] = ld4(brow + min(k, d - 4));
            if (k >= d) a4[g] = b4[g] = f4zero();
            if (r != 0) a4[g] = f4zero();
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (t0 + g < steps) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[g].x, b4[g].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[g].y, b4[g].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[g].z, b4[g].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[g].w, b4[g].w, acc, 0, 0, 0);
            }
    }
    return acc;
}

// c(i, gold[i]) of every row, from the product's own contraction sequence (sim_tile_32x32: v_mfma_f32_32x32x2_f32 over k in
// sim_gemm_kernel's order), so that the value carries the bits the tile kernel produces for that element -- the count epilogue's
// "equal, lower index first" test is then exact at the gold column itself.  One wave per 32 rows: row t of the MFMA tile is row t
// of A, column t the gold row of B; only the diagonal is kept.  Also presets rank[i] = 1.  The body of score.hip's csls_gold_kernel
// and screen.hip's screen_gold_kernel (blocks of TK_THREADS).
__device__ __forceinline__ void csls_gold_body(const float* __restrict__ A, int64_t lda, const float* __restrict__ Bm, int64_t ldb, int M,
                                               int d, const float* __restrict__ r1, const float* __restrict__ r2,
                                               const int32_t* __restrict__ gold, float* __restrict__ gval, int32_t* __restrict__ rank) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = (blockIdx.x * (TK_THREADS / 64) + wave) * 32;
    if (m0 >= M) return;                                       // wave-uniform
    const int m = min(m0 + r, M - 1), g = gold[m];
    const f32x16 acc = sim_tile_32x32<false>(A + (int64_t)m * lda, Bm + (int64_t)g * ldb, d);
    // C/D map: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  Element (t, t) lives in lane t + 32 ((t >> 2) & 1),
    // register (t & 3) + 4 (t >> 3): the lane whose r is t holds it iff its h matches
    if (h != ((r >> 2) & 1) || m0 + r >= M) return;
    const int want = (r & 3) + 4 * (r >> 3);
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) s = q == want ? acc[q] : s;
    gval[m] = r1 != nullptr ? csls_value(s, r1[m], r2[g]) : s;
    rank[m] = 1;
}

// f(n, s(row, n)) for every column n of the row, the block's TK_THREADS / 64 waves taking 32 columns each per step
template <class F>
__device__ __forceinline__ void for_each_row_score(const float* __restrict__ arow, const float* __restrict__ Bm, int64_t ldb, int N,
                                                   int d, F f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    for (int n0 = wave * 32; n0 < N; n0 += 32 * (TK_THREADS / 64)) {
        const f32x16 acc = sim_tile_32x32<true>(arow, Bm + (int64_t)min(n0 + r, N - 1) * ldb, d);
        if (h == 0 && n0 + r < N) f(n0 + r, acc[0]);           // C/D map: row 0 = register 0 of the lanes with h == 0
    }
}

}  // namespace jmac
