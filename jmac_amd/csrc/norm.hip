// norm.hip -- BatchNorm1d + tanh over [N,d] for gfx950 (replaces self.layer_act(self.bn(.)),
// src/jmac_model.py:52; nn.BatchNorm1d semantics: biased batch variance for normalisation, unbiased
// for the running estimate, eps inside the sqrt).
//
// HBM-bound streaming passes with 16 B per lane.  Column statistics use sums shifted by row 0 of the
// column (single pass, no catastrophic cancellation), reduced deterministically: per-block partial
// rows -> one finalising block.  No atomics.
#include <initializer_list>
#include <type_traits>

#include "common.h"

using namespace jmac;

namespace {

constexpr int kBlock = 256;
constexpr int kStatBlocks = 512;

// ---- plain and segmented forms.  Segmented: the rows are a stack of `nb` blocks (KGs of one launch set: the reference's training
// ---- step encodes two KGs per batch, src/jmac_model.py:325-326,263-264, each forward_base call with batch statistics of ITS rows).
// Every block has its own batch statistics (mean / invstd [nb, d]); weight, bias and the running estimates are the layer's
// (shared), and the running estimates are updated once per block in the callers' CALL order (seg.order), exactly what nb
// separate forward_base calls leave behind:  r <- (1-m)((1-m) r + m b_1) + m b_2 ...
// The plain form is the one-block case; every kernel below is one body for both, and the plain instantiation sees the constants
// (block 0, first row 0) that make the block arithmetic vanish.
constexpr int kMaxSeg = JMAC_BN_MAX_BLOCKS;
struct SegTab {
    int nb;
    int order[kMaxSeg];        // block processed k-th by the running-statistics update
    int gofs[kMaxSeg + 1];     // first statistics workgroup (= partial row) of each block
    int64_t ptr[kMaxSeg + 1];  // first row of each block; ptr[nb] = rows in all
};
template <bool SEG> using BnRows = std::conditional_t<SEG, SegTab, int64_t>;   // the plain kernels take the row count alone

__device__ __forceinline__ int seg_of_row(const SegTab& s, int64_t r) {
    int b = 0;
    for (int k = 1; k < s.nb; ++k) b += r >= s.ptr[k] ? 1 : 0;
    return b;
}
__device__ __forceinline__ int seg_of_group(const SegTab& s, int wg) {
    int b = 0;
    for (int k = 1; k < s.nb; ++k) b += wg >= s.gofs[k] ? 1 : 0;
    return b;
}

// one block as the statistics passes see it: its rows [r0, r1) and its statistics workgroups = partial rows [p0, p1)
struct StatBlock {
    int b;
    int64_t r0, r1;
    int p0, p1;
};
__device__ __forceinline__ StatBlock stat_block(const SegTab& s, int b) { return {b, s.ptr[b], s.ptr[b + 1], s.gofs[b], s.gofs[b + 1]}; }
// the block this workgroup of a partial pass works on
__device__ __forceinline__ StatBlock own_block(int64_t N) { return {0, 0, N, 0, (int)gridDim.x}; }
__device__ __forceinline__ StatBlock own_block(const SegTab& s) { return stat_block(s, seg_of_group(s, (int)blockIdx.x)); }

// ---- column sums: partial[wg][0][c], partial[wg][1][c] = two sums over the rows dealt to workgroup wg ------------------------
// The slots' sums, which the caller has put into red [2][rpb][D4], added in slot order -> this workgroup's two partial rows.
__device__ __forceinline__ void col_sums_fold(const float4* red, int rpb, int D4, float* __restrict__ partial) {
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < D4) {
        float4 a1 = red[tid], a2 = red[rpb * D4 + tid];
        for (int q = 1; q < rpb; ++q) {
            const float4 b1 = red[q * D4 + tid], b2 = red[(rpb + q) * D4 + tid];
            a1.x += b1.x; a1.y += b1.y; a1.z += b1.z; a1.w += b1.w;
            a2.x += b2.x; a2.y += b2.y; a2.z += b2.z; a2.w += b2.w;
        }
        st4(partial + ((int64_t)blockIdx.x * 2 + 0) * D4 * 4 + tid * 4, a1);
        st4(partial + ((int64_t)blockIdx.x * 2 + 1) * D4 * 4 + tid * 4, a2);
    }
}

// One workgroup's share of a column-sum pass over block `blk`: the block's rows are dealt to its workgroups round-robin in groups
// of rpb = kBlock / D4 rows, one row slot per group member; a slot sums its rows in row order (acc.row), the slots are added in
// slot order.  acc.column(c4, r0) gives what a slot keeps per column quad.  stat_smem(D4) bytes of LDS.
template <class Acc>
__device__ __forceinline__ void col_sums_block(const Acc& acc, const StatBlock& blk, int D4, float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4* red = reinterpret_cast<float4*>(smem);   // [2][rpb][D4]
    const int lb = (int)blockIdx.x - blk.p0, gb = blk.p1 - blk.p0;
    const int rpb = kBlock / D4 > 0 ? kBlock / D4 : 1;
    const int tid = threadIdx.x;
    // when D4 > kBlock a thread covers several column chunks
    for (int cbase = 0; cbase < D4; cbase += kBlock) {
        const int rsub = D4 >= kBlock ? 0 : tid / D4;
        const int c4 = D4 >= kBlock ? cbase + tid : tid % D4;
        const bool active = (D4 >= kBlock ? c4 < D4 : tid < rpb * D4);
        float4 s1 = f4zero(), s2 = f4zero();
        if (active) {
            const auto col = acc.column(c4, blk.r0);
            for (int64_t r = blk.r0 + (int64_t)lb * rpb + rsub; r < blk.r1; r += (int64_t)gb * rpb) acc.row(col, r, c4, s1, s2);
        }
        if (D4 >= kBlock) {
            if (active) {
                st4(partial + ((int64_t)blockIdx.x * 2 + 0) * D4 * 4 + c4 * 4, s1);
                st4(partial + ((int64_t)blockIdx.x * 2 + 1) * D4 * 4 + c4 * 4, s2);
            }
        } else {
            if (active) {
                red[(0 * rpb + rsub) * D4 + c4] = s1;
                red[(1 * rpb + rsub) * D4 + c4] = s2;
            }
            col_sums_fold(red, rpb, D4, partial);
            break;
        }
    }
}

// shifted statistics: s1 = sum_r (x[r][c]-K[c]),  s2 = sum_r (x[r][c]-K[c])^2,  K = the block's first row
struct ShiftedStatsAcc {
    const float* x;
    int64_t ldx;
    __device__ __forceinline__ float4 column(int c4, int64_t r0) const { return ld4(x + r0 * ldx + c4 * 4); }
    __device__ __forceinline__ void row(const float4& K, int64_t r, int c4, float4& s1, float4& s2) const {
        float4 v = ld4(x + r * ldx + c4 * 4);
        v.x -= K.x; v.y -= K.y; v.z -= K.z; v.w -= K.w;
        s1.x += v.x; s1.y += v.y; s1.z += v.z; s1.w += v.w;
        s2.x = fmaf(v.x, v.x, s2.x); s2.y = fmaf(v.y, v.y, s2.y); s2.z = fmaf(v.z, v.z, s2.z); s2.w = fmaf(v.w, v.w, s2.w);
    }
};
template <bool SEG>
__global__ __launch_bounds__(kBlock) void col_stats_partial_kernel(const float* __restrict__ x, int64_t ldx,
                                                                   BnRows<SEG> rows, int D4,
                                                                   float* __restrict__ partial) {
    col_sums_block(ShiftedStatsAcc{x, ldx}, own_block(rows), D4, partial);
}

// One element of the BatchNorm + tanh backward (gz = g (1 - y^2), xhat = (x - mean) invstd) with its contractions spelt out.  Every
// backward kernel -- plain, segmented, and fused with the normalise adjoint -- calls these two, so their launches agree bit for bit
// because they share this text; in particular both passes form gz the same way, so that a one-row batch gets the exact zero it must.
// FUSED_GZ, the segmented apply alone: gz is fused into the subtraction, fma(1 - y^2, g, -u), where the other kernels round gz first.
// A one-row block of that form therefore gets the rounding residue of gz instead of the zero.  Each form keeps its rounding: making
// them agree changes the results of one of them (profiles/bn_one_body.txt).
__device__ __forceinline__ void bn_bwd_sums_elem(float g, float y, float x, float mu, float is, float& s1, float& s2) {
#pragma clang fp contract(off)
    const float om = fmaf(-y, y, 1.f), gz = om * g;
    s1 = fmaf(om, g, s1);
    s2 = fmaf(gz, (x - mu) * is, s2);
}
template <bool FUSED_GZ = false>
__device__ __forceinline__ float bn_bwd_apply_elem(float g, float y, float x, float mu, float is, float w, float gw, float gb,
                                                   int training, float invn) {
#pragma clang fp contract(off)
    const float om = fmaf(-y, y, 1.f), gz = om * g;
    if (!training) return w * is * gz;
    const float u = invn * fmaf((x - mu) * is, gw, gb);
    return w * is * (FUSED_GZ ? fmaf(om, g, -u) : gz - u);
}

// backward column sums: s1 = sum gz, s2 = sum gz * xhat, gz = gy*(1-y^2); mean / invstd are the block's
struct BnBwdSumsAcc {
    const float *x, *y, *gy, *gy2;
    int64_t ldx, ldy, ldgy, ldgy2;
    const float *mean, *invstd;
    struct Col {
        float4 mu, is;
    };
    __device__ __forceinline__ Col column(int c4, int64_t) const { return {ld4(mean + c4 * 4), ld4(invstd + c4 * 4)}; }
    __device__ __forceinline__ void row(const Col& k, int64_t r, int c4, float4& s1, float4& s2) const {
        const float4 xv = ld4(x + r * ldx + c4 * 4), yv = ld4(y + r * ldy + c4 * 4);
        float4 g = ld4(gy + r * ldgy + c4 * 4);
        if (gy2) {                              // the output fed two consumers: their gradients are summed here
            const float4 g2 = ld4(gy2 + r * ldgy2 + c4 * 4);
            g.x += g2.x; g.y += g2.y; g.z += g2.z; g.w += g2.w;
        }
        bn_bwd_sums_elem(g.x, yv.x, xv.x, k.mu.x, k.is.x, s1.x, s2.x);
        bn_bwd_sums_elem(g.y, yv.y, xv.y, k.mu.y, k.is.y, s1.y, s2.y);
        bn_bwd_sums_elem(g.z, yv.z, xv.z, k.mu.z, k.is.z, s1.z, s2.z);
        bn_bwd_sums_elem(g.w, yv.w, xv.w, k.mu.w, k.is.w, s1.w, s2.w);
    }
};
template <bool SEG>
__global__ __launch_bounds__(kBlock) void bn_bwd_partial_kernel(const float* __restrict__ x, int64_t ldx,
                                                                const float* __restrict__ y, int64_t ldy,
                                                                const float* __restrict__ gy, int64_t ldgy,
                                                                const float* __restrict__ gy2, int64_t ldgy2,
                                                                BnRows<SEG> rows, int D4,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                float* __restrict__ partial) {
    const StatBlock blk = own_block(rows);
    const int64_t so = (int64_t)blk.b * D4 * 4;
    col_sums_block(BnBwdSumsAcc{x, y, gy, gy2, ldx, ldy, ldgy, ldgy2, mean + so, invstd + so}, blk, D4, partial);
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
// reduce_rows over the partial sums and the finalize in one launch: a workgroup owns 16 features; block after block in CALL order
// it sums both their s1 and s2 columns over the block's partial rows (64 row lanes each) and finalises the block's statistics,
// carrying the running estimates of its features through the blocks in registers.  `nparts`: the plain form's partial rows
constexpr int RF_COLS = 16, RF_LANES = 1024 / RF_COLS;
// One feature's statistics of one block from its shifted sums (K = the feature in the block's first row), and the step of the running
// estimates r <- (1-m) r + m b, with every contraction spelt out so that both instantiations and every compiler round alike.
// The running step alone differs between the forms: the plain form rounds both products, the segmented form fuses the first.  Each
// form keeps its rounding: making them agree changes the results of one of them (profiles/bn_one_body.txt).
template <bool SEG>
__device__ __forceinline__ void bn_finalize_elem(float s1, float s2, float K, int64_t nrow, float eps, float m, float& mean,
                                                 float& invstd, float& rm, float& rv) {
#pragma clang fp contract(off)
    const float n = (float)nrow;
    const float mshift = s1 / n;
    mean = K + mshift;
    float var = fmaf(-mshift, mshift, s2 / n);
    var = var > 0.f ? var : 0.f;
    invstd = rsqrtf(var + eps);
    const float unbiased = nrow > 1 ? var * n / (n - 1.f) : var;
    rm = SEG ? fmaf(1.f - m, rm, m * mean) : (1.f - m) * rm + m * mean;
    rv = SEG ? fmaf(1.f - m, rv, m * unbiased) : (1.f - m) * rv + m * unbiased;
}
template <bool SEG>
__global__ __launch_bounds__(1024) void bn_reduce_finalize_kernel(const float* __restrict__ partial, BnRows<SEG> rows,
                                                                  int nparts, const float* __restrict__ x, int64_t ldx, int d, float eps,
                                                                  float momentum, float* __restrict__ running_mean,
                                                                  float* __restrict__ running_var, float* __restrict__ save_mean,
                                                                  float* __restrict__ save_invstd) {
    __shared__ float red1[RF_LANES][RF_COLS], red2[RF_LANES][RF_COLS];
    const int cl = threadIdx.x % RF_COLS, rl = threadIdx.x / RF_COLS;
    const int c = blockIdx.x * RF_COLS + cl;
    float rm = 0.f, rv = 0.f;
    if (rl == 0 && c < d) {
        if (running_mean) rm = running_mean[c];
        if (running_var) rv = running_var[c];
    }
    int nb = 1;
    if constexpr (SEG) nb = rows.nb;
    for (int k = 0; k < nb; ++k) {
        StatBlock blk;
        if constexpr (SEG) blk = stat_block(rows, rows.order[k]);
        else blk = {0, 0, rows, 0, nparts};                     // the one block: all N rows, all `nparts` partial rows
        float a1 = 0.f, a2 = 0.f, b1 = 0.f, b2 = 0.f;
        if (c < d) {
            int p = blk.p0 + rl;
            for (; p + RF_LANES < blk.p1; p += 2 * RF_LANES) {
                a1 += partial[(int64_t)p * 2 * d + c];
                a2 += partial[(int64_t)p * 2 * d + d + c];
                b1 += partial[(int64_t)(p + RF_LANES) * 2 * d + c];
                b2 += partial[(int64_t)(p + RF_LANES) * 2 * d + d + c];
            }
            if (p < blk.p1) {
                a1 += partial[(int64_t)p * 2 * d + c];
                a2 += partial[(int64_t)p * 2 * d + d + c];
            }
        }
        red1[rl][cl] = a1 + b1;
        red2[rl][cl] = a2 + b2;
        __syncthreads();
        if (rl == 0 && c < d) {
            float s1 = red1[0][cl], s2 = red2[0][cl];
#pragma unroll 8
            for (int r = 1; r < RF_LANES; ++r) {
                s1 += red1[r][cl];
                s2 += red2[r][cl];
            }
            float mean, invstd;
            bn_finalize_elem<SEG>(s1, s2, x[blk.r0 * ldx + c], blk.r1 - blk.r0, eps, momentum, mean, invstd, rm, rv);
            save_mean[(int64_t)blk.b * d + c] = mean;
            save_invstd[(int64_t)blk.b * d + c] = invstd;
        }
        if (SEG) __syncthreads();              // red is written again for the next block
    }
    if (rl == 0 && c < d) {
        if (running_mean) running_mean[c] = rm;
        if (running_var) running_var[c] = rv;
    }
}

// local column moments from the shifted sums: mean = K + s1/n, M2 = sum (x - mean)^2 = s2 - s1^2/n
__global__ void moments_finalize_kernel(const float* __restrict__ sums, const float* __restrict__ x, int64_t N, int d,
                                        float* __restrict__ mean, float* __restrict__ m2) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= d) return;
    const float s1 = sums[c], s2 = sums[d + c], n = (float)N;
    mean[c] = x[c] + s1 / n;
    const float v = s2 - s1 * s1 / n;
    m2[c] = v > 0.f ? v : 0.f;
}

__global__ void bn_eval_stats_kernel(const float* __restrict__ running_mean, const float* __restrict__ running_var, int d,
                                     float eps, float* __restrict__ save_mean, float* __restrict__ save_invstd) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < d) {
        save_mean[c] = running_mean[c];
        save_invstd[c] = rsqrtf(running_var[c] + eps);
    }
}

// y = tanh((x - mean) invstd weight + bias), mean / invstd [blocks, d] those of the row's block
template <bool SEG>
__global__ __launch_bounds__(kBlock) void bn_tanh_apply_kernel(const float* __restrict__ x, int64_t ldx, BnRows<SEG> rows, int D4,
                                                               const float* __restrict__ weight, const float* __restrict__ bias,
                                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               float* __restrict__ y, int64_t ldy, float* __restrict__ y2,
                                                               int64_t ldy2) {
    int64_t total;
    if constexpr (SEG) total = rows.ptr[rows.nb] * D4;
    else total = rows * D4;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / D4;
        const int c4 = (int)(i % D4);
        int64_t so = 0;
        if constexpr (SEG) so = (int64_t)seg_of_row(rows, r) * D4 * 4;
        const float4 v = ld4(x + r * ldx + c4 * 4);
        const float4 mu = ld4(mean + so + c4 * 4), is = ld4(invstd + so + c4 * 4), w = ld4(weight + c4 * 4), b = ld4(bias + c4 * 4);
        float4 o;
        o.x = tanhf(fmaf((v.x - mu.x) * is.x, w.x, b.x));
        o.y = tanhf(fmaf((v.y - mu.y) * is.y, w.y, b.y));
        o.z = tanhf(fmaf((v.z - mu.z) * is.z, w.z, b.z));
        o.w = tanhf(fmaf((v.w - mu.w) * is.w, w.w, b.w));
        st4(y + r * ldy + c4 * 4, o);
        if (y2) st4(y2 + r * ldy2 + c4 * 4, o);         // the same rows into a second (strided) destination: a cat operand
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
__global__ void bn_bwd_finalize_kernel(const float* __restrict__ sums, int d, float* __restrict__ gweight,
                                       float* __restrict__ gbias) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= d) return;
    gbias[c] = sums[c];
    gweight[c] = sums[d + c];
}

// per-block sums of the backward partial rows -> bsums [nb, 2d] (sum gz | sum gz*xhat of each block) and their totals over
// the blocks in block order -> gbw [2d] = [grad bias | grad weight] (the parameters are shared by the blocks)
// Not merged with launch_reduce_rows: two accumulators per lane here, four there, a different association beyond 128 partial rows.
__global__ __launch_bounds__(1024) void bn_bwd_reduce_seg_kernel(const float* __restrict__ partial, SegTab seg, int W,
                                                                 float* __restrict__ bsums, float* __restrict__ gbias,
                                                                 float* __restrict__ gweight, int d) {
    __shared__ float red[RF_LANES][RF_COLS];
    const int cl = threadIdx.x % RF_COLS, rl = threadIdx.x / RF_COLS;
    const int c = blockIdx.x * RF_COLS + cl;
    float total = 0.f;
    for (int b = 0; b < seg.nb; ++b) {
        const int p0 = seg.gofs[b], p1 = seg.gofs[b + 1];
        float a0 = 0.f, a1 = 0.f;
        if (c < W) {
            int p = p0 + rl;
            for (; p + RF_LANES < p1; p += 2 * RF_LANES) {
                a0 += partial[(int64_t)p * W + c];
                a1 += partial[(int64_t)(p + RF_LANES) * W + c];
            }
            if (p < p1) a0 += partial[(int64_t)p * W + c];
        }
        red[rl][cl] = a0 + a1;
        __syncthreads();
        if (rl == 0 && c < W) {
            float s = red[0][cl];
#pragma unroll 8
            for (int r = 1; r < RF_LANES; ++r) s += red[r][cl];
            bsums[(int64_t)b * W + c] = s;
            total += s;
        }
        __syncthreads();
    }
    if (rl == 0 && c < W) {
        if (c < d) gbias[c] = total;
        else gweight[c - d] = total;
    }
}

// gx from the column sums of the row's block: sum gz at gbsum + b ldsum, sum gz * xhat at gwsum + b ldsum (plain: gbias, gweight;
// segmented: the two halves of a bsums row).  `training` and `invn` = 1 / (rows the statistics were taken over, which is not N where
// the batch spans ranks) are the plain form's; the segmented form is training-only and takes invn from its block
template <bool SEG>
__global__ __launch_bounds__(kBlock) void bn_bwd_apply_kernel(const float* __restrict__ x, int64_t ldx,
                                                              const float* __restrict__ y, int64_t ldy,
                                                              const float* __restrict__ gy, int64_t ldgy,
                                                              const float* __restrict__ gy2, int64_t ldgy2, BnRows<SEG> rows, int D4,
                                                              const float* __restrict__ weight, const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, const float* __restrict__ gwsum,
                                                              const float* __restrict__ gbsum, int64_t ldsum, int training,
                                                              float invn, float* __restrict__ gx, int64_t ldgx) {
    int64_t total;
    if constexpr (SEG) total = rows.ptr[rows.nb] * D4;
    else total = rows * D4;
    const int tr = SEG ? 1 : training;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / D4;
        const int c4 = (int)(i % D4);
        int b = 0;
        if constexpr (SEG) {
            b = seg_of_row(rows, r);
            invn = 1.f / (float)(rows.ptr[b + 1] - rows.ptr[b]);
        }
        const int64_t so = (int64_t)b * D4 * 4;
        const float4 xv = ld4(x + r * ldx + c4 * 4), yv = ld4(y + r * ldy + c4 * 4);
        float4 g = ld4(gy + r * ldgy + c4 * 4);
        if (gy2) {
            const float4 g2 = ld4(gy2 + r * ldgy2 + c4 * 4);
            g.x += g2.x; g.y += g2.y; g.z += g2.z; g.w += g2.w;
        }
        const float4 mu = ld4(mean + so + c4 * 4), is = ld4(invstd + so + c4 * 4), w = ld4(weight + c4 * 4);
        const float4 gw = ld4(gwsum + b * ldsum + c4 * 4), gb = ld4(gbsum + b * ldsum + c4 * 4);
        float4 o;
        o.x = bn_bwd_apply_elem<SEG>(g.x, yv.x, xv.x, mu.x, is.x, w.x, gw.x, gb.x, tr, invn);
        o.y = bn_bwd_apply_elem<SEG>(g.y, yv.y, xv.y, mu.y, is.y, w.y, gw.y, gb.y, tr, invn);
        o.z = bn_bwd_apply_elem<SEG>(g.z, yv.z, xv.z, mu.z, is.z, w.z, gw.z, gb.z, tr, invn);
        o.w = bn_bwd_apply_elem<SEG>(g.w, yv.w, xv.w, mu.w, is.w, w.w, gw.w, gb.w, tr, invn);
        st4(gx + r * ldgx + c4 * 4, o);
    }
}

inline unsigned stat_grid(int64_t N, int D4) {
    const int rpb = kBlock / D4 > 0 ? kBlock / D4 : 1;
    int64_t need = (N + rpb - 1) / rpb;
    if (need < 1) need = 1;
    return (unsigned)(need < kStatBlocks ? need : kStatBlocks);
}
inline size_t stat_smem(int D4) {
    const int rpb = kBlock / D4 > 0 ? kBlock / D4 : 1;
    return D4 >= kBlock ? 16 : (size_t)2 * rpb * D4 * 16;
}
inline unsigned stream_grid(int64_t total) {
    int64_t need = (total + kBlock - 1) / kBlock;
    if (need < 1) need = 1;
    return (unsigned)(need < 8192 ? need : 8192);
}

// ---- row L2 normalisation: y = x / max(||x||_2, eps)  (F.normalize(x, 2, -1), src/jmac_model.py:179,191,227-228) ------
// one wave per row, scalar lane layout (any d, any 4-byte-aligned leading dimension); inv[r] = 1 / max(||x_r||, eps).
__global__ __launch_bounds__(kBlock) void row_normalize_fwd_kernel(const float* __restrict__ x, int64_t ldx, int64_t N, int d,
                                                                   float eps, float* __restrict__ y, int64_t ldy,
                                                                   float* __restrict__ inv) {
    const int lane = lane_id();
    const int64_t w0 = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t r = w0; r < N; r += nw) {
        const float* xr = x + r * ldx;
        float ss = 0.f;
        for (int c = lane; c < d; c += 64) ss = fmaf(xr[c], xr[c], ss);
        ss = wave_sum(ss);
        const float iv = 1.f / fmaxf(sqrtf(ss), eps);
        for (int c = lane; c < d; c += 64) y[r * ldy + c] = xr[c] * iv;
        if (lane == 0) inv[r] = iv;
    }
}

// gx = inv * (g - y (g.y))   where the norm exceeds eps; gx = inv * g where it was clamped (constant denominator)
__global__ __launch_bounds__(kBlock) void row_normalize_bwd_kernel(const float* __restrict__ y, int64_t ldy,
                                                                   const float* __restrict__ g, int64_t ldg,
                                                                   const float* __restrict__ inv, int64_t N, int d, float eps,
                                                                   float* __restrict__ gx, int64_t ldgx) {
    const int lane = lane_id();
    const int64_t w0 = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t r = w0; r < N; r += nw) {
        const float* yr = y + r * ldy;
        const float* gr = g + r * ldg;
        float dot = 0.f;
        for (int c = lane; c < d; c += 64) dot = fmaf(gr[c], yr[c], dot);
        dot = wave_sum(dot);
        const float iv = inv[r];
        if (iv * eps >= 1.f) dot = 0.f;                // ||x|| <= eps: y = x / eps, no radial term
        for (int c = lane; c < d; c += 64) gx[r * ldgx + c] = iv * (gr[c] - yr[c] * dot);
    }
}

// ---- F.normalize followed by dropout (src/jmac_model.py:179,191: completion_dropout(F.normalize(.))), one pass each way --------
// y = x * inv * m  with m = mask * scale (mask: the caller's {0,1} draws; NULL = no dropout).  The backward recomputes the
// normalised row from x and inv (nothing but inv [N] is kept from the forward):
//   gn = g * m;  gx (+)= inv * (gn - xn (gn . xn)),  xn = x * inv   (no radial term on rows whose norm was clamped)
// 16 bytes per lane (d % 4 == 0, leading dimensions % 4 == 0).
// Dropout draws made in the kernel (SEED form): Philox4x32-10 keyed by the caller's device-resident seed, counter = index of
// the float4 (row * d/4 + column quad): its four words decide the four elements.  The backward regenerates the same draws, so
// no mask tensor is written or read (28 MB each way at DBP-5L size, plus the launch that drew it).  (philox4x32_10: common.h)
struct DropSrc {
    const float* mask;       // {0,1} draws of the caller, or NULL
    int64_t ldm;
    const int64_t* seed;     // SEED form: device int64
    uint32_t keep_thr;       // keep iff word < keep_thr  (keep probability = keep_thr / 2^32)
    float scale;
};
__device__ __forceinline__ uint2 drop_key(const DropSrc& ds, bool seeded) {
    if (!seeded) return make_uint2(0u, 0u);
    const uint64_t sd = (uint64_t)ds.seed[0];
    return make_uint2((uint32_t)sd, (uint32_t)(sd >> 32));
}
template <bool SEED>
__device__ __forceinline__ float4 drop_factors(const DropSrc& s, uint2 key, int64_t r, int c, int D4) {
    if (SEED) {
        const uint64_t idx = (uint64_t)r * (uint64_t)D4 + (uint64_t)c;
        const uint4 w = philox4x32_10(make_uint4((uint32_t)idx, (uint32_t)(idx >> 32), 0u, 0u), key);
        return make_float4(w.x < s.keep_thr ? s.scale : 0.f, w.y < s.keep_thr ? s.scale : 0.f, w.z < s.keep_thr ? s.scale : 0.f,
                           w.w < s.keep_thr ? s.scale : 0.f);
    }
    const float4 m = ld4(s.mask + r * s.ldm + c * 4);
    return make_float4(m.x * s.scale, m.y * s.scale, m.z * s.scale, m.w * s.scale);
}

// Where a lane stands: its wave among the grid's (kBlock / 64 per block; waves take rows or row groups w0, w0 + nw, ...) and, for
// the kernels that hold whole rows in registers (d <= 512), its two column quads cc[k] with ok[k] = inside the row.
struct WaveLanes {
    int lane;
    int64_t w0, nw;
    int cc[2];
    bool ok[2];
    __device__ __forceinline__ explicit WaveLanes(int D4)
        : lane(lane_id()), w0((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)), nw((int64_t)gridDim.x * (kBlock / 64)),
          cc{lane, lane + 64}, ok{cc[0] < D4, cc[1] < D4} {}
};

// The element arithmetic of every kernel of this group, one float4 at a time, each rounding spelt out (no contraction beyond the
// fmaf written here), so that kernels which call the same function round alike whatever the compiler would have chosen.
//   forward    ss = sumsq4 over the row;  y = mul4(scale4(x, inv), m)
//   backward   dot = adjoint_dot4 over the row (b = g m, rounded);  s = adjoint_combine4;  gx = adjoint_scale[_add]
// The adjoint has two forms, which the launches have always rounded differently (profiles/normalize_one_body.txt); each keeps its
// rounding, making them agree changes the results of one:
//   ROWFORM (R rows per wave, serving N >= kDropRowsMinN)   s = fma(-xn, dot, g m)      gx = inv s   accumulating: fma(inv, s, old)
//   otherwise (the row-per-wave kernels' form)              s = fma(m, g, -(xn dot)) with the draws made in the kernel (SEED),
//                                                           fma(-xn, dot, g m) with a mask or none
//                                                                                       gx = inv s   accumulating: inv s + old
__device__ __forceinline__ float sumsq4(float4 v, float acc) {
#pragma clang fp contract(off)
    return fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, acc))));
}
__device__ __forceinline__ float4 scale4(float4 v, float s) {
#pragma clang fp contract(off)
    return make_float4(v.x * s, v.y * s, v.z * s, v.w * s);
}
__device__ __forceinline__ float4 mul4(float4 a, float4 b) {
#pragma clang fp contract(off)
    return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
#pragma clang fp contract(off)
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
// acc + b . xn, xn = a inv
__device__ __forceinline__ float adjoint_dot4(float4 b, float4 a, float iv, float acc) {
#pragma clang fp contract(off)
    return fmaf(b.x, a.x * iv, fmaf(b.y, a.y * iv, fmaf(b.z, a.z * iv, fmaf(b.w, a.w * iv, acc))));
}
// FUSE_M: q = g, the factors m fused into the subtraction; otherwise q = g m, rounded (or g where nothing is dropped)
template <bool FUSE_M>
__device__ __forceinline__ float4 adjoint_combine4(float4 a, float iv, float dot, float4 q, const float4& m) {
#pragma clang fp contract(off)
    if (FUSE_M)
        return make_float4(fmaf(m.x, q.x, -(a.x * iv * dot)), fmaf(m.y, q.y, -(a.y * iv * dot)), fmaf(m.z, q.z, -(a.z * iv * dot)),
                           fmaf(m.w, q.w, -(a.w * iv * dot)));
    return make_float4(fmaf(-(a.x * iv), dot, q.x), fmaf(-(a.y * iv), dot, q.y), fmaf(-(a.z * iv), dot, q.z), fmaf(-(a.w * iv), dot, q.w));
}
// the adjoint's last factor, and the table an accumulating launch adds
__device__ __forceinline__ float4 adjoint_scale(float iv, float4 s) {
#pragma clang fp contract(off)
    return make_float4(iv * s.x, iv * s.y, iv * s.z, iv * s.w);
}
template <bool ROWFORM>
__device__ __forceinline__ float4 adjoint_scale_add(float iv, float4 s, float4 p) {
#pragma clang fp contract(off)
    if (ROWFORM) return make_float4(fmaf(iv, s.x, p.x), fmaf(iv, s.y, p.y), fmaf(iv, s.z, p.z), fmaf(iv, s.w, p.w));
    return make_float4(iv * s.x + p.x, iv * s.y + p.y, iv * s.z + p.z, iv * s.w + p.w);
}

// ---- one wave per row: any d, and every N below kDropRowsMinN.  A wave reads its row, reduces, reads it again and writes.
template <bool SEED>
__global__ __launch_bounds__(kBlock) void row_normalize_drop_fwd_kernel(const float* __restrict__ x, int64_t ldx, int64_t N, int D4,
                                                                        float eps, DropSrc ds, float* __restrict__ y, int64_t ldy,
                                                                        float* __restrict__ inv) {
    const WaveLanes L(D4);
    const uint2 key = drop_key(ds, SEED);
    const bool drop = SEED || ds.mask != nullptr;
    for (int64_t r = L.w0; r < N; r += L.nw) {
        const float* xr = x + r * ldx;
        float ss = 0.f;
        for (int c = L.lane; c < D4; c += 64) ss = sumsq4(ld4(xr + c * 4), ss);
        ss = wave_sum(ss);
        const float iv = 1.f / fmaxf(sqrtf(ss), eps);
        for (int c = L.lane; c < D4; c += 64) {
            float4 v = scale4(ld4(xr + c * 4), iv);
            if (drop) v = mul4(v, drop_factors<SEED>(ds, key, r, c, D4));
            st4(y + r * ldy + c * 4, v);
        }
        if (L.lane == 0) inv[r] = iv;
    }
}

template <bool SEED>
__global__ __launch_bounds__(kBlock) void row_normalize_drop_bwd_kernel(const float* __restrict__ x, int64_t ldx,
                                                                        const float* __restrict__ inv, DropSrc ds,
                                                                        const float* __restrict__ g, int64_t ldg, int64_t N, int D4,
                                                                        float eps, float* __restrict__ gx, int64_t ldgx,
                                                                        int accumulate) {
    const WaveLanes L(D4);
    const uint2 key = drop_key(ds, SEED);
    const bool drop = SEED || ds.mask != nullptr;
    for (int64_t r = L.w0; r < N; r += L.nw) {
        const float* xr = x + r * ldx;
        const float* gr = g + r * ldg;
        const float iv = inv[r];
        float dot = 0.f;
        for (int c = L.lane; c < D4; c += 64) {
            float4 q = ld4(gr + c * 4);
            if (drop) q = mul4(q, drop_factors<SEED>(ds, key, r, c, D4));
            dot = adjoint_dot4(q, ld4(xr + c * 4), iv, dot);
        }
        dot = wave_sum(dot);
        if (iv * eps >= 1.f) dot = 0.f;                // ||x|| <= eps: y = x / eps, no radial term
        for (int c = L.lane; c < D4; c += 64) {
            float4 q = ld4(gr + c * 4), m = f4zero();
            if (drop) m = drop_factors<SEED>(ds, key, r, c, D4);
            if (drop && !SEED) q = mul4(q, m);
            float4 o = adjoint_scale(iv, adjoint_combine4<SEED>(ld4(xr + c * 4), iv, dot, q, m));
            if (accumulate) o = add4(o, ld4(gx + r * ldgx + c * 4));
            st4(gx + r * ldgx + c * 4, o);
        }
    }
}

// ---- R rows per wave in flight (rows of up to 128 float4: d <= 512) -------------------------------------------------------------
// The kernels above give every row a wave that makes two dependent round trips per row and (backward) two Philox evaluations per
// element; at DBP-5L size (11 805 rows x 300) they move 28-56 MB at 2.2 TB/s.  Here a wave keeps R rows in registers (two float4 per
// lane and row), issues all their loads before the first reduction (interleaved DPP chains: wave_sum_n) and writes from registers.
// Per-lane summation order as above.  One body per pass -- normalize_drop_store_rows forward, normalize_drop_adjoint_rows backward --
// serves the plain launches (PLAIN: drop_fwd / drop_bwd from kDropRowsMinN rows on; dropout from a mask, a seed or none) and the
// fused row passes of the encoder node's completion chain (jmac_amd/encoder.py, FUSE_ROW_PASSES; dropout from a seed or none).
// The node runs its entities in class order (a row permutation) and normalises + drops what it hands from layer to layer; run as
// separate launches, four of those passes only re-read a [N, d] table the launch before has just written.  The fused forms take an
// optional int64 row map `map` (class-order row -> caller's row; entries in [0, N)):
//   rows_normalize_drop_fwd      x[map[r]] -> a copy in class order, normalise + dropout, inv          (gather + normalise)
//   bn_tanh_normalize_drop_fwd   BatchNorm apply + tanh -> y[r], y[map[r]], normalise + dropout of the row in registers, inv
//   bn_bwd_{partial,apply}_adj   BatchNorm + tanh backward whose incoming gradient is the normalise/dropout ADJOINT of g, formed per
//                                row from y (the adjoint's x), inv and the draws -- never stored; gy2 read as gy2[map[r]]
//                                (the partial pass deals rows to waves as bn_bwd_partial_kernel deals them to threads: same sums)
//   row_normalize_drop_bwd_scatter   the adjoint + add[r], stored (or accumulated) to dst[map[r]]       (adjoint + scatter)
// The Philox index stays (class-order row, chunk).  A fused launch takes the adjoint's form (ROWFORM, above) of the separate launch
// of its row count, and the BatchNorm backward's column sums keep their association: the bits of the separate launches.
constexpr int kDropRows = 4;             // rows per wave of the plain launches
constexpr int64_t kDropRowsMinN = 2048;  // below this the one-row-per-wave kernels have more waves to hide latency with
constexpr int kFuseRows = 4;             // rows per wave of the fused passes: one or two tables in flight
constexpr int kFuseBwdRows = 2;          // ... four tables in flight

// normalise + dropout of R rows held in registers (v: zero on lanes past the row) -> y rows, inv; rows r0 + u >= N are skipped.
// MASK: ds.mask may be set (the plain launches alone: the test for it costs the fused forms registers)
template <bool SEED, bool MASK, int R>
__device__ __forceinline__ void normalize_drop_store_rows(const DropSrc& ds, uint2 key, int64_t r0, int64_t N, int D4, const WaveLanes& L,
                                                          float eps, const float4 (&v)[R][2], float* __restrict__ y, int64_t ldy,
                                                          float* __restrict__ inv) {
    const bool drop = SEED || (MASK && ds.mask != nullptr);
    float ss[R];
#pragma unroll
    for (int u = 0; u < R; ++u) ss[u] = sumsq4(v[u][1], sumsq4(v[u][0], 0.f));
    wave_sum_n<R>(ss);
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const int64_t r = r0 + u;
        if (r >= N) break;                                     // wave-uniform
        const float iv = 1.f / fmaxf(sqrtf(ss[u]), eps);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!L.ok[k]) continue;
            float4 q = scale4(v[u][k], iv);
            if (drop) q = mul4(q, drop_factors<SEED>(ds, key, r, L.cc[k], D4));
            st4(y + r * ldy + L.cc[k] * 4, q);
        }
        if (L.lane == 0) inv[r] = iv;
    }
}

// q <- the normalise/dropout adjoint of R rows held in registers, up to its last factor inv (adjoint_scale[_add]); row[u]: their
// class-order rows, for the draws; v and q come back zero on lanes past the row.  ROWFORM, MASK: see above.
template <bool SEED, bool ROWFORM, bool MASK, int R>
__device__ __forceinline__ void normalize_drop_adjoint_rows(const DropSrc& ds, uint2 key, const int64_t (&row)[R], int D4,
                                                            const WaveLanes& L, float eps, const float (&iv)[R], float4 (&v)[R][2],
                                                            float4 (&q)[R][2]) {
    constexpr bool FUSE_M = SEED && !ROWFORM;
    const bool drop = SEED || (MASK && ds.mask != nullptr);
    float dot[R];
    float4 m[R][2];
#pragma unroll
    for (int u = 0; u < R; ++u) {
        dot[u] = 0.f;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            float4 b = q[u][k];
            if (!L.ok[k]) {
                b = q[u][k] = f4zero();
                v[u][k] = f4zero();
            } else if (drop) {
                m[u][k] = drop_factors<SEED>(ds, key, row[u], L.cc[k], D4);
                b = mul4(b, m[u][k]);
                if (!FUSE_M) q[u][k] = b;
            }
            dot[u] = adjoint_dot4(b, v[u][k], iv[u], dot[u]);
        }
    }
    wave_sum_n<R>(dot);
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const float d_ = iv[u] * eps >= 1.f ? 0.f : dot[u];       // ||x|| <= eps: y = x / eps, no radial term
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (L.ok[k]) q[u][k] = adjoint_combine4<FUSE_M>(v[u][k], iv[u], d_, q[u][k], m[u][k]);
    }
}

// PLAIN: the plain launch -- no row map, no copy (map and xr are not read), dropout from a mask too
template <bool SEED, bool PLAIN, int R>
__global__ __launch_bounds__(kBlock) void rows_normalize_drop_fwd_kernel(const float* __restrict__ x, int64_t ldx,
                                                                         const int64_t* __restrict__ map, int64_t N, int D4, float eps,
                                                                         DropSrc ds, float* __restrict__ xr, int64_t ldxr,
                                                                         float* __restrict__ y, int64_t ldy, float* __restrict__ inv) {
    const WaveLanes L(D4);
    const uint2 key = drop_key(ds, SEED);
    for (int64_t r0 = L.w0 * R; r0 < N; r0 += L.nw * R) {
        float4 v[R][2];
        int64_t s[R];
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int64_t r = r0 + u < N ? r0 + u : N - 1;
            s[u] = !PLAIN && map ? map[r] : r;
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
#pragma unroll
            for (int k = 0; k < 2; ++k) v[u][k] = ld4(x + s[u] * ldx + (L.ok[k] ? L.cc[k] : 0) * 4);
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!L.ok[k]) v[u][k] = f4zero();
                else if (!PLAIN && xr && r0 + u < N) st4(xr + (r0 + u) * ldxr + L.cc[k] * 4, v[u][k]);
            }
        }
        normalize_drop_store_rows<SEED, PLAIN, R>(ds, key, r0, N, D4, L, eps, v, y, ldy, inv);
    }
}

template <bool SEED, int R>
__global__ __launch_bounds__(kBlock) void bn_tanh_normalize_drop_fwd_kernel(const float* __restrict__ x, int64_t ldx, int64_t N, int D4,
                                                                            const float* __restrict__ weight, const float* __restrict__ bias,
                                                                            const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                            float* __restrict__ y, int64_t ldy,
                                                                            const int64_t* __restrict__ map, float* __restrict__ yr,
                                                                            int64_t ldyr, float eps, DropSrc ds, float* __restrict__ yn,
                                                                            int64_t ldyn, float* __restrict__ inv) {
    const WaveLanes L(D4);
    const uint2 key = drop_key(ds, SEED);
    float4 mu[2], is[2], w[2], b[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = (L.ok[k] ? L.cc[k] : 0) * 4;
        mu[k] = ld4(mean + c); is[k] = ld4(invstd + c); w[k] = ld4(weight + c); b[k] = ld4(bias + c);
    }
    for (int64_t r0 = L.w0 * R; r0 < N; r0 += L.nw * R) {
        float4 v[R][2];
        int64_t s[R];
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int64_t r = r0 + u < N ? r0 + u : N - 1;
            s[u] = map ? map[r] : r;
#pragma unroll
            for (int k = 0; k < 2; ++k) v[u][k] = ld4(x + r * ldx + (L.ok[k] ? L.cc[k] : 0) * 4);
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!L.ok[k]) {
                    v[u][k] = f4zero();
                    continue;
                }
                float4 o;
                o.x = tanhf(fmaf((v[u][k].x - mu[k].x) * is[k].x, w[k].x, b[k].x));
                o.y = tanhf(fmaf((v[u][k].y - mu[k].y) * is[k].y, w[k].y, b[k].y));
                o.z = tanhf(fmaf((v[u][k].z - mu[k].z) * is[k].z, w[k].z, b[k].z));
                o.w = tanhf(fmaf((v[u][k].w - mu[k].w) * is[k].w, w[k].w, b[k].w));
                v[u][k] = o;
                if (r0 + u < N) {
                    st4(y + (r0 + u) * ldy + L.cc[k] * 4, o);
                    if (yr) st4(yr + s[u] * ldyr + L.cc[k] * 4, o);   // the same row at its place in the caller's order
                }
            }
        }
        normalize_drop_store_rows<SEED, false, R>(ds, key, r0, N, D4, L, eps, v, yn, ldyn, inv);
    }
}

// The column sums keep bn_bwd_partial_kernel's association, so that gweight / gbias (and with them gx) come out bit for bit: a block
// owns the rows that kernel's block owns -- rpb = kBlock / D4 row slots, slot `rsub` of block b holding rows (b rpb + rsub) + k (grid
// rpb), k = 0, 1, ... summed in that order -- a wave takes the slots wave, wave + waves, ... one after the other (R consecutive k in
// flight), and the slots are added in slot order at the end.  Launched with 64 min(rpb, 4) threads (>= D4) and stat_smem(D4) bytes.
template <bool SEED, bool ROWFORM, int R>
__global__ __launch_bounds__(kBlock) void bn_bwd_partial_adj_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ y,
                                                                    int64_t ldy, const float* __restrict__ g, int64_t ldg,
                                                                    const float* __restrict__ inv, DropSrc ds, float eps,
                                                                    const float* __restrict__ gy2, int64_t ldgy2,
                                                                    const int64_t* __restrict__ map, int64_t N, int D4,
                                                                    const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                    float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4* red = reinterpret_cast<float4*>(smem);   // [2][rpb][D4]
    const int rpb = kBlock / D4;                      // >= 2 (D4 <= 128)
    const WaveLanes L(D4);
    const int wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    const uint2 key = drop_key(ds, SEED);
    float4 mu[2], is[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = (L.ok[k] ? L.cc[k] : 0) * 4;
        mu[k] = ld4(mean + c); is[k] = ld4(invstd + c);
    }
    const int64_t stride = (int64_t)gridDim.x * rpb;
    for (int rsub = wv; rsub < rpb; rsub += nwv) {
        float4 s1[2] = {f4zero(), f4zero()}, s2[2] = {f4zero(), f4zero()};
        for (int64_t rb = (int64_t)blockIdx.x * rpb + rsub; rb < N; rb += stride * R) {
            float4 xv[R][2], yv[R][2], q[R][2], g2[R][2];
            float iv[R];
            int64_t row[R], s[R];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                row[u] = rb + u * stride < N ? rb + u * stride : N - 1;
                s[u] = map ? map[row[u]] : row[u];
            }
#pragma unroll
            for (int u = 0; u < R; ++u) {
                iv[u] = inv[row[u]];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int c = (L.ok[k] ? L.cc[k] : 0) * 4;
                    xv[u][k] = ld4(x + row[u] * ldx + c);
                    yv[u][k] = ld4(y + row[u] * ldy + c);
                    q[u][k] = ld4(g + row[u] * ldg + c);
                    if (gy2) g2[u][k] = ld4(gy2 + s[u] * ldgy2 + c);
                }
            }
            normalize_drop_adjoint_rows<SEED, ROWFORM, false, R>(ds, key, row, D4, L, eps, iv, yv, q);
#pragma unroll
            for (int u = 0; u < R; ++u) {
                if (rb + u * stride >= N) break;                   // wave-uniform
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    if (!L.ok[k]) continue;
                    float4 gg = adjoint_scale(iv[u], q[u][k]);
                    if (gy2) gg = add4(gg, g2[u][k]);
                    const float4 yy = yv[u][k], xx = xv[u][k];
                    bn_bwd_sums_elem(gg.x, yy.x, xx.x, mu[k].x, is[k].x, s1[k].x, s2[k].x);
                    bn_bwd_sums_elem(gg.y, yy.y, xx.y, mu[k].y, is[k].y, s1[k].y, s2[k].y);
                    bn_bwd_sums_elem(gg.z, yy.z, xx.z, mu[k].z, is[k].z, s1[k].z, s2[k].z);
                    bn_bwd_sums_elem(gg.w, yy.w, xx.w, mu[k].w, is[k].w, s1[k].w, s2[k].w);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (L.ok[k]) {
                red[(0 * rpb + rsub) * D4 + L.cc[k]] = s1[k];
                red[(1 * rpb + rsub) * D4 + L.cc[k]] = s2[k];
            }
        }
    }
    col_sums_fold(red, rpb, D4, partial);
}

template <bool SEED, bool ROWFORM, int R>
__global__ __launch_bounds__(kBlock) void bn_bwd_apply_adj_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ y,
                                                                  int64_t ldy, const float* __restrict__ g, int64_t ldg,
                                                                  const float* __restrict__ inv, DropSrc ds, float eps,
                                                                  const float* __restrict__ gy2, int64_t ldgy2,
                                                                  const int64_t* __restrict__ map, int64_t N, int D4,
                                                                  const float* __restrict__ weight, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, const float* __restrict__ gweight,
                                                                  const float* __restrict__ gbias, int training, float invn,
                                                                  float* __restrict__ gx, int64_t ldgx) {
    const WaveLanes L(D4);
    const uint2 key = drop_key(ds, SEED);
    float4 mu[2], is[2], w[2], gw[2], gb[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = (L.ok[k] ? L.cc[k] : 0) * 4;
        mu[k] = ld4(mean + c); is[k] = ld4(invstd + c); w[k] = ld4(weight + c);
        gw[k] = training ? ld4(gweight + c) : f4zero(); gb[k] = training ? ld4(gbias + c) : f4zero();
    }
    for (int64_t r0 = L.w0 * R; r0 < N; r0 += L.nw * R) {
        float4 xv[R][2], yv[R][2], q[R][2], g2[R][2];
        float iv[R];
        int64_t row[R], s[R];
#pragma unroll
        for (int u = 0; u < R; ++u) {
            row[u] = r0 + u < N ? r0 + u : N - 1;
            s[u] = map ? map[row[u]] : row[u];
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
            iv[u] = inv[row[u]];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int c = (L.ok[k] ? L.cc[k] : 0) * 4;
                xv[u][k] = ld4(x + row[u] * ldx + c);
                yv[u][k] = ld4(y + row[u] * ldy + c);
                q[u][k] = ld4(g + row[u] * ldg + c);
                if (gy2) g2[u][k] = ld4(gy2 + s[u] * ldgy2 + c);
            }
        }
        normalize_drop_adjoint_rows<SEED, ROWFORM, false, R>(ds, key, row, D4, L, eps, iv, yv, q);
#pragma unroll
        for (int u = 0; u < R; ++u) {
            if (r0 + u >= N) break;                                // wave-uniform
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!L.ok[k]) continue;
                float4 gg = adjoint_scale(iv[u], q[u][k]);
                if (gy2) gg = add4(gg, g2[u][k]);
                const float4 yy = yv[u][k], xx = xv[u][k];
                float4 o;
                o.x = bn_bwd_apply_elem(gg.x, yy.x, xx.x, mu[k].x, is[k].x, w[k].x, gw[k].x, gb[k].x, training, invn);
                o.y = bn_bwd_apply_elem(gg.y, yy.y, xx.y, mu[k].y, is[k].y, w[k].y, gw[k].y, gb[k].y, training, invn);
                o.z = bn_bwd_apply_elem(gg.z, yy.z, xx.z, mu[k].z, is[k].z, w[k].z, gw[k].z, gb[k].z, training, invn);
                o.w = bn_bwd_apply_elem(gg.w, yy.w, xx.w, mu[k].w, is[k].w, w[k].w, gw[k].w, gb[k].w, training, invn);
                st4(gx + (r0 + u) * ldgx + L.cc[k] * 4, o);
            }
        }
    }
}

// PLAIN: the plain launch -- the row map is not read, dropout may come from a mask, and an accumulating launch passes its
// destination as `add` with accumulate = 0 (gx += adjoint is fma(inv, s, old), the add table's rounding): one table less in flight.
// There add and dst are the same memory, so neither is __restrict__ in that instantiation.
template <bool ALIASED, class T> using MaybeAliased = std::conditional_t<ALIASED, T*, T* __restrict__>;
template <bool SEED, bool ROWFORM, bool PLAIN, int R>
__global__ __launch_bounds__(kBlock) void row_normalize_drop_bwd_scatter_kernel(const float* __restrict__ x, int64_t ldx,
                                                                                const float* __restrict__ inv, DropSrc ds,
                                                                                const float* __restrict__ g, int64_t ldg,
                                                                                MaybeAliased<PLAIN, const float> add, int64_t ldadd,
                                                                                const int64_t* __restrict__ map, int64_t N, int D4,
                                                                                float eps, MaybeAliased<PLAIN, float> dst, int64_t lddst,
                                                                                int accumulate) {
    const WaveLanes L(D4);
    const uint2 key = drop_key(ds, SEED);
    const bool onto = !PLAIN && accumulate;
    for (int64_t r0 = L.w0 * R; r0 < N; r0 += L.nw * R) {
        float4 v[R][2], q[R][2], p[R][2], old[R][2];
        float iv[R];
        int64_t row[R], s[R];
#pragma unroll
        for (int u = 0; u < R; ++u) {
            row[u] = r0 + u < N ? r0 + u : N - 1;
            s[u] = !PLAIN && map ? map[row[u]] : row[u];
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
            iv[u] = inv[row[u]];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int c = (L.ok[k] ? L.cc[k] : 0) * 4;
                v[u][k] = ld4(x + row[u] * ldx + c);
                q[u][k] = ld4(g + row[u] * ldg + c);
                if (add) p[u][k] = ld4(add + row[u] * ldadd + c);
                if (onto) old[u][k] = ld4(dst + s[u] * lddst + c);
            }
        }
        normalize_drop_adjoint_rows<SEED, ROWFORM, PLAIN, R>(ds, key, row, D4, L, eps, iv, v, q);
#pragma unroll
        for (int u = 0; u < R; ++u) {
            if (r0 + u >= N) break;                                // wave-uniform
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!L.ok[k]) continue;
                float4 o = add ? adjoint_scale_add<ROWFORM>(iv[u], q[u][k], p[u][k]) : adjoint_scale(iv[u], q[u][k]);
                if (onto) o = add4(o, old[u][k]);
                st4(dst + s[u] * lddst + L.cc[k] * 4, o);
            }
        }
    }
}

inline unsigned rows_grid(int64_t N, int R) {                      // a wave per R rows, kBlock / 64 waves per block
    const int64_t rb = ((N + R - 1) / R + kBlock / 64 - 1) / (kBlock / 64);
    return (unsigned)(rb > 8192 ? 8192 : rb);
}
// f(SEED, ROWFORM) with the two as std::bool_constant values, so that a generic lambda names its kernel's instantiation by them
template <class F>
inline void with_drop_form(bool seeded, bool rowform, F&& f) {
    if (seeded && rowform) f(std::true_type{}, std::true_type{});
    else if (seeded) f(std::true_type{}, std::false_type{});
    else if (rowform) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
}

}  // namespace

extern "C" {

size_t jmac_bn_tanh_workspace_bytes(int64_t N, int64_t d) {
    (void)N;
    return align_up((size_t)(kStatBlocks + 1) * 2 * (d > 0 ? d : 0) * 4) + 256;
}

// the forward's statistics into save_mean / save_invstd: training = the batch's (partial sums -> reduce + finalize, which also
// updates the running estimates), else the running estimates'
static int launch_bn_fwd_stats(const float* x, int64_t ldx, int64_t N, int64_t d, float* running_mean, float* running_var,
                               int32_t training, float momentum, float eps, float* save_mean, float* save_invstd, void* ws,
                               size_t ws_bytes, hipStream_t st) {
    if (training) {
        if (!ws || ws_bytes < jmac_bn_tanh_workspace_bytes(N, d)) return JMAC_EWORKSPACE;
        const int D4 = (int)(d / 4);
        float* partial = (float*)ws;
        const unsigned g = stat_grid(N, D4);
        hipLaunchKernelGGL(col_stats_partial_kernel<false>, dim3(g), dim3(kBlock), stat_smem(D4), st, x, ldx, N, D4, partial);
        hipLaunchKernelGGL(bn_reduce_finalize_kernel<false>, dim3((unsigned)((d + RF_COLS - 1) / RF_COLS)), dim3(1024), 0, st, partial,
                           N, (int)g, x, ldx, (int)d, eps, momentum, running_mean, running_var, save_mean, save_invstd);
    } else {
        if (!running_mean || !running_var) return JMAC_EINVAL;
        hipLaunchKernelGGL(bn_eval_stats_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, running_mean, running_var,
                           (int)d, eps, save_mean, save_invstd);
    }
    return JMAC_OK;
}

// the backward's partial rows [g, 2d] summed into gbias and gweight
static void launch_bn_bwd_param_grads(float* partial, unsigned g, int64_t d, float* gweight, float* gbias, hipStream_t st) {
    if (gweight == gbias + d) {                  // [gbias | gweight] contiguous: the reduction writes them directly
        launch_reduce_rows(partial, (int)g, (int)(2 * d), 1.f, gbias, st);
    } else {
        float* sums = partial + (size_t)kStatBlocks * 2 * d;
        launch_reduce_rows(partial, (int)g, (int)(2 * d), 1.f, sums, st);
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, sums, (int)d, gweight, gbias);
    }
}

int jmac_bn_tanh_fwd2_f32(const float* x, int64_t ldx, int64_t N, int64_t d, const float* weight, const float* bias,
                          float* running_mean, float* running_var, int32_t training, float momentum, float eps, float* y,
                          int64_t ldy, float* y2, int64_t ldy2, float* save_mean, float* save_invstd, void* ws, size_t ws_bytes,
                          jmac_stream_t stream) {
    if (N < 0 || !weight || !bias || !save_mean || !save_invstd) return JMAC_EINVAL;
    if (d <= 0 || d % 4 || ldx % 4 || ldy % 4 || (y2 && ldy2 % 4)) return JMAC_EDIM;
    if (N == 0) return JMAC_OK;
    if (!x || !y) return JMAC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int D4 = (int)(d / 4);
    if (int rc = launch_bn_fwd_stats(x, ldx, N, d, running_mean, running_var, training, momentum, eps, save_mean, save_invstd, ws,
                                     ws_bytes, st))
        return rc;
    hipLaunchKernelGGL(bn_tanh_apply_kernel<false>, dim3(stream_grid(N * D4)), dim3(kBlock), 0, st, x, ldx, N, D4, weight, bias,
                       (const float*)save_mean, (const float*)save_invstd, y, ldy, y2, ldy2);
    return (int)hipGetLastError();
}

int jmac_bn_tanh_bwd2_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* gy, int64_t ldgy,
                          const float* gy2, int64_t ldgy2, int64_t N, int64_t d, const float* weight, const float* save_mean,
                          const float* save_invstd, int32_t training, float* gx, int64_t ldgx, float* gweight, float* gbias,
                          void* ws, size_t ws_bytes, jmac_stream_t stream) {
    if (N < 0 || !weight || !save_mean || !save_invstd || !gweight || !gbias) return JMAC_EINVAL;
    if (d <= 0 || d % 4 || ldx % 4 || ldy % 4 || ldgy % 4 || ldgx % 4 || (gy2 && ldgy2 % 4)) return JMAC_EDIM;
    if (!ws || ws_bytes < jmac_bn_tanh_workspace_bytes(N, d)) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int D4 = (int)(d / 4);
    float* partial = (float*)ws;
    unsigned g = 0;
    if (N > 0) {
        if (!x || !y || !gy || !gx) return JMAC_EINVAL;
        g = stat_grid(N, D4);
        hipLaunchKernelGGL(bn_bwd_partial_kernel<false>, dim3(g), dim3(kBlock), stat_smem(D4), st, x, ldx, y, ldy, gy, ldgy, gy2, ldgy2,
                           N, D4, save_mean, save_invstd, partial);
    }
    launch_bn_bwd_param_grads(partial, g, d, gweight, gbias, st);
    if (N > 0)
        hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, dim3(stream_grid(N * D4)), dim3(kBlock), 0, st, x, ldx, y, ldy, gy, ldgy, gy2,
                           ldgy2, N, D4, weight, save_mean, save_invstd, (const float*)gweight, (const float*)gbias, (int64_t)0, training,
                           1.f / (float)N, gx, ldgx);
    return (int)hipGetLastError();
}

int jmac_row_normalize_fwd_f32(const float* x, int64_t ldx, int64_t N, int64_t d, float eps, float* y, int64_t ldy, float* inv,
                               jmac_stream_t stream) {
    if (N < 0 || d <= 0 || d >= INT32_MAX) return JMAC_EINVAL;
    if (N == 0) return JMAC_OK;
    if (!x || !y || !inv) return JMAC_EINVAL;
    hipLaunchKernelGGL(row_normalize_fwd_kernel, dim3(rows_grid(N, 1)), dim3(kBlock), 0, (hipStream_t)stream, x, ldx, N, (int)d, eps,
                       y, ldy, inv);
    return (int)hipGetLastError();
}

int jmac_row_normalize_bwd_f32(const float* y, int64_t ldy, const float* g, int64_t ldg, const float* inv, int64_t N, int64_t d,
                               float eps, float* gx, int64_t ldgx, jmac_stream_t stream) {
    if (N < 0 || d <= 0 || d >= INT32_MAX) return JMAC_EINVAL;
    if (N == 0) return JMAC_OK;
    if (!y || !g || !inv || !gx) return JMAC_EINVAL;
    hipLaunchKernelGGL(row_normalize_bwd_kernel, dim3(rows_grid(N, 1)), dim3(kBlock), 0, (hipStream_t)stream, y, ldy, g, ldg, inv, N,
                       (int)d, eps, gx, ldgx);
    return (int)hipGetLastError();
}

// the plain launches: from kDropRowsMinN rows of up to 512 columns on, the R-rows bodies (PLAIN); else a wave per row
static int drop_fwd(const float* x, int64_t ldx, int64_t N, int64_t d, float eps, const DropSrc& ds, bool seeded, float* y, int64_t ldy,
                    float* inv, jmac_stream_t stream) {
    if (N < 0 || d <= 0 || d >= INT32_MAX) return JMAC_EINVAL;
    if (d % 4 || ldx % 4 || ldy % 4 || (ds.mask && ds.ldm % 4)) return JMAC_EDIM;
    if (N == 0) return JMAC_OK;
    if (!x || !y || !inv) return JMAC_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)ds.mask) & 15) != 0) return JMAC_EDIM;
    const bool rowform = d <= 512 && N >= kDropRowsMinN;
    with_drop_form(seeded, rowform, [&](auto SD, auto RF) {
        if constexpr (RF.value)
            hipLaunchKernelGGL((rows_normalize_drop_fwd_kernel<SD.value, true, kDropRows>), dim3(rows_grid(N, kDropRows)), dim3(kBlock), 0,
                               (hipStream_t)stream, x, ldx, (const int64_t*)nullptr, N, (int)(d / 4), eps, ds, (float*)nullptr,
                               (int64_t)0, y, ldy, inv);
        else
            hipLaunchKernelGGL(row_normalize_drop_fwd_kernel<SD.value>, dim3(rows_grid(N, 1)), dim3(kBlock), 0, (hipStream_t)stream, x, ldx,
                               N, (int)(d / 4), eps, ds, y, ldy, inv);
    });
    return (int)hipGetLastError();
}

static int drop_bwd(const float* x, int64_t ldx, const float* inv, const DropSrc& ds, bool seeded, const float* g, int64_t ldg, int64_t N,
                    int64_t d, float eps, float* gx, int64_t ldgx, int32_t accumulate, jmac_stream_t stream) {
    if (N < 0 || d <= 0 || d >= INT32_MAX) return JMAC_EINVAL;
    if (d % 4 || ldx % 4 || ldg % 4 || ldgx % 4 || (ds.mask && ds.ldm % 4)) return JMAC_EDIM;
    if (N == 0) return JMAC_OK;
    if (!x || !inv || !g || !gx) return JMAC_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)g | (uintptr_t)gx | (uintptr_t)ds.mask) & 15) != 0) return JMAC_EDIM;
    const bool rowform = d <= 512 && N >= kDropRowsMinN;
    with_drop_form(seeded, rowform, [&](auto SD, auto RF) {
        if constexpr (RF.value)                                    // accumulating: gx is the table that is added
            hipLaunchKernelGGL((row_normalize_drop_bwd_scatter_kernel<SD.value, true, true, kDropRows>), dim3(rows_grid(N, kDropRows)),
                               dim3(kBlock), 0, (hipStream_t)stream, x, ldx, inv, ds, g, ldg, accumulate ? (const float*)gx : nullptr,
                               ldgx, (const int64_t*)nullptr, N, (int)(d / 4), eps, gx, ldgx, 0);
        else
            hipLaunchKernelGGL(row_normalize_drop_bwd_kernel<SD.value>, dim3(rows_grid(N, 1)), dim3(kBlock), 0, (hipStream_t)stream, x, ldx,
                               inv, ds, g, ldg, N, (int)(d / 4), eps, gx, ldgx, accumulate ? 1 : 0);
    });
    return (int)hipGetLastError();
}

// keep probability 1 - p as a 32-bit threshold; scale = 1 / (1 - p)
static int seeded_src(const int64_t* seed, float p_drop, DropSrc& ds) {
    if (!seed || !(p_drop >= 0.f) || !(p_drop < 1.f)) return JMAC_EINVAL;
    const double keep = 1.0 - (double)p_drop, t = keep * 4294967296.0;
    ds = DropSrc{nullptr, 0, seed, t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t, (float)(1.0 / keep)};
    return JMAC_OK;
}

int jmac_row_normalize_drop_fwd_f32(const float* x, int64_t ldx, int64_t N, int64_t d, float eps, const float* mask, int64_t ldm,
                                    float scale, float* y, int64_t ldy, float* inv, jmac_stream_t stream) {
    return drop_fwd(x, ldx, N, d, eps, DropSrc{mask, ldm, nullptr, 0u, scale}, false, y, ldy, inv, stream);
}

int jmac_row_normalize_drop_bwd_f32(const float* x, int64_t ldx, const float* inv, const float* mask, int64_t ldm, float scale,
                                    const float* g, int64_t ldg, int64_t N, int64_t d, float eps, float* gx, int64_t ldgx,
                                    int32_t accumulate, jmac_stream_t stream) {
    return drop_bwd(x, ldx, inv, DropSrc{mask, ldm, nullptr, 0u, scale}, false, g, ldg, N, d, eps, gx, ldgx, accumulate, stream);
}

int jmac_row_normalize_dropseed_fwd_f32(const float* x, int64_t ldx, int64_t N, int64_t d, float eps, const int64_t* seed,
                                        float p_drop, float* y, int64_t ldy, float* inv, jmac_stream_t stream) {
    DropSrc ds;
    if (int rc = seeded_src(seed, p_drop, ds)) return rc;
    return drop_fwd(x, ldx, N, d, eps, ds, true, y, ldy, inv, stream);
}

int jmac_row_normalize_dropseed_bwd_f32(const float* x, int64_t ldx, const float* inv, const int64_t* seed, float p_drop,
                                        const float* g, int64_t ldg, int64_t N, int64_t d, float eps, float* gx, int64_t ldgx,
                                        int32_t accumulate, jmac_stream_t stream) {
    DropSrc ds;
    if (int rc = seeded_src(seed, p_drop, ds)) return rc;
    return drop_bwd(x, ldx, inv, ds, true, g, ldg, N, d, eps, gx, ldgx, accumulate, stream);
}

// ---- fused row passes (kernels: "fused row passes of the encoder node's completion chain" above) --------------------------------
// seed NULL: no dropout
static int fused_src(const int64_t* seed, float p_drop, DropSrc& ds) {
    if (seed) return seeded_src(seed, p_drop, ds);
    ds = DropSrc{nullptr, 0, nullptr, 0u, 1.f};
    return JMAC_OK;
}
static bool aligned16(std::initializer_list<const void*> ps) {
    uintptr_t a = 0;
    for (const void* p : ps) a |= (uintptr_t)p;
    return (a & 15) == 0;
}
int jmac_rows_normalize_dropseed_fwd_f32(const float* x, int64_t ldx, const int64_t* row_map, int64_t N, int64_t d, float eps,
                                         const int64_t* seed, float p_drop, float* x_rows, int64_t ldxr, float* y, int64_t ldy,
                                         float* inv, jmac_stream_t stream) {
    DropSrc ds;
    if (int rc = fused_src(seed, p_drop, ds)) return rc;
    if (N < 0) return JMAC_EINVAL;
    if (d <= 0 || d > 512 || d % 4 || ldx % 4 || ldy % 4 || (x_rows && ldxr % 4)) return JMAC_EDIM;
    if (N == 0) return JMAC_OK;
    if (!x || !y || !inv) return JMAC_EINVAL;
    if (!aligned16({x, y, x_rows})) return JMAC_EDIM;
    with_drop_form(ds.seed != nullptr, false, [&](auto SD, auto) {
        hipLaunchKernelGGL((rows_normalize_drop_fwd_kernel<SD.value, false, kFuseRows>), dim3(rows_grid(N, kFuseRows)), dim3(kBlock), 0,
                           (hipStream_t)stream, x, ldx, row_map, N, (int)(d / 4), eps, ds, x_rows, ldxr, y, ldy, inv);
    });
    return (int)hipGetLastError();
}

int jmac_bn_tanh_normalize_dropseed_fwd_f32(const float* x, int64_t ldx, int64_t N, int64_t d, const float* weight, const float* bias,
                                            float* running_mean, float* running_var, int32_t training, float momentum, float eps,
                                            float* y, int64_t ldy, const int64_t* row_map, float* y_rows, int64_t ldyr, float norm_eps,
                                            const int64_t* seed, float p_drop, float* yn, int64_t ldyn, float* inv, float* save_mean,
                                            float* save_invstd, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    DropSrc ds;
    if (int rc = fused_src(seed, p_drop, ds)) return rc;
    if (N < 0 || !weight || !bias || !save_mean || !save_invstd || (row_map == nullptr) != (y_rows == nullptr)) return JMAC_EINVAL;
    if (d <= 0 || d > 512 || d % 4 || ldx % 4 || ldy % 4 || ldyn % 4 || (y_rows && ldyr % 4)) return JMAC_EDIM;
    if (N == 0) return JMAC_OK;
    if (!x || !y || !yn || !inv) return JMAC_EINVAL;
    if (!aligned16({x, y, y_rows, yn, weight, bias, save_mean, save_invstd})) return JMAC_EDIM;
    hipStream_t st = (hipStream_t)stream;
    const int D4 = (int)(d / 4);
    if (int rc = launch_bn_fwd_stats(x, ldx, N, d, running_mean, running_var, training, momentum, eps, save_mean, save_invstd, ws,
                                     ws_bytes, st))
        return rc;
    with_drop_form(ds.seed != nullptr, false, [&](auto SD, auto) {
        hipLaunchKernelGGL((bn_tanh_normalize_drop_fwd_kernel<SD.value, kFuseRows>), dim3(rows_grid(N, kFuseRows)), dim3(kBlock), 0, st, x,
                           ldx, N, D4, weight, bias, (const float*)save_mean, (const float*)save_invstd, y, ldy, row_map, y_rows, ldyr,
                           norm_eps, ds, yn, ldyn, inv);
    });
    return (int)hipGetLastError();
}

int jmac_bn_tanh_bwd_normadj_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* inv, const float* g,
                                 int64_t ldg, float norm_eps, const int64_t* seed, float p_drop, const float* gy2, int64_t ldgy2,
                                 const int64_t* row_map, int64_t N, int64_t d, const float* weight, const float* save_mean,
                                 const float* save_invstd, int32_t training, float* gx, int64_t ldgx, float* gweight, float* gbias,
                                 void* ws, size_t ws_bytes, jmac_stream_t stream) {
    DropSrc ds;
    if (int rc = fused_src(seed, p_drop, ds)) return rc;
    if (N < 0 || !weight || !save_mean || !save_invstd || !gweight || !gbias) return JMAC_EINVAL;
    if (d <= 0 || d > 512 || d % 4 || ldx % 4 || ldy % 4 || ldg % 4 || ldgx % 4 || (gy2 && ldgy2 % 4)) return JMAC_EDIM;
    if (!ws || ws_bytes < jmac_bn_tanh_workspace_bytes(N, d)) return JMAC_EWORKSPACE;
    if (!aligned16({x, y, g, gy2, gx, weight, save_mean, save_invstd, gweight, gbias, ws})) return JMAC_EDIM;
    hipStream_t st = (hipStream_t)stream;
    const int D4 = (int)(d / 4);
    float* partial = (float*)ws;
    unsigned pg = 0;
    const bool rowform = N >= kDropRowsMinN;                      // the adjoint as the separate launch forms it at this N
    if (N > 0) {
        if (!x || !y || !inv || !g || !gx) return JMAC_EINVAL;
        pg = stat_grid(N, D4);                                    // bn_bwd_partial_kernel's blocks and row slots: the same sums
        const int rpb = kBlock / D4;
        const unsigned threads = 64u * (unsigned)(rpb < kBlock / 64 ? rpb : kBlock / 64);
        with_drop_form(ds.seed != nullptr, rowform, [&](auto SD, auto RF) {
            hipLaunchKernelGGL((bn_bwd_partial_adj_kernel<SD.value, RF.value, kFuseBwdRows>), dim3(pg), dim3(threads), stat_smem(D4), st, x,
                               ldx, y, ldy, g, ldg, inv, ds, norm_eps, gy2, ldgy2, row_map, N, D4, save_mean, save_invstd, partial);
        });
    }
    launch_bn_bwd_param_grads(partial, pg, d, gweight, gbias, st);
    if (N > 0)
        with_drop_form(ds.seed != nullptr, rowform, [&](auto SD, auto RF) {
            hipLaunchKernelGGL((bn_bwd_apply_adj_kernel<SD.value, RF.value, kFuseBwdRows>), dim3(rows_grid(N, kFuseBwdRows)), dim3(kBlock),
                               0, st, x, ldx, y, ldy, g, ldg, inv, ds, norm_eps, gy2, ldgy2, row_map, N, D4, weight, save_mean,
                               save_invstd, (const float*)gweight, (const float*)gbias, training ? 1 : 0, 1.f / (float)N, gx, ldgx);
        });
    return (int)hipGetLastError();
}

int jmac_row_normalize_dropseed_bwd_rows_f32(const float* x, int64_t ldx, const float* inv, const int64_t* seed, float p_drop,
                                             const float* g, int64_t ldg, const float* add, int64_t ldadd, const int64_t* row_map,
                                             int64_t N, int64_t d, float eps, float* dst, int64_t lddst, int32_t accumulate,
                                             jmac_stream_t stream) {
    DropSrc ds;
    if (int rc = fused_src(seed, p_drop, ds)) return rc;
    if (N < 0) return JMAC_EINVAL;
    if (d <= 0 || d > 512 || d % 4 || ldx % 4 || ldg % 4 || lddst % 4 || (add && ldadd % 4)) return JMAC_EDIM;
    if (N == 0) return JMAC_OK;
    if (!x || !inv || !g || !dst) return JMAC_EINVAL;
    if (!aligned16({x, g, add, dst})) return JMAC_EDIM;
    with_drop_form(ds.seed != nullptr, N >= kDropRowsMinN, [&](auto SD, auto RF) {
        hipLaunchKernelGGL((row_normalize_drop_bwd_scatter_kernel<SD.value, RF.value, false, kFuseBwdRows>),
                           dim3(rows_grid(N, kFuseBwdRows)), dim3(kBlock), 0, (hipStream_t)stream, x, ldx, inv, ds, g, ldg, add, ldadd,
                           row_map, N, (int)(d / 4), eps, dst, lddst, accumulate ? 1 : 0);
    });
    return (int)hipGetLastError();
}

// ---- segmented BatchNorm + tanh (block-batched encoder: several KGs in one launch set) ------------------------------
static int make_seg(int32_t nblocks, const int64_t* blk_ptr, const int32_t* order, int D4, SegTab& s) {
    if (nblocks < 1 || nblocks > kMaxSeg || !blk_ptr || blk_ptr[0] != 0) return JMAC_EINVAL;
    s.nb = nblocks;
    unsigned seen = 0;
    s.gofs[0] = 0;
    for (int b = 0; b < kMaxSeg; ++b) s.order[b] = 0;
    for (int b = 0; b < nblocks; ++b) {
        const int64_t n = blk_ptr[b + 1] - blk_ptr[b];
        if (n <= 0) return JMAC_EINVAL;
        s.ptr[b] = blk_ptr[b];
        s.gofs[b + 1] = s.gofs[b] + (int)stat_grid(n, D4);
        const int o = order ? order[b] : b;
        if (o < 0 || o >= nblocks || (seen >> o & 1u)) return JMAC_EINVAL;    // a permutation of the blocks
        seen |= 1u << o;
        s.order[b] = o;
    }
    for (int b = nblocks; b <= kMaxSeg; ++b) s.ptr[b] = blk_ptr[nblocks];
    for (int b = nblocks + 1; b <= kMaxSeg; ++b) s.gofs[b] = s.gofs[nblocks];
    return JMAC_OK;
}

size_t jmac_bn_tanh_seg_workspace_bytes(int32_t nblocks, int64_t d) {
    if (nblocks < 1) nblocks = 1;
    if (d < 0) d = 0;
    // partial rows of every block (<= kStatBlocks each) + the per-block backward sums [nb, 2d]
    return align_up((size_t)nblocks * kStatBlocks * 2 * d * 4) + align_up((size_t)nblocks * 2 * d * 4) + 256;
}

int jmac_bn_tanh_seg_fwd2_f32(const float* x, int64_t ldx, int64_t d, int32_t nblocks, const int64_t* blk_ptr,
                              const int32_t* order, const float* weight, const float* bias, float* running_mean,
                              float* running_var, float momentum, float eps, float* y, int64_t ldy, float* y2, int64_t ldy2,
                              float* save_mean, float* save_invstd, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    if (!x || !y || !weight || !bias || !save_mean || !save_invstd) return JMAC_EINVAL;
    if (d <= 0 || d % 4 || ldx % 4 || ldy % 4 || (y2 && ldy2 % 4)) return JMAC_EDIM;
    const int D4 = (int)(d / 4);
    SegTab seg;
    if (int rc = make_seg(nblocks, blk_ptr, order, D4, seg)) return rc;
    if (!ws || ws_bytes < jmac_bn_tanh_seg_workspace_bytes(nblocks, d)) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)ws;
    hipLaunchKernelGGL(col_stats_partial_kernel<true>, dim3((unsigned)seg.gofs[nblocks]), dim3(kBlock), stat_smem(D4), st, x, ldx, seg,
                       D4, partial);
    hipLaunchKernelGGL(bn_reduce_finalize_kernel<true>, dim3((unsigned)((d + RF_COLS - 1) / RF_COLS)), dim3(1024), 0, st, partial, seg,
                       0, x, ldx, (int)d, eps, momentum, running_mean, running_var, save_mean, save_invstd);
    hipLaunchKernelGGL(bn_tanh_apply_kernel<true>, dim3(stream_grid(seg.ptr[nblocks] * D4)), dim3(kBlock), 0, st, x, ldx, seg, D4,
                       weight, bias, (const float*)save_mean, (const float*)save_invstd, y, ldy, y2, ldy2);
    return (int)hipGetLastError();
}

int jmac_bn_tanh_seg_bwd2_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* gy, int64_t ldgy,
                              const float* gy2, int64_t ldgy2, int64_t d, int32_t nblocks, const int64_t* blk_ptr,
                              const float* weight, const float* save_mean, const float* save_invstd, float* gx, int64_t ldgx,
                              float* gweight, float* gbias, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    if (!x || !y || !gy || !gx || !weight || !save_mean || !save_invstd || !gweight || !gbias) return JMAC_EINVAL;
    if (d <= 0 || d % 4 || ldx % 4 || ldy % 4 || ldgy % 4 || ldgx % 4 || (gy2 && ldgy2 % 4)) return JMAC_EDIM;
    const int D4 = (int)(d / 4);
    SegTab seg;
    if (int rc = make_seg(nblocks, blk_ptr, nullptr, D4, seg)) return rc;
    if (!ws || ws_bytes < jmac_bn_tanh_seg_workspace_bytes(nblocks, d)) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)ws;
    float* bsums = (float*)((char*)ws + align_up((size_t)nblocks * kStatBlocks * 2 * d * 4));
    hipLaunchKernelGGL(bn_bwd_partial_kernel<true>, dim3((unsigned)seg.gofs[nblocks]), dim3(kBlock), stat_smem(D4), st, x, ldx, y, ldy,
                       gy, ldgy, gy2, ldgy2, seg, D4, save_mean, save_invstd, partial);
    hipLaunchKernelGGL(bn_bwd_reduce_seg_kernel, dim3((unsigned)((2 * d + RF_COLS - 1) / RF_COLS)), dim3(1024), 0, st, partial, seg,
                       (int)(2 * d), bsums, gbias, gweight, (int)d);
    hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, dim3(stream_grid(seg.ptr[nblocks] * D4)), dim3(kBlock), 0, st, x, ldx, y, ldy, gy, ldgy,
                       gy2, ldgy2, seg, D4, weight, save_mean, save_invstd, (const float*)(bsums + d), (const float*)bsums, 2 * d, 1,
                       0.f, gx, ldgx);
    return (int)hipGetLastError();
}

// ---- phased forms for batch statistics that span several ranks (destination-sharded layer, jmac_amd/dist.py) ---------
// moments -> [combine across ranks on the host side of the ABI] -> apply;  backward: sums -> [all-reduce] -> apply.

int jmac_col_moments_f32(const float* x, int64_t ldx, int64_t N, int64_t d, float* mean, float* m2, void* ws, size_t ws_bytes,
                         jmac_stream_t stream) {
    if (N <= 0 || !x || !mean || !m2) return JMAC_EINVAL;
    if (d <= 0 || d % 4 || ldx % 4) return JMAC_EDIM;
    if (!ws || ws_bytes < jmac_bn_tanh_workspace_bytes(N, d)) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int D4 = (int)(d / 4);
    float* partial = (float*)ws;
    const unsigned g = stat_grid(N, D4);
    hipLaunchKernelGGL(col_stats_partial_kernel<false>, dim3(g), dim3(kBlock), stat_smem(D4), st, x, ldx, N, D4, partial);
    float* sums = partial + (size_t)kStatBlocks * 2 * d;
    launch_reduce_rows(partial, (int)g, (int)(2 * d), 1.f, sums, st);
    hipLaunchKernelGGL(moments_finalize_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, sums, x, N, (int)d, mean, m2);
    return (int)hipGetLastError();
}

int jmac_bn_tanh_apply_f32(const float* x, int64_t ldx, int64_t N, int64_t d, const float* weight, const float* bias,
                           const float* mean, const float* invstd, float* y, int64_t ldy, jmac_stream_t stream) {
    if (N < 0 || !weight || !bias || !mean || !invstd) return JMAC_EINVAL;
    if (d <= 0 || d % 4 || ldx % 4 || ldy % 4) return JMAC_EDIM;
    if (N == 0) return JMAC_OK;
    if (!x || !y) return JMAC_EINVAL;
    const int D4 = (int)(d / 4);
    hipLaunchKernelGGL(bn_tanh_apply_kernel<false>, dim3(stream_grid(N * D4)), dim3(kBlock), 0, (hipStream_t)stream, x, ldx, N,
                       D4, weight, bias, mean, invstd, y, ldy, (float*)nullptr, (int64_t)0);
    return (int)hipGetLastError();
}

int jmac_bn_tanh_bwd_sums_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* gy, int64_t ldgy, int64_t N,
                              int64_t d, const float* mean, const float* invstd, float* sums, void* ws, size_t ws_bytes,
                              jmac_stream_t stream) {
    if (N < 0 || !mean || !invstd || !sums) return JMAC_EINVAL;
    if (d <= 0 || d % 4 || ldx % 4 || ldy % 4 || ldgy % 4) return JMAC_EDIM;
    if (!ws || ws_bytes < jmac_bn_tanh_workspace_bytes(N, d)) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int D4 = (int)(d / 4);
    float* partial = (float*)ws;
    unsigned g = 0;
    if (N > 0) {
        if (!x || !y || !gy) return JMAC_EINVAL;
        g = stat_grid(N, D4);
        hipLaunchKernelGGL(bn_bwd_partial_kernel<false>, dim3(g), dim3(kBlock), stat_smem(D4), st, x, ldx, y, ldy, gy, ldgy,
                           (const float*)nullptr, (int64_t)0, N, D4, mean, invstd, partial);
    }
    launch_reduce_rows(partial, (int)g, (int)(2 * d), 1.f, sums, st);     // sums[0:d] = sum gz, sums[d:2d] = sum gz * xhat
    return (int)hipGetLastError();
}

int jmac_bn_tanh_bwd_apply_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* gy, int64_t ldgy, int64_t N,
                               int64_t d, const float* weight, const float* mean, const float* invstd, const float* sums,
                               int64_t n_total, float* gx, int64_t ldgx, jmac_stream_t stream) {
    if (N < 0 || n_total <= 0 || !weight || !mean || !invstd || !sums) return JMAC_EINVAL;
    if (d <= 0 || d % 4 || ldx % 4 || ldy % 4 || ldgy % 4 || ldgx % 4) return JMAC_EDIM;
    if (N == 0) return JMAC_OK;
    if (!x || !y || !gy || !gx) return JMAC_EINVAL;
    const int D4 = (int)(d / 4);
    hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, dim3(stream_grid(N * D4)), dim3(kBlock), 0, (hipStream_t)stream, x, ldx, y, ldy, gy,
                       ldgy, (const float*)nullptr, (int64_t)0, N, D4, weight, mean, invstd, sums + d, sums, (int64_t)0, 1,
                       1.f / (float)n_total, gx, ldgx);
    return (int)hipGetLastError();
}

}  // extern "C"
