// score.hip -- triple and entity-pair scoring for gfx950.
//
//  * jmac_l1_score_f32      torch.cdist(er, all_kg_emb, p=1)            src/jmac_model.py:312
//  * jmac_filtered_rank_f32 filter + sort + np.where ranking loop        src/validate.py:50-64
//  * jmac_linkpred_rank_{,indexed_}*  forward_linkpred + that loop, ranks only; the filter from a per-batch CSR or from the
//                            device-resident known-tail index                 src/jmac_model.py:302-313, src/validate.py:50-64
//  * jmac_linkpred_topk_*   the k nearest tails the index does not list (the model's predictions; no counterpart)
//  * jmac_linkpred_stats_*, jmac_linkpred_ens_stats_f32   the softmax over tails of every query -- nearest candidate, normaliser,
//                            entropy, the gold's log-probability -- from the L1 tile kernel's epilogue (no counterpart)
//  * jmac_linkpred_ens_*    those ranks and top-k on the cross-KG ensemble distance: supporting KGs vote through link maps (no counterpart)
//  * jmac_sim_matrix_f32    torch.mm(ILL_vec, KG_vec.t())              modules/utils/util.py:52, train.py:239
//  * jmac_row_topk_f32 / jmac_sim_topk_f32   sim.topk(k, dim=1)          modules/utils/util.py:53
//  * jmac_softmax_entropy_f32, jmac_row_softmax_f32                      train.py:241-257
//  * jmac_sim_softmax_stats_f32  the same softmax's maxima, arg-maxima, sums and entropies per row and per column from the
//                                product's epilogue, the matrix never written                   train.py:160-169, 231-259
//  * jmac_sim_lse_f32            log-sum-exp of scale S + offsets per row and per column from the same epilogue: the half-steps
//                                of log-domain Sinkhorn (no counterpart in the reference's sim())
//
// L1 distance is |a-b| accumulation: not a contraction, so it runs on the VALU (register-tiled through
// LDS); the similarity matrices are contractions and run on the matrix cores with the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate), so top-k indices are decided on
// full-precision scores.
#include "common.h"
#include "sim_rescore.h"
#include "topk_select.h"
#include <type_traits>

using namespace jmac;

namespace {

constexpr int kBlock = 256;
static_assert(TK_THREADS == kBlock, "the selection routines stride by the block size");

// ------------------------------------------------------------------------------------------------
// The L1 (Manhattan) tile family: 64x64 output tile per block, 4x4 per thread, K staged 16 at a time (transposed in LDS).
// Three kernels -- l1_score_kernel (one table), link_rank_tile_kernel (the layers of one KG) and link_ens_tile_kernel (members x
// layers, candidate rows read through link maps) -- are assembled from ONE set of pieces, so a pair (b, n) gets the same bits
// wherever it is evaluated:
//   l1_load, l1_stage, l1_step   a thread's operand quad from global memory, its transposed copy in LDS, one 16-deep slab
//   l1_slab_loop                 the double-buffered loop; a kernel passes in where slab s's operands come from
//   l1_epi_store / l1_epi_append / l1_epi_count   the epilogues, on the 4x4 values a thread decides on
//   l1_seq_sum                   the same sum for ONE pair: the one-lane-per-candidate sites (prep, select, gold kernels)
// ------------------------------------------------------------------------------------------------
constexpr int L1_T = 64, L1_K = 16, L1_LD = L1_T + 4;

// acc + |a - b| in two full-rate VALU ops (v_sub_f32, v_add_f32 with the |.| source modifier).  Left to the
// compiler, fabsf() becomes v_and_b32 and the adds are SLP-packed into half-rate v_pk_add_f32: 3 issue slots.
// (Round 6, tools/r6_l1_probe.py: with -fno-slp-vectorize the compiler's own form keeps the |.| modifier and has none of the
// hazard s_nops hipcc puts between dependent asm statements -- one per sub/add pair here -- but it hoists a slab's 32 fragment
// reads: 165 VGPRs against 56, three waves per SIMD, and the tile kernels run 8-60 % SLOWER; at eight waves per SIMD the nops
// cost nothing, another wave issues in their slot.)
__device__ __forceinline__ float add_absdiff(float acc, float a, float b) {
    float d, r;
    asm("v_sub_f32_e32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    asm("v_add_f32_e64 %0, %1, |%2|" : "=v"(r) : "v"(acc), "v"(d));
    return r;
}

__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const bf16_t* p) { return __uint_as_float((uint32_t)(*p) << 16); }

// where a thread stands in its block's tile: it owns outputs (b0 + ty * 4 + i, n0 + tx * 4 + j) and loads one quad (4 consecutive
// k from lk) of row lrow of either operand
struct L1Pos {
    int b0, n0, tx, ty, lrow, lk;
};
__device__ __forceinline__ L1Pos l1_pos(int b0, int n0, int tid = threadIdx.x) {
    return L1Pos{b0, n0, tid & 15, tid >> 4, tid >> 2, (tid & 3) * 4};
}
// threadIdx.x, opaque to the compiler (an empty asm, no instruction): what is derived from it is computed where it is used.
// Without this the compiler forms a later phase's lane-dependent values ahead of a loop and holds them in VGPRs across it.
// This steers one compiler's register allocation, nothing else: the figures next to its uses are hipcc 7.2 (AMD clang 22) for
// gfx950, profiles/l1_tile_refactor_resources.txt is the table to regenerate under another compiler, and the code is correct
// with or without it.  link_ens_tile_kernel does not need it: its 96-100 VGPRs are what it took written out in full.
__device__ __forceinline__ int tid_again() {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    return tid;
}
// the same position for the epilogue: its indices are then formed after the slab loop (2-3 VGPRs in the append forms)
__device__ __forceinline__ L1Pos l1_pos_again(const L1Pos& p) { return l1_pos(p.b0, p.n0, tid_again()); }

// Elements k .. k + 3 of a row (k = slab offset + lk).  TT = float or bf16_t (raw bits): bf16 operands are widened here, the
// |a - b| accumulation is fp32 either way (the kernels are VALU-bound, so the narrower tables change the bytes, not the time).
// Every global load is UNCONDITIONAL at a clamped address: a load behind an exec-mask branch gets its s_waitcnt inside the branch
// (hipcc), i.e. the next slab's prefetch would be waited for before the current slab's arithmetic instead of after it.  So `row`
// is always a row of the table -- a row past the end is clamped by the caller to one that exists, ok = false, and only feeds
// outputs that are never stored -- and a k quad past d re-reads the last quad; l1_stage zeroes both.
// VEC = false (d % 4 != 0, or a base or leading dimension that rules 4-element loads out): the scalar form, zeros where VEC pads.
template <typename TT, bool VEC>
__device__ __forceinline__ float4 l1_load(const TT* base, int64_t ld, int64_t row, bool ok, int k, int d) {
    if constexpr (VEC) return cvt4(ldraw(base + row * ld + (k < d ? k : d - 4)));
    float4 v = f4zero();
    if (ok) {
        const TT* p = base + row * ld;
        if (k + 0 < d) v.x = ld1(p + k + 0);
        if (k + 1 < d) v.y = ld1(p + k + 1);
        if (k + 2 < d) v.z = ld1(p + k + 2);
        if (k + 3 < d) v.w = ld1(p + k + 3);
    }
    return v;
}
// ... into one LDS buffer, transposed; keep = the row exists and the quad lies inside d
template <bool VEC>
__device__ __forceinline__ void l1_stage(float (*S)[L1_LD], float4 v, const L1Pos& p, bool keep) {
    if (VEC && !keep) v = f4zero();                              // the clamped loads' padding: |0 - 0| adds nothing
    S[p.lk + 0][p.lrow] = v.x;
    S[p.lk + 1][p.lrow] = v.y;
    S[p.lk + 2][p.lrow] = v.z;
    S[p.lk + 3][p.lrow] = v.w;
}
// acc[i][j] += sum over the slab's 16 k, in order, of |A[k][ty * 4 + i] - B[k][tx * 4 + j]|
__device__ __forceinline__ void l1_step(float (&acc)[4][4], const float (*As)[L1_LD], const float (*Bs)[L1_LD], const L1Pos& p) {
#pragma unroll
    for (int k = 0; k < L1_K; ++k) {
        const float4 a = *reinterpret_cast<const float4*>(&As[k][p.ty * 4]);
        const float4 b = *reinterpret_cast<const float4*>(&Bs[k][p.tx * 4]);
        const float av[4] = {a.x, a.y, a.z, a.w};
        const float bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = add_absdiff(acc[i][j], av[i], bv[j]);
    }
}
// acc += slabs 0 .. ns-1, double-buffered: slab s + 1 is loaded before slab s's arithmetic and staged after it.
// src(s, ra, rb) loads the thread's two quads of slab s and returns the slab's k offset.
template <bool VEC, class Src>
__device__ __forceinline__ void l1_slab_loop(float (&acc)[4][4], float (&As)[2][L1_K][L1_LD], float (&Bs)[2][L1_K][L1_LD],
                                             const L1Pos& p, int ns, int d, bool a_ok, bool b_ok, Src src) {
    float4 ra, rb;
    src(0, ra, rb);
    l1_stage<VEC>(As[0], ra, p, a_ok && p.lk < d);
    l1_stage<VEC>(Bs[0], rb, p, b_ok && p.lk < d);
    __syncthreads();
    for (int s = 0; s < ns; ++s) {
        const int cur = s & 1;
        int k0 = 0;
        if (s + 1 < ns) k0 = src(s + 1, ra, rb);
        l1_step(acc, As[cur], Bs[cur], p);
        if (s + 1 < ns) {
            l1_stage<VEC>(As[cur ^ 1], ra, p, a_ok && k0 + p.lk < d);
            l1_stage<VEC>(Bs[cur ^ 1], rb, p, b_ok && k0 + p.lk < d);
        }
        __syncthreads();
    }
}

// acc + |a[0] - b[0]| + ... + |a[d-1] - b[d-1]|, one add after the other.  This IS a tile kernel's order of additions for one
// output element (its zero padding adds exact zeros; a caller with layers carries acc from one layer into the next), so every
// one-lane-per-pair site has the tile's bits.  QUAD (the prep kernels, whose B lanes each run the whole chain out of LDS): four
// pairs are loaded at a time -- the loads are independent, the adds are not -- which takes 2 more VGPRs than the plain loop.
template <bool QUAD = false, typename TA, typename TB>
__device__ __forceinline__ float l1_seq_sum(float acc, const TA* a, const TB* b, int d) {
    int k = 0;
    if constexpr (QUAD)
        for (; k + 4 <= d; k += 4) {
            const float a0 = ld1(a + k), a1 = ld1(a + k + 1), a2 = ld1(a + k + 2), a3 = ld1(a + k + 3);
            const float b0 = ld1(b + k), b1 = ld1(b + k + 1), b2 = ld1(b + k + 2), b3 = ld1(b + k + 3);
            acc = add_absdiff(acc, a0, b0);
            acc = add_absdiff(acc, a1, b1);
            acc = add_absdiff(acc, a2, b2);
            acc = add_absdiff(acc, a3, b3);
        }
    for (; k < d; ++k) acc = add_absdiff(acc, ld1(a + k), ld1(b + k));
    return acc;
}

// store epilogue: out[b * ld + n - n_off] = v, 16 bytes at a time where the quad is whole and aligned; row(i, v) fills v[0..3] with
// the values of the thread's output row i
template <class Row>
__device__ __forceinline__ void l1_epi_store(Row row, const L1Pos& p, int B, int N, float* out, int64_t ld, int n_off) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = p.b0 + p.ty * 4 + i;
        if (b >= B) continue;
        const int n = p.n0 + p.tx * 4;
        float* o = out + (int64_t)b * ld + (n - n_off);
        float v[4];
        row(i, v);
        if (n + 3 < N && (ld % 4 == 0) && (n_off % 4 == 0)) st4(o, make_float4(v[0], v[1], v[2], v[3]));
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n + j < N) o[j] = v[j];
        }
    }
}

template <typename TT, bool VEC>
__global__ __launch_bounds__(kBlock) void l1_score_kernel(const TT* __restrict__ er, int64_t lder,
                                                          const TT* __restrict__ tab, int64_t ldt, int B, int N, int d,
                                                          float* __restrict__ out, int64_t ldout, int accumulate) {
    __shared__ __attribute__((aligned(16))) float As[2][L1_K][L1_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][L1_K][L1_LD];
    const L1Pos p = l1_pos(blockIdx.y * L1_T, blockIdx.x * L1_T);
    const bool a_ok = p.b0 + p.lrow < B, b_ok = p.n0 + p.lrow < N;
    const int64_t arow = a_ok ? p.b0 + p.lrow : B - 1, brow = b_ok ? p.n0 + p.lrow : N - 1;
    float acc[4][4] = {};
    l1_slab_loop<VEC>(acc, As, Bs, p, (d + L1_K - 1) / L1_K, d, a_ok, b_ok, [&](int s, float4& ra, float4& rb) {
        ra = l1_load<TT, VEC>(er, lder, arow, a_ok, s * L1_K + p.lk, d);
        rb = l1_load<TT, VEC>(tab, ldt, brow, b_ok, s * L1_K + p.lk, d);
        return s * L1_K;
    });
    // the store epilogue in its accumulate form, this kernel's alone: through l1_epi_store the bf16 vector form takes 56 VGPRs, not 54
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t b = p.b0 + p.ty * 4 + i;
        if (b >= B) continue;
        const int64_t n = p.n0 + p.tx * 4;
        float* o = out + b * ldout + n;
        if (n + 3 < N && (ldout % 4 == 0)) {
            float4 v = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
            if (accumulate) {
                const float4 q = ld4(o);
                v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
            }
            st4(o, v);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n + j < N) o[j] = accumulate ? o[j] + acc[i][j] : acc[i][j];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// filtered rank: one block per query
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void filtered_rank_kernel(const float* __restrict__ score, int64_t lds,
                                                               const int32_t* __restrict__ gold,
                                                               const int32_t* __restrict__ filt_ptr,
                                                               const int32_t* __restrict__ filt_idx, int N, int descending,
                                                               int32_t* __restrict__ rank) {
    __shared__ int red[kBlock / 64];
    const int b = blockIdx.x;
    const float* row = score + (int64_t)b * lds;
    const int g = gold[b];
    const float gs = row[g];
    // ascending: a DISTANCE (smaller ranks first); descending: a SIMILARITY (larger first) -- no negated copy needed
    auto before = [&](float s, int n) { return (descending ? s > gs : s < gs) || (s == gs && n < g); };
    int cnt = 0;
    for (int n = threadIdx.x; n < N; n += kBlock) cnt += before(row[n], n) ? 1 : 0;
    if (filt_ptr) {
        for (int f = filt_ptr[b] + threadIdx.x; f < filt_ptr[b + 1]; f += kBlock) {
            const int n = filt_idx[f];
            if (n == g || n < 0 || n >= N) continue;
            cnt -= before(row[n], n) ? 1 : 0;
        }
    }
    cnt = wave_sum_i(cnt);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kBlock / 64; ++w) t += red[w];
        rank[b] = t + 1;
    }
}

// ------------------------------------------------------------------------------------------------
// fused link prediction: ranks of the gold tails WITHOUT the [B, N] distance matrix
//   dist[b, n] = sum over layers l, then k, of |(E_l[h_b] +/- R_l[r_b])[k] - T_l[n, k]|   (ONE running fp32 sum, in that order)
//   rank[b]    = 1 + #{n : dist[b, n] before dist[b, gold_b]} - #{filtered n != gold : ... before ...}
// "before" = smaller, or equal with the lower index (jmac_filtered_rank_f32).  Two launches: the prep kernel builds the
// query rows, the gold distances and the filter correction; the tile kernel is the L1 tile body over layer-major slabs with
// a compare-and-count epilogue (integer atomics: order-independent) instead of the [B, N] store.
// ------------------------------------------------------------------------------------------------
constexpr int LR_MAX_LAYERS = 4;
struct LinkRankArgs {
    const float* ent[LR_MAX_LAYERS];      // [*, d] fp32 entity tables the query rows are gathered from
    const float* rel[LR_MAX_LAYERS];      // [*, d] fp32 relation tables
    const void* tab[LR_MAX_LAYERS];       // [N, d] candidate tables of element type TT (== ent for fp32)
    int64_t ld_ent[LR_MAX_LAYERS], ld_rel[LR_MAX_LAYERS], ld_tab[LR_MAX_LAYERS];
    int32_t nl, B, N, d, dq;              // dq = d rounded up to 4: row stride of the query workspace
    int32_t rows;                         // candidate rows the prep kernel stages per pass (LDS budget)
    float sign;                           // +1: E[h] + R[r] (tail prediction), -1: E[h] - R[r]
    float scale;                          // STATS: the temperature, logit = -scale * dist
    const int32_t *h, *r, *gold, *filt_ptr, *filt_idx;
    void* er;                             // workspace [nl][B][dq] of TT
    float* gs;                            // workspace [B]
    int32_t* rank;                        // [B]: the counters themselves
    // known-tail index (jmac_tail_index_t): key != nullptr replaces the per-batch CSR -- filt_ptr / filt_idx then hold the
    // index's tail_ptr / tail_idx and query b's range is looked up under (h_b << 32 | r_b)
    const int64_t* key;
    int64_t n_keys;
    // top-k (jmac_linkpred_topk_*): the tile kernel's STORE and FILTER epilogues score columns [n_off, N)
    int2* rng;                            // workspace [B]: every query's [begin, end) in filt_idx (the prep kernel's lookup)
    int32_t n_off;
    float* S;                             // STORE: S[b * ldS + n - n_off] = -dist[b, n]
    int64_t ldS;                          // STATS: S = the partials, float4 [ceil(N / 64)][B] (max -dist, sum e, sum e u, arg)
    const float* ntau;                    // FILTER: ntau[b * tau_stride] = -tau_b; (dist, n) with -dist >= -tau_b are appended
    int32_t tau_stride, cap;
    int32_t* cnt;                         // [B] entries appended (may exceed cap: that row overflowed)
    float* cval;                          // [B, cap] -dist
    int32_t* cidx;                        // [B, cap] n
    // Manhattan alignment (jmac_l1_csls_*): nl = 1, er = the row operand itself (dq = its leading dimension), tab[0] = the column
    // operand.  The LR_CSLS_* epilogues decide on c(b, n) = csls_value(1 - dist[b, n], r1[b], r2[n]) (r1 == NULL, with r2: on
    // s = 1 - dist): gs holds c(b, gold_b), ntau the thresholds tau_b in c, cval the appended c.
    const float *r1, *r2;                 // [B], [N]
    const int32_t* row_id;                // VIABLE: [B] the suitor id of row b
    const unsigned long long* best;       // VIABLE: [N] the reviewers' words, 0 = free
};

// [begin, end) of query (h, r)'s tails in the index, searched by ONE WAVE (all 64 lanes call this): every round the lanes
// probe 64 evenly spaced keys of the remaining range and a ballot picks the bracket -- 3 rounds of dependent loads for up to
// 262 144 keys (a one-lane binary search needs 18), 6 at 2^31.  An absent key has no tails.  The result is wave-uniform.
__device__ __forceinline__ int2 tail_range(const LinkRankArgs& a, int h, int r) {
    const int64_t q = ((int64_t)h << 32) | (int64_t)(uint32_t)r;
    const int lane = threadIdx.x & 63;
    int64_t lo = 0, hi = a.n_keys;                                 // the first key >= q lies in [lo, hi]
    while (lo < hi) {
        const int64_t step = (hi - lo + 63) >> 6, p = lo + lane * step;
        const bool below = p < hi && a.key[p] < q;                 // ascending keys: the lanes that see a smaller key are a prefix
        const int c = __popcll(__ballot(below));
        if (c == 0) break;                                         // key[lo] >= q
        const int64_t last = lo + (int64_t)(c - 1) * step;         // the last probe below q; the next probe (if any) is not
        hi = last + step < hi ? last + step : hi;
        lo = last + 1;
    }
    if (lo < a.n_keys && a.key[lo] == q) return make_int2(a.filt_ptr[lo], a.filt_ptr[lo + 1]);
    return make_int2(0, 0);
}

// whether n is among the (ascending) tails tail_idx[f0, f1) of a query
__device__ __forceinline__ bool tail_listed(const int32_t* __restrict__ tail_idx, int f0, int f1, int n) {
    while (f0 < f1) {
        const int mid = (f0 + f1) >> 1;
        const int t = tail_idx[mid];
        if (t == n) return true;
        if (t < n) f0 = mid + 1;
        else f1 = mid;
    }
    return false;
}

__device__ __forceinline__ uint16_t f32_to_bf16_rne(float x) {
    uint32_t u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);     // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(bf16_t* p, float v) { *p = f32_to_bf16_rne(v); }

// (the softmax-statistics epilogues of both tile families, sim_gemm_kernel's SG_STATS and LR_STATS below)
// e^x and e^x x of one logit difference x = scale (s - max) <= 0; an excluded element (s = -inf, or the whole part excluded:
// NaN) is clamped to -1e30, where e^x is 0 and the product -0
__device__ __forceinline__ void sg_exp_term(float s, float mx, float scale, float& l, float& t) {
    const float x = fmaxf(scale * (s - mx), -1e30f);
    const float e = fast_exp(x);
    l += e;
    t = fmaf(e, x, t);
}

// The epilogues below decide on 4x4 values that a tile kernel hands over one row at a time: row(i, v) fills v[0..3] with the values
// of output row i (computing them inside the row loop keeps 4, not 16, of them live beside the accumulators).
// append epilogue: (v, n) goes to row b's candidate list where v >= ntau[b] and extra(i, j, v) holds.  The 16 lanes of a row claim
// their slots with ONE integer atomic (list order varies from run to run; the select kernel sorts, so the results do not).
template <class Row, class Extra>
__device__ __forceinline__ void l1_epi_append(Row row, const L1Pos& p, const LinkRankArgs& a, Extra extra) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = p.b0 + p.ty * 4 + i;
        const bool row_ok = b < a.B;
        const float nt = row_ok ? a.ntau[(int64_t)b * a.tau_stride] : INFINITY;
        bool pass[4];
        float v[4];
        row(i, v);
        int c = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pass[j] = row_ok && p.n0 + p.tx * 4 + j < a.N && v[j] >= nt;
            pass[j] = pass[j] && extra(i, j, v[j]);
            c += pass[j] ? 1 : 0;
        }
        if (!__any(c)) continue;                              // wave-uniform: most tiles append nothing
        int inc = c;                                          // inclusive prefix over the row's 16 lanes
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const int t = __shfl_up(inc, o, 16);
            if (p.tx >= o) inc += t;
        }
        const int tot = __shfl(inc, 15, 16);
        int base = 0;
        if (p.tx == 0 && tot) base = atomicAdd(a.cnt + b, tot);
        base = __shfl(base, 0, 16);
        int slot = base + inc - c;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (pass[j]) {
                if (slot < a.cap) {
                    a.cval[(int64_t)b * a.cap + slot] = v[j];
                    a.cidx[(int64_t)b * a.cap + slot] = p.n0 + p.tx * 4 + j;
                }
                ++slot;
            }
    }
}

// count epilogue: rank[b] += #{n : v(b, n) before gs[b]}, "before" = smaller (LARGER: larger), or equal with an index below gold_b.
// 4 rows x 4 columns per thread; the 16 threads of a row (tx = 0..15: consecutive lanes) are summed with DPP; integer atomics.
template <bool LARGER, class Row>
__device__ __forceinline__ void l1_epi_count(Row row, const L1Pos& p, const LinkRankArgs& a) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = p.b0 + p.ty * 4 + i;
        const bool row_ok = b < a.B;
        const float gs = row_ok ? a.gs[b] : 0.f;
        const int g = row_ok ? a.gold[b] : 0;
        float v[4];
        row(i, v);
        int c = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = p.n0 + p.tx * 4 + j;
            const float sc = v[j];
            c += (row_ok && n < a.N && ((LARGER ? sc > gs : sc < gs) || (sc == gs && n < g))) ? 1 : 0;
        }
        c += __shfl_xor(c, 1);
        c += __shfl_xor(c, 2);
        c += __shfl_xor(c, 4);
        c += __shfl_xor(c, 8);
        if (p.tx == 0 && row_ok && c) atomicAdd(a.rank + b, c);
    }
}

// stats epilogue: the softmax statistics of row b's logits scale * v(b, n), v = -dist, over THIS tile's 64 columns, the candidates
// outside C_b (include/jmac_hip.h: listed by the index and not the row's gold) masked to -inf BEFORE anything is reduced.  The 16
// lanes of a row agree on (max v, lowest n that attains it), then sum e^u and e^u u with u = scale (v - max) <= 0, and lane 0
// plain-stores ONE float4 (max v, sum e, sum e u, arg) at part[tile column][b]: no atomics, every (part, b) written exactly once
// by a fixed lane in a fixed order of additions, so the bits do not depend on the grid or on which rows share the tile.  A part
// with nothing left stores sum = 0 (SsState skips it).  This is sim_gemm_kernel's SG_STATS row side on -dist.
template <class Row>
__device__ __forceinline__ void l1_epi_stats(Row row, const L1Pos& p, const LinkRankArgs& a) {
    float4* const part = reinterpret_cast<float4*>(a.S) + (int64_t)(p.n0 / L1_T) * a.B;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = p.b0 + p.ty * 4 + i;
        const bool row_ok = b < a.B;                              // the same for the row's 16 lanes
        const int2 rg = row_ok ? a.rng[b] : make_int2(0, 0);
        const int g = (row_ok && a.gold != nullptr) ? a.gold[b] : -1;
        float v[4];
        row(i, v);
        float best = -INFINITY;
        int arg = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = p.n0 + p.tx * 4 + j;
            bool in = row_ok && n < a.N;
            if (in && rg.x < rg.y && n != g) in = !tail_listed(a.filt_idx, rg.x, rg.y, n);
            v[j] = in ? v[j] : -INFINITY;
            if (v[j] > best) {                                    // strict: the lowest index keeps a tie
                best = v[j];
                arg = n;
            }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const float ob = __shfl_xor(best, o);
            const int oa = __shfl_xor(arg, o);
            if (ob > best || (ob == best && oa < arg)) {
                best = ob;
                arg = oa;
            }
        }
        float z = 0.f, y = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) sg_exp_term(v[j], best, a.scale, z, y);
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            z += __shfl_xor(z, o);
            y += __shfl_xor(y, o);
        }
        if (p.tx == 0 && row_ok) part[b] = make_float4(best, z, y, __int_as_float(arg));
    }
}

// The prep kernels' walk over query b's listed candidates -- entry 0 the gold g, then the filter entries [f0, f1) -- a.rows at a
// time: rank[b] starts at 1 - #{filtered entries before the gold}, gs[b] = the gold's value.  value(nc, cand) is called by the whole
// block once cand[0, nc) is visible and may use barriers; lane t < nc returns the value of candidate cand[t] (-1: a skipped entry,
// any value will do) with the tile kernel's bits, so exact ties resolve by index as in the materialised path.
constexpr int LR_ROWS = 16;                        // at most; fewer when nl * d is large (60 KB of LDS)
template <class Value>
__device__ __forceinline__ void link_prep_walk(const LinkRankArgs& a, int b, int g, int f0, int f1, Value value) {
    __shared__ float gs_sh;
    __shared__ int cand[LR_ROWS];
    __shared__ int red[kBlock / 64];
    const int n_list = 1 + (f1 - f0);               // entry 0 = the gold
    float gs = 0.f;
    int cnt = 0;
    for (int c0 = 0; c0 < n_list; c0 += a.rows) {
        const int nc = min(a.rows, n_list - c0);
        __syncthreads();                            // previous chunk consumed; the caller's own LDS rows complete
        if (threadIdx.x < nc) {
            const int c = c0 + threadIdx.x;
            int n = c == 0 ? g : a.filt_idx[f0 + c - 1];
            if (c > 0 && (n == g || n < 0 || n >= a.N)) n = -1;      // skipped entries (as jmac_filtered_rank_f32)
            cand[threadIdx.x] = n;
        }
        __syncthreads();
        const float sc = value(nc, cand);
        if (c0 == 0 && threadIdx.x == 0) gs_sh = sc;
        __syncthreads();
        gs = gs_sh;
        if (threadIdx.x < nc && !(c0 == 0 && threadIdx.x == 0)) {
            const int n = cand[threadIdx.x];
            if (n >= 0) cnt += (sc < gs || (sc == gs && n < g)) ? 1 : 0;
        }
    }
    cnt = wave_sum_i(cnt);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kBlock / 64; ++w) t += red[w];
        a.gs[b] = gs;
        a.rank[b] = 1 - t;
    }
}

// one block per query: (1) its rows er_l = E_l[h] +/- R_l[r] (rounded to TT) -> workspace and LDS; (2) link_prep_walk over the
// listed candidates: their table rows are staged into LDS with coalesced loads, then one lane per candidate runs l1_seq_sum.
// INDEXED: the filter range comes from the known-tail index -- wave 0 searches (h_b, r_b), the block reads the range from LDS.
// RANK = false (top-k, statistics without gold): only (1) and the lookup, whose range goes to a.rng[b].  RNG: the range is written
// (always without RANK; with it for the statistics in evaluation mode, which need gs AND the range).
template <typename TT, bool INDEXED, bool RANK = true, bool RNG = !RANK>
__global__ __launch_bounds__(kBlock) void link_rank_prep_kernel(LinkRankArgs a) {
    extern __shared__ float lr_sh[];                // [nl*dq] query rows (widened) + [LR_ROWS][nl*dq + 1] candidate rows
    __shared__ int2 rng_sh;
    const int b = blockIdx.x, d = a.d, dq = a.dq, W = a.nl * dq, WS = W + 1;
    float* const erow = lr_sh;
    float* const crow = lr_sh + W;
    const int hb = a.h[b], rb = a.r[b], g = RANK ? a.gold[b] : 0;
    TT* const er = static_cast<TT*>(a.er);
    if constexpr (INDEXED)
        if (threadIdx.x < 64) {                     // wave 0 looks the range up while the others start on the query rows
            const int2 rg = tail_range(a, hb, rb);
            if (threadIdx.x == 0) rng_sh = rg;
        }
    for (int l = 0; l < a.nl; ++l)
        for (int k = threadIdx.x; k < dq; k += kBlock) {
            float v = 0.f;
            if (k < d) v = a.ent[l][(int64_t)hb * a.ld_ent[l] + k] + a.sign * a.rel[l][(int64_t)rb * a.ld_rel[l] + k];
            TT* dst = er + ((int64_t)l * a.B + b) * dq + k;
            st1(dst, v);
            erow[l * dq + k] = ld1(dst);            // what the tile kernel will read back (bf16: rounded)
        }
    int f0, f1;
    if constexpr (INDEXED) {
        __syncthreads();
        f0 = rng_sh.x, f1 = rng_sh.y;
    } else {
        f0 = a.filt_ptr ? a.filt_ptr[b] : 0, f1 = a.filt_ptr ? a.filt_ptr[b + 1] : 0;
    }
    if constexpr (RNG)
        if (threadIdx.x == 0) a.rng[b] = make_int2(f0, f1);
    if constexpr (!RANK) return;
    link_prep_walk(a, b, g, f0, f1, [&](int nc, const int* cand) -> float {
        for (int i = threadIdx.x; i < nc * W; i += kBlock) {
            const int rI = i / W, q = i - rI * W, l = q / dq, k = q - l * dq;
            const int n = cand[rI];
            float v = 0.f;
            if (n >= 0 && k < d) v = ld1(static_cast<const TT*>(a.tab[l]) + (int64_t)n * a.ld_tab[l] + k);
            crow[rI * WS + q] = v;
        }
        __syncthreads();
        float acc = 0.f;
        const int t = tid_again();                  // (the lane's row address is formed here, not held across the chunk loop)
        if (t < nc)
            for (int l = 0; l < a.nl; ++l) acc = l1_seq_sum<true>(acc, erow + l * dq, crow + t * WS + l * dq, d);
        return acc;
    });
}

// the tile body over one KG's concatenated (layer, k) axis, with these epilogues:
//   LR_COUNT   count the entries that rank before the gold                                   (jmac_linkpred_rank_*)
//   LR_STORE   S[b, n - n_off] = -dist[b, n]: the column sample (or the whole narrow matrix)  (jmac_linkpred_topk_*)
//   LR_FILTER  append (-dist, n) where dist <= tau_b to row b's candidate list
// STORE, FILTER and STATS cover columns [n_off, N) (STATS: n_off = 0).
// The same epilogues on the Manhattan alignment value c = csls_value(1 - dist, r1, r2), or s = 1 - dist when r1 == NULL, larger
// first (jmac_l1_csls_*; what sim_gemm_kernel's SG_CSLS_* epilogues are to the cosine similarity):
//   LR_CSLS_COUNT   count the columns whose c beats gs[b] = c(b, gold_b): larger, or equal with an index below gold_b
//   LR_CSLS_FILTER  append (c, n) where c >= tau_b
//   LR_CSLS_VIABLE  ... and tk_pack(c, row_id[b]) > best[n]: the suitor would displace what reviewer n holds
// and, on -dist again:
//   LR_STATS   per 64-column part, the softmax statistics of -scale * dist over the query's candidate set (jmac_linkpred_stats_*)
enum { LR_COUNT = 0, LR_STORE = 1, LR_FILTER = 2, LR_CSLS_COUNT = 3, LR_CSLS_FILTER = 4, LR_CSLS_VIABLE = 5, LR_STATS = 6 };

// the epilogue EPI on a tile's distances: it decides on dist (COUNT), -dist (STORE, FILTER) or the alignment value (LR_CSLS_*)
template <int EPI>
__device__ __forceinline__ void l1_epilogue(const float (&dist)[4][4], const L1Pos& p, const LinkRankArgs& a) {
    constexpr bool CSLS = EPI >= LR_CSLS_COUNT && EPI <= LR_CSLS_VIABLE;
    const bool cs = CSLS && a.r1 != nullptr;                   // block-uniform
    float r2v[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (CSLS)
        if (cs) {
#pragma unroll
            for (int j = 0; j < 4; ++j) r2v[j] = a.r2[min(p.n0 + p.tx * 4 + j, a.N - 1)];
        }
    auto row = [&](int i, float (&v)[4]) {
        float r1b = 0.f;
        if constexpr (CSLS) r1b = (cs && p.b0 + p.ty * 4 + i < a.B) ? a.r1[p.b0 + p.ty * 4 + i] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (CSLS) v[j] = cs ? csls_value(1.f - dist[i][j], r1b, r2v[j]) : 1.f - dist[i][j];
            else v[j] = EPI == LR_COUNT ? dist[i][j] : -dist[i][j];
        }
    };
    if constexpr (EPI == LR_STORE) l1_epi_store(row, p, a.B, a.N, a.S, a.ldS, a.n_off);
    else if constexpr (EPI == LR_FILTER || EPI == LR_CSLS_FILTER) l1_epi_append(row, p, a, [](int, int, float) { return true; });
    else if constexpr (EPI == LR_CSLS_VIABLE) {
        unsigned long long bw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bw[j] = a.best[min(p.n0 + p.tx * 4 + j, a.N - 1)];
        l1_epi_append(row, p, a, [&](int i, int j, float c) {
            const int b = p.b0 + p.ty * 4 + i;
            return tk_pack(c, b < a.B ? a.row_id[b] : 0) > bw[j];
        });
    } else if constexpr (EPI == LR_STATS) l1_epi_stats(row, p, a);
    else l1_epi_count<CSLS>(row, p, a);
}

template <typename TT, bool VEC, int EPI = LR_COUNT>
__global__ __launch_bounds__(kBlock) void link_rank_tile_kernel(LinkRankArgs a) {
    __shared__ __attribute__((aligned(16))) float As[2][L1_K][L1_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][L1_K][L1_LD];
    const int B = a.B, N = a.N, d = a.d;
    const L1Pos p = l1_pos(blockIdx.y * L1_T, (EPI == LR_COUNT ? 0 : a.n_off) + blockIdx.x * L1_T);
    const bool a_ok = p.b0 + p.lrow < B, b_ok = p.n0 + p.lrow < N;
    const int64_t arow = a_ok ? p.b0 + p.lrow : B - 1, brow = b_ok ? p.n0 + p.lrow : N - 1;
    const int nk = (d + L1_K - 1) / L1_K;                      // slabs: layer-major, k inside
    const TT* const er = static_cast<const TT*>(a.er);
    float acc[4][4] = {};
    l1_slab_loop<VEC>(acc, As, Bs, p, a.nl * nk, d, a_ok, b_ok, [&](int s, float4& ra, float4& rb) {
        const int l = s / nk, k0 = (s - l * nk) * L1_K;
        ra = l1_load<TT, VEC>(er + (int64_t)l * B * a.dq, a.dq, arow, a_ok, k0 + p.lk, d);
        rb = l1_load<TT, VEC>(static_cast<const TT*>(a.tab[l]), a.ld_tab[l], brow, b_ok, k0 + p.lk, d);
        return k0;
    });
    l1_epilogue<EPI>(acc, l1_pos_again(p), a);
}

// ------------------------------------------------------------------------------------------------
// similarity GEMM  C = A * B^T  on the fp32-input MFMA (32x32x2), 128x128 or 128x256 tile per 4-wave block, K staged 16 deep
// ------------------------------------------------------------------------------------------------
// Tile: 128 rows x (64 WJ) columns per 4-wave block, wave grid 2 x 2, a wave owns 64 x (32 WJ).  WJ = 2: the 128 x 128 tile of
// rounds 1-5 (64 accumulator registers, 3 blocks per CU); WJ = 4: 128 x 256 (128 accumulator registers, 2 blocks per CU): per flop
// a quarter fewer operand bytes through L2 and LDS and half as many barriers (round 6: +3.5 % where its rounds of resident blocks are
// no coarser, profiles/r6_simgemm_ablation.txt).  launch_sim picks per shape.  The contraction order per output
// element is the same for both (planes k = 8q + 4h + s), so the results are bit-identical whichever runs.
constexpr int SG_T = 128;             // (SG_K, the 16-deep k slab: sim_rescore.h)
constexpr int SG_PLANE = SG_T * 4 + 8;      // floats per (sub-slab q, k-half h) plane; +8: the 4 planes a wave store
                                            // instruction touches start on different banks
constexpr int SG_IMG = 4 * SG_PLANE;        // one operand slab: planes (q, h) = (0,0) (0,1) (1,0) (1,1)
template <int WJ>
struct SgTile {
    static constexpr int TN = 64 * WJ;              // tile columns
    static constexpr int PLANE_B = TN * 4 + 8;      // B operand's plane
    static constexpr int IMG_B = 4 * PLANE_B;
    static constexpr int LB = TN / 64;              // float4s per thread of one B slab (A: 2)
    static constexpr int SUPER_N = 8 * 2 / WJ;      // super-tile of 1024 x 1024 outputs: 8 x 8 tiles of 128 x 128, or 8 x 4 of 128 x 256
    static constexpr int OCC = WJ == 2 ? 3 : 2;     // resident blocks per CU the register budget is set for
};
constexpr int SG_SUPER = 8;                 // super-tile of 1024 x 1024 outputs per XCD visit (L2: 2 x 1.2 MB of operand rows at d=300)
constexpr int SG_FL_CAP = 256;              // list epilogues: passing elements a wave collects before it claims their slots

// What happens to a finished tile: the kernel's one epilogue choice.  SgEpiTraits<EPI> states, beside each epilogue's description
// below: Ext, the epilogue's arguments (the kernel's last parameter); LISTS, whether it keeps per-wave candidate lists in LDS;
// WIDE, whether the 128 x 256 tile exists for it (launch_sim chooses between the tiles only then).
enum SgEpi { SG_STORE, SG_FILTER, SG_STATS, SG_CSLS_COUNT, SG_CSLS_FILTER, SG_CSLS_VIABLE, SG_LSE };
template <int EPI> struct SgEpiTraits;

// SG_STORE: C = A B^T is stored.
struct SimStore {};
template <> struct SgEpiTraits<SG_STORE> {
    typedef SimStore Ext;
    static constexpr bool LISTS = false, WIDE = true;
};

// SG_FILTER: the scores are not stored.  An element that reaches its row's threshold tau (a lower bound of the row's k-th
// largest score, taken from a column sample: jmac_sim_topk_f32) is appended to the row's candidate list instead -- the running
// top-k of SURVEY K8: the L x N matrix never exists.
struct SimFilter {
    const float* tau;        // tau[m * tau_stride]
    int64_t tau_stride;
    int* cnt;                // [M] candidates seen per row (may exceed cap: the row then recomputes its scores, see below)
    float* cval;             // [M, cap]
    int* cidx;               // [M, cap]
    int cap;
    int n_off;               // the product covers columns [n_off, n_off + N) of the full matrix: candidate index = n_off + n
};
template <> struct SgEpiTraits<SG_FILTER> {
    typedef SimFilter Ext;
    static constexpr bool LISTS = true, WIDE = true;
    static __device__ const SimFilter& lists(const Ext& e) { return e; }
};

// SG_STATS: the scores are not stored either.  Every wave reduces its 64 x 64 part of the tile to partial softmax statistics of
// the logits z = scale * S, once along its rows and once along its columns (jmac_sim_softmax_stats_f32): per row and 64-column
// part (max S, l = sum e^(z - max z), t = sum e^(z - max z) (z - max z), first column of the maximum), per column and 64-row part
// the same.  A part's maximum is exact (taken before the exponentials), the parts are combined by sim_stats_merge_kernel with the
// online form.  Partials are addressed by the part's POSITION in the matrix, written once with plain stores and merged in
// ascending order: the results do not depend on the grid, the tile walk or the device's CU count.  The reductions stay in
// registers (DPP inside a 16-lane row, one cross-lane exchange per further step): no wave touches the operand LDS buffers behind
// the last slab's barrier, as in the other epilogues.  Written for the 128 x 128 tile only (one partial layout: a part is 64 rows
// or 64 columns).
struct SimStats {
    float4* rpart;           // [ceil(N / 64)][M]    (max S, l, t, column index bits)
    float* cpart;            // [ceil(M / 64)][N][3] (scale * max S, l, t): the format of col_softmax_stats_kernel; NULL: rows only
    float2* cbest;           // [ceil(M / 64)][N]    (max S, row index bits)
    float scale;             // > 0
};
template <> struct SgEpiTraits<SG_STATS> {
    typedef SimStats Ext;
    static constexpr bool LISTS = false, WIDE = false;
};
// SG_CSLS_COUNT / SG_CSLS_FILTER: the scores are not stored, and every epilogue decision is taken on the CSLS-rescored value
// c(m, n) = csls_value(S[m, n], r1[m], r2[n]) (jmac_sim_csls_rank_f32 / jmac_sim_csls_topk_f32).
//   COUNT   per row m: the columns whose c beats the row's gold value gval[m] (larger, or equal with a column index below
//           gold[m]) are counted inside the wave and added to rank[m] with ONE integer atomic per (wave, row): sums of integers,
//           so the result is the same bits whatever the grid, the tile or the order of the blocks.
//   FILTER  the SimFilter scheme with tau, the comparison and the appended value all in c.
struct SimCsls {
    SimFilter f;             // FILTER: as above (tau in c; n_off also offsets r2).  COUNT: unused
    const float* r1;         // [M]; NULL (with r2): c = S
    const float* r2;         // [n_off + N]
    const float* gval;       // COUNT: [M] c(m, gold[m]), the bits this kernel produces for that element (csls_gold_kernel)
    const int32_t* gold;     // COUNT: [M]
    int32_t* rank;           // COUNT: [M], preset to 1
};
template <> struct SgEpiTraits<SG_CSLS_COUNT> {
    typedef SimCsls Ext;
    static constexpr bool LISTS = false, WIDE = true;
};
template <> struct SgEpiTraits<SG_CSLS_FILTER> {
    typedef SimCsls Ext;
    static constexpr bool LISTS = true, WIDE = true;
    static __device__ const SimFilter& lists(const Ext& e) { return e.f; }
};
// SG_CSLS_VIABLE: the FILTER form for a suitor that may only list the reviewers it can still win (jmac_sim_csls_topk_viable_f32):
// an element is appended iff it reaches tau AND tk_pack(c(m, n), row_id[m]) > best[n] -- it would displace what reviewer n holds.
// r1 == NULL (with r2) is decided at run time here: c = S.
struct SimViable : SimCsls {
    const int32_t* row_id;               // [M] the suitor id of row m (the rows are a gathered subset): the tie-break of the word
    const unsigned long long* best;      // [n_off + N] the reviewers' words, 0 = free
};
template <> struct SgEpiTraits<SG_CSLS_VIABLE> {
    typedef SimViable Ext;
    static constexpr bool LISTS = true, WIDE = true;
    static __device__ const SimFilter& lists(const Ext& e) { return e.f; }
};
// SG_LSE: the scores are not stored; every wave reduces its 64 x 64 part to partial log-sum-exps with additive offsets
// (jmac_sim_lse_f32: the half-steps of a log-domain Sinkhorn iteration).  Per row and 64-column part (max z, sum e^(z - max z)) of
// z = fma(scale, S[m, n], col_add[n]); per column and 64-row part the same of z = fma(scale, S[m, n], row_add[m]).  The SimStats
// scheme otherwise: exact part maxima, partials addressed by the part's position, plain stores, merged in ascending order by
// sim_lse_merge_kernel; reductions in registers.  A side whose partial pointer is NULL is skipped.  128 x 128 tile only.
struct SimLse {
    float2* rpart;           // [ceil(N / 64)][M] (max z, l); NULL: no row side
    float2* cpart;           // [ceil(M / 64)][N] (max z, l); NULL: no column side
    const float* col_add;    // [N] added to the logits of the row side; NULL: 0
    const float* row_add;    // [M] added to the logits of the column side; NULL: 0
    float scale;             // > 0
};
template <> struct SgEpiTraits<SG_LSE> {
    typedef SimLse Ext;
    static constexpr bool LISTS = false, WIDE = false;
};

// the DPP-selected lane's v (old = 0 with bound_ctrl: every source lane of the controls used here exists; ROWS: rows written)
template <int CTRL, int ROWS = 0xF>
__device__ __forceinline__ float sg_dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROWS, 0xF, true));
}
// max(v, v of the DPP-selected lane) as ONE instruction.  Through fmaxf the compiler emits a move, a NaN-quieting v_max x, x of
// the moved value (it knows nothing about it) and the v_max: three.  s_nop 1 = the two wait states between a VALU write of v and
// a DPP read of it (nothing pads the inside of an asm statement).  No NaN reaches these (excluded elements are -inf).
#define JMAC_SG_MAX_DPP(v, ctrl) asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=v"(v) : "v"(v))
__device__ __forceinline__ float sg_max(float a, float b) {
    float d;
    asm("v_max_f32_e32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
// Reductions over the 32 lanes of a half-wave.  xor 1, xor 2 as quad permutes, then row_half_mirror and row_mirror (the values
// are uniform inside the groups they exchange): every lane of a 16-lane row holds its row's result.
// max: the other row's value comes through one bpermute, every lane of the half ends with the same bits.
__device__ __forceinline__ float sg_half_max(float v) {
    JMAC_SG_MAX_DPP(v, "quad_perm:[1,0,3,2]");
    JMAC_SG_MAX_DPP(v, "quad_perm:[2,3,0,1]");
    JMAC_SG_MAX_DPP(v, "row_half_mirror");
    JMAC_SG_MAX_DPP(v, "row_mirror");
    return sg_max(v, __shfl_xor(v, 16, 64));
}
// sum: row_bcast:15 adds the lower row's sum into the upper row -- only lanes 16..31 / 48..63 hold the half's sum (lower + upper)
__device__ __forceinline__ float sg_half_sum_upper(float v) {
    v += sg_dpp_f<0xB1>(v);
    v += sg_dpp_f<0x4E>(v);
    v += sg_dpp_f<0x141>(v);
    v += sg_dpp_f<0x140>(v);
    return v + sg_dpp_f<0x142, 0xA>(v);
}
// Both halves' values of x in every lane: lo = x of lane (l & 31), hi = x of lane (l & 31) + 32.  v_permlane32_swap of two copies
// (inline asm with its wait states, for the reason given at halves_meet in aggregate.hip).
__device__ __forceinline__ void sg_halves(float x, float& lo, float& hi) {
    lo = x;
    hi = x;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 0" : "+v"(lo), "+v"(hi));
}

// e^(z - max z) of one logit of the log-sum-exp epilogue; an excluded element (z = -inf, or the whole part excluded: NaN) gives 0
__device__ __forceinline__ float sg_lse_term(float z, float mx) { return fast_exp(fmaxf(z - mx, -1e30f)); }

// Where a lane stands in the tile it has just accumulated: built once per tile, read by every epilogue.
// C/D map of the 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
struct SgPos {
    int m0, n0, M, N;        // the tile's first row and column, the matrix
    int wm, wn;              // the wave's place in the block's 2 x 2 grid: it owns rows m0 + 64 wm .., columns n0 + 32 WJ wn ..
    int lane, r, h;          // r = lane & 31, h = lane >> 5
    bool full;               // block-uniform: the whole tile is inside the matrix
};

// SG_CSLS_COUNT (SimCsls above)
template <int WJ>
__device__ __forceinline__ void sg_epi_count(f32x16 (&acc)[2][WJ], const SgPos& p, const SimCsls& ext) {
    const int m0 = p.m0, n0 = p.n0, M = p.M, N = p.N, wm = p.wm, wn = p.wn, lane = p.lane, r = p.r, h = p.h;
    // lane l <-> row l of the wave's 64-row block for everything that is per row: ONE coalesced load each, the value
    // of accumulator row (i, reg) comes out with v_readlane (rows (i, reg, h = 0 / 1) are 4 apart), as tau below
    const int mrow = min(m0 + wm * 64 + lane, M - 1);
    float grow = ext.gval[mrow];
    int gcol = ext.gold[mrow];
    const bool rescore = ext.r1 != nullptr;
    float r1row = rescore ? ext.r1[mrow] : 0.f;
    float r2col[WJ];
    unsigned long long inside[WJ];                  // columns >= N hold zero-padded operands: they never count
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
        const int n = n0 + wn * 32 * WJ + j * 32 + r;
        r2col[j] = rescore ? ext.r2[min(n, N - 1)] : 0.f;
        inside[j] = __ballot(n < N);
    }
    int hits = 0;                                      // of row `lane` of the block
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int rbase = i * 32 + (reg & 3) + 8 * (reg >> 2);           // compile-time
            // One row pair at a time: the empty statement makes this pair's v_readlane sources depend on the previous
            // pair's sum.  Left free, the scheduler hoists all 192 lane reads and keeps all 64 popcounts in scalar
            // registers (218 / 346 spilled SGPRs at WJ = 2 / 4).
            asm volatile("" : "+v"(grow), "+v"(r1row), "+v"(gcol), "+v"(hits));
            // (both lane reads first, then a select: read inside the arms of `h ? :` they become two exec-masked branches)
            const float gs0 = bcast_f(grow, rbase), gs1 = bcast_f(grow, rbase + 4);
            const float ra0 = bcast_f(r1row, rbase), ra1 = bcast_f(r1row, rbase + 4);
            const int g0 = __builtin_amdgcn_readlane(gcol, rbase), g1 = __builtin_amdgcn_readlane(gcol, rbase + 4);
            const float gs = h ? gs1 : gs0, r1v = h ? ra1 : ra0;
            const int g = h ? g1 : g0;
            int c0 = 0, c1 = 0;                        // wave-uniform: the hits of row rbase / rbase + 4
#pragma unroll
            for (int j = 0; j < WJ; ++j) {
                const int n = n0 + wn * 32 * WJ + j * 32 + r;
                const float v = rescore ? csls_value(acc[i][j][reg], r1v, r2col[j]) : acc[i][j][reg];
                const unsigned long long mask = __ballot(v > gs || (v == gs && n < g)) & inside[j];
                c0 += __popc((unsigned)mask);
                c1 += __popc((unsigned)(mask >> 32));
            }
            // every lane is written exactly once per tile: (i, reg) -> rbase, rbase + 4 covers 0 .. 63 (a select on
            // lane == rbase instead keeps 64 loop-invariant compare masks alive across the tile loop: 95 spilled SGPRs)
            asm("s_nop 0\n\tv_writelane_b32 %0, %1, %2\n\tv_writelane_b32 %0, %3, %4"
                : "+v"(hits)
                : "s"(c0), "n"(rbase), "s"(c1), "n"(rbase + 4));
        }
    if (hits != 0 && m0 + wm * 64 + lane < M) atomicAdd(ext.rank + m0 + wm * 64 + lane, hits);      // rows >= M: no such row
}

// SG_LSE (SimLse above)
__device__ __forceinline__ void sg_epi_lse(f32x16 (&acc)[2][2], const SgPos& p, const SimLse& ext) {
    const int m0 = p.m0, n0 = p.n0, M = p.M, N = p.N, wm = p.wm, wn = p.wn, lane = p.lane, r = p.r, h = p.h;
    const float scale = ext.scale;
    const int mrow0 = m0 + wm * 64, ncol0 = n0 + wn * 64;
    const int ncol[2] = {ncol0 + r, ncol0 + 32 + r};
    const int mlim = M - mrow0 - 4 * h;                       // row (i, reg) of this lane is inside iff its base < mlim
    // elements outside the matrix become -inf, and so do their logits (scale > 0, finite offsets): as in STATS below
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int rbase = i * 32 + (reg & 3) + 8 * (reg >> 2);
                const unsigned inside = (unsigned)(rbase - mlim) & (unsigned)(ncol[j] - N) & 0x80000000u;
                acc[i][j][reg] = fminf(acc[i][j][reg], __uint_as_float(0xff800000u ^ inside));
            }
    // rows: (i, reg) is one row per half-wave; the lane's two columns carry their offsets.  Lane 16 of the half stores.
    if (ext.rpart != nullptr) {
        const float ca0 = ext.col_add ? ext.col_add[min(ncol[0], N - 1)] : 0.f;
        const float ca1 = ext.col_add ? ext.col_add[min(ncol[1], N - 1)] : 0.f;
        float2* const rdst = ext.rpart + (int64_t)(ncol0 >> 6) * M + mrow0 + 4 * h;
        const bool rstore = r == 16 && ncol0 < N;             // (a part wholly outside the matrix does not exist)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int rbase = i * 32 + (reg & 3) + 8 * (reg >> 2);
                const float z0 = fmaf(scale, acc[i][0][reg], ca0), z1 = fmaf(scale, acc[i][1][reg], ca1);
                const float mx = sg_half_max(sg_max(z0, z1));
                float l = sg_lse_term(z0, mx) + sg_lse_term(z1, mx);
                l = sg_half_sum_upper(l);
                if (rstore && rbase < mlim) rdst[rbase] = make_float2(mx, l);
                if (reg & 1) __builtin_amdgcn_sched_barrier(0);      // two rows' chains interleave, no more
            }
    }
    // columns: a lane holds 32 rows of its column per j, the other half-wave the other 32.  The rows' offsets: ONE
    // coalesced load (lane l <-> row l of the wave's 64 rows), read out per accumulator row as in the count epilogue; the
    // logits replace the scores in place (the row side is done with them).
    if (ext.cpart != nullptr) {
        float radd = ext.row_add ? ext.row_add[min(mrow0 + lane, M - 1)] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int rbase = i * 32 + (reg & 3) + 8 * (reg >> 2);
                const float a0 = bcast_f(radd, rbase), a1 = bcast_f(radd, rbase + 4);
                const float av = h ? a1 : a0;
                acc[i][0][reg] = fmaf(scale, acc[i][0][reg], av);
                acc[i][1][reg] = fmaf(scale, acc[i][1][reg], av);
            }
        float cm[2], cl[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) mx = sg_max(mx, acc[i][j][reg]);
            float lo, hi;
            sg_halves(mx, lo, hi);
            mx = sg_max(lo, hi);
            float l = 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) l += sg_lse_term(acc[i][j][reg], mx);
            sg_halves(l, lo, hi);
            cl[j] = lo + hi;
            cm[j] = mx;
        }
        // the lower half-wave stores the columns of j = 0, the upper half those of j = 1
        const int col = h ? ncol[1] : ncol[0];
        if (col < N && mrow0 < M) ext.cpart[(int64_t)(mrow0 >> 6) * N + col] = make_float2(h ? cm[1] : cm[0], h ? cl[1] : cl[0]);
    }
}

// SG_STATS (SimStats above)
__device__ __forceinline__ void sg_epi_stats(f32x16 (&acc)[2][2], const SgPos& p, const SimStats& ext) {
    const int m0 = p.m0, n0 = p.n0, M = p.M, N = p.N, wm = p.wm, wn = p.wn, r = p.r, h = p.h;
    const float scale = ext.scale;
    const int mrow0 = m0 + wm * 64, ncol0 = n0 + wn * 64;
    const int ncol[2] = {ncol0 + r, ncol0 + 32 + r};
    // elements outside the matrix (ragged tiles: the clamped loads' duplicates) leave both reductions as -inf
    const int mlim = M - mrow0 - 4 * h;                       // row (i, reg) of this lane is inside iff its base < mlim
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                // min(s, +inf) = s inside, min(s, -inf) outside; the bound's sign comes from the two differences' sign bits
                // (64 compare masks would not fit the scalar registers)
                const int rbase = i * 32 + (reg & 3) + 8 * (reg >> 2);
                const unsigned inside = (unsigned)(rbase - mlim) & (unsigned)(ncol[j] - N) & 0x80000000u;
                acc[i][j][reg] = fminf(acc[i][j][reg], __uint_as_float(0xff800000u ^ inside));
            }
    // rows: (i, reg) is one row per half-wave, its 64 columns are 2 registers x 32 lanes.  The maximum reaches every lane
    // (the exponentials need it), the two sums only the half's upper 16 lanes, and lane 16 of the half stores the row at
    // once (16 bytes; results kept for one wide store at the end would stay live through all 32 chains and spill).  The
    // first column of the maximum is scalar work: ballots of v == max, lowest set bit of each half.
    float4* const rdst = ext.rpart + (int64_t)(ncol0 >> 6) * M + mrow0 + 4 * h;
    const bool rstore = r == 16 && ncol0 < N;                 // (a part wholly outside the matrix does not exist)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int rbase = i * 32 + (reg & 3) + 8 * (reg >> 2);
            const float v0 = acc[i][0][reg], v1 = acc[i][1][reg];
            const float mx = sg_half_max(sg_max(v0, v1));
            const unsigned long long e0 = __ballot(v0 == mx), e1 = __ballot(v1 == mx);
            // per half: bits 0..31 = its lanes' j = 0 columns, 32..63 = their j = 1 columns, i.e. the part's column order
            const int al = __builtin_ffsll((long long)((e0 & 0xffffffffull) | (e1 << 32))) - 1;      // wave-uniform
            const int ah = __builtin_ffsll((long long)((e0 >> 32) | (e1 & 0xffffffff00000000ull))) - 1;
            float l = 0.f, t = 0.f;
            sg_exp_term(v0, mx, scale, l, t);
            sg_exp_term(v1, mx, scale, l, t);
            l = sg_half_sum_upper(l);
            t = sg_half_sum_upper(t);
            if (rstore && rbase < mlim) rdst[rbase] = make_float4(mx, l, t, __int_as_float(ncol0 + (h ? ah : al)));
            // two rows' chains interleave (they fill each other's DPP wait states), no more
            if (reg & 1) __builtin_amdgcn_sched_barrier(0);
        }
    // columns: a lane holds 32 rows of its column per j, the other half-wave the other 32
    if (ext.cpart != nullptr) {
        float cm[2], cl[2], ct[2];
        int ca[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) mx = sg_max(mx, acc[i][j][reg]);
            float lo, hi;
            sg_halves(mx, lo, hi);
            mx = sg_max(lo, hi);
            // the lane's rows in DESCENDING order: the last match is its lowest row of the maximum (128: none)
            int a = 128;
            float l = 0.f, t = 0.f;
#pragma unroll
            for (int i = 1; i >= 0; --i)
#pragma unroll
                for (int reg = 15; reg >= 0; --reg) {
                    a = acc[i][j][reg] == mx ? i * 32 + (reg & 3) + 8 * (reg >> 2) : a;
                    sg_exp_term(acc[i][j][reg], mx, scale, l, t);
                    if ((reg & 3) == 0) __builtin_amdgcn_sched_barrier(0);
                }
            sg_halves(l, lo, hi);
            cl[j] = lo + hi;
            sg_halves(t, lo, hi);
            ct[j] = lo + hi;
            sg_halves(__int_as_float(a + 4 * h), lo, hi);
            ca[j] = mrow0 + min(__float_as_int(lo), __float_as_int(hi));
            cm[j] = mx;
        }
        // the lower half-wave stores the columns of j = 0, the upper half those of j = 1
        const int col = h ? ncol[1] : ncol[0];
        if (col < N && mrow0 < M) {
            const int64_t e = (int64_t)(mrow0 >> 6) * N + col;
            const float mxs = h ? cm[1] : cm[0];
            ext.cpart[e * 3 + 0] = scale * mxs;
            ext.cpart[e * 3 + 1] = h ? cl[1] : cl[0];
            ext.cpart[e * 3 + 2] = h ? ct[1] : ct[0];
            ext.cbest[e] = make_float2(mxs, __int_as_float(h ? ca[1] : ca[0]));
        }
    }
}

// SG_FILTER, SG_CSLS_FILTER, SG_CSLS_VIABLE: one body.  fl_m, fl_n, fl_v: the wave's own lists of SG_FL_CAP entries in LDS.
template <int EPI, int WJ>
__device__ __forceinline__ void sg_epi_lists(f32x16 (&acc)[2][WJ], const SgPos& p, const typename SgEpiTraits<EPI>::Ext& ext, int* fl_m,
                                             int* fl_n, float* fl_v) {
    constexpr bool VIABLE = EPI == SG_CSLS_VIABLE;
    const SimFilter& flt = SgEpiTraits<EPI>::lists(ext);
    const int m0 = p.m0, n0 = p.n0, M = p.M, N = p.N, wm = p.wm, wn = p.wn, lane = p.lane, r = p.r, h = p.h;
    // Passing elements are rare (~k * N / Ns per row: under 1 % of the tile).  A returned global atomic per passing
    // element inside the scan would cost one memory round trip each (measured: the product ran 1.6x longer); the wave
    // first compacts its passing elements into a small LDS list (ballot + prefix popcount, no memory traffic) and
    // then claims their slots with ONE batch of atomics per flush.
    int fcount = 0;                                    // wave-uniform
    auto flush = [&]() {
        __threadfence_block();                         // the list's LDS writes are visible to the whole wave
        for (int e = lane; e < fcount; e += 64) {
            const int m = fl_m[e];
            const int pos = atomicAdd(flt.cnt + m, 1);
            if (pos < flt.cap) {
                flt.cval[(int64_t)m * flt.cap + pos] = fl_v[e];
                flt.cidx[(int64_t)m * flt.cap + pos] = fl_n[e];
            }
        }
        __threadfence_block();
        fcount = 0;
    };
    // thresholds of the wave's 64 rows: ONE coalesced load (lane l <-> row l of the wave's row block); the value for
    // accumulator register (i, reg) comes out of it with two v_readlane (rows (i, reg, h = 0 / 1) are 4 apart)
    const float trow = flt.tau[(int64_t)min(m0 + wm * 64 + lane, M - 1) * flt.tau_stride];
    // CSLS: the row terms travel like tau, a lane's WJ column terms are loaded once per tile
    float r1row = 0.f, r2col[EPI == SG_CSLS_FILTER || VIABLE ? WJ : 1] = {};
    if constexpr (EPI == SG_CSLS_FILTER) {
        r1row = ext.r1[min(m0 + wm * 64 + lane, M - 1)];
#pragma unroll
        for (int j = 0; j < WJ; ++j) r2col[j] = ext.r2[flt.n_off + min(n0 + wn * 32 * WJ + j * 32 + r, N - 1)];
    }
    // VIABLE: the rows' suitor ids travel like tau too, a lane's WJ reviewer words are loaded once per tile
    int ridrow = 0;
    unsigned long long bcol[VIABLE ? WJ : 1] = {};
    bool rescore = false;                              // block-uniform
    if constexpr (VIABLE) {
        rescore = ext.r1 != nullptr;
        ridrow = ext.row_id[min(m0 + wm * 64 + lane, M - 1)];
        if (rescore) r1row = ext.r1[min(m0 + wm * 64 + lane, M - 1)];
#pragma unroll
        for (int j = 0; j < WJ; ++j) {
            const int n = flt.n_off + min(n0 + wn * 32 * WJ + j * 32 + r, N - 1);
            if (rescore) r2col[j] = ext.r2[n];
            bcol[j] = ext.best[n];
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int rbase = i * 32 + (reg & 3) + 8 * (reg >> 2);           // compile-time
            const int m = m0 + wm * 64 + rbase + 4 * h;
            const float tau = h ? bcast_f(trow, rbase + 4) : bcast_f(trow, rbase);
            float r1v = 0.f;
            if constexpr (EPI == SG_CSLS_FILTER || VIABLE) r1v = h ? bcast_f(r1row, rbase + 4) : bcast_f(r1row, rbase);
            int rid = 0;
            if constexpr (VIABLE) rid = h ? bcast_i(ridrow, rbase + 4) : bcast_i(ridrow, rbase);
#pragma unroll
            for (int j = 0; j < WJ; ++j) {
                const int n = n0 + wn * 32 * WJ + j * 32 + r;
                float v = acc[i][j][reg];
                if constexpr (EPI == SG_CSLS_FILTER) v = csls_value(v, r1v, r2col[j]);
                if constexpr (VIABLE) v = rescore ? csls_value(v, r1v, r2col[j]) : v;
                bool pass = m < M && n < N && v >= tau;
                if constexpr (VIABLE) pass = pass && tk_pack(v, rid) > bcol[j];
                const unsigned long long mask = __ballot(pass);
                if (mask != 0ull) {                    // wave-uniform
                    const int np = __popcll(mask);
                    if (fcount + np > SG_FL_CAP) flush();
                    if (pass) {
                        const int slot = fcount + __popcll(mask & ((1ull << lane) - 1ull));
                        fl_m[slot] = m;
                        fl_n[slot] = n + flt.n_off;
                        fl_v[slot] = v;
                    }
                    fcount += np;
                }
            }
        }
    flush();
}

// SG_STORE, interior tile: 32 WJ unconditional stores per wave (the caller follows them with its own instance of the next tile's
// first slab: see tile_prologue)
template <int WJ>
__device__ __forceinline__ void sg_epi_store_interior(const f32x16 (&acc)[2][WJ], const SgPos& p, float* __restrict__ C, int64_t ldc) {
    const int m0 = p.m0, n0 = p.n0, wm = p.wm, wn = p.wn, r = p.r, h = p.h;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < WJ; ++j) {
            float* cbase = C + (int64_t)(m0 + wm * 64 + i * 32 + 4 * h) * ldc + (n0 + wn * 32 * WJ + j * 32 + r);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) cbase[(int64_t)((reg & 3) + 8 * (reg >> 2)) * ldc] = acc[i][j][reg];
        }
}

// SG_STORE, a tile that crosses the matrix's edge: every store behind its bounds test
template <int WJ>
__device__ __forceinline__ void sg_epi_store_ragged(const f32x16 (&acc)[2][WJ], const SgPos& p, float* __restrict__ C, int64_t ldc) {
    const int m0 = p.m0, n0 = p.n0, M = p.M, N = p.N, wm = p.wm, wn = p.wn, r = p.r, h = p.h;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < WJ; ++j)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int64_t m = m0 + wm * 64 + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                const int64_t n = n0 + wn * 32 * WJ + j * 32 + r;
                if (m < M && n < N) C[m * ldc + n] = acc[i][j][reg];
            }
}

// The kernel: the persistent tile walk, the software pipeline, the request for the next tile's first slab, and the dispatch to the
// tile's epilogue above.
template <int EPI, int WJ>
__global__ __launch_bounds__(kBlock, SgTile<WJ>::OCC) void sim_gemm_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ Bm,
                                                          int64_t ldb, int M, int N, int d, float* __restrict__ C, int64_t ldc,
                                                          int tiles_m, int tiles_n, int super_order, int n_ids,
                                                          typename SgEpiTraits<EPI>::Ext ext) {
    static_assert(WJ == 2 || (WJ == 4 && SgEpiTraits<EPI>::WIDE), "this epilogue is written for the 128 x 128 tile only");
    constexpr bool LISTS = SgEpiTraits<EPI>::LISTS;
    // LDS image of one operand slab (16 k): plane (q, h) holds, for every tile row, the 4 floats k = 8q + 4h .. +3.
    // Lane (r = l&31, h = l>>5) of a wave reads its float4 of row r from plane (q, h): 32 lanes x 16 B contiguous,
    // conflict free for ds_read_b128's lane groups.  The MFMA step s of a sub-slab contracts k = {8q+s, 8q+4+s}.
    __shared__ __attribute__((aligned(16))) float As[2][SG_IMG];
    constexpr int SG_TN = SgTile<WJ>::TN, SG_PLANE_B = SgTile<WJ>::PLANE_B, SG_LB = SgTile<WJ>::LB, SG_SUPER_N = SgTile<WJ>::SUPER_N;
    __shared__ __attribute__((aligned(16))) float Bs[2][SgTile<WJ>::IMG_B];
    __shared__ int fl_m[LISTS ? kBlock / 64 : 1][LISTS ? SG_FL_CAP : 1];        // LISTS: per-wave lists of passing elements
    __shared__ int fl_n[LISTS ? kBlock / 64 : 1][LISTS ? SG_FL_CAP : 1];
    __shared__ float fl_v[LISTS ? kBlock / 64 : 1][LISTS ? SG_FL_CAP : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;           // wave grid 2 x 2, each wave 64 x 64

    // Tile ids are walked persistently: block b takes ids b, b + gridDim, ... (gridDim is a multiple of 8, so a block's
    // ids stay on its XCD).  XCD-aware order: workgroup ids are dealt round-robin to the 8 XCDs, so ids {x, x+8, ...}
    // share one L2; those ids walk ONE super-tile of SG_SUPER x SG_SUPER tiles before moving on: its A and B panels
    // stay L2-resident.  Ids that fall outside the matrix (ragged super-tiles) are skipped.
    auto tile_of = [&](int id, int& tm, int& tn) -> bool {
        if (super_order) {
            const int sup_n = (tiles_n + SG_SUPER_N - 1) / SG_SUPER_N, sup_m = (tiles_m + SG_SUPER - 1) / SG_SUPER;
            const int per = SG_SUPER * SG_SUPER_N;
            const int xcd = id & 7, local = id >> 3;
            const int sup = (local / per) * 8 + xcd, within = local % per;
            if (sup >= sup_m * sup_n) return false;
            tm = (sup / sup_n) * SG_SUPER + within / SG_SUPER_N;
            tn = (sup % sup_n) * SG_SUPER_N + within % SG_SUPER_N;
            return tm < tiles_m && tn < tiles_n;
        }
        tm = id / tiles_n;                           // few tiles: plain row-major order, every XCD busy
        tn = id % tiles_n;
        return true;
    };
    auto next_tile = [&](int id, int& tm, int& tn) -> int {     // first valid id >= id, or n_ids
        while (id < n_ids && !tile_of(id, tm, tn)) id += gridDim.x;
        return id < n_ids ? id : n_ids;
    };

    // loader: float4 f = tid + 256 i (i < 2): row = f / 4, k quad kq = f % 4 (4 consecutive lanes read 64 contiguous
    // bytes of a row).  Every load is unconditional at a clamped address (a load behind an exec-mask branch is not
    // overlapped with the MFMAs): rows past the end re-read the last row -- they only feed outputs that are never
    // stored -- and float4s past d (d % 4 == 0, enforced by the launcher) are zeroed at store time.
    auto gload = [&](const float* base, int64_t ld, int row0, int nrows, int k0, auto& v) {
        constexpr int CNT = sizeof(v) / sizeof(float4);
#pragma unroll
        for (int i = 0; i < CNT; ++i) {
            const int f = tid + 256 * i;
            const int row = min(row0 + (f >> 2), nrows - 1), k = k0 + 4 * (f & 3);
            v[i] = ld4(base + (int64_t)row * ld + min(k, d - 4));     // zeroing waits for the data: done at store time
        }
    };
    auto sstore = [&](float* S, const auto& v, int k0) {
        constexpr int CNT = sizeof(v) / sizeof(float4);
        constexpr int PLANE = CNT == 2 ? SG_PLANE : SG_PLANE_B;       // (WJ = 2: the two planes are the same size)
#pragma unroll
        for (int i = 0; i < CNT; ++i) {
            const int f = tid + 256 * i;
            // zeroing as a bit mask (exact, and no select the compiler could turn into a branch: the slab body stays ONE basic block)
            const unsigned keep = k0 + 4 * (f & 3) < d ? 0xffffffffu : 0u;
            const float4 x = make_float4(__uint_as_float(__float_as_uint(v[i].x) & keep), __uint_as_float(__float_as_uint(v[i].y) & keep),
                                         __uint_as_float(__float_as_uint(v[i].z) & keep), __uint_as_float(__float_as_uint(v[i].w) & keep));
            *reinterpret_cast<float4*>(S + (f & 3) * PLANE + (f >> 2) * 4) = x;      // plane index = kq = 2q + h
        }
    };
    const int r = lane & 31, h = lane >> 5;
    const int aoff = h * SG_PLANE + (wm * 64 + r) * 4, boff = h * SG_PLANE_B + (wn * 32 * WJ + r) * 4;
    auto frags = [&](int buf, int q, float4 (&af)[2], float4 (&bf)[WJ]) {
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const float4*>(As[buf] + q * 2 * SG_PLANE + aoff + i * 32 * 4);
#pragma unroll
        for (int j = 0; j < WJ; ++j) bf[j] = *reinterpret_cast<const float4*>(Bs[buf] + q * 2 * SG_PLANE_B + boff + j * 32 * 4);
    };
    f32x16 acc[2][WJ];
    // the 2 WJ accumulators rotate (dependency distance 2 WJ >= 4)
    auto mfma16 = [&](const float4 (&af)[2], const float4 (&bf)[WJ]) {
#define JMAC_SG_STEP(c)                                                                                              \
        _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                                \
            _Pragma("unroll") for (int j = 0; j < WJ; ++j)                                                        \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].c, bf[j].c, acc[i][j], 0, 0, 0);
        JMAC_SG_STEP(x)
        JMAC_SG_STEP(y)
        JMAC_SG_STEP(z)
        JMAC_SG_STEP(w)
#undef JMAC_SG_STEP
    };

    const int nk = (d + SG_K - 1) / SG_K;
    float4 ra[2], rb[SG_LB], af0[2], bf0[WJ], af1[2], bf1[WJ];
    int tm, tn;
    int id = next_tile(blockIdx.x, tm, tn);
    if (id >= n_ids) return;
    // A tile's first slab: staged rows -> LDS buffer 0, slab 1 requested, the first fragments read.  Called for the block's first
    // tile here and for every further tile at the END of the loop body, behind the previous tile's epilogue: a separate instance
    // of the code, so that its wait for the slab's loads is counted on that path alone -- the loads were issued BEFORE the epilogue's
    // stores and vmcnt retires in order, so the wait can leave stores in flight.  At WJ = 2 a wave has 64 stores behind the loads and
    // vmcnt(63) keeps them in flight.  At WJ = 4 it has 128, the 6-bit counter saturates at 63, and the same vmcnt(63) first waits
    // for about 65 of them to be acknowledged: a cost in time only, the results are the same bits.  With the prologue at the loop's top the
    // kernel-entry path (nothing but four loads pending) and the back edge merged into vmcnt(3): every tile began by waiting for
    // the previous tile's stores to be acknowledged (round 6: the "nostore" ablation's 6 %).
    auto tile_prologue = [&](const int m0, const int n0) {
        sstore(As[0], ra, 0);
        sstore(Bs[0], rb, 0);
        if (nk > 1) {
            gload(A, lda, m0, M, SG_K, ra);
            gload(Bm, ldb, n0, N, SG_K, rb);
        }
        __syncthreads();
        frags(0, 0, af0, bf0);
    };
    gload(A, lda, tm * SG_T, M, 0, ra);
    gload(Bm, ldb, tn * SG_TN, N, 0, rb);
    tile_prologue(tm * SG_T, tn * SG_TN);
    while (id < n_ids) {
        const int m0 = tm * SG_T, n0 = tn * SG_TN;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < WJ; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
        // Software pipeline, one barrier per slab.  At the top of slab kt: fragment set 0 holds (kt, q=0), the staging registers
        // hold slab kt+1 (loads in flight).  One slab is ONE basic block (round 6): no zeroing select, no loop-carried branch --
        // HAS1 = slab kt+1 exists (its staged rows go to LDS, its first fragments are read behind the barrier), HAS2 = slab kt+2
        // exists (requested); the steady state (both) runs in the loop, the last two slabs are peeled -- and inside it the LDS and
        // memory operations are spread between the MFMAs (sched_group_barrier): one operation behind each MFMA instead of a burst
        // behind sixteen of them (ablation and A/B: profiles/r6_simgemm_ablation.txt; +3 % over the burst form).
        auto slab_body = [&](const int kt, auto has1, auto has2) {
            constexpr bool HAS1 = decltype(has1)::value, HAS2 = decltype(has2)::value;
            const int cur = kt & 1;
            frags(cur, 1, af1, bf1);
            mfma16(af0, bf0);
            if constexpr (HAS1) {
                sstore(As[cur ^ 1], ra, (kt + 1) * SG_K);
                sstore(Bs[cur ^ 1], rb, (kt + 1) * SG_K);
                if constexpr (HAS2) {
                    gload(A, lda, m0, M, (kt + 2) * SG_K, ra);
                    gload(Bm, ldb, n0, N, (kt + 2) * SG_K, rb);
                }
            }
            // 2 + WJ fragment reads, 8 WJ MFMAs, then per staged float4 one LDS store and (HAS2) one global load
#pragma unroll
            for (int i = 0; i < 2 + WJ; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 8 * WJ - (2 + WJ) - (HAS1 ? 2 + SG_LB : 0) - (HAS2 ? 2 + SG_LB : 0), 0);
            if constexpr (HAS1) {
#pragma unroll
                for (int i = 0; i < 2 + SG_LB; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                }
            }
            if constexpr (HAS2) {
#pragma unroll
                for (int i = 0; i < 2 + SG_LB; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                }
            }
            __syncthreads();
            if constexpr (HAS1) frags(cur ^ 1, 0, af0, bf0);
            mfma16(af1, bf1);
            if constexpr (HAS1) {
#pragma unroll
                for (int i = 0; i < 2 + WJ; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                }
            }
        };
        {
            int kt = 0;
            for (; kt + 2 < nk; ++kt) slab_body(kt, std::true_type{}, std::true_type{});
            if (kt + 1 < nk) {
                slab_body(kt, std::true_type{}, std::false_type{});
                ++kt;
            }
            slab_body(kt, std::false_type{}, std::false_type{});
        }
        // the next tile's first slab is requested BEFORE this tile's epilogue runs (the store epilogue: 64 KB of results at WJ = 2,
        // 128 KB at WJ = 4): the stores and the loads overlap, and no wave reads LDS any more (the last fragment reads precede the
        // last barrier)
        int ntm = 0, ntn = 0;
        const int nid = next_tile(id + gridDim.x, ntm, ntn);
        if (nid < n_ids) {
            gload(A, lda, ntm * SG_T, M, 0, ra);
            gload(Bm, ldb, ntn * SG_TN, N, 0, rb);
        }
        const bool full = m0 + SG_T <= M && n0 + SG_TN <= N;      // block-uniform: interior tiles store without bounds tests
        const SgPos pos{m0, n0, M, N, wm, wn, lane, r, h, full};
        if constexpr (EPI == SG_CSLS_COUNT) {
            sg_epi_count<WJ>(acc, pos, ext);
        } else if constexpr (EPI == SG_LSE) {
            sg_epi_lse(acc, pos, ext);
        } else if constexpr (EPI == SG_STATS) {
            sg_epi_stats(acc, pos, ext);
        } else if constexpr (LISTS) {
            sg_epi_lists<EPI, WJ>(acc, pos, ext, fl_m[wave], fl_n[wave], fl_v[wave]);
        } else if (full) {
            sg_epi_store_interior<WJ>(acc, pos, C, ldc);
            if (nid < n_ids) tile_prologue(ntm * SG_T, ntn * SG_TN);      // its own instance: see tile_prologue
            id = nid;
            tm = ntm;
            tn = ntn;
            continue;
        } else {
            sg_epi_store_ragged<WJ>(acc, pos, C, ldc);
        }
        id = nid;
        tm = ntm;
        tn = ntn;
        if (id < n_ids) tile_prologue(tm * SG_T, tn * SG_TN);     // (no wave reads LDS any more: see above)
    }
}

// ------------------------------------------------------------------------------------------------
// row top-k: one block per row.  Order: value descending, ties -> lower index first.
//   pass A  histogram of the 12 leading bits of an order-preserving key -> the bin b* that holds the k-th largest value
//   pass B  every entry of bins >= b* (a few dozen for similarity rows) is collected in LDS
//   select  each candidate counts the candidates that beat it: that count is its output slot
// Two streaming passes over the row instead of k; rows whose candidate set exceeds the LDS list (e.g. constant rows)
// take k rounds of (value, index) arg-max over the row in place.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void row_topk_kernel(const float* __restrict__ S, int64_t lds, int N, int k,
                                                          float* __restrict__ val, int32_t* __restrict__ idx) {
    __shared__ int hist[TK_BINS];
    __shared__ unsigned ckey[TK_CAP];
    __shared__ int cidx[TK_CAP];
    __shared__ int chunk_sum[kBlock];
    __shared__ int sh_bin, sh_above, sh_cnt;
    __shared__ TkExchange xch;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = S + (int64_t)b * lds;
    const bool vec = (((uintptr_t)row) & 15) == 0;
    for (int i = tid; i < TK_BINS; i += kBlock) hist[i] = 0;
    if (tid == 0) sh_cnt = 0;
    __syncthreads();
    // ---- pass A
    const int N4 = vec ? (N >> 2) : 0;
    for (int q = tid; q < N4; q += kBlock) {
        const float4 v = ld4(row + 4 * q);
        atomicAdd(&hist[tk_key(v.x) >> 20], 1);
        atomicAdd(&hist[tk_key(v.y) >> 20], 1);
        atomicAdd(&hist[tk_key(v.z) >> 20], 1);
        atomicAdd(&hist[tk_key(v.w) >> 20], 1);
    }
    for (int n = 4 * N4 + tid; n < N; n += kBlock) atomicAdd(&hist[tk_key(row[n]) >> 20], 1);
    __syncthreads();
    // ---- b*: chunk c = bins [BINS - 16(c+1), BINS - 16c), scanned from the top
    {
        int s16 = 0;
        const int hi = TK_BINS - 16 * tid;
#pragma unroll
        for (int j = 1; j <= 16; ++j) s16 += hist[hi - j];
        chunk_sum[tid] = s16;
        __syncthreads();
        if (tid < 64) {          // one wave: inclusive scan of the 256 chunk sums, 4 per lane
            int a0 = chunk_sum[4 * tid], a1 = chunk_sum[4 * tid + 1], a2 = chunk_sum[4 * tid + 2], a3 = chunk_sum[4 * tid + 3];
            const int tot = a0 + a1 + a2 + a3;
            int inc = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(inc, o, 64);
                if (tid >= o) inc += t;
            }
            int before = inc - tot;                       // entries in chunks above this lane's four
            const int sums[4] = {a0, a1, a2, a3};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (before < k && before + sums[j] >= k) {   // the k-th largest lies in chunk 4*tid + j
                    const int top = TK_BINS - 16 * (4 * tid + j);
                    int above = before;
                    for (int t = 1; t <= 16; ++t) {
                        const int h = hist[top - t];
                        if (above + h >= k) {
                            sh_bin = top - t;
                            sh_above = above;
                            break;
                        }
                        above += h;
                    }
                }
                before += sums[j];
            }
        }
        __syncthreads();
    }
    const int bstar = sh_bin;
    const int C = sh_above + hist[bstar];               // candidates = all entries of bins >= b*  (C >= k)
    if (C <= TK_CAP) {
        // ---- pass B
        for (int q = tid; q < N4; q += kBlock) {
            const float4 v = ld4(row + 4 * q);
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned key = tk_key(e[j]);
                if ((int)(key >> 20) >= bstar) {
                    const int slot = atomicAdd(&sh_cnt, 1);
                    ckey[slot] = key;
                    cidx[slot] = 4 * q + j;
                }
            }
        }
        for (int n = 4 * N4 + tid; n < N; n += kBlock) {
            const unsigned key = tk_key(row[n]);
            if ((int)(key >> 20) >= bstar) {
                const int slot = atomicAdd(&sh_cnt, 1);
                ckey[slot] = key;
                cidx[slot] = n;
            }
        }
        __syncthreads();
        // ---- select: slot = number of candidates that beat this one (keys are distinct as (key, index) pairs)
        for (int c = tid; c < C; c += kBlock) {
            const unsigned kc = ckey[c];
            const int ic = cidx[c];
            int better = 0;
            int o = 0;
            for (; o + 8 <= C; o += 8) {                     // eight independent LDS reads in flight per trip (a rolled loop
                unsigned k8[8];                                // waits out the LDS latency once per candidate: 80 cycles each)
                int i8[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    k8[u] = ckey[o + u];
                    i8[u] = cidx[o + u];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) better += tk_beats(k8[u], i8[u], kc, ic) ? 1 : 0;
            }
            for (; o < C; ++o) better += tk_beats(ckey[o], cidx[o], kc, ic) ? 1 : 0;
            if (better < k) {
                idx[(int64_t)b * k + better] = ic;
                if (val) val[(int64_t)b * k + better] = row[ic];
            }
        }
        return;
    }
    // ---- fallback: k rounds of arg-max over the stored row
    tk_argmax_rounds(
        xch, k,
        [&](auto f) {
            for (int n = tid; n < N; n += kBlock) f(n, row[n]);
        },
        [&](int r, float v, int n) {
            if (val) val[(int64_t)b * k + r] = v;
            idx[(int64_t)b * k + r] = n == INT32_MAX ? -1 : n;
        });
}

// ------------------------------------------------------------------------------------------------
// top-k of a row from its candidate list (fused similarity + top-k, jmac_sim_topk_f32): every element >= tau was listed, and
// at least k elements are (tau is the k-th largest of a column sample), so the list's k best ARE the row's k best; order and
// ties as row_topk_kernel (value descending, lower index first).
// A row whose list overflowed (more than cap elements reach tau: e.g. a constant row) recomputes its N scores with the
// SAME instruction sequence per element as sim_gemm_kernel -- v_mfma_f32_32x32x2_f32 over k in the same order, so the bits
// are the GEMM's -- once per pass of the two-pass selection (and per arg-max round if even that overflows).  Slow by design:
// it exists so that degenerate inputs still get the exact answer.
// ------------------------------------------------------------------------------------------------
// (sim_tile_32x32 and for_each_row_score, the recomputation itself: sim_rescore.h -- screen.hip rescores with them too)

// s(m, n) = 1 - dist(m, n) of ONE pair of rows (l1_seq_sum).  One lane per pair.
__device__ __forceinline__ float l1_row_sim(const float* __restrict__ arow, const float* __restrict__ brow, int d) {
    return 1.f - l1_seq_sum(0.f, arow, brow, d);
}
template <class F>
__device__ __forceinline__ void for_each_row_l1(const float* __restrict__ arow, const float* __restrict__ Bm, int64_t ldb, int N,
                                                int d, F f) {
    for (int n = threadIdx.x; n < N; n += kBlock) f(n, l1_row_sim(arow, Bm + (int64_t)n * ldb, d));
}

// CS: the lists hold CSLS-rescored values (jmac_sim_csls_topk_f32), so a recomputed score is rescored too before it is used
// (r1 / r2 are not read otherwise)
// VIABLE (jmac_sim_csls_topk_viable_f32): the lists hold viable columns only; the sample's k best may end in masked (-inf)
// entries and a recomputed row skips the columns whose word best[n] the row's own word tk_pack(c, row_id[b]) does not beat;
// what is missing of the k comes out as (idx -1, val -inf).  CS is then decided at run time (r1 != NULL).
// L1 (jmac_l1_csls_topk_*): the Manhattan form -- a recomputed score is s = 1 - dist (l1_row_sim), CS decided at run time
template <bool CS, bool VIABLE, bool L1 = false>
__device__ __forceinline__ void cand_select_body(const float* __restrict__ A, int64_t lda, const float* __restrict__ Bm,
                                                 int64_t ldb, int N, int d, int k, const int* __restrict__ cnt,
                                                 const float* __restrict__ cval, const int* __restrict__ cidx, int cap,
                                                 const float* __restrict__ sval, const int32_t* __restrict__ sidx,
                                                 float* __restrict__ val, int32_t* __restrict__ idx,
                                                 const float* __restrict__ r1, const float* __restrict__ r2,
                                                 const int32_t* __restrict__ row_id, const unsigned long long* __restrict__ best) {
    __shared__ TkShared tk;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int C = cnt[b];
    auto emit = [&](int c, unsigned long long e) {
        if constexpr (VIABLE) {
            const bool none = e == 0ull || tk_unpack_value(e) == -INFINITY;
            idx[(int64_t)b * k + c] = none ? -1 : tk_unpack_index(e);
            val[(int64_t)b * k + c] = none ? -INFINITY : tk_unpack_value(e);
        } else {
            idx[(int64_t)b * k + c] = tk_unpack_index(e);
            if (val) val[(int64_t)b * k + c] = tk_unpack_value(e);
        }
    };
    if (C + k <= cap) {                                        // the normal case (cap <= TK_CAP)
        // candidates: the row's list (columns past the sample) + the sample's own k best (the threshold came from them; a
        // sample element tied with tau but outside that list has a higher index than every listed tie: it cannot win)
        for (int c = tid; c < C; c += kBlock) tk.skey[c] = tk_pack(cval[(int64_t)b * cap + c], cidx[(int64_t)b * cap + c]);
        for (int c = tid; c < k; c += kBlock) tk.skey[C + c] = tk_pack(sval[(int64_t)b * k + c], sidx[(int64_t)b * k + c]);
        tk_sort_emit(tk.skey, C + k, k, emit);
        return;
    }
    // ---- overflow: the selection over recomputed scores
    const float* arow = A + (int64_t)b * lda;
    float r1b = 0.f;
    if constexpr (CS) r1b = r1[b];
    if constexpr (VIABLE || L1) r1b = r1 != nullptr ? r1[b] : 0.f;
    auto rescored = [&](int n, float v) -> float {
        if constexpr (CS) return csls_value(v, r1b, r2[n]);
        else if constexpr (VIABLE || L1) return r1 != nullptr ? csls_value(v, r1b, r2[n]) : v;
        else return v;
    };
    auto for_each_score = [&](auto f) {
        if constexpr (L1) for_each_row_l1(arow, Bm, ldb, N, d, f);
        else for_each_row_score(arow, Bm, ldb, N, d, f);
    };
    if constexpr (VIABLE) {
        const int rid = row_id[b];
        tk_select_recomputed(
            tk, k,
            [&](auto f) {
                for_each_score([&](int n, float v) {
                    const float c = rescored(n, v);
                    if (tk_pack(c, rid) > best[n]) f(n, c);
                });
            },
            emit);
    } else {
        tk_select_recomputed(
            tk, k, [&](auto f) { for_each_score([&](int n, float v) { f(n, rescored(n, v)); }); }, emit);
    }
}

template <bool CS, bool L1 = false>
__global__ __launch_bounds__(kBlock) void cand_select_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ Bm,
                                                             int64_t ldb, int N, int d, int k, const int* __restrict__ cnt,
                                                             const float* __restrict__ cval, const int* __restrict__ cidx, int cap,
                                                             const float* __restrict__ sval, const int32_t* __restrict__ sidx,
                                                             float* __restrict__ val, int32_t* __restrict__ idx,
                                                             const float* __restrict__ r1, const float* __restrict__ r2) {
    cand_select_body<CS, false, L1>(A, lda, Bm, ldb, N, d, k, cnt, cval, cidx, cap, sval, sidx, val, idx, r1, r2, nullptr, nullptr);
}
template <bool L1 = false>
__global__ __launch_bounds__(kBlock) void cand_select_viable_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ Bm,
                                                                    int64_t ldb, int N, int d, int k, const int* __restrict__ cnt,
                                                                    const float* __restrict__ cval, const int* __restrict__ cidx, int cap,
                                                                    const float* __restrict__ sval, const int32_t* __restrict__ sidx,
                                                                    float* __restrict__ val, int32_t* __restrict__ idx,
                                                                    const float* __restrict__ r1, const float* __restrict__ r2,
                                                                    const int32_t* __restrict__ row_id,
                                                                    const unsigned long long* __restrict__ best) {
    cand_select_body<false, true, L1>(A, lda, Bm, ldb, N, d, k, cnt, cval, cidx, cap, sval, sidx, val, idx, r1, r2, row_id, best);
}

// c(i, gold[i]) of every row with the bits the tile kernel produces for that element, and rank[i] = 1 (csls_gold_body, sim_rescore.h:
// screen.hip's ranks take their gold values from the same body)
__global__ __launch_bounds__(kBlock) void csls_gold_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ Bm,
                                                           int64_t ldb, int M, int d, const float* __restrict__ r1,
                                                           const float* __restrict__ r2, const int32_t* __restrict__ gold,
                                                           float* __restrict__ gval, int32_t* __restrict__ rank) {
    csls_gold_body(A, lda, Bm, ldb, M, d, r1, r2, gold, gval, rank);
}

// S[i][j] = csls_value(S[i][j], r1[i], r2[j]) in place: the column sample (or a narrow matrix) staged in the workspace
__global__ __launch_bounds__(kBlock) void csls_inplace_kernel(float* __restrict__ S, int64_t lds, int n2, const float* __restrict__ r1,
                                                              const float* __restrict__ r2) {
    float* row = S + (int64_t)blockIdx.x * lds;
    const float a = r1[blockIdx.x];
    for (int n = threadIdx.x; n < n2; n += kBlock) row[n] = csls_value(row[n], a, r2[n]);
}
// the same pass for the viable top-k: rescored (r1 != NULL), and an entry whose word does not beat its reviewer's becomes -inf
__global__ __launch_bounds__(kBlock) void viable_inplace_kernel(float* __restrict__ S, int64_t lds, int n2, const float* __restrict__ r1,
                                                                const float* __restrict__ r2, const int32_t* __restrict__ row_id,
                                                                const unsigned long long* __restrict__ best) {
    float* row = S + (int64_t)blockIdx.x * lds;
    const float a = r1 != nullptr ? r1[blockIdx.x] : 0.f;
    const int rid = row_id[blockIdx.x];
    for (int n = threadIdx.x; n < n2; n += kBlock) {
        const float c = r1 != nullptr ? csls_value(row[n], a, r2[n]) : row[n];
        row[n] = tk_pack(c, rid) > best[n] ? c : -INFINITY;
    }
}
// row_topk_kernel's output over such a masked row: a masked entry among the k (fewer than k viable columns) -> (-inf, -1)
__global__ __launch_bounds__(kBlock) void viable_topk_finish_kernel(const float* __restrict__ val, int32_t* __restrict__ idx, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n && val[i] == -INFINITY) idx[i] = -1;
}

// ---- Manhattan alignment (jmac_l1_csls_*): csls_gold_kernel / csls_inplace_kernel / viable_inplace_kernel for s = 1 - dist ----
// gval[m] = c(m, gold[m]) from l1_row_sim (the count's "equal, lower index first" is exact at the gold column itself);
// rank[m] = 1.  One lane per row.
__global__ __launch_bounds__(kBlock) void l1_csls_gold_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ Bm,
                                                              int64_t ldb, int M, int d, const float* __restrict__ r1,
                                                              const float* __restrict__ r2, const int32_t* __restrict__ gold,
                                                              float* __restrict__ gval, int32_t* __restrict__ rank) {
    const int m = blockIdx.x * kBlock + threadIdx.x;
    if (m >= M) return;
    const int g = gold[m];
    const float s = l1_row_sim(A + (int64_t)m * lda, Bm + (int64_t)g * ldb, d);
    gval[m] = r1 != nullptr ? csls_value(s, r1[m], r2[g]) : s;
    rank[m] = 1;
}
// a stored slab of -dist (the tile kernel's LR_STORE) -> c in place: s = 1 - dist, rescored when r1 != NULL, and with best != NULL
// an entry whose word does not beat its reviewer's becomes -inf
__global__ __launch_bounds__(kBlock) void l1_csls_inplace_kernel(float* __restrict__ S, int64_t lds, int n2, const float* __restrict__ r1,
                                                                 const float* __restrict__ r2, const int32_t* __restrict__ row_id,
                                                                 const unsigned long long* __restrict__ best) {
    float* row = S + (int64_t)blockIdx.x * lds;
    const float a = r1 != nullptr ? r1[blockIdx.x] : 0.f;
    const int rid = best != nullptr ? row_id[blockIdx.x] : 0;
    for (int n = threadIdx.x; n < n2; n += kBlock) {
        const float s = 1.f + row[n];                          // == 1 - dist, bit for bit
        const float c = r1 != nullptr ? csls_value(s, a, r2[n]) : s;
        row[n] = (best == nullptr || tk_pack(c, rid) > best[n]) ? c : -INFINITY;
    }
}

// ------------------------------------------------------------------------------------------------
// link-prediction top-k (jmac_linkpred_topk_*): the k nearest unlisted candidates of every query.  Scores travel NEGATED
// (-dist), so "k smallest distances, lower index first" is the k largest with row_topk_kernel's tie rule.
// ------------------------------------------------------------------------------------------------
// one block per query: its listed tails among the stored columns [0, ncols) -> -inf (never selected before an unlisted one)
__global__ __launch_bounds__(kBlock) void link_mask_kernel(float* __restrict__ S, int64_t ldS, int ncols, const int2* __restrict__ rng,
                                                           const int32_t* __restrict__ tail_idx) {
    const int b = blockIdx.x;
    const int2 r = rng[b];
    for (int f = r.x + threadIdx.x; f < r.y; f += kBlock) {
        const int n = tail_idx[f];
        if (n >= 0 && n < ncols) S[(int64_t)b * ldS + n] = -INFINITY;
    }
}

// row_topk_kernel's (-dist, index) -> (dist, index); a masked entry (fewer than k unlisted candidates) -> (+inf, -1)
__global__ __launch_bounds__(kBlock) void link_topk_finish_kernel(float* __restrict__ val, int32_t* __restrict__ idx, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float v = val[i];
    if (v == -INFINITY) {
        val[i] = INFINITY;
        idx[i] = -1;
    } else {
        val[i] = v == 0.f ? 0.f : -v;
    }
}

// The select kernels (one block per query), single-KG and ensemble: the k best of (candidate list + the sample's k best), listed
// candidates dropped (the sample's were masked before its selection).  Every unlisted n with dist <= tau_b is in that set and at
// least k of them exist (tau_b is the k-th smallest unlisted SAMPLE distance), so its k best are the row's; a sample entry tied
// with tau_b outside the sample's k best has k entries before it already.
// A row whose list overflowed (a constant table, a huge tie, or fewer than k unlisted sample entries: tau_b = +inf) recomputes
// its N distances (l1_seq_sum), one lane per candidate, once per pass of the two-pass selection and once per arg-max round if the
// top bin overflows too.  Slow by design, exact.  The kernels differ in that recomputation only.
struct LinkEmit {                                              // rank c of row b: (-dist, n) -> (dist, n)
    float* ov;
    int32_t* oi;
    __device__ __forceinline__ void operator()(int c, unsigned long long e) const {
        if (e == 0ull) {                                       // padding: fewer than k unlisted candidates
            oi[c] = -1;
            ov[c] = INFINITY;
            return;
        }
        oi[c] = tk_unpack_index(e);
        const float v = tk_unpack_value(e);
        ov[c] = v == 0.f ? 0.f : -v;
    }
};
// the normal case (cap <= TK_CAP); false: the list overflowed and nothing was emitted
__device__ __forceinline__ bool link_select_listed(const LinkRankArgs& a, int b, int2 r, int k, const float* __restrict__ sval,
                                                   const int32_t* __restrict__ sidx, TkShared& tk, const LinkEmit& emit) {
    const int tid = threadIdx.x;
    const int C = a.cnt[b];
    if (C + k > a.cap) return false;
    for (int c = tid; c < C; c += kBlock) {
        const int n = a.cidx[(int64_t)b * a.cap + c];
        tk.skey[c] = tail_listed(a.filt_idx, r.x, r.y, n) ? 0ull : tk_pack(a.cval[(int64_t)b * a.cap + c], n);
    }
    for (int c = tid; c < k; c += kBlock) {
        const float v = sval[(int64_t)b * k + c];
        tk.skey[C + c] = v == -INFINITY ? 0ull : tk_pack(v, sidx[(int64_t)b * k + c]);
    }
    tk_sort_emit(tk.skey, C + k, k, emit);
    return true;
}

template <typename TT>
__global__ __launch_bounds__(kBlock) void link_select_kernel(LinkRankArgs a, int k, const float* __restrict__ sval,
                                                             const int32_t* __restrict__ sidx, float* __restrict__ val,
                                                             int32_t* __restrict__ idx) {
    extern __shared__ float ls_sh[];                           // [nl * dq] the query's rows (overflow path)
    __shared__ TkShared tk;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int2 r = a.rng[b];                                   // the query's listed tails
    const LinkEmit emit{val + (int64_t)b * k, idx + (int64_t)b * k};
    if (link_select_listed(a, b, r, k, sval, sidx, tk, emit)) return;
    const int d = a.d, dq = a.dq, W = a.nl * dq;
    for (int i = tid; i < W; i += kBlock) {
        const int l = i / dq, q = i - l * dq;
        ls_sh[i] = ld1(static_cast<const TT*>(a.er) + ((int64_t)l * a.B + b) * dq + q);
    }
    auto for_each_unlisted = [&](auto f) {                      // f(n, -dist[b, n]) for every n in [0, N) the index does not list
        for (int n = tid; n < a.N; n += kBlock) {
            if (tail_listed(a.filt_idx, r.x, r.y, n)) continue;
            float acc = 0.f;
            for (int l = 0; l < a.nl; ++l)
                acc = l1_seq_sum(acc, ls_sh + l * dq, static_cast<const TT*>(a.tab[l]) + (int64_t)n * a.ld_tab[l], d);
            f(n, -acc);
        }
    };
    tk_select_recomputed(tk, k, for_each_unlisted, emit);       // (its first barrier completes ls_sh)
}

// ------------------------------------------------------------------------------------------------
// column top-k values (CSLS column term, similarity.py:58-78 on the transposed matrix) without transposing:
// one lane per column (a wave reads 256 contiguous bytes of a row), rows split over the 4 waves of a block and over
// gridDim.y row ranges; every (block, wave) keeps its column's k largest values in registers (branch-free bubble
// insertion, skipped by the whole wave when no lane's value beats its current k-th) and writes them as a candidate
// list; a second kernel merges the lists of a column.  Output [n2, k] sorted descending.
// ------------------------------------------------------------------------------------------------
constexpr int CT_KMAX = 16;

// inserts v into the descending list top[0..k) and returns its new k-th (smallest kept) value; register-only:
// the list is never indexed with a run-time subscript
__device__ __forceinline__ float ct_insert(float (&top)[CT_KMAX], int k, float v) {
    float x = v, kth = -INFINITY;
#pragma unroll
    for (int j = 0; j < CT_KMAX; ++j)
        if (j < k) {
            const float hi = fmaxf(top[j], x);
            x = fminf(top[j], x);
            top[j] = hi;
            kth = j == k - 1 ? hi : kth;
        }
    return kth;
}

__global__ __launch_bounds__(kBlock) void col_topk_partial_kernel(const float* __restrict__ S, int64_t lds, int n1, int n2, int k,
                                                                  float* __restrict__ cand) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    const int rows_per = (n1 + gridDim.y - 1) / gridDim.y;
    const int r0 = blockIdx.y * rows_per, r1 = min(n1, r0 + rows_per);
    float top[CT_KMAX];
#pragma unroll
    for (int j = 0; j < CT_KMAX; ++j) top[j] = -INFINITY;
    const int cc = min(col, n2 - 1);
    float kth = -INFINITY;
    for (int r = r0 + wave; r < r1; r += kBlock / 64) {
        const float v = col < n2 ? S[(int64_t)r * lds + cc] : -INFINITY;
        if (__any(v > kth)) kth = ct_insert(top, k, v);
    }
    const int part = blockIdx.y * (kBlock / 64) + wave;
    if (col < n2) {
        float* o = cand + ((int64_t)part * n2 + col) * k;
#pragma unroll
        for (int j = 0; j < CT_KMAX; ++j)
            if (j < k) o[j] = top[j];
    }
}

__global__ __launch_bounds__(kBlock) void col_topk_merge_kernel(const float* __restrict__ cand, int parts, int n2, int k,
                                                                float* __restrict__ out) {
    const int col = blockIdx.x * kBlock + threadIdx.x;
    if (col >= n2) return;
    float top[CT_KMAX];
#pragma unroll
    for (int j = 0; j < CT_KMAX; ++j) top[j] = -INFINITY;
    float kth = -INFINITY;
    for (int p = 0; p < parts; ++p) {
        const float* c = cand + ((int64_t)p * n2 + col) * k;
        for (int j = 0; j < k; ++j) {
            const float v = c[j];
            if (!(v > kth)) break;                        // lists are sorted: nothing further of this one can enter
            kth = ct_insert(top, k, v);
        }
    }
#pragma unroll
    for (int j = 0; j < CT_KMAX; ++j)
        if (j < k) out[(int64_t)col * k + j] = top[j];
}

// ------------------------------------------------------------------------------------------------
// softmax entropy of the rows of scale*S;  masked row softmax
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_max(float v, float* sh) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sh[0];
    for (int w = 1; w < kBlock / 64; ++w) r = fmaxf(r, sh[w]);
    __syncthreads();
    return r;
}
__device__ __forceinline__ float block_sum(float v, float* sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sh[0];
    for (int w = 1; w < kBlock / 64; ++w) r += sh[w];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kBlock) void row_entropy_kernel(const float* __restrict__ S, int64_t lds, int N, float scale,
                                                             float* __restrict__ ent) {
    __shared__ float sh[kBlock / 64];
    const float* row = S + (int64_t)blockIdx.x * lds;
    float m = -INFINITY;
    for (int n = threadIdx.x; n < N; n += kBlock) m = fmaxf(m, row[n] * scale);
    m = block_max(m, sh);
    float z = 0.f, y = 0.f;
    for (int n = threadIdx.x; n < N; n += kBlock) {
        const float x = row[n] * scale - m;
        const float e = expf(x);
        z += e;
        y = fmaf(e, x, y);
    }
    z = block_sum(z, sh);
    y = block_sum(y, sh);
    if (threadIdx.x == 0) ent[blockIdx.x] = logf(z) - y / z;
}

// softmax over a ROW of the masked, scaled matrix; out (the probabilities) and ent (the row's softmax entropy) are optional
__global__ __launch_bounds__(kBlock) void masked_row_softmax_kernel(const float* __restrict__ S, int64_t lds, int N,
                                                                    const uint8_t* __restrict__ row_mask,
                                                                    const uint8_t* __restrict__ col_mask, float fill, float scale,
                                                                    float* __restrict__ out, int64_t ldo, float* __restrict__ ent) {
    __shared__ float sh[kBlock / 64];
    const int i = blockIdx.x;
    const float* row = S + (int64_t)i * lds;
    const bool rk = row_mask ? row_mask[i] != 0 : true;
    auto val = [&](int n) -> float {
        const bool keep = rk && (col_mask ? col_mask[n] != 0 : true);
        return (keep ? row[n] : fill) * scale;
    };
    float m = -INFINITY;
    for (int n = threadIdx.x; n < N; n += kBlock) m = fmaxf(m, val(n));
    m = block_max(m, sh);
    float z = 0.f, y = 0.f;
    for (int n = threadIdx.x; n < N; n += kBlock) {
        const float x = val(n) - m;
        const float e = expf(x);
        z += e;
        y = fmaf(e, x, y);
    }
    z = block_sum(z, sh);
    if (ent) {
        y = block_sum(y, sh);
        if (threadIdx.x == 0) ent[i] = logf(z) - y / z;
    }
    if (out) {
        float* orow = out + (int64_t)i * ldo;
        const float iz = 1.f / z;
        for (int n = threadIdx.x; n < N; n += kBlock) orow[n] = expf(val(n) - m) * iz;
    }
}

// ------------------------------------------------------------------------------------------------
// softmax over the COLUMNS of the same masked, scaled matrix, from the one row-major S (no second, transposed GEMM):
//   stats   one lane per column (a wave reads 256 contiguous bytes of a row), rows split over the 4 waves of a block and
//           over gridDim.y row ranges; online (max, sum e^x, sum e^x x) per lane, one partial triple per (part, column)
//   merge   combines the partials of a column in part order -> (max, 1/sum) per column and the column's entropy
//   apply   64x64 tile through LDS: p = exp(x - max_j) / sum_j, written TRANSPOSED ([n2, n1], coalesced both ways)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cs_push(float& m, float& z, float& y, float x) {
    // running (m, z = sum e^(x-m), y = sum e^(x-m) (x-m)) with a new element x
    const float mn = fmaxf(m, x);
    const float f = expf(m - mn);                  // m = -inf: f = 0 (z = y = 0 there)
    const float dm = m - mn;                       // <= 0; -inf - finite = -inf only while z = y = 0
    y = f * (y + (z > 0.f ? dm * z : 0.f));
    z = f * z;
    const float xe = x - mn;
    const float e = expf(xe);
    z += e;
    y = fmaf(e, xe, y);
    m = mn;
}

__global__ __launch_bounds__(kBlock) void col_softmax_stats_kernel(const float* __restrict__ S, int64_t lds, int n1, int n2,
                                                                   const uint8_t* __restrict__ row_mask,
                                                                   const uint8_t* __restrict__ col_mask, float fill, float scale,
                                                                   float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    const int rows_per = (n1 + gridDim.y - 1) / gridDim.y;
    const int r0 = blockIdx.y * rows_per, r1 = min(n1, r0 + rows_per);
    const int cc = min(col, n2 - 1);
    const bool ck = col_mask ? col_mask[cc] != 0 : true;
    float m = -INFINITY, z = 0.f, y = 0.f;
    for (int r = r0 + wave; r < r1; r += kBlock / 64) {
        const bool keep = ck && (row_mask ? row_mask[r] != 0 : true);
        const float v = S[(int64_t)r * lds + cc];
        cs_push(m, z, y, (keep ? v : fill) * scale);
    }
    const int p = blockIdx.y * (kBlock / 64) + wave;
    if (col < n2) {
        float* o = part + ((int64_t)p * n2 + col) * 3;
        o[0] = m;
        o[1] = z;
        o[2] = y;
    }
}

__global__ __launch_bounds__(kBlock) void col_softmax_merge_kernel(const float* __restrict__ part, int parts, int n2,
                                                                   float* __restrict__ cmax, float* __restrict__ cinv,
                                                                   float* __restrict__ ent) {
    const int col = blockIdx.x * kBlock + threadIdx.x;
    if (col >= n2) return;
    float m = -INFINITY, z = 0.f, y = 0.f;
    for (int p = 0; p < parts; ++p) {
        const float* q = part + ((int64_t)p * n2 + col) * 3;
        const float pm = q[0], pz = q[1], py = q[2];
        if (!(pz > 0.f)) continue;                                  // a part without rows
        const float mn = fmaxf(m, pm);
        const float fa = expf(m - mn), fb = expf(pm - mn);
        const float da = m - mn, db = pm - mn;
        const float ya = z > 0.f ? fa * (y + da * z) : 0.f;
        const float yb = fb * (py + db * pz);
        y = ya + yb;
        z = fa * z + fb * pz;
        m = mn;
    }
    cmax[col] = m;
    cinv[col] = 1.f / z;
    if (ent) ent[col] = logf(z) - y / z;
}

__global__ __launch_bounds__(kBlock) void col_softmax_apply_kernel(const float* __restrict__ S, int64_t lds, int n1, int n2,
                                                                   const uint8_t* __restrict__ row_mask,
                                                                   const uint8_t* __restrict__ col_mask, float fill, float scale,
                                                                   const float* __restrict__ cmax, const float* __restrict__ cinv,
                                                                   float* __restrict__ out_t, int64_t ldo) {
    __shared__ float tile[64][65];
    const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int j = j0 + tx;
    const bool jin = j < n2;
    const int jc = min(j, n2 - 1);
    const bool ck = col_mask ? col_mask[jc] != 0 : true;
    const float mj = cmax[jc], zj = cinv[jc];
    for (int r = ty; r < 64; r += kBlock / 64) {
        const int i = i0 + r;
        float p = 0.f;
        if (i < n1 && jin) {
            const bool keep = ck && (row_mask ? row_mask[i] != 0 : true);
            const float x = (keep ? S[(int64_t)i * lds + j] : fill) * scale;
            p = expf(x - mj) * zj;
        }
        tile[r][tx] = p;
    }
    __syncthreads();
    const int i = i0 + tx;
    for (int c = ty; c < 64; c += kBlock / 64) {
        const int jj = j0 + c;
        if (jj < n2 && i < n1) out_t[(int64_t)jj * ldo + i] = tile[tx][c];
    }
}

// out[i][j] = 2*S[i][j] - r1[i] - r2[j]   (CSLS, modules/finding/similarity.py:58-78)
__global__ __launch_bounds__(kBlock) void csls_apply_kernel(const float* __restrict__ S, int64_t lds, int64_t n1, int64_t n2,
                                                            const float* __restrict__ r1, const float* __restrict__ r2,
                                                            float* __restrict__ out, int64_t ldo) {
    const int64_t total = n1 * n2;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / n2, c = i % n2;
        out[r * ldo + c] = csls_value(S[r * lds + c], r1[r], r2[c]);
    }
}

// rank of column gold[i] in row i of the CSLS-rescored matrix 2 S - r1[i] - r2[j], descending, ties -> lower index first:
// csls_apply + filtered_rank(descending) without writing or re-reading the rescored matrix.
__global__ __launch_bounds__(kBlock) void csls_rank_kernel(const float* __restrict__ S, int64_t lds, int n2,
                                                           const float* __restrict__ r1, const float* __restrict__ r2,
                                                           const int32_t* __restrict__ gold, int32_t* __restrict__ rank) {
    __shared__ int red[kBlock / 64];
    const int i = blockIdx.x;
    const float* row = S + (int64_t)i * lds;
    const float a = r1[i];
    const int g = gold[i];
    const float gs = csls_value(row[g], a, r2[g]);
    int cnt = 0;
    for (int n = threadIdx.x; n < n2; n += kBlock) {
        const float v = csls_value(row[n], a, r2[n]);
        cnt += (v > gs || (v == gs && n < g)) ? 1 : 0;
    }
    cnt = wave_sum_i(cnt);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kBlock / 64; ++w) t += red[w];
        rank[i] = t + 1;
    }
}

// One shape's launch geometry with WJ column sub-tiles per wave: tiles, the XCD-aware id space and the blocks resident at once.
template <int WJ>
struct SimGeom {
    int tiles_m, tiles_n, super_order;
    int64_t n_ids, tiles;
    SimGeom(int64_t M, int64_t N) {
        tiles_m = (int)((M + SG_T - 1) / SG_T);
        tiles_n = (int)((N + SgTile<WJ>::TN - 1) / SgTile<WJ>::TN);
        const int64_t sup = (int64_t)((tiles_m + SG_SUPER - 1) / SG_SUPER) * ((tiles_n + SgTile<WJ>::SUPER_N - 1) / SgTile<WJ>::SUPER_N);
        super_order = sup >= 64 ? 1 : 0;                                  // >= 8 super-tiles per XCD: the tail imbalance is small
        tiles = (int64_t)tiles_m * tiles_n;
        n_ids = super_order ? (sup + 7) / 8 * 8 * SG_SUPER * SgTile<WJ>::SUPER_N : tiles;
    }
};

// persistent grids: as many blocks as are resident at once (occupancy query: 3 per CU for the 128 x 128 tile -- 64 accumulation
// VGPRs, 33 KB of LDS -- and 2 for 128 x 256), rounded down to a multiple of 8 so that a block's tile ids stay on its XCD
template <int EPI, int WJ>
int sim_resident(int dev) {
    static int resident_of[64] = {0};                                     // per device: CU counts may differ between devices
    int& resident = resident_of[dev >= 0 && dev < 64 ? dev : 0];
    if (resident == 0 || dev >= 64) {
        int cus = 256, occ = SgTile<WJ>::OCC;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, reinterpret_cast<const void*>(sim_gemm_kernel<EPI, WJ>), kBlock, 0) != hipSuccess || occ < 1)
            occ = SgTile<WJ>::OCC;
        resident = (cus * occ) / 8 * 8;
        if (resident < 8) resident = 8;
    }
    return resident;
}

// one launch of the product with the epilogue EPI and tile width WJ; ext = that epilogue's arguments
template <int EPI, int WJ>
int launch_sim_tile(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t M, int64_t N, int64_t d, float* C, int64_t ldc,
                    const typename SgEpiTraits<EPI>::Ext& ext, hipStream_t st, int dev) {
    const SimGeom<WJ> g(M, N);
    if (g.n_ids >= INT32_MAX) return JMAC_ERANGE;
    const int resident = sim_resident<EPI, WJ>(dev);
    const unsigned grid = (unsigned)(g.n_ids < resident ? g.n_ids : resident);
    hipLaunchKernelGGL((sim_gemm_kernel<EPI, WJ>), dim3(grid), dim3(kBlock), 0, st, A, lda, B, ldb, (int)M, (int)N, (int)d, C, ldc,
                       g.tiles_m, g.tiles_n, g.super_order, (int)g.n_ids, ext);
    return (int)hipGetLastError();
}

// THE launcher of the similarity product, whatever the epilogue (C, ldc: SG_STORE only).  An epilogue that has no wide tile
// (SgEpiTraits<EPI>::WIDE) runs on the 128 x 128 one.  The others choose.  Which tile?  Both give the same bits.  A round of resident
// blocks is (resident blocks) x (tile area) of matrix-pipe work, and the wide tile does a given amount of it ~3.5 % faster (fewer
// barriers and operand bytes per flop) -- but its rounds are coarser.  Take it when its quantised makespan, rounds x resident x
// area, is no larger than the narrow tile's (measured, config-5 shapes: 12 000^2 and 3 000 x 30 000 tie on that count and gain
// 3.4 / 3.5 %; 10 500^2 needs 7 168 against 6 912 units and loses 4 %).
template <int EPI>
int launch_sim(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t M, int64_t N, int64_t d, float* C, int64_t ldc,
               const typename SgEpiTraits<EPI>::Ext& ext, hipStream_t st) {
    if (M == 0 || N == 0) return 0;
    if (d % 4) return JMAC_EDIM;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if constexpr (SgEpiTraits<EPI>::WIDE) {
        const SimGeom<2> g2(M, N);
        const SimGeom<4> g4(M, N);
        const int64_t r2 = sim_resident<EPI, 2>(dev), r4 = sim_resident<EPI, 4>(dev);
        const int64_t cost2 = (g2.tiles + r2 - 1) / r2 * r2, cost4 = (g4.tiles + r4 - 1) / r4 * r4 * 2;
        if (g4.tiles >= r4 && cost4 <= cost2) return launch_sim_tile<EPI, 4>(A, lda, B, ldb, M, N, d, C, ldc, ext, st, dev);
    }
    return launch_sim_tile<EPI, 2>(A, lda, B, ldb, M, N, d, C, ldc, ext, st, dev);
}

// 64 rows (blocks [0, row_blocks)) or 64 columns (the blocks behind them) per block.  Wave g combines the g-th quarter of a
// line's partials in ascending part order with the arithmetic of col_softmax_merge_kernel (loads four parts ahead: one thread
// walking all of a line's parts alone is a chain of dependent memory latencies), wave 0 then combines the four quarters in
// order.  The maximum moves on strict > only, so ties keep the lowest index.  Every output is optional.
constexpr int SM_G = kBlock / 64;
struct SsState {
    float m = -INFINITY, z = 0.f, y = 0.f, best = -INFINITY;      // m: max logit, best: max similarity
    int arg = 0;
    __device__ __forceinline__ void push(float pm, float pz, float py, float pbest, int parg) {
        if (!(pz > 0.f)) return;                                   // nothing behind this partial
        if (pbest > best) {
            best = pbest;
            arg = parg;
        }
        const float mn = fmaxf(m, pm);
        const float fa = expf(m - mn), fb = expf(pm - mn);
        const float da = m - mn, db = pm - mn;
        const float ya = z > 0.f ? fa * (y + da * z) : 0.f;
        const float yb = fb * (py + db * pz);
        y = ya + yb;
        z = fa * z + fb * pz;
        m = mn;
    }
};
__global__ __launch_bounds__(kBlock) void sim_stats_merge_kernel(const float4* __restrict__ rpart, const float* __restrict__ cpart,
                                                                 const float2* __restrict__ cbest, int n1, int n2, float scale,
                                                                 int row_blocks, float* __restrict__ row_max, int32_t* __restrict__ row_arg,
                                                                 float* __restrict__ row_sum, float* __restrict__ row_ent,
                                                                 float* __restrict__ col_max, int32_t* __restrict__ col_arg,
                                                                 float* __restrict__ col_sum, float* __restrict__ col_ent) {
    __shared__ float sh[SM_G][4][64];
    __shared__ int sha[SM_G][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const bool rows = (int)blockIdx.x < row_blocks;
    const int e = ((int)blockIdx.x - (rows ? 0 : row_blocks)) * 64 + lane;
    const int n = rows ? n1 : n2, parts = ((rows ? n2 : n1) + 63) / 64;
    const int per = (parts + SM_G - 1) / SM_G, p0 = g * per, p1 = min(parts, p0 + per);
    const int ec = min(e, n - 1);
    SsState s;
    for (int pb = p0; pb < p1; pb += 4) {
        float pm[4], pz[4], py[4], pbest[4];
        int parg[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t at = (int64_t)min(pb + k, p1 - 1) * n + ec;
            if (rows) {
                const float4 q = rpart[at];
                pbest[k] = q.x; pm[k] = scale * q.x; pz[k] = q.y; py[k] = q.z; parg[k] = __float_as_int(q.w);
            } else {
                const float2 bq = cbest[at];
                pm[k] = cpart[at * 3]; pz[k] = cpart[at * 3 + 1]; py[k] = cpart[at * 3 + 2]; pbest[k] = bq.x; parg[k] = __float_as_int(bq.y);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (pb + k < p1) s.push(pm[k], pz[k], py[k], pbest[k], parg[k]);
    }
    sh[g][0][lane] = s.m; sh[g][1][lane] = s.z; sh[g][2][lane] = s.y; sh[g][3][lane] = s.best;
    sha[g][lane] = s.arg;
    __syncthreads();
    if (g != 0 || e >= n) return;
    for (int q = 1; q < SM_G; ++q) s.push(sh[q][0][lane], sh[q][1][lane], sh[q][2][lane], sh[q][3][lane], sha[q][lane]);
    float* const omax = rows ? row_max : col_max;
    int32_t* const oarg = rows ? row_arg : col_arg;
    float* const osum = rows ? row_sum : col_sum;
    float* const oent = rows ? row_ent : col_ent;
    if (omax) omax[e] = s.best;
    if (oarg) oarg[e] = s.arg;
    if (osum) osum[e] = s.z;
    if (oent) oent[e] = logf(s.z) - s.y / s.z;
}

// The log-sum-exp partials' merge, in sim_stats_merge_kernel's shape: 64 lines per block, wave g walks the g-th quarter of a line's
// parts in ascending order (loads four ahead), wave 0 combines the quarters in order; out = shift - log sum e^z = shift - (m + log l).
struct LseState {
    float m = -INFINITY, l = 0.f;
    __device__ __forceinline__ void push(float pm, float pl) {
        if (!(pl > 0.f)) return;                                   // nothing behind this partial
        const float mn = fmaxf(m, pm);
        l = expf(m - mn) * l + expf(pm - mn) * pl;
        m = mn;
    }
};
__global__ __launch_bounds__(kBlock) void sim_lse_merge_kernel(const float2* __restrict__ rpart, const float2* __restrict__ cpart, int n1,
                                                               int n2, int row_blocks, float row_shift, float col_shift,
                                                               float* __restrict__ row_out, float* __restrict__ col_out) {
    __shared__ float sh[SM_G][2][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const bool rows = (int)blockIdx.x < row_blocks;
    const int e = ((int)blockIdx.x - (rows ? 0 : row_blocks)) * 64 + lane;
    const int n = rows ? n1 : n2, parts = ((rows ? n2 : n1) + 63) / 64;
    const int per = (parts + SM_G - 1) / SM_G, p0 = g * per, p1 = min(parts, p0 + per);
    const int ec = min(e, n - 1);
    const float2* const part = rows ? rpart : cpart;
    LseState s;
    for (int pb = p0; pb < p1; pb += 4) {
        float2 q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = part[(int64_t)min(pb + k, p1 - 1) * n + ec];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (pb + k < p1) s.push(q[k].x, q[k].y);
    }
    sh[g][0][lane] = s.m;
    sh[g][1][lane] = s.l;
    __syncthreads();
    if (g != 0 || e >= n) return;
    for (int q = 1; q < SM_G; ++q) s.push(sh[q][0][lane], sh[q][1][lane]);
    (rows ? row_out : col_out)[e] = (rows ? row_shift : col_shift) - (s.m + logf(s.l));
}

struct SlWs { size_t rpart, cpart, total; };
SlWs sl_layout(int64_t n1, int64_t n2) {
    SlWs w{};
    size_t off = 0;
    w.rpart = off; off += align_up((size_t)((n2 + 63) / 64) * (size_t)n1 * 8);
    w.cpart = off; off += align_up((size_t)((n1 + 63) / 64) * (size_t)n2 * 8);
    w.total = off + 256;
    return w;
}

struct SsWs { size_t rpart, cpart, cbest, total; };
SsWs ss_layout(int64_t n1, int64_t n2) {
    SsWs w{};
    const size_t pn = (size_t)((n2 + 63) / 64), pm = (size_t)((n1 + 63) / 64);
    size_t off = 0;
    w.rpart = off; off += align_up(pn * (size_t)n1 * 16);
    w.cpart = off; off += align_up(pm * (size_t)n2 * 12);
    w.cbest = off; off += align_up(pm * (size_t)n2 * 8);
    w.total = off + 256;
    return w;
}

int launch_topk(const float* S, int64_t lds, int64_t L, int64_t N, int32_t k, float* val, int32_t* idx, hipStream_t st) {
    if (L == 0) return 0;
    hipLaunchKernelGGL(row_topk_kernel, dim3((unsigned)L), dim3(kBlock), 0, st, S, lds, (int)N, (int)k, val, idx);
    return (int)hipGetLastError();
}

}  // namespace

// the tile kernel with epilogue EPI over the first ncols columns of a's tables
template <typename TT, int EPI>
static void launch_link_tile(const LinkRankArgs& a, bool vec, int64_t ncols, hipStream_t st) {
    dim3 grid((unsigned)((ncols + L1_T - 1) / L1_T), (unsigned)((a.B + L1_T - 1) / L1_T));
    if (vec) hipLaunchKernelGGL((link_rank_tile_kernel<TT, true, EPI>), grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((link_rank_tile_kernel<TT, false, EPI>), grid, dim3(kBlock), 0, st, a);
}

// a jmac_tail_index_t an entry point may read
static bool tail_index_ok(const jmac_tail_index_t* index) {
    return index->n_keys >= 0 && index->n_keys < INT32_MAX && index->key && index->tail_ptr && index->tail_idx;
}

// what every link-prediction entry point, single-KG or ensemble, fills of LinkRankArgs alike: sizes, sign, queries and the index
static void link_base_args(LinkRankArgs& a, int32_t n_layers, const int32_t* h, const int32_t* r, int32_t pred_head,
                           const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d) {
    a.nl = n_layers; a.B = (int32_t)B; a.N = (int32_t)N; a.d = (int32_t)d; a.dq = (int32_t)((d + 3) / 4 * 4);
    a.sign = pred_head ? -1.f : 1.f;
    a.h = h; a.r = r;
    if (index) {
        a.key = index->key; a.n_keys = index->n_keys; a.filt_ptr = index->tail_ptr; a.filt_idx = index->tail_idx;
    }
}

// The prep kernels' LDS: the query's nl * dq words and a.rows candidate rows of one word more, within 60 KB.  false: not even one
// candidate row fits (JMAC_ERANGE at every entry point; the top-k prep kernels stage nothing, but their select kernels do)
static bool prep_lds(LinkRankArgs& a, size_t& shm) {
    const int64_t W = (int64_t)a.nl * a.dq, words = 60 * 1024 / 4;
    const int64_t rows = (words - W) / (W + 1);
    if (rows < 1) return false;
    a.rows = (int32_t)(rows < LR_ROWS ? rows : LR_ROWS);
    shm = (size_t)(W + a.rows * (W + 1)) * sizeof(float);
    return true;
}

// ... and of the single-KG ones: the layer tables.  vec: whether the tile kernel may take its vector form, which issues
// 4-element loads (16 B fp32, 8 B bf16) -- every table's leading dimension AND base pointer must allow it
template <typename TT>
static int link_args(LinkRankArgs& a, bool& vec, const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r,
                     int32_t pred_head, const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d) {
    link_base_args(a, n_layers, h, r, pred_head, index, B, N, d);
    vec = d % 4 == 0;
    for (int l = 0; l < n_layers; ++l) {
        if (!layers[l].ent || !layers[l].rel || !layers[l].table) return JMAC_EINVAL;
        a.ent[l] = layers[l].ent; a.rel[l] = layers[l].rel; a.tab[l] = layers[l].table;
        a.ld_ent[l] = layers[l].ld_ent; a.ld_rel[l] = layers[l].ld_rel; a.ld_tab[l] = layers[l].ld_table;
        if (a.ld_tab[l] % 4 || ((uintptr_t)a.tab[l] % (4 * sizeof(TT)))) vec = false;
    }
    return JMAC_OK;
}

template <typename TT>
static int launch_link_rank(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r, int32_t pred_head,
                            const int32_t* gold, const int32_t* filt_ptr, const int32_t* filt_idx, const jmac_tail_index_t* index,
                            int64_t B, int64_t N, int64_t d, int32_t* rank, void* ws, size_t ws_bytes, hipStream_t st) {
    if (B < 0 || N <= 0 || d <= 0 || n_layers <= 0 || n_layers > LR_MAX_LAYERS) return JMAC_EINVAL;
    if (B == 0) return JMAC_OK;
    if (!layers || !h || !r || !gold || !rank || (filt_ptr && !filt_idx)) return JMAC_EINVAL;
    if (index && !tail_index_ok(index)) return JMAC_EINVAL;
    if (B >= INT32_MAX || N >= INT32_MAX || d > 512) return JMAC_ERANGE;
    if (!ws || ws_bytes < jmac_linkpred_rank_workspace_bytes(B, d, n_layers)) return JMAC_EWORKSPACE;
    LinkRankArgs a{};
    bool vec;
    a.gold = gold; a.filt_ptr = filt_ptr; a.filt_idx = filt_idx;            // the per-batch CSR: an index takes its place
    if (int rc = link_args<TT>(a, vec, layers, n_layers, h, r, pred_head, index, B, N, d)) return rc;
    a.gs = (float*)ws;
    a.er = (char*)ws + align_up((size_t)B * 4);
    a.rank = rank;
    size_t shm;
    if (!prep_lds(a, shm)) return JMAC_ERANGE;
    if (index) hipLaunchKernelGGL((link_rank_prep_kernel<TT, true>), dim3((unsigned)B), dim3(kBlock), shm, st, a);
    else hipLaunchKernelGGL((link_rank_prep_kernel<TT, false>), dim3((unsigned)B), dim3(kBlock), shm, st, a);
    launch_link_tile<TT, LR_COUNT>(a, vec, N, st);
    return (int)hipGetLastError();
}

extern "C" {

int jmac_l1_score_f32(const float* er, int64_t lder, const float* table, int64_t ldt, int64_t B, int64_t N, int64_t d,
                      float* out, int64_t ldout, int32_t accumulate, jmac_stream_t stream) {
    if (B < 0 || N < 0 || d <= 0) return JMAC_EINVAL;
    if (B == 0 || N == 0) return JMAC_OK;
    if (!er || !table || !out) return JMAC_EINVAL;
    if (lder % 4 || ldt % 4) return JMAC_EDIM;
    if (B >= INT32_MAX || N >= INT32_MAX) return JMAC_ERANGE;
    dim3 grid((unsigned)((N + L1_T - 1) / L1_T), (unsigned)((B + L1_T - 1) / L1_T));
    // 4-element vector loads need 4-element-aligned base pointers too (a column-offset view is not): scalar form otherwise
    const bool aligned = (((uintptr_t)er | (uintptr_t)table) % (4 * sizeof(float))) == 0;
    if (d % 4 == 0 && aligned)
        hipLaunchKernelGGL((l1_score_kernel<float, true>), grid, dim3(kBlock), 0, (hipStream_t)stream, er, lder, table, ldt, (int)B,
                           (int)N, (int)d, out, ldout, accumulate);
    else
        hipLaunchKernelGGL((l1_score_kernel<float, false>), grid, dim3(kBlock), 0, (hipStream_t)stream, er, lder, table, ldt, (int)B,
                           (int)N, (int)d, out, ldout, accumulate);
    return (int)hipGetLastError();
}

int jmac_l1_score_bf16(const uint16_t* er, int64_t lder, const uint16_t* table, int64_t ldt, int64_t B, int64_t N, int64_t d,
                       float* out, int64_t ldout, int32_t accumulate, jmac_stream_t stream) {
    if (B < 0 || N < 0 || d <= 0) return JMAC_EINVAL;
    if (B == 0 || N == 0) return JMAC_OK;
    if (!er || !table || !out) return JMAC_EINVAL;
    if (lder % 4 || ldt % 4) return JMAC_EDIM;
    if (B >= INT32_MAX || N >= INT32_MAX) return JMAC_ERANGE;
    dim3 grid((unsigned)((N + L1_T - 1) / L1_T), (unsigned)((B + L1_T - 1) / L1_T));
    // 4-element vector loads need 4-element-aligned base pointers too (a column-offset view is not): scalar form otherwise
    const bool aligned = (((uintptr_t)er | (uintptr_t)table) % (4 * sizeof(uint16_t))) == 0;
    if (d % 4 == 0 && aligned)
        hipLaunchKernelGGL((l1_score_kernel<bf16_t, true>), grid, dim3(kBlock), 0, (hipStream_t)stream, er, lder, table, ldt, (int)B,
                           (int)N, (int)d, out, ldout, accumulate);
    else
        hipLaunchKernelGGL((l1_score_kernel<bf16_t, false>), grid, dim3(kBlock), 0, (hipStream_t)stream, er, lder, table, ldt,
                           (int)B, (int)N, (int)d, out, ldout, accumulate);
    return (int)hipGetLastError();
}

int jmac_filtered_rank_f32(const float* score, int64_t lds, const int32_t* gold, const int32_t* filt_ptr,
                           const int32_t* filt_idx, int64_t B, int64_t N, int32_t descending, int32_t* rank,
                           jmac_stream_t stream) {
    if (B < 0 || N <= 0) return JMAC_EINVAL;
    if (B == 0) return JMAC_OK;
    if (!score || !gold || !rank || (filt_ptr && !filt_idx && false)) return JMAC_EINVAL;
    if (N >= INT32_MAX) return JMAC_ERANGE;
    hipLaunchKernelGGL(filtered_rank_kernel, dim3((unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, score, lds, gold, filt_ptr,
                       filt_idx, (int)N, descending ? 1 : 0, rank);
    return (int)hipGetLastError();
}

size_t jmac_linkpred_rank_workspace_bytes(int64_t B, int64_t d, int32_t n_layers) {
    if (B < 0 || d <= 0 || n_layers <= 0) return 0;
    return align_up((size_t)B * 4) + align_up((size_t)n_layers * (size_t)B * (size_t)((d + 3) / 4 * 4) * 4) + 256;
}

int jmac_linkpred_rank_f32(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r,
                           int32_t pred_head, const int32_t* gold, const int32_t* filt_ptr, const int32_t* filt_idx, int64_t B,
                           int64_t N, int64_t d, int32_t* rank, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    return launch_link_rank<float>(layers, n_layers, h, r, pred_head, gold, filt_ptr, filt_idx, nullptr, B, N, d, rank, ws, ws_bytes,
                                   (hipStream_t)stream);
}

int jmac_linkpred_rank_bf16(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r,
                            int32_t pred_head, const int32_t* gold, const int32_t* filt_ptr, const int32_t* filt_idx, int64_t B,
                            int64_t N, int64_t d, int32_t* rank, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    return launch_link_rank<bf16_t>(layers, n_layers, h, r, pred_head, gold, filt_ptr, filt_idx, nullptr, B, N, d, rank, ws, ws_bytes,
                                    (hipStream_t)stream);
}

int jmac_linkpred_rank_indexed_f32(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r,
                                   int32_t pred_head, const int32_t* gold, const jmac_tail_index_t* index, int64_t B, int64_t N,
                                   int64_t d, int32_t* rank, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    return launch_link_rank<float>(layers, n_layers, h, r, pred_head, gold, nullptr, nullptr, index, B, N, d, rank, ws, ws_bytes,
                                   (hipStream_t)stream);
}

int jmac_linkpred_rank_indexed_bf16(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r,
                                    int32_t pred_head, const int32_t* gold, const jmac_tail_index_t* index, int64_t B, int64_t N,
                                    int64_t d, int32_t* rank, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    return launch_link_rank<bf16_t>(layers, n_layers, h, r, pred_head, gold, nullptr, nullptr, index, B, N, d, rank, ws, ws_bytes,
                                    (hipStream_t)stream);
}

int jmac_sim_matrix_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t M, int64_t N, int64_t d, float* C,
                        int64_t ldc, jmac_stream_t stream) {
    if (M < 0 || N < 0 || d <= 0) return JMAC_EINVAL;
    if (M == 0 || N == 0) return JMAC_OK;
    if (!A || !B || !C) return JMAC_EINVAL;
    if (lda % 4 || ldb % 4) return JMAC_EDIM;
    if (M >= INT32_MAX || N >= INT32_MAX) return JMAC_ERANGE;
    return launch_sim<SG_STORE>(A, lda, B, ldb, M, N, d, C, ldc, SimStore{}, (hipStream_t)stream);
}

}  // extern "C"

// ---- the two-stage row top-k every fused form runs: used when the matrix is wide enough for the column sample to pay ----
constexpr int ST_CAP = TK_CAP;            // candidates kept per row
constexpr int ST_KMAX = 64;
constexpr int64_t ST_MIN_N = 8192;
static inline bool st_fused(int64_t N, int64_t k) { return N >= ST_MIN_N && k <= ST_KMAX; }
static inline int64_t st_sample(int64_t N) {
    int64_t ns = N / 12 > 2048 ? N / 12 : 2048;            // expected candidates per row ~ k * N / Ns <= 12k (cap: 1024)
    return (ns + 127) / 128 * 128;
}
// the fused workspace: the sample's scores at offset 0, its k best per row, every row's candidate list
struct StWs { size_t val0, idx0, cnt, cval, cidx, total; };
static StWs st_layout(int64_t L, int64_t N, int64_t k) {
    StWs w{};
    size_t off = align_up((size_t)L * (size_t)st_sample(N) * 4);
    w.val0 = off; off += align_up((size_t)L * (size_t)k * 4);
    w.idx0 = off; off += align_up((size_t)L * (size_t)k * 4);
    w.cnt = off;  off += align_up((size_t)L * 4);
    w.cval = off; off += align_up((size_t)L * ST_CAP * 4);
    w.cidx = off; off += align_up((size_t)L * ST_CAP * 4);
    w.total = off + 256;
    return w;
}

// One driver for every score source -- the similarity product, the Manhattan alignment, link prediction.  It owns the scheme: the
// narrow / fused decision, the workspace carving, the sample pass, the row passes, the candidate counters, the filter pass, the
// select.  A source scores L rows against N columns (larger is better) and supplies what differs:
//   store(S, ldS, n) -> rc      the scores of the first n columns at (S, ldS), rescored / masked in place
//   filter(f) -> rc             its filter epilogue over the columns from f.n_off: what reaches f.tau is appended to f's lists
//   select(f, val0, idx0)       its select kernel: the k best of every list and of the sample (val0, idx0); an overflowing row recomputes
//   finish                      the kernel the narrow exit runs over (val, idx, L * k) behind the row pass, or nullptr
// wb: the workspace behind the source's own prefix, laid out as st_layout says; ld_narrow: the row stride of the narrow matrix.
template <class Store, class Filter, class Select, class Finish>
static int topk_drive(int64_t L, int64_t N, int32_t k, float* val, int32_t* idx, char* wb, int64_t ld_narrow, hipStream_t st,
                      Store store, Filter filter, Select select, Finish finish) {
    float* S = (float*)wb;                                   // either layout begins with the stored scores
    if (!st_fused(N, k)) {                                   // narrow matrices: every score, then the row pass
        if (int rc = store(S, ld_narrow, N)) return rc;
        if (int rc = launch_topk(S, ld_narrow, L, N, k, val, idx, st)) return rc;
        if (finish) hipLaunchKernelGGL(finish, dim3((unsigned)((L * k + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, val, idx, L * k);
        return (int)hipGetLastError();
    }
    // 1. tau[m] = k-th best score of row m among the first Ns columns: a bound of the row's final k-th score
    const StWs w = st_layout(L, N, k);
    const int64_t Ns = st_sample(N);
    float* val0 = (float*)(wb + w.val0);
    int32_t* idx0 = (int32_t*)(wb + w.idx0);
    if (int rc = store(S, Ns, Ns)) return rc;
    if (int rc = launch_topk(S, Ns, L, Ns, k, val0, idx0, st)) return rc;
    // 2. the REMAINING columns with the filtering epilogue: candidates instead of the matrix
    SimFilter f{};
    f.tau = val0 + (k - 1); f.tau_stride = k;
    f.cnt = (int*)(wb + w.cnt); f.cval = (float*)(wb + w.cval); f.cidx = (int*)(wb + w.cidx); f.cap = ST_CAP; f.n_off = (int)Ns;
    if (hipMemsetAsync(f.cnt, 0, (size_t)L * 4, st) != hipSuccess) return (int)hipGetLastError();
    if (int rc = filter(f)) return rc;
    // 3. the k best of every candidate list (+ the sample's k best)
    select(f, val0, idx0);
    return (int)hipGetLastError();
}

// the similarity product as the source.  jmac_sim_topk_f32 (r1 == nullptr) and jmac_sim_csls_topk_f32: every step works on
// c = csls_value(S, r1, r2), or on S itself.  best != nullptr (jmac_sim_csls_topk_viable_f32): of the columns n with
// tk_pack(c(m, n), row_id[m]) > best[n] only -- one more predicate in each stage; a row with fewer than k of them ends in (idx -1, val -inf)
static int sim_topk_impl(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N, int64_t d, const float* r1,
                         const float* r2, int32_t k, float* val, int32_t* idx, void* ws, hipStream_t st,
                         const int32_t* row_id = nullptr, const unsigned long long* best = nullptr) {
    const dim3 rows((unsigned)L), block(kBlock);
    return topk_drive(L, N, k, val, idx, (char*)ws, N, st,
        [&](float* S, int64_t ldS, int64_t n) -> int {       // the product of A with B's first n rows
            if (int rc = launch_sim<SG_STORE>(A, lda, B, ldb, L, n, d, S, ldS, SimStore{}, st)) return rc;
            if (best) hipLaunchKernelGGL(viable_inplace_kernel, rows, block, 0, st, S, ldS, (int)n, r1, r2, row_id, best);
            else if (r1) hipLaunchKernelGGL(csls_inplace_kernel, rows, block, 0, st, S, ldS, (int)n, r1, r2);
            return 0;
        },
        [&](const SimFilter& f) -> int {
            SimViable cx{};
            cx.f = f; cx.r1 = r1; cx.r2 = r2; cx.row_id = row_id; cx.best = best;
            const float* Br = B + f.n_off * ldb;
            return best ? launch_sim<SG_CSLS_VIABLE>(A, lda, Br, ldb, L, N - f.n_off, d, nullptr, 0, cx, st)
                   : r1 ? launch_sim<SG_CSLS_FILTER>(A, lda, Br, ldb, L, N - f.n_off, d, nullptr, 0, cx, st)
                        : launch_sim<SG_FILTER>(A, lda, Br, ldb, L, N - f.n_off, d, nullptr, 0, f, st);
        },
        [&](const SimFilter& f, const float* val0, const int32_t* idx0) {      // an overflowing row recomputes (and rescores)
            if (best)
                hipLaunchKernelGGL(cand_select_viable_kernel<false>, rows, block, 0, st, A, lda, B, ldb, (int)N, (int)d, (int)k, f.cnt, f.cval,
                                   f.cidx, f.cap, val0, idx0, val, idx, r1, r2, row_id, best);
            else
                hipLaunchKernelGGL(r1 ? cand_select_kernel<true> : cand_select_kernel<false>, rows, block, 0, st, A, lda, B, ldb, (int)N, (int)d,
                                   (int)k, f.cnt, f.cval, f.cidx, f.cap, val0, idx0, val, idx, r1, r2);
        },
        best ? viable_topk_finish_kernel : nullptr);
}

extern "C" {

size_t jmac_sim_topk_workspace_bytes(int64_t L, int64_t N, int32_t k) {
    if (L < 0 || N < 0 || k <= 0) return 0;
    if (st_fused(N, k)) return st_layout(L, N, k).total;      // sample scores + candidate lists: no L x N matrix
    return align_up((size_t)L * (size_t)N * 4) + 256;
}

int jmac_row_topk_f32(const float* S, int64_t lds, int64_t L, int64_t N, int32_t k, float* val, int32_t* idx,
                      jmac_stream_t stream) {
    if (L < 0 || N <= 0 || k <= 0 || k > N) return JMAC_EINVAL;
    if (L == 0) return JMAC_OK;
    if (!S || !idx) return JMAC_EINVAL;
    return launch_topk(S, lds, L, N, k, val, idx, (hipStream_t)stream);
}

int jmac_sim_topk_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N, int64_t d, int32_t k,
                      float* val, int32_t* idx, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    if (L < 0 || N <= 0 || d <= 0 || k <= 0 || k > N) return JMAC_EINVAL;
    if (L == 0) return JMAC_OK;
    if (!A || !B || !idx) return JMAC_EINVAL;
    if (lda % 4 || ldb % 4) return JMAC_EDIM;
    if (!ws || ws_bytes < jmac_sim_topk_workspace_bytes(L, N, k)) return JMAC_EWORKSPACE;
    return sim_topk_impl(A, lda, B, ldb, L, N, d, nullptr, nullptr, k, val, idx, ws, (hipStream_t)stream);
}

}  // extern "C"

// ---- link-prediction top-k: the L1 tile loop over prepared query rows as the source ---------------------------------------------
// the prefix (query rows, index ranges), then jmac_sim_topk_f32's workspace for B rows; narrow: rows padded to 4 elements
struct LtWs { size_t er, rng, tail, total; int64_t ld_narrow; };
static LtWs lt_layout(int64_t B, int64_t N, int64_t d, int64_t nl, int64_t k) {
    LtWs w{};
    size_t off = 0;
    w.er = off;  off += align_up((size_t)nl * (size_t)B * (size_t)((d + 3) / 4 * 4) * 4);
    w.rng = off; off += align_up((size_t)B * 8);
    w.tail = off;
    w.ld_narrow = (N + 3) / 4 * 4;
    w.total = off + (st_fused(N, k) ? st_layout(B, N, k).total : align_up((size_t)B * (size_t)w.ld_narrow * 4) + 256);
    return w;
}

// the tile kernel's STORE epilogue over the first n columns, and a with the filter epilogues' thresholds and candidate lists (S and
// ldS stay unset there: only the STORE epilogue reads them)
template <typename TT>
static void launch_link_store(LinkRankArgs a, bool vec, float* S, int64_t ldS, int64_t n, hipStream_t st) {
    a.N = (int32_t)n; a.S = S; a.ldS = ldS; a.n_off = 0;
    launch_link_tile<TT, LR_STORE>(a, vec, n, st);
}
static LinkRankArgs link_filter_args(LinkRankArgs a, const SimFilter& f) {
    a.ntau = f.tau; a.tau_stride = (int32_t)f.tau_stride; a.cap = f.cap;
    a.cnt = f.cnt; a.cval = f.cval; a.cidx = f.cidx; a.n_off = f.n_off;
    return a;
}

// the scores are -dist; the index's listed tails are masked in the stored scores and skipped by the filter and the select
template <typename TT>
static int launch_link_topk(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r, int32_t pred_head,
                            const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d, int32_t k, float* val, int32_t* idx,
                            void* ws, size_t ws_bytes, hipStream_t st) {
    if (B < 0 || N <= 0 || d <= 0 || n_layers <= 0 || n_layers > LR_MAX_LAYERS) return JMAC_EINVAL;
    if (k <= 0 || k > ST_KMAX || k > N) return JMAC_EINVAL;
    if (d > 512) return JMAC_EDIM;
    if (B == 0) return JMAC_OK;
    if (!layers || !h || !r || !val || !idx) return JMAC_EINVAL;
    if (index && !tail_index_ok(index)) return JMAC_EINVAL;
    if (B >= INT32_MAX || N >= INT32_MAX) return JMAC_ERANGE;
    if (!ws || ws_bytes < jmac_linkpred_topk_workspace_bytes(B, N, d, n_layers, k)) return JMAC_EWORKSPACE;
    LinkRankArgs a{};
    bool vec;
    if (int rc = link_args<TT>(a, vec, layers, n_layers, h, r, pred_head, index, B, N, d)) return rc;
    const int64_t W = (int64_t)n_layers * a.dq;
    size_t shm;                                                // unused: RANK = false stages only the W query words
    if (!prep_lds(a, shm)) return JMAC_ERANGE;                 // jmac_linkpred_rank_*'s LDS limit
    const LtWs w = lt_layout(B, N, d, n_layers, k);
    char* wb = (char*)ws;
    a.er = wb + w.er;
    a.rng = (int2*)(wb + w.rng);
    // the query rows and every query's range in the index
    if (index) hipLaunchKernelGGL((link_rank_prep_kernel<TT, true, false>), dim3((unsigned)B), dim3(kBlock), (size_t)W * 4, st, a);
    else hipLaunchKernelGGL((link_rank_prep_kernel<TT, false, false>), dim3((unsigned)B), dim3(kBlock), (size_t)W * 4, st, a);
    return topk_drive(B, N, k, val, idx, wb + w.tail, w.ld_narrow, st,
        [&](float* S, int64_t ldS, int64_t n) -> int {
            launch_link_store<TT>(a, vec, S, ldS, n, st);
            if (index) hipLaunchKernelGGL(link_mask_kernel, dim3((unsigned)B), dim3(kBlock), 0, st, S, ldS, (int)n, a.rng, a.filt_idx);
            return 0;
        },
        [&](const SimFilter& f) -> int {
            launch_link_tile<TT, LR_FILTER>(link_filter_args(a, f), vec, N - f.n_off, st);
            return 0;
        },
        [&](const SimFilter& f, const float* val0, const int32_t* idx0) {
            hipLaunchKernelGGL((link_select_kernel<TT>), dim3((unsigned)B), dim3(kBlock), (size_t)W * 4, st, link_filter_args(a, f), (int)k, val0,
                               idx0, val, idx);
        },
        link_topk_finish_kernel);
}

extern "C" {

size_t jmac_linkpred_topk_workspace_bytes(int64_t B, int64_t N, int64_t d, int32_t n_layers, int32_t k) {
    if (B < 0 || N <= 0 || d <= 0 || n_layers <= 0 || k <= 0) return 0;
    return lt_layout(B, N, d, n_layers, k).total;
}

int jmac_linkpred_topk_f32(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r, int32_t pred_head,
                           const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d, int32_t k, float* val, int32_t* idx,
                           void* ws, size_t ws_bytes, jmac_stream_t stream) {
    return launch_link_topk<float>(layers, n_layers, h, r, pred_head, index, B, N, d, k, val, idx, ws, ws_bytes, (hipStream_t)stream);
}

int jmac_linkpred_topk_bf16(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r, int32_t pred_head,
                            const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d, int32_t k, float* val, int32_t* idx,
                            void* ws, size_t ws_bytes, jmac_stream_t stream) {
    return launch_link_topk<bf16_t>(layers, n_layers, h, r, pred_head, index, B, N, d, k, val, idx, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"

// ---- link-prediction confidence (jmac_linkpred_stats_*, jmac_linkpred_ens_stats_f32): the LR_STATS epilogue, merged -------------
// The definition is include/jmac_hip.h's.  After the prep kernel (query rows, every query's range in the index, and with gold the
// gold distance gs) the tile kernel's LR_STATS epilogue leaves one float4 per (64-column part, query); sim_stats_merge_kernel's row
// side folds a query's parts in ascending order with SsState -- the merge jmac_sim_softmax_stats_f32 runs, on max = -dist_min --
// and link_stats_finish_kernel turns (max, arg, sum, entropy) into the outputs: the empty set's values, dmin = -max, logp_gold.
namespace {

__global__ __launch_bounds__(kBlock) void link_stats_finish_kernel(int B, float scale, const float* __restrict__ mbest,
                                                                   const int32_t* __restrict__ marg, const float* __restrict__ msum,
                                                                   const float* __restrict__ ment, const float* __restrict__ gs,
                                                                   int32_t* __restrict__ near, float* __restrict__ dmin,
                                                                   float* __restrict__ sum, float* __restrict__ ent,
                                                                   float* __restrict__ logp_gold) {
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    const float best = mbest[b], l = msum[b];
    const bool some = l > 0.f;                                 // false: every candidate is listed (prediction mode only)
    if (near) near[b] = some ? marg[b] : -1;
    if (dmin) dmin[b] = some ? (best == 0.f ? 0.f : -best) : INFINITY;       // jmac_linkpred_topk_*'s bits of the distance
    if (sum) sum[b] = some ? l : 0.f;
    if (ent) ent[b] = some ? ment[b] : 0.f;
    // the gold is in the set: l >= 1.  best = -dmin, so -(gs + best) = dmin - gs <= 0, and where the gold is the nearest it is -0
    // exactly: that row is -log(sum) bit for bit, the sign of -log(1) included.  The logarithm is taken in double precision and
    // rounded once -- the correctly rounded fp32 value, which a caller can reproduce; logf's last bit varies between libraries
    if (logp_gold) logp_gold[b] = scale * -(gs[b] + best) - (float)log((double)l);
}

// what both statistics calls append to their rank workspace: rng, the merge's four vectors and the partials
struct LsWs { size_t rank, rng, mbest, marg, msum, ment, part, total; };
LsWs ls_layout(size_t off, int64_t B, int64_t N) {
    LsWs w{};
    const size_t vec = align_up((size_t)B * 4);
    w.rank = off;  off += vec;                                 // the prep walk's filter correction: written, not read
    w.rng = off;   off += align_up((size_t)B * 8);
    w.mbest = off; off += vec;
    w.marg = off;  off += vec;
    w.msum = off;  off += vec;
    w.ment = off;  off += vec;
    w.part = off;  off += align_up((size_t)((N + L1_T - 1) / L1_T) * (size_t)B * 16);
    w.total = off + 256;
    return w;
}

// the argument checks both calls share beyond the rank entry points' (the caller has checked the sizes and B > 0)
int link_stats_check(const int32_t* gold, const int32_t* near, const float* dmin, const float* sum, const float* ent,
                     const float* logp_gold) {
    if (!(near || dmin || sum || ent || logp_gold) || (logp_gold && !gold)) return JMAC_EINVAL;
    return JMAC_OK;
}

// merge + finish over the partials the tile kernel has left in a.S
int link_stats_finish(const LinkRankArgs& a, const LsWs& w, char* wb, int32_t* near, float* dmin, float* sum, float* ent,
                      float* logp_gold, hipStream_t st) {
    float* const mbest = (float*)(wb + w.mbest);
    int32_t* const marg = (int32_t*)(wb + w.marg);
    float* const msum = (float*)(wb + w.msum);
    float* const ment = (float*)(wb + w.ment);
    const int rb = (a.B + 63) / 64;
    hipLaunchKernelGGL(sim_stats_merge_kernel, dim3((unsigned)rb), dim3(kBlock), 0, st, (const float4*)a.S, nullptr, nullptr, a.B, a.N,
                       a.scale, rb, mbest, marg, msum, ment, nullptr, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(link_stats_finish_kernel, dim3((unsigned)((a.B + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a.B, a.scale, mbest,
                       marg, msum, ment, a.gs, near, dmin, sum, ent, logp_gold);
    return (int)hipGetLastError();
}

}  // namespace

template <typename TT>
static int launch_link_stats(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r, int32_t pred_head,
                             const int32_t* gold, const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d, float scale,
                             int32_t* near, float* dmin, float* sum, float* ent, float* logp_gold, void* ws, size_t ws_bytes,
                             hipStream_t st) {
    if (B < 0 || N <= 0 || d <= 0 || n_layers <= 0 || n_layers > LR_MAX_LAYERS) return JMAC_EINVAL;
    if (!(scale > 0.f) || !std::isfinite(scale)) return JMAC_EINVAL;
    if (int rc = link_stats_check(gold, near, dmin, sum, ent, logp_gold)) return rc;
    if (B == 0) return JMAC_OK;
    if (!layers || !h || !r) return JMAC_EINVAL;
    if (index && !tail_index_ok(index)) return JMAC_EINVAL;
    if (B >= INT32_MAX || N >= INT32_MAX || d > 512) return JMAC_ERANGE;
    if (!ws || ws_bytes < jmac_linkpred_stats_workspace_bytes(B, N, d, n_layers)) return JMAC_EWORKSPACE;
    LinkRankArgs a{};
    bool vec;
    a.gold = gold;
    if (int rc = link_args<TT>(a, vec, layers, n_layers, h, r, pred_head, index, B, N, d)) return rc;
    const size_t rank_ws = jmac_linkpred_rank_workspace_bytes(B, d, n_layers) - 256;
    const LsWs w = ls_layout(rank_ws, B, N);
    char* wb = (char*)ws;
    a.gs = (float*)wb;                                         // (jmac_linkpred_rank_*'s layout: gs, then the query rows)
    a.er = wb + align_up((size_t)B * 4);
    a.rank = (int32_t*)(wb + w.rank);
    a.rng = (int2*)(wb + w.rng);
    a.S = (float*)(wb + w.part);
    a.scale = scale;
    size_t shm;
    if (!prep_lds(a, shm)) return JMAC_ERANGE;
    const size_t shq = (size_t)n_layers * a.dq * 4;            // without gold the prep kernel stages the query rows only
    const dim3 grid((unsigned)B), block(kBlock);
    if (gold && index) hipLaunchKernelGGL((link_rank_prep_kernel<TT, true, true, true>), grid, block, shm, st, a);
    else if (gold) hipLaunchKernelGGL((link_rank_prep_kernel<TT, false, true, true>), grid, block, shm, st, a);
    else if (index) hipLaunchKernelGGL((link_rank_prep_kernel<TT, true, false>), grid, block, shq, st, a);
    else hipLaunchKernelGGL((link_rank_prep_kernel<TT, false, false>), grid, block, shq, st, a);
    launch_link_tile<TT, LR_STATS>(a, vec, N, st);
    return link_stats_finish(a, w, wb, near, dmin, sum, ent, logp_gold, st);
}

extern "C" {

size_t jmac_linkpred_stats_workspace_bytes(int64_t B, int64_t N, int64_t d, int32_t n_layers) {
    if (B < 0 || N <= 0 || d <= 0 || n_layers <= 0) return 0;
    return ls_layout(jmac_linkpred_rank_workspace_bytes(B, d, n_layers) - 256, B, N).total;
}

int jmac_linkpred_stats_f32(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r, int32_t pred_head,
                            const int32_t* gold, const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d, float scale,
                            int32_t* near, float* dmin, float* sum, float* ent, float* logp_gold, void* ws, size_t ws_bytes,
                            jmac_stream_t stream) {
    return launch_link_stats<float>(layers, n_layers, h, r, pred_head, gold, index, B, N, d, scale, near, dmin, sum, ent, logp_gold, ws,
                                    ws_bytes, (hipStream_t)stream);
}

int jmac_linkpred_stats_bf16(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r, int32_t pred_head,
                             const int32_t* gold, const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d, float scale,
                             int32_t* near, float* dmin, float* sum, float* ent, float* logp_gold, void* ws, size_t ws_bytes,
                             jmac_stream_t stream) {
    return launch_link_stats<bf16_t>(layers, n_layers, h, r, pred_head, gold, index, B, N, d, scale, near, dmin, sum, ent, logp_gold, ws,
                                     ws_bytes, (hipStream_t)stream);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// cross-KG ensemble link prediction (jmac_linkpred_ens_*): ranks and top-k of the target KG's tails on a distance that several
// KGs vote on through alignment links.  Members g = 0 .. S (S <= 3): member 0 is the target with N candidate rows; a supporting
// member s >= 1 has its own layer tables (same n_layers and d, n_rows_s rows), a link map link_s [N] (the row of KG s aligned with
// target row n, or -1) and a weight w_s >= 0; the weights need not sum to 1.  For query b = (h_b, r_b) and candidate n
//     d_g[b, n]      jmac_linkpred_rank_*'s single running fp32 sum over (layer, k) of member g's tables, with
//                    (query row, candidate row) = (h_b, n) for g = 0 and (link_s[h_b], link_s[n]) for g = s
//     present_s(b,n) = link_s[h_b] >= 0 and link_s[n] >= 0     (a link outside [0, n_rows_s) is absent: never dereferenced)
//     D = w_0 * d_0;  for s = 1 .. S in that order:  D = fmaf(w_s, present_s ? d_s : d_0, D)
// A missing link falls back to the target's own distance: an entity is never penalised for being unaligned.  One member with
// w_0 = 1 gives d_0 bit for bit.  Ranks, top-k, the tie rule, pred_head (the sign applies in every member) and the padding are
// jmac_linkpred_rank_* / jmac_linkpred_topk_*'s, decided on D; the filter is the TARGET's known-tail index.  ens_fold below is
// the ONE place D is formed -- prep kernel (gold and filter entries), tile kernel, select kernel's recompute -- so the j-th
// prediction ranks j + 1 and two calls return identical bits; no float atomics, nothing depends on the grid or the CU count.
// These are kernels of their own (three accumulator sets: 96-102 VGPRs against the single-KG tile kernel's 56,
// profiles/linkpred_ensemble_resources.txt) that share the single-KG kernels' body: slab loop, epilogues, sequential sum, prep walk
// and select merge are the L1 tile family's pieces, called here with the members' sources.
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int LE_MAX = 4;                  // members
struct LinkEnsArgs {
    LinkRankArgs base;                     // sizes, sign, queries, gold, index and the epilogues' arguments; er = [ng][nl][B][dq]
    const float* ent[LE_MAX][LR_MAX_LAYERS];
    const float* rel[LE_MAX][LR_MAX_LAYERS];
    const float* tab[LE_MAX][LR_MAX_LAYERS];
    int64_t ld_ent[LE_MAX][LR_MAX_LAYERS], ld_rel[LE_MAX][LR_MAX_LAYERS], ld_tab[LE_MAX][LR_MAX_LAYERS];
    const int32_t* link[LE_MAX];           // [N]; link[0] == nullptr (the identity)
    int32_t n_rows[LE_MAX];
    float w[LE_MAX];
    int32_t ng;
    int32_t* hq;                           // workspace [ng][B]: the query's head row in member g, -1 = not linked
};

// D after member g: the only place the combination is evaluated.  g = 0 is ens_fold(0, w_0, true, d_0, d_0) == w_0 * d_0.
__device__ __forceinline__ float ens_fold(float D, float w, bool present, float dg, float d0) { return fmaf(w, present ? dg : d0, D); }

// the row of member g aligned with target row n (0 <= n < N), -1 if there is none
__device__ __forceinline__ int ens_row(const LinkEnsArgs& e, int g, int n) {
    if (g == 0) return n;
    const int v = e.link[g][n];
    return (v >= 0 && v < e.n_rows[g]) ? v : -1;
}

// link_rank_prep_kernel for the ensemble.  One block per query: (1) its head row and query rows in every member (rows of an
// unlinked head are zero) -> workspace; (2) RANK: link_prep_walk on D -- the members take turns in the SAME LDS (their query
// rows, then the candidates' rows read through the link), one lane per candidate runs l1_seq_sum and folds it into its D.
template <bool INDEXED, bool RANK, bool RNG = !RANK>
__global__ __launch_bounds__(kBlock) void link_ens_prep_kernel(LinkEnsArgs e) {
    const LinkRankArgs& a = e.base;
    extern __shared__ float le_sh[];                // RANK: [nl*dq] query rows + [rows][nl*dq + 1] candidate rows, one member at a time
    __shared__ int2 rng_sh;
    const int b = blockIdx.x, d = a.d, dq = a.dq, W = a.nl * dq, WS = W + 1;
    const int hb = a.h[b], rb = a.r[b], g = RANK ? a.gold[b] : 0;
    float* const er = static_cast<float*>(a.er);
    if constexpr (INDEXED)
        if (threadIdx.x < 64) {
            const int2 rg = tail_range(a, hb, rb);
            if (threadIdx.x == 0) rng_sh = rg;
        }
    for (int m = 0; m < e.ng; ++m) {
        const int hq = ens_row(e, m, hb);
        if (threadIdx.x == 0) e.hq[(int64_t)m * a.B + b] = hq;
        for (int l = 0; l < a.nl; ++l)
            for (int k = threadIdx.x; k < dq; k += kBlock) {
                float v = 0.f;
                if (hq >= 0 && k < d) v = e.ent[m][l][(int64_t)hq * e.ld_ent[m][l] + k] + a.sign * e.rel[m][l][(int64_t)rb * e.ld_rel[m][l] + k];
                er[(((int64_t)m * a.nl + l) * a.B + b) * dq + k] = v;
            }
    }
    int f0, f1;
    if constexpr (INDEXED) {
        __syncthreads();
        f0 = rng_sh.x, f1 = rng_sh.y;
    } else {
        f0 = 0, f1 = 0;
    }
    if constexpr (RNG)
        if (threadIdx.x == 0) a.rng[b] = make_int2(f0, f1);
    if constexpr (!RANK) return;
    float* const erow = le_sh;
    float* const crow = le_sh + W;
    link_prep_walk(a, b, g, f0, f1, [&](int nc, const int* cand) -> float {
        float D = 0.f, d0 = 0.f;
        for (int m = 0; m < e.ng; ++m) {
            const int hq = ens_row(e, m, hb);
            if (m > 0) __syncthreads();             // the previous member's rows consumed
            for (int l = 0; l < a.nl; ++l)          // the thread that wrote an element above reads it back
                for (int k = threadIdx.x; k < dq; k += kBlock) erow[l * dq + k] = er[(((int64_t)m * a.nl + l) * a.B + b) * dq + k];
            for (int i = threadIdx.x; i < nc * W; i += kBlock) {
                const int rI = i / W, q = i - rI * W, l = q / dq, k = q - l * dq;
                const int n = cand[rI];
                const int cn = (n >= 0 && hq >= 0) ? ens_row(e, m, n) : -1;
                float v = 0.f;
                if (cn >= 0 && k < d) v = e.tab[m][l][(int64_t)cn * e.ld_tab[m][l] + k];
                crow[rI * WS + q] = v;
            }
            __syncthreads();
            if (threadIdx.x < nc) {
                float acc = 0.f;
                for (int l = 0; l < a.nl; ++l) acc = l1_seq_sum<true>(acc, erow + l * dq, crow + threadIdx.x * WS + l * dq, d);
                const int n = cand[threadIdx.x];
                const bool present = hq >= 0 && n >= 0 && ens_row(e, m, n) >= 0;
                if (m == 0) d0 = acc;
                D = ens_fold(D, e.w[m], m == 0 || present, acc, d0);
            }
        }
        return D;
    });
}

// link_rank_tile_kernel for the ensemble: the same body with the member loop OUTSIDE the layer / slab loop.  Member 0's sums are
// kept (d0), every member's sums are folded into the total when its slabs end, and the COUNT / STORE / FILTER epilogues run on
// the total.  A supporting member's candidate rows are read THROUGH the link map: a thread loads link_s[n0 + lrow], then its
// 16-byte pieces of that row; an absent link reads row 0 and is zeroed when staged, and its sums are never selected.  A tile in
// which member s has no linked head or no linked candidate skips that member's slabs (the fold takes d0 for every pair: no bit
// changes); the decision is block-uniform (__syncthreads_or).
template <bool VEC, int EPI>
__global__ __launch_bounds__(kBlock) void link_ens_tile_kernel(LinkEnsArgs e) {
    const LinkRankArgs& a = e.base;
    __shared__ __attribute__((aligned(16))) float As[2][L1_K][L1_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][L1_K][L1_LD];
    __shared__ int qbits[L1_T], cbits[L1_T];        // bit g: the row's head / the column's candidate has a row in member g
    const int B = a.B, N = a.N, d = a.d;
    const L1Pos p = l1_pos(blockIdx.y * L1_T, (EPI == LR_COUNT ? 0 : a.n_off) + blockIdx.x * L1_T);
    const int arow = p.b0 + p.lrow, brow = p.n0 + p.lrow;
    const bool a_ok = arow < B, b_ok = brow < N;
    int qb = 0, cb = 0;
    for (int g = 0; g < e.ng; ++g) {
        qb |= (a_ok && e.hq[(int64_t)g * B + arow] >= 0) ? 1 << g : 0;
        cb |= (b_ok && ens_row(e, g, brow) >= 0) ? 1 << g : 0;
    }
    if (p.lk == 0) {
        qbits[p.lrow] = qb;
        cbits[p.lrow] = cb;
    }
    float acc[4][4], d0[4][4], tot[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = d0[i][j] = tot[i][j] = 0.f;
    const int nk = (d + L1_K - 1) / L1_K;                      // slabs of one member: layer-major, k inside
    const float* const er = static_cast<const float*>(a.er);
    const int64_t arow_c = a_ok ? arow : B - 1;
    for (int g = 0; g < e.ng; ++g) {
        // block-uniform: does any pair of this tile use member g's distance?  (also the barrier that completes qbits / cbits)
        const int any_q = __syncthreads_or((qb >> g) & 1), any_c = __syncthreads_or((cb >> g) & 1);
        if (any_q && any_c) {
            const int cn = b_ok ? ens_row(e, g, brow) : -1;
            const bool c_ok = cn >= 0;
            const int64_t crow = c_ok ? cn : 0;
            l1_slab_loop<VEC>(acc, As, Bs, p, a.nl * nk, d, a_ok, c_ok, [&](int s, float4& ra, float4& rb) {
                const int l = s / nk, k0 = (s - l * nk) * L1_K;
                ra = l1_load<float, VEC>(er + ((int64_t)g * a.nl + l) * B * a.dq, a.dq, arow_c, a_ok, k0 + p.lk, d);
                rb = l1_load<float, VEC>(e.tab[g][l], e.ld_tab[g][l], crow, c_ok, k0 + p.lk, d);
                return k0;
            });
        }
        const float w = e.w[g];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool qp = (qbits[p.ty * 4 + i] >> g) & 1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool present = g == 0 || (qp && ((cbits[p.tx * 4 + j] >> g) & 1));
                if (g == 0) d0[i][j] = acc[i][j];
                tot[i][j] = ens_fold(tot[i][j], w, present, acc[i][j], d0[i][j]);
                acc[i][j] = 0.f;
            }
        }
    }
    static_assert(EPI == LR_COUNT || EPI == LR_STORE || EPI == LR_FILTER || EPI == LR_STATS, "the ensemble has no alignment epilogues");
    l1_epilogue<EPI>(tot, p, a);
}

// link_select_kernel for the ensemble: an overflowing row recomputes D of its N candidates with the prep kernel's sums and folds,
// one lane per candidate (the query rows come from the workspace: every lane reads the same address).
__global__ __launch_bounds__(kBlock) void link_ens_select_kernel(LinkEnsArgs e, int k, const float* __restrict__ sval,
                                                                 const int32_t* __restrict__ sidx, float* __restrict__ val,
                                                                 int32_t* __restrict__ idx) {
    const LinkRankArgs& a = e.base;
    __shared__ TkShared tk;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int2 r = a.rng[b];                                   // the query's listed tails
    const LinkEmit emit{val + (int64_t)b * k, idx + (int64_t)b * k};
    if (link_select_listed(a, b, r, k, sval, sidx, tk, emit)) return;
    const int d = a.d, dq = a.dq;
    const float* const er = static_cast<const float*>(a.er);
    auto for_each_unlisted = [&](auto f) {                      // f(n, -D[b, n]) for every n in [0, N) the index does not list
        for (int n = tid; n < a.N; n += kBlock) {
            if (tail_listed(a.filt_idx, r.x, r.y, n)) continue;
            float D = 0.f, d0 = 0.f;
            for (int g = 0; g < e.ng; ++g) {
                const int cn = e.hq[(int64_t)g * a.B + b] >= 0 ? ens_row(e, g, n) : -1;
                float acc = 0.f;
                if (cn >= 0)
                    for (int l = 0; l < a.nl; ++l)
                        acc = l1_seq_sum(acc, er + (((int64_t)g * a.nl + l) * a.B + b) * dq, e.tab[g][l] + (int64_t)cn * e.ld_tab[g][l], d);
                if (g == 0) d0 = acc;
                D = ens_fold(D, e.w[g], cn >= 0, acc, d0);
            }
            f(n, -D);
        }
    };
    tk_select_recomputed(tk, k, for_each_unlisted, emit);
}

}  // namespace

template <int EPI>
static void launch_ens_tile(const LinkEnsArgs& e, bool vec, int64_t ncols, hipStream_t st) {
    dim3 grid((unsigned)((ncols + L1_T - 1) / L1_T), (unsigned)((e.base.B + L1_T - 1) / L1_T));
    if (vec) hipLaunchKernelGGL((link_ens_tile_kernel<true, EPI>), grid, dim3(kBlock), 0, st, e);
    else hipLaunchKernelGGL((link_ens_tile_kernel<false, EPI>), grid, dim3(kBlock), 0, st, e);
}

// argument checks and LinkEnsArgs of both entry points (the caller has checked the sizes, B > 0 and its own pointers)
static int ens_args(LinkEnsArgs& e, bool& vec, const jmac_link_member_t* members, int32_t n_members, int32_t n_layers, const int32_t* h,
                    const int32_t* r, int32_t pred_head, const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d) {
    if (!members || !h || !r) return JMAC_EINVAL;
    if (index && !tail_index_ok(index)) return JMAC_EINVAL;
    for (int g = 0; g < n_members; ++g) {
        const jmac_link_member_t& m = members[g];
        if (!m.layers || (g == 0) != (m.link == nullptr) || m.n_rows <= 0 || (g == 0 && m.n_rows != N)) return JMAC_EINVAL;
        if (!(m.weight >= 0.f) || !std::isfinite(m.weight)) return JMAC_EINVAL;
        if (m.n_rows >= INT32_MAX) return JMAC_ERANGE;
    }
    link_base_args(e.base, n_layers, h, r, pred_head, index, B, N, d);
    e.ng = n_members;
    vec = d % 4 == 0;
    for (int g = 0; g < n_members; ++g) {
        e.link[g] = members[g].link; e.n_rows[g] = (int32_t)members[g].n_rows; e.w[g] = members[g].weight;
        for (int l = 0; l < n_layers; ++l) {
            const jmac_link_layer_t& y = members[g].layers[l];
            if (!y.ent || !y.rel || !y.table) return JMAC_EINVAL;
            e.ent[g][l] = y.ent; e.rel[g][l] = y.rel; e.tab[g][l] = static_cast<const float*>(y.table);
            e.ld_ent[g][l] = y.ld_ent; e.ld_rel[g][l] = y.ld_rel; e.ld_tab[g][l] = y.ld_table;
            if (y.ld_table % 4 || ((uintptr_t)y.table % 16)) vec = false;
        }
    }
    return JMAC_OK;
}

// the prefix of both workspaces: every member's query rows and head rows
struct LeWs { size_t er, hq, end; };
static LeWs le_layout(int64_t B, int64_t d, int64_t nl, int64_t ng) {
    LeWs w{};
    size_t off = 0;
    w.er = off; off += align_up((size_t)ng * (size_t)nl * (size_t)B * (size_t)((d + 3) / 4 * 4) * 4);
    w.hq = off; off += align_up((size_t)ng * (size_t)B * 4);
    w.end = off;
    return w;
}

extern "C" {

size_t jmac_linkpred_ens_rank_workspace_bytes(int64_t B, int64_t d, int32_t n_layers, int32_t n_members) {
    if (B < 0 || d <= 0 || n_layers <= 0 || n_members <= 0) return 0;
    return le_layout(B, d, n_layers, n_members).end + align_up((size_t)B * 4) + 256;
}

int jmac_linkpred_ens_rank_f32(const jmac_link_member_t* members, int32_t n_members, int32_t n_layers, const int32_t* h, const int32_t* r,
                               int32_t pred_head, const int32_t* gold, const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d,
                               int32_t* rank, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    if (B < 0 || N <= 0 || d <= 0 || n_layers <= 0 || n_layers > LR_MAX_LAYERS || n_members < 1 || n_members > LE_MAX) return JMAC_EINVAL;
    if (B == 0) return JMAC_OK;
    if (!gold || !rank) return JMAC_EINVAL;
    if (B >= INT32_MAX || N >= INT32_MAX || d > 512) return JMAC_ERANGE;
    LinkEnsArgs e{};
    bool vec;
    if (int rc = ens_args(e, vec, members, n_members, n_layers, h, r, pred_head, index, B, N, d)) return rc;
    if (!ws || ws_bytes < jmac_linkpred_ens_rank_workspace_bytes(B, d, n_layers, n_members)) return JMAC_EWORKSPACE;
    LinkRankArgs& a = e.base;
    const LeWs w = le_layout(B, d, n_layers, n_members);
    a.gold = gold; a.rank = rank;
    a.er = (char*)ws + w.er;
    e.hq = (int32_t*)((char*)ws + w.hq);
    a.gs = (float*)((char*)ws + w.end);
    size_t shm;
    if (!prep_lds(a, shm)) return JMAC_ERANGE;                 // jmac_linkpred_rank_*'s LDS limit: the members share that LDS
    if (index) hipLaunchKernelGGL((link_ens_prep_kernel<true, true>), dim3((unsigned)B), dim3(kBlock), shm, st, e);
    else hipLaunchKernelGGL((link_ens_prep_kernel<false, true>), dim3((unsigned)B), dim3(kBlock), shm, st, e);
    launch_ens_tile<LR_COUNT>(e, vec, N, st);
    return (int)hipGetLastError();
}

size_t jmac_linkpred_ens_topk_workspace_bytes(int64_t B, int64_t N, int64_t d, int32_t n_layers, int32_t n_members, int32_t k) {
    if (B < 0 || N <= 0 || d <= 0 || n_layers <= 0 || n_members <= 0 || k <= 0) return 0;
    const LtWs t = lt_layout(B, N, d, 0, k);                   // (no query rows of its own: rng, then the driver's workspace)
    return le_layout(B, d, n_layers, n_members).end + t.total;
}

int jmac_linkpred_ens_topk_f32(const jmac_link_member_t* members, int32_t n_members, int32_t n_layers, const int32_t* h, const int32_t* r,
                               int32_t pred_head, const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d, int32_t k, float* val,
                               int32_t* idx, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    if (B < 0 || N <= 0 || d <= 0 || n_layers <= 0 || n_layers > LR_MAX_LAYERS || n_members < 1 || n_members > LE_MAX) return JMAC_EINVAL;
    if (k <= 0 || k > ST_KMAX || k > N) return JMAC_EINVAL;
    if (d > 512) return JMAC_EDIM;
    if (B == 0) return JMAC_OK;
    if (!val || !idx) return JMAC_EINVAL;
    if (B >= INT32_MAX || N >= INT32_MAX) return JMAC_ERANGE;
    LinkEnsArgs e{};
    bool vec;
    if (int rc = ens_args(e, vec, members, n_members, n_layers, h, r, pred_head, index, B, N, d)) return rc;
    if (!ws || ws_bytes < jmac_linkpred_ens_topk_workspace_bytes(B, N, d, n_layers, n_members, k)) return JMAC_EWORKSPACE;
    LinkRankArgs& a = e.base;
    size_t shm;                                                // unused: RANK = false stages nothing
    if (!prep_lds(a, shm)) return JMAC_ERANGE;                 // jmac_linkpred_rank_*'s LDS limit
    const LeWs w = le_layout(B, d, n_layers, n_members);
    const LtWs t = lt_layout(B, N, d, 0, k);
    char* wb = (char*)ws;
    a.er = wb + w.er;
    e.hq = (int32_t*)(wb + w.hq);
    a.rng = (int2*)(wb + w.end + t.rng);
    if (index) hipLaunchKernelGGL((link_ens_prep_kernel<true, false>), dim3((unsigned)B), dim3(kBlock), 0, st, e);
    else hipLaunchKernelGGL((link_ens_prep_kernel<false, false>), dim3((unsigned)B), dim3(kBlock), 0, st, e);
    auto filter_args = [&](const SimFilter& f) {
        LinkEnsArgs x = e;
        x.base = link_filter_args(e.base, f);
        return x;
    };
    return topk_drive(B, N, k, val, idx, wb + w.end + t.tail, t.ld_narrow, st,
        [&](float* S, int64_t ldS, int64_t n) -> int {
            LinkEnsArgs x = e;
            x.base.N = (int32_t)n; x.base.S = S; x.base.ldS = ldS; x.base.n_off = 0;
            launch_ens_tile<LR_STORE>(x, vec, n, st);
            if (index) hipLaunchKernelGGL(link_mask_kernel, dim3((unsigned)B), dim3(kBlock), 0, st, S, ldS, (int)n, a.rng, a.filt_idx);
            return 0;
        },
        [&](const SimFilter& f) -> int {
            launch_ens_tile<LR_FILTER>(filter_args(f), vec, N - f.n_off, st);
            return 0;
        },
        [&](const SimFilter& f, const float* val0, const int32_t* idx0) {
            hipLaunchKernelGGL(link_ens_select_kernel, dim3((unsigned)B), dim3(kBlock), 0, st, filter_args(f), (int)k, val0, idx0, val, idx);
        },
        link_topk_finish_kernel);
}

size_t jmac_linkpred_ens_stats_workspace_bytes(int64_t B, int64_t N, int64_t d, int32_t n_layers, int32_t n_members) {
    if (B < 0 || N <= 0 || d <= 0 || n_layers <= 0 || n_members <= 0) return 0;
    return ls_layout(jmac_linkpred_ens_rank_workspace_bytes(B, d, n_layers, n_members) - 256, B, N).total;
}

// jmac_linkpred_stats_f32 on the folded D: the ensemble's prep and tile kernels, the same epilogue, merge and finish
int jmac_linkpred_ens_stats_f32(const jmac_link_member_t* members, int32_t n_members, int32_t n_layers, const int32_t* h, const int32_t* r,
                                int32_t pred_head, const int32_t* gold, const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d,
                                float scale, int32_t* near, float* dmin, float* sum, float* ent, float* logp_gold, void* ws,
                                size_t ws_bytes, jmac_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    if (B < 0 || N <= 0 || d <= 0 || n_layers <= 0 || n_layers > LR_MAX_LAYERS || n_members < 1 || n_members > LE_MAX) return JMAC_EINVAL;
    if (!(scale > 0.f) || !std::isfinite(scale)) return JMAC_EINVAL;
    if (int rc = link_stats_check(gold, near, dmin, sum, ent, logp_gold)) return rc;
    if (B == 0) return JMAC_OK;
    if (B >= INT32_MAX || N >= INT32_MAX || d > 512) return JMAC_ERANGE;
    LinkEnsArgs e{};
    bool vec;
    if (int rc = ens_args(e, vec, members, n_members, n_layers, h, r, pred_head, index, B, N, d)) return rc;
    if (!ws || ws_bytes < jmac_linkpred_ens_stats_workspace_bytes(B, N, d, n_layers, n_members)) return JMAC_EWORKSPACE;
    LinkRankArgs& a = e.base;
    const LeWs lw = le_layout(B, d, n_layers, n_members);
    const LsWs w = ls_layout(jmac_linkpred_ens_rank_workspace_bytes(B, d, n_layers, n_members) - 256, B, N);
    char* wb = (char*)ws;
    a.gold = gold;
    a.er = wb + lw.er;
    e.hq = (int32_t*)(wb + lw.hq);
    a.gs = (float*)(wb + lw.end);                              // (jmac_linkpred_ens_rank_f32's layout)
    a.rank = (int32_t*)(wb + w.rank);
    a.rng = (int2*)(wb + w.rng);
    a.S = (float*)(wb + w.part);
    a.scale = scale;
    size_t shm;
    if (!prep_lds(a, shm)) return JMAC_ERANGE;
    const dim3 grid((unsigned)B), block(kBlock);
    if (gold && index) hipLaunchKernelGGL((link_ens_prep_kernel<true, true, true>), grid, block, shm, st, e);
    else if (gold) hipLaunchKernelGGL((link_ens_prep_kernel<false, true, true>), grid, block, shm, st, e);
    else if (index) hipLaunchKernelGGL((link_ens_prep_kernel<true, false>), grid, block, 0, st, e);
    else hipLaunchKernelGGL((link_ens_prep_kernel<false, false>), grid, block, 0, st, e);
    launch_ens_tile<LR_STATS>(e, vec, N, st);
    return link_stats_finish(a, w, wb, near, dmin, sum, ent, logp_gold, st);
}

size_t jmac_softmax_entropy_workspace_bytes(int64_t n1, int64_t n2) {
    if (n1 < 0 || n2 < 0) return 0;
    return align_up((size_t)n1 * (size_t)n2 * 4) + jmac_col_softmax_workspace_bytes(n1, n2) + 256;
}

int jmac_softmax_entropy_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d,
                             float scale, float* ent_rows, float* ent_cols, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    if (n1 < 0 || n2 < 0 || d <= 0) return JMAC_EINVAL;
    if (n1 == 0 || n2 == 0) return JMAC_OK;
    if (!A || !B || !ent_rows || !ent_cols) return JMAC_EINVAL;
    if (lda % 4 || ldb % 4) return JMAC_EDIM;
    if (!ws || ws_bytes < jmac_softmax_entropy_workspace_bytes(n1, n2)) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    // ONE GEMM: the column entropies come from a column-wise pass over the same row-major S (the reference's
    // softmax(simi.t()) of train.py:245 reads the transpose of the same matrix, not a second product)
    float* S = (float*)ws;
    const size_t soff = align_up((size_t)n1 * (size_t)n2 * 4);
    if (int rc = launch_sim<SG_STORE>(A, lda, B, ldb, n1, n2, d, S, n2, SimStore{}, st)) return rc;
    hipLaunchKernelGGL(row_entropy_kernel, dim3((unsigned)n1), dim3(kBlock), 0, st, S, n2, (int)n2, scale, ent_rows);
    return jmac_col_softmax_f32(S, n2, n1, n2, nullptr, nullptr, 0.f, scale, nullptr, 0, ent_cols, (char*)ws + soff,
                                ws_bytes - soff, stream);
}

size_t jmac_sim_softmax_stats_workspace_bytes(int64_t n1, int64_t n2) {
    if (n1 < 0 || n2 < 0) return 0;
    return ss_layout(n1, n2).total;
}

int jmac_sim_softmax_stats_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d, float scale,
                               float* row_max, int32_t* row_arg, float* row_sum, float* row_ent, float* col_max, int32_t* col_arg,
                               float* col_sum, float* col_ent, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    if (n1 < 0 || n2 < 0 || d <= 0 || !(scale > 0.f)) return JMAC_EINVAL;
    if (n1 == 0 || n2 == 0) return JMAC_OK;
    const bool want_rows = row_max || row_arg || row_sum || row_ent, want_cols = col_max || col_arg || col_sum || col_ent;
    if (!A || !B || !(want_rows || want_cols)) return JMAC_EINVAL;
    if (lda % 4 || ldb % 4) return JMAC_EDIM;
    if (n1 >= INT32_MAX || n2 >= INT32_MAX) return JMAC_ERANGE;
    if (!ws || ws_bytes < jmac_sim_softmax_stats_workspace_bytes(n1, n2)) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const SsWs w = ss_layout(n1, n2);
    SimStats sx{};
    sx.rpart = (float4*)((char*)ws + w.rpart);
    sx.cpart = want_cols ? (float*)((char*)ws + w.cpart) : nullptr;
    sx.cbest = (float2*)((char*)ws + w.cbest);
    sx.scale = scale;
    if (int rc = launch_sim<SG_STATS>(A, lda, B, ldb, n1, n2, d, nullptr, 0, sx, st)) return rc;
    const int rb = want_rows ? (int)((n1 + 63) / 64) : 0, cb = want_cols ? (int)((n2 + 63) / 64) : 0;
    hipLaunchKernelGGL(sim_stats_merge_kernel, dim3((unsigned)(rb + cb)), dim3(kBlock), 0, st, sx.rpart, sx.cpart, sx.cbest, (int)n1,
                       (int)n2, scale, rb, row_max, row_arg, row_sum, row_ent, col_max, col_arg, col_sum, col_ent);
    return (int)hipGetLastError();
}

size_t jmac_sim_lse_workspace_bytes(int64_t n1, int64_t n2) {
    if (n1 < 0 || n2 < 0) return 0;
    return sl_layout(n1, n2).total;
}

int jmac_sim_lse_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d, float scale,
                     const float* col_add, const float* row_add, float row_shift, float col_shift, float* row_out, float* col_out,
                     void* ws, size_t ws_bytes, jmac_stream_t stream) {
    if (n1 < 0 || n2 < 0 || d <= 0 || !(scale > 0.f)) return JMAC_EINVAL;
    if (n1 == 0 || n2 == 0) return JMAC_OK;
    if (!A || !B || !(row_out || col_out)) return JMAC_EINVAL;
    if (lda % 4 || ldb % 4 || d % 4) return JMAC_EDIM;
    if (n1 >= INT32_MAX || n2 >= INT32_MAX) return JMAC_ERANGE;
    if (!ws || ws_bytes < jmac_sim_lse_workspace_bytes(n1, n2)) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const SlWs w = sl_layout(n1, n2);
    SimLse lx{};
    lx.rpart = row_out ? (float2*)((char*)ws + w.rpart) : nullptr;
    lx.cpart = col_out ? (float2*)((char*)ws + w.cpart) : nullptr;
    lx.col_add = col_add;
    lx.row_add = row_add;
    lx.scale = scale;
    if (int rc = launch_sim<SG_LSE>(A, lda, B, ldb, n1, n2, d, nullptr, 0, lx, st)) return rc;
    const int rb = row_out ? (int)((n1 + 63) / 64) : 0, cb = col_out ? (int)((n2 + 63) / 64) : 0;
    hipLaunchKernelGGL(sim_lse_merge_kernel, dim3((unsigned)(rb + cb)), dim3(kBlock), 0, st, lx.rpart, lx.cpart, (int)n1, (int)n2, rb,
                       row_shift, col_shift, row_out, col_out);
    return (int)hipGetLastError();
}

int jmac_csls_apply_f32(const float* S, int64_t lds, int64_t n1, int64_t n2, const float* r1, const float* r2, float* out,
                        int64_t ldo, jmac_stream_t stream) {
    if (n1 < 0 || n2 < 0) return JMAC_EINVAL;
    if (n1 == 0 || n2 == 0) return JMAC_OK;
    if (!S || !r1 || !r2 || !out) return JMAC_EINVAL;
    int64_t blocks = (n1 * n2 + kBlock - 1) / kBlock;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(csls_apply_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, S, lds, n1, n2, r1, r2, out,
                       ldo);
    return (int)hipGetLastError();
}

int jmac_row_softmax_f32(const float* S, int64_t lds, int64_t n1, int64_t n2, const uint8_t* row_mask,
                         const uint8_t* col_mask, float fill, float scale, float* out, int64_t ldo, float* ent,
                         jmac_stream_t stream) {
    if (n1 < 0 || n2 <= 0) return JMAC_EINVAL;
    if (n1 == 0) return JMAC_OK;
    if (!S || (!out && !ent)) return JMAC_EINVAL;
    if (n2 >= INT32_MAX) return JMAC_ERANGE;
    hipLaunchKernelGGL(masked_row_softmax_kernel, dim3((unsigned)n1), dim3(kBlock), 0, (hipStream_t)stream, S, lds, (int)n2,
                       row_mask, col_mask, fill, scale, out, ldo, ent);
    return (int)hipGetLastError();
}

static int col_softmax_row_splits(int64_t n1, int64_t n2) {
    const int64_t strips = (n2 + 63) / 64;
    int64_t rs = (2048 + strips - 1) / strips;            // ~2k blocks
    const int64_t max_rs = (n1 + 63) / 64;                // at least 64 rows per block
    if (rs > max_rs) rs = max_rs;
    if (rs < 1) rs = 1;
    return (int)rs;
}

size_t jmac_col_softmax_workspace_bytes(int64_t n1, int64_t n2) {
    if (n1 < 0 || n2 < 0) return 0;
    return align_up((size_t)col_softmax_row_splits(n1, n2) * (kBlock / 64) * (size_t)n2 * 12) + 2 * align_up((size_t)n2 * 4) + 256;
}

int jmac_col_softmax_f32(const float* S, int64_t lds, int64_t n1, int64_t n2, const uint8_t* row_mask,
                         const uint8_t* col_mask, float fill, float scale, float* out_t, int64_t ldo, float* ent,
                         void* ws, size_t ws_bytes, jmac_stream_t stream) {
    if (n1 <= 0 || n2 < 0) return JMAC_EINVAL;
    if (n2 == 0) return JMAC_OK;
    if (!S || (!out_t && !ent)) return JMAC_EINVAL;
    if (n1 >= INT32_MAX || n2 >= INT32_MAX) return JMAC_ERANGE;
    if (!ws || ws_bytes < jmac_col_softmax_workspace_bytes(n1, n2)) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int rs = col_softmax_row_splits(n1, n2);
    const int parts = rs * (kBlock / 64);
    float* part = (float*)ws;
    float* cmax = (float*)((char*)ws + align_up((size_t)parts * (size_t)n2 * 12));
    float* cinv = (float*)((char*)cmax + align_up((size_t)n2 * 4));
    hipLaunchKernelGGL(col_softmax_stats_kernel, dim3((unsigned)((n2 + 63) / 64), (unsigned)rs), dim3(kBlock), 0, st, S, lds,
                       (int)n1, (int)n2, row_mask, col_mask, fill, scale, part);
    hipLaunchKernelGGL(col_softmax_merge_kernel, dim3((unsigned)((n2 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, part, parts,
                       (int)n2, cmax, cinv, ent);
    if (out_t)
        hipLaunchKernelGGL(col_softmax_apply_kernel, dim3((unsigned)((n2 + 63) / 64), (unsigned)((n1 + 63) / 64)), dim3(kBlock), 0, st,
                           S, lds, (int)n1, (int)n2, row_mask, col_mask, fill, scale, cmax, cinv, out_t, ldo);
    return (int)hipGetLastError();
}

static int col_topk_row_splits(int64_t n1, int64_t n2) {
    const int64_t strips = (n2 + 63) / 64;
    int64_t rs = (2048 + strips - 1) / strips;            // ~2k blocks
    const int64_t max_rs = (n1 + 63) / 64;                // at least 64 rows per block
    if (rs > max_rs) rs = max_rs;
    if (rs < 1) rs = 1;
    return (int)rs;
}

size_t jmac_col_topk_workspace_bytes(int64_t n1, int64_t n2, int32_t k) {
    if (n1 < 0 || n2 < 0 || k <= 0) return 0;
    return align_up((size_t)col_topk_row_splits(n1, n2) * (kBlock / 64) * (size_t)n2 * (size_t)k * 4) + 256;
}

int jmac_col_topk_f32(const float* S, int64_t lds, int64_t n1, int64_t n2, int32_t k, float* val, void* ws, size_t ws_bytes,
                      jmac_stream_t stream) {
    if (n1 <= 0 || n2 <= 0 || k <= 0 || k > n1) return JMAC_EINVAL;
    if (k > CT_KMAX) return JMAC_EDIM;
    if (!S || !val) return JMAC_EINVAL;
    if (n1 >= INT32_MAX || n2 >= INT32_MAX) return JMAC_ERANGE;
    if (!ws || ws_bytes < jmac_col_topk_workspace_bytes(n1, n2, k)) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int rs = col_topk_row_splits(n1, n2);
    float* cand = (float*)ws;
    hipLaunchKernelGGL(col_topk_partial_kernel, dim3((unsigned)((n2 + 63) / 64), (unsigned)rs), dim3(kBlock), 0, st, S, lds, (int)n1,
                       (int)n2, (int)k, cand);
    hipLaunchKernelGGL(col_topk_merge_kernel, dim3((unsigned)((n2 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, cand,
                       rs * (kBlock / 64), (int)n2, (int)k, val);
    return (int)hipGetLastError();
}

int jmac_csls_rank_f32(const float* S, int64_t lds, int64_t n1, int64_t n2, const float* r1, const float* r2, const int32_t* gold,
                       int32_t* rank, jmac_stream_t stream) {
    if (n1 < 0 || n2 <= 0) return JMAC_EINVAL;
    if (n1 == 0) return JMAC_OK;
    if (!S || !r1 || !r2 || !gold || !rank) return JMAC_EINVAL;
    if (n2 >= INT32_MAX) return JMAC_ERANGE;
    hipLaunchKernelGGL(csls_rank_kernel, dim3((unsigned)n1), dim3(kBlock), 0, (hipStream_t)stream, S, lds, (int)n2, r1, r2, gold, rank);
    return (int)hipGetLastError();
}

size_t jmac_sim_csls_rank_workspace_bytes(int64_t n1, int64_t n2) {
    if (n1 < 0 || n2 < 0) return 0;
    return align_up((size_t)n1 * 4) + 256;                   // the rows' gold values: nothing grows with n2
}

size_t jmac_sim_csls_topk_workspace_bytes(int64_t L, int64_t N, int32_t k) {
    return jmac_sim_topk_workspace_bytes(L, N, k);            // the same layout: r1 / r2 are the caller's
}

}  // extern "C"

// ---- alignment top-k and ranks: the similarity product (cosine, inner) or the L1 tile loop (Manhattan) as the source ----------------
// Manhattan: s = 1 - dist(A_m, B_n) (similarity.py:47-49), c = csls_value(s, r1, r2) or s; the tile kernel reads its query rows straight
// from A (one layer, er = A), so dist carries jmac_l1_score_f32's bits.
static bool l1_align_args(LinkRankArgs& a, const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N, int64_t d,
                          const float* r1, const float* r2) {
    a.nl = 1; a.B = (int32_t)L; a.N = (int32_t)N; a.d = (int32_t)d; a.dq = (int32_t)lda;
    a.er = const_cast<float*>(A);
    a.tab[0] = B; a.ld_tab[0] = ldb;
    a.r1 = r1; a.r2 = r2;
    return d % 4 == 0 && (((uintptr_t)A | (uintptr_t)B) % (4 * sizeof(float))) == 0;      // the vector form's loads (lda, ldb % 4 == 0)
}

static int l1_topk_impl(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N, int64_t d, const float* r1,
                        const float* r2, int32_t k, float* val, int32_t* idx, void* ws, hipStream_t st, const int32_t* row_id,
                        const unsigned long long* best) {
    LinkRankArgs a{};
    const bool vec = l1_align_args(a, A, lda, B, ldb, L, N, d, r1, r2);
    a.row_id = row_id; a.best = best;
    const dim3 rows((unsigned)L), block(kBlock);
    return topk_drive(L, N, k, val, idx, (char*)ws, N, st,
        [&](float* S, int64_t ldS, int64_t n) -> int {       // the tile kernel's -dist slab, rescored (and masked) in place
            launch_link_store<float>(a, vec, S, ldS, n, st);
            hipLaunchKernelGGL(l1_csls_inplace_kernel, rows, block, 0, st, S, ldS, (int)n, r1, r2, row_id, best);
            return 0;
        },
        [&](const SimFilter& f) -> int {
            if (best) launch_link_tile<float, LR_CSLS_VIABLE>(link_filter_args(a, f), vec, N - f.n_off, st);
            else launch_link_tile<float, LR_CSLS_FILTER>(link_filter_args(a, f), vec, N - f.n_off, st);
            return 0;
        },
        [&](const SimFilter& f, const float* val0, const int32_t* idx0) {
            if (best)
                hipLaunchKernelGGL(cand_select_viable_kernel<true>, rows, block, 0, st, A, lda, B, ldb, (int)N, (int)d, (int)k, f.cnt, f.cval,
                                   f.cidx, f.cap, val0, idx0, val, idx, r1, r2, row_id, best);
            else
                hipLaunchKernelGGL((cand_select_kernel<false, true>), rows, block, 0, st, A, lda, B, ldb, (int)N, (int)d, (int)k, f.cnt, f.cval,
                                   f.cidx, f.cap, val0, idx0, val, idx, r1, r2);
        },
        best ? viable_topk_finish_kernel : nullptr);
}

// jmac_{sim,l1}_csls_topk{,_viable}_f32: one argument check, then the source.  ALIGN_L1: the Manhattan forms take any d and need lda
// to be the tile kernel's int32 row stride; TOPK_VIABLE: row_id and best are arguments; val may be NULL in the plain similarity form only.
enum AlignMetric { ALIGN_SIM, ALIGN_L1 };
enum TopkForm { TOPK_PLAIN, TOPK_VIABLE };
static int csls_topk_entry(AlignMetric metric, TopkForm form, const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N, int64_t d,
                           const float* r1, const float* r2, const int32_t* row_id, const uint64_t* best, int32_t k, float* val,
                           int32_t* idx, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    if (L < 0 || N <= 0 || d <= 0 || k <= 0 || k > N || k > ST_KMAX || (r1 == nullptr) != (r2 == nullptr)) return JMAC_EINVAL;
    if (L == 0) return JMAC_OK;
    const bool l1 = metric == ALIGN_L1, viable = form == TOPK_VIABLE;
    if (!A || !B || !idx || (!val && (l1 || viable)) || (viable && (!row_id || !best))) return JMAC_EINVAL;
    if (lda % 4 || ldb % 4 || (!l1 && d % 4)) return JMAC_EDIM;
    if (L >= INT32_MAX || N >= INT32_MAX || (l1 && lda >= INT32_MAX)) return JMAC_ERANGE;
    if (!ws || ws_bytes < (l1 ? jmac_l1_csls_topk_workspace_bytes(L, N, d, k) : jmac_sim_csls_topk_workspace_bytes(L, N, k))) return JMAC_EWORKSPACE;
    const auto* words = reinterpret_cast<const unsigned long long*>(best);
    return l1 ? l1_topk_impl(A, lda, B, ldb, L, N, d, r1, r2, k, val, idx, ws, (hipStream_t)stream, row_id, words)
              : sim_topk_impl(A, lda, B, ldb, L, N, d, r1, r2, k, val, idx, ws, (hipStream_t)stream, row_id, words);     // r1 == NULL: c = S
}

// jmac_{sim,l1}_csls_rank_f32: the same for the ranks -- the gold values, then the count epilogue over all columns
static int csls_rank_entry(AlignMetric metric, const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d,
                           const float* r1, const float* r2, const int32_t* gold, int32_t* rank, void* ws, size_t ws_bytes,
                           jmac_stream_t stream) {
    if (n1 < 0 || n2 <= 0 || d <= 0 || (r1 == nullptr) != (r2 == nullptr)) return JMAC_EINVAL;
    if (n1 == 0) return JMAC_OK;
    const bool l1 = metric == ALIGN_L1;
    if (!A || !B || !gold || !rank) return JMAC_EINVAL;
    if (lda % 4 || ldb % 4 || (!l1 && d % 4)) return JMAC_EDIM;
    if (n1 >= INT32_MAX || n2 >= INT32_MAX || (l1 && lda >= INT32_MAX)) return JMAC_ERANGE;
    if (!ws || ws_bytes < (l1 ? jmac_l1_csls_rank_workspace_bytes(n1, n2) : jmac_sim_csls_rank_workspace_bytes(n1, n2))) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (!l1) {
        SimCsls cx{};
        cx.r1 = r1; cx.r2 = r2; cx.gval = (float*)ws; cx.gold = gold; cx.rank = rank;
        hipLaunchKernelGGL(csls_gold_kernel, dim3((unsigned)((n1 + 32 * (kBlock / 64) - 1) / (32 * (kBlock / 64)))), dim3(kBlock), 0, st, A, lda,
                           B, ldb, (int)n1, (int)d, r1, r2, gold, (float*)ws, rank);
        return launch_sim<SG_CSLS_COUNT>(A, lda, B, ldb, n1, n2, d, nullptr, 0, cx, st);
    }
    LinkRankArgs a{};
    const bool vec = l1_align_args(a, A, lda, B, ldb, n1, n2, d, r1, r2);
    a.gs = (float*)ws; a.gold = gold; a.rank = rank;
    hipLaunchKernelGGL(l1_csls_gold_kernel, dim3((unsigned)((n1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, A, lda, B, ldb, (int)n1, (int)d,
                       r1, r2, gold, a.gs, rank);
    launch_link_tile<float, LR_CSLS_COUNT>(a, vec, n2, st);
    return (int)hipGetLastError();
}

extern "C" {

int jmac_sim_csls_rank_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d, const float* r1,
                           const float* r2, const int32_t* gold, int32_t* rank, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    return csls_rank_entry(ALIGN_SIM, A, lda, B, ldb, n1, n2, d, r1, r2, gold, rank, ws, ws_bytes, stream);
}

int jmac_sim_csls_topk_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N, int64_t d, const float* r1,
                           const float* r2, int32_t k, float* val, int32_t* idx, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    return csls_topk_entry(ALIGN_SIM, TOPK_PLAIN, A, lda, B, ldb, L, N, d, r1, r2, nullptr, nullptr, k, val, idx, ws, ws_bytes, stream);
}

int jmac_sim_csls_topk_viable_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N, int64_t d, const float* r1,
                                  const float* r2, const int32_t* row_id, const uint64_t* best, int32_t k, float* val, int32_t* idx,
                                  void* ws, size_t ws_bytes, jmac_stream_t stream) {
    return csls_topk_entry(ALIGN_SIM, TOPK_VIABLE, A, lda, B, ldb, L, N, d, r1, r2, row_id, best, k, val, idx, ws, ws_bytes, stream);
}

size_t jmac_l1_csls_topk_workspace_bytes(int64_t L, int64_t N, int64_t d, int32_t k) {
    if (d <= 0) return 0;
    return jmac_sim_topk_workspace_bytes(L, N, k);            // the same layout: the query rows are A's own, nothing grows with d
}

int jmac_l1_csls_topk_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N, int64_t d, const float* r1,
                          const float* r2, int32_t k, float* val, int32_t* idx, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    return csls_topk_entry(ALIGN_L1, TOPK_PLAIN, A, lda, B, ldb, L, N, d, r1, r2, nullptr, nullptr, k, val, idx, ws, ws_bytes, stream);
}

int jmac_l1_csls_topk_viable_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N, int64_t d, const float* r1,
                                 const float* r2, const int32_t* row_id, const uint64_t* best, int32_t k, float* val, int32_t* idx,
                                 void* ws, size_t ws_bytes, jmac_stream_t stream) {
    return csls_topk_entry(ALIGN_L1, TOPK_VIABLE, A, lda, B, ldb, L, N, d, r1, r2, row_id, best, k, val, idx, ws, ws_bytes, stream);
}

size_t jmac_l1_csls_rank_workspace_bytes(int64_t n1, int64_t n2) {
    return jmac_sim_csls_rank_workspace_bytes(n1, n2);        // the rows' gold values
}

int jmac_l1_csls_rank_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d, const float* r1,
                          const float* r2, const int32_t* gold, int32_t* rank, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    return csls_rank_entry(ALIGN_L1, A, lda, B, ldb, n1, n2, d, r1, r2, gold, rank, ws, ws_bytes, stream);
}

}  // extern "C"
