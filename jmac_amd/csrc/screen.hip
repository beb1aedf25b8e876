// screen.hip -- jmac_sim_topk_screened_f32: jmac_sim_topk_f32's result, bit for bit, with the L x N x d work done on the bf16
// matrix cores (v_mfma_f32_32x32x16_bf16) and only a few dozen columns per row on the fp32-input MFMA.
//
// The bf16 product never decides anything by itself.  Its score sh(i, j) of a pair -- both operands rounded once to bf16, fp32
// accumulate -- differs from the fp32 product's score s(i, j) by at most
//      e(i, j) = KAPPA (na_i + TAU) (nb_j + TAU) + ETA                                         (the proof)
// with na, nb upper bounds of the rows' l2 norms.  So sh - e <= s <= sh + e, and
//   prepare   bf16 copies of A and B (rows zero-padded to 32 k) and the two factors of e per row          screen_prepare_kernel
//   sample    sh - e over the first Ns columns, stored; its k-th largest per row is lower_i <= the row's exact k-th best score
//                                                                            screen_gemm_kernel<false>, jmac_row_topk_f32
//   filter    the bf16 product over ALL N columns; (sh, j) joins row i's list unless sh + e < lower_i: every member of the exact
//             top-k, ties included, is listed (slots claimed with integer atomics, one per row and flush)  screen_gemm_kernel<true>
//   select    per row: lower'_i = the k-th largest sh - e of the list (>= lower_i); the entries with sh + e >= lower'_i are rescored
//             with the fp32 product's own instruction sequence (sim_rescore.h), the k best of those exact scores are the answer;
//                                                                                                          screen_select_kernel
//             a row whose list overflowed recomputes all N scores (for_each_row_score + tk_select_recomputed)  screen_overflow_kernel
// Comparisons are written !(x < y): a NaN passes and is then rescored exactly.  No float atomics; list order varies between runs,
// the selection (a sort of (score, index) words) does not depend on it.
//
// jmac_sim_csls_topk_screened_f32 / jmac_sim_csls_topk_viable_screened_f32: the same stages deciding on the alignment value
// c = csls_value(s, r1, r2).  For finite r1, r2 that is a non-decreasing function of s with its own roundings included (2 s is exact,
// each subtraction rounds once, rounding is monotone), so with lo = fl(sh - e) <= s <= fl(sh + e) = hi
//      c_lo = csls_value(lo, r1, r2) <= c <= csls_value(hi, r1, r2) = c_hi
// and c_lo / c_hi take the places of sh - e / sh + e in all three decisions (the lists still hold sh: the select stage recomputes
// both bounds).  The viable predicate tk_pack(c, row_id) > best[j] is monotone in c too: tk_pack(c_lo, id) > best[j] is "certainly
// viable", !(tk_pack(c_hi, id) > best[j]) "certainly not".  Only certainly viable columns may raise a threshold, only certainly
// non-viable ones are dropped unseen; the exact predicate runs on the rescored value (ScMode, ScreenAlign below).
//
// jmac_sim_csls_rank_screened_f32: rank_i = 1 + #{j : before(c(i, j), j)} with before(c, j) := c > g || (c == g && j < G), g the gold
// value of row i (the fp32 product's bits, csls_gold_body) and G its column.  before is monotone in c, so with c_lo <= c <= c_hi
//   certainly before    before(c_lo, j): counted in the bf16 product's epilogue (ballots, popcounts, integer atomics), never rescored
//   certainly not       c_hi < g || (c_hi == g && j > G): dropped
//   everything else     g lies in [c_lo, c_hi]: the column joins the row's list (the gold column always does: n_rescored >= 1) and
//                       screen_rank_resolve_kernel puts its rescored c to the exact predicate.
// No sample stage: the threshold is g, known before the product starts.  A non-finite sh or e decides nothing (the column is listed).
// A row with more than RK_CAP undecided columns is recounted densely -- by the entry (finish != 0) or by the caller.
#include "common.h"
#include "sim_rescore.h"
#include "topk_select.h"

using namespace jmac;

namespace {

constexpr int kBlock = 256;
static_assert(TK_THREADS == kBlock, "the selection routines stride by the block size");

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));        // 16 staged bytes (a native vector: stays in registers)

constexpr int SC_T = 128;                   // 128 x 128 outputs per 4-wave block, waves 2 x 2, 64 x 64 each
constexpr int SC_BK = 32;                   // k slab: two MFMA k-steps of 16
constexpr int SC_ROWB = 2 * SC_BK;          // bytes per LDS row
constexpr int SC_IMG = SC_T * SC_ROWB;      // one operand slab: 8 KB
constexpr int SC_FL_CAP = 512;              // entries of a wave's LDS list
constexpr int SC_FL_ROOM = 192;             // flush when a list has less room than this at a tile's end (a typical tile adds ~60)
constexpr int SC_STRIP_MAX = 64;            // tiles per strip at most: a column's offset in its strip fits 16 bits
constexpr int SC_CAP = TK_CAP;              // list entries per row
// list entries per row of the ranks.  A listed column costs about 32 dense ones (sim_row_tile_grouped uses one row of a 32 x 32 tile),
// so a row with more than ~N / 32 undecided columns is cheaper on the dense product: 256 at the narrowest screened width, ~940 at
// N = 30000; 512 lies between (profiles/rank_screen_timing.txt has 256 and 1024 next to it).  tests/screen_rank_ref.py restates it.
constexpr int RK_CAP = 512;
constexpr int SC_KMAX = 64;
constexpr int64_t SC_MIN_N = 8192;
constexpr int64_t SC_DMAX = 512;

// the bound's constants: KAPPA >= 2u + u^2 + 2 (d + 2) 2^-23 (1 + u)^2 for d <= 512 (0.0079513: u = 2^-8, the
// accumulation counted at one ulp per operation) with 0.6 % to spare for the bound's own roundings; TAU and ETA cover what
// underflows or is flushed on either path.  The prepare pass writes
// ka_i = KAPPA (na_i + TAU) for A's rows and nbt_j = nb_j + TAU for B's: e is ONE fma per element, the same one in every kernel.
constexpr float SC_KAPPA = 0.008f, SC_TAU = 0x1p-110f, SC_ETA = 0x1p-110f;
__device__ __forceinline__ float screen_err(float ka, float nbt) { return __fmaf_rn(ka, nbt, SC_ETA); }

// what a kernel decides on: the score itself (jmac_sim_topk_screened_f32), c = csls_value(s, r1, r2), or c over the viable columns
// only -- there the rescoring is decided at run time (r1 == NULL: c = s), as in score.hip's viable forms
// -- or, SC_RANK (jmac_sim_csls_rank_screened_f32), the count of the columns that come before a row's gold column
enum ScMode { SC_PLAIN, SC_CSLS, SC_VIABLE, SC_RANK };
struct ScreenAlign {
    const float* r1;                    // [M]
    const float* r2;                    // [N]
    const int32_t* row_id;              // SC_VIABLE: [M] the suitor a row stands for (the predicate's tie-break)
    const unsigned long long* best;     // SC_VIABLE: [N] the reviewers' words
    const int32_t* gold;                // SC_RANK: [M] the gold column G (its value g is the epilogue's tau)
    int32_t* rank;                      // SC_RANK: [M], preset to 1: the certain counts are added to it
};
template <int MODE>
__device__ __forceinline__ float sc_value(float s, float r1v, float r2v, bool cs) {
    if constexpr (MODE == SC_PLAIN) return s;
    else if constexpr (MODE == SC_CSLS) return csls_value(s, r1v, r2v);
    else return cs ? csls_value(s, r1v, r2v) : s;
}

static inline bool sc_fused(int64_t N, int64_t k) { return N >= SC_MIN_N && k <= SC_KMAX; }
// jmac_sim_csls_topk_viable_screened_f32 -- the matching runs' refill, a handful of gathered rows against the whole table -- screens
// calls of at least this many rows.  Every call pays the bf16 copy of all of B; measured at 30000 x 300 against the fp32 entry
// (profiles/align_screen_timing.txt): 1 row 0.095 / 0.084 ms, 32 rows 0.099 / 0.093 (the screen loses), 256 rows
// 0.108 / 0.120, 2048 rows 0.278 / 0.475 (it wins): the smallest measured count at which it wins.
constexpr int64_t SC_VIABLE_MIN_ROWS = 256;
static inline bool sc_fused_viable(int64_t L, int64_t N, int64_t k) { return sc_fused(N, k) && L >= SC_VIABLE_MIN_ROWS; }
static inline int64_t sc_dp(int64_t d) { return (d + SC_BK - 1) / SC_BK * SC_BK; }
// the sample: an eighth of the columns (the fp32 path takes a twelfth: the product is cheap here, and a larger sample is a tighter
// lower_i, hence shorter lists)
static inline int64_t sc_sample(int64_t N) {
    const int64_t ns = N / 8 > 2048 ? N / 8 : 2048;
    return (ns + 127) / 128 * 128;
}
struct ScWs { size_t ab, bb, na, nb, S, val0, idx0, cnt, cval, cidx, total; };
static ScWs sc_layout(int64_t L, int64_t N, int64_t d, int64_t k) {
    ScWs w{};
    size_t off = 0;
    w.ab = off;   off += align_up((size_t)L * (size_t)sc_dp(d) * 2);
    w.bb = off;   off += align_up((size_t)N * (size_t)sc_dp(d) * 2);
    w.na = off;   off += align_up((size_t)L * 4);
    w.nb = off;   off += align_up((size_t)N * 4);
    w.S = off;    off += align_up((size_t)L * (size_t)sc_sample(N) * 4);
    w.val0 = off; off += align_up((size_t)L * (size_t)k * 4);
    w.idx0 = off; off += align_up((size_t)L * (size_t)k * 4);
    w.cnt = off;  off += align_up((size_t)L * 4);
    w.cval = off; off += align_up((size_t)L * SC_CAP * 4);
    w.cidx = off; off += align_up((size_t)L * SC_CAP * 4);
    w.total = off + 256;
    return w;
}

// ---- prepare: one wave per row: the row rounded to bf16 (nearest even), zero-padded to dp; norm[row] = scale (nrm + TAU) with
// nrm >= ||row||_2 rounded up to fp32 --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void screen_prepare_kernel(const float* __restrict__ X, int64_t ldx, int rows, int d, int dp,
                                                                float scale, bf16_t* __restrict__ Xb, float* __restrict__ norm) {
    const int row = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* x = X + (int64_t)row * ldx;
    double ss = 0.0;                        // float64: the squares of the smallest fp32 rows do not underflow
    for (int c = lane * 4; c < dp; c += 256) {
        const float4 v = c < d ? ld4(x + c) : f4zero();
        bf16x2 lo, hi;
        lo.x = (__bf16)v.x;
        lo.y = (__bf16)v.y;
        hi.x = (__bf16)v.z;
        hi.y = (__bf16)v.w;
        *reinterpret_cast<uint2*>(Xb + (int64_t)row * dp + c) = make_uint2(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi));
        ss += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if (lane == 0) {
        // rounded UP to fp32: 1 + 2^-30 covers the float64 sum's and root's roundings; below the normal range the smallest normal
        const double root = sqrt(ss) * (1.0 + 0x1p-30);
        float f = (float)root;
        if ((double)f < root) f = __uint_as_float(__float_as_uint(f) + 1u);
        if (root > 0.0 && root < 0x1p-126) f = 0x1p-126f;
        norm[row] = scale * (f + SC_TAU);
    }
}

// ---- the bf16 product --------------------------------------------------------------------------------------------------------
// LDS image of one operand slab: [row][32 k] bf16, 64-byte rows; the 16-byte chunk q (k = 8q .. 8q+7) of row r sits at chunk
// q ^ ((r >> 2) & 3): the 16 rows a ds_read_b128 lane group touches cover all sixteen 4-dword bank slots (gemm3.hip's image)
__device__ __forceinline__ int sc_lds_off(int row, int chunk) { return row * SC_ROWB + ((chunk ^ ((row >> 2) & 3)) << 4); }

struct ScreenEpi {
    const float* na;         // [M] ka: KAPPA (norm bound + TAU)
    const float* nb;         // [N] nbt: norm bound + TAU
    float* C;                // store: sh - e at C[m * ldc + n]
    int64_t ldc;
    const float* tau;        // filter: lower_m = tau[m * tau_stride]
    int64_t tau_stride;
    int* cnt;                // [M] entries seen per row (may exceed cap: the row then recomputes)
    float* cval;             // [M, cap] sh
    int* cidx;               // [M, cap]
    int cap;
};

// A block owns a strip of `strip` consecutive 128 x 128 tiles of one row tile (m fastest over the blocks: those that share B tiles run
// together; A's bf16 copy stays in L2).  Operands are the prepared bf16 rows (stride dp, a multiple of 32, zero-padded: no k clamp),
// staged through registers into two LDS buffers, one barrier per slab; the next tile's first slab is requested before the epilogue.
// The accumulator of v_mfma_f32_32x32x16_bf16 has the C/D map of the fp32 32x32x2 one (col = lane & 31, row = (reg & 3) +
// 8 (reg >> 2) + 4 (lane >> 5)), so the epilogues are sim_gemm_kernel's with e folded in -- with one difference in the list form.
// There a wave claims a list slot per passing element with a returned global atomic; behind the fp32 MFMAs those hide, behind the
// bf16 ones they were half the kernel's time.  Here each wave compacts into its own LDS list across the
// strip's tiles, and at a tile's end, when a list is nearly full (and after the last tile), the block counts its entries per row
// in LDS and claims each row's slots with ONE integer atomic: ~10 x fewer.  A wave whose list is full claims slots directly.
// MODE (FILTER only): the test is on c_hi = sc_value(sh + e) and, SC_VIABLE, on its word against best[n]; the entry stays (sh, n).
// SC_RANK: tau is the row's gold value and both ends of the bound are tested -- certainly-before columns are counted (one ballot per
// accumulator register, the two rows' popcounts written into the lanes that stand for them), undecided ones take the list path, index only.
// The alignment forms' terms are a trailing ScreenAlign argument that SC_PLAIN does not have (AL is empty there: the plain
// instantiations keep the argument list, and the instructions, they had before the alignment forms existed).
__device__ __forceinline__ ScreenAlign sc_align() { return ScreenAlign{}; }
__device__ __forceinline__ const ScreenAlign& sc_align(const ScreenAlign& al) { return al; }
template <bool FILTER, int MODE = SC_PLAIN, class... AL>
__global__ __launch_bounds__(kBlock, 3) void screen_gemm_kernel(const bf16_t* __restrict__ Ab, const bf16_t* __restrict__ Bb, int dp, int M,
                                                                int N, int tiles_m, int tiles_n, int strip, ScreenEpi ext, AL... alp) {
    static_assert(sizeof...(AL) == (MODE == SC_PLAIN ? 0 : 1), "SC_CSLS and SC_VIABLE take one ScreenAlign");
    const ScreenAlign al = sc_align(alp...);
    static_assert(FILTER || MODE == SC_PLAIN, "the sample is rescored by screen_sample_align_kernel");
    __shared__ __attribute__((aligned(16))) unsigned char As[2][SC_IMG];
    __shared__ __attribute__((aligned(16))) unsigned char Bs[2][SC_IMG];
    __shared__ int fl_e[FILTER ? kBlock / 64 : 1][FILTER ? SC_FL_CAP : 1];      // (row in tile) << 16 | column in strip
    __shared__ float fl_v[FILTER ? kBlock / 64 : 1][FILTER ? SC_FL_CAP : 1];
    __shared__ int fl_count[kBlock / 64];
    __shared__ int row_cnt[FILTER ? SC_T : 1], row_base[FILTER ? SC_T : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = (int)(blockIdx.x % (unsigned)tiles_m) * SC_T;
    const int tn0 = (int)(blockIdx.x / (unsigned)tiles_m) * strip, tn1 = min(tn0 + strip, tiles_n);
    const int ns0 = tn0 * SC_T;             // the strip's first column

    // loader: 16-byte chunk f = tid + 256 i (i < 2): row = f >> 2, chunk = f & 3 (4 consecutive lanes read one 64-byte row piece);
    // unconditional at a clamped row (rows past the end re-read the last row: they feed outputs no epilogue keeps)
    auto gload = [&](const bf16_t* base, int row0, int nrows, int k0, u32x4 (&v)[2]) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f = tid + kBlock * i;
            const int row = min(row0 + (f >> 2), nrows - 1);
            v[i] = *reinterpret_cast<const u32x4*>(base + (int64_t)row * dp + k0 + 8 * (f & 3));
        }
    };
    auto sstore = [&](unsigned char* S, const u32x4 (&v)[2]) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f = tid + kBlock * i;
            *reinterpret_cast<u32x4*>(S + sc_lds_off(f >> 2, f & 3)) = v[i];
        }
    };
    // the epilogue's arguments as locals (the lambdas below capture values, not the by-value struct's address)
    const float* const na_p = ext.na;
    const float* const nb_p = ext.nb;
    float* const C = ext.C;
    const int64_t ldc = ext.ldc, tau_stride = ext.tau_stride;
    const float* const tau_p = ext.tau;
    int* const cnt = ext.cnt;
    float* const cval = ext.cval;
    int* const cidx = ext.cidx;
    const int cap = ext.cap;
    // per-row terms: lane l <-> row l of the wave's 64 rows, ONE coalesced load each, the value for accumulator register (i, reg)
    // comes out with two v_readlane (sg_epi_lists' scheme)
    const int mrow = min(m0 + wm * 64 + lane, M - 1);
    const float narow = na_p[mrow];
    float trow = 0.f;
    if constexpr (FILTER) trow = tau_p[(int64_t)mrow * tau_stride];
    // MODE: the row's r1 and id ride with narow; cs: the value is rescored at all
    bool cs = MODE == SC_CSLS;
    float r1row = 0.f;
    int ridrow = 0;
    if constexpr (MODE != SC_PLAIN) {
        if constexpr (MODE == SC_VIABLE) {
            cs = al.r1 != nullptr;
            ridrow = al.row_id[mrow];
        }
        if constexpr (MODE == SC_RANK) {                      // the gold column rides where the suitor id does
            cs = al.r1 != nullptr;
            ridrow = al.gold[mrow];
        }
        r1row = cs ? al.r1[mrow] : 0.f;
    }
    int before_row = 0;                     // SC_RANK: the certainly-before columns of row `lane` of the wave's 64, over the strip
    int fcount = 0;                         // FILTER: entries in the wave's list (wave-uniform)
    int* const fle = fl_e[FILTER ? wave : 0];
    float* const flv = fl_v[FILTER ? wave : 0];
    // FILTER, called by the whole block: the four lists -> the rows' candidate lists, one global atomic per row that has entries
    auto flush_block = [&]() {
        if (lane == 0) fl_count[wave] = fcount;
        if (tid < SC_T) row_cnt[tid] = 0;
        __syncthreads();
        for (int w = 0; w < kBlock / 64; ++w)
            for (int e = tid; e < fl_count[w]; e += kBlock) atomicAdd(&row_cnt[fl_e[w][e] >> 16], 1);
        __syncthreads();
        if (tid < SC_T) {
            const int c = row_cnt[tid];
            if (c > 0) row_base[tid] = atomicAdd(cnt + m0 + tid, c);
            row_cnt[tid] = 0;
        }
        __syncthreads();
        for (int w = 0; w < kBlock / 64; ++w)
            for (int e = tid; e < fl_count[w]; e += kBlock) {
                const int ml = fl_e[w][e] >> 16;
                const int pos = row_base[ml] + atomicAdd(&row_cnt[ml], 1);
                if (pos < cap) {
                    if constexpr (MODE != SC_RANK) cval[(int64_t)(m0 + ml) * cap + pos] = fl_v[w][e];      // (the ranks need the column only)
                    cidx[(int64_t)(m0 + ml) * cap + pos] = ns0 + (fl_e[w][e] & 0xffff);
                }
            }
        __syncthreads();
        fcount = 0;
    };

    const int nk = dp / SC_BK;
    u32x4 ra[2], rb[2];
    gload(Ab, m0, M, 0, ra);
    gload(Bb, ns0, N, 0, rb);
    for (int tn = tn0; tn < tn1; ++tn) {
        const int n0 = tn * SC_T;
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
        // (no wave reads the operand buffers any more: the last slab's barrier, or the flush's)
        sstore(As[0], ra);
        sstore(Bs[0], rb);
        if (nk > 1) {
            gload(Ab, m0, M, SC_BK, ra);
            gload(Bb, n0, N, SC_BK, rb);
        }
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int cur = kt & 1;
#pragma unroll
            for (int s = 0; s < SC_BK / 16; ++s) {
                // lane (r, h) holds k = 16 s + 8 h .. + 7 of its row = chunk 2 s + h: one 16-byte read per 32 x 32 operand block
                bf16x8 af[2], bf[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const bf16x8*>(As[cur] + sc_lds_off(wm * 64 + i * 32 + r, 2 * s + h));
#pragma unroll
                for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const bf16x8*>(Bs[cur] + sc_lds_off(wn * 64 + j * 32 + r, 2 * s + h));
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
            if (kt + 1 < nk) {              // the other buffer: every wave's reads of it ended before the last barrier
                sstore(As[cur ^ 1], ra);
                sstore(Bs[cur ^ 1], rb);
                if (kt + 2 < nk) {
                    gload(Ab, m0, M, (kt + 2) * SC_BK, ra);
                    gload(Bb, n0, N, (kt + 2) * SC_BK, rb);
                }
            }
            __syncthreads();
        }
        if (tn + 1 < tn1) {                 // the next tile's first slab flies across the epilogue
            gload(Ab, m0, M, 0, ra);
            gload(Bb, n0 + SC_T, N, 0, rb);
        }
        // (opaque copies: the per-register row terms and row addresses below are tile-invariant, and hoisted out of the strip loop
        // they would hold over a hundred VGPRs across the MFMA loop)
        float narow_t = narow, trow_t = trow;
        int m0_t = m0, h_t = h;
        asm volatile("" : "+v"(narow_t), "+v"(trow_t), "+s"(m0_t), "+v"(h_t));
        float nbcol[2];                     // a lane's two column terms
#pragma unroll
        for (int j = 0; j < 2; ++j) nbcol[j] = nb_p[min(n0 + wn * 64 + j * 32 + r, N - 1)];
        float r1row_t = r1row, r2col[2] = {0.f, 0.f};
        int ridrow_t = ridrow;
        unsigned long long bestcol[2] = {0ull, 0ull};
        if constexpr (MODE != SC_PLAIN) {
            asm volatile("" : "+v"(r1row_t), "+v"(ridrow_t));
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int nc = min(n0 + wn * 64 + j * 32 + r, N - 1);
                if (cs) r2col[j] = al.r2[nc];
                if constexpr (MODE == SC_VIABLE) bestcol[j] = al.best[nc];
            }
        }
        int before_tile = 0;                // SC_RANK: this tile's part of before_row
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int rbase = i * 32 + (reg & 3) + 8 * (reg >> 2);           // compile-time
                const int ml = wm * 64 + rbase + 4 * h_t, m = m0_t + ml;
                const float na = h_t ? bcast_f(narow_t, rbase + 4) : bcast_f(narow_t, rbase);
                float tau = 0.f;
                if constexpr (FILTER) tau = h_t ? bcast_f(trow_t, rbase + 4) : bcast_f(trow_t, rbase);
                float r1v = 0.f;
                int rid = 0;
                if constexpr (MODE != SC_PLAIN) r1v = h_t ? bcast_f(r1row_t, rbase + 4) : bcast_f(r1row_t, rbase);
                if constexpr (MODE == SC_VIABLE || MODE == SC_RANK)
                    rid = __float_as_int(h_t ? bcast_f(__int_as_float(ridrow_t), rbase + 4) : bcast_f(__int_as_float(ridrow_t), rbase));
                int c0 = 0, c1 = 0;            // SC_RANK, wave-uniform: the certainly-before columns of rows rbase / rbase + 4
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int n = n0 + wn * 64 + j * 32 + r;
                    const float v = acc[i][j][reg], e = screen_err(na, nbcol[j]);
                    if constexpr (!FILTER) {
                        if (m < M && n < N) C[(int64_t)m * ldc + n] = v - e;
                    } else {
                        bool pass;
                        if constexpr (MODE == SC_PLAIN) {
                            pass = m < M && n < N && !(v + e < tau);
                        } else if constexpr (MODE == SC_RANK) {
                            // tau = g, rid = G.  Both certain tests fail on a NaN bound, and `fin` keeps a non-finite sh or e (bf16
                            // overflow) from deciding: such a column is listed and rescored.  Columns >= N never count.
                            const float clo = sc_value<MODE>(v - e, r1v, r2col[j], cs), chi = sc_value<MODE>(v + e, r1v, r2col[j], cs);
                            const bool in = m < M && n < N, fin = fabsf(v) + e < INFINITY;
                            const bool before = in && fin && (clo > tau || (clo == tau && n < rid));
                            const bool never = fin && (chi < tau || (chi == tau && n > rid));
                            pass = in && !before && !never;
                            const unsigned long long bm = __ballot(before);
                            c0 += __popc((unsigned)bm);
                            c1 += __popc((unsigned)(bm >> 32));
                        } else {
                            const float chi = sc_value<MODE>(v + e, r1v, r2col[j], cs);
                            pass = m < M && n < N && !(chi < tau);
                            if constexpr (MODE == SC_VIABLE) pass = pass && tk_pack(chi, rid) > bestcol[j];
                        }
                        const unsigned long long mask = __ballot(pass);
                        if (mask != 0ull) {                    // wave-uniform
                            if (pass) {
                                const int slot = fcount + __popcll(mask & ((1ull << lane) - 1ull));
                                if (slot < SC_FL_CAP) {
                                    fle[slot] = (ml << 16) | (n - ns0);
                                    if constexpr (MODE != SC_RANK) flv[slot] = v;
                                } else {                       // the wave's list is full: its own slot, directly
                                    const int pos = atomicAdd(cnt + m, 1);
                                    if (pos < cap) {
                                        if constexpr (MODE != SC_RANK) cval[(int64_t)m * cap + pos] = v;
                                        cidx[(int64_t)m * cap + pos] = n;
                                    }
                                }
                            }
                            fcount = min(fcount + __popcll(mask), SC_FL_CAP);
                        }
                    }
                }
                // SC_RANK: rows rbase and rbase + 4 are lanes rbase and rbase + 4 of before_row; (i, reg) covers every lane once per
                // tile (sg_epi_count's scheme: the counts are scalars, a lane write each, no compare masks kept alive)
                if constexpr (MODE == SC_RANK)
                    asm("s_nop 0\n\tv_writelane_b32 %0, %1, %2\n\tv_writelane_b32 %0, %3, %4"
                        : "+v"(before_tile)
                        : "s"(c0), "n"(rbase), "s"(c1), "n"(rbase + 4));
                // (one register's tests at a time: scheduled ahead, the e and tau of all 64 would be live at once)
                if constexpr (FILTER) __builtin_amdgcn_sched_barrier(0);
            }
        before_row += before_tile;
        if constexpr (FILTER) {
            // block-uniform: flush when some wave's list could not take a typical tile any more
            const bool last = tn + 1 == tn1;
            if (__syncthreads_or(fcount > SC_FL_CAP - SC_FL_ROOM) || last) flush_block();
        }
    }
    // SC_RANK: one integer atomic per (wave, row) and strip; sums of integers: the same bits whatever the grid (rows >= M: no such row)
    if constexpr (MODE == SC_RANK)
        if (before_row != 0 && m0 + wm * 64 + lane < M) atomicAdd(al.rank + m0 + wm * 64 + lane, before_row);
}

// The sample of the alignment forms, in place behind screen_gemm_kernel<false>: S[m][n] = sh - e becomes c_lo, and -inf in the viable
// form unless the column is certainly viable (fewer than k of those: lower_m = -inf, every possibly viable column is listed)
template <bool VIABLE>
__global__ __launch_bounds__(kBlock) void screen_sample_align_kernel(float* __restrict__ S, int64_t lds, int n, ScreenAlign al) {
    float* row = S + (int64_t)blockIdx.x * lds;
    const bool cs = al.r1 != nullptr;
    const float r1b = cs ? al.r1[blockIdx.x] : 0.f;
    int rid = 0;
    if constexpr (VIABLE) rid = al.row_id[blockIdx.x];
    for (int j = threadIdx.x; j < n; j += kBlock) {
        const float clo = cs ? csls_value(row[j], r1b, al.r2[j]) : row[j];
        if constexpr (VIABLE) row[j] = tk_pack(clo, rid) > al.best[j] ? clo : -INFINITY;
        else row[j] = clo;
    }
}

// ---- prune, rescore, select: one block per row ---------------------------------------------------------------------------------
// The rows whose list fits.  12 KB of LDS (the list's entries stay in their threads' registers between the two passes over them),
// so eight blocks share a CU and their gathers of B's rows overlap; the overflowing rows are screen_overflow_kernel's.
static_assert(SC_CAP == 4 * kBlock, "a thread holds four list entries");
// a viable row may run out of columns: (idx -1, val -inf), cand_select_body's rule
__device__ __forceinline__ void sc_emit_viable(int64_t at, unsigned long long e, float* __restrict__ val, int32_t* __restrict__ idx) {
    const bool none = e == 0ull || tk_unpack_value(e) == -INFINITY;
    idx[at] = none ? -1 : tk_unpack_index(e);
    val[at] = none ? -INFINITY : tk_unpack_value(e);
}

// MODE: lower' is the k-th largest c_lo (SC_VIABLE: of the certainly viable entries), an entry is kept unless c_hi < lower' (or it
// is certainly not viable), the exact score is rescored to c and, SC_VIABLE, put to the exact predicate before the last sort
template <int MODE = SC_PLAIN, class... AL>
__global__ __launch_bounds__(kBlock) void screen_select_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ Bm,
                                                               int64_t ldb, int d, int k, const float* __restrict__ na,
                                                               const float* __restrict__ nb, const int* __restrict__ cnt,
                                                               const float* __restrict__ cval, const int* __restrict__ cidx, int cap,
                                                               float* __restrict__ val, int32_t* __restrict__ idx,
                                                               int32_t* __restrict__ n_rescored, AL... alp) {
    static_assert(sizeof...(AL) == (MODE == SC_PLAIN ? 0 : 1), "SC_CSLS and SC_VIABLE take one ScreenAlign");
    const ScreenAlign al = sc_align(alp...);
    __shared__ unsigned long long skey[SC_CAP];
    __shared__ int kept_n[SC_CAP];
    __shared__ int s_kept;
    __shared__ float s_lower;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int C = cnt[b];
    if (C > cap) return;
    const float* arow = A + (int64_t)b * lda;
    // lower' = the k-th largest sh - e of the list (-inf if it has fewer than k entries)
    const float nab = na[b];
    bool cs = MODE == SC_CSLS;
    float r1b = 0.f;
    int rid = 0;
    if constexpr (MODE != SC_PLAIN) {
        if constexpr (MODE == SC_VIABLE) {
            cs = al.r1 != nullptr;
            rid = al.row_id[b];
        }
        r1b = cs ? al.r1[b] : 0.f;
    }
    if (tid == 0) s_kept = 0;
    float hi[4];                            // sh + e of the thread's entries
    int nn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tid + kBlock * i;
        hi[i] = -INFINITY;
        nn[i] = 0;
        if (c < C) {
            const float v = cval[(int64_t)b * cap + c];
            nn[i] = cidx[(int64_t)b * cap + c];
            const float e = screen_err(nab, nb[nn[i]]);
            if constexpr (MODE == SC_PLAIN) {
                hi[i] = v + e;
                skey[c] = tk_pack(v - e, nn[i]);
            } else {
                const float r2n = cs ? al.r2[nn[i]] : 0.f;
                const float clo = sc_value<MODE>(v - e, r1b, r2n, cs);
                hi[i] = sc_value<MODE>(v + e, r1b, r2n, cs);
                if constexpr (MODE == SC_VIABLE) {
                    const unsigned long long held = al.best[nn[i]];
                    skey[c] = tk_pack(clo, rid) > held ? tk_pack(clo, nn[i]) : 0ull;
                    if (!(tk_pack(hi[i], rid) > held)) nn[i] = -1;         // certainly not viable
                } else {
                    skey[c] = tk_pack(clo, nn[i]);
                }
            }
        }
    }
    tk_sort_emit(skey, C, k, [&](int c, unsigned long long e) {
        if (c == k - 1) s_lower = e == 0ull ? -INFINITY : tk_unpack_value(e);
    });
    __syncthreads();
    // the entries that can still be among the k best; their order in the kept list is free (the last sort decides)
    const float lower = s_lower;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (tid + kBlock * i < C && !(hi[i] < lower) && (MODE != SC_VIABLE || nn[i] >= 0)) kept_n[atomicAdd(&s_kept, 1)] = nn[i];
    __syncthreads();
    const int K = s_kept;
    // exact scores: the fp32 product's own sequence, 32 kept columns per wave step.  K is mostly under 64, two steps: odd rows give
    // them to waves 2 and 3, so that a CU's blocks keep all four SIMDs' matrix pipes busy, not two.
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    for (int c0 = ((wave + 2 * (b & 1)) & 3) * 32; c0 < K; c0 += 32 * (kBlock / 64)) {
        const int n = kept_n[min(c0 + r, K - 1)];
        const f32x16 acc = sim_row_tile_grouped(arow, Bm + (int64_t)n * ldb, d);
        if (h == 0 && c0 + r < K) {
            if constexpr (MODE == SC_PLAIN) {
                skey[c0 + r] = tk_pack(acc[0], n);
            } else {
                const float c = sc_value<MODE>(acc[0], r1b, cs ? al.r2[n] : 0.f, cs);
                if constexpr (MODE == SC_VIABLE) skey[c0 + r] = tk_pack(c, rid) > al.best[n] ? tk_pack(c, n) : 0ull;
                else skey[c0 + r] = tk_pack(c, n);
            }
        }
    }
    if constexpr (MODE == SC_VIABLE) {
        tk_sort_emit(skey, K, k, [&](int c, unsigned long long e) { sc_emit_viable((int64_t)b * k + c, e, val, idx); });
    } else {
        tk_sort_emit(skey, K, k, [&](int c, unsigned long long e) {
            idx[(int64_t)b * k + c] = tk_unpack_index(e);
            if (val) val[(int64_t)b * k + c] = tk_unpack_value(e);
        });
    }
    if (tid == 0 && n_rescored) n_rescored[b] = K;
}
// A row whose list overflowed (mass ties: more than cap columns within e of its k-th score): every score recomputed with the
// product's sequence and selected as jmac_sim_topk_f32's overflowing rows are: slow, exact.  The other rows' blocks return at once.
// MODE: on c, and SC_VIABLE over the columns that pass the exact predicate, as cand_select_body's overflowing rows.
template <int MODE = SC_PLAIN, class... AL>
__global__ __launch_bounds__(kBlock) void screen_overflow_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ Bm,
                                                                 int64_t ldb, int N, int d, int k, const int* __restrict__ cnt, int cap,
                                                                 float* __restrict__ val, int32_t* __restrict__ idx,
                                                                 int32_t* __restrict__ n_rescored, AL... alp) {
    static_assert(sizeof...(AL) == (MODE == SC_PLAIN ? 0 : 1), "SC_CSLS and SC_VIABLE take one ScreenAlign");
    const ScreenAlign al = sc_align(alp...);
    __shared__ TkShared tk;
    const int b = blockIdx.x;
    if (cnt[b] <= cap) return;
    const float* arow = A + (int64_t)b * lda;
    if constexpr (MODE == SC_PLAIN) {
        tk_select_recomputed(tk, k, [&](auto f) { for_each_row_score(arow, Bm, ldb, N, d, f); },
                             [&](int c, unsigned long long e) {
                                 idx[(int64_t)b * k + c] = tk_unpack_index(e);
                                 if (val) val[(int64_t)b * k + c] = tk_unpack_value(e);
                             });
    } else {
        const bool cs = MODE == SC_CSLS || al.r1 != nullptr;
        const float r1b = cs ? al.r1[b] : 0.f;
        int rid = 0;
        if constexpr (MODE == SC_VIABLE) rid = al.row_id[b];
        tk_select_recomputed(
            tk, k,
            [&](auto f) {
                for_each_row_score(arow, Bm, ldb, N, d, [&](int n, float v) {
                    const float c = sc_value<MODE>(v, r1b, cs ? al.r2[n] : 0.f, cs);
                    if (MODE != SC_VIABLE || tk_pack(c, rid) > al.best[n]) f(n, c);
                });
            },
            [&](int c, unsigned long long e) {
                if constexpr (MODE == SC_VIABLE) {
                    sc_emit_viable((int64_t)b * k + c, e, val, idx);
                } else {
                    idx[(int64_t)b * k + c] = tk_unpack_index(e);
                    if (val) val[(int64_t)b * k + c] = tk_unpack_value(e);
                }
            });
    }
    if (threadIdx.x == 0 && n_rescored) n_rescored[b] = -1;
}
__global__ __launch_bounds__(kBlock) void screen_fill_kernel(int32_t* __restrict__ p, int64_t n, int32_t v) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- the ranks: gold values, then (behind screen_gemm_kernel<true, SC_RANK>) the undecided columns, one block per row ------------
__global__ __launch_bounds__(kBlock) void screen_gold_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ Bm,
                                                             int64_t ldb, int M, int d, const float* __restrict__ r1,
                                                             const float* __restrict__ r2, const int32_t* __restrict__ gold,
                                                             float* __restrict__ gval, int32_t* __restrict__ rank) {
    csls_gold_body(A, lda, Bm, ldb, M, d, r1, r2, gold, gval, rank);
}

// rank[b] holds 1 + the certainly-before count.  A list that fits: its columns rescored with the fp32 product's own sequence, the exact
// predicate's hits added.  One that does not (more than cap columns within the bound of the gold value): the partial count is dropped;
// finish != 0 recounts the row over all N columns here (slow, exact, as the top-k forms' overflowing rows), finish == 0 leaves
// rank = 0 for the caller's dense pass.  Hits are integers summed through LDS: no order dependence.
__global__ __launch_bounds__(kBlock) void screen_rank_resolve_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ Bm,
                                                                     int64_t ldb, int N, int d, const float* __restrict__ r1,
                                                                     const float* __restrict__ r2, const int32_t* __restrict__ gold,
                                                                     const float* __restrict__ gval, const int* __restrict__ cnt,
                                                                     const int* __restrict__ cidx, int cap, int finish,
                                                                     int32_t* __restrict__ rank, int32_t* __restrict__ n_rescored) {
    __shared__ int s_hits;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int C = cnt[b];
    const bool over = C > cap;              // block-uniform
    if (over && !finish) {
        if (tid == 0) {
            rank[b] = 0;
            if (n_rescored) n_rescored[b] = -1;
        }
        return;
    }
    if (tid == 0) s_hits = 0;
    __syncthreads();
    const float* arow = A + (int64_t)b * lda;
    const bool cs = r1 != nullptr;
    const float r1b = cs ? r1[b] : 0.f, g = gval[b];
    const int G = gold[b];
    int hits = 0;
    auto test = [&](int n, float s) {
        const float c = cs ? csls_value(s, r1b, r2[n]) : s;
        hits += c > g || (c == g && n < G);
    };
    if (over) {
        for_each_row_score(arow, Bm, ldb, N, d, test);
    } else {
        // 32 listed columns per wave step; odd rows start at waves 2 and 3 (screen_select_kernel's spread over the SIMDs)
        const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
        for (int c0 = ((wave + 2 * (b & 1)) & 3) * 32; c0 < C; c0 += 32 * (kBlock / 64)) {
            const int n = cidx[(int64_t)b * cap + min(c0 + r, C - 1)];
            const f32x16 acc = sim_row_tile_grouped(arow, Bm + (int64_t)n * ldb, d);
            if (h == 0 && c0 + r < C) test(n, acc[0]);
        }
    }
    if (hits) atomicAdd(&s_hits, hits);
    __syncthreads();
    if (tid == 0) {
        rank[b] = (over ? 1 : rank[b]) + s_hits;
        if (n_rescored) n_rescored[b] = over ? -1 : C;
    }
}

// strip: as few tiles per block as fill the device once (3 resident blocks per CU): more blocks than that would queue behind them,
// fewer leave CUs idle; the lists' contents do not depend on it
template <bool FILTER, int MODE = SC_PLAIN>
static int launch_screen_gemm(const bf16_t* Ab, const bf16_t* Bb, int64_t dp, int64_t M, int64_t N, const ScreenEpi& ext, hipStream_t st,
                              const ScreenAlign& al = ScreenAlign{}) {
    const int64_t tiles_m = (M + SC_T - 1) / SC_T, tiles_n = (N + SC_T - 1) / SC_T;
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const int64_t resident = 3 * (int64_t)(cus > 0 ? cus : 256);
    int64_t strip = (tiles_m * tiles_n + resident - 1) / resident;
    strip = strip < 1 ? 1 : strip > SC_STRIP_MAX ? SC_STRIP_MAX : strip;
    const int64_t blocks = tiles_m * ((tiles_n + strip - 1) / strip);
    if (blocks >= INT32_MAX) return JMAC_ERANGE;
    if constexpr (MODE == SC_PLAIN)
        hipLaunchKernelGGL((screen_gemm_kernel<FILTER>), dim3((unsigned)blocks), dim3(kBlock), 0, st, Ab, Bb, (int)dp, (int)M, (int)N,
                           (int)tiles_m, (int)tiles_n, (int)strip, ext);
    else
        hipLaunchKernelGGL((screen_gemm_kernel<FILTER, MODE, ScreenAlign>), dim3((unsigned)blocks), dim3(kBlock), 0, st, Ab, Bb, (int)dp,
                           (int)M, (int)N, (int)tiles_m, (int)tiles_n, (int)strip, ext, al);
    return (int)hipGetLastError();
}

static int sc_fill_unscreened(int32_t* n_rescored, int64_t L, hipStream_t st) {
    if (n_rescored) hipLaunchKernelGGL(screen_fill_kernel, dim3((unsigned)((L + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, n_rescored, L, -2);
    return (int)hipGetLastError();
}

// the four stages for a screened shape (sc_fused), every decision on what MODE names; al: SC_CSLS / SC_VIABLE's terms
template <int MODE>
static int sc_run(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N, int64_t d, int32_t k, float* val,
                  int32_t* idx, int32_t* n_rescored, void* ws, hipStream_t st, const ScreenAlign& al = ScreenAlign{}) {
    char* wb = (char*)ws;
    const ScWs w = sc_layout(L, N, d, k);
    const int64_t dp = sc_dp(d), Ns = sc_sample(N);
    bf16_t* Ab = (bf16_t*)(wb + w.ab);
    bf16_t* Bb = (bf16_t*)(wb + w.bb);
    float* val0 = (float*)(wb + w.val0);
    ScreenEpi e{};
    e.na = (float*)(wb + w.na); e.nb = (float*)(wb + w.nb);
    e.C = (float*)(wb + w.S); e.ldc = Ns;
    e.tau = val0 + (k - 1); e.tau_stride = k;
    e.cnt = (int*)(wb + w.cnt); e.cval = (float*)(wb + w.cval); e.cidx = (int*)(wb + w.cidx); e.cap = SC_CAP;
    const dim3 rows((unsigned)L), block(kBlock);
    // 1. bf16 copies and norm bounds
    hipLaunchKernelGGL(screen_prepare_kernel, dim3((unsigned)((L + 3) / 4)), block, 0, st, A, lda, (int)L, (int)d, (int)dp, SC_KAPPA, Ab, (float*)e.na);
    hipLaunchKernelGGL(screen_prepare_kernel, dim3((unsigned)((N + 3) / 4)), block, 0, st, B, ldb, (int)N, (int)d, (int)dp, 1.f, Bb, (float*)e.nb);
    // 2. lower_m = the k-th largest sh - e (c_lo; of the certainly viable columns) of row m over the first Ns columns
    if (int rc = launch_screen_gemm<false>(Ab, Bb, dp, L, Ns, e, st)) return rc;
    if constexpr (MODE != SC_PLAIN) hipLaunchKernelGGL(screen_sample_align_kernel<MODE == SC_VIABLE>, rows, block, 0, st, e.C, Ns, (int)Ns, al);
    if (int rc = jmac_row_topk_f32(e.C, Ns, L, Ns, k, val0, (int32_t*)(wb + w.idx0), (jmac_stream_t)st)) return rc;
    // 3. all N columns, the sample's included, through the list epilogue
    if (hipMemsetAsync(e.cnt, 0, (size_t)L * 4, st) != hipSuccess) return (int)hipGetLastError();
    if (int rc = launch_screen_gemm<true, MODE>(Ab, Bb, dp, L, N, e, st, al)) return rc;
    // 4. prune, rescore exactly, select
    if constexpr (MODE == SC_PLAIN) {
        hipLaunchKernelGGL((screen_select_kernel<>), rows, block, 0, st, A, lda, B, ldb, (int)d, (int)k, e.na, e.nb, e.cnt, e.cval, e.cidx, e.cap,
                           val, idx, n_rescored);
        hipLaunchKernelGGL((screen_overflow_kernel<>), rows, block, 0, st, A, lda, B, ldb, (int)N, (int)d, (int)k, e.cnt, e.cap, val, idx, n_rescored);
    } else {
        hipLaunchKernelGGL((screen_select_kernel<MODE, ScreenAlign>), rows, block, 0, st, A, lda, B, ldb, (int)d, (int)k, e.na, e.nb, e.cnt, e.cval,
                           e.cidx, e.cap, val, idx, n_rescored, al);
        hipLaunchKernelGGL((screen_overflow_kernel<MODE, ScreenAlign>), rows, block, 0, st, A, lda, B, ldb, (int)N, (int)d, (int)k, e.cnt, e.cap, val,
                           idx, n_rescored, al);
    }
    return (int)hipGetLastError();
}

// jmac_sim_csls_topk_screened_f32 (best == NULL) and jmac_sim_csls_topk_viable_screened_f32: the fp32 entries' checks in their order,
// with the screen's two (row length, 2^31) ahead of the workspace
static int sc_align_entry(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N, int64_t d, const float* r1,
                          const float* r2, bool viable, const int32_t* row_id, const uint64_t* best, int32_t k, float* val, int32_t* idx,
                          int32_t* n_rescored, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    if (L < 0 || N <= 0 || d <= 0 || k <= 0 || k > N || k > SC_KMAX || (r1 == nullptr) != (r2 == nullptr)) return JMAC_EINVAL;
    if (L == 0) return JMAC_OK;
    if (!A || !B || !idx || (viable && (!val || !row_id || !best))) return JMAC_EINVAL;
    if (lda % 4 || ldb % 4 || d % 4 || d > SC_DMAX) return JMAC_EDIM;
    if (L >= INT32_MAX || N >= INT32_MAX) return JMAC_ERANGE;
    const bool screened = viable ? sc_fused_viable(L, N, k) : sc_fused(N, k);
    if (!ws || ws_bytes < jmac_sim_csls_topk_screened_workspace_bytes(L, N, d, k)) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (!screened) {                                         // narrow, or a refill of a few rows: no screen, the fp32 entry's own code
        const int rc = viable ? jmac_sim_csls_topk_viable_f32(A, lda, B, ldb, L, N, d, r1, r2, row_id, best, k, val, idx, ws, ws_bytes, stream)
                              : jmac_sim_csls_topk_f32(A, lda, B, ldb, L, N, d, r1, r2, k, val, idx, ws, ws_bytes, stream);
        return rc ? rc : sc_fill_unscreened(n_rescored, L, st);
    }
    ScreenAlign al{};
    al.r1 = r1; al.r2 = r2; al.row_id = row_id; al.best = reinterpret_cast<const unsigned long long*>(best);
    if (viable) return sc_run<SC_VIABLE>(A, lda, B, ldb, L, N, d, k, val, idx, n_rescored, ws, st, al);
    if (r1) return sc_run<SC_CSLS>(A, lda, B, ldb, L, N, d, k, val, idx, n_rescored, ws, st, al);
    return sc_run<SC_PLAIN>(A, lda, B, ldb, L, N, d, k, val, idx, n_rescored, ws, st);      // c = s: jmac_sim_topk_screened_f32's launches
}

// jmac_sim_csls_rank_screened_f32's workspace and stages
struct RkWs { size_t ab, bb, na, nb, gval, cnt, cidx, total; };
static RkWs rk_layout(int64_t L, int64_t N, int64_t d) {
    RkWs w{};
    size_t off = 0;
    w.ab = off;   off += align_up((size_t)L * (size_t)sc_dp(d) * 2);
    w.bb = off;   off += align_up((size_t)N * (size_t)sc_dp(d) * 2);
    w.na = off;   off += align_up((size_t)L * 4);
    w.nb = off;   off += align_up((size_t)N * 4);
    w.gval = off; off += align_up((size_t)L * 4);
    w.cnt = off;  off += align_up((size_t)L * 4);
    w.cidx = off; off += align_up((size_t)L * RK_CAP * 4);
    w.total = off + 256;
    return w;
}

static int rk_run(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N, int64_t d, const float* r1,
                  const float* r2, const int32_t* gold, int32_t* rank, int32_t* n_rescored, int32_t finish, void* ws, hipStream_t st) {
    char* wb = (char*)ws;
    const RkWs w = rk_layout(L, N, d);
    const int64_t dp = sc_dp(d);
    bf16_t* Ab = (bf16_t*)(wb + w.ab);
    bf16_t* Bb = (bf16_t*)(wb + w.bb);
    float* gval = (float*)(wb + w.gval);
    ScreenEpi e{};
    e.na = (float*)(wb + w.na); e.nb = (float*)(wb + w.nb);
    e.tau = gval; e.tau_stride = 1;
    e.cnt = (int*)(wb + w.cnt); e.cidx = (int*)(wb + w.cidx); e.cap = RK_CAP;
    ScreenAlign al{};
    al.r1 = r1; al.r2 = r2; al.gold = gold; al.rank = rank;
    const dim3 block(kBlock);
    // 1. bf16 copies and norm bounds
    hipLaunchKernelGGL(screen_prepare_kernel, dim3((unsigned)((L + 3) / 4)), block, 0, st, A, lda, (int)L, (int)d, (int)dp, SC_KAPPA, Ab, (float*)e.na);
    hipLaunchKernelGGL(screen_prepare_kernel, dim3((unsigned)((N + 3) / 4)), block, 0, st, B, ldb, (int)N, (int)d, (int)dp, 1.f, Bb, (float*)e.nb);
    // 2. g_i with the fp32 product's bits; rank = 1
    hipLaunchKernelGGL(screen_gold_kernel, dim3((unsigned)((L + 32 * (kBlock / 64) - 1) / (32 * (kBlock / 64)))), block, 0, st, A, lda, B, ldb,
                       (int)L, (int)d, r1, r2, gold, gval, rank);
    // 3. all N columns: certain ones counted into rank, undecided ones listed
    if (hipMemsetAsync(e.cnt, 0, (size_t)L * 4, st) != hipSuccess) return (int)hipGetLastError();
    if (int rc = launch_screen_gemm<true, SC_RANK>(Ab, Bb, dp, L, N, e, st, al)) return rc;
    // 4. the lists rescored; 5. the rows whose list overflowed
    hipLaunchKernelGGL(screen_rank_resolve_kernel, dim3((unsigned)L), block, 0, st, A, lda, B, ldb, (int)N, (int)d, r1, r2, gold, gval, e.cnt,
                       e.cidx, e.cap, (int)finish, rank, n_rescored);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t jmac_sim_topk_screened_workspace_bytes(int64_t L, int64_t N, int64_t d, int32_t k) {
    if (L < 0 || N < 0 || d <= 0 || k <= 0) return 0;
    if (!sc_fused(N, k)) return jmac_sim_topk_workspace_bytes(L, N, k);
    return sc_layout(L, N, d, k).total;
}

int jmac_sim_topk_screened_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N, int64_t d, int32_t k,
                               float* val, int32_t* idx, int32_t* n_rescored, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    if (L < 0 || N <= 0 || d <= 0 || k <= 0 || k > N) return JMAC_EINVAL;
    if (L == 0) return JMAC_OK;
    if (!A || !B || !idx) return JMAC_EINVAL;
    if (lda % 4 || ldb % 4 || d % 4 || d > SC_DMAX) return JMAC_EDIM;
    if (L >= INT32_MAX || N >= INT32_MAX) return JMAC_ERANGE;
    if (!ws || ws_bytes < jmac_sim_topk_screened_workspace_bytes(L, N, d, k)) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (!sc_fused(N, k)) {                                   // narrow: no screen, the fp32 entry's own code
        if (int rc = jmac_sim_topk_f32(A, lda, B, ldb, L, N, d, k, val, idx, ws, ws_bytes, stream)) return rc;
        return sc_fill_unscreened(n_rescored, L, st);
    }
    return sc_run<SC_PLAIN>(A, lda, B, ldb, L, N, d, k, val, idx, n_rescored, ws, st);
}

size_t jmac_sim_csls_topk_screened_workspace_bytes(int64_t n1, int64_t n2, int64_t d, int32_t k) {
    if (n1 < 0 || n2 < 0 || d <= 0 || k <= 0) return 0;
    const size_t fp32 = jmac_sim_csls_topk_workspace_bytes(n1, n2, k);
    if (!sc_fused(n2, k)) return fp32;
    const size_t screened = sc_layout(n1, n2, d, k).total;    // (a viable call of a few rows runs the fp32 code in the same workspace)
    return screened > fp32 ? screened : fp32;
}

int jmac_sim_csls_topk_screened_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d,
                                    const float* r1, const float* r2, int32_t k, float* val, int32_t* idx, int32_t* n_rescored, void* ws,
                                    size_t ws_bytes, jmac_stream_t stream) {
    return sc_align_entry(A, lda, B, ldb, n1, n2, d, r1, r2, false, nullptr, nullptr, k, val, idx, n_rescored, ws, ws_bytes, stream);
}

int jmac_sim_csls_topk_viable_screened_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d,
                                           const float* r1, const float* r2, const int32_t* row_id, const uint64_t* best, int32_t k,
                                           float* val, int32_t* idx, int32_t* n_rescored, void* ws, size_t ws_bytes,
                                           jmac_stream_t stream) {
    return sc_align_entry(A, lda, B, ldb, n1, n2, d, r1, r2, true, row_id, best, k, val, idx, n_rescored, ws, ws_bytes, stream);
}

size_t jmac_sim_csls_rank_screened_workspace_bytes(int64_t n1, int64_t n2, int64_t d) {
    if (n1 < 0 || n2 < 0 || d <= 0) return 0;
    const size_t fp32 = jmac_sim_csls_rank_workspace_bytes(n1, n2);
    if (n2 < SC_MIN_N) return fp32;
    const size_t screened = rk_layout(n1, n2, d).total;
    return screened > fp32 ? screened : fp32;
}

int jmac_sim_csls_rank_screened_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d,
                                    const float* r1, const float* r2, const int32_t* gold, int32_t* rank, int32_t* n_rescored,
                                    int32_t finish, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    // jmac_sim_csls_rank_f32's checks in its order, the screen's row-length check ahead of the workspace
    if (n1 < 0 || n2 <= 0 || d <= 0 || (r1 == nullptr) != (r2 == nullptr)) return JMAC_EINVAL;
    if (n1 == 0) return JMAC_OK;
    if (!A || !B || !gold || !rank) return JMAC_EINVAL;
    if (lda % 4 || ldb % 4 || d % 4 || d > SC_DMAX) return JMAC_EDIM;
    if (n1 >= INT32_MAX || n2 >= INT32_MAX) return JMAC_ERANGE;
    if (!ws || ws_bytes < jmac_sim_csls_rank_screened_workspace_bytes(n1, n2, d)) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (n2 < SC_MIN_N) {                                     // narrow: no screen, the fp32 entry's own code
        if (int rc = jmac_sim_csls_rank_f32(A, lda, B, ldb, n1, n2, d, r1, r2, gold, rank, ws, ws_bytes, stream)) return rc;
        return sc_fill_unscreened(n_rescored, n1, st);
    }
    return rk_run(A, lda, B, ldb, n1, n2, d, r1, r2, gold, rank, n_rescored, finish, ws, st);
}

}  // extern "C"
