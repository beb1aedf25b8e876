// topk_select.h -- the exact "k best of a row" selection that every top-k kernel of score.hip shares.
// Order: value descending, ties -> lower index first.  One block of TK_THREADS threads per row; every routine here is called by
// the whole block (it synchronises), and its LDS is declared once by the calling kernel and passed in.
#pragma once
#include "common.h"

namespace jmac {

constexpr int TK_BINS = 4096, TK_CAP = 1024, TK_THREADS = 256;

__device__ __forceinline__ unsigned tk_key(float v) {          // ascending float order == ascending unsigned order
    const unsigned u = v == 0.f ? 0u : __float_as_uint(v);    // -0 and +0 compare equal: one key
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// a beats b: larger value, or equal value and lower index
__device__ __forceinline__ bool tk_beats(unsigned ka, int ia, unsigned kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

// (key, ~index) in one word: descending order of the words is the selection order.  0 is no element (below every real one).
__device__ __forceinline__ unsigned long long tk_pack(float v, int n) { return ((unsigned long long)tk_key(v) << 32) | (unsigned)(~n); }
__device__ __forceinline__ int tk_unpack_index(unsigned long long e) { return (int)~(unsigned)(e & 0xffffffffull); }
__device__ __forceinline__ float tk_unpack_value(unsigned long long e) {                  // tk_key inverted (-0 comes back as +0)
    const unsigned key = (unsigned)(e >> 32);
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

struct TkExchange {                        // the arg-max rounds' block reduction
    float wv[TK_THREADS / 64];
    int wi[TK_THREADS / 64];
    float pick_v;
    int pick_i;
};
struct TkShared {
    int hist[TK_BINS];
    unsigned long long skey[TK_CAP];
    int bin, above, cnt;
    TkExchange x;
};

// the bin b* that holds the k-th best and the elements above it, scanned from the top bin by one thread (bin 0 is reached when
// the row has fewer than k elements).  Returns the elements of bins >= b*.
__device__ __forceinline__ int tk_bin_scan(TkShared& s, int k) {
    if (threadIdx.x == 0) {
        int above = 0, bin = TK_BINS - 1;
        for (; bin > 0; --bin) {
            if (above + s.hist[bin] >= k) break;
            above += s.hist[bin];
        }
        s.bin = bin;
        s.above = above;
    }
    __syncthreads();
    return s.above + s.hist[s.bin];
}

// skey[0, Cn) (written by the caller, no barrier needed in between; Cn <= TK_CAP) -> emit(c, skey'[c]) for the k best, c in
// [0, k): a descending bitonic sort of the words, padded to a power of two with 0.  Ranking every element against every other
// one costs Cn^2 compares per row: 70 us for 3 000 rows of ~300; the sort is Cn log^2 Cn.
template <class Emit>
__device__ __forceinline__ void tk_sort_emit(unsigned long long* skey, int Cn, int k, Emit emit) {
    const int tid = threadIdx.x;
    int P = 64;
    while (P < Cn) P <<= 1;
    for (int c = Cn + tid; c < P; c += TK_THREADS) skey[c] = 0ull;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += TK_THREADS) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;            // descending runs first: the result is descending overall
                const unsigned long long x = skey[lo], y = skey[hi];
                if ((x < y) == desc) {
                    skey[lo] = y;
                    skey[hi] = x;
                }
            }
            __syncthreads();
        }
    for (int c = tid; c < k; c += TK_THREADS) emit(c, skey[c]);
}

// k rounds of (value, index) arg-max after the previous pick: for_each(f) calls f(n, v) for the thread's share of the row's
// live elements, thread 0 calls emit(round, v, n) with n == INT32_MAX (and v == -inf) once the row is used up
template <class ForEach, class Emit>
__device__ __forceinline__ void tk_argmax_rounds(TkExchange& x, int k, ForEach for_each, Emit emit) {
    const int tid = threadIdx.x;
    float pv = INFINITY;
    int pi = -1;
    for (int r = 0; r < k; ++r) {
        float bv = -INFINITY;
        int bi = INT32_MAX;
        for_each([&](int n, float v) {
            const bool after = (v < pv) || (v == pv && n > pi);       // not yet picked
            const bool better = (v > bv) || (v == bv && n < bi);
            if (after && better) {
                bv = v;
                bi = n;
            }
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if ((tid & 63) == 0) {
            x.wv[tid >> 6] = bv;
            x.wi[tid >> 6] = bi;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < TK_THREADS / 64; ++w)
                if (x.wv[w] > bv || (x.wv[w] == bv && x.wi[w] < bi)) {
                    bv = x.wv[w];
                    bi = x.wi[w];
                }
            x.pick_v = bv;
            x.pick_i = bi;
            emit(r, bv, bi);
        }
        __syncthreads();
        pv = x.pick_v;
        pi = x.pick_i;
    }
}

// The k best of a row whose elements are recomputed on every pass: emit(c, word) for c in [0, k), word = tk_pack of the c-th
// best or 0 when the row has fewer than c + 1 elements.  Pass 1 histograms the 12 leading key bits, pass 2 collects bins >= b*
// and sorts them; if even those overflow the list (e.g. a constant row), k arg-max rounds of one pass each.
template <class ForEach, class Emit>
__device__ __forceinline__ void tk_select_recomputed(TkShared& s, int k, ForEach for_each, Emit emit) {
    for (int i = threadIdx.x; i < TK_BINS; i += TK_THREADS) s.hist[i] = 0;
    if (threadIdx.x == 0) s.cnt = 0;
    __syncthreads();
    for_each([&](int n, float v) { atomicAdd(&s.hist[tk_key(v) >> 20], 1); });
    __syncthreads();
    const int C = tk_bin_scan(s, k);
    if (C <= TK_CAP) {
        const int bstar = s.bin;
        for_each([&](int n, float v) {
            if ((int)(tk_key(v) >> 20) >= bstar) s.skey[atomicAdd(&s.cnt, 1)] = tk_pack(v, n);
        });
        tk_sort_emit(s.skey, C, k, emit);
        return;
    }
    tk_argmax_rounds(s.x, k, for_each, [&](int r, float v, int n) { emit(r, n == INT32_MAX ? 0ull : tk_pack(v, n)); });
}

}  // namespace jmac
