// sample.hip -- the completion batch of one training step, built on the device (gfx950, wave64): for every training triple
// (h, r, t) of the batch, K DISTINCT entities drawn uniformly from the entities that are NOT a true tail of (h, r), written
// in the batch layout the loss kernels read.  Replaces, per batch, TrainDataset.get_neg_sample (modules/load/data_loader.py:36-47:
// np.random.choice(all_ent[mask], num_negative, replace=False) over the (h, r) -> tails dictionary of train.py:262-285, run in
// 12 DataLoader workers), the collate of the DataLoader and the repeat / cat of train.py:347-352.
//
// The draw is a sequential process over a counter-based stream, so the result does not depend on the wave width:
//   candidate i of batch row b = word i % 4 of philox4x32_10(counter = (b, lo32(step[0]), i / 4, hi32(step[0])),
//                                                            key = (lo32(seed[0]), lo32(seed[1])));
//   m = word * num_ent (64-bit), c_i = m >> 32;  c_i is INVALID if lo32(m) < 2^32 mod num_ent (Lemire's rejection), or if c_i is
//   a true tail of the row's (h, r) (binary search in its sorted CSR slice), or if c_i equals a candidate accepted before it;
//   neg[b, 0..K) = the first K valid candidates in stream order.
// One wave per batch row.  Each round the 64 lanes take 64 consecutive candidates (lane l: word l % 4 of block l / 4 of the
// round); the values accepted so far live one per lane (slot s in lane s) and are read with v_readlane; repeats inside a round
// are resolved in lane order; __ballot + mbcnt give every valid lane its slot.  At DBP-5L size (K = 25 of 11 805 entities) one
// round serves practically every row (it would take 40 invalid candidates of 64).  ~150 B read and (K + 1) * 24 B written per row: the launch is latency-bound.
//
// The truncated form (jmac_sample_completion_batch_truncated; BootEA's hard negatives, modules/train/batch.py:88-165 with neighbor=)
// is the same kernel with a first stage in front: lane l < M holds neighbour l of the gold tail (nbr[t, l]) and is ELIGIBLE if
// that id is in range, is not a true tail of (h, r) and does not repeat a lower lane's; the first min(n_hard, eligible) slots are a
// uniform draw without replacement from the eligible lanes over a stream of their own (third counter word 0x80000000 | i / 4: the
// candidate is a lane number, Lemire's rejection over M), and the stage above fills the rest, skipping what stage 1 placed.
#include "common.h"

using namespace jmac;

namespace {

constexpr int kBlock = 256;

// n-th (0-based) set bit of mask; n < popcount(mask)
__device__ __forceinline__ int nth_set_bit(uint64_t mask, int n) {
    int pos = 0;
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
        const int cnt = __popcll((mask >> pos) & ((1ull << w) - 1ull));
        if (n >= cnt) {
            n -= cnt;
            pos += w;
        }
    }
    return pos;
}

// kHard: stage 1 from the neighbour table in front of the uniform fill; false compiles the plain sampler, nbr .. n_hard unread
template <bool kHard>
__global__ __launch_bounds__(kBlock) void sample_batch_kernel(const int64_t* __restrict__ triples, int64_t T,
                                                              const int64_t* __restrict__ perm,
                                                              const int32_t* __restrict__ key_of_triple,
                                                              const int32_t* __restrict__ tail_ptr,
                                                              const int32_t* __restrict__ tail_idx, uint32_t num_ent,
                                                              uint32_t lemire_thr, int64_t B, int K,
                                                              const int32_t* __restrict__ nbr, int64_t ldn, uint32_t M,
                                                              uint32_t nbr_thr, int n_hard,
                                                              const int64_t* __restrict__ seed, const int64_t* __restrict__ step,
                                                              int64_t* __restrict__ batch_h, int64_t* __restrict__ batch_r,
                                                              int64_t* __restrict__ batch_t) {
    const int lane = lane_id();
    const int64_t b = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (b >= B) return;                                                   // whole waves leave: b is wave-uniform
    const uint64_t draws = (uint64_t)step[0];
    const uint64_t nb = (uint64_t)step[1] % (uint64_t)(T / B);           // one replay too many wraps to batch 0: never past perm[T)
    const uint2 key = make_uint2((uint32_t)(uint64_t)seed[0], (uint32_t)(uint64_t)seed[1]);
    const int64_t ti = perm[nb * (uint64_t)B + (uint64_t)b];
    const int64_t h = triples[3 * ti], r = triples[3 * ti + 1], t = triples[3 * ti + 2];
    const int32_t row = key_of_triple[ti];
    const int lo = tail_ptr[row], hi = tail_ptr[row + 1];
    for (int j = lane; j <= K; j += 64) {                                 // sub.repeat(K + 1), rel.repeat(K + 1)   (train.py:348-349)
        batch_h[(int64_t)j * B + b] = h;
        batch_r[(int64_t)j * B + b] = r;
    }
    if (lane == 0) batch_t[b] = t;
    int64_t* neg = batch_t + B + b * (int64_t)K;                          // cat(obj, neg.view(-1))                 (train.py:350)
    // a key that leaves fewer than K entities cannot be served (the host refuses it before the launch): the loop below still
    // ends -- it places what there is and the rest of the row repeats the gold tail (in range, never read by a valid caller)
    const int64_t allowed = (int64_t)num_ent - (int64_t)(hi - lo);
    const int want = allowed < (int64_t)K ? (int)(allowed < 0 ? 0 : allowed) : K;
    for (int s = want + lane; s < K; s += 64) neg[s] = t;

    int acc = -1;                                                         // lane s: the value placed in slot s
    int placed = 0;
    if constexpr (kHard) {
        // eligible lanes: an id in range that is no true tail of (h, r) (the gold tail and the row's own entry of an inner-product
        // table go here) and repeats no lower lane's.  A <= allowed, so want1 <= want; A >= want1 ends the loop below.
        const int nl = lane < (int)M ? nbr[t * ldn + lane] : -1;
        bool elig = lane < (int)M && (uint32_t)nl < num_ent;
        if (elig) {
            int a = lo, e = hi;
            while (a < e) {
                const int mid = (a + e) >> 1;
                if (tail_idx[mid] < nl) a = mid + 1;
                else e = mid;
            }
            elig = !(a < hi && tail_idx[a] == nl);
        }
        for (int j = 0; j + 1 < (int)M; ++j) {
            const int nj = bcast_i(nl, j);
            elig = elig && !(j < lane && nj == nl);
        }
        const uint64_t emask = __ballot(elig);
        const int A = __popcll(emask);
        const int want1 = n_hard < A ? n_hard : A;
        uint64_t used = 0;                                                // lanes accepted so far
        for (uint32_t round = 0; placed < want1; ++round) {
            const uint4 w4 = philox4x32_10(make_uint4((uint32_t)b, (uint32_t)draws, 0x80000000u | (round * 16u + (uint32_t)(lane >> 2)),
                                                      (uint32_t)(draws >> 32)), key);
            const int q = lane & 3;
            const uint32_t word = q == 0 ? w4.x : q == 1 ? w4.y : q == 2 ? w4.z : w4.w;
            const uint64_t m = (uint64_t)word * (uint64_t)M;
            const int s = (int)(m >> 32);                                 // < M
            const int c = __shfl(nl, s, 64);
            bool valid = (uint32_t)m >= nbr_thr && ((emask & ~used) >> s & 1ull);
            const int se = valid ? s : -1;
            bool taken = false;                                           // my lane number was drawn in this round
#pragma unroll 8
            for (int j = 0; j < 64; ++j) {                                // repeats inside the round, in lane order
                const int sj = bcast_i(se, j);
                valid = valid && !(j < lane && sj == s);
                taken = taken || sj == lane;
            }
            used |= __ballot(taken);
            const uint64_t mask = __ballot(valid);
            const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            if (valid && placed + before < want1) neg[placed + before] = (int64_t)c;
            const int n = __popcll(mask);
            const int mine = lane - placed;
            const int src = (mine >= 0 && mine < n) ? nth_set_bit(mask, mine) : lane;
            const int got = __shfl(c, src, 64);
            if (mine >= 0 && mine < n) acc = got;
            placed += n;
        }
        placed = want1;                                                   // a last round's surplus sits in lanes >= want1: rewritten
    }                                                                     // below before `placed` reaches them
    for (uint32_t round = 0; placed < want; ++round) {
        const uint4 w4 = philox4x32_10(make_uint4((uint32_t)b, (uint32_t)draws, round * 16u + (uint32_t)(lane >> 2), (uint32_t)(draws >> 32)), key);
        const int q = lane & 3;
        const uint32_t word = q == 0 ? w4.x : q == 1 ? w4.y : q == 2 ? w4.z : w4.w;
        const uint64_t m = (uint64_t)word * (uint64_t)num_ent;
        const int c = (int)(m >> 32);
        bool valid = (uint32_t)m >= lemire_thr;
        if (valid) {                                                      // true tail of (h, r)?
            int a = lo, e = hi;
            while (a < e) {
                const int mid = (a + e) >> 1;
                if (tail_idx[mid] < c) a = mid + 1;
                else e = mid;
            }
            valid = !(a < hi && tail_idx[a] == c);
        }
        for (int s = 0; s < placed; ++s) valid = valid && bcast_i(acc, s) != c;        // accepted in an earlier round
        const int ce = valid ? c : -1;
#pragma unroll 8
        for (int j = 0; j < 63; ++j) {                                    // repeats inside the round, in lane order
            const int cj = bcast_i(ce, j);
            valid = valid && !(j < lane && cj == c);
        }
        const uint64_t mask = __ballot(valid);
        const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (valid && placed + before < want) neg[placed + before] = (int64_t)c;
        const int n = __popcll(mask);
        const int mine = lane - placed;                                   // slot `lane` is filled by the mine-th valid lane
        const int src = (mine >= 0 && mine < n) ? nth_set_bit(mask, mine) : lane;
        const int got = __shfl(c, src, 64);
        if (mine >= 0 && mine < n) acc = got;
        placed += n;
    }
}

__global__ void sample_advance_kernel(int64_t* __restrict__ step) {
    step[0] += 1;
    step[1] += 1;
}

}  // namespace

extern "C" {

int jmac_sample_completion_batch(const int64_t* triples, int64_t T, const int64_t* perm, const int32_t* key_of_triple,
                                 const int32_t* tail_ptr, const int32_t* tail_idx, int64_t num_ent, int64_t B, int64_t K,
                                 const int64_t* seed, int64_t* step, int64_t* batch_h, int64_t* batch_r, int64_t* batch_t,
                                 jmac_stream_t stream) {
    if (K < 1 || K > 64 || B < 1 || T < B || num_ent < 1) return JMAC_EINVAL;
    if (num_ent >= ((int64_t)1 << 31) || B >= ((int64_t)1 << 31) || T >= ((int64_t)1 << 31)) return JMAC_ERANGE;
    if (!triples || !perm || !key_of_triple || !tail_ptr || !tail_idx || !seed || !step || !batch_h || !batch_r || !batch_t)
        return JMAC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n = (uint32_t)num_ent;
    const uint32_t thr = (uint32_t)(0u - n) % n;                          // 2^32 mod num_ent
    const unsigned grid = (unsigned)((B + kBlock / 64 - 1) / (kBlock / 64));
    hipLaunchKernelGGL(sample_batch_kernel<false>, dim3(grid), dim3(kBlock), 0, st, triples, T, perm, key_of_triple, tail_ptr, tail_idx,
                       n, thr, B, (int)K, (const int32_t*)nullptr, (int64_t)0, 0u, 0u, 0, seed, (const int64_t*)step, batch_h, batch_r,
                       batch_t);
    // every wave above has read the step words before this runs (stream order): a captured launch advances on every replay
    hipLaunchKernelGGL(sample_advance_kernel, dim3(1), dim3(1), 0, st, step);
    return (int)hipGetLastError();
}

int jmac_sample_completion_batch_truncated(const int64_t* triples, int64_t T, const int64_t* perm, const int32_t* key_of_triple,
                                           const int32_t* tail_ptr, const int32_t* tail_idx, int64_t num_ent, int64_t B, int64_t K,
                                           const int32_t* nbr, int64_t ldn, int64_t M, int64_t n_hard, const int64_t* seed,
                                           int64_t* step, int64_t* batch_h, int64_t* batch_r, int64_t* batch_t, jmac_stream_t stream) {
    if (K < 1 || K > 64 || B < 1 || T < B || num_ent < 1 || M < 1 || M > 64 || ldn < M || n_hard < 0 || n_hard > K) return JMAC_EINVAL;
    if (num_ent >= ((int64_t)1 << 31) || B >= ((int64_t)1 << 31) || T >= ((int64_t)1 << 31)) return JMAC_ERANGE;
    if (!triples || !perm || !key_of_triple || !tail_ptr || !tail_idx || !nbr || !seed || !step || !batch_h || !batch_r || !batch_t)
        return JMAC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n = (uint32_t)num_ent, m = (uint32_t)M;
    const unsigned grid = (unsigned)((B + kBlock / 64 - 1) / (kBlock / 64));
    hipLaunchKernelGGL(sample_batch_kernel<true>, dim3(grid), dim3(kBlock), 0, st, triples, T, perm, key_of_triple, tail_ptr, tail_idx,
                       n, (uint32_t)(0u - n) % n, B, (int)K, nbr, ldn, m, (uint32_t)(0u - m) % m, (int)n_hard, seed,
                       (const int64_t*)step, batch_h, batch_r, batch_t);
    hipLaunchKernelGGL(sample_advance_kernel, dim3(1), dim3(1), 0, st, step);
    return (int)hipGetLastError();
}

}  // extern "C"
