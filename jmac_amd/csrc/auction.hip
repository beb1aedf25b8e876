// auction.hip -- Bertsekas' auction algorithm on candidate lists for gfx950: the one-to-one alignment that MAXIMISES the total
// rescored similarity ("Hungarian" in the entity-alignment literature), without the n1 x n2 matrix.
//
//  * jmac_auction_rounds_f32   up to `rounds` synchronous bidding rounds on the state the caller keeps
//
// A row (bidder) only ever needs its best and second-best value of c(i, j) - price[j].  Its list holds k columns with
// val = c - price AS OF THE REFILL and pref = the price then, so the value now is  cur = val - (price[j] - pref)  -- two fp32
// subtractions in that order, the same in every form and in tests/auction_ref.py.  Prices only rise, so an unlisted column is now
// worth at most bound = val[k - 1]: a row whose second-best listed value has sunk below that cannot decide any more and marks
// itself -2 (the host refills it from the fused top-k under the current prices).
//
// One round: every row open (-1) at its start places ONE bid -- atomicMax(&bidword[j1], tk_pack(bid, i)), topk_select.h's word:
// highest bid first, equal bids -> lower row -- and after all bids the winner of every column that received one takes it: the
// previous owner is opened, owner / match1 / price are set from the word, the word is cleared.  A column is resolved by the ONE
// thread whose row is named in its word; a loser reads either that word or the 0 that follows it, never its own id.  The floats
// depend on no atomic order: the only atomics are that max on packed words and integer counter adds.
//
// Two forms run the same rounds (same starting state -> same bits):
//   grid            one bid launch (one wave per row, lane = list entry) and one resolve launch (one thread per row) per round;
//                   a round without a bidder sets a flag in the workspace that turns the launches behind it into no-ops.
//   one workgroup   ONE launch; the open rows are a queue in LDS (a winner's slot is handed to the row it evicts, so the queue
//                   never grows), its waves take the slots in turn, __syncthreads() stands between bidding and resolving.
//                   Hundreds of rounds on a handful of open rows cost one launch instead of two launches each.
// No thread waits for another workgroup; every device loop is bounded by `rounds`, by k or by n1.
#include "common.h"
#include "topk_select.h"

using namespace jmac;

namespace {

constexpr int kBlock = 256;                         // grid form: 4 waves = 4 rows per block in the bid launch
constexpr int kOneBlock = 1024;                     // one-workgroup form: 16 waves take the queue's slots in turn
constexpr int kQueue = JMAC_AUCTION_QUEUE_ROWS;
constexpr int kRoundsMax = 4096;

struct AuLists {
    const int32_t* idx;                             // [n1, ld] column ids, every entry of a row a different column
    const float* val;                               // [n1, ld] c - price as of the refill, best first
    const float* pref;                              // [n1, ld] the price then
    int64_t ld;
    int k, n1, n2;
};

struct AuControl {                                  // head of the workspace (grid form), zeroed by every call
    unsigned round_bids[2];                         // bids of round r in [r & 1]
    unsigned done;                                  // a round had no bidder: the launches behind it do nothing
};

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// The whole wave runs row i (wave-uniform, open at the start of the round).  Returns the column it bid on, or -1 after marking
// the row -2 (its list can no longer decide).
__device__ __forceinline__ int auction_bid_row(const AuLists& l, int i, const float* price, unsigned long long* bidword,
                                               int32_t* match1, float eps) {
    const int m = lane_id();
    const int64_t row = (int64_t)i * l.ld;
    int j = -1;
    float cur = -INFINITY, pj = 0.f;
    if (m < l.k) {
        j = l.idx[row + m];
        if ((unsigned)j < (unsigned)l.n2) {
            pj = price[j];
            cur = l.val[row + m] - (pj - l.pref[row + m]);
        } else {
            j = -1;                                 // not a column: the entry does not count
        }
    }
    const unsigned long long w = j >= 0 ? tk_pack(cur, j) : 0ull;
    const unsigned long long best = wave_max_u64(w);
    const int lane1 = best != 0ull ? __ffsll((unsigned long long)__ballot(w == best)) - 1 : 0;
    const float w1 = __shfl(cur, lane1, 64), p1 = __shfl(pj, lane1, 64);
    const int j1 = __shfl(j, lane1, 64);
    const float w2 = wave_max(m == lane1 ? -INFINITY : cur);
    const float bound = l.k < l.n2 ? l.val[row + l.k - 1] : -INFINITY;
    if (best == 0ull || w2 < bound) {
        if (m == 0) match1[i] = -2;
        return -1;
    }
    float bid = (p1 + (w1 - w2)) + eps;
    if (!(bid > p1)) bid = nextafterf(p1, INFINITY);
    if (m == 0) atomicMax(bidword + j1, tk_pack(bid, i));
    return j1;
}

// Row i bid on column j this round.  If the column's word names it, it takes the column; returns the row it evicts (-1: the column
// was free), or -2 if another row won.
__device__ __forceinline__ int auction_resolve(int i, int j, int n1, float* price, int32_t* owner, int32_t* match1,
                                               unsigned long long* bidword) {
    const unsigned long long w = __hip_atomic_load(bidword + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (w == 0ull || tk_unpack_index(w) != i) return -2;
    int prev = owner[j];
    if ((unsigned)prev < (unsigned)n1) match1[prev] = -1;
    else prev = -1;
    owner[j] = i;
    match1[i] = j;
    price[j] = tk_unpack_value(w);
    bidword[j] = 0ull;
    return prev;
}

// ---- grid form ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void auction_bid_kernel(AuLists l, const float* __restrict__ price, unsigned long long* bidword,
                                                             int32_t* match1, float eps, AuControl* ctl, int32_t* __restrict__ bid_col,
                                                             int r) {
    __shared__ unsigned s_bids;
    if (ctl->done) return;                                            // block-uniform
    if (threadIdx.x == 0) s_bids = 0u;
    __syncthreads();
    const int i = blockIdx.x * (kBlock / kWave) + (int)(threadIdx.x >> 6);
    if (i < l.n1) {
        int j1 = -1;
        if (match1[i] == -1) j1 = auction_bid_row(l, i, price, bidword, match1, eps);
        if (lane_id() == 0) {
            bid_col[i] = j1;
            if (j1 >= 0) atomicAdd(&s_bids, 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_bids) atomicAdd(&ctl->round_bids[r & 1], s_bids);
}

__global__ __launch_bounds__(kBlock) void auction_resolve_kernel(int n1, float* price, int32_t* owner, int32_t* match1,
                                                                 unsigned long long* bidword, AuControl* ctl,
                                                                 const int32_t* __restrict__ bid_col, unsigned long long* counters, int r) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const unsigned bids = ctl->round_bids[r & 1];
    if (i == 0) {
        ctl->round_bids[(r + 1) & 1] = 0u;                            // the next round's counter: nobody reads it in this launch
        if (bids == 0u) {
            ctl->done = 1u;
        } else {
            counters[2] += 1ull;
            counters[3] += bids;
        }
    }
    if (bids == 0u || i >= n1) return;
    const int j = bid_col[i];
    if (j >= 0) auction_resolve(i, j, n1, price, owner, match1, bidword);
}

// ---- one-workgroup form ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kOneBlock) void auction_one_block_kernel(AuLists l, float* price, int32_t* owner, int32_t* match1,
                                                                      unsigned long long* bidword, float eps, int rounds,
                                                                      unsigned long long* counters) {
    __shared__ int s_row[kQueue];                   // the open rows (-1: an empty slot)
    __shared__ int s_col[kQueue];                   // the column a slot's row bid on this round (-1: none)
    __shared__ int s_n;
    __shared__ unsigned s_bids;
    const int tid = threadIdx.x, wave = tid >> 6;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int i = tid; i < l.n1; i += kOneBlock)
        if (match1[i] == -1) {
            const int p = atomicAdd(&s_n, 1);
            if (p < kQueue) s_row[p] = i;           // (the entry point refuses a call whose open rows do not fit)
        }
    __syncthreads();
    const int Q = min(s_n, kQueue);
    unsigned long long done_rounds = 0ull, made = 0ull;
    for (int r = 0; r < rounds; ++r) {
        if (tid == 0) s_bids = 0u;
        __syncthreads();
        for (int q = wave; q < Q; q += kOneBlock / kWave) {
            const int i = s_row[q];
            int j1 = -1;
            if (i >= 0) j1 = auction_bid_row(l, i, price, bidword, match1, eps);
            if (lane_id() == 0) {
                s_col[q] = j1;
                if (j1 >= 0) atomicAdd(&s_bids, 1u);
                else s_row[q] = -1;                 // marked -2: it sits the rest of the call out
            }
        }
        __syncthreads();
        const unsigned bids = s_bids;
        if (bids == 0u) break;                      // block-uniform
        for (int q = tid; q < Q; q += kOneBlock) {
            const int j = s_col[q];
            if (j < 0) continue;
            const int prev = auction_resolve(s_row[q], j, l.n1, price, owner, match1, bidword);
            if (prev != -2) s_row[q] = prev;        // the winner leaves the queue, the row it evicted takes its slot
        }
        done_rounds += 1ull;
        made += bids;
        __syncthreads();
    }
    if (tid == 0) {
        counters[2] = done_rounds;
        counters[3] = made;
    }
}

// counters[0] = rows open (-1 or -2), counters[1] = rows at -2, after the rounds
__global__ __launch_bounds__(kBlock) void auction_count_kernel(int n1, const int32_t* __restrict__ match1, unsigned long long* counters) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int st = i < n1 ? match1[i] : 0;
    const int open = __popcll((unsigned long long)__ballot(st < 0)), waiting = __popcll((unsigned long long)__ballot(st == -2));
    if (lane_id() == 0) {
        if (open) atomicAdd(counters, (unsigned long long)open);
        if (waiting) atomicAdd(counters + 1, (unsigned long long)waiting);
    }
}

}  // namespace

extern "C" {

size_t jmac_auction_rounds_workspace_bytes(int64_t n1, int64_t n2) {
    if (n1 < 0 || n2 < 0) return 0;
    // AuControl, the columns' bid words (0 between rounds: every call clears them), the column every row bid on this round
    return 256 + align_up((size_t)n2 * 8) + align_up((size_t)n1 * 4);
}

int jmac_auction_rounds_f32(const int32_t* idx, const float* val, const float* pref, int64_t ld, int64_t n1, int64_t n2, int32_t k,
                            float* price, int32_t* owner, int32_t* match1, float eps, int32_t rounds, int32_t form, int64_t n_open,
                            uint64_t* counters, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    if (n1 < 0 || n2 < 0 || n_open < 0 || rounds < 0 || rounds > kRoundsMax || form < 0 || form > 2) return JMAC_EINVAL;
    if (k < 2 || k > 64 || k > n2 || ld < k) return JMAC_EINVAL;
    if (!(eps > 0.f) || !(eps < INFINITY)) return JMAC_EINVAL;
    if (!counters || !price || !owner) return JMAC_EINVAL;
    if (n1 > 0 && (!idx || !val || !pref || !match1)) return JMAC_EINVAL;
    if (n1 >= INT32_MAX || n2 >= INT32_MAX) return JMAC_ERANGE;
    if (form == 2 && n_open > kQueue) return JMAC_EINVAL;
    if (!ws || ws_bytes < jmac_auction_rounds_workspace_bytes(n1, n2)) return JMAC_EWORKSPACE;
    if (form == 0) form = n_open <= kQueue ? 2 : 1;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
    AuControl* ctl = reinterpret_cast<AuControl*>(ws);
    unsigned long long* bw = reinterpret_cast<unsigned long long*>(static_cast<char*>(ws) + 256);
    int32_t* bid_col = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + 256 + align_up((size_t)n2 * 8));
    if (hipMemsetAsync(cnt, 0, 32, st) != hipSuccess) return (int)hipGetLastError();
    if (n1 == 0) return (int)hipGetLastError();
    if (hipMemsetAsync(ws, 0, 256 + align_up((size_t)n2 * 8), st) != hipSuccess) return (int)hipGetLastError();
    const AuLists l{idx, val, pref, ld, (int)k, (int)n1, (int)n2};
    if (form == 2) {
        if (rounds > 0)
            hipLaunchKernelGGL(auction_one_block_kernel, dim3(1), dim3(kOneBlock), 0, st, l, price, owner, match1, bw, eps, (int)rounds, cnt);
    } else {
        const unsigned bid_grid = (unsigned)((n1 + kBlock / kWave - 1) / (kBlock / kWave));
        const unsigned row_grid = (unsigned)((n1 + kBlock - 1) / kBlock);
        for (int r = 0; r < rounds; ++r) {
            hipLaunchKernelGGL(auction_bid_kernel, dim3(bid_grid), dim3(kBlock), 0, st, l, (const float*)price, bw, match1, eps, ctl, bid_col, r);
            hipLaunchKernelGGL(auction_resolve_kernel, dim3(row_grid), dim3(kBlock), 0, st, (int)n1, price, owner, match1, bw, ctl,
                               (const int32_t*)bid_col, cnt, r);
        }
    }
    hipLaunchKernelGGL(auction_count_kernel, dim3((unsigned)((n1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, (int)n1,
                       (const int32_t*)match1, cnt);
    return (int)hipGetLastError();
}

}  // extern "C"
