// stable.hip -- deferred acceptance (Gale-Shapley) on candidate lists for gfx950: the one-to-one alignment of
// modules/finding/alignment.py:115-168 without preference lists on the reviewers' side.
//
//  * jmac_stable_match_f32   every suitor (row of the lists) proposes down its list until a reviewer keeps it or the list ends
//
// Order, both sides: larger value first, equal values -> lower index first -- topk_select.h's tk_pack word.  The state of
// reviewer j is ONE 64-bit word, best[j] = tk_pack(c(i, j), i) of the best proposal it has ever received (0: free): a reviewer
// only trades up, so a proposal is atomicMax(&best[j], word) (one returning global_atomic_umax_x2) and its answer is the
// returned word --
//   larger            rejected, for good (best only grows);
//   smaller, not 0    accepted, and suitor tk_unpack_index(returned) has just lost j;
//   0                 accepted by a free reviewer.
// Suitor i holds j iff best[j] is its own word.  The fixpoint is the suitor-optimal stable matching of the instance the lists
// describe; with strict preferences it is unique, so the integers do not depend on which thread ran when.
//
// One launch reaches the fixpoint without any thread waiting for another: the thread that displaces a suitor CONTINUES AS that
// suitor (its place in its own list is found by looking its lost reviewer up there; the lists are read-only during the call),
// so at every moment each suitor is either holding, out of candidates, or carried by exactly one running thread -- the one
// whose atomic saw its word come back.  A thread ends when its chain reaches a free reviewer or the end of a list; every
// accepted proposal raises some best[j] and every other one advances a list position, so all chains end.  A second launch
// reads the state off `best`.
#include "common.h"
#include "topk_select.h"

using namespace jmac;

namespace {

constexpr int kBlock = 256;
constexpr int SM_HELD_BIT = INT32_MIN;      // ptr[i]: list position, with this bit set while the suitor holds that entry

struct SmLists {
    const int32_t* idx;                     // [n1, ld] reviewer ids, -1 ends a list
    const float* val;                       // [n1, ld] c(i, idx[i, p])
    int64_t ld;
    int k;
    __device__ __forceinline__ int reviewer(int i, int p) const { return p < k ? idx[(int64_t)i * ld + p] : -1; }
    __device__ __forceinline__ unsigned long long word(int i, int p) const { return tk_pack(val[(int64_t)i * ld + p], i); }
};

// thread i starts suitor i unless it holds already (or has nothing left), from the position ptr[i] remembers
__global__ __launch_bounds__(kBlock) void stable_propose_kernel(SmLists l, int n1, int n2, const int32_t* __restrict__ ptr,
                                                                unsigned long long* __restrict__ best,
                                                                unsigned long long* __restrict__ proposals) {
    int i = blockIdx.x * kBlock + threadIdx.x;
    unsigned made = 0;
    if (i < n1 && ptr[i] >= 0) {
        int p = ptr[i];
        for (;;) {
            const int j = l.reviewer(i, p);
            if (j < 0 || j >= n2) break;                       // suitor i is out of candidates (an id past n2 ends a list too)
            const unsigned long long w = l.word(i, p);
            const unsigned long long old = atomicMax(best + j, w);
            ++made;
            if (old > w) {                                     // rejected
                ++p;
                continue;
            }
            if (old == 0ull || old == w) break;                // j was free (or the list names j twice): the chain ends
            // accepted, and suitor `old` has lost j: carry on as that suitor, behind j in its list
            i = tk_unpack_index(old);
            for (p = 0; l.reviewer(i, p) != j && l.reviewer(i, p) >= 0; ++p) {}
            ++p;
        }
    }
    // one counter update per wave
    made = (unsigned)wave_sum_i((int)made);
    if (lane_id() == 0 && made) atomicAdd(proposals, (unsigned long long)made);
}

// the state after the fixpoint, per suitor: the list entry it holds (searched from the remembered position on: nothing before it
// can be held) -> match1, ptr; none -> "exhausted" if its list has entries, plain unmatched if the list is empty
__global__ __launch_bounds__(kBlock) void stable_suitors_kernel(SmLists l, int n1, int n2, int32_t* __restrict__ ptr,
                                                                const unsigned long long* __restrict__ best,
                                                                int32_t* __restrict__ match1, int32_t* __restrict__ exhausted,
                                                                unsigned long long* __restrict__ n_exhausted) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n1) return;
    int p = ptr[i] & ~SM_HELD_BIT, held = -1;
    for (;; ++p) {
        const int j = l.reviewer(i, p);
        if (j < 0 || j >= n2) break;
        if (best[j] == l.word(i, p)) {
            held = j;
            break;
        }
    }
    match1[i] = held;
    ptr[i] = held >= 0 ? (p | SM_HELD_BIT) : p;
    if (held < 0 && l.reviewer(i, 0) >= 0) exhausted[atomicAdd(n_exhausted, 1ull)] = i;
}

__global__ __launch_bounds__(kBlock) void stable_reviewers_kernel(int n2, const unsigned long long* __restrict__ best,
                                                                  int32_t* __restrict__ match2) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j < n2) match2[j] = best[j] != 0ull ? tk_unpack_index(best[j]) : -1;
}

}  // namespace

extern "C" {

size_t jmac_stable_match_workspace_bytes(int64_t n1, int64_t n2) {
    if (n1 < 0 || n2 < 0) return 0;
    return align_up((size_t)n1 * 4) + 256;                     // the exhausted suitors' ids
}

int jmac_stable_match_f32(const int32_t* cand_idx, const float* cand_val, int64_t ld, int64_t n1, int64_t n2, int32_t k, int32_t* ptr,
                          uint64_t* best, int32_t* match1, int32_t* match2, uint64_t* counters, void* ws, size_t ws_bytes,
                          jmac_stream_t stream) {
    if (n1 < 0 || n2 < 0 || k <= 0 || ld < k) return JMAC_EINVAL;
    if (!counters) return JMAC_EINVAL;
    if ((n1 > 0 && (!cand_idx || !cand_val || !ptr || !match1)) || (n2 > 0 && (!best || !match2))) return JMAC_EINVAL;
    if (n1 >= INT32_MAX || n2 >= INT32_MAX) return JMAC_ERANGE;
    if (!ws || ws_bytes < jmac_stable_match_workspace_bytes(n1, n2)) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
    unsigned long long* bw = reinterpret_cast<unsigned long long*>(best);
    if (hipMemsetAsync(cnt, 0, 16, st) != hipSuccess) return (int)hipGetLastError();
    const SmLists l{cand_idx, cand_val, ld, (int)k};
    if (n1 > 0) {
        const unsigned grid = (unsigned)((n1 + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(stable_propose_kernel, dim3(grid), dim3(kBlock), 0, st, l, (int)n1, (int)n2, (const int32_t*)ptr, bw, cnt + 1);
        hipLaunchKernelGGL(stable_suitors_kernel, dim3(grid), dim3(kBlock), 0, st, l, (int)n1, (int)n2, ptr, (const unsigned long long*)bw,
                           match1, (int32_t*)ws, cnt);
    }
    if (n2 > 0)
        hipLaunchKernelGGL(stable_reviewers_kernel, dim3((unsigned)((n2 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, (int)n2,
                           (const unsigned long long*)bw, match2);
    return (int)hipGetLastError();
}

}  // extern "C"
