// attention.hip -- export of the relation-aware layer's per-edge attention weights (include/jmac_hip.h,
// jmac_rel_attn_edge_weights_*): what the fused forward kernel (aggregate.hip) folds into its online softmax and never writes.
//
//   h_e = P[i] + Q[j] - Rq[t]      s_e = sum_k a_k LeakyReLU(h_e[k])      alpha = softmax of s over the in-edges of i
//
// Pass 1 (attn_logit_kernel) walks the by-destination schedule, one wave per item: every item of every class is a run of CSR
// slots of one destination and the items cover each slot exactly once, so the partial-slot field is not read.  A group of G
// lanes (G = 8 .. 64, chosen from the row width) holds one edge, 64 / G edges per wave instruction and kU such steps in
// flight; P[i] and a_att stay in registers across the item.  s goes to the workspace in SLOT order.
// Pass 2 (attn_segment_*_kernel) is per destination over s[rowptr[i] : rowptr[i+1]]: max, denominator, alpha, entropy, argmax,
// written through perm.  It moves O(E) floats.
// Every reduction has a fixed order (shuffle / DPP butterflies, LDS slots read in index order): no float atomics, results are
// bitwise reproducible.
#include "common.h"

using namespace jmac;

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kU = 4;                   // edge steps in flight per wave (pass 1)
constexpr int kWaveSegMax = 512;        // pass 2: destinations up to this many in-edges take one wave, longer ones a block
constexpr int kLogitBlocksMax = 8192;   // grid caps; the kernels stride over the rest
constexpr int kSegWaveBlocksMax = 4096;
constexpr int kSegBlockBlocksMax = 512;

// ---- a lane's chunk of a table row: CH consecutive elements, kept raw until the arithmetic needs them -----------------------
template <typename TT, int CH> struct Chunk;
template <> struct Chunk<float, 4> {
    typedef float4 raw;
    static __device__ __forceinline__ raw zero() { return f4zero(); }
    static __device__ __forceinline__ raw load(const float* p) { return ld4(p); }
    static __device__ __forceinline__ void cvt(raw r, float (&v)[4]) { v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w; }
};
template <> struct Chunk<bf16_t, 4> {
    typedef uint2 raw;
    static __device__ __forceinline__ raw zero() { return make_uint2(0u, 0u); }
    static __device__ __forceinline__ raw load(const bf16_t* p) { return ldraw(p); }
    static __device__ __forceinline__ void cvt(raw r, float (&v)[4]) {
        const float4 f = cvt4(r);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    }
};
template <> struct Chunk<bf16_t, 8> {
    typedef uint4 raw;
    static __device__ __forceinline__ raw zero() { return make_uint4(0u, 0u, 0u, 0u); }
    static __device__ __forceinline__ raw load(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
    static __device__ __forceinline__ void cvt(raw r, float (&v)[8]) {   // bf16 -> fp32 is a 16-bit shift: exact
        v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xffff0000u);
        v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xffff0000u);
        v[4] = __uint_as_float(r.z << 16); v[5] = __uint_as_float(r.z & 0xffff0000u);
        v[6] = __uint_as_float(r.w << 16); v[7] = __uint_as_float(r.w & 0xffff0000u);
    }
};

struct LogitArgs {
    const void *P, *QZ, *RR;
    const float* a_att;
    int64_t ldp, ldqz, ldrr;
    const int32_t *col, *etype;
    const jmac_item_t* items;
    const int32_t* counts;
    int32_t n_items_max, d;
    float slope;
    float* s;                           // [E], slot order
};

// ---- pass 1: s[slot] for every CSR slot ------------------------------------------------------------------------------------
// Lane (es, sub) = (lane / G, lane % G) holds chunks sub, sub + G, .. of the edge its group works on; elements past d (the zero
// pad columns of padded bf16 rows) meet a zero a_att element.
template <typename TT, int CH, int G, int NCH>
__global__ __launch_bounds__(kBlock) void attn_logit_kernel(LogitArgs a) {
    typedef Chunk<TT, CH> C;
    typedef typename C::raw raw;
    constexpr int EPW = kWave / G;
    const int lane = lane_id(), sub = lane % G, es = lane / G;
    const TT* __restrict__ P = static_cast<const TT*>(a.P);
    const TT* __restrict__ QZ = static_cast<const TT*>(a.QZ);
    const TT* __restrict__ RR = static_cast<const TT*>(a.RR);
    const int nchunk = (a.d + CH - 1) / CH;
    int n_items = a.counts[0];
    if (n_items > a.n_items_max) n_items = a.n_items_max;

    bool on[NCH];
    float av[NCH][CH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int c = sub + k * G;
        on[k] = c < nchunk;
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int e = c * CH + j;
            av[k][j] = (on[k] && e < a.d) ? a.a_att[e] : 0.f;
        }
    }

    for (int it = blockIdx.x * kWaves + (int)(threadIdx.x >> 6); it < n_items; it += gridDim.x * kWaves) {
        const jmac_item_t x = a.items[it];
        if (x.end <= x.beg) continue;                                   // empty destination (wave-uniform)
        float pv[NCH][CH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const raw r = on[k] ? C::load(P + (int64_t)x.seg * a.ldp + (sub + k * G) * CH) : C::zero();
            C::cvt(r, pv[k]);
        }
        for (int base = x.beg; base < x.end; base += EPW * kU) {
            int slot[kU];
            bool ok[kU];
            raw q[kU][NCH], r[kU][NCH];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                slot[u] = base + u * EPW + es;
                ok[u] = slot[u] < x.end;
                const int sl = ok[u] ? slot[u] : x.beg;                 // idle groups repeat the item's first edge (no store)
                const int64_t j = a.col[sl], t = a.etype[sl];
#pragma unroll
                for (int k = 0; k < NCH; ++k) {
                    const int off = (sub + k * G) * CH;
                    q[u][k] = on[k] ? C::load(QZ + j * a.ldqz + off) : C::zero();
                    r[u][k] = on[k] ? C::load(RR + t * a.ldrr + off) : C::zero();
                }
            }
            float acc[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                acc[u] = 0.f;
#pragma unroll
                for (int k = 0; k < NCH; ++k) {
                    float qv[CH], rv[CH];
                    C::cvt(q[u][k], qv);
                    C::cvt(r[u][k], rv);
#pragma unroll
                    for (int j = 0; j < CH; ++j) acc[u] += av[k][j] * leaky(pv[k][j] + qv[j] - rv[j], a.slope);
                }
            }
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) {
#pragma unroll
                for (int u = 0; u < kU; ++u) acc[u] += __shfl_xor(acc[u], o, kWave);
            }
#pragma unroll
            for (int u = 0; u < kU; ++u)
                if (ok[u] && sub == 0) a.s[slot[u]] = acc[u];
        }
    }
}

// ---- pass 2: per destination ------------------------------------------------------------------------------------------------
struct SegArgs {
    const int32_t* rowptr;
    const int32_t* perm;                // original edge id of a slot, or NULL (outputs in slot order)
    const float* s;
    int32_t N, scale_by_degree;
    float *alpha, *logit, *entropy;
    int32_t* argmax;
};

// (weight, original edge id) of the running maximum: larger weight first, lower id among equal weights.  A total order, so the
// result does not depend on how the candidates are paired.
struct Best { float w; int32_t id; };
__device__ __forceinline__ Best better(Best a, Best b) { return (b.w > a.w || (b.w == a.w && b.id < a.id)) ? b : a; }
__device__ __forceinline__ Best wave_best(Best v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Best p;
        p.w = __shfl_xor(v.w, o, kWave);
        p.id = __shfl_xor(v.id, o, kWave);
        v = better(v, p);
    }
    return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// the three sweeps of one destination by NT threads starting at `tid`; RED reduces across them.  The denominator and the
// entropy sum are carried in double (O(E) work next to pass 1's O(E d)): a long row's weights then sum to 1 to fp32 rounding
template <int NT, class RED>
__device__ __forceinline__ void segment_body(const SegArgs& a, const int i, const int beg, const int end, const int tid, RED& red) {
    float m = -INFINITY;
    for (int x = beg + tid; x < end; x += NT) m = fmaxf(m, a.s[x]);
    m = red.max(m);
    double den = 0.0, wsum = 0.0;                                        // sum e, sum e * (s - m)
    for (int x = beg + tid; x < end; x += NT) {
        const float t = a.s[x] - m, e = expf(t);
        den += (double)e;
        wsum += (double)e * (double)t;
    }
    den = red.sum(den);
    wsum = red.sum(wsum);
    const double sq = a.scale_by_degree ? sqrt((double)(end - beg)) : 1.0;
    Best b{-1.f, INT32_MAX};
    for (int x = beg + tid; x < end; x += NT) {
        const float sx = a.s[x];
        const double al = (double)expf(sx - m) / den;                   // a single in-edge: 1 / 1
        const int32_t id = a.perm ? a.perm[x] : x;
        a.alpha[id] = (float)(al * sq);
        if (a.logit) a.logit[id] = sx;
        b = better(b, Best{(float)al, id});
    }
    if (a.argmax) {
        b = red.best(b);
        if (tid == 0) a.argmax[i] = b.id;
    }
    // -sum alpha log alpha with log alpha = (s - m) - log den
    if (a.entropy && tid == 0) a.entropy[i] = (float)(log(den) - wsum / den);
}

struct WaveRed {
    __device__ __forceinline__ float max(float v) { return wave_max(v); }
    __device__ __forceinline__ double sum(double v) { return wave_sum_d(v); }
    __device__ __forceinline__ Best best(Best v) { return wave_best(v); }
};

struct BlockRed {                      // wave results through LDS, read back in wave order by every thread
    float* f;
    double (*dd)[kWaves];
    Best* b;
    int n;                              // double rows used so far (each sum takes a fresh one: one barrier per reduction)
    __device__ __forceinline__ float max(float v) {
        v = wave_max(v);
        if (lane_id() == 0) f[threadIdx.x >> 6] = v;
        __syncthreads();
        float r = f[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) r = fmaxf(r, f[w]);
        return r;
    }
    __device__ __forceinline__ double sum(double v) {
        v = wave_sum_d(v);
        double* row = dd[n++];
        if (lane_id() == 0) row[threadIdx.x >> 6] = v;
        __syncthreads();
        double r = row[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) r += row[w];
        return r;
    }
    __device__ __forceinline__ Best best(Best v) {
        v = wave_best(v);
        if (lane_id() == 0) b[threadIdx.x >> 6] = v;
        __syncthreads();
        Best r = b[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) r = better(r, b[w]);
        return r;
    }
};

__global__ __launch_bounds__(kBlock) void attn_segment_wave_kernel(SegArgs a) {
    const int lane = lane_id();
    WaveRed red;
    for (int i = blockIdx.x * kWaves + (int)(threadIdx.x >> 6); i < a.N; i += gridDim.x * kWaves) {
        const int beg = a.rowptr[i], end = a.rowptr[i + 1];
        if (end - beg > kWaveSegMax) continue;                          // attn_segment_block_kernel's
        if (end <= beg) {
            if (lane == 0) {
                if (a.entropy) a.entropy[i] = 0.f;
                if (a.argmax) a.argmax[i] = -1;
            }
            continue;
        }
        segment_body<kWave>(a, i, beg, end, lane, red);
    }
}

// Long destinations are rare: every thread looks at one destination of a tile of kBlock (a scan by one thread per block is a
// chain of dependent loads as long as the tile count), the block then takes the flagged ones of its tile in index order.
__global__ __launch_bounds__(kBlock) void attn_segment_block_kernel(SegArgs a) {
    __shared__ float red_f[kWaves];
    __shared__ double red_d[2][kWaves];
    __shared__ Best red_b[kWaves];
    __shared__ int32_t is_long[kBlock];
    const int tid = (int)threadIdx.x;
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < a.N; base += (int64_t)gridDim.x * kBlock) {
        const int64_t mine = base + tid;
        is_long[tid] = mine < a.N && a.rowptr[mine + 1] - a.rowptr[mine] > kWaveSegMax;
        __syncthreads();
        for (int k = 0; k < kBlock; ++k) {
            if (!is_long[k]) continue;                                  // block-uniform
            const int i = (int)(base + k);
            BlockRed red{red_f, red_d, red_b, 0};
            segment_body<kBlock>(a, i, a.rowptr[i], a.rowptr[i + 1], tid, red);
            __syncthreads();                                            // the LDS rows are reused by the next destination
        }
        __syncthreads();                                                // ... and the flags by the next tile
    }
}

__global__ void attn_fill_empty_kernel(float* entropy, int32_t* argmax, int64_t N) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        if (entropy) entropy[i] = 0.f;
        if (argmax) argmax[i] = -1;
    }
}

template <typename TT, int CH>
void launch_logits(const LogitArgs& a, unsigned grid, hipStream_t st) {
    const int nchunk = (a.d + CH - 1) / CH;
    // lanes per edge x chunks per lane: the narrowest group that holds the row, three chunks per lane where a power of two wastes
    // more than a quarter of the lanes (75 fp32 chunks of d = 300: 32 x 3; 38 bf16 chunks of the padded 304: 16 x 3)
    if (nchunk <= 8) hipLaunchKernelGGL((attn_logit_kernel<TT, CH, 8, 1>), dim3(grid), dim3(kBlock), 0, st, a);
    else if (nchunk <= 16) hipLaunchKernelGGL((attn_logit_kernel<TT, CH, 16, 1>), dim3(grid), dim3(kBlock), 0, st, a);
    else if (nchunk <= 32) hipLaunchKernelGGL((attn_logit_kernel<TT, CH, 32, 1>), dim3(grid), dim3(kBlock), 0, st, a);
    else if (nchunk <= 48) hipLaunchKernelGGL((attn_logit_kernel<TT, CH, 16, 3>), dim3(grid), dim3(kBlock), 0, st, a);
    else if (nchunk <= 64) hipLaunchKernelGGL((attn_logit_kernel<TT, CH, 64, 1>), dim3(grid), dim3(kBlock), 0, st, a);
    else if (nchunk <= 96) hipLaunchKernelGGL((attn_logit_kernel<TT, CH, 32, 3>), dim3(grid), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((attn_logit_kernel<TT, CH, 64, 2>), dim3(grid), dim3(kBlock), 0, st, a);
}

size_t ws_bytes_needed(int64_t E) { return align_up((size_t)(E > 0 ? E : 0) * sizeof(float)) + 256; }

// dh: pitch of the Q half of a [Q|Z] / [Rq|Rz] row and width of a P row in elements (d, or the padded pitch of bf16 tables)
template <typename TT>
int launch_edge_weights(const TT* P, int64_t ldp, const TT* QZ, int64_t ldqz, const TT* RR, int64_t ldrr, int64_t dh,
                        const float* a_att, const int32_t* col, const int32_t* etype, const int32_t* perm, const jmac_view_t* v,
                        int64_t N, int64_t E, int64_t d, float slope, int32_t scale_by_degree, float* alpha, float* logit,
                        float* seg_entropy, int32_t* seg_argmax, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    if (N < 0 || E < 0 || !v || v->n_items_max < 0) return JMAC_EINVAL;
    if (N == 0) return E == 0 ? JMAC_OK : JMAC_EINVAL;
    if (!v->ptr) return JMAC_EINVAL;
    if (E > 0 && (!P || !QZ || !RR || !a_att || !col || !etype || !v->items || !v->counts || !alpha)) return JMAC_EINVAL;
    if (d <= 0 || d % 4 != 0 || d > 512 || ldp % 4 || ldqz % 4 || ldrr % 4) return JMAC_EDIM;
    if (dh < d || dh % 4 || ldp < dh || ldqz < dh || ldrr < dh) return JMAC_EDIM;
    if (N >= INT32_MAX || E >= INT32_MAX) return JMAC_ERANGE;
    if (E > 0 && (!ws || ws_bytes < ws_bytes_needed(E))) return JMAC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (E == 0) {
        if (seg_entropy || seg_argmax) {
            const unsigned g = (unsigned)((N + kBlock - 1) / kBlock < 1024 ? (N + kBlock - 1) / kBlock : 1024);
            hipLaunchKernelGGL(attn_fill_empty_kernel, dim3(g), dim3(kBlock), 0, st, seg_entropy, seg_argmax, N);
        }
        return (int)hipGetLastError();
    }
    LogitArgs a;
    a.P = P; a.QZ = QZ; a.RR = RR; a.a_att = a_att;
    a.ldp = ldp; a.ldqz = ldqz; a.ldrr = ldrr;
    a.col = col; a.etype = etype;
    a.items = v->items; a.counts = v->counts;
    a.n_items_max = (int32_t)(v->n_items_max < INT32_MAX ? v->n_items_max : INT32_MAX);
    a.d = (int32_t)d; a.slope = slope;
    a.s = static_cast<float*>(ws);
    if (a.n_items_max > 0) {
        const int64_t need = ((int64_t)a.n_items_max + kWaves - 1) / kWaves;
        const unsigned grid = (unsigned)(need < kLogitBlocksMax ? need : kLogitBlocksMax);
        if constexpr (sizeof(TT) == 4) {
            launch_logits<TT, 4>(a, grid, st);
        } else {
            // 16-byte lane loads where the rows and their halves allow them (the padded layout, or d % 8 == 0)
            const bool wide = ((((uintptr_t)P | (uintptr_t)QZ | (uintptr_t)RR) & 15) == 0) && ldp % 8 == 0 && ldqz % 8 == 0 &&
                              ldrr % 8 == 0 && dh % 8 == 0;
            if (wide) launch_logits<TT, 8>(a, grid, st); else launch_logits<TT, 4>(a, grid, st);
        }
    }
    SegArgs sa;
    sa.rowptr = v->ptr; sa.perm = perm; sa.s = a.s;
    sa.N = (int32_t)N; sa.scale_by_degree = scale_by_degree;
    sa.alpha = alpha; sa.logit = logit; sa.entropy = seg_entropy; sa.argmax = seg_argmax;
    const int64_t wneed = (N + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(attn_segment_wave_kernel, dim3((unsigned)(wneed < kSegWaveBlocksMax ? wneed : kSegWaveBlocksMax)), dim3(kBlock),
                       0, st, sa);
    const int64_t tiles = (N + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(attn_segment_block_kernel, dim3((unsigned)(tiles < kSegBlockBlocksMax ? tiles : kSegBlockBlocksMax)), dim3(kBlock),
                       0, st, sa);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t jmac_rel_attn_edge_weights_workspace_bytes(int64_t N, int64_t E) {
    (void)N;
    return ws_bytes_needed(E);
}

int jmac_rel_attn_edge_weights_f32(const float* P, int64_t ldp, const float* QZ, int64_t ldqz, const float* RR, int64_t ldrr,
                                   const float* a_att, const int32_t* col, const int32_t* etype, const int32_t* perm,
                                   const jmac_view_t* by_dst, int64_t N, int64_t E, int64_t d, float slope,
                                   int32_t scale_by_degree, float* alpha, float* logit, float* seg_entropy, int32_t* seg_argmax,
                                   void* ws, size_t ws_bytes, jmac_stream_t stream) {
    return launch_edge_weights<float>(P, ldp, QZ, ldqz, RR, ldrr, d, a_att, col, etype, perm, by_dst, N, E, d, slope,
                                      scale_by_degree, alpha, logit, seg_entropy, seg_argmax, ws, ws_bytes, stream);
}

int jmac_rel_attn_edge_weights_bf16(const uint16_t* P, int64_t ldp, const uint16_t* QZ, int64_t ldqz, const uint16_t* RR,
                                    int64_t ldrr, int64_t dh, const float* a_att, const int32_t* col, const int32_t* etype,
                                    const int32_t* perm, const jmac_view_t* by_dst, int64_t N, int64_t E, int64_t d, float slope,
                                    int32_t scale_by_degree, float* alpha, float* logit, float* seg_entropy,
                                    int32_t* seg_argmax, void* ws, size_t ws_bytes, jmac_stream_t stream) {
    return launch_edge_weights<bf16_t>(P, ldp, QZ, ldqz, RR, ldrr, dh, a_att, col, etype, perm, by_dst, N, E, d, slope,
                                       scale_by_degree, alpha, logit, seg_entropy, seg_argmax, ws, ws_bytes, stream);
}

}  // extern "C"
