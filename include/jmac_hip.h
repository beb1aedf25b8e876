/*
 * jmac_hip.h -- C ABI of libjmac_hip.so: the MI355X (gfx950) implementation of JMAC's relation-aware
 * GNN layer and triple / entity-pair scoring hot path.
 *
 * The reference (vinhsuhi/JMAC) is pure Python/PyTorch and has no FFI of its own; the seams this
 * library replaces are the Python call sites cited on every entry point below (paths relative to the
 * reference tree).  INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to contiguous row-major data unless the name starts with h_;
 *  - the caller owns every buffer; the library never allocates device memory.  Scratch space is
 *    passed in (`ws`, `ws_bytes`); its size comes from the matching *_workspace_bytes() function;
 *  - row tables carry a leading dimension in ELEMENTS (ld*): rows must be 16-byte aligned
 *    (ld % 4 == 0, base 16-B aligned) and d % 4 == 0, d <= 512 (the Python host pads d);
 *  - indices on the device side are int32 (edge / node / relation ids), sizes are int64;
 *    the reference's int64 edge lists are converted by jmac_csr_build;
 *  - every function takes the stream to launch on (pass torch.cuda.current_stream().cuda_stream),
 *    is asynchronous, never synchronises, and is hipGraph-capturable;
 *  - return value: 0 = ok, negative = JMAC_E* argument error, positive = hipError_t;
 *  - no global state; re-entrant; one host thread per device.
 */
#ifndef JMAC_HIP_H_
#define JMAC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* jmac_stream_t; /* hipStream_t */

#define JMAC_OK 0
#define JMAC_EINVAL (-1)    /* bad argument (null pointer, negative size)            */
#define JMAC_EDIM (-2)      /* unsupported d (d % 4 != 0 or d > 512) or ld           */
#define JMAC_EWORKSPACE (-3) /* workspace too small                                   */
#define JMAC_ERANGE (-4)    /* size exceeds int32 indexing                           */

/* A schedule item: one wavefront's unit of work = a run of at most `chunk` consecutive entries of one
 * segment (segment = destination node, source node or relation type).  pslot < 0: the item covers its
 * whole segment and finalises it; pslot >= 0: partial result slot, merged by the combine pass. */
typedef struct { int32_t seg, beg, end, pslot; } jmac_item_t;
/* A segment that was split over several items. */
typedef struct { int32_t seg, pslot0, nchunks, pad; } jmac_split_t;

const char* jmac_strerror(int rc);
int jmac_version(void);

/* ---------------------------------------------------------------------------------------------
 * Graph ingest (replaces: compute_norm's scatter_add degree, src/jmac_model.py:99-109; the implicit
 * COO edge lists of train.py:116-135 and src/utils.py:112-149).
 * --------------------------------------------------------------------------------------------- */

/* Bytes of scratch needed by jmac_csr_build / jmac_group_build for E entries and S segments. */
size_t jmac_graph_workspace_bytes(int64_t E, int64_t S);

/* Range check of an index array (elem_bytes = 4: int32, 8: int64): *bad (device int32, zeroed by the caller) +=
 * number of entries outside [lo, hi).  The reference raises IndexError on such an id (torch indexing); the kernels
 * of this library TRUST their indices, so a host that cannot vouch for them runs this first and reads *bad back
 * (jmac_amd does: once per graph at build time, once per index tensor for the loss / ranking entry points). */
int jmac_index_check(const void* idx, int32_t elem_bytes, int64_t n, int64_t lo, int64_t hi, int32_t* bad,
                     jmac_stream_t stream);

/* COO (edge_index [2,E] int64: row 0 = aggregation destination, row 1 = message source;
 * edge_type [E] int64) -> CSR by destination with a DETERMINISTIC order inside each row:
 *   nrel > 0 (types in [0, nrel)): by relation type, then input order (edges of a row that share a relation are
 *            neighbours: their [Rq|Rz] row is read once per group of gathers);
 *   nrel = 0: input order.
 *   rowptr [N+1], col [E] (source of each CSR slot), etype [E], perm [E] (original edge id).
 * Precondition: destinations in [0,N) (check with jmac_index_check; sources / types are range-checked against the
 * tables by the caller the same way). */
int jmac_csr_build(const int64_t* edge_index, const int64_t* edge_type, int64_t E, int64_t N, int64_t nrel,
                   int32_t* rowptr, int32_t* col, int32_t* etype, int32_t* perm,
                   void* ws, size_t ws_bytes, jmac_stream_t stream);

/* Generic stable grouping of E int32 keys in [0,S): ptr [S+1], order [E] (positions sorted by key).
 * Used for the by-source (CSC) and by-relation views of the CSR slots needed by the backward. */
int jmac_group_build(const int32_t* keys, int64_t E, int64_t S, int32_t* ptr, int32_t* order,
                     void* ws, size_t ws_bytes, jmac_stream_t stream);

/* Upper bounds for the arrays jmac_items_build fills (coop_min as passed to it; 0 = no cooperative splits). */
int64_t jmac_items_max(int64_t S, int64_t E, int32_t chunk, int32_t coop_min);   /* items          */
int64_t jmac_splits_max(int64_t E, int32_t chunk, int32_t coop_min);             /* split segments */
int64_t jmac_parts_max(int64_t E, int32_t chunk, int32_t coop_min);              /* partial slots  */

/* Cut segments (ptr [S+1]) into items (one wavefront's unit of work each).
 *   items [jmac_items_max], splits [jmac_splits_max],
 *   counts [8] = {n_items, n_splits, n_parts, n_empty, n_coop, 0, 0, 0}  (device ints: kernels read the counts, the
 *   host never has to).
 * Segment classes: empty (no entries); plain (<= chunk entries: one item, finalised by its wave); split (> chunk
 * entries: items of <= chunk entries each, merged by the combine pass); and, when coop_max > 0, cooperative
 * (coop_min < len <= coop_max: exactly 4 items of ceil(len/4) entries -- the four wavefronts of one workgroup, whose
 * partial results the forward kernel merges through LDS; for every other consumer they are ordinary split segments
 * with 4 partial slots).  coop_max = 0 disables the class (schedules of the backward's by-source / by-relation views,
 * large graphs).
 * Item order: [cooperative items, 4 per segment][split items][plain segments in segment order][the n_empty empty
 * segments]; the splits array lists the n_coop cooperative segments first (their .pad = 1). */
int jmac_items_build(const int32_t* ptr, int64_t S, int32_t chunk, int32_t coop_min, int32_t coop_max,
                     jmac_item_t* items, jmac_split_t* splits, int32_t* counts, void* ws, size_t ws_bytes,
                     jmac_stream_t stream);

/* item_edges [n_items_max][4] int32 = {col[beg], etype[beg], col[beg+1], etype[beg+1]} per item (-1 where the item is
 * shorter): the first two entries of an item inline with its header, optional input of the kernels on small graphs (one
 * dependent round trip fewer per wavefront).  By-destination schedule: col / etype of the CSR (forward, backward pass A).
 * By-source / by-relation schedules: pass `order` as col and the view's `entry_dst` as etype (backward passes B / C). */
int jmac_item_edges_build(const jmac_item_t* items, const int32_t* counts, int64_t n_items_max,
                          const int32_t* col, const int32_t* etype, int32_t* item_edges,
                          jmac_stream_t stream);

/* One schedule over the CSR slots: the CSR by destination itself (order = NULL) or a regrouping of its slots by source /
 * by relation (jmac_group_build), cut into items by jmac_items_build.  n_*_max: array bounds (the exact counts after a
 * host read of `counts`, or the jmac_*_max upper bounds).  n_empty / n_coop: HOST copies of counts[3] / counts[4] -- exact
 * values (read `counts` back once after jmac_items_build; 0 / 0 for a schedule built with coop_max = 0 whose empty
 * segments need not be packed): they fix the launch geometry of the forward kernel without a device-side wait. */
typedef struct {
    const int32_t* ptr;          /* [S+1]                         */
    const int32_t* order;        /* [E] CSR slot per entry, or NULL for the CSR itself */
    const jmac_item_t* items;
    const jmac_split_t* splits;
    const int32_t* counts;       /* device {n_items,n_splits,n_parts,n_empty,n_coop,0,0,0} */
    int64_t n_items_max, n_splits_max, n_parts_max;
    const int32_t* item_edges;   /* jmac_item_edges_build's array for `items`, or NULL */
    int64_t n_empty, n_coop;
    const int32_t* entry_dst;    /* by-source / by-relation views: destination node of every entry IN GROUPED ORDER
                                  * (= dst_of_slot[order[x]]; saves the backward a dependent load), or NULL */
} jmac_view_t;

/* ---------------------------------------------------------------------------------------------
 * Relation-aware attention aggregation (replaces: MessagePassing.propagate + message + scatter_,
 * modules/helper/message_passing.py:4-29,55-90 and src/jmac_model.py:56-89; the self-loop
 * propagate of src/jmac_model.py:44-45,50; the (nb+self)/2 of :52), in the factorised form
 *     h_e = P[i] + Q[j] - Rq[t]        s_e = a . LeakyReLU(h_e)      alpha = softmax over in(i)
 *     out[i] = out_scale * ( sqrt(deg_i) * sum_e alpha_e (Z[j] - Rz[t])  +  [Z[i] - Rz[loop]] )
 * for edges e = (i <- j, type t).  Tables: P [N,d] (ldp); QZ [N,2d] = Q|Z per node (ldqz);
 * RR [nr+1,2d] = Rq|Rz per relation (ldrr); a_att [d].  loop_rel < 0 drops the bracketed self term.
 * seg_max/seg_den [N] receive the per-destination softmax max / denominator for the backward.
 * Destinations (rows of P / out, N of them) and sources (rows of QZ, Nsrc >= max(col)+1 of them) may be
 * different index spaces (destination-sharded multi-GPU: P holds the rank's rows, QZ the all-gathered
 * table); the fused self term (loop_rel >= 0) reads QZ[self_off + i]: self_off = 0 when the two spaces coincide,
 * = the row of the gathered table that holds the rank's destination 0 when the destinations are a slice of it.
 * by_dst: the schedule over the CSR rows (by_dst->ptr = rowptr [N+1], order = NULL).
 * --------------------------------------------------------------------------------------------- */
size_t jmac_rel_attn_fwd_workspace_bytes(int64_t n_parts_max, int64_t d);

int jmac_rel_attn_aggregate_fwd_f32(
    const float* P, int64_t ldp, const float* QZ, int64_t ldqz, const float* RR, int64_t ldrr,
    const float* a_att, const int32_t* col, const int32_t* etype, const jmac_view_t* by_dst,
    int64_t N, int64_t d, float slope, int32_t loop_rel, int64_t self_off, float out_scale,
    float* out, int64_t ldo, float* seg_max, float* seg_den,
    void* ws, size_t ws_bytes, jmac_stream_t stream);

/* Same op with bf16 TABLES (P, QZ, RR: raw bf16 bits, rows 8-byte aligned: ld % 4 == 0, d % 4 == 0);
 * a_att, the logits, the softmax, the accumulators and every output stay fp32 ("keep
 * P/Q/Z tables bf16 but logits, softmax, accumulators ... in fp32").  Halves the gathered bytes of
 * the HBM-bound kernel; forward only (BASELINE config 3: bf16 union-graph scoring is inference). */
int jmac_rel_attn_aggregate_fwd_bf16(
    const uint16_t* P, int64_t ldp, const uint16_t* QZ, int64_t ldqz, const uint16_t* RR, int64_t ldrr,
    const float* a_att, const int32_t* col, const int32_t* etype, const jmac_view_t* by_dst,
    int64_t N, int64_t d, float slope, int32_t loop_rel, int64_t self_off, float out_scale,
    float* out, int64_t ldo, float* seg_max, float* seg_den,
    void* ws, size_t ws_bytes, jmac_stream_t stream);

/* The same on bf16 tables whose row halves are PADDED to `dh` elements (dh >= d, dh % 8 == 0: 16-byte aligned halves, e.g.
 * d = 300 -> dh = 304): P rows hold dh elements, a [Q|Z] / [Rq|Rz] row is Q at 0 and Z at dh (2 dh elements), pad columns
 * are ZERO (the host pads the projection weights, so the GEMM writes them).  With (d, dh) = (300, 304) or (256, 256) and
 * 16-byte aligned rows the persistent-grid form of the kernel (large graphs) takes 16 bytes per lane and two edges per wave
 * instruction (half a wave per edge) -- the 8-byte lane loads of the unpadded d = 300 layout run at 0.54-0.70 x the 16-byte
 * rate; every other case reads the same layout with the 64-lane map (dh % 4 == 0).  out stays [N, d] fp32. */
int jmac_rel_attn_aggregate_fwd_bf16_padded(const uint16_t* P, int64_t ldp, const uint16_t* QZ, int64_t ldqz,
                                            const uint16_t* RR, int64_t ldrr, int64_t dh, const float* a_att,
                                            const int32_t* col, const int32_t* etype, const jmac_view_t* by_dst,
                                            int64_t N, int64_t d, float slope, int32_t loop_rel, int64_t self_off,
                                            float out_scale, float* out, int64_t ldo, float* seg_max, float* seg_den,
                                            void* ws, size_t ws_bytes, jmac_stream_t stream);

/* Up to TWO independent calls of jmac_rel_attn_aggregate_fwd_f32 as ONE launch (round 5): the first two layers of
 * JMAC.forward_name (conv1_alignment, conv1_completion: src/jmac_model.py:183,190) read different tables / weights / loop rows but
 * the same graph and do not depend on each other; at DBP-5L size each launch is a chain of dependent round trips with most of the
 * chip idle.  A job = the arguments of the single call.  Jobs whose form is the one-wave-per-item kernel (small graphs, fp32)
 * share a grid (blocks [0, g0) job 0, the rest job 1); any other pair runs as two launches.  Results: those of the single calls,
 * bit for bit. */
typedef struct {
    const float *P; int64_t ldp; const float *QZ; int64_t ldqz; const float *RR; int64_t ldrr; const float *a_att;
    const int32_t *col, *etype; const jmac_view_t *by_dst; int64_t N, d; float slope; int32_t loop_rel; int64_t self_off;
    float out_scale; float *out; int64_t ldo; float *seg_max, *seg_den; void *ws; size_t ws_bytes;
} jmac_agg_fwd_job_t;
int jmac_rel_attn_aggregate_fwd_jobs_f32(const jmac_agg_fwd_job_t* jobs, int32_t n_jobs, jmac_stream_t stream);

/* Attention export: the per-edge softmax weights of the layer above, which its forward kernel folds into an online softmax
 * and never writes (the reference computes them as scatter_softmax(s, dst) of the neighbour branch, src/jmac_model.py:71-89 and
 * modules/helper/message_passing.py:24-28).  On the same factorised tables, for an edge e = (i <- j, type t):
 *     h_e = P[i] + Q[j] - Rq[t]          s_e = sum_k a_k LeakyReLU_slope(h_e[k])          (the forward kernel's logit)
 *     alpha_e = exp(s_e - m_i) / sum_{e' in in(i)} exp(s_e' - m_i),   m_i = max over in(i)   (sums to 1 over a non-empty i)
 *     scale_by_degree != 0: alpha_e * sqrt(deg_i)      (what message_passing.py:26 multiplies the messages with)
 *     seg_entropy[i] = -sum_e alpha_e log alpha_e      (0 for an empty destination; always of the UNscaled alpha)
 *     seg_argmax[i]  = ORIGINAL edge id of the largest alpha of destination i, ties -> the lowest original edge id; -1 for an
 *                      empty destination
 * alpha [E] and logit [E] (may be NULL) are in the CALLER's edge order: the value of CSR slot x goes to position perm[x]
 * (jmac_csr_build's perm; NULL: slot order, and seg_argmax holds slots).  The self-loop branch (src/jmac_model.py:50) is not
 * exported: one edge per node and no norm, its weight is identically 1.  Only the Q half of QZ and the Rq half of RR are read.
 * by_dst: the forward's schedule over the CSR rows (ptr = rowptr [N+1]); col / etype [E] as there.  seg_entropy [N] and
 * seg_argmax [N] may be NULL.  Read-only on every input, fp32 logits / softmax / outputs, fixed-order reductions and no float
 * atomics: bitwise reproducible.  Checks, in this order: null pointers, negative sizes (JMAC_EINVAL); d % 4 != 0, d > 512,
 * ld % 4 != 0, ld < dh (JMAC_EDIM); N or E >= 2^31 - 1 (JMAC_ERANGE); ws (JMAC_EWORKSPACE).  E == 0: seg_entropy = 0,
 * seg_argmax = -1, JMAC_OK.
 * The _bf16 form reads bf16 tables in the padded layout of jmac_rel_attn_aggregate_fwd_bf16_padded (P rows of dh elements, Q
 * at 0 of a [Q|Z] row, pad columns zero; dh == d: unpadded); 16-byte lane loads where dh % 8 == 0 and the rows are 16-byte
 * aligned, 8-byte ones otherwise. */
size_t jmac_rel_attn_edge_weights_workspace_bytes(int64_t N, int64_t E);

int jmac_rel_attn_edge_weights_f32(const float* P, int64_t ldp, const float* QZ, int64_t ldqz, const float* RR, int64_t ldrr,
                                   const float* a_att, const int32_t* col, const int32_t* etype, const int32_t* perm,
                                   const jmac_view_t* by_dst, int64_t N, int64_t E, int64_t d, float slope,
                                   int32_t scale_by_degree, float* alpha, float* logit, float* seg_entropy, int32_t* seg_argmax,
                                   void* ws, size_t ws_bytes, jmac_stream_t stream);

int jmac_rel_attn_edge_weights_bf16(const uint16_t* P, int64_t ldp, const uint16_t* QZ, int64_t ldqz, const uint16_t* RR,
                                    int64_t ldrr, int64_t dh, const float* a_att, const int32_t* col, const int32_t* etype,
                                    const int32_t* perm, const jmac_view_t* by_dst, int64_t N, int64_t E, int64_t d, float slope,
                                    int32_t scale_by_degree, float* alpha, float* logit, float* seg_entropy,
                                    int32_t* seg_argmax, void* ws, size_t ws_bytes, jmac_stream_t stream);

/* Merge of per-source-chunk partial aggregations: the slab-pipelined exchange of the destination-sharded layer
 * (jmac_amd/dist.py; the reference has one process and no exchange: modules/helper/message_passing.py:24,28 are the
 * per-destination softmax / sum that make the partials mergeable).  Part c = the forward above on the edges whose SOURCE is
 * in chunk c (loop_rel < 0, out_scale 1): out_c [N,d], its seg_max_c / seg_den_c [N], and the chunk graph's rowptr_c [N+1]
 * (in-degree within the chunk).  Writes out [N,d] = out_scale * (nb + self), nb = sqrt(deg) * sum_e softmax(e) x_e over ALL
 * edges, self = Zself[i] - rz_loop (the fused self loop, src/jmac_model.py:49-50; Zself NULL: none), and the whole graph's
 * seg_max / seg_den (what jmac_rel_attn_aggregate_bwd_f32 on the whole graph expects).  h_* are HOST arrays of n_parts
 * device pointers (n_parts <= JMAC_MERGE_MAX_PARTS); parts are combined in index order (bitwise reproducible). */
#define JMAC_MERGE_MAX_PARTS 16
int jmac_softmax_parts_merge_f32(const float* const* h_out, int64_t ldo, const float* const* h_seg_max,
                                 const float* const* h_seg_den, const int32_t* const* h_rowptr, int32_t n_parts,
                                 int64_t N, int64_t d, const float* Zself, int64_t ldz, const float* rz_loop,
                                 float out_scale, float* out, int64_t ldo2, float* seg_max, float* seg_den,
                                 jmac_stream_t stream);

/* Backward of the op above (replaces autograd through the same reference lines).
 *   G [N,d] (ldg) = dL/dout;  outputs: dP [N,d] (lddp), dQZ [N,2d] (lddqz), dRR [nr+1,2d] (lddrr),
 *   da [d].  All outputs are fully written (no pre-zeroing needed).
 * mode 0 ("atomic"): one pass by destination, float atomics into dQZ / dRR.
 * mode 1 ("deterministic", default): pass A by destination writes per-edge records, pass B by source
 *   and pass C by relation sum them with plain stores: bitwise reproducible, no atomics.
 *   Needs the by-source view (sptr [N+1], sorder [E], sitems ...) and the by-relation view
 *   (tptr [nrel+1], torder [E], titems ...) of the CSR slots, built with jmac_group_build +
 *   jmac_items_build. dst_of_slot [E] = destination node of each CSR slot. */
size_t jmac_rel_attn_bwd_workspace_bytes(int64_t N, int64_t E, int64_t nrel, int64_t d,
                                         int64_t n_parts_max_dst, int64_t n_parts_max_src,
                                         int64_t n_parts_max_rel, int32_t mode);

int jmac_rel_attn_aggregate_bwd_f32(
    const float* P, int64_t ldp, const float* QZ, int64_t ldqz, const float* RR, int64_t ldrr,
    const float* a_att, const int32_t* col, const int32_t* etype, const int32_t* dst_of_slot,
    const jmac_view_t* by_dst, const jmac_view_t* by_src, const jmac_view_t* by_rel,
    int64_t N, int64_t Nsrc, int64_t E, int64_t nrel, int64_t d, float slope, int32_t loop_rel,
    int64_t self_off, float out_scale, const float* out, int64_t ldo, const float* seg_max, const float* seg_den,
    const float* G, int64_t ldg,
    float* dP, int64_t lddp, float* dQZ, int64_t lddqz, float* dRR, int64_t lddrr, float* da,
    int32_t mode, void* ws, size_t ws_bytes, jmac_stream_t stream);

/* The deterministic backward above in separately callable PHASES (bit mask; 15 = the whole backward = the call above, mode 1):
 *   1 = pass A by destination (dP of plain destinations, the per-edge records in ws, da / column-sum partials)
 *   2 = pass B by source (d[Q|Z], + the merge of its split sources)       4 = pass C by relation (d[Rq|Rz], + its merge)
 *   8 = the merges that hang on pass A alone: dP of split destinations, da, dRz[loop] (run with or after phase 4)
 * The same ws (sized for the whole graph's views by jmac_rel_attn_bwd_workspace_bytes) must be passed to every call of one
 * backward: the records pass A leaves in it are read by passes B and C.
 * A phase-2 call may cover a SLAB of the source rows, so that a destination-sharded layer can reduce-scatter slab c of d[Q|Z]
 * over xGMI while pass B works on slab c+1 (jmac_amd.dist; adjoint of the all-gather in front of
 * modules/helper/message_passing.py:24,28): by_src = a view built by jmac_items_build on the slab's slice of the by-source
 * segment pointer (segments numbered from the slab's first row; `order` / `entry_dst` the whole graph's), dQZ = the slab's first
 * row, Nsrc = its rows, self_off = (whole-table self_off) - (slab's first row): negative or past the slab where the rank's own
 * rows lie elsewhere. */
int jmac_rel_attn_aggregate_bwd_phases_f32(
    const float* P, int64_t ldp, const float* QZ, int64_t ldqz, const float* RR, int64_t ldrr,
    const float* a_att, const int32_t* col, const int32_t* etype, const int32_t* dst_of_slot,
    const jmac_view_t* by_dst, const jmac_view_t* by_src, const jmac_view_t* by_rel,
    int64_t N, int64_t Nsrc, int64_t E, int64_t nrel, int64_t d, float slope, int32_t loop_rel,
    int64_t self_off, float out_scale, const float* out, int64_t ldo, const float* seg_max, const float* seg_den,
    const float* G, int64_t ldg,
    float* dP, int64_t lddp, float* dQZ, int64_t lddqz, float* dRR, int64_t lddrr, float* da,
    int32_t phases, void* ws, size_t ws_bytes, jmac_stream_t stream);

/* BatchNorm1d (batch statistics or running statistics) + tanh on [N,d]
 * (replaces: self.layer_act(self.bn(.)), src/jmac_model.py:52).
 * training != 0: mean/var are computed over the N rows (biased var), written to save_mean /
 * save_invstd [d], and running_mean/var (may be NULL) are updated with `momentum` (unbiased var).
 * The layer's output is an operand of two concatenations in JMAC.forward_name (src/jmac_model.py:192 cat(comp_l1, align_l1)
 * and :203 cat(align_layers)): the forward writes the rows into both cat buffers (y2 / ldy2, may be NULL), the backward sums
 * the two incoming gradients (gy2 / ldgy2, may be NULL) while it reads them -- no cat copy, no gradient add. */
size_t jmac_bn_tanh_workspace_bytes(int64_t N, int64_t d);
int jmac_bn_tanh_fwd2_f32(const float* x, int64_t ldx, int64_t N, int64_t d, const float* weight,
                          const float* bias, float* running_mean, float* running_var,
                          int32_t training, float momentum, float eps, float* y, int64_t ldy,
                          float* y2, int64_t ldy2, float* save_mean, float* save_invstd, void* ws,
                          size_t ws_bytes, jmac_stream_t stream);
int jmac_bn_tanh_bwd2_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* gy,
                          int64_t ldgy, const float* gy2, int64_t ldgy2, int64_t N, int64_t d,
                          const float* weight, const float* save_mean, const float* save_invstd,
                          int32_t training, float* gx, int64_t ldgx, float* gweight, float* gbias,
                          void* ws, size_t ws_bytes, jmac_stream_t stream);

/* Segmented form (train mode): the N rows are a STACK of `nblocks` row blocks, h_blk_ptr [nblocks+1] (HOST array, h_blk_ptr[0] = 0)
 * -- the KGs of one launch set.  The reference's training step encodes two KGs per batch with one set of layer weights
 * (src/jmac_model.py:325-326, 263-264: forward_base(graph1), forward_base(graph2)); each of those calls normalises with the
 * batch statistics of ITS rows and moves the layer's running estimates once.  Here every block gets its own statistics
 * (save_mean / save_invstd [nblocks, d]); weight / bias / running_mean / running_var are the layer's; the running estimates
 * are updated block after block in the order h_order [nblocks] (HOST; NULL = 0,1,2,...; a permutation: the reference's
 * call order), i.e. r <- (1-m)((1-m) r + m b_first) + m b_second ...; the caller bumps num_batches_tracked by nblocks.
 * The backward sums grad weight / grad bias over the blocks (shared parameters) and applies every block's own sums and
 * row count.  nblocks <= JMAC_BN_MAX_BLOCKS; blocks must be non-empty. */
#define JMAC_BN_MAX_BLOCKS 16
size_t jmac_bn_tanh_seg_workspace_bytes(int32_t nblocks, int64_t d);
int jmac_bn_tanh_seg_fwd2_f32(const float* x, int64_t ldx, int64_t d, int32_t nblocks, const int64_t* h_blk_ptr,
                              const int32_t* h_order, const float* weight, const float* bias,
                              float* running_mean, float* running_var, float momentum, float eps, float* y,
                              int64_t ldy, float* y2, int64_t ldy2, float* save_mean, float* save_invstd,
                              void* ws, size_t ws_bytes, jmac_stream_t stream);
int jmac_bn_tanh_seg_bwd2_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* gy,
                              int64_t ldgy, const float* gy2, int64_t ldgy2, int64_t d, int32_t nblocks,
                              const int64_t* h_blk_ptr, const float* weight, const float* save_mean,
                              const float* save_invstd, float* gx, int64_t ldgx, float* gweight, float* gbias,
                              void* ws, size_t ws_bytes, jmac_stream_t stream);

/* Phased forms of the same BatchNorm + tanh for batch statistics that span several ranks (destination-sharded
 * layer): the caller combines the per-rank moments / sums between the phases (torch.distributed over RCCL).
 *   forward : jmac_col_moments_f32 -> mean[d], m2[d] = sum (x - mean)^2 of THIS rank's N rows
 *             [all-gather, Chan's parallel combination -> global mean, invstd]
 *             jmac_bn_tanh_apply_f32
 *   backward: jmac_bn_tanh_bwd_sums_f32 -> sums[0:d] = sum gz, sums[d:2d] = sum gz*xhat over this rank's rows
 *             (gz = gy (1 - y^2); these are also the rank's contributions to grad bias / grad weight)
 *             [all-reduce]   jmac_bn_tanh_bwd_apply_f32 with the global sums and the global row count n_total. */
int jmac_col_moments_f32(const float* x, int64_t ldx, int64_t N, int64_t d, float* mean, float* m2,
                         void* ws, size_t ws_bytes, jmac_stream_t stream);
int jmac_bn_tanh_apply_f32(const float* x, int64_t ldx, int64_t N, int64_t d, const float* weight,
                           const float* bias, const float* mean, const float* invstd, float* y,
                           int64_t ldy, jmac_stream_t stream);
int jmac_bn_tanh_bwd_sums_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* gy,
                              int64_t ldgy, int64_t N, int64_t d, const float* mean,
                              const float* invstd, float* sums, void* ws, size_t ws_bytes,
                              jmac_stream_t stream);
int jmac_bn_tanh_bwd_apply_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* gy,
                               int64_t ldgy, int64_t N, int64_t d, const float* weight,
                               const float* mean, const float* invstd, const float* sums,
                               int64_t n_total, float* gx, int64_t ldgx, jmac_stream_t stream);

/* Row L2 normalisation  y = x / max(||x||_2, eps)  (replaces F.normalize(x, 2, -1) of JMAC.forward_name and get_emb,
 * src/jmac_model.py:179,191,227-228; eps = 1e-12 is torch's default).  inv [N] receives 1 / max(||x_r||, eps) for the
 * backward:  gx = inv (g - y (g.y)),  or inv g on rows whose norm was clamped.  Any d and leading dimensions. */
int jmac_row_normalize_fwd_f32(const float* x, int64_t ldx, int64_t N, int64_t d, float eps, float* y,
                               int64_t ldy, float* inv, jmac_stream_t stream);
int jmac_row_normalize_bwd_f32(const float* y, int64_t ldy, const float* g, int64_t ldg, const float* inv,
                               int64_t N, int64_t d, float eps, float* gx, int64_t ldgx,
                               jmac_stream_t stream);

/* completion_dropout(F.normalize(x)) in one pass each way (src/jmac_model.py:179,191).  mask [N,d] holds the caller's
 * {0,1} Bernoulli draws (NULL: no dropout), scale = 1/(1-p); y may be a strided slice of a cat buffer.  The backward keeps
 * only inv [N] from the forward and recomputes the normalised row from x:  gx (+)= d/dx of the forward applied to g
 * (accumulate != 0 adds into gx).  d % 4 == 0, leading dimensions % 4 == 0, 16-byte aligned bases. */
int jmac_row_normalize_drop_fwd_f32(const float* x, int64_t ldx, int64_t N, int64_t d, float eps,
                                    const float* mask, int64_t ldm, float scale, float* y, int64_t ldy,
                                    float* inv, jmac_stream_t stream);
int jmac_row_normalize_drop_bwd_f32(const float* x, int64_t ldx, const float* inv, const float* mask,
                                    int64_t ldm, float scale, const float* g, int64_t ldg, int64_t N,
                                    int64_t d, float eps, float* gx, int64_t ldgx, int32_t accumulate,
                                    jmac_stream_t stream);

/* The same with the Bernoulli draws made INSIDE the kernels (torch's F.dropout draws them with its own Philox stream: the
 * draws are equally i.i.d. Bernoulli(1 - p_drop) but not the same bits).  seed: ONE device-resident int64 the caller fills from
 * its generator (a device value, so that a captured step draws a fresh mask on every replay); element (r, c) is kept iff word
 * c % 4 of Philox4x32-10(key = seed, counter = r * d/4 + c/4) < (1 - p_drop) * 2^32, kept elements are scaled by 1/(1 - p_drop).
 * The backward regenerates the draws from the same seed: no mask tensor exists.  0 <= p_drop < 1. */
int jmac_row_normalize_dropseed_fwd_f32(const float* x, int64_t ldx, int64_t N, int64_t d, float eps,
                                        const int64_t* seed, float p_drop, float* y, int64_t ldy,
                                        float* inv, jmac_stream_t stream);
int jmac_row_normalize_dropseed_bwd_f32(const float* x, int64_t ldx, const float* inv, const int64_t* seed,
                                        float p_drop, const float* g, int64_t ldg, int64_t N, int64_t d,
                                        float eps, float* gx, int64_t ldgx, int32_t accumulate,
                                        jmac_stream_t stream);

/* Fused row passes of the encoder node's completion chain (jmac_amd/encoder.py, FUSE_ROW_PASSES): the normalise + dropout passes
 * above folded into the launch that produces their input or consumes their output, with an optional row permutation on the way.
 * Common to the four: d % 4 == 0 and d <= 512 (a wave holds whole rows in registers), leading dimensions % 4 == 0, 16-byte
 * aligned bases; seed as for jmac_row_normalize_dropseed_*_f32, NULL = no dropout; the draws are indexed by the row r the
 * kernel works on (NOT by row_map[r]); row_map [N] int64 device (may be NULL = identity), entries in [0, N) -- not checked.
 *
 * jmac_rows_normalize_dropseed_fwd_f32: row r of the result is x[row_map[r]]: the gathered rows themselves -> x_rows (may be NULL),
 *   their normalised + dropped form -> y, 1 / max(||row||, eps) -> inv.  The bits of a jmac_rows_compact_f32 gather followed by
 *   jmac_row_normalize_dropseed_fwd_f32.
 * jmac_bn_tanh_normalize_dropseed_fwd_f32: jmac_bn_tanh_fwd2_f32 (same statistics launches, same arguments up to ldy) whose apply
 *   pass also writes row r to y_rows[row_map[r]] (both NULL or both given) and the normalised + dropped row (norm taken from the
 *   registers) to yn, inv [N].  The bits of jmac_bn_tanh_fwd2_f32, a gather and jmac_row_normalize_dropseed_fwd_f32 of y.
 * jmac_bn_tanh_bwd_normadj_f32: jmac_bn_tanh_bwd2_f32 whose first incoming gradient is not a table but the adjoint that
 *   jmac_row_normalize_dropseed_bwd_f32(x = y, inv, seed, p_drop, g) would write, formed per row in registers by both of its
 *   passes; the second one (may be NULL) is read as gy2[row_map[r]].  The column sums keep jmac_bn_tanh_bwd2_f32's
 *   association: the bits of the adjoint launch, a gather of gy2 and jmac_bn_tanh_bwd2_f32.
 * jmac_row_normalize_dropseed_bwd_rows_f32: dst[row_map[r]] (+)= adjoint of row r (as jmac_row_normalize_dropseed_bwd_f32)
 *   + add[r] (may be NULL); accumulate != 0 adds onto dst.  dst must not alias the inputs.  The bits of the accumulating
 *   adjoint launch followed by jmac_rows_expand_f32. */
int jmac_rows_normalize_dropseed_fwd_f32(const float* x, int64_t ldx, const int64_t* row_map, int64_t N, int64_t d,
                                         float eps, const int64_t* seed, float p_drop, float* x_rows, int64_t ldxr,
                                         float* y, int64_t ldy, float* inv, jmac_stream_t stream);
int jmac_bn_tanh_normalize_dropseed_fwd_f32(const float* x, int64_t ldx, int64_t N, int64_t d, const float* weight,
                                            const float* bias, float* running_mean, float* running_var,
                                            int32_t training, float momentum, float eps, float* y, int64_t ldy,
                                            const int64_t* row_map, float* y_rows, int64_t ldyr, float norm_eps,
                                            const int64_t* seed, float p_drop, float* yn, int64_t ldyn, float* inv,
                                            float* save_mean, float* save_invstd, void* ws, size_t ws_bytes,
                                            jmac_stream_t stream);
int jmac_bn_tanh_bwd_normadj_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* inv,
                                 const float* g, int64_t ldg, float norm_eps, const int64_t* seed, float p_drop,
                                 const float* gy2, int64_t ldgy2, const int64_t* row_map, int64_t N, int64_t d,
                                 const float* weight, const float* save_mean, const float* save_invstd,
                                 int32_t training, float* gx, int64_t ldgx, float* gweight, float* gbias, void* ws,
                                 size_t ws_bytes, jmac_stream_t stream);
int jmac_row_normalize_dropseed_bwd_rows_f32(const float* x, int64_t ldx, const float* inv, const int64_t* seed,
                                             float p_drop, const float* g, int64_t ldg, const float* add,
                                             int64_t ldadd, const int64_t* row_map, int64_t N, int64_t d, float eps,
                                             float* dst, int64_t lddst, int32_t accumulate, jmac_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Completion scoring (replaces: torch.cdist(er, all_kg_emb, p=1), src/jmac_model.py:312; the
 * filter/sort/np.where ranking loop of src/validate.py:50-64).
 * --------------------------------------------------------------------------------------------- */
/* out[b,n] (+)= sum_k |er[b,k] - table[n,k]|;  accumulate != 0 adds to out (layer loop of :302). */
int jmac_l1_score_f32(const float* er, int64_t lder, const float* table, int64_t ldt, int64_t B,
                      int64_t N, int64_t d, float* out, int64_t ldout, int32_t accumulate,
                      jmac_stream_t stream);
/* Same with bf16 operands (raw bits; rows 8-byte aligned), fp32 accumulation and output
 * (BASELINE config 3: bf16 entity tables scored against all entities of the union graph). */
int jmac_l1_score_bf16(const uint16_t* er, int64_t lder, const uint16_t* table, int64_t ldt, int64_t B,
                       int64_t N, int64_t d, float* out, int64_t ldout, int32_t accumulate,
                       jmac_stream_t stream);

/* Fused link prediction (replaces: forward_linkpred's layer loop src/jmac_model.py:302-313 TOGETHER WITH the ranking loop of
 * src/validate.py:50-64, for callers that want the ranks and not the [B,N] matrix -- CompletionEvaluator.test):
 *     dist[b,n] = sum over layers l of || (ent_l[h[b]] +/- rel_l[r[b]]) - table_l[n] ||_1      (pred_head != 0: minus)
 *     rank[b]   = 1 + #{n in [0,N): dist[b,n] before dist[b,gold[b]]} - #{filtered n != gold[b]: dist[b,n] before ...}
 * with "before" = smaller, or equal and lower index, exactly as jmac_filtered_rank_f32.  The distance is ONE running fp32 sum
 * over (layer, k) -- the materialised path rounds once more per layer (out += layer), so the two agree to fp32 rounding and
 * give the same rank wherever the gold is not tied with a neighbour at that level.  ent / rel: fp32 tables the query rows are
 * gathered from; table: the N candidate rows, fp32 (== ent) for _f32, raw bf16 for _bf16 (the query rows are then rounded to
 * bf16 as well: BASELINE config 3).  n_layers <= 4, n_layers * d <= ~15 000 (the prep kernel stages candidate rows through
 * 60 KB of LDS; JMAC_ERANGE beyond), d <= 512.  The [B,N] matrix is never written. */
typedef struct {
    const float* ent;  int64_t ld_ent;      /* [*, d] */
    const float* rel;  int64_t ld_rel;      /* [*, d] */
    const void* table; int64_t ld_table;    /* [N, d] fp32 or bf16 */
} jmac_link_layer_t;
size_t jmac_linkpred_rank_workspace_bytes(int64_t B, int64_t d, int32_t n_layers);
int jmac_linkpred_rank_f32(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r,
                           int32_t pred_head, const int32_t* gold, const int32_t* filt_ptr, const int32_t* filt_idx,
                           int64_t B, int64_t N, int64_t d, int32_t* rank, void* ws, size_t ws_bytes, jmac_stream_t stream);
int jmac_linkpred_rank_bf16(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r,
                            int32_t pred_head, const int32_t* gold, const int32_t* filt_ptr, const int32_t* filt_idx,
                            int64_t B, int64_t N, int64_t d, int32_t* rank, void* ws, size_t ws_bytes, jmac_stream_t stream);

/* The known tails of every (head, relation) as a sorted CSR on the device (jmac_amd.sampling.TrueTailIndex): the filter of a
 * whole run, built once, instead of one CSR per batch.  key[i] = h << 32 | r, strictly ascending; the tails of key i are
 * tail_idx[tail_ptr[i] .. tail_ptr[i+1]), ascending and distinct, in the row space of the candidate table.  For head
 * prediction the caller builds it from the triples' columns (t, r, h). */
typedef struct {
    const int64_t* key;        /* [n_keys] ascending (h << 32 | r) */
    int64_t        n_keys;
    const int32_t* tail_ptr;   /* [n_keys + 1] */
    const int32_t* tail_idx;   /* ascending within a key */
} jmac_tail_index_t;

/* jmac_linkpred_rank_* with the filter of query b taken from the index: one wave of the query's block searches
 * (h[b] << 32 | r[b]) in key, 64 probes per round -- 3 rounds of dependent loads for up to 262 144 keys, where a one-lane
 * binary search takes 18 (15 at ja's 19 520 keys) -- and the block reads the range from LDS; a query whose key is absent
 * ranks raw, and so does every query when index is NULL.  Everything after the lookup is jmac_linkpred_rank_*'s code: the
 * ranks are the same integers as with a CSR that holds the same lists.  Workspace: jmac_linkpred_rank_workspace_bytes. */
int jmac_linkpred_rank_indexed_f32(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r,
                                   int32_t pred_head, const int32_t* gold, const jmac_tail_index_t* index, int64_t B,
                                   int64_t N, int64_t d, int32_t* rank, void* ws, size_t ws_bytes, jmac_stream_t stream);
int jmac_linkpred_rank_indexed_bf16(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r,
                                    int32_t pred_head, const int32_t* gold, const jmac_tail_index_t* index, int64_t B,
                                    int64_t N, int64_t d, int32_t* rank, void* ws, size_t ws_bytes, jmac_stream_t stream);

/* Link-prediction top-k: the model's predictions without the [B,N] matrix.  val[b,j], idx[b,j] for j < k are the k smallest
 * dist[b,n] over the n in [0,N) that the index does not list for (h[b], r[b]) -- EVERY listed entry is excluded, there is no
 * gold -- in ascending distance, equal distances by ascending index.  dist is jmac_linkpred_rank_*'s single running fp32 sum
 * over (layer, k), bit for bit: jmac_linkpred_rank_indexed_*(gold = idx[b,j]) is j + 1 for every returned entry.  A query with
 * fewer than k unlisted candidates ends its row with idx = -1, val = +inf.  index NULL: nothing is excluded.
 * 1 <= k <= 64 and k <= N (JMAC_EINVAL), d <= 512 (JMAC_EDIM); n_layers and the LDS limit as jmac_linkpred_rank_*.
 * N >= 8192: a column sample is scored into the workspace, its k-th smallest unlisted distance bounds the row's, the other
 * columns append the entries under that bound to a per-row list (integer atomics claim the slots; the list is sorted
 * afterwards), and one block per query selects; the workspace holds no B x N buffer.  A row whose list overflows (a constant
 * table, a huge tie) is recomputed and selected in passes: slow, exact.  N < 8192: the [B,N] scores go through the workspace.
 * No float atomics; results do not depend on the grid or the CU count, and two calls return identical bits. */
size_t jmac_linkpred_topk_workspace_bytes(int64_t B, int64_t N, int64_t d, int32_t n_layers, int32_t k);
int jmac_linkpred_topk_f32(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r,
                           int32_t pred_head, const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d, int32_t k,
                           float* val, int32_t* idx, void* ws, size_t ws_bytes, jmac_stream_t stream);
int jmac_linkpred_topk_bf16(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r,
                            int32_t pred_head, const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d, int32_t k,
                            float* val, int32_t* idx, void* ws, size_t ws_bytes, jmac_stream_t stream);

/* Cross-KG ensemble link prediction: jmac_linkpred_rank_indexed_f32 and jmac_linkpred_topk_f32 on a distance that several KGs
 * vote on through alignment links (ensemble knowledge transfer between the KGs of a jointly trained model; no counterpart in
 * the reference).  Members g = 0 .. S, S <= 3.  Member 0 is the target KG with N candidate rows (link == NULL, n_rows == N).  A
 * supporting member s >= 1 has its own per-layer entity and relation tables (the same n_layers and d, n_rows rows; relation
 * ids are shared) and a link map link [N] on the device: link[n] is the row of KG s aligned with target row n, or -1.  Every
 * member has a weight >= 0, passed by value; the weights need not sum to 1.  For query b = (h[b], r[b]) and candidate n:
 *     d_g[b,n]       = jmac_linkpred_rank_*'s distance -- the single running fp32 sum over (layer, k) -- in member g's tables,
 *                      query row E^g_l[hq] +/- R^g_l[r[b]], candidate row T^g_l[cn], with (hq, cn) = (h[b], n) for member 0
 *                      and (link_s[h[b]], link_s[n]) for member s
 *     present_s(b,n) = link_s[h[b]] >= 0 and link_s[n] >= 0
 *     D = w_0 * d_0;  then for s = 1 .. S in that order  D = fmaf(w_s, present_s ? d_s : d_0, D)
 * A missing link falls back to the target's own distance: the ensemble never penalises an entity for being unaligned.  With
 * one member and w_0 = 1, D is d_0 bit for bit.  Ranks and top-k, the tie rule (smaller first, equal by lower index), pred_head
 * (the sign applies in every member) and the padding (idx = -1, val = +inf) are the single-KG entry points', decided on D; the
 * filter is the TARGET's known-tail index (NULL: raw).  One device function forms D wherever it is needed (gold and filter
 * correction, tile loop, the select's recompute), so jmac_linkpred_ens_rank_f32(gold = idx[b,j]) is j + 1 for every returned
 * entry and two calls return identical bits; no float atomics, nothing depends on the grid or the CU count.
 * Supporting rows are read through the link map inside the kernel (no permuted copies of the tables); a link value outside
 * [0, n_rows) counts as absent and is never dereferenced.  A 64 x 64 tile without a linked head or without a linked candidate
 * in member s skips that member's share of the loop (no bit changes).  Cost: about (S + 1) x the single-KG call.
 * 1 <= n_members <= 4, member 0 without and every other member with a link, finite weights >= 0 (JMAC_EINVAL); the other
 * limits and error codes are jmac_linkpred_rank_indexed_f32's and jmac_linkpred_topk_f32's.  fp32 tables only. */
typedef struct {
    const jmac_link_layer_t* layers;   /* n_layers entries; table == ent (fp32) */
    const int32_t* link;               /* [N] or NULL for member 0 */
    int64_t n_rows;                    /* rows of this member's tables */
    float weight;
} jmac_link_member_t;
size_t jmac_linkpred_ens_rank_workspace_bytes(int64_t B, int64_t d, int32_t n_layers, int32_t n_members);
int jmac_linkpred_ens_rank_f32(const jmac_link_member_t* members, int32_t n_members, int32_t n_layers, const int32_t* h,
                               const int32_t* r, int32_t pred_head, const int32_t* gold, const jmac_tail_index_t* index,
                               int64_t B, int64_t N, int64_t d, int32_t* rank, void* ws, size_t ws_bytes, jmac_stream_t stream);
size_t jmac_linkpred_ens_topk_workspace_bytes(int64_t B, int64_t N, int64_t d, int32_t n_layers, int32_t n_members, int32_t k);
int jmac_linkpred_ens_topk_f32(const jmac_link_member_t* members, int32_t n_members, int32_t n_layers, const int32_t* h,
                               const int32_t* r, int32_t pred_head, const jmac_tail_index_t* index, int64_t B, int64_t N,
                               int64_t d, int32_t k, float* val, int32_t* idx, void* ws, size_t ws_bytes, jmac_stream_t stream);

/* Link-prediction confidence: the softmax over tails of every query, without the [B,N] matrix (no counterpart in the reference;
 * what a caller otherwise gets from softmax(-scale * forward_linkpred(...)) ).  THE DEFINITION -- every other place refers here:
 *   dist[b,n]   jmac_linkpred_rank_*'s distance of query b = (h[b], r[b]) to candidate n, bit for bit: one running fp32 sum over
 *               (layer, k); pred_head and the bf16 rounding of query and table as there.  Ensemble form: the folded D above.
 *   z[b,n]      = -scale * dist[b,n], scale > 0 and finite (a temperature; JMAC_EINVAL otherwise)
 *   C_b         the candidate set.  gold == NULL (prediction mode, as jmac_linkpred_topk_*): every n in [0,N) the index does not
 *               list for (h[b], r[b]); index NULL or an absent key: all of [0,N).  gold != NULL (evaluation mode, as the ranks):
 *               the same set plus gold[b], even where the index lists it.
 *   near[b]     the n in C_b of smallest dist, the lowest index on ties        dmin[b]  that distance, jmac_linkpred_topk_*'s bits
 *   sum[b]      = sum over C_b of exp(z[b,n] - zmax_b) >= 1, zmax_b = -scale * dmin[b]: 1 / sum is the top-1 probability
 *   ent[b]      = log(l) - t / l with l = sum[b], t = sum over C_b of e^u u, u = z - zmax_b: the entropy of softmax over C_b of z,
 *               in jmac_sim_softmax_stats_f32's form
 *   logp_gold[b] = scale * (dmin[b] - dist[b,gold[b]]) - log(sum[b]), the gold's log-probability; it needs gold (JMAC_EINVAL with
 *               gold == NULL).  dist[b,gold[b]] is the prep kernel's gold distance, which has the tile kernel's bits, so
 *               near[b] == gold[b] implies logp_gold[b] == -logf(sum[b]) exactly, logf being the correctly rounded one here
 *               ((float)log((double)sum[b])), so a caller can reproduce the bits.
 * Every output pointer may be NULL, at least one must be given (JMAC_EINVAL).  An empty C_b (prediction mode, everything listed):
 * near = -1, dmin = +inf, sum = 0, ent = 0.
 * An excluded candidate contributes NOTHING: it is masked to -inf before any reduction, never subtracted afterwards (the known
 * tails are the nearest candidates by training; subtracting them would cancel the whole sum).  The tile kernel's epilogue takes
 * the maximum of every 64-column part before any exponential and plain-stores one partial per (part, query); the partials are
 * merged in ascending part order (jmac_sim_softmax_stats_f32's merge).  No float atomics: results are bitwise reproducible and do
 * not depend on the grid, the CU count or on which other queries share the call.
 * Limits and error codes are jmac_linkpred_rank_indexed_*'s (n_layers <= 4, the LDS limit, d <= 512: JMAC_ERANGE); the ensemble
 * form's are jmac_linkpred_ens_rank_f32's.  Workspace: the rank call's, a few [B] vectors and the partials [ceil(N/64)][B] of
 * 16 bytes -- never B x N. */
size_t jmac_linkpred_stats_workspace_bytes(int64_t B, int64_t N, int64_t d, int32_t n_layers);
int jmac_linkpred_stats_f32(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r,
                            int32_t pred_head, const int32_t* gold, const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d,
                            float scale, int32_t* near, float* dmin, float* sum, float* ent, float* logp_gold, void* ws,
                            size_t ws_bytes, jmac_stream_t stream);
int jmac_linkpred_stats_bf16(const jmac_link_layer_t* layers, int32_t n_layers, const int32_t* h, const int32_t* r,
                             int32_t pred_head, const int32_t* gold, const jmac_tail_index_t* index, int64_t B, int64_t N, int64_t d,
                             float scale, int32_t* near, float* dmin, float* sum, float* ent, float* logp_gold, void* ws,
                             size_t ws_bytes, jmac_stream_t stream);
size_t jmac_linkpred_ens_stats_workspace_bytes(int64_t B, int64_t N, int64_t d, int32_t n_layers, int32_t n_members);
int jmac_linkpred_ens_stats_f32(const jmac_link_member_t* members, int32_t n_members, int32_t n_layers, const int32_t* h,
                                const int32_t* r, int32_t pred_head, const int32_t* gold, const jmac_tail_index_t* index,
                                int64_t B, int64_t N, int64_t d, float scale, int32_t* near, float* dmin, float* sum, float* ent,
                                float* logp_gold, void* ws, size_t ws_bytes, jmac_stream_t stream);

/* rank[b] = 1 +#{n : score[b,n] < score[b,gold] or (== and n < gold[b])}, where entries listed in
 * the filter CSR (filt_ptr [B+1], filt_idx) other than the gold are skipped.  descending == 0: `score` is a
 * DISTANCE (the reference's predictions = -dist, sorted descending); descending != 0: `score` is a SIMILARITY
 * and `<` reads `>` (alignment ranks, modules/finding/alignment.py:87-112).  filt_ptr may be NULL (raw ranking). */
int jmac_filtered_rank_f32(const float* score, int64_t lds, const int32_t* gold,
                           const int32_t* filt_ptr, const int32_t* filt_idx, int64_t B, int64_t N,
                           int32_t descending, int32_t* rank, jmac_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Alignment scoring (replaces: get_neg's mm + topk, modules/utils/util.py:52-53; the mm / softmax /
 * entropy of compute_alignment_quality, train.py:239-248).
 * --------------------------------------------------------------------------------------------- */
/* C[m,n] = sum_k A[m,k] * B[n,k]  (fp32-in / fp32-accumulate MFMA: exact fp32 products). */
int jmac_sim_matrix_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t M,
                        int64_t N, int64_t d, float* C, int64_t ldc, jmac_stream_t stream);

size_t jmac_sim_topk_workspace_bytes(int64_t L, int64_t N, int32_t k);
/* Per row of A: the k largest similarities against all rows of B, descending, ties -> lower index
 * first.  val [L,k] (may be NULL), idx [L,k] int32.
 * N >= 8192 and k <= 64: the L x N score matrix is never written (running top-k in the product's epilogue): a column sample
 * gives every row a threshold (the k-th largest of its first ~N/8 scores, a lower bound of its final k-th score), the full
 * product appends the scores that reach it to per-row candidate lists, a last pass takes the k best of each list; a row whose
 * list overflows (mass ties) recomputes its scores with the product's own instruction sequence.  Same scores bit for bit,
 * hence the same indices as the two-step form; workspace O(L * N / 8) instead of L * N * 4. */
int jmac_sim_topk_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N,
                      int64_t d, int32_t k, float* val, int32_t* idx, void* ws, size_t ws_bytes,
                      jmac_stream_t stream);

size_t jmac_sim_topk_screened_workspace_bytes(int64_t L, int64_t N, int64_t d, int32_t k);
/* jmac_sim_topk_f32's result bit for bit -- values, indices, tie order -- with the L x N x d work on the bf16 matrix cores.  The
 * bf16 product (operands rounded once to bf16, fp32 accumulate) only SCREENS: its score sh of a pair differs from the fp32 score
 * s by at most e = 0.008 (na + 2^-110)(nb + 2^-110) + 2^-110 (na, nb: upper bounds of the rows' l2 norms; proof: DESIGN section 5),
 * so the k-th largest sh - e of any set of columns bounds the row's exact k-th score from below and every pair with sh + e under
 * that bound is out.  What survives (a few dozen columns per row) is rescored with the fp32 product's own instruction sequence and
 * the k best of those exact scores are returned.  N >= 8192 and k <= 64; any other shape runs jmac_sim_topk_f32's code unchanged.
 * d % 4 == 0 and d <= 512 (JMAC_EDIM); the other checks and their order are jmac_sim_topk_f32's (+ JMAC_ERANGE for L or N >= 2^31).
 * n_rescored [L] (may be NULL): the columns row i rescored exactly; -1: the row's candidate list overflowed (mass ties) and it
 * recomputed all N scores; -2: the shape took the unscreened path.  Finite inputs; no float atomics: two calls return the same bits. */
int jmac_sim_topk_screened_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t L, int64_t N, int64_t d,
                               int32_t k, float* val, int32_t* idx, int32_t* n_rescored, void* ws, size_t ws_bytes,
                               jmac_stream_t stream);

/* Row top-k of an existing score matrix (same ordering rule). */
int jmac_row_topk_f32(const float* S, int64_t lds, int64_t L, int64_t N, int32_t k, float* val,
                      int32_t* idx, jmac_stream_t stream);

size_t jmac_softmax_entropy_workspace_bytes(int64_t n1, int64_t n2);
/* S = A B^T (n1 x n2); ent_rows[i] = H(softmax_j(scale*S[i,:])), ent_cols[j] = H(softmax_i(scale*S[:,j])). */
int jmac_softmax_entropy_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1,
                             int64_t n2, int64_t d, float scale, float* ent_rows, float* ent_cols,
                             void* ws, size_t ws_bytes, jmac_stream_t stream);

/* Softmax STATISTICS of S = A B^T (n1 x n2) without the matrix: the products are the fp32-MFMA products of jmac_sim_matrix_f32,
 * bit for bit, and are reduced in the product kernel's epilogue -- S is never written; the workspace holds partial statistics,
 * O((n1 + n2) * n / 64) words (about an eighth of one matrix), never n1 * n2.  With the logits z = scale * S, scale > 0:
 *   row_max[i] = max_j S[i,j]  (the raw similarity, == jmac_sim_matrix_f32's row maximum bitwise)
 *   row_arg[i] = the column of that maximum; TIES: the lowest index
 *   row_sum[i] = sum_j e^(scale (S[i,j] - row_max[i]))           (softmax(z)[i, row_arg[i]] == 1 / row_sum[i])
 *   row_ent[i] = log(l) - t / l,  l = row_sum[i],  t = sum_j e^(z - max z) (z - max z)   (the entropy of softmax_j(z[i,:]))
 * and col_* the same along the columns (col_arg[j]: the lowest row index of column j's maximum).  Every output pointer may be
 * NULL (not wanted); at least one must be given.  Run-to-run bitwise reproducible and independent of the device's CU count:
 * partials are stored per 64-column / 64-row part and merged in ascending order.  lda, ldb % 4 == 0 (d padded with zeros). */
size_t jmac_sim_softmax_stats_workspace_bytes(int64_t n1, int64_t n2);
int jmac_sim_softmax_stats_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d,
                               float scale, float* row_max, int32_t* row_arg, float* row_sum, float* row_ent, float* col_max,
                               int32_t* col_arg, float* col_sum, float* col_ent, void* ws, size_t ws_bytes,
                               jmac_stream_t stream);

/* Log-sum-exp of S = A B^T (n1 x n2) with additive offsets, without the matrix (the half-steps of log-domain Sinkhorn):
 *   row_out[i] = row_shift - log sum_j exp(scale S[i,j] + col_add[j])
 *   col_out[j] = col_shift - log sum_i exp(scale S[i,j] + row_add[i])
 * S is jmac_sim_matrix_f32's fp32-MFMA product, bit for bit, reduced in the product kernel's epilogue and never written.  A logit
 * is fma(scale, s, add); every 64-element part takes its maximum exactly before any exponential.  col_add [n2] / row_add [n1]
 * may be NULL (= 0); the offsets must be finite (the caller vouches), scale > 0.  row_out / col_out may be NULL: that side is
 * not reduced at all (no partials, no epilogue work); at least one must be given.  An output may not alias an offset vector the
 * same call reads.  The workspace holds the partials, [ceil(n2/64)][n1] and [ceil(n1/64)][n2] float2 -- O((n1 + n2) n / 64),
 * never n1 * n2 -- written once and merged in ascending part order: bitwise reproducible, independent of the grid, the tile
 * walk and the device's CU count; a one-sided call gives the bits of the two-sided one.  lda, ldb, d % 4 == 0 (JMAC_EDIM). */
size_t jmac_sim_lse_workspace_bytes(int64_t n1, int64_t n2);
int jmac_sim_lse_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d, float scale,
                     const float* col_add, const float* row_add, float row_shift, float col_shift, float* row_out,
                     float* col_out, void* ws, size_t ws_bytes, jmac_stream_t stream);

/* Softmax of an existing score matrix S [n1,n2] (row-major) with rows in `row_mask` and columns in `col_mask` (uint8, 1 = keep;
 * NULL mask = keep all) left as they are and every other entry replaced by `fill` (train.py:252-257: fill = -1), all scaled by
 * `scale`, then
 *   jmac_row_softmax_f32: softmax over each ROW    -> out [n1,n2] (may be NULL), ent [n1] = entropy of the row (may be NULL)
 *   jmac_col_softmax_f32: softmax over each COLUMN -> out_t [n2,n1] = the TRANSPOSED probabilities, i.e.
 *                         softmax(scale * S^T, dim=1) (may be NULL), ent [n2] (may be NULL)
 * so that both orientations of compute_alignment_quality (train.py:241-257; DBPv1 trainer/jmac_trainer.py:281-300:
 * softmax(simi) and softmax(simi.t())) come from ONE similarity GEMM. */
int jmac_row_softmax_f32(const float* S, int64_t lds, int64_t n1, int64_t n2, const uint8_t* row_mask,
                         const uint8_t* col_mask, float fill, float scale, float* out, int64_t ldo, float* ent,
                         jmac_stream_t stream);
size_t jmac_col_softmax_workspace_bytes(int64_t n1, int64_t n2);
int jmac_col_softmax_f32(const float* S, int64_t lds, int64_t n1, int64_t n2, const uint8_t* row_mask,
                         const uint8_t* col_mask, float fill, float scale, float* out_t, int64_t ldo, float* ent,
                         void* ws, size_t ws_bytes, jmac_stream_t stream);

/* The k largest values of every COLUMN of S [n1,n2], descending (val [n2,k]; k <= 16) -- the column term of CSLS
 * (calculate_nearest_k on sim_mat.T, modules/finding/similarity.py:66-67,81-84) without materialising the transpose. */
size_t jmac_col_topk_workspace_bytes(int64_t n1, int64_t n2, int32_t k);
int jmac_col_topk_f32(const float* S, int64_t lds, int64_t n1, int64_t n2, int32_t k, float* val, void* ws,
                      size_t ws_bytes, jmac_stream_t stream);

/* CSLS rescoring (replaces csls_sim, modules/finding/similarity.py:58-78):
 * out[i,j] = 2*S[i,j] - r1[i] - r2[j], r1/r2 = mean of the k largest entries of row i / column j. */
int jmac_csls_apply_f32(const float* S, int64_t lds, int64_t n1, int64_t n2, const float* r1,
                        const float* r2, float* out, int64_t ldo, jmac_stream_t stream);

/* rank[i] = 1 + #{j : c(i,j) > c(i,gold[i]) or (== and j < gold[i])} with c(i,j) = 2*S[i,j] - r1[i] - r2[j]:
 * jmac_csls_apply_f32 followed by the descending rank count, fused (the rescored matrix is neither written nor
 * re-read; same arithmetic, identical ranks).  Alignment evaluation: alignment.py:87-112 on similarity.py:58-78. */
int jmac_csls_rank_f32(const float* S, int64_t lds, int64_t n1, int64_t n2, const float* r1, const float* r2,
                       const int32_t* gold, int32_t* rank, jmac_stream_t stream);

/* Matrix-free alignment evaluation: the two entry points above without the stored matrix.  S = A B^T (n1 x n2) is the product of
 * jmac_sim_matrix_f32, bit for bit, and is never written; c(i,j) = 2*S[i,j] - r1[i] - r2[j], computed in that order everywhere.
 * r1 == r2 == NULL: plain similarity, c = S; give both or neither (JMAC_EINVAL).  lda, ldb, d % 4 == 0 (JMAC_EDIM).
 *
 * jmac_sim_csls_rank_f32: rank[i] = 1 + #{j < n2 : c(i,j) > c(i,gold[i]) or (== and j < gold[i])}, jmac_csls_rank_f32's rule.  A prep
 * launch takes every row's gold value from the product's own contraction sequence; the product then runs with a count epilogue
 * (compare, reduce inside the wave, integer atomics only): bitwise reproducible, independent of grid and CU count.  gold entries
 * in [0, n2) are the caller's to vouch for.  Workspace O(n1): nothing grows with n2. */
size_t jmac_sim_csls_rank_workspace_bytes(int64_t n1, int64_t n2);
int jmac_sim_csls_rank_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d,
                           const float* r1, const float* r2, const int32_t* gold, int32_t* rank, void* ws, size_t ws_bytes,
                           jmac_stream_t stream);
/* jmac_sim_csls_topk_f32: per row of A the k columns with the largest c(i,j), descending, ties -> lower index first; val [n1,k]
 * (may be NULL), idx [n1,k] int32; 1 <= k <= min(64, n2) (JMAC_EINVAL).  jmac_sim_topk_f32's scheme with the rescored value in
 * every stage (sample threshold, filter epilogue, overflow recompute); below 8192 columns the scores are staged in the
 * workspace.  With NULL r1 / r2 the result is jmac_sim_topk_f32's bit for bit.  Workspace: jmac_sim_topk_workspace_bytes's. */
size_t jmac_sim_csls_topk_workspace_bytes(int64_t n1, int64_t n2, int32_t k);
int jmac_sim_csls_topk_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d,
                           const float* r1, const float* r2, int32_t k, float* val, int32_t* idx, void* ws, size_t ws_bytes,
                           jmac_stream_t stream);
/* jmac_sim_csls_topk_viable_f32: the same top-k over the VIABLE columns of every row only -- column j is viable for row m iff
 * tk(c(m,j), row_id[m]) > best[j], where tk(v, i) is the 64-bit word (order-preserving key of v) << 32 | ~i: larger value first,
 * equal values -> lower index first, the order of every top-k here; best[j] = 0 means nothing is held.  The rows of A are a gathered
 * subset of the suitors of jmac_stable_match_f32 (below), row_id [n1] int32 names them (the tie-break), best [n2] is that entry
 * point's reviewer state.  A row with fewer than k viable columns ends in (idx -1, val -inf); val is required.  The predicate
 * runs in all three stages (sample threshold, filter epilogue, overflow recompute; a sample with fewer than k viable entries gives
 * the threshold -inf: every viable column is listed, slow but exact), so with best all zero the result is jmac_sim_csls_topk_f32's
 * bit for bit.  Error codes and workspace: jmac_sim_csls_topk_f32's. */
int jmac_sim_csls_topk_viable_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d,
                                  const float* r1, const float* r2, const int32_t* row_id, const uint64_t* best, int32_t k,
                                  float* val, int32_t* idx, void* ws, size_t ws_bytes, jmac_stream_t stream);

/* jmac_sim_csls_topk_screened_f32 / jmac_sim_csls_topk_viable_screened_f32: the two entry points above, values, indices and tie
 * order bit for bit, with the n1 x n2 x d work on the bf16 matrix cores -- jmac_sim_topk_screened_f32's scheme deciding on c.  For
 * finite r1, r2 the value c = 2 s - r1 - r2, roundings included, is a non-decreasing function of s, so the screen's bounds
 * fl(sh - e) <= s <= fl(sh + e) give c_lo <= c <= c_hi with the same expression: the k-th largest c_lo bounds a row's k-th best c
 * from below, a column with c_hi under it is out, the survivors are rescored with the fp32 product's own instructions and c is
 * formed from that exact s.  The viable predicate is monotone in c as well: a column raises a threshold only when it is viable at
 * c_lo, is dropped unseen only when it is not viable at c_hi, and the exact predicate runs on the rescored c.  With r1 == r2 ==
 * NULL the plain form is jmac_sim_topk_screened_f32 bit for bit.  n2 >= 8192 (k <= 64 always holds here); a narrower n2 runs the
 * fp32 entry's code unchanged, with that entry's workspace, and n_rescored = -2; so does a viable call of fewer than 256 rows (a
 * refill of a few gathered rows would pay the bf16 copy of all of B for less than it saves: measured), in the
 * workspace sized below.  Checks and their order: the fp32 entries', then
 * d % 4 == 0 and d <= 512 (JMAC_EDIM) and n1, n2 < 2^31 (JMAC_ERANGE), both ahead of the workspace check.  n_rescored [n1] (may be
 * NULL): the columns row i rescored exactly; -1: the row's list overflowed and it recomputed all n2 values.  r1, r2 finite; no float
 * atomics: two calls return the same bits. */
size_t jmac_sim_csls_topk_screened_workspace_bytes(int64_t n1, int64_t n2, int64_t d, int32_t k);
int jmac_sim_csls_topk_screened_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d,
                                    const float* r1, const float* r2, int32_t k, float* val, int32_t* idx, int32_t* n_rescored,
                                    void* ws, size_t ws_bytes, jmac_stream_t stream);
int jmac_sim_csls_topk_viable_screened_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2,
                                           int64_t d, const float* r1, const float* r2, const int32_t* row_id, const uint64_t* best,
                                           int32_t k, float* val, int32_t* idx, int32_t* n_rescored, void* ws, size_t ws_bytes,
                                           jmac_stream_t stream);

/* jmac_sim_csls_rank_screened_f32: jmac_sim_csls_rank_f32's ranks bit for bit with the n1 x n2 x d work on the bf16 matrix cores.  The
 * count predicate before(c, j) = c > g || (c == g && j < G) -- g = c(i, gold[i]) with the fp32 product's bits, G = gold[i] -- is
 * monotone in c, and the screen bounds every element, c_lo <= c <= c_hi (above): a column with before(c_lo, j) is counted unseen, one
 * with c_hi < g || (c_hi == g && j > G) is dropped, and only the columns with g inside [c_lo, c_hi] are rescored with the fp32
 * product's own instructions and put to the exact predicate (the gold column is always one of them).  n_rescored [n1] (may be NULL):
 * that many columns of row i were rescored.  A row with more than 512 of them overflows: n_rescored = -1, and with finish != 0 the
 * entry recounts the row over all n2 columns (slow, exact), with finish == 0 it returns rank[i] = 0 for the caller to run the row
 * through jmac_sim_csls_rank_f32 (a valid rank is >= 1).  n2 >= 8192; a narrower n2 runs the fp32 entry's code unchanged in the
 * workspace sized below, n_rescored = -2.  Checks and their order: jmac_sim_csls_rank_f32's, with d <= 512 next to d % 4 == 0
 * (JMAC_EDIM) ahead of the range and workspace checks.  r1, r2 finite (both NULL: c = S); integer atomics only, no host
 * synchronisation: two calls return the same bits. */
size_t jmac_sim_csls_rank_screened_workspace_bytes(int64_t n1, int64_t n2, int64_t d);
int jmac_sim_csls_rank_screened_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d,
                                    const float* r1, const float* r2, const int32_t* gold, int32_t* rank, int32_t* n_rescored,
                                    int32_t finish, void* ws, size_t ws_bytes, jmac_stream_t stream);

/* Manhattan alignment (sim(metric='manhattan'), modules/finding/similarity.py:47-49): the three entry points above for
 * s(i,j) = 1 - dist(i,j), dist(i,j) = the single running fp32 sum over k = 0 .. d-1 of |A[i,k] - B[j,k]| -- jmac_l1_score_f32's bits,
 * the same from either side (|x - y| == |y - x|) -- and c(i,j) = 2*s(i,j) - r1[i] - r2[j]; r1 == r2 == NULL: c = s.  Every decision
 * is taken on c, larger first, equal values -> lower index first; the n1 x n2 matrix is never written.  The L1 tile kernel of the
 * link-prediction entry points runs with count / filter / viable epilogues on c; narrow matrices (n2 < 8192) are staged in the
 * workspace.  lda, ldb % 4 == 0 (JMAC_EDIM); any d.  1 <= k <= min(64, n2); val is required.  Otherwise the contracts, error codes
 * and workspace sizes of jmac_sim_csls_topk_f32, jmac_sim_csls_topk_viable_f32 and jmac_sim_csls_rank_f32. */
size_t jmac_l1_csls_topk_workspace_bytes(int64_t n1, int64_t n2, int64_t d, int32_t k);
int jmac_l1_csls_topk_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d,
                          const float* r1, const float* r2, int32_t k, float* val, int32_t* idx, void* ws, size_t ws_bytes,
                          jmac_stream_t stream);
int jmac_l1_csls_topk_viable_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d,
                                 const float* r1, const float* r2, const int32_t* row_id, const uint64_t* best, int32_t k,
                                 float* val, int32_t* idx, void* ws, size_t ws_bytes, jmac_stream_t stream);
size_t jmac_l1_csls_rank_workspace_bytes(int64_t n1, int64_t n2);
int jmac_l1_csls_rank_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t n1, int64_t n2, int64_t d,
                          const float* r1, const float* r2, const int32_t* gold, int32_t* rank, void* ws, size_t ws_bytes,
                          jmac_stream_t stream);

/* Stable one-to-one alignment (replaces galeshapley, modules/finding/alignment.py:115-168, run to convergence): deferred acceptance
 * of the n1 suitors (rows) on candidate lists cand_idx / cand_val [n1, ld >= k] (int32 reviewer ids in [0, n2), best first, -1 ends
 * a list, no id twice in a list; cand_val[i,p] = c(i, cand_idx[i,p]) fp32, finite).  Order relation on both sides: larger c first,
 * equal c -> lower index first (suitor i prefers j to j' iff c(i,j) > c(i,j') or == and j < j'; reviewer j prefers i to i' iff
 * c(i,j) > c(i',j) or == and i < i'); the result is the suitor-optimal stable matching of the instance the lists describe, which
 * is unique: bitwise reproducible, independent of scheduling.  The fixpoint is reached on the device, no host read.
 * State kept between calls (zero-fill BOTH before the first call): best [n2] uint64, the tk word (see above) of the best proposal
 * reviewer j has received, 0 = free; ptr [n1] int32, the suitor's list position, bit 31 set while it holds that entry.  To continue
 * with new lists for some suitors (jmac_sim_csls_topk_viable_f32's for the exhausted ones), overwrite their rows and zero their ptr.
 * Out: match1 [n1] reviewer held or -1, match2 [n2] suitor kept or -1; counters [2] uint64 = {exhausted suitors (not holding, list
 * not empty), proposals made by this call}; the exhausted suitors' ids, in no particular order, are the first counters[0] int32 of
 * ws.  A suitor with an empty list is unmatched and not counted. */
size_t jmac_stable_match_workspace_bytes(int64_t n1, int64_t n2);
int jmac_stable_match_f32(const int32_t* cand_idx, const float* cand_val, int64_t ld, int64_t n1, int64_t n2, int32_t k, int32_t* ptr,
                          uint64_t* best, int32_t* match1, int32_t* match2, uint64_t* counters, void* ws, size_t ws_bytes,
                          jmac_stream_t stream);

/* Optimal one-to-one alignment ("Hungarian" in the entity-alignment literature): Bertsekas' auction algorithm on candidate lists,
 * up to `rounds` synchronous bidding rounds per call.  Rows i in [0, n1) bid for columns j in [0, n2).
 * Lists (read-only during a call): idx / val / pref [n1, ld >= k], 2 <= k <= min(64, n2) (JMAC_EINVAL); every entry of a row a
 * different column in [0, n2); val = c(i,j) - price[j] AS OF THE REFILL, best first (equal values -> lower column), pref = the price
 * of that column then.
 * State kept between calls: price [n2] fp32 (start: 0), owner [n2] int32 (start: -1 = free), match1 [n1] int32: >= 0 the column
 * held, -1 open, -2 open and waiting for a refill (start: -1).
 * One round: every row at -1 at its start takes cur_m = val[i,m] - (price[idx[i,m]] - pref[i,m]) (two fp32 subtractions, in that
 * order), w1 = the largest (equal values -> lower column), j1 its column, w2 = the largest of the others, bound = val[i,k-1]
 * (k == n2: -inf).  w2 < bound: no unlisted column is known to be worse than w2 any more; the row becomes -2 and sits the rest of the
 * call out.  Otherwise it bids (price[j1] + (w1 - w2)) + eps in fp32 (nextafter(price[j1], +inf) if that does not exceed price[j1])
 * by an atomic max on the column's 64-bit word tk(bid, i) -- highest bid first, equal bids -> lower row.  After all bids every
 * column with a bid is resolved: its previous owner gets -1, owner / match1 / price are set from the word.  A call stops early once
 * a round has no bidder.  Any subset of the open rows may bid in a round: the final matching satisfies eps-complementary slackness.
 * The floats depend on no atomic order (atomic max on packed words and integer counter adds only): bitwise reproducible.
 * form: 1 = grid (one bid and one resolve launch per round; after a round without a bidder the remaining launches do nothing);
 *       2 = one workgroup (ONE launch loops over the rounds, the open rows are a queue in LDS of JMAC_AUCTION_QUEUE_ROWS entries;
 *           n_open above that: JMAC_EINVAL); 0 = 2 if n_open <= JMAC_AUCTION_QUEUE_ROWS, else 1.  Both forms run the same rounds:
 *           the same state gives the same bits.  n_open: an upper bound of the rows at -1 (the count never grows during a run: a bid
 *           assigns one row and evicts at most one); rows beyond the queue would sit the call out.
 * 0 <= rounds <= 4096, eps finite and > 0 (JMAC_EINVAL).  Out: counters [4] uint64 = {rows open (-1 or -2) after the call, rows at
 * -2, rounds with a bidder run by this call, bids made by this call}.  The workspace holds the columns' bid words; nothing in it is
 * kept between calls. */
#define JMAC_AUCTION_QUEUE_ROWS 256
size_t jmac_auction_rounds_workspace_bytes(int64_t n1, int64_t n2);
int jmac_auction_rounds_f32(const int32_t* idx, const float* val, const float* pref, int64_t ld, int64_t n1, int64_t n2, int32_t k,
                            float* price, int32_t* owner, int32_t* match1, float eps, int32_t rounds, int32_t form, int64_t n_open,
                            uint64_t* counters, void* ws, size_t ws_bytes, jmac_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Small fp32 GEMM for the relation-side projections (replaces the torch.mm calls on the ~10^3-row
 * relation tables: src/jmac_model.py:40-42 rel_transform_weight1/2, :195-196 relation MLPs, and the
 * hoisted rel'' @ [Wb|Wg] of the factorised layer) and their backward forms.
 *   C[M,N] = op(A) op(B), row-major; transX != 0: op(X) = X^T, i.e. A is stored [K,M] / B is stored [N,K].
 * Exact fp32 products on the fp32-input MFMA, fixed summation order (bitwise reproducible).  Any M, N, K, ld.
 * --------------------------------------------------------------------------------------------- */
int jmac_gemm_f32(const float* A, int64_t lda, int32_t transA, const float* B, int64_t ldb,
                  int32_t transB, int64_t M, int64_t N, int64_t K, float* C, int64_t ldc,
                  jmac_stream_t stream);

/* Grouped form: up to JMAC_GEMM_MAX_TASKS independent small products in ONE launch (the relation side of a training step is
 * ~40 such products, each launch-bound on its own: products of one dependency level go out together).  `tasks` is a HOST
 * array; it is copied into the kernel arguments, so the call is safe under stream capture.  Per task:
 *   C[M,N] (+)= epilogue( op(A) op(B) ),  op as in jmac_gemm_f32;
 *   a_split > 0: the MEMORY rows >= a_split of A are read from A2 (row index - a_split) -- cat(rel_emb, loop_rel) of
 *                src/jmac_model.py:39 without the copy; c_split > 0: output rows >= c_split are written to C2 (its adjoint);
 *   act: JMAC_GEMM_ACT_LEAKY / _RELU apply the activation to the product (src/jmac_model.py:41; DBPv1 :51: ReLU);
 *        JMAC_GEMM_DACT_LEAKY / _RELU multiply the product by act'(z) where act_src holds act(z) (same shape as C; the
 *        sign of act(z) is the sign of z for slope > 0) -- the activation's backward fused into the product that
 *        produces its incoming gradient;
 *   accumulate != 0: C += (applied after the epilogue); rows that go to C2 are always stored, never accumulated.
 * Exact fp32 products (fp32-input MFMA), fixed summation order per element (bitwise reproducible). */
#define JMAC_GEMM_MAX_TASKS 24
#define JMAC_GEMM_ACT_NONE 0
#define JMAC_GEMM_ACT_LEAKY 1
#define JMAC_GEMM_ACT_RELU 2
#define JMAC_GEMM_DACT_LEAKY 3
#define JMAC_GEMM_DACT_RELU 4
typedef struct {
    const float* A;  const float* A2;  int64_t lda;  int64_t a_split;  int32_t transA;  int32_t transB;
    const float* B;  int64_t ldb;
    float* C;  float* C2;  int64_t ldc;  int64_t c_split;
    int64_t M, N, K;
    const float* act_src;  int64_t ld_act_src;
    int32_t act;  int32_t accumulate;  float slope;  int32_t pad_;
} jmac_gemm_task_t;
int jmac_gemm_grouped_f32(const jmac_gemm_task_t* tasks, int32_t n_tasks, jmac_stream_t stream);

/* [Wt | Wb | Wg] [d, 3d] of up to JMAC_WCAT_MAX layers in one launch (w_att = [Wt; Wb] [2d, d] stacked by rows,
 * src/jmac_model.py:24,75-76; gcn_weight [d, d]) -- the operand of the hoisted node projection X [Wt|Wb|Wg] -- and its adjoint:
 * d w_att [2d, d] and d gcn_weight [d, d] cut out of d[Wt|Wb|Wg].  The pointer arrays are HOST arrays of device pointers
 * (copied into the kernel arguments: capture-safe); all matrices contiguous; d % 4 == 0.
 * extra_src / extra_dst / extra_floats: one more contiguous copy in the same launch (the encoder's U11 block of the folded
 * name projection, src/jmac_model.py:177,180, and its adjoint), 16-byte aligned, a multiple of 4 floats; 0 floats: none.
 * counters (pack only): up to JMAC_WCAT_MAX device int64 incremented by one in the same launch -- nn.BatchNorm1d's
 * num_batches_tracked of the layers a training-mode encoder call is about to run (src/jmac_model.py:52). */
#define JMAC_WCAT_MAX 4
/* The step's DROPOUT SEEDS ride along in the pack (round 5): seed_state [2] = persistent device int64 words, advanced by one
 * per launch; seed_out [2] receives the advanced values -- the seeds jmac_row_normalize_dropseed_{fwd,bwd}_f32 draw from in this
 * step (completion_dropout, src/jmac_model.py:179,191).  No torch RNG op per step: a captured step that uses none is replayed
 * without the generator-state fills torch puts in front of every replay of a graph that does.  Both NULL: no seeds. */
int jmac_wcat_pack_seed_f32(const float* const* w_att, const float* const* gcn, float* const* wcat, int32_t n_layers,
                            int64_t d, const float* extra_src, float* extra_dst, int64_t extra_floats,
                            int64_t* const* counters, int32_t n_counters, int64_t* seed_state, int64_t* seed_out,
                            jmac_stream_t stream);
int jmac_wcat_unpack_f32(const float* const* dwcat, float* const* d_watt, float* const* d_gcn,
                         int32_t n_layers, int64_t d, const float* extra_src, float* extra_dst,
                         int64_t extra_floats, jmac_stream_t stream);

/* Adam over every parameter tensor of the model in ONE launch (round 5).  train.py:406-407 build torch.optim.Adam(model.parameters(),
 * lr) and :358-359 step it once per batch; torch's fused multi-tensor form gives each 65 536-element chunk to one workgroup -- 125
 * workgroups for the 6.3 M parameters of the DBP-5L model, under half of the 256 CUs.  Same arithmetic as torch.optim.Adam (defaults:
 * betas 0.9 / 0.999, eps 1e-8, weight_decay 0; decoupled != 0 = AdamW's decay; amsgrad is not offered), bias corrections in double:
 *   g' = (maximize ? -g : g) (+ wd p);  m = m + (g' - m)(1 - b1);  v = b2 v + (1 - b2) g'^2
 *   p = p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps),      t = step[0] + 1
 * tasks: HOST array (copied into the kernel arguments: capture-safe; more than JMAC_ADAM_MAX_TASKS: several launches); p / g / m / v
 * contiguous fp32 of n elements (`vec4` is set by the library).  step [1] device float = completed steps, advanced by one by the
 * call.  aux [3] device double, 8-byte aligned = { beta1^step, beta2^step, 0 }: the running powers the bias corrections are made
 * from (advanced by the call; the caller initialises them for the count it starts from -- {1, 1, 0} for a fresh optimizer -- and
 * again if it changes the betas) and a word that is zero at rest (the last workgroup to finish advances step and powers: every
 * workgroup has read them by then). */
#define JMAC_ADAM_MAX_TASKS 64
typedef struct {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    int32_t vec4;
} jmac_adam_task_t;
int jmac_adam_step_f32(const jmac_adam_task_t* tasks, int32_t n_tasks, float* step, double* aux, double lr, double beta1,
                       double beta2, double eps, double weight_decay, int32_t decoupled, int32_t maximize, jmac_stream_t stream);

/* Used-relation compaction.  A DBP-5L KG names 153-833 of its 961 relation rows in its edges (ja: 158), and the layer's
 * relation transform + projection (src/jmac_model.py:39-42 and the hoisted R''[Wb|Wg]) matter for named rows only: the encoder
 * runs those products on the COMPACT table of used rows (+ the loop row), with edge types renumbered accordingly.
 *   compact: dst[t][p, :] = src[t][idx[p], :]            p < n_used            (idx: device int64 [n_used], ascending)
 *   expand : dst[t][r, :] = src[t][pos[r], :] or 0       r < rows              (pos: device int32 [rows], -1 = unused row;
 *            h_accumulate[t] != 0: dst[t][r, :] += src[t][pos[r], :] on used rows, other rows untouched)
 * Up to 4 tables per launch (host arrays of device pointers); compact tables are dense [., d]; d % 4 == 0, 16-byte rows. */
int jmac_rows_compact_f32(const float* const* h_src, const int64_t* h_ld_src, float* const* h_dst, int32_t n_tables,
                          const int64_t* idx, int64_t n_used, int64_t d, jmac_stream_t stream);
int jmac_rows_expand_f32(const float* const* h_src, float* const* h_dst, const int64_t* h_ld_dst,
                         const int32_t* h_accumulate, int32_t n_tables, const int32_t* pos, int64_t rows, int64_t d,
                         jmac_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Loss gathers.  Indices are the reference's int64 tensors (batch_h /
 * batch_r / batch_t, links, neg_left ...), values in range; rows may have any d (16-byte aligned rows
 * with d % 4 == 0 take the vector path).
 * --------------------------------------------------------------------------------------------- */

/* score[x] = || ent[h[x]] + rel[r[x]] - ent[t[x]] ||_1   (replaces the three gathers, the sum and
 * torch.norm(score, 1, -1) of completion_loss, src/jmac_model.py:345-350).  d <= 512.
 * period: a HINT that triples x, x+period, x+2*period ... share (h, r) -- the reference's batch is
 * sub.repeat(K+1), rel.repeat(K+1), cat(obj, negatives) with period = batch size (train.py:347-352) --
 * so that one wavefront reads E[h]+R[r] once per run.  Any input is correct (a triple of the run with
 * another (h, r) is handled on its own); period <= 0 or >= T: no grouping. */
int jmac_triple_l1_fwd_f32(const float* ent, int64_t lde, const float* rel, int64_t ldr,
                           const int64_t* h, const int64_t* r, const int64_t* t, int64_t T,
                           int64_t period, int64_t d, float* score, jmac_stream_t stream);
/* Adjoint: dent[h[x]] += g s, drel[r[x]] += g s, dent[t[x]] -= g s with s = sign(ent[h]+rel[r]-ent[t])
 * (sign(0) = 0, as torch's norm backward).  dent [N,d] / drel [nrel,d] must be ZEROED by the caller (or
 * hold a gradient to accumulate into); float atomics; with `period` the run's dent[h] / drel[r] terms are
 * summed in registers and added once. */
int jmac_triple_l1_bwd_f32(const float* ent, int64_t lde, const float* rel, int64_t ldr,
                           const int64_t* h, const int64_t* r, const int64_t* t, int64_t T,
                           int64_t period, int64_t d, const float* gscore, float* dent, int64_t ldde, float* drel, int64_t lddr,
                           jmac_stream_t stream);
/* Pair cosine distance with a bitwise reproducible backward (src/jmac_model.py:237-249): the forward also leaves stats [L,4] =
 * (a.b, a.a, b.b, 0) per pair.  The backward walks the 2 L (pair, side) incidences in the order the HOST sorted them by the
 * gradient row they touch (stable: ties in pair order) and is the FIRST WRITER of its gradient tables (no zero fill by the caller):
 * one wave per gradient ROW over [0, n1 + n2) (rows [0,n1) of de1, then n2 rows of de2; n2 = 0 when both sides share one table)
 * sums its run in sorted order and writes the row once with a plain store; rows without incidences are written as zeros.
 * rec [2L][4] int32, one record per SORTED position: {pair x, own table row, partner table row, flags | gradient row} -- own /
 * partner rows relative to the e1 / e2 pointers passed here; flags: bit 31 = first incidence of its gradient row, bit 30 = side 1
 * (own row in e2, partner in e1), bit 29 = the gradient row is a row of de2 (else de1); bits 0-28 = the gradient row.
 * rowptr [n1+n2+1] = first sorted position (into rec) of every row's run.  The incoming gradient is gdist [L], or the scalar
 * gscalar[0] / gscale for every pair (the .mean() over the pairs of alignment_loss_simple, :249).  The index vectors of an
 * alignment loss are constant over many steps (seed links: train.py:347-352), so the host sorts once per index tensor
 * (jmac_amd.losses._pair_index). */
int jmac_pair_cosine_fwd_stats_f32(const float* e1, int64_t ld1, const float* e2, int64_t ld2, const int64_t* i1,
                                   const int64_t* i2, int64_t L, int64_t d, float* dist, float* stats,
                                   jmac_stream_t stream);
int jmac_pair_cosine_bwd_rows_f32(const float* e1, int64_t ld1, const float* e2, int64_t ld2, int64_t L, int64_t d,
                                  const float* gdist, const float* gscalar, float gscale, const float* stats,
                                  const int32_t* rec, const int32_t* rowptr, int64_t n1, int64_t n2, float* de1,
                                  int64_t ldd1, float* de2, int64_t ldd2, jmac_stream_t stream);

/* Bitwise REPRODUCIBLE adjoint of the triple L1 scores for a score vector that fed the margin ranking loss of completion_loss
 * directly (T = B (K + 1) triples, the batch layout of train.py:347-352, src/jmac_model.py:345-378): the score gradient is derived
 * inside the kernel from the scores, gamma (device scalar) and gloss (device scalar, the loss' incoming gradient) by
 * jmac_margin_loss_bwd_f32's rule -- no dscore vector, no launch for it.  That gradient is (gloss / (2 B K)) times an INTEGER
 * matrix (the weights of torch.max are 0, 1/2 or 1), so the float atomics add exact small integers -- order-independent below
 * 2^24 -- into PERSISTENT count tables cnt_ent [rows_ent, d] / cnt_rel [rows_rel, d] (dense, 16-byte aligned, ZERO on entry and
 * left at zero again) at the windows [ent_off ..), [rel_off ..) the ids are local to; a scaling pass writes dent / drel (dense,
 * all rows) = cnt * gloss / (2 B K) as their FIRST WRITER, or on top of their contents where acc_ent / acc_rel != 0 (e.g. the
 * rows jmac_pair_cosine_bwd_rows_f32 wrote).  d % 4 == 0; 4 B K >= 2^24: JMAC_ERANGE (use jmac_margin_loss_bwd_f32 and
 * jmac_triple_l1_bwd_f32). */
int jmac_triple_l1_margin_bwd_exact2_f32(const float* ent, int64_t lde, const float* rel, int64_t ldr, const int64_t* h,
                                         const int64_t* r, const int64_t* t, int64_t B, int64_t K, int64_t d,
                                         const float* score, const float* gamma, const float* gloss, int64_t ent_off,
                                         int64_t rel_off, float* cnt_ent, float* cnt_rel, float* dent, int64_t rows_ent,
                                         int32_t acc_ent, float* drel, int64_t rows_rel, int32_t acc_rel,
                                         jmac_stream_t stream);

/* The same adjoint in ONE pass over the rows: the forward of a pass that needs table gradients.  Writes score [B (K + 1)] --
 * bit-identical to jmac_triple_l1_fwd_f32's with period = B -- and adds the integer counts of the adjoint above (2 w sgn(.), w
 * from the fresh scores and gamma) into cnt_ent / cnt_rel (dense, pitch d, ZERO on entry) at the windows [ent_off ..),
 * [rel_off ..): they do not depend on the loss' incoming gradient.  One workgroup per run b (the K + 1 triples b, B + kB + b that
 * share (h, r)); a run adds its h row, its r row and the positive's tail row once, each negative's tail row once; a negative
 * whose (h, r) is not the run's is still handled correctly.  The tables then hold what jmac_triple_l1_margin_bwd_exact2_f32 holds
 * before its scaling pass, and jmac_margin_counts_scale_clear_f32 is that pass alone: dent / drel (dense, all rows, first writer
 * or on top of their contents where acc_ent / acc_rel != 0) = cnt * gloss / (2 B K), cnt = 0 again.  The caller owns the tables
 * between the two calls (jmac_amd.losses: one pair per pending autograd node).  Same limits as the adjoint above. */
int jmac_triple_l1_margin_fwd_counts_f32(const float* ent, int64_t lde, const float* rel, int64_t ldr, const int64_t* h,
                                         const int64_t* r, const int64_t* t, int64_t B, int64_t K, int64_t d,
                                         const float* gamma, int64_t ent_off, int64_t rel_off, float* cnt_ent,
                                         float* cnt_rel, float* score, jmac_stream_t stream);
int jmac_margin_counts_scale_clear_f32(float* cnt_ent, float* cnt_rel, const float* gloss, int64_t B, int64_t K, int64_t d,
                                       float* dent, int64_t rows_ent, int32_t acc_ent, float* drel, int64_t rows_rel,
                                       int32_t acc_rel, jmac_stream_t stream);

/* out[0] = mean(x[0..n)) + (add_to ? add_to[0] : 0), fixed summation order -- a step's loss terms chain through add_to instead
 * of through element-wise adds. */
int jmac_vec_mean_acc_f32(const float* x, int64_t n, const float* add_to, float* out, jmac_stream_t stream);

/* dist[x] = 1 - <u, v>, u = e1[i1[x]] / max(||.||, 1e-12), v = e2[i2[x]] / max(||.||, 1e-12)
 * (replaces F.normalize(E[idx]) x2 + sum of alignment_loss / alignment_loss_simple,
 * src/jmac_model.py:245-247, 271-291). */
int jmac_pair_cosine_fwd_f32(const float* e1, int64_t ld1, const float* e2, int64_t ld2,
                             const int64_t* i1, const int64_t* i2, int64_t L, int64_t d, float* dist,
                             jmac_stream_t stream);
/* Adjoint into de1 [N1,d] / de2 [N2,d] (zeroed by the caller); float atomics. */
int jmac_pair_cosine_bwd_f32(const float* e1, int64_t ld1, const float* e2, int64_t ld2,
                             const int64_t* i1, const int64_t* i2, int64_t L, int64_t d,
                             const float* gdist, float* de1, int64_t ldd1, float* de2, int64_t ldd2,
                             jmac_stream_t stream);

/* Margin ranking loss of completion_loss (src/jmac_model.py:351-378) on the [B + B*K] score vector of one batch, with the
 * reference's n-major consumption of the negative block kept (neg_{b,k} = score[B + k*B + b]):
 *   loss[0] = mean_{b<B,k<K} max(score[b] - neg_{b,k}, -gamma[0]) + gamma[0] + (add_to ? add_to[0] : 0)
 * gamma: DEVICE pointer (the model's margin_completion parameter); add_to: the step's running loss (may be NULL).
 * bwd: dscore [B + B*K] = gloss[0] * d loss / d score (a tie diff == -gamma receives half the gradient, as torch.max(a, b)
 * gives it).  One launch each way, fixed summation order. */
int jmac_margin_loss_fwd_acc_f32(const float* score, int64_t B, int64_t K, const float* gamma, const float* add_to,
                                 float* loss, jmac_stream_t stream);
int jmac_margin_loss_bwd_f32(const float* score, int64_t B, int64_t K, const float* gamma,
                             const float* gloss, float* dscore, jmac_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Completion batches (replaces: TrainDataset.get_neg_sample, modules/load/data_loader.py:36-47 -- K distinct entities drawn
 * uniformly from those that are not a true tail of (h, r), the dictionary of train.py:262-285 -- its DataLoader workers, and
 * the repeat / cat of train.py:347-352).
 * --------------------------------------------------------------------------------------------- */

/* One training batch, built on the device: row b is triple perm[(step[1] mod (T / B)) * B + b] of triples [T,3] (h, r, t), and
 *   batch_h[j*B + b] = h_b, batch_r[j*B + b] = r_b (j = 0..K), batch_t[b] = t_b, batch_t[B + b*K + k] = neg[b, k]
 * ([B (K+1)] each: the layout of train.py:347-352, where neg.view(-1) pairs row b's negatives with other heads; kept).
 * neg[b, 0..K) = the first K VALID candidates of row b's stream, where candidate i = word i % 4 of
 *   philox4x32_10(counter = (b, lo32(step[0]), i / 4, hi32(step[0])), key = (lo32(seed[0]), lo32(seed[1]))),
 * m = word * num_ent (64-bit product), c_i = m >> 32, and c_i is invalid if lo32(m) < 2^32 mod num_ent, or c_i is in
 * tail_idx[tail_ptr[key_of_triple[.]] .. tail_ptr[. + 1]) (the SORTED DISTINCT true tails of the row's (h, r)), or c_i equals a
 * candidate accepted before it: a uniform draw without replacement from the allowed entities, one wave per row.
 * seed: device, 2 words, read.  step: device, 2 words, both read and then advanced by 1 on the device ([0] launches so far,
 * never reset by the caller; [1] batch number in the epoch, zeroed by the caller with every new perm), so a captured launch
 * replayed N times gives the N batches of N calls.  1 <= K <= 64, B >= 1, T >= B (JMAC_EINVAL), num_ent, B, T < 2^31
 * (JMAC_ERANGE).  Preconditions the host vouches for: perm and key_of_triple entries in range, triples' ids in [0, num_ent),
 * and every key leaves at least K entities (a row that cannot be filled ends with copies of its gold tail). */
int jmac_sample_completion_batch(const int64_t* triples, int64_t T, const int64_t* perm, const int32_t* key_of_triple,
                                 const int32_t* tail_ptr, const int32_t* tail_idx, int64_t num_ent, int64_t B, int64_t K,
                                 const int64_t* seed, int64_t* step, int64_t* batch_h, int64_t* batch_r, int64_t* batch_t,
                                 jmac_stream_t stream);

/* The same batch with HARD negatives in front (BootEA's truncated sampling: --neg_sampling truncated, generate_neg_triples* with
 * neighbor=, modules/train/batch.py:88-165): nbr[e * ldn + j], j < M, is the j-th neighbour of entity e (int32; any content).  Row b
 * with triple (h, r, t) and true-tail slice F of (h, r):
 *   lane l < M holds n_l = nbr[t * ldn + l] and is ELIGIBLE if n_l is in [0, num_ent), n_l is not in F (t itself is) and no j < l has
 *   n_j == n_l; A = eligible lanes, want1 = min(n_hard, A).
 *   Stage 1: candidate i = word i % 4 of philox4x32_10(counter = (b, lo32(step[0]), 0x80000000 | i / 4, hi32(step[0])), same key) --
 *   the top bit keeps the stream apart from stage 2's -- m = word * M, s = m >> 32; the candidate is invalid if lo32(m) < 2^32 mod M,
 *   if lane s is not eligible, or if s was accepted before; neg[b, 0..want1) = n_s of the first want1 valid candidates.
 *   Stage 2: neg[b, want1..K) by jmac_sample_completion_batch's rule on its own counters (third word i / 4 from 0), a candidate
 *   being invalid also when it equals a value stage 1 placed.
 * Hence n_hard == 0, or a table with no eligible lane, gives jmac_sample_completion_batch's batch bit for bit.  Stage 2 exists
 * because A < n_hard is ordinary (neighbours that are true tails; a short or repeating list) and the loss needs K negatives.
 * 1 <= M <= 64, ldn >= M, 0 <= n_hard <= K (JMAC_EINVAL); everything else -- layout, seed, step, perm, the other checks and
 * preconditions -- as above. */
int jmac_sample_completion_batch_truncated(const int64_t* triples, int64_t T, const int64_t* perm, const int32_t* key_of_triple,
                                           const int32_t* tail_ptr, const int32_t* tail_idx, int64_t num_ent, int64_t B, int64_t K,
                                           const int32_t* nbr, int64_t ldn, int64_t M, int64_t n_hard, const int64_t* seed,
                                           int64_t* step, int64_t* batch_h, int64_t* batch_r, int64_t* batch_t, jmac_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * torch_scatter-compatible primitives (replace the third-party calls at src/jmac_model.py:105 and
 * modules/helper/message_passing.py:24,28) so the UNMODIFIED reference layer can run on this library.
 * index need not be sorted.  out must be pre-zeroed by the caller for scatter_sum.
 * --------------------------------------------------------------------------------------------- */
int jmac_scatter_sum_f32(const float* src, const int64_t* index, int64_t E, int64_t d, int64_t N,
                         float* out, jmac_stream_t stream);
size_t jmac_scatter_softmax_workspace_bytes(int64_t N, int64_t d);
int jmac_scatter_softmax_f32(const float* src, const int64_t* index, int64_t E, int64_t d, int64_t N,
                             float* out, void* ws, size_t ws_bytes, jmac_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* JMAC_HIP_H_ */
