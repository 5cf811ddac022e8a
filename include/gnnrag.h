/* gnnrag.h - C ABI of libgnnrag_hip.so: the MI355X (gfx950) implementation of the
 * GNN-RAG / ReaRev reasoning hot path.
 *
 * The reference (cmavro/GNN-RAG @ v2) is pure Python: it has NO plugin / operator / FFI
 * interface for this path.  The seam is the Python class
 * `ReasonGNNLayer` (gnn/modules/kg_reasoning/reasongnn.py:10-174) plus `TypeLayer`
 * (gnn/modules/layer_init.py:9-65); the entry points below are what a ctypes binding inside
 * those classes calls (the binding itself is shown in INTEGRATION.md and shipped as
 * gnn-rag_amd/modules/).  Each entry point cites the reference code it replaces.
 *
 * Conventions
 *  - plain C: pointers + sizes only, no torch types.  All data pointers are DEVICE pointers
 *    owned by the caller; the library never allocates, frees or retains them.
 *  - all work is enqueued on the given hipStream_t (passed as void*); no internal
 *    synchronisation (one exception: gnnrag_csr_build waits for the stream once, to hand the
 *    relation counts back to the host), re-entrant per stream.  No state that affects results:
 *    the only process-wide data are idempotent per-device caches of launch attributes (raised
 *    dynamic-LDS caps, CU counts), keyed by the device current at the call, so one process may
 *    drive several GPUs.
 *  - buffers: every output is written at exactly the stated shape and every workspace / structure memory / scratch
 *    block within the bytes its gnnrag_*_bytes function states - nothing in front of or behind them is read into a
 *    result or written, and no result depends on what an output or a workspace held before the call (outputs are
 *    fully written unless an entry point says that it updates listed rows only).  A byte count below the stated size
 *    is refused with GNNRAG_E_WORKSPACE before anything is launched, also where the kernel form a particular call
 *    takes would get by with less.  tests/test_gpu_guarded.py holds every entry point to this.
 *  - fp32 values, int32 indices, row-major contiguous.
 *  - return value: 0 = success; > 0 = hipError_t of a failed runtime call / launch;
 *    < 0 = GNNRAG_E_* argument error.  gnnrag_error_string() renders either.
 *  - node index = question * N + slot (the reference pre-offsets heads/tails the same
 *    way, gnn/dataset_load.py:483,492-493); direction 0 = forward (head -> tail),
 *    direction 1 = inverse (tail -> head).
 */
#ifndef GNNRAG_H_
#define GNNRAG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNNRAG_ABI_VERSION 16

#define GNNRAG_E_BADARG      (-1)  /* null pointer / negative size / inconsistent sizes   */
#define GNNRAG_E_UNSUPPORTED (-2)  /* shape outside the compiled kernel set (see DESIGN)  */
#define GNNRAG_E_WORKSPACE   (-3)  /* caller-provided buffer too small                    */
#define GNNRAG_E_TUPLE       (-4)  /* edge tuple invalid: node / relation id out of range,
                                      or a fact whose head and tail lie in two questions  */

typedef void* gnnrag_stream_t; /* hipStream_t */

/* Destination-sorted structure of one batch of question subgraphs, both directions.
 * Replaces the 7 COO tensors of BaseGNNLayer.build_matrix (base_gnn.py:19-51), of which
 * ReaRev uses fact2tail/head2fact (forward) and fact2head/tail2fact (inverse).
 * Facts of one destination are stored in ascending fact id - except hub rows (more than heavy_deg
 * facts), which are stored in ascending (relation id, fact id) so that the walk can add the priors of
 * a run of equal relations and fetch the run's table row once - so every sum has one fixed order
 * (bit-reproducible, independent of how a batch is sharded over GPUs). */
typedef struct gnnrag_csr {
  int32_t B;            /* questions in the batch                                          */
  int32_t N;            /* max_local_entity: node slots per question                       */
  int32_t R1;           /* rows of the relation tables (num_kb_relation + 1)               */
  int32_t heavy_deg;    /* rows with more facts than this are walked by a whole workgroup  */
  int64_t F;            /* facts (typed edges + self loops) in the batch                   */
  int32_t* row_ptr[2];  /* [B*N+1]  first fact of each destination node                    */
  int32_t* edge[2];     /* [F][2]   (source node, relation id) per fact, sorted by dst     */
  int32_t* perm[2];     /* [F]      sorted position -> fact id of the caller's tuple       */
  float*   w_gnn[2];    /* [F] v_f^2 (normalized_gnn: weight enters both sparse products,
                                      base_gnn.py:38-47) or NULL                           */
  float*   w_rel[2];    /* [F] weight_rel_list (TypeLayer norm_rel, layer_init.py:39-40)
                                      or NULL                                              */
  int32_t* heavy[2];    /* [heavy_cap] list of heavy destination nodes, ascending          */
  int32_t* chunk_off[2];/* [heavy_cap+1] first 256-fact chunk of each heavy node (prefix)  */
  int32_t* n_heavy;     /* [2] device counters: heavy nodes per direction                  */
  int32_t* n_chunks;    /* [2] device counters: heavy chunks per direction                 */
  int32_t  heavy_cap;
  int32_t  max_chunks;  /* upper bound of n_chunks[d] (sizes the partial-sum workspace)    */
  int32_t* big_cnt;     /* [B]    nodes of each question with > big_deg facts in a direction */
  int32_t* big_nodes;   /* [B][N] their node ids (order irrelevant)                         */
  int32_t  big_deg;
  int32_t  hub_sorted;  /* 1: hub rows are in (relation, fact id) order (built with R1 > 1024), 0: fact order   */
  /* Per-question relation compaction (fused path).  A question's subgraph touches a small part of
   * the KB's relation vocabulary (hundreds of Freebase's ~6k relations), so its relation tables
   * are built over the relations it USES: compact row rel_off[b] + j  <->  (b, j-th smallest
   * relation id used by question b). */
  int32_t* edge_l[2];   /* [F][2]   (source node, compact relation index within its question)  */
  int32_t* rel_off;     /* [B+1]    first compact row of each question (prefix sum)            */
  int32_t* rel_rows;    /* [rel_total][2]  (question, relation id) of every compact row        */
  int32_t  rel_total;   /* compact rows in the batch (host copy, filled by gnnrag_csr_build)   */
  int32_t  rel_max;     /* largest number of relations used by one question                    */
  /* Merged rows (fused LDS walk): the facts arriving at node n in direction 0 followed by those of direction 1 form
   * ONE run [row_ptr[0][n] + row_ptr[1][n], row_ptr[0][n+1] + row_ptr[1][n+1]) of a 2F-long stream.  edge_m holds the
   * (source node, compact relation) records in that order - direction 1's relation index offset by the question's
   * relation count + 1, so that it addresses the second table slice behind the first one's zero row - and m_from
   * where each record came from (d * F + sorted position in direction d: the per-fact weights are read through it).
   * The walk then steps through a node's facts of both directions in one loop (same summation order: direction 0's
   * facts in ascending fact id, then direction 1's). */
  int32_t* edge_m;      /* [2F][2]                                                              */
  int32_t* m_from;      /* [2F]                                                                 */
  int32_t* m_dst;       /* [2F]  destination node of every merged record: for callers that cut the merged stream into
                                 equal fact ranges (no kernel of this library reads it any more)         */
  /* Dense hub form of the gather walk (tables larger than LDS): the hubs of question b are the list entries
   * hub_q_off[d][b] .. hub_q_off[d][b+1]; hub_wbase[d][b] = sum over earlier questions of hubs x relations in use
   * (rounded up to 4) = offset of the question's hub-by-relation weight block (saturates at INT32_MAX). */
  int32_t* hub_q_off[2];/* [B+1]                                                                */
  int32_t* hub_wbase[2];/* [B+1]                                                                */
} gnnrag_csr;

/* Bytes of caller-owned device memory a gnnrag_csr needs (persistent part / build scratch). */
size_t gnnrag_csr_bytes(int64_t F, int32_t B, int32_t N, int32_t R1, int has_w_gnn, int has_w_rel);
size_t gnnrag_csr_scratch_bytes(int64_t F, int32_t B, int32_t N, int32_t R1);

/* Builds the structure on the device.  heads/rels/tails are the batch tuple's first three
 * arrays (dataset_load.py:527) narrowed to int32; w_gnn = weight_list (used when
 * args['normalized_gnn']), w_rel = weight_rel_list (used when norm_rel), either may be NULL.
 * Replaces BaseGNNLayer.build_matrix (base_gnn.py:19-51) and the two COO builds inside
 * TypeLayer.forward (layer_init.py:35-36,53-54).  The tuple is validated on the device (node ids in
 * [0, B*N), relation ids in [0, R1), no fact across two questions): GNNRAG_E_TUPLE otherwise.
 * Synchronises `stream` once at the end (rel_total / rel_max are returned in *out). */
int gnnrag_csr_build(const int32_t* heads, const int32_t* rels, const int32_t* tails,
                     const float* w_gnn, const float* w_rel,
                     int64_t F, int32_t B, int32_t N, int32_t R1,
                     void* csr_mem, size_t csr_bytes, void* scratch, size_t scratch_bytes,
                     gnnrag_csr* out, gnnrag_stream_t stream);

/* gnnrag_csr_build WITHOUT the wait for the stream: the caller passes what the build would otherwise read back -
 * rel_total = sum over the questions of the distinct relation ids among a question's facts, rel_max = the largest such
 * count (a fact cache knows both per question when it caches it).  Everything is enqueued and
 * the call returns; the tuple's validation bits and the device-side counts stay behind the structure and
 * gnnrag_csr_status reads them back (one stream wait) whenever the caller wants the check.  Wrong counts are the
 * caller's error: a too small rel_total makes the fused path's tables too short.  rel_total < 0 or rel_max < 0: the
 * waiting form (= gnnrag_csr_build).  Replaces the same reference code (base_gnn.py:19-51). */
int gnnrag_csr_build_counts(const int32_t* heads, const int32_t* rels, const int32_t* tails,
                            const float* w_gnn, const float* w_rel,
                            int64_t F, int32_t B, int32_t N, int32_t R1, int32_t rel_total, int32_t rel_max,
                            void* csr_mem, size_t csr_bytes, void* scratch, size_t scratch_bytes,
                            gnnrag_csr* out, gnnrag_stream_t stream);
/* 0 when the structure's tuple passed the device-side validation and its relation counts equal the device's;
 * GNNRAG_E_TUPLE / GNNRAG_E_BADARG otherwise.  Waits for `stream`. */
int gnnrag_csr_status(const gnnrag_csr* csr, gnnrag_stream_t stream);

/* The structure of a batch as the CONCATENATION of per-question structures that are already on the device (SURVEY.md
 * section 8 f-1: "cached per-question int32 CSR built once at load time, batch = concatenation with offsets").
 * parts: HOST array of B structures, each built by gnnrag_csr_build with B = 1 for ONE question (node ids 0 .. N-1,
 * the same N and R1); question b of the batch gets node ids b * N .., facts in the order of `parts` (the order of the
 * reference's batch tuple, dataset_load.py:481-506).  Questions are disjoint node ranges and the structure is sorted
 * by destination node, so no sort is needed: every array is a copy with offsets added.  The result is bit-identical
 * to gnnrag_csr_build on the concatenated tuple.  No scratch, no synchronisation (rel_total / rel_max are sums / the
 * maximum of the parts' host fields).  Per-fact weights are attached afterwards (gnnrag_csr_permute_weight).
 * csr_mem: gnnrag_csr_bytes(sum of the parts' F, B, N, R1, 0, 0) bytes. */
int gnnrag_csr_concat(const gnnrag_csr* const* parts, int32_t B, int32_t N, int32_t R1, void* csr_mem, size_t csr_bytes,
                      gnnrag_csr* out, gnnrag_stream_t stream);

/* HOST helper (no device work): narrows the batch tuple's int64 id arrays (dataset_load.py:527) into one [3, F]
 * int32 block (heads, rels, tails) with up to `nthreads` threads and checks that every id lies in [0, 2^31):
 * GNNRAG_E_TUPLE otherwise.  `out` is host memory (pinned memory makes the following upload faster). */
int gnnrag_narrow_tuple(const int64_t* heads, const int64_t* rels, const int64_t* tails, int64_t F,
                        int32_t* out, int32_t nthreads);

/* Permutes a per-fact weight array of the caller's tuple into the structure's sorted order for
 * both directions: out_d[i] = w[perm_d[i]] (squared if square != 0).  Lets a binding attach
 * weight_list / weight_rel_list lazily (only when normalized_gnn / norm_rel ask for them). */
int gnnrag_csr_permute_weight(const gnnrag_csr* csr, const float* w_per_fact, int square,
                              float* out_fwd, float* out_inv, gnnrag_stream_t stream);

/* Math mode of the dense projections, an argument of every entry point that multiplies matrices
 * (gnnrag_linear*, gnnrag_update_score*, gnnrag_relation_tables, gnnrag_reason_layer):
 *   GNNRAG_MATH_FP32   v_mfma_f32_16x16x4_f32: bit-exact fp32 fmaf chains;
 *   GNNRAG_MATH_BF16X3 each fp32 operand split EXACTLY into three bf16 planes, six plane products
 *                      on v_mfma_f32_16x16x32_bf16 with fp32 accumulation: per-product relative
 *                      error <= 3*2^-24 (fp32 class), about 2.5x the fp32 MFMA rate. */
#define GNNRAG_MATH_FP32   0
#define GNNRAG_MATH_BF16X3 1
/* GNNRAG_MATH_MIXED: per kernel the faster of the two fp32-class forms - bf16x3 where a W-resident bf16x3 kernel
 * exists (relation tables, self-block update at hidden size 193..208) and on the k-tiled kernel, exact fp32 on the
 * W-resident fp32 update kernel (other hidden sizes) and on the skinny kernel (small M: the relation transforms). */
#define GNNRAG_MATH_MIXED  2

/* C[M,Nout] = act( A[M,K] . W[Nout,K]^T + bias[Nout] + add[row < add_rows, :] ), fp32 MFMA.
 * Used for  T_d = rel_linear_step(rel_features_d) (+ pos_emb_d(rel)), computed once per
 * relation row instead of once per fact (reasongnn.py:71,75-79 / :98,102-105), and for
 * TypeLayer's kb_self_linear(rel_features) (layer_init.py:47-49).
 * bias/add may be NULL.  relu != 0 applies max(.,0). */
int gnnrag_linear(const float* A, int64_t M, int32_t K, const float* W, const float* bias,
                  const float* add, int64_t add_rows, int relu,
                  float* C, int32_t Nout, int32_t math, gnnrag_stream_t stream);

/* Two gnnrag_linear problems that share W, bias and shapes (the forward and inverse relation
 * transforms of one layer call) in ONE launch. */
int gnnrag_linear_pair(const float* A0, const float* A1, int64_t M, int32_t K, const float* W,
                       const float* bias, const float* add0, const float* add1, int64_t add_rows,
                       float* C0, float* C1, int32_t Nout, int32_t math, gnnrag_stream_t stream);

/* agg[n, 2i+d, :] = sum_{f: dst_d(f)=n} w_f * dist[src_d(f)] * relu(T_d[rel_f,:] * ins[n/N, i, :])
 * = reason_layer (reasongnn.py:61-89, d=0) and reason_layer_inv (reasongnn.py:91-116, d=1)
 * for every instruction i, in the concat order of reasongnn.py:150-158.
 * dist [B*N], ins [B,I,D], T_fwd/T_inv [R1,D], agg [B*N, 2*I*D]. */
size_t gnnrag_aggregate_workspace_bytes(const gnnrag_csr* csr, int32_t D, int32_t I);
int gnnrag_aggregate(const gnnrag_csr* csr, const float* dist, const float* ins,
                     const float* T_fwd, const float* T_inv, float* agg,
                     int32_t D, int32_t I, void* workspace, size_t workspace_bytes,
                     gnnrag_stream_t stream);

/* Fused form of the same aggregation: e2e_linear is linear over the concatenated blocks, so it is
 * applied to the per-question relation tables first (gnnrag_relation_tables) and the walk emits
 *   out[n,:] = sum_d sum_{f: dst_d(f)=n} w_f * dist[src_d(f)] * P[d, row(n/N, rel_f), :]    [B*N, D]
 * = sum_k W_e2e[:, block k] . agg[n,k,:], i.e. the neighbour part of reasongnn.py:161-163 without
 * ever writing agg.  P [2,rel_total,D] over the compact rows.
 * workspace: gnnrag_aggregate_workspace_bytes(csr, D, 1). */
int gnnrag_aggregate_fused(const gnnrag_csr* csr, const float* dist, const float* P, float* out,
                           int32_t D, void* workspace, size_t workspace_bytes,
                           gnnrag_stream_t stream);

/* Which kernel gnnrag_aggregate_fused dispatches for this structure and hidden size (decided on the
 * host from rel_max and D, nothing is launched): lets tests and bench.py name the kernel they ran. */
#define GNNRAG_WALK_L2_GATHER 0  /* k_walk_light<FUSED>: table rows gathered from L2 (tables exceed a CU's LDS) */
#define GNNRAG_WALK_LDS_16    1  /* k_walk_slice<FUSED,1>: 16-column table slices in LDS                      */
#define GNNRAG_WALK_LDS_32    2  /* k_walk_slice<FUSED,2>: 32-column slices (small per-question tables)       */
int gnnrag_aggregate_fused_variant(const gnnrag_csr* csr, int32_t D);

/* Which form the HUB ROWS of the gather walk take in a gnnrag_aggregate_fused call with this structure, hidden size and
 * workspace (the sizes of the hub-by-relation weight blocks live on the device, so the kernels decide; this entry runs
 * the same predicate on the same kernel arguments in a one-thread launch).  form_dev: 4 device int32 -
 * [0] GNNRAG_HUB_FORM_*, [1] / [2] hub rows of direction 0 / 1, [3] relation ranges per question.  Diagnostics for
 * tests and bench.py ("which kernel ran"); nothing on the product path calls it.  No size is stated for `workspace`:
 * pass what the gnnrag_aggregate_fused call in question gets (the answer depends on it); less than the walk's partial
 * sums need is GNNRAG_E_WORKSPACE. */
#define GNNRAG_HUB_FORM_NONE    0  /* the call has no dense hub kernels (LDS walk, or the form is switched off)   */
#define GNNRAG_HUB_FORM_DENSE   1  /* k_hub_weights / k_hub_dense / k_hub_finish                                   */
#define GNNRAG_HUB_FORM_CHUNKED 2  /* weight blocks do not fit the workspace: k_heavy_partial / k_heavy_reduce     */
int gnnrag_aggregate_fused_hub_form(const gnnrag_csr* csr, int32_t D, void* workspace, size_t workspace_bytes,
                                    int32_t* form_dev, gnnrag_stream_t stream);

/* h_out = relu(e2e_linear(cat(h, agg)))            (reasongnn.py:161-163)
 * score = score_func(h_out) + (1 - mask) * -1e11   (reasongnn.py:165-168), mask add in fp32.
 * h [BN,D], agg [BN,2I*D], W [D,(2I+1)D], b [D], w_s [D], b_s [1] (device), mask [BN]. */
int gnnrag_update_score(const float* h, const float* agg, const float* W, const float* b,
                        const float* w_s, const float* b_s, const float* mask,
                        float* h_out, float* score, int64_t BN, int32_t D, int32_t I, int32_t math,
                        gnnrag_stream_t stream);

/* dist[g,:] = softmax(score[g,:]) over the N slots of each question (reasongnn.py:169). */
int gnnrag_masked_softmax(const float* score, float* dist, int32_t B, int32_t N,
                          gnnrag_stream_t stream);

/* h0[n,:] = relu( sum_{tail_f=n} v_f T[rel_f,:] + sum_{head_f=n} v_f T[rel_f,:] ),
 * v_f = w_rel if use_w_rel else 1   (TypeLayer.forward, layer_init.py:53-57);
 * T [R1,D] = kb_self_linear(rel_features) from gnnrag_linear.
 * workspace: gnnrag_aggregate_workspace_bytes(csr, D, 1). */
int gnnrag_typelayer(const gnnrag_csr* csr, const float* T, int use_w_rel, float* h0,
                     int32_t D, void* workspace, size_t workspace_bytes, gnnrag_stream_t stream);

/* Facts of a batch ordered by (question, relation), for the backward's table gradients: row = compact
 * relation row of gnnrag_csr (rel_rows), facts of a row in ascending fact id, rows cut into chunks of
 * at most 256 facts.  Built on first use (training only) from the same int32 tuple as the structure. */
typedef struct gnnrag_relorder {
  int64_t  F;
  int32_t  rel_total;
  int32_t  n_chunks;    /* host copy, filled by gnnrag_relorder_build                                */
  int32_t* ht;          /* [F][2]  (head node, tail node) per fact in (question, relation) order     */
  int32_t* perm;        /* [F]     position in that order -> fact id of the caller's tuple           */
  float*   w;           /* [F]     v_f^2 in that order (normalized_gnn) or NULL                      */
  int32_t* row_ptr;     /* [rel_total+1] first position of each compact relation row                 */
  int32_t* chunk_ptr;   /* [rel_total+1] first chunk of each row (prefix of ceil(len/256))           */
} gnnrag_relorder;
size_t gnnrag_relorder_bytes(const gnnrag_csr* csr, int has_w);
size_t gnnrag_relorder_scratch_bytes(const gnnrag_csr* csr);
/* heads/rels/tails: the tuple the structure was built from; w_per_fact: weight_list (squared inside) or
 * NULL.  Synchronises `stream` once (n_chunks is returned in *out). */
int gnnrag_relorder_build(const gnnrag_csr* csr, const int32_t* heads, const int32_t* rels,
                          const int32_t* tails, const float* w_per_fact,
                          void* mem, size_t mem_bytes, void* scratch, size_t scratch_bytes,
                          gnnrag_relorder* out, gnnrag_stream_t stream);

/* Backward of gnnrag_aggregate (what autograd derives for reasongnn.py:61-116), so that training
 * (train_model.py:209-233) runs on the HIP operator.  g_agg [BN,2I*D] is the gradient of agg;
 *   g_dist [BN], g_ins [B,I,D], g_T_fwd / g_T_inv [R1,D]  are fully written (not accumulated into).
 * relorder != NULL (and D % 4 == 0, I <= 4): the table / instruction gradients are gathered over the
 * facts of each (question, relation) row - no atomics, one fixed summation order, any number of
 * relations per question.  relorder == NULL: relation-bucketed sums in LDS (ds_add_f32; reproducible
 * to rounding only; GNNRAG_E_UNSUPPORTED when one question uses more relations than one CU's LDS
 * holds, ~1200).
 * workspace: gnnrag_backward_workspace_bytes(csr, relorder, D, I) bytes of device scratch.  D <= 1024. */
size_t gnnrag_backward_workspace_bytes(const gnnrag_csr* csr, const gnnrag_relorder* relorder, int32_t D,
                                       int32_t I);
int gnnrag_aggregate_backward(const gnnrag_csr* csr, const gnnrag_relorder* relorder,
                              const float* dist, const float* ins,
                              const float* T_fwd, const float* T_inv, const float* g_agg,
                              float* g_dist, float* g_ins, float* g_T_fwd, float* g_T_inv,
                              int32_t D, int32_t I, void* workspace, size_t workspace_bytes,
                              gnnrag_stream_t stream);

/* Backward of gnnrag_aggregate_fused (training on the fused form, linear_dropout = 0):
 *   nbr[n, :] = sum_d sum_{f: dst_d(f)=n} w_f * dist[src_d(f)] * P[d, row(b, rel_f), :]
 *   g_dist[s]        = sum_d sum_{f: src_d(f)=s} w_f * < g_nbr[dst_d(f), :], P[d, row(b, rel_f), :] >
 *   g_P[d, row, :]   = sum_{f in row} w_f * dist[src_d(f)] * g_nbr[dst_d(f), :]
 * both fully written; the relation tables P themselves are a differentiable dense expression of a few ten thousand
 * rows on the caller's side (gnn-rag_amd/autograd.py: relation_tables_dense) or gnnrag_relation_tables with its own
 * backward, gnnrag_relation_tables_backward.  P and g_P must be real pointers also for
 * a batch without facts (rel_total == 0: nothing is read or written there; NULL is GNNRAG_E_BADARG, as for
 * gnnrag_aggregate_fused).  Needs the (question, relation) ordering
 * (gnnrag_relorder) and D % 4 == 0; gather kernels, chunk partials summed in a fixed order, no atomics.
 * workspace: gnnrag_backward_workspace_bytes(csr, relorder, D, 1). */
int gnnrag_aggregate_fused_backward(const gnnrag_csr* csr, const gnnrag_relorder* relorder, const float* dist,
                                    const float* P, const float* g_nbr, float* g_dist, float* g_P, int32_t D,
                                    void* workspace, size_t workspace_bytes, gnnrag_stream_t stream);

/* Backward of gnnrag_typelayer with respect to T (layer_init.py:47-57):
 *   g_T[r,:] = sum_{f: rel_f=r} v_f (g_pre[tail_f,:] + g_pre[head_f,:]),
 * g_pre [BN,D] = gradient of the pre-activation (= g_h0 where h0 > 0, else 0).  g_T [R1,D] is fully
 * written.  relorder != NULL and D % 4 == 0: atomic-free gather over the (question, relation) rows, v_f read
 * from w_rel_per_fact (weight_rel_list in the caller's fact order) when use_w_rel; else the LDS form with the
 * structure's own w_rel (limits as for gnnrag_aggregate_backward).
 * workspace: gnnrag_backward_workspace_bytes(csr, relorder, D, 1). */
int gnnrag_typelayer_backward(const gnnrag_csr* csr, const gnnrag_relorder* relorder, const float* g_pre,
                              const float* w_rel_per_fact, int use_w_rel, float* g_T,
                              int32_t D, void* workspace, size_t workspace_bytes, gnnrag_stream_t stream);

/* Weight gradient of a dense projection (what autograd derives for nn.Linear.weight):
 *   C[N1, N2] = A[M, N1]^T . B[M, N2]      e.g. dW = dY^T . X with A = dY [M, Nout], B = X [M, K].
 * Exact fp32 on the matrix cores; the row range is cut into chunks whose partial blocks are added in chunk order
 * (no atomics).  N1 % 4 == 0, N2 % 4 == 0, 16-byte aligned operands, else GNNRAG_E_UNSUPPORTED.
 * workspace: gnnrag_gemm_tn_workspace_bytes(M, N1, N2) bytes of device scratch. */
size_t gnnrag_gemm_tn_workspace_bytes(int64_t M, int32_t N1, int32_t N2);
int gnnrag_gemm_tn(const float* A, const float* B, int64_t M, int32_t N1, int32_t N2, float* C,
                   void* workspace, size_t workspace_bytes, gnnrag_stream_t stream);

/* Per-question relation tables of the fused path, one row per (question b, relation r used by b):
 *   P[d,row(b,r),:] = sum_i W_e2e[:, (1+2i+d)D : (2+2i+d)D] . relu(T_d[r,:] * ins[b,i,:])   [2,rel_total,D]
 * (the e2e_linear column blocks in the concat order of reasongnn.py:150-161).  The operand
 * relu(T_d * ins) is generated inside the GEMM's tile loader and never stored. */
int gnnrag_relation_tables(const gnnrag_csr* csr, const float* T_fwd, const float* T_inv, const float* ins,
                           const float* W_e2e, float* P, int32_t D, int32_t I, int32_t math,
                           gnnrag_stream_t stream);

/* h_out = relu(h . W_e2e[:, 0:D]^T + b + nbr), nbr [BN,D] from gnnrag_aggregate_fused; score as in
 * gnnrag_update_score.  Together: reasongnn.py:161-168. */
int gnnrag_update_score_fused(const float* h, const float* nbr, const float* W_e2e, const float* b,
                              const float* w_s, const float* b_s, const float* mask,
                              float* h_out, float* score, int64_t BN, int32_t D, int32_t I, int32_t math,
                              gnnrag_stream_t stream);

/* ---- Which kernel a dense call runs (additive to ABI 16) ---------------------------------------------------------------
 * HOST ONLY: no device, no HIP call.  Describes a gnnrag_linear / gnnrag_linear_pair / gnnrag_update_score /
 * gnnrag_update_score_fused call and returns what the launcher would choose - it runs the launchers' own decision
 * function on the same arguments (stand-in pointers carry the alignment), so tests can assert the kernel they mean to
 * test and a moved threshold fails a test instead of emptying it (the dense twin of gnnrag_aggregate_fused_variant).
 *   entry            GNNRAG_DENSE_ENTRY_*
 *   M, K, Nout       of the linear entry points; the update entry points pass (BN, D, I) in their place
 *   math             GNNRAG_MATH_*
 *   has_add/add_rows the linear entry points' `add` (ignored for the update entry points: nbr is always there)
 *   misaligned       OR of GNNRAG_DENSE_MISALIGNED_*: operands that are NOT 16-byte aligned
 *   block            column block (208 columns each) of a call that makes several launches; 0 otherwise
 * GNNRAG_E_BADARG: sizes <= 0, unknown entry / math, a block the call does not launch. */
#define GNNRAG_DENSE_ENTRY_LINEAR       0
#define GNNRAG_DENSE_ENTRY_LINEAR_PAIR  1   /* above the skinny bound: two gnnrag_linear calls, the form is theirs       */
#define GNNRAG_DENSE_ENTRY_UPDATE       2   /* gnnrag_update_score                                                     */
#define GNNRAG_DENSE_ENTRY_UPDATE_FUSED 3   /* gnnrag_update_score_fused                                               */
/* gnnrag_update_drop_train / _backward, (BN, D, I) as (M, K, Nout); has_add / add_rows are ignored.  _DX: the masked input
 * gradient, blocks 0 .. ceil(D / 208) - 1 are the launches of g_h, the following ceil(2 I D / 208) those of g_agg.
 * _DW: the masked weight gradient (GNNRAG_DENSE_GEMM_TN).  A shape or alignment outside the entries' limits:
 * GNNRAG_DENSE_NONE. */
#define GNNRAG_DENSE_ENTRY_UPDATE_DROP    4
#define GNNRAG_DENSE_ENTRY_UPDATE_DROP_DX 5
#define GNNRAG_DENSE_ENTRY_UPDATE_DROP_DW 6
/* gnnrag_relation_tables_backward, (rel_total, D, I) as (M, K, Nout); has_add / add_rows are ignored.  _DX: ONE of the 2 I
 * equal gnnrag_linear products [rel_total, D] x [D, D] in front of G (blocks 0 .. ceil(D / 208) - 1 above the skinny bound).
 * _DW: the weight gradient with the generated B operand (GNNRAG_DENSE_GEMM_TN).  Outside the entry's limits:
 * GNNRAG_DENSE_NONE. */
#define GNNRAG_DENSE_ENTRY_REL_TABLES_DX  7
#define GNNRAG_DENSE_ENTRY_REL_TABLES_DW  8
#define GNNRAG_DENSE_MISALIGNED_A   1       /* A / A0 / h                                                              */
#define GNNRAG_DENSE_MISALIGNED_W   2
#define GNNRAG_DENSE_MISALIGNED_C   4       /* C / C0 / h_out                                                          */
#define GNNRAG_DENSE_MISALIGNED_ADD 8       /* add / add0 / nbr                                                        */
#define GNNRAG_DENSE_MISALIGNED_A1  16      /* A1 of the pair / agg                                                    */
#define GNNRAG_DENSE_NONE          0        /* nothing is launched (GNNRAG_E_UNSUPPORTED)                              */
#define GNNRAG_DENSE_SKINNY        1        /* k_gemm_skinny: exact fp32 in every math mode, all columns in one launch  */
#define GNNRAG_DENSE_KTILED        2        /* k_gemm_f32<NT, MT, V4, EPI, AMODE_PLAIN, MATH, NW>                      */
#define GNNRAG_DENSE_WRES          3        /* k_gemm_wres<NT, NC, EPI_UPDATE, HAS_ADD, KGUARD, false>                 */
#define GNNRAG_DENSE_UPDATE_SKINNY 4        /* k_update_skinny                                                         */
#define GNNRAG_DENSE_UPDATE_B3     5        /* k_update_b3 (tables_b3.hip)                                             */
#define GNNRAG_DENSE_WIDE          6        /* D > 208: EPI_LINEAR column blocks, then k_score_rows                    */
#define GNNRAG_DENSE_GEMM_TN       7        /* k_gemm_tn with the masked split B operand, then k_tn_reduce (REL_TABLES_DW:
                                               the generated B operand, then k_rtb_w_reduce)                           */
typedef struct gnnrag_dense_form_t {
  int32_t family;        /* GNNRAG_DENSE_*                                                                               */
  int32_t block_family;  /* family of the described GEMM launch: = family, except WIDE (SKINNY or KTILED)                */
  int32_t launches;      /* GEMM launches of the call (column blocks; x 2 for a pair above the skinny bound)             */
  int32_t epi;           /* KTILED: 0 = EPI_LINEAR, 1 = EPI_UPDATE, 2 = EPI_KEEP (UPDATE_DROP_DX)                        */
  int32_t nt, mt, v4, math, nw;   /* KTILED template arguments (nt also WRES; v4 also SKINNY)                            */
  int32_t v4out, n0;     /* KTILED runtime: float4 epilogue, first output column of the block                            */
  int32_t nc, has_add, kguard;    /* WRES template arguments                                                             */
} gnnrag_dense_form_t;
int gnnrag_dense_form(int32_t entry, int64_t M, int32_t K, int32_t Nout, int32_t math, int32_t has_add, int64_t add_rows,
                      int32_t misaligned, int32_t block, gnnrag_dense_form_t* out);

/* One whole ReasonGNNLayer.forward (reasongnn.py:134-174) enqueued with a single call:
 * rel transform (both directions) -> aggregation -> update+score -> softmax.
 * path: GNNRAG_PATH_UNFUSED = aggregate [BN,2I*D] then one [(2I+1)D -> D] GEMM (the reference's
 * operator boundaries); GNNRAG_PATH_FUSED = relation tables -> fused aggregation -> self-block
 * GEMM (2.3x fewer flops and 4x less aggregation traffic when 2*rel_total*I < ~0.8*B*N*2I);
 * GNNRAG_PATH_AUTO picks by that flop model.  Results agree to fp32 rounding (re-association).
 * pos_fwd/pos_inv: pos_emb{step}.weight / pos_emb_inv{step}.weight [pos_rows,D] or NULL.
 * workspace: gnnrag_layer_workspace_bytes() bytes of device scratch. */
#define GNNRAG_PATH_AUTO    0
#define GNNRAG_PATH_UNFUSED 1
#define GNNRAG_PATH_FUSED   2
/* OR-ed into `path`: a layer that aggregates along ONE direction (NSMLayer: head -> tail, NSMLayer_back: tail ->
 * head; the caller's e2e weight block of the other direction must be zero).  Where the kernels at hand can leave a
 * direction out (V-form tables + LDS walk) only that direction's tables are built and walked; elsewhere both run and
 * the zero block makes the other contribute exactly 0 - results are identical either way. */
#define GNNRAG_PATH_ONLY_FWD 0x10
#define GNNRAG_PATH_ONLY_INV 0x20
/* OR-ed into `path`: the caller states that `dist` (gnnrag_reason_stack: dist0, i.e. layer 0 only) is a SEED
 * distribution - the first layer of every ReaRev iteration (rearev.py:208 resets curr_dist to seed_dist).  fact_prior
 * (reasongnn.py:80,106) is then zero for every fact that does not start at a seed, so the fused path computes only the
 * relation-table rows the seeds' facts use and the neighbour sums of the nodes they reach (the frontier, derived from
 * `dist` on the device: gnnrag_frontier_build).  A hint, not a promise: any prior gives the same results as without
 * the flag (to rounding of the relation-table products), a dense one slowly.  Needs D % 4 == 0, D <= 256, both
 * directions, the fused path; ignored otherwise. */
#define GNNRAG_PATH_SEED_PRIOR 0x40
/* OR-ed into `path` of gnnrag_reason_stack (with a gnnrag_stack_workspace_bytes workspace): the workspace still holds
 * the relation projections (and their bf16 planes) that an EARLIER gnnrag_reason_stack call on the same workspace
 * computed for the same layers' parameters and the same relation features - they depend on nothing else
 * (reasongnn.py:75-79: rel_linear{j}(rel_features)), so the iterations 2..T of one ReaRev forward skip that launch.
 * The caller vouches for "same parameters, same relation features, workspace untouched in between". */
#define GNNRAG_PATH_REUSE_PROJ 0x80
size_t gnnrag_layer_workspace_bytes(const gnnrag_csr* csr, int32_t D, int32_t I);
int gnnrag_reason_layer(const gnnrag_csr* csr,
                        const float* h, const float* dist, const float* ins,
                        const float* relfeat_fwd, const float* relfeat_inv,
                        const float* W_rel, const float* b_rel,
                        const float* pos_fwd, const float* pos_inv, int32_t pos_rows,
                        const float* W_e2e, const float* b_e2e,
                        const float* w_score, const float* b_score, const float* mask,
                        float* h_out, float* score_out, float* dist_out,
                        void* workspace, size_t workspace_bytes,
                        int32_t D, int32_t I, int32_t path, int32_t math, gnnrag_stream_t stream);

/* L consecutive ReasonGNNLayer.forward calls on one batch - what one iteration of ReaRev.forward does
 * (rearev.py:208-210: `for j in range(num_gnn): curr_dist, global_rep = reasoning(curr_dist, relation_ins, step=j)`)
 * enqueued with ONE call: layer j reads h[j-1] / dist[j-1] (h0 / dist0 for j = 0) and writes h_out[j], score_out[j],
 * dist_out[j] ([L, B*N, D] / [L, B*N] / [L, B*N], every layer's outputs are kept: the reference returns each of them
 * to its caller).  `layers` is a HOST array of L parameter sets.  Same arithmetic, kernels and workspace as L calls
 * of gnnrag_reason_layer (bit-identical results); what it removes is the per-call host work in front of ~8 short
 * kernels per layer, which bounds small batches (one question per batch: SURVEY.md section 8 f-3). */
typedef struct gnnrag_layer_params {
  const float* W_rel;    /* rel_linear{j}.weight [D, D]                      */
  const float* b_rel;    /* rel_linear{j}.bias   [D]                         */
  const float* pos_fwd;  /* pos_emb{j}.weight [pos_rows, D] or NULL          */
  const float* pos_inv;  /* pos_emb_inv{j}.weight [pos_rows, D] or NULL      */
  const float* W_e2e;    /* e2e_linear{j}.weight [D, (2I+1) D]               */
  const float* b_e2e;    /* e2e_linear{j}.bias [D]                           */
} gnnrag_layer_params;
/* Workspace of gnnrag_reason_stack that lets it compute the relation projections of all L layers up front in ONE
 * launch.  The size is gnnrag_layer_workspace_bytes + an [L][2][R1][D] fp32 block for the projections + L layers' bf16
 * planes of them where the V-form relation-table kernel applies to (D, I), the two additions each rounded up to 256
 * bytes - and nothing else.  A larger workspace is accepted.  With only gnnrag_layer_workspace_bytes the stack call
 * still works and projects per layer (same results bit for bit). */
size_t gnnrag_stack_workspace_bytes(const gnnrag_csr* csr, int32_t L, int32_t D, int32_t I);

/* T_out[j][d][r, :] = rel_linear{j}(rel_features_d[r, :]) (+ pos_emb{j}_d[r, :] for r < pos_rows), j < L, d = 0
 * forward / 1 inverse (reasongnn.py:75-79, :102-105): the relation projections of all layers in one launch, exact
 * fp32 on the matrix cores.  `layers` is a HOST array (only W_rel, b_rel, pos_fwd, pos_inv are read; pos_* are
 * ignored when pos_rows == 0).  D % 4 == 0, else GNNRAG_E_UNSUPPORTED.  T_out: [L, 2, R1, D] floats.
 * planes_out (may be NULL; D <= 224): gnnrag_rel_planes_bytes(R1, D, L) bytes, [L][2][3][R1][448] bf16 - per layer
 * and direction the three planes of the exact 3-way bf16 split of [relu(T[r, :]) | relu(-T[r, :])], each half padded
 * with zeros to 224 columns: the left operand of gnnrag_relation_tables_planes. */
size_t gnnrag_rel_planes_bytes(int64_t R1, int32_t D, int32_t L);
int gnnrag_rel_transform(const float* relfeat_fwd, const float* relfeat_inv, int64_t R1, int32_t D, int32_t L,
                         const gnnrag_layer_params* layers, int32_t pos_rows, float* T_out, void* planes_out,
                         gnnrag_stream_t stream);

/* gnnrag_relation_tables in the bf16x3 math mode from ONE layer's pre-split relation planes (gnnrag_rel_transform's
 * planes_out for that layer: [2][3][R1][448] bf16): since relu(t q) = max(q,0) relu(t) + max(-q,0) relu(-t),
 *   P[d,row(b,r),:] = [relu(T_d[r,:]), relu(-T_d[r,:])] . V_{b,d},
 *   V_{b,d} = [sum_i W_{i,d}^T diag(max(ins[b,i,:],0)) ; sum_i W_{i,d}^T diag(max(-ins[b,i,:],0))]   (W_{i,d} as above)
 * - the left operand is question independent and arrives as ready matrix-core fragments, the question sits in the
 * per-question right operand built in LDS.  Shapes: 193 <= D <= 208, D % 8 == 0, rel_total >= 1024; otherwise
 * GNNRAG_E_UNSUPPORTED (nothing launched; use gnnrag_relation_tables). */
int gnnrag_relation_tables_planes(const gnnrag_csr* csr, const void* planes, const float* ins, const float* W,
                                  float* P, int32_t D, int32_t I, gnnrag_stream_t stream);

/* The same two calls on the PACKED form of the left operand - what the layer sequence itself uses (additive to ABI 16).
 * Of relu(t) and relu(-t) at most one is not zero, so the 2:4 sparse product takes the planes of |T| and one sign bit per
 * element.  packed_out: gnnrag_rel_packed_bytes(R1, D, L) bytes (0 for D > 224), [L][2][R1][1408] bytes: per row the
 * three bf16 planes of the exact 3-way split of |T[r, :]| (224 values each, zeros from D on), then 64 index bytes.  The
 * index byte of the four columns 4q .. 4q+3 is 0x88 | s0 | s1 << 2 | s2 << 4 | s3 << 6, s = (T[r, k] < 0), stored at
 * byte (q % 8 / 2) * 16 + (q / 8) * 2 + q % 2 of the 64; the eight bytes without columns are 0.
 * gnnrag_relation_tables_packed: one layer's [2][R1][1408]; every element of P equals gnnrag_relation_tables_planes' bit
 * for bit.  only_dir: -1 both directions, 0 / 1 that direction alone (the other half of P is left unwritten). */
size_t gnnrag_rel_packed_bytes(int64_t R1, int32_t D, int32_t L);
int gnnrag_rel_transform_packed(const float* relfeat_fwd, const float* relfeat_inv, int64_t R1, int32_t D, int32_t L,
                                const gnnrag_layer_params* layers, int32_t pos_rows, float* T_out, void* packed_out,
                                gnnrag_stream_t stream);
int gnnrag_relation_tables_packed(const gnnrag_csr* csr, const void* packed, const float* ins, const float* W,
                                  float* P, int32_t D, int32_t I, int32_t only_dir, gnnrag_stream_t stream);

int gnnrag_reason_stack(const gnnrag_csr* csr, int32_t L, const gnnrag_layer_params* layers,
                        const float* h0, const float* dist0, const float* ins,
                        const float* relfeat_fwd, const float* relfeat_inv, int32_t pos_rows,
                        const float* w_score, const float* b_score, const float* mask,
                        float* h_out, float* score_out, float* dist_out,
                        void* workspace, size_t workspace_bytes,
                        int32_t D, int32_t I, int32_t path, int32_t math, gnnrag_stream_t stream);

/* The same L-layer sequence captured as a hipGraph (stream capture on `stream`, which must not be capturing): every
 * pointer and size is baked in, so a replay repeats the sequence on whatever the buffers hold then.  One batch's
 * T iterations replay one graph when the caller keeps the buffers in place: h0 = h_out + (L-1)*B*N*D (the previous
 * iteration's last layer; rearev.py:208-211 carries the node state over), dist0 = the seed distribution, `ins`
 * rewritten in place between replays (rearev.py:217-221).  Results are bit-identical to the eager sequence.
 * Run the eager call once before capturing (launch attributes are raised on first use). */
typedef struct gnnrag_graph gnnrag_graph;
int gnnrag_reason_stack_capture(const gnnrag_csr* csr, int32_t L, const gnnrag_layer_params* layers,
                                const float* h0, const float* dist0, const float* ins,
                                const float* relfeat_fwd, const float* relfeat_inv, int32_t pos_rows,
                                const float* w_score, const float* b_score, const float* mask,
                                float* h_out, float* score_out, float* dist_out,
                                void* workspace, size_t workspace_bytes,
                                int32_t D, int32_t I, int32_t path, int32_t math, gnnrag_stream_t stream,
                                gnnrag_graph** out);
int gnnrag_graph_launch(gnnrag_graph* graph, gnnrag_stream_t stream);
int gnnrag_graph_destroy(gnnrag_graph* graph);

/* The frontier form of the fused layer for a sparse prior (see GNNRAG_PATH_SEED_PRIOR), exposed piecewise for tests:
 *   gnnrag_frontier_build: nodes with dist != 0 are the sources; marks the nodes their facts reach (row gates: one
 *     byte per node at workspace offset ...) and the compact relation rows those facts use, and lists both;
 *   gnnrag_relation_tables_frontier: the listed rows of P [2, rel_total, D], written in place (exact fp32 MFMA);
 *   gnnrag_aggregate_fused_frontier: out[n, :] = sum_d sum_f p_f P[d, row(b, rel_f), :] for the listed nodes n ONLY
 *     (facts with p_f = 0 are skipped: they add exact zeros); every other row of `out` is left untouched.
 * fws: gnnrag_frontier_workspace_bytes(csr) bytes of device scratch shared by the three calls.
 * gnnrag_frontier_read copies (rows listed, relation rows listed) to the host (synchronises the stream; tests). */
size_t gnnrag_frontier_workspace_bytes(const gnnrag_csr* csr);
int gnnrag_frontier_supported(const gnnrag_csr* csr, int32_t D);
int gnnrag_frontier_build(const gnnrag_csr* csr, const float* dist, void* fws, size_t fws_bytes, gnnrag_stream_t stream);
int gnnrag_relation_tables_frontier(const gnnrag_csr* csr, const void* fws, const float* T_fwd, const float* T_inv,
                                    const float* ins, const float* W_e2e, float* P, int32_t D, int32_t I,
                                    gnnrag_stream_t stream);
int gnnrag_aggregate_fused_frontier(const gnnrag_csr* csr, const void* fws, const float* dist, const float* P,
                                    float* out, int32_t D, gnnrag_stream_t stream);
int gnnrag_frontier_read(const gnnrag_csr* csr, const void* fws, int32_t* counts2, uint8_t* row_flag_host,
                         gnnrag_stream_t stream);
/* Byte offsets inside fws (tests, tools): offsets8 = counts [B][2] int32 (listed nodes, listed relation rows of each
 * question), row gates [B N + 64] uint8, node lists [B N] int32 (question g's at g N), relation-row flags, relation-row
 * lists [rel_total] int32 (question g's at rel_off[g]), seeds [B][32] int32 (ascending; used when there are at most 32),
 * seedinfo [B][2] int32 (number of seeds or -1, facts that touch them), total bytes. */
int gnnrag_frontier_layout(const gnnrag_csr* csr, uint64_t* offsets8);
/* What gnnrag_reason_stack launches in front of a seed layer (GNNRAG_PATH_SEED_PRIOR): gnnrag_rel_transform_packed
 * (packed_out may be null: T alone) for csr->R1 relation rows AND gnnrag_frontier_build of `dist`, which also zeroes
 * zero_na floats at zero_a and zero_nb at zero_b (either may be null / 0), in ONE launch whose workgroups run one or the
 * other - neither reads what the other writes.  The one launch covers L <= 8 layers, 0 < R1 <= 2048 and the operands
 * gnnrag_rel_transform takes; outside that range the same call makes the two launches.  Every byte written equals what
 * the two stand-alone calls write.  *combined (may be null): 1 when the one launch was taken. */
int gnnrag_seed_prologue(const gnnrag_csr* csr, const float* dist, void* fws, size_t fws_bytes, float* zero_a,
                         int64_t zero_na, float* zero_b, int64_t zero_nb, const float* relfeat_fwd,
                         const float* relfeat_inv, int32_t D, int32_t L, const gnnrag_layer_params* layers,
                         int32_t pos_rows, float* T_out, void* packed_out, int32_t* combined, gnnrag_stream_t stream);

/* Candidate selection of Evaluator.evaluate (evaluate.py:188-207) + the sort and top-p cut of
 * f1_and_hits (evaluate.py:34-51), one workgroup per question:
 *   keep slot j iff eligible[b,j] (host: query_entities != 1 and local_entity != pad id) and
 *   (double)pred_dist[b,j] >= ignore_prob;  order: probability descending, ties by ascending slot;
 *   out_slot [B,N]: the kept slots in that order, then -1;  out_cnt [B,2]: (kept, retrieved) where
 *   retrieved = shortest prefix whose running fp64 sum exceeds eps (or all kept).  N <= 16384. */
int gnnrag_topp_candidates(const float* pred_dist, const uint8_t* eligible, int32_t B, int32_t N,
                           double ignore_prob, double eps, int32_t* out_slot, int32_t* out_cnt,
                           gnnrag_stream_t stream);
/* The same selection for ANY N: questions with more than 16384 node slots (BASELINE config 5: 20 000) filter first,
 * compact the survivors into `workspace` (gnnrag_topp_workspace_bytes(B, N) bytes of device scratch; 0 for N <= 16384)
 * and sort them there - in LDS when at most 16384 slots survive the filter, else in the workspace. */
size_t gnnrag_topp_workspace_bytes(int32_t B, int32_t N);
int gnnrag_topp_candidates_ws(const float* pred_dist, const uint8_t* eligible, int32_t B, int32_t N,
                              double ignore_prob, double eps, int32_t* out_slot, int32_t* out_cnt,
                              void* workspace, size_t workspace_bytes, gnnrag_stream_t stream);

/* out[b,:] = sum_n seed_info[b,n] * ent_emb[b,n,:]  - the seed retrieval of QueryReform.forward
 * (gnn/modules/query_update.py:40, torch.bmm over all N rows); only rows with a non-zero flag are
 * read, in ascending n.  seed_info [B,N], ent_emb [B,N,D], out [B,D]. */
int gnnrag_seed_retrieve(const float* seed_info, const float* ent_emb, float* out, int32_t B, int32_t N,
                         int32_t D, gnnrag_stream_t stream);

/* QueryReform.forward as ONE launch (gnn/modules/query_update.py:26-44; Fusion :6-16; called once per instruction between
 * two ReaRev iterations, gnn/models/ReaRev/rearev.py:217-221):
 *   y = seed retrieval as above;  feats = [x, y, x - y];  out = sigmoid(W_g feats) * (W_r feats) + (1 - sigmoid(..)) * x
 * with x = q_node [B, D], W_r / W_g = fusion.r.weight / fusion.g.weight [D, 3 D] (no bias), ent_emb [B, N, ld_ent]
 * (row stride ld_ent >= D: a zero-padded node state is read in place), out [B, D].  The reference's attention over all
 * N node states (:36-38) does not enter its return value and is not computed.  D <= 4096 (GNNRAG_E_UNSUPPORTED beyond).
 * (ABI 16) */
int gnnrag_query_reform(const float* q_node, const float* seed_info, const float* ent_emb, int64_t ld_ent,
                        const float* W_r, const float* W_g, float* out, int32_t B, int32_t N, int32_t D,
                        gnnrag_stream_t stream);

/* Training form of the instruction update (additive to ABI 16): the n reforms of one ReaRev iteration
 * (gnn/models/ReaRev/rearev.py:217-221) in ONE launch.  The reforms share seed_info [B, N] and ent_emb [B, N, ld_ent]; reform
 * j < n has its own instruction q[j] [B, D] and Fusion weights W_r[j], W_g[j] [D, 3 D] - host arrays of n device pointers,
 * carried in the kernel arguments.  out: [n, B, D]; out[j] carries the bits of a gnnrag_query_reform call on reform j's
 * operands (the same kernel body), whatever grid the launcher picks.  reserve: caller-owned device memory of
 * gnnrag_query_reform_reserve_bytes(B, D, n) bytes (0 for a shape outside the limits) that the backward reads: the retrieved
 * y [B, D] once, then a_r = W_r f and the gate g = sigmoid(W_g f) as [n, B, 2 D].
 * Limits: 1 <= n <= GNNRAG_MAX_REFORMS, D <= GNNRAG_QUERY_REFORM_MAX_D, else GNNRAG_E_UNSUPPORTED; a NULL entry in an array,
 * n <= 0 or ld_ent < D is GNNRAG_E_BADARG; a reserve below the stated size is GNNRAG_E_WORKSPACE.  All are answered before
 * anything is launched. */
#define GNNRAG_MAX_REFORMS 8
#define GNNRAG_QUERY_REFORM_MAX_D 4096
size_t gnnrag_query_reform_reserve_bytes(int32_t B, int32_t D, int32_t n);
int gnnrag_query_reform_train(const float* const* q, const float* seed_info, const float* ent_emb, int64_t ld_ent,
                              const float* const* W_r, const float* const* W_g, float* out, void* reserve,
                              size_t reserve_bytes, int32_t B, int32_t N, int32_t D, int32_t n, gnnrag_stream_t stream);

/* Backward of gnnrag_query_reform_train (query_update_bwd.hip).  q, seed_info, W_r, W_g as given to the forward, its
 * reserve, and g_out: n device pointers [B, D], the gradients of out[j]; a NULL ENTRY means that reform's output was not
 * used: nothing is computed for it and it adds nothing to d_ent (a dq / dW asked for it anyway is written as zeros).  With
 * x = q[j][b], f = [x, y, x - y], G = g_out[j][b]:
 *   da_r = G g    da_g = G (a_r - x) g (1 - g)    df = W_r^T da_r + W_g^T da_g
 *   dq[j][b] = G (1 - g) + df[0:D] + df[2D:3D]     dy_j = df[D:2D] - df[2D:3D]
 *   dW_r[j] = sum_b da_r[b] (x) f[b]   dW_g[j] alike   d_ent[b,n,:] = seed_info[b,n] * (dy_j[b] added in ascending j)
 * Outputs, each optional (a NULL array or entry is not computed): dq [n] x [B, D], dW_r / dW_g [n] x [D, 3 D], d_ent
 * [B, N, D] contiguous - EVERY element is written (zero where seed_info is zero), nothing is accumulated into what it held.
 * No atomics, no allocation, nothing waits for the stream; one summation order (rows of W ascending, questions ascending,
 * reforms ascending): a second call gives the same bits, dq and d_ent of a question do not depend on B or on its place in
 * the batch.  LDS: 5 D floats, inside a CU's 160 KB at the forward's limit: the limits are the forward's.  workspace:
 * gnnrag_query_reform_backward_workspace_bytes(B, N, D, n) bytes (0 outside the limits); too small a reserve or workspace is
 * GNNRAG_E_WORKSPACE before anything is launched. */
size_t gnnrag_query_reform_backward_workspace_bytes(int32_t B, int32_t N, int32_t D, int32_t n);
int gnnrag_query_reform_backward(const float* const* q, const float* seed_info, const float* const* W_r,
                                 const float* const* W_g, const void* reserve, size_t reserve_bytes,
                                 const float* const* g_out, float* const* dq, float* const* dW_r, float* const* dW_g,
                                 float* d_ent, int32_t B, int32_t N, int32_t D, int32_t n, void* workspace,
                                 size_t workspace_bytes, gnnrag_stream_t stream);

/* The tail of the reasoning layer under autograd (additive to ABI 16; layer_tail.hip): what
 * gnn/modules/kg_reasoning/reasongnn.py:163-169 does after the dense products.  Rows r = b N + n, all tensors contiguous.
 *   h     = max(pre_a + pre_b, 0)                       one fp32 add (pre_b NULL: none), then the relu
 *   s     = scale * sum_d h[d] keep[d] w_score[d] + b_score        keep: 0/1 bytes, the dropout in front of score_func;
 *                                                                   keep NULL: no dropout, scale is taken as 1
 *   score = s + (1 - mask) * (-1e11)                    added in fp32 without contraction: a masked score is float(-1e11)
 *   dist  = gnnrag_masked_softmax(score): the same launch, the same bits
 * Two launches.  float4 accesses where D % 4 == 0 and the bases are 16-byte aligned (keep: 4-byte), element accesses with
 * the same summation order otherwise: the same bits either way.  b_score is read on the device.
 * Limits: D <= GNNRAG_LAYER_TAIL_MAX_D and B N < 2^31, else GNNRAG_E_UNSUPPORTED; a NULL among the required pointers or a
 * size <= 0 is GNNRAG_E_BADARG.  Both are answered before anything is launched. */
#define GNNRAG_LAYER_TAIL_MAX_D 4096
int gnnrag_layer_tail_train(const float* pre_a, const float* pre_b, const uint8_t* keep, float scale,
                            const float* w_score, const float* b_score, const float* mask, int32_t B, int32_t N, int32_t D,
                            float* h_out, float* score, float* dist, gnnrag_stream_t stream);

/* Backward of gnnrag_layer_tail_train from g_h [B N, D] (the gradient of h) and g_dist [B, N]; h and dist as the forward
 * wrote them, keep / scale / w_score as it was given them.  Per question sigma = sum_n dist g_dist in one fixed order and
 * gs[n] = dist[n] (g_dist[n] - sigma): the mask addition passes the gradient with derivative 1, as autograd does (a fully
 * padded question has dist = 1/N and a non-zero gs).
 *   g_pre[r,d] = h[r,d] > 0 ? g_h[r,d] + gs[r] w_score[d] keep[r,d] scale : 0     the gradient of pre_a and of pre_b alike;
 *                                                                                 EVERY element is written
 *   dw_score[d] = sum_r gs[r] keep[r,d] scale h[r,d]            db_score = 0 exactly (a softmax does not move under a shift)
 * g_dist NULL: gs = 0 (g_pre = (h > 0) g_h, dw_score written as zeros); g_h NULL: that term is absent; both NULL is
 * GNNRAG_E_BADARG.  dw_score / db_score NULL: not wanted.  Up to three launches, no atomics, no allocation, nothing waits
 * for the stream; the grid and every summation order depend on (B, N, D) only: a second call gives the same bits, g_pre of a
 * question does not depend on the batch around it.  workspace: gnnrag_layer_tail_backward_workspace_bytes(B, N, D) bytes (0
 * outside the limits); a smaller one is GNNRAG_E_WORKSPACE before anything is launched. */
size_t gnnrag_layer_tail_backward_workspace_bytes(int32_t B, int32_t N, int32_t D);
int gnnrag_layer_tail_backward(const float* h, const float* dist, const uint8_t* keep, float scale, const float* w_score,
                               const float* g_h, const float* g_dist, int32_t B, int32_t N, int32_t D, float* g_pre,
                               float* dw_score, float* db_score, void* workspace, size_t workspace_bytes,
                               gnnrag_stream_t stream);

/* ---- The concatenated update under dropout, for training (additive to ABI 16; gemm_f32.hip, gemm_tn.hip) -----------------
 * gnn/modules/kg_reasoning/reasongnn.py:161-163 at --linear_dropout > 0: e2e_linear(linear_drop(cat(h, agg))).  Let
 * x = [h | agg] (rows r < BN, columns k < K = (2I+1) D, h = columns < D), keep [BN, K] uint8 0/1 in that concatenation
 * order and xd[r,k] = keep[r,k] ? x[r,k] * scale : +0; keep NULL: no dropout, scale is taken as 1 (the convention of
 * gnnrag_layer_tail_train).  xd is formed inside the products' tile loaders and never stored.
 *   pre [BN, D] = xd . W^T + b          W [D, K] = e2e_linear.weight, b [D]
 * The product xd is one fp32 multiply per element, made before the bf16 split of the bf16x3 form, so pre carries the bits
 * gnnrag_linear gives on a materialised xd wherever the two calls run the same kernel form (gnnrag_dense_form).  One launch
 * per column block of 208; no relu and no score (gnnrag_layer_tail_train follows).
 * Common rules of the forward and the backward: no atomics, no allocation, nothing waits for the stream; the grid and
 * every summation order depend on (BN, D, I, math) only, so a second call gives the same bits.  A missing required pointer
 * or a size <= 0 is GNNRAG_E_BADARG; then D % 4 == 0, 16-byte aligned float operands, a 4-byte aligned keep and BN < 2^31,
 * else GNNRAG_E_UNSUPPORTED; then a short workspace is GNNRAG_E_WORKSPACE.  All are answered before anything is launched. */
int gnnrag_update_drop_train(const float* h, const float* agg, const uint8_t* keep, float scale, const float* W,
                             const float* b, int64_t BN, int32_t D, int32_t I, float* pre, int32_t math,
                             gnnrag_stream_t stream);

/* Backward of gnnrag_update_drop_train from g_pre [BN, D]; h / agg / keep / scale / W as the forward was given them.
 *   g_h [BN, D], g_agg [BN, 2I D]   element (r,k) of [g_h | g_agg] = keep[r,k] ? scale * sum_o g_pre[r,o] W[o,k] : +0.
 *                                   Each is contiguous and written by the product's own epilogue, EVERY element; a dropped
 *                                   one is a select, not a multiply (an Inf beside it does not become NaN).  One launch per
 *                                   column block of 208 of each output, against the transposed weight in the workspace
 *   dW [D, K] = g_pre^T . xd        the chunking and the chunk-order reduce of gnnrag_gemm_tn, the mask applied to its
 *                                   B operand as it is loaded: the bits of gnnrag_gemm_tn on a materialised xd
 *   db [D]                          column sums of g_pre in one fixed order (partial sums over row blocks and over the
 *                                   rows' index mod 16 in a first launch, the partial rows added by a second)
 * Any output NULL: not wanted, and its launches are not made; all four NULL is GNNRAG_E_BADARG.  W is required for g_h /
 * g_agg, h and agg for dW.  workspace: gnnrag_update_drop_backward_workspace_bytes(BN, D, I) bytes, 16-byte aligned (0 for
 * a shape outside the limits; like gnnrag_gemm_tn_workspace_bytes it depends on the current device). */
size_t gnnrag_update_drop_backward_workspace_bytes(int64_t BN, int32_t D, int32_t I);
int gnnrag_update_drop_backward(const float* g_pre, const float* h, const float* agg, const uint8_t* keep, float scale,
                                const float* W, int64_t BN, int32_t D, int32_t I, float* g_h, float* g_agg, float* dW,
                                float* db, void* workspace, size_t workspace_bytes, int32_t math, gnnrag_stream_t stream);

/* ---- Backward of gnnrag_relation_tables, for training on the fused form (additive to ABI 16; rel_tables_bwd.hip) ----------
 * M = rel_total, (b_m, r_m) = csr->rel_rows[m], blk(i,d) = (1 + 2 i + d) D, a[d,m,i,k] = T_d[r_m,k] * ins[b_m,i,k] (one fp32
 * multiply, as the forward's loader forms it), z = relu(a).  From g_P [2, rel_total, D]:
 *   G[d,m,i,k]         = ( sum_o g_P[d,m,o] W_e2e[o, blk(i,d)+k] ) * [a[d,m,i,k] > 0]
 *   g_W[o, blk(i,d)+k] = sum_m g_P[d,m,o] z[d,m,i,k]                 [D, (2I+1) D], columns 0 .. D-1 exactly +0
 *   g_T_d[r,k]         = sum_{m: r_m = r} sum_i G[d,m,i,k] ins[b_m,i,k]     [R1, D]; a relation no question uses: +0
 *   g_ins[b,i,k]       = sum_d sum_{m: b_m = b} G[d,m,i,k] T_d[r_m,k]       [B, I, D]; a question without facts: +0
 * The gate is a > 0 (torch's relu rule: a product that is 0, -0 or negative passes nothing).  z is never stored: the weight
 * gradient forms it on the loaded pieces of k_gemm_tn's B operand (gnnrag_gemm_tn's chunks, added in chunk order).  The
 * ungated product in front of G is 2 I gnnrag_linear calls (`math` selects their form; gnnrag_dense_form:
 * GNNRAG_DENSE_ENTRY_REL_TABLES_DX) against one transposed copy of W_e2e, kept in the workspace [2, I, M, D]; its two
 * readers apply the gate.  g_ins is a segmented column sum over a question's contiguous rows, g_T one workgroup per
 * (relation, direction) over the questions in ascending order; every reduction is fp32.  No atomics, no allocation, nothing
 * waits for the stream; each output element has one writer and one summation order that depends on the structure and
 * (D, I, math) only: a second call gives the same bits.  Every wanted output is fully written.
 * Any output NULL: not wanted, and its launches are not made; all four NULL is GNNRAG_E_BADARG, as are a NULL csr or input.
 * Then D % 4 == 0, D <= 1024, I <= GNNRAG_MAX_INS and 16-byte aligned operands, else GNNRAG_E_UNSUPPORTED; then a short
 * workspace is GNNRAG_E_WORKSPACE.  All are answered before anything is launched.  rel_total == 0: every wanted output is
 * zero-filled, nothing else is touched and no workspace is needed (pointers must still be real).
 * workspace: gnnrag_relation_tables_backward_workspace_bytes(csr, D, I) bytes, 16-byte aligned (0 for a shape outside the
 * limits or a structure without facts; like gnnrag_gemm_tn_workspace_bytes it depends on the current device). */
size_t gnnrag_relation_tables_backward_workspace_bytes(const gnnrag_csr* csr, int32_t D, int32_t I);
int gnnrag_relation_tables_backward(const gnnrag_csr* csr,
                                    const float* T_fwd, const float* T_inv, const float* ins, const float* W_e2e,
                                    const float* g_P, float* g_T_fwd, float* g_T_inv, float* g_ins, float* g_W,
                                    int32_t D, int32_t I, int32_t math,
                                    void* workspace, size_t workspace_bytes, gnnrag_stream_t stream);

/* ---- Training loss and batch metrics (additive to ABI 16; train_tail.hip) -------------------------------------------------
 * What follows the last dist of a training forward (gnn/models/ReaRev/rearev.py:227-243, gnn/models/NSM/nsm.py:242-250).
 *
 * gnnrag_kl_loss_train: calc_loss_label with loss_type 'kl' (base_model.py:193-215).  pred, teacher [B, N] contiguous,
 * label_valid [B].  Per question b, in fp32:
 *   len_b = sum_n teacher (0 is replaced by 1)         t = teacher / len_b
 *   l_b   = label_valid_b sum_n (t > 0 ? t (log t - log(pred + 1e-8)) : 0)           KLDivLoss(reduction='none') summed
 *   loss  = (sum_b l_b) / B
 * One workgroup per question (thread-strided sums, a fixed xor tree, the waves in order), then one launch that adds the l_b
 * in ascending b.  len_b goes to the caller-owned reserve [B] (the backward reads it); the l_b pass through the workspace,
 * gnnrag_kl_loss_workspace_bytes(B) bytes (a smaller one is GNNRAG_E_WORKSPACE before anything is launched).  No atomics,
 * no allocation, nothing waits for the stream; a second call gives the same bits and l_b does not depend on the batch
 * around question b.  A NULL pointer, B <= 0 or N <= 0 is GNNRAG_E_BADARG before a device is touched. */
size_t gnnrag_kl_loss_workspace_bytes(int32_t B);
int gnnrag_kl_loss_train(const float* pred, const float* teacher, const float* label_valid, int32_t B, int32_t N,
                         float* loss, float* reserve, void* workspace, size_t workspace_bytes, gnnrag_stream_t stream);

/* Backward of gnnrag_kl_loss_train: g_loss [1] ON THE DEVICE (never read on the host), reserve as the forward wrote it.
 *   d_pred[b, n] = -g label_valid_b t / (pred + 1e-8) / B       exactly 0 where teacher == 0 or label_valid_b == 0
 * One streaming pass that writes EVERY element of d_pred [B, N] (no memset, nothing accumulated into what it held): float4
 * accesses where N % 4 == 0 and pred, teacher and d_pred are 16-byte aligned, element accesses with the same ownership and
 * the same bits otherwise.  teacher receives no gradient. */
int gnnrag_kl_loss_backward(const float* g_loss, const float* pred, const float* teacher, const float* label_valid,
                            const float* reserve, int32_t B, int32_t N, float* d_pred, gnnrag_stream_t stream);

/* get_eval_metric of a training step (base_model.py:217-298: calc_h1, calc_f1_new, f1_and_hits) in one launch, one
 * workgroup per question.  pred, answer, seed [B, N] float, local_entity [B, N] int64, all contiguous.
 *   out_pred [B]    argmax of pred over all N slots (seeds and pads included), the lowest slot among equal maxima
 *   out_h1 [B]      answer[argmax] > 1e-10 as 0 / 1
 *   eligible        !(seed > 0) and local_entity != pad_id
 *   n_ans           eligible slots with answer > 0 (counted before the probability filter)
 *   kept            eligible and !((double)pred < ignore_prob), ignore_prob = (1 - eps) / N formed on the host in double;
 *                   ordered by probability descending, ties in ascending slot order
 *   n_ret           the shortest prefix whose sequential fp64 running sum exceeds eps, else everything kept
 *   correct         retrieved slots with answer > 0 (the slot's own flag: equal to the reference's membership test by
 *                   entity id whenever a question's non-pad ids are distinct)
 *   out_f1 [B]      n_ans == 0: (n_ret == 0 ? 1 : 0); n_ret == 0: 0; else p = correct / n_ret, r = correct / n_ans,
 *                   (p != 0 && r != 0) ? 2.0 / (1.0 / p + 1.0 / r) : 0 in double; rounded to fp32 once; 0 where h1 == 0
 *   out_cnt [B, 4]  (kept, n_ret, correct, n_ans)
 * N <= GNNRAG_TRAIN_METRICS_MAX_N (the keys of a question live in LDS), else GNNRAG_E_UNSUPPORTED; a NULL pointer, B <= 0
 * or N <= 0 is GNNRAG_E_BADARG.  Both are answered before anything is launched. */
#define GNNRAG_TRAIN_METRICS_MAX_N 16384
int gnnrag_train_metrics(const float* pred, const float* answer, const float* seed, const int64_t* local_entity,
                         int64_t pad_id, double eps, int32_t B, int32_t N, int32_t* out_pred, float* out_h1, float* out_f1,
                         int32_t* out_cnt, gnnrag_stream_t stream);

/* The question encoder's LSTM (the instruction path): one layer, one direction, batch_first,
 * torch.nn.LSTM semantics and parameter layout (gate order i, f, g, o) - what
 * gnn/modules/question_encoding/lstm_encoder.py:27-36 builds and calls as
 *   query_hidden_emb, (h_n, c_n) = self.node_encoder(x, (h0, c0))          x [B, T, E], h0 = c0 = zeros [1, B, H]
 * x [B,T,E], w_ih [4H,E], w_hh [4H,H], b_ih / b_hh [4H] or NULL, h0 / c0 [B,H] or NULL (zeros); out [B,T,H], h_n and
 * c_n [B,H].  4 H <= 1024.  workspace: gnnrag_lstm_workspace_bytes(E, H) bytes (transposed weights). */
size_t gnnrag_lstm_workspace_bytes(int32_t E, int32_t H);
int gnnrag_lstm_forward(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                        const float* h0, const float* c0, float* out, float* h_n, float* c_n, int32_t B, int32_t T,
                        int32_t E, int32_t H, void* workspace, size_t workspace_bytes, gnnrag_stream_t stream);

/* ---- Training form of the LSTM (additive to ABI 16; SURVEY.md section 8 f-4, the instruction side) ---------------------
 * gnnrag_lstm_forward_train is gnnrag_lstm_forward - same arguments, same kernel, same arithmetic in the same order:
 * out, h_n and c_n are the same bits - that also fills the caller-owned `reserve` the backward reads:
 *   act [B,T,4H]  the four activated gates of every step (sigmoid i, sigmoid f, tanh g, sigmoid o), then
 *   cs  [B,T,H]   the cell state after every step;
 * gnnrag_lstm_reserve_bytes(B, T, H) bytes, fully written.  The reserve belongs to ONE forward call: a module that is
 * called twice before its backward passes run (base_encoder.py:74-80) needs two. */
size_t gnnrag_lstm_reserve_bytes(int32_t B, int32_t T, int32_t H);
int gnnrag_lstm_forward_train(const float* x, const float* w_ih, const float* w_hh, const float* b_ih,
                              const float* b_hh, const float* h0, const float* c0, float* out, float* h_n, float* c_n,
                              int32_t B, int32_t T, int32_t E, int32_t H, void* reserve, size_t reserve_bytes,
                              void* workspace, size_t workspace_bytes, gnnrag_stream_t stream);

/* Backward of the call above: what autograd derives for nn.LSTM in Trainer_KBQA.train_epoch (train_model.py:209-233).
 * x, w_ih, w_hh, h0, c0 (NULL = zeros) as given to the forward, `out` and `reserve` as it left them; g_out [B,T,H],
 * g_hn / g_cn [B,H]: the incoming gradients of out, h_n, c_n - each may be NULL (zeros).
 * dw_ih [4H,E] and dw_hh [4H,H] are required; dx [B,T,E], db [4H] (the gradient of b_ih AND of b_hh: the same values),
 * dh0 / dc0 [B,H] may be NULL: not wanted, not computed.  Every requested output is fully written.
 * One workgroup per sequence walks t = T-1 .. 0 with dc in registers and leaves the pre-activation gate gradients
 * dG [B,T,4H] in the workspace; dh_{t-1} = W_hh^T dG_t is four per-gate-block partial sums (ascending gate row) added
 * in block order; dx = dG W_ih (the exact-fp32 gnnrag_linear), dw_ih = dG^T x and dw_hh = dG^T h_prev
 * (gnnrag_gemm_tn), db = column sums of dG (rows in 8 slices, slices added in order): one fixed summation order, no
 * atomics, fp32 throughout, nothing waits for the stream.
 * 4 H <= 1024, E % 4 == 0, x / dw_ih / workspace 16-byte aligned, else GNNRAG_E_UNSUPPORTED.  A reserve below
 * gnnrag_lstm_reserve_bytes or a workspace below gnnrag_lstm_backward_workspace_bytes(B, T, E, H) (which, like
 * gnnrag_gemm_tn_workspace_bytes, depends on the current device) is GNNRAG_E_WORKSPACE before anything is launched. */
size_t gnnrag_lstm_backward_workspace_bytes(int32_t B, int32_t T, int32_t E, int32_t H);
int gnnrag_lstm_backward(const float* x, const float* w_ih, const float* w_hh, const float* h0, const float* c0,
                         const float* out, const void* reserve, size_t reserve_bytes, const float* g_out,
                         const float* g_hn, const float* g_cn, float* dx, float* dw_ih, float* dw_hh, float* db,
                         float* dh0, float* dc0, int32_t B, int32_t T, int32_t E, int32_t H, void* workspace,
                         size_t workspace_bytes, gnnrag_stream_t stream);

/* ---- Instruction generation (additive to ABI 16; SURVEY.md section 8 f-3, the instruction path) -------------------------
 * BaseInstruction.get_instruction (gnn/modules/question_encoding/base_encoder.py:82-101) for n_steps chained steps in ONE
 * launch.  Per question b, starting from r = r_in[b] (NULL = zeros), for step s:
 *   q_s  = W_q[s] node[b] + b_q[s]                               (:92)
 *   cq   = W_cq [r, q_s, q_s - r, q_s * r] + b_cq                (:93)
 *   ca_t = sum_d w_ca[d] cq[d] hidden[b,t,d] + b_ca              (:95)
 *   a    = softmax_t(ca_t + (1 - mask[b,t]) * -1e11)             (:98; the fp32 sum as written, row maximum subtracted)
 *   r    = sum_t a_t hidden[b,t,:]                               (:100)   ins_out[s,b,:] = r, attn_out[s,b,:] = a
 * hidden [B,T,D] (the encoder's token states), node [B,D], mask [B,T] (1 = token, 0 = padding; a question of padding only
 * gets the uniform 1/T, as in the reference), W_cq [D,4D], b_cq [D], w_ca [D], b_ca [1] - all device memory, b_ca is
 * read by the kernel.  W_q / b_q: HOST arrays of n_steps device pointers ([D,D] and [D] each; question_linear{s} are
 * separate parameters) - read during the call and carried in the kernel's arguments, nothing is packed or copied.
 * ins_out [n_steps,B,D], attn_out [n_steps,B,T], both fully written.  One workgroup per question, its token states in
 * LDS; one fixed summation order (no atomics: the same bits on every call, and a chain cut into several calls gives the
 * bits of one call); no allocation, no workspace, nothing waits for the stream; safe under stream capture.
 * n_steps > GNNRAG_MAX_INS, or a working set of 4 * (ceil4(T D) + (n_steps + 2) D + T) bytes above 160 KB, is
 * GNNRAG_E_UNSUPPORTED (every T D <= 16384 with D <= 2048 fits); any D >= 1 inside that is taken. */
#define GNNRAG_MAX_INS 8
int gnnrag_instructions(const float* hidden, const float* node, const float* mask, const float* r_in,
                        const float* const* W_q, const float* const* b_q, const float* W_cq, const float* b_cq,
                        const float* w_ca, const float* b_ca, int32_t B, int32_t T, int32_t D, int32_t n_steps,
                        float* ins_out, float* attn_out, gnnrag_stream_t stream);

/* ---- Training form of instruction generation (additive to ABI 16; SURVEY.md section 8 f-4, the instruction side) --------
 * gnnrag_instructions_train is gnnrag_instructions - the same kernel behind compile-time switches - plus
 *   drop_node [n_steps,B,D], drop_cat [n_steps,B,4D], drop_tok [n_steps,B,T,D]: the three multipliers of linear_drop
 *     (base_encoder.py:92, :93, :95; 0 or 1/(1-p)), each may be NULL (all ones):
 *       n_s = node * drop_node[s]          z = [r, q, q - r, q * r] * drop_cat[s]
 *       ca_t = sum_d w_ca[d] ((cq[d] hidden[t,d]) * drop_tok[s,t,d]) + b_ca
 *   reserve: caller-owned, gnnrag_instructions_reserve_bytes(B, T, D, n_steps) bytes, fully written: q_s [D] then cq [D]
 *     of every (step, question), [n_steps,B,2D].  It belongs to ONE forward call.
 * With all three multipliers NULL, ins_out / attn_out are the bits of gnnrag_instructions.  Limits as there; a reserve below
 * the stated size is GNNRAG_E_WORKSPACE before anything is launched. */
size_t gnnrag_instructions_reserve_bytes(int32_t B, int32_t T, int32_t D, int32_t n_steps);
int gnnrag_instructions_train(const float* hidden, const float* node, const float* mask, const float* r_in,
                              const float* const* W_q, const float* const* b_q, const float* W_cq, const float* b_cq,
                              const float* w_ca, const float* b_ca, const float* drop_node, const float* drop_cat,
                              const float* drop_tok, int32_t B, int32_t T, int32_t D, int32_t n_steps, float* ins_out,
                              float* attn_out, void* reserve, size_t reserve_bytes, gnnrag_stream_t stream);

/* Backward of the call above: what autograd derives for get_instruction in Trainer_KBQA.train_epoch
 * (train_model.py:209-233).  hidden, node, r_in (NULL = zeros), W_q, W_cq, w_ca and the multipliers as given to the
 * forward, ins / attn / reserve as it left them; g_ins [n_steps,B,D], g_attn [n_steps,B,T]: the incoming gradients, each
 * may be NULL (zeros).  With r = the instruction before step s and dr' = g_ins[s] + carry, for s = n_steps-1 .. 0:
 *   da_t  = dr' . hidden[t,:] + g_attn[s,t]          dca_t = a_t (da_t - sum_u a_u da_u)
 *   dhidden[t,d] += a_t dr'[d] + dca_t w_ca[d] cq[d] drop_tok[t,d]
 *   u[d]  = sum_t dca_t hidden[t,d] drop_tok[t,d]    dcq = w_ca * u          dw_ca += cq * u
 *   dz    = (W_cq^T dcq) * drop_cat                  carry = dz0 - dz2 + dz3 * q        dq = dz1 + dz2 + dz3 * r
 *   dW_cq += dcq (x) z    db_cq += dcq    dW_q[s] += dq (x) n_s    db_q[s] += dq    dnode += (W_q[s]^T dq) * drop_node
 * and dr_in = carry after step 0.  The gradient passes the mask addition with derivative 1, as autograd's does (a question
 * of padding only has a = 1/T and a non-zero dca).  b_ca does not move the softmax: db_ca is written as exactly 0.
 * dhidden [B,T,D], dnode [B,D], dr_in [B,D], dW_q / db_q (HOST arrays of n_steps device pointers, [D,D] and [D]; the
 * array or an entry may be NULL), dW_cq [D,4D], db_cq [D], dw_ca [D], db_ca [1]: each may be NULL - not wanted, not
 * computed; every requested output is fully written.
 * One workgroup per question walks the chain with its token states in LDS; a dhidden element belongs to one thread in
 * every step; the transposed products sum over the rows of W in ascending order; the token sums use the forward's
 * __shfl_xor tree and ascending t.  The parameter gradients are gnnrag_gemm_tn products over the per-(step, question) rows
 * the kernel leaves in the workspace (zero-padded copies for D % 4 != 0) and column sums in 8 row slices added in order.
 * One fixed summation order, no atomics, no allocation, nothing waits for the stream: a repeated call gives the same bits.
 * Limits: n_steps <= GNNRAG_MAX_INS and a working set of 4 * (ceil4(T D) + 12 D + 3 T) bytes within 160 KB (every
 * T <= 64 with D <= 256 fits), workspace 16-byte aligned, else GNNRAG_E_UNSUPPORTED.  A reserve below
 * gnnrag_instructions_reserve_bytes or a workspace below gnnrag_instructions_backward_workspace_bytes(B, T, D, n_steps)
 * (0 for a shape outside the limits; like gnnrag_gemm_tn_workspace_bytes it depends on the current device) is
 * GNNRAG_E_WORKSPACE.  Both are answered before anything is launched. */
size_t gnnrag_instructions_backward_workspace_bytes(int32_t B, int32_t T, int32_t D, int32_t n_steps);
int gnnrag_instructions_backward(const float* hidden, const float* node, const float* r_in, const float* const* W_q,
                                 const float* W_cq, const float* w_ca, const float* drop_node, const float* drop_cat,
                                 const float* drop_tok, const float* ins, const float* attn, const void* reserve,
                                 size_t reserve_bytes, const float* g_ins, const float* g_attn, float* dhidden,
                                 float* dnode, float* dr_in, float* const* dW_q, float* const* db_q, float* dW_cq,
                                 float* db_cq, float* dw_ca, float* db_ca, int32_t B, int32_t T, int32_t D,
                                 int32_t n_steps, void* workspace, size_t workspace_bytes, gnnrag_stream_t stream);

/* ---- Frozen BERT-class question encoder, inference only (additive to ABI 16) --------------------
 * What BERTInstruction.encode_question reads from `self.node_encoder(query_text)[0]` (gnn/modules/question_encoding/
 * bert_encoder.py:94): transformers' BertModel on input ids alone - absolute positions 0 .. T-1, token type 0, NO
 * attention mask (pad tokens are attended like any other token), erf GELU, post-LayerNorm blocks; no pooler.
 *   x = LN(word_emb[id] + pos_emb[t] + type_emb[0]);  per layer:
 *   qkv = x W_qkv^T + b_qkv;  ctx = softmax(q k^T / sqrt(dh)) v per head;  x = LN(ctx W_o^T + b_o + x);
 *   x = LN(gelu(x W_i^T + b_i) W_f^T + b_f + x),  gelu(u) = 0.5 u (1 + erf(u / sqrt 2))
 * LN: biased variance, two passes, ln_eps inside the root.  ids [B,T] int64; word_emb [vocab,H], pos_emb [max_pos,H],
 * type_emb [>= 1,H] (row 0 is read), ln_g / ln_b [H]; out [B,T,H], fully written.  An id outside [0, vocab) reads no
 * memory: its output row is NaN (through every layer; with L > 0 all rows of that question are NaN, no other question's).
 * layers: HOST array of L structs of device pointers, read during the call (as gnnrag_layer_params is).  W_qkv
 * [3H,H] / b_qkv [3H]: the query, key and value weights stacked in that order; W_o [H,H], W_i [I,H], W_f [H,I].  L = 0 is
 * legal: out is the embedding LayerNorm, layers and ws are not read.
 * The four dense products of a layer are gnnrag_linear calls (math: GNNRAG_MATH_*), a layer is 8 launches.  fp32
 * throughout, no atomics, every reduction in an order the shape fixes, no allocation, nothing waits for the stream, safe
 * under capture: a second call gives the same bits and a question's rows do not depend on B.
 * GNNRAG_E_UNSUPPORTED before anything is launched (the shape rules are answered first, whatever the pointers are):
 * H % heads != 0, H / heads not in {32, 64}, T > 128, T > max_pos, H % 4 != 0, ws_bytes below
 * gnnrag_bert_workspace_bytes(B, T, H, I) (L > 0), a pointer that is not 16-byte aligned (ids: 8).  A NULL pointer or a
 * size <= 0 is GNNRAG_E_BADARG.
 * gnnrag_bert_attention is the attention step alone: qkv [B T, 3 heads dh] packed as above, ctx [B T, heads dh].
 *
 * gnnrag_bert_encode_ex / gnnrag_bert_attention_bias (additive to ABI 16): the same block as RobertaModel and MPNetModel
 * run it on input ids alone (--lm roberta / relbert / sbert2), by three more inputs; with type_emb given, pad_id < 0 and
 * rel_bias NULL they are gnnrag_bert_encode / gnnrag_bert_attention, bit for bit.
 *   type_emb NULL: no token-type term (MPNet); not read.
 *   pad_id >= 0:   positions come from the ids (transformers' create_position_ids_from_input_ids): a token that is not
 *                  pad_id sits at pad_id + (number of non-pad ids among ids[b, 0 .. t]), a pad at pad_id.  Pads are still
 *                  attended (no mask).  An id outside [0, vocab) counts as non-pad for the rows after it (its own row is
 *                  NaN as above).  A wave counts its own question's ids only: no dependence on B.  A position outside
 *                  [0, max_pos) reads nothing (its row is NaN); the shape rule below excludes it.
 *   rel_bias:      [heads, 2T-1] or NULL.  The score of query i and key j of a head is (q_i . k_j) / sqrt(dh) +
 *                  rel_bias[head][j - i + T - 1], in every layer (MPNet's relative_attention_bias gathered at the
 *                  bucket of j - i).  Not read when L = 0.
 * One more GNNRAG_E_UNSUPPORTED rule, answered with the shape rules: pad_id >= 0 and T + pad_id > max_pos - 1 (a full row
 * reaches position T + pad_id; transformers raises there too).  A rel_bias that is not 16-byte aligned is UNSUPPORTED.
 * Workspace, launches per layer, capture safety, "no allocation" and "nothing waits" are as above.  Attention masks, T5
 * (RMS norm, unscaled scores, its own bias rule) and gradients remain outside; dropout: gnnrag_bert_encode_train below. */
typedef struct gnnrag_bert_layer { const float *W_qkv, *b_qkv, *W_o, *b_o, *ln1_g, *ln1_b,
                                               *W_i, *b_i, *W_f, *b_f, *ln2_g, *ln2_b; } gnnrag_bert_layer;
size_t gnnrag_bert_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t I);
int gnnrag_bert_attention(const float* qkv, int32_t B, int32_t T, int32_t heads, int32_t dh, float* ctx,
                          gnnrag_stream_t stream);
int gnnrag_bert_encode(const int64_t* ids, const float* word_emb, int32_t vocab, const float* pos_emb, int32_t max_pos,
                       const float* type_emb, const float* ln_g, const float* ln_b, float ln_eps,
                       int32_t L, const gnnrag_bert_layer* layers, int32_t B, int32_t T, int32_t H, int32_t heads,
                       int32_t I, float* out /* [B,T,H] */, void* ws, size_t ws_bytes, int32_t math,
                       gnnrag_stream_t stream);
int gnnrag_bert_attention_bias(const float* qkv, int32_t B, int32_t T, int32_t heads, int32_t dh,
                               const float* rel_bias /* [heads,2T-1] or NULL */, float* ctx, gnnrag_stream_t stream);
int gnnrag_bert_encode_ex(const int64_t* ids, const float* word_emb, int32_t vocab, const float* pos_emb, int32_t max_pos,
                          const float* type_emb /* or NULL */, int32_t pad_id /* < 0: positions 0 .. T-1 */,
                          const float* rel_bias /* [heads,2T-1] or NULL */, const float* ln_g, const float* ln_b,
                          float ln_eps, int32_t L, const gnnrag_bert_layer* layers, int32_t B, int32_t T, int32_t H,
                          int32_t heads, int32_t I, float* out /* [B,T,H] */, void* ws, size_t ws_bytes, int32_t math,
                          gnnrag_stream_t stream);

/* ---- The same encoder in training mode: forward only (additive to ABI 16) -----------------------
 * Trainer_KBQA calls model.train(), which puts the frozen LM into training mode too: transformers then applies dropout
 * (hidden_dropout_prob, attention_probs_dropout_prob) at four sites of the forward.  The LM is frozen, so nothing needs a
 * backward.  The caller draws the keep bytes (one uint8 per element, != 0 keeps; read-only, caller-owned) and every site is
 * part of the launch that already produces the value - a layer stays 8 launches, the embedding 1:
 *   embedding output:          x = LN(...) * m                          m = keep ? scale_hidden : 0
 *   attention probabilities:   p_j = softmax_j(...) * (keep ? scale_att : 0); NOT renormalised; a row whose keys are all
 *                              dropped gives a zero context row
 *   W_o / W_f outputs:         x = LN((a W^T + b) * m + x)              the residual is added behind the dropout
 * The product with 0 keeps a non-finite value NaN, as transformers' `x * mask` does: a row whose id or position is out of
 * range is NaN in every element whatever its keep bytes are.
 * keep_hidden: 1 + 2L planes of [B T, H] bytes, row-major.  Plane 0: the embedding output; plane 1 + 2l: layer l's attention
 *              output projection; plane 2 + 2l: layer l's FFN output projection.  With L = 0 only plane 0 is read.
 *              gnnrag_bert_keep_hidden_bytes(L, B, T, H) = (1 + 2L) B T H (0 for L < 0 or a size <= 0).
 * keep_att:    [L, B, heads, T, T], query row i, key column j.  gnnrag_bert_keep_att_bytes(L, B, T, heads) = L B heads T T
 *              (0 for any argument <= 0).
 * keep_hidden NULL: no hidden dropout - those sites run the inference sequence (the residual in the product's epilogue) and
 * scale_hidden is not read; keep_att NULL likewise.  Both NULL enqueues exactly what gnnrag_bert_encode_ex enqueues: equal
 * bits.  The workspace is that of gnnrag_bert_workspace_bytes, unchanged.  No atomics, no allocation, nothing waits for the
 * stream, safe under capture; the same masks give the same bits, and a question's rows depend on its own ids and its own
 * slices of the masks only.
 * Rules, in the order of gnnrag_bert_encode_ex: sizes (BADARG), the shape rules whatever the pointers are (UNSUPPORTED), NULL
 * pointers (BADARG), then: a scale of a given mask that is not finite or not > 0 is GNNRAG_E_BADARG; a keep_hidden that is
 * not 4-byte aligned is GNNRAG_E_UNSUPPORTED (a lane reads the 4 bytes of its float4 as one word); keep_att may have any
 * alignment.
 * gnnrag_bert_attention_drop is the attention step alone with one [B, heads, T, T] mask (keep NULL: gnnrag_bert_attention_bias). */
size_t gnnrag_bert_keep_hidden_bytes(int32_t L, int32_t B, int32_t T, int32_t H);
size_t gnnrag_bert_keep_att_bytes(int32_t L, int32_t B, int32_t T, int32_t heads);
int gnnrag_bert_attention_drop(const float* qkv, int32_t B, int32_t T, int32_t heads, int32_t dh,
                               const float* rel_bias /* [heads,2T-1] or NULL */, const uint8_t* keep /* [B,heads,T,T] */,
                               float scale, float* ctx, gnnrag_stream_t stream);
int gnnrag_bert_encode_train(const int64_t* ids, const float* word_emb, int32_t vocab, const float* pos_emb,
                             int32_t max_pos, const float* type_emb /* or NULL */, int32_t pad_id, const float* rel_bias,
                             const float* ln_g, const float* ln_b, float ln_eps, int32_t L,
                             const gnnrag_bert_layer* layers, int32_t B, int32_t T, int32_t H, int32_t heads, int32_t I,
                             const uint8_t* keep_hidden /* or NULL */, float scale_hidden,
                             const uint8_t* keep_att /* or NULL */, float scale_att, float* out /* [B,T,H] */, void* ws,
                             size_t ws_bytes, int32_t math, gnnrag_stream_t stream);

/* ---- Fine-tuning the encoder: the layers under autograd (additive to ABI 16; DESIGN.md section 8 f-6, Fine-tuning) --------
 * The reference's --lm_frozen 0 trains the LM with the GNN.  These two entries are the layers: the embedding stage's output
 * x0 [B T, H] comes in, its gradient g_x0 goes out (the stage itself: gnnrag_bert_embed_forward_save / _backward in the
 * next block, or the caller's own); BertModel / RobertaModel layers (no rel_bias; MPNet's table and its gradient: the
 * _ex forms of the next block).
 *
 * gnnrag_bert_layers_forward_save: the L layers of gnnrag_bert_encode_train on x0 - the same launches on the same values in
 * the same order, so `out` [B T, H] has the bits gnnrag_bert_encode_train gives for the same x0 and masks (keep_hidden: the
 * (1 + 2L)-plane buffer of that call, planes 1 .. 2L are read; keep_att as there; NULL: the inference sequence of the site).
 * out may be x0.  ws: gnnrag_bert_workspace_bytes(B, T, H, I).  It additionally leaves in `reserve`
 * (gnnrag_bert_reserve_bytes(L, B, T, H, I) = L M (8 H + I) 4 bytes, M = B T; 0 for a size <= 0 or H % 4 / I % 4 != 0) per
 * layer, in this order, without padding:
 *   xin [M,H] the layer input | qkv [M,3H] | ctx [M,H] | sum1 [M,H] | x1 [M,H] LayerNorm 1's output | pre [M,I] the FFN
 *   pre-activation (the value in front of the GELU) | sum2 [M,H]
 * sum1 / sum2: the dense output in front of the LayerNorm - dense + bias under hidden dropout (the residual is added
 * behind the dropout), dense + bias + residual without it.  The blocks the products write are written in place; xin, x1
 * and pre are kept by a device copy.
 *
 * gnnrag_bert_layers_backward: from g_out [M,H] (the gradient of `out`), the reserve and the masks and scales of the
 * forward: g_x0 [M,H] and per layer (grads: HOST array of L structs of device pointers, or NULL) dW_qkv [3H,H], db_qkv [3H],
 * dW_o, db_o, dW_i, db_i, dW_f, db_f and the four LayerNorm vectors.  A NULL output pointer: that gradient is not wanted
 * and its product is not launched.  Layers L-1 .. 0; per layer LayerNorm 2, FFN-out, GELU, FFN-in, LayerNorm 1, attention
 * output, attention, QKV.  Every dense product is exact fp32 on existing entry points: gnnrag_linear on a transposed copy
 * of the weight (the residual's gradient in its add epilogue), gnnrag_gemm_tn for the weights, 8-slice column sums for the
 * biases and LayerNorm vectors.  The key third of db_qkv is written as exactly +0: every row of dS sums to zero, so that
 * gradient is mathematically zero and autograd leaves rounding residue there; dW_qkv and g_x0 keep their key terms.
 * The attention step recomputes the probabilities from qkv (nothing [T,T] is stored by the forward); one workgroup per
 * (question, head), no atomics: a wave owns a query row for dQ, the owner of key j sums dK_j and dV_j over the query rows
 * in ascending order; a query row whose keys are all dropped gives a zero dQ row and adds nothing to dK, dV.
 * Workspace: gnnrag_bert_layers_backward_workspace_bytes(B, T, H, heads, I) (0 for a shape outside the rules; like
 * gnnrag_gemm_tn_workspace_bytes it depends on the current device).  fp32 throughout, nothing allocated, nothing waits for
 * the stream, a second call gives the same bits, the rows of g_x0 of a question do not depend on the batch around it.
 * Rules of both calls, answered in this order before anything is launched: a size <= 0 (L <= 0 included) or an unknown
 * math is GNNRAG_E_BADARG; then the shape rules whatever the pointers are: H % heads != 0, H / heads not in {32, 64}, T > 128,
 * H % 4 != 0, I % 4 != 0 are GNNRAG_E_UNSUPPORTED; then a NULL among x0 / g_out, layers, out, reserve, ws or a needed layer
 * pointer, or a scale of a given mask that is not finite and > 0, is GNNRAG_E_BADARG; then a pointer that is not 16-byte
 * aligned (keep_hidden: 4) is GNNRAG_E_UNSUPPORTED; then a reserve or workspace below the stated size is GNNRAG_E_WORKSPACE.
 *
 * The three kernels alone (tests): gnnrag_bert_attention_backward (d_qkv [M,3H] fully written; ws of
 * gnnrag_bert_attention_backward_workspace_bytes(B, T, heads) = B heads 2 T T 4 bytes), gnnrag_bert_ln_backward (the row is
 * rebuilt as d m + res with keep given - res and dY are then required, dY = dz m - and as d without; summ [M,H] receives
 * dy xhat; dgamma / dbeta [H] or NULL are its and dy's column sums) and gnnrag_bert_gelu_backward (d_pre = d_act gelu'(pre),
 * gelu' = Phi(x) + x phi(x) with Phi by erf; d_pre may be d_act; act [n] or NULL receives gelu(pre)). */
typedef struct gnnrag_bert_layer_grads { float *dW_qkv, *db_qkv, *dW_o, *db_o, *dln1_g, *dln1_b,
                                               *dW_i, *db_i, *dW_f, *db_f, *dln2_g, *dln2_b; } gnnrag_bert_layer_grads;
size_t gnnrag_bert_reserve_bytes(int32_t L, int32_t B, int32_t T, int32_t H, int32_t I);
int gnnrag_bert_layers_forward_save(const float* x0 /* [B T,H] */, int32_t L, const gnnrag_bert_layer* layers, float ln_eps,
                                    int32_t B, int32_t T, int32_t H, int32_t heads, int32_t I,
                                    const uint8_t* keep_hidden /* or NULL */, float scale_hidden,
                                    const uint8_t* keep_att /* or NULL */, float scale_att, float* out /* [B T,H] */,
                                    void* reserve, size_t reserve_bytes, void* ws, size_t ws_bytes, int32_t math,
                                    gnnrag_stream_t stream);
size_t gnnrag_bert_layers_backward_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t heads, int32_t I);
int gnnrag_bert_layers_backward(const float* g_out /* [B T,H] */, int32_t L, const gnnrag_bert_layer* layers, float ln_eps,
                                int32_t B, int32_t T, int32_t H, int32_t heads, int32_t I,
                                const uint8_t* keep_hidden /* or NULL */, float scale_hidden,
                                const uint8_t* keep_att /* or NULL */, float scale_att, const void* reserve,
                                size_t reserve_bytes, float* g_x0 /* [B T,H] or NULL */,
                                const gnnrag_bert_layer_grads* grads /* or NULL */, void* ws, size_t ws_bytes,
                                gnnrag_stream_t stream);
size_t gnnrag_bert_attention_backward_workspace_bytes(int32_t B, int32_t T, int32_t heads);
int gnnrag_bert_attention_backward(const float* qkv, const float* d_ctx, int32_t B, int32_t T, int32_t heads, int32_t dh,
                                   const uint8_t* keep /* [B,heads,T,T] or NULL */, float scale, float* d_qkv, void* ws,
                                   size_t ws_bytes, gnnrag_stream_t stream);
int gnnrag_bert_ln_backward(const float* dy, const float* d, const uint8_t* keep /* or NULL */, float scale,
                            const float* res /* or NULL */, const float* g, float eps, int64_t M, int32_t H, float* dz,
                            float* dY /* or NULL */, float* summ, float* dgamma /* or NULL */, float* dbeta /* or NULL */,
                            gnnrag_stream_t stream);
int gnnrag_bert_gelu_backward(const float* pre, const float* d_act, int64_t n, float* d_pre, float* act /* or NULL */,
                              gnnrag_stream_t stream);

/* ---- Fine-tuning the whole encoder: the embedding stage and MPNet's relative bias (additive to ABI 16) ----
 * With these the three classes run from the ids to last_hidden_state and back to every parameter on the library.
 *
 * gnnrag_bert_embed_forward_save: the embedding launch of gnnrag_bert_encode_train on the same arguments (pad_id >= 0:
 * positions from the ids; type_emb NULL: no token-type term; keep: plane 0 of keep_hidden, [M,H] bytes, or NULL), so `out`
 * [M,H] has that call's bits, M = B T.  A second launch leaves in `reserve` (gnnrag_bert_embed_reserve_bytes(B, T, H) =
 * M (H + 1) 4 bytes; 0 for a size <= 0 or H % 4 != 0), without padding: sum0 [M,H], the row in front of the LayerNorm, then
 * pos [M] int32, the position row of every token; -1 for a token whose id or position lies outside its table (the forward
 * makes that row NaN, and its sum0 row NaN).
 *
 * gnnrag_bert_embed_backward: from g_x0 [M,H], the reserve, the ids, the keep bytes and scale of the forward and the
 * LayerNorm weight.  The dropout sits BEHIND this LayerNorm: dy = g_x0 m, then the LayerNorm backward on sum0 gives dz
 * [M,H], d_ln_g = colsum(dy xhat), d_ln_b = colsum(dy) (8-slice column sums).  The tables are dense, fully written outputs:
 *   d_word [vocab,H], d_pos [max_pos,H]: row k is the sum of the dz rows of the tokens that name it, in ascending row order;
 *     a row no token names is exactly +0, and so is row word_pad / pos_pad (transformers' padding_idx; -1: none).  A token
 *     with pos = -1, a pos >= max_pos or an id outside [0, vocab) adds to neither table and indexes nothing.
 *   d_type [n_type,H]: row 0 is the column sum of dz (every token has type 0), the other rows +0.
 * No sort and no atomics: a wave per (token, table) compares its key with the keys of all rows, 64 per ballot; the first
 * row of a key owns the table row.  That is M M / 64 ballots per table: M <= 65536 rows, more is GNNRAG_E_UNSUPPORTED.
 * Any of the five outputs may be NULL: not wanted, not computed.  Workspace: gnnrag_bert_embed_backward_workspace_bytes(B,
 * T, H) = three [M,H] blocks on 256-byte boundaries (0 for a size <= 0 or a shape outside the rules).
 * Rules of both calls, in this order before anything is launched: a size <= 0 (n_type with d_type given included) is
 * GNNRAG_E_BADARG; then the shape rules whatever the pointers are - H % 4 != 0, M too large, and for the forward T > 128,
 * T > max_pos, T + pad_id > max_pos - 1 - are GNNRAG_E_UNSUPPORTED; then a NULL among the required pointers or a scale of a
 * given mask that is not finite and > 0 is GNNRAG_E_BADARG; then a pointer that is not 16-byte aligned (ids: 8, keep: 4) is
 * GNNRAG_E_UNSUPPORTED; then a reserve or workspace below the stated size is GNNRAG_E_WORKSPACE.
 *
 * gnnrag_bert_layers_forward_save_ex / gnnrag_bert_layers_backward_ex: the two entries of the block above plus rel_bias
 * [heads, 2T-1] or NULL (MPNet: rel_bias[h][j - i + T - 1] is added to the scaled score of query i and key j of every
 * layer, as gnnrag_bert_encode_train adds it) and, backward, d_rel_bias [heads, 2T-1] or NULL.  With rel_bias NULL they
 * enqueue what the entries above enqueue, which are these calls with NULL.  The attention backward recomputes the
 * probabilities with the bias; an all-zero table gives the bits of the call without one.  d_rel_bias[h][d + T - 1] =
 * sum_b sum_{i, j = i + d} dS[b,h,i,j], read from the dS squares the attention backward leaves in its scratch: one owner
 * per entry, b ascending, then i ascending; the layers share the table, their sums are added in the order L-1 .. 0 and the
 * output is fully written.  The key third of db_qkv stays +0: the rows of dS still sum to zero.  d_rel_bias without
 * rel_bias is GNNRAG_E_BADARG; both pointers are 16-byte aligned; every other rule, the reserve and the workspaces are
 * those of the block above.
 *
 * The two kernels alone (tests): gnnrag_bert_attention_backward_bias (gnnrag_bert_attention_backward plus rel_bias or NULL;
 * ws receives [B heads, 2, T, T]: the dS and the dropped-probability square of every (question, head)) and
 * gnnrag_bert_rel_bias_reduce (d_bias [heads, 2T-1], fully written, from such a scratch); and the table step of the
 * embedding backward alone, gnnrag_bert_embed_scatter: d_word / d_pos (either may be NULL) from a given dz [M,H], ids [M] and
 * pos [M] int32, with that call's rules for M, H, the two pads and the tokens that name no row. */
size_t gnnrag_bert_embed_reserve_bytes(int32_t B, int32_t T, int32_t H);
int gnnrag_bert_embed_forward_save(const int64_t* ids, const float* word_emb, int32_t vocab, const float* pos_emb,
                                   int32_t max_pos, const float* type_emb /* or NULL */, int32_t pad_id /* -1: 0..T-1 */,
                                   const float* ln_g, const float* ln_b, float ln_eps, int32_t B, int32_t T, int32_t H,
                                   const uint8_t* keep /* [B T,H] or NULL */, float scale, float* out /* [B T,H] */,
                                   void* reserve, size_t reserve_bytes, gnnrag_stream_t stream);
size_t gnnrag_bert_embed_backward_workspace_bytes(int32_t B, int32_t T, int32_t H);
int gnnrag_bert_embed_backward(const float* g_x0 /* [B T,H] */, const int64_t* ids, const void* reserve,
                               size_t reserve_bytes, int32_t B, int32_t T, int32_t H, int32_t vocab, int32_t max_pos,
                               int32_t n_type, int32_t word_pad /* or -1 */, int32_t pos_pad /* or -1 */,
                               const uint8_t* keep /* [B T,H] or NULL */, float scale, const float* ln_g, float ln_eps,
                               float* d_word /* [vocab,H] or NULL */, float* d_pos /* [max_pos,H] or NULL */,
                               float* d_type /* [n_type,H] or NULL */, float* d_ln_g /* [H] or NULL */,
                               float* d_ln_b /* [H] or NULL */, void* ws, size_t ws_bytes, gnnrag_stream_t stream);
int gnnrag_bert_layers_forward_save_ex(const float* x0 /* [B T,H] */, int32_t L, const gnnrag_bert_layer* layers,
                                       const float* rel_bias /* [heads,2T-1] or NULL */, float ln_eps, int32_t B, int32_t T,
                                       int32_t H, int32_t heads, int32_t I, const uint8_t* keep_hidden /* or NULL */,
                                       float scale_hidden, const uint8_t* keep_att /* or NULL */, float scale_att,
                                       float* out /* [B T,H] */, void* reserve, size_t reserve_bytes, void* ws,
                                       size_t ws_bytes, int32_t math, gnnrag_stream_t stream);
int gnnrag_bert_layers_backward_ex(const float* g_out /* [B T,H] */, int32_t L, const gnnrag_bert_layer* layers,
                                   const float* rel_bias /* [heads,2T-1] or NULL */, float ln_eps, int32_t B, int32_t T,
                                   int32_t H, int32_t heads, int32_t I, const uint8_t* keep_hidden /* or NULL */,
                                   float scale_hidden, const uint8_t* keep_att /* or NULL */, float scale_att,
                                   const void* reserve, size_t reserve_bytes, float* g_x0 /* [B T,H] or NULL */,
                                   const gnnrag_bert_layer_grads* grads /* or NULL */,
                                   float* d_rel_bias /* [heads,2T-1] or NULL */, void* ws, size_t ws_bytes,
                                   gnnrag_stream_t stream);
int gnnrag_bert_attention_backward_bias(const float* qkv, const float* d_ctx, int32_t B, int32_t T, int32_t heads,
                                        int32_t dh, const float* rel_bias /* [heads,2T-1] or NULL */,
                                        const uint8_t* keep /* [B,heads,T,T] or NULL */, float scale, float* d_qkv,
                                        void* ws, size_t ws_bytes, gnnrag_stream_t stream);
int gnnrag_bert_rel_bias_reduce(const float* sq /* [B heads,2,T,T] */, int32_t B, int32_t T, int32_t heads,
                                float* d_bias /* [heads,2T-1] */, gnnrag_stream_t stream);
int gnnrag_bert_embed_scatter(const float* dz /* [M,H] */, const int64_t* ids, const int32_t* pos, int64_t M, int32_t H,
                              int32_t vocab, int32_t max_pos, int32_t word_pad /* or -1 */, int32_t pos_pad /* or -1 */,
                              float* d_word /* [vocab,H] or NULL */, float* d_pos /* [max_pos,H] or NULL */,
                              gnnrag_stream_t stream);

/* ---- Split-K linear for few rows, and the inference encoder on it (additive to ABI 16) ------------
 * C = epilogue(A W^T + bias): A [M, K], W [Nout, K], bias [Nout] or NULL, C [M, Nout], all fp32.  K is cut into `splits`
 * chunks of k_chunk (the last may be short); the first launch writes the chunks' partial products P[s] [M, Nout] into the
 * workspace - exact fp32 MFMA, k ascending inside a chunk, a weight read once per group of up to 64 rows - and the second adds
 * them in chunk order and applies the epilogue:  x = ((P[0] + P[1]) + ... + P[splits-1]) + bias, then
 *   GNNRAG_SPLITK_EPI_BIAS     C = x
 *   GNNRAG_SPLITK_EPI_GELU     C = 0.5 x (1 + erf(x / sqrt 2))     the encoder's own function: equal bits for equal x
 *   GNNRAG_SPLITK_EPI_ADD_LN   C = LayerNorm(x + add) ln_g + ln_b   add [M, Nout]; biased variance, two passes, ln_eps inside
 *                              the root, a wave per row as in the encoder; C may be the buffer add is.  Any Nout % 4 == 0.
 * Two launches (at splits = 1 too), no atomics, no flags or counters between workgroups, no allocation, nothing waits for
 * the stream, safe under capture.
 * Value rule: C[r, c] depends on A[r, :], W[c, :] (all of W for a LayerNorm row), bias, add[r, :], ln_g, ln_b, K and the
 * effective (splits, k_chunk) only - never on M, on where row r sits, or on the device.  splits = 0 takes the library's
 * rule, a host-only function of (K, Nout) alone, so a question's bits do not depend on the batch it rides in; splits >= 1
 * forces the value: k_chunk is then ceil(K / splits) rounded up to a multiple of 4.
 * gnnrag_linear_splitk_plan reports the effective values and the launches (host only; M enters the argument checks only).
 * gnnrag_linear_splitk_workspace_bytes: splits M Nout 4 bytes with the effective splits, rounded up to a multiple of 256;
 * 0 for arguments the call refuses.
 * Rules, answered in this order before anything is launched: a size <= 0, splits < 0 or an unknown epilogue is
 * GNNRAG_E_BADARG; then the shape rules, whatever the pointers are: K % 4 != 0, Nout % 4 != 0, M >= 2^31, splits above
 * GNNRAG_SPLITK_MAX_SPLITS, a forced value that would leave an empty chunk ((splits - 1) k_chunk >= K) or a workspace below
 * the stated size are GNNRAG_E_UNSUPPORTED; then a NULL among A, W, C, ws (ADD_LN: add, ln_g, ln_b) or a NULL plan is
 * GNNRAG_E_BADARG; then a pointer that is not 16-byte aligned is GNNRAG_E_UNSUPPORTED.
 *
 * gnnrag_bert_encode_splitk: gnnrag_bert_encode_ex (its arguments, its rules, its embedding and attention launches) with the
 * four dense products of a layer on gnnrag_linear_splitk at splits = 0: QKV with BIAS, the attention output projection
 * with ADD_LN (add = the residual, C = the residual's buffer), FFN-in with GELU, FFN-out with ADD_LN.  The separate GELU and
 * LayerNorm launches are gone: 9 launches per layer.  Inference only.  The products are exact fp32 whatever `math` is (it is
 * checked, not used).  The workspace is gnnrag_bert_splitk_workspace_bytes(B, T, H, I): qkv, ctx, ffn and the largest of
 * the four products' partials (0 for a size <= 0 or H % 4 / I % 4 != 0, which the call refuses as UNSUPPORTED). */
#define GNNRAG_SPLITK_EPI_BIAS   0
#define GNNRAG_SPLITK_EPI_GELU   1
#define GNNRAG_SPLITK_EPI_ADD_LN 2
#define GNNRAG_SPLITK_MAX_SPLITS 128
typedef struct gnnrag_splitk_plan_t { int32_t splits, k_chunk, launches, reserved[5]; } gnnrag_splitk_plan_t;
int gnnrag_linear_splitk_plan(int64_t M, int32_t K, int32_t Nout, int32_t splits, gnnrag_splitk_plan_t* out);
size_t gnnrag_linear_splitk_workspace_bytes(int64_t M, int32_t K, int32_t Nout, int32_t splits);
int gnnrag_linear_splitk(const float* A, int64_t M, int32_t K, const float* W, const float* bias /* or NULL */,
                         int32_t epi, const float* add, const float* ln_g, const float* ln_b, float ln_eps, float* C,
                         int32_t Nout, int32_t splits, void* ws, size_t ws_bytes, gnnrag_stream_t stream);
size_t gnnrag_bert_splitk_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t I);
int gnnrag_bert_encode_splitk(const int64_t* ids, const float* word_emb, int32_t vocab, const float* pos_emb,
                              int32_t max_pos, const float* type_emb /* or NULL */, int32_t pad_id,
                              const float* rel_bias /* [heads,2T-1] or NULL */, const float* ln_g, const float* ln_b,
                              float ln_eps, int32_t L, const gnnrag_bert_layer* layers, int32_t B, int32_t T, int32_t H,
                              int32_t heads, int32_t I, float* out /* [B,T,H] */, void* ws, size_t ws_bytes,
                              int32_t math, gnnrag_stream_t stream);

/* ---- Relation-text features (additive to ABI 16; SURVEY.md section 8 f-3, the relation-text branch) ----------------------
 * get_rel_feature with --relation_word_emb True (gnn/models/ReaRev/rearev.py:101-106, gnn/models/NSM/nsm.py:103-105):
 * question_emb over the frozen LM token states of the relation vocabulary, then AttnEncoder
 * (gnn/modules/query_update.py:46-61).  Per relation row r and direction, with W [D,K], b [D] = question_emb and
 * a [D] = self_att_r.attn_linear.weight:
 *   h_t   = W x_t + b                                              (rearev.py:102-103)
 *   s_t   = a . h_t = u . x_t + c,   u = W^T a,  c = a . b          (query_update.py:58)
 *   al    = softmax_t(s_t - (1 - mask[r,t]) * 1e8)                  (:59-60; the fp32 difference as written, row maximum
 *                                                                    subtracted)
 *   out_r = sum_t al_t h_t = W xbar_r + b,   xbar_r = sum_t al_t x_t   (:61; sum_t al_t = 1)
 * A padded token of a row that has tokens gets exactly 0; a row of padding only gets the softmax of the ROUNDED values
 * s_t - 1e8 (the uniform 1/T while |s| < 4, multiples of 8 beyond), as the reference does.
 * X_fwd / X_inv [R,T,K] (X_inv NULL: one direction, out_inv must be NULL too), mask [R,T] (1 = token, shared by both
 * directions: rearev.py:105-106), out_fwd / out_inv [R,D], fully written.  xbar [n_dir,R,K] / alpha [n_dir,R,T]: what the
 * backward reads, fully written; xbar NULL: forward only, it lives in the workspace; alpha NULL: not stored.
 * One launch computes u and c (ascending d), one streams X (a workgroup per direction and row, X read from HBM once where
 * T K + K + 2 ceil4(T) floats fit 80 KB of LDS, else the second use re-reads the row), then out = xbar W^T + b on the
 * exact-fp32 gnnrag_linear_pair / gnnrag_linear.  One fixed summation order, no atomics, no allocation, nothing waits for
 * the stream; a row's xbar / alpha bits do not depend on R.
 * Limits: 1 <= T <= GNNRAG_REL_TEXT_MAX_T, K % 4 == 0 and K <= GNNRAG_REL_TEXT_MAX_K, 1 <= D <= GNNRAG_REL_TEXT_MAX_D,
 * 1 <= R <= 2^24, X / xbar / workspace 16-byte aligned, else GNNRAG_E_UNSUPPORTED before anything is launched.  A workspace
 * below gnnrag_rel_text_workspace_bytes(R, T, K, D, n_dir) (0 for a shape outside the limits) is GNNRAG_E_WORKSPACE. */
#define GNNRAG_REL_TEXT_MAX_T 256
#define GNNRAG_REL_TEXT_MAX_K 4096
#define GNNRAG_REL_TEXT_MAX_D 4096
size_t gnnrag_rel_text_workspace_bytes(int64_t R, int32_t T, int32_t K, int32_t D, int32_t n_dir);
int gnnrag_rel_text_pool(const float* X_fwd, const float* X_inv, const float* mask, const float* W, const float* b,
                         const float* a, int64_t R, int32_t T, int32_t K, int32_t D, float* out_fwd, float* out_inv,
                         float* xbar, float* alpha, void* workspace, size_t workspace_bytes, gnnrag_stream_t stream);

/* Backward of the call above: what autograd derives for question_emb.weight, .bias and attn_linear.weight (X is frozen
 * and gets no gradient).  xbar / alpha as the forward left them, g_fwd / g_inv [R,D] the incoming gradients of out_fwd /
 * out_inv - either may be NULL (zeros: that direction is not read).  Both directions accumulate, forward first:
 *   dxbar = g W                                   [R,K]  (gnnrag_linear on a transposed copy of W)
 *   dal_t = dxbar_r . x_t,   ds_t = al_t (dal_t - sum_t' al_t' dal_t')          (the second streaming pass over X)
 *   du    = sum_r sum_t ds_t x_t                  [K]   512 workgroups per direction stride over the rows; their partial
 *                                                       sums are added in 16 slices of workgroup order, slices in order
 *   dW    = g^T xbar (gnnrag_gemm_tn over the stacked directions, g zero-padded to D % 4 == 0)  +  a (x) du
 *   db    = sum_r g_r  (row slices in ascending rows, a fixed tree over the slices)        da = W du
 * c does not move the softmax, so nothing reaches db or da through it; the stored alpha is used on rows of padding too.
 * dW [D,K], db [D], da [D]: each may be NULL - not wanted, not computed; every requested output is fully written.
 * No atomics, no allocation, nothing waits for the stream: a repeated call gives the same bits.  Limits as above, dW
 * 16-byte aligned; a workspace below gnnrag_rel_text_backward_workspace_bytes (which, like gnnrag_gemm_tn_workspace_bytes,
 * depends on the current device) is GNNRAG_E_WORKSPACE before anything is launched. */
size_t gnnrag_rel_text_backward_workspace_bytes(int64_t R, int32_t T, int32_t K, int32_t D, int32_t n_dir);
int gnnrag_rel_text_pool_backward(const float* X_fwd, const float* X_inv, const float* W, const float* a,
                                  const float* xbar, const float* alpha, const float* g_fwd, const float* g_inv,
                                  int64_t R, int32_t T, int32_t K, int32_t D, float* dW, float* db, float* da,
                                  void* workspace, size_t workspace_bytes, gnnrag_stream_t stream);

/* ---- Reasoning paths (additive to ABI 16: new entry points only, nothing above changes) ----------------------------------
 * The retrieval step of GNN-RAG: all shortest paths between the question's entities and the retrieved candidates in the
 * question's subgraph taken as a SIMPLE UNDIRECTED graph - what llm/src/utils/graph_utils.py builds with networkx
 * (build_graph :9-15) and searches with nx.all_shortest_paths per pair (get_truth_paths :37-60), called from
 * llm/src/qa_prediction/build_qa_input.py:114-127.
 *
 * Graph of a question: its facts with head != tail; all facts joining one unordered pair {u, v} (any relation, either
 * orientation) are ONE edge whose relation is that of the fact with the largest fact id (G.add_edge overwrites the
 * attribute): the pair's winning fact. */
typedef struct gnnrag_ugraph {
  int32_t B;        /* questions                                                                  */
  int32_t N;        /* node slots per question                                                    */
  int64_t F;        /* facts of the structure it was made from                                    */
  int64_t cap;      /* records u_adj has room for (2 F); the count in use is u_ptr[B*N], on the device */
  int32_t* u_ptr;   /* [B*N+1]  first neighbour record of each node                               */
  int32_t* u_adj;   /* [cap][2] (neighbour node, winning fact id), neighbours of a node ascending */
} gnnrag_ugraph;

/* Caller-owned device memory of a gnnrag_ugraph / of its build (0 on negative or overflowing sizes). */
size_t gnnrag_ugraph_bytes(int64_t F, int32_t B, int32_t N);
size_t gnnrag_ugraph_scratch_bytes(int64_t F, int32_t B, int32_t N);
/* Derives the adjacency from a structure made by gnnrag_csr_build, gnnrag_csr_build_counts or gnnrag_csr_concat (rows in
 * any order, hub-sorted rows included; only row_ptr / edge / perm are read): a 64-bit-key radix sort of (node,
 * neighbour), run heads flagged and scanned, the largest fact id of each run kept.  No wait for the stream.  Replaces
 * build_graph (graph_utils.py:9-15). */
int gnnrag_ugraph_build(const gnnrag_csr* csr, void* mem, size_t mem_bytes, void* scratch, size_t scratch_bytes,
                        gnnrag_ugraph* out, gnnrag_stream_t stream);

/* Device scratch of gnnrag_shortest_paths: levels (bytes) and path counts of every (question, seed).  0 on bad sizes
 * and for N > 65536 (the levels of a question live in one CU's LDS; larger questions are GNNRAG_E_UNSUPPORTED). */
size_t gnnrag_paths_workspace_bytes(int32_t B, int32_t N, int32_t max_seeds, int32_t max_cands);
/* Worst-case bytes of the five output arrays of gnnrag_shortest_paths, each rounded up to 256 bytes, in the order
 * q_info, pair_info, path_off, path_nodes, path_facts (a caller may carve one block that way).  With P = B * max_seeds *
 * max_cands pairs: q_info [B,2], pair_info [P,2], path_off [P+1], path_nodes [P*max_paths, max_hops+1], path_facts
 * [P*max_paths, max_hops].  0 on bad sizes, max_hops > 254 or P * max_paths >= 2^31. */
size_t gnnrag_paths_out_bytes(int32_t B, int32_t max_seeds, int32_t max_cands, int32_t max_paths, int32_t max_hops);
/* Pairs of question b = its seeds (slots with seed_flag != 0, ascending, the first max_seeds) x its candidates (the first
 * min(cand_cnt[b,1], max_cands) entries of row b of cand_slot: exactly the outputs of gnnrag_topp_candidates, so
 * selection -> paths runs on one stream without a host round trip).  Pair index = (b * max_seeds + seed index) *
 * max_cands + candidate index.  Replaces get_truth_paths (graph_utils.py:37-60).
 *   q_info[b]    = (seeds found, candidates offered): larger than max_seeds / max_cands means the question was cut
 *   pair_info[p] = (n_paths, hops): the true number of shortest paths, saturating at INT32_MAX, and their length; (0, -1)
 *                  when the candidate was not reached within max_hops, an endpoint has no edge, or the pair does not
 *                  exist; seed == candidate with an edge: (1, 0)
 *   path_off     = exclusive scan of min(n_paths, max_paths): the records of pair p are path_off[p] .. path_off[p+1]
 *   path_nodes   = per record max_hops + 1 node ids (question * N + slot) from the seed to the candidate, then -1
 *   path_facts   = per record max_hops winning fact ids (hop i joins nodes i and i + 1), then -1
 * The records of a pair are its paths of rank 0 .. min(n_paths, max_paths) - 1 in rank order, paths ranked
 * lexicographically by their node sequence read from the candidate back to the seed.  Records are written compactly:
 * path_off[P] of them exist, the rest of the two arrays is not touched.  max_hops <= 254 and N <= 65536, else
 * GNNRAG_E_UNSUPPORTED.  Nothing waits for the stream. */
int gnnrag_shortest_paths(const gnnrag_ugraph* graph, const uint8_t* seed_flag, const int32_t* cand_slot,
                          const int32_t* cand_cnt, int32_t max_seeds, int32_t max_cands, int32_t max_paths,
                          int32_t max_hops, int32_t* q_info, int32_t* pair_info, int32_t* path_off, int32_t* path_nodes,
                          int32_t* path_facts, void* workspace, size_t workspace_bytes, gnnrag_stream_t stream);

/* Rule-guided walks: the other path set the reference hands to the LLM.  bfs_with_rule (graph_utils.py:24-47, called for
 * every question entity and every predicted relation path by apply_rules, build_qa_input.py:56-64) returns every WALK
 * seed = v0, v1 .. vL of the question's graph (the gnnrag_ugraph above) whose hop i is an edge of relation rule[i], L =
 * the rule's length.  Walks are not simple paths: nodes repeat, a walk may go back over the edge it just took.  The
 * relation of an edge is that of its winning fact: fact_rel[u_adj[e][1]], fact_rel [F] = the relation id of every fact of
 * the caller's tuple, on the device.
 *
 * Device scratch: the relation of every adjacency record, staged once per call (2 max(F, 1) int32), then the counts
 * down[B][max_rules][max_hops][N] uint32 (walks from a node that complete the rule from hop l on; they do not depend on
 * the seed), each part rounded up to 256 bytes.  0 on bad or overflowing sizes, max_hops > 254 and N > 65536. */
size_t gnnrag_rule_paths_workspace_bytes(int64_t F, int32_t B, int32_t N, int32_t max_rules, int32_t max_hops);
/* Worst-case bytes of the five output arrays, laid out as gnnrag_paths_out_bytes lays them out, with P = B * max_seeds *
 * max_rules pairs.  0 on bad sizes, max_hops > 254 or P * max_paths >= 2^31. */
size_t gnnrag_rule_paths_out_bytes(int32_t B, int32_t max_seeds, int32_t max_rules, int32_t max_paths, int32_t max_hops);
/* Pairs of question b = its seeds (slots with seed_flag != 0, ascending, the first max_seeds) x its rules: rule k of
 * question b is rule_rel[b,k,0 .. rule_len[b,k]) (rules are per question, as predicted_paths is).  Pair index = (b *
 * max_seeds + seed index) * max_rules + rule index.  A rule_len outside [1, max_hops] marks an empty or rejected slot -
 * the one deliberate difference: the reference answers an empty rule with one empty path, which carries no triple.  A
 * relation id that no winning fact carries (negative ids included) never matches.
 *   q_info[b]    = (seeds found, rules with rule_len in [1, max_hops]): a first value above max_seeds means the question
 *                  was cut
 *   pair_info[p] = (n_paths, hops): the true number of walks, saturating at INT32_MAX, and hops = rule_len (also when
 *                  n_paths == 0); (0, -1) where the seed index or the rule does not exist
 *   path_off     = exclusive scan of min(n_paths, max_paths): the records of pair p are path_off[p] .. path_off[p+1]
 *   path_nodes   = per record max_hops + 1 node ids (question * N + slot) from the seed outwards, then -1
 *   path_facts   = per record max_hops winning fact ids (hop i joins nodes i and i + 1), then -1
 * The records of a pair are its walks of rank 0 .. min(n_paths, max_paths) - 1 in rank order, walks ranked
 * lexicographically by their node sequence read from the seed outwards (ascending node id): deterministic, independent
 * of the question's place in the batch; the reference's own order (networkx insertion order) is not reproduced.  Records
 * are written compactly: path_off[P] of them exist, the rest of the two arrays is not touched.  max_hops <= 254 and N <=
 * 65536, else GNNRAG_E_UNSUPPORTED; a workspace below the stated size is GNNRAG_E_WORKSPACE before anything is
 * launched.  Nothing waits for the stream, no atomics, no result depends on what an output or the workspace held. */
int gnnrag_rule_paths(const gnnrag_ugraph* graph, const int32_t* fact_rel, const uint8_t* seed_flag,
                      const int32_t* rule_rel, const int32_t* rule_len, int32_t max_seeds, int32_t max_rules,
                      int32_t max_paths, int32_t max_hops, int32_t* q_info, int32_t* pair_info, int32_t* path_off,
                      int32_t* path_nodes, int32_t* path_facts, void* workspace, size_t workspace_bytes,
                      gnnrag_stream_t stream);

/* ---- Optimiser step (additive to ABI 16; optim.hip) -----------------------------------------------------------------------
 * The two statements that end a training step (gnn/train_model.py:228-230): torch.nn.utils.clip_grad_norm_ over a list of
 * gradients and torch.optim.Adam.step (torch/optim/adam.py::_single_tensor_adam, non-capturable; no amsgrad, no maximize,
 * coupled weight decay) over a list of tensors, in three launches whatever the number of tensors.  All math is fp32 except
 * the one sum named below; no atomics; one summation order, so a second call on the same inputs gives the same bits.
 *
 * A DEVICE array of gnnrag_optim_seg, one entry per tensor, drives the three kernels.  The unit of work is a chunk of
 * GNNRAG_OPTIM_CHUNK elements of one tensor; first_chunk is the prefix sum of ceil(n / GNNRAG_OPTIM_CHUNK) over the entries
 * before this one (entry 0: 0) and n_chunks of the calls below is that sum over all T entries.  A tensor's last chunk is
 * handled by element count (nothing is padded, nothing is read or written past n).  A tensor whose pointers (g alone for
 * the norm; p, g, m and v for the step) are all 16-byte aligned is accessed 16 bytes at a time, any other 4 bytes at a time:
 * the same values either way.  An entry with n == 0 owns no chunk and is never touched.
 *
 * The scalars are what torch forms on the host in double and hands to fp32 ops, each rounded to fp32 once: beta2,
 * om_beta1 = 1 - beta1 and om_beta2 = 1 - beta2 (the weights of lerp_ and addcmul_), eps, weight_decay,
 * step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) with t the tensor's step count AFTER its increment.
 * Per-tensor scalars cover parameter groups and per-parameter step counts without further machinery.  80 bytes: four
 * pointers, two int64 and eight floats (the six named quantities do not fit the 64 bytes first planned for them, and
 * 1 - beta formed in fp32 from a rounded beta would be off by 1e-5 relative for beta2 = 0.999). */
#define GNNRAG_OPTIM_CHUNK 4096
typedef struct gnnrag_optim_seg {
  float* p;              /* parameter, updated in place (gnnrag_adam_step only)                      */
  const float* g;        /* gradient, never written                                                  */
  float* m;              /* exp_avg, updated in place (gnnrag_adam_step only)                        */
  float* v;              /* exp_avg_sq, updated in place (gnnrag_adam_step only)                     */
  int64_t n;             /* elements                                                                 */
  int64_t first_chunk;   /* chunks of the entries before this one                                    */
  float beta1, beta2, om_beta1, om_beta2, eps, weight_decay, step_size, bc2_sqrt;
} gnnrag_optim_seg;

/* gnnrag_grad_norm: out2[0] = total_norm = sqrt(sum over all tensors of sum g^2), out2[1] = clip_coef =
 * min(1, max_norm / (total_norm + 1e-6)) as clip_grad_norm_ forms it (a NaN norm gives a NaN coefficient; an infinite one
 * gives 0).  Reads g, n and first_chunk of an entry only.  Two launches: per chunk, the thread-strided fp32 sum of squares
 * through the library's block sum into the workspace; then one workgroup adds the chunks' sums in ascending chunk order in
 * double and rounds the root to fp32 once.  workspace: gnnrag_optim_workspace_bytes(n_chunks) bytes (0 for n_chunks <= 0);
 * every byte the second launch reads was written by the first.
 * gnnrag_adam_step: per element, in torch's order,
 *   g' = g * clip_coef[0]  (clip_coef a DEVICE pointer, e.g. out2 + 1; NULL: no clipping)
 *   g' += weight_decay * p  (if weight_decay != 0)
 *   m  += (g' - m) * om_beta1                      (lerp_; the other branch of lerp's formula where om_beta1 >= 0.5)
 *   v   = v * beta2 + om_beta2 * g' * g'
 *   p  -= step_size * m / (sqrt(v) / bc2_sqrt + eps)        with IEEE division and square root
 * One launch; writes p, m and v and nothing else: g is NOT rescaled (clip_grad_norm_ rescales .grad in place).
 * Both: a NULL segs / out2, T <= 0, n_chunks <= 0 or max_norm not > 0 (NaN included) is GNNRAG_E_BADARG, a workspace that is
 * NULL or below the stated size GNNRAG_E_WORKSPACE, both before a device is touched.  Nothing is allocated, nothing waits
 * for the stream.  The table must stay unchanged until the launches have run (it is read on the device). */
size_t gnnrag_optim_workspace_bytes(int64_t n_chunks);
int gnnrag_grad_norm(const gnnrag_optim_seg* segs, int32_t T, int64_t n_chunks, float max_norm, float* out2,
                     void* workspace, size_t workspace_bytes, gnnrag_stream_t stream);
int gnnrag_adam_step(const gnnrag_optim_seg* segs, int32_t T, int64_t n_chunks, const float* clip_coef,
                     gnnrag_stream_t stream);

/* Plain HBM copy kernel (float4 per lane) used by bench.py to measure the achievable
 * streaming ceiling next to the 8 TB/s spec.  n = number of floats (multiple of 4). */
int gnnrag_stream_copy(const float* src, float* dst, int64_t n, gnnrag_stream_t stream);

int gnnrag_abi_version(void);
const char* gnnrag_error_string(int code);

#ifdef __cplusplus
}
#endif
#endif /* GNNRAG_H_ */
