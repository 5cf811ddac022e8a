// Internal entry points shared by the dense kernels' translation units and the layer driver (softmax_layer.hip).
#pragma once
#include "gnnrag_common.h"

namespace gnnrag {

// tables_vq_launch that ALSO zeroes `zero_n` floats at `zero` (may be null): the layer driver passes the layer's score
// buffer, onto which k_update_b3 accumulates its two column parts' shares - that kernel's own memset launch (~5 us
// per layer) is then skipped (update_score_fused_z(..., score_zeroed = true)).
// packed: `planes` is the packed sparse operand (gnnrag_rel_transform_packed: [2][R1][1408 B] of one layer) instead of
// the public planes - what the layer driver passes
int tables_vq_launch_z(const gnnrag_csr* csr, const void* planes, const float* ins, const float* W, float* P, int32_t D,
                       int32_t I, int32_t only_dir, float* zero, int64_t zero_n, hipStream_t stream, bool packed);
// bytes of one layer's packed operand (fits the slot of tables_vq_planes_bytes: 2 * 1408 against 6 * 896 per row)
size_t tables_vq_packed_bytes(int64_t R1);

// Row-gated form of the self-block update: `nbr` holds valid data only in the rows whose byte in add_flag is non-zero,
// every other row reads the ZERO ROW behind the buffer (row index BN), so the unflagged rows of nbr are never
// touched (frontier layers: frontier.hip).  add_flag: [BN + at least 16 bytes of readable padding] (the kernels
// read a lane's four row gates as one dword at tile granularity: up to 15 bytes past BN when BN % 16 != 0; the frontier
// workspace pads by 64), 4-byte aligned.
// Returns GNNRAG_E_UNSUPPORTED (nothing launched) when the kernel the shape would take has no gated form.
int update_score_fused_rows(const float* h, const float* nbr, const uint8_t* add_flag, const float* W, const float* b,
                            const float* w_s, const float* b_s, const float* mask, float* h_out, float* score,
                            int64_t BN, int32_t D, int32_t I, int32_t math, hipStream_t stream, bool score_zeroed);
int update_b3_launch_f(const float* h, const float* nbr, const uint8_t* add_flag, const float* W, const float* b,
                       const float* w_s, const float* b_s, const float* mask, float* h_out, float* score, int64_t BN,
                       int32_t D, int32_t ldw, hipStream_t stream, bool score_zeroed);

// true when update_score_fused_rows has a row-gated kernel for this shape / alignment / math mode (gemm_f32.hip)
bool update_rows_supported(const float* h, const float* nbr, const float* W, const float* h_out, int64_t BN, int32_t D,
                           int32_t I, int32_t math);
bool update_b3_shape_ok(int64_t BN, int32_t D, int32_t ldw);
// frontier.hip: relation tables of small batches on the one-workgroup-per-tile, split-k kernel (exact fp32)
int tables_small_launch(const gnnrag_csr* csr, const float* T_fwd, const float* T_inv, const float* ins, const float* W,
                        float* P, int32_t D, int32_t I, hipStream_t stream);

// frontier.hip: the frontier of a (sparse) prior; also zeroes two float ranges on the way (score buffer, zero row)
int frontier_build_z(const gnnrag_csr* csr, const float* dist, void* fws, size_t fws_bytes, float* zero_a,
                     int64_t zero_na, float* zero_b, int64_t zero_nb, hipStream_t stream);
const uint8_t* frontier_row_flags(const gnnrag_csr* csr, const void* fws);
struct FrontierArgs;                       // seed_prologue.h
int frontier_args(const gnnrag_csr* csr, const float* dist, void* fws, size_t fws_bytes, float* zero_a, int64_t zero_na,
                  float* zero_b, int64_t zero_nb, FrontierArgs* a);

// gemm_tn.hip: C [N1, N2] = A^T . Bd with Bd = keep ? [B0 | B1] * scale : +0 (B0 [M, K0], B1 [M, N2 - K0], keep [M, N2]
// 0/1 bytes or null) formed as B is loaded; gnnrag_gemm_tn's chunks, reduce and workspace.  The caller has checked
// N1 % 4 == K0 % 4 == N2 % 4 == 0, 16-byte aligned float operands and a 4-byte aligned keep.
int gemm_tn_drop(const float* A, const float* B0, const float* B1, const uint8_t* keep, float scale, int64_t M, int32_t N1,
                 int32_t K0, int32_t N2, float* C, void* workspace, size_t workspace_bytes, hipStream_t stream);

// gemm_tn.hip: the chunks' partial blocks part [chunks][N1][I D] of A^T . Z with Z[m, i D + k] = relu(T[r_m, k] *
// ins[b_m, i, k]), (b_m, r_m) = rows[m], formed as B is loaded (gnnrag_relation_tables' generated operand); chunks =
// gemm_tn_gen_chunks(M, N1, I D), gnnrag_gemm_tn's.  The caller adds the chunks in chunk order (rel_tables_bwd.hip) and has
// checked N1 % 4 == D % 4 == 0 and 16-byte aligned float operands.
int gemm_tn_gen_chunks(int64_t M, int32_t N1, int32_t N2);
int gemm_tn_gen_partials(const float* A, const float* T, const float* ins, const int32_t* rows, int64_t M, int32_t N1,
                         int32_t D, int32_t I, float* part, hipStream_t stream);

// gnnrag_update_score_fused with the promise that `score` already holds zeros
int update_score_fused_z(const float* h, const float* nbr, const float* W, const float* b, const float* w_s,
                         const float* b_s, const float* mask, float* h_out, float* score, int64_t BN, int32_t D,
                         int32_t I, int32_t math, hipStream_t stream, bool score_zeroed);

// rel_transform.hip: whether gnnrag_rel_transform takes these operands (then, and only then, it writes T and the planes)
bool rel_transform_accepts(const float* relfeat_fwd, const float* relfeat_inv, int64_t R1, int32_t D, int32_t L,
                           const gnnrag_layer_params* layers, int32_t pos_rows, const float* T_out, const void* planes_out);
// gnnrag_rel_transform with the planes (planes_out), the packed sparse operand (packed_out) or neither beside T
int rel_transform_launch(const float* relfeat_fwd, const float* relfeat_inv, int64_t R1, int32_t D, int32_t L,
                         const gnnrag_layer_params* layers, int32_t pos_rows, float* T_out, void* planes_out,
                         void* packed_out, gnnrag_stream_t stream);
// The same projections AND the frontier build of `dist` (frontier_build_z's arguments) in ONE launch, each workgroup
// running one or the other (k_seed_prologue).  Returns GNNRAG_E_UNSUPPORTED, nothing launched, outside its range
// (rel_transform_accepts false, L > 8 layers, R1 > 2048 or no relation rows): the caller then makes the two launches.
int seed_prologue_launch(const gnnrag_csr* csr, const float* dist, void* fws, size_t fws_bytes, float* zero_a,
                         int64_t zero_na, float* zero_b, int64_t zero_nb, const float* relfeat_fwd,
                         const float* relfeat_inv, int32_t D, int32_t L, const gnnrag_layer_params* layers,
                         int32_t pos_rows, float* T_out, void* packed_out, gnnrag_stream_t stream);

}  // namespace gnnrag
