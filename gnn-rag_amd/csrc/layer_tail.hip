// The tail of the reasoning layer under autograd (gnn/modules/kg_reasoning/reasongnn.py:163-169): what follows the dense
// products of ReasonGNNLayer._forward_autograd, forward and backward.  With pre = pre_a (+ pre_b), the dropout keep flags
// k (0/1 bytes, scale = 1 / (1 - p)), the score vector w, its bias and the node mask:
//   h     = max(pre, 0)                                                    (:163, one fp32 add, then the relu)
//   s     = scale * sum_d h[d] k[d] w[d] + b_score                         (:167: score_func(linear_drop(h)))
//   score = s + (1 - mask) * kVeryNeg                                      (:168, fp32, no contraction)
//   dist  = softmax over a question's nodes                                (:169: the k_masked_softmax launch)
// Backward, from g_h (the node state's gradient) and g_dist:
//   sigma = sum_n dist g_dist (per question)      gs[n] = dist[n] (g_dist[n] - sigma)
//   g_pre = h > 0 ? g_h + gs w k scale : 0        dw[d] = sum_r gs[r] k[r,d] scale h[r,d]        db_score = 0
//
//   k_lt_fwd     streams the rows, a wave per row (the pattern of k_qr_dent); lane l owns the columns 4 (l + 64 j) .. + 3 of a
//                row, as one float4 where D % 4 == 0 and every base is 16-byte aligned (keep: 4-byte), else element by
//                element with the SAME ownership - both forms add a row's products in the same order and give the same
//                bits.  The row sum goes over a fixed __shfl_xor tree.  Grid capped and grid-strided.
//   k_lt_gs      one workgroup per question: sigma in one fixed order (thread-strided sums, then block_sum),
//                then gs [B, N] to the workspace.
//   k_lt_bwd     the same row walk; writes EVERY element of g_pre.  A lane keeps the dw sums of its columns in registers
//                over all rows its wave walks, the workgroup's waves combine through LDS in wave order and the workgroup
//                writes one partial row to the workspace.
//   k_lt_dw_sum  adds the partial rows in 16 fixed slices, the slices in order (the pattern of k_rt_du_reduce).
// No atomics, no allocation, nothing waits for the stream.  Grids and summation orders depend on (B, N, D) only: a second
// call gives the same bits; h, score, dist and g_pre of a question do not depend on the batch around it.
#include "gnnrag_common.h"

namespace gnnrag {

constexpr int kLtWaves = 4;              // waves (= rows in flight) per workgroup of the row kernels
constexpr int kLtFwdGrid = 2048;         // 256 CUs x 8 workgroups: the cap of the forward's grid
constexpr int kLtBwdGrid = 1024;         // the backward's cap = the most partial rows k_lt_dw_sum adds
constexpr int kLtSlices = 16;            // slices of the partial rows in k_lt_dw_sum

// columns 4 c .. 4 c + 3 of a row of D floats; beyond D: zeros
template <bool VEC>
__device__ __forceinline__ f32x4 lt_ld4(const float* __restrict__ row, int c, int D) {
  if (VEC) return ((const f32x4*)row)[c];
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  const int d = 4 * c;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (d + e < D) v[e] = row[d + e];
  return v;
}

template <bool VEC>
__device__ __forceinline__ void lt_st4(float* __restrict__ row, int c, int D, f32x4 v) {
  if (VEC) {
    ((f32x4*)row)[c] = v;
    return;
  }
  const int d = 4 * c;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (d + e < D) row[d + e] = v[e];
}

// the keep flags of the same columns as 0.f / 1.f; keep == null: all 1
template <bool VEC>
__device__ __forceinline__ f32x4 lt_keep4(const uint8_t* __restrict__ row, int c, int D) {
  f32x4 k = {1.f, 1.f, 1.f, 1.f};
  if (!row) return k;
  if (VEC) {
    const uint32_t u = ((const uint32_t*)row)[c];
#pragma unroll
    for (int e = 0; e < 4; ++e) k[e] = ((u >> (8 * e)) & 0xffu) ? 1.f : 0.f;
    return k;
  }
  const int d = 4 * c;
#pragma unroll
  for (int e = 0; e < 4; ++e) k[e] = (d + e < D && row[d + e]) ? 1.f : 0.f;
  return k;
}

template <bool VEC>
__global__ __launch_bounds__(kLtWaves * 64) void k_lt_fwd(const float* __restrict__ pre_a, const float* __restrict__ pre_b,
                                                          const uint8_t* __restrict__ keep, float scale,
                                                          const float* __restrict__ w, const float* __restrict__ b_score,
                                                          const float* __restrict__ mask, int64_t rows, int D,
                                                          float* __restrict__ h_out, float* __restrict__ score) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int C = (D + 3) >> 2;
  const float bs = b_score[0];
  const int64_t step = (int64_t)gridDim.x * kLtWaves;
#pragma unroll 1
  for (int64_t r = (int64_t)blockIdx.x * kLtWaves + wave; r < rows; r += step) {
    const size_t base = (size_t)r * D;
    const uint8_t* kr = keep ? keep + base : nullptr;
    float acc = 0.f;
    for (int c = lane; c < C; c += 64) {
      f32x4 v = lt_ld4<VEC>(pre_a + base, c, D);
      if (pre_b) v += lt_ld4<VEC>(pre_b + base, c, D);
      const f32x4 k = lt_keep4<VEC>(kr, c, D);
      const f32x4 wv = lt_ld4<VEC>(w, c, D);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = !(v[e] <= 0.f) ? v[e] : 0.f;            // relu; a NaN stays a NaN, as torch's does
        acc = fmaf(v[e] * k[e], wv[e], acc);
      }
      lt_st4<VEC>(h_out + base, c, D, v);
    }
    acc = wave_sum(acc);
    // the fp32 sum the reference writes (no contraction): a padded node's score is kVeryNeg for any |s| < 4096
    if (lane == 0)
      score[r] = __fadd_rn(__fadd_rn(__fmul_rn(acc, scale), bs), __fmul_rn(__fsub_rn(1.f, mask[r]), kVeryNeg));
  }
}

// gs[b, n] = dist (g_dist - sigma_b); one workgroup per question
__global__ __launch_bounds__(1024) void k_lt_gs(const float* __restrict__ dist, const float* __restrict__ g_dist, int N,
                                                float* __restrict__ gs) {
  __shared__ float red[16];
  __shared__ float bcast;
  const size_t off = (size_t)blockIdx.x * N;
  const float* __restrict__ p = dist + off;
  const float* __restrict__ g = g_dist + off;
  float s = 0.f;
  for (int i = threadIdx.x; i < N; i += 1024) s = fmaf(p[i], g[i], s);
  const float sigma = block_sum(s, red, &bcast);
  for (int i = threadIdx.x; i < N; i += 1024) gs[off + i] = p[i] * (g[i] - sigma);
}

// NR: float4 rounds per row a lane owns (D <= 256 NR); part == null: no dw wanted; gs == null: g_dist was not given
template <int NR, bool VEC>
__global__ __launch_bounds__(kLtWaves * 64) void k_lt_bwd(const float* __restrict__ h, const uint8_t* __restrict__ keep,
                                                          float scale, const float* __restrict__ w,
                                                          const float* __restrict__ g_h, const float* __restrict__ gs,
                                                          int64_t rows, int D, float* __restrict__ g_pre,
                                                          float* __restrict__ part, float* __restrict__ db) {
  __shared__ f32x4 comb[kLtWaves][NR * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int C = (D + 3) >> 2;
  if (db && blockIdx.x == 0 && threadIdx.x == 0) db[0] = 0.f;     // the softmax does not move under a shift
  const bool sums = part && gs;
  f32x4 wv[NR], acc[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int c = lane + 64 * j;
    acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    wv[j] = (gs && c < C) ? lt_ld4<VEC>(w, c, D) : acc[j];
  }
  const int64_t step = (int64_t)gridDim.x * kLtWaves;
#pragma unroll 1
  for (int64_t r = (int64_t)blockIdx.x * kLtWaves + wave; r < rows; r += step) {
    const size_t base = (size_t)r * D;
    const uint8_t* kr = keep ? keep + base : nullptr;
    const float t = gs ? gs[r] * scale : 0.f;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int c = lane + 64 * j;
      if (c < C) {
        const f32x4 hv = lt_ld4<VEC>(h + base, c, D);
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (g_h) g = lt_ld4<VEC>(g_h + base, c, D);
        if (gs) {
          const f32x4 tk = t * lt_keep4<VEC>(kr, c, D);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            g[e] = fmaf(tk[e], wv[j][e], g[e]);
            acc[j][e] = fmaf(tk[e], hv[e], acc[j][e]);
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = hv[e] > 0.f ? g[e] : 0.f;
        lt_st4<VEC>(g_pre + base, c, D, g);
      }
    }
  }
  if (!part) return;
  if (sums) {
#pragma unroll
    for (int j = 0; j < NR; ++j) comb[wave][lane + 64 * j] = acc[j];
  }
  __syncthreads();
  float* __restrict__ prow = part + (size_t)blockIdx.x * D;
  for (int c = threadIdx.x; c < C; c += kLtWaves * 64) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (sums) {
      v = comb[0][c];
#pragma unroll
      for (int k = 1; k < kLtWaves; ++k) v += comb[k][c];
    }
    lt_st4<false>(prow, c, D, v);
  }
}

// dw[d] = the P partial rows added in kLtSlices fixed slices, the slices in order; P == 0 writes zeros
__global__ __launch_bounds__(kLtSlices * 64) void k_lt_dw_sum(const float* __restrict__ part, float* __restrict__ dw, int P,
                                                              int D) {
  __shared__ float s[kLtSlices][64];
  const int dx = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + dx;
  const int per = (P + kLtSlices - 1) / kLtSlices;
  const int p0 = sl * per, p1 = p0 + per < P ? p0 + per : P;
  float acc = 0.f;
  if (d < D) {
#pragma unroll 8
    for (int q = p0; q < p1; ++q) acc += part[(size_t)q * D + d];
  }
  s[sl][dx] = acc;
  __syncthreads();
  if (sl == 0 && d < D) {
    float v = s[0][dx];
#pragma unroll
    for (int i = 1; i < kLtSlices; ++i) v += s[i][dx];
    dw[d] = v;
  }
}

static inline int lt_grid(int64_t rows, int cap) {
  const int64_t blocks = (rows + kLtWaves - 1) / kLtWaves;
  return (int)(blocks < cap ? blocks : cap);
}

struct LtBwdLayout {
  size_t gs, part, total;
  int grid;
};

static LtBwdLayout lt_bwd_layout(int32_t B, int32_t N, int32_t D) {
  LtBwdLayout l;
  const int64_t rows = (int64_t)B * N;
  l.grid = lt_grid(rows, kLtBwdGrid);
  Carve cv;
  l.gs = cv.take((size_t)rows * sizeof(float));
  l.part = cv.take((size_t)l.grid * D * sizeof(float));
  l.total = cv.off;
  return l;
}

static inline bool lt_shape_ok(int32_t B, int32_t N, int32_t D) {
  return D <= GNNRAG_LAYER_TAIL_MAX_D && (int64_t)B * N <= INT32_MAX;
}

template <int NR>
static void lt_bwd_launch(bool vec, int grid, hipStream_t stream, const float* h, const uint8_t* keep, float scale,
                          const float* w, const float* g_h, const float* gs, int64_t rows, int D, float* g_pre, float* part,
                          float* db) {
  if (vec)
    hipLaunchKernelGGL((k_lt_bwd<NR, true>), dim3(grid), dim3(kLtWaves * 64), 0, stream, h, keep, scale, w, g_h, gs, rows, D,
                       g_pre, part, db);
  else
    hipLaunchKernelGGL((k_lt_bwd<NR, false>), dim3(grid), dim3(kLtWaves * 64), 0, stream, h, keep, scale, w, g_h, gs, rows,
                       D, g_pre, part, db);
}

}  // namespace gnnrag

using namespace gnnrag;

extern "C" int gnnrag_layer_tail_train(const float* pre_a, const float* pre_b, const uint8_t* keep, float scale,
                                       const float* w_score, const float* b_score, const float* mask, int32_t B, int32_t N,
                                       int32_t D, float* h_out, float* score, float* dist, gnnrag_stream_t stream_) {
  if (!pre_a || !w_score || !b_score || !mask || !h_out || !score || !dist || B <= 0 || N <= 0 || D <= 0)
    return GNNRAG_E_BADARG;
  if (!lt_shape_ok(B, N, D)) return GNNRAG_E_UNSUPPORTED;
  if (!keep) scale = 1.f;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t rows = (int64_t)B * N;
  const int grid = lt_grid(rows, kLtFwdGrid);
  const bool vec = (D & 3) == 0 && aligned16(pre_a, pre_b, w_score, h_out) && ((uintptr_t)keep & 3) == 0;
  if (vec)
    hipLaunchKernelGGL(k_lt_fwd<true>, dim3(grid), dim3(kLtWaves * 64), 0, stream, pre_a, pre_b, keep, scale, w_score,
                       b_score, mask, rows, D, h_out, score);
  else
    hipLaunchKernelGGL(k_lt_fwd<false>, dim3(grid), dim3(kLtWaves * 64), 0, stream, pre_a, pre_b, keep, scale, w_score,
                       b_score, mask, rows, D, h_out, score);
  GNNRAG_LAUNCH_CHECK();
  return gnnrag_masked_softmax(score, dist, B, N, stream_);
}

extern "C" size_t gnnrag_layer_tail_backward_workspace_bytes(int32_t B, int32_t N, int32_t D) {
  if (B <= 0 || N <= 0 || D <= 0 || !lt_shape_ok(B, N, D)) return 0;
  return lt_bwd_layout(B, N, D).total;
}

extern "C" int gnnrag_layer_tail_backward(const float* h, const float* dist, const uint8_t* keep, float scale,
                                          const float* w_score, const float* g_h, const float* g_dist, int32_t B, int32_t N,
                                          int32_t D, float* g_pre, float* dw_score, float* db_score, void* workspace,
                                          size_t workspace_bytes, gnnrag_stream_t stream_) {
  if (!h || !dist || !w_score || !g_pre || B <= 0 || N <= 0 || D <= 0) return GNNRAG_E_BADARG;
  if (!g_h && !g_dist) return GNNRAG_E_BADARG;
  if (!lt_shape_ok(B, N, D)) return GNNRAG_E_UNSUPPORTED;
  const LtBwdLayout l = lt_bwd_layout(B, N, D);
  if (!workspace || workspace_bytes < l.total) return GNNRAG_E_WORKSPACE;
  if (!keep) scale = 1.f;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t rows = (int64_t)B * N;
  float* gs = g_dist ? (float*)((char*)workspace + l.gs) : nullptr;
  float* part = (dw_score && g_dist) ? (float*)((char*)workspace + l.part) : nullptr;
  if (g_dist) {
    hipLaunchKernelGGL(k_lt_gs, dim3(B), dim3(1024), 0, stream, dist, g_dist, N, gs);
    GNNRAG_LAUNCH_CHECK();
  }
  const bool vec = (D & 3) == 0 && aligned16(h, g_h, w_score, g_pre) && ((uintptr_t)keep & 3) == 0;
  const int C = (D + 3) / 4;
  if (C <= 64) lt_bwd_launch<1>(vec, l.grid, stream, h, keep, scale, w_score, g_h, gs, rows, D, g_pre, part, db_score);
  else if (C <= 128) lt_bwd_launch<2>(vec, l.grid, stream, h, keep, scale, w_score, g_h, gs, rows, D, g_pre, part, db_score);
  else if (C <= 256) lt_bwd_launch<4>(vec, l.grid, stream, h, keep, scale, w_score, g_h, gs, rows, D, g_pre, part, db_score);
  else if (C <= 512) lt_bwd_launch<8>(vec, l.grid, stream, h, keep, scale, w_score, g_h, gs, rows, D, g_pre, part, db_score);
  else lt_bwd_launch<16>(vec, l.grid, stream, h, keep, scale, w_score, g_h, gs, rows, D, g_pre, part, db_score);
  GNNRAG_LAUNCH_CHECK();
  if (dw_score) {
    hipLaunchKernelGGL(k_lt_dw_sum, dim3((D + 63) / 64), dim3(kLtSlices * 64), 0, stream, part, dw_score, part ? l.grid : 0,
                       D);
    GNNRAG_LAUNCH_CHECK();
  }
  return 0;
}
