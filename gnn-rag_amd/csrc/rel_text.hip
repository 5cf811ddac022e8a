// Relation-text features (the relation-text branch): get_rel_feature with
// --relation_word_emb True (reference gnn/models/ReaRev/rearev.py:101-106, gnn/models/NSM/nsm.py:103-105) -
// question_emb (a Linear(word_dim, entity_dim)) over the frozen LM token states of the whole relation vocabulary
// X [R,T,K], then AttnEncoder (gnn/modules/query_update.py:46-61).  With W, b = question_emb, a = attn_linear.weight:
//   h_rt  = W x_rt + b                                            (rearev.py:102)
//   s_rt  = a . h_rt = u . x_rt + c,   u = W^T a [K],  c = a . b  (query_update.py:58)
//   al_r  = softmax_t(s_rt - (1 - m_rt) * 1e8)                    (:59-60; the fp32 arithmetic as written)
//   out_r = sum_t al_rt h_rt = W xbar_r + b,   xbar_r = sum_t al_rt x_rt     (:61; sum_t al_rt = 1)
// so the [R T, K] x [K, D] product of the reference becomes ONE streaming pass over X (scores, softmax, xbar; memory
// bound) and an [R, K] x [K, D] product; the [R,T,D] intermediate is never written.
//
// k_rt_pool: one workgroup per (direction, row).  A wave takes a token: its lanes read x_t as float4 (coalesced), keep it
// in LDS when the row fits (else the second use re-reads it: the row was just read, L2 / Infinity Cache), and reduce
// u . x_t over a fixed __shfl_xor tree.  Softmax as in k_instructions (every wave derives the same maximum and sum), then
// thread j forms float4 column j of xbar in ascending t.  A row's bits do not depend on R or on the other rows.
//
// Backward (what autograd derives for question_emb.weight / .bias and attn_linear.weight; X is frozen):
//   dxbar = g W [R,K];  dal_rt = dxbar_r . x_rt;  ds_rt = al_rt (dal_rt - sum_t' al_rt' dal_rt');  du = sum_r sum_t ds_rt x_rt
//   dW = g^T xbar + a (x) du,   db = sum_r g_r,   da = W du           (c does not move the softmax: nothing through c)
// k_rt_bwd: the second streaming pass over X; a fixed grid of workgroups strides over the rows and keeps its share of du
// in registers, the per-workgroup partial sums are added in workgroup order (k_rt_du_reduce).  No atomics anywhere.
#include "gnnrag_common.h"

#ifndef GNNRAG_RT_THREADS
#define GNNRAG_RT_THREADS 256        // 128 .. 1024, a multiple of 64; never changes a result
#endif

namespace gnnrag {

constexpr int kRtThreads = GNNRAG_RT_THREADS;
constexpr int kRtMaxK = GNNRAG_REL_TEXT_MAX_K;
constexpr int kRtMaxT = GNNRAG_REL_TEXT_MAX_T;
constexpr int kRtMaxD = GNNRAG_REL_TEXT_MAX_D;
constexpr int64_t kRtMaxR = (int64_t)1 << 24;
constexpr int kRtNJ = (kRtMaxK / 4 + kRtThreads - 1) / kRtThreads;    // float4 columns of du one thread owns
constexpr size_t kRtStageBytes = 80 * 1024;      // a row is kept in LDS when two workgroups still share a CU's 160 KB
constexpr int kRtBwdGrid = 512;                  // workgroups per direction of k_rt_bwd: a function of nothing
constexpr int kRtColSlices = 64;                 // row slices of the db column sum: one lane each in the last step
constexpr float kRtMaskOff = 100000000.0f;       // query_update.py:59 (1e8: exact in fp32)

static_assert(kRtThreads % 64 == 0 && kRtThreads >= 128 && kRtThreads <= 1024, "GNNRAG_RT_THREADS");

__device__ __forceinline__ float rt_dot4(f32x4 x, f32x4 w, float acc) {
  acc = fmaf(x[0], w[0], acc);
  acc = fmaf(x[1], w[1], acc);
  acc = fmaf(x[2], w[2], acc);
  return fmaf(x[3], w[3], acc);
}

// floats of dynamic LDS: the row's vector (u or dxbar_r) [K], two [T] arrays (rounded up to 4), the row itself if staged
static inline size_t rt_lds_bytes(int T, int K, bool stage) {
  const size_t T4 = (size_t)(T + 3) / 4 * 4;
  return ((size_t)K + 2 * T4 + (stage ? (size_t)T * K : 0)) * sizeof(float);
}
static inline bool rt_stage(int T, int K) { return rt_lds_bytes(T, K, true) <= kRtStageBytes; }

// u[k] = sum_d a[d] W[d,k] (ascending d), uc[K] = c = sum_d a[d] b[d]
__global__ __launch_bounds__(256) void k_rt_uc(const float* __restrict__ W, const float* __restrict__ b,
                                               const float* __restrict__ a, int K, int D, float* __restrict__ uc) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k > K) return;
  float acc = 0.f;
  if (k < K) {
#pragma unroll 4
    for (int d = 0; d < D; ++d) acc = fmaf(a[d], W[(size_t)d * K + k], acc);
  } else {
    for (int d = 0; d < D; ++d) acc = fmaf(a[d], b[d], acc);
  }
  uc[k] = acc;
}

struct RtPoolArgs {
  const float* X[2];     // [R,T,K] per direction
  const float* mask;     // [R,T]
  const float* uc;       // [K + 1]
  float* xbar;           // [n_dir,R,K]
  float* alpha;          // [n_dir,R,T] or null
  int64_t R;
  int32_t T, K;
};

template <bool STAGE>
__global__ __launch_bounds__(kRtThreads) void k_rt_pool(const RtPoolArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int T = p.T, K4 = p.K >> 2, T4 = (T + 3) / 4 * 4;
  f32x4* uv = (f32x4*)smem;                      // [K4]
  float* sc = smem + p.K;                        // [T]  scores, then attention weights
  f32x4* xs = (f32x4*)(sc + 2 * T4);             // [T, K4]  the row (STAGE)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = kRtThreads >> 6;
  const int dir = blockIdx.y;
  const size_t row = blockIdx.x, orow = (size_t)dir * p.R + row;
  const f32x4* __restrict__ X = (const f32x4*)p.X[dir] + row * T * K4;
  for (int j = tid; j < K4; j += kRtThreads) uv[j] = ((const f32x4*)p.uc)[j];
  const float c = p.uc[p.K];
  const float* mk = p.mask + row * T;
  __syncthreads();
  for (int t = wave; t < T; t += nw) {
    const f32x4* xt = X + (size_t)t * K4;
    float acc = 0.f;
    for (int j = lane; j < K4; j += 64) {
      const f32x4 v = xt[j];
      if (STAGE) xs[t * K4 + j] = v;
      acc = rt_dot4(v, uv[j], acc);
    }
    acc = wave_sum(acc);
    // the fp32 difference the reference writes: a token keeps s, padding becomes s - 1e8 rounded (multiples of 8)
    if (lane == 0) sc[t] = __fsub_rn(__fadd_rn(acc, c), __fmul_rn(__fsub_rn(1.f, mk[t]), kRtMaskOff));
  }
  __syncthreads();
  float m = -INFINITY;
  for (int t = lane; t < T; t += 64) m = fmaxf(m, sc[t]);
  m = wave_max(m);
  float sum = 0.f;
  for (int t = lane; t < T; t += 64) sum += expf(sc[t] - m);
  sum = wave_sum(sum);
  __syncthreads();                               // every wave has read the scores
  for (int t = tid; t < T; t += kRtThreads) {
    const float al = expf(sc[t] - m) / sum;
    sc[t] = al;
    if (p.alpha) p.alpha[orow * T + t] = al;
  }
  __syncthreads();
  f32x4* xb = (f32x4*)p.xbar + orow * K4;
  for (int j = tid; j < K4; j += kRtThreads) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < T; ++t) {
      const f32x4 v = STAGE ? xs[t * K4 + j] : X[(size_t)t * K4 + j];
      acc += sc[t] * v;
    }
    xb[j] = acc;
  }
}

struct RtBwdArgs {
  const float* X[2];       // the active directions' token states
  const float* alpha[2];   // [R,T]
  const float* dxbar;      // [n_act,R,K]
  float* part;             // [n_act, grid, K]
  int64_t R;
  int32_t T, K;
};

template <bool STAGE>
__global__ __launch_bounds__(kRtThreads) void k_rt_bwd(const RtBwdArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int T = p.T, K4 = p.K >> 2, T4 = (T + 3) / 4 * 4;
  f32x4* dv = (f32x4*)smem;                      // [K4]  dxbar_r
  float* sd = smem + p.K;                        // [T]  dal, then ds
  float* sa = sd + T4;                           // [T]  alpha_r
  f32x4* xs = (f32x4*)(sa + T4);                 // [T, K4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = kRtThreads >> 6;
  const int dir = blockIdx.y;
  f32x4 acc[kRtNJ];
#pragma unroll
  for (int i = 0; i < kRtNJ; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int64_t row = blockIdx.x; row < p.R; row += gridDim.x) {
    const f32x4* __restrict__ X = (const f32x4*)p.X[dir] + (size_t)row * T * K4;
    const f32x4* dx = (const f32x4*)p.dxbar + ((size_t)dir * p.R + row) * K4;
    for (int j = tid; j < K4; j += kRtThreads) dv[j] = dx[j];
    for (int t = tid; t < T; t += kRtThreads) sa[t] = p.alpha[dir][(size_t)row * T + t];
    __syncthreads();
    for (int t = wave; t < T; t += nw) {
      const f32x4* xt = X + (size_t)t * K4;
      float d = 0.f;
      for (int j = lane; j < K4; j += 64) {
        const f32x4 v = xt[j];
        if (STAGE) xs[t * K4 + j] = v;
        d = rt_dot4(v, dv[j], d);
      }
      d = wave_sum(d);
      if (lane == 0) sd[t] = d;
    }
    __syncthreads();
    float dot = 0.f;                             // every thread, the same order
    for (int t = 0; t < T; ++t) dot = fmaf(sa[t], sd[t], dot);
    __syncthreads();
    for (int t = tid; t < T; t += kRtThreads) sd[t] = sa[t] * (sd[t] - dot);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kRtNJ; ++i) {
      const int j = tid + i * kRtThreads;
      if (j < K4) {
        for (int t = 0; t < T; ++t) {
          const f32x4 v = STAGE ? xs[t * K4 + j] : X[(size_t)t * K4 + j];
          acc[i] += sd[t] * v;
        }
      }
    }
    __syncthreads();                             // the next row overwrites dv, sd, sa, xs
  }
  f32x4* out = (f32x4*)p.part + ((size_t)dir * gridDim.x + blockIdx.x) * K4;
#pragma unroll
  for (int i = 0; i < kRtNJ; ++i) {
    const int j = tid + i * kRtThreads;
    if (j < K4) out[j] = acc[i];
  }
}

// du[k] = sum of the P partial sums in order: 16 contiguous slices, a slice in ascending p, the slices added in order
// (not colsum_launch: that one cuts the rows into 8 slices, another summation order)
__global__ __launch_bounds__(1024) void k_rt_du_reduce(const float* __restrict__ part, float* __restrict__ du, int P,
                                                       int K) {
  __shared__ float s[16][64];
  const int kx = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + kx;
  const int per = (P + 15) / 16;
  const int p0 = sl * per, p1 = p0 + per < P ? p0 + per : P;
  float acc = 0.f;
  if (k < K) {
#pragma unroll 8
    for (int q = p0; q < p1; ++q) acc += part[(size_t)q * K + k];
  }
  s[sl][kx] = acc;
  __syncthreads();
  if (sl == 0 && k < K) {
    float v = s[0][kx];
#pragma unroll
    for (int i = 1; i < 16; ++i) v += s[i][kx];
    du[k] = v;
  }
}

// gcat [n_act R, Dp] = the active directions' upstream gradients stacked, columns D .. Dp zero (gnnrag_gemm_tn wants
// N1 % 4 == 0, as lstm_bwd.hip pads h_prev)
__global__ __launch_bounds__(256) void k_rt_gcat(const float* __restrict__ g0, const float* __restrict__ g1, int64_t R,
                                                 int D, int Dp, int64_t n, float* __restrict__ gcat) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t m = i / Dp;
  const int d = (int)(i - m * Dp);
  float v = 0.f;
  if (d < D) v = m < R ? g0[m * D + d] : g1[(m - R) * D + d];
  gcat[i] = v;
}

// column sums of gcat, first level: workgroup (x, y) = 32 columns x the y-th of S row slices; inside, 8 sub-slices in
// ascending rows, added in order -> cpart[y, Dp]
// (not colsum_launch: the sub-slice length comes from the nominal slice height rows_per, not from the slice's own rows)
__global__ __launch_bounds__(256) void k_rt_colsum(const float* __restrict__ gcat, float* __restrict__ cpart, int64_t M,
                                                   int Dp, int64_t rows_per) {
  __shared__ float s[8][32];
  const int cx = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cx;
  const int64_t b0 = (int64_t)blockIdx.y * rows_per, b1 = b0 + rows_per < M ? b0 + rows_per : M;
  const int64_t per = (rows_per + 7) / 8;
  const int64_t m0 = b0 + sl * per, m1 = m0 + per < b1 ? m0 + per : b1;
  float acc = 0.f;
  if (c < Dp) {
#pragma unroll 4
    for (int64_t m = m0; m < m1; ++m) acc += gcat[m * Dp + c];
  }
  s[sl][cx] = acc;
  __syncthreads();
  if (sl == 0 && c < Dp) {
    float v = s[0][cx];
#pragma unroll
    for (int i = 1; i < 8; ++i) v += s[i][cx];
    cpart[(size_t)blockIdx.y * Dp + c] = v;
  }
}

// the last step: workgroups [0, nbw) write dW = tn + a (x) du; the others take 4 rows d each (a wave per row):
// da[d] = W[d,:] . du, db[d] = the S slice sums of column d over the fixed tree
__global__ __launch_bounds__(256) void k_rt_finish(const float* __restrict__ tn, const float* __restrict__ a,
                                                   const float* __restrict__ du, const float* __restrict__ W,
                                                   const float* __restrict__ cpart, int S, int D, int Dp, int K, int nbw,
                                                   float* __restrict__ dW, float* __restrict__ da,
                                                   float* __restrict__ db) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < nbw) {
    const int K4 = K >> 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    if (i >= (int64_t)D * K4) return;
    const int d = (int)(i / K4), j = (int)(i - (int64_t)d * K4);
    f32x4 v = ((const f32x4*)tn)[i];
    if (du) v += a[d] * ((const f32x4*)du)[j];
    ((f32x4*)dW)[i] = v;
    return;
  }
  const int lane = tid & 63, d = ((int)blockIdx.x - nbw) * 4 + (tid >> 6);
  if (d >= D) return;
  if (da) {
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) acc = fmaf(W[(size_t)d * K + k], du[k], acc);
    acc = wave_sum(acc);
    if (lane == 0) da[d] = acc;
  }
  if (db) {
    const float v = wave_sum(lane < S ? cpart[(size_t)lane * Dp + d] : 0.f);
    if (lane == 0) db[d] = v;
  }
}

static bool rt_shape_ok(int64_t R, int32_t T, int32_t K, int32_t D) {
  return R <= kRtMaxR && T <= kRtMaxT && K <= kRtMaxK && (K & 3) == 0 && D <= kRtMaxD;
}

struct RtFwdLayout { size_t uc, xbar, total; };

static RtFwdLayout rt_fwd_layout(int64_t R, int32_t K, int32_t n_dir) {
  RtFwdLayout l;
  Carve cv;
  l.uc = cv.take(((size_t)K + 1) * sizeof(float));
  l.xbar = cv.take((size_t)n_dir * R * K * sizeof(float));
  l.total = cv.off;
  return l;
}

struct RtBwdLayout {
  size_t wt, dxbar, gcat, part, du, tn_out, tn, tn_bytes, cpart, total;
  int32_t Dp;
};

static RtBwdLayout rt_bwd_layout(int64_t R, int32_t K, int32_t D, int32_t n_dir) {
  RtBwdLayout l;
  const size_t M = (size_t)n_dir * R;
  l.Dp = (D + 3) / 4 * 4;
  Carve cv;
  l.wt = cv.take((size_t)K * D * sizeof(float));
  l.dxbar = cv.take(M * K * sizeof(float));
  l.gcat = cv.take(M * l.Dp * sizeof(float));
  l.part = cv.take((size_t)n_dir * kRtBwdGrid * K * sizeof(float));
  l.du = cv.take((size_t)K * sizeof(float));
  l.tn_out = cv.take((size_t)l.Dp * K * sizeof(float));
  l.tn_bytes = gnnrag_gemm_tn_workspace_bytes((int64_t)M, l.Dp, K);
  l.tn = cv.take(l.tn_bytes);
  l.cpart = cv.take((size_t)kRtColSlices * l.Dp * sizeof(float));
  l.total = cv.off;
  return l;
}

template <typename Kern>
static int rt_lds_prepare(Kern kern, size_t lds, DeviceMask& raised) {
  if (lds > 48 * 1024) GNNRAG_RC(raise_lds_cap(kern, raised));
  return 0;
}

}  // namespace gnnrag

using namespace gnnrag;

extern "C" size_t gnnrag_rel_text_workspace_bytes(int64_t R, int32_t T, int32_t K, int32_t D, int32_t n_dir) {
  if (R <= 0 || T <= 0 || K <= 0 || D <= 0 || n_dir < 1 || n_dir > 2 || !rt_shape_ok(R, T, K, D)) return 0;
  return rt_fwd_layout(R, K, n_dir).total;
}

extern "C" int gnnrag_rel_text_pool(const float* X_fwd, const float* X_inv, const float* mask, const float* W,
                                    const float* b, const float* a, int64_t R, int32_t T, int32_t K, int32_t D,
                                    float* out_fwd, float* out_inv, float* xbar, float* alpha, void* ws, size_t ws_bytes,
                                    gnnrag_stream_t stream_) {
  if (!X_fwd || !mask || !W || !b || !a || !out_fwd || (X_inv != nullptr) != (out_inv != nullptr) || R <= 0 || T <= 0 ||
      K <= 0 || D <= 0)
    return GNNRAG_E_BADARG;
  if (!rt_shape_ok(R, T, K, D)) return GNNRAG_E_UNSUPPORTED;
  if (!aligned16(X_fwd, X_inv, xbar, ws)) return GNNRAG_E_UNSUPPORTED;
  const int n_dir = X_inv ? 2 : 1;
  const RtFwdLayout l = rt_fwd_layout(R, K, n_dir);
  if (!ws || ws_bytes < l.total) return GNNRAG_E_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  float* uc = (float*)((char*)ws + l.uc);
  float* xb = xbar ? xbar : (float*)((char*)ws + l.xbar);
  hipLaunchKernelGGL(k_rt_uc, dim3(K / 256 + 1), dim3(256), 0, stream, W, b, a, K, D, uc);
  GNNRAG_LAUNCH_CHECK();
  RtPoolArgs p;
  p.X[0] = X_fwd; p.X[1] = X_inv; p.mask = mask; p.uc = uc; p.xbar = xb; p.alpha = alpha; p.R = R; p.T = T; p.K = K;
  const bool stage = rt_stage(T, K);
  const size_t lds = rt_lds_bytes(T, K, stage);
  const dim3 grid((unsigned)R, (unsigned)n_dir);
  if (stage) {
    static DeviceMask raised{0};
    GNNRAG_RC(rt_lds_prepare(k_rt_pool<true>, lds, raised));
    hipLaunchKernelGGL(k_rt_pool<true>, grid, dim3(kRtThreads), lds, stream, p);
  } else {
    hipLaunchKernelGGL(k_rt_pool<false>, grid, dim3(kRtThreads), lds, stream, p);
  }
  GNNRAG_LAUNCH_CHECK();
  if (n_dir == 2)
    return gnnrag_linear_pair(xb, xb + (size_t)R * K, R, K, W, b, nullptr, nullptr, 0, out_fwd, out_inv, D,
                              GNNRAG_MATH_FP32, stream_);
  return gnnrag_linear(xb, R, K, W, b, nullptr, 0, 0, out_fwd, D, GNNRAG_MATH_FP32, stream_);
}

extern "C" size_t gnnrag_rel_text_backward_workspace_bytes(int64_t R, int32_t T, int32_t K, int32_t D, int32_t n_dir) {
  if (R <= 0 || T <= 0 || K <= 0 || D <= 0 || n_dir < 1 || n_dir > 2 || !rt_shape_ok(R, T, K, D)) return 0;
  return rt_bwd_layout(R, K, D, n_dir).total;
}

extern "C" int gnnrag_rel_text_pool_backward(const float* X_fwd, const float* X_inv, const float* W, const float* a,
                                             const float* xbar, const float* alpha, const float* g_fwd,
                                             const float* g_inv, int64_t R, int32_t T, int32_t K, int32_t D, float* dW,
                                             float* db, float* da, void* ws, size_t ws_bytes, gnnrag_stream_t stream_) {
  if (!X_fwd || !W || !a || !xbar || !alpha || (g_inv && !X_inv) || R <= 0 || T <= 0 || K <= 0 || D <= 0)
    return GNNRAG_E_BADARG;
  if (!rt_shape_ok(R, T, K, D)) return GNNRAG_E_UNSUPPORTED;
  if (!aligned16(X_fwd, X_inv, xbar, dW, ws)) return GNNRAG_E_UNSUPPORTED;
  const int n_dir = X_inv ? 2 : 1;
  const RtBwdLayout l = rt_bwd_layout(R, K, D, n_dir);
  if (!ws || ws_bytes < l.total) return GNNRAG_E_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  if (!dW && !db && !da) return 0;
  // a direction whose upstream gradient is NULL (zeros) contributes nothing and is not read
  const int n_act = (g_fwd ? 1 : 0) + (g_inv ? 1 : 0);
  if (n_act == 0) {
    if (dW) GNNRAG_HIP(hipMemsetAsync(dW, 0, (size_t)D * K * sizeof(float), stream));
    if (db) GNNRAG_HIP(hipMemsetAsync(db, 0, (size_t)D * sizeof(float), stream));
    if (da) GNNRAG_HIP(hipMemsetAsync(da, 0, (size_t)D * sizeof(float), stream));
    return 0;
  }
  const size_t RK = (size_t)R * K, RT = (size_t)R * T;
  const int first = g_fwd ? 0 : 1;               // the direction of the first active block
  const float* gA = g_fwd ? g_fwd : g_inv;
  const float* gB = n_act == 2 ? g_inv : nullptr;
  const float* xbar_act = xbar + first * RK;     // both active: [2,R,K] as it lies
  const int64_t M = (int64_t)n_act * R;
  char* w8 = (char*)ws;
  float* wt = (float*)(w8 + l.wt);
  float* dxbar = (float*)(w8 + l.dxbar);
  float* gcat = (float*)(w8 + l.gcat);
  float* part = (float*)(w8 + l.part);
  float* du = (float*)(w8 + l.du);
  float* tn_out = (float*)(w8 + l.tn_out);
  float* cpart = (float*)(w8 + l.cpart);
  const bool need_du = dW || da;
  int S = 0;
  if (dW || db) {
    const int64_t n = M * l.Dp;
    hipLaunchKernelGGL(k_rt_gcat, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, gA, gB, R, D, l.Dp, n, gcat);
    GNNRAG_LAUNCH_CHECK();
  }
  if (db) {
    const int64_t s0 = (M + 255) / 256;               // at least 256 rows per slice
    S = (int)(s0 < kRtColSlices ? s0 : kRtColSlices);
    const int64_t rows_per = (M + S - 1) / S;
    S = (int)((M + rows_per - 1) / rows_per);
    hipLaunchKernelGGL(k_rt_colsum, dim3((l.Dp + 31) / 32, S), dim3(256), 0, stream, gcat, cpart, M, l.Dp, rows_per);
    GNNRAG_LAUNCH_CHECK();
  }
  if (need_du) {
    GNNRAG_RC(transpose_launch(W, wt, D, K, stream));
    if (n_act == 2) {
      GNNRAG_RC(gnnrag_linear_pair(g_fwd, g_inv, R, D, wt, nullptr, nullptr, nullptr, 0, dxbar, dxbar + RK, K,
                                   GNNRAG_MATH_FP32, stream_));
    } else {
      GNNRAG_RC(gnnrag_linear(gA, R, D, wt, nullptr, nullptr, 0, 0, dxbar, K, GNNRAG_MATH_FP32, stream_));
    }
    RtBwdArgs q;
    q.X[0] = first ? X_inv : X_fwd; q.X[1] = X_inv;
    q.alpha[0] = alpha + first * RT; q.alpha[1] = alpha + RT;
    q.dxbar = dxbar; q.part = part; q.R = R; q.T = T; q.K = K;
    const int G = (int)(R < kRtBwdGrid ? R : kRtBwdGrid);
    const bool stage = rt_stage(T, K);
    const size_t lds = rt_lds_bytes(T, K, stage);
    const dim3 grid((unsigned)G, (unsigned)n_act);
    if (stage) {
      static DeviceMask raised{0};
      GNNRAG_RC(rt_lds_prepare(k_rt_bwd<true>, lds, raised));
      hipLaunchKernelGGL(k_rt_bwd<true>, grid, dim3(kRtThreads), lds, stream, q);
    } else {
      hipLaunchKernelGGL(k_rt_bwd<false>, grid, dim3(kRtThreads), lds, stream, q);
    }
    GNNRAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rt_du_reduce, dim3((K + 63) / 64), dim3(1024), 0, stream, part, du, n_act * G, K);
    GNNRAG_LAUNCH_CHECK();
  }
  if (dW) GNNRAG_RC(gnnrag_gemm_tn(gcat, xbar_act, M, l.Dp, K, tn_out, w8 + l.tn, l.tn_bytes, stream_));
  const int nbw = dW ? (int)(((int64_t)D * (K / 4) + 255) / 256) : 0;
  const int nbd = (da || db) ? (D + 3) / 4 : 0;
  hipLaunchKernelGGL(k_rt_finish, dim3(nbw + nbd), dim3(256), 0, stream, tn_out, a, need_du ? du : nullptr, W, cpart, S,
                     D, l.Dp, K, nbw, dW, da, db);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}
