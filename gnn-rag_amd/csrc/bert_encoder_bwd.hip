// Backward of the encoder layers of a BERT-class question encoder (bert_encoder.hip, gnnrag_bert_layers_forward_save):
// what fine-tuning the LM (the reference's --lm_frozen 0, gnn/modules/question_encoding/bert_encoder.py:80-87) derives
// for transformers' BertModel / RobertaModel / MPNetModel layers, and of the embedding stage in front of them.
//
// Layers run L-1 .. 0; g is the gradient of the layer's output.  With m = keep ? scale : 0 of the site (1 without a mask):
//   LayerNorm 2   dz2 = LN'(g) on the rebuilt row z = sum2 m + x1; dY = dz2 m             k_bert_ln_bwd
//                 dln2_g = colsum(g xhat), dln2_b = colsum(g)                              colsum_launch
//   FFN out       d_act = dY W_f (gnnrag_linear on W_f^T); db_f = colsum(dY)
//   GELU          d_pre = d_act gelu'(pre), act = gelu(pre)                                k_bert_gelu_bwd
//                 dW_f = dY^T act                                                          gnnrag_gemm_tn
//   FFN in        dW_i = d_pre^T x1; db_i = colsum(d_pre); dx1 = dz2 + d_pre W_i           (the add epilogue of gnnrag_linear)
//   LayerNorm 1   dz1, dY1 from dx1 on z = sum1 m + xin; dln1_g, dln1_b
//   attention out dW_o = dY1^T ctx; db_o = colsum(dY1); d_ctx = dY1 W_o
//   attention     d_qkv from qkv, d_ctx, keep_att                                          k_bert_attention_bwd
//   QKV           dW_qkv = d_qkv^T xin; db_qkv = colsum(d_qkv) with the key third written as +0 (every row of dS sums to
//                 zero: the gradient is mathematically zero, autograd leaves rounding residue); g = dz1 + d_qkv W_qkv
// MPNet (rel_bias given): the attention step recomputes the probabilities with the bias (k_bert_attention_bwd_bias) and the
// table's gradient is the sum of the dS squares along their diagonals, the layers added in the order L-1 .. 0
// (k_bert_rel_bias_reduce).
// The embedding stage (gnnrag_bert_embed_backward; x0 = LN(word[id] + type[0] + pos[p]) m, the dropout BEHIND the LayerNorm):
//   dy = g_x0 m                                                                            k_bert_mask_mul
//   dz = LN'(dy) on the saved row sum0; d_ln_g = colsum(dy xhat), d_ln_b = colsum(dy)      k_bert_ln_bwd<false>, colsum_launch
//   d_type[0] = colsum(dz); d_word[k], d_pos[k] = the dz rows that name k, ascending       k_bert_embed_scatter
// Every backward product is exact fp32 (gnnrag_gemm_tn has no other form).  fp32 throughout, no atomics, every reduction in
// an order the shape alone fixes, nothing allocated, nothing waits for the stream: a second call gives the same bits, and
// the rows of g_x0 of a question depend on that question's rows only (LayerNorm: a wave per row; attention: a workgroup
// per (question, head); the products: a row of C depends on its row of A only).
#include "bert_device.h"
#include "bert_host.h"

#ifndef GNNRAG_BERT_ATT_BWD_THREADS
#define GNNRAG_BERT_ATT_BWD_THREADS 512  // 64 .. 1024, a multiple of 64; decides who owns a row, never a summation order
#endif

namespace gnnrag {

// kBertMaxT, kBertLnRows and the entry points' shape, scale and pointer rules: bert_host.h

// LayerNorm backward of one row by one wave.  The row is rebuilt as the forward formed it: DROP: z = d m + res (d the
// dense output without the residual, m from the keep bytes); else z = d (dense + residual).  Statistics as bert_ln_row
// (two passes, the wave's tree).  With a = dy g and xhat = (z - mean) rstd:
//   dz = rstd (a - mean(a) - xhat mean(a xhat));  summ = dy xhat (the summands of dgamma; those of dbeta are dy itself)
// and, DROP only, dY = dz m: the gradient of the dense output (without a mask it is dz, and dY is not written).
template <bool DROP>
__global__ __launch_bounds__(64 * kBertLnRows) void k_bert_ln_bwd(const float* __restrict__ dy, const float* __restrict__ d,
                                                                  const uint8_t* __restrict__ keep, float scale,
                                                                  const float* __restrict__ res,
                                                                  const float* __restrict__ g, float eps, int M, int H4,
                                                                  float* __restrict__ dz, float* __restrict__ dY,
                                                                  float* __restrict__ summ) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kBertLnRows + (threadIdx.x >> 6);
  if (row >= M) return;
  const size_t off = (size_t)row * H4 * 4;
  const f32x4* src = (const f32x4*)(d + off);
  const f32x4* gy = (const f32x4*)(dy + off);
  const uint32_t* kr = DROP ? (const uint32_t*)(keep + off) : nullptr;
  const f32x4* rr = DROP ? (const f32x4*)(res + off) : nullptr;
  auto load = [&](int i) -> f32x4 {
    if (DROP) return src[i] * bert_keep4(kr[i], scale) + rr[i];
    return src[i];
  };
  const float inv_h = 1.f / (float)(H4 * 4);
  float s = 0.f;
  for (int i = lane; i < H4; i += 64) {
    const f32x4 v = load(i);
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  const float mean = wave_sum(s) * inv_h;
  float q = 0.f;
  for (int i = lane; i < H4; i += 64) {
    const f32x4 v = load(i);
    const float d0 = v[0] - mean, d1 = v[1] - mean, d2 = v[2] - mean, d3 = v[3] - mean;
    q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  const float rstd = 1.f / sqrtf(wave_sum(q) * inv_h + eps);
  float a1 = 0.f, a2 = 0.f;
  for (int i = lane; i < H4; i += 64) {
    const f32x4 v = load(i), y = gy[i], gg = ((const f32x4*)g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = y[e] * gg[e];
      a1 += a;
      a2 += a * ((v[e] - mean) * rstd);
    }
  }
  const float c1 = wave_sum(a1) * inv_h, c2 = wave_sum(a2) * inv_h;
  for (int i = lane; i < H4; i += 64) {
    const f32x4 v = load(i), y = gy[i], gg = ((const f32x4*)g)[i];
    f32x4 o, sm;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = (v[e] - mean) * rstd;
      o[e] = rstd * ((y[e] * gg[e] - c1) - xh * c2);
      sm[e] = y[e] * xh;
    }
    ((f32x4*)(dz + off))[i] = o;
    ((f32x4*)(summ + off))[i] = sm;
    if (DROP) ((f32x4*)(dY + off))[i] = o * bert_keep4(kr[i], scale);
  }
}

// the derivative of bert_gelu: Phi(x) + x phi(x), Phi by erf as the forward has it
__device__ __forceinline__ float bert_gelu_grad(float x) {
  return 0.5f * (1.f + erff(x * 0.70710678118654752440f)) + x * (0.39894228040143267794f * expf(-0.5f * x * x));
}

// d_pre = d_act gelu'(pre) over n floats (16-byte aligned; d_pre may be d_act); ACT: act = gelu(pre) as well.  The last
// n % 4 by the first lanes, as k_bert_gelu.
template <bool ACT>
__global__ __launch_bounds__(256) void k_bert_gelu_bwd(const float* __restrict__ pre, const float* d_act, float* d_pre,
                                                       float* __restrict__ act, size_t n) {
  const size_t n4 = n / 4, stride = (size_t)gridDim.x * blockDim.x;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = tid; i < n4; i += stride) {
    const f32x4 x = ((const f32x4*)pre)[i], gy = ((const f32x4*)d_act)[i];
    f32x4 o, a;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = gy[e] * bert_gelu_grad(x[e]);
      if (ACT) a[e] = bert_gelu(x[e]);
    }
    ((f32x4*)d_pre)[i] = o;
    if (ACT) ((f32x4*)act)[i] = a;
  }
  if (tid < n - n4 * 4) {
    const size_t i = n4 * 4 + tid;
    const float x = pre[i];
    d_pre[i] = d_act[i] * bert_gelu_grad(x);
    if (ACT) act[i] = bert_gelu(x);
  }
}

// the value unchanged, behind a barrier the optimiser does not look through (bert_opaque of bert_encoder.hip)
__device__ __forceinline__ float bert_att_opaque(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// Attention backward: one workgroup per (question, head), T <= 128, DH in {32, 64} (bert_att_shape_ok).  LDS: the head's
// K, V, Q and dO slices [T, DH] with the forward's odd row stride DH + 1, then per wave one row of dS [kBertMaxT].
// Phase 1, a wave per query row i (lanes are keys: lane and lane + 64): the probabilities are recomputed as the forward
// forms them (the scaled dot product, wave_max, expf, wave_sum), then with pt = p m (m = keep ? scale : 0, 1 without DROP)
//   dPt_j = dO_i . V_j     r = sum_j pt_j dPt_j (the wave's tree)     dS_j = p_j (dPt_j m_j - r)
//   dQ_i[d] = (sum_j dS_j K_j[d]) / sqrt(dh)       j ascending, lane d
// and the rows dS_i, pt_i go to the workgroup's two [T, T] squares of `sq` (global scratch: the four slices already take
// 133 KB of the CU's 160 KB at the largest shape).  Behind the workgroup's barrier, phase 2: thread (j, d) owns dK_j[d] and
// dV_j[d] and sums over i in ascending order:
//   dK_j[d] = (sum_i dS_ij Q_i[d]) / sqrt(dh)      dV_j[d] = sum_i pt_ij dO_i[d]
// No atomics.  A query row whose keys are all dropped has pt = 0, r = 0 and dS = 0: a zero dQ row, nothing added to dK, dV.
// The dot products are explicit fmaf chains: the two instantiations of a DH compute the same bits where the masks are all
// ones at scale 1.
// BIAS (k_bert_attention_bwd_bias, MPNet): the head's row of rel_bias [heads, 2T-1] sits in LDS behind dO (2T floats
// reserved) and the score of (t, j) is (q . k) scale + bias[j - t + T - 1], added in blocks of their own behind
// bert_att_opaque as k_bert_attention<DH, true> adds it: an all-zero table gives the bits of the kernel without a bias,
// and without BIAS rel_bias is not read and the LDS layout is the one above.  The bias's own gradient is the sum of the
// dS squares along their diagonals: k_bert_rel_bias_reduce.
template <int DH, bool DROP>
__global__ __launch_bounds__(GNNRAG_BERT_ATT_BWD_THREADS) void k_bert_attention_bwd(
    const float* __restrict__ qkv, const float* __restrict__ dctx, int T, int heads, const uint8_t* __restrict__ keep,
    float keep_scale, float* __restrict__ dqkv, float* sq) {
  constexpr bool BIAS = false;
  const float* rel_bias = nullptr;
#include "bert_attention_bwd_body.h"
}

template <int DH, bool DROP>
__global__ __launch_bounds__(GNNRAG_BERT_ATT_BWD_THREADS) void k_bert_attention_bwd_bias(
    const float* __restrict__ qkv, const float* __restrict__ rel_bias, const float* __restrict__ dctx, int T, int heads,
    const uint8_t* __restrict__ keep, float keep_scale, float* __restrict__ dqkv, float* sq) {
  constexpr bool BIAS = true;
#include "bert_attention_bwd_body.h"
}

// d_bias[h][d + T - 1] (+)= sum_b sum_{i, j = i + d} dS[b, h, i, j] from the squares k_bert_attention_bwd left in `sq`
// ([B heads, 2, T, T]: the dS square of every pair first).  One thread owns an entry and adds b ascending, then i
// ascending; add != 0: the entry's present value comes first (the layers share one table: their sums are added in the
// order the backward visits them).
__global__ __launch_bounds__(256) void k_bert_rel_bias_reduce(const float* __restrict__ sq, int B, int T, int heads,
                                                              int add, float* d_bias) {
  const int W = 2 * T - 1;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= heads * W) return;
  const int h = idx / W, d = idx % W - (T - 1);
  const int i0 = d < 0 ? -d : 0, i1 = d < 0 ? T : T - d;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* s = sq + ((size_t)b * heads + h) * 2 * T * T + d;
    for (int i = i0; i < i1; ++i) acc += s[i * (T + 1)];
  }
  d_bias[idx] = add ? d_bias[idx] + acc : acc;
}

// dy = g m over n4 float4s (m from the keep bytes): the embedding's dropout sits behind its LayerNorm
__global__ __launch_bounds__(256) void k_bert_mask_mul(const float* __restrict__ g, const uint8_t* __restrict__ keep,
                                                       float scale, size_t n4, float* __restrict__ dy) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
    ((f32x4*)dy)[i] = ((const f32x4*)g)[i] * bert_keep4(((const uint32_t*)keep)[i], scale);
}

// Gradient of an embedding table from dz [M, H]: out[k] = the sum of the rows dz[q] with key(q) == k in ascending q, where
// key(q) is the table row token q names - ids[q] (blockIdx.y == 0, d_word) or pos[q] (blockIdx.y == 1, d_pos) - and no row
// at all for a token whose id lies outside [0, vocab), whose pos lies outside [0, max_pos) (the forward's -1 included) or
// whose key is the table's padding row (word_pad / pos_pad; -1: none).  A wave per (token r, table): 64 rows per ballot,
// it leaves when a row below r has r's key, else it owns table row key(r) and adds the matching rows of r .. M - 1, lanes
// over the float4s of a row.  No atomics; the rows nobody owns keep the zeros the host's fill gave them.
__global__ __launch_bounds__(64 * kBertLnRows) void k_bert_embed_scatter(const int64_t* __restrict__ ids,
                                                                         const int32_t* __restrict__ pos,
                                                                         const float* __restrict__ dz, int M, int H4,
                                                                         int vocab, int max_pos, int word_pad, int pos_pad,
                                                                         float* __restrict__ d_word,
                                                                         float* __restrict__ d_pos) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * kBertLnRows + (threadIdx.x >> 6);
  if (r >= M) return;
  const bool word = blockIdx.y == 0;
  float* out = word ? d_word : d_pos;
  if (!out) return;
  const int pad = word ? word_pad : pos_pad;
  auto key = [&](int q) -> int {
    const int64_t id = ids[q];
    const int p = pos[q];
    if (id < 0 || id >= (int64_t)vocab || p < 0 || p >= max_pos) return -1;
    const int k = word ? (int)id : p;
    return k == pad ? -1 : k;
  };
  const int mine = key(r);
  if (mine < 0) return;
  for (int base = 0; base < r; base += 64) {
    const int q = base + lane;
    if (__ballot(q < r && key(q) == mine)) return;
  }
  f32x4* dst = (f32x4*)(out + (size_t)mine * H4 * 4);
  for (int c0 = 0; c0 < H4; c0 += 64) {
    const int c = c0 + lane;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int base = r & ~63; base < M; base += 64) {
      const int q = base + lane;
      unsigned long long hits = __ballot(q >= r && q < M && key(q) == mine);
      while (hits) {
        const int q1 = base + __builtin_ctzll(hits);
        hits &= hits - 1;
        if (c < H4) acc = acc + ((const f32x4*)(dz + (size_t)q1 * H4 * 4))[c];
      }
    }
    if (c < H4) dst[c] = acc;
  }
}

static inline size_t bert_att_bwd_lds_bytes(int T, int dh, int threads, bool bias = false) {
  return ((size_t)4 * T * (dh + 1) + (bias ? (size_t)2 * T : 0) + (size_t)(threads / 64) * kBertMaxT) * sizeof(float);
}

static inline size_t bert_att_bwd_scratch_bytes(int64_t B, int32_t T, int32_t heads) {
  return (size_t)B * heads * 2 * T * T * sizeof(float);
}

template <int DH, bool DROP>
static int bert_attention_bwd_launch_as(const float* qkv, const float* dctx, const uint8_t* keep, float keep_scale,
                                        int32_t B, int32_t T, int32_t heads, float* dqkv, float* sq, hipStream_t stream) {
  const int threads = GNNRAG_BERT_ATT_BWD_THREADS;
  const size_t lds = bert_att_bwd_lds_bytes(T, DH, threads);
  if (lds > 64 * 1024) {
    static DeviceMask raised{0};
    GNNRAG_RC(raise_lds_cap(k_bert_attention_bwd<DH, DROP>, raised));
  }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bert_attention_bwd<DH, DROP>), dim3((unsigned)((int64_t)B * heads)), dim3(threads),
                     lds, stream, qkv, dctx, T, heads, keep, keep_scale, dqkv, sq);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

template <int DH, bool DROP>
static int bert_attention_bwd_bias_launch_as(const float* qkv, const float* rel_bias, const float* dctx,
                                             const uint8_t* keep, float keep_scale, int32_t B, int32_t T, int32_t heads,
                                             float* dqkv, float* sq, hipStream_t stream) {
  const int threads = GNNRAG_BERT_ATT_BWD_THREADS;
  const size_t lds = bert_att_bwd_lds_bytes(T, DH, threads, true);
  if (lds > 64 * 1024) {
    static DeviceMask raised{0};
    GNNRAG_RC(raise_lds_cap(k_bert_attention_bwd_bias<DH, DROP>, raised));
  }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bert_attention_bwd_bias<DH, DROP>), dim3((unsigned)((int64_t)B * heads)),
                     dim3(threads), lds, stream, qkv, rel_bias, dctx, T, heads, keep, keep_scale, dqkv, sq);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

// keep NULL: no dropout (the kernel never sees a NULL pointer's argument); rel_bias NULL: the kernels without a bias
static int bert_attention_bwd_launch(const float* qkv, const float* dctx, const uint8_t* keep, float keep_scale, int32_t B,
                                     int32_t T, int32_t heads, int32_t dh, float* dqkv, float* sq, hipStream_t stream,
                                     const float* rel_bias = nullptr) {
  if (rel_bias) {
    if (dh == 32)
      return keep ? bert_attention_bwd_bias_launch_as<32, true>(qkv, rel_bias, dctx, keep, keep_scale, B, T, heads, dqkv, sq,
                                                                stream)
                  : bert_attention_bwd_bias_launch_as<32, false>(qkv, rel_bias, dctx, nullptr, 0.f, B, T, heads, dqkv, sq,
                                                                 stream);
    return keep ? bert_attention_bwd_bias_launch_as<64, true>(qkv, rel_bias, dctx, keep, keep_scale, B, T, heads, dqkv, sq,
                                                              stream)
                : bert_attention_bwd_bias_launch_as<64, false>(qkv, rel_bias, dctx, nullptr, 0.f, B, T, heads, dqkv, sq,
                                                               stream);
  }
  if (dh == 32)
    return keep ? bert_attention_bwd_launch_as<32, true>(qkv, dctx, keep, keep_scale, B, T, heads, dqkv, sq, stream)
                : bert_attention_bwd_launch_as<32, false>(qkv, dctx, nullptr, 0.f, B, T, heads, dqkv, sq, stream);
  return keep ? bert_attention_bwd_launch_as<64, true>(qkv, dctx, keep, keep_scale, B, T, heads, dqkv, sq, stream)
              : bert_attention_bwd_launch_as<64, false>(qkv, dctx, nullptr, 0.f, B, T, heads, dqkv, sq, stream);
}

// keep NULL: z = d, dY is not written (the gradient of the dense output is dz)
static int bert_ln_bwd_launch(const float* dy, const float* d, const uint8_t* keep, float scale, const float* res,
                              const float* g, float eps, int64_t M, int32_t H, float* dz, float* dY, float* summ,
                              hipStream_t stream) {
  const dim3 grid((unsigned)((M + kBertLnRows - 1) / kBertLnRows)), block(64 * kBertLnRows);
  if (keep)
    hipLaunchKernelGGL(k_bert_ln_bwd<true>, grid, block, 0, stream, dy, d, keep, scale, res, g, eps, (int)M, H / 4, dz, dY,
                       summ);
  else
    hipLaunchKernelGGL(k_bert_ln_bwd<false>, grid, block, 0, stream, dy, d, (const uint8_t*)nullptr, 0.f,
                       (const float*)nullptr, g, eps, (int)M, H / 4, dz, (float*)nullptr, summ);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

static int bert_gelu_bwd_launch(const float* pre, const float* d_act, float* d_pre, float* act, size_t n,
                                hipStream_t stream) {
  const size_t blocks = (n / 4 + 255) / 256;
  const dim3 grid((unsigned)(blocks < 1 ? 1 : blocks > 65536 ? 65536 : blocks));
  if (act) hipLaunchKernelGGL(k_bert_gelu_bwd<true>, grid, dim3(256), 0, stream, pre, d_act, d_pre, act, n);
  else hipLaunchKernelGGL(k_bert_gelu_bwd<false>, grid, dim3(256), 0, stream, pre, d_act, d_pre, (float*)nullptr, n);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

// column sums of up to two [M, cols] blocks in one launch
static int bert_colsum2(const float* s0, float* d0, const float* s1, float* d1, int64_t M, int32_t ld, int32_t cols,
                        hipStream_t stream) {
  ColsumJobs jobs;
  memset(&jobs, 0, sizeof(jobs));
  int n = 0;
  if (d0) { jobs.src[n] = s0; jobs.dst[n] = d0; jobs.rows[n] = M; jobs.ld[n] = ld; ++n; }
  if (d1) { jobs.src[n] = s1; jobs.dst[n] = d1; jobs.rows[n] = M; jobs.ld[n] = ld; ++n; }
  if (!n) return 0;
  jobs.cols = cols;
  return colsum_launch(jobs, n, stream);
}

// the workspace of gnnrag_bert_layers_backward, each block on a 256-byte boundary:
//   g0, g1 [M, H]   the gradient of a layer's output (two buffers in turn)
//   dz, dY, summ, dx1, dctx [M, H]
//   dact, act [M, I];  dqkv [M, 3H]
//   wt     max(3 H H, H I) floats: the transposed copy of the weight of the running product
//   att    [B heads, 2, T, T]: the squares of k_bert_attention_bwd
//   tn     the largest gnnrag_gemm_tn_workspace_bytes of the four weight gradients
struct BertBwdWs {
  size_t g0, g1, dz, dY, summ, dx1, dctx, dact, act, dqkv, wt, att, tn, tn_bytes, total;
};

static inline BertBwdWs bert_bwd_ws(int64_t B, int32_t T, int32_t H, int32_t heads, int32_t I) {
  BertBwdWs w;
  const int64_t M = B * T;
  const size_t mh = (size_t)M * H * sizeof(float), mi = (size_t)M * I * sizeof(float);
  Carve cv;
  w.g0 = cv.take(mh);
  w.g1 = cv.take(mh);
  w.dz = cv.take(mh);
  w.dY = cv.take(mh);
  w.summ = cv.take(mh);
  w.dx1 = cv.take(mh);
  w.dctx = cv.take(mh);
  w.dact = cv.take(mi);
  w.act = cv.take(mi);
  w.dqkv = cv.take(3 * mh);
  w.wt = cv.take((size_t)H * (3 * (size_t)H > (size_t)I ? 3 * (size_t)H : (size_t)I) * sizeof(float));
  w.att = cv.take(bert_att_bwd_scratch_bytes(B, T, heads));
  const size_t t[4] = {gnnrag_gemm_tn_workspace_bytes(M, H, I), gnnrag_gemm_tn_workspace_bytes(M, I, H),
                       gnnrag_gemm_tn_workspace_bytes(M, H, H), gnnrag_gemm_tn_workspace_bytes(M, 3 * H, H)};
  w.tn_bytes = 0;
  for (int i = 0; i < 4; ++i)
    if (t[i] > w.tn_bytes) w.tn_bytes = t[i];
  w.tn = cv.take(w.tn_bytes);
  w.total = cv.off;
  return w;
}

static int bert_rel_bias_reduce_launch(const float* sq, int32_t B, int32_t T, int32_t heads, bool add, float* d_bias,
                                       hipStream_t stream) {
  const int n = heads * (2 * T - 1);
  hipLaunchKernelGGL(k_bert_rel_bias_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sq, B, T, heads,
                     add ? 1 : 0, d_bias);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

// the workspace of gnnrag_bert_embed_backward, each block on a 256-byte boundary: dz, summ, dy [M, H]
struct BertEmbedBwdWs {
  size_t dz, summ, dy, total;
};

static inline BertEmbedBwdWs bert_embed_bwd_ws(int64_t M, int32_t H) {
  BertEmbedBwdWs w;
  const size_t mh = (size_t)M * H * sizeof(float);
  Carve cv;
  w.dz = cv.take(mh);
  w.summ = cv.take(mh);
  w.dy = cv.take(mh);
  w.total = cv.off;
  return w;
}

// the fill of the two tables (a NULL one is not wanted) and k_bert_embed_scatter on them
static int bert_embed_scatter_launch(const int64_t* ids, const int32_t* pos, const float* dz, int64_t M, int32_t H,
                                     int32_t vocab, int32_t max_pos, int32_t word_pad, int32_t pos_pad, float* d_word,
                                     float* d_pos, hipStream_t st) {
  if (d_word) GNNRAG_HIP(hipMemsetAsync(d_word, 0, (size_t)vocab * H * sizeof(float), st));
  if (d_pos) GNNRAG_HIP(hipMemsetAsync(d_pos, 0, (size_t)max_pos * H * sizeof(float), st));
  if (!d_word && !d_pos) return 0;
  hipLaunchKernelGGL(k_bert_embed_scatter, dim3((unsigned)((M + kBertLnRows - 1) / kBertLnRows), 2), dim3(64 * kBertLnRows),
                     0, st, ids, pos, dz, (int)M, H / 4, vocab, max_pos, word_pad, pos_pad, d_word, d_pos);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

static inline bool bert_embed_bwd_shape_ok(int32_t B, int32_t T, int32_t H) {
  return !(H & 3) && (int64_t)B * T <= kBertEmbedBwdMaxRows;
}

static inline bool bert_bwd_shape_ok(int32_t B, int32_t T, int32_t H, int32_t heads, int32_t I) {
  if (H % heads != 0 || (H & 3) || (I & 3) || (int64_t)3 * H > INT32_MAX) return false;
  return bert_att_shape_ok(B, T, heads, H / heads) && (int64_t)B * T < ((int64_t)1 << 31);
}

}  // namespace gnnrag

using namespace gnnrag;

extern "C" size_t gnnrag_bert_attention_backward_workspace_bytes(int32_t B, int32_t T, int32_t heads) {
  if (B <= 0 || T <= 0 || heads <= 0) return 0;
  return bert_att_bwd_scratch_bytes(B, T, heads);
}

extern "C" int gnnrag_bert_attention_backward_bias(const float* qkv, const float* d_ctx, int32_t B, int32_t T,
                                                   int32_t heads, int32_t dh, const float* rel_bias, const uint8_t* keep,
                                                   float scale, float* d_qkv, void* ws, size_t ws_bytes,
                                                   gnnrag_stream_t stream) {
  if (B <= 0 || T <= 0 || heads <= 0 || dh <= 0) return GNNRAG_E_BADARG;
  if (!bert_att_shape_ok(B, T, heads, dh)) return GNNRAG_E_UNSUPPORTED;
  if (!qkv || !d_ctx || !d_qkv || !ws || !bert_scale_ok(keep, scale)) return GNNRAG_E_BADARG;
  if (!aligned16(qkv, d_ctx, d_qkv, ws, rel_bias)) return GNNRAG_E_UNSUPPORTED;
  if (ws_bytes < bert_att_bwd_scratch_bytes(B, T, heads)) return GNNRAG_E_WORKSPACE;
  return bert_attention_bwd_launch(qkv, d_ctx, keep, scale, B, T, heads, dh, d_qkv, (float*)ws, (hipStream_t)stream,
                                   rel_bias);
}

extern "C" int gnnrag_bert_attention_backward(const float* qkv, const float* d_ctx, int32_t B, int32_t T, int32_t heads,
                                              int32_t dh, const uint8_t* keep, float scale, float* d_qkv, void* ws,
                                              size_t ws_bytes, gnnrag_stream_t stream) {
  return gnnrag_bert_attention_backward_bias(qkv, d_ctx, B, T, heads, dh, nullptr, keep, scale, d_qkv, ws, ws_bytes, stream);
}

extern "C" int gnnrag_bert_rel_bias_reduce(const float* sq, int32_t B, int32_t T, int32_t heads, float* d_bias,
                                           gnnrag_stream_t stream) {
  if (B <= 0 || T <= 0 || heads <= 0) return GNNRAG_E_BADARG;
  if (!bert_att_shape_ok(B, T, heads, 32)) return GNNRAG_E_UNSUPPORTED;
  if (!sq || !d_bias) return GNNRAG_E_BADARG;
  if (!aligned16(sq, d_bias)) return GNNRAG_E_UNSUPPORTED;
  return bert_rel_bias_reduce_launch(sq, B, T, heads, false, d_bias, (hipStream_t)stream);
}

extern "C" size_t gnnrag_bert_embed_backward_workspace_bytes(int32_t B, int32_t T, int32_t H) {
  if (B <= 0 || T <= 0 || H <= 0 || !bert_embed_bwd_shape_ok(B, T, H)) return 0;
  return bert_embed_bwd_ws((int64_t)B * T, H).total;
}

// Backward of gnnrag_bert_embed_forward_save: dy = g_x0 m (k_bert_mask_mul; keep NULL: g_x0 itself), the LayerNorm
// backward on the saved rows (k_bert_ln_bwd without a mask: the dropout sits behind this LayerNorm), the column sums,
// then the tables: one fill and k_bert_embed_scatter for d_word / d_pos, the column sum of dz for row 0 of d_type.
extern "C" int gnnrag_bert_embed_backward(const float* g_x0, const int64_t* ids, const void* reserve, size_t reserve_bytes,
                                          int32_t B, int32_t T, int32_t H, int32_t vocab, int32_t max_pos, int32_t n_type,
                                          int32_t word_pad, int32_t pos_pad, const uint8_t* keep, float scale,
                                          const float* ln_g, float ln_eps, float* d_word, float* d_pos, float* d_type,
                                          float* d_ln_g, float* d_ln_b, void* ws, size_t ws_bytes,
                                          gnnrag_stream_t stream) {
  if (B <= 0 || T <= 0 || H <= 0 || vocab <= 0 || max_pos <= 0 || (d_type && n_type <= 0)) return GNNRAG_E_BADARG;
  if (!bert_embed_bwd_shape_ok(B, T, H)) return GNNRAG_E_UNSUPPORTED;
  if (!g_x0 || !ids || !reserve || !ln_g || !ws || !bert_scale_ok(keep, scale)) return GNNRAG_E_BADARG;
  if (!aligned16(g_x0, reserve, ln_g, d_word, d_pos, d_type, d_ln_g, d_ln_b, ws) || ((uintptr_t)ids & 7) ||
      ((uintptr_t)keep & 3))
    return GNNRAG_E_UNSUPPORTED;
  const int64_t M = (int64_t)B * T;
  const BertEmbedReserve r = bert_embed_reserve(M, H);
  const BertEmbedBwdWs w = bert_embed_bwd_ws(M, H);
  if (reserve_bytes < r.total || ws_bytes < w.total) return GNNRAG_E_WORKSPACE;

  hipStream_t st = (hipStream_t)stream;
  const float* sum0 = (const float*)((const char*)reserve + r.sum0);
  const int32_t* pos = (const int32_t*)((const char*)reserve + r.pos);
  float* dz = (float*)((char*)ws + w.dz);
  float* summ = (float*)((char*)ws + w.summ);
  const float* dy = g_x0;
  if (keep) {
    float* dyb = (float*)((char*)ws + w.dy);
    const size_t n4 = (size_t)M * H / 4, blocks = (n4 + 255) / 256;
    hipLaunchKernelGGL(k_bert_mask_mul, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, st, g_x0, keep,
                       scale, n4, dyb);
    GNNRAG_LAUNCH_CHECK();
    dy = dyb;
  }
  GNNRAG_RC(bert_ln_bwd_launch(dy, sum0, nullptr, 0.f, nullptr, ln_g, ln_eps, M, H, dz, nullptr, summ, st));
  GNNRAG_RC(bert_colsum2(summ, d_ln_g, dy, d_ln_b, M, H, H, st));
  if (d_type) {
    GNNRAG_RC(bert_colsum2(dz, d_type, nullptr, nullptr, M, H, H, st));
    if (n_type > 1) GNNRAG_HIP(hipMemsetAsync(d_type + H, 0, (size_t)(n_type - 1) * H * sizeof(float), st));
  }
  return bert_embed_scatter_launch(ids, pos, dz, M, H, vocab, max_pos, word_pad, pos_pad, d_word, d_pos, st);
}

extern "C" int gnnrag_bert_embed_scatter(const float* dz, const int64_t* ids, const int32_t* pos, int64_t M, int32_t H,
                                         int32_t vocab, int32_t max_pos, int32_t word_pad, int32_t pos_pad, float* d_word,
                                         float* d_pos, gnnrag_stream_t stream) {
  if (M <= 0 || H <= 0 || vocab <= 0 || max_pos <= 0) return GNNRAG_E_BADARG;
  if ((H & 3) || M > kBertEmbedBwdMaxRows) return GNNRAG_E_UNSUPPORTED;
  if (!dz || !ids || !pos) return GNNRAG_E_BADARG;
  if (!aligned16(dz, d_word, d_pos) || ((uintptr_t)ids & 7) || ((uintptr_t)pos & 3)) return GNNRAG_E_UNSUPPORTED;
  return bert_embed_scatter_launch(ids, pos, dz, M, H, vocab, max_pos, word_pad, pos_pad, d_word, d_pos,
                                   (hipStream_t)stream);
}

extern "C" int gnnrag_bert_ln_backward(const float* dy, const float* d, const uint8_t* keep, float scale, const float* res,
                                       const float* g, float eps, int64_t M, int32_t H, float* dz, float* dY, float* summ,
                                       float* dgamma, float* dbeta, gnnrag_stream_t stream) {
  if (M <= 0 || H <= 0) return GNNRAG_E_BADARG;
  if ((H & 3) || M >= ((int64_t)1 << 31)) return GNNRAG_E_UNSUPPORTED;
  if (!dy || !d || !g || !dz || !summ || (keep && (!res || !dY)) || !bert_scale_ok(keep, scale))
    return GNNRAG_E_BADARG;
  if (!aligned16(dy, d, res, g, dz, dY, summ) || ((uintptr_t)keep & 3)) return GNNRAG_E_UNSUPPORTED;
  GNNRAG_RC(bert_ln_bwd_launch(dy, d, keep, scale, res, g, eps, M, H, dz, dY, summ, (hipStream_t)stream));
  return bert_colsum2(summ, dgamma, dy, dbeta, M, H, H, (hipStream_t)stream);
}

extern "C" int gnnrag_bert_gelu_backward(const float* pre, const float* d_act, int64_t n, float* d_pre, float* act,
                                         gnnrag_stream_t stream) {
  if (n <= 0 || !pre || !d_act || !d_pre) return GNNRAG_E_BADARG;
  if (!aligned16(pre, d_act, d_pre, act)) return GNNRAG_E_UNSUPPORTED;
  return bert_gelu_bwd_launch(pre, d_act, d_pre, act, (size_t)n, (hipStream_t)stream);
}

extern "C" size_t gnnrag_bert_layers_backward_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t heads, int32_t I) {
  if (B <= 0 || T <= 0 || H <= 0 || heads <= 0 || I <= 0 || !bert_bwd_shape_ok(B, T, H, heads, I)) return 0;
  return bert_bwd_ws(B, T, H, heads, I).total;
}

extern "C" int gnnrag_bert_layers_backward(const float* g_out, int32_t L, const gnnrag_bert_layer* layers, float ln_eps,
                                           int32_t B, int32_t T, int32_t H, int32_t heads, int32_t I,
                                           const uint8_t* keep_hidden, float scale_hidden, const uint8_t* keep_att,
                                           float scale_att, const void* reserve, size_t reserve_bytes, float* g_x0,
                                           const gnnrag_bert_layer_grads* grads, void* ws, size_t ws_bytes,
                                           gnnrag_stream_t stream_) {
  return gnnrag_bert_layers_backward_ex(g_out, L, layers, nullptr, ln_eps, B, T, H, heads, I, keep_hidden, scale_hidden,
                                        keep_att, scale_att, reserve, reserve_bytes, g_x0, grads, nullptr, ws, ws_bytes,
                                        stream_);
}

// rel_bias NULL: the launches of gnnrag_bert_layers_backward.  With it the attention step is k_bert_attention_bwd_bias and,
// d_rel_bias given, k_bert_rel_bias_reduce follows it on the same squares: layer L-1 writes the table, the others add.
extern "C" int gnnrag_bert_layers_backward_ex(const float* g_out, int32_t L, const gnnrag_bert_layer* layers,
                                              const float* rel_bias, float ln_eps, int32_t B, int32_t T, int32_t H,
                                              int32_t heads, int32_t I, const uint8_t* keep_hidden, float scale_hidden,
                                              const uint8_t* keep_att, float scale_att, const void* reserve,
                                              size_t reserve_bytes, float* g_x0, const gnnrag_bert_layer_grads* grads,
                                              float* d_rel_bias, void* ws, size_t ws_bytes, gnnrag_stream_t stream_) {
  if (B <= 0 || T <= 0 || H <= 0 || heads <= 0 || I <= 0 || L <= 0) return GNNRAG_E_BADARG;
  if (!bert_bwd_shape_ok(B, T, H, heads, I)) return GNNRAG_E_UNSUPPORTED;
  if (!g_out || !layers || !reserve || !ws || (d_rel_bias && !rel_bias)) return GNNRAG_E_BADARG;
  if (!bert_scale_ok(keep_hidden, scale_hidden) || !bert_scale_ok(keep_att, scale_att)) return GNNRAG_E_BADARG;
  if (!aligned16(g_out, reserve, g_x0, ws, rel_bias, d_rel_bias) || ((uintptr_t)keep_hidden & 3))
    return GNNRAG_E_UNSUPPORTED;
  for (int l = 0; l < L; ++l) {
    GNNRAG_RC(bert_layer_ptrs_check(layers[l], kBertFieldsBwd));      // the biases are not read: NULL is legal
    if (grads) {
      const gnnrag_bert_layer_grads& o = grads[l];
      if (!aligned16(o.dW_qkv, o.db_qkv, o.dW_o, o.db_o, o.dW_i, o.db_i, o.dW_f, o.db_f)) return GNNRAG_E_UNSUPPORTED;
    }
  }
  const int64_t M = (int64_t)B * T;
  const BertReserve r = bert_reserve(M, H, I);
  const BertBwdWs w = bert_bwd_ws(B, T, H, heads, I);
  if (reserve_bytes < (size_t)L * r.layer || ws_bytes < w.total) return GNNRAG_E_WORKSPACE;

  hipStream_t st = (hipStream_t)stream_;
  char* wsb = (char*)ws;
  float* gbuf[2] = {(float*)(wsb + w.g0), (float*)(wsb + w.g1)};
  float* dz = (float*)(wsb + w.dz);
  float* dYb = (float*)(wsb + w.dY);
  float* summ = (float*)(wsb + w.summ);
  float* dx1 = (float*)(wsb + w.dx1);
  float* dctx = (float*)(wsb + w.dctx);
  float* dact = (float*)(wsb + w.dact);
  float* act = (float*)(wsb + w.act);
  float* dqkv = (float*)(wsb + w.dqkv);
  float* wt = (float*)(wsb + w.wt);
  float* att = (float*)(wsb + w.att);
  void* tn = wsb + w.tn;
  const int32_t dh = H / heads;
  const BertKeep keep(keep_hidden, keep_att, B, T, H, heads);
  const gnnrag_bert_layer_grads none{};
  const float* g = g_out;
  for (int l = L - 1; l >= 0; --l) {
    const gnnrag_bert_layer& p = layers[l];
    const gnnrag_bert_layer_grads& o = grads ? grads[l] : none;
    const char* rl = (const char*)reserve + (size_t)l * r.layer;
    const float* xin = (const float*)(rl + r.xin);
    const float* qkv = (const float*)(rl + r.qkv);
    const float* ctx = (const float*)(rl + r.ctx);
    const float* sum1 = (const float*)(rl + r.sum1);
    const float* x1 = (const float*)(rl + r.x1);
    const float* pre = (const float*)(rl + r.pre);
    const float* sum2 = (const float*)(rl + r.sum2);
    const uint8_t *k1 = keep.att_out(l), *k2 = keep.ffn_out(l);
    const float* dY = keep_hidden ? dYb : dz;     // the gradient of a dense output in front of a LayerNorm

    // LayerNorm 2 and the FFN
    GNNRAG_RC(bert_ln_bwd_launch(g, sum2, k2, scale_hidden, x1, p.ln2_g, ln_eps, M, H, dz, dYb, summ, st));
    GNNRAG_RC(bert_colsum2(summ, o.dln2_g, g, o.dln2_b, M, H, H, st));
    GNNRAG_RC(transpose_launch(p.W_f, wt, H, I, st));
    GNNRAG_RC(gnnrag_linear(dY, M, H, wt, nullptr, nullptr, 0, 0, dact, I, GNNRAG_MATH_FP32, stream_));
    GNNRAG_RC(bert_gelu_bwd_launch(pre, dact, dact, o.dW_f ? act : nullptr, (size_t)M * I, st));
    if (o.dW_f) GNNRAG_RC(gnnrag_gemm_tn(dY, act, M, H, I, o.dW_f, tn, w.tn_bytes, stream_));
    GNNRAG_RC(bert_colsum2(dY, o.db_f, nullptr, nullptr, M, H, H, st));
    if (o.dW_i) GNNRAG_RC(gnnrag_gemm_tn(dact, x1, M, I, H, o.dW_i, tn, w.tn_bytes, stream_));
    GNNRAG_RC(bert_colsum2(dact, o.db_i, nullptr, nullptr, M, I, I, st));
    GNNRAG_RC(transpose_launch(p.W_i, wt, I, H, st));
    GNNRAG_RC(gnnrag_linear(dact, M, I, wt, nullptr, dz, M, 0, dx1, H, GNNRAG_MATH_FP32, stream_));

    // LayerNorm 1 and the attention block
    GNNRAG_RC(bert_ln_bwd_launch(dx1, sum1, k1, scale_hidden, xin, p.ln1_g, ln_eps, M, H, dz, dYb, summ, st));
    GNNRAG_RC(bert_colsum2(summ, o.dln1_g, dx1, o.dln1_b, M, H, H, st));
    if (o.dW_o) GNNRAG_RC(gnnrag_gemm_tn(dY, ctx, M, H, H, o.dW_o, tn, w.tn_bytes, stream_));
    GNNRAG_RC(bert_colsum2(dY, o.db_o, nullptr, nullptr, M, H, H, st));
    GNNRAG_RC(transpose_launch(p.W_o, wt, H, H, st));
    GNNRAG_RC(gnnrag_linear(dY, M, H, wt, nullptr, nullptr, 0, 0, dctx, H, GNNRAG_MATH_FP32, stream_));
    GNNRAG_RC(bert_attention_bwd_launch(qkv, dctx, keep.probs(l), scale_att, B, T, heads, dh, dqkv, att, st, rel_bias));
    if (d_rel_bias) GNNRAG_RC(bert_rel_bias_reduce_launch(att, B, T, heads, l != L - 1, d_rel_bias, st));
    if (o.dW_qkv) GNNRAG_RC(gnnrag_gemm_tn(dqkv, xin, M, 3 * H, H, o.dW_qkv, tn, w.tn_bytes, stream_));
    if (o.db_qkv) {
      // the query and value thirds; the key third is exactly +0
      ColsumJobs jobs;
      memset(&jobs, 0, sizeof(jobs));
      jobs.src[0] = dqkv; jobs.dst[0] = o.db_qkv; jobs.rows[0] = M; jobs.ld[0] = 3 * H;
      jobs.src[1] = dqkv + 2 * H; jobs.dst[1] = o.db_qkv + 2 * H; jobs.rows[1] = M; jobs.ld[1] = 3 * H;
      jobs.cols = H;
      GNNRAG_RC(colsum_launch(jobs, 2, st));
      GNNRAG_HIP(hipMemsetAsync(o.db_qkv + H, 0, (size_t)H * sizeof(float), st));
    }
    float* gx = l > 0 ? gbuf[l & 1] : g_x0;
    if (gx) {
      GNNRAG_RC(transpose_launch(p.W_qkv, wt, 3 * H, H, st));
      GNNRAG_RC(gnnrag_linear(dqkv, M, 3 * H, wt, nullptr, dz, M, 0, gx, H, GNNRAG_MATH_FP32, stream_));
    }
    g = gx;
  }
  return 0;
}
