// Backward of the encoder layers of a BERT-class question encoder (bert_encoder.hip, gnnrag_bert_layers_forward_save):
// what fine-tuning the LM (the reference's --lm_frozen 0, gnn/modules/question_encoding/bert_encoder.py:80-87) derives
// for transformers' BertModel / RobertaModel layers.  The embedding stage stays outside (its gradient is g_x0).
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
template <int DH, bool DROP>
__global__ __launch_bounds__(GNNRAG_BERT_ATT_BWD_THREADS) void k_bert_attention_bwd(
    const float* __restrict__ qkv, const float* __restrict__ dctx, int T, int heads, const uint8_t* __restrict__ keep,
    float keep_scale, float* __restrict__ dqkv, float* sq) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LD = DH + 1;
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int H = heads * DH;
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  float* ks = smem;                                   // [T, LD]
  float* vs = ks + T * LD;                            // [T, LD]
  float* qs = vs + T * LD;                            // [T, LD]
  float* gs = qs + T * LD;                            // [T, LD]  dO
  float* ds = gs + T * LD + wave * kBertMaxT;         // [kBertMaxT]  this wave's row of dS
  float* dsg = sq + (size_t)blockIdx.x * 2 * T * T;   // [T, T]  dS, query row i, key column j
  float* ptg = dsg + (size_t)T * T;                   // [T, T]  pt

  const float* base = qkv + (size_t)b * T * 3 * H + h * DH;
  const float* gbase = dctx + (size_t)b * T * H + h * DH;
  float* obase = dqkv + (size_t)b * T * 3 * H + h * DH;
  for (int i = tid; i < T * (DH / 4); i += nthr) {
    const int j = i / (DH / 4), c = (i % (DH / 4)) * 4;
    const float* row = base + (size_t)j * 3 * H;
    const f32x4 qv = *(const f32x4*)(row + c);
    const f32x4 kv = *(const f32x4*)(row + H + c);
    const f32x4 vv = *(const f32x4*)(row + 2 * H + c);
    const f32x4 gv = *(const f32x4*)(gbase + (size_t)j * H + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qs[j * LD + c + e] = qv[e];
      ks[j * LD + c + e] = kv[e];
      vs[j * LD + c + e] = vv[e];
      gs[j * LD + c + e] = gv[e];
    }
  }
  __syncthreads();

  const float scale = 1.f / sqrtf((float)DH);
  const int j0 = lane, j1 = lane + 64;
  for (int t = wave; t < T; t += nw) {
    const float* q = qs + t * LD;
    const float* go = gs + t * LD;
    float s0 = -INFINITY, s1 = -INFINITY, dp0 = 0.f, dp1 = 0.f;
    if (j0 < T) {
      const float *k = ks + j0 * LD, *v = vs + j0 * LD;
      float a = 0.f, c = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) {
        a = fmaf(q[d], k[d], a);
        c = fmaf(go[d], v[d], c);
      }
      s0 = a * scale;
      dp0 = c;
    }
    if (j1 < T) {
      const float *k = ks + j1 * LD, *v = vs + j1 * LD;
      float a = 0.f, c = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) {
        a = fmaf(q[d], k[d], a);
        c = fmaf(go[d], v[d], c);
      }
      s1 = a * scale;
      dp1 = c;
    }
    const float m = wave_max(fmaxf(s0, s1));
    const float e0 = j0 < T ? expf(s0 - m) : 0.f, e1 = j1 < T ? expf(s1 - m) : 0.f;
    const float sum = wave_sum(e0 + e1);
    const float p0 = e0 / sum, p1 = e1 / sum;
    float m0 = 1.f, m1 = 1.f;
    if (DROP) {
      const uint8_t* kr = keep + ((size_t)blockIdx.x * T + t) * T;     // blockIdx.x = b heads + h
      m0 = j0 < T && kr[j0] ? keep_scale : 0.f;
      m1 = j1 < T && kr[j1] ? keep_scale : 0.f;
    }
    const float pt0 = DROP ? p0 * m0 : p0, pt1 = DROP ? p1 * m1 : p1;
    const float r = wave_sum(fmaf(pt0, dp0, pt1 * dp1));
    // the masked product is rounded on its own (behind bert_att_opaque it cannot be fused into the subtraction): with
    // one key p = 1, r is that same rounded product and dS is exactly 0, as it is in exact arithmetic
    const float dS0 = p0 * ((DROP ? bert_att_opaque(dp0 * m0) : dp0) - r);
    const float dS1 = p1 * ((DROP ? bert_att_opaque(dp1 * m1) : dp1) - r);
    if (j0 < T) {
      ds[j0] = dS0;
      dsg[t * T + j0] = dS0;
      ptg[t * T + j0] = pt0;
    }
    if (j1 < T) {
      ds[j1] = dS1;
      dsg[t * T + j1] = dS1;
      ptg[t * T + j1] = pt1;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < DH) {
      float acc = 0.f;
      for (int j = 0; j < T; ++j) acc = fmaf(ds[j], ks[j * LD + lane], acc);
      obase[(size_t)t * 3 * H + lane] = acc * scale;
    }
    // the next row's writes to ds follow this row's reads in program order (one wave, LDS in order)
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();          // the squares are written by this workgroup and read by it: visible behind the barrier

  for (int idx = tid; idx < T * DH; idx += nthr) {
    const int j = idx / DH, d = idx % DH;
    float ak = 0.f, av = 0.f;
    for (int i = 0; i < T; ++i) {
      ak = fmaf(dsg[i * T + j], qs[i * LD + d], ak);
      av = fmaf(ptg[i * T + j], gs[i * LD + d], av);
    }
    obase[(size_t)j * 3 * H + H + d] = ak * scale;
    obase[(size_t)j * 3 * H + 2 * H + d] = av;
  }
}

static inline size_t bert_att_bwd_lds_bytes(int T, int dh, int threads) {
  return ((size_t)4 * T * (dh + 1) + (size_t)(threads / 64) * kBertMaxT) * sizeof(float);
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

// keep NULL: no dropout (the kernel never sees a NULL pointer's argument)
static int bert_attention_bwd_launch(const float* qkv, const float* dctx, const uint8_t* keep, float keep_scale, int32_t B,
                                     int32_t T, int32_t heads, int32_t dh, float* dqkv, float* sq, hipStream_t stream) {
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

extern "C" int gnnrag_bert_attention_backward(const float* qkv, const float* d_ctx, int32_t B, int32_t T, int32_t heads,
                                              int32_t dh, const uint8_t* keep, float scale, float* d_qkv, void* ws,
                                              size_t ws_bytes, gnnrag_stream_t stream) {
  if (B <= 0 || T <= 0 || heads <= 0 || dh <= 0) return GNNRAG_E_BADARG;
  if (!bert_att_shape_ok(B, T, heads, dh)) return GNNRAG_E_UNSUPPORTED;
  if (!qkv || !d_ctx || !d_qkv || !ws || !bert_scale_ok(keep, scale)) return GNNRAG_E_BADARG;
  if (!aligned16(qkv, d_ctx, d_qkv, ws)) return GNNRAG_E_UNSUPPORTED;
  if (ws_bytes < bert_att_bwd_scratch_bytes(B, T, heads)) return GNNRAG_E_WORKSPACE;
  return bert_attention_bwd_launch(qkv, d_ctx, keep, scale, B, T, heads, dh, d_qkv, (float*)ws, (hipStream_t)stream);
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
  if (B <= 0 || T <= 0 || H <= 0 || heads <= 0 || I <= 0 || L <= 0) return GNNRAG_E_BADARG;
  if (!bert_bwd_shape_ok(B, T, H, heads, I)) return GNNRAG_E_UNSUPPORTED;
  if (!g_out || !layers || !reserve || !ws) return GNNRAG_E_BADARG;
  if (!bert_scale_ok(keep_hidden, scale_hidden) || !bert_scale_ok(keep_att, scale_att)) return GNNRAG_E_BADARG;
  if (!aligned16(g_out, reserve, g_x0, ws) || ((uintptr_t)keep_hidden & 3)) return GNNRAG_E_UNSUPPORTED;
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
    GNNRAG_RC(bert_attention_bwd_launch(qkv, dctx, keep.probs(l), scale_att, B, T, heads, dh, dqkv, att, st));
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
