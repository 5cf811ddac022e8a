// Inference forward of a frozen BERT-class question encoder: what the reference's
// BERTInstruction.encode_question gets from `self.node_encoder(query_text)[0]` (gnn/modules/question_encoding/
// bert_encoder.py:94) - transformers' BertModel on input ids alone: absolute positions, token type 0, NO attention mask
// (pad tokens are attended like any other token), erf GELU, post-LayerNorm residual blocks; the pooler is never read.
//
//   x   = LN(word_emb[id] + pos_emb[t] + type_emb[0])                                   k_bert_embed_ln
//   per layer:
//     qkv = x W_qkv^T + b_qkv                    [B T, 3 H]   gnnrag_linear (packed weight)
//     ctx = softmax(q k^T / sqrt(dh)) v          per head     k_bert_attention
//     x   = LN(ctx W_o^T + b_o + x)                           gnnrag_linear (add = x), k_bert_add_ln
//     f   = gelu(x W_i^T + b_i)                  [B T, I]     gnnrag_linear, k_bert_gelu
//     x   = LN(f W_f^T + b_f + x)                             gnnrag_linear (add = x), k_bert_add_ln
//
// RobertaModel and MPNetModel (--lm roberta / relbert / sbert2) are the same block with two differences, both taken by
// gnnrag_bert_encode_ex:
//   * positions from the ids (pad_id >= 0): pos = pad_id + #{t' <= t : id[t'] != pad_id} for a non-pad token, pad_id for a
//     pad (transformers' create_position_ids_from_input_ids); MPNet has no token-type term (type_emb NULL);
//   * MPNet adds a relative-position bias to the scaled scores of every layer: s(i, j) += rel_bias[head][j - i + T - 1],
//     one table [heads, 2T-1] for all layers (k_bert_attention<DH, true>).
//
// Training-mode forward (gnnrag_bert_encode_train): the encoder is frozen, so there is no backward, but transformers draws
// dropout at four sites when the module is in training mode.  The caller brings the keep bytes (one per element, != 0
// keeps) and each site is fused into the launch that already produces the value:
//   embedding output           k_bert_embed_ln<.., DROP>     LN(...) * (keep ? scale : 0)
//   attention probabilities    k_bert_attention<.., DROP>    p_j * (keep ? scale : 0) behind the row's sum: not renormalised
//   W_o and W_f outputs        k_bert_drop_add_ln            LN(d * (keep ? scale : 0) + x); the product is a gnnrag_linear
//                                                            WITHOUT the residual (it is added behind the dropout)
// The product with 0 (not a select) keeps a non-finite value NaN as transformers' x * mask does.  DROP is a compile-time
// switch: the `DROP = false` instantiations take the two arguments last and never load them - their instructions are those
// of the kernels before the switch existed.
//
// Eight launches per layer.  fp32 throughout, no atomics, every reduction in an order the shape alone fixes (a wave's
// __shfl_xor tree, keys in ascending order), nothing allocated, nothing waits for the stream: safe under capture, a second
// call returns the same bits, and a question's rows never depend on the batch around it (LayerNorm: a wave per row;
// attention: a workgroup per (question, head); the dense products: a row of C depends on its row of A only).
#include "bert_device.h"
#include "bert_host.h"

#ifndef GNNRAG_BERT_ATT_THREADS
#define GNNRAG_BERT_ATT_THREADS 512  // 64 .. 1024, a multiple of 64; never changes a result
#endif

namespace gnnrag {

// kBertMaxT, kBertLnRows and the entry points' shape, scale and pointer rules: bert_host.h
// bert_keep4, bert_ln_row (the LayerNorm of one row by one wave) and bert_gelu: bert_device.h

// x[row] = LN(word_emb[id] + pos_emb[pos] + type_emb[0]); an id outside [0, vocab) reads nothing: its row is NaN.
// IDPOS = false: pos = row % T.  IDPOS = true (pad_id >= 0): the wave counts the non-pad ids among ids[b, 0 .. t] itself
// (two ids per lane, T <= 128, a ballot and a popcount; it reads its own question's ids only) and pos = pad_id + count for
// a non-pad token, pad_id for a pad; an id outside the vocabulary counts as non-pad.  A position outside [0, max_pos)
// reads nothing either: its row is NaN (the entry point's shape rule excludes it; this is the kernel's own bound).
// TYPE = false: no token-type term, type_emb is not read.
// DROP: the LayerNorm result goes through the keep bytes of plane [M, H]; a NaN row stays NaN whatever they are.
template <bool IDPOS, bool TYPE, bool DROP>
__global__ __launch_bounds__(64 * kBertLnRows) void k_bert_embed_ln(const int64_t* __restrict__ ids,
                                                                    const float* __restrict__ word_emb, int vocab,
                                                                    const float* __restrict__ pos_emb, int max_pos,
                                                                    const float* __restrict__ type_emb, int pad_id,
                                                                    const float* __restrict__ g,
                                                                    const float* __restrict__ bt, float eps, int M, int T,
                                                                    int H4, float* __restrict__ out,
                                                                    const uint8_t* __restrict__ keep, float scale) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kBertLnRows + (threadIdx.x >> 6);
  if (row >= M) return;
  float* dst = out + (size_t)row * H4 * 4;
  const int64_t id = ids[row];
  int pos = row % T;
  if (IDPOS) {
    const int64_t* q = ids + (size_t)(row - pos);       // this question's ids; lanes read q[0 .. pos] only
    const bool n0 = lane <= pos && q[lane] != (int64_t)pad_id;
    const bool n1 = lane + 64 <= pos && q[lane + 64] != (int64_t)pad_id;
    const int count = __popcll(__ballot(n0)) + __popcll(__ballot(n1));
    pos = id != (int64_t)pad_id ? pad_id + count : pad_id;
  }
  if (id < 0 || id >= (int64_t)vocab || pos < 0 || pos >= max_pos) {
    const float nan = __uint_as_float(0x7fc00000u);
    for (int i = lane; i < H4; i += 64) ((f32x4*)dst)[i] = (f32x4){nan, nan, nan, nan};
    return;
  }
  const f32x4* w = (const f32x4*)(word_emb + (size_t)id * H4 * 4);
  const f32x4* p = (const f32x4*)(pos_emb + (size_t)pos * H4 * 4);
  const uint8_t* kr = DROP ? keep + (size_t)row * H4 * 4 : nullptr;
  if (TYPE) {
    const f32x4* ty = (const f32x4*)type_emb;
    bert_ln_row<DROP>([&](int i) { return (w[i] + ty[i]) + p[i]; }, g, bt, eps, H4, lane, dst, kr, scale);
  } else {
    bert_ln_row<DROP>([&](int i) { return w[i] + p[i]; }, g, bt, eps, H4, lane, dst, kr, scale);
  }
}

// What the embedding backward needs of k_bert_embed_ln's row: sum0[row] = word_emb[id] + type_emb[0] + pos_emb[pos] - the
// same additions in the same order, so the value that kernel normalises - and pos_out[row] = pos.  A row that kernel makes
// NaN (an id or a position outside its table) gets a NaN sum0 row and pos_out = -1.  IDPOS / TYPE as there.
template <bool IDPOS, bool TYPE>
__global__ __launch_bounds__(64 * kBertLnRows) void k_bert_embed_save(const int64_t* __restrict__ ids,
                                                                      const float* __restrict__ word_emb, int vocab,
                                                                      const float* __restrict__ pos_emb, int max_pos,
                                                                      const float* __restrict__ type_emb, int pad_id, int M,
                                                                      int T, int H4, float* __restrict__ sum0,
                                                                      int32_t* __restrict__ pos_out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kBertLnRows + (threadIdx.x >> 6);
  if (row >= M) return;
  f32x4* dst = (f32x4*)(sum0 + (size_t)row * H4 * 4);
  const int64_t id = ids[row];
  int pos = row % T;
  if (IDPOS) {
    const int64_t* q = ids + (size_t)(row - pos);
    const bool n0 = lane <= pos && q[lane] != (int64_t)pad_id;
    const bool n1 = lane + 64 <= pos && q[lane + 64] != (int64_t)pad_id;
    const int count = __popcll(__ballot(n0)) + __popcll(__ballot(n1));
    pos = id != (int64_t)pad_id ? pad_id + count : pad_id;
  }
  if (id < 0 || id >= (int64_t)vocab || pos < 0 || pos >= max_pos) {
    const float nan = __uint_as_float(0x7fc00000u);
    for (int i = lane; i < H4; i += 64) dst[i] = (f32x4){nan, nan, nan, nan};
    if (lane == 0) pos_out[row] = -1;
    return;
  }
  const f32x4* w = (const f32x4*)(word_emb + (size_t)id * H4 * 4);
  const f32x4* p = (const f32x4*)(pos_emb + (size_t)pos * H4 * 4);
  const f32x4* ty = (const f32x4*)type_emb;
  for (int i = lane; i < H4; i += 64) dst[i] = TYPE ? (w[i] + ty[i]) + p[i] : w[i] + p[i];
  if (lane == 0) pos_out[row] = pos;
}

// out[row] = LN(in[row]); in already holds dense(x) + bias + residual.  out == in is allowed (no __restrict__ on the two).
__global__ __launch_bounds__(64 * kBertLnRows) void k_bert_add_ln(const float* in, const float* __restrict__ g,
                                                                  const float* __restrict__ bt, float eps, int M, int H4,
                                                                  float* out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kBertLnRows + (threadIdx.x >> 6);
  if (row >= M) return;
  const f32x4* src = (const f32x4*)(in + (size_t)row * H4 * 4);
  bert_ln_row([&](int i) { return src[i]; }, g, bt, eps, H4, lane, out + (size_t)row * H4 * 4);
}

// out[row] = LN(d[row] * (keep ? scale : 0) + out[row]): d = dense(x) + bias WITHOUT the residual, out holds the residual and
// receives the result (a lane writes only the elements it has read itself, after both reductions; d is another buffer).
// keep [M, H] bytes, 4-byte aligned.  A NaN in d or in the residual makes the row NaN whatever the keep bytes are.
__global__ __launch_bounds__(64 * kBertLnRows) void k_bert_drop_add_ln(const float* __restrict__ d,
                                                                       const uint8_t* __restrict__ keep, float scale,
                                                                       const float* __restrict__ g,
                                                                       const float* __restrict__ bt, float eps, int M,
                                                                       int H4, float* out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kBertLnRows + (threadIdx.x >> 6);
  if (row >= M) return;
  const f32x4* src = (const f32x4*)(d + (size_t)row * H4 * 4);
  const uint32_t* kr = (const uint32_t*)(keep + (size_t)row * H4 * 4);
  float* dst = out + (size_t)row * H4 * 4;
  bert_ln_row([&](int i) { return src[i] * bert_keep4(kr[i], scale) + ((const f32x4*)dst)[i]; }, g, bt, eps, H4, lane, dst);
}

// x = 0.5 x (1 + erf(x / sqrt 2)) in place over n floats (16-byte aligned); the last n % 4 by the first lanes
__global__ __launch_bounds__(256) void k_bert_gelu(float* __restrict__ x, size_t n) {
  const size_t n4 = n / 4, stride = (size_t)gridDim.x * blockDim.x;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = tid; i < n4; i += stride) {
    f32x4 v = ((f32x4*)x)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = bert_gelu(v[e]);
    ((f32x4*)x)[i] = v;
  }
  if (tid < n - n4 * 4) x[n4 * 4 + tid] = bert_gelu(x[n4 * 4 + tid]);
}

// The value unchanged, behind a barrier the optimiser does not look through: what is computed before it is compiled as if
// nothing followed.  k_bert_attention<DH, true> puts the scaled score through it before the bias is added, so that the dot
// product in front of it compiles to the instructions of k_bert_attention<DH, false> (the compiler mixes fused and
// unfused multiply-adds there by its own cost model) and an all-zero table gives that kernel's bits.
__device__ __forceinline__ float bert_opaque(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// One workgroup per (question, head).  LDS: the head's K and V slices [T, DH] with a row stride of DH + 1 floats (odd: the
// 32 lanes of a ds_read_b32 group that read k[lane][d] fall on 32 different banks), then per wave the query row [DH] and
// its T probabilities.  A wave owns a query row: lanes are keys (lane and lane + 64), the maximum and the sum of the row
// come from the fixed wave tree, then lanes run over d and add p[j] v[j][d] for j = 0 .. T - 1 in order.  No mask.
// BIAS: the head's row of rel_bias [heads, 2T-1] sits in LDS behind V (2T floats reserved) and the score of (t, j) is
// (q . k) scale + bias[j - t + T - 1]; without it rel_bias is not read and the LDS layout is the one above.
// DROP: keep [B, heads, T, T] bytes (query row t, key column j; any alignment).  After the row's maximum and sum the
// probability of key j is multiplied by scale where keep[b, h, t, j] != 0 and by 0 elsewhere; the row is NOT renormalised
// (transformers drops the probabilities behind the softmax).  A row whose keys are all dropped gives a zero context row.
template <int DH, bool BIAS, bool DROP>
__global__ __launch_bounds__(1024) void k_bert_attention(const float* __restrict__ qkv,
                                                         const float* __restrict__ rel_bias, int T, int heads,
                                                         float* __restrict__ ctx, const uint8_t* __restrict__ keep,
                                                         float keep_scale) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LD = DH + 1;
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int H = heads * DH;
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  float* ks = smem;                                   // [T, LD]
  float* vs = ks + T * LD;                            // [T, LD]
  float* bs = vs + T * LD;                            // [2T - 1] the head's bias row (BIAS only)
  float* qs = bs + (BIAS ? 2 * T : 0) + wave * (DH + kBertMaxT);  // [DH]   this wave's query row
  float* ps = qs + DH;                                // [kBertMaxT]  its probabilities

  const float* base = qkv + (size_t)b * T * 3 * H + h * DH;
  for (int i = tid; i < T * (DH / 4); i += nthr) {
    const int j = i / (DH / 4), c = (i % (DH / 4)) * 4;
    const float* row = base + (size_t)j * 3 * H;
    const f32x4 kv = *(const f32x4*)(row + H + c);
    const f32x4 vv = *(const f32x4*)(row + 2 * H + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ks[j * LD + c + e] = kv[e];
      vs[j * LD + c + e] = vv[e];
    }
  }
  if (BIAS) {
    const float* br = rel_bias + (size_t)h * (2 * T - 1);
    for (int i = tid; i < 2 * T - 1; i += nthr) bs[i] = br[i];
  }
  __syncthreads();

  const float scale = 1.f / sqrtf((float)DH);
  const int j0 = lane, j1 = lane + 64;
  for (int t = wave; t < T; t += nw) {
    if (lane < DH) qs[lane] = base[(size_t)t * 3 * H + lane];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    float s0 = -INFINITY, s1 = -INFINITY;
    if (j0 < T) {
      const float* k = ks + j0 * LD;
      float a = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) a += qs[d] * k[d];
      s0 = a * scale;
    }
    if (j1 < T) {
      const float* k = ks + j1 * LD;
      float a = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) a += qs[d] * k[d];
      s1 = a * scale;
    }
    if (BIAS) {  // in blocks of their own, behind the barrier: the two blocks above are those of the kernel without a bias
      if (j0 < T) s0 = bert_opaque(s0) + bs[j0 - t + T - 1];
      if (j1 < T) s1 = bert_opaque(s1) + bs[j1 - t + T - 1];
    }
    const float m = wave_max(fmaxf(s0, s1));
    const float e0 = j0 < T ? expf(s0 - m) : 0.f, e1 = j1 < T ? expf(s1 - m) : 0.f;
    const float sum = wave_sum(e0 + e1);
    if (DROP) {
      const uint8_t* kr = keep + ((size_t)blockIdx.x * T + t) * T;     // blockIdx.x = b heads + h
      if (j0 < T) ps[j0] = (e0 / sum) * (kr[j0] ? keep_scale : 0.f);
      if (j1 < T) ps[j1] = (e1 / sum) * (kr[j1] ? keep_scale : 0.f);
    } else {
      if (j0 < T) ps[j0] = e0 / sum;
      if (j1 < T) ps[j1] = e1 / sum;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < DH) {
      float acc = 0.f;
      for (int j = 0; j < T; ++j) acc += ps[j] * vs[j * LD + lane];
      ctx[((size_t)b * T + t) * H + h * DH + lane] = acc;
    }
    // the next row's writes to qs / ps follow this row's reads in program order (one wave, LDS in order)
    __builtin_amdgcn_wave_barrier();
  }
}

static inline size_t bert_att_lds_bytes(int T, int dh, int threads, bool bias) {
  return ((size_t)2 * T * (dh + 1) + (bias ? (size_t)2 * T : 0) + (size_t)(threads / 64) * (dh + kBertMaxT)) *
         sizeof(float);
}

template <int DH, bool BIAS, bool DROP>
static int bert_attention_launch_as(const float* qkv, const float* rel_bias, const uint8_t* keep, float keep_scale,
                                    int32_t B, int32_t T, int32_t heads, float* ctx, hipStream_t stream) {
  const int threads = GNNRAG_BERT_ATT_THREADS;
  const size_t lds = bert_att_lds_bytes(T, DH, threads, BIAS);
  const dim3 grid((unsigned)((int64_t)B * heads));
  if (lds > 64 * 1024) {
    static DeviceMask raised{0};
    GNNRAG_RC(raise_lds_cap(k_bert_attention<DH, BIAS, DROP>, raised));
  }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bert_attention<DH, BIAS, DROP>), grid, dim3(threads), lds, stream, qkv, rel_bias, T,
                     heads, ctx, keep, keep_scale);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

template <int DH>
static int bert_attention_launch_dh(const float* qkv, const float* rel_bias, const uint8_t* keep, float keep_scale, int32_t B,
                                    int32_t T, int32_t heads, float* ctx, hipStream_t stream) {
  if (keep)
    return rel_bias ? bert_attention_launch_as<DH, true, true>(qkv, rel_bias, keep, keep_scale, B, T, heads, ctx, stream)
                    : bert_attention_launch_as<DH, false, true>(qkv, nullptr, keep, keep_scale, B, T, heads, ctx, stream);
  return rel_bias ? bert_attention_launch_as<DH, true, false>(qkv, rel_bias, nullptr, 0.f, B, T, heads, ctx, stream)
                  : bert_attention_launch_as<DH, false, false>(qkv, nullptr, nullptr, 0.f, B, T, heads, ctx, stream);
}

// rel_bias NULL: no bias; keep NULL: no dropout (the kernel never sees a NULL pointer's argument)
static int bert_attention_launch(const float* qkv, const float* rel_bias, const uint8_t* keep, float keep_scale, int32_t B,
                                 int32_t T, int32_t heads, int32_t dh, float* ctx, hipStream_t stream) {
  return dh == 32 ? bert_attention_launch_dh<32>(qkv, rel_bias, keep, keep_scale, B, T, heads, ctx, stream)
                  : bert_attention_launch_dh<64>(qkv, rel_bias, keep, keep_scale, B, T, heads, ctx, stream);
}

// the workspace: qkv [M, 3H], ctx [M, H], sum [M, H] (dense + residual, the LayerNorm's input), ffn [M, I]; each block
// starts on a 256-byte boundary
struct BertWs {
  size_t qkv, ctx, sum, ffn, total;
};

static inline BertWs bert_ws(int64_t M, int64_t H, int64_t I) {
  BertWs w;
  Carve cv;
  w.qkv = cv.take((size_t)M * 3 * H * sizeof(float));
  w.ctx = cv.take((size_t)M * H * sizeof(float));
  w.sum = cv.take((size_t)M * H * sizeof(float));
  w.ffn = cv.take((size_t)M * I * sizeof(float));
  w.total = cv.off;
  return w;
}

// the workspace of the split-K form: qkv, ctx, ffn as above (no sum: the LayerNorm is the reduce's epilogue) and the
// partial products of the largest of a layer's four products; total 0 for a shape gnnrag_linear_splitk refuses
struct BertSplitkWs {
  size_t qkv, ctx, ffn, part, part_bytes, total;
};

static inline BertSplitkWs bert_splitk_ws(int64_t M, int32_t H, int32_t I) {
  BertSplitkWs w;
  memset(&w, 0, sizeof(w));
  const size_t p[4] = {gnnrag_linear_splitk_workspace_bytes(M, H, 3 * H, 0), gnnrag_linear_splitk_workspace_bytes(M, H, H, 0),
                       gnnrag_linear_splitk_workspace_bytes(M, H, I, 0), gnnrag_linear_splitk_workspace_bytes(M, I, H, 0)};
  for (int i = 0; i < 4; ++i) {
    if (!p[i]) return w;
    if (p[i] > w.part_bytes) w.part_bytes = p[i];
  }
  Carve cv;
  w.qkv = cv.take((size_t)M * 3 * H * sizeof(float));
  w.ctx = cv.take((size_t)M * H * sizeof(float));
  w.ffn = cv.take((size_t)M * I * sizeof(float));
  w.part = cv.take(w.part_bytes);
  w.total = cv.off;
  return w;
}

// where one layer's values go.  pre == ffn: the GELU runs in place on the product's output (no copy); xin / x1 NULL: the
// layer's input and LayerNorm 1's output are not kept.
struct BertLayerDst {
  float *qkv, *ctx, *sum1, *sum2, *pre, *ffn, *xin, *x1;
};

// The L layers on the running buffer `out` [M, H]: the one layer sequence of every entry point but the split-K one.
// dst_of(l) names layer l's destinations.  With workspace blocks, pre == ffn and no save slots these are the eight
// launches per layer of the inference and training forward; the saving forward points the products into its reserve and
// gets three device copies on top, each in front of the launch that overwrites what it keeps: xin before the QKV product,
// x1 behind LayerNorm 1, pre -> ffn before the GELU.  The same kernels on the same values in the same order either way:
// equal bits in `out`.
template <typename DstOf>
static int bert_layers_run(int32_t L, const gnnrag_bert_layer* layers, const float* rel_bias, float ln_eps, int32_t B,
                           int32_t T, int32_t H, int32_t heads, int32_t I, const BertKeep& keep, float scale_hidden,
                           float scale_att, float* out, DstOf dst_of, int32_t math, gnnrag_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  const int64_t M = (int64_t)B * T;
  const int32_t dh = H / heads;
  const int H4 = H / 4;
  const dim3 ln_grid((unsigned)((M + kBertLnRows - 1) / kBertLnRows)), ln_block(64 * kBertLnRows);
  const size_t n_ffn = (size_t)M * I, mh = (size_t)M * H * sizeof(float);
  const size_t gelu_blocks = (n_ffn / 4 + 255) / 256;
  const dim3 gelu_grid((unsigned)(gelu_blocks < 1 ? 1 : gelu_blocks > 65536 ? 65536 : gelu_blocks));
  // x = LN(dense(a) + b + x).  Inference: the residual rides in the product's epilogue.  With hidden dropout the product
  // goes without it and the LayerNorm launch drops, adds the residual and normalises (kp: the site's keep bytes).
  auto residual_block = [&](const float* a, int32_t K, const float* W, const float* b, const float* g, const float* bt,
                            const uint8_t* kp, float* sum) -> int {
    if (kp) {
      GNNRAG_RC(gnnrag_linear(a, M, K, W, b, nullptr, 0, 0, sum, H, math, stream));
      hipLaunchKernelGGL(k_bert_drop_add_ln, ln_grid, ln_block, 0, st, sum, kp, scale_hidden, g, bt, ln_eps, (int)M, H4,
                         out);
    } else {
      GNNRAG_RC(gnnrag_linear(a, M, K, W, b, out, M, 0, sum, H, math, stream));
      hipLaunchKernelGGL(k_bert_add_ln, ln_grid, ln_block, 0, st, sum, g, bt, ln_eps, (int)M, H4, out);
    }
    GNNRAG_LAUNCH_CHECK();
    return 0;
  };
  for (int l = 0; l < L; ++l) {
    const gnnrag_bert_layer& p = layers[l];
    const BertLayerDst d = dst_of(l);
    if (d.xin) GNNRAG_HIP(hipMemcpyAsync(d.xin, out, mh, hipMemcpyDeviceToDevice, st));
    GNNRAG_RC(gnnrag_linear(out, M, H, p.W_qkv, p.b_qkv, nullptr, 0, 0, d.qkv, 3 * H, math, stream));
    GNNRAG_RC(bert_attention_launch(d.qkv, rel_bias, keep.probs(l), scale_att, B, T, heads, dh, d.ctx, st));
    GNNRAG_RC(residual_block(d.ctx, H, p.W_o, p.b_o, p.ln1_g, p.ln1_b, keep.att_out(l), d.sum1));
    if (d.x1) GNNRAG_HIP(hipMemcpyAsync(d.x1, out, mh, hipMemcpyDeviceToDevice, st));
    GNNRAG_RC(gnnrag_linear(out, M, H, p.W_i, p.b_i, nullptr, 0, 0, d.pre, I, math, stream));
    if (d.pre != d.ffn) GNNRAG_HIP(hipMemcpyAsync(d.ffn, d.pre, n_ffn * sizeof(float), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_bert_gelu, gelu_grid, dim3(256), 0, st, d.ffn, n_ffn);
    GNNRAG_LAUNCH_CHECK();
    GNNRAG_RC(residual_block(d.ffn, I, p.W_f, p.b_f, p.ln2_g, p.ln2_b, keep.ffn_out(l), d.sum2));
  }
  return 0;
}

// The embedding launch of every entry point: pad_id >= 0 takes the positions from the ids, type_emb NULL leaves the
// token-type term out, keep NULL (plane 0 of keep_hidden otherwise) is the inference kernel.
static int bert_embed_ln_launch(const int64_t* ids, const float* word_emb, int32_t vocab, const float* pos_emb,
                                int32_t max_pos, const float* type_emb, int32_t pad_id, const float* ln_g,
                                const float* ln_b, float ln_eps, int64_t M, int32_t T, int32_t H, float* out,
                                const uint8_t* keep_hidden, float scale_hidden, hipStream_t st) {
  const int H4 = H / 4;
  const dim3 ln_grid((unsigned)((M + kBertLnRows - 1) / kBertLnRows)), ln_block(64 * kBertLnRows);
#define GNNRAG_EMBED_LN(IDPOS, TYPE)                                                                                    \
  if (keep_hidden)                                                                                                      \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bert_embed_ln<IDPOS, TYPE, true>), ln_grid, ln_block, 0, st, ids, word_emb,    \
                       vocab, pos_emb, max_pos, type_emb, pad_id, ln_g, ln_b, ln_eps, (int)M, T, H4, out, keep_hidden,  \
                       scale_hidden);                                                                                   \
  else                                                                                                                  \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bert_embed_ln<IDPOS, TYPE, false>), ln_grid, ln_block, 0, st, ids, word_emb,   \
                       vocab, pos_emb, max_pos, type_emb, pad_id, ln_g, ln_b, ln_eps, (int)M, T, H4, out,               \
                       (const uint8_t*)nullptr, 0.f)
  if (pad_id >= 0 && type_emb) {
    GNNRAG_EMBED_LN(true, true);
  } else if (pad_id >= 0) {
    GNNRAG_EMBED_LN(true, false);
  } else if (type_emb) {
    GNNRAG_EMBED_LN(false, true);
  } else {
    GNNRAG_EMBED_LN(false, false);
  }
#undef GNNRAG_EMBED_LN
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

// k_bert_embed_save on the same arguments
static int bert_embed_save_launch(const int64_t* ids, const float* word_emb, int32_t vocab, const float* pos_emb,
                                  int32_t max_pos, const float* type_emb, int32_t pad_id, int64_t M, int32_t T, int32_t H,
                                  float* sum0, int32_t* pos, hipStream_t st) {
  const dim3 grid((unsigned)((M + kBertLnRows - 1) / kBertLnRows)), block(64 * kBertLnRows);
#define GNNRAG_EMBED_SAVE(IDPOS, TYPE)                                                                                  \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bert_embed_save<IDPOS, TYPE>), grid, block, 0, st, ids, word_emb, vocab, pos_emb, \
                     max_pos, type_emb, pad_id, (int)M, T, H / 4, sum0, pos)
  if (pad_id >= 0 && type_emb) {
    GNNRAG_EMBED_SAVE(true, true);
  } else if (pad_id >= 0) {
    GNNRAG_EMBED_SAVE(true, false);
  } else if (type_emb) {
    GNNRAG_EMBED_SAVE(false, true);
  } else {
    GNNRAG_EMBED_SAVE(false, false);
  }
#undef GNNRAG_EMBED_SAVE
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

}  // namespace gnnrag

using namespace gnnrag;

extern "C" size_t gnnrag_bert_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t I) {
  if (B <= 0 || T <= 0 || H <= 0 || I <= 0) return 0;
  return bert_ws((int64_t)B * T, H, I).total;
}

extern "C" size_t gnnrag_bert_splitk_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t I) {
  if (B <= 0 || T <= 0 || H <= 0 || I <= 0 || (int64_t)3 * H > INT32_MAX) return 0;
  return bert_splitk_ws((int64_t)B * T, H, I).total;
}

extern "C" size_t gnnrag_bert_keep_hidden_bytes(int32_t L, int32_t B, int32_t T, int32_t H) {
  if (L < 0 || B <= 0 || T <= 0 || H <= 0) return 0;      // L = 0 is legal: plane 0 alone
  return (size_t)(1 + 2 * (int64_t)L) * B * T * H;
}

extern "C" size_t gnnrag_bert_keep_att_bytes(int32_t L, int32_t B, int32_t T, int32_t heads) {
  if (L <= 0 || B <= 0 || T <= 0 || heads <= 0) return 0;
  return (size_t)L * B * heads * T * T;
}

extern "C" int gnnrag_bert_attention_drop(const float* qkv, int32_t B, int32_t T, int32_t heads, int32_t dh,
                                          const float* rel_bias, const uint8_t* keep, float scale, float* ctx,
                                          gnnrag_stream_t stream) {
  if (B <= 0 || T <= 0 || heads <= 0 || dh <= 0) return GNNRAG_E_BADARG;
  if (!bert_att_shape_ok(B, T, heads, dh)) return GNNRAG_E_UNSUPPORTED;
  if (!qkv || !ctx || !bert_scale_ok(keep, scale)) return GNNRAG_E_BADARG;
  if (!aligned16(qkv, ctx, rel_bias)) return GNNRAG_E_UNSUPPORTED;
  return bert_attention_launch(qkv, rel_bias, keep, scale, B, T, heads, dh, ctx, (hipStream_t)stream);
}

extern "C" int gnnrag_bert_attention_bias(const float* qkv, int32_t B, int32_t T, int32_t heads, int32_t dh,
                                          const float* rel_bias, float* ctx, gnnrag_stream_t stream) {
  return gnnrag_bert_attention_drop(qkv, B, T, heads, dh, rel_bias, nullptr, 0.f, ctx, stream);
}

extern "C" int gnnrag_bert_attention(const float* qkv, int32_t B, int32_t T, int32_t heads, int32_t dh, float* ctx,
                                     gnnrag_stream_t stream) {
  return gnnrag_bert_attention_bias(qkv, B, T, heads, dh, nullptr, ctx, stream);
}

// all encode entry points: the argument rules, the embedding launch, then the layers on bert_layers_run with every
// destination in the workspace.  need_type: a NULL type_emb is an argument error (gnnrag_bert_encode), not "no token-type
// term".  keep_hidden / keep_att NULL: that dropout site keeps the inference sequence (its scale is not read); both NULL
// is the inference call, launch for launch.
// splitk (inference only, both keeps NULL): the four products of a layer on gnnrag_linear_splitk, the GELU and the two
// LayerNorms in its reduce; the embedding and attention launches are the same.
static int bert_encode_run(const int64_t* ids, const float* word_emb, int32_t vocab, const float* pos_emb,
                           int32_t max_pos, const float* type_emb, bool need_type, int32_t pad_id, const float* rel_bias,
                           const float* ln_g, const float* ln_b, float ln_eps, int32_t L, const gnnrag_bert_layer* layers,
                           int32_t B, int32_t T, int32_t H, int32_t heads, int32_t I, const uint8_t* keep_hidden,
                           float scale_hidden, const uint8_t* keep_att, float scale_att, float* out, void* ws,
                           size_t ws_bytes, int32_t math, gnnrag_stream_t stream, bool splitk = false) {
  if (B <= 0 || T <= 0 || H <= 0 || heads <= 0 || I <= 0 || L < 0 || vocab <= 0 || max_pos <= 0) return GNNRAG_E_BADARG;
  if (math != GNNRAG_MATH_FP32 && math != GNNRAG_MATH_BF16X3 && math != GNNRAG_MATH_MIXED) return GNNRAG_E_BADARG;
  // the shape rules first: they are answered whatever the pointers are
  if (H % heads != 0 || H % 4 != 0 || T > kBertMaxT || T > max_pos) return GNNRAG_E_UNSUPPORTED;
  // positions from the ids: a full row reaches position T + pad_id, which must be a row of pos_emb
  if (pad_id >= 0 && (int64_t)T + pad_id > (int64_t)max_pos - 1) return GNNRAG_E_UNSUPPORTED;
  const int32_t dh = H / heads;
  if (!bert_att_shape_ok(B, T, heads, dh) || (int64_t)B * T >= ((int64_t)1 << 31)) return GNNRAG_E_UNSUPPORTED;
  const int64_t M = (int64_t)B * T;
  const BertWs w = bert_ws(M, H, I);
  BertSplitkWs sw{};
  if (splitk) {
    if (I % 4 != 0 || (int64_t)3 * H > INT32_MAX) return GNNRAG_E_UNSUPPORTED;
    sw = bert_splitk_ws(M, H, I);
    if (L > 0 && (!sw.total || ws_bytes < sw.total)) return GNNRAG_E_UNSUPPORTED;
  } else if (L > 0 && ws_bytes < w.total) {
    return GNNRAG_E_UNSUPPORTED;
  }
  if (!ids || !word_emb || !pos_emb || (need_type && !type_emb) || !ln_g || !ln_b || !out || (L > 0 && (!layers || !ws)))
    return GNNRAG_E_BADARG;
  if (!bert_scale_ok(keep_hidden, scale_hidden) || !bert_scale_ok(keep_att, scale_att)) return GNNRAG_E_BADARG;
  // keep_hidden is read a 32-bit word per float4; keep_att byte by byte (any alignment)
  if (!aligned16(word_emb, pos_emb, type_emb, rel_bias, ln_g, ln_b, out) || ((uintptr_t)ids & 7) ||
      (L > 0 && !aligned16(ws)) || ((uintptr_t)keep_hidden & 3))
    return GNNRAG_E_UNSUPPORTED;
  for (int l = 0; l < L; ++l) GNNRAG_RC(bert_layer_ptrs_check(layers[l], kBertFieldsAll));

  hipStream_t st = (hipStream_t)stream;
  GNNRAG_RC(bert_embed_ln_launch(ids, word_emb, vocab, pos_emb, max_pos, type_emb, pad_id, ln_g, ln_b, ln_eps, M, T, H, out,
                                 keep_hidden, scale_hidden, st));
  if (L == 0) return 0;

  if (splitk) {
    float* qkv = (float*)((char*)ws + sw.qkv);
    float* ctx = (float*)((char*)ws + sw.ctx);
    float* ffn = (float*)((char*)ws + sw.ffn);
    void* part = (char*)ws + sw.part;
    for (int l = 0; l < L; ++l) {
      const gnnrag_bert_layer& p = layers[l];
      GNNRAG_RC(gnnrag_linear_splitk(out, M, H, p.W_qkv, p.b_qkv, GNNRAG_SPLITK_EPI_BIAS, nullptr, nullptr, nullptr, 0.f,
                                     qkv, 3 * H, 0, part, sw.part_bytes, stream));
      GNNRAG_RC(bert_attention_launch(qkv, rel_bias, nullptr, 0.f, B, T, heads, dh, ctx, st));
      GNNRAG_RC(gnnrag_linear_splitk(ctx, M, H, p.W_o, p.b_o, GNNRAG_SPLITK_EPI_ADD_LN, out, p.ln1_g, p.ln1_b, ln_eps, out,
                                     H, 0, part, sw.part_bytes, stream));
      GNNRAG_RC(gnnrag_linear_splitk(out, M, H, p.W_i, p.b_i, GNNRAG_SPLITK_EPI_GELU, nullptr, nullptr, nullptr, 0.f, ffn,
                                     I, 0, part, sw.part_bytes, stream));
      GNNRAG_RC(gnnrag_linear_splitk(ffn, M, I, p.W_f, p.b_f, GNNRAG_SPLITK_EPI_ADD_LN, out, p.ln2_g, p.ln2_b, ln_eps, out,
                                     H, 0, part, sw.part_bytes, stream));
    }
    return 0;
  }

  // one set of workspace blocks for every layer, the GELU in place, nothing saved
  char* wsb = (char*)ws;
  float* sum = (float*)(wsb + w.sum);
  float* ffn = (float*)(wsb + w.ffn);
  const BertLayerDst d{(float*)(wsb + w.qkv), (float*)(wsb + w.ctx), sum, sum, ffn, ffn, nullptr, nullptr};
  return bert_layers_run(L, layers, rel_bias, ln_eps, B, T, H, heads, I, BertKeep(keep_hidden, keep_att, B, T, H, heads),
                         scale_hidden, scale_att, out, [&](int) { return d; }, math, stream);
}

extern "C" int gnnrag_bert_encode_train(const int64_t* ids, const float* word_emb, int32_t vocab, const float* pos_emb,
                                        int32_t max_pos, const float* type_emb, int32_t pad_id, const float* rel_bias,
                                        const float* ln_g, const float* ln_b, float ln_eps, int32_t L,
                                        const gnnrag_bert_layer* layers, int32_t B, int32_t T, int32_t H, int32_t heads,
                                        int32_t I, const uint8_t* keep_hidden, float scale_hidden, const uint8_t* keep_att,
                                        float scale_att, float* out, void* ws, size_t ws_bytes, int32_t math,
                                        gnnrag_stream_t stream) {
  return bert_encode_run(ids, word_emb, vocab, pos_emb, max_pos, type_emb, false, pad_id, rel_bias, ln_g, ln_b, ln_eps, L,
                         layers, B, T, H, heads, I, keep_hidden, scale_hidden, keep_att, scale_att, out, ws, ws_bytes, math,
                         stream);
}

extern "C" int gnnrag_bert_encode(const int64_t* ids, const float* word_emb, int32_t vocab, const float* pos_emb,
                                  int32_t max_pos, const float* type_emb, const float* ln_g, const float* ln_b,
                                  float ln_eps, int32_t L, const gnnrag_bert_layer* layers, int32_t B, int32_t T, int32_t H,
                                  int32_t heads, int32_t I, float* out, void* ws, size_t ws_bytes, int32_t math,
                                  gnnrag_stream_t stream) {
  return bert_encode_run(ids, word_emb, vocab, pos_emb, max_pos, type_emb, true, -1, nullptr, ln_g, ln_b, ln_eps, L, layers,
                         B, T, H, heads, I, nullptr, 0.f, nullptr, 0.f, out, ws, ws_bytes, math, stream);
}

extern "C" int gnnrag_bert_encode_ex(const int64_t* ids, const float* word_emb, int32_t vocab, const float* pos_emb,
                                     int32_t max_pos, const float* type_emb, int32_t pad_id, const float* rel_bias,
                                     const float* ln_g, const float* ln_b, float ln_eps, int32_t L,
                                     const gnnrag_bert_layer* layers, int32_t B, int32_t T, int32_t H, int32_t heads,
                                     int32_t I, float* out, void* ws, size_t ws_bytes, int32_t math,
                                     gnnrag_stream_t stream) {
  return bert_encode_run(ids, word_emb, vocab, pos_emb, max_pos, type_emb, false, pad_id, rel_bias, ln_g, ln_b, ln_eps, L,
                         layers, B, T, H, heads, I, nullptr, 0.f, nullptr, 0.f, out, ws, ws_bytes, math, stream);
}

extern "C" int gnnrag_bert_encode_splitk(const int64_t* ids, const float* word_emb, int32_t vocab, const float* pos_emb,
                                         int32_t max_pos, const float* type_emb, int32_t pad_id, const float* rel_bias,
                                         const float* ln_g, const float* ln_b, float ln_eps, int32_t L,
                                         const gnnrag_bert_layer* layers, int32_t B, int32_t T, int32_t H, int32_t heads,
                                         int32_t I, float* out, void* ws, size_t ws_bytes, int32_t math,
                                         gnnrag_stream_t stream) {
  return bert_encode_run(ids, word_emb, vocab, pos_emb, max_pos, type_emb, false, pad_id, rel_bias, ln_g, ln_b, ln_eps, L,
                         layers, B, T, H, heads, I, nullptr, 0.f, nullptr, 0.f, out, ws, ws_bytes, math, stream, true);
}

extern "C" size_t gnnrag_bert_reserve_bytes(int32_t L, int32_t B, int32_t T, int32_t H, int32_t I) {
  if (L <= 0 || B <= 0 || T <= 0 || H <= 0 || I <= 0 || (H & 3) || (I & 3)) return 0;
  return (size_t)L * bert_reserve((int64_t)B * T, H, I).layer;
}

// bert_layers_run - the layer loop bert_encode_run calls - on a caller-given x0, with the values the backward needs left in
// the reserve (bert_reserve.h) instead of the workspace: the products write their blocks of the reserve directly; the
// layer input, LayerNorm 1's output and the FFN pre-activation go to its save slots.  rel_bias NULL: no relative attention
// bias (gnnrag_bert_layers_forward_save).  Its own argument rules: a short reserve or workspace is GNNRAG_E_WORKSPACE,
// behind every pointer rule.
extern "C" int gnnrag_bert_layers_forward_save_ex(const float* x0, int32_t L, const gnnrag_bert_layer* layers,
                                                  const float* rel_bias, float ln_eps, int32_t B, int32_t T, int32_t H,
                                                  int32_t heads, int32_t I, const uint8_t* keep_hidden, float scale_hidden,
                                                  const uint8_t* keep_att, float scale_att, float* out, void* reserve,
                                                  size_t reserve_bytes, void* ws, size_t ws_bytes, int32_t math,
                                                  gnnrag_stream_t stream) {
  if (B <= 0 || T <= 0 || H <= 0 || heads <= 0 || I <= 0 || L <= 0) return GNNRAG_E_BADARG;
  if (math != GNNRAG_MATH_FP32 && math != GNNRAG_MATH_BF16X3 && math != GNNRAG_MATH_MIXED) return GNNRAG_E_BADARG;
  if (H % heads != 0 || H % 4 != 0 || I % 4 != 0 || T > kBertMaxT) return GNNRAG_E_UNSUPPORTED;
  const int32_t dh = H / heads;
  if (!bert_att_shape_ok(B, T, heads, dh) || (int64_t)B * T >= ((int64_t)1 << 31)) return GNNRAG_E_UNSUPPORTED;
  const int64_t M = (int64_t)B * T;
  const BertWs w = bert_ws(M, H, I);
  const BertReserve r = bert_reserve(M, H, I);
  if (!x0 || !layers || !out || !reserve || !ws) return GNNRAG_E_BADARG;
  if (!bert_scale_ok(keep_hidden, scale_hidden) || !bert_scale_ok(keep_att, scale_att)) return GNNRAG_E_BADARG;
  if (!aligned16(x0, out, reserve, ws, rel_bias) || ((uintptr_t)keep_hidden & 3)) return GNNRAG_E_UNSUPPORTED;
  for (int l = 0; l < L; ++l) GNNRAG_RC(bert_layer_ptrs_check(layers[l], kBertFieldsAll));
  if (reserve_bytes < (size_t)L * r.layer || ws_bytes < w.total) return GNNRAG_E_WORKSPACE;

  if (out != x0)
    GNNRAG_HIP(hipMemcpyAsync(out, x0, (size_t)M * H * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  float* ffn = (float*)((char*)ws + w.ffn);
  auto dst_of = [&](int l) {
    char* rl = (char*)reserve + (size_t)l * r.layer;
    return BertLayerDst{(float*)(rl + r.qkv), (float*)(rl + r.ctx), (float*)(rl + r.sum1), (float*)(rl + r.sum2),
                        (float*)(rl + r.pre), ffn,                  (float*)(rl + r.xin),  (float*)(rl + r.x1)};
  };
  return bert_layers_run(L, layers, rel_bias, ln_eps, B, T, H, heads, I, BertKeep(keep_hidden, keep_att, B, T, H, heads),
                         scale_hidden, scale_att, out, dst_of, math, stream);
}

extern "C" int gnnrag_bert_layers_forward_save(const float* x0, int32_t L, const gnnrag_bert_layer* layers, float ln_eps,
                                               int32_t B, int32_t T, int32_t H, int32_t heads, int32_t I,
                                               const uint8_t* keep_hidden, float scale_hidden, const uint8_t* keep_att,
                                               float scale_att, float* out, void* reserve, size_t reserve_bytes, void* ws,
                                               size_t ws_bytes, int32_t math, gnnrag_stream_t stream) {
  return gnnrag_bert_layers_forward_save_ex(x0, L, layers, nullptr, ln_eps, B, T, H, heads, I, keep_hidden, scale_hidden,
                                            keep_att, scale_att, out, reserve, reserve_bytes, ws, ws_bytes, math, stream);
}

extern "C" size_t gnnrag_bert_embed_reserve_bytes(int32_t B, int32_t T, int32_t H) {
  if (B <= 0 || T <= 0 || H <= 0 || (H & 3)) return 0;
  return bert_embed_reserve((int64_t)B * T, H).total;
}

// The embedding stage of gnnrag_bert_encode_train - its k_bert_embed_ln launch on the same arguments, so its bits in
// `out` - and k_bert_embed_save for the reserve of gnnrag_bert_embed_backward.
extern "C" int gnnrag_bert_embed_forward_save(const int64_t* ids, const float* word_emb, int32_t vocab,
                                              const float* pos_emb, int32_t max_pos, const float* type_emb, int32_t pad_id,
                                              const float* ln_g, const float* ln_b, float ln_eps, int32_t B, int32_t T,
                                              int32_t H, const uint8_t* keep, float scale, float* out, void* reserve,
                                              size_t reserve_bytes, gnnrag_stream_t stream) {
  if (B <= 0 || T <= 0 || H <= 0 || vocab <= 0 || max_pos <= 0) return GNNRAG_E_BADARG;
  if (H % 4 != 0 || T > kBertMaxT || T > max_pos) return GNNRAG_E_UNSUPPORTED;
  if (pad_id >= 0 && (int64_t)T + pad_id > (int64_t)max_pos - 1) return GNNRAG_E_UNSUPPORTED;
  if ((int64_t)B * T >= ((int64_t)1 << 31)) return GNNRAG_E_UNSUPPORTED;
  if (!ids || !word_emb || !pos_emb || !ln_g || !ln_b || !out || !reserve || !bert_scale_ok(keep, scale))
    return GNNRAG_E_BADARG;
  if (!aligned16(word_emb, pos_emb, type_emb, ln_g, ln_b, out, reserve) || ((uintptr_t)ids & 7) || ((uintptr_t)keep & 3))
    return GNNRAG_E_UNSUPPORTED;
  const int64_t M = (int64_t)B * T;
  const BertEmbedReserve r = bert_embed_reserve(M, H);
  if (reserve_bytes < r.total) return GNNRAG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  GNNRAG_RC(bert_embed_ln_launch(ids, word_emb, vocab, pos_emb, max_pos, type_emb, pad_id, ln_g, ln_b, ln_eps, M, T, H, out,
                                 keep, scale, st));
  return bert_embed_save_launch(ids, word_emb, vocab, pos_emb, max_pos, type_emb, pad_id, M, T, H,
                                (float*)((char*)reserve + r.sum0), (int32_t*)((char*)reserve + r.pos), st);
}
