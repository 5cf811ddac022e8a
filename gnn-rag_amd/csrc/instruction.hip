// Instruction generation of the question encoder (the instruction path):
// BaseInstruction.get_instruction (reference gnn/modules/question_encoding/base_encoder.py:82-101) for ALL steps of a
// question in ONE launch.  Per question b, with r = r_in[b] (zeros when there is none), for step s:
//   q_s  = W_q[s] node[b] + b_q[s]                                  (:92)
//   cq   = W_cq [r, q_s, q_s - r, q_s * r] + b_cq                   (:93)
//   ca_t = sum_d w_ca[d] (cq[d] hidden[b,t,d]) + b_ca               (:95)
//   a    = softmax_t(ca_t + (1 - mask[b,t]) * kVeryNeg)             (:98)
//   r    = sum_t a_t hidden[b,t,:]                                  (:100)   -> ins_out[s,b,:], attn_out[s,b,:]
// The torch form is ~14 small launches per step, num_ins steps, twice per forward.  Here: one workgroup per question (the
// steps are a dependent chain; no grid-wide barrier), the question's token states stay in LDS (read twice per step), the
// products q_s - which do not depend on the chain - are all computed before the first step.  Matrix-vector products as in
// k_query_reform: a wave owns an output, its lanes stride over the terms (rows of W are read coalesced), a fixed
// __shfl_xor tree: one summation order, whatever the workgroup size.  No atomics: a second call returns the same bits.
//
// Training form (gnnrag_instructions_train; the backward is instruction_bwd.hip): the same kernel with two compile-time
// switches, as lstm.hip does SAVE.  TRAIN also leaves q_s and cq of every step in the caller's reserve [n, B, 2 D] - the
// arithmetic and its order are untouched, ins / attn are the bits of the inference form.  MASKS applies the three dropout
// multipliers of linear_drop (base_encoder.py:92, :93, :95): node * m1, [r, q, q - r, q * r] * m2 and (cq * hidden) * m3;
// there w_ca is no longer folded into cq ahead of the token products (the multiplier sits between them, :95).
#include "gnnrag_common.h"

#ifndef GNNRAG_INS_THREADS
#define GNNRAG_INS_THREADS 512       // 256 .. 1024, a multiple of 64; never changes a result
#endif

namespace gnnrag {

struct InsLinears {                  // question_linear{s}: separate parameters, carried in the kernel arguments
  const float* W[GNNRAG_MAX_INS];    // [D, D]
  const float* b[GNNRAG_MAX_INS];    // [D]
};

constexpr size_t kInsLdsBytes = 160 * 1024;      // a CU's LDS: the budget of one question's working set

// floats of LDS one question needs: token states (rounded up to 4), q_s of every step, r, w_ca * cq, the T logits
static inline size_t ins_lds_floats(int64_t T, int64_t D, int64_t n_steps) {
  return (size_t)((T * D + 3) / 4 * 4 + (n_steps + 2) * D + T);
}

struct InsTrain {                    // what the training form adds (all NULL / unused in the inference form)
  const float* m1;                   // [n, B, D]     multiplier of node, or NULL (ones)
  const float* m2;                   // [n, B, 4 D]   multiplier of [r, q, q - r, q * r], or NULL
  const float* m3;                   // [n, B, T, D]  multiplier of cq * hidden, or NULL
  float* reserve;                    // [n, B, 2 D]   q_s, then cq
};

template <bool TRAIN, bool MASKS>
__global__ __launch_bounds__(1024) void k_instructions(const float* __restrict__ hidden, const float* __restrict__ node,
                                                       const float* __restrict__ mask, const float* __restrict__ r_in,
                                                       const InsLinears ql, const float* __restrict__ W_cq,
                                                       const float* __restrict__ b_cq, const float* __restrict__ w_ca,
                                                       const float* __restrict__ b_ca, int B, int T, int D, int n_steps,
                                                       float* __restrict__ ins_out, float* __restrict__ attn_out,
                                                       const InsTrain tr) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int TD = T * D;
  float* hid = smem;                           // [T, D]  the question's token states
  float* qs = hid + (TD + 3) / 4 * 4;          // [n_steps, D]
  float* rv = qs + n_steps * D;                // [D]  the running instruction
  float* cv = rv + D;                          // [D]  w_ca * cq
  float* lg = cv + D;                          // [T]  logits, then attention weights
  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;

  const float* hb = hidden + (size_t)b * TD;
  if ((TD & 3) == 0 && ((uintptr_t)hb & 15) == 0) {
    const f32x4* src = (const f32x4*)hb;
    f32x4* dst = (f32x4*)hid;
    for (int i = tid; i < TD / 4; i += nthr) dst[i] = src[i];
  } else {
    for (int i = tid; i < TD; i += nthr) hid[i] = hb[i];
  }
  for (int d = tid; d < D; d += nthr) rv[d] = r_in ? r_in[(size_t)b * D + d] : 0.f;

  // q_s of every step: two outputs per wave and round (independent load streams; the loop is a chain of L2 round trips)
  const float* nd = node + (size_t)b * D;
#pragma unroll
  for (int s = 0; s < GNNRAG_MAX_INS; ++s) {
    if (s < n_steps) {
      const float* W = ql.W[s];
      const float* bq = ql.b[s];
      const float* m1 = (MASKS && tr.m1) ? tr.m1 + ((size_t)s * B + b) * D : nullptr;
      for (int j = wave; j < D; j += 2 * nw) {
        const int j2 = j + nw < D ? j + nw : j;
        const float* w0 = W + (size_t)j * D;
        const float* w1 = W + (size_t)j2 * D;
        float a0 = 0.f, a1 = 0.f;
        for (int k = lane; k < D; k += 64) {
          float x = nd[k];
          if (MASKS && m1) x *= m1[k];
          a0 += w0[k] * x;
          a1 += w1[k] * x;
        }
        a0 = wave_sum(a0);
        a1 = wave_sum(a1);
        if (lane == 0) qs[s * D + j] = a0 + bq[j];
        if (lane == 1 && j2 != j) qs[s * D + j2] = a1 + bq[j2];
      }
    }
  }
  __syncthreads();

  const float bca = b_ca[0];
  const float* mk = mask + (size_t)b * T;
  for (int s = 0; s < n_steps; ++s) {
    const float* q = qs + s * D;
    const float* m2 = (MASKS && tr.m2) ? tr.m2 + ((size_t)s * B + b) * 4 * D : nullptr;
    float* rs = TRAIN ? tr.reserve + ((size_t)s * B + b) * 2 * D : nullptr;
    if (TRAIN)
      for (int d = tid; d < D; d += nthr) rs[d] = q[d];
    // cv = w_ca * (W_cq [r, q, q - r, q * r] + b_cq): the four blocks of a row are four load streams
    for (int j = wave; j < D; j += 2 * nw) {
      const int j2 = j + nw < D ? j + nw : j;
      const float* w0 = W_cq + (size_t)j * 4 * D;
      const float* w1 = W_cq + (size_t)j2 * 4 * D;
      float a0 = 0.f, a1 = 0.f;
      for (int k = lane; k < D; k += 64) {
        float r = rv[k], x = q[k], df = x - r, pr = x * r;
        if (MASKS && m2) {
          r *= m2[k];
          x *= m2[D + k];
          df *= m2[2 * D + k];
          pr *= m2[3 * D + k];
        }
        a0 += w0[k] * r;
        a1 += w1[k] * r;
        a0 += w0[D + k] * x;
        a1 += w1[D + k] * x;
        a0 += w0[2 * D + k] * df;
        a1 += w1[2 * D + k] * df;
        a0 += w0[3 * D + k] * pr;
        a1 += w1[3 * D + k] * pr;
      }
      a0 = wave_sum(a0);
      a1 = wave_sum(a1);
      if (lane == 0) {
        const float c = a0 + b_cq[j];
        if (TRAIN) rs[D + j] = c;
        cv[j] = MASKS ? c : c * w_ca[j];
      }
      if (lane == 1 && j2 != j) {
        const float c = a1 + b_cq[j2];
        if (TRAIN) rs[D + j2] = c;
        cv[j2] = MASKS ? c : c * w_ca[j2];
      }
    }
    __syncthreads();
    // logits: a wave per token
    for (int t = wave; t < T; t += nw) {
      const float* h = hid + t * D;
      float acc = 0.f;
      if (MASKS) {
        // the reference's order: (cq * hidden) * m3, then the products with w_ca (no contraction across the multiplier)
        const float* m3 = tr.m3 ? tr.m3 + (((size_t)s * B + b) * T + t) * D : nullptr;
        for (int d = lane; d < D; d += 64) {
          float p = __fmul_rn(cv[d], h[d]);
          if (m3) p = __fmul_rn(p, m3[d]);
          acc += w_ca[d] * p;
        }
      } else {
        for (int d = lane; d < D; d += 64) acc += cv[d] * h[d];
      }
      acc = wave_sum(acc);
      // the fp32 sum the reference writes (no contraction): a padded token's logit is kVeryNeg for any |ca| < 4096
      if (lane == 0) lg[t] = __fadd_rn(__fadd_rn(acc, bca), __fmul_rn(__fsub_rn(1.f, mk[t]), kVeryNeg));
    }
    __syncthreads();
    // softmax over the T tokens: every wave derives the same maximum and the same sum (same order), no hand-over
    float m = -INFINITY;
    for (int t = lane; t < T; t += 64) m = fmaxf(m, lg[t]);
    m = wave_max(m);
    float sum = 0.f;
    for (int t = lane; t < T; t += 64) sum += expf(lg[t] - m);
    sum = wave_sum(sum);
    __syncthreads();                                       // every wave has read the logits
    float* ao = attn_out + ((size_t)s * B + b) * T;
    for (int t = tid; t < T; t += nthr) {
      const float a = expf(lg[t] - m) / sum;
      lg[t] = a;
      ao[t] = a;
    }
    __syncthreads();
    // r = sum_t a_t hidden[t, :], ascending t
    float* io = ins_out + ((size_t)s * B + b) * D;
    for (int d = tid; d < D; d += nthr) {
      float acc = 0.f;
      for (int t = 0; t < T; ++t) acc += lg[t] * hid[t * D + d];
      rv[d] = acc;
      io[d] = acc;
    }
    __syncthreads();
  }
}

}  // namespace gnnrag

using namespace gnnrag;

template <bool TRAIN, bool MASKS>
static int ins_launch(const float* hidden, const float* node, const float* mask, const float* r_in, const InsLinears& ql,
                      const float* W_cq, const float* b_cq, const float* w_ca, const float* b_ca, int32_t B, int32_t T,
                      int32_t D, int32_t n_steps, float* ins_out, float* attn_out, const InsTrain& tr, size_t lds,
                      hipStream_t stream) {
  if (lds > 64 * 1024) {
    static DeviceMask raised{0};
    GNNRAG_RC(raise_lds_cap(k_instructions<TRAIN, MASKS>, raised));
  }
  hipLaunchKernelGGL((k_instructions<TRAIN, MASKS>), dim3(B), dim3(GNNRAG_INS_THREADS), lds, stream, hidden, node, mask,
                     r_in, ql, W_cq, b_cq, w_ca, b_ca, B, T, D, n_steps, ins_out, attn_out, tr);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

// the argument checks and the launch of both entry points; reserve == nullptr: the inference form
static int ins_run(const float* hidden, const float* node, const float* mask, const float* r_in, const float* const* W_q,
                   const float* const* b_q, const float* W_cq, const float* b_cq, const float* w_ca, const float* b_ca,
                   int32_t B, int32_t T, int32_t D, int32_t n_steps, float* ins_out, float* attn_out, const InsTrain& tr,
                   bool train, size_t reserve_bytes, gnnrag_stream_t stream) {
  if (!hidden || !node || !mask || !W_q || !b_q || !W_cq || !b_cq || !w_ca || !b_ca || !ins_out || !attn_out || B <= 0 ||
      T <= 0 || D <= 0 || n_steps <= 0)
    return GNNRAG_E_BADARG;
  if (n_steps > GNNRAG_MAX_INS) return GNNRAG_E_UNSUPPORTED;
  InsLinears ql;
  for (int s = 0; s < GNNRAG_MAX_INS; ++s) {
    ql.W[s] = s < n_steps ? W_q[s] : nullptr;
    ql.b[s] = s < n_steps ? b_q[s] : nullptr;
    if (s < n_steps && (!ql.W[s] || !ql.b[s])) return GNNRAG_E_BADARG;
  }
  // one question's working set lives in one CU's LDS: every T * D <= 16384 with D <= 2048 fits at GNNRAG_MAX_INS steps
  if ((int64_t)T * D > (int64_t)(kInsLdsBytes / sizeof(float))) return GNNRAG_E_UNSUPPORTED;
  const size_t lds = ins_lds_floats(T, D, n_steps) * sizeof(float);
  if (lds > kInsLdsBytes) return GNNRAG_E_UNSUPPORTED;
  if (train && (!tr.reserve || reserve_bytes < gnnrag_instructions_reserve_bytes(B, T, D, n_steps)))
    return GNNRAG_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (!train)
    return ins_launch<false, false>(hidden, node, mask, r_in, ql, W_cq, b_cq, w_ca, b_ca, B, T, D, n_steps, ins_out,
                                    attn_out, tr, lds, st);
  if (tr.m1 || tr.m2 || tr.m3)
    return ins_launch<true, true>(hidden, node, mask, r_in, ql, W_cq, b_cq, w_ca, b_ca, B, T, D, n_steps, ins_out,
                                  attn_out, tr, lds, st);
  return ins_launch<true, false>(hidden, node, mask, r_in, ql, W_cq, b_cq, w_ca, b_ca, B, T, D, n_steps, ins_out,
                                 attn_out, tr, lds, st);
}

extern "C" int gnnrag_instructions(const float* hidden, const float* node, const float* mask, const float* r_in,
                                   const float* const* W_q, const float* const* b_q, const float* W_cq, const float* b_cq,
                                   const float* w_ca, const float* b_ca, int32_t B, int32_t T, int32_t D, int32_t n_steps,
                                   float* ins_out, float* attn_out, gnnrag_stream_t stream) {
  const InsTrain tr = {nullptr, nullptr, nullptr, nullptr};
  return ins_run(hidden, node, mask, r_in, W_q, b_q, W_cq, b_cq, w_ca, b_ca, B, T, D, n_steps, ins_out, attn_out, tr, false,
                 0, stream);
}

extern "C" size_t gnnrag_instructions_reserve_bytes(int32_t B, int32_t T, int32_t D, int32_t n_steps) {
  if (B <= 0 || T <= 0 || D <= 0 || n_steps <= 0 || n_steps > GNNRAG_MAX_INS) return 0;
  return (size_t)n_steps * B * 2 * D * sizeof(float);
}

extern "C" int gnnrag_instructions_train(const float* hidden, const float* node, const float* mask, const float* r_in,
                                         const float* const* W_q, const float* const* b_q, const float* W_cq,
                                         const float* b_cq, const float* w_ca, const float* b_ca, const float* drop_node,
                                         const float* drop_cat, const float* drop_tok, int32_t B, int32_t T, int32_t D,
                                         int32_t n_steps, float* ins_out, float* attn_out, void* reserve,
                                         size_t reserve_bytes, gnnrag_stream_t stream) {
  const InsTrain tr = {drop_node, drop_cat, drop_tok, (float*)reserve};
  return ins_run(hidden, node, mask, r_in, W_q, b_q, W_cq, b_cq, w_ca, b_ca, B, T, D, n_steps, ins_out, attn_out, tr, true,
                 reserve_bytes, stream);
}
