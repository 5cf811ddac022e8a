// What follows the last `dist` of a training forward (gnn/models/ReaRev/rearev.py:227-243, gnn/models/NSM/nsm.py:242-250):
// the KL loss with its backward, and the batch metrics H@1 / F1 that get_eval_metric computes on every training step.
//
// Loss (base_model.py:193-199 under calc_loss_label, rearev.py:156-160).  Per question b:
//   len_b = sum_n teacher (0 -> 1)     t = teacher / len_b     l_b = label_valid_b sum_n (t > 0 ? t (log t - log(pred + 1e-8)) : 0)
//   loss  = (sum_b l_b) / B            d_pred = -g label_valid_b t / (pred + 1e-8) / B
//
//   k_kl_fwd   one workgroup per question: len_b, then l_b, each in one fixed order (thread-strided sums, then
//              block_sum).  len_b goes to the caller's reserve, l_b to the workspace.
//   k_kl_sum   one thread adds the l_b in ascending b and divides by B.
//   k_kl_bwd   one streaming pass; a thread owns the columns 4 c .. 4 c + 3 of a row, as one float4 where N % 4 == 0 and the
//              bases are 16-byte aligned, else element by element: the same values either way.  EVERY element is written.
//
// Metrics (base_model.py:217-298: calc_h1, calc_f1_new, f1_and_hits).  k_train_metrics, one workgroup per question:
//   argmax over all N slots (lowest slot among equal maxima), h1 = answer[argmax] > 1e-10;
//   eligible = not a seed and not the pad entity; n_ans = eligible slots with answer > 0 (before the probability filter);
//   kept = eligible and not ((double)p < ignore_prob), ordered by topp_keys.h; the cut = the shortest prefix whose sequential
//   fp64 sum exceeds eps (or all kept); correct = retrieved slots with answer > 0; F1 in double as f1_and_hits writes it,
//   rounded to fp32 once, 0 where h1 == 0.
// Integer / ordering work and one correctly rounded double expression: bit-exact against tests/train_tail_oracle.py.
// No atomics, no allocation, nothing waits for the stream; results of a question do not depend on the batch around it.
#include "gnnrag_common.h"
#include "topp_keys.h"

namespace gnnrag {

constexpr int kKlBwdThreads = 256;
constexpr int kKlBwdGrid = 2048;         // 256 CUs x 8 workgroups: the cap of the backward's grid (grid-strided beyond)
constexpr float kKlEps = 1e-8f;          // base_model.py:197

__global__ __launch_bounds__(1024) void k_kl_fwd(const float* __restrict__ pred, const float* __restrict__ teacher,
                                                 const float* __restrict__ label_valid, int N, float* __restrict__ len_out,
                                                 float* __restrict__ l_out) {
  __shared__ float red[16];
  __shared__ float bcast;
  const size_t off = (size_t)blockIdx.x * N;
  const float* __restrict__ p = pred + off;
  const float* __restrict__ t = teacher + off;
  float s = 0.f;
  for (int i = threadIdx.x; i < N; i += 1024) s += t[i];
  float len = block_sum(s, red, &bcast);
  if (len == 0.f) len = 1.f;                                               // base_model.py:195
  float acc = 0.f;
  for (int i = threadIdx.x; i < N; i += 1024) {
    const float th = __fdiv_rn(t[i], len);
    if (th > 0.f) acc += th * (logf(th) - logf(p[i] + kKlEps));            // KLDivLoss: a zero target contributes 0
  }
  const float l = block_sum(acc, red, &bcast);
  if (threadIdx.x == 0) {
    len_out[blockIdx.x] = len;
    l_out[blockIdx.x] = label_valid[blockIdx.x] * l;
  }
}

__global__ void k_kl_sum(const float* __restrict__ l, int B, float* __restrict__ loss) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += l[b];
    loss[0] = __fdiv_rn(s, (float)B);
  }
}

template <bool VEC>
__global__ __launch_bounds__(kKlBwdThreads) void k_kl_bwd(const float* __restrict__ g_loss, const float* __restrict__ pred,
                                                          const float* __restrict__ teacher,
                                                          const float* __restrict__ label_valid,
                                                          const float* __restrict__ len, int B, int N,
                                                          float* __restrict__ d_pred) {
  const int C = (N + 3) >> 2;                                              // float4 columns of a row
  const int64_t total = (int64_t)B * C;
  const float g = g_loss[0], fB = (float)B;
  const int64_t step = (int64_t)gridDim.x * kKlBwdThreads;
  for (int64_t i = (int64_t)blockIdx.x * kKlBwdThreads + threadIdx.x; i < total; i += step) {
    const int b = (int)(i / C), c = (int)(i - (int64_t)b * C);
    const float lv = label_valid[b], ln = len[b];
    const float coef = __fdiv_rn(-g * lv, fB);
    const size_t base = (size_t)b * N;
    f32x4 pv = {1.f, 1.f, 1.f, 1.f}, tv = {0.f, 0.f, 0.f, 0.f}, d;
    if (VEC) {
      pv = ((const f32x4*)(pred + base))[c];
      tv = ((const f32x4*)(teacher + base))[c];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * c + e < N) {
          pv[e] = pred[base + 4 * c + e];
          tv[e] = teacher[base + 4 * c + e];
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float th = __fdiv_rn(tv[e], ln);
      d[e] = (th > 0.f && lv != 0.f) ? coef * __fdiv_rn(th, pv[e] + kKlEps) : 0.f;
    }
    if (VEC) {
      ((f32x4*)(d_pred + base))[c] = d;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * c + e < N) d_pred[base + 4 * c + e] = d[e];
    }
  }
}

// All LDS of this kernel is dynamic (a kernel with static LDS cannot be given the CU's whole 160 KB as dynamic LDS):
// keys [M], then 16 x (float, int) of the argmax, 16 ints per counter, and the broadcasts.
constexpr int kTmTailBytes = 512;

template <int LOG2>
__global__ __launch_bounds__(1024) void k_train_metrics(const float* __restrict__ pred, const float* __restrict__ answer,
                                                        const float* __restrict__ seed,
                                                        const int64_t* __restrict__ local_entity, int64_t pad_id, int N,
                                                        double ignore_prob, double eps, int32_t* __restrict__ out_pred,
                                                        float* __restrict__ out_h1, float* __restrict__ out_f1,
                                                        int32_t* __restrict__ out_cnt) {
  constexpr int M = 1 << LOG2;
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];   // [M] + the tail
  float* s_val = reinterpret_cast<float*>(keys + M);                           // [16]
  int* s_idx = reinterpret_cast<int*>(s_val + 16);                             // [16]
  int* s_ans = s_idx + 16;                                                     // [16]
  int* s_kept = s_ans + 16;                                                    // [16]
  int* s_cor = s_kept + 16;                                                    // [16]
  int* s_cut = s_cor + 16;                                                     // [1]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t off = (size_t)b * N;
  const float* __restrict__ p = pred + off;
  const float* __restrict__ ans = answer + off;
  const float* __restrict__ sd = seed + off;
  const int64_t* __restrict__ le = local_entity + off;

  // one pass: the argmax candidate of this thread, its counts, its keys
  float best = 0.f;
  int best_i = N;                                   // N = nothing seen yet
  int n_ans = 0, kept = 0;
  for (int j = tid; j < M; j += 1024) {
    unsigned long long k = kToppNone;
    if (j < N) {
      const float v = p[j];
      if (best_i == N || v > best) {                // ascending j: an equal later value does not replace
        best = v;
        best_i = j;
      }
      const bool eligible = !(sd[j] > 0.f) && le[j] != pad_id;             // base_model.py:270-274
      if (eligible && ans[j] > 0.f) ++n_ans;                               // :275-276, before the probability filter
      k = topp_key(v, eligible, ignore_prob, j);                           // :277-279
      if (k != kToppNone) ++kept;
    }
    keys[j] = k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(best_i, o, 64);
    if (oi != N && (best_i == N || ov > best || (ov == best && oi < best_i))) {
      best = ov;
      best_i = oi;
    }
  }
  n_ans = wave_sum(n_ans);
  kept = wave_sum(kept);
  if (lane == 0) {
    s_val[wave] = best;
    s_idx[wave] = best_i;
    s_ans[wave] = n_ans;
    s_kept[wave] = kept;
  }
  __syncthreads();                                   // also: the keys are written
  topp_bitonic_sort(keys, M);
  if (tid == 0) {
    int cut = 0;
    double tp = 0.0;
    for (int j = 0; j < N; ++j) {
      const unsigned long long k = keys[j];
      if (k == kToppNone) break;
      tp += (double)topp_key_prob(k);                                      // base_model.py:229
      ++cut;
      if (tp > eps) break;                                                 // :232-233
    }
    *s_cut = cut;
  }
  __syncthreads();
  const int n_ret = *s_cut;
  int cor = 0;
  for (int j = tid; j < n_ret; j += 1024)
    if (ans[topp_key_slot(keys[j])] > 0.f) ++cor;                          // :230: the slot's own answer flag
  cor = wave_sum(cor);
  if (lane == 0) s_cor[wave] = cor;
  __syncthreads();
  if (tid == 0) {
    int a_i = N, n_a = 0, n_k = 0, correct = 0;
    float a_v = 0.f;
    for (int w = 0; w < 16; ++w) {
      const int oi = s_idx[w];
      const float ov = s_val[w];
      if (oi != N && (a_i == N || ov > a_v || (ov == a_v && oi < a_i))) {
        a_v = ov;
        a_i = oi;
      }
      n_a += s_ans[w];
      n_k += s_kept[w];
      correct += s_cor[w];
    }
    const bool h1 = ans[a_i] > 1e-10f;                                     // calc_h1 with VERY_SMALL_NUMBER
    double f1;
    if (n_a == 0) {
      f1 = n_ret == 0 ? 1.0 : 0.0;                                         // base_model.py:234-238
    } else if (n_ret == 0) {
      f1 = 0.0;                                                            // :241-242
    } else {
      const double pr = (double)correct / (double)n_ret, rc = (double)correct / (double)n_a;
      f1 = (pr != 0.0 && rc != 0.0) ? 2.0 / (1.0 / pr + 1.0 / rc) : 0.0;   // :244-245
    }
    out_pred[b] = a_i;
    out_h1[b] = h1 ? 1.f : 0.f;
    out_f1[b] = h1 ? (float)f1 : 0.f;                                      // calc_f1_new:259-262
    out_cnt[4 * b] = n_k;
    out_cnt[4 * b + 1] = n_ret;
    out_cnt[4 * b + 2] = correct;
    out_cnt[4 * b + 3] = n_a;
  }
}

}  // namespace gnnrag

using namespace gnnrag;

extern "C" size_t gnnrag_kl_loss_workspace_bytes(int32_t B) {
  if (B <= 0) return 0;
  return align_up((size_t)B * sizeof(float), 256);
}

extern "C" int gnnrag_kl_loss_train(const float* pred, const float* teacher, const float* label_valid, int32_t B, int32_t N,
                                    float* loss, float* reserve, void* workspace, size_t workspace_bytes,
                                    gnnrag_stream_t stream_) {
  if (!pred || !teacher || !label_valid || !loss || !reserve || B <= 0 || N <= 0) return GNNRAG_E_BADARG;
  if (!workspace || workspace_bytes < gnnrag_kl_loss_workspace_bytes(B)) return GNNRAG_E_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  float* l = (float*)workspace;
  hipLaunchKernelGGL(k_kl_fwd, dim3(B), dim3(1024), 0, stream, pred, teacher, label_valid, N, reserve, l);
  GNNRAG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_kl_sum, dim3(1), dim3(64), 0, stream, l, B, loss);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnnrag_kl_loss_backward(const float* g_loss, const float* pred, const float* teacher, const float* label_valid,
                                       const float* reserve, int32_t B, int32_t N, float* d_pred, gnnrag_stream_t stream_) {
  if (!g_loss || !pred || !teacher || !label_valid || !reserve || !d_pred || B <= 0 || N <= 0) return GNNRAG_E_BADARG;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t total = (int64_t)B * ((N + 3) / 4);
  const int64_t blocks = (total + kKlBwdThreads - 1) / kKlBwdThreads;
  const int grid = (int)(blocks < kKlBwdGrid ? blocks : kKlBwdGrid);
  const bool vec = (N & 3) == 0 && aligned16(pred, teacher, d_pred);
  if (vec)
    hipLaunchKernelGGL(k_kl_bwd<true>, dim3(grid), dim3(kKlBwdThreads), 0, stream, g_loss, pred, teacher, label_valid,
                       reserve, B, N, d_pred);
  else
    hipLaunchKernelGGL(k_kl_bwd<false>, dim3(grid), dim3(kKlBwdThreads), 0, stream, g_loss, pred, teacher, label_valid,
                       reserve, B, N, d_pred);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnnrag_train_metrics(const float* pred, const float* answer, const float* seed, const int64_t* local_entity,
                                    int64_t pad_id, double eps, int32_t B, int32_t N, int32_t* out_pred, float* out_h1,
                                    float* out_f1, int32_t* out_cnt, gnnrag_stream_t stream_) {
  if (!pred || !answer || !seed || !local_entity || !out_pred || !out_h1 || !out_f1 || !out_cnt || B <= 0 || N <= 0)
    return GNNRAG_E_BADARG;
  if (N > GNNRAG_TRAIN_METRICS_MAX_N) return GNNRAG_E_UNSUPPORTED;        // 16384 keys x 8 B = 128 KB of LDS
  hipStream_t stream = (hipStream_t)stream_;
  const double ignore_prob = (1.0 - eps) / (double)N;                      // base_model.py:254, in double like Python
  int log2 = 1;
  while ((1 << log2) < N) ++log2;
  const size_t lds = ((size_t)1 << log2) * sizeof(unsigned long long) + kTmTailBytes;
#define GNNRAG_TM(L)                                                                                               \
  case L: {                                                                                                        \
    static DeviceMask cap_raised;                                                                                  \
    if (lds > 64 * 1024) {                                                                                         \
      const int rc_ = raise_lds_cap(k_train_metrics<L>, cap_raised);                                               \
      if (rc_) return rc_;                                                                                         \
    }                                                                                                              \
    hipLaunchKernelGGL(k_train_metrics<L>, dim3(B), dim3(1024), lds, stream, pred, answer, seed, local_entity,     \
                       pad_id, N, ignore_prob, eps, out_pred, out_h1, out_f1, out_cnt);                            \
  } break;
  switch (log2) {
    GNNRAG_TM(1) GNNRAG_TM(2) GNNRAG_TM(3) GNNRAG_TM(4) GNNRAG_TM(5) GNNRAG_TM(6) GNNRAG_TM(7)
    GNNRAG_TM(8) GNNRAG_TM(9) GNNRAG_TM(10) GNNRAG_TM(11) GNNRAG_TM(12) GNNRAG_TM(13) GNNRAG_TM(14)
    default: return GNNRAG_E_UNSUPPORTED;
  }
#undef GNNRAG_TM
  GNNRAG_LAUNCH_CHECK();
  return 0;
}
