// Backward of instruction generation (instruction.hip, gnnrag_instructions_train): what training
// (Trainer_KBQA.train_epoch, train_model.py:209-233) derives for BaseInstruction.get_instruction
// (gnn/modules/question_encoding/base_encoder.py:82-101), all steps of a question in one launch.  The training forward
// left q_s and cq of every step in the caller's reserve [n, B, 2 D]; r before step s is r_in (or zeros) or ins[s - 1], z is
// rebuilt from r, q_s and m2, a is attn[s].  With dr' = g_ins[s] + carry, for s = n-1 .. 0:
//   da_t  = dr' . h[t,:] + g_attn[s,t]           dca_t = a_t (da_t - sum_u a_u da_u)
//   dh[t,d] += a_t dr'[d] + dca_t w_ca[d] cq[d] m3[t,d]
//   u[d]  = sum_t dca_t h[t,d] m3[t,d]           dcq = w_ca * u          (cq * u: the rows of dw_ca)
//   dz    = (W_cq^T dcq) * m2                    carry = dz0 - dz2 + dz3 * q        dq = dz1 + dz2 + dz3 * r
//   dnode += (W_q[s]^T dq) * m1
// and dr_in = carry after step 0.  The mask addition passes the gradient with derivative 1, as autograd does (a question of
// padding only has a = 1/T and a non-zero dca); b_ca does not move the softmax: db_ca is written as zero.
//
//   chain (k_ins_bwd): one workgroup per question, its token states in LDS as in the forward.  da_t: a wave per token,
//   lanes stride over d, the forward's __shfl_xor tree; the softmax inner sum: lanes stride over t, the same tree (every
//   wave derives the same bits); u[d] and nothing else sums over t: ascending t, thread d.  dh[t,d] belongs to thread
//   (t D + d) mod blockDim in every step: the first step walked writes it, the later ones read, add and write - no atomics.
//   W_cq^T dcq and W_q[s]^T dq: thread k owns output k and sums over the rows in ascending order, W as it lies, coalesced
//   over k (the pattern of dh_{t-1} in lstm_bwd.hip).
//   The kernel leaves per (step, question) rows in the workspace: dcq, dq, n_s = node * m1 (each [n B, Dp], Dp = D rounded
//   up to 4, zero padded), z [n B, 4 D] and cq * u [n B, D].
//   dense parts: dW_cq = dcq^T z (one gnnrag_gemm_tn over M = n B rows), dW_q[s] = dq[s]^T n_s (one per step); the padded
//   rows / columns are dropped by a copy.  db_cq, db_q[s], dw_ca: column sums, rows in 8 slices, slices added in order (one
//   launch for all of them).
// Latency-bound at encoder shapes (a chain of n dependent steps per question): no share of peak is claimed.
#include "gnnrag_common.h"

#ifndef GNNRAG_INS_BWD_THREADS
#define GNNRAG_INS_BWD_THREADS 1024  // a multiple of 64; decides who owns a dh element, never a summation order
#endif

namespace gnnrag {

constexpr size_t kInsBwdLdsBytes = 160 * 1024;

// floats of LDS one question needs: token states (rounded up to 4), twelve [D] vectors (r, q, cq, dr', carry, u -> dcq,
// dq, dnode and the four blocks of dz) and three [T] vectors (a, da, dca)
static inline size_t ins_bwd_lds_floats(int64_t T, int64_t D) { return (size_t)((T * D + 3) / 4 * 4 + 12 * D + 3 * T); }

struct InsBwdArgs {
  const float* hidden;            // [B, T, D]
  const float* node;              // [B, D]
  const float* r_in;              // [B, D] or null
  const float* Wq[GNNRAG_MAX_INS];  // [D, D]
  const float* W_cq;              // [D, 4D]
  const float* w_ca;              // [D]
  const float* m1;                // [n, B, D] or null
  const float* m2;                // [n, B, 4D] or null
  const float* m3;                // [n, B, T, D] or null
  const float* ins;               // [n, B, D]
  const float* attn;              // [n, B, T]
  const float* reserve;           // [n, B, 2D]
  const float* g_ins;             // [n, B, D] or null
  const float* g_attn;            // [n, B, T] or null
  float* dhidden;                 // [B, T, D] or null
  float* dnode;                   // [B, D] or null
  float* dr_in;                   // [B, D] or null
  float* w_dcq;                   // [n B, Dp]
  float* w_dq;                    // [n B, Dp]
  float* w_ns;                    // [n B, Dp]
  float* w_z;                     // [n B, 4D]
  float* w_cqu;                   // [n B, D]
  int32_t B, T, D, Dp, n;
};

__global__ __launch_bounds__(1024) void k_ins_bwd(const InsBwdArgs g) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int T = g.T, D = g.D, Dp = g.Dp, B = g.B, TD = T * D;
  float* hid = smem;                       // [T, D]
  float* rv = hid + (TD + 3) / 4 * 4;      // [D]  r before the step
  float* qv = rv + D;                      // [D]  q_s
  float* cqv = qv + D;                     // [D]  cq
  float* drp = cqv + D;                    // [D]  dr' = g_ins[s] + carry
  float* car = drp + D;                    // [D]  carry
  float* dcq = car + D;                    // [D]
  float* dqv = dcq + D;                    // [D]
  float* dnv = dqv + D;                    // [D]  dnode of this question, summed over the steps
  float* dz = dnv + D;                     // [4D]
  float* av = dz + 4 * D;                  // [T]
  float* dav = av + T;                     // [T]
  float* dca = dav + T;                    // [T]
  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;

  const float* hb = g.hidden + (size_t)b * TD;
  if ((TD & 3) == 0 && ((uintptr_t)hb & 15) == 0) {
    const f32x4* src = (const f32x4*)hb;
    f32x4* dst = (f32x4*)hid;
    for (int i = tid; i < TD / 4; i += nthr) dst[i] = src[i];
  } else {
    for (int i = tid; i < TD; i += nthr) hid[i] = hb[i];
  }
  for (int d = tid; d < D; d += nthr) {
    car[d] = 0.f;
    dnv[d] = 0.f;
  }
  __syncthreads();

  float* dhb = g.dhidden ? g.dhidden + (size_t)b * TD : nullptr;
  for (int s = g.n - 1; s >= 0; --s) {
    const size_t row = (size_t)s * B + b;
    const float* rs = g.reserve + row * 2 * D;
    const float* m1 = g.m1 ? g.m1 + row * D : nullptr;
    const float* m2 = g.m2 ? g.m2 + row * 4 * D : nullptr;
    const float* m3 = g.m3 ? g.m3 + row * TD : nullptr;
    const float* rprev = s > 0 ? g.ins + ((size_t)(s - 1) * B + b) * D : (g.r_in ? g.r_in + (size_t)b * D : nullptr);
    // the step's vectors; the rows of z and n_s (operands of the dense parts)
    for (int d = tid; d < Dp; d += nthr) {
      float* nsr = g.w_ns + row * Dp;
      if (d < D) {
        const float r = rprev ? rprev[d] : 0.f, q = rs[d];
        rv[d] = r;
        qv[d] = q;
        cqv[d] = rs[D + d];
        drp[d] = (g.g_ins ? g.g_ins[row * D + d] : 0.f) + car[d];
        float z0 = r, z1 = q, z2 = q - r, z3 = q * r;
        if (m2) {
          z0 *= m2[d];
          z1 *= m2[D + d];
          z2 *= m2[2 * D + d];
          z3 *= m2[3 * D + d];
        }
        float* zr = g.w_z + row * 4 * D;
        zr[d] = z0;
        zr[D + d] = z1;
        zr[2 * D + d] = z2;
        zr[3 * D + d] = z3;
        const float x = g.node[(size_t)b * D + d];
        nsr[d] = m1 ? x * m1[d] : x;
      } else {
        nsr[d] = 0.f;
      }
    }
    for (int t = tid; t < T; t += nthr) av[t] = g.attn[row * T + t];
    __syncthreads();
    // da_t: a wave per token
    for (int t = wave; t < T; t += nw) {
      const float* h = hid + t * D;
      float acc = 0.f;
      for (int d = lane; d < D; d += 64) acc += drp[d] * h[d];
      acc = wave_sum(acc);
      if (lane == 0) dav[t] = acc + (g.g_attn ? g.g_attn[row * T + t] : 0.f);
    }
    __syncthreads();
    // dca_t = a_t (da_t - sum_u a_u da_u): every wave derives the same inner sum (same order), no hand-over
    float inner = 0.f;
    for (int t = lane; t < T; t += 64) inner += av[t] * dav[t];
    inner = wave_sum(inner);
    for (int t = tid; t < T; t += nthr) dca[t] = av[t] * (dav[t] - inner);
    __syncthreads();
    // dh: element i belongs to thread i mod nthr in every step
    if (dhb) {
      for (int i = tid; i < TD; i += nthr) {
        const int t = i / D, d = i - t * D;
        float w = g.w_ca[d] * cqv[d];
        if (m3) w *= m3[i];
        const float v = av[t] * drp[d] + dca[t] * w;
        dhb[i] = s == g.n - 1 ? v : dhb[i] + v;
      }
    }
    // u[d] = sum_t dca_t h[t,d] m3[t,d], ascending t
    for (int d = tid; d < Dp; d += nthr) {
      float* dr = g.w_dcq + row * Dp;
      if (d < D) {
        float u = 0.f;
        if (m3) {
          for (int t = 0; t < T; ++t) u += dca[t] * (hid[t * D + d] * m3[t * D + d]);
        } else {
          for (int t = 0; t < T; ++t) u += dca[t] * hid[t * D + d];
        }
        const float v = g.w_ca[d] * u;
        dcq[d] = v;
        dr[d] = v;
        g.w_cqu[row * D + d] = cqv[d] * u;
      } else {
        dr[d] = 0.f;
      }
    }
    __syncthreads();
    // dz = (W_cq^T dcq) * m2: thread k owns output k, rows in ascending order
    for (int k = tid; k < 4 * D; k += nthr) {
      const float* __restrict__ w = g.W_cq + k;
      float p = 0.f;
#pragma unroll 8
      for (int j = 0; j < D; ++j) p = fmaf(w[(size_t)j * 4 * D], dcq[j], p);
      dz[k] = m2 ? p * m2[k] : p;
    }
    __syncthreads();
    for (int d = tid; d < Dp; d += nthr) {
      float* dr = g.w_dq + row * Dp;
      if (d < D) {
        const float z0 = dz[d], z1 = dz[D + d], z2 = dz[2 * D + d], z3 = dz[3 * D + d];
        car[d] = (z0 - z2) + z3 * qv[d];
        const float v = (z1 + z2) + z3 * rv[d];
        dqv[d] = v;
        dr[d] = v;
      } else {
        dr[d] = 0.f;
      }
    }
    __syncthreads();
    // dnode += (W_q[s]^T dq) * m1 (off the chain: the next step does not read it)
    if (g.dnode) {
      const float* __restrict__ W = g.Wq[s];
      for (int k = tid; k < D; k += nthr) {
        float p = 0.f;
#pragma unroll 8
        for (int j = 0; j < D; ++j) p = fmaf(W[(size_t)j * D + k], dqv[j], p);
        dnv[k] += m1 ? p * m1[k] : p;
      }
    }
    // the next step rewrites rv .. drp and dqv only after its first barrier has been passed by every thread of this one:
    // dqv is read above and rewritten three barriers later, rv / qv / cqv / drp are no longer read here
  }
  __syncthreads();
  for (int d = tid; d < D; d += nthr) {
    if (g.dr_in) g.dr_in[(size_t)b * D + d] = car[d];
    if (g.dnode) g.dnode[(size_t)b * D + d] = dnv[d];
  }
}

struct InsBwdLayout {
  size_t dcq, dq, ns, z, cqu, cpad, tn, tn_bytes, total;
  int32_t Dp;
};

static InsBwdLayout ins_bwd_layout(int32_t B, int32_t D, int32_t n) {
  InsBwdLayout l;
  const size_t M = (size_t)n * B;
  l.Dp = (D + 3) / 4 * 4;
  Carve cv;
  l.dcq = cv.take(M * l.Dp * sizeof(float));
  l.dq = cv.take(M * l.Dp * sizeof(float));
  l.ns = cv.take(M * l.Dp * sizeof(float));
  l.z = cv.take(M * 4 * D * sizeof(float));
  l.cqu = cv.take(M * D * sizeof(float));
  l.cpad = cv.take((size_t)l.Dp * 4 * D * sizeof(float));                          // >= Dp * Dp
  const size_t t1 = gnnrag_gemm_tn_workspace_bytes((int64_t)M, l.Dp, 4 * D);
  const size_t t2 = gnnrag_gemm_tn_workspace_bytes((int64_t)B, l.Dp, l.Dp);
  l.tn_bytes = t1 > t2 ? t1 : t2;
  l.tn = cv.take(l.tn_bytes);
  l.total = cv.off;
  return l;
}

static bool ins_bwd_shape_ok(int32_t B, int32_t T, int32_t D, int32_t n) {
  if (B <= 0 || T <= 0 || D <= 0 || n <= 0 || n > GNNRAG_MAX_INS) return false;
  if ((int64_t)T * D > (int64_t)(kInsBwdLdsBytes / sizeof(float))) return false;
  return ins_bwd_lds_floats(T, D) * sizeof(float) <= kInsBwdLdsBytes;
}

}  // namespace gnnrag

using namespace gnnrag;

extern "C" size_t gnnrag_instructions_backward_workspace_bytes(int32_t B, int32_t T, int32_t D, int32_t n_steps) {
  if (!ins_bwd_shape_ok(B, T, D, n_steps)) return 0;
  return ins_bwd_layout(B, D, n_steps).total;
}

extern "C" int gnnrag_instructions_backward(const float* hidden, const float* node, const float* r_in,
                                            const float* const* W_q, const float* W_cq, const float* w_ca,
                                            const float* drop_node, const float* drop_cat, const float* drop_tok,
                                            const float* ins, const float* attn, const void* reserve, size_t reserve_bytes,
                                            const float* g_ins, const float* g_attn, float* dhidden, float* dnode,
                                            float* dr_in, float* const* dW_q, float* const* db_q, float* dW_cq,
                                            float* db_cq, float* dw_ca, float* db_ca, int32_t B, int32_t T, int32_t D,
                                            int32_t n_steps, void* workspace, size_t workspace_bytes,
                                            gnnrag_stream_t stream_) {
  if (!hidden || !node || !W_q || !W_cq || !w_ca || !ins || !attn || B <= 0 || T <= 0 || D <= 0 || n_steps <= 0)
    return GNNRAG_E_BADARG;
  if (!ins_bwd_shape_ok(B, T, D, n_steps)) return GNNRAG_E_UNSUPPORTED;
  for (int s = 0; s < n_steps; ++s)
    if (!W_q[s]) return GNNRAG_E_BADARG;
  if (!aligned16(workspace)) return GNNRAG_E_UNSUPPORTED;                         // gemm_tn
  if (!reserve || reserve_bytes < gnnrag_instructions_reserve_bytes(B, T, D, n_steps)) return GNNRAG_E_WORKSPACE;
  const InsBwdLayout l = ins_bwd_layout(B, D, n_steps);
  if (!workspace || workspace_bytes < l.total) return GNNRAG_E_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  const int Dp = l.Dp;
  const int64_t M = (int64_t)n_steps * B;
  InsBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.hidden = hidden; a.node = node; a.r_in = r_in; a.W_cq = W_cq; a.w_ca = w_ca;
  for (int s = 0; s < n_steps; ++s) a.Wq[s] = W_q[s];
  a.m1 = drop_node; a.m2 = drop_cat; a.m3 = drop_tok; a.ins = ins; a.attn = attn; a.reserve = (const float*)reserve;
  a.g_ins = g_ins; a.g_attn = g_attn; a.dhidden = dhidden; a.dnode = dnode; a.dr_in = dr_in;
  a.w_dcq = (float*)(ws + l.dcq); a.w_dq = (float*)(ws + l.dq); a.w_ns = (float*)(ws + l.ns);
  a.w_z = (float*)(ws + l.z); a.w_cqu = (float*)(ws + l.cqu);
  a.B = B; a.T = T; a.D = D; a.Dp = Dp; a.n = n_steps;
  const size_t lds = ins_bwd_lds_floats(T, D) * sizeof(float);
  if (lds > 64 * 1024) {
    static DeviceMask raised{0};
    GNNRAG_RC(raise_lds_cap(k_ins_bwd, raised));
  }
  hipLaunchKernelGGL(k_ins_bwd, dim3(B), dim3(GNNRAG_INS_BWD_THREADS), lds, stream, a);
  GNNRAG_LAUNCH_CHECK();

  float* cpad = (float*)(ws + l.cpad);
  if (dW_cq)
    GNNRAG_RC(gemm_tn_unpadded(a.w_dcq, a.w_z, M, Dp, 4 * D, D, 4 * D, dW_cq, cpad, ws + l.tn, l.tn_bytes, stream));
  for (int s = 0; dW_q && s < n_steps; ++s) {
    if (!dW_q[s]) continue;
    const float* dq = a.w_dq + (size_t)s * B * Dp;
    const float* ns = a.w_ns + (size_t)s * B * Dp;
    GNNRAG_RC(gemm_tn_unpadded(dq, ns, B, Dp, Dp, D, D, dW_q[s], cpad, ws + l.tn, l.tn_bytes, stream));
  }
  ColsumJobs jobs;
  memset(&jobs, 0, sizeof(jobs));
  jobs.cols = D;
  int nj = 0;
  if (db_cq) { jobs.src[nj] = a.w_dcq; jobs.dst[nj] = db_cq; jobs.rows[nj] = M; jobs.ld[nj] = Dp; ++nj; }
  if (dw_ca) { jobs.src[nj] = a.w_cqu; jobs.dst[nj] = dw_ca; jobs.rows[nj] = M; jobs.ld[nj] = D; ++nj; }
  for (int s = 0; db_q && s < n_steps; ++s) {
    if (!db_q[s]) continue;
    jobs.src[nj] = a.w_dq + (size_t)s * B * Dp; jobs.dst[nj] = db_q[s]; jobs.rows[nj] = B; jobs.ld[nj] = Dp; ++nj;
  }
  if (nj) GNNRAG_RC(colsum_launch(jobs, nj, stream));
  if (db_ca) GNNRAG_HIP(hipMemsetAsync(db_ca, 0, sizeof(float), stream));
  return 0;
}
