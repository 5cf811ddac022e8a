// Backward of the question encoder's LSTM (lstm.hip; torch.nn.LSTM semantics, gate order i, f, g, o): what training
// (Trainer_KBQA.train_epoch, train_model.py:209-233) derives for nn.LSTM(word_dim, entity_dim, batch_first=True) of
// lstm_encoder.py:27-36.  The training forward (k_lstm<R, true>) left the activated gates act [B,T,4H] and the cell
// states cs [B,T,H] in the caller's reserve.
//
//   recurrent part (k_lstm_bwd): one workgroup per sequence walks t = T-1 .. 0.  Thread j < H keeps dc_j in a register:
//     dh = g_out[b,t] + dh_rec           (dh_rec starts as g_hn)         dc += dh o (1 - tanh^2 c_t)   (dc starts as g_cn)
//     dG_i = dc g i (1-i)   dG_f = dc c_{t-1} f (1-f)   dG_g = dc i (1-g^2)   dG_o = dh tanh(c_t) o (1-o)   dc *= f
//   dG goes to the workspace ([B,T,4H], the operand of the dense parts) and to LDS; after a barrier thread (q, k) of the
//   4H forms the partial sum of gate block q, sum_jj W_hh[q H + jj][k] dG[q H + jj] in ascending jj - W_hh as it lies,
//   coalesced over k - and thread k adds the four partial sums in block order: dh_rec[k].  One fixed order, no atomics.
//   The same kernel lays h_prev [B,T,Hp] (h0 or 0 at t = 0, else out[b,t-1]; Hp = H rounded up to 4, zero padded) next
//   to dG.
//   dense parts over M = B T rows: dX = dG W_ih (gnnrag_linear on the [E,4H] transposed copy, exact fp32),
//   dW_ih = dG^T X and dW_hh = dG^T h_prev (gnnrag_gemm_tn; the padded columns are dropped by a copy), db = column sums
//   of dG (rows in 8 slices, slices added in order).
// Latency-bound at encoder shapes (a chain of T small steps per sequence): no share of peak is claimed.
#include "gnnrag_common.h"

namespace gnnrag {

struct LstmBwdArgs {
  const float* w_hh;     // [4H, H] as the module holds it
  const float* h0;       // [B, H] or null
  const float* c0;       // [B, H] or null
  const float* out;      // [B, T, H]
  const float* act;      // [B, T, 4H]
  const float* cs;       // [B, T, H]
  const float* g_out;    // [B, T, H] or null
  const float* g_hn;     // [B, H] or null
  const float* g_cn;     // [B, H] or null
  float* dG;             // [B, T, 4H]
  float* hp;             // [B, T, Hp]
  float* dh0;            // [B, H] or null
  float* dc0;            // [B, H] or null
  int32_t B, T, H, Hp;
};

__global__ __launch_bounds__(1024) void k_lstm_bwd(const LstmBwdArgs a) {
  __shared__ float s_dg[1024];
  __shared__ float s_part[1024];
  const int H = a.H, T = a.T, G = 4 * H, Hp = a.Hp;
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  // h_prev rows of this sequence (outside the chain)
  for (int idx = tid; idx < T * Hp; idx += blockDim.x) {
    const int t = idx / Hp, j = idx - t * Hp;
    float v = 0.f;
    if (j < H) v = t > 0 ? a.out[(b * T + t - 1) * H + j] : (a.h0 ? a.h0[b * H + j] : 0.f);
    a.hp[(b * T + t) * Hp + j] = v;
  }
  const bool own = tid < H;
  const int j = own ? tid : 0;
  const int q = tid < G ? tid / H : 0, k = tid < G ? tid - q * H : 0;
  const float* __restrict__ w = a.w_hh + (size_t)q * H * H + k;
  float dc = (own && a.g_cn) ? a.g_cn[b * H + j] : 0.f;
  float dh_rec = (own && a.g_hn) ? a.g_hn[b * H + j] : 0.f;
  // operands of step t are loaded one step ahead
  float ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, tc = 0.f, go = 0.f;        // tc = tanh(c_t)
  if (own) {
    const size_t row = b * T + (T - 1);
    const float* ar = a.act + row * G;
    ig = ar[j]; fg = ar[H + j]; gg = ar[2 * H + j]; og = ar[3 * H + j];
    tc = tanhf(a.cs[row * H + j]);
    go = a.g_out ? a.g_out[row * H + j] : 0.f;
  }
  for (int t = T - 1; t >= 0; --t) {
    if (own) {
      const size_t row = b * T + t;
      const float cprev = t > 0 ? a.cs[(row - 1) * H + j] : (a.c0 ? a.c0[b * H + j] : 0.f);
      const float dh = go + dh_rec;
      dc = fmaf(dh * og, 1.f - tc * tc, dc);
      const float d_i = dc * gg * (ig * (1.f - ig));
      const float d_f = dc * cprev * (fg * (1.f - fg));
      const float d_g = dc * ig * (1.f - gg * gg);
      const float d_o = dh * tc * (og * (1.f - og));
      dc *= fg;
      float* gr = a.dG + row * G;
      gr[j] = d_i; gr[H + j] = d_f; gr[2 * H + j] = d_g; gr[3 * H + j] = d_o;
      s_dg[j] = d_i; s_dg[H + j] = d_f; s_dg[2 * H + j] = d_g; s_dg[3 * H + j] = d_o;
      if (t > 0) {
        const float* ar = a.act + (row - 1) * G;
        ig = ar[j]; fg = ar[H + j]; gg = ar[2 * H + j]; og = ar[3 * H + j];
        tc = tanhf(cprev);
        go = a.g_out ? a.g_out[(row - 1) * H + j] : 0.f;
      }
    }
    __syncthreads();
    if (tid < G) {
      const float* __restrict__ d = s_dg + q * H;
      float p = 0.f;
#pragma unroll 8
      for (int jj = 0; jj < H; ++jj) p = fmaf(w[(size_t)jj * H], d[jj], p);
      s_part[tid] = p;
    }
    __syncthreads();
    if (own) dh_rec = ((s_part[j] + s_part[H + j]) + s_part[2 * H + j]) + s_part[3 * H + j];
  }
  if (own) {
    if (a.dh0) a.dh0[b * H + j] = dh_rec;
    if (a.dc0) a.dc0[b * H + j] = dc;
  }
}

struct LstmBwdLayout {
  size_t dG, hp, wih_t, cpad, tn, tn_bytes, total;
  int32_t Hp;
};

static LstmBwdLayout lstm_bwd_layout(int32_t B, int32_t T, int32_t E, int32_t H) {
  LstmBwdLayout l;
  const size_t M = (size_t)B * T, G = 4 * (size_t)H;
  l.Hp = (H + 3) / 4 * 4;
  Carve cv;
  l.dG = cv.take(M * G * sizeof(float));
  l.hp = cv.take(M * l.Hp * sizeof(float));
  l.wih_t = cv.take((size_t)E * G * sizeof(float));
  l.cpad = cv.take(G * l.Hp * sizeof(float));
  const size_t t1 = gnnrag_gemm_tn_workspace_bytes((int64_t)M, (int32_t)G, E);
  const size_t t2 = gnnrag_gemm_tn_workspace_bytes((int64_t)M, (int32_t)G, l.Hp);
  l.tn_bytes = t1 > t2 ? t1 : t2;
  l.tn = cv.take(l.tn_bytes);
  l.total = cv.off;
  return l;
}

}  // namespace gnnrag

using namespace gnnrag;

extern "C" size_t gnnrag_lstm_backward_workspace_bytes(int32_t B, int32_t T, int32_t E, int32_t H) {
  if (B <= 0 || T <= 0 || E <= 0 || H <= 0 || 4 * H > 1024) return 0;
  return lstm_bwd_layout(B, T, E, H).total;
}

extern "C" int gnnrag_lstm_backward(const float* x, const float* w_ih, const float* w_hh, const float* h0,
                                    const float* c0, const float* out, const void* reserve, size_t reserve_bytes,
                                    const float* g_out, const float* g_hn, const float* g_cn, float* dx, float* dw_ih,
                                    float* dw_hh, float* db, float* dh0, float* dc0, int32_t B, int32_t T, int32_t E,
                                    int32_t H, void* workspace, size_t workspace_bytes, gnnrag_stream_t stream_) {
  if (!x || !w_ih || !w_hh || !out || !dw_ih || !dw_hh || B <= 0 || T <= 0 || E <= 0 || H <= 0) return GNNRAG_E_BADARG;
  if (4 * H > 1024 || (E & 3)) return GNNRAG_E_UNSUPPORTED;
  if (!aligned16(x, dw_ih, workspace)) return GNNRAG_E_UNSUPPORTED;   // gemm_tn
  if (!reserve || reserve_bytes < gnnrag_lstm_reserve_bytes(B, T, H)) return GNNRAG_E_WORKSPACE;
  const LstmBwdLayout l = lstm_bwd_layout(B, T, E, H);
  if (!workspace || workspace_bytes < l.total) return GNNRAG_E_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int G = 4 * H;
  const int64_t M = (int64_t)B * T;
  char* ws = (char*)workspace;
  float* dG = (float*)(ws + l.dG);
  float* hp = (float*)(ws + l.hp);
  float* wih_t = (float*)(ws + l.wih_t);
  float* cpad = (float*)(ws + l.cpad);
  LstmBwdArgs a;
  a.w_hh = w_hh; a.h0 = h0; a.c0 = c0; a.out = out;
  a.act = (const float*)reserve; a.cs = (const float*)reserve + (size_t)M * G;
  a.g_out = g_out; a.g_hn = g_hn; a.g_cn = g_cn; a.dG = dG; a.hp = hp; a.dh0 = dh0; a.dc0 = dc0;
  a.B = B; a.T = T; a.H = H; a.Hp = l.Hp;
  hipLaunchKernelGGL(k_lstm_bwd, dim3(B), dim3((G + 63) / 64 * 64), 0, stream, a);
  GNNRAG_LAUNCH_CHECK();
  GNNRAG_RC(gnnrag_gemm_tn(dG, x, M, G, E, dw_ih, ws + l.tn, l.tn_bytes, stream_));
  GNNRAG_RC(gemm_tn_unpadded(dG, hp, M, G, l.Hp, G, H, dw_hh, cpad, ws + l.tn, l.tn_bytes, stream));
  if (dx) {
    GNNRAG_RC(transpose_launch(w_ih, wih_t, G, E, stream));
    GNNRAG_RC(gnnrag_linear(dG, M, G, wih_t, nullptr, nullptr, 0, 0, dx, E, GNNRAG_MATH_FP32, stream_));
  }
  if (db) {
    ColsumJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    jobs.src[0] = dG; jobs.dst[0] = db; jobs.rows[0] = M; jobs.ld[0] = G; jobs.cols = G;
    GNNRAG_RC(colsum_launch(jobs, 1, stream));
  }
  return 0;
}
