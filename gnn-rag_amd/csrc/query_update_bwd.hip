// Backward of the instruction update (query_update.hip, gnnrag_query_reform_train): what training
// (Trainer_KBQA.train_epoch, train_model.py:209-233) derives for the reforms of one ReaRev iteration
// (gnn/models/ReaRev/rearev.py:217-221 -> gnn/modules/query_update.py:26-44, Fusion :6-16).  For reform j and question b,
// with x = q_j[b], y = the retrieved seed rows (reserve), f = [x, y, x - y], a_r and the gate g (reserve), G = g_out[j][b]:
//   da_r = G g                      da_g = G (a_r - x) g (1 - g)            df = W_r^T da_r + W_g^T da_g
//   dx   = G (1 - g) + df[0:D] + df[2D:3D]                                  dy = df[D:2D] - df[2D:3D]
//   dW_r = sum_b da_r[b] (x) f[b]   dW_g = sum_b da_g[b] (x) f[b]           d_ent[b,n,:] = seed[b,n] sum_j dy_j[b]
// A reform whose g_out is NULL was not used: nothing is computed for it, it is left out of the sum over j, and the dq / dW
// the caller asked for anyway are written as zeros.
//
//   k_qr_bwd   one workgroup per (b, j).  da_r, da_g to LDS and, with f, to the workspace; the two transposed products:
//              thread k owns output k < 3 D and sums over the rows in ascending order, W as it lies, coalesced over k (the
//              pattern of instruction_bwd.hip); then dq and the row dy_j.
//   k_qr_dw    dW_r[j], dW_g[j] of every reform in one launch: thread (i, k) owns dW[i, k] and adds the questions in
//              ascending b.  M = B rows only (16 .. 64 in training): one launch of B-step chains replaces 2 n matrix-core
//              products of two launches each, needs no zero-padded rows for D % 4 != 0 and no alignment.
//   k_qr_dent  one streaming pass writes EVERY element of d_ent [B, N, D]: zero where seed[b,n] == 0, else
//              seed[b,n] * (dy_j[b] added in ascending j); float4 stores where D % 4 == 0 and the base is 16-byte aligned.
//              No memset, nothing is accumulated into what the buffer held.  The only memory-bound kernel here.
// No atomics, no allocation, nothing waits for the stream; one summation order: a second call gives the same bits, and dq /
// d_ent of a question do not depend on B or on its position in the batch.
// LDS: 5 D floats (da_r, da_g, df) - 80 KB at the forward's limit D = 4096, inside a CU's 160 KB: no tighter limit.
#include "gnnrag_common.h"

#ifndef GNNRAG_QR_BWD_THREADS
#define GNNRAG_QR_BWD_THREADS 512   // a multiple of 64; decides who owns an output, never a summation order
#endif

namespace gnnrag {

struct QrBwdArgs {
  const float* q[GNNRAG_MAX_REFORMS];      // [B, D]
  const float* Wr[GNNRAG_MAX_REFORMS];     // [D, 3D]
  const float* Wg[GNNRAG_MAX_REFORMS];     // [D, 3D]
  const float* g_out[GNNRAG_MAX_REFORMS];  // [B, D] or null (reform not used)
  float* dq[GNNRAG_MAX_REFORMS];           // [B, D] or null
  const float* y;                          // reserve [B, D]
  const float* ag;                         // reserve [n, B, 2D]
  float* w_da;                             // [n B, 2D]  (da_r, da_g)
  float* w_f;                              // [n B, 3D]
  float* w_dy;                             // [n B, D]
  int32_t B, D, need_df;
};

__global__ __launch_bounds__(GNNRAG_QR_BWD_THREADS) void k_qr_bwd(const QrBwdArgs g) {
  extern __shared__ float smem[];
  const int D = g.D, B = g.B, K = 3 * D;
  const int b = blockIdx.x, j = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  const size_t row = (size_t)j * B + b;
  const float* __restrict__ G = g.g_out[j];
  float* dq = g.dq[j] ? g.dq[j] + (size_t)b * D : nullptr;
  if (!G) {
    if (dq)
      for (int d = tid; d < D; d += nthr) dq[d] = 0.f;
    return;
  }
  G += (size_t)b * D;
  float* dar = smem;            // [D]
  float* dag = dar + D;         // [D]
  float* df = dag + D;          // [3D]
  const float* __restrict__ x = g.q[j] + (size_t)b * D;
  const float* __restrict__ yv = g.y + (size_t)b * D;
  const float* __restrict__ ag = g.ag + row * 2 * D;
  float* wda = g.w_da + row * 2 * D;
  float* wf = g.w_f + row * K;
  for (int d = tid; d < D; d += nthr) {
    const float xv = x[d], y = yv[d], ar = ag[d], gt = ag[D + d], Gv = G[d];
    const float a = Gv * gt;
    const float c = (Gv * (ar - xv)) * (gt * (1.f - gt));
    dar[d] = a;
    dag[d] = c;
    wda[d] = a;
    wda[D + d] = c;
    wf[d] = xv;
    wf[D + d] = y;
    wf[2 * D + d] = xv - y;
  }
  if (!g.need_df) return;
  __syncthreads();
  // df = W_r^T da_r + W_g^T da_g: thread k owns output k, rows in ascending order, two chains added at the end
  const float* __restrict__ Wr = g.Wr[j];
  const float* __restrict__ Wg = g.Wg[j];
  for (int k = tid; k < K; k += nthr) {
    const float* __restrict__ wr = Wr + k;
    const float* __restrict__ wg = Wg + k;
    float pr = 0.f, pg = 0.f;
#pragma unroll 8
    for (int i = 0; i < D; ++i) {
      pr = fmaf(wr[(size_t)i * K], dar[i], pr);
      pg = fmaf(wg[(size_t)i * K], dag[i], pg);
    }
    df[k] = pr + pg;
  }
  __syncthreads();
  float* wdy = g.w_dy + row * D;
  for (int d = tid; d < D; d += nthr) {
    const float gt = ag[D + d];
    if (dq) dq[d] = (G[d] * (1.f - gt) + df[d]) + df[2 * D + d];
    wdy[d] = df[D + d] - df[2 * D + d];
  }
}

// dW_r[j] / dW_g[j] [D, 3D] of every reform: blockIdx.z = 2 j + (0: r, 1: g), blockIdx.y = the row i, thread = the column k
struct QrDwArgs {
  float* dW[2 * GNNRAG_MAX_REFORMS];       // null: not wanted
  uint32_t active;                         // bit j: reform j has a g_out
  const float* w_da;
  const float* w_f;
  int32_t B, D;
};

__global__ __launch_bounds__(256) void k_qr_dw(const QrDwArgs g) {
  float* dW = g.dW[blockIdx.z];
  if (!dW) return;
  const int D = g.D, K = 3 * D, B = g.B;
  const int j = blockIdx.z >> 1, which = blockIdx.z & 1, i = blockIdx.y;
  const int k = blockIdx.x * 256 + (int)threadIdx.x;
  if (k >= K) return;
  float acc = 0.f;
  if ((g.active >> j) & 1u) {
    const float* __restrict__ da = g.w_da + (size_t)j * B * 2 * D + (size_t)which * D + i;
    const float* __restrict__ f = g.w_f + (size_t)j * B * K + k;
#pragma unroll 4
    for (int b = 0; b < B; ++b) acc = fmaf(da[(size_t)b * 2 * D], f[(size_t)b * K], acc);
  }
  dW[(size_t)i * K + k] = acc;
}

constexpr int kDentRows = 16;   // rows of d_ent per workgroup (4 per wave)

// VEC: float4 per lane (D % 4 == 0, 16-byte aligned base), else one float per lane
template <bool VEC>
__global__ __launch_bounds__(256) void k_qr_dent(const float* __restrict__ seed, const float* __restrict__ w_dy,
                                                 float* __restrict__ d_ent, int64_t rows, int N, int D, int B, int n,
                                                 uint32_t active) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t r0 = (int64_t)blockIdx.x * kDentRows;
#pragma unroll 1
  for (int u = wave; u < kDentRows; u += 4) {
    const int64_t r = r0 + u;                       // r = b N + node
    if (r >= rows) return;
    const float sv = seed[r];
    float* dst = d_ent + (size_t)r * D;
    if (VEC) {
      const int D4 = D >> 2;
      f32x4* dst4 = (f32x4*)dst;
      if (sv == 0.f) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int c = lane; c < D4; c += 64) dst4[c] = z;
      } else {
        const int64_t b = r / N;
        for (int c = lane; c < D4; c += 64) {
          f32x4 s = {0.f, 0.f, 0.f, 0.f};
          for (int j = 0; j < n; ++j)
            if ((active >> j) & 1u) s += ((const f32x4*)(w_dy + ((size_t)j * B + b) * D))[c];
          dst4[c] = sv * s;
        }
      }
    } else {
      if (sv == 0.f) {
        for (int c = lane; c < D; c += 64) dst[c] = 0.f;
      } else {
        const int64_t b = r / N;
        for (int c = lane; c < D; c += 64) {
          float s = 0.f;
          for (int j = 0; j < n; ++j)
            if ((active >> j) & 1u) s += w_dy[((size_t)j * B + b) * D + c];
          dst[c] = sv * s;
        }
      }
    }
  }
}

struct QrBwdLayout {
  size_t da, f, dy, total;
};

static QrBwdLayout qr_bwd_layout(int32_t B, int32_t D, int32_t n) {
  QrBwdLayout l;
  const size_t M = (size_t)n * B;
  Carve cv;
  l.da = cv.take(M * 2 * D * sizeof(float));
  l.f = cv.take(M * 3 * D * sizeof(float));
  l.dy = cv.take(M * D * sizeof(float));
  l.total = cv.off;
  return l;
}

}  // namespace gnnrag

using namespace gnnrag;

extern "C" size_t gnnrag_query_reform_backward_workspace_bytes(int32_t B, int32_t N, int32_t D, int32_t n) {
  if (B <= 0 || N <= 0 || D <= 0 || D > GNNRAG_QUERY_REFORM_MAX_D || n <= 0 || n > GNNRAG_MAX_REFORMS) return 0;
  return qr_bwd_layout(B, D, n).total;
}

extern "C" int gnnrag_query_reform_backward(const float* const* q, const float* seed_info, const float* const* W_r,
                                            const float* const* W_g, const void* reserve, size_t reserve_bytes,
                                            const float* const* g_out, float* const* dq, float* const* dW_r,
                                            float* const* dW_g, float* d_ent, int32_t B, int32_t N, int32_t D, int32_t n,
                                            void* workspace, size_t workspace_bytes, gnnrag_stream_t stream_) {
  if (!q || !seed_info || !W_r || !W_g || !g_out || B <= 0 || N <= 0 || D <= 0 || n <= 0) return GNNRAG_E_BADARG;
  if (n > GNNRAG_MAX_REFORMS || D > GNNRAG_QUERY_REFORM_MAX_D) return GNNRAG_E_UNSUPPORTED;
  for (int j = 0; j < n; ++j)
    if (!q[j] || !W_r[j] || !W_g[j]) return GNNRAG_E_BADARG;
  if (!reserve || reserve_bytes < gnnrag_query_reform_reserve_bytes(B, D, n)) return GNNRAG_E_WORKSPACE;
  const QrBwdLayout l = qr_bwd_layout(B, D, n);
  if (!workspace || workspace_bytes < l.total) return GNNRAG_E_WORKSPACE;
  const int64_t rows = (int64_t)B * N;
  const int64_t dent_blocks = (rows + kDentRows - 1) / kDentRows;
  if (d_ent && dent_blocks > INT32_MAX) return GNNRAG_E_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  QrBwdArgs a;
  memset(&a, 0, sizeof(a));
  QrDwArgs w;
  memset(&w, 0, sizeof(w));
  bool any_dq = false, any_dw = false;
  for (int j = 0; j < n; ++j) {
    a.q[j] = q[j];
    a.Wr[j] = W_r[j];
    a.Wg[j] = W_g[j];
    a.g_out[j] = g_out[j];
    a.dq[j] = dq ? dq[j] : nullptr;
    w.dW[2 * j] = dW_r ? dW_r[j] : nullptr;
    w.dW[2 * j + 1] = dW_g ? dW_g[j] : nullptr;
    if (g_out[j]) w.active |= 1u << j;
    any_dq = any_dq || a.dq[j];
    any_dw = any_dw || w.dW[2 * j] || w.dW[2 * j + 1];
  }
  if (!any_dq && !any_dw && !d_ent) return 0;
  a.y = (const float*)reserve;
  a.ag = a.y + (size_t)B * D;
  a.w_da = (float*)(ws + l.da); a.w_f = (float*)(ws + l.f); a.w_dy = (float*)(ws + l.dy);
  a.B = B; a.D = D;
  a.need_df = (any_dq || d_ent) ? 1 : 0;
  const size_t lds = (size_t)5 * D * sizeof(float);
  if (lds > 64 * 1024) {
    static DeviceMask raised{0};
    GNNRAG_RC(raise_lds_cap(k_qr_bwd, raised));
  }
  hipLaunchKernelGGL(k_qr_bwd, dim3(B, n), dim3(GNNRAG_QR_BWD_THREADS), lds, stream, a);
  GNNRAG_LAUNCH_CHECK();
  if (any_dw) {
    w.w_da = a.w_da; w.w_f = a.w_f; w.B = B; w.D = D;
    hipLaunchKernelGGL(k_qr_dw, dim3((3 * D + 255) / 256, D, 2 * n), dim3(256), 0, stream, w);
    GNNRAG_LAUNCH_CHECK();
  }
  if (d_ent) {
    const int64_t blocks = dent_blocks;
    if ((D & 3) == 0 && aligned16(d_ent)) {
      hipLaunchKernelGGL(k_qr_dent<true>, dim3((unsigned)blocks), dim3(256), 0, stream, seed_info, a.w_dy, d_ent, rows, N,
                         D, B, n, w.active);
    } else {
      hipLaunchKernelGGL(k_qr_dent<false>, dim3((unsigned)blocks), dim3(256), 0, stream, seed_info, a.w_dy, d_ent, rows, N,
                         D, B, n, w.active);
    }
    GNNRAG_LAUNCH_CHECK();
  }
  return 0;
}
