// Seed retrieval of QueryReform: between two ReaRev iterations every
// instruction is fused with  seed_retrieve[b,:] = sum_n seed_info[b,n] * ent_emb[b,n,:]
// (reference gnn/modules/query_update.py:40, a [B,1,N] x [B,N,D] bmm that streams the whole node
// state, 102 MB at C2, to pick the one or two seed rows).  seed_info is the questions' seed indicator:
// here a wave scans the N flags of its question 64 at a time and reads only the rows whose flag is
// non-zero, in ascending node order (one fixed summation order).
#include "gnnrag_common.h"

namespace gnnrag {

__global__ __launch_bounds__(256) void k_seed_retrieve(const float* __restrict__ seed, const float* __restrict__ ent,
                                                       float* __restrict__ out, int N, int D) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const float* s = seed + (size_t)b * N;
  const float* e = ent + (size_t)b * N * D;
  for (int c0 = 0; c0 < D; c0 += 256) {
    const int c = c0 + (int)threadIdx.x;
    float acc = 0.f;
    for (int base = 0; base < N; base += 64) {
      const int n = base + lane;
      const float v = n < N ? s[n] : 0.f;
      unsigned long long m = __ballot(v != 0.f);
      while (m) {
        const int j = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float sv = __shfl(v, j, 64);
        if (c < D) acc += sv * e[(size_t)(base + j) * D + c];
      }
    }
    if (c < D) out[(size_t)b * D + c] = acc;
  }
}

// QueryReform.forward in ONE launch (query_update.py:26-44 -> Fusion, :6-16): the seed retrieval above, then
//   feats = [x, y, x - y]   gate = sigmoid(W_g feats)   out = gate * (W_r feats) + (1 - gate) * x
// for x = q_node[b] and y = seed_retrieve[b].  The torch form is ~11 launches per call and 6 calls per forward; at
// batch 1 that is 0.7 ms of the forward's 2.8 ms of host time (profiles/r05i_forward_host_time.txt).
// Workgroup (b, s): part s of the D outputs of question b (every part retrieves y itself: one or two rows); a wave
// owns an output at a time, its lanes stride over the 3 D terms (coalesced rows of W), fixed shuffle tree: one
// summation order.  ent_emb rows may be padded (row stride ldE >= D).
// The body of k_query_reform / k_query_reform_train for question b, output part `part` of `nparts`.  SAVE (training form):
// the retrieved y (once per question: by part 0 when save_y) and a_r = W_r feats, the gate of every output go to the caller's
// reserve; the arithmetic and its order are the same instructions either way, so the outputs carry the same bits.
template <bool SAVE>
__device__ __forceinline__ void query_reform_body(const float* __restrict__ q, const float* __restrict__ seed,
                                                  const float* __restrict__ ent, const float* __restrict__ Wr,
                                                  const float* __restrict__ Wg, float* __restrict__ out, int N, int D,
                                                  int ldE, int b, int part, int nparts, float* __restrict__ y_res,
                                                  float* __restrict__ ag_res, bool save_y) {
  extern __shared__ float feats[];                       // [3 D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* s = seed + (size_t)b * N;
  const float* e = ent + (size_t)b * N * ldE;
  for (int c0 = 0; c0 < D; c0 += 256) {
    const int c = c0 + (int)threadIdx.x;
    float acc = 0.f;
    for (int base = 0; base < N; base += 64) {
      const int n = base + lane;
      const float v = n < N ? s[n] : 0.f;
      unsigned long long m = __ballot(v != 0.f);
      while (m) {
        const int j = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float sv = __shfl(v, j, 64);
        if (c < D) acc += sv * e[(size_t)(base + j) * ldE + c];
      }
    }
    if (c < D) {
      const float x = q[(size_t)b * D + c];
      feats[c] = x;
      feats[D + c] = acc;
      feats[2 * D + c] = x - acc;
      if (SAVE && save_y) y_res[(size_t)b * D + c] = acc;
    }
  }
  __syncthreads();
  const int K = 3 * D;
  const int j0 = (int)((long long)D * part / nparts), j1 = (int)((long long)D * (part + 1) / nparts);
  // two outputs per wave and round: four independent load streams in flight (the loop is a chain of L2 round trips)
  for (int j = j0 + wave; j < j1; j += 8) {
    const int jb = j + 4 < j1 ? j + 4 : j;               // the second output of the round (the first again at the end)
    const float* wr0 = Wr + (size_t)j * K;
    const float* wg0 = Wg + (size_t)j * K;
    const float* wr1 = Wr + (size_t)jb * K;
    const float* wg1 = Wg + (size_t)jb * K;
    float ar0 = 0.f, ag0 = 0.f, ar1 = 0.f, ag1 = 0.f;
    for (int k = lane; k < K; k += 64) {
      const float f = feats[k];
      ar0 += wr0[k] * f;
      ag0 += wg0[k] * f;
      ar1 += wr1[k] * f;
      ag1 += wg1[k] * f;
    }
    // wave_sum's tree, the four sums interleaved: four calls give the same bits but another instruction schedule
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      ar0 += __shfl_xor(ar0, o, 64);
      ag0 += __shfl_xor(ag0, o, 64);
      ar1 += __shfl_xor(ar1, o, 64);
      ag1 += __shfl_xor(ag1, o, 64);
    }
    if (lane == 0) {
      const float gate = 1.f / (1.f + expf(-ag0));
      out[(size_t)b * D + j] = gate * ar0 + (1.f - gate) * feats[j];
      if (SAVE) {
        ag_res[(size_t)b * 2 * D + j] = ar0;
        ag_res[(size_t)b * 2 * D + D + j] = gate;
      }
    }
    if (lane == 1 && jb != j) {
      const float gate = 1.f / (1.f + expf(-ag1));
      out[(size_t)b * D + jb] = gate * ar1 + (1.f - gate) * feats[jb];
      if (SAVE) {
        ag_res[(size_t)b * 2 * D + jb] = ar1;
        ag_res[(size_t)b * 2 * D + D + jb] = gate;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_query_reform(const float* __restrict__ q, const float* __restrict__ seed,
                                                      const float* __restrict__ ent, const float* __restrict__ Wr,
                                                      const float* __restrict__ Wg, float* __restrict__ out, int N, int D,
                                                      int ldE) {
  query_reform_body<false>(q, seed, ent, Wr, Wg, out, N, D, ldE, blockIdx.x, blockIdx.y, gridDim.y, nullptr, nullptr,
                           false);
}

// The reforms of one iteration (rearev.py:217-221) in one launch: workgroup (b, part, j) is k_query_reform's (b, part) on
// reform j's instruction and Fusion weights; the reforms share the node state and the seeds.
struct QrTrainArgs {
  const float* q[GNNRAG_MAX_REFORMS];    // [B, D]
  const float* Wr[GNNRAG_MAX_REFORMS];   // [D, 3D]
  const float* Wg[GNNRAG_MAX_REFORMS];   // [D, 3D]
  const float* seed;                     // [B, N]
  const float* ent;                      // [B, N, ldE]
  float* out;                            // [n, B, D]
  float* y;                              // reserve: [B, D]
  float* ag;                             // reserve: [n, B, 2D]  (a_r, gate)
  int32_t B, N, D, ldE;
};

__global__ __launch_bounds__(256) void k_query_reform_train(const QrTrainArgs g) {
  const int j = blockIdx.z;
  query_reform_body<true>(g.q[j], g.seed, g.ent, g.Wr[j], g.Wg[j], g.out + (size_t)j * g.B * g.D, g.N, g.D, g.ldE,
                          blockIdx.x, blockIdx.y, gridDim.y, g.y, g.ag + (size_t)j * g.B * 2 * g.D,
                          j == 0 && blockIdx.y == 0);
}

}  // namespace gnnrag

using namespace gnnrag;

extern "C" int gnnrag_seed_retrieve(const float* seed_info, const float* ent_emb, float* out, int32_t B, int32_t N,
                                    int32_t D, gnnrag_stream_t stream) {
  if (!seed_info || !ent_emb || !out || B <= 0 || N <= 0 || D <= 0) return GNNRAG_E_BADARG;
  hipLaunchKernelGGL(k_seed_retrieve, dim3(B), dim3(256), 0, (hipStream_t)stream, seed_info, ent_emb, out, N, D);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnnrag_query_reform(const float* q_node, const float* seed_info, const float* ent_emb, int64_t ld_ent,
                                   const float* W_r, const float* W_g, float* out, int32_t B, int32_t N, int32_t D,
                                   gnnrag_stream_t stream) {
  if (!q_node || !seed_info || !ent_emb || !W_r || !W_g || !out || B <= 0 || N <= 0 || D <= 0 || ld_ent < D)
    return GNNRAG_E_BADARG;
  if ((size_t)3 * D * sizeof(float) > 48 * 1024) return GNNRAG_E_UNSUPPORTED;       // feats in LDS: D <= 4096
  // workgroups of a question share its outputs: about one workgroup per CU at batch 64, at most 8 per question
  int parts = (256 + B - 1) / B;
  parts = parts < 1 ? 1 : parts > 8 ? 8 : parts;
  hipLaunchKernelGGL(k_query_reform, dim3(B, parts), dim3(256), (size_t)3 * D * sizeof(float), (hipStream_t)stream, q_node,
                     seed_info, ent_emb, W_r, W_g, out, N, D, (int)ld_ent);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t gnnrag_query_reform_reserve_bytes(int32_t B, int32_t D, int32_t n) {
  if (B <= 0 || D <= 0 || D > GNNRAG_QUERY_REFORM_MAX_D || n <= 0 || n > GNNRAG_MAX_REFORMS) return 0;
  return ((size_t)B * D + (size_t)n * B * 2 * D) * sizeof(float);
}

extern "C" int gnnrag_query_reform_train(const float* const* q, const float* seed_info, const float* ent_emb,
                                         int64_t ld_ent, const float* const* W_r, const float* const* W_g, float* out,
                                         void* reserve, size_t reserve_bytes, int32_t B, int32_t N, int32_t D, int32_t n,
                                         gnnrag_stream_t stream) {
  if (!q || !seed_info || !ent_emb || !W_r || !W_g || !out || B <= 0 || N <= 0 || D <= 0 || n <= 0 || ld_ent < D)
    return GNNRAG_E_BADARG;
  if (n > GNNRAG_MAX_REFORMS || D > GNNRAG_QUERY_REFORM_MAX_D || ld_ent > INT32_MAX) return GNNRAG_E_UNSUPPORTED;
  for (int j = 0; j < n; ++j)
    if (!q[j] || !W_r[j] || !W_g[j]) return GNNRAG_E_BADARG;
  if (!reserve || reserve_bytes < gnnrag_query_reform_reserve_bytes(B, D, n)) return GNNRAG_E_WORKSPACE;
  QrTrainArgs a;
  memset(&a, 0, sizeof(a));
  for (int j = 0; j < n; ++j) {
    a.q[j] = q[j];
    a.Wr[j] = W_r[j];
    a.Wg[j] = W_g[j];
  }
  a.seed = seed_info; a.ent = ent_emb; a.out = out;
  a.y = (float*)reserve;
  a.ag = a.y + (size_t)B * D;
  a.B = B; a.N = N; a.D = D; a.ldE = (int32_t)ld_ent;
  // as gnnrag_query_reform, counting the (question, reform) pairs: no output depends on the number of parts
  int parts = (int)((256 + (int64_t)B * n - 1) / ((int64_t)B * n));
  parts = parts < 1 ? 1 : parts > 8 ? 8 : parts;
  hipLaunchKernelGGL(k_query_reform_train, dim3(B, parts, n), dim3(256), (size_t)3 * D * sizeof(float),
                     (hipStream_t)stream, a);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}
