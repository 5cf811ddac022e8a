// Backward of the per-question relation tables of the fused training form (gnnrag_relation_tables_backward):
//
//   P[d, m, :] = sum_i W[:, blk(i,d) : blk(i,d) + D] . z[d, m, i, :],   z = relu(a),   a[d, m, i, k] = T_d[r_m, k] * ins[b_m, i, k]
//
// over the compact rows m = (b_m, r_m) of a structure, blk(i, d) = (1 + 2 i + d) D.  From g_P [2, M, D]:
//
//   H[d, i, m, k]      = sum_o g_P[d, m, o] W[o, blk(i,d) + k]           2 I products on gnnrag_linear against the rows
//                                                                        blk(i,d).. of W^T (one transposed copy)
//   G                  = H where a > 0, else 0                           formed by H's two readers, never stored
//   g_ins[b, i, k]     = sum_d sum_{m of b} G[d, m, i, k] T_d[r_m, k]    k_rtb_ins: a question's rows are contiguous
//   g_T_d[r, k]        = sum_{m: r_m = r} sum_i G[d, m, i, k] ins[b_m, i, k]   k_rtb_tables: one workgroup per (r, d)
//   g_W[o, blk(i,d)+k] = sum_m g_P[d, m, o] z[d, m, i, k]                k_gemm_tn with the generated B operand (z is
//                                                                        formed on the loaded pieces), k_rtb_w_reduce
//
// No atomics: every output element has one writer and one summation order that depends on the structure and (D, I) alone.
#include "gnnrag_common.h"
#include "dense_internal.h"

namespace gnnrag {

struct RtbArgs {
  const int2* rows;          // [M] (question, relation)
  const int32_t* rel_off;    // [B + 1]
  const float* T[2];         // [R1, D]
  const float* ins;          // [B, I, D]
  const float* H;            // [2][I][M][D]
  float* g_T[2];             // [R1, D] or null
  float* g_ins;              // [B, I, D]
  int32_t M, B, D, I;
};

// Both kernels: 256 threads = `groups` row groups x D / 4 float4 columns (D <= 1024); a group adds its rows in ascending
// order, the groups' sums are added in group order.
__device__ __forceinline__ f32x4 rtb_group_sum(f32x4 acc, f32x4* red, int nc4, int groups, int c4, int grp) {
  red[threadIdx.x] = acc;
  __syncthreads();
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (grp == 0) {
    s = red[c4];
    for (int g2 = 1; g2 < groups; ++g2) s += red[g2 * nc4 + c4];
  }
  return s;
}

// g_ins[b, i, :]: grid (B, I).  A question without rows writes +0.
__global__ __launch_bounds__(256) void k_rtb_ins(const RtbArgs a) {
  __shared__ f32x4 red[256];
  const int b = blockIdx.x, i = blockIdx.y, D = a.D;
  const int nc4 = D >> 2, groups = 256 / nc4;
  const int grp = (int)threadIdx.x / nc4, c4 = (int)threadIdx.x - grp * nc4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (grp < groups) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(a.ins + ((size_t)b * a.I + i) * D + 4 * c4);
    const int end = a.rel_off[b + 1];
    for (int m = a.rel_off[b] + grp; m < end; m += groups) {
      const int r = a.rows[m].y;
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(a.T[d] + (size_t)r * D + 4 * c4);
        const f32x4 h = *reinterpret_cast<const f32x4*>(a.H + (((size_t)d * a.I + i) * a.M + m) * D + 4 * c4);
        const f32x4 pa = t * q;                               // the forward's product: the gate is a > 0
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (pa[e] > 0.f) acc[e] += h[e] * t[e];
      }
    }
  }
  const f32x4 s = rtb_group_sum(acc, red, nc4, groups, c4, grp);
  if (grp == 0) *reinterpret_cast<f32x4*>(a.g_ins + ((size_t)b * a.I + i) * D + 4 * c4) = s;
}

// g_T_d[r, :]: grid (R1, 2).  The questions that use relation r are found by binary search in each question's sorted
// relation list (as k_bwd_reduce_tables does); a relation nobody uses writes +0.
__global__ __launch_bounds__(256) void k_rtb_tables(const RtbArgs a) {
  __shared__ f32x4 red[256];
  __shared__ int found[256];
  const int r = blockIdx.x, d = blockIdx.y, D = a.D;
  if (!a.g_T[d]) return;
  const int nc4 = D >> 2, groups = 256 / nc4;
  const int grp = (int)threadIdx.x / nc4, c4 = (int)threadIdx.x - grp * nc4;
  const bool live = grp < groups;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  f32x4 t = acc;
  if (live) t = *reinterpret_cast<const f32x4*>(a.T[d] + (size_t)r * D + 4 * c4);
  for (int b0 = 0; b0 < a.B; b0 += 256) {
    const int b = b0 + (int)threadIdx.x;
    int row = -1;
    if (b < a.B) {
      int lo = a.rel_off[b], hi = a.rel_off[b + 1];          // first row with relation >= r
      const int end = hi;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.rows[mid].y < r) lo = mid + 1; else hi = mid;
      }
      if (lo < end && a.rows[lo].y == r) row = lo;
    }
    found[threadIdx.x] = row;
    __syncthreads();
    const int nb = min(256, a.B - b0);
    if (live) {
      for (int j = grp; j < nb; j += groups) {
        const int m = found[j];
        if (m < 0) continue;
        for (int i = 0; i < a.I; ++i) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(a.ins + ((size_t)(b0 + j) * a.I + i) * D + 4 * c4);
          const f32x4 h = *reinterpret_cast<const f32x4*>(a.H + (((size_t)d * a.I + i) * a.M + m) * D + 4 * c4);
          const f32x4 pa = t * q;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (pa[e] > 0.f) acc[e] += h[e] * q[e];
        }
      }
    }
    __syncthreads();
  }
  const f32x4 s = rtb_group_sum(acc, red, nc4, groups, c4, grp);
  if (grp == 0) *reinterpret_cast<f32x4*>(a.g_T[d] + (size_t)r * D + 4 * c4) = s;
}

// g_W [D, (2I+1) D] from the chunks' partial blocks part [2][chunks][D][I D] of the two directions, in chunk order; the
// self block (columns < D) does not enter the tables: +0.
__global__ __launch_bounds__(256) void k_rtb_w_reduce(const float* __restrict__ part, float* __restrict__ g_W, int D, int I,
                                                      int chunks) {
  const int K4 = (2 * I + 1) * (D >> 2);
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)D * K4) return;
  const int o = (int)(idx / K4), c = 4 * (int)(idx - (int64_t)o * K4);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (c >= D) {
    const int blk = c / D - 1, i = blk >> 1, d = blk & 1, k = c - (blk + 1) * D;
    const size_t n = (size_t)D * I * D;                      // floats of one chunk's block
    const float* p = part + (size_t)d * chunks * n + (size_t)o * I * D + (size_t)i * D + k;
    s = *reinterpret_cast<const f32x4*>(p);
    for (int ch = 1; ch < chunks; ++ch) s += *reinterpret_cast<const f32x4*>(p + (size_t)ch * n);
  }
  *reinterpret_cast<f32x4*>(g_W + (size_t)o * (2 * I + 1) * D + c) = s;
}

struct RtbLayout {
  size_t wt, h, tn, total;
  int chunks;
};

static bool rtb_shape_ok(int32_t D, int32_t I) {
  return D > 0 && I > 0 && D % 4 == 0 && D <= 1024 && I <= GNNRAG_MAX_INS;
}

// M > 0
static RtbLayout rtb_layout(int64_t M, int32_t D, int32_t I) {
  RtbLayout l;
  Carve cv;
  l.wt = cv.take((size_t)(2 * I + 1) * D * D * sizeof(float));
  l.h = cv.take((size_t)2 * I * M * D * sizeof(float));
  l.chunks = gemm_tn_gen_chunks(M, D, I * D);
  l.tn = cv.take((size_t)2 * l.chunks * D * I * D * sizeof(float));
  l.total = cv.off;
  return l;
}

}  // namespace gnnrag

using namespace gnnrag;

extern "C" size_t gnnrag_relation_tables_backward_workspace_bytes(const gnnrag_csr* csr, int32_t D, int32_t I) {
  if (!csr || !rtb_shape_ok(D, I) || csr->rel_total <= 0) return 0;
  return rtb_layout(csr->rel_total, D, I).total;
}

extern "C" int gnnrag_relation_tables_backward(const gnnrag_csr* csr, const float* T_fwd, const float* T_inv,
                                               const float* ins, const float* W_e2e, const float* g_P, float* g_T_fwd,
                                               float* g_T_inv, float* g_ins, float* g_W, int32_t D, int32_t I, int32_t math,
                                               void* workspace, size_t workspace_bytes, gnnrag_stream_t stream_) {
  if (!csr || !T_fwd || !T_inv || !ins || !W_e2e || !g_P || D <= 0 || I <= 0 || csr->rel_total < 0 || csr->B <= 0 ||
      csr->R1 <= 0)
    return GNNRAG_E_BADARG;
  if (math != GNNRAG_MATH_FP32 && math != GNNRAG_MATH_BF16X3 && math != GNNRAG_MATH_MIXED) return GNNRAG_E_BADARG;
  if (!g_T_fwd && !g_T_inv && !g_ins && !g_W) return GNNRAG_E_BADARG;
  if (!rtb_shape_ok(D, I) || !aligned16(T_fwd, T_inv, ins, W_e2e, g_P, g_T_fwd, g_T_inv, g_ins, g_W, workspace))
    return GNNRAG_E_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  const int32_t M = csr->rel_total, K = (2 * I + 1) * D;
  if (M == 0) {                                     // no facts, no tables: every gradient is zero
    float* const outs[4] = {g_T_fwd, g_T_inv, g_ins, g_W};
    const size_t n[4] = {(size_t)csr->R1 * D, (size_t)csr->R1 * D, (size_t)csr->B * I * D, (size_t)D * K};
    for (int j = 0; j < 4; ++j)
      if (outs[j]) GNNRAG_HIP(hipMemsetAsync(outs[j], 0, n[j] * sizeof(float), stream));
    return 0;
  }
  const RtbLayout l = rtb_layout(M, D, I);
  if (!workspace || workspace_bytes < l.total) return GNNRAG_E_WORKSPACE;
  if (g_T_fwd || g_T_inv || g_ins) {
    float* Wt = (float*)((char*)workspace + l.wt);
    float* H = (float*)((char*)workspace + l.h);
    GNNRAG_RC(transpose_launch(W_e2e, Wt, D, K, stream));
    for (int d = 0; d < 2; ++d) {
      if (!g_ins && !(d ? g_T_inv : g_T_fwd)) continue;       // nobody reads this direction's H
      for (int i = 0; i < I; ++i)
        GNNRAG_RC(gnnrag_linear(g_P + (size_t)d * M * D, M, D, Wt + (size_t)(1 + 2 * i + d) * D * D, nullptr, nullptr, 0, 0,
                                H + ((size_t)d * I + i) * M * D, D, math, stream_));
    }
    RtbArgs a;
    memset(&a, 0, sizeof(a));
    a.rows = (const int2*)csr->rel_rows; a.rel_off = csr->rel_off;
    a.T[0] = T_fwd; a.T[1] = T_inv; a.ins = ins; a.H = H;
    a.g_T[0] = g_T_fwd; a.g_T[1] = g_T_inv; a.g_ins = g_ins;
    a.M = M; a.B = csr->B; a.D = D; a.I = I;
    if (g_ins) {
      hipLaunchKernelGGL(k_rtb_ins, dim3(csr->B, I), dim3(256), 0, stream, a);
      GNNRAG_LAUNCH_CHECK();
    }
    if (g_T_fwd || g_T_inv) {
      hipLaunchKernelGGL(k_rtb_tables, dim3(csr->R1, 2), dim3(256), 0, stream, a);
      GNNRAG_LAUNCH_CHECK();
    }
  }
  if (g_W) {
    float* part = (float*)((char*)workspace + l.tn);
    const float* const Ts[2] = {T_fwd, T_inv};
    for (int d = 0; d < 2; ++d)
      GNNRAG_RC(gemm_tn_gen_partials(g_P + (size_t)d * M * D, Ts[d], ins, csr->rel_rows, M, D, D, I,
                                     part + (size_t)d * l.chunks * D * I * D, stream));
    const int64_t n4 = (int64_t)D * K / 4;
    hipLaunchKernelGGL(k_rtb_w_reduce, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, (const float*)part, g_W, D, I,
                       l.chunks);
    GNNRAG_LAUNCH_CHECK();
  }
  return 0;
}
