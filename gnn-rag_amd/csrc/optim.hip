// The optimiser step of the reference trainer (gnn/train_model.py:228-230): torch.nn.utils.clip_grad_norm_ over the model's
// gradients and torch.optim.Adam.step over its trainable tensors - in torch a few dozen multi-tensor launches over ~60 small
// tensors and two or three embedding tables - as three launches driven by one device table (gnnrag_optim_seg, gnnrag.h).
//
//   k_optim_sqnorm       work item = chunk of GNNRAG_OPTIM_CHUNK elements of one tensor; 1024 threads, a thread owns the
//                        elements 4 t .. 4 t + 3 of the chunk and adds their squares in that order; block_sum; one float per
//                        chunk.  Reads g, n and first_chunk only.
//   k_optim_norm_finish  one workgroup: the chunks' sums staged through LDS 1024 at a time, added by one thread in ascending
//                        chunk order in double; total_norm and the clip coefficient of clip_grad_norm_.
//   k_optim_adam         work item = chunk; 256 threads, a thread owns the elements 4 (256 i + t) .. + 3, i < 4.  The update
//                        of _single_tensor_adam (non-capturable) per element; g is read, never written.
//
// A workgroup finds the tensor of a chunk by binary search over first_chunk (the last entry with first_chunk <= chunk: an
// entry without elements shares its first_chunk with its successor and is never chosen).  Grids are capped at 2048 workgroups
// and stride over the chunks.  16-byte accesses where the tensor's pointers allow, 4-byte accesses otherwise, the same
// ownership and - the element update is one function compiled without contraction - the same bits.  The last, partial chunk
// of a tensor is handled by element count: nothing at or past n is read or written.
// No atomics, no allocation, nothing waits for the stream.
#include "gnnrag_common.h"

static_assert(sizeof(gnnrag_optim_seg) == 80, "gnnrag_optim_seg: the layout the binding mirrors");
static_assert(GNNRAG_OPTIM_CHUNK == 4096, "a chunk is 1024 threads x 4 elements (sqnorm), 256 x 4 x 4 (adam)");

namespace gnnrag {

constexpr int kOptimGrid = 2048;          // 256 CUs x 8 workgroups: the cap of a memory-bound grid
constexpr int kAdamThreads = 256;
constexpr float kClipEps = 1e-6f;         // torch/nn/utils/clip_grad.py: max_norm / (total_norm + 1e-6)

// a pointer read from the table is generic to the compiler; the tensors are global memory: say so (global_load / _store)
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

__device__ __forceinline__ bool optim_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr,
                                                const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

// the entry that owns `chunk`: the last t with segs[t].first_chunk <= chunk (segs[0].first_chunk == 0)
__device__ __forceinline__ int optim_find(const gnnrag_optim_seg* __restrict__ segs, int T, int64_t chunk) {
  int lo = 0, hi = T - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(1024) void k_optim_sqnorm(const gnnrag_optim_seg* __restrict__ segs, int T, int64_t n_chunks,
                                                       float* __restrict__ partial) {
  __shared__ float red[16];
  __shared__ float bcast;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int t = optim_find(segs, T, c);
    const gfloat* __restrict__ g = (const gfloat*)segs[t].g;
    const int64_t off = (c - segs[t].first_chunk) * GNNRAG_OPTIM_CHUNK;
    const int64_t left = segs[t].n - off;                                   // elements of this chunk and after it
    const int cnt = left >= GNNRAG_OPTIM_CHUNK ? GNNRAG_OPTIM_CHUNK : (left > 0 ? (int)left : 0);
    const int e0 = 4 * threadIdx.x;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (e0 + 3 < cnt && optim_aligned16(segs[t].g)) {
      x = *(const gf32x4*)(g + off + e0);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e0 + e < cnt) x[e] = g[off + e0 + e];
    }
    float s = x[0] * x[0];
    s = fmaf(x[1], x[1], s);
    s = fmaf(x[2], x[2], s);
    s = fmaf(x[3], x[3], s);
    s = block_sum(s, red, &bcast);
    if (threadIdx.x == 0) partial[c] = s;
  }
}

__global__ __launch_bounds__(1024) void k_optim_norm_finish(const float* __restrict__ partial, int64_t n_chunks,
                                                            float max_norm, float* __restrict__ out2) {
  __shared__ float stage[1024];
  double total = 0.0;
  for (int64_t base = 0; base < n_chunks; base += 1024) {
    const int64_t rest = n_chunks - base;
    const int cnt = rest < 1024 ? (int)rest : 1024;
    if ((int)threadIdx.x < cnt) stage[threadIdx.x] = partial[base + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int k = 0; k < cnt; ++k) total += (double)stage[k];             // ascending chunk order
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(total);
    float coef = __fdiv_rn(max_norm, norm + kClipEps);
    if (coef == coef) coef = fminf(coef, 1.f);                             // clamp(max=1) keeps a NaN; fminf would drop it
    out2[0] = norm;
    out2[1] = coef;
  }
}

// One element of _single_tensor_adam.  Every rounding is written out (no contraction): the vector and the element path of
// k_optim_adam give the same bits.
struct AdamScalars {
  float coef, beta2, w1, w2, eps, wd, neg_step, bc2;
};

__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const AdamScalars& a) {
#pragma clang fp contract(off)
  float gp = g * a.coef;                                                   // clip_grad_norm_: grad.mul_(clip_coef)
  if (a.wd != 0.f) gp = fmaf(a.wd, p, gp);                                 // grad.add(param, alpha=weight_decay)
  const float d = gp - m;                                                  // exp_avg.lerp_(grad, 1 - beta1)
  m = a.w1 < 0.5f ? fmaf(a.w1, d, m) : fmaf(a.w1 - 1.f, d, gp);
  v = fmaf(a.w2 * gp, gp, v * a.beta2);                                    // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
  const float denom = __fdiv_rn(__fsqrt_rn(v), a.bc2) + a.eps;             // (exp_avg_sq.sqrt() / bc2_sqrt).add_(eps)
  p = p + __fdiv_rn(a.neg_step * m, denom);                                // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ __launch_bounds__(kAdamThreads) void k_optim_adam(const gnnrag_optim_seg* __restrict__ segs, int T,
                                                             int64_t n_chunks, const float* __restrict__ clip_coef) {
  const float coef = clip_coef ? clip_coef[0] : 1.f;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int t = optim_find(segs, T, c);
    const gnnrag_optim_seg sg = segs[t];
    const int64_t off = (c - sg.first_chunk) * GNNRAG_OPTIM_CHUNK;
    const int64_t left = sg.n - off;
    const int cnt = left >= GNNRAG_OPTIM_CHUNK ? GNNRAG_OPTIM_CHUNK : (left > 0 ? (int)left : 0);
    const AdamScalars a = {coef, sg.beta2, sg.om_beta1, sg.om_beta2, sg.eps, sg.weight_decay, -sg.step_size, sg.bc2_sqrt};
    gfloat* __restrict__ p = (gfloat*)(sg.p + off);
    const gfloat* __restrict__ g = (const gfloat*)(sg.g + off);
    gfloat* __restrict__ m = (gfloat*)(sg.m + off);
    gfloat* __restrict__ v = (gfloat*)(sg.v + off);
    const bool vec = optim_aligned16(sg.p, sg.g, sg.m, sg.v);           // a chunk starts 16 KB into its tensor: as aligned
#pragma unroll
    for (int i = 0; i < GNNRAG_OPTIM_CHUNK / (4 * kAdamThreads); ++i) {
      const int e0 = 4 * (i * kAdamThreads + (int)threadIdx.x);
      if (e0 >= cnt) break;
      if (vec && e0 + 3 < cnt) {
        f32x4 pv = *(const gf32x4*)(p + e0), mv = *(const gf32x4*)(m + e0), vv = *(const gf32x4*)(v + e0);
        const f32x4 gv = *(const gf32x4*)(g + e0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float pe = pv[e], me = mv[e], ve = vv[e];
          adam_element(pe, gv[e], me, ve, a);
          pv[e] = pe;
          mv[e] = me;
          vv[e] = ve;
        }
        *(gf32x4*)(p + e0) = pv;
        *(gf32x4*)(m + e0) = mv;
        *(gf32x4*)(v + e0) = vv;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e0 + e < cnt) {
            float pe = p[e0 + e], me = m[e0 + e], ve = v[e0 + e];
            adam_element(pe, g[e0 + e], me, ve, a);
            p[e0 + e] = pe;
            m[e0 + e] = me;
            v[e0 + e] = ve;
          }
      }
    }
  }
}

}  // namespace gnnrag

using namespace gnnrag;

extern "C" size_t gnnrag_optim_workspace_bytes(int64_t n_chunks) {
  if (n_chunks <= 0) return 0;
  return align_up((size_t)n_chunks * sizeof(float), 256);
}

extern "C" int gnnrag_grad_norm(const gnnrag_optim_seg* segs, int32_t T, int64_t n_chunks, float max_norm, float* out2,
                                void* workspace, size_t workspace_bytes, gnnrag_stream_t stream_) {
  if (!segs || !out2 || T <= 0 || n_chunks <= 0 || !(max_norm > 0.f)) return GNNRAG_E_BADARG;
  if (!workspace || workspace_bytes < gnnrag_optim_workspace_bytes(n_chunks)) return GNNRAG_E_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  float* partial = (float*)workspace;
  const int grid = (int)(n_chunks < kOptimGrid ? n_chunks : kOptimGrid);
  hipLaunchKernelGGL(k_optim_sqnorm, dim3(grid), dim3(1024), 0, stream, segs, T, n_chunks, partial);
  GNNRAG_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_optim_norm_finish, dim3(1), dim3(1024), 0, stream, partial, n_chunks, max_norm, out2);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnnrag_adam_step(const gnnrag_optim_seg* segs, int32_t T, int64_t n_chunks, const float* clip_coef,
                                gnnrag_stream_t stream_) {
  if (!segs || T <= 0 || n_chunks <= 0) return GNNRAG_E_BADARG;
  hipStream_t stream = (hipStream_t)stream_;
  const int grid = (int)(n_chunks < kOptimGrid ? n_chunks : kOptimGrid);
  hipLaunchKernelGGL(k_optim_adam, dim3(grid), dim3(kAdamThreads), 0, stream, segs, T, n_chunks, clip_coef);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}
