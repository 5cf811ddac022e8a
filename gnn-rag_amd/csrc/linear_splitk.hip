// Split-K linear for few rows: C = epilogue(A W^T + bias), A [M, K], W [Nout, K], with K cut
// into `splits` chunks of k_chunk that run on different waves, and a second launch that adds the chunks' partial products
// in chunk order and applies the epilogue.  For the frozen LM encoder at B T = 12 .. 20 rows, where k_gemm_skinny (one wave
// per 16 x 64 tile, all of K in that wave) leaves a 768 x 3072 weight to 12 waves and 768 dependent MFMA steps each.
//
//   k_splitk_product   P[s, r, c] = sum over k in [s k_chunk, min((s + 1) k_chunk, K)) of A[r, k] W[c, k]
//                      grid (row tiles, 64-column tiles, splits), one wave per workgroup; a wave owns MT 16-row tiles and
//                      four 16-column tiles, reads its MFMA fragments straight from global memory (every byte of W is read
//                      by exactly one wave per row-tile group: at M <= 64 the weights are read once) and walks its chunk 32 k
//                      at a time with all of a step's loads issued before its MFMAs.  Exact fp32 (v_mfma_f32_16x16x4_f32),
//                      k ascending; a chunk longer than 256 k is added up in blocks of 256 (one chain per block).
//   k_splitk_reduce    x = ((P[0] + P[1]) + ... + P[S-1]) + bias per element, s ascending; C = x or bert_gelu(x)
//   k_splitk_reduce_ln the same x + add per row, held in registers by the wave that owns the row, then the LayerNorm
//                      arithmetic of k_bert_add_ln (bert_device.h); C may be the buffer add is
//
// No atomics, no flags between workgroups, no counters: two launches, the second ordered behind the first by the stream.
// Value rule: an accumulator of row r and column c sees A[r, :] and W[c, :] only, in an order that (K, k_chunk) fixes -
// whichever row tile, row-tile group (MT) or batch the row sits in; the reduce adds the chunks in chunk order.  The
// automatic choice of splits reads (K, Nout) alone: never M, never the device.
#include "bert_device.h"
#include "gnnrag_common.h"

namespace gnnrag {

// The automatic rule (host only): kSplitkAutoSplits chunks - more only where the 64-column tiles times the chunks would
// stay below kSplitkAutoWaves waves - a chunk being a multiple of 16 k (one MFMA group of the k loop) and at least
// kSplitkMinChunk.  Measured at 12 rows: at K = 384 .. 3072 and Nout = 384 .. 3072 the time has
// its minimum at 4 .. 8 chunks and 8 is within 10 % of it everywhere; beyond that the reduce's reads and the second
// launch's share grow faster than the chains shrink.  The wave floor (narrow outputs) is an extrapolation, not measured.
constexpr int kSplitkAutoSplits = 8;
constexpr int kSplitkAutoWaves = 32;
constexpr int kSplitkMinChunk = 32;
constexpr int kSplitkFold = 256;         // k per MFMA chain inside a chunk (a multiple of the 32-wide k step)
constexpr int kSplitkLnRows = 4;         // rows (waves) per workgroup of k_splitk_reduce_ln

struct SplitkPlan {
  int32_t splits, k_chunk;
};

// GNNRAG_E_UNSUPPORTED: K % 4, a forced value above the maximum or one that leaves an empty chunk
static int splitk_plan(int32_t K, int32_t Nout, int32_t splits, SplitkPlan* p) {
  if (K % 4 != 0) return GNNRAG_E_UNSUPPORTED;
  if (splits == 0) {
    const int64_t tiles = ((int64_t)Nout + 63) / 64;
    const int64_t floor_ = (kSplitkAutoWaves + tiles - 1) / tiles;
    const int64_t want = floor_ > kSplitkAutoSplits ? floor_ : kSplitkAutoSplits;
    int64_t chunk = (int64_t)align_up((size_t)((K + want - 1) / want), 16);
    if (chunk < kSplitkMinChunk) chunk = kSplitkMinChunk;
    if ((K + chunk - 1) / chunk > GNNRAG_SPLITK_MAX_SPLITS)
      chunk = (int64_t)align_up((size_t)((K + GNNRAG_SPLITK_MAX_SPLITS - 1) / GNNRAG_SPLITK_MAX_SPLITS), 16);
    if (chunk > K) chunk = K;
    p->k_chunk = (int32_t)chunk;
    p->splits = (int32_t)((K + chunk - 1) / chunk);
    return 0;
  }
  if (splits > GNNRAG_SPLITK_MAX_SPLITS) return GNNRAG_E_UNSUPPORTED;
  const int64_t chunk = (int64_t)align_up((size_t)((K + splits - 1) / splits), 4);
  if ((int64_t)(splits - 1) * chunk >= K) return GNNRAG_E_UNSUPPORTED;      // the last chunk would be empty
  p->splits = splits;
  p->k_chunk = (int32_t)chunk;
  return 0;
}

// sizes first (BADARG), then the shape rules (UNSUPPORTED); pointers are never looked at here
static int splitk_shape(int64_t M, int32_t K, int32_t Nout, int32_t splits, SplitkPlan* p) {
  if (M <= 0 || K <= 0 || Nout <= 0 || splits < 0) return GNNRAG_E_BADARG;
  if (Nout % 4 != 0 || M >= ((int64_t)1 << 31) || ((int64_t)Nout + 63) / 64 > 65535) return GNNRAG_E_UNSUPPORTED;
  return splitk_plan(K, Nout, splits, p);
}

template <int MT>
__global__ __launch_bounds__(64) void k_splitk_product(const float* __restrict__ A, const float* __restrict__ W,
                                                       float* __restrict__ P, int M, int K, int Nout, int k_chunk) {
  const int lane = threadIdx.x, fr = lane & 15, fg = lane >> 4;
  const int m0 = blockIdx.x * (16 * MT), c0 = blockIdx.y * 64;
  const int kb = blockIdx.z * k_chunk, ke = min(kb + k_chunk, K);
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  // rows and columns past the end read the last one (valid memory); their accumulators are not stored
  const float* arow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) arow[mt] = A + (size_t)min(m0 + mt * 16 + fr, M - 1) * K;
  const float* wrow[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) wrow[nt] = W + (size_t)min(c0 + nt * 16 + fr, Nout - 1) * K;
  // A chunk is summed in blocks of kSplitkFold k: an MFMA chain per block, the blocks added in ascending order.  A long
  // chunk (a forced splits = 1 at K = 3072) then carries the rounding error of a blocked sum, not of one 3072-step chain;
  // a chunk of up to kSplitkFold is one chain, and 0 + chain is the chain.
  f32x4 sum[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) sum[mt][nt] = zero4;
  for (int kf = kb; kf < ke; kf += kSplitkFold) {
    const int kfe = min(kf + kSplitkFold, ke);
    f32x4 acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = zero4;
    for (int k0 = kf; k0 < kfe; k0 += 32) {
      f32x4 a[2][MT], b[2][4];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int k = k0 + c * 16 + fg * 4;
        const bool ok = k < kfe;                          // multiples of 4: a float4 is in or out as a whole
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) b[c][nt] = ok ? *reinterpret_cast<const f32x4*>(wrow[nt] + k) : zero4;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[c][mt] = ok ? *reinterpret_cast<const f32x4*>(arow[mt] + k) : zero4;
      }
      // an accumulator takes its 8 steps in (c, e) order: k ascending; between two of them run the other 4 MT - 1
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][mt][e], b[c][nt][e], acc[mt][nt], 0, 0, 0);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) sum[mt][nt] = sum[mt][nt] + acc[mt][nt];
  }
  // the MFMA C layout: lane (fr, fg) holds rows 4 fg + q of column fr
  float* plane = P + (size_t)blockIdx.z * M * Nout;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int col = c0 + nt * 16 + fr;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = m0 + mt * 16 + fg * 4 + q;
        if (row < M && col < Nout) plane[(size_t)row * Nout + col] = sum[mt][nt][q];
      }
    }
}

// the S partials of float4 number i (of n4 per plane), added in chunk order
__device__ __forceinline__ f32x4 splitk_sum(const f32x4* __restrict__ P4, size_t n4, size_t i, int S) {
  f32x4 x = P4[i];
  for (int s = 1; s < S; ++s) x = x + P4[(size_t)s * n4 + i];
  return x;
}

template <bool GELU>
__global__ __launch_bounds__(256) void k_splitk_reduce(const float* __restrict__ P, const float* __restrict__ bias,
                                                       float* __restrict__ C, size_t n4, int N4, int S) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 x = splitk_sum((const f32x4*)P, n4, i, S);
    if (bias) x = x + ((const f32x4*)bias)[i % (size_t)N4];
    if (GELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = bert_gelu(x[e]);
    }
    ((f32x4*)C)[i] = x;
  }
}

// A wave owns a row and holds it in NV float4 per lane (H4 <= 64 NV).  C may be add: a lane reads the elements of add that
// it writes itself, before it writes them (no __restrict__ on the two).
template <int NV>
__global__ __launch_bounds__(64 * kSplitkLnRows) void k_splitk_reduce_ln(const float* __restrict__ P,
                                                                         const float* __restrict__ bias, const float* add,
                                                                         const float* __restrict__ g,
                                                                         const float* __restrict__ bt, float eps, int M,
                                                                         int H4, int S, float* C) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kSplitkLnRows + (threadIdx.x >> 6);
  if (row >= M) return;
  const size_t n4 = (size_t)M * H4, r4 = (size_t)row * H4;
  f32x4 v[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i = lane + 64 * j;
    v[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (i < H4) {
      f32x4 x = splitk_sum((const f32x4*)P, n4, r4 + i, S);
      if (bias) x = x + ((const f32x4*)bias)[i];
      v[j] = x + ((const f32x4*)add)[r4 + i];
    }
  }
  bert_ln_row_regs<NV>(v, g, bt, eps, H4, lane, C + r4 * 4);
}

// Rows too long for the registers (Nout > 4096): the wave writes x + add into its row of C (each lane its own elements,
// which with C == add are the ones it has just read) and normalises the row from there as k_bert_add_ln does.
__global__ __launch_bounds__(64 * kSplitkLnRows) void k_splitk_reduce_ln_long(const float* __restrict__ P,
                                                                              const float* __restrict__ bias,
                                                                              const float* add, const float* __restrict__ g,
                                                                              const float* __restrict__ bt, float eps,
                                                                              int M, int H4, int S, float* C) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kSplitkLnRows + (threadIdx.x >> 6);
  if (row >= M) return;
  const size_t n4 = (size_t)M * H4, r4 = (size_t)row * H4;
  f32x4* dst = (f32x4*)C + r4;
  for (int i = lane; i < H4; i += 64) {
    f32x4 x = splitk_sum((const f32x4*)P, n4, r4 + i, S);
    if (bias) x = x + ((const f32x4*)bias)[i];
    dst[i] = x + ((const f32x4*)add)[r4 + i];
  }
  // a lane reads back what it wrote itself (same i = lane + 64 j in every pass): program order, no other lane's data
  bert_ln_row([&](int i) { return dst[i]; }, g, bt, eps, H4, lane, (float*)dst);
}

static inline size_t splitk_ws_bytes(int64_t M, int32_t Nout, int32_t splits) {
  return align_up((size_t)splits * (size_t)M * (size_t)Nout * sizeof(float), 256);
}

}  // namespace gnnrag

using namespace gnnrag;

extern "C" int gnnrag_linear_splitk_plan(int64_t M, int32_t K, int32_t Nout, int32_t splits, gnnrag_splitk_plan_t* out) {
  SplitkPlan p;
  GNNRAG_RC(splitk_shape(M, K, Nout, splits, &p));
  if (!out) return GNNRAG_E_BADARG;
  memset(out, 0, sizeof(*out));
  out->splits = p.splits;
  out->k_chunk = p.k_chunk;
  out->launches = 2;                       // the product and the reduce, at splits = 1 too
  return 0;
}

extern "C" size_t gnnrag_linear_splitk_workspace_bytes(int64_t M, int32_t K, int32_t Nout, int32_t splits) {
  SplitkPlan p;
  if (splitk_shape(M, K, Nout, splits, &p)) return 0;
  return splitk_ws_bytes(M, Nout, p.splits);
}

extern "C" int gnnrag_linear_splitk(const float* A, int64_t M, int32_t K, const float* W, const float* bias, int32_t epi,
                                    const float* add, const float* ln_g, const float* ln_b, float ln_eps, float* C,
                                    int32_t Nout, int32_t splits, void* ws, size_t ws_bytes, gnnrag_stream_t stream) {
  if (epi != GNNRAG_SPLITK_EPI_BIAS && epi != GNNRAG_SPLITK_EPI_GELU && epi != GNNRAG_SPLITK_EPI_ADD_LN)
    return GNNRAG_E_BADARG;
  SplitkPlan p;
  GNNRAG_RC(splitk_shape(M, K, Nout, splits, &p));
  if (ws_bytes < splitk_ws_bytes(M, Nout, p.splits)) return GNNRAG_E_UNSUPPORTED;
  const bool ln = epi == GNNRAG_SPLITK_EPI_ADD_LN;
  if (!A || !W || !C || !ws || (ln && (!add || !ln_g || !ln_b))) return GNNRAG_E_BADARG;
  if (!aligned16(A, W, bias, C) || !aligned16(ws) || (ln && !aligned16(add, ln_g, ln_b))) return GNNRAG_E_UNSUPPORTED;

  hipStream_t st = (hipStream_t)stream;
  float* P = (float*)ws;
  const int Mi = (int)M, S = p.splits;
  const int mt = M <= 16 ? 1 : M <= 32 ? 2 : 4;
  const dim3 grid((unsigned)((M + 16 * mt - 1) / (16 * mt)), (unsigned)((Nout + 63) / 64), (unsigned)S);
  if (mt == 1) hipLaunchKernelGGL(k_splitk_product<1>, grid, dim3(64), 0, st, A, W, P, Mi, K, Nout, p.k_chunk);
  else if (mt == 2) hipLaunchKernelGGL(k_splitk_product<2>, grid, dim3(64), 0, st, A, W, P, Mi, K, Nout, p.k_chunk);
  else hipLaunchKernelGGL(k_splitk_product<4>, grid, dim3(64), 0, st, A, W, P, Mi, K, Nout, p.k_chunk);
  GNNRAG_LAUNCH_CHECK();

  const int N4 = Nout / 4;
  if (!ln) {
    const size_t n4 = (size_t)M * N4, blocks = (n4 + 255) / 256;
    const dim3 rgrid((unsigned)(blocks > 65536 ? 65536 : blocks));
    if (epi == GNNRAG_SPLITK_EPI_GELU)
      hipLaunchKernelGGL(k_splitk_reduce<true>, rgrid, dim3(256), 0, st, (const float*)P, bias, C, n4, N4, S);
    else
      hipLaunchKernelGGL(k_splitk_reduce<false>, rgrid, dim3(256), 0, st, (const float*)P, bias, C, n4, N4, S);
  } else {
    const dim3 lgrid((unsigned)((M + kSplitkLnRows - 1) / kSplitkLnRows)), lblock(64 * kSplitkLnRows);
#define GNNRAG_SPLITK_LN(NV)                                                                                         \
  hipLaunchKernelGGL(k_splitk_reduce_ln<NV>, lgrid, lblock, 0, st, (const float*)P, bias, add, ln_g, ln_b, ln_eps, Mi, \
                     N4, S, C)
    if (N4 <= 64) GNNRAG_SPLITK_LN(1);
    else if (N4 <= 128) GNNRAG_SPLITK_LN(2);
    else if (N4 <= 256) GNNRAG_SPLITK_LN(4);
    else if (N4 <= 512) GNNRAG_SPLITK_LN(8);
    else if (N4 <= 1024) GNNRAG_SPLITK_LN(16);
    else
      hipLaunchKernelGGL(k_splitk_reduce_ln_long, lgrid, lblock, 0, st, (const float*)P, bias, add, ln_g, ln_b, ln_eps,
                         Mi, N4, S, C);
#undef GNNRAG_SPLITK_LN
  }
  GNNRAG_LAUNCH_CHECK();
  return 0;
}
