// Device functions of the BERT-class encoder shared by bert_encoder.hip and linear_splitk.hip: the erf GELU and the
// LayerNorm of one row by one wave.  One definition each, so that the same value gives the same bits wherever it is used.
#pragma once
#include "gnnrag_common.h"

namespace gnnrag {

// the multipliers of the 4 keep bytes in one 32-bit word (little endian: byte e belongs to element e)
__device__ __forceinline__ f32x4 bert_keep4(uint32_t w, float scale) {
  return (f32x4){(w & 0xffu) ? scale : 0.f, (w & 0xff00u) ? scale : 0.f, (w & 0xff0000u) ? scale : 0.f,
                 (w & 0xff000000u) ? scale : 0.f};
}

// LayerNorm of one row by one wave: biased variance, two passes (mean, then sum (x - mean)^2); `load(i)` returns the
// i-th float4 of the row (called three times per element: the row is L2 / L1 resident).  dst may be the row `load` reads:
// a lane writes only the elements it has read itself, after both reductions.
// DROP: the result is multiplied by scale where the row's keep byte is not 0, by 0 elsewhere (keep: the row's H bytes,
// 4-byte aligned; a lane reads the 4 bytes of its float4 as one word).
template <bool DROP = false, typename Load>
__device__ __forceinline__ void bert_ln_row(Load load, const float* __restrict__ g, const float* __restrict__ bt,
                                            float eps, int H4, int lane, float* dst,
                                            const uint8_t* __restrict__ keep = nullptr, float scale = 0.f) {
  const float inv_h = 1.f / (float)(H4 * 4);
  float s = 0.f;
  for (int i = lane; i < H4; i += 64) {
    const f32x4 v = load(i);
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  const float mean = wave_sum(s) * inv_h;
  float q = 0.f;
  for (int i = lane; i < H4; i += 64) {
    const f32x4 v = load(i);
    const float d0 = v[0] - mean, d1 = v[1] - mean, d2 = v[2] - mean, d3 = v[3] - mean;
    q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  const float rstd = 1.f / sqrtf(wave_sum(q) * inv_h + eps);
  for (int i = lane; i < H4; i += 64) {
    const f32x4 v = load(i);
    const f32x4 gg = ((const f32x4*)g)[i], bb = ((const f32x4*)bt)[i];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (v[e] - mean) * rstd * gg[e] + bb[e];
    if (DROP) o = o * bert_keep4(((const uint32_t*)keep)[i], scale);
    ((f32x4*)dst)[i] = o;
  }
}

// bert_ln_row of a row the wave already holds in registers: v[j] is float4 number lane + 64 j of the row (H4 <= 64 NV;
// the slots at or past H4 are not read).  The same statistics in the same order: a lane adds its float4s in ascending j,
// which is ascending i = lane + 64 j, then the wave's xor tree.
template <int NV>
__device__ __forceinline__ void bert_ln_row_regs(const f32x4 (&v)[NV], const float* __restrict__ g,
                                                 const float* __restrict__ bt, float eps, int H4, int lane, float* dst) {
  const float inv_h = 1.f / (float)(H4 * 4);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j)
    if (lane + 64 * j < H4) s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
  const float mean = wave_sum(s) * inv_h;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j)
    if (lane + 64 * j < H4) {
      const float d0 = v[j][0] - mean, d1 = v[j][1] - mean, d2 = v[j][2] - mean, d3 = v[j][3] - mean;
      q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  const float rstd = 1.f / sqrtf(wave_sum(q) * inv_h + eps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i = lane + 64 * j;
    if (i < H4) {
      const f32x4 gg = ((const f32x4*)g)[i], bb = ((const f32x4*)bt)[i];
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (v[j][e] - mean) * rstd * gg[e] + bb[e];
      ((f32x4*)dst)[i] = o;
    }
  }
}

__device__ __forceinline__ float bert_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

}  // namespace gnnrag
