// Device-side pieces shared by the bf16x3 kernels (tables_b3.hip: k_tables_b3, k_tables_vq, k_update_b3; gemm_f32.hip:
// the bf16x3 form of k_gemm_f32 and the register epilogues): the LDS layout of the resident weight planes, the order of
// the six plane products, the A planes of a k block, the products of a pair of column tiles, the table epilogue, and the
// DPP row helpers.  Everything is inlined; the header holds no kernel.  (The staging of the weight planes is not here:
// see the note at its first copy in tables_b3.hip.)
#pragma once
#include "gnnrag_common.h"

namespace gnnrag {

// ---- cross-lane helpers of the register epilogues: VALU only (DPP row operations), no LDS crossbar round trips (the
// first version reduced every row's score with six dependent ds_bpermute shuffles: 96 LDS round trips per wave and tile)
template <int CTRL, int BANK>
__device__ __forceinline__ float dpp_f(float old, float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(x), CTRL, 0xf, BANK, false));
}
__device__ __forceinline__ float lane_xor1(float x) { return dpp_f<0xB1, 0xf>(x, x); }   // quad_perm [1,0,3,2]
__device__ __forceinline__ float lane_xor2(float x) { return dpp_f<0x4E, 0xf>(x, x); }   // quad_perm [2,3,0,1]
__device__ __forceinline__ float lane_xor4(float x) {
  const float t = dpp_f<0x104, 0x5>(x, x);      // row_shl:4 into lanes 0-3, 8-11 of a 16-lane row (they read lane + 4)
  return dpp_f<0x114, 0xA>(t, x);               // row_shr:4 into lanes 4-7, 12-15 (they read lane - 4)
}
__device__ __forceinline__ float lane_xor8(float x) { return dpp_f<0x128, 0xf>(x, x); }  // row_ror:8

// Sums 4 values per lane over the 16 lanes of a DPP row with 6 DPP moves (instead of 4 x 4 shuffles): two
// reduce-scatter steps over lane bits 0 and 1 halve the values a lane carries, two all-reduce steps over bits 2
// and 3 finish.  Returns the total of value index 2*(lane&1) + ((lane>>1)&1); one fixed summation order.
__device__ __forceinline__ float row16_sum4(const float (&v)[4], int lane) {
  const bool b0 = lane & 1, b1 = lane & 2;
  float w2[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) w2[j] = (b0 ? v[j + 2] : v[j]) + lane_xor1(b0 ? v[j] : v[j + 2]);
  float w = (b1 ? w2[1] : w2[0]) + lane_xor2(b1 ? w2[0] : w2[1]);
  w += lane_xor4(w);
  w += lane_xor8(w);
  return w;
}
__device__ __forceinline__ int row16_sum4_index(int lane) { return 2 * (lane & 1) + ((lane >> 1) & 1); }

// Opaque copy of a lane-dependent value: address arithmetic derived from it is redone where it is used instead of
// being hoisted out of the row-tile loop and kept in (spilled) registers across the k loop.
__device__ __forceinline__ int opaque(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

// ---- the resident weight planes: three bf16 planes of an exact 3-way split (gnnrag_common.h: split3) -------------------
constexpr int kTabNTH = 7;        // column tiles per column part (two parts cover up to 13 tiles = 208 columns)
constexpr int kTabNKB = 7;        // k blocks of 32: 192 < D <= 208 (the hidden size of the BASELINE configs is 200)
constexpr int kTabSlots = 26;     // LDS row stride of a weight plane in 16-byte slots (26 % 4 == 2: conflict free)
constexpr int kTabRowB = kTabSlots * 16;              // bytes per weight row of one plane
constexpr int kTabPlaneB = kTabNTH * 16 * kTabRowB;   // bytes per plane

// (A plane, B plane) pairs of the six products, smallest terms first: mid*mid, lo*hi, hi*lo, mid*hi, hi*mid, hi*hi
constexpr int kB3PA[6] = {1, 2, 0, 1, 0, 0};
constexpr int kB3PB[6] = {1, 0, 2, 0, 1, 0};

// LDS row of column slot: the first four column tiles of a part are interleaved so that a lane holds four
// consecutive columns (float4 stores in the epilogue), the others keep the plain order
__device__ __forceinline__ int tab_lds_row(int j) {
  if (j < 64) return ((j & 3) << 4) + (j >> 2);
  return j;
}

// Weight rows a column part stages per plane: its CTN x 16 columns (columns past the part's last real one as zeros)
// PLUS ONE zero row when the part does not fill the plane - the last k block of a row reads up to 32 bytes past the
// row's end (k >= D; the A side is zero there), i.e. the head of the NEXT row, and 0 x (whatever an unwritten LDS row
// holds) is NaN when that happens to be an Inf / NaN pattern.  With D = 200 the next row is one of the part's own zero
// rows; with D = 208 the 6-tile part ends exactly at its last staged row (found by the D = 208 shape-sweep test:
// column 207 came out as relu(NaN) = 0 for some rows).  A full plane (7 tiles) is followed by the next plane's row 0
// or the zeroed slack.
__device__ __forceinline__ constexpr int tab_stage_rows(int ctn) { return ctn < kTabNTH ? ctn * 16 + 1 : ctn * 16; }

// The three A planes of a k block from the splits of a lane's two float4 (8 consecutive k).  By value: a Split3 passed
// by reference stays in scratch memory (32 bytes per lane in k_tables_b3 and k_update_b3).
__device__ __forceinline__ void b3_pack_a(Split3 s0, Split3 s1, bf16x8 (&ap)[3]) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  ap[0] = __builtin_bit_cast(bf16x8, (u32x4){s0.hi.x, s0.hi.y, s1.hi.x, s1.hi.y});
  ap[1] = __builtin_bit_cast(bf16x8, (u32x4){s0.mid.x, s0.mid.y, s1.mid.x, s1.mid.y});
  ap[2] = __builtin_bit_cast(bf16x8, (u32x4){s0.lo.x, s0.lo.y, s1.lo.x, s1.lo.y});
}

// The six plane products of one accumulator row on column tiles nt and nt + 1 (nt even; the second only when the
// part has it), the two tiles' dependent chains alternating.  w0 / w1 / w2 + koff is the lane's fragment of column
// tile 0 in the hi / mid / lo plane: the caller chooses how the three planes are addressed.
template <int CTN>
__device__ __forceinline__ void b3_products_pair(f32x4 (&acc)[CTN], int nt, const bf16x8 (&ap)[3], const unsigned char* w0,
                                                 const unsigned char* w1, const unsigned char* w2, int koff) {
  bf16x8 b0[3], b1[3];
  auto read_pair = [&](int pl, const unsigned char* w) {
    b0[pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const f32x4*>(w + (nt * 16 * kTabRowB + koff)));
    b1[pl] = b0[pl];
    if (nt + 1 < CTN)
      b1[pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const f32x4*>(w + ((nt + 1) * 16 * kTabRowB + koff)));
  };
  read_pair(0, w0);
  read_pair(1, w1);
  read_pair(2, w2);
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[kB3PA[p]], b0[kB3PB[p]], acc[nt], 0, 0, 0);
    if (nt + 1 < CTN)
      acc[nt + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ap[kB3PA[p]], b1[kB3PB[p]], acc[nt + 1], 0, 0, 0);
  }
}

// Table epilogue: one 16-row tile's accumulators leave the registers (C layout: rows row0 + 4 fg + q, column slot fr)
// for rows below row_end and the part's ncol columns from col0.
template <int CTN>
__device__ __forceinline__ void tab_store_tiles(const f32x4 (&acc)[CTN], float* P, int D, int row0, int row_end,
                                                int col0, int ncol, int fr, int fg) {
  static_assert(CTN >= 4, "a column part holds at least the interleaved group");
  const int rbase = row0 + 4 * fg;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = rbase + q;
    if (row < row_end) {
      float* prow = P + (size_t)row * D + col0;
      // interleaved group (column tiles 0..3): columns 4 fr .. 4 fr + 3
      {
        const f32x4 v = {acc[0][q], acc[1][q], acc[2][q], acc[3][q]};
        const int c = 4 * fr;
        if (c + 4 <= ncol) *reinterpret_cast<f32x4*>(prow + c) = v;
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e < ncol) prow[c + e] = v[e];
        }
      }
#pragma unroll
      for (int nt = 4; nt < CTN; ++nt) {
        const int c = nt * 16 + fr;
        if (c < ncol) prow[c] = acc[nt][q];
      }
    }
  }
}

}  // namespace gnnrag
