// The bf16x3 W-resident kernels of the fused path (gfx950):
//   k_tables_b3   relation tables, operand relu(T * ins) generated in registers (a lone gnnrag_relation_tables call)
//   k_tables_vq   relation tables in "V form" from pre-split relation planes (<false>: the public planes; <true>: the
//                 packed sparse operand, what a layer / stack call runs)
//   k_update_b3   the self-block update h' = relu(h W^T + b + nbr) with the fused score
// They share the LDS weight-plane layout (three bf16 planes of an exact 3-way split, 26-slot row stride), the six
// plane products on v_mfma_f32_16x16x32_bf16 with fp32 accumulation, and the register epilogue: b3_tile.h holds each of
// these once (layout constants, kB3PA / kB3PB, b3_pack_a, b3_products_pair, tab_store_tiles); only the staging of the
// weight planes is still written twice (tables_b3_part says why).
//
// ---- k_tables_b3: per-question relation tables of the fused path, operand generated on the fly ----------------------
//
//   P[d, m, :] = sum_i  W_e2e[:, (1+2i+d)D : (2+2i+d)D] . relu( T_d[r_m, :] * ins[b_m, i, :] )      m = compact row (b_m, r_m)
//
// (reference: the e2e_linear column blocks applied to the per-fact messages of reasongnn.py:71-79 / :98-105, once
// per (question, relation in use) instead of once per fact - see gemm_f32.hip / DESIGN.md section 3.3).
//
// Why a second kernel: on the k-tiled kernel (gemm_f32.hip) this product ran at ~30 % of the bf16 matrix rate at C2
// (127 us): 150 rows per workgroup leave a 22-row remainder tile that costs a full tile, and every 32 k the
// workgroup restages operands and synchronises twice.  The operand here is GENERATED from two small L2-resident
// tables, so nothing has to stream from HBM and the weights can stay put:
//   * workgroup = (direction d, column part h, row chunk): 8 waves, one per CU;
//   * per instruction i the workgroup splits its weight block W_{i,d}[columns of h, :] into three bf16 planes ONCE
//     (exact 3-way split, gnnrag_common.h) and keeps them in LDS (3 x 112 x 416 B = 140 KB at D = 200; row stride
//     26 x 16 B keeps the ds_read_b128 fragment reads bank-conflict free);
//   * every wave owns up to 5 of the chunk's 16-row tiles and keeps ALL their accumulators in registers across the
//     instructions (5 x 7 column tiles x 4 = 140 VGPRs), so P is written once and nothing is re-read;
//   * the A fragment of (tile, i, 32 k) - relu(T * ins), split into planes in registers - is built by the lane
//     that feeds it to the MFMA, from loads issued one k block ahead; six v_mfma_f32_16x16x32_bf16 per (column
//     tile, k block): hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid, smallest terms first, fp32 accumulation.
// Two barriers per instruction and workgroup instead of two per 32 k.
#include "gnnrag_common.h"
#include "dense_internal.h"
#include "b3_tile.h"
#include <type_traits>

namespace gnnrag {

#ifndef GNNRAG_TAB_TPW
#define GNNRAG_TAB_TPW 3
#endif
#ifndef GNNRAG_TAB_MINBLK
#define GNNRAG_TAB_MINBLK 2       // waves per SIMD: one 8-wave workgroup per CU (the planes fill its LDS) = 2, 256 registers each
#endif
constexpr int kTabTPW = GNNRAG_TAB_TPW;        // row tiles per wave and pass (accumulators in registers; 5 spill: 140 + 40 + 36 VGPRs)
constexpr int kTabQBytes = 160 * 1024 - 3 * kTabPlaneB - 64;   // LDS left for instruction rows (24 000 B)

struct TabArgs {
  const float* T[2];       // [R1, D] relation tables of the two directions
  const float* ins;        // [B, I, D]
  const float* W;          // e2e_linear.weight [D, (2I+1) D]
  float* P;                // [2, M, D]
  const int2* rows;        // [M] (question, relation id) of every compact row
  int32_t M, D, I, ldw;
  int32_t ct0;             // column tiles of part 0 (part 1 takes the rest)
  int32_t npass;           // passes of kTabTPW tiles per wave
};

// One column part with CTN column tiles (compile time: the MFMA loop has no branches).  QLDS: the instruction rows
// of the chunk's questions are in LDS (the usual case) - also compile time: a run-time branch around the global-memory
// variant's loads would make every vmcnt wait of the loop conservative, i.e. wait for the prefetch just issued.
template <int CTN, bool QLDS>
__device__ __forceinline__ void tables_b3_part(const TabArgs& a, unsigned char* lds, int col0, int bmin, int nq) {
  constexpr int RB = kTabRowB, PL = kTabPlaneB;
  constexpr int ctn = CTN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int d = blockIdx.y;
  const int D = a.D, I = a.I;
  const int ncol = min(ctn * 16, D - col0);                 // valid columns of this part
  const float* T = a.T[d];
  float* P = a.P + (size_t)d * a.M * D;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  constexpr int NKB = kTabNKB;                              // 32-wide k blocks
  const int KC = D >> 2;                                    // float4 chunks of a weight row

  // this wave's 16-row tiles: the chunk's tiles are dealt out contiguously to the 8 waves
  const long long U = ((long long)a.M + 15) >> 4;
  const int c0 = (int)(U * blockIdx.x / gridDim.x), c1 = (int)(U * (blockIdx.x + 1) / gridDim.x);
  const int nchunk = c1 - c0;
  const int w0 = c0 + (int)((long long)nchunk * wave / 8), w1 = c0 + (int)((long long)nchunk * (wave + 1) / 8);

  if (tid < 16) reinterpret_cast<unsigned*>(lds + 3 * PL)[tid] = 0u;   // slack behind the last plane: finite (k >= D reads)
  // the instruction rows ins[b, :, :] of the questions this chunk's rows belong to (rows are sorted by question):
  // LDS behind the planes when they fit, else they are read from global memory (cache resident)
  float* qarea = reinterpret_cast<float*>(lds + 3 * PL + 64);
  constexpr bool q_in_lds = QLDS;
  if (q_in_lds) {
    const float* src = a.ins + (size_t)bmin * I * D;
    for (int x = tid * 4; x < nq * I * D; x += 512 * 4)
      *reinterpret_cast<f32x4*>(qarea + x) = *reinterpret_cast<const f32x4*>(src + x);
  }

  for (int pass = 0; pass < a.npass; ++pass) {
    const int tbase = w0 + pass * kTabTPW;
    const int ntile = max(0, min(kTabTPW, w1 - tbase));     // wave-uniform
    f32x4 acc[kTabTPW][CTN];
#pragma unroll
    for (int j = 0; j < kTabTPW; ++j)
#pragma unroll
      for (int nt = 0; nt < CTN; ++nt) acc[j][nt] = zero4;

    for (int i = 0; i < I; ++i) {
      __syncthreads();                                      // the previous block's fragment reads are done
      // ---- this instruction's weight block -> three bf16 planes in LDS.  The same text as in update_b3_part but for
      // wcol, and it stays text: as a function in b3_tile.h the array v comes out as one 24-register tuple that is
      // copied after every load, each load waited for at once (k_tables_b3: 256 registers and 256 bytes of scratch);
      // `#pragma nounroll` on the loop over `base` avoids that (204, none) but leaves the loop rolled ----
      {
        const int wcol = (1 + 2 * i + d) * D;               // first k column of the block inside e2e_linear.weight
        const int total = tab_stage_rows(ctn) * kTabSlots * 2;      // 8-byte pieces (4 k) per plane: rows x 52
        constexpr int UN = 6;                               // requests in flight per thread before the first split
        for (int base = 0; base < total; base += 512 * UN) {
          f32x4 v[UN];
          int off[UN];
#pragma unroll
          for (int u = 0; u < UN; ++u) {
            const int idx = base + u * 512 + tid;
            const int j = idx / (kTabSlots * 2), kc = idx - j * (kTabSlots * 2);
            v[u] = zero4;
            off[u] = idx < total ? tab_lds_row(j) * RB + kc * 8 : -1;
            if (idx < total && j < ncol && kc < KC)
              v[u] = *reinterpret_cast<const f32x4*>(a.W + (size_t)(col0 + j) * a.ldw + wcol + 4 * kc);
          }
#pragma unroll
          for (int u = 0; u < UN; ++u) {
            if (off[u] >= 0) {
              const Split3 sp = split3(v[u]);
              unsigned char* dst = lds + off[u];
              *reinterpret_cast<uint2*>(dst) = sp.hi;
              *reinterpret_cast<uint2*>(dst + PL) = sp.mid;
              *reinterpret_cast<uint2*>(dst + 2 * PL) = sp.lo;
            }
          }
        }
      }
      __syncthreads();

      // ---- MFMA phase: k blocks outermost, the wave's tiles inside: a tile's T row piece for k block kb + 1 is
      // requested right after the piece for kb has been consumed, i.e. a whole round of tiles (kTabTPW x 42 MFMAs)
      // before its use; the instruction rows come from LDS ----
      int toff[kTabTPW], qoff[kTabTPW];                     // per tile: this lane's row offsets (floats) into T / the q area
#pragma unroll
      for (int j = 0; j < kTabTPW; ++j) {
        const int m = min((tbase + (j < ntile ? j : 0)) * 16 + fr, a.M - 1);
        const int2 br = a.rows[m];
        toff[j] = br.y * D + 8 * fg;
        qoff[j] = ((br.x - bmin) * I + i) * D + 8 * fg;
      }
      const int kmax = D - 8;                               // last valid 8-element start of a row
      f32x4 traw[kTabTPW][2];
#pragma unroll
      for (int j = 0; j < kTabTPW; ++j) {
        const float* tp = T + toff[j] + (min(8 * fg, kmax) - 8 * fg);
        traw[j][0] = *reinterpret_cast<const f32x4*>(tp);
        traw[j][1] = *reinterpret_cast<const f32x4*>(tp + 4);
      }
      for (int kb = 0; kb < NKB; ++kb) {      // (not unrolled: the unrolled loop spills 200 registers)
        const bool kok = 32 * kb + 8 * fg <= kmax;
        const int kbn = min(kb + 1, NKB - 1);               // (the last block requests itself again: no branch)
        const int kon = min(32 * kbn + 8 * fg, kmax) - 8 * fg;
        const int koq = min(32 * kb + 8 * fg, kmax) - 8 * fg;
        const unsigned char* wb = lds + fr * RB + kb * 64 + fg * 16;
#pragma unroll
        for (int j = 0; j < kTabTPW; ++j) {
          if (j < ntile) {                                  // wave-uniform
            const f32x4 t0 = traw[j][0], t1 = traw[j][1];
            {
              const float* tp = T + toff[j] + kon;
              traw[j][0] = *reinterpret_cast<const f32x4*>(tp);
              traw[j][1] = *reinterpret_cast<const f32x4*>(tp + 4);
            }
            __builtin_amdgcn_sched_barrier(0);              // the requests stay ABOVE the MFMAs
            f32x4 q0, q1;
            if constexpr (QLDS) {
              const float* qp = qarea + qoff[j] + koq;
              q0 = *reinterpret_cast<const f32x4*>(qp);
              q1 = *reinterpret_cast<const f32x4*>(qp + 4);
            } else {
              const float* qp = a.ins + (size_t)bmin * I * D + qoff[j] + koq;
              q0 = *reinterpret_cast<const f32x4*>(qp);
              q1 = *reinterpret_cast<const f32x4*>(qp + 4);
            }
            // A planes of this k block: relu(T * ins), exact 3-way bf16 split
            const Split3 s0 = split3(kok ? __builtin_elementwise_max(t0 * q0, zero4) : zero4);
            const Split3 s1 = split3(kok ? __builtin_elementwise_max(t1 * q1, zero4) : zero4);
            bf16x8 ap[3];
            b3_pack_a(s0, s1, ap);
#pragma unroll
            for (int nt = 0; nt < CTN; nt += 2) b3_products_pair<CTN>(acc[j], nt, ap, wb, wb + PL, wb + 2 * PL, 0);
          }
        }
      }
    }

    // ---- epilogue: the pass's tiles leave the registers ----
#pragma unroll
    for (int j = 0; j < kTabTPW; ++j)
      if (j < ntile) tab_store_tiles<CTN>(acc[j], P, D, (tbase + j) * 16, a.M, col0, ncol, fr, fg);
  }
}

__global__ __launch_bounds__(512, GNNRAG_TAB_MINBLK) void k_tables_b3(TabArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int NT = (a.D + 15) >> 4;
  const int h = blockIdx.z;
  const int ctn = h == 0 ? a.ct0 : NT - a.ct0;              // column tiles of this part
  const int col0 = h == 0 ? 0 : a.ct0 * 16;                 // first column of this part
  // questions this chunk's rows belong to (rows are sorted by question)
  const long long U = ((long long)a.M + 15) >> 4;
  const int c0 = (int)(U * blockIdx.x / gridDim.x), c1 = (int)(U * (blockIdx.x + 1) / gridDim.x);
  const int rlo = min(c0 * 16, a.M - 1), rhi = min(c1 * 16, a.M) - 1;
  const int bmin = a.rows[rlo].x, bmax = a.rows[max(rhi, rlo)].x;
  const int nq = bmax - bmin + 1;
  const bool q_in_lds = (size_t)nq * a.I * a.D * sizeof(float) <= kTabQBytes;
#define GNNRAG_TAB_CASE(N)                                                  \
  case N:                                                                   \
    if (q_in_lds) tables_b3_part<N, true>(a, lds, col0, bmin, nq);          \
    else tables_b3_part<N, false>(a, lds, col0, bmin, nq);                  \
    break;
  switch (ctn) {
    GNNRAG_TAB_CASE(6) GNNRAG_TAB_CASE(7)
    default: break;
  }
#undef GNNRAG_TAB_CASE
}

// ---- relation tables from PRE-SPLIT relation planes and per-question weights ("V form") -------------------------------
// relu(t * q) = max(q, 0) * relu(t) + max(-q, 0) * relu(-t) for every real t, q - so with Tp = relu(T_d), Tn = relu(-T_d)
//
//   P[d, (b, r), :] = sum_i W_{i,d} . relu(T_d[r, :] * ins[b, i, :])  =  [Tp[r, :], Tn[r, :]] . V_{b,d}
//   V_{b,d}[k, :]     = sum_i W_{i,d}[:, k] * max( ins[b,i,k], 0)          (rows 0 .. D-1,   "half" 0)
//   V_{b,d}[D + k, :] = sum_i W_{i,d}[:, k] * max(-ins[b,i,k], 0)          (rows D .. 2D-1,  "half" 1)
//
// The left operand no longer depends on the question: its three bf16 planes are written ONCE per layer by the relation
// projection kernel (rel_transform.hip: a few hundred rows, L2 resident) and arrive in the MFMA loop as ready 16-byte
// fragments - no multiply / relu / 3-way split beside the MFMAs (the VALU work that held k_tables_b3 at ~1/3 of the
// matrix rate; a packed-fp32 VALU instruction beside MFMAs costs far more than its issue slot on this chip), and the
// k extent is 2 D for every number of instructions I.  The question moves into the RIGHT operand: workgroup =
// (question, row chunk, direction, column part); it builds V's three planes for its column part in LDS, a range of k
// at a time (I weight blocks x the question's instruction rows), all row tiles of the question (<= 5 per wave: one
// pass at C2) multiply against them with the accumulators held across the ranges.  Same 6 plane products and fp32
// accumulation as above; V is rounded to fp32 once per element before its exact split.
//
// The product runs on the 2:4 structured-sparse instruction.  Of relu(T)[r, k] and relu(-T)[r, k] at most one is not
// zero, so with K interleaved as k+, k-, (k+1)+, (k+1)- every group of four holds at most two non-zeros, one from each
// (+, -) pair: the form v_smfmac_f32_16x16x64_bf16 takes.  Its compressed left operand is the planes of |T| - plane+
// OR plane-, bit for bit, because the half that is zero holds 0x0000 in all three planes - and the 2-bit positions are
// the signs of T, read off the - half (vq_compress); one index word serves all three planes.  7 sparse blocks of 32 k
// replace 14 dense ones per (row tile, column tile, plane product).  The relation planes stay as k_rel_transform writes
// them ([+ half | - half], kVqHalf apart); V is what gets interleaved, by the staging (vq_stage), in k ranges of 3, 3
// and 1 blocks - a whole interleaved row does not fit the planes' LDS.  B fragments cost the same LDS bytes per k as
// before against half the matrix-pipe time, so two row tiles share each one (one column tile at a time, the two
// tiles' accumulator chains alternating) where the dense form took two column tiles of one row tile.
//
// What the instruction expects, as measured by tools/probe/smfmac_probe.hip (profiles/r07a_smfmac_probe.txt):
//   * A (compressed, 8 bf16 per lane): lane l holds compressed k 8 (l / 16) .. + 7 of row l % 16; compressed k c belongs
//     to the group of four c / 2 and lands at interleaved K 4 (c / 2) + its 2-bit position;
//   * the positions of the lane's 8 values are 16 bits of the index register, element e at bits 2 e; abid selects the
//     half of the register (abid 0: bits 15:0), the other 16 bits are ignored;
//   * B (dense, 16 bf16 per lane) comes in TWO halves of 32 K, not as 16 contiguous K: elements 0-7 are K 8 (l / 16)
//     .. + 7, elements 8-15 are K 32 + 8 (l / 16) .. + 7, of column l % 16;
//   * the accumulator is the dense 16x16 one: rows 4 (l / 16) + q, column l % 16;
//   * rate: 8 independent accumulators, one or two waves per SIMD: 1.08 - 1.13 x the time of v_mfma_f32_16x16x32_bf16
//     per instruction, i.e. 1.77 - 1.86 x its K rate.
constexpr int kVqHalf = 32 * kTabNKB;          // bf16 elements per half row of the relation planes (224: k >= D are zero)
constexpr int kVqRowB = 2 * kVqHalf * 2;       // bytes per plane row: [relu(T) | relu(-T)]
#ifndef GNNRAG_VQ_TPW
#define GNNRAG_VQ_TPW 5
#endif
#ifndef GNNRAG_VQ_UN
#define GNNRAG_VQ_UN 2       // staging pieces per thread and round (3 spills beside the 140 accumulators)
#endif
constexpr int kVqTPW = GNNRAG_VQ_TPW;          // row tiles per wave and pass

struct VqArgs {
  const unsigned char* planes;   // [2 directions][3 planes][R1][kVqRowB]
  const float* ins;              // [B, I, D]
  const float* W;                // e2e_linear.weight [D, (2I+1) D]
  float* P;                      // [2, M, D]
  const int2* rows;              // [M] (question, relation id) of every compact row
  const int* rel_off;            // [B+1] first compact row of each question
  int32_t M, D, I, ldw, R1;
  int32_t ct0;                   // column tiles of part 0
  int32_t nchunk;                // row chunks per question (> 1 only when the batch has few questions)
  int32_t dir0;                  // first direction of the launch (grid y counts on from it)
  float* zero;                   // null or a buffer the launch also zeroes (the layer's score, see dense_internal.h)
  int64_t zero_n;
};

typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));
constexpr int kVqSub = 3 * 64;                 // byte offset of the second sub-plane in a V plane row (see vq_stage)

// (V+[k], V-[k]) dwords of 4 consecutive k from the packed planes of V+ and V-
__device__ __forceinline__ uint4 vq_interleave(uint2 p, uint2 n) {
  return make_uint4((p.x & 0xffffu) | (n.x << 16), (p.x >> 16) | (n.x & 0xffff0000u), (p.y & 0xffffu) | (n.y << 16),
                    (p.y >> 16) | (n.y & 0xffff0000u));
}
// the lane's B fragment of one plane: 16 bytes from each sub-plane (see vq_stage)
__device__ __forceinline__ bf16x16 vq_read_b(const unsigned char* p) {
  struct { f32x4 lo, hi; } v = {*reinterpret_cast<const f32x4*>(p), *reinterpret_cast<const f32x4*>(p + kVqSub)};
  return __builtin_bit_cast(bf16x16, v);
}

// row of (row, block) slot x when a row has nb = 3 or 1 blocks (x < 43690)
__device__ __forceinline__ int vq_row(int x, int nb) { return nb == 3 ? (int)(((unsigned)x * 43691u) >> 17) : x; }

// V planes of nb k blocks (32 k each, from block blk0) and one column part -> LDS, in the interleaved order of the sparse
// product:  V+[n, k] = sum_i W[col0 + n, (1 + 2 i + d) D + k] * max(ins[g, i, k], 0),  V-[n, k] the same with -ins; one
// dword holds (V+[n, k], V-[n, k]), so both signs of a k come from one read of W and ins.  Row n of a plane (kTabSlots
// x 16 B) holds two sub-planes of 3 x 64 B (a stage of one block fills a third of each): the lane of k-group fg reads
// the dwords of k = 4 fg .. 4 fg + 3 of a block from sub-plane 0 and those of k = 16 + 4 fg .. + 3 from sub-plane 1
// (kVqSub further: the instruction takes B in two halves of 32 interleaved K), each at row * RB + block * 64 + fg * 16 - the bank pattern of the dense kernels' fragment reads,
// conflict free; the lane's 32 bytes in one piece (fg * 32) would put lanes 4-11 of a ds_read_b128 group on the
// banks of lanes 0-3 and 12-15 at the 416-byte row stride: 2-way.  UN pieces (4 k: 16 bytes per plane) per thread and
// round; indices are recomputed rather than kept (register pressure).  Pieces with k >= D and columns past the part
// are written as zeros: every byte the fragment reads touch is written by the stage that precedes them (the reads
// stay inside the staged rows: no slack row as in the dense kernels).
template <int CTN, int UN>
__device__ __forceinline__ void vq_stage(const VqArgs& a, unsigned char* lds, const float* qarea, int col0, int ncol,
                                         int d, int blk0, int nb) {
  constexpr int RB = kTabRowB, PL = kTabPlaneB;
  const int total = CTN * 16 * 8 * nb;                         // 8 pieces per (row, block); nb is 3 or 1
  const int tid = threadIdx.x;
  const int D = a.D, I = a.I, KC = D >> 2;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int base = 0; base < total; base += 512 * UN) {
    f32x4 vp[UN], vn[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) vp[u] = vn[u] = zero4;
    for (int i = 0; i < I; ++i) {
      f32x4 w[UN];
      const float* wsrc = a.W + (size_t)col0 * a.ldw + (1 + 2 * i + d) * D;
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int idx = base + u * 512 + tid;
        const int j = vq_row(idx >> 3, nb), kc = (blk0 + (idx >> 3) - j * nb) * 8 + (idx & 7);
        // dead pieces (k >= D, columns past the part, idx >= total) read a valid address and are zeroed / skipped below
        w[u] = *reinterpret_cast<const f32x4*>(wsrc + (size_t)min(j, ncol - 1) * a.ldw + 4 * min(kc, KC - 1));
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int idx = base + u * 512 + tid;
        const int kc = (blk0 + (idx >> 3) - vq_row(idx >> 3, nb) * nb) * 8 + (idx & 7);
        const f32x4 q = *reinterpret_cast<const f32x4*>(qarea + i * D + 4 * min(kc, KC - 1));
        vp[u] += w[u] * __builtin_elementwise_max(q, zero4);
        vn[u] += w[u] * __builtin_elementwise_max(-q, zero4);
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int idx = base + u * 512 + tid;
      const int j = vq_row(idx >> 3, nb), b = (idx >> 3) - j * nb, pc = idx & 7, kc = (blk0 + b) * 8 + pc;
      if (idx < total) {
        const bool live = j < ncol && kc < KC;
        const Split3 sp = split3(live ? vp[u] : zero4), sn = split3(live ? vn[u] : zero4);
        unsigned char* dst = lds + tab_lds_row(j) * RB + (pc >> 2) * kVqSub + b * 64 + (pc & 3) * 16;
        *reinterpret_cast<uint4*>(dst) = vq_interleave(sp.hi, sn.hi);
        *reinterpret_cast<uint4*>(dst + PL) = vq_interleave(sp.mid, sn.mid);
        *reinterpret_cast<uint4*>(dst + 2 * PL) = vq_interleave(sp.lo, sn.lo);
      }
    }
  }
}

// The lane's operands of one (row tile, k block) for the sparse product: the three planes of |T| and the index word.
struct VqA {
  bf16x8 pl[3];
  int idx;
};
// ... as they arrive from the relation planes: the lane's 16 bytes of the + half and of the - half of each plane
struct VqRaw {
  uint4 p[3], n[3];
};
__device__ __forceinline__ VqRaw vq_load_a(const unsigned char* const (&plane_base)[3], unsigned off) {
  VqRaw r;
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) {
    r.p[pl] = *reinterpret_cast<const uint4*>(plane_base[pl] + off);
    r.n[pl] = *reinterpret_cast<const uint4*>(plane_base[pl] + (off + (unsigned)(kVqHalf * 2)));
  }
  return r;
}
// |T|'s planes are plane+ OR plane- (the half that is zero holds 0 in all three planes); the 2-bit index of the lane's
// compressed element e sits at bits 2 e of the index word: element 2 i (the first of group i) is at position 0 (+) or
// 1 (-) of its group of four, element 2 i + 1 at position 2 (+) or 3 (-) - always ascending.  "-" is decided on
// hi | mid | lo of the - half, so a value whose hi plane is zero still selects its own half of V.
__device__ __forceinline__ VqA vq_compress(const VqRaw& r) {
  VqA o;
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) {
    const uint4 c = make_uint4(r.p[pl].x | r.n[pl].x, r.p[pl].y | r.n[pl].y, r.p[pl].z | r.n[pl].z, r.p[pl].w | r.n[pl].w);
    o.pl[pl] = __builtin_bit_cast(bf16x8, c);
  }
  const unsigned m[4] = {r.n[0].x | r.n[1].x | r.n[2].x, r.n[0].y | r.n[1].y | r.n[2].y, r.n[0].z | r.n[1].z | r.n[2].z,
                         r.n[0].w | r.n[1].w | r.n[2].w};
  unsigned ix = 0x8888u;
#pragma unroll
  for (int i = 0; i < 4; ++i)      // (min with 1, shifts and ors with inline constants: selects would hold their masks in registers)
    ix |= (min(m[i] & 0xffffu, 1u) | (min(m[i] >> 16, 1u) << 2)) << (4 * i);
  o.idx = (int)ix;
  return o;
}

// The packed operand (rel_transform.hip: k_rel_transform writes it once per projection): per relation row the three planes
// of |T| (kVqHalf bf16 each) and 64 index bytes, the 16-bit index word of (k block, lane group fg) at fg * 16 + block * 2
// - already what vq_compress builds.  Three 16-byte loads and one 16-bit load per (row tile, k block) on one lane offset,
// against six 16-byte loads, ~55 VALU instructions and 24 transient registers for the public planes.
constexpr int kVqPackPlaneB = kVqHalf * 2;           // bytes per plane of a packed row
constexpr int kVqPackIdxB = 3 * kVqPackPlaneB;       // offset of the index bytes
constexpr int kVqPackRowB = kVqPackIdxB + 64;        // 1408
__device__ __forceinline__ VqA vq_load_packed(const unsigned char* row_base, unsigned off, int blk) {
  VqA o;
  // 32-bit offsets from the uniform base (scalar base + lane offset).  Folding the k block into the base and the rest into
  // immediates - (row_base + blk * 64) + off - makes the compiler form 64-bit lane addresses instead: 256 registers, 52 B scratch
#pragma unroll
  for (int pl = 0; pl < 3; ++pl)
    o.pl[pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(row_base + (off + (unsigned)(pl * kVqPackPlaneB + blk * 64))));
  o.idx = *reinterpret_cast<const unsigned short*>(row_base + (off + (unsigned)(kVqPackIdxB + blk * 2)));
  return o;
}

// PACKED: the A operand comes from the packed form (the layer sequence) instead of the public planes - the only difference
template <int CTN, bool PACKED>
__device__ __forceinline__ void tables_vq_part(const VqArgs& a, unsigned char* lds, int col0) {
  constexpr int RB = kTabRowB, PL = kTabPlaneB;
  constexpr unsigned AROWB = PACKED ? kVqPackRowB : kVqRowB;      // bytes of a relation row of the A operand
  constexpr int NPAIR = (kVqTPW + 1) / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int d = a.dir0 + blockIdx.y;
  const int g = blockIdx.x / a.nchunk, ch = blockIdx.x - g * a.nchunk;
  const int D = a.D, I = a.I;
  const int r0 = a.rel_off[g], r1 = a.rel_off[g + 1];
  if (r1 <= r0) return;                                       // a question without facts has no rows
  const int ncol = min(CTN * 16, D - col0);
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  float* P = a.P + (size_t)d * a.M * D;
  const unsigned char* planes = a.planes + (size_t)d * (PACKED ? 1 : 3) * a.R1 * AROWB;
  const size_t plane_stride = (size_t)a.R1 * kVqRowB;          // (public planes)

  // 16-row tiles of the question start at its first row; the chunk's tiles are dealt out contiguously to the 8 waves
  const int U = (r1 - r0 + 15) >> 4;
  const int c0 = U * ch / a.nchunk, c1 = U * (ch + 1) / a.nchunk;
  const int wv = __builtin_amdgcn_readfirstlane(wave);        // scalar: the tile-count branches below stay uniform
  const int w0 = c0 + (c1 - c0) * wv / 8, w1 = c0 + (c1 - c0) * (wv + 1) / 8;
  const int npass = ((c1 - c0 + 7) / 8 + kVqTPW - 1) / kVqTPW;     // workgroup-uniform (the barriers below)

  float* qarea = reinterpret_cast<float*>(lds + 3 * PL + 64);          // ins[g, :, :]
  for (int x = tid * 4; x < I * D; x += 512 * 4)
    *reinterpret_cast<f32x4*>(qarea + x) = *reinterpret_cast<const f32x4*>(a.ins + (size_t)g * I * D + x);

  for (int pass = 0; pass < npass; ++pass) {
    const int tbase = w0 + pass * kVqTPW;
    const int ntile = max(0, min(kVqTPW, w1 - tbase));        // wave-uniform
    f32x4 acc[kVqTPW][CTN];
#pragma unroll
    for (int j = 0; j < kVqTPW; ++j)
#pragma unroll
      for (int nt = 0; nt < CTN; ++nt) acc[j][nt] = zero4;
    // this lane's plane row of every tile (rows past the question / the wave's run read a valid row, never stored)
    unsigned aoff[kVqTPW];     // 32-bit byte offsets from the planes' (uniform) bases: scalar base + lane offset + immediate
#pragma unroll
    for (int j = 0; j < kVqTPW; ++j) {
      const int m = min(r0 + (tbase + (j < ntile ? j : 0)) * 16 + fr, r1 - 1);
      aoff[j] = (unsigned)a.rows[m].y * AROWB + (unsigned)fg * 16u;
    }
    const unsigned char* const plane_base[3] = {planes, planes + plane_stride, planes + 2 * plane_stride};

    // A operands are requested where they are used: the pair's 12 plane loads (packed: 6 + 2 index words; L2 hits) go out
    // together and the other wave of the SIMD has a pair's products (84 instructions) to issue meanwhile.  Holding the
    // next pair's raw loads beside the pair in use (48 registers, or 37 in a two-step form) spills: 140 accumulators +
    // 26 A + 2 x 24 B; so does holding the next pair's first PACKED tile (13 registers: 12 B of scratch).
    for (int s = 0; s < 3; ++s) {           // k blocks 0-2, 3-5, 6 (rolled: register pressure)
      __syncthreads();                                        // q rows staged / the previous stage's fragment reads done
      const int nblk = s < 2 ? 3 : 1;
      vq_stage<CTN, GNNRAG_VQ_UN>(a, lds, qarea, col0, ncol, d, 3 * s, nblk);
      __syncthreads();
      for (int kb = 0; kb < nblk; ++kb) {       // (not unrolled: register pressure)
        const int blk = 3 * s + kb;
        const unsigned char* wb = lds + fr * RB + kb * 64 + fg * 16;
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) {
          const int j0 = 2 * p, j1 = 2 * p + 1 < kVqTPW ? 2 * p + 1 : 2 * p;
          const bool two = 2 * p + 1 < kVqTPW;
          VqA cur[2];
          if constexpr (PACKED) {
            cur[0] = vq_load_packed(planes, aoff[j0], blk);
            cur[1] = two ? vq_load_packed(planes, aoff[j1], blk) : cur[0];
          } else {
            cur[0] = vq_compress(vq_load_a(plane_base, aoff[j0] + (unsigned)(blk * 64)));
            cur[1] = two ? vq_compress(vq_load_a(plane_base, aoff[j1] + (unsigned)(blk * 64))) : cur[0];
          }
          // the six plane products of this k block on every column tile, for row tile j0 or (two_c) for j0 and j1, which
          // then share each B fragment, their accumulator chains alternating
          auto products = [&](auto two_c) {
#pragma unroll
            for (int nt = 0; nt < CTN; ++nt) {
              bf16x16 b[3];
#pragma unroll
              for (int pl = 0; pl < 3; ++pl) b[pl] = vq_read_b(wb + pl * PL + nt * 16 * RB);
#pragma unroll
              for (int q = 0; q < 6; ++q) {
                acc[j0][nt] = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(cur[0].pl[kB3PA[q]], b[kB3PB[q]], acc[j0][nt], cur[0].idx, 0, 0);
                if (decltype(two_c)::value)
                  acc[j1][nt] = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(cur[1].pl[kB3PA[q]], b[kB3PB[q]], acc[j1][nt], cur[1].idx, 0, 0);
              }
            }
          };
          // wave-uniform.  Two row tiles share every B fragment; a slot whose second tile is past the wave's run still
          // computes it (never stored: at most one tile per wave and k block for nothing, none with 4 or 5 tiles as at
          // C2) - a third branch for it sinks the second tile's loads behind the branch, where they are issued one at
          // a time, each waiting for the one before
          if (two && j0 < ntile) products(std::true_type{});
          else if (!two && j0 < ntile) products(std::false_type{});      // the odd last row tile
        }
      }
    }

    // ---- epilogue: the pass's tiles leave the registers ----
#pragma unroll
    for (int j = 0; j < kVqTPW; ++j)
      if (j < ntile) tab_store_tiles<CTN>(acc[j], P, D, r0 + (tbase + j) * 16, r1, col0, ncol, fr, fg);
  }
}

template <bool PACKED>
__global__ __launch_bounds__(512, 2) void k_tables_vq(VqArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  if (a.zero) {               // every workgroup zeroes its share (a few floats per thread)
    const int64_t nb = (int64_t)gridDim.x * gridDim.y * gridDim.z;
    const int64_t lin = blockIdx.x + (int64_t)gridDim.x * (blockIdx.y + (int64_t)gridDim.y * blockIdx.z);
    for (int64_t i = lin * 512 + threadIdx.x; i < a.zero_n; i += nb * 512) a.zero[i] = 0.f;
  }
  const int NT = (a.D + 15) >> 4;
  const int h = blockIdx.z;
  const int ctn = h == 0 ? a.ct0 : NT - a.ct0;
  const int col0 = h == 0 ? 0 : a.ct0 * 16;
  switch (ctn) {
    case 6: tables_vq_part<6, PACKED>(a, lds, col0); break;
    case 7: tables_vq_part<7, PACKED>(a, lds, col0); break;
    default: break;
  }
}

// ---- the self-block update in bf16x3 on the same weight-plane layout -------------------------------------------------
//   h'[m, :] = relu( h[m, :] . W_e2e[:, 0:D]^T + b + nbr[m, :] ),   score[m] = w_s . h'[m, :] + b_s + (1 - mask[m]) * -1e11
// (reasongnn.py:161-168 with the neighbour blocks already reduced into nbr).  Workgroup = (row chunk, column part of
// 7 / 6 column tiles): the part's three weight planes are split and staged ONCE and stay in LDS for all row tiles of
// the chunk; every wave owns a contiguous run of 16-row tiles and, as in k_gemm_wres, reads a tile's A fragments in
// the MFMA layout straight from global memory (two float4 = 8 consecutive k per lane and k block, 128-byte lines) a
// whole tile ahead and splits them into planes in registers; the epilogue works from the registers.  A is read by
// both parts of a chunk - they sit next to each other in the grid and on one XCD, so the second read hits L2.  The
// two parts' score dots are two commutative atomic adds onto a zeroed score (x + y == y + x: deterministic); the part
// that owns column 0 adds bias and mask term to its share first, so a masked slot still ends exactly at -1e11.
struct UpdB3Args {
  const float* A;        // h [M, D]
  const float* W;        // e2e_linear.weight [D, ldw]; columns 0..D-1 are the self block
  const float* bias;     // [D]
  const float* add;      // nbr [M, D]
  const float* w_s;      // [D]
  const float* b_s;      // [1]
  const float* mask;     // [M]
  float* C;              // [M, D]
  float* score;          // [M], zeroed before the launch
  const uint8_t* add_flag;   // FL: [M + 4] row gates of `add`; a row whose byte is 0 reads the zero row `add + M * D`
  int32_t M, D, ldw, ct0;
};

template <int CTN, bool FL>
__device__ __forceinline__ void update_b3_part(const UpdB3Args& a, unsigned char* lds, int col0, bool first_part,
                                               int chunk, int nchunks) {
  constexpr int RB = kTabRowB, PL = kTabPlaneB;
  constexpr int NKB = kTabNKB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int D = a.D;
  const int ncol = min(CTN * 16, D - col0);
  const int KC = D >> 2;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  float* Bl = reinterpret_cast<float*>(lds + 3 * PL + 64);      // bias / score weights of this part's columns
  float* Sl = Bl + kTabNTH * 16;

  if (tid < 16) reinterpret_cast<unsigned*>(lds + 3 * PL)[tid] = 0u;
  for (int j = tid; j < kTabNTH * 16; j += 512) {
    Bl[j] = (j < ncol && a.bias) ? a.bias[col0 + j] : 0.f;
    Sl[j] = j < ncol ? a.w_s[col0 + j] : 0.f;
  }
  {   // weight planes of this column part (self block: columns 0..D-1 of e2e_linear.weight; see tables_b3_part)
    const int total = tab_stage_rows(CTN) * kTabSlots * 2;
    constexpr int UN = 6;
    for (int base = 0; base < total; base += 512 * UN) {
      f32x4 v[UN];
      int off[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int idx = base + u * 512 + tid;
        const int j = idx / (kTabSlots * 2), kc = idx - j * (kTabSlots * 2);
        v[u] = zero4;
        off[u] = idx < total ? tab_lds_row(j) * RB + kc * 8 : -1;
        if (idx < total && j < ncol && kc < KC)
          v[u] = *reinterpret_cast<const f32x4*>(a.W + (size_t)(col0 + j) * a.ldw + 4 * kc);
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        if (off[u] >= 0) {
          const Split3 sp = split3(v[u]);
          unsigned char* dst = lds + off[u];
          *reinterpret_cast<uint2*>(dst) = sp.hi;
          *reinterpret_cast<uint2*>(dst + PL) = sp.mid;
          *reinterpret_cast<uint2*>(dst + 2 * PL) = sp.lo;
        }
      }
    }
  }
  // this wave's 16-row tiles
  const long long U = ((long long)a.M + 15) >> 4;
  const int c0 = (int)(U * chunk / nchunks), c1 = (int)(U * (chunk + 1) / nchunks);
  const int nch = c1 - c0;
  int t = c0 + (int)((long long)nch * wave / 8);
  const int tend = c0 + (int)((long long)nch * (wave + 1) / 8);
  const int kmax = D - 8;
  // Addresses (round 5).  PMC showed the VALU pipe as busy as the matrix pipe (14.9 M VALU against 4.4 M MFMA instructions
  // per launch, profiles/r05c_pmc_update_b3.txt), and the ISA showed why: ~40 % of the loop's VALU instructions were
  // 64-bit address arithmetic the compiler rematerialised per access (v_lshl_add_u64, v_mad_i64_i32, clamps) and v_add_u32
  // for LDS offsets beyond the 16-bit immediate.  Now every global access is SCALAR BASE + 32-BIT LANE OFFSET + immediate
  // (the launcher admits (M + 1) * D * 4 < 2^32): one row offset per tile, lane constants for the column pieces; the
  // three LDS planes have one base register each, so that every fragment offset fits the immediate.
  const unsigned char* Ab = reinterpret_cast<const unsigned char*>(a.A);
  const unsigned char* addb = reinterpret_cast<const unsigned char*>(a.add);
  unsigned char* Cb = reinterpret_cast<unsigned char*>(a.C);
  const unsigned rowB = (unsigned)D * 4u;
  const unsigned k6B = (unsigned)min(32 * (NKB - 1) + 8 * fg, kmax) * 4u;      // the last k block's (clamped) piece
  auto a_rowoff = [&](int tile) -> unsigned { return (unsigned)min(tile * 16 + fr, a.M - 1) * rowB; };
  // raw A pieces of a tile: per k block two float4 (k = 32 kb + 8 fg .. + 7), unconditional (clamped addresses)
  auto a_piece = [&](unsigned rowoff, int kb, int half) -> f32x4 {
    const unsigned off = kb < NKB - 1 ? rowoff + 32u * (unsigned)fg + (unsigned)(128 * kb + 16 * half)
                                      : rowoff + k6B + (unsigned)(16 * half);
    return *reinterpret_cast<const f32x4*>(Ab + off);
  };
  f32x4 ra[NKB][2];
  if (t < tend) {
    const unsigned ro = a_rowoff(t);
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      ra[kb][0] = a_piece(ro, kb, 0);
      ra[kb][1] = a_piece(ro, kb, 1);
    }
  }
  const float bs = a.b_s[0];
  // lane constants of the epilogue's column pieces (bytes inside a row of nbr / h')
  const unsigned cgB = (unsigned)(col0 + min(4 * fr, ncol - 4)) * 4u;
  unsigned ctB[CTN > 4 ? CTN - 4 : 1];
#pragma unroll
  for (int nt = 4; nt < CTN; ++nt) ctB[nt - 4] = (unsigned)(col0 + min(nt * 16 + fr, ncol - 1)) * 4u;
  // FL: the four row gates of a lane's rows (one dword), requested a tile ahead like the A pieces
  unsigned fl_next = 0x01010101u;
  if (FL && t < tend) fl_next = *reinterpret_cast<const unsigned*>(a.add_flag + (size_t)t * 16 + 4 * fg);
  __syncthreads();

  for (; t < tend; ++t) {
    const int rbase = t * 16 + 4 * fg;                       // C layout: rows rbase + q, column slot fr
    const unsigned fl = fl_next;
    if (FL) fl_next = *reinterpret_cast<const unsigned*>(a.add_flag + (size_t)(t + 1 < tend ? t + 1 : t) * 16 + 4 * fg);
    // the epilogue's operands: nbr in the register layout (interleaved group: 4 consecutive columns per lane)
    f32x4 addg[4];                                           // group 0 (column tiles 0..3), per row q
    float addt[CTN > 4 ? CTN - 4 : 1][4];                    // plain tiles 4.., per row q
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      int row = min(rbase + q, a.M - 1);
      if (FL && ((fl >> (8 * q)) & 0xffu) == 0u) row = a.M;      // not a frontier row: the zero row behind the buffer
      const unsigned ro = (unsigned)row * rowB;
      addg[q] = *reinterpret_cast<const f32x4*>(addb + (ro + cgB));
#pragma unroll
      for (int nt = 4; nt < CTN; ++nt) addt[nt - 4][q] = *reinterpret_cast<const float*>(addb + (ro + ctB[nt - 4]));
    }
    const float mrow = a.mask[min(rbase + row16_sum4_index(fr), a.M - 1)];
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc[CTN];
#pragma unroll
    for (int nt = 0; nt < CTN; ++nt) acc[nt] = zero4;
    const unsigned ro_next = a_rowoff(t + 1 < tend ? t + 1 : t);
    // one base register per LDS plane (made opaque once per tile: keeps the loop-invariant plane reads inside the loop)
    const unsigned char* wbp[3];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) wbp[pl] = lds + (unsigned)opaque(fr * RB + fg * 16 + pl * PL);
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      bf16x8 ap[3];
      // only the LAST k block can reach past D (the launcher admits 192 < D <= 208): no select in the others
      const bool kok = kb < NKB - 1 || 32 * kb + 8 * fg <= kmax;
      const Split3 s0 = split3(kok ? ra[kb][0] : zero4);
      const Split3 s1 = split3(kok ? ra[kb][1] : zero4);
      b3_pack_a(s0, s1, ap);
      ra[kb][0] = a_piece(ro_next, kb, 0);                   // refill: the next tile's k block kb
      ra[kb][1] = a_piece(ro_next, kb, 1);
#pragma unroll
      for (int nt = 0; nt < CTN; nt += 2) b3_products_pair<CTN>(acc, nt, ap, wbp[0], wbp[1], wbp[2], kb * 64);
    }
    // epilogue from the registers.  h' leaves with nontemporal stores: nothing in this launch reads it again (100 MB at
    // C2, next read a layer later).  Measured, not derived: the C2 step is 11-15 us shorter with them while the
    // kernel's own traced time and counters stay where they were
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    const f32x4 bias_g = *reinterpret_cast<const f32x4*>(Bl + min(4 * fr, kTabNTH * 16 - 4));
    const f32x4 ws_g = *reinterpret_cast<const f32x4*>(Sl + min(4 * fr, kTabNTH * 16 - 4));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = rbase + q;
      const unsigned ro = (unsigned)min(row, a.M - 1) * rowB;
      f32x4 v = {acc[0][q], acc[1][q], acc[2][q], acc[3][q]};
      v = __builtin_elementwise_max((v + bias_g) + addg[q], zero4);
      const int c = 4 * fr;
      if (c + 4 > ncol) {                                    // (ncol % 4 == 0: a lane's group is all in or all out)
        v = zero4;
      } else if (row < a.M) {
        __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(Cb + (ro + cgB)));
      }
      part[q] += v[0] * ws_g[0] + v[1] * ws_g[1] + v[2] * ws_g[2] + v[3] * ws_g[3];
#pragma unroll
      for (int nt = 4; nt < CTN; ++nt) {
        const int cc = nt * 16 + fr;
        float x = fmaxf((acc[nt][q] + Bl[cc]) + addt[nt - 4][q], 0.f);
        if (cc >= ncol) x = 0.f;
        else if (row < a.M) __builtin_nontemporal_store(x, reinterpret_cast<float*>(Cb + (ro + ctB[nt - 4])));
        part[q] += x * Sl[cc];
      }
    }
    {
      const float tot = row16_sum4(part, lane);
      const int srow = rbase + row16_sum4_index(fr);
      if (fr < 4 && srow < a.M) {
        // this part's share of the score; the first part carries bias and mask term (fp32 adds: a masked slot's
        // share is exactly -1e11 and stays there when the other part's share is added)
        const float share = first_part ? (tot + bs) + (1.0f - mrow) * kVeryNeg : tot;
        atomicAdd(a.score + srow, share);
      }
    }
  }
}

template <bool FL>
__global__ __launch_bounds__(512, 2) void k_update_b3(UpdB3Args a, int nchunks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int blk = blockIdx.x;
  const int NT = (a.D + 15) >> 4;
  // the two parts of a row chunk are neighbours in the grid AND on one XCD (blocks b and b + 8):
  // block = 16*(c/8) + 8*h + c%8
  const int h = (blk >> 3) & 1;
  const int chunk = (blk >> 4) * 8 + (blk & 7);
  if (chunk >= nchunks) return;
  if (h == 0) update_b3_part<kTabNTH, FL>(a, lds, 0, true, chunk, nchunks);
  else if (NT - a.ct0 == 6) update_b3_part<6, FL>(a, lds, a.ct0 * 16, false, chunk, nchunks);
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// Hidden sizes the three kernels take: D a multiple of 8 (a lane's 8 consecutive k), kTabNKB k blocks of 32 and two
// column parts of 7 + 6 tiles, i.e. 192 < D <= 208
constexpr int kTabNT = 2 * kTabNTH - 1;
static bool b3_shape_ok(int32_t D) { return D % 8 == 0 && (D + 31) / 32 == kTabNKB && (D + 15) / 16 == kTabNT; }

// Row chunks of a launch over `tiles` 16-row tiles: `target` of them (from the CU count), at least one, and no more than
// leave a chunk 8 tiles (one per wave)
static int b3_row_chunks(int target, long long tiles) {
  int chunks = target < 1 ? 1 : target;
  if ((long long)chunks * 8 > tiles) chunks = (int)((tiles + 7) / 8);
  return chunks;
}

int update_b3_launch(const float* h, const float* nbr, const float* W, const float* b, const float* w_s, const float* b_s,
                     const float* mask, float* h_out, float* score, int64_t BN, int32_t D, int32_t ldw,
                     hipStream_t stream) {
  return update_b3_launch_f(h, nbr, nullptr, W, b, w_s, b_s, mask, h_out, score, BN, D, ldw, stream, false);
}

bool update_b3_shape_ok(int64_t BN, int32_t D, int32_t ldw) {
  // (32-bit byte offsets from the kernel's base pointers: the zero row behind nbr included)
  return b3_shape_ok(D) && BN >= 8192 && (BN + 1) * D * 4 < ((int64_t)1 << 32) && ldw % 4 == 0;
}

int update_b3_launch_f(const float* h, const float* nbr, const uint8_t* add_flag, const float* W, const float* b,
                       const float* w_s, const float* b_s, const float* mask, float* h_out, float* score, int64_t BN,
                       int32_t D, int32_t ldw, hipStream_t stream, bool score_zeroed) {
  if (!update_b3_shape_ok(BN, D, ldw)) return GNNRAG_E_UNSUPPORTED;
  if (!aligned16(h, nbr, W, h_out)) return GNNRAG_E_UNSUPPORTED;
  UpdB3Args a;
  memset(&a, 0, sizeof(a));
  a.A = h; a.W = W; a.bias = b; a.add = nbr; a.w_s = w_s; a.b_s = b_s; a.mask = mask; a.C = h_out; a.score = score;
  a.M = (int32_t)BN; a.D = D; a.ldw = ldw; a.ct0 = kTabNTH;
  a.add_flag = add_flag;
  if (add_flag && ((uintptr_t)add_flag & 3)) return GNNRAG_E_UNSUPPORTED;
  int cus = 0;
  {
    const int rc = device_cu_count(&cus);
    if (rc) return rc;
  }
  const int chunks = b3_row_chunks(cus / 2, (BN + 15) / 16);
  if (!score_zeroed) GNNRAG_HIP(hipMemsetAsync(score, 0, (size_t)BN * sizeof(float), stream));
  static DeviceMask cap, cap_f;
  {
    const int rc = add_flag ? raise_lds_cap(k_update_b3<true>, cap_f) : raise_lds_cap(k_update_b3<false>, cap);
    if (rc) return rc;
  }
  const int nblk = ((chunks + 7) / 8) * 16;
  if (add_flag) hipLaunchKernelGGL(k_update_b3<true>, dim3(nblk), dim3(512), 160 * 1024, stream, a, chunks);
  else hipLaunchKernelGGL(k_update_b3<false>, dim3(nblk), dim3(512), 160 * 1024, stream, a, chunks);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

size_t tables_vq_planes_bytes(int64_t R1) { return (size_t)2 * 3 * R1 * kVqRowB; }
size_t tables_vq_packed_bytes(int64_t R1) { return (size_t)2 * R1 * kVqPackRowB; }
static_assert(2 * kVqPackRowB <= 2 * 3 * kVqRowB, "a layer's packed operand fits the slot of its planes");

bool tables_vq_shape_ok(int32_t D, int32_t I) {
  return b3_shape_ok(D) && I >= 1 && (size_t)I * D * sizeof(float) <= (size_t)kTabQBytes;
}

int tables_vq_launch(const gnnrag_csr* csr, const void* planes, const float* ins, const float* W, float* P, int32_t D,
                     int32_t I, int32_t only_dir, hipStream_t stream) {
  return tables_vq_launch_z(csr, planes, ins, W, P, D, I, only_dir, nullptr, 0, stream, false);
}

int tables_vq_launch_z(const gnnrag_csr* csr, const void* planes, const float* ins, const float* W, float* P, int32_t D,
                       int32_t I, int32_t only_dir, float* zero, int64_t zero_n, hipStream_t stream, bool packed) {
  if (!tables_vq_shape_ok(D, I) || csr->rel_total < 1024 || only_dir > 1) return GNNRAG_E_UNSUPPORTED;
  // (32-bit byte offsets from the operand's base)
  if ((int64_t)csr->R1 * (packed ? kVqPackRowB : kVqRowB) >= ((int64_t)1 << 32)) return GNNRAG_E_UNSUPPORTED;
  if (!aligned16(planes, ins, W, P)) return GNNRAG_E_UNSUPPORTED;
  VqArgs a;
  memset(&a, 0, sizeof(a));
  a.planes = (const unsigned char*)planes; a.ins = ins; a.W = W; a.P = P;
  a.rows = (const int2*)csr->rel_rows; a.rel_off = csr->rel_off;
  a.M = csr->rel_total; a.D = D; a.I = I; a.ldw = (2 * I + 1) * D; a.R1 = csr->R1;
  const int NT = (D + 15) / 16;
  a.ct0 = (NT + 1) / 2;
  int cus = 0;
  {
    const int rc = device_cu_count(&cus);
    if (rc) return rc;
  }
  // one workgroup per (question, direction, column part) fills the chip from 64 questions on; smaller batches cut a
  // question's rows into chunks (each builds the question's V again), as long as a chunk keeps >= 8 tiles
  const int ndir = only_dir < 0 ? 2 : 1;
  a.dir0 = only_dir < 0 ? 0 : only_dir;
  int nchunk = cus / (csr->B * 2 * ndir);
  const int tiles_max = (csr->rel_max + 15) / 16;
  if (nchunk > tiles_max / 8) nchunk = tiles_max / 8;
  if (nchunk < 1) nchunk = 1;
  a.nchunk = nchunk;
  a.zero = zero;
  a.zero_n = zero ? zero_n : 0;
  static DeviceMask cap, cap_p;
  {
    const int rc = packed ? raise_lds_cap(k_tables_vq<true>, cap_p) : raise_lds_cap(k_tables_vq<false>, cap);
    if (rc) return rc;
  }
  if (packed) hipLaunchKernelGGL(k_tables_vq<true>, dim3(csr->B * nchunk, ndir, 2), dim3(512), 160 * 1024, stream, a);
  else hipLaunchKernelGGL(k_tables_vq<false>, dim3(csr->B * nchunk, ndir, 2), dim3(512), 160 * 1024, stream, a);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

int tables_b3_launch(const gnnrag_csr* csr, const float* T_fwd, const float* T_inv, const float* ins, const float* W,
                     float* P, int32_t D, int32_t I, hipStream_t stream) {
  // shapes of the kernel: b3_shape_ok, 4-byte offsets that keep float4 accesses aligned, enough rows to fill the chip
  if (!b3_shape_ok(D) || csr->rel_total < 1024) return GNNRAG_E_UNSUPPORTED;
  if (!aligned16(T_fwd, T_inv, ins, W, P)) return GNNRAG_E_UNSUPPORTED;
  TabArgs a;
  memset(&a, 0, sizeof(a));
  a.T[0] = T_fwd; a.T[1] = T_inv; a.ins = ins; a.W = W; a.P = P;
  a.rows = (const int2*)csr->rel_rows;
  a.M = csr->rel_total; a.D = D; a.I = I; a.ldw = (2 * I + 1) * D;
  const int NT = (D + 15) / 16;
  a.ct0 = NT <= kTabNTH ? NT : (NT + 1) / 2;
  const int parts = NT <= kTabNTH ? 1 : 2;
  int cus = 0;
  {
    const int rc = device_cu_count(&cus);
    if (rc) return rc;
  }
  const long long U = ((long long)a.M + 15) / 16;
  const int chunks = b3_row_chunks(cus / (2 * parts), U);
  const int tiles_per_wave = (int)((((U + chunks - 1) / chunks) + 7) / 8);         // largest w1 - w0 of the floor split
  a.npass = (tiles_per_wave + kTabTPW - 1) / kTabTPW;
  const size_t lds = 160 * 1024;          // three weight planes, 64 B of slack, instruction rows
  static DeviceMask cap;
  {
    const int rc = raise_lds_cap(k_tables_b3, cap);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_tables_b3, dim3(chunks, 2, parts), dim3(512), lds, stream, a);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

}  // namespace gnnrag

extern "C" int gnnrag_relation_tables_planes(const gnnrag_csr* csr, const void* planes, const float* ins, const float* W,
                                             float* P, int32_t D, int32_t I, gnnrag_stream_t stream) {
  if (!csr || !planes || !ins || !W || !P || D <= 0 || I <= 0 || csr->rel_total < 0) return GNNRAG_E_BADARG;
  if (csr->rel_total == 0) return 0;
  return gnnrag::tables_vq_launch(csr, planes, ins, W, P, D, I, -1, (hipStream_t)stream);
}

extern "C" int gnnrag_relation_tables_packed(const gnnrag_csr* csr, const void* packed, const float* ins, const float* W,
                                             float* P, int32_t D, int32_t I, int32_t only_dir, gnnrag_stream_t stream) {
  if (!csr || !packed || !ins || !W || !P || D <= 0 || I <= 0 || csr->rel_total < 0 || only_dir < -1 || only_dir > 1)
    return GNNRAG_E_BADARG;
  if (csr->rel_total == 0) return 0;
  return gnnrag::tables_vq_launch_z(csr, packed, ins, W, P, D, I, only_dir, nullptr, 0, (hipStream_t)stream, true);
}
