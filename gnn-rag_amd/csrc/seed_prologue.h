// The device bodies of the two launches in front of a seed layer - the relation projections of all layers
// (rel_transform.hip) and the frontier of the seed distribution (frontier.hip) - as functions, so that one launch can run
// either in a workgroup (k_seed_prologue) while the stand-alone kernels stay thin wrappers around them.
#pragma once
#include "gnnrag_common.h"

namespace gnnrag {

constexpr int kRtMaxL = 8;        // layers per launch (more layers: more launches)
constexpr int kRtUnroll = 7;      // k groups (16 columns each) of A in flight per wave: K = 200 -> 13 groups -> 2 rounds
constexpr int kRtStage = 16;      // pieces of the weight slice a thread requests before it waits (one per k group)

struct RelTArgs {
  const float* A[2];              // rel_features, rel_features_inv  [M, K]
  const float* W[kRtMaxL];        // rel_linear{j}.weight [N, K]
  const float* b[kRtMaxL];        // rel_linear{j}.bias [N] or null
  const float* add[kRtMaxL][2];   // pos_emb{j} / pos_emb_inv{j} [add_rows, N] or null
  float* C;                       // [L][2][M][N]
  unsigned short* planes;         // null or [L][2][3][M][kPlaneRow] bf16: planes of relu(T) | relu(-T), see below
  unsigned char* packed;          // null or [L][2][M][kPackRowB]: planes of |T| and its signs, see below (never both)
  int M, K, N, add_rows;
};

// Planes for the "V form" of the relation tables (tables_b3.hip: k_tables_vq): per (layer, direction) three bf16
// planes (exact 3-way split) of [relu(T[r, :]) | relu(-T[r, :])], each half padded with zeros to 7 k blocks of 32.
constexpr int kPlaneHalf = 224;
constexpr int kPlaneRow = 2 * kPlaneHalf;     // bf16 elements per plane row (896 bytes)
// The same operand as the sparse product of k_tables_vq takes it ("packed"): of relu(T) and relu(-T) at most one is not
// zero, so the compressed left operand of v_smfmac is the three planes of |T| plus one sign bit per element.  Per (layer,
// direction, relation row) kPackRowB bytes: three planes of |T| (kPlaneHalf bf16 each, k >= D zero), then 64 index bytes.
// The index byte of the four k of group q = k / 4 is 0x88 | s0 | s1 << 2 | s2 << 4 | s3 << 6 with s = (T[r, k] < 0): two
// of them are the finished 16-bit index word of a lane's 8 k (positions 0 / 1 for the first value of a pair, 2 / 3 for the
// second).  They are stored in the order the lanes read them - the byte of q at (q % 8 / 2) * 16 + (q / 8) * 2 + q % 2,
// i.e. the word of (k block q / 8, lane group fg = q % 8 / 2) at fg * 16 + block * 2 - so that a lane's planes and its
// index word share one lane offset (fg * 16).  The 8 bytes no k stands behind are 0.
// -0.0 and values whose three planes are all zero (fp32 denormals below the smallest bf16) may get either sign bit: their
// operand is zero, and 0 times either half of the (finite) right operand adds nothing to a sum that starts at +0.
constexpr int kPackPlaneB = kPlaneHalf * 2;             // bytes per plane of a packed row (448)
constexpr int kPackIdxB = 3 * kPackPlaneB;              // offset of the index bytes (1344)
constexpr int kPackRowB = kPackIdxB + 64;               // 1408

// one round of a lane's A fragments: k groups c0 .. c0 + kRtUnroll - 1 of its row; k groups past K: a clamped (valid)
// address, zeroed at use - no branch around a load
__device__ __forceinline__ void load_a_round(const float* __restrict__ ap, int c0, int fg, int K, f32x4 (&av)[kRtUnroll]) {
#pragma unroll
  for (int u = 0; u < kRtUnroll; ++u) av[u] = *reinterpret_cast<const f32x4*>(ap + min(16 * (c0 + u) + 4 * fg, K - 4));
}

// TPW: 16-row tiles per wave (1: few relation rows, many small workgroups; 4: large vocabularies, the weight slice
// staged once per 256 rows)
// Workgroup (bx, by, bz) of 256 threads = (row block, column group, 2 * layer + direction); Wf: the workgroup's dynamic
// LDS, where the weight slice goes in FRAGMENT order, see below
template <int TPW>
__device__ __forceinline__ void rel_transform_body(const RelTArgs& g, int bx, int by, int bz, float* Wf) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int j = bz >> 1, d = bz & 1;
  const int colg = by * 64;                                  // this workgroup's 64 columns: four MFMA tiles
  const int K = g.K;
  const int nch = (K + 15) >> 4;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const bool compute = colg < g.N;                           // (column groups past N only write the planes' zero padding)
  // column slot fr of tile a stands for column colg + 4 fr + a: a lane ends up with 4 CONSECUTIVE columns of its rows
  // (16-byte stores of T, 8-byte stores of the bf16 planes).  LDS holds W[colg .. colg+63][:] as the lanes will read
  // it: float4 number ((c * 4 + a) * 64 + lane) = W[colg + 4 fr + a][16 c + 4 fg ..] - one contiguous KB per
  // (k group c, tile a) and wave instruction, conflict free.
  // Staging: wave w moves tile a = w of every k group, lane l the float4 fgq = l & 3 of column slot frq = l >> 2 - piece i
  // of a thread is k group c = i of ITS row of W, nch pieces in all.  All of a round's pieces (kRtStage: every admitted
  // D <= 256 in one round) are requested before the first is written to LDS; addresses past N / K are clamped to valid
  // ones and the value zeroed at use - no branch around a load.
  const float* __restrict__ ap0 = g.A[d] + (size_t)min(bx * TPW * 64 + wave * 16 + fr, g.M - 1) * K;
  f32x4 av[kRtUnroll];
  if (compute) {
    const int a = wave, frq = lane >> 2, fgq = lane & 3;
    const int col = colg + 4 * frq + a;
    const float* __restrict__ wrow = g.W[j] + (size_t)min(col, g.N - 1) * K;
    float* __restrict__ wdst = Wf + (size_t)(a * 64 + fgq * 16 + frq) * 4;
    // (pieces past the last k group repeat it - same address, same value: neither a branch around a load nor one around
    // a write, which would let the compiler move the load to the write)
    f32x4 wv[kRtStage];
    auto request = [&](int i0) {
#pragma unroll
      for (int u = 0; u < kRtStage; ++u)
        wv[u] = *reinterpret_cast<const f32x4*>(wrow + min(16 * min(i0 + u, nch - 1) + 4 * fgq, K - 4));
    };
    auto write = [&](int i0) {
#pragma unroll
      for (int u = 0; u < kRtStage; ++u) {
        const int i = min(i0 + u, nch - 1);
        const bool live = col < g.N && 16 * i + 4 * fgq < K;
        *reinterpret_cast<f32x4*>(wdst + (size_t)i * 1024) = live ? wv[u] : zero4;
      }
    };
    request(0);
    // the tile's first round of A fragments does not depend on LDS: requested behind the slice, in front of the barrier
    load_a_round(ap0, 0, fg, K, av);
    __builtin_amdgcn_sched_barrier(0);                       // every request stands in front of the first wait
    write(0);
    for (int i0 = kRtStage; i0 < nch; i0 += kRtStage) {      // (D > 256)
      request(i0);
      write(i0);
    }
  }
  __syncthreads();
  const int c4 = colg + 4 * fr;
  const bool in_T = c4 < g.N;                                // (N % 4 == 0: a lane's 4 columns are all in or all out)
  const bool in_pad = !in_T && c4 < kPlaneHalf;
  f32x4 bias = zero4;
  const float* __restrict__ bp = g.b[j];
  if (in_T && bp) bias = *reinterpret_cast<const f32x4*>(bp + c4);
  const float* __restrict__ addp = g.add[j][d];
  float* __restrict__ cp = g.C + ((size_t)(2 * j + d) * g.M) * g.N;
  unsigned short* pp = g.planes ? g.planes + ((size_t)(2 * j + d) * 3 * g.M) * kPlaneRow : nullptr;
  unsigned char* pk = g.packed ? g.packed + ((size_t)(2 * j + d) * g.M) * kPackRowB : nullptr;

#pragma unroll 1
  for (int t = 0; t < TPW; ++t) {
    const int row0 = (bx * TPW + t) * 64 + wave * 16;
    if (row0 >= g.M) break;
    f32x4 acc[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a][0] = acc[a][1] = zero4;
    if (compute) {
      // rows past the end read the last valid one (never stored); the A fragments come straight from global memory
      const float* __restrict__ ap = g.A[d] + (size_t)min(row0 + fr, g.M - 1) * K;
      if (t > 0) load_a_round(ap, 0, fg, K, av);             // (tile 0's first round: in front of the staging barrier)
      for (int c0 = 0; c0 < nch; c0 += kRtUnroll) {
        // the next round is requested in front of this round's products
        f32x4 nx[kRtUnroll];
        const bool more = c0 + kRtUnroll < nch;
        if (more) load_a_round(ap, c0 + kRtUnroll, fg, K, nx);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kRtUnroll; ++u) {
          const int c = min(c0 + u, nch - 1);
          const bool live = 16 * (c0 + u) + 4 * fg < K;
          const f32x4 x = live ? av[u] : zero4;
          f32x4 wv[4];
#pragma unroll
          for (int a = 0; a < 4; ++a) wv[a] = *reinterpret_cast<const f32x4*>(Wf + ((size_t)((c * 4 + a) * 64 + lane)) * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int a = 0; a < 4; ++a)
              acc[a][e & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[e], wv[a][e], acc[a][e & 1], 0, 0, 0);
        }
        if (more) {
#pragma unroll
          for (int u = 0; u < kRtUnroll; ++u) av[u] = nx[u];
        }
      }
    }
    // accumulator element r of lane (fr, fg), tile a = C[row0 + 4 fg + r][colg + 4 fr + a]
    if (!in_T && !(pp && in_pad) && !pk) continue;
    // the lane's four pos_emb rows, requested together (rows past add_rows: a clamped address, not added)
    f32x4 addv[4] = {zero4, zero4, zero4, zero4};
    if (in_T && addp && g.add_rows > 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        addv[r] = *reinterpret_cast<const f32x4*>(addp + (size_t)min(row0 + 4 * fg + r, g.add_rows - 1) * g.N + c4);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * fg + r;
      if (row >= g.M) continue;
      f32x4 v = zero4;
      if (in_T) {
#pragma unroll
        for (int a = 0; a < 4; ++a) v[a] = acc[a][0][r] + acc[a][1][r];
        v += bias;
        if (addp && row < g.add_rows) v += addv[r];
        *reinterpret_cast<f32x4*>(cp + (size_t)row * g.N + c4) = v;
      }
      if (pp) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          // exact 3-way bf16 split of relu(+-T) (gnnrag_common.h: split3); the padding columns get zeros
          const Split3 sp = split3(__builtin_elementwise_max(half ? -v : v, zero4));
          const size_t e = (size_t)row * kPlaneRow + half * kPlaneHalf + c4;
          *reinterpret_cast<uint2*>(pp + e) = sp.hi;
          *reinterpret_cast<uint2*>(pp + (size_t)g.M * kPlaneRow + e) = sp.mid;
          *reinterpret_cast<uint2*>(pp + (size_t)2 * g.M * kPlaneRow + e) = sp.lo;
        }
      }
      if (pk) {
        // the same register values, packed: split3(|v|) and the signs; padding columns get zero planes and "all +"
        unsigned char* rowp = pk + (size_t)row * kPackRowB;
        if (c4 < kPlaneHalf) {
          const Split3 sp = split3(__builtin_elementwise_abs(v));
          *reinterpret_cast<uint2*>(rowp + 2 * c4) = sp.hi;
          *reinterpret_cast<uint2*>(rowp + kPackPlaneB + 2 * c4) = sp.mid;
          *reinterpret_cast<uint2*>(rowp + 2 * kPackPlaneB + 2 * c4) = sp.lo;
        }
        const int q = c4 >> 2;                               // (the column groups run on to 256: q < 64)
        const unsigned ix = 0x88u | (unsigned)(v[0] < 0.f) | (unsigned)(v[1] < 0.f) << 2 | (unsigned)(v[2] < 0.f) << 4 |
                            (unsigned)(v[3] < 0.f) << 6;
        rowp[kPackIdxB + ((q & 7) >> 1) * 16 + (q >> 3) * 2 + (q & 1)] = (unsigned char)(c4 < kPlaneHalf ? ix : 0u);
      }
    }
  }
}

// ---- frontier of one question ---------------------------------------------------------------------------------------
// Question g of nq, by a workgroup of NT threads (the zeroing side jobs are shared out over the nq workgroups); its LDS:
// s_seed [kFrSeedCap], s_ns [1], s_wsum [kFrPass / 64].  The lists, counts and flags do not depend on NT: the compaction is
// ordered, and the seeds' LDS order (atomic) only decides the order in which their facts set flags.
// kFrSeedCap / kFrAltSeeds: frontier.hip's constants of these names (it passes them; k_seed_prologue takes them from here)
constexpr int kSpSeedCap = 2048, kSpAltSeeds = 32;
constexpr int kFrPass = 2048;             // node slots / flags per pass: kFrPass / NT per thread in flight
constexpr int kFrLdsInts = kSpSeedCap + 1 + kFrPass / 64;   // s_wsum: one count per (round, wave) of a pass
template <int NT, int kFrSeedCap = kSpSeedCap, int kFrAltSeeds = kSpAltSeeds>
__device__ __forceinline__ void frontier_body(
    const float* __restrict__ dist, const int32_t* __restrict__ rp0, const int32_t* __restrict__ rp1,
    const int2* __restrict__ el0, const int2* __restrict__ el1, const int32_t* __restrict__ rel_off, int N,
    uint8_t* __restrict__ row_flag, int32_t* __restrict__ rows, uint8_t* __restrict__ tflag,
    int32_t* __restrict__ trows, int32_t* __restrict__ counts, int32_t* __restrict__ seeds,
    int32_t* __restrict__ seedinfo, float* __restrict__ zero_a, long long zero_na, float* __restrict__ zero_b,
    long long zero_nb, int g, int nq, int* s_seed, int& s_ns, int* s_wsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int roff = rel_off[g], Rg = rel_off[g + 1] - roff;
  const size_t n0 = (size_t)g * N;
  // side jobs of this launch (it runs in front of the layer's other kernels): zero the score buffer the bf16x3 update
  // accumulates onto, and the zero row behind nbr that unflagged rows read
  for (long long i = (long long)g * NT + tid; i < zero_na; i += (long long)nq * NT) zero_a[i] = 0.f;
  for (long long i = (long long)g * NT + tid; i < zero_nb; i += (long long)nq * NT) zero_b[i] = 0.f;
  if (tid == 0) s_ns = 0;
  if (g == nq - 1 && tid < 64) row_flag[(size_t)nq * N + tid] = 0;     // the padding behind the flags
  for (int i = tid; i < N; i += NT) row_flag[n0 + i] = 0;
  for (int i = tid; i < Rg; i += NT) tflag[roff + i] = 0;
  __syncthreads();
  // a pass = kFrPass node slots, U per thread: all of a thread's values are requested before the first is looked at
  constexpr int U = kFrPass / NT;
  for (int i0 = 0; i0 < N; i0 += kFrPass) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * NT + tid;
      v[u] = i < N ? dist[n0 + i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (v[u] != 0.f) {
        const int k = atomicAdd(&s_ns, 1);
        if (k < kFrSeedCap) s_seed[k] = (int)n0 + i0 + u * NT + tid;
      }
    }
  }
  __syncthreads();
  const int ns = s_ns;
  if (tid == 0) {
    // the seeds in ascending order and the number of facts that touch them, for k_walk_frontier: a listed HUB finds its
    // few facts from a seed in the seeds' short rows instead of scanning its own (the LDS list is in atomic order)
    int cnt = -1, facts = 0;
    if (ns <= kFrAltSeeds) {
      cnt = ns;
      for (int i = 1; i < ns; ++i) {
        const int v = s_seed[i];
        int j = i - 1;
        for (; j >= 0 && s_seed[j] > v; --j) s_seed[j + 1] = s_seed[j];
        s_seed[j + 1] = v;
      }
      for (int i = 0; i < ns; ++i) {
        const int sn = s_seed[i];
        seeds[g * kFrAltSeeds + i] = sn;
        facts += (rp0[sn + 1] - rp0[sn]) + (rp1[sn + 1] - rp1[sn]);
      }
    }
    seedinfo[2 * g] = cnt;
    seedinfo[2 * g + 1] = facts;
  }
  __syncthreads();
  if (ns > kFrSeedCap) {                   // not a seed distribution: everything is frontier
    for (int i = tid; i < N; i += NT) row_flag[n0 + i] = 1;
    for (int i = tid; i < Rg; i += NT) tflag[roff + i] = 1;
  } else {
    for (int k = 0; k < ns; ++k) {
      const int s = s_seed[k];
#pragma unroll
      for (int dd = 0; dd < 2; ++dd) {     // row s of structure dd = the facts of direction 1 - dd that START at s
        const int32_t* rp = dd ? rp1 : rp0;
        const int2* el = dd ? el1 : el0;
        const int beg = rp[s], end = rp[s + 1];
        for (int j = beg + tid; j < end; j += NT) {
          const int2 e = el[j];            // (destination of the fact in direction 1 - dd, compact relation)
          row_flag[e.x] = 1;
          tflag[roff + e.y] = 1;
        }
      }
    }
  }
  __syncthreads();
  // ordered compaction (ballot + wave prefix) into the question's own list segment
  auto compact = [&](const uint8_t* flag, int n, int first, int32_t* list, int32_t* count_out) {
    // a pass = U rounds of NT flags (position = c0 + u NT + tid, i.e. list order = (round, wave, lane)), all loaded before
    // any is looked at; every (round, wave) count goes to LDS, ONE barrier, then each lane adds up the counts in front of it
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += kFrPass) {
      uint8_t fl[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = c0 + u * NT + tid;
        fl[u] = i < n ? flag[i] : (uint8_t)0;
      }
      unsigned long long mk[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        mk[u] = __ballot(fl[u] != 0);
        if (lane == 0) s_wsum[u * (NT / 64) + wave] = __popcll(mk[u]);
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < U; ++u) {
        int off = base;
        for (int w = 0; w < NT / 64; ++w) {
          const int c = s_wsum[u * (NT / 64) + w];
          if (w < wave) off += c;
          base += c;
        }
        if (fl[u] != 0) list[off + __popcll(mk[u] & ((1ull << lane) - 1))] = first + c0 + u * NT + tid;
      }
      __syncthreads();
    }
    if (tid == 0) *count_out = base;
  };
  compact(row_flag + n0, N, (int)n0, rows + n0, counts + 2 * g);
  compact(tflag + roff, Rg, roff, trows + roff, counts + 2 * g + 1);
}

struct FrontierArgs {                     // k_frontier_build's arguments, for the launch that runs it beside the projections
  const float* dist;
  const int32_t* rp0;
  const int32_t* rp1;
  const int2* el0;
  const int2* el1;
  const int32_t* rel_off;
  uint8_t* row_flag;
  int32_t* rows;
  uint8_t* tflag;
  int32_t* trows;
  int32_t* counts;
  int32_t* seeds;
  int32_t* seedinfo;
  float* zero_a;
  float* zero_b;
  long long zero_na, zero_nb;
  int N, B;
};

}  // namespace gnnrag
