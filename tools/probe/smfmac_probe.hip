// Probe for the 2:4 structured-sparse bf16 matrix instruction of gfx950, v_smfmac_f32_16x16x64_bf16 (DESIGN.md
// Appendix; the findings are repeated above k_tables_vq in gnn-rag_amd/csrc/tables_b3.hip).  Stand-alone, HIP runtime only:
//   hipcc --offload-arch=gfx950 -O3 -o tools/probe/smfmac_probe tools/probe/smfmac_probe.hip && tools/probe/smfmac_probe
// Part 1 (layout, one wave): one instruction on random operands with random VALID index words (ascending positions in
//   every group of four), compared on the host against every combination of candidate layouts for the compressed A
//   operand (8 bf16 per lane), the dense B operand (16 bf16 per lane), the position of the 2-bit indices in the index
//   register and the meaning of abid.  The accumulator layout is the dense 16x16 one in all candidates (row 4 (lane/16)
//   + q, column lane % 16).  Exactly one combination may match (operand values are small integers: products and sums
//   are exact, so "match" is bit equality).
// Part 2 (rate): a long run of the sparse instruction on 8 independent accumulators, then the same count of the dense
//   v_mfma_f32_16x16x32_bf16, one workgroup per CU at one and two waves per SIMD.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));
typedef unsigned short u16;

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

struct U8 { u16 v[8]; };
struct U16 { u16 v[16]; };

// ---- part 1: one instruction, one wave ----
template <int ABID>
__global__ __launch_bounds__(64) void k_one(const U8* a, const U16* b, const unsigned* idx, f32x4* c) {
  const int lane = threadIdx.x;
  const bf16x8 av = __builtin_bit_cast(bf16x8, a[lane]);
  const bf16x16 bv = __builtin_bit_cast(bf16x16, b[lane]);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(av, bv, acc, (int)idx[lane], 0, ABID);
  c[lane] = acc;
}

// ---- part 2: issue rate ----
template <bool SPARSE>
__global__ __launch_bounds__(512) void k_rate(const float* __restrict__ src, float* __restrict__ dst, int loops) {
  f32x4 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const f32x4 v0 = *reinterpret_cast<const f32x4*>(src + threadIdx.x * 4);
  const f32x4 v1 = *reinterpret_cast<const f32x4*>(src + 4096 + threadIdx.x * 4);
  const f32x4 v2 = *reinterpret_cast<const f32x4*>(src + 8192 + threadIdx.x * 4);
  const bf16x8 a = __builtin_bit_cast(bf16x8, v0);
  const bf16x8 b8 = __builtin_bit_cast(bf16x8, v1);
  struct { f32x4 lo, hi; } b2 = {v1, v2};
  const bf16x16 b16 = __builtin_bit_cast(bf16x16, b2);
  int idx = 0x44444444;            // positions (0, 1) in every group: valid
  for (int it = 0; it < loops; ++it) {
    asm volatile("" : "+v"(idx));
#pragma unroll
    for (int m = 0; m < 48; ++m) {
      if (SPARSE) acc[m % 8] = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(a, b16, acc[m % 8], idx, 0, 0);
      else acc[m % 8] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b8, acc[m % 8], 0, 0, 0);
    }
  }
  f32x4 s = acc[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) s += acc[i];
  if (s[0] == 1234.567f) dst[threadIdx.x] = s[0] + s[1] + s[2] + s[3];
}

static u16 bf16_of_int(int v) {       // small integers are exact in bf16
  float f = (float)v;
  unsigned u;
  memcpy(&u, &f, 4);
  return (u16)(u >> 16);
}
static float f_of_bf16(u16 h) {
  unsigned u = (unsigned)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

static unsigned rng_state = 12345u;
static unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// candidate layouts
//  A: 0: lane holds compressed k 8 (lane/16) + e of row lane % 16
//     1: two 16-wide halves: e < 4: 4 (lane/16) + e, e >= 4: 16 + 4 (lane/16) + e - 4
//  B: 0: lane holds k 16 (lane/16) + e of column lane % 16
//     1: two 32-wide halves: e < 8: 8 (lane/16) + e, e >= 8: 32 + 8 (lane/16) + e - 8
//  X: 0: the lane's 16 index bits are (idx >> 16 abid) & 0xffff, field of compressed element e at bits 2 e
//     1: abid ignored, low 16 bits
//     2: abid ignored, high 16 bits
//     3: the lane's 16 index bits are bytes abid and abid + 2
static int a_ck(int A, int lane, int e) {
  const int g = lane >> 4;
  return A == 0 ? 8 * g + e : (e < 4 ? 4 * g + e : 16 + 4 * g + e - 4);
}
static int b_k(int B, int lane, int e) {
  const int g = lane >> 4;
  return B == 0 ? 16 * g + e : (e < 8 ? 8 * g + e : 32 + 8 * g + e - 8);
}
static unsigned idx16(int X, unsigned w, int abid) {
  switch (X) {
    case 0: return (w >> (16 * abid)) & 0xffffu;
    case 1: return w & 0xffffu;
    case 2: return w >> 16;
    default: return ((w >> (8 * abid)) & 0xffu) | (((w >> (8 * abid + 16)) & 0xffu) << 8);
  }
}

int main() {
  U8* da; U16* db; unsigned* di; f32x4* dc;
  CHECK(hipMalloc(&da, 64 * sizeof(U8)));
  CHECK(hipMalloc(&db, 64 * sizeof(U16)));
  CHECK(hipMalloc(&di, 64 * 4));
  CHECK(hipMalloc(&dc, 64 * sizeof(f32x4)));
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  printf("device: %s (%s), %d CUs\n", prop.name, prop.gcnArchName, prop.multiProcessorCount);

  printf("== layout: v_smfmac_f32_16x16x64_bf16, one wave, random small-integer operands, random valid indices ==\n");
  static const unsigned pairs[6] = {0x4, 0x8, 0xC, 0x9, 0xD, 0xE};      // (idx0 | idx1 << 2) with idx0 < idx1
  int nmatch_total[2][2][4] = {};
  const int ntrial = 8;
  for (int trial = 0; trial < ntrial; ++trial) {
    const int abid = trial & 1;
    std::vector<U8> ha(64);
    std::vector<U16> hb(64);
    std::vector<unsigned> hi(64);
    for (int l = 0; l < 64; ++l) {
      for (int e = 0; e < 8; ++e) ha[l].v[e] = bf16_of_int((int)(rnd() % 15) - 7);
      for (int e = 0; e < 16; ++e) hb[l].v[e] = bf16_of_int((int)(rnd() % 15) - 7);
      unsigned w = 0;
      for (int gq = 0; gq < 8; ++gq) w |= pairs[rnd() % 6] << (4 * gq);
      hi[l] = w;
    }
    CHECK(hipMemcpy(da, ha.data(), 64 * sizeof(U8), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(db, hb.data(), 64 * sizeof(U16), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(di, hi.data(), 64 * 4, hipMemcpyHostToDevice));
    if (abid) hipLaunchKernelGGL(k_one<1>, dim3(1), dim3(64), 0, 0, da, db, di, dc);
    else hipLaunchKernelGGL(k_one<0>, dim3(1), dim3(64), 0, 0, da, db, di, dc);
    CHECK(hipDeviceSynchronize());
    std::vector<f32x4> hc(64);
    CHECK(hipMemcpy(hc.data(), dc, 64 * sizeof(f32x4), hipMemcpyDeviceToHost));
    for (int A = 0; A < 2; ++A)
      for (int B = 0; B < 2; ++B)
        for (int X = 0; X < 4; ++X) {
          float Ad[16][64] = {}, Bd[64][16];
          for (int l = 0; l < 64; ++l) {
            const unsigned bits = idx16(X, hi[l], abid);
            for (int e = 0; e < 8; ++e) {
              const int ck = a_ck(A, l, e);                    // compressed k of the row: group ck / 2
              const int pos = (bits >> (2 * e)) & 3;
              Ad[l & 15][4 * (ck >> 1) + pos] += f_of_bf16(ha[l].v[e]);
            }
            for (int e = 0; e < 16; ++e) Bd[b_k(B, l, e)][l & 15] = f_of_bf16(hb[l].v[e]);
          }
          int bad = 0;
          for (int l = 0; l < 64; ++l)
            for (int q = 0; q < 4; ++q) {
              const int row = 4 * (l >> 4) + q, col = l & 15;
              float s = 0.f;
              for (int k = 0; k < 64; ++k) s += Ad[row][k] * Bd[k][col];
              bad += s != hc[l][q];
            }
          if (!bad) ++nmatch_total[A][B][X];
          if (trial == 0 || !bad) printf("trial %d abid %d  A%d B%d X%d: %s (%d of 256 differ)\n", trial, abid, A, B, X, bad ? "no" : "MATCH", bad);
        }
  }
  int winners = 0;
  for (int A = 0; A < 2; ++A)
    for (int B = 0; B < 2; ++B)
      for (int X = 0; X < 4; ++X)
        if (nmatch_total[A][B][X] == ntrial) {
          ++winners;
          printf("LAYOUT: A%d B%d X%d matches all %d trials (both abid values)\n", A, B, X, ntrial);
        }
  if (winners != 1) printf("LAYOUT: %d candidates match every trial - NOT settled\n", winners);

  // one-hot dumps (raw, for the record): B[lane 0..63 step 16, e] = 1 with A all ones and index (0,1) / (2,3) everywhere
  printf("== one-hot record: A compressed all 1; B one-hot at (lane, e); reported: which index pairs see it and in which C column ==\n");
  for (int l0 = 0; l0 < 64; l0 += 16)
    for (int e0 = 0; e0 < 16; ++e0) {
      printf("B(lane %2d, e %2d):", l0 + 3, e0);
      for (int pr = 0; pr < 6; ++pr) {
        std::vector<U8> ha(64);
        std::vector<U16> hb(64);
        std::vector<unsigned> hi(64, pairs[pr] * 0x11111111u);
        for (int l = 0; l < 64; ++l) {
          for (int e = 0; e < 8; ++e) ha[l].v[e] = bf16_of_int(e & 1 ? 2 : 1);     // idx0's value 1, idx1's value 2
          for (int e = 0; e < 16; ++e) hb[l].v[e] = 0;
        }
        hb[l0 + 3].v[e0] = bf16_of_int(1);
        CHECK(hipMemcpy(da, ha.data(), 64 * sizeof(U8), hipMemcpyHostToDevice));
        CHECK(hipMemcpy(db, hb.data(), 64 * sizeof(U16), hipMemcpyHostToDevice));
        CHECK(hipMemcpy(di, hi.data(), 64 * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_one<0>, dim3(1), dim3(64), 0, 0, da, db, di, dc);
        CHECK(hipDeviceSynchronize());
        std::vector<f32x4> hc(64);
        CHECK(hipMemcpy(hc.data(), dc, 64 * sizeof(f32x4), hipMemcpyDeviceToHost));
        // C[row 0][col 3] lives in lane 3, q 0
        printf(" idx(%d,%d)->%g", (int)(pairs[pr] & 3), (int)(pairs[pr] >> 2), hc[3][0]);
      }
      printf("\n");
    }

  // ---- rate ----
  printf("== rate: 8 independent accumulators, 48 instructions per loop, one workgroup per CU ==\n");
  float *src, *dst;
  CHECK(hipMalloc(&src, 1 << 20));
  CHECK(hipMalloc(&dst, 1 << 20));
  std::vector<float> h(1 << 18);
  for (size_t i = 0; i < h.size(); ++i) h[i] = 0.001f * (float)((i * 2654435761u) % 1000) - 0.5f;
  CHECK(hipMemcpy(src, h.data(), 1 << 20, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const int loops = 4000, cus = prop.multiProcessorCount;
  printf("%-34s %9s %16s %22s\n", "case", "us", "ns/instr/SIMD", "dense-equivalent TFLOP/s");
  double rate[2][2] = {};
  for (int rep = 0; rep < 3; ++rep)
    for (int wps = 1; wps <= 2; ++wps)
      for (int sp = 0; sp < 2; ++sp) {
        CHECK(hipEventRecord(e0, 0));
        if (sp) hipLaunchKernelGGL(k_rate<true>, dim3(cus), dim3(256 * wps), 0, 0, src, dst, loops);
        else hipLaunchKernelGGL(k_rate<false>, dim3(cus), dim3(256 * wps), 0, 0, src, dst, loops);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (!rep) continue;      // warm-up
        const double n = (double)loops * 48 * wps;
        const double kk = sp ? 64 : 32;
        const double tf = n * 4 * cus * 2.0 * 16 * 16 * kk / (ms * 1e-3) / 1e12;
        rate[sp][wps - 1] = ms * 1e6 / n;
        printf("%-22s %dw/SIMD rep %d %9.1f %16.3f %22.1f\n", sp ? "smfmac 16x16x64 bf16" : "mfma 16x16x32 bf16", wps, rep, ms * 1e3,
               ms * 1e6 / n, tf);
      }
  for (int wps = 1; wps <= 2; ++wps)
    printf("RATE %dw/SIMD: sparse instruction takes %.2f x the dense one's time for 2 x the K -> K-rate ratio %.2f\n", wps,
           rate[1][wps - 1] / rate[0][wps - 1], 2.0 * rate[0][wps - 1] / rate[1][wps - 1]);
  return 0;
}
