// Relation projections of ALL layers of one iteration in one launch:
//
//   T[j][d][r, :] = rel_linear{j}(rel_features_d[r, :]) (+ pos_emb{j}_d[r, :])     reasongnn.py:75-79 / :102-105
//
// for layer j = 0..L-1 and direction d (forward / inverse relation features).  None of them depends on the node
// state or on the distribution, so the L x 2 skinny products ([R1, D] x [D, D], R1 = a few hundred to a few thousand
// relation rows) that used to head every layer call - each a ~13-25 us launch of a few dozen workgroups waiting on a
// dependent k loop - become one launch of (row blocks x column tiles x 2L) small workgroups in front of the layer
// sequence.  Exact fp32 on the matrix cores (v_mfma_f32_16x16x4_f32).
//
// Workgroup = 4 waves x (1 or 4) 16-row tiles x columns [64 by, +64) of T[z] as four MFMA tiles that share the A
// fragment.  The weight slice W[64 by .. +63][:] is staged ONCE per workgroup into LDS in fragment order (51 KB at
// K = 200); lane (fr, fg) loads the float4 A[row fr][16 c + 4 fg ..] of k group c straight from global memory
// (kRtUnroll groups in flight) and reads, per tile a, the float4 W[column 64 by + 4 fr + a][16 c + 4 fg ..] from LDS;
// component s of the float4s feeds MFMA s (the k order inside a group is a permutation both operands share).  The
// column slots are interleaved (slot fr of tile a = column 4 fr + a), so the epilogue stores 4 consecutive columns
// per lane - T as float4, the bf16 planes as 8-byte pieces.
#include "gnnrag_common.h"
#include "dense_internal.h"
#include "seed_prologue.h"

namespace gnnrag {

// (the kernel body: seed_prologue.h)
// TPW: 16-row tiles per wave (1: few relation rows, many small workgroups; 4: large vocabularies, the weight slice
// staged once per 256 rows)
template <int TPW>
__global__ __launch_bounds__(256) void k_rel_transform(RelTArgs g) {
  extern __shared__ __attribute__((aligned(16))) float Wf[];
  rel_transform_body<TPW>(g, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, Wf);
}

// The projections AND the frontier of the seed distribution in one launch: both are needed first by k_tables_frontier
// and neither reads what the other writes.  Workgroups [0, f.B) build the frontier of one question each (256 threads
// instead of k_frontier_build's 1024: more rounds of the same ordered compaction, the same lists), the others run
// workgroup (bx, by, bz) of k_rel_transform<1>'s grid (gx, gy, ..).  A workgroup runs one body or the other; nothing
// passes between workgroups.  The frontier's LDS lies at the head of the dynamic LDS the projection stages W in.
constexpr int kSpThreads = 256;
__global__ __launch_bounds__(kSpThreads) void k_seed_prologue(RelTArgs g, FrontierArgs f, int gx, int gy) {
  extern __shared__ __attribute__((aligned(16))) float Wf[];
  if ((int)blockIdx.x < f.B) {
    int* s = reinterpret_cast<int*>(Wf);
    frontier_body<kSpThreads>(f.dist, f.rp0, f.rp1, f.el0, f.el1, f.rel_off, f.N, f.row_flag, f.rows, f.tflag, f.trows,
                              f.counts, f.seeds, f.seedinfo, f.zero_a, f.zero_na, f.zero_b, f.zero_nb, (int)blockIdx.x, f.B,
                              s, s[kSpSeedCap], s + kSpSeedCap + 1);
    return;
  }
  const int r = (int)blockIdx.x - f.B;
  rel_transform_body<1>(g, r % gx, (r / gx) % gy, r / (gx * gy), Wf);
}

}  // namespace gnnrag

using namespace gnnrag;

extern "C" size_t gnnrag_rel_planes_bytes(int64_t R1, int32_t D, int32_t L) {
  if (R1 <= 0 || D <= 0 || D > kPlaneHalf || L <= 0) return 0;
  return (size_t)L * 2 * 3 * R1 * kPlaneRow * sizeof(unsigned short);
}

// THE acceptance test of gnnrag_rel_transform (shapes, offsets, alignment of every operand incl. the outputs, LDS) as
// one function: the layer stack's GNNRAG_PATH_REUSE_PROJ call asks it, with the real pointers, whether the projecting
// call took this kernel (and so wrote the planes) or fell back to the k-tiled projection.
bool gnnrag::rel_transform_accepts(const float* relfeat_fwd, const float* relfeat_inv, int64_t R1, int32_t D, int32_t L,
                                   const gnnrag_layer_params* layers, int32_t pos_rows, const float* T_out,
                                   const void* planes_out) {
  if (D <= 0 || (D & 3)) return false;                                  // float4 operand loads
  if (planes_out && D > kPlaneHalf) return false;
  if (R1 >= ((int64_t)1 << 31) / D) return false;
  uintptr_t align = (uintptr_t)relfeat_fwd | (uintptr_t)relfeat_inv | (uintptr_t)T_out | (uintptr_t)planes_out;
  for (int j = 0; j < L; ++j) {
    align |= (uintptr_t)layers[j].W_rel | (uintptr_t)layers[j].b_rel;
    if (pos_rows > 0) align |= (uintptr_t)layers[j].pos_fwd | (uintptr_t)layers[j].pos_inv;
  }
  if (align & 15) return false;                                         // float4 accesses
  return (size_t)64 * ((D + 15) / 16) * 16 * sizeof(float) <= 160 * 1024;   // 64 columns x K padded to k groups in LDS
}

extern "C" size_t gnnrag_rel_packed_bytes(int64_t R1, int32_t D, int32_t L) {
  if (R1 <= 0 || D <= 0 || D > kPlaneHalf || L <= 0) return 0;
  return (size_t)L * 2 * R1 * kPackRowB;
}

// the projections with the planes (planes_out), the packed operand (packed_out) or neither; never both
int gnnrag::rel_transform_launch(const float* relfeat_fwd, const float* relfeat_inv, int64_t R1, int32_t D, int32_t L,
                                 const gnnrag_layer_params* layers, int32_t pos_rows, float* T_out, void* planes_out,
                                 void* packed_out, gnnrag_stream_t stream) {
  if (planes_out && packed_out) return GNNRAG_E_BADARG;
  void* const side_out = planes_out ? planes_out : packed_out;
  if (!relfeat_fwd || !relfeat_inv || !layers || !T_out || R1 < 0 || D <= 0 || L <= 0 || pos_rows < 0)
    return GNNRAG_E_BADARG;
  for (int j = 0; j < L; ++j) {
    if (!layers[j].W_rel) return GNNRAG_E_BADARG;
    if ((layers[j].pos_fwd == nullptr) != (layers[j].pos_inv == nullptr)) return GNNRAG_E_BADARG;
  }
  if (!gnnrag::rel_transform_accepts(relfeat_fwd, relfeat_inv, R1, D, L, layers, pos_rows, T_out, side_out))
    return GNNRAG_E_UNSUPPORTED;
  if (R1 == 0) return 0;
  for (int j0 = 0; j0 < L; j0 += kRtMaxL) {
    const int n = L - j0 < kRtMaxL ? L - j0 : kRtMaxL;
    RelTArgs g;
    memset(&g, 0, sizeof(g));
    g.A[0] = relfeat_fwd;
    g.A[1] = relfeat_inv;
    for (int j = 0; j < n; ++j) {
      const gnnrag_layer_params& p = layers[j0 + j];
      g.W[j] = p.W_rel;
      g.b[j] = p.b_rel;
      g.add[j][0] = pos_rows > 0 ? p.pos_fwd : nullptr;
      g.add[j][1] = pos_rows > 0 ? p.pos_inv : nullptr;
    }
    g.C = T_out + (size_t)j0 * 2 * R1 * D;
    g.planes = planes_out ? (unsigned short*)planes_out + (size_t)j0 * 2 * 3 * R1 * kPlaneRow : nullptr;
    g.packed = packed_out ? (unsigned char*)packed_out + (size_t)j0 * 2 * R1 * kPackRowB : nullptr;
    g.M = (int)R1; g.K = D; g.N = D;
    g.add_rows = (int)(pos_rows < R1 ? pos_rows : R1);
    // with planes / the packed operand the column groups run on to 224 columns: the part past D only writes the padding
    const unsigned gy = (unsigned)(((side_out ? kPlaneHalf : D) + 63) / 64), gz = (unsigned)(2 * n);
    const size_t lds = (size_t)64 * ((D + 15) / 16) * 16 * sizeof(float);      // 64 columns x K padded to k groups
    static DeviceMask cap1, cap4;
    if (R1 > 2048) {
      if (lds > 64 * 1024) { const int rc = raise_lds_cap(k_rel_transform<4>, cap4); if (rc) return rc; }
      hipLaunchKernelGGL(k_rel_transform<4>, dim3((unsigned)((R1 + 255) / 256), gy, gz), dim3(256), lds,
                         (hipStream_t)stream, g);
    } else {
      if (lds > 64 * 1024) { const int rc = raise_lds_cap(k_rel_transform<1>, cap1); if (rc) return rc; }
      hipLaunchKernelGGL(k_rel_transform<1>, dim3((unsigned)((R1 + 63) / 64), gy, gz), dim3(256), lds,
                         (hipStream_t)stream, g);
    }
    GNNRAG_LAUNCH_CHECK();
  }
  return 0;
}

int gnnrag::seed_prologue_launch(const gnnrag_csr* csr, const float* dist, void* fws, size_t fws_bytes, float* zero_a,
                                 int64_t zero_na, float* zero_b, int64_t zero_nb, const float* relfeat_fwd,
                                 const float* relfeat_inv, int32_t D, int32_t L, const gnnrag_layer_params* layers,
                                 int32_t pos_rows, float* T_out, void* packed_out, gnnrag_stream_t stream) {
  if (!csr || !relfeat_fwd || !relfeat_inv || !layers || !T_out || D <= 0 || L <= 0 || pos_rows < 0) return GNNRAG_E_BADARG;
  for (int j = 0; j < L; ++j) {
    if (!layers[j].W_rel) return GNNRAG_E_BADARG;
    if ((layers[j].pos_fwd == nullptr) != (layers[j].pos_inv == nullptr)) return GNNRAG_E_BADARG;
  }
  const int64_t R1 = csr->R1;
  // one launch, one block size: the range of k_rel_transform<1>, all layers in one grid
  if (L > kRtMaxL || R1 <= 0 || R1 > 2048 || csr->B <= 0) return GNNRAG_E_UNSUPPORTED;
  if (!gnnrag::rel_transform_accepts(relfeat_fwd, relfeat_inv, R1, D, L, layers, pos_rows, T_out, packed_out))
    return GNNRAG_E_UNSUPPORTED;
  FrontierArgs f;
  int rc = frontier_args(csr, dist, fws, fws_bytes, zero_a, zero_na, zero_b, zero_nb, &f);
  if (rc) return rc;
  RelTArgs g;
  memset(&g, 0, sizeof(g));
  g.A[0] = relfeat_fwd;
  g.A[1] = relfeat_inv;
  for (int j = 0; j < L; ++j) {
    g.W[j] = layers[j].W_rel;
    g.b[j] = layers[j].b_rel;
    g.add[j][0] = pos_rows > 0 ? layers[j].pos_fwd : nullptr;
    g.add[j][1] = pos_rows > 0 ? layers[j].pos_inv : nullptr;
  }
  g.C = T_out;
  g.packed = (unsigned char*)packed_out;
  g.M = (int)R1; g.K = D; g.N = D;
  g.add_rows = (int)(pos_rows < R1 ? pos_rows : R1);
  const int gx = (int)((R1 + 63) / 64), gy = ((packed_out ? kPlaneHalf : D) + 63) / 64, gz = 2 * L;
  size_t lds = (size_t)64 * ((D + 15) / 16) * 16 * sizeof(float);
  const size_t fr_lds = align_up((size_t)kFrLdsInts * sizeof(int), 16);
  if (lds < fr_lds) lds = fr_lds;
  static DeviceMask cap;
  if (lds > 64 * 1024) { rc = raise_lds_cap(k_seed_prologue, cap); if (rc) return rc; }
  hipLaunchKernelGGL(k_seed_prologue, dim3((unsigned)(csr->B + gx * gy * gz)), dim3(kSpThreads), lds, (hipStream_t)stream,
                     g, f, gx, gy);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

// the exported form: the one launch where it applies, else the two it stands for - the same bytes either way
extern "C" int gnnrag_seed_prologue(const gnnrag_csr* csr, const float* dist, void* fws, size_t fws_bytes, float* zero_a,
                                    int64_t zero_na, float* zero_b, int64_t zero_nb, const float* relfeat_fwd,
                                    const float* relfeat_inv, int32_t D, int32_t L, const gnnrag_layer_params* layers,
                                    int32_t pos_rows, float* T_out, void* packed_out, int32_t* combined,
                                    gnnrag_stream_t stream) {
  if (combined) *combined = 0;
  if (!csr || !dist || !fws) return GNNRAG_E_BADARG;
  int rc = gnnrag::seed_prologue_launch(csr, dist, fws, fws_bytes, zero_a, zero_na, zero_b, zero_nb, relfeat_fwd, relfeat_inv,
                                        D, L, layers, pos_rows, T_out, packed_out, stream);
  if (rc == 0 && combined) *combined = 1;
  if (rc != GNNRAG_E_UNSUPPORTED) return rc;
  rc = gnnrag::rel_transform_launch(relfeat_fwd, relfeat_inv, csr->R1, D, L, layers, pos_rows, T_out, nullptr, packed_out, stream);
  if (rc) return rc;
  return gnnrag::frontier_build_z(csr, dist, fws, fws_bytes, zero_a, zero_na, zero_b, zero_nb, (hipStream_t)stream);
}

extern "C" int gnnrag_rel_transform(const float* relfeat_fwd, const float* relfeat_inv, int64_t R1, int32_t D,
                                    int32_t L, const gnnrag_layer_params* layers, int32_t pos_rows, float* T_out,
                                    void* planes_out, gnnrag_stream_t stream) {
  return gnnrag::rel_transform_launch(relfeat_fwd, relfeat_inv, R1, D, L, layers, pos_rows, T_out, planes_out, nullptr, stream);
}

extern "C" int gnnrag_rel_transform_packed(const float* relfeat_fwd, const float* relfeat_inv, int64_t R1, int32_t D,
                                           int32_t L, const gnnrag_layer_params* layers, int32_t pos_rows, float* T_out,
                                           void* packed_out, gnnrag_stream_t stream) {
  if (!packed_out) return GNNRAG_E_BADARG;
  return gnnrag::rel_transform_launch(relfeat_fwd, relfeat_inv, R1, D, L, layers, pos_rows, T_out, nullptr, packed_out, stream);
}
