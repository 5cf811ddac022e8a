// The small dense auxiliaries the training backwards share: a transpose, a padded-copy drop, column sums in one fixed
// order, and gnnrag_gemm_tn into a gradient whose leading dimension the MFMA kernel cannot write directly.  None of them
// uses atomics, allocates or waits for the stream; a second call gives the same bits.
#include "gnnrag_common.h"

namespace gnnrag {

// dst[k][j] = src[j][k]  (src [rows][cols])
__global__ __launch_bounds__(256) void k_transpose(const float* __restrict__ src, float* __restrict__ dst, int rows,
                                                   int cols) {
  __shared__ float tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int r = by + i, c = bx + tx;
    tile[i][tx] = (r < rows && c < cols) ? src[(size_t)r * cols + c] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = bx + i, r = by + tx;
    if (c < cols && r < rows) dst[(size_t)c * rows + r] = tile[tx][i];
  }
}

int transpose_launch(const float* src, float* dst, int rows, int cols, hipStream_t stream) {
  hipLaunchKernelGGL(k_transpose, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0, stream, src, dst, rows, cols);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

// dst [rows, cols] = the first cols columns of the first rows rows of src [., ld]
__global__ __launch_bounds__(256) void k_unpad(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols,
                                               int ld) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cols) return;
  const int r = i / cols, c = i - r * cols;
  dst[i] = src[(size_t)r * ld + c];
}

int unpad_launch(const float* src, float* dst, int rows, int cols, int ld, hipStream_t stream) {
  hipLaunchKernelGGL(k_unpad, dim3((rows * cols + 255) / 256), dim3(256), 0, stream, src, dst, rows, cols, ld);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

// blockIdx.y = the job: 32 columns x 8 row slices per workgroup, a slice in ascending rows, the slices added in slice
// order
__global__ __launch_bounds__(256) void k_colsum(const ColsumJobs jobs) {
  __shared__ float sm[8][32];
  const int job = blockIdx.y;
  const float* __restrict__ src = jobs.src[job];
  float* dst = jobs.dst[job];
  const int64_t M = jobs.rows[job];
  const int ld = jobs.ld[job];
  const int cx = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cx;
  const int64_t per = (M + 7) / 8;
  const int64_t m0 = sl * per, m1 = m0 + per < M ? m0 + per : M;
  float acc = 0.f;
  if (c < jobs.cols)
    for (int64_t m = m0; m < m1; ++m) acc += src[m * ld + c];
  sm[sl][cx] = acc;
  __syncthreads();
  if (sl == 0 && c < jobs.cols) {
    float v = sm[0][cx];
#pragma unroll
    for (int i = 1; i < 8; ++i) v += sm[i][cx];
    dst[c] = v;
  }
}

int colsum_launch(const ColsumJobs& jobs, int n_jobs, hipStream_t stream) {
  hipLaunchKernelGGL(k_colsum, dim3((jobs.cols + 31) / 32, n_jobs), dim3(256), 0, stream, jobs);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

int gemm_tn_unpadded(const float* A, const float* B, int64_t M, int32_t N1p, int32_t N2p, int32_t N1, int32_t N2,
                     float* dst, float* cpad, void* tn_ws, size_t tn_bytes, hipStream_t stream) {
  if (N1p == N1 && N2p == N2 && aligned16(dst))
    return gnnrag_gemm_tn(A, B, M, N1, N2, dst, tn_ws, tn_bytes, (gnnrag_stream_t)stream);
  GNNRAG_RC(gnnrag_gemm_tn(A, B, M, N1p, N2p, cpad, tn_ws, tn_bytes, (gnnrag_stream_t)stream));
  return unpad_launch(cpad, dst, N1, N2, N2p, stream);
}

}  // namespace gnnrag
