// 64-bit sort keys of the top-p selections (eval_tail.hip: Evaluator.evaluate; train_tail.hip: calc_f1_new) and the bitonic
// network that orders them, one workgroup of 1024 threads per question.
//
//   key = (~bits(p)) << 32 | slot : ascending key order = p descending (p >= 0), slot ascending - the order of Python's stable
//                                   sorted(..., key=prob, reverse=True)
//   a slot that is filtered out carries kToppNone, which sorts behind every kept slot
#pragma once
#include "gnnrag_common.h"

namespace gnnrag {

constexpr unsigned long long kToppNone = ~0ull;

// keep  <=>  eligible and not ((double)p < ignore_prob)      (evaluate.py:198-205, base_model.py:270-279)
__device__ __forceinline__ unsigned long long topp_key(float p, bool eligible, double ignore_prob, int slot) {
  if (eligible && !((double)p < ignore_prob)) return ((unsigned long long)(~__float_as_uint(p)) << 32) | (unsigned)slot;
  return kToppNone;
}

__device__ __forceinline__ float topp_key_prob(unsigned long long k) { return __uint_as_float(~(unsigned)(k >> 32)); }
__device__ __forceinline__ int32_t topp_key_slot(unsigned long long k) { return (int32_t)(k & 0xffffffffu); }

// ascending bitonic sort of a[0 .. M), M a power of two (M = 1: nothing to do), by the whole workgroup (1024 threads); the caller has
// synchronised after writing a, and a is synchronised on return
__device__ __forceinline__ void topp_bitonic_sort(unsigned long long* a, int M) {
  for (int size = 2; size <= M; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < M / 2; t += 1024) {
        const int lo = ((t / stride) * stride * 2) + (t % stride);
        const int hi = lo + stride;
        const bool up = ((lo & size) == 0);
        const unsigned long long x = a[lo], y = a[hi];
        if ((x > y) == up) {
          a[lo] = y;
          a[hi] = x;
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace gnnrag
