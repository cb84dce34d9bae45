// rank_layout.h -- the class-major layout ahead of the per-class descending sort, shared by eval_metrics.hip
// (dvt_average_precision) and rank_metrics.hip (dvt_rank_metrics).  Each translation unit gets its own copy of the kernels.
#pragma once
#include "common.h"

namespace {

// [N, C] -> class-major keys [C, N] (f32) and labels [C, N] (u8)
__global__ void to_class_major_kernel(const float* __restrict__ probs, const unsigned char* __restrict__ labels,
                                      int64_t N, int C, float* __restrict__ keys, unsigned char* __restrict__ vals) {
  const int64_t total = N * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / C;
    const int c = (int)(i % C);
    keys[(int64_t)c * N + n] = probs[i];
    vals[(int64_t)c * N + n] = labels[i] != 0;
  }
}

__global__ void offsets_kernel(int* __restrict__ off, int C, int64_t N) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c <= C) off[c] = (int)(c * N);
}

}  // namespace
