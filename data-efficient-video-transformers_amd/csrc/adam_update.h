// adam_update.h -- the Adam update, its bias correction, the step-counter ticket and the mirror dispatch, each stated once
// for the optimizer units: optim.hip (the uniform steps) and optim_groups.hip (the grouped step and the weight EMA).
#pragma once
#include "common.h"

// 1 - b1^t and sqrt(1 - b2^t).  Two ways to fill it that round differently and stay apart: dvt_adamw_step computes the
// pair from its host step in double, every device-counter kernel with bias_corr_dev in float.
struct BiasCorr {
  float bc1, bc2_sqrt;
};

__device__ __forceinline__ BiasCorr bias_corr_dev(float b1, float b2, int64_t steps_taken) {
  const float t = (float)(steps_taken + 1);
  return {1.0f - powf(b1, t), sqrtf(1.0f - powf(b2, t))};
}

struct AdamCoef {
  float b1, b2, eps, wd, step_size, decay, bc2_sqrt;
};

__device__ __forceinline__ AdamCoef adam_coef(float lr, float b1, float b2, float eps, float wd, BiasCorr bc) {
  return {b1, b2, eps, wd, lr / bc.bc1, 1.0f - lr * wd, bc.bc2_sqrt};
}

// One element of Adam: m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// with the weight decay either decoupled (AdamW: p *= 1 - lr wd first) or coupled (torch.optim.Adam: g += wd p first).
template <bool kCoupled>
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamCoef& c) {
  if (kCoupled) g = fmaf(c.wd, p, g);
  else p *= c.decay;
  m = fmaf(c.b1, m, (1.0f - c.b1) * g);
  v = fmaf(c.b2, v, (1.0f - c.b2) * g * g);
  p -= c.step_size * (m / (sqrtf(v) / c.bc2_sqrt + c.eps));
}

// The step counter of the one-launch steps, step_dev = int64[2]: steps taken, launch ticket.  Every block reads
// step_dev[0] (`steps`) before it comes here; relaxed device-scope ticket: the last block publishes the increment.
__device__ __forceinline__ void publish_step(int64_t* step_dev, int64_t steps) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long ticket = __hip_atomic_fetch_add((unsigned long long*)(step_dev + 1), 1ull, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT);
    if (ticket == (unsigned long long)gridDim.x - 1) {
      step_dev[0] = steps + 1;
      step_dev[1] = 0;
    }
  }
}

// KERNEL<M>(..., M* mirror) for the 16-bit mirror of the updated weights: M = float and a null pointer for none.
#define DVT_LAUNCH_MIRRORED(KERNEL, mirror, mirror_dtype, grid, block, st, ...)                            \
  do {                                                                                                     \
    if (!(mirror))                                                                                         \
      hipLaunchKernelGGL((KERNEL<float>), grid, block, 0, st, __VA_ARGS__, (float*)nullptr);               \
    else if ((mirror_dtype) == DVT_BF16)                                                                   \
      hipLaunchKernelGGL((KERNEL<bf16>), grid, block, 0, st, __VA_ARGS__, (bf16*)(mirror));                \
    else                                                                                                   \
      hipLaunchKernelGGL((KERNEL<f16>), grid, block, 0, st, __VA_ARGS__, (f16*)(mirror));                  \
  } while (0)
