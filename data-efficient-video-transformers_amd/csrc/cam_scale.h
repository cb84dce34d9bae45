// cam_scale.h -- the per-clip scaling of a saliency map to [0, 1] (pytorch_grad_cam's scale_cam_image), stated once:
// cam.hip scales the class-activation maps with it, attn_rollout.hip the attention-rollout volume.
#pragma once
#include "common.h"

// minimum and maximum of the workgroup's (mn, mx) -> every thread.  red: 2 * waves floats of LDS.  The extrema are
// order-free, so the result does not depend on how the values were dealt to the threads.
__device__ __forceinline__ void block_extrema(float& mn, float& mx, float* red, int waves) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if (lane == 0) { red[2 * wid] = mn; red[2 * wid + 1] = mx; }
  __syncthreads();
  mn = red[0]; mx = red[1];
  for (int w = 1; w < waves; ++w) { mn = fminf(mn, red[2 * w]); mx = fmaxf(mx, red[2 * w + 1]); }
  __syncthreads();
}

// scaled = (raw - min) / (1e-7 + (max - min)): the denominator of a clip, and a value under it
__device__ __forceinline__ float cam_scale_den(float mn, float mx) { return 1e-7f + (mx - mn); }
__device__ __forceinline__ float cam_scale_value(float r, float mn, float den) { return (r - mn) / den; }
