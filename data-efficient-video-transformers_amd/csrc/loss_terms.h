// loss_terms.h -- the pointwise terms of the binary cross-entropy objectives, stated once for the stand-alone kernels
// (losses.hip) and the fused ones (head_bce_kernel of head.hip, probe_loss_kernel of probe.hip).  The clamp constants and
// the order of evaluation are torch's: the direct float64 tests are tuned to them.
#pragma once
#include "common.h"

// nn.BCEWithLogitsLoss term of logit x against target y: max(x, 0) - x y + log(1 + exp(-|x|))
__device__ __forceinline__ float bce_logits_term(float x, float y) {
  return fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
}
// ... and its gradient with respect to x, given s = sigmoidf_(x)
__device__ __forceinline__ float bce_logits_grad(float s, float y) { return s - y; }

// nn.BCELoss term of probability p against target y, each log clamped at -100 as torch does
__device__ __forceinline__ float bce_clamped_term(float p, float y) {
  return (y - 1.f) * fmaxf(log1pf(-p), -100.f) - y * fmaxf(logf(p), -100.f);
}
// Gradient with respect to the logit z of p = sigmoid(z), g the gradient arriving at the term:
// g (p - y) / max(p (1 - p), 1e-12) * p (1 - p): BCELoss's backward, then sigmoid's, as torch evaluates them.
__device__ __forceinline__ float bce_clamped_grad_logit(float p, float y, float g) {
  const float dp = g * (p - y) / fmaxf((1.f - p) * p, 1e-12f);
  return dp * ((1.f - p) * p);
}
