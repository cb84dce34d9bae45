// optim_groups.hip -- the fine-tuning recipe on the flat fp32 buffer in ONE launch: AdamW whose learning rate and
// weight decay are chosen per 64-element block from a device table of parameter groups (decay on the matrices only,
// layer-wise learning-rate decay), the 16-bit mirror, the step counter, and optionally the exponential moving average of
// the weights -- and that average as a stand-alone streaming launch for the other optimizers.
//
// The Adam update, bias correction, ticket and mirror dispatch are adam_update.h's: the grouped kernel expands the same
// adam_update<false> as adamw_fused_kernel of optim.hip, with step_size and decay taken per block instead of per launch.
#include "adam_update.h"
#include <type_traits>

namespace {

constexpr int kMaxGroups = 255;                        // a map byte selects the row; 255 rows at the most

// timm's ModelEmaV2: ema = d ema + (1 - d) p.  The one statement of it, for the fused and the stand-alone launch.
__device__ __forceinline__ float ema_blend(float ema, float p, float d) { return fmaf(d, ema, (1.0f - d) * p); }

// adamw_fused_kernel with per-block coefficients.  group64[b] (one byte per 64 elements, the granularity of skip64: a
// parameter slice of the flat buffer is 64-element aligned and a thread's quad never spans two blocks) selects a row
// {lr_scale, weight_decay} of `table`; the group's rate is lr_dev[0] * lr_scale, formed in fp32.  Each workgroup turns the
// table into {step_size, decay} pairs in LDS once (one thread per row: ngroups <= 255 < 256 threads), so that a quad costs
// one byte load and one 8-byte LDS read on top of the uniform step, and no division.  The LDS array has 256 entries: a
// map byte the host did not validate still reads inside it.
// kEma: ema = ema_blend(ema, p_new, ema_decay_dev[0]) for EVERY element, skipped blocks included (p_new = p there).
// The two kEma forms are two compilations of the update: p * decay - step_size * q may contract either way round, and the
// compiler picks per pair of lanes, so a step with the EMA can differ from one without in the last bit of p (measured:
// lanes 2 and 3 of a quad).  Both forms are held to the same float64 rule; kEma = false is bit-equal to adamw_fused_kernel.
template <typename M, bool kEma>
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                           const float* __restrict__ lr_dev, float b1, float b2, float eps,
                                                           const uint8_t* __restrict__ group64,
                                                           const f32x2* __restrict__ table, int ngroups, int64_t* step_dev,
                                                           const uint8_t* __restrict__ skip, float* __restrict__ ema,
                                                           const float* __restrict__ ema_decay_dev,
                                                           M* __restrict__ mirror) {
  __shared__ f32x2 coef[256];                           // {step_size, decay} of every group
  const int64_t steps = step_dev[0];
  const BiasCorr bc = bias_corr_dev(b1, b2, steps);     // the counter is read before the rate
  const float lr = lr_dev[0];
  if ((int)threadIdx.x < ngroups) {
    const f32x2 row = table[threadIdx.x];
    const AdamCoef cg = adam_coef(lr * row[0], b1, b2, eps, row[1], bc);
    coef[threadIdx.x] = f32x2{cg.step_size, cg.decay};
  }
  __syncthreads();
  AdamCoef c = adam_coef(lr, b1, b2, eps, 0.f, bc);     // step_size and decay are replaced per block
  const float d = kEma ? ema_decay_dev[0] : 0.f;
  const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const int64_t e = i << 2;
    f32x4 pv = *reinterpret_cast<const f32x4*>(p + e);
    if (!(skip && skip[e >> 6])) {                     // parameter without a gradient this step: untouched (torch: grad None)
      const f32x2 sd = coef[group64[e >> 6]];
      c.step_size = sd[0]; c.decay = sd[1];
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + e);
      f32x4 mv = *reinterpret_cast<const f32x4*>(m + e), vv = *reinterpret_cast<const f32x4*>(v + e);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pi = pv[k], mi = mv[k], vi = vv[k];
        adam_update<false>(pi, gv[k], mi, vi, c);
        pv[k] = pi; mv[k] = mi; vv[k] = vi;
      }
      *reinterpret_cast<f32x4*>(p + e) = pv;
      *reinterpret_cast<f32x4*>(m + e) = mv;
      *reinterpret_cast<f32x4*>(v + e) = vv;
    }
    if (kEma) {
      f32x4 ev = *reinterpret_cast<const f32x4*>(ema + e);
#pragma unroll
      for (int k = 0; k < 4; ++k) ev[k] = ema_blend(ev[k], pv[k], d);
      *reinterpret_cast<f32x4*>(ema + e) = ev;
    }
    if (!std::is_same<M, float>::value) {
      typedef M m4 __attribute__((ext_vector_type(4)));
      m4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (M)pv[k];
      *reinterpret_cast<m4*>(mirror + e) = o;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {       // tail of a buffer whose length is not a multiple of 4
    const int64_t i = (n4 << 2) + threadIdx.x;
    float pi = p[i];
    if (!(skip && skip[i >> 6])) {
      const f32x2 sd = coef[group64[i >> 6]];
      c.step_size = sd[0]; c.decay = sd[1];
      float mi = m[i], vi = v[i];
      adam_update<false>(pi, g[i], mi, vi, c);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
    if (kEma) ema[i] = ema_blend(ema[i], pi, d);
    if (!std::is_same<M, float>::value) mirror[i] = (M)pi;
  }
  publish_step(step_dev, steps);
}

// DVT_LAUNCH_MIRRORED instantiates KERNEL<M>: the two kEma forms under one-parameter names
template <typename M> constexpr auto adamw_groups_plain = &adamw_groups_kernel<M, false>;
template <typename M> constexpr auto adamw_groups_ema = &adamw_groups_kernel<M, true>;

// The weight EMA alone, after any other step: 8 B read and 4 B written per element, four elements per thread.
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n,
                                                         const float* __restrict__ ema_decay_dev) {
  const float d = ema_decay_dev[0];
  const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const int64_t e = i << 2;
    const f32x4 pv = *reinterpret_cast<const f32x4*>(p + e);
    f32x4 ev = *reinterpret_cast<const f32x4*>(ema + e);
#pragma unroll
    for (int k = 0; k < 4; ++k) ev[k] = ema_blend(ev[k], pv[k], d);
    *reinterpret_cast<f32x4*>(ema + e) = ev;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = (n4 << 2) + threadIdx.x;
    ema[i] = ema_blend(ema[i], p[i], d);
  }
}

}  // namespace

extern "C" {

int dvt_adamw_groups_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                          const float* lr_dev, float beta1, float beta2, float eps, const uint8_t* group64,
                          const float* group_table, int ngroups, int64_t* step_dev2, const uint8_t* skip64, void* mirror,
                          int mirror_dtype, float* ema, const float* ema_decay_dev, dvt_stream_t stream) {
  if (n == 0) return DVT_OK;
  DVT_REQUIRE(param && grad && exp_avg && exp_avg_sq && lr_dev && group64 && group_table && step_dev2 && n >= 0,
              "dvt_adamw_groups_step: bad arguments");
  DVT_REQUIRE(ngroups >= 1 && ngroups <= kMaxGroups, "dvt_adamw_groups_step: ngroups must be in 1 .. 255");
  DVT_REQUIRE(!ema || ema_decay_dev, "dvt_adamw_groups_step: ema needs ema_decay_dev");
  DVT_REQUIRE(dvt_aligned16(param) && dvt_aligned16(grad) && dvt_aligned16(exp_avg) && dvt_aligned16(exp_avg_sq) &&
                  dvt_aligned16(ema),
              "dvt_adamw_groups_step: buffers must be 16-byte aligned");
  DVT_REQUIRE(((uintptr_t)group_table & 7u) == 0, "dvt_adamw_groups_step: group_table must be 8-byte aligned");
  DVT_REQUIRE(!mirror || (dvt_is_16bit(mirror_dtype) && ((uintptr_t)mirror & 7u) == 0),
              "dvt_adamw_groups_step: mirror must be bf16 / f16 and 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(dvt_grid((n >> 2) + 1)), block(256);
  const f32x2* table = (const f32x2*)group_table;
  if (ema)
    DVT_LAUNCH_MIRRORED(adamw_groups_ema, mirror, mirror_dtype, grid, block, st, param, grad, exp_avg, exp_avg_sq, n, lr_dev,
                        beta1, beta2, eps, group64, table, ngroups, step_dev2, skip64, ema, ema_decay_dev);
  else
    DVT_LAUNCH_MIRRORED(adamw_groups_plain, mirror, mirror_dtype, grid, block, st, param, grad, exp_avg, exp_avg_sq, n,
                        lr_dev, beta1, beta2, eps, group64, table, ngroups, step_dev2, skip64, (float*)nullptr,
                        (const float*)nullptr);
  DVT_LAUNCH_CHECK("dvt_adamw_groups_step");
  return DVT_OK;
}

int dvt_ema_update(float* ema, const float* param, int64_t n, const float* ema_decay_dev, dvt_stream_t stream) {
  if (n == 0) return DVT_OK;
  DVT_REQUIRE(ema && param && ema_decay_dev && n >= 0, "dvt_ema_update: bad arguments");
  DVT_REQUIRE(dvt_aligned16(ema) && dvt_aligned16(param), "dvt_ema_update: buffers must be 16-byte aligned");
  hipLaunchKernelGGL(ema_update_kernel, dim3(dvt_grid((n >> 2) + 1)), dim3(256), 0, (hipStream_t)stream, ema, param, n,
                     ema_decay_dev);
  DVT_LAUNCH_CHECK("dvt_ema_update");
  return DVT_OK;
}

}  // extern "C"
