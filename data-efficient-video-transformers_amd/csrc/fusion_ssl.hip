// fusion_ssl.hip -- multi-modal gating and the row normaliser of the contrastive objective.
//
//   * row L2 normalisation  F.normalize(x) / the cosine-similarity normaliser
//       (src/models/collabgating.py:70 GatedEmbeddingUnit; src/models/losses/ntxent.py:63)
//   * context gating        F.glu(cat(x, x + x1), -1) = x * sigmoid(x + x1)   (collabgating.py:83-86)
// Small HBM-bound kernels; the similarity matrix itself is a GEMM (dvt_gemm) and its row loss is losses.hip's.
#include "common.h"

namespace {

// one wave per row: y = x / max(||x||, eps); inv[r] = 1 / max(||x||, eps)
template <typename T>
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                         float* __restrict__ inv, int64_t rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float s = 0.f;
  for (int c = lane; c < D; c += 64) { const float v = to_f32<T>(x[r * D + c]); s = fmaf(v, v, s); }
  s = wave_sum(s);
  const float iv = 1.0f / fmaxf(sqrtf(s), eps);
  for (int c = lane; c < D; c += 64) y[r * D + c] = from_f32<T>(to_f32<T>(x[r * D + c]) * iv);
  if (lane == 0) inv[r] = iv;
}

// dx = inv * (dy - y * <y, dy>)      (rows clamped by eps have y = x*inv with ||y|| < 1: same formula as torch
// only away from the clamp; the clamp region is the zero vector, whose gradient is inv * dy)
template <typename T>
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y,
                                                         const float* __restrict__ inv, T* __restrict__ dx,
                                                         int64_t rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float dot = 0.f;
  for (int c = lane; c < D; c += 64) dot = fmaf(to_f32<T>(y[r * D + c]), to_f32<T>(dy[r * D + c]), dot);
  dot = wave_sum(dot);
  const float iv = inv[r];
  const bool clamped = iv >= 1.0f / eps;
  for (int c = lane; c < D; c += 64) {
    const float g = to_f32<T>(dy[r * D + c]);
    dx[r * D + c] = from_f32<T>(clamped ? iv * g : iv * (g - to_f32<T>(y[r * D + c]) * dot));
  }
}

// out[r] = <a[r], b[r]> / (max(||a[r]||, eps) * max(||b[r]||, eps)): each norm is clamped on its own, as torch's
// nn.CosineSimilarity(dim=1) does (frame_transformer.py:121,257) and as l2norm_fwd_kernel above does for NT-Xent
template <typename T>
__global__ __launch_bounds__(256) void cosine_rows_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                          float* __restrict__ out, int64_t rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float ab = 0.f, aa = 0.f, bb = 0.f;
  for (int c = lane; c < D; c += 64) {
    const float x = to_f32<T>(a[r * D + c]), y = to_f32<T>(b[r * D + c]);
    ab = fmaf(x, y, ab); aa = fmaf(x, x, aa); bb = fmaf(y, y, bb);
  }
  ab = wave_sum(ab); aa = wave_sum(aa); bb = wave_sum(bb);
  if (lane == 0) out[r] = ab / (fmaxf(sqrtf(aa), eps) * fmaxf(sqrtf(bb), eps));
}

// y = a * sigmoid(b)
template <typename T>
__global__ void gate_fwd_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float s = sigmoidf_(to_f32<T>(b[i]));
    y[i] = from_f32<T>(to_f32<T>(a[i]) * s);
  }
}

// da = dy * s;  db = dy * a * s * (1 - s)
template <typename T>
__global__ void gate_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ a, const T* __restrict__ b,
                                T* __restrict__ da, T* __restrict__ db, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float s = sigmoidf_(to_f32<T>(b[i]));
    const float g = to_f32<T>(dy[i]);
    da[i] = from_f32<T>(g * s);
    db[i] = from_f32<T>(g * to_f32<T>(a[i]) * s * (1.0f - s));
  }
}

}  // namespace

extern "C" {

int dvt_l2norm_rows_fwd(const void* x, void* y, float* inv_norm, int64_t rows, int D, float eps, int dtype,
                        dvt_stream_t stream) {
  DVT_REQUIRE(x && y && inv_norm && rows >= 0 && D > 0 && eps > 0.f, "dvt_l2norm_rows_fwd: bad arguments");
  if (rows == 0) return DVT_OK;
  DVT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((l2norm_fwd_kernel<T>), dim3((unsigned)dvt_cdiv(rows, 4)), dim3(256), 0,
                                                  (hipStream_t)stream, (const T*)x, (T*)y, inv_norm, rows, D, eps));
  DVT_LAUNCH_CHECK("dvt_l2norm_rows_fwd");
  return DVT_OK;
}

int dvt_l2norm_rows_bwd(const void* dy, const void* y, const float* inv_norm, void* dx, int64_t rows, int D, float eps,
                        int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(dy && y && inv_norm && dx && rows >= 0 && D > 0 && eps > 0.f, "dvt_l2norm_rows_bwd: bad arguments");
  if (rows == 0) return DVT_OK;
  DVT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((l2norm_bwd_kernel<T>), dim3((unsigned)dvt_cdiv(rows, 4)), dim3(256), 0,
                                                  (hipStream_t)stream, (const T*)dy, (const T*)y, inv_norm, (T*)dx, rows,
                                                  D, eps));
  DVT_LAUNCH_CHECK("dvt_l2norm_rows_bwd");
  return DVT_OK;
}

int dvt_cosine_rows(const void* a, const void* b, float* out, int64_t rows, int D, float eps, int dtype,
                    dvt_stream_t stream) {
  DVT_REQUIRE(rows >= 0 && D > 0 && eps > 0.f && (rows == 0 || (a && b && out)), "dvt_cosine_rows: bad arguments");
  if (rows == 0) return DVT_OK;
  DVT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((cosine_rows_kernel<T>), dim3((unsigned)dvt_cdiv(rows, 4)), dim3(256), 0,
                                                  (hipStream_t)stream, (const T*)a, (const T*)b, out, rows, D, eps));
  DVT_LAUNCH_CHECK("dvt_cosine_rows");
  return DVT_OK;
}

int dvt_gate_fwd(const void* a, const void* b, void* y, int64_t n, int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(a && b && y && n >= 0, "dvt_gate_fwd: bad arguments");
  if (n == 0) return DVT_OK;
  DVT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((gate_fwd_kernel<T>), dim3(dvt_grid(n)), dim3(256), 0, (hipStream_t)stream,
                                                  (const T*)a, (const T*)b, (T*)y, n));
  DVT_LAUNCH_CHECK("dvt_gate_fwd");
  return DVT_OK;
}

int dvt_gate_bwd(const void* dy, const void* a, const void* b, void* da, void* db, int64_t n, int dtype,
                 dvt_stream_t stream) {
  DVT_REQUIRE(dy && a && b && da && db && n >= 0, "dvt_gate_bwd: bad arguments");
  if (n == 0) return DVT_OK;
  DVT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((gate_bwd_kernel<T>), dim3(dvt_grid(n)), dim3(256), 0, (hipStream_t)stream,
                                                  (const T*)dy, (const T*)a, (const T*)b, (T*)da, (T*)db, n));
  DVT_LAUNCH_CHECK("dvt_gate_bwd");
  return DVT_OK;
}

}  // extern "C"
