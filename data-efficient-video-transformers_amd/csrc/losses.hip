// losses.hip -- the training objectives that are launches of their own.  The pointwise BCE terms are loss_terms.h's.
//
//   * nn.BCEWithLogitsLoss() (mean): src/models/frame_transformer.py:89,263,268,273              dvt_bce_logits_*
//       (fused with the classification head it is head_bce_kernel of head.hip)
//   * hard-label distillation CE(student, argmax(teacher)): frame_transformer.py:90,250          dvt_ce_argmax_*
//   * nn.BCELoss()(torch.sigmoid(z), y) of LSTMRegressor.training_step: src/models/LSTM.py:55-57 dvt_sigmoid_bce_*
//       (fused with the online probe it is probe_loss_kernel of probe.hip)
//   * nn.CrossEntropyLoss() on integer labels: src/models/basicmlp.py:38                         dvt_ce_labels_*
//   * contrastive (NT-Xent) row loss -log( exp(pos/T) / sum_{j != k} exp(sim_kj/T) ) and its mean:
//       src/models/losses/ntxent.py:66-74                                                        dvt_contrastive_*
//
// Every kernel keeps its own reduction, in a fixed order with no atomics: two identical calls give bitwise-equal results.
#include "common.h"
#include "loss_terms.h"

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ float block_sum(float v, float* smem /* >= 4 floats */) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) smem[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += smem[i];
  return t;
}

// ------------------------------------------------------------------ BCE with logits
template <typename T>
__global__ void bce_fwd_kernel(const T* __restrict__ z, const float* __restrict__ y, float* __restrict__ loss, int64_t n) {
  __shared__ float red[kBlock / 64];
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    const float x = to_f32<T>(z[i]);
    acc += bce_logits_term(x, y[i]);
  }
  const float t = block_sum(acc, red);
  if (threadIdx.x == 0) loss[0] = t / (float)n;
}

template <typename T>
__global__ void bce_bwd_kernel(const T* __restrict__ z, const float* __restrict__ y, const float* __restrict__ gloss,
                               T* __restrict__ dz, int64_t n) {
  const float g = gloss[0] / (float)n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float x = to_f32<T>(z[i]);
    dz[i] = from_f32<T>(g * bce_logits_grad(sigmoidf_(x), y[i]));
  }
}

// ------------------------------------------------------------------ CE against the teacher's argmax
// One wave per row: lse(student) - student[argmax teacher]; first max wins (torch.argmax).  A lane's first element is
// taken whatever its value, so a teacher row that is all -inf yields index 0 as torch.argmax does, never C.
template <typename T, bool FWD>
__global__ void ce_argmax_kernel(const T* __restrict__ st, const T* __restrict__ te, const float* __restrict__ gloss,
                                 float* __restrict__ loss, T* __restrict__ dst, int64_t rows, int64_t C) {
  __shared__ float red[kBlock / 64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nw = blockDim.x >> 6;
  float total = 0.f;
  for (int64_t r = wave; r < rows; r += nw) {
    const T* s = st + r * C;
    const T* t = te + r * C;
    float m = -INFINITY, tm = -INFINITY;
    int64_t ti = C;
    for (int64_t c = lane; c < C; c += 64) {
      m = fmaxf(m, to_f32<T>(s[c]));
      const float tv = to_f32<T>(t[c]);
      if (tv > tm || ti == C) { tm = tv; ti = c; }
    }
    m = wave_max(m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(tm, o, 64);
      const int64_t oi = __shfl_xor((long long)ti, o, 64);
      if (om > tm || (om == tm && oi < ti)) { tm = om; ti = oi; }
    }
    float se = 0.f;
    for (int64_t c = lane; c < C; c += 64) se += expf(to_f32<T>(s[c]) - m);
    se = wave_sum(se);
    if (FWD) {
      if (lane == 0) total += m + logf(se) - to_f32<T>(s[ti]);
    } else {
      const float g = gloss[0] / (float)rows;
      for (int64_t c = lane; c < C; c += 64) {
        const float p = expf(to_f32<T>(s[c]) - m) / se;
        dst[r * C + c] = from_f32<T>(g * (p - (c == ti ? 1.f : 0.f)));
      }
    }
  }
  if (FWD) {
    const float t = block_sum(total, red);
    if (threadIdx.x == 0) loss[0] = t / (float)rows;
  }
}

// ------------------------------------------------------------------ BCELoss on sigmoid
// nn.BCELoss()(sigmoid(z), y), mean over n; p = sigmoid(z) in fp32.
// One workgroup, per-thread partials summed in a fixed tree: bitwise reproducible.
template <typename T>
__global__ __launch_bounds__(256) void sigmoid_bce_fwd_kernel(const T* __restrict__ z, const float* __restrict__ y,
                                                             float* __restrict__ loss, float* __restrict__ prob, int64_t n) {
  __shared__ float part[256];
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const float p = sigmoidf_(to_f32<T>(z[i]));
    if (prob) prob[i] = p;
    const float yi = y[i];
    acc += bce_clamped_term(p, yi);
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = part[0] / (float)n;
}

template <typename T>
__global__ __launch_bounds__(256) void sigmoid_bce_bwd_kernel(const T* __restrict__ z, const float* __restrict__ y,
                                                             const float* __restrict__ gloss, T* __restrict__ dz, int64_t n) {
  const float g = gloss[0] / (float)n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float p = sigmoidf_(to_f32<T>(z[i]));
    dz[i] = from_f32<T>(bce_clamped_grad_logit(p, y[i], g));
  }
}

// ------------------------------------------------------------------ CE on integer labels
constexpr int kCeWaves = 16;

// One workgroup: wave w takes rows w, w + 16, ...; per row the log-sum-exp (max, then sum of exp, each butterfly-reduced:
// the same order on every call), its NLL term summed by the wave in row order, the 16 wave sums in wave order.
// lse[M] = number of counted rows.  A label outside [0, C) (and not ignore_index) reads class 0 and makes the loss NaN.
template <typename T>
__global__ __launch_bounds__(kCeWaves * DVT_WAVE) void ce_labels_fwd_kernel(
    const T* __restrict__ x, int64_t ld, const int64_t* __restrict__ labels, float* __restrict__ loss,
    float* __restrict__ lse, int64_t M, int64_t C, int64_t ignore) {
  __shared__ float part[kCeWaves];
  __shared__ int cnt[kCeWaves];
  const int lane = threadIdx.x % DVT_WAVE, wv = threadIdx.x / DVT_WAVE;
  float acc = 0.f;
  int n = 0;
  for (int64_t r = wv; r < M; r += kCeWaves) {
    const T* row = x + r * ld;
    float mx = -INFINITY;
    for (int64_t c = lane; c < C; c += DVT_WAVE) mx = fmaxf(mx, to_f32<T>(row[c]));
    mx = wave_max(mx);
    float se = 0.f;
    for (int64_t c = lane; c < C; c += DVT_WAVE) se += expf(to_f32<T>(row[c]) - mx);
    se = wave_sum(se);
    const float l = mx + logf(se);
    if (lane == 0) lse[r] = l;
    const int64_t y = labels[r];
    if (y == ignore) continue;
    const bool bad = y < 0 || y >= C;
    const float xy = to_f32<T>(row[bad ? 0 : y]);
    acc += bad ? NAN : (l - xy);
    ++n;
  }
  if (lane == 0) { part[wv] = acc; cnt[wv] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    int k = 0;
    for (int w = 0; w < kCeWaves; ++w) { s += part[w]; k += cnt[w]; }
    loss[0] = s / (float)k;                              // k == 0: NaN, as torch's mean over no rows
    lse[M] = (float)k;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ce_labels_bwd_kernel(
    const T* __restrict__ x, int64_t ld, const int64_t* __restrict__ labels, const float* __restrict__ lse,
    const float* __restrict__ gloss, T* __restrict__ dx, int64_t lddx, int64_t M, int64_t C, int64_t ignore) {
  const int64_t r = blockIdx.x;
  const int64_t y = labels[r];
  const T* row = x + r * ld;
  T* drow = dx + r * lddx;
  const float scale = gloss[0] / lse[M];
  const bool skip = y == ignore, bad = y < 0 || y >= C;
  const float l = lse[r];
  for (int64_t c = threadIdx.x; c < C; c += blockDim.x) {
    float d = 0.f;
    if (!skip) d = bad ? NAN : scale * (expf(to_f32<T>(row[c]) - l) - (c == y ? 1.f : 0.f));
    T* o = drow + c;                       // address first, then the conversion: keeps the 16-bit listings as they were
    *o = from_f32<T>(d);
  }
}

// ------------------------------------------------------------------ contrastive rows
// sim [M, M] f32 (M = 2B): row k's positive is column (k + B) mod M.  One wave per row.
// row_loss[k] = log(sum_{j != k} exp(sim_kj / T)) - sim_k,pos / T
__global__ __launch_bounds__(256) void contrastive_rows_fwd_kernel(const float* __restrict__ sim, int M, int B,
                                                                   float inv_t, float* __restrict__ row_loss,
                                                                   float* __restrict__ row_lse) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= M) return;
  const float* s = sim + (int64_t)k * M;
  float mx = -INFINITY;
  for (int j = lane; j < M; j += 64) if (j != k) mx = fmaxf(mx, s[j] * inv_t);
  mx = wave_max(mx);
  float acc = 0.f;
  for (int j = lane; j < M; j += 64) if (j != k) acc += expf(s[j] * inv_t - mx);
  acc = wave_sum(acc);
  if (lane == 0) {
    const float lse = mx + logf(acc);
    row_lse[k] = lse;
    row_loss[k] = lse - s[(k + B) % M] * inv_t;
  }
}

// dsim_kj = gscale * inv_t * (softmax_kj [j != k] - 1[j == pos(k)]),  gscale = dloss / M
__global__ void contrastive_rows_bwd_kernel(const float* __restrict__ sim, const float* __restrict__ row_lse, int M,
                                            int B, float inv_t, const float* __restrict__ gloss, float inv_m,
                                            float* __restrict__ dsim) {
  const int64_t total = (int64_t)M * M;
  const float g = gloss[0] * inv_m * inv_t;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i / M), j = (int)(i % M);
    float p = (j == k) ? 0.f : expf(sim[i] * inv_t - row_lse[k]);
    if (j == (k + B) % M) p -= 1.0f;
    dsim[i] = g * p;
  }
}

// out[0] = mean of x[0..n)   (fixed order, single block)
__global__ void mean_kernel(const float* __restrict__ x, int n, float* __restrict__ out) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)x[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(red[0] / n);
}

}  // namespace

extern "C" {

int dvt_bce_logits_fwd(const void* z, const float* target, float* loss, int64_t n, int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(z && target && loss && n > 0, "dvt_bce_logits_fwd: null pointer or n <= 0");
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((bce_fwd_kernel<T>), dim3(1), dim3(kBlock), 0, st, (const T*)z, target, loss, n));
  DVT_LAUNCH_CHECK("dvt_bce_logits_fwd");
  return DVT_OK;
}

int dvt_bce_logits_bwd(const void* z, const float* target, const float* gloss, void* dz, int64_t n, int dtype,
                       dvt_stream_t stream) {
  DVT_REQUIRE(z && target && gloss && dz && n > 0, "dvt_bce_logits_bwd: null pointer or n <= 0");
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((bce_bwd_kernel<T>), dim3(dvt_grid(n)), dim3(kBlock), 0, st,
                                        (const T*)z, target, gloss, (T*)dz, n));
  DVT_LAUNCH_CHECK("dvt_bce_logits_bwd");
  return DVT_OK;
}

int dvt_ce_argmax_fwd(const void* student, const void* teacher, float* loss, int64_t rows, int64_t C, int dtype,
                      dvt_stream_t stream) {
  DVT_REQUIRE(student && teacher && loss && rows > 0 && C > 0, "dvt_ce_argmax_fwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((ce_argmax_kernel<T, true>), dim3(1), dim3(kBlock), 0, st, (const T*)student,
                                        (const T*)teacher, (const float*)nullptr, loss, (T*)nullptr, rows, C));
  DVT_LAUNCH_CHECK("dvt_ce_argmax_fwd");
  return DVT_OK;
}

int dvt_ce_argmax_bwd(const void* student, const void* teacher, const float* gloss, void* dstudent,
                      int64_t rows, int64_t C, int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(student && teacher && gloss && dstudent && rows > 0 && C > 0, "dvt_ce_argmax_bwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((ce_argmax_kernel<T, false>), dim3(1), dim3(kBlock), 0, st, (const T*)student,
                                        (const T*)teacher, gloss, (float*)nullptr, (T*)dstudent, rows, C));
  DVT_LAUNCH_CHECK("dvt_ce_argmax_bwd");
  return DVT_OK;
}

int dvt_sigmoid_bce_fwd(const void* z, const float* target, float* loss, float* prob, int64_t n, int dtype,
                        dvt_stream_t stream) {
  DVT_REQUIRE(z && target && loss && n > 0, "dvt_sigmoid_bce_fwd: null pointer or n <= 0");
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((sigmoid_bce_fwd_kernel<T>), dim3(1), dim3(256), 0, st, (const T*)z, target, loss,
                                        prob, n));
  DVT_LAUNCH_CHECK("dvt_sigmoid_bce_fwd");
  return DVT_OK;
}

int dvt_sigmoid_bce_bwd(const void* z, const float* target, const float* gloss, void* dz, int64_t n, int dtype,
                        dvt_stream_t stream) {
  DVT_REQUIRE(z && target && gloss && dz && n > 0, "dvt_sigmoid_bce_bwd: null pointer or n <= 0");
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)(dvt_cdiv(n, 256) < 1024 ? dvt_cdiv(n, 256) : 1024);
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((sigmoid_bce_bwd_kernel<T>), dim3(blocks), dim3(256), 0, st, (const T*)z, target,
                                        gloss, (T*)dz, n));
  DVT_LAUNCH_CHECK("dvt_sigmoid_bce_bwd");
  return DVT_OK;
}

int dvt_ce_labels_fwd(const void* logits, int64_t ld, const int64_t* labels, float* loss, float* lse, int64_t M, int64_t C,
                      int64_t ignore_index, int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(logits && labels && loss && lse && M >= 1 && C >= 1 && ld >= C && (dtype == DVT_F32 || dvt_is_16bit(dtype)),
              "dvt_ce_labels_fwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((ce_labels_fwd_kernel<T>), dim3(1), dim3(kCeWaves * DVT_WAVE), 0, st,
                                        (const T*)logits, ld, labels, loss, lse, M, C, ignore_index));
  DVT_LAUNCH_CHECK("dvt_ce_labels_fwd");
  return DVT_OK;
}

int dvt_ce_labels_bwd(const void* logits, int64_t ld, const int64_t* labels, const float* lse, const float* gloss,
                      void* dlogits, int64_t lddl, int64_t M, int64_t C, int64_t ignore_index, int dtype,
                      dvt_stream_t stream) {
  DVT_REQUIRE(logits && labels && lse && gloss && dlogits && M >= 1 && C >= 1 && ld >= C && lddl >= C &&
                  (dtype == DVT_F32 || dvt_is_16bit(dtype)),
              "dvt_ce_labels_bwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((ce_labels_bwd_kernel<T>), dim3((unsigned)M), dim3(256), 0, st, (const T*)logits,
                                        ld, labels, lse, gloss, (T*)dlogits, lddl, M, C, ignore_index));
  DVT_LAUNCH_CHECK("dvt_ce_labels_bwd");
  return DVT_OK;
}

int dvt_contrastive_fwd(const float* sim, int M, float temperature, float* loss, float* row_lse, float* row_loss,
                        dvt_stream_t stream) {
  DVT_REQUIRE(sim && loss && row_lse && row_loss && M >= 2 && M % 2 == 0 && temperature > 0.f,
              "dvt_contrastive_fwd: bad arguments (M = 2 * batch, temperature > 0)");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(contrastive_rows_fwd_kernel, dim3((unsigned)dvt_cdiv(M, 4)), dim3(256), 0, st, sim, M, M / 2,
                     1.0f / temperature, row_loss, row_lse);
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, st, (const float*)row_loss, M, loss);
  DVT_LAUNCH_CHECK("dvt_contrastive_fwd");
  return DVT_OK;
}

int dvt_contrastive_bwd(const float* sim, const float* row_lse, int M, float temperature, const float* gloss,
                        float* dsim, dvt_stream_t stream) {
  DVT_REQUIRE(sim && row_lse && gloss && dsim && M >= 2 && M % 2 == 0 && temperature > 0.f,
              "dvt_contrastive_bwd: bad arguments");
  hipLaunchKernelGGL(contrastive_rows_bwd_kernel, dim3(dvt_grid((int64_t)M * M)), dim3(256), 0, (hipStream_t)stream,
                     sim, row_lse, M, M / 2, 1.0f / temperature, gloss, 1.0f / (float)M, dsim);
  DVT_LAUNCH_CHECK("dvt_contrastive_bwd");
  return DVT_OK;
}

}  // extern "C"
