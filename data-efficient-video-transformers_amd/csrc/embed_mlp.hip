// embed_mlp.hip -- the kernels under the two MLPs that train on expert embeddings: SpatioTemporalContrastiveModel
// (src/models/contrastivemodel.py) and BasicMLP (src/models/basicmlp.py).
//
// The GEMMs of both stay on dvt_gemm (bias and ReLU in its epilogues, ReLU' in the data-gradient epilogue); what is here:
//   - BatchNorm1d that READS A RECTIFIED TENSOR (Linear -> ReLU -> BatchNorm1d, contrastivemodel.py:28-30 and
//     basicmlp.py:35), forward and backward, over S = 1 or 2 row segments ("views") that keep their own batch statistics;
//   - the gather that turns a list-of-lists expert batch into one [rows, D] input.
//
// Reductions run in a fixed order with no atomics: two identical calls give bitwise-equal results.
#include "common.h"

namespace {

constexpr int kCols = 64;             // BatchNorm: one lane per column, a workgroup owns 64 columns
constexpr int kRowWaves = 4;          // ... and its four waves split the rows (row r -> wave r % 4)
constexpr int kBnThreads = kCols * kRowWaves;

template <typename T> __device__ __forceinline__ float ldf(const T* p) { return to_f32<T>(*p); }
template <typename T> __device__ __forceinline__ void stf(T* p, float v) { *p = (T)v; }

// Sum of the four waves' partials of one column, in wave order (every thread of the column gets the same value).
__device__ __forceinline__ float wave_sum4(float* lds, float v, int col, int wv) {
  __syncthreads();
  lds[wv * kCols + col] = v;
  __syncthreads();
  return ((lds[col] + lds[kCols + col]) + lds[2 * kCols + col]) + lds[3 * kCols + col];
}

template <typename T>
__global__ __launch_bounds__(kBnThreads) void bn1d_relu_fwd_kernel(
    const T* __restrict__ z, int64_t ldz, T* __restrict__ y, int64_t ldy, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar, int64_t* __restrict__ nbt,
    float* __restrict__ smean, float* __restrict__ sinv, int64_t B, int64_t C, int S, float eps, float momentum,
    int training) {
  __shared__ float lds[kRowWaves * kCols];
  const int col = threadIdx.x % kCols, wv = threadIdx.x / kCols;
  const int64_t c = (int64_t)blockIdx.x * kCols + col;
  const bool ok = c < C;
  const float g = ok ? gamma[c] : 0.f, b = ok ? beta[c] : 0.f;
  if (!training) {
    const float m = ok ? rmean[c] : 0.f, inv = ok ? 1.0f / sqrtf(rvar[c] + eps) : 0.f;
    if (ok && wv == 0 && smean) { smean[c] = m; sinv[c] = inv; }
    if (!ok) return;
    for (int64_t r = wv; r < S * B; r += kRowWaves) {
      const float x = fmaxf(ldf(z + r * ldz + c), 0.f);
      stf(y + r * ldy + c, (x - m) * inv * g + b);
    }
    return;
  }
  for (int s = 0; s < S; ++s) {
    const T* zs = z + (int64_t)s * B * ldz;
    float acc = 0.f;
    if (ok)
      for (int64_t r = wv; r < B; r += kRowWaves) acc += fmaxf(ldf(zs + r * ldz + c), 0.f);
    const float mean = wave_sum4(lds, acc, col, wv) / (float)B;
    // centred second pass: a post-ReLU column can have a mean far above its spread
    acc = 0.f;
    if (ok)
      for (int64_t r = wv; r < B; r += kRowWaves) {
        const float d = fmaxf(ldf(zs + r * ldz + c), 0.f) - mean;
        acc = fmaf(d, d, acc);
      }
    const float var = wave_sum4(lds, acc, col, wv) / (float)B;
    const float inv = 1.0f / sqrtf(var + eps);
    if (ok) {
      if (wv == 0) {
        smean[(int64_t)s * C + c] = mean;
        sinv[(int64_t)s * C + c] = inv;
        if (rmean) {                                  // segment by segment: two successive torch calls
          rmean[c] = (1.f - momentum) * rmean[c] + momentum * mean;
          rvar[c] = (1.f - momentum) * rvar[c] + momentum * (var * (float)B / (float)(B - 1));
        }
      }
      T* ys = y + (int64_t)s * B * ldy;
      for (int64_t r = wv; r < B; r += kRowWaves) {
        const float x = fmaxf(ldf(zs + r * ldz + c), 0.f);
        stf(ys + r * ldy + c, (x - mean) * inv * g + b);
      }
    }
  }
  if (nbt && blockIdx.x == 0 && threadIdx.x == 0) nbt[0] += S;
}

// dz = [z > 0] * dx, dx the gradient of BatchNorm1d(x) with x = relu(z).  Per segment (training): Sdy, Sdy*xhat, then
// dx = g inv (dy - Sdy / B - xhat Sdyx / B).  Eval: dx = g inv dy.  dgamma / dbeta sum the segments in order.
template <typename T>
__global__ __launch_bounds__(kBnThreads) void bn1d_relu_bwd_kernel(
    const T* __restrict__ dy, int64_t lddy, const T* __restrict__ z, int64_t ldz, const float* __restrict__ gamma,
    const float* __restrict__ smean, const float* __restrict__ sinv, T* __restrict__ dz, int64_t lddz,
    float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate, int64_t B, int64_t C, int S, int training) {
  __shared__ float lds[kRowWaves * kCols];
  const int col = threadIdx.x % kCols, wv = threadIdx.x / kCols;
  const int64_t c = (int64_t)blockIdx.x * kCols + col;
  const bool ok = c < C;
  const float g = ok ? gamma[c] : 0.f;
  float dg = 0.f, db = 0.f;
  for (int s = 0; s < S; ++s) {
    const int64_t so = training ? (int64_t)s * C : 0;
    const float mean = ok ? smean[so + c] : 0.f, inv = ok ? sinv[so + c] : 0.f;
    const T* zs = z + (int64_t)s * B * ldz;
    const T* dys = dy + (int64_t)s * B * lddy;
    float a1 = 0.f, a2 = 0.f;
    if (ok)
      for (int64_t r = wv; r < B; r += kRowWaves) {
        const float d = ldf(dys + r * lddy + c);
        const float xh = (fmaxf(ldf(zs + r * ldz + c), 0.f) - mean) * inv;
        a1 += d;
        a2 = fmaf(d, xh, a2);
      }
    const float sdy = wave_sum4(lds, a1, col, wv);
    const float sdyx = wave_sum4(lds, a2, col, wv);
    db += sdy;
    dg += sdyx;
    if (!ok) continue;
    T* dzs = dz + (int64_t)s * B * lddz;
    const float k = g * inv, mdy = sdy / (float)B, mdx = sdyx / (float)B;
    for (int64_t r = wv; r < B; r += kRowWaves) {
      const float zv = ldf(zs + r * ldz + c);
      const float d = ldf(dys + r * lddy + c);
      float dx;
      if (training) {
        const float xh = (fmaxf(zv, 0.f) - mean) * inv;
        dx = k * (d - mdy - xh * mdx);
      } else {
        dx = k * d;
      }
      stf(dzs + r * lddz + c, zv > 0.f ? dx : 0.f);
    }
  }
  if (ok && wv == 0) {
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + dg : dg;
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + db : db;
  }
}

// out[r, :] = cat_j src_j (cast to the output dtype); entry (r, j) of the table: {address, width, dtype}.
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_ptr_kernel(const int64_t* __restrict__ table, int parts,
                                                              T* __restrict__ out, int64_t ldo, int64_t D) {
  const int64_t r = blockIdx.x;
  const int64_t* e = table + r * parts * 3;
  T* o = out + r * ldo;
  int64_t base = 0;
  for (int j = 0; j < parts; ++j) {
    const int64_t w = e[3 * j + 1];
    const int sdt = (int)e[3 * j + 2];
    // the table holds device addresses: read them as global memory (a generic pointer would compile to FLAT loads)
    typedef const __attribute__((address_space(1))) float* gf32;
    typedef const __attribute__((address_space(1))) bf16* gbf16;
    typedef const __attribute__((address_space(1))) f16* gf16;
    const uintptr_t src = (uintptr_t)e[3 * j];
    const int64_t lim = w < D - base ? w : D - base;
    for (int64_t c = threadIdx.x; c < lim; c += blockDim.x) {
      float v;
      if (sdt == DVT_F32) v = ((gf32)src)[c];
      else if (sdt == DVT_BF16) v = (float)((gbf16)src)[c];
      else v = (float)((gf16)src)[c];
      stf(o + base + c, v);
    }
    base += lim;
  }
  for (int64_t c = base + threadIdx.x; c < D; c += blockDim.x) stf(o + c, 0.f);
}

}  // namespace

extern "C" {

int dvt_bn1d_relu_fwd(const void* z, int64_t ldz, void* y, int64_t ldy, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save_mean,
                      float* save_invstd, int64_t B, int64_t C, int S, float eps, float momentum, int training, int dtype,
                      dvt_stream_t stream) {
  DVT_REQUIRE(z && y && gamma && beta && B >= 1 && C >= 1 && (S == 1 || S == 2) && ldz >= C && ldy >= C &&
                  (dtype == DVT_F32 || dvt_is_16bit(dtype)),
              "dvt_bn1d_relu_fwd: bad arguments");
  DVT_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "dvt_bn1d_relu_fwd: running_mean / running_var: "
              "both or neither");
  if (training) {
    DVT_REQUIRE(B > 1, "dvt_bn1d_relu_fwd: expected more than 1 value per channel when training (B = 1)");
    DVT_REQUIRE(save_mean && save_invstd, "dvt_bn1d_relu_fwd: training needs save_mean / save_invstd [S, C]");
  } else {
    DVT_REQUIRE(running_mean, "dvt_bn1d_relu_fwd: eval mode needs the running statistics");
    DVT_REQUIRE((save_mean == nullptr) == (save_invstd == nullptr), "dvt_bn1d_relu_fwd: save_mean / save_invstd: both or "
                "neither");
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)dvt_cdiv(C, kCols)), block(kBnThreads);
  int64_t* nbt = training ? num_batches_tracked : nullptr;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((bn1d_relu_fwd_kernel<T>), grid, block, 0, st, (const T*)z, ldz, (T*)y, ldy, gamma,
                                        beta, running_mean, running_var, nbt, save_mean, save_invstd, B, C, S, eps,
                                        momentum, training));
  DVT_LAUNCH_CHECK("dvt_bn1d_relu_fwd");
  return DVT_OK;
}

int dvt_bn1d_relu_bwd(const void* dy, int64_t lddy, const void* z, int64_t ldz, const float* gamma, const float* save_mean,
                      const float* save_invstd, void* dz, int64_t lddz, float* dgamma, float* dbeta, int accumulate,
                      int64_t B, int64_t C, int S, int training, int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(dy && z && gamma && save_mean && save_invstd && dz && B >= 1 && C >= 1 && (S == 1 || S == 2) && lddy >= C &&
                  ldz >= C && lddz >= C && (dtype == DVT_F32 || dvt_is_16bit(dtype)),
              "dvt_bn1d_relu_bwd: bad arguments");
  DVT_REQUIRE(!training || B > 1, "dvt_bn1d_relu_bwd: expected more than 1 value per channel when training (B = 1)");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)dvt_cdiv(C, kCols)), block(kBnThreads);
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((bn1d_relu_bwd_kernel<T>), grid, block, 0, st, (const T*)dy, lddy, (const T*)z,
                                        ldz, gamma, save_mean, save_invstd, (T*)dz, lddz, dgamma, dbeta, accumulate, B, C,
                                        S, training));
  DVT_LAUNCH_CHECK("dvt_bn1d_relu_bwd");
  return DVT_OK;
}

int dvt_gather_rows_ptr(const int64_t* table, int64_t rows, int parts, void* out, int64_t ldo, int64_t D, int dtype,
                        dvt_stream_t stream) {
  DVT_REQUIRE(table && out && rows >= 1 && parts >= 1 && D >= 1 && ldo >= D && (dtype == DVT_F32 || dvt_is_16bit(dtype)),
              "dvt_gather_rows_ptr: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((gather_rows_ptr_kernel<T>), dim3((unsigned)rows), dim3(256), 0, st, table, parts,
                                        (T*)out, ldo, D));
  DVT_LAUNCH_CHECK("dvt_gather_rows_ptr");
  return DVT_OK;
}

}  // extern "C"
