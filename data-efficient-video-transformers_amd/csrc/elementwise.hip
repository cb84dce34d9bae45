// elementwise.hip -- HBM-bound data-movement kernels of the clip path:
// casts, residual add, token assembly (CLS + positional add), CLS row gather,
// dropout.  All are streaming kernels: 16-byte accesses per lane,
// grid-stride over at most 256 CUs x 8 blocks.  (The patch gather is a unit of
// its own.)
#include "common.h"

namespace {

constexpr int kBlock = 256;

// ------------------------------------------------------------------ cast / add / axpby
template <typename S, typename D>
__global__ void cast_kernel(const S* __restrict__ src, D* __restrict__ dst, int64_t n) {
  const int64_t nvec = n >> 3;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    float v[8];
    load8<S>(src + i * 8, v);
    store8<D>(dst + i * 8, v);
  }
  if (blockIdx.x == 0) {  // tail (n % 8)
    const int64_t t = (nvec << 3) + threadIdx.x;
    if (t < n) dst[t] = from_f32<D>(to_f32<S>(src[t]));
  }
}

template <typename T>
__global__ void add_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out,
                           int64_t n) {
  const int64_t nvec = n >> 3;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    float x[8], y[8];
    load8<T>(a + i * 8, x);
    load8<T>(b + i * 8, y);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] += y[j];
    store8<T>(out + i * 8, x);
  }
  if (blockIdx.x == 0) {
    const int64_t t = (nvec << 3) + threadIdx.x;
    if (t < n) out[t] = from_f32<T>(to_f32<T>(a[t]) + to_f32<T>(b[t]));
  }
}

template <typename T>
__global__ void add_rowtable_kernel(const T* __restrict__ x, const float* __restrict__ table,
                                    T* __restrict__ out, int64_t rows, int64_t d, int64_t rpe) {
  const int64_t dv = d >> 3;
  const int64_t items = rows * dv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const int64_t c = (it % dv) << 3, r = it / dv;
    float v[8], t[8];
    load8<T>(x + r * d + c, v);
    load8<float>(table + (r / rpe) * d + c, t);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] += t[k];
    store8<T>(out + r * d + c, v);
  }
}

template <typename T>
__global__ void copy2d_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t rows, int64_t cols,
                              int64_t src_ld, int64_t dst_ld, int vec) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (vec) {
    const int64_t cv = cols >> 3;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < rows * cv; it += stride) {
      const int64_t c = (it % cv) << 3, r = it / cv;
      float v[8];
      load8<T>(src + r * src_ld + c, v);
      store8<T>(dst + r * dst_ld + c, v);
    }
  } else {
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < rows * cols; it += stride) {
      const int64_t c = it % cols, r = it / cols;
      dst[r * dst_ld + c] = src[r * src_ld + c];
    }
  }
}

template <typename T>
__global__ void permute021_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t A, int64_t B,
                                  int64_t Cc) {
  const int64_t cv = Cc >> 3;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < A * B * cv; it += stride) {
    const int64_t c = (it % cv) << 3;
    const int64_t ab = it / cv;           // destination row index (b, a)
    const int64_t a = ab % A, b = ab / A;
    float v[8];
    load8<T>(src + (a * B + b) * Cc + c, v);
    store8<T>(dst + ab * Cc + c, v);
  }
}

template <typename S>
__global__ void axpby_kernel(const S* __restrict__ src, float alpha, float* __restrict__ dst,
                             float beta, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float s = alpha * to_f32<S>(src[i]);
    dst[i] = beta == 0.0f ? s : fmaf(beta, dst[i], s);
  }
}

template <typename T, bool FWD>
__global__ void act_kernel(const T* __restrict__ dy, const T* __restrict__ x, T* __restrict__ out,
                           int64_t n, int act) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float v = to_f32<T>(x[i]);
    float r;
    if (act == 3) {                       // sigmoid (TPN.py:99)
      const float sg = 1.0f / (1.0f + __expf(-v));
      r = FWD ? sg : to_f32<T>(dy[i]) * sg * (1.0f - sg);
    } else if (FWD) r = act == 1 ? gelu_erf_f(v) : fmaxf(v, 0.f);
    else r = to_f32<T>(dy[i]) * (act == 1 ? gelu_erf_grad_f(v) : (v > 0.f ? 1.f : 0.f));
    out[i] = from_f32<T>(r);
  }
}

// ------------------------------------------------------------------ token assembly
template <typename T>
__global__ void tokens_fwd_kernel(const T* __restrict__ emb, const float* __restrict__ cls,
                                  const float* __restrict__ pos, T* __restrict__ out, int64_t S,
                                  int64_t Tn, int64_t n, int64_t d, int64_t pos_rows) {
  const int64_t dv = d >> 3;
  const int64_t items = S * (n + 1) * dv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const int64_t c = (it % dv) << 3;
    const int64_t row = it / dv;
    const int64_t j = row % (n + 1);
    const int64_t s = row / (n + 1);
    float v[8], p[8];
    load8<float>(pos + ((s % Tn) * pos_rows + j) * d + c, p);
    if (j == 0) load8<float>(cls + c, v);
    else load8<T>(emb + (s * n + (j - 1)) * d + c, v);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] += p[k];
    store8<T>(out + row * d + c, v);
  }
}

template <typename T>
__global__ void tokens_bwd_emb_kernel(const T* __restrict__ dout, T* __restrict__ demb, int64_t S,
                                      int64_t n, int64_t d) {
  const int64_t dv = d >> 3;
  const int64_t items = S * n * dv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const int64_t c = (it % dv) << 3;
    const int64_t row = it / dv;  // = s*n + j
    const int64_t j = row % n;
    const int64_t s = row / n;
    float v[8];
    load8<T>(dout + (s * (n + 1) + j + 1) * d + c, v);
    store8<T>(demb + row * d + c, v);
  }
}

// dpos[t, j, :] (+)= sum_b dout[b*T + t, j, :]   (rows j > n get 0 when overwriting)
// demb != nullptr: the same pass also writes the patch-row gradients demb[(b*T + t)*n + j - 1, :] = dout[b*T + t, j, :]
// (j >= 1): one read of dout serves both (tokens_bwd_emb_kernel alone re-read it).
template <typename T>
__global__ void tokens_bwd_pos_kernel(const T* __restrict__ dout, float* __restrict__ dpos,
                                      int64_t S, int64_t Tn, int64_t n, int64_t d, int64_t pos_rows,
                                      int accumulate, T* __restrict__ demb = nullptr) {
  const int64_t dv = d >> 3;
  const int64_t items = Tn * pos_rows * dv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t B = S / Tn;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const int64_t c = (it % dv) << 3;
    const int64_t row = it / dv;
    const int64_t j = row % pos_rows;
    const int64_t t = row / pos_rows;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (j <= n) {
      for (int64_t b = 0; b < B; ++b) {
        float v[8];
        load8<T>(dout + ((b * Tn + t) * (n + 1) + j) * d + c, v);
        if (demb && j >= 1) store8<T>(demb + ((b * Tn + t) * n + j - 1) * d + c, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += v[k];
      }
    }
    float* o = dpos + row * d + c;
    if (accumulate) {
      float p[8];
      load8<float>(o, p);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += p[k];
    }
    store8<float>(o, acc);
  }
}

// out[c] (+)= sum_{r < R} src[r * row_stride + c]; one block per 8-column chunk.
template <typename T>
__device__ __forceinline__ void strided_rows_sum_block(const T* __restrict__ src, int64_t row_stride, int64_t R,
                                                       float* __restrict__ out, int accumulate, int64_t blk) {
  __shared__ float red[8][kBlock / 64];
  const int64_t c = blk << 3;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t r = threadIdx.x; r < R; r += blockDim.x) {
    float v[8];
    load8<T>(src + r * row_stride + c, v);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] += v[k];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float s = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    float t = 0.f;
    for (int i = 0; i < kBlock / 64; ++i) t += red[threadIdx.x][i];
    float* o = out + c + threadIdx.x;
    *o = accumulate ? *o + t : t;
  }
}

template <typename T>
__global__ void strided_rows_sum_kernel(const T* __restrict__ src, int64_t row_stride, int64_t R,
                                        float* __restrict__ out, int accumulate) {
  strided_rows_sum_block<T>(src, row_stride, R, out, accumulate, blockIdx.x);
}

// The same sum for FEW rows of MANY columns (the learnable pixel-space CLS chunk of FrameTransformer: B = 2 rows of 451 k
// values, frame_transformer.py:105,195): a thread per 8-column chunk walks the rows -- the block-per-chunk form above spent a
// 256-thread workgroup and two barriers on each 32 bytes (56,448 workgroups, 119 us).
template <typename T>
__global__ void few_rows_sum_kernel(const T* __restrict__ src, int64_t row_stride, int64_t R, int64_t chunks,
                                    float* __restrict__ out, int accumulate) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t ch = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ch < chunks; ch += stride) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t r = 0; r < R; ++r) {
      float v[8];
      load8<T>(src + r * row_stride + (ch << 3), v);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += v[k];
    }
    if (accumulate) {
      float o[8];
      load8<float>(out + (ch << 3), o);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += o[k];
    }
    store8<float>(out + (ch << 3), acc);
  }
}

// ------------------------------------------------------------------ CLS row gather
template <typename T>
__global__ void rows_gather_fwd_kernel(const T* __restrict__ src, int64_t src_row_stride,
                                       const float* __restrict__ tok, T* __restrict__ out, int64_t B,
                                       int64_t Tn, int64_t d, int lead) {
  const int64_t dv = d >> 3;
  const int64_t items = B * (Tn + lead) * dv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const int64_t c = (it % dv) << 3;
    const int64_t row = it / dv;
    const int64_t j = row % (Tn + lead);
    const int64_t b = row / (Tn + lead);
    float v[8];
    if (lead && j == 0) load8<float>(tok + c, v);
    else load8<T>(src + (b * Tn + (j - lead)) * src_row_stride + c, v);
    store8<T>(out + row * d + c, v);
  }
}

// The last `tok_blocks` workgroups of the grid sum the token rows (row 0 of every sequence) into dtok instead -- the token
// parameter's gradient in the same launch as the scatter of the other rows.
template <typename T>
__global__ void rows_gather_bwd_kernel(const T* __restrict__ dout, T* __restrict__ dsrc,
                                       int64_t src_row_stride, int64_t B, int64_t Tn, int64_t d,
                                       int lead, float* __restrict__ dtok, int accumulate, int tok_blocks) {
  const int64_t dv = d >> 3;
  const int64_t items = B * Tn * dv;
  const int gather_blocks = (int)gridDim.x - tok_blocks;
  if ((int)blockIdx.x >= gather_blocks) {
    strided_rows_sum_block<T>(dout, (Tn + 1) * d, B, dtok, accumulate, (int)blockIdx.x - gather_blocks);
    return;
  }
  const int64_t stride = (int64_t)gather_blocks * blockDim.x;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const int64_t c = (it % dv) << 3;
    const int64_t row = it / dv;  // b*T + t
    const int64_t t = row % Tn;
    const int64_t b = row / Tn;
    float v[8];
    load8<T>(dout + (b * (Tn + lead) + t + lead) * d + c, v);
    store8<T>(dsrc + row * src_row_stride + c, v);
  }
}

// ------------------------------------------------------------------ mean over rows
template <typename T, bool FWD>
__global__ void mean_rows_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t B, int64_t Ln,
                                 int64_t d, float inv) {
  const int64_t dv = d >> 3;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (FWD) {
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < B * dv; it += stride) {
      const int64_t c = (it % dv) << 3, b = it / dv;
      float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      // sixteen rows requested before the first is added (same order of additions): a rolled loop waited for every row's
      // load in turn -- 98 round trips = 31.6 us for the 2.8 MB pooling in front of the frametransformer's encoder
      int64_t j = 0;
      for (; j + 16 <= Ln; j += 16) {
        float v[16][8];
#pragma unroll
        for (int u = 0; u < 16; ++u) load8<T>(src + (b * Ln + j + u) * d + c, v[u]);
#pragma unroll
        for (int u = 0; u < 16; ++u)
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[k] += v[u][k];
      }
      for (; j < Ln; ++j) {
        float v[8];
        load8<T>(src + (b * Ln + j) * d + c, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += v[k];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] *= inv;
      store8<T>(dst + b * d + c, acc);
    }
  } else {
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < B * Ln * dv; it += stride) {
      const int64_t c = (it % dv) << 3, row = it / dv, b = row / Ln;
      float v[8];
      load8<T>(src + b * d + c, v);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] *= inv;
      store8<T>(dst + row * d + c, v);
    }
  }
}

// ---- dropout (nn.Dropout in training mode: frame_transformer.py:22,41-44; TPN.py:92,95; vit.py:23,25,43,104)
// Counter-based Philox4x32-10: element i draws word (i & 3) of block (offset + i / 4) under the key (seed).  No mask
// is stored: backward re-draws the same words.  state[0] = seed, state[1] = per-step base offset live on the device
// (advanced by dvt_rng_advance once per step), so a captured hipGraph draws fresh masks on every replay.
template <typename T>
__global__ void dropout_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n, uint32_t threshold, float scale,
                               const uint64_t* __restrict__ state, uint64_t call_offset) {
  const uint64_t seed = state[0], base = state[1] + call_offset;
  const int64_t nblk = (n + 3) >> 2;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nblk; b += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t ctr = base + (uint64_t)b;
    uint32_t r[4];
    philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t i = b * 4 + e;
      if (i < n) y[i] = from_f32<T>(r[e] >= threshold ? to_f32<T>(x[i]) * scale : 0.f);
    }
  }
}

// The same mask around its neighbours (dvt_dropout_fused): y = residual? + keep * scale * relu?(x), or -- state == nullptr,
// the backward of the ReLU form -- y = gate != 0 ? scale * x : 0 with the forward's OUTPUT as gate (an element the mask
// dropped and one the ReLU zeroed both pass no gradient).
template <typename T>
__global__ void dropout_fused_kernel(const T* __restrict__ x, const T* __restrict__ res, const T* __restrict__ gate,
                                     T* __restrict__ y, int64_t n, uint32_t threshold, float scale,
                                     const uint64_t* __restrict__ state, uint64_t call_offset, int relu) {
  const uint64_t seed = state ? state[0] : 0, base = state ? state[1] + call_offset : 0;
  const int64_t nblk = (n + 3) >> 2;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nblk; b += (int64_t)gridDim.x * blockDim.x) {
    uint32_t r[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    if (state) {
      const uint64_t ctr = base + (uint64_t)b;
      philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t i = b * 4 + e;
      if (i < n) {
        float v = to_f32<T>(x[i]);
        if (relu) v = fmaxf(v, 0.f);
        bool keep = r[e] >= threshold;
        if (gate) keep = to_f32<T>(gate[i]) != 0.f;
        v = keep ? v * scale : 0.f;
        if (res) v += to_f32<T>(res[i]);
        y[i] = from_f32<T>(v);
      }
    }
  }
}

__global__ void rng_advance_kernel(uint64_t* state, uint64_t delta) { state[1] += delta; }
}  // namespace

extern "C" {

int dvt_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n,
             dvt_stream_t stream) {
  if (n == 0) return DVT_OK;   // empty tensors carry null pointers: nothing to validate, nothing to launch
  DVT_REQUIRE(src && dst && n >= 0, "dvt_cast: null pointer or negative size");
  DVT_REQUIRE(dvt_aligned16(src) && dvt_aligned16(dst), "dvt_cast: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int g = dvt_grid((n >> 3) + 1);
#define DVT_CAST_CASE(SD, S, DD, D)                                                        \
  if (src_dtype == SD && dst_dtype == DD) {                                                \
    hipLaunchKernelGGL((cast_kernel<S, D>), dim3(g), dim3(kBlock), 0, st, (const S*)src, (D*)dst, n); \
    DVT_LAUNCH_CHECK("dvt_cast");                                                          \
    return DVT_OK;                                                                         \
  }
  DVT_CAST_CASE(DVT_F32, float, DVT_BF16, bf16)
  DVT_CAST_CASE(DVT_F32, float, DVT_F16, f16)
  DVT_CAST_CASE(DVT_BF16, bf16, DVT_F32, float)
  DVT_CAST_CASE(DVT_F16, f16, DVT_F32, float)
  DVT_CAST_CASE(DVT_F32, float, DVT_F32, float)
  DVT_CAST_CASE(DVT_BF16, bf16, DVT_BF16, bf16)
  DVT_CAST_CASE(DVT_F16, f16, DVT_F16, f16)
#undef DVT_CAST_CASE
  DVT_UNSUPPORTED("dvt_cast: dtype pair (%d -> %d) not supported", src_dtype, dst_dtype);
}

int dvt_add(const void* a, const void* b, void* out, int64_t n, int dtype, dvt_stream_t stream) {
  if (n == 0) return DVT_OK;   // empty tensors carry null pointers: nothing to validate, nothing to launch
  DVT_REQUIRE(a && b && out && n >= 0, "dvt_add: null pointer or negative size");
  DVT_REQUIRE(dvt_aligned16(a) && dvt_aligned16(b) && dvt_aligned16(out),
              "dvt_add: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((add_kernel<T>), dim3(dvt_grid((n >> 3) + 1)), dim3(kBlock),
                                        0, st, (const T*)a, (const T*)b, (T*)out, n));
  DVT_LAUNCH_CHECK("dvt_add");
  return DVT_OK;
}

int dvt_act_fwd(const void* x, void* y, int64_t n, int act, int dtype, dvt_stream_t stream) {
  if (n == 0) return DVT_OK;   // empty tensors carry null pointers: nothing to validate, nothing to launch
  DVT_REQUIRE(x && y && n >= 0 && act >= 1 && act <= 3, "dvt_act_fwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((act_kernel<T, true>), dim3(dvt_grid(n)), dim3(kBlock), 0, st,
                                        (const T*)nullptr, (const T*)x, (T*)y, n, act));
  DVT_LAUNCH_CHECK("dvt_act_fwd");
  return DVT_OK;
}

int dvt_act_bwd(const void* dy, const void* x, void* dx, int64_t n, int act, int dtype,
                dvt_stream_t stream) {
  if (n == 0) return DVT_OK;   // empty tensors carry null pointers: nothing to validate, nothing to launch
  DVT_REQUIRE(dy && x && dx && n >= 0 && act >= 1 && act <= 3, "dvt_act_bwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((act_kernel<T, false>), dim3(dvt_grid(n)), dim3(kBlock), 0, st,
                                        (const T*)dy, (const T*)x, (T*)dx, n, act));
  DVT_LAUNCH_CHECK("dvt_act_bwd");
  return DVT_OK;
}

int dvt_add_rowtable(const void* x, const float* table, void* out, int64_t rows, int64_t d,
                     int64_t rows_per_entry, int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(x && table && out && rows >= 0 && d > 0 && rows_per_entry > 0, "dvt_add_rowtable: bad arguments");
  DVT_REQUIRE(d % 8 == 0, "dvt_add_rowtable: d must be a multiple of 8");
  DVT_REQUIRE(dvt_aligned16(x) && dvt_aligned16(table) && dvt_aligned16(out), "dvt_add_rowtable: misaligned buffer");
  if (rows == 0) return DVT_OK;
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((add_rowtable_kernel<T>), dim3(dvt_grid(rows * (d >> 3))), dim3(kBlock),
                                        0, st, (const T*)x, table, (T*)out, rows, d, rows_per_entry));
  DVT_LAUNCH_CHECK("dvt_add_rowtable");
  return DVT_OK;
}

int dvt_copy2d(const void* src, void* dst, int64_t rows, int64_t cols, int64_t src_ld, int64_t dst_ld,
               int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(src && dst && rows >= 0 && cols >= 0 && src_ld >= 0 && dst_ld >= cols, "dvt_copy2d: bad arguments");
  if (rows == 0 || cols == 0) return DVT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int vec = (cols % 8 == 0) && (src_ld % 8 == 0) && (dst_ld % 8 == 0) && dvt_aligned16(src) && dvt_aligned16(dst);
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((copy2d_kernel<T>), dim3(dvt_grid(rows * (vec ? cols >> 3 : cols))),
                                        dim3(kBlock), 0, st, (const T*)src, (T*)dst, rows, cols, src_ld, dst_ld, vec));
  DVT_LAUNCH_CHECK("dvt_copy2d");
  return DVT_OK;
}

int dvt_rows_sum(const void* src, int64_t row_stride, int64_t rows, int64_t cols, float* out, int dtype,
                 int accumulate, dvt_stream_t stream) {
  DVT_REQUIRE(src && out && rows >= 0 && cols > 0, "dvt_rows_sum: bad arguments");
  DVT_REQUIRE(cols % 8 == 0 && row_stride % 8 == 0 && dvt_aligned16(src) && dvt_aligned16(out),
              "dvt_rows_sum: cols / row stride must be multiples of 8 and buffers 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (rows <= 16 && cols >= 8192) {
    DVT_DISPATCH_DTYPE(dtype, T,
                       hipLaunchKernelGGL((few_rows_sum_kernel<T>), dim3(dvt_grid(cols >> 3)), dim3(kBlock), 0, st,
                                          (const T*)src, row_stride, rows, cols >> 3, out, accumulate));
  } else {
    DVT_DISPATCH_DTYPE(dtype, T,
                       hipLaunchKernelGGL((strided_rows_sum_kernel<T>), dim3((unsigned)(cols >> 3)), dim3(kBlock), 0,
                                          st, (const T*)src, row_stride, rows, out, accumulate));
  }
  DVT_LAUNCH_CHECK("dvt_rows_sum");
  return DVT_OK;
}

int dvt_permute_021(const void* src, void* dst, int64_t A, int64_t B, int64_t C, int dtype,
                    dvt_stream_t stream) {
  DVT_REQUIRE(src && dst && A >= 0 && B >= 0 && C > 0 && C % 8 == 0, "dvt_permute_021: bad arguments (C % 8 == 0)");
  DVT_REQUIRE(dvt_aligned16(src) && dvt_aligned16(dst), "dvt_permute_021: misaligned buffer");
  if (A == 0 || B == 0) return DVT_OK;
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((permute021_kernel<T>), dim3(dvt_grid(A * B * (C >> 3))), dim3(kBlock), 0,
                                        st, (const T*)src, (T*)dst, A, B, C));
  DVT_LAUNCH_CHECK("dvt_permute_021");
  return DVT_OK;
}

int dvt_axpby_f32(const void* src, int src_dtype, float alpha, float* dst, float beta, int64_t n,
                  dvt_stream_t stream) {
  if (n == 0) return DVT_OK;   // empty tensors carry null pointers: nothing to validate, nothing to launch
  DVT_REQUIRE(src && dst && n >= 0, "dvt_axpby_f32: null pointer or negative size");
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(src_dtype, T,
                     hipLaunchKernelGGL((axpby_kernel<T>), dim3(dvt_grid(n)), dim3(kBlock), 0, st,
                                        (const T*)src, alpha, dst, beta, n));
  DVT_LAUNCH_CHECK("dvt_axpby_f32");
  return DVT_OK;
}

int dvt_tokens_assemble_fwd(const void* emb, const float* cls, const float* pos, void* out,
                            int64_t S, int64_t T, int64_t n, int64_t d, int64_t pos_rows, int dtype,
                            dvt_stream_t stream) {
  DVT_REQUIRE(emb && cls && pos && out, "dvt_tokens_assemble_fwd: null pointer");
  DVT_REQUIRE(S >= 0 && T > 0 && n >= 0 && d > 0 && S % T == 0, "dvt_tokens_assemble_fwd: bad sizes");
  DVT_REQUIRE(pos_rows >= n + 1, "dvt_tokens_assemble_fwd: positional table has %lld rows < n+1 = %lld",
              (long long)pos_rows, (long long)(n + 1));
  DVT_REQUIRE(d % 8 == 0, "dvt_tokens_assemble_fwd: d = %lld must be a multiple of 8", (long long)d);
  DVT_REQUIRE(dvt_aligned16(emb) && dvt_aligned16(cls) && dvt_aligned16(pos) && dvt_aligned16(out),
              "dvt_tokens_assemble_fwd: buffers must be 16-byte aligned");
  if (S == 0) return DVT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t items = S * (n + 1) * (d >> 3);
  DVT_DISPATCH_DTYPE(dtype, Tt,
                     hipLaunchKernelGGL((tokens_fwd_kernel<Tt>), dim3(dvt_grid(items)), dim3(kBlock),
                                        0, st, (const Tt*)emb, cls, pos, (Tt*)out, S, T, n, d,
                                        pos_rows));
  DVT_LAUNCH_CHECK("dvt_tokens_assemble_fwd");
  return DVT_OK;
}

int dvt_tokens_assemble_bwd(const void* dout, void* demb, float* dcls, float* dpos, int64_t S,
                            int64_t T, int64_t n, int64_t d, int64_t pos_rows, int dtype,
                            int accumulate, dvt_stream_t stream) {
  DVT_REQUIRE(dout, "dvt_tokens_assemble_bwd: null dout");
  DVT_REQUIRE(S > 0 && T > 0 && n >= 0 && d > 0 && S % T == 0, "dvt_tokens_assemble_bwd: bad sizes");
  DVT_REQUIRE(pos_rows >= n + 1 && d % 8 == 0, "dvt_tokens_assemble_bwd: bad pos_rows / d");
  DVT_REQUIRE(dvt_aligned16(dout) && dvt_aligned16(demb) && dvt_aligned16(dcls) && dvt_aligned16(dpos),
              "dvt_tokens_assemble_bwd: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t dv = d >> 3;
  DVT_DISPATCH_DTYPE(dtype, Tt, {
    const bool one_pass = demb && n > 0 && dpos;     // the positional-gradient pass reads all of dout: it writes demb as well
    if (demb && n > 0 && !one_pass)
      hipLaunchKernelGGL((tokens_bwd_emb_kernel<Tt>), dim3(dvt_grid(S * n * dv)), dim3(kBlock), 0, st,
                         (const Tt*)dout, (Tt*)demb, S, n, d);
    if (dpos)
      hipLaunchKernelGGL((tokens_bwd_pos_kernel<Tt>), dim3(dvt_grid(T * pos_rows * dv)), dim3(kBlock),
                         0, st, (const Tt*)dout, dpos, S, T, n, d, pos_rows, accumulate, one_pass ? (Tt*)demb : (Tt*)nullptr);
    if (dcls)
      hipLaunchKernelGGL((strided_rows_sum_kernel<Tt>), dim3((unsigned)dv), dim3(kBlock), 0, st,
                         (const Tt*)dout, (n + 1) * d, S, dcls, accumulate);
  });
  DVT_LAUNCH_CHECK("dvt_tokens_assemble_bwd");
  return DVT_OK;
}

int dvt_rows_gather_fwd(const void* src, int64_t src_row_stride, const float* tok, void* out,
                        int64_t B, int64_t T, int64_t d, int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(src && out, "dvt_rows_gather_fwd: null pointer");
  DVT_REQUIRE(B >= 0 && T >= 0 && d > 0 && d % 8 == 0 && src_row_stride % 8 == 0,
              "dvt_rows_gather_fwd: bad sizes (d and row stride must be multiples of 8)");
  DVT_REQUIRE(dvt_aligned16(src) && dvt_aligned16(out) && dvt_aligned16(tok),
              "dvt_rows_gather_fwd: buffers must be 16-byte aligned");
  if (B == 0) return DVT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int lead = tok ? 1 : 0;
  const int64_t items = B * (T + lead) * (d >> 3);
  DVT_DISPATCH_DTYPE(dtype, Tt,
                     hipLaunchKernelGGL((rows_gather_fwd_kernel<Tt>), dim3(dvt_grid(items)),
                                        dim3(kBlock), 0, st, (const Tt*)src, src_row_stride, tok,
                                        (Tt*)out, B, T, d, lead));
  DVT_LAUNCH_CHECK("dvt_rows_gather_fwd");
  return DVT_OK;
}

int dvt_rows_gather_bwd(const void* dout, void* dsrc, int64_t src_row_stride, float* dtok, int64_t B,
                        int64_t T, int64_t d, int dtype, int accumulate, dvt_stream_t stream) {
  DVT_REQUIRE(dout && dsrc, "dvt_rows_gather_bwd: null pointer");
  DVT_REQUIRE(B > 0 && T >= 0 && d > 0 && d % 8 == 0 && src_row_stride % 8 == 0,
              "dvt_rows_gather_bwd: bad sizes");
  DVT_REQUIRE(dvt_aligned16(dout) && dvt_aligned16(dsrc) && dvt_aligned16(dtok),
              "dvt_rows_gather_bwd: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int lead = dtok ? 1 : 0;
  const int64_t dv = d >> 3;
  DVT_DISPATCH_DTYPE(dtype, Tt, {
    if (T > 0)
      hipLaunchKernelGGL((rows_gather_bwd_kernel<Tt>), dim3(dvt_grid(B * T * dv) + (dtok ? (unsigned)dv : 0u)), dim3(kBlock),
                         0, st, (const Tt*)dout, (Tt*)dsrc, src_row_stride, B, T, d, lead, dtok, accumulate,
                         dtok ? (int)dv : 0);
    else if (dtok)
      hipLaunchKernelGGL((strided_rows_sum_kernel<Tt>), dim3((unsigned)dv), dim3(kBlock), 0, st,
                         (const Tt*)dout, (T + 1) * d, B, dtok, accumulate);
  });
  DVT_LAUNCH_CHECK("dvt_rows_gather_bwd");
  return DVT_OK;
}

int dvt_mean_rows_fwd(const void* x, void* out, int64_t B, int64_t L, int64_t d, float scale, int dtype,
                      dvt_stream_t stream) {
  DVT_REQUIRE(x && out && B >= 0 && L > 0 && d > 0 && d % 8 == 0, "dvt_mean_rows_fwd: bad arguments");
  DVT_REQUIRE(dvt_aligned16(x) && dvt_aligned16(out), "dvt_mean_rows_fwd: misaligned buffer");
  if (B == 0) return DVT_OK;
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((mean_rows_kernel<T, true>), dim3(dvt_grid(B * (d >> 3))), dim3(kBlock), 0,
                                        st, (const T*)x, (T*)out, B, L, d, scale));
  DVT_LAUNCH_CHECK("dvt_mean_rows_fwd");
  return DVT_OK;
}

int dvt_mean_rows_bwd(const void* dout, void* dx, int64_t B, int64_t L, int64_t d, float scale, int dtype,
                      dvt_stream_t stream) {
  DVT_REQUIRE(dout && dx && B >= 0 && L > 0 && d > 0 && d % 8 == 0, "dvt_mean_rows_bwd: bad arguments");
  DVT_REQUIRE(dvt_aligned16(dout) && dvt_aligned16(dx), "dvt_mean_rows_bwd: misaligned buffer");
  if (B == 0) return DVT_OK;
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((mean_rows_kernel<T, false>), dim3(dvt_grid(B * L * (d >> 3))),
                                        dim3(kBlock), 0, st, (const T*)dout, (T*)dx, B, L, d, scale));
  DVT_LAUNCH_CHECK("dvt_mean_rows_bwd");
  return DVT_OK;
}

int dvt_dropout(const void* x, void* y, int64_t n, float p, const uint64_t* rng_state, uint64_t call_offset, int dtype,
                dvt_stream_t stream) {
  if (n == 0) return DVT_OK;   // empty tensors carry null pointers: nothing to validate, nothing to launch
  DVT_REQUIRE(x && y && rng_state && n >= 0 && p >= 0.f && p < 1.f, "dvt_dropout: bad arguments (0 <= p < 1)");
  // keep iff word >= threshold, threshold = round(p * 2^32): P(drop) = p to 2^-32
  const double th = (double)p * 4294967296.0;
  const uint32_t threshold = th >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)(th + 0.5);
  const float scale = 1.0f / (1.0f - p);
  DVT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((dropout_kernel<T>), dim3(dvt_grid((n + 3) >> 2)), dim3(kBlock), 0,
                                                  (hipStream_t)stream, (const T*)x, (T*)y, n, threshold, scale, rng_state,
                                                  call_offset));
  DVT_LAUNCH_CHECK("dvt_dropout");
  return DVT_OK;
}

int dvt_dropout_fused(const void* x, const void* residual, const void* gate, void* y, int64_t n, float p,
                      const uint64_t* rng_state, uint64_t call_offset, int relu, int dtype, dvt_stream_t stream) {
  if (n == 0) return DVT_OK;
  DVT_REQUIRE(x && y && n >= 0 && p >= 0.f && p < 1.f && (rng_state != nullptr) != (gate != nullptr),
              "dvt_dropout_fused: bad arguments (0 <= p < 1; exactly one of rng_state and gate)");
  const double th = (double)p * 4294967296.0;
  const uint32_t threshold = th >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)(th + 0.5);
  const float scale = 1.0f / (1.0f - p);
  DVT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((dropout_fused_kernel<T>), dim3(dvt_grid((n + 3) >> 2)), dim3(kBlock), 0,
                                                  (hipStream_t)stream, (const T*)x, (const T*)residual, (const T*)gate, (T*)y, n,
                                                  threshold, scale, rng_state, call_offset, relu));
  DVT_LAUNCH_CHECK("dvt_dropout_fused");
  return DVT_OK;
}

int dvt_rng_advance(uint64_t* rng_state, uint64_t delta, dvt_stream_t stream) {
  DVT_REQUIRE(rng_state, "dvt_rng_advance: null state");
  hipLaunchKernelGGL(rng_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, rng_state, delta);
  DVT_LAUNCH_CHECK("dvt_rng_advance");
  return DVT_OK;
}

}  // extern "C"
