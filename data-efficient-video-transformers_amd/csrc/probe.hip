// probe.hip -- the online probe of the contrastive model (SSLOnlineEval, src/callbacks/callbacks.py:147-300): one training
// step of pl_bolts' SSLEvaluator
//     Dropout(p) -> Linear(D, H, no bias) -> BatchNorm1d(H) -> ReLU -> Dropout(p) -> Linear(H, C) -> sigmoid -> BCELoss
// with its backward and torch.optim.SGD in three launches, no atomics.
//
// BatchNorm1d statistics are per hidden column over the batch, so a workgroup that owns a slab of 16 hidden columns needs
// nothing from its neighbours for Linear -> BN -> ReLU -> Dropout, nor, in the backward, for the BN backward, the weight
// gradient of its 16 rows of W1 and their SGD update.  Only the C <= 32 logits of a row sum over the slabs: every slab writes
// its partial logits, and one workgroup sums them in slab order (probe_loss_kernel).
//
//   probe_fwd_kernel       grid H / 16: z = drop(x) W1[slab]^T on MFMA (16-bit: 16x16x32, fp32: 16x16x4 f32), x staged
//                          through LDS with the dropout mask drawn by counter from the Philox stream; BN (training: batch
//                          statistics, centred two-pass; running statistics as nn.BatchNorm1d keeps them), ReLU, second
//                          dropout; stores h, z (f32, training), save_mean / save_invstd and the partial logits.
//   probe_loss_kernel      one workgroup: logits, p = sigmoid, BCELoss (mean, logs clamped at -100), dlogits; bias gradient
//                          and its SGD update.
//   probe_bwd_step_kernel  grid H / 16: dW2[:, slab], dh from W2 before its update, dropout / ReLU masks (h != 0), BN
//                          backward with column-local sums, dW1[slab] = dz^T drop(x) on MFMA with the mask regenerated,
//                          then SGD on W1[slab], gamma, beta, W2[:, slab].
//
// Every reduction runs in a fixed order: two identical calls from the same state give bitwise-equal results.
#include "common.h"
#include "loss_terms.h"

#include <type_traits>

namespace {

constexpr int kSlab = 16;                 // hidden columns per workgroup (one MFMA tile)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / DVT_WAVE;
constexpr int kParts = kThreads / kSlab;  // row partitions of the column-wise passes: thread = (part, column)
constexpr int kZs = kSlab + 1;            // row stride of the [rows][16] f32 LDS arrays
constexpr int kRows = 64;                 // rows of x per staged tile (forward: 16 per wave; backward: the K chunk)
constexpr int kKC = 128;                  // forward: columns of x per staged tile (the K chunk)
constexpr int kDC = 64;                   // backward: columns of x per staged tile (one output tile per wave)
constexpr int kMaxC = 32;
constexpr int kLossThreads = 1024;
constexpr int kLossParts = kLossThreads / kMaxC;

// One 16 x 16 x K matrix instruction per element type.  Both operands are read from LDS rows whose K runs contiguously:
// lane l holds row (l % 16) and the K values of its quad (l / 16) -- the same K values for A and B, whatever their order.
template <typename T> struct ProbeMma {
  static constexpr int K = 32, PAD = 8;
  typedef typename Elem16<T>::v8 frag;
  static __device__ __forceinline__ frag load(const T* row_k0, int quad) { return *reinterpret_cast<const frag*>(row_k0 + 8 * quad); }
  static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return Elem16<T>::mma(a, b, c); }
  // 8 values of a [rows][kZs] f32 array, rows k0 + 8 quad ..., column col
  static __device__ __forceinline__ frag gather(const float* zs, int k0, int quad, int col) {
    frag v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (T)zs[(k0 + 8 * quad + i) * kZs + col];
    return v;
  }
};
template <> struct ProbeMma<float> {
  static constexpr int K = 4, PAD = 1;
  typedef float frag;
  static __device__ __forceinline__ frag load(const float* row_k0, int quad) { return row_k0[quad]; }
  static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ frag gather(const float* zs, int k0, int quad, int col) {
    return zs[(k0 + quad) * kZs + col];
  }
};

struct DropArgs {
  uint64_t seed, base;       // Philox key and the block counter of element 0
  uint32_t thr;              // keep iff word >= thr
  float scale;               // 1 / (1 - p)
  int on;
};

// The masks of the two dropouts of a training step: the first takes the Philox blocks from rng_state[1] + rng_offset on
// ((B D + 3) / 4 of them), the second the (B H + 3) / 4 blocks after those -- what dvt_dropout would draw for the two
// tensors at successive call offsets.  The generator state stays on the device (a captured step draws fresh masks).
__device__ __forceinline__ DropArgs probe_drop(const dvt_probe_desc& a, uint32_t thr, int second) {
  DropArgs d{0, 0, thr, 1.0f / (1.0f - a.p), a.training && a.p > 0.f};
  if (d.on) {
    d.seed = a.rng_state[0];
    d.base = a.rng_state[1] + a.rng_offset + (second ? (uint64_t)((a.B * a.D + 3) >> 2) : 0);
  }
  return d;
}

// tile[r][k] (TR: tile[k][r]) = drop(x)[b0 + r][d0 + k] for r < kRows, k < NK, zero outside [0, B) x [0, D).
// With dropout a thread draws one Philox block (4 consecutive elements of the flat [B, D] index) and writes the ones that
// fall into this tile's part of their row, so no word is drawn twice for a tile.
template <typename T, int NK, bool TR>
__device__ __forceinline__ void stage_x(const T* __restrict__ x, int B, int D, int b0, int d0, T* tile, int stride,
                                        const DropArgs& dr) {
  const int t = threadIdx.x;
  if (!dr.on) {
    for (int i = t; i < kRows * NK; i += kThreads) {
      const int r = i / NK, k = i % NK, b = b0 + r, d = d0 + k;
      const T v = (b < B && d < D) ? x[(int64_t)b * D + d] : (T)0.f;
      tile[TR ? k * stride + r : r * stride + k] = v;
    }
    return;
  }
  const int dend = min(d0 + NK, D);
  for (int i = t; i < kRows * NK; i += kThreads) {                 // the zero border
    const int r = i / NK, k = i % NK;
    if (b0 + r >= B || d0 + k >= dend) tile[TR ? k * stride + r : r * stride + k] = (T)0.f;
  }
  constexpr int NBLK = NK / 4 + 1;
  for (int i = t; i < kRows * NBLK; i += kThreads) {
    const int r = i / NBLK, q = i % NBLK, b = b0 + r;
    if (b >= B || d0 >= dend) continue;
    const int64_t lo = (int64_t)b * D + d0, hi = (int64_t)b * D + dend;
    const int64_t blk = (lo >> 2) + q;
    if (blk * 4 >= hi) continue;
    const uint64_t ctr = dr.base + (uint64_t)blk;
    uint32_t w[4];
    philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)dr.seed, (uint32_t)(dr.seed >> 32), w);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t f = blk * 4 + e;
      if (f >= lo && f < hi) {
        const int k = (int)(f - lo);
        const float v = w[e] >= dr.thr ? to_f32<T>(x[f]) * dr.scale : 0.f;
        tile[TR ? k * stride + r : r * stride + k] = (T)v;
      }
    }
  }
}

// Sum over the kParts row partitions of one column in partition order; every thread of the column gets the same value.
__device__ __forceinline__ float parts_sum(float* red, float v, int part, int col) {
  __syncthreads();
  red[part * kSlab + col] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int p = 0; p < kParts; ++p) s += red[p * kSlab + col];
  return s;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void probe_fwd_kernel(dvt_probe_desc a, uint32_t thr) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef ProbeMma<T> M;
  constexpr int KCp = kKC + M::PAD;
  const int B = (int)a.B, D = a.D, H = a.H, C = a.C;
  float* zb = reinterpret_cast<float*>(smem);                                   // [B][kZs]
  float* w2s = zb + (size_t)((B + 3) / 4 * 4) * kZs;                            // [C][16]
  float* red = w2s + kMaxC * kSlab;                                             // [kParts][16]
  T* xs = reinterpret_cast<T*>(red + kParts * kSlab);                           // [kRows][KCp]
  T* ws = xs + kRows * KCp;                                                     // [16][KCp]
  const int t = threadIdx.x, lane = t % DVT_WAVE, wave = t / DVT_WAVE, quad = lane / 16, l16 = lane % 16;
  const int slab = blockIdx.x, c0 = slab * kSlab;
  const T* x = static_cast<const T*>(a.x);
  const DropArgs d1 = probe_drop(a, thr, 0), d2 = probe_drop(a, thr, 1);

  for (int i = t; i < C * kSlab; i += kThreads)
    w2s[i] = to_f32<T>((T)a.w2[(int64_t)(i / kSlab) * H + c0 + i % kSlab]);

  // ---- z[:, slab] = drop(x) W1[slab, :]^T
  for (int b0 = 0; b0 < B; b0 += kRows) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int d0 = 0; d0 < D; d0 += kKC) {
      __syncthreads();
      for (int i = t; i < kSlab * kKC; i += kThreads) {
        const int j = i / kKC, k = i % kKC, d = d0 + k;
        ws[j * KCp + k] = d < D ? (T)a.w1[(int64_t)(c0 + j) * D + d] : (T)0.f;
      }
      stage_x<T, kKC, false>(x, B, D, b0, d0, xs, KCp, d1);
      __syncthreads();
      const int kend = min(kKC, (D - d0 + M::K - 1) / M::K * M::K);
      const T* arow = xs + (wave * 16 + l16) * KCp;
      const T* brow = ws + l16 * KCp;
      for (int kk = 0; kk < kend; kk += M::K) acc = M::mma(M::load(arow + kk, quad), M::load(brow + kk, quad), acc);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int b = b0 + wave * 16 + 4 * quad + i;
      if (b < B) zb[b * kZs + l16] = acc[i];
    }
  }

  // ---- BatchNorm1d per column
  const int col = t % kSlab, part = t / kSlab, c = c0 + col;
  const float g = a.gamma[c], be = a.beta[c];
  float mean, inv;
  if (a.training) {
    float s = 0.f;
    __syncthreads();
    for (int b = part; b < B; b += kParts) s += zb[b * kZs + col];
    mean = parts_sum(red, s, part, col) / (float)B;
    s = 0.f;
    for (int b = part; b < B; b += kParts) {
      const float d = zb[b * kZs + col] - mean;
      s = fmaf(d, d, s);
    }
    const float var = parts_sum(red, s, part, col) / (float)B;
    inv = 1.0f / sqrtf(var + a.eps);
    if (part == 0) {
      a.save_mean[c] = mean;
      a.save_invstd[c] = inv;
      if (a.running_mean) {
        a.running_mean[c] = (1.f - a.momentum) * a.running_mean[c] + a.momentum * mean;
        a.running_var[c] = (1.f - a.momentum) * a.running_var[c] + a.momentum * (var * (float)B / (float)(B - 1));
      }
    }
    if (a.num_batches_tracked && slab == 0 && t == 0) a.num_batches_tracked[0] += 1;
  } else {
    mean = a.running_mean[c];
    inv = 1.0f / sqrtf(a.running_var[c] + a.eps);
    __syncthreads();
  }

  // ---- ReLU, second dropout, h (rounded to the compute dtype: what the second Linear and the backward read)
  T* h = static_cast<T*>(a.h);
  for (int b = part; b < B; b += kParts) {
    const float zv = zb[b * kZs + col];
    if (a.training) a.z[(int64_t)b * H + c] = zv;
    float y = fmaxf((zv - mean) * inv * g + be, 0.f);
    if (d2.on) y = dvt_dropout_keep(d2.seed, d2.base, (uint64_t)((int64_t)b * H + c), d2.thr) ? y * d2.scale : 0.f;
    const T hv = (T)y;
    h[(int64_t)b * H + c] = hv;
    zb[b * kZs + col] = to_f32<T>(hv);
  }
  __syncthreads();

  // ---- this slab's share of the logits
  float* part_out = static_cast<float*>(a.workspace) + (int64_t)slab * B * C;
  for (int i = t; i < B * C; i += kThreads) {
    const int b = i / C, cc = i % C;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kSlab; ++j) s = fmaf(zb[b * kZs + j], w2s[cc * kSlab + j], s);
    part_out[i] = s;
  }
}

// p - lr * g as torch.optim.SGD evaluates it in fp32: the product rounded, then the difference (no contraction to an fma)
__device__ __forceinline__ float sgd(float p, float lr, float g) {
#pragma clang fp contract(off)
  const float step = lr * g;
  return p - step;
}

__global__ __launch_bounds__(kLossThreads) void probe_loss_kernel(dvt_probe_desc a, int slabs) {
  __shared__ float red[kLossThreads];
  const int t = threadIdx.x, C = a.C;
  const int n = (int)a.B * C;
  const float* part = static_cast<const float*>(a.workspace);
  const float gscale = 1.0f / (float)n;
  float acc = 0.f;
  for (int i = t; i < n; i += kLossThreads) {
    float lg = 0.f;
    for (int s = 0; s < slabs; ++s) lg += part[(int64_t)s * n + i];
    lg += a.b2[i % C];
    if (a.logits) a.logits[i] = lg;
    if (!a.target) continue;
    const float p = sigmoidf_(lg);
    const float y = a.target[i];
    a.prob[i] = p;
    acc += bce_clamped_term(p, y);
    if (a.training) a.dlogits[i] = bce_clamped_grad_logit(p, y, gscale);
  }
  red[t] = acc;
  __syncthreads();
  for (int s = kLossThreads / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  if (t == 0 && a.target) a.loss[0] = red[0] / (float)n;
  if (!a.training) return;
  __syncthreads();                                       // dlogits written above are read back below (same workgroup)
  const int cc = t % kMaxC, p = t / kMaxC;
  float s = 0.f;
  if (cc < C)
    for (int b = p; b < (int)a.B; b += kLossParts) s += a.dlogits[b * C + cc];
  red[p * kMaxC + cc] = s;
  __syncthreads();
  if (t < C) {
    float db = 0.f;
    for (int q = 0; q < kLossParts; ++q) db += red[q * kMaxC + t];
    const float gb = a.accumulate ? a.g_b2[t] + db : db;
    a.g_b2[t] = gb;
    a.b2[t] = sgd(a.b2[t], a.lr, gb);
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void probe_bwd_step_kernel(dvt_probe_desc a, uint32_t thr) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef ProbeMma<T> M;
  constexpr int RTp = kRows + M::PAD;
  const int B = (int)a.B, D = a.D, H = a.H, C = a.C;
  const int Bp = (B + kRows - 1) / kRows * kRows;
  float* dzb = reinterpret_cast<float*>(smem);                                  // [Bp][kZs]
  float* w2s = dzb + (size_t)Bp * kZs;                                          // [C][16]
  float* tot = w2s + kMaxC * kSlab;                                             // [C + 2][16]
  float* red = tot + (kMaxC + 2) * kSlab;                                       // [kParts][C + 2][16], then the x tile
  T* xt = reinterpret_cast<T*>(red);                                            // [kDC][RTp]
  const int t = threadIdx.x, lane = t % DVT_WAVE, wave = t / DVT_WAVE, quad = lane / 16, l16 = lane % 16;
  const int slab = blockIdx.x, c0 = slab * kSlab;
  const int col = t % kSlab, part = t / kSlab, c = c0 + col;
  const T* x = static_cast<const T*>(a.x);
  const T* h = static_cast<const T*>(a.h);
  const float* __restrict__ dl = a.dlogits;
  const DropArgs d1 = probe_drop(a, thr, 0);
  const float scale2 = d1.scale;

  for (int i = t; i < C * kSlab; i += kThreads)
    w2s[i] = to_f32<T>((T)a.w2[(int64_t)(i / kSlab) * H + c0 + i % kSlab]);
  for (int i = B * kZs + t; i < Bp * kZs; i += kThreads) dzb[i] = 0.f;
  const float g = a.gamma[c], mean = a.save_mean[c], inv = a.save_invstd[c];
  __syncthreads();

  // ---- dy = mask * (dlogits W2[:, slab]); per column: sum dy, sum dy xhat, dlogits^T h
  float accw[kMaxC];
#pragma unroll
  for (int k = 0; k < kMaxC; ++k) accw[k] = 0.f;
  float a1 = 0.f, a2 = 0.f;
  for (int b = part; b < B; b += kParts) {
    const float hv = to_f32<T>(h[(int64_t)b * H + c]);
    const float xh = (a.z[(int64_t)b * H + c] - mean) * inv;
    const float* dlr = dl + (int64_t)b * C;
    float dh = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxC; ++k)
      if (k < C) {
        const float d = dlr[k];
        dh = fmaf(d, w2s[k * kSlab + col], dh);
        accw[k] = fmaf(d, hv, accw[k]);
      }
    const float dy = hv != 0.f ? dh * scale2 : 0.f;    // h == 0: dropped, or rectified away
    a1 += dy;
    a2 = fmaf(dy, xh, a2);
    dzb[b * kZs + col] = dy;
  }
  const int V = C + 2;
#pragma unroll
  for (int k = 0; k < kMaxC; ++k)
    if (k < C) red[(part * V + k) * kSlab + col] = accw[k];
  red[(part * V + C) * kSlab + col] = a1;
  red[(part * V + C + 1) * kSlab + col] = a2;
  __syncthreads();
  for (int i = t; i < V * kSlab; i += kThreads) {
    float s = 0.f;
#pragma unroll
    for (int p = 0; p < kParts; ++p) s += red[p * V * kSlab + i];
    tot[i] = s;
  }
  __syncthreads();
  const float sdy = tot[C * kSlab + col], sdyx = tot[(C + 1) * kSlab + col];

  // ---- BatchNorm backward: dz = gamma invstd (dy - mean(dy) - xhat mean(dy xhat))
  {
    const float k = g * inv, mdy = sdy / (float)B, mdx = sdyx / (float)B;
    for (int b = part; b < B; b += kParts) {
      const float xh = (a.z[(int64_t)b * H + c] - mean) * inv;
      dzb[b * kZs + col] = k * (dzb[b * kZs + col] - mdy - xh * mdx);
    }
  }

  // ---- dW1[slab, :] = dz^T drop(x), then SGD on these rows
  for (int d0 = 0; d0 < D; d0 += kDC) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < B; b0 += kRows) {
      __syncthreads();
      stage_x<T, kDC, true>(x, B, D, b0, d0, xt, RTp, d1);
      __syncthreads();
      const int kend = min(kRows, (B - b0 + M::K - 1) / M::K * M::K);
      const T* brow = xt + (wave * 16 + l16) * RTp;
      for (int kk = 0; kk < kend; kk += M::K) acc = M::mma(M::gather(dzb, b0 + kk, quad, l16), M::load(brow + kk, quad), acc);
    }
    const int d = d0 + wave * 16 + l16;
    if (d < D) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t idx = (int64_t)(c0 + 4 * quad + i) * D + d;
        const float gw = a.accumulate ? a.g_w1[idx] + acc[i] : acc[i];
        a.g_w1[idx] = gw;
        a.w1[idx] = sgd(a.w1[idx], a.lr, gw);
      }
    }
  }

  // ---- gamma, beta, W2[:, slab]
  if (part == 0) {
    const float gg = a.accumulate ? a.g_gamma[c] + sdyx : sdyx;
    const float gb = a.accumulate ? a.g_beta[c] + sdy : sdy;
    a.g_gamma[c] = gg;
    a.g_beta[c] = gb;
    a.gamma[c] = sgd(g, a.lr, gg);
    a.beta[c] = sgd(a.beta[c], a.lr, gb);
  }
  for (int i = t; i < C * kSlab; i += kThreads) {
    const int64_t idx = (int64_t)(i / kSlab) * H + c0 + i % kSlab;
    const float gw = a.accumulate ? a.g_w2[idx] + tot[i] : tot[i];
    a.g_w2[idx] = gw;
    a.w2[idx] = sgd(a.w2[idx], a.lr, gw);
  }
}

inline size_t fwd_lds(int64_t B, int dtype) {
  const size_t e = dvt_dtype_size(dtype), pad = dtype == DVT_F32 ? 1 : 8;
  return sizeof(float) * ((size_t)((B + 3) / 4 * 4) * kZs + kMaxC * kSlab + kParts * kSlab) + e * (kRows + kSlab) * (kKC + pad);
}
inline size_t bwd_lds(int64_t B, int dtype) {
  const size_t e = dvt_dtype_size(dtype), pad = dtype == DVT_F32 ? 1 : 8;
  const size_t Bp = (size_t)dvt_cdiv(B, kRows) * kRows;
  const size_t red = sizeof(float) * kParts * (kMaxC + 2) * kSlab, tile = e * kDC * (kRows + pad);
  return sizeof(float) * (Bp * kZs + kMaxC * kSlab + (kMaxC + 2) * kSlab) + (red > tile ? red : tile);
}

int probe_check(const char* fn, const dvt_probe_desc* d) {
  DVT_REQUIRE(d, "%s: null descriptor", fn);
  if (!dvt_probe_supported(d->B, d->D, d->H, d->C, d->dtype))
    DVT_UNSUPPORTED("%s: B=%lld D=%d H=%d C=%d dtype=%d outside the probe kernels' range (1 <= B <= 1024, 1 <= D <= 4096, H a "
                    "multiple of 16 up to 2048, 1 <= C <= 32, f32 / bf16 / f16)", fn, (long long)d->B, d->D, d->H, d->C,
                    d->dtype);
  DVT_REQUIRE(!d->training || d->B > 1, "%s: expected more than 1 value per channel when training (B = 1)", fn);
  DVT_REQUIRE(d->p >= 0.f && d->p < 1.f, "%s: dropout p must be in [0, 1)", fn);
  return DVT_OK;
}

inline uint32_t drop_threshold(float p) {              // keep iff word >= round(p 2^32), as dvt_dropout
  const double th = (double)p * 4294967296.0;
  return th >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)(th + 0.5);
}

inline int dtype_slot(int dtype) { return dtype == DVT_F32 ? 0 : dtype == DVT_BF16 ? 1 : 2; }

}  // namespace

extern "C" {

int dvt_probe_supported(int64_t B, int D, int H, int C, int dtype) {
  return B >= 1 && B <= 1024 && D >= 1 && D <= 4096 && H >= kSlab && H <= 2048 && H % kSlab == 0 && C >= 1 && C <= kMaxC &&
         (dtype == DVT_F32 || dtype == DVT_BF16 || dtype == DVT_F16);
}

size_t dvt_probe_workspace_bytes(int64_t B, int H, int C) {
  if (B <= 0 || H <= 0 || C <= 0) return 0;
  return sizeof(float) * (size_t)(H / kSlab) * (size_t)B * (size_t)C;
}

int dvt_probe_fwd(const dvt_probe_desc* d, dvt_stream_t stream) {
  const int rc = probe_check("dvt_probe_fwd", d);
  if (rc != DVT_OK) return rc;
  DVT_REQUIRE(d->x && d->w1 && d->gamma && d->beta && d->w2 && d->h && d->workspace, "dvt_probe_fwd: null pointer");
  if (d->training) {
    DVT_REQUIRE(d->z && d->save_mean && d->save_invstd, "dvt_probe_fwd: training needs z, save_mean and save_invstd");
    DVT_REQUIRE((d->running_mean == nullptr) == (d->running_var == nullptr), "dvt_probe_fwd: running_mean / running_var: "
                "both or neither");
    DVT_REQUIRE(d->p == 0.f || d->rng_state, "dvt_probe_fwd: dropout needs rng_state");
  } else {
    DVT_REQUIRE(d->running_mean && d->running_var, "dvt_probe_fwd: eval mode needs the running statistics");
  }
  static DvtLdsAttr attr[3];
  const size_t lds = fwd_lds(d->B, d->dtype);
  DVT_DISPATCH_DTYPE(d->dtype, T, {
    dvt_lds_attr(attr[dtype_slot(d->dtype)], (const void*)probe_fwd_kernel<T>, (int)fwd_lds(1024, d->dtype));
    hipLaunchKernelGGL((probe_fwd_kernel<T>), dim3(d->H / kSlab), dim3(kThreads), lds, (hipStream_t)stream, *d,
                       drop_threshold(d->p));
  });
  DVT_LAUNCH_CHECK("dvt_probe_fwd");
  return DVT_OK;
}

int dvt_probe_loss(const dvt_probe_desc* d, dvt_stream_t stream) {
  const int rc = probe_check("dvt_probe_loss", d);
  if (rc != DVT_OK) return rc;
  DVT_REQUIRE(d->workspace && d->b2, "dvt_probe_loss: null pointer");
  DVT_REQUIRE(d->target ? (d->prob && d->loss) : (d->logits && !d->training),
              "dvt_probe_loss: a target needs prob and loss; without one only eval-mode logits are formed");
  DVT_REQUIRE(!d->training || (d->dlogits && d->g_b2), "dvt_probe_loss: training needs dlogits and g_b2");
  hipLaunchKernelGGL(probe_loss_kernel, dim3(1), dim3(kLossThreads), 0, (hipStream_t)stream, *d, d->H / kSlab);
  DVT_LAUNCH_CHECK("dvt_probe_loss");
  return DVT_OK;
}

int dvt_probe_bwd_step(const dvt_probe_desc* d, dvt_stream_t stream) {
  const int rc = probe_check("dvt_probe_bwd_step", d);
  if (rc != DVT_OK) return rc;
  DVT_REQUIRE(d->training, "dvt_probe_bwd_step: the backward belongs to a training-mode forward");
  DVT_REQUIRE(d->x && d->dlogits && d->h && d->z && d->save_mean && d->save_invstd && d->w1 && d->gamma && d->beta && d->w2 &&
                  d->g_w1 && d->g_gamma && d->g_beta && d->g_w2, "dvt_probe_bwd_step: null pointer");
  DVT_REQUIRE(d->p == 0.f || d->rng_state, "dvt_probe_bwd_step: dropout needs rng_state");
  static DvtLdsAttr attr[3];
  const size_t lds = bwd_lds(d->B, d->dtype);
  DVT_DISPATCH_DTYPE(d->dtype, T, {
    dvt_lds_attr(attr[dtype_slot(d->dtype)], (const void*)probe_bwd_step_kernel<T>, (int)bwd_lds(1024, d->dtype));
    hipLaunchKernelGGL((probe_bwd_step_kernel<T>), dim3(d->H / kSlab), dim3(kThreads), lds, (hipStream_t)stream, *d,
                       drop_threshold(d->p));
  });
  DVT_LAUNCH_CHECK("dvt_probe_bwd_step");
  return DVT_OK;
}

}  // extern "C"
