// mae.hip -- masked-autoencoder pre-training on the ViViT tokeniser (MAE / MAE-ST / VideoMAE; the reference has none): what
// the patch-dropout unit (csrc/patch_dropout.hip) lacks to turn "the space stack on the kept tokens" into a reconstruction
// task.  S sequences of n positions, k kept: keep [S, k] int32 ascending, slot [S, n] int32 its inverse (-1 = dropped).
//
//   restore_fwd_kernel     out[s, j] = (slot[s, j] in [0, k) ? y[s, skip + slot[s, j]] : mask) + pos[s % T, j]: the encoded
//                          kept rows back at their positions, the learned mask token everywhere else, plus the decoder's
//                          positional row.  One fp32 add, one rounding; every row of out written once.
//   restore_dy_kernel      dy[s, skip + i] = dout[s, keep[s, i]]; the skip leading rows zero.
//   restore_dpos_kernel    item = 8 columns of one positional row (tau, j): walks the clips b in ascending order once and
//                          leaves dpos[tau, j] (+)= sum_b dout[(b, tau), j] and, in `partial`, the same sum over the clips that
//                          DROPPED (tau, j) -- a fixed order, no float atomics.
//   colsum_kernel          dmask (+)= sum of the rows of partial, one workgroup per 8 columns, a fixed order.
//
//   loss_vec_kernel        the masked patch loss and its gradient.  The target of a dropped (s, j) is row (s, j) of the
//   loss_any_kernel        tubelet gather (csrc/patchify.hip: column ((kf P + p1) P + p2) C + c = clip[s pt + kf, c,
//                          ph P + p1, pw P + p2]), read from the clip: no [S, n, D] target is ever written.  vec: a group of
//                          G = 8 .. 64 lanes per patch, lane = patch row (kf, p1) -- C P/8 16-byte pixel loads, P C/8 16-byte
//                          loads of pred; the patch stays in registers, so the statistics are two passes over registers
//                          (sum; sum of squared deviations from the mean) and the clip is read once.  any: one wave per
//                          patch, scalar accesses, any P, C, alignment; the passes re-read the patch (it sits in L1 / L2).
//                          Both: sums by butterflies inside the group -- a fixed order.  Kept positions get exact zeros.
//   loss_finalize_kernel   loss = sum(per_patch) / M, summed and divided in double, one workgroup, a fixed order.
//
// Index safety: an entry of slot outside [0, k) counts as dropped and an entry of keep outside [0, n) yields a zero row -- each
// is compared as unsigned against its bound before any address is formed from it.
#include "common.h"

namespace {

constexpr int kBlock = 256;

// ------------------------------------------------------------------ restore and its adjoint
template <typename T>
__global__ void restore_fwd_kernel(const T* __restrict__ y, const float* __restrict__ mask, const float* __restrict__ pos,
                                   const int32_t* __restrict__ slot, T* __restrict__ out, int64_t S, int64_t Tn, int n, int k,
                                   int skip, int64_t d) {
  const int64_t dv = d >> 3;
  const int64_t items = S * n * dv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const int64_t c = (it % dv) << 3;
    const int64_t row = it / dv;
    const int64_t j = row % n;
    const int64_t s = row / n;
    const int32_t sl = slot[row];
    float v[8], p[8];
    if ((unsigned)sl < (unsigned)k) load8<T>(y + (s * (skip + k) + skip + sl) * d + c, v);
    else load8<float>(mask + c, v);
    load8<float>(pos + ((s % Tn) * n + j) * d + c, p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += p[e];
    store8<T>(out + row * d + c, v);
  }
}

template <typename T>
__global__ void restore_dy_kernel(const T* __restrict__ dout, const int32_t* __restrict__ keep, T* __restrict__ dy, int64_t S,
                                  int n, int k, int skip, int64_t d) {
  const int64_t dv = d >> 3;
  const int64_t rows_per = (int64_t)skip + k;
  const int64_t items = S * rows_per * dv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const int64_t c = (it % dv) << 3;
    const int64_t row = it / dv;
    const int64_t r = row % rows_per;
    const int64_t s = row / rows_per;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r >= skip) {
      const int32_t q = keep[s * k + (r - skip)];
      if ((unsigned)q < (unsigned)n) load8<T>(dout + (s * n + q) * d + c, v);
    }
    store8<T>(dy + row * d + c, v);
  }
}

template <typename T>
__global__ void restore_dpos_kernel(const T* __restrict__ dout, const int32_t* __restrict__ slot, float* __restrict__ dpos,
                                    float* __restrict__ partial, int64_t S, int64_t Tn, int n, int k, int64_t d,
                                    int accumulate) {
  const int64_t dv = d >> 3;
  const int64_t items = Tn * n * dv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t B = S / Tn;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const int64_t c = (it % dv) << 3;
    const int64_t row = it / dv;                               // tau * n + j
    const int64_t j = row % n;
    const int64_t t = row / n;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, macc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t b = 0; b < B; ++b) {
      const int64_t src = (b * Tn + t) * n + j;
      float v[8];
      load8<T>(dout + src * d + c, v);
      const bool dropped = !((unsigned)slot[src] < (unsigned)k);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        acc[e] += v[e];
        if (dropped) macc[e] += v[e];
      }
    }
    float* o = dpos + row * d + c;
    if (accumulate) {
      float p[8];
      load8<float>(o, p);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += p[e];
    }
    store8<float>(o, acc);
    store8<float>(partial + row * d + c, macc);
  }
}

// out[c] (+)= sum_{r < R} x[r * d + c]: one workgroup per 8-column chunk, a fixed order of additions
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, int64_t d, int64_t R, float* __restrict__ out,
                                                     int accumulate) {
  __shared__ float red[8][kBlock / 64];
  const int64_t c = (int64_t)blockIdx.x << 3;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t r = threadIdx.x; r < R; r += kBlock) {
    float v[8];
    load8<float>(x + r * d + c, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += v[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float s = wave_sum(acc[e]);
    if ((threadIdx.x & 63) == 0) red[e][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    float t = 0.f;
    for (int i = 0; i < kBlock / 64; ++i) t += red[threadIdx.x][i];
    float* o = out + c + threadIdx.x;
    *o = accumulate ? *o + t : t;
  }
}

// ------------------------------------------------------------------ masked patch loss
// sum over the aligned group of G lanes (a power of two) a lane sits in; every lane of the wave takes part
__device__ __forceinline__ float group_sum(float v, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// BWD false: per_patch[row] = mean_D (pred - target)^2, stats_out[row] = {mean, rstd} (norm_pix), zeros at kept positions.
// BWD true:  dpred[row, :] = gloss[0] * scale * (pred - target), zeros at kept positions; the statistics come from stats_in.
// Lane gl of a group holds patch row (kf, p1) = (gl / P, gl % P) in vector order (p2 C + c); lanes gl >= pt P idle.  The trip
// count of the row loop is the same for every lane of the grid, so the butterflies see whole waves.
template <int P, int C, typename S, typename T, bool BWD>
__global__ __launch_bounds__(256) void loss_vec_kernel(const T* __restrict__ pred, const S* __restrict__ x,
                                                       const int32_t* __restrict__ slot, float* __restrict__ per_patch,
                                                       float* __restrict__ stats_out, const float* __restrict__ stats_in,
                                                       const float* __restrict__ gloss, float scale, T* __restrict__ dpred,
                                                       int64_t rows, int H, int W, int pt, int n, int k, int G, int norm_pix,
                                                       float eps) {
  constexpr int PC = P * C;
  const int nw = W / P;
  const int lpr = pt * P;
  const int64_t D = (int64_t)lpr * PC;
  const int gl = threadIdx.x & (G - 1);
  const int64_t per_block = kBlock / G;
  const int64_t gstride = (int64_t)gridDim.x * per_block;
  const int64_t trips = (rows + gstride - 1) / gstride;
  float coef = 0.f;
  if constexpr (BWD) coef = gloss[0] * scale;
  for (int64_t trip = 0; trip < trips; ++trip) {
    const int64_t row = (int64_t)blockIdx.x * per_block + threadIdx.x / G + trip * gstride;
    const bool valid = row < rows;
    const int32_t sl = valid ? slot[row] : 0;
    const bool dropped = valid && !((unsigned)sl < (unsigned)k);
    const bool active = dropped && gl < lpr;
    float xv[PC];
#pragma unroll
    for (int e = 0; e < PC; ++e) xv[e] = 0.f;
    if (active) {
      const int64_t s = row / n;
      const int j = (int)(row - s * n);
      const int ph = j / nw, pw = j - ph * nw;
      const int kf = gl / P, p1 = gl - kf * P;
      const int64_t xoff = (((s * pt + kf) * C) * H + (int64_t)ph * P + p1) * W + (int64_t)pw * P;
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int q = 0; q < P / 8; ++q) {
          float t[8];
          load8<S>(x + xoff + (int64_t)c * H * W + q * 8, t);
#pragma unroll
          for (int e = 0; e < 8; ++e) xv[(q * 8 + e) * C + c] = t[e];
        }
    }
    const int64_t poff = row * D + (int64_t)gl * PC;
    if constexpr (BWD) {
      if (!valid || gl >= lpr) continue;                        // no butterflies in this direction
      float mean = 0.f, rstd = 1.f;
      if (norm_pix && dropped) { mean = stats_in[2 * row]; rstd = stats_in[2 * row + 1]; }
#pragma unroll
      for (int q = 0; q < PC / 8; ++q) {
        float o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (dropped) {
          float p[8];
          load8<T>(pred + poff + q * 8, p);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = coef * (p[e] - (xv[q * 8 + e] - mean) * rstd);
        }
        store8<T>(dpred + poff + q * 8, o);
      }
    } else {
      float mean = 0.f, rstd = 1.f;
      if (norm_pix) {
        float s1 = 0.f;
#pragma unroll
        for (int e = 0; e < PC; ++e) s1 += xv[e];
        mean = group_sum(s1, G) / (float)D;
        float s2 = 0.f;
        if (active) {
#pragma unroll
          for (int e = 0; e < PC; ++e) {
            const float dl = xv[e] - mean;
            s2 += dl * dl;
          }
        }
        rstd = 1.0f / sqrtf(group_sum(s2, G) / (float)(D - 1) + eps);
      }
      float acc = 0.f;
      if (active) {
#pragma unroll
        for (int q = 0; q < PC / 8; ++q) {
          float p[8];
          load8<T>(pred + poff + q * 8, p);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float df = p[e] - (xv[q * 8 + e] - mean) * rstd;
            acc += df * df;
          }
        }
      }
      acc = group_sum(acc, G);
      if (valid && gl == 0) {
        per_patch[row] = dropped ? acc / (float)D : 0.f;
        if (stats_out) {
          stats_out[2 * row] = dropped ? mean : 0.f;
          stats_out[2 * row + 1] = dropped ? rstd : 0.f;
        }
      }
    }
  }
}

// Any P, C and alignment: one wave per patch, lanes stride the D columns of the row.
template <typename S, typename T, bool BWD>
__global__ __launch_bounds__(256) void loss_any_kernel(const T* __restrict__ pred, const S* __restrict__ x,
                                                       const int32_t* __restrict__ slot, float* __restrict__ per_patch,
                                                       float* __restrict__ stats_out, const float* __restrict__ stats_in,
                                                       const float* __restrict__ gloss, float scale, T* __restrict__ dpred,
                                                       int64_t rows, int C, int H, int W, int P, int pt, int n, int k,
                                                       int norm_pix, float eps) {
  const unsigned nw = W / P;
  const unsigned pd = (unsigned)P * P * C, pc = (unsigned)P * C;
  const unsigned D = pd * pt;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (kBlock / 64);
  float coef = 0.f;
  if constexpr (BWD) coef = gloss[0] * scale;
  for (int64_t row = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); row < rows; row += nwaves) {   // wave-uniform
    const bool dropped = !((unsigned)slot[row] < (unsigned)k);
    if (!dropped) {
      if constexpr (BWD) {
        for (unsigned col = lane; col < D; col += 64) dpred[row * D + col] = from_f32<T>(0.f);
      } else if (lane == 0) {
        per_patch[row] = 0.f;
        if (stats_out) { stats_out[2 * row] = 0.f; stats_out[2 * row + 1] = 0.f; }
      }
      continue;
    }
    const int64_t s = row / n;
    const unsigned j = (unsigned)(row - s * n);
    const unsigned ph = j / nw, pw = j - ph * nw;
    auto pixel = [&](unsigned col) -> float {
      const unsigned kf = col / pd, e = col - kf * pd;
      const unsigned p1 = e / pc, r = e - p1 * pc;
      const unsigned p2 = r / C, c = r - p2 * C;
      const int64_t f = s * pt + kf;
      return to_f32<S>(x[((f * C + c) * H + (int64_t)(ph * P + p1)) * W + (int64_t)(pw * P + p2)]);
    };
    float mean = 0.f, rstd = 1.f;
    if constexpr (BWD) {
      if (norm_pix) { mean = stats_in[2 * row]; rstd = stats_in[2 * row + 1]; }
      for (unsigned col = lane; col < D; col += 64) {
        const float p = to_f32<T>(pred[row * D + col]);
        dpred[row * D + col] = from_f32<T>(coef * (p - (pixel(col) - mean) * rstd));
      }
    } else {
      if (norm_pix) {
        float s1 = 0.f;
        for (unsigned col = lane; col < D; col += 64) s1 += pixel(col);
        mean = wave_sum(s1) / (float)D;
        float s2 = 0.f;
        for (unsigned col = lane; col < D; col += 64) {
          const float dl = pixel(col) - mean;
          s2 += dl * dl;
        }
        rstd = 1.0f / sqrtf(wave_sum(s2) / (float)(D - 1) + eps);
      }
      float acc = 0.f;
      for (unsigned col = lane; col < D; col += 64) {
        const float df = to_f32<T>(pred[row * D + col]) - (pixel(col) - mean) * rstd;
        acc += df * df;
      }
      acc = wave_sum(acc);
      if (lane == 0) {
        per_patch[row] = acc / (float)D;
        if (stats_out) { stats_out[2 * row] = mean; stats_out[2 * row + 1] = rstd; }
      }
    }
  }
}

// loss[0] = sum(per_patch[0 .. rows)) / M, in double (kept positions hold zeros); one workgroup, a fixed order
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* __restrict__ per_patch, int64_t rows, double M,
                                                            float* __restrict__ loss) {
  __shared__ double red[kBlock];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < rows; i += kBlock) s += (double)per_patch[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0] / M);
}

struct LossArgs {
  const void* pred;
  const void* clip;
  const int32_t* slot;
  float* per_patch;
  float* stats_out;
  const float* stats_in;
  const float* gloss;
  float scale;
  void* dpred;
  int64_t rows;
  int C, H, W, P, pt, n, k, norm_pix;
  float eps;
};

template <typename S, typename T, bool BWD>
int loss_dispatch(const LossArgs& a, hipStream_t st, const char* name) {
  const int64_t D = (int64_t)a.pt * a.P * a.P * a.C;
  const int lpr = a.pt * a.P;
  const bool vec_ok = (a.W % 8 == 0) && (a.P % 8 == 0) && ((a.P * a.C) % 8 == 0) && ((int64_t)a.H * a.W % 8 == 0) &&
                      dvt_aligned16(a.pred) && dvt_aligned16(a.clip) && (!BWD || dvt_aligned16(a.dpred)) && lpr <= 64;
  auto pred = (const T*)a.pred;
  auto x = (const S*)a.clip;
  auto dpred = (T*)a.dpred;
  if (vec_ok && a.C == 3 && (a.P == 16 || a.P == 8)) {
    int G = 8;
    while (G < lpr) G <<= 1;
    const int64_t per_block = kBlock / G;
    int64_t blocks = dvt_cdiv(a.rows, per_block);
    const int64_t cap = (int64_t)dvt_num_cus() * 8;
    if (blocks > cap) blocks = cap;
    if (a.P == 16)
      hipLaunchKernelGGL((loss_vec_kernel<16, 3, S, T, BWD>), dim3((unsigned)blocks), dim3(kBlock), 0, st, pred, x, a.slot,
                         a.per_patch, a.stats_out, a.stats_in, a.gloss, a.scale, dpred, a.rows, a.H, a.W, a.pt, a.n, a.k, G,
                         a.norm_pix, a.eps);
    else
      hipLaunchKernelGGL((loss_vec_kernel<8, 3, S, T, BWD>), dim3((unsigned)blocks), dim3(kBlock), 0, st, pred, x, a.slot,
                         a.per_patch, a.stats_out, a.stats_in, a.gloss, a.scale, dpred, a.rows, a.H, a.W, a.pt, a.n, a.k, G,
                         a.norm_pix, a.eps);
  } else {
    if (D >= ((int64_t)1 << 31)) DVT_UNSUPPORTED("%s: a row of pt*P*P*C >= 2^31 elements", name);
    hipLaunchKernelGGL((loss_any_kernel<S, T, BWD>), dim3(dvt_grid(a.rows * 64)), dim3(kBlock), 0, st, pred, x, a.slot,
                       a.per_patch, a.stats_out, a.stats_in, a.gloss, a.scale, dpred, a.rows, a.C, a.H, a.W, a.P, a.pt, a.n,
                       a.k, a.norm_pix, a.eps);
  }
  DVT_LAUNCH_CHECK(name);
  return DVT_OK;
}

template <bool BWD>
int loss_entry(LossArgs a, int pred_dtype, int clip_dtype, int64_t frames, dvt_stream_t stream, double* M_out,
               const char* name) {
  DVT_REQUIRE(a.pred && a.clip && a.slot, "%s: null pointer", name);
  DVT_REQUIRE(a.pt >= 1, "%s: tubelet length %d < 1", name, a.pt);
  DVT_REQUIRE(frames > 0 && a.C > 0 && a.H > 0 && a.W > 0 && a.P > 0, "%s: bad sizes", name);
  DVT_REQUIRE(frames % a.pt == 0, "%s: %lld frames are not whole tubelets of %d", name, (long long)frames, a.pt);
  DVT_REQUIRE(a.H % a.P == 0 && a.W % a.P == 0, "%s: image %dx%d not divisible by patch %d", name, a.H, a.W, a.P);
  DVT_REQUIRE((int64_t)(a.H / a.P) * (a.W / a.P) < ((int64_t)1 << 31), "%s: 2^31 positions or more per frame", name);
  a.n = (a.H / a.P) * (a.W / a.P);
  DVT_REQUIRE(a.k >= 1 && a.k < a.n, "%s: k = %d outside 1 .. n - 1 = %d: no masked patch (M == 0) or no kept one", name, a.k,
              a.n - 1);
  const int64_t D = (int64_t)a.pt * a.P * a.P * a.C;
  DVT_REQUIRE(!a.norm_pix || D >= 2, "%s: the unbiased variance needs patches of 2 values or more", name);
  DVT_REQUIRE(!a.norm_pix || a.eps > 0.f, "%s: eps = %g must be positive", name, (double)a.eps);
  a.rows = (frames / a.pt) * a.n;
  const double M = (double)(frames / a.pt) * (double)(a.n - a.k);
  a.scale = (float)(2.0 / (M * (double)D));
  *M_out = M;
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(clip_dtype, Sx,
                     DVT_DISPATCH_DTYPE(pred_dtype, Tp, return (loss_dispatch<Sx, Tp, BWD>(a, st, name))));
  return DVT_OK;
}

int restore_args(const char* name, int64_t S, int64_t T, int n, int k, int skip, int64_t d) {
  DVT_REQUIRE(S > 0 && T > 0 && n >= 1 && d > 0 && S % T == 0, "%s: bad sizes", name);
  DVT_REQUIRE(k >= 1 && k <= n, "%s: k = %d outside 1 .. n = %d", name, k, n);
  DVT_REQUIRE(skip >= 0, "%s: skip = %d < 0", name, skip);
  DVT_REQUIRE(d % 8 == 0, "%s: d = %lld must be a multiple of 8", name, (long long)d);
  return DVT_OK;
}

}  // namespace

extern "C" {

int dvt_tokens_restore_fwd(const void* y, const float* mask, const float* pos, const int32_t* slot, void* out, int64_t S,
                           int64_t T, int n, int k, int skip, int64_t d, int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(y && mask && pos && slot && out, "dvt_tokens_restore_fwd: null pointer");
  if (int rc = restore_args("dvt_tokens_restore_fwd", S, T, n, k, skip, d)) return rc;
  DVT_REQUIRE(dvt_aligned16(y) && dvt_aligned16(mask) && dvt_aligned16(pos) && dvt_aligned16(out),
              "dvt_tokens_restore_fwd: buffers must be 16-byte aligned");
  DVT_DISPATCH_DTYPE(dtype, Tt,
                     hipLaunchKernelGGL((restore_fwd_kernel<Tt>), dim3(dvt_grid(S * n * (d >> 3))), dim3(kBlock), 0,
                                        (hipStream_t)stream, (const Tt*)y, mask, pos, slot, (Tt*)out, S, T, n, k, skip, d));
  DVT_LAUNCH_CHECK("dvt_tokens_restore_fwd");
  return DVT_OK;
}

int dvt_tokens_restore_bwd(const void* dout, const int32_t* keep, const int32_t* slot, void* dy, float* dmask, float* dpos,
                           float* partial, int64_t S, int64_t T, int n, int k, int skip, int64_t d, int dtype, int accumulate,
                           dvt_stream_t stream) {
  DVT_REQUIRE(dout && keep && slot && dy && dmask && dpos && partial, "dvt_tokens_restore_bwd: null pointer");
  if (int rc = restore_args("dvt_tokens_restore_bwd", S, T, n, k, skip, d)) return rc;
  DVT_REQUIRE(dvt_aligned16(dout) && dvt_aligned16(dy) && dvt_aligned16(dmask) && dvt_aligned16(dpos) && dvt_aligned16(partial),
              "dvt_tokens_restore_bwd: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t dv = d >> 3;
  DVT_DISPATCH_DTYPE(dtype, Tt, {
    hipLaunchKernelGGL((restore_dy_kernel<Tt>), dim3(dvt_grid(S * ((int64_t)skip + k) * dv)), dim3(kBlock), 0, st,
                       (const Tt*)dout, keep, (Tt*)dy, S, n, k, skip, d);
    hipLaunchKernelGGL((restore_dpos_kernel<Tt>), dim3(dvt_grid(T * n * dv)), dim3(kBlock), 0, st, (const Tt*)dout, slot, dpos,
                       partial, S, T, n, k, d, accumulate);
  });
  hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)dv), dim3(kBlock), 0, st, (const float*)partial, d, T * n, dmask,
                     accumulate);
  DVT_LAUNCH_CHECK("dvt_tokens_restore_bwd");
  return DVT_OK;
}

int dvt_mae_loss_fwd(const void* pred, int pred_dtype, const void* clip, int clip_dtype, const int32_t* slot, float* per_patch,
                     float* stats, float* loss, int64_t frames, int C, int H, int W, int P, int pt, int k, int norm_pix,
                     float eps, dvt_stream_t stream) {
  DVT_REQUIRE(per_patch && loss, "dvt_mae_loss_fwd: null pointer");
  DVT_REQUIRE(!norm_pix || stats, "dvt_mae_loss_fwd: norm_pix needs stats [S, n, 2]");
  LossArgs a{pred, clip, slot, per_patch, norm_pix ? stats : nullptr, nullptr, nullptr, 0.f, nullptr, 0, C, H, W, P, pt, 0, k,
             norm_pix, eps};
  double M = 0.0;
  if (int rc = loss_entry<false>(a, pred_dtype, clip_dtype, frames, stream, &M, "dvt_mae_loss_fwd")) return rc;
  const int64_t rows = (frames / pt) * (int64_t)((H / P) * (W / P));
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const float*)per_patch, rows, M,
                     loss);
  DVT_LAUNCH_CHECK("dvt_mae_loss_fwd");
  return DVT_OK;
}

int dvt_mae_loss_bwd(const void* pred, int pred_dtype, const void* clip, int clip_dtype, const int32_t* slot,
                     const float* stats, const float* gloss, void* dpred, int64_t frames, int C, int H, int W, int P, int pt,
                     int k, int norm_pix, dvt_stream_t stream) {
  DVT_REQUIRE(gloss && dpred, "dvt_mae_loss_bwd: null pointer");
  DVT_REQUIRE(!norm_pix || stats, "dvt_mae_loss_bwd: norm_pix needs the forward's stats [S, n, 2]");
  LossArgs a{pred, clip, slot, nullptr, nullptr, norm_pix ? stats : nullptr, gloss, 0.f, dpred, 0, C, H, W, P, pt, 0, k,
             norm_pix, 1.f};
  double M = 0.0;
  return loss_entry<true>(a, pred_dtype, clip_dtype, frames, stream, &M, "dvt_mae_loss_bwd");
}

}  // extern "C"
