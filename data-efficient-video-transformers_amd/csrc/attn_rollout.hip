// attn_rollout.hip -- attention rollout (Abnar & Zuidema, 2020) without score matrices.
//
// With A_l = rho I + (1 - rho) mean_h softmax(scale Q_l^h K_l^h^T) the rollout of a start vector r0 is the ROW
// r0^T A_L ... A_1, so a layer is one vector-matrix product
//     r_out[s, j] = rho r_in[s, j] + (1 - rho) / H sum_h sum_i r_in[s, i] exp(scale q_i . k_j - lse[s, h, i])
// with the lse dvt_attention_fwd wrote: a Q K^T tile, an exponential and a weighted column sum.  No N x N tensor exists,
// the probabilities and r stay fp32 (nothing is rounded to 16 bits after the exponential).
//
//   rollout_step_mfma_kernel      16-bit, dh == 64, N <= 512.  One workgroup per sequence, a loop over the heads inside.  The
//       head's Q is staged in LDS as a swizzled [query][64] image (double-buffered: head h + 1 lands while head h computes),
//       with -lse log2(e) and r beside it (0 for the padded queries, whose image rows are 0 too: they add exact zeros and no
//       lse of theirs is read).  Wave (kp, part) owns the 32-key step kp -- its four K fragments come straight from global
//       memory, clamped to the last key for the padded ones, which are never written -- and every `parts`-th 16-query tile:
//       S^T = K Q^T on mfma_f32_16x16x32 with the query on the MFMA column, so a lane owns one query and scales its eight
//       scores by that query's r.  The eight per-lane accumulators run over tiles and heads; the sum over the queries then is
//         1. across the 16 query lanes (DPP butterfly, fixed),  2. across the wave rows `part` through LDS, in order,
//         3. (the heads were summed in order inside each lane).
//   rollout_step_generic_kernel   any dtype / dh / N that fits LDS, fp32 FMA, one workgroup per sequence, a thread per key,
//       eight queries at a time from LDS.  Every one-hot start (one query row; Lq == 1 layers) takes it: that is a
//       matrix-vector product of N x dh per head.
//   rollout_from_probs_kernel     r = rho e_query + (1 - rho) mean_h P from the folded single-query layer's P [S][N][8].
//   rollout_video_kernel          time x space per clip and the per-clip scaling of cam.hip (cam_scale.h), one launch.
// No float atomics anywhere: identical calls give bitwise-equal results, whatever the grid order.
#include "common.h"
#include "cam_scale.h"

namespace {

constexpr int kMaxLds = 160 * 1024;
constexpr float kLog2e = 1.4426950408889634f;
constexpr int kRowBytes = 128;                    // a 64-element 16-bit row
constexpr int kQC = 8;                            // generic form: queries per LDS chunk
constexpr int kGenericThreads = 256;

struct RolloutParams {
  const void *q, *k;
  const float *lse, *r_in;
  float* r_out;
  int S, H, N, Lq, dh;
  int64_t q_sb, q_sh, q_sl, k_sb, k_sh, k_sl;
  int query;                                      // r_in == nullptr: one-hot token, or DVT_ROLLOUT_UNIFORM
  float rho, scale;
  int nkp, parts, nqt;                            // MFMA form: 32-key steps, wave rows, 16-query tiles
};

// entry i of sequence s's start vector
__device__ __forceinline__ float start_value(const RolloutParams& p, int s, int i) {
  if (p.r_in != nullptr) return p.r_in[(int64_t)s * p.N + i];
  if (p.query < 0) return 1.0f / (float)p.N;
  return i == p.query ? 1.0f : 0.0f;
}

// ======================================================================= generic
// LDS: r [N] | acc [N] | nl [kQC] | rw [kQC] | q chunk [kQC][dh]
template <typename T>
__global__ __launch_bounds__(kGenericThreads) void rollout_step_generic_kernel(const RolloutParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  float* rs = lds_f;
  float* acc = rs + p.N;
  float* nl = acc + p.N;
  float* rw = nl + kQC;
  float* qv = rw + kQC;
  const int s = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < p.N; j += kGenericThreads) {
    rs[j] = start_value(p, s, j);
    acc[j] = 0.f;
  }
  const bool one = p.r_in == nullptr && p.query >= 0;
  const int i0 = one ? p.query : 0, i1 = one ? p.query + 1 : p.N;
  for (int h = 0; h < p.H; ++h) {
    const T* qb = (const T*)p.q + (int64_t)s * p.q_sb + (int64_t)h * p.q_sh;
    const T* kb = (const T*)p.k + (int64_t)s * p.k_sb + (int64_t)h * p.k_sh;
    const float* lse = p.lse + ((int64_t)s * p.H + h) * p.Lq;
    for (int ic = i0; ic < i1; ic += kQC) {
      __syncthreads();                              // the previous chunk is consumed (and rs / acc are initialised)
      const int nq = min(kQC, i1 - ic);
      for (int idx = tid; idx < kQC * p.dh; idx += kGenericThreads) {
        const int qi = idx / p.dh, e = idx - qi * p.dh;
        const int row = p.Lq == 1 ? 0 : ic + qi;
        qv[idx] = qi < nq ? to_f32<T>(qb[(int64_t)row * p.q_sl + e]) : 0.f;
      }
      if (tid < kQC) {
        const int row = p.Lq == 1 ? 0 : ic + tid;
        nl[tid] = tid < nq ? lse[row] : 0.f;         // a padded query: zero row, zero lse, zero weight
        rw[tid] = tid < nq ? rs[ic + tid] : 0.f;
      }
      __syncthreads();
      for (int j = tid; j < p.N; j += kGenericThreads) {
        const T* kj = kb + (int64_t)j * p.k_sl;
        float sc[kQC];
#pragma unroll
        for (int qi = 0; qi < kQC; ++qi) sc[qi] = 0.f;
        for (int e = 0; e < p.dh; ++e) {
          const float kv = to_f32<T>(kj[e]);
#pragma unroll
          for (int qi = 0; qi < kQC; ++qi) sc[qi] = fmaf(qv[qi * p.dh + e], kv, sc[qi]);
        }
        float a = acc[j];
#pragma unroll
        for (int qi = 0; qi < kQC; ++qi) a = fmaf(rw[qi], expf(fmaf(sc[qi], p.scale, -nl[qi])), a);
        acc[j] = a;
      }
    }
  }
  __syncthreads();
  const float w = (1.0f - p.rho) / (float)p.H;
  for (int j = tid; j < p.N; j += kGenericThreads) p.r_out[(int64_t)s * p.N + j] = fmaf(p.rho, rs[j], w * acc[j]);
}

// ======================================================================= MFMA, 16-bit, dh = 64
// byte offset of 16-byte chunk c (0..7) of row r in a [rows][64] image: 32-byte units XOR-swizzled by (r >> 1) & 3, which
// keeps the ds_read_b128 row reads of a fragment (16 rows x one chunk column) off each other's banks
__device__ __forceinline__ int img_off(int r, int c) {
  return r * kRowBytes + ((((c >> 1) ^ ((r >> 1) & 3)) << 5) | ((c & 1) << 4));
}

// LDS: Q image [2][nqt*16][128 B] | nl [2][nqt*16] | r [nqt*16] | part [parts][nkp*32]
template <typename E>
__global__ __launch_bounds__(1024) void rollout_step_mfma_kernel(const RolloutParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using V8 = typename Elem16<E>::v8;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nt = blockDim.x;
  const int g = lane >> 4, li = lane & 15;
  const int s = blockIdx.x;
  const int nq16 = p.nqt * 16, nk32 = p.nkp * 32;
  const int img_bytes = nq16 * kRowBytes;
  float* nlv = reinterpret_cast<float*>(smem + 2 * img_bytes);
  float* rs = nlv + 2 * nq16;
  float* part = rs + nq16;
  const int kp = wid % p.nkp, qpart = wid / p.nkp;

  auto stage = [&](int h) {                          // head h's Q rows and -lse log2(e) into buffer h & 1
    char* img = smem + (h & 1) * img_bytes;
    float* nl = nlv + (h & 1) * nq16;
    const E* qb = (const E*)p.q + (int64_t)s * p.q_sb + (int64_t)h * p.q_sh;
    const float* lse = p.lse + ((int64_t)s * p.H + h) * p.N;
    for (int idx = tid; idx < nq16 * 8; idx += nt) {
      const int r = idx >> 3, c = idx & 7;
      V8 v = V8{0, 0, 0, 0, 0, 0, 0, 0};
      if (r < p.N) v = *reinterpret_cast<const V8*>(qb + (int64_t)r * p.q_sl + c * 8);
      *reinterpret_cast<V8*>(img + img_off(r, c)) = v;
    }
    for (int i = tid; i < nq16; i += nt) nl[i] = i < p.N ? -lse[i] * kLog2e : 0.f;
  };

  for (int i = tid; i < nq16; i += nt) rs[i] = i < p.N ? start_value(p, s, i) : 0.f;
  stage(0);

  const float c2 = p.scale * kLog2e;
  f32x4 acc[2];
  acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
  acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int h = 0; h < p.H; ++h) {
    // this wave's 32 keys of head h: fragment (tt, kk) = K[(2 kp + tt) 16 + li][kk 32 + 8 g .. + 7]
    const E* kb = (const E*)p.k + (int64_t)s * p.k_sb + (int64_t)h * p.k_sh;
    V8 kf[2][2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int key = min((2 * kp + tt) * 16 + li, p.N - 1);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) kf[tt][kk] = *reinterpret_cast<const V8*>(kb + (int64_t)key * p.k_sl + kk * 32 + g * 8);
    }
    __syncthreads();                                 // buffer h & 1 is staged; everyone is done with buffer (h + 1) & 1
    if (h + 1 < p.H) stage(h + 1);
    const char* img = smem + (h & 1) * img_bytes;
    const float* nl = nlv + (h & 1) * nq16;
    for (int qt = qpart; qt < p.nqt; qt += p.parts) {
      f32x4 sc[2];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        sc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const V8 qf = *reinterpret_cast<const V8*>(img + img_off(qt * 16 + li, kk * 4 + g));
          sc[tt] = Elem16<E>::mma(kf[tt][kk], qf, sc[tt]);
        }
      }
      const float nli = nl[qt * 16 + li], ri = rs[qt * 16 + li];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[tt][r] = fmaf(ri, __builtin_amdgcn_exp2f(fmaf(sc[tt][r], c2, nli)), acc[tt][r]);
    }
  }
  // 1. across the 16 query lanes of a row: every lane of the row ends with the row's total
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc[tt][r];
      v += dpp_mov<kDppXor1>(v);
      v += dpp_mov<kDppXor2>(v);
      v += dpp_mov<kDppHalfMirror>(v);
      v += dpp_mov<kDppMirror>(v);
      acc[tt][r] = v;
    }
  if (li == 0) {
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int r = 0; r < 4; ++r) part[qpart * nk32 + (2 * kp + tt) * 16 + 4 * g + r] = acc[tt][r];
  }
  __syncthreads();
  // 2. across the wave rows, in order; the padded keys are not written
  const float w = (1.0f - p.rho) / (float)p.H;
  for (int j = tid; j < p.N; j += nt) {
    float t = part[j];
    for (int q = 1; q < p.parts; ++q) t += part[q * nk32 + j];
    p.r_out[(int64_t)s * p.N + j] = fmaf(p.rho, rs[j], w * t);
  }
}

// ======================================================================= the start from the folded layer's probabilities
__global__ __launch_bounds__(256) void rollout_from_probs_kernel(const float* __restrict__ P, int64_t total, int N, int H,
                                                                 int query, float rho, float* __restrict__ r_out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx % N);
  float t = 0.f;
  for (int h = 0; h < H; ++h) t += P[idx * 8 + h];
  r_out[idx] = fmaf(rho, j == query ? 1.f : 0.f, (1.0f - rho) / (float)H * t);
}

// ======================================================================= time x space, scaled per clip
// One workgroup per clip; the product is formed twice (extrema, then write) and never stored in between.  A handful of
// clips cannot fill the chip, so the launch is a chain of dependent loads per thread: sixteen waves keep that chain short.
constexpr int kVideoThreads = 1024;
__global__ __launch_bounds__(kVideoThreads) void rollout_video_kernel(const float* __restrict__ r_space,
                                                                      const float* __restrict__ r_time, int T, int n,
                                                                      float* __restrict__ raw, float* __restrict__ scaled) {
  __shared__ float red[2 * (kVideoThreads / 64)];
  const int64_t b = blockIdx.x;
  const int P = T * n;
  auto value = [&](int i) {
    const int f = i / n, pp = i - f * n;
    return r_time[b * (T + 1) + 1 + f] * r_space[(b * T + f) * (int64_t)(n + 1) + 1 + pp];
  };
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < P; i += kVideoThreads) {
    const float v = value(i);
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  block_extrema(mn, mx, red, kVideoThreads / 64);
  const float den = cam_scale_den(mn, mx);
  for (int i = threadIdx.x; i < P; i += kVideoThreads) {
    const float v = value(i);
    if (raw) raw[b * P + i] = v;
    scaled[b * P + i] = cam_scale_value(v, mn, den);
  }
}

// ======================================================================= host: one place for the decisions
bool vec_ok(const dvt_rollout_desc* d) {
  const int64_t st[] = {d->q_sb, d->q_sh, d->q_sl, d->k_sb, d->k_sh, d->k_sl};
  for (int64_t x : st)
    if (x % 8) return false;
  return dvt_aligned16(d->q) && dvt_aligned16(d->k);
}

size_t mfma_lds(int nqt, int nkp, int parts) {
  return (size_t)2 * nqt * 16 * kRowBytes + (size_t)3 * nqt * 16 * sizeof(float) + (size_t)parts * nkp * 32 * sizeof(float);
}

// Validates desc, fills p and info; refuses what the launcher refuses.  Needs no device.
int resolve(const dvt_rollout_desc* d, RolloutParams& p, dvt_rollout_plan_info& r, const char* name) {
  r = dvt_rollout_plan_info{};
  DVT_REQUIRE(d, "%s: null descriptor", name);
  DVT_REQUIRE(d->S >= 0 && d->H > 0 && d->N > 0 && d->dh > 0, "%s: bad shape S = %lld, H = %lld, N = %lld, dh = %lld", name,
              (long long)d->S, (long long)d->H, (long long)d->N, (long long)d->dh);
  DVT_REQUIRE(d->Lq == d->N || d->Lq == 1, "%s: Lq = %lld is neither N = %lld nor 1", name, (long long)d->Lq, (long long)d->N);
  DVT_REQUIRE(d->r_in != nullptr || d->query == DVT_ROLLOUT_UNIFORM || (d->query >= 0 && d->query < d->N),
              "%s: without r_in, query = %lld must be a token index below N = %lld or DVT_ROLLOUT_UNIFORM", name,
              (long long)d->query, (long long)d->N);
  const bool one = d->r_in == nullptr && d->query >= 0;
  DVT_REQUIRE(d->Lq == d->N || one, "%s: a layer with one query row (Lq == 1) takes the one-hot start (r_in NULL, query >= 0)", name);
  DVT_REQUIRE(d->rho >= 0.f && d->rho <= 1.f, "%s: rho = %g is outside [0, 1]", name, (double)d->rho);
  DVT_REQUIRE(d->dtype == DVT_F32 || dvt_is_16bit(d->dtype), "%s: dtype %d not supported", name, d->dtype);
  if (d->S >= ((int64_t)1 << 31) || d->N >= ((int64_t)1 << 24) || d->H >= 65536 || d->dh >= 65536)
    DVT_UNSUPPORTED("%s: S = %lld, H = %lld, N = %lld, dh = %lld: split the batch", name, (long long)d->S, (long long)d->H,
                    (long long)d->N, (long long)d->dh);
  p = RolloutParams{};
  p.q = d->q; p.k = d->k; p.lse = d->lse; p.r_in = d->r_in; p.r_out = d->r_out;
  p.S = (int)d->S; p.H = (int)d->H; p.N = (int)d->N; p.Lq = (int)d->Lq; p.dh = (int)d->dh;
  p.q_sb = d->q_sb; p.q_sh = d->q_sh; p.q_sl = d->q_sl; p.k_sb = d->k_sb; p.k_sh = d->k_sh; p.k_sl = d->k_sl;
  p.query = (int)d->query; p.rho = d->rho; p.scale = d->scale;
  if (d->S == 0) return DVT_OK;
  DVT_REQUIRE(d->q && d->k && d->lse && d->r_out, "%s: null q / k / lse / r_out", name);
  DVT_REQUIRE(d->r_out != d->r_in, "%s: r_out must not be r_in", name);
  if (!one && dvt_is_16bit(d->dtype) && d->dh == 64 && d->N <= DVT_ROLLOUT_MFMA_MAX_N && d->scale > 0.f && vec_ok(d)) {
    p.nkp = (p.N + 31) / 32;
    p.nqt = (p.N + 15) / 16;
    p.parts = 16 / p.nkp < p.nqt ? 16 / p.nkp : p.nqt;       // up to 16 waves: nkp columns x parts rows
    r.form = DVT_ROLLOUT_F_MFMA; r.key_steps = p.nkp; r.query_parts = p.parts; r.waves = p.nkp * p.parts;
    r.lds = (int64_t)mfma_lds(p.nqt, p.nkp, p.parts);
    return DVT_OK;
  }
  const size_t lds = ((size_t)2 * p.N + 2 * kQC + (size_t)kQC * p.dh) * sizeof(float);
  if (lds > (size_t)kMaxLds)
    DVT_UNSUPPORTED("%s: N = %d, dh = %d exceed the LDS budget of the generic form", name, p.N, p.dh);
  r.form = DVT_ROLLOUT_F_GENERIC; r.waves = kGenericThreads / 64; r.lds = (int64_t)lds;
  return DVT_OK;
}

template <typename K>
int set_lds(K kernel, size_t bytes) {
  if (bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return dvt_fail_hip(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
  }
  return 0;
}

}  // namespace

extern "C" {

int dvt_rollout_plan(const dvt_rollout_desc* d, dvt_rollout_plan_info* info) {
  DVT_REQUIRE(info, "dvt_rollout_plan: null info");
  RolloutParams p;
  return resolve(d, p, *info, "dvt_rollout_plan");
}

int dvt_rollout_step(const dvt_rollout_desc* d, dvt_stream_t stream) {
  RolloutParams p;
  dvt_rollout_plan_info r;
  int rc = resolve(d, p, r, "dvt_rollout_step");
  if (rc) return rc;
  if (r.form == DVT_ROLLOUT_F_NONE) return DVT_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.S);
  if (r.form == DVT_ROLLOUT_F_MFMA) {
    DVT_DISPATCH_16BIT(d->dtype, E, {
      if (int rc_ = set_lds(rollout_step_mfma_kernel<E>, (size_t)r.lds)) return rc_;
      hipLaunchKernelGGL((rollout_step_mfma_kernel<E>), grid, dim3(64 * r.waves), (size_t)r.lds, st, p);
    });
    DVT_LAUNCH_CHECK("dvt_rollout_step (mfma)");
    return DVT_OK;
  }
  DVT_DISPATCH_DTYPE(d->dtype, T, {
    if (int rc_ = set_lds(rollout_step_generic_kernel<T>, (size_t)r.lds)) return rc_;
    hipLaunchKernelGGL((rollout_step_generic_kernel<T>), grid, dim3(kGenericThreads), (size_t)r.lds, st, p);
  });
  DVT_LAUNCH_CHECK("dvt_rollout_step (generic)");
  return DVT_OK;
}

int dvt_rollout_from_probs(const float* P, int64_t S, int64_t N, int64_t H, int64_t query, float rho, float* r_out,
                           dvt_stream_t stream) {
  DVT_REQUIRE(S >= 0 && N > 0 && H > 0 && H <= 8, "dvt_rollout_from_probs: bad shape S = %lld, N = %lld, H = %lld (at most 8 heads)",
              (long long)S, (long long)N, (long long)H);
  DVT_REQUIRE(query >= 0 && query < N, "dvt_rollout_from_probs: query = %lld is no token index below N = %lld", (long long)query,
              (long long)N);
  DVT_REQUIRE(rho >= 0.f && rho <= 1.f, "dvt_rollout_from_probs: rho = %g is outside [0, 1]", (double)rho);
  if (N >= ((int64_t)1 << 31) || S * N >= ((int64_t)1 << 38))
    DVT_UNSUPPORTED("dvt_rollout_from_probs: [%lld][%lld]: split the batch", (long long)S, (long long)N);
  if (S == 0) return DVT_OK;
  DVT_REQUIRE(P && r_out, "dvt_rollout_from_probs: null P / r_out");
  hipLaunchKernelGGL(rollout_from_probs_kernel, dim3((unsigned)dvt_cdiv(S * N, 256)), dim3(256), 0, (hipStream_t)stream, P,
                     S * N, (int)N, (int)H, (int)query, rho, r_out);
  DVT_LAUNCH_CHECK("dvt_rollout_from_probs");
  return DVT_OK;
}

int dvt_rollout_video(const float* r_space, const float* r_time, int64_t B, int64_t T, int64_t n, float* raw, float* scaled,
                      dvt_stream_t stream) {
  DVT_REQUIRE(B >= 0 && T > 0 && n > 0, "dvt_rollout_video: bad shape B = %lld, T = %lld, n = %lld", (long long)B, (long long)T,
              (long long)n);
  if (B >= ((int64_t)1 << 31) || T * n >= ((int64_t)1 << 30))
    DVT_UNSUPPORTED("dvt_rollout_video: %lld clips of %lld x %lld: split the batch", (long long)B, (long long)T, (long long)n);
  if (B == 0) return DVT_OK;
  DVT_REQUIRE(r_space && r_time && scaled, "dvt_rollout_video: null r_space / r_time / scaled");
  hipLaunchKernelGGL(rollout_video_kernel, dim3((unsigned)B), dim3(kVideoThreads), 0, (hipStream_t)stream, r_space, r_time, (int)T,
                     (int)n, raw, scaled);
  DVT_LAUNCH_CHECK("dvt_rollout_video");
  return DVT_OK;
}

}  // extern "C"
