// lstm.hip -- the recurrent chain of nn.LSTM(batch_first=True) (src/models/LSTM.py:32-38 forward, :40-45 its use).
//
// One layer over a whole sequence is T dependent steps.  The input projection x W_ih^T of every step is one large GEMM
// done before the chain (dvt_gemm), and the weight / bias / input gradients are large GEMMs done after the backward chain;
// only the h_{t-1} W_hh^T product and the cell update are inside the chain.  Each step is one launch: the dependent-kernel
// boundary (~1.5 us) is priced below a grid-wide barrier of a persistent launch (~4-5 us at 256 workgroups), and a launch
// needs no spin, so a step can never hang the device.  DESIGN.md section "The LSTM baseline" has the prices.
//
// Work split of one step: a workgroup of four waves owns 16 batch rows x 16 hidden units and ALL FOUR gates of those
// units, so the cell state c of a (row, unit) is read and written by the same thread in every step and only h_t leaves
// through memory.  The four waves split the reduction dimension in 32-wide chunks (round robin), and the partial 16x16
// tiles are summed in LDS in wave order: no atomics, bitwise reproducible.  The product is v_mfma_f32_16x16x32_{bf16,f16}
// on 16-bit data and v_mfma_f32_16x16x4_f32 (exact fp32) on fp32 data; gates, c and dc are fp32 in every mode.
#include "common.h"

namespace {

constexpr int kTile = 16;      // batch rows x hidden units per workgroup
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * DVT_WAVE;
constexpr int kChunk = 32;     // reduction elements per MFMA step of one wave

// acc += A(16 x 32) * B(32 x 16) for one 32-wide chunk; the lane holds A[l & 15][8 (l >> 4) + j] and B[8 (l >> 4) + j][l & 15].
// Any pairing of k between A and B is fine as long as it is the same on both sides (k is only summed over).
template <typename T> struct Frag;
template <> struct Frag<bf16> {
  bf16x8 v;
  __device__ __forceinline__ void load(const bf16* p, bool ok) {
    if (ok) v = *reinterpret_cast<const bf16x8*>(p);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (bf16)0.f;
    }
  }
};
template <> struct Frag<f16> {
  f16x8 v;
  __device__ __forceinline__ void load(const f16* p, bool ok) {
    if (ok) v = *reinterpret_cast<const f16x8*>(p);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (f16)0.f;
    }
  }
};
template <> struct Frag<float> {
  float v[8];
  __device__ __forceinline__ void load(const float* p, bool ok) {
    if (ok) load8<float>(p, v);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
    }
  }
};

__device__ __forceinline__ f32x4 mma(const Frag<bf16>& a, const Frag<bf16>& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma(const Frag<f16>& a, const Frag<f16>& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a.v, b.v, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma(const Frag<float>& a, const Frag<float>& b, f32x4 c) {
#pragma unroll
  for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], c, 0, 0, 0);
  return c;
}

// Step t of the forward chain.  G [B, T, 4H] = x W_ih^T (no bias); b_ih, b_hh [4H] f32 (nullable); whh [4H, H];
// hprev [B, T, H]: hprev[:, t] = h_{t-1} (the step reads it; it writes h_t to hprev[:, t + 1] and the zero h_{-1} at t = 0);
// hout [B, T, H] = h_t; gates [B, T, 4H] f32 post-activation (i, f, g, o); cst [B, T, H] f32 = c_t; hlast [B, H] (nullable).
template <typename T>
__global__ __launch_bounds__(kThreads) void lstm_step_fwd_kernel(
    const T* __restrict__ G, const float* __restrict__ b_ih, const float* __restrict__ b_hh, const T* __restrict__ whh,
    T* __restrict__ hprev, T* __restrict__ hout, float* __restrict__ gates, float* __restrict__ cst, T* __restrict__ hlast,
    int B, int Tn, int H, int t) {
  __shared__ float red[kWaves][4][kTile][kTile];
  const int wave = threadIdx.x / DVT_WAVE, lane = threadIdx.x % DVT_WAVE;
  const int u0 = blockIdx.x * kTile, r0 = blockIdx.y * kTile;
  f32x4 acc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (t > 0) {
    const int arow = r0 + (lane & 15);
    const bool arow_ok = arow < B;
    const T* ap = hprev + ((int64_t)arow * Tn + t) * H;
    for (int k0 = wave * kChunk + 8 * (lane >> 4); k0 - 8 * (lane >> 4) < H; k0 += kWaves * kChunk) {
      const bool kok = k0 < H;
      Frag<T> a;
      a.load(ap + k0, arow_ok && kok);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        Frag<T> b;
        b.load(whh + ((int64_t)g * H + u0 + (lane & 15)) * H + k0, kok);
        acc[g] = mma(a, b, acc[g]);
      }
    }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][g][(lane >> 4) * 4 + i][lane & 15] = acc[g][i];
  __syncthreads();

  const int rr = threadIdx.x / kTile, cc = threadIdx.x % kTile;
  const int row = r0 + rr, u = u0 + cc;
  if (row >= B) return;
  const int64_t rt = (int64_t)row * Tn + t;
  float s[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float v = red[0][g][rr][cc] + red[1][g][rr][cc] + red[2][g][rr][cc] + red[3][g][rr][cc];
    v += to_f32<T>(G[rt * 4 * H + g * H + u]);
    if (b_ih) v += b_ih[g * H + u];
    if (b_hh) v += b_hh[g * H + u];
    s[g] = v;
  }
  const float ig = sigmoidf_(s[0]), fg = sigmoidf_(s[1]), gg = tanhf(s[2]), og = sigmoidf_(s[3]);
  const float cprev = t > 0 ? cst[(rt - 1) * H + u] : 0.f;
  const float c = fg * cprev + ig * gg;
  const T h = from_f32<T>(og * tanhf(c));
  float* gp = gates + rt * 4 * H + u;
  gp[0] = ig;
  gp[H] = fg;
  gp[2 * H] = gg;
  gp[3 * H] = og;
  cst[rt * H + u] = c;
  hout[rt * H + u] = h;
  if (t == 0) hprev[rt * H + u] = from_f32<T>(0.f);
  if (t + 1 < Tn) hprev[(rt + 1) * H + u] = h;
  if (hlast && t == Tn - 1) hlast[(int64_t)row * H + u] = h;
}

// Step t of the backward chain (t = T-1 down to 0).  whhT [H, 4H] = W_hh^T; dG [B, T, 4H]: the step reads dG[:, t + 1]
// and writes dG[:, t] (the gradient of the pre-activation gates); dh_seq [B, T, H] the gradient arriving at h_t from above
// (nullable), dh_last [B, H] the one arriving at h_{T-1} (nullable); dc [B, H] f32 carries dL/dc_t between steps.
template <typename T>
__global__ __launch_bounds__(kThreads) void lstm_step_bwd_kernel(
    const T* __restrict__ whhT, const float* __restrict__ gates, const float* __restrict__ cst,
    const T* __restrict__ dh_seq, const T* __restrict__ dh_last, T* __restrict__ dG, float* __restrict__ dc,
    int B, int Tn, int H, int t) {
  __shared__ float red[kWaves][kTile][kTile];
  const int wave = threadIdx.x / DVT_WAVE, lane = threadIdx.x % DVT_WAVE;
  const int u0 = blockIdx.x * kTile, r0 = blockIdx.y * kTile;
  const int K = 4 * H;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  if (t + 1 < Tn) {
    const int arow = r0 + (lane & 15);
    const bool arow_ok = arow < B;
    const T* ap = dG + ((int64_t)arow * Tn + t + 1) * K;
    const T* bp = whhT + (int64_t)(u0 + (lane & 15)) * K;
    // K = 4H is a multiple of 64: every chunk is whole; two accumulators halve the dependent MFMA chain
    for (int k0 = wave * kChunk + 8 * (lane >> 4); k0 < K; k0 += 2 * kWaves * kChunk) {
      Frag<T> a, b;
      a.load(ap + k0, arow_ok);
      b.load(bp + k0, true);
      acc0 = mma(a, b, acc0);
      const int k1 = k0 + kWaves * kChunk;
      if (k1 < K) {
        a.load(ap + k1, arow_ok);
        b.load(bp + k1, true);
        acc1 = mma(a, b, acc1);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wave][(lane >> 4) * 4 + i][lane & 15] = acc0[i] + acc1[i];
  __syncthreads();

  const int rr = threadIdx.x / kTile, cc = threadIdx.x % kTile;
  const int row = r0 + rr, u = u0 + cc;
  if (row >= B) return;
  const int64_t rt = (int64_t)row * Tn + t;
  float dh = red[0][rr][cc] + red[1][rr][cc] + red[2][rr][cc] + red[3][rr][cc];
  if (dh_seq) dh += to_f32<T>(dh_seq[rt * H + u]);
  if (dh_last && t == Tn - 1) dh += to_f32<T>(dh_last[(int64_t)row * H + u]);
  const float* gp = gates + rt * 4 * H + u;
  const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
  const float c = cst[rt * H + u];
  const float cprev = t > 0 ? cst[(rt - 1) * H + u] : 0.f;
  const float tc = tanhf(c);
  float* dcp = dc + (int64_t)row * H + u;
  const float dcv = (t + 1 < Tn ? *dcp : 0.f) + dh * og * (1.f - tc * tc);
  *dcp = dcv * fg;
  T* dp = dG + rt * 4 * H + u;
  dp[0] = from_f32<T>(dcv * gg * ig * (1.f - ig));
  dp[H] = from_f32<T>(dcv * cprev * fg * (1.f - fg));
  dp[2 * H] = from_f32<T>(dcv * ig * (1.f - gg * gg));
  dp[3 * H] = from_f32<T>(dh * tc * og * (1.f - og));
}

// dst [C, R] = src [R, C]^T through a 32x32 LDS tile.
template <typename T>
__global__ __launch_bounds__(256) void transpose_kernel(const T* __restrict__ src, T* __restrict__ dst, int R, int Cc) {
  __shared__ T tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int tx = threadIdx.x % 32, ty = threadIdx.x / 32;
  for (int i = ty; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + tx;
    if (r < R && c < Cc) tile[i][tx] = src[(int64_t)r * Cc + c];
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + tx;
    if (r < R && c < Cc) dst[(int64_t)c * R + r] = tile[tx][i];
  }
}

int lstm_check(const char* fn, int64_t B, int64_t T, int64_t H, int dtype) {
  DVT_REQUIRE(B > 0 && T > 0 && H > 0, "%s: B, T, H must be positive (got %lld, %lld, %lld)", fn, (long long)B,
              (long long)T, (long long)H);
  if (dtype != DVT_F32 && dtype != DVT_BF16 && dtype != DVT_F16) DVT_UNSUPPORTED("%s: dtype %d not supported", fn, dtype);
  if (H % kTile != 0) DVT_UNSUPPORTED("%s: hidden size %lld is not a multiple of %d", fn, (long long)H, kTile);
  if (H > (1 << 20) || B > (int64_t)kTile * 65535 || T > (1 << 30))
    DVT_UNSUPPORTED("%s: B=%lld T=%lld H=%lld outside the kernel's index range", fn, (long long)B, (long long)T,
                    (long long)H);
  return DVT_OK;
}

}  // namespace

size_t dvt_lstm_seq_bwd_workspace_bytes(int64_t B, int64_t H, int dtype) {
  if (B <= 0 || H <= 0) return 0;
  const size_t wt = (size_t)(4 * H * H) * dvt_dtype_size(dtype);
  return (wt + 255) / 256 * 256 + (size_t)(B * H) * sizeof(float);
}

int dvt_lstm_seq_fwd(const void* G, const float* b_ih, const float* b_hh, const void* w_hh, void* h_prev, void* h_out,
                     float* gates, float* c, void* h_last, int64_t B, int64_t T, int64_t H, int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(G && w_hh && h_prev && h_out && gates && c, "dvt_lstm_seq_fwd: null pointer");
  const int rc = lstm_check("dvt_lstm_seq_fwd", B, T, H, dtype);
  if (rc != DVT_OK) return rc;
  DVT_REQUIRE(dvt_aligned16(G) && dvt_aligned16(w_hh) && dvt_aligned16(h_prev), "dvt_lstm_seq_fwd: misaligned buffer");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(H / kTile), (unsigned)dvt_cdiv(B, kTile));
  DVT_DISPATCH_DTYPE(dtype, Tt, {
    for (int64_t t = 0; t < T; ++t) {
      hipLaunchKernelGGL((lstm_step_fwd_kernel<Tt>), grid, dim3(kThreads), 0, st, (const Tt*)G, b_ih, b_hh,
                         (const Tt*)w_hh, (Tt*)h_prev, (Tt*)h_out, gates, c, (Tt*)h_last, (int)B, (int)T, (int)H, (int)t);
      DVT_LAUNCH_CHECK("dvt_lstm_seq_fwd");
    }
  });
  return DVT_OK;
}

int dvt_lstm_seq_bwd(const void* w_hh, const float* gates, const float* c, const void* dh_seq, const void* dh_last,
                     void* dG, void* workspace, int64_t B, int64_t T, int64_t H, int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(w_hh && gates && c && dG && workspace, "dvt_lstm_seq_bwd: null pointer");
  DVT_REQUIRE(dh_seq || dh_last, "dvt_lstm_seq_bwd: no incoming gradient (dh_seq and dh_last are both NULL)");
  const int rc = lstm_check("dvt_lstm_seq_bwd", B, T, H, dtype);
  if (rc != DVT_OK) return rc;
  DVT_REQUIRE(dvt_aligned16(w_hh) && dvt_aligned16(dG) && dvt_aligned16(workspace), "dvt_lstm_seq_bwd: misaligned buffer");
  hipStream_t st = (hipStream_t)stream;
  const size_t wt = (size_t)(4 * H * H) * dvt_dtype_size(dtype);
  float* dcbuf = reinterpret_cast<float*>(static_cast<char*>(workspace) + (wt + 255) / 256 * 256);
  const dim3 grid((unsigned)(H / kTile), (unsigned)dvt_cdiv(B, kTile));
  DVT_DISPATCH_DTYPE(dtype, Tt, {
    Tt* whhT = static_cast<Tt*>(workspace);
    hipLaunchKernelGGL((transpose_kernel<Tt>), dim3((unsigned)dvt_cdiv(H, 32), (unsigned)dvt_cdiv(4 * H, 32)), dim3(256),
                       0, st, (const Tt*)w_hh, whhT, (int)(4 * H), (int)H);
    DVT_LAUNCH_CHECK("dvt_lstm_seq_bwd (transpose)");
    for (int64_t t = T - 1; t >= 0; --t) {
      hipLaunchKernelGGL((lstm_step_bwd_kernel<Tt>), grid, dim3(kThreads), 0, st, (const Tt*)whhT, gates, c,
                         (const Tt*)dh_seq, (const Tt*)dh_last, (Tt*)dG, dcbuf, (int)B, (int)T, (int)H, (int)t);
      DVT_LAUNCH_CHECK("dvt_lstm_seq_bwd");
    }
  });
  return DVT_OK;
}
