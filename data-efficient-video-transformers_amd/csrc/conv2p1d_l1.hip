// conv2p1d_l1.hip -- inference kernels for layer 1 of R(2+1)D-18 (the four Conv2Plus1D pairs at 56 x 56): the spatial
// half 64 -> 144, (1,3,3) / 1 / (0,1,1), with the mid BatchNorm + ReLU folded, and the temporal half 144 -> 64,
// (3,1,1) / 1 / (1,0,0), with the block's BatchNorm, shortcut add and ReLU folded.  One launch per half.
//
// The same implicit GEMM as conv3d.hip (y[m, co] = sum_k gather(x)[m, k] * w[co, k], k = ((dt*kh + dh)*kw + dw)*C + c,
// weights packed by dvt_conv3d_weight_pack, epilogue y = relu?(acc * scale + shift + residual)), with the geometry a
// compile-time constant:
//   * spatial: one 128 x 144 output tile per workgroup -- all 144 mid channels at once, so every gathered input row feeds
//     nine MFMA columns (the general kernel splits 144 into a 128-wide and a 16-wide tile and gathers the input twice);
//   * temporal: a 128 x 64 tile with the 144-channel tap walk unrolled at compile time (no division, no carry loop);
//   * k-tiles of 32, two LDS stages, one barrier per k-tile; v_mfma_f32_16x16x32_{bf16,f16} only (one MFMA shape on
//     every accumulator);
//   * every operand byte comes through buffer_load_dwordx4 from descriptors sized to the two buffers: padded taps, rows
//     past M and k columns past the filter read zeros.  No atomics: two identical calls are bitwise equal.
// This translation unit instantiates none of the training kernels' templates.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTM = 128;
constexpr int kTK = 32;
constexpr unsigned kOOB = 0x80000000u;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

struct L1Params {
  const void* x;
  const void* w;
  void* y;
  const float* scale;
  const float* shift;
  const void* res;
  int T, H, W, M, relu;
  unsigned xbytes, wbytes;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}

template <typename T> __device__ __forceinline__ f32x4 mma(u32x4 a, u32x4 b, f32x4 c);
template <> __device__ __forceinline__ f32x4 mma<bf16>(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4 mma<f16>(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// C input channels, COUT output channels, a KT x KH x KW filter, stride 1, padding (KT/2, KH/2, KW/2)
template <int C, int COUT, int KT, int KH, int KW>
struct Geo {
  static constexpr int K = KT * KH * KW * C;
  static constexpr int LD = (K + kTK - 1) / kTK * kTK;
  static constexpr int NK = LD / kTK;
  static constexpr int PT = KT / 2, PH = KH / 2, PW = KW / 2;
};

template <typename T, int C, int COUT, int KT, int KH, int KW>
__global__ __launch_bounds__(kThreads) void conv2p1d_l1_kernel(L1Params p) {
  using G = Geo<C, COUT, KT, KH, KW>;
  constexpr int EPC = 8;                      // 16-bit elements per 16-byte chunk
  constexpr int CPR = kTK / EPC;              // 4 chunks per k-tile row
  constexpr int RPP = kThreads / CPR;         // 64 rows per pass
  constexpr int AJ = kTM / RPP;               // 2
  constexpr int BJ = (COUT + RPP - 1) / RPP;  // 3 (144) / 1 (64)
  constexpr int RS = kTK + EPC;               // LDS row stride: 80 bytes
  constexpr int FM = kTM / 4 / 16;            // 4 waves along M: 32 rows each
  constexpr int FN = COUT / 16;               // every output channel in the wave
  static_assert(C % EPC == 0 && COUT % 16 == 0, "geometry");
  __shared__ __attribute__((aligned(16))) T As[2][kTM * RS];
  __shared__ __attribute__((aligned(16))) T Bs[2][COUT * RS];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int m0 = (int)blockIdx.x * kTM;
  const int q = tid % CPR, rr = tid / CPR;
  const __amdgpu_buffer_rsrc_t xr = buf_rsrc(p.x, p.xbytes), wr = buf_rsrc(p.w, p.wbytes);
  const int HW = p.H * p.W;

  int rbase[AJ], rt[AJ], rh[AJ], rw[AJ];
#pragma unroll
  for (int j = 0; j < AJ; ++j) {
    const int m = m0 + rr + j * RPP;
    if (m < p.M) {
      const int f = m / HW;                   // frame (n, t) in order
      const int pix = m - f * HW;
      const int ho = pix / p.W;
      const int t = f % p.T;
      rbase[j] = (f - t) * HW;                // first pixel of the clip
      rt[j] = t - G::PT;
      rh[j] = ho - G::PH;
      rw[j] = pix - ho * p.W - G::PW;
    } else {
      rbase[j] = 0;
      rt[j] = -(1 << 24);
      rh[j] = rw[j] = 0;
    }
  }
  unsigned boff[BJ];
#pragma unroll
  for (int j = 0; j < BJ; ++j) {
    const int co = rr + j * RPP;
    boff[j] = co < COUT ? (unsigned)co * (unsigned)(G::LD * 2) : kOOB;
  }

  u32x4 ra[AJ], rb[BJ];
  auto gload = [&](int kt) {
    const int kcol = kt * kTK + q * EPC;
    const int tap = kcol / C;                 // compile-time divisor
    const int c = kcol - tap * C;
    const int dt = tap / (KH * KW), dh = (tap / KW) % KH, dw = tap % KW;
    const bool tap_ok = tap < KT * KH * KW;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int ti = rt[j] + dt, hi = rh[j] + dh, wi = rw[j] + dw;
      const bool ok = tap_ok && (unsigned)ti < (unsigned)p.T && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
      const unsigned off = ok ? ((unsigned)(rbase[j] + (ti * p.H + hi) * p.W + wi) * (unsigned)C + (unsigned)c) * 2u : kOOB;
      ra[j] = __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0);
    }
    const unsigned kb = (unsigned)kcol * 2u;
#pragma unroll
    for (int j = 0; j < BJ; ++j) rb[j] = __builtin_amdgcn_raw_buffer_load_b128(wr, boff[j] + kb, 0, 0);
  };
  auto lstore = [&](int s) {
#pragma unroll
    for (int j = 0; j < AJ; ++j) *reinterpret_cast<u32x4*>(&As[s][(rr + j * RPP) * RS + q * EPC]) = ra[j];
#pragma unroll
    for (int j = 0; j < BJ; ++j)
      if (rr + j * RPP < COUT) *reinterpret_cast<u32x4*>(&Bs[s][(rr + j * RPP) * RS + q * EPC]) = rb[j];
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fk = 8 * (lane >> 4);
  gload(0);
  lstore(0);
  __syncthreads();
  for (int kt = 0; kt < G::NK; ++kt) {
    const int s = kt & 1;
    const bool more = kt + 1 < G::NK;
    if (more) gload(kt + 1);
    u32x4 a[FM];
#pragma unroll
    for (int i = 0; i < FM; ++i) a[i] = *reinterpret_cast<const u32x4*>(&As[s][(wid * FM * 16 + i * 16 + frow) * RS + fk]);
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const u32x4 b = *reinterpret_cast<const u32x4*>(&Bs[s][(j * 16 + frow) * RS + fk]);
#pragma unroll
      for (int i = 0; i < FM; ++i) acc[i][j] = mma<T>(a[i], b, acc[i][j]);
    }
    if (more) lstore(s ^ 1);
    __syncthreads();
  }

  // accumulator (i, j)[e] = y[row 4 (l >> 4) + e, column l & 15] of the wave's 16 x 16 block (i, j)
  const T* res = static_cast<const T*>(p.res);
  T* y = static_cast<T*>(p.y);
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int col = j * 16 + (lane & 15);
    const float sc = p.scale ? p.scale[col] : 1.f, sh = p.shift ? p.shift[col] : 0.f;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = m0 + wid * FM * 16 + i * 16 + 4 * (lane >> 4) + e;
        if (row >= p.M) continue;
        const int64_t idx = (int64_t)row * COUT + col;
        float v = acc[i][j][e] * sc + sh;
        if (res) v += to_f32<T>(res[idx]);
        y[idx] = from_f32<T>(p.relu ? fmaxf(v, 0.f) : v);
      }
  }
}

enum Kind { kNone = 0, kSpatial = 1, kTemporal = 2 };

// which of the two layer-1 halves the descriptor is (kNone: neither, or outside the 32-bit buffer offsets)
Kind classify(const dvt_conv3d_desc* d) {
  if (!d || (d->dtype != DVT_BF16 && d->dtype != DVT_F16)) return kNone;
  if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0) return kNone;
  if (d->st != 1 || d->sh != 1 || d->sw != 1) return kNone;
  Kind k = kNone;
  if (d->C == 64 && d->Cout == 144 && d->kt == 1 && d->kh == 3 && d->kw == 3 && d->pt == 0 && d->ph == 1 && d->pw == 1)
    k = kSpatial;
  else if (d->C == 144 && d->Cout == 64 && d->kt == 3 && d->kh == 1 && d->kw == 1 && d->pt == 1 && d->ph == 0 && d->pw == 0)
    k = kTemporal;
  if (k == kNone) return kNone;
  const int64_t M = d->N * d->T * d->H * d->W;
  if (M * (int64_t)d->C * 2 >= (int64_t)kOOB || M * (int64_t)d->Cout >= ((int64_t)1 << 31)) return kNone;
  return k;
}

template <typename T, int C, int COUT, int KT, int KH, int KW>
int launch(const dvt_conv3d_desc* d, hipStream_t st) {
  using G = Geo<C, COUT, KT, KH, KW>;
  L1Params p{};
  p.x = d->x;
  p.w = d->w;
  p.y = d->y;
  p.scale = d->scale;
  p.shift = d->shift;
  p.res = d->residual;
  p.T = d->T; p.H = d->H; p.W = d->W;
  p.M = (int)(d->N * d->T * d->H * d->W);
  p.relu = d->relu;
  p.xbytes = (unsigned)((int64_t)p.M * C * 2);
  p.wbytes = (unsigned)(COUT * G::LD * 2);
  hipLaunchKernelGGL((conv2p1d_l1_kernel<T, C, COUT, KT, KH, KW>), dim3((unsigned)dvt_cdiv(p.M, kTM)), dim3(kThreads), 0, st,
                     p);
  DVT_LAUNCH_CHECK("dvt_conv2p1d_l1");
  return DVT_OK;
}

}  // namespace

extern "C" {

int dvt_conv2p1d_l1_supported(const dvt_conv3d_desc* desc) { return classify(desc) != kNone; }

int dvt_conv2p1d_l1(const dvt_conv3d_desc* d, dvt_stream_t stream) {
  const Kind k = classify(d);
  if (k == kNone)
    DVT_UNSUPPORTED("dvt_conv2p1d_l1: not a layer-1 half of R(2+1)D-18 in bf16 / fp16 (64 -> 144 (1,3,3) or 144 -> 64 "
                    "(3,1,1), stride 1), or the map is too large");
  DVT_REQUIRE(d->x && d->w && d->y, "dvt_conv2p1d_l1: null x / w / y");
  DVT_REQUIRE(dvt_aligned16(d->x) && dvt_aligned16(d->w), "dvt_conv2p1d_l1: x and w must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == DVT_BF16)
    return k == kSpatial ? launch<bf16, 64, 144, 1, 3, 3>(d, st) : launch<bf16, 144, 64, 3, 1, 1>(d, st);
  return k == kSpatial ? launch<f16, 64, 144, 1, 3, 3>(d, st) : launch<f16, 144, 64, 3, 1, 1>(d, st);
}

}  // extern "C"
