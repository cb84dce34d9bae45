// conv3d.hip -- full 3-D convolution forward as an implicit GEMM on MFMA (torchvision r3d_18: Conv3DSimple, BasicStem,
// the 1x1x1 strided downsamples), for inference.  The R(2+1)D path never needs it: its (1,k,k) and (3,1,1) halves map onto
// the 2-D kernels.  This translation unit leaves those kernels' templates alone.
//
//   y[m, co] = sum_k gather(x)[m, k] * w[co, k],   m = ((n * To + to) * Ho + ho) * Wo + wo,   k = ((dt * kh + dh) * kw + dw) * C + c
//
// x NDHWC [N*T*H*W, C] (C = the packed channel count, a multiple of 8: the stem's 3 planes arrive zero-extended to 8),
// w [Cout][ld] with ld = kt*kh*kw*C rounded up to the k-tile (zero columns beyond), y [M, Cout].
//
// Workgroup: 4 waves, a 128-row output tile x TN columns (TN = 64 for Cout <= 64 and for fp32, else 128), k-tiles of 32.
//   * every operand byte is read with buffer_load_dwordx4 from a descriptor built from kernel arguments: a padded tap, a row
//     past M or a column past Cout gets an offset beyond num_records and reads zeros -- no branch around the load, and no
//     access outside the two buffers is possible whatever the geometry;
//   * each thread owns one 16-byte column chunk of the k-tile and AJ / BJ rows of it; the chunk's filter tap (dt, dh, dw, c)
//     is carried from k-tile to k-tile by adding 32 to c (no division in the loop), and the per-row source coordinates
//     (clip, first t / h / w of the window) are computed once;
//   * two LDS stages, rows padded by 16 bytes (row strides of 80 / 144 bytes keep the 16 ds_read_b128 of a lane group on
//     16 distinct bank slots); the next k-tile is loaded into registers while the MFMAs of the current one run, one barrier
//     per k-tile;
//   * MFMA v_mfma_f32_16x16x32_{bf16,f16}, or eight exact v_mfma_f32_16x16x4_f32 per 32-wide k-step on fp32 data (the
//     fragment layout of lstm.hip);
//   * epilogue on the fp32 accumulators: y = relu?(acc * scale[co] + shift[co] + residual[m, co]) -- the eval-mode
//     BatchNorm folded to a per-channel affine (dvt_bn_fold), the block's shortcut, the ReLU -- then one rounding;
//   * few output tiles x deep K (layers 3-4 at one clip): the k-tiles are split over blockIdx.z, each slice writes its raw
//     sums to an fp32 slab, and a second launch sums the slabs in slice order and applies the epilogue.  No atomics
//     anywhere: two identical calls give bitwise-equal results.
#include "common.h"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr int kTM = 128;
constexpr int kTK = 32;
constexpr unsigned kOOB = 0x80000000u;        // buffer offset past every num_records this file accepts (< 2^31): reads 0
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

struct Conv3dParams {
  const void* x;
  const void* w;
  void* y;
  float* slab;                 // split-K: [splits][M][Cout] fp32, else nullptr
  const float* scale;
  const float* shift;
  const void* res;
  int T, H, W, C, To, Ho, Wo, Cout;
  int kt, kh, kw, st, sh, sw, pt, ph, pw;
  int M, ld, nk, kps, relu, tiles_n;
  unsigned xbytes, wbytes;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}

template <typename T> struct Mma;
template <> struct Mma<bf16> {
  static constexpr int kSteps = 1;
  static __device__ __forceinline__ f32x4 run(const u32x4 (&a)[2], const u32x4 (&b)[2], f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[0]), __builtin_bit_cast(bf16x8, b[0]), c, 0,
                                                   0, 0);
  }
};
template <> struct Mma<f16> {
  static constexpr int kSteps = 1;
  static __device__ __forceinline__ f32x4 run(const u32x4 (&a)[2], const u32x4 (&b)[2], f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a[0]), __builtin_bit_cast(f16x8, b[0]), c, 0, 0,
                                                  0);
  }
};
template <> struct Mma<float> {
  static constexpr int kSteps = 2;
  static __device__ __forceinline__ f32x4 run(const u32x4 (&a)[2], const u32x4 (&b)[2], f32x4 c) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // element by value first: __builtin_bit_cast of a vector-element lvalue reads element 0 with this compiler
        const unsigned ua = a[h][j], ub = b[h][j];
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua), __uint_as_float(ub), c, 0, 0, 0);
      }
    return c;
  }
};

template <typename T>
__device__ __forceinline__ float finish(float v, int64_t idx, int col, const float* __restrict__ scale,
                                        const float* __restrict__ shift, const T* __restrict__ res, int relu) {
  if (scale) v *= scale[col];
  if (shift) v += shift[col];
  if (res) v += to_f32<T>(res[idx]);
  return relu ? fmaxf(v, 0.f) : v;
}

template <typename T, int TN>
__global__ __launch_bounds__(kThreads) void conv3d_implicit_kernel(Conv3dParams p) {
  constexpr int EPC = 16 / (int)sizeof(T);     // elements per 16-byte chunk
  constexpr int CPR = kTK / EPC;               // chunks per k-tile row
  constexpr int RPP = kThreads / CPR;          // rows per pass of the workgroup
  constexpr int AJ = kTM / RPP, BJ = TN / RPP;
  constexpr int RS = kTK + EPC;                // LDS row stride (elements): 80 / 144 bytes
  constexpr int WGM = TN == 64 ? 4 : 2;        // wave grid over the tile
  constexpr int FM = kTM / WGM / 16, FN = TN / (4 / WGM) / 16;
  static_assert(AJ >= 1 && BJ >= 1 && FM >= 1 && FN >= 1, "tile shape");
  __shared__ __attribute__((aligned(16))) T As[2][kTM * RS];
  __shared__ __attribute__((aligned(16))) T Bs[2][TN * RS];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int tn = (int)(blockIdx.x % (unsigned)p.tiles_n), tm = (int)(blockIdx.x / (unsigned)p.tiles_n);
  const int m0 = tm * kTM, n0 = tn * TN;
  const int q = tid % CPR, rr = tid / CPR;
  const int kt_beg = (int)blockIdx.z * p.kps;
  const int kt_end = min(p.nk, kt_beg + p.kps);

  const __amdgpu_buffer_rsrc_t xr = buf_rsrc(p.x, p.xbytes), wr = buf_rsrc(p.w, p.wbytes);

  // source coordinates of the thread's gather rows: first input pixel of the clip, window origin in t / h / w
  int rbase[AJ], rt[AJ], rh[AJ], rw[AJ];
#pragma unroll
  for (int j = 0; j < AJ; ++j) {
    const int m = m0 + rr + j * RPP;
    if (m < p.M) {
      int t = m / p.Wo;
      const int wo = m - t * p.Wo;
      int u = t / p.Ho;
      const int ho = t - u * p.Ho;
      const int n = u / p.To;
      const int to = u - n * p.To;
      rbase[j] = n * p.T * p.H * p.W;
      rt[j] = to * p.st - p.pt;
      rh[j] = ho * p.sh - p.ph;
      rw[j] = wo * p.sw - p.pw;
    } else {
      rbase[j] = 0;
      rt[j] = -(1 << 24);                      // every tap out of range: the row reads zeros
      rh[j] = rw[j] = 0;
    }
  }
  unsigned boff[BJ];
#pragma unroll
  for (int j = 0; j < BJ; ++j) {
    const int co = n0 + rr + j * RPP;
    boff[j] = co < p.Cout ? (unsigned)co * (unsigned)p.ld * (unsigned)sizeof(T) : kOOB;
  }
  // the chunk's filter tap, carried across k-tiles
  int kcol = kt_beg * kTK + q * EPC;
  int tap = kcol / p.C;
  int c = kcol - tap * p.C;
  const int khw = p.kh * p.kw;
  int dt = tap / khw;
  tap -= dt * khw;
  int dh = tap / p.kw;
  int dw = tap - dh * p.kw;

  u32x4 ra[AJ], rb[BJ];
  auto gload = [&]() {
    const bool tap_ok = dt < p.kt;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
      const int ti = rt[j] + dt, hi = rh[j] + dh, wi = rw[j] + dw;
      const bool ok = tap_ok && (unsigned)ti < (unsigned)p.T && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
      const unsigned off = ok ? (unsigned)(((rbase[j] + (ti * p.H + hi) * p.W + wi) * p.C + c) * (int)sizeof(T)) : kOOB;
      ra[j] = __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0);
    }
    const unsigned kb = (unsigned)kcol * (unsigned)sizeof(T);
#pragma unroll
    for (int j = 0; j < BJ; ++j) rb[j] = __builtin_amdgcn_raw_buffer_load_b128(wr, boff[j] + kb, 0, 0);
    kcol += kTK;
    c += kTK;
    while (c >= p.C) {
      c -= p.C;
      if (++dw == p.kw) {
        dw = 0;
        if (++dh == p.kh) { dh = 0; ++dt; }
      }
    }
  };
  auto lstore = [&](int s) {
#pragma unroll
    for (int j = 0; j < AJ; ++j) *reinterpret_cast<u32x4*>(&As[s][(rr + j * RPP) * RS + q * EPC]) = ra[j];
#pragma unroll
    for (int j = 0; j < BJ; ++j) *reinterpret_cast<u32x4*>(&Bs[s][(rr + j * RPP) * RS + q * EPC]) = rb[j];
  };

  const int wm = wid % WGM, wn = wid / WGM;
  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fk = 8 * (lane >> 4);   // fragment: row (l & 15), k 8 (l >> 4) .. + 7 of the 32-wide step
  if (kt_beg < kt_end) {
    gload();
    lstore(0);
    __syncthreads();
    for (int kt = kt_beg; kt < kt_end; ++kt) {
      const int s = (kt - kt_beg) & 1;
      const bool more = kt + 1 < kt_end;
      if (more) gload();
      u32x4 a[FM][2], b[FN][2];
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const T* src = &As[s][(wm * FM * 16 + i * 16 + frow) * RS + fk];
#pragma unroll
        for (int h = 0; h < Mma<T>::kSteps; ++h) a[i][h] = reinterpret_cast<const u32x4*>(src)[h];
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const T* src = &Bs[s][(wn * FN * 16 + j * 16 + frow) * RS + fk];
#pragma unroll
        for (int h = 0; h < Mma<T>::kSteps; ++h) b[j][h] = reinterpret_cast<const u32x4*>(src)[h];
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = Mma<T>::run(a[i], b[j], acc[i][j]);
      if (more) lstore(s ^ 1);
      __syncthreads();
    }
  }

  // accumulator (i, j)[e] = y[row 4 (l >> 4) + e, column l & 15] of the wave's 16 x 16 block (i, j)
  const T* res = static_cast<const T*>(p.res);
  T* y = static_cast<T*>(p.y);
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int col = n0 + wn * FN * 16 + j * 16 + (lane & 15);
      if (col >= p.Cout) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = m0 + wm * FM * 16 + i * 16 + 4 * (lane >> 4) + e;
        if (row >= p.M) continue;
        const int64_t idx = (int64_t)row * p.Cout + col;
        if (p.slab) p.slab[(int64_t)blockIdx.z * p.M * p.Cout + idx] = acc[i][j][e];
        else y[idx] = from_f32<T>(finish<T>(acc[i][j][e], idx, col, p.scale, p.shift, res, p.relu));
      }
    }
}

// y = epilogue(sum over the slices, in slice order, of the fp32 slabs)
template <typename T>
__global__ __launch_bounds__(256) void conv3d_splitk_reduce_kernel(const float* __restrict__ slab, int splits, int64_t MN,
                                                                  int Cout, const float* __restrict__ scale,
                                                                  const float* __restrict__ shift, const T* __restrict__ res,
                                                                  int relu, T* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < MN; i += (int64_t)gridDim.x * 256) {
    float v = 0.f;
    for (int z = 0; z < splits; ++z) v += slab[(int64_t)z * MN + i];
    y[i] = from_f32<T>(finish<T>(v, i, (int)(i % Cout), scale, shift, res, relu));
  }
}

// dst[co][k] (k = tap * Cp + c, tap = (dt * kh + dh) * kw + dw) = w[co][c][dt][dh][dw] for c < Cin, tap < taps; 0 elsewhere
template <typename T>
__global__ __launch_bounds__(256) void conv3d_weight_pack_kernel(const float* __restrict__ w, T* __restrict__ dst, int Cout,
                                                                int Cin, int taps, int Cp, int64_t ld) {
  const int64_t n = (int64_t)Cout * ld;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int co = (int)(i / ld);
    const int k = (int)(i - (int64_t)co * ld);
    const int tap = k / Cp, c = k - tap * Cp;
    const float v = tap < taps && c < Cin ? w[((int64_t)co * Cin + c) * taps + tap] : 0.f;
    dst[i] = from_f32<T>(v);
  }
}

// eval-mode BatchNorm as an affine: scale = gamma / sqrt(var + eps), shift = beta - mean * scale
__global__ __launch_bounds__(256) void bn_fold_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                      float* __restrict__ scale, float* __restrict__ shift, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C) return;
  const float s = (gamma ? gamma[i] : 1.f) / sqrtf(var[i] + eps);
  scale[i] = s;
  shift[i] = (beta ? beta[i] : 0.f) - mean[i] * s;
}

struct Geom {
  int64_t To, Ho, Wo, M, K, ld, xbytes, wbytes;
  int TN, tiles_n, tiles, nk, split, kps;
};

// shape checks and the launch plan, shared by every entry point (the workspace query and the launch agree by construction)
int conv3d_plan(const dvt_conv3d_desc* d, Geom& g) {
  DVT_REQUIRE(d != nullptr, "dvt_conv3d_implicit: null descriptor");
  DVT_REQUIRE(d->N > 0 && d->T > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->Cout > 0,
              "dvt_conv3d_implicit: N, T, H, W, C, Cout must be positive");
  DVT_REQUIRE(d->kt > 0 && d->kh > 0 && d->kw > 0 && d->st > 0 && d->sh > 0 && d->sw > 0,
              "dvt_conv3d_implicit: kernel sizes and strides must be positive");
  DVT_REQUIRE(d->pt >= 0 && d->ph >= 0 && d->pw >= 0, "dvt_conv3d_implicit: negative padding");
  if (d->dtype != DVT_F32 && d->dtype != DVT_BF16 && d->dtype != DVT_F16)
    DVT_UNSUPPORTED("dvt_conv3d_implicit: dtype %d not supported", (int)d->dtype);
  if (d->C % 8 != 0)
    DVT_UNSUPPORTED("dvt_conv3d_implicit: C = %d is not a multiple of 8 (zero-extend the channels, dvt_conv3d_weight_pack)",
                    (int)d->C);
  if (d->kt > 64 || d->kh > 64 || d->kw > 64 || d->pt >= d->kt || d->ph >= d->kh || d->pw >= d->kw)
    DVT_UNSUPPORTED("dvt_conv3d_implicit: kernel (%d, %d, %d) / padding (%d, %d, %d) outside the supported range", d->kt,
                    d->kh, d->kw, d->pt, d->ph, d->pw);
  g.To = ((int64_t)d->T + 2 * d->pt - d->kt) / d->st + 1;
  g.Ho = ((int64_t)d->H + 2 * d->ph - d->kh) / d->sh + 1;
  g.Wo = ((int64_t)d->W + 2 * d->pw - d->kw) / d->sw + 1;
  DVT_REQUIRE(d->T + 2 * d->pt >= d->kt && d->H + 2 * d->ph >= d->kh && d->W + 2 * d->pw >= d->kw,
              "dvt_conv3d_implicit: the window is larger than the padded input");
  const size_t es = dvt_dtype_size(d->dtype);
  g.M = d->N * g.To * g.Ho * g.Wo;
  g.K = (int64_t)d->kt * d->kh * d->kw * d->C;
  g.ld = dvt_cdiv(g.K, kTK) * kTK;
  g.xbytes = d->N * d->T * d->H * d->W * d->C * (int64_t)es;
  g.wbytes = (int64_t)d->Cout * g.ld * (int64_t)es;
  // 32-bit buffer offsets: every byte offset (and kOOB + a k offset) stays below 2^32; y is indexed in 64 bits
  if (g.xbytes >= (int64_t)kOOB || g.wbytes >= (int64_t)kOOB || g.M >= (int64_t)1 << 31 || g.M * d->Cout >= (int64_t)1 << 40)
    DVT_UNSUPPORTED("dvt_conv3d_implicit: map of %lld bytes / weights of %lld bytes / %lld output rows: split the batch",
                    (long long)g.xbytes, (long long)g.wbytes, (long long)g.M);
  g.TN = (d->Cout <= 64 || d->dtype == DVT_F32) ? 64 : 128;
  g.tiles_n = (int)dvt_cdiv(d->Cout, g.TN);
  const int64_t tiles = dvt_cdiv(g.M, kTM) * g.tiles_n;
  if (tiles >= (int64_t)1 << 31) DVT_UNSUPPORTED("dvt_conv3d_implicit: %lld output tiles", (long long)tiles);
  g.tiles = (int)tiles;
  g.nk = (int)(g.ld / kTK);
  // split K when the tiles cannot fill the device twice over and every slice keeps >= 8 k-tiles
  const int64_t target = 2 * (int64_t)dvt_num_cus();
  int split = 1;
  if (tiles < target && g.nk >= 16) {
    split = (int)std::min<int64_t>(dvt_cdiv(target, tiles), std::min<int64_t>(g.nk / 8, 64));
    if (split < 2) split = 1;
  }
  g.kps = (int)dvt_cdiv(g.nk, split);
  g.split = (int)dvt_cdiv(g.nk, g.kps);
  return DVT_OK;
}

template <typename T, int TN>
int launch(const dvt_conv3d_desc* d, const Geom& g, hipStream_t st) {
  Conv3dParams p{};
  p.x = d->x;
  p.w = d->w;
  p.y = d->y;
  p.slab = g.split > 1 ? static_cast<float*>(d->workspace) : nullptr;
  p.scale = d->scale;
  p.shift = d->shift;
  p.res = d->residual;
  p.T = d->T; p.H = d->H; p.W = d->W; p.C = d->C;
  p.To = (int)g.To; p.Ho = (int)g.Ho; p.Wo = (int)g.Wo; p.Cout = d->Cout;
  p.kt = d->kt; p.kh = d->kh; p.kw = d->kw;
  p.st = d->st; p.sh = d->sh; p.sw = d->sw;
  p.pt = d->pt; p.ph = d->ph; p.pw = d->pw;
  p.M = (int)g.M; p.ld = (int)g.ld; p.nk = g.nk; p.kps = g.kps; p.relu = d->relu; p.tiles_n = g.tiles_n;
  p.xbytes = (unsigned)g.xbytes;
  p.wbytes = (unsigned)g.wbytes;
  hipLaunchKernelGGL((conv3d_implicit_kernel<T, TN>), dim3((unsigned)g.tiles, 1, (unsigned)g.split), dim3(kThreads), 0, st, p);
  DVT_LAUNCH_CHECK("dvt_conv3d_implicit");
  if (g.split > 1) {
    const int64_t MN = g.M * d->Cout;
    const unsigned blocks = (unsigned)std::min<int64_t>(dvt_cdiv(MN, 256), 4 * (int64_t)dvt_num_cus());
    hipLaunchKernelGGL((conv3d_splitk_reduce_kernel<T>), dim3(blocks), dim3(256), 0, st, (const float*)d->workspace, g.split,
                       MN, d->Cout, d->scale, d->shift, (const T*)d->residual, d->relu, (T*)d->y);
    DVT_LAUNCH_CHECK("dvt_conv3d_implicit (split-K reduce)");
  }
  return DVT_OK;
}

}  // namespace

int dvt_conv3d_implicit_supported(const dvt_conv3d_desc* desc) {
  Geom g;
  return conv3d_plan(desc, g) == DVT_OK ? 1 : 0;
}

int64_t dvt_conv3d_implicit_k(const dvt_conv3d_desc* desc) {
  Geom g;
  return conv3d_plan(desc, g) == DVT_OK ? g.ld : -1;
}

size_t dvt_conv3d_implicit_workspace_bytes(const dvt_conv3d_desc* desc) {
  Geom g;
  if (conv3d_plan(desc, g) != DVT_OK || g.split <= 1) return 0;
  return (size_t)g.split * (size_t)g.M * (size_t)desc->Cout * sizeof(float);
}

int dvt_conv3d_implicit(const dvt_conv3d_desc* d, dvt_stream_t stream) {
  Geom g;
  const int rc = conv3d_plan(d, g);
  if (rc != DVT_OK) return rc;
  DVT_REQUIRE(d->x && d->w && d->y, "dvt_conv3d_implicit: null x / w / y");
  DVT_REQUIRE(dvt_aligned16(d->x) && dvt_aligned16(d->w), "dvt_conv3d_implicit: x and w must be 16-byte aligned");
  DVT_REQUIRE(g.split <= 1 || (d->workspace && dvt_aligned16(d->workspace)),
              "dvt_conv3d_implicit: this geometry splits K and needs dvt_conv3d_implicit_workspace_bytes of workspace");
  hipStream_t st = (hipStream_t)stream;
  if (d->dtype == DVT_F32) return launch<float, 64>(d, g, st);
  if (d->dtype == DVT_BF16) return g.TN == 64 ? launch<bf16, 64>(d, g, st) : launch<bf16, 128>(d, g, st);
  return g.TN == 64 ? launch<f16, 64>(d, g, st) : launch<f16, 128>(d, g, st);
}

int dvt_conv3d_weight_pack(const float* w, void* dst, int dst_dtype, int Cout, int Cin, int kt, int kh, int kw, int Cp,
                           int64_t ld, dvt_stream_t stream) {
  DVT_REQUIRE(w && dst, "dvt_conv3d_weight_pack: null pointer");
  DVT_REQUIRE(Cout > 0 && Cin > 0 && kt > 0 && kh > 0 && kw > 0 && Cp >= Cin, "dvt_conv3d_weight_pack: bad shape");
  DVT_REQUIRE(ld >= (int64_t)kt * kh * kw * Cp && ld < ((int64_t)1 << 31), "dvt_conv3d_weight_pack: ld %lld too small",
              (long long)ld);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)Cout * ld;
  const unsigned blocks = (unsigned)std::min<int64_t>(dvt_cdiv(n, 256), 4096);
  DVT_DISPATCH_DTYPE(dst_dtype, T,
                     hipLaunchKernelGGL((conv3d_weight_pack_kernel<T>), dim3(blocks), dim3(256), 0, st, w, (T*)dst, Cout, Cin,
                                        kt * kh * kw, Cp, ld));
  DVT_LAUNCH_CHECK("dvt_conv3d_weight_pack");
  return DVT_OK;
}

int dvt_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                float* scale, float* shift, int C, dvt_stream_t stream) {
  DVT_REQUIRE(running_mean && running_var && scale && shift && C > 0, "dvt_bn_fold: null pointer or C <= 0");
  hipLaunchKernelGGL(bn_fold_kernel, dim3((unsigned)dvt_cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, gamma, beta,
                     running_mean, running_var, eps, scale, shift, C);
  DVT_LAUNCH_CHECK("dvt_bn_fold");
  return DVT_OK;
}
