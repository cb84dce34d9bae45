// audio.hip -- the VGGish audio expert's input side (the reference names the network at pretrained/models.py:13 and calls
// it at :55-57): waveform -> log-mel examples (dvt_logmel_examples) and the network's first layer,
// Conv2d(1, 64, 3, padding=1) + bias + ReLU + MaxPool2d(2, 2), as one direct kernel (dvt_vggish_conv1_pool).
//
// Front end, all fp32:  frames of kWin samples every kHop (no padding) -> periodic Hann -> |rfft_512| -> mel [257, 64] ->
// log(mel + kLogOffset) -> examples of kExFrames frames every kExHop.  The constants of the definition are in the block
// below; Python asks dvt_logmel_num_examples for the counts and repeats only the example's shape, 96 x 64, to size its output.
//
// One workgroup (4 waves) owns FPB consecutive frames of one example: it stages their waveform span in LDS once (consecutive
// frames overlap by 60 %), leaves the magnitudes of bins 0 .. kBinsUsed-1 in LDS (the mel matrix is zero from 7500 Hz = bin
// 240 up; dvt_logmel_tables checks that), and multiplies them with the mel matrix on v_mfma_f32_16x16x4_f32.  Two forms of
// the spectrum, chosen by `variant` (DESIGN 4.16 has both timed on the same run):
//   DVT_LOGMEL_DFT  the windowed DFT as a table product on v_mfma_f32_16x16x4_f32: [FPB = 48 frames] x [400 samples] times
//                   [400] x [240 cos | 240 sin], the window folded into the table; the table streams from L2 (768 KB);
//   DVT_LOGMEL_FFT  FPB = 16; each wave runs two 512-point radix-2 FFTs in LDS, each on a PAIR of frames packed as
//                   real + i imag, and separates the two spectra by conjugate symmetry.
// The k index of a 16x16x4 step is free as long as A and B agree, so the tables are laid out such that one 16-byte read per
// lane feeds four consecutive steps: lane (row / column n = l & 15, g = l >> 4) holds k = 16 kb + 4 g + j for step j.
// No atomics; every sum has a fixed order: identical calls give bitwise-equal results.
#include "common.h"

#include <cmath>
#include <vector>

namespace {

// ---------------------------------------------------------------- the definition (the issue's text is the contract)
constexpr int kWin = 400;                  // 25 ms at 16 kHz
constexpr int kHop = 160;                  // 10 ms
constexpr int kFft = 512;
constexpr int kBins = kFft / 2 + 1;        // 257
constexpr int kMel = 64;
constexpr double kSampleRate = 16000.0;
constexpr double kMelLoHz = 125.0, kMelHiHz = 7500.0;
constexpr double kMelBreakHz = 700.0, kMelQ = 1127.0;       // HTK: m(f) = 1127 ln(1 + f / 700)
constexpr float kLogOffset = 0.01f;
constexpr int kExFrames = 96, kExHop = 96;

// ---------------------------------------------------------------- kernel shapes
constexpr int kBinsUsed = 240;             // bins at and above this have zero mel weight
constexpr int kBinTiles = kBinsUsed / 16;  // 15
constexpr int kKB = kWin / 16;             // 25 k-blocks of 16 samples
constexpr int kMagLd = kBinsUsed + 4;      // LDS row of magnitudes (976 bytes: 16-byte aligned rows, odd count of 16-byte slots)
constexpr int kSpanPad = 4;                // floats inserted after every kHop samples of the staged span (row stride 164)
static_assert(kWin % 16 == 0 && kBinsUsed % 16 == 0 && kHop % 4 == 0 && kMel == 64 && kFft == 512, "kernel shapes");

// table image (floats): window | FFT twiddles | windowed DFT table | mel matrix
constexpr int kOffWin = 0;
constexpr int kOffTw = kOffWin + kWin;                          // 256 x (cos, -sin)
constexpr int kOffDft = kOffTw + kFft;                          // [kKB][2 kBinTiles][64 lanes][4]
constexpr int kOffMel = kOffDft + kKB * 2 * kBinTiles * 256;    // [kBinTiles][4][64 lanes][4]
constexpr int kTableFloats = kOffMel + kBinTiles * 4 * 256;
static_assert(kOffTw % 4 == 0 && kOffDft % 4 == 0 && kOffMel % 4 == 0, "16-byte aligned tables");

__host__ __device__ constexpr int span_len(int fpb) { return (fpb - 1) * kHop + kWin; }
__host__ __device__ constexpr int span_lds(int fpb) { return span_len(fpb) + (span_len(fpb) / kHop + 1) * kSpanPad; }
__device__ __forceinline__ int span_addr(int s) { return s + (s / kHop) * kSpanPad; }

__device__ __forceinline__ f32x4 mma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

template <int VARIANT> struct Shape;
template <> struct Shape<DVT_LOGMEL_DFT> {
  static constexpr int FPB = 48;
  static constexpr int kMag = 0;                                // the magnitudes take the span's place
  static constexpr int kFloats = FPB * kMagLd > span_lds(FPB) ? FPB * kMagLd : span_lds(FPB);
};
template <> struct Shape<DVT_LOGMEL_FFT> {
  static constexpr int FPB = 16;
  static constexpr int kBuf = (span_lds(FPB) + 3) / 4 * 4;      // 4 waves x 512 complex
  static constexpr int kTw = kBuf + 4 * 2 * kFft;
  static constexpr int kMag = kTw + kFft;
  static constexpr int kFloats = kMag + FPB * kMagLd;
};

template <typename T, int VARIANT>
__global__ __launch_bounds__(256) void logmel_kernel(const float* __restrict__ wave, int64_t L, int E,
                                                     const float* __restrict__ tab, T* __restrict__ out) {
  typedef Shape<VARIANT> S;
  constexpr int FPB = S::FPB, PARTS = kExFrames / FPB, MT = FPB / 16, SPAN = span_len(FPB);
  static_assert(kExFrames % FPB == 0 && FPB % 16 == 0, "frames per workgroup");
  __shared__ __attribute__((aligned(16))) float smem[S::kFloats];
  float* span = smem;
  float* mag = smem + S::kMag;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, n = lane & 15;
  const int part = (int)(blockIdx.x % PARTS);
  const int e = (int)((blockIdx.x / PARTS) % (unsigned)E);
  const int64_t r = blockIdx.x / ((unsigned)PARTS * (unsigned)E);
  const float* src = wave + r * L + ((int64_t)e * kExHop + part * FPB) * kHop;      // the last frame ends inside the row
  for (int s = tid; s < SPAN; s += 256) span[span_addr(s)] = src[s];

  if constexpr (VARIANT == DVT_LOGMEL_DFT) {
    __syncthreads();
    // wave `wid` owns the bin tiles wid, wid + 4, ..: cos and sin accumulators of one bin share a lane
    f32x4 acc[MT][4][2];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[mi][q][0] = acc[mi][q][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4* dft = reinterpret_cast<const f32x4*>(tab + kOffDft);
    f32x4 bcur[4][2], bnext[4][2];
    auto load_b = [&](int kb, f32x4(&b)[4][2]) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (wid + 4 * q < kBinTiles) {
#pragma unroll
          for (int p = 0; p < 2; ++p) b[q][p] = dft[(kb * 2 * kBinTiles + (wid + 4 * q) * 2 + p) * 64 + lane];
        }
    };
    load_b(0, bcur);
    for (int kb = 0; kb < kKB; ++kb) {
      if (kb + 1 < kKB) load_b(kb + 1, bnext);
      f32x4 a[MT];
#pragma unroll
      for (int mi = 0; mi < MT; ++mi)
        a[mi] = *reinterpret_cast<const f32x4*>(&span[span_addr((mi * 16 + n) * kHop + kb * 16 + 4 * g)]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (wid + 4 * q < kBinTiles) {
#pragma unroll
            for (int mi = 0; mi < MT; ++mi)
#pragma unroll
              for (int p = 0; p < 2; ++p) acc[mi][q][p] = mma4(a[mi][j], bcur[q][p][j], acc[mi][q][p]);
          }
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int p = 0; p < 2; ++p) bcur[q][p] = bnext[q][p];
    }
    __syncthreads();                       // every wave has read its last sample: the magnitudes overwrite the span
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (wid + 4 * q < kBinTiles) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float re = acc[mi][q][0][i], im = acc[mi][q][1][i];
            mag[(mi * 16 + 4 * g + i) * kMagLd + (wid + 4 * q) * 16 + n] = sqrtf(re * re + im * im);
          }
        }
  } else {
    typedef __attribute__((ext_vector_type(2))) float c32;
    c32* buf = reinterpret_cast<c32*>(smem + S::kBuf) + wid * kFft;
    c32* tw = reinterpret_cast<c32*>(smem + S::kTw);
    tw[tid] = reinterpret_cast<const c32*>(tab + kOffTw)[tid];
    const float* win = tab + kOffWin;
    __syncthreads();
    // the four waves run the same loops on buffers of their own: every barrier below is reached by all of them
#pragma unroll 1
    for (int pair = 0; pair < FPB / 8; ++pair) {
      const int fa = wid * (FPB / 4) + 2 * pair;                 // frames fa (real part) and fa + 1 (imaginary part)
#pragma unroll
      for (int q = 0; q < kFft / 64; ++q) {
        const int i = lane + 64 * q;
        c32 z = {0.f, 0.f};
        if (i < kWin) {
          const float w = win[i];
          z[0] = span[span_addr(fa * kHop + i)] * w;
          z[1] = span[span_addr((fa + 1) * kHop + i)] * w;
        }
        buf[__brev((unsigned)i) >> 23] = z;
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 9; ++s) {
        const int half = 1 << s;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int b = lane + 64 * q, j = b & (half - 1), i0 = ((b >> s) << (s + 1)) | j, i1 = i0 + half;
          const c32 w = tw[j << (8 - s)], u = buf[i0], v = buf[i1];
          const float tr = v[0] * w[0] - v[1] * w[1], ti = v[0] * w[1] + v[1] * w[0];
          buf[i0] = c32{u[0] + tr, u[1] + ti};
          buf[i1] = c32{u[0] - tr, u[1] - ti};
        }
        __syncthreads();
      }
      // Z = A + i B with A, B the spectra of two real frames: 2 A[k] = Z[k] + conj(Z[-k]), 2 i B[k] = Z[k] - conj(Z[-k])
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = lane + 64 * q;
        if (k < kBinsUsed) {
          const c32 z = buf[k], y = buf[(kFft - k) & (kFft - 1)];
          const float ar = z[0] + y[0], ai = z[1] - y[1], br = z[0] - y[0], bi = z[1] + y[1];
          mag[fa * kMagLd + k] = 0.5f * sqrtf(ar * ar + ai * ai);
          mag[(fa + 1) * kMagLd + k] = 0.5f * sqrtf(br * br + bi * bi);
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();

  // mel[frame][m] = sum over the bins of mag[frame][bin] * M[bin][m]: wave `wid` owns mel columns 16 wid .. + 15
  f32x4 macc[MT];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi) macc[mi] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4* mel = reinterpret_cast<const f32x4*>(tab + kOffMel);
#pragma unroll 3
  for (int kb = 0; kb < kBinTiles; ++kb) {
    const f32x4 b = mel[(kb * 4 + wid) * 64 + lane];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(&mag[(mi * 16 + n) * kMagLd + kb * 16 + 4 * g]);
#pragma unroll
      for (int j = 0; j < 4; ++j) macc[mi] = mma4(a[j], b[j], macc[mi]);
    }
  }
  // the logarithm in double, rounded once: the fp32 result is the correctly rounded one whatever the library's logf does
  T* dst = out + ((r * E + e) * kExFrames + part * FPB) * (int64_t)kMel;
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      dst[(mi * 16 + 4 * g + i) * kMel + wid * 16 + n] = from_f32<T>((float)log((double)(macc[mi][i] + kLogOffset)));
}

inline int64_t num_frames(int64_t L) { return L < kWin ? 0 : 1 + (L - kWin) / kHop; }
inline int64_t num_examples(int64_t L) {
  const int64_t F = num_frames(L);
  return F < kExFrames ? 0 : 1 + (F - kExFrames) / kExHop;
}

double hz_to_mel(double f) { return kMelQ * std::log(1.0 + f / kMelBreakHz); }

// ---------------------------------------------------------------- Conv2d(1, 64, 3, p 1) + bias + ReLU + MaxPool2d(2, 2)
// One workgroup per pooled row: 4 input rows (zero halo) and the 64 x 9 weights in LDS; thread (pooled column, 8 channels)
// evaluates its 2 x 2 window and stores 8 channels at once.  max(relu(z + b)) = relu(max z + b): adding b and rounding are
// monotone, so the bias, the ReLU and the one rounding come after the maximum.
constexpr int kC1 = 64, kC1W = 64;
template <typename T>
__global__ __launch_bounds__(256) void vggish_conv1_pool_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, T* __restrict__ y, int H) {
  __shared__ float xs[4][kC1W + 4];
  __shared__ __attribute__((aligned(16))) float ws[9][kC1];
  __shared__ __attribute__((aligned(16))) float bs[kC1];
  const int tid = threadIdx.x, Hp = H / 2;
  const int ph = (int)(blockIdx.x % (unsigned)Hp);
  const int64_t nimg = blockIdx.x / (unsigned)Hp;
  for (int i = tid; i < 9 * kC1; i += 256) ws[i / kC1][i % kC1] = w[(i % kC1) * 9 + i / kC1];
  if (tid < kC1) bs[tid] = bias[tid];
  for (int i = tid; i < 4 * (kC1W + 2); i += 256) {
    const int rr = i / (kC1W + 2), cc = i % (kC1W + 2) - 1, h = 2 * ph - 1 + rr;
    xs[rr][cc + 1] = (h >= 0 && h < H && cc >= 0 && cc < kC1W) ? to_f32<T>(x[(nimg * H + h) * kC1W + cc]) : 0.f;
  }
  __syncthreads();
  const int pw = tid >> 3, c0 = (tid & 7) * 8;
  float best[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) best[c] = -INFINITY;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const float xv = xs[dy + kh][2 * pw + dx + kw];
          float wv[8];
          load8<float>(&ws[kh * 3 + kw][c0], wv);
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[c] = fmaf(xv, wv[c], acc[c]);
        }
#pragma unroll
      for (int c = 0; c < 8; ++c) best[c] = fmaxf(best[c], acc[c]);
    }
#pragma unroll
  for (int c = 0; c < 8; ++c) best[c] = fmaxf(best[c] + bs[c0 + c], 0.f);
  store8<T>(y + ((nimg * Hp + ph) * (kC1W / 2) + pw) * kC1 + c0, best);
}

}  // namespace

extern "C" {

int64_t dvt_logmel_num_examples(int64_t L) { return num_examples(L); }

size_t dvt_logmel_examples_workspace_bytes(void) { return (size_t)kTableFloats * sizeof(float); }

int dvt_logmel_tables(float* dst, size_t bytes) {
  DVT_REQUIRE(dst && bytes >= (size_t)kTableFloats * sizeof(float),
              "dvt_logmel_tables: needs a host buffer of dvt_logmel_examples_workspace_bytes");
  const double two_pi = 6.283185307179586476925286766559;
  std::vector<double> win(kWin), melw((size_t)kBins * kMel, 0.0);
  for (int i = 0; i < kWin; ++i) win[i] = 0.5 - 0.5 * std::cos(two_pi * i / kWin);
  const double mlo = hz_to_mel(kMelLoHz), mhi = hz_to_mel(kMelHiHz);
  for (int k = 1; k < kBins; ++k) {                           // the DC row stays zero
    const double m = hz_to_mel(k * (kSampleRate / 2.0) / (kBins - 1));
    for (int b = 0; b < kMel; ++b) {
      const double lo = mlo + (mhi - mlo) * b / (kMel + 1), ctr = mlo + (mhi - mlo) * (b + 1) / (kMel + 1),
                   hi = mlo + (mhi - mlo) * (b + 2) / (kMel + 1);
      const double v = std::fmin((m - lo) / (ctr - lo), (hi - m) / (hi - ctr));
      melw[(size_t)k * kMel + b] = v > 0.0 ? v : 0.0;
    }
  }
  for (int k = kBinsUsed; k < kBins; ++k)
    for (int b = 0; b < kMel; ++b)
      DVT_REQUIRE(melw[(size_t)k * kMel + b] == 0.0, "dvt_logmel_tables: bin %d carries mel weight; raise kBinsUsed", k);
  for (int i = 0; i < kWin; ++i) dst[kOffWin + i] = (float)win[i];
  for (int t = 0; t < kFft / 2; ++t) {
    dst[kOffTw + 2 * t] = (float)std::cos(two_pi * t / kFft);
    dst[kOffTw + 2 * t + 1] = (float)-std::sin(two_pi * t / kFft);
  }
  for (int kb = 0; kb < kKB; ++kb)
    for (int t = 0; t < 2 * kBinTiles; ++t)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 4; ++j) {
          const int k = kb * 16 + 4 * (lane >> 4) + j, bin = (t >> 1) * 16 + (lane & 15);
          const double ang = two_pi * ((k * bin) % kFft) / kFft;
          dst[kOffDft + ((kb * 2 * kBinTiles + t) * 64 + lane) * 4 + j] = (float)(win[k] * ((t & 1) ? std::sin(ang) : std::cos(ang)));
        }
  for (int kb = 0; kb < kBinTiles; ++kb)
    for (int nt = 0; nt < 4; ++nt)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 4; ++j) {
          const int bin = kb * 16 + 4 * (lane >> 4) + j, m = nt * 16 + (lane & 15);
          dst[kOffMel + ((kb * 4 + nt) * 64 + lane) * 4 + j] = (float)melw[(size_t)bin * kMel + m];
        }
  return DVT_OK;
}

int dvt_logmel_examples(const float* wave, int64_t R, int64_t L, const float* tables, void* out, int dtype, int variant,
                        dvt_stream_t stream) {
  DVT_REQUIRE(R >= 0 && L >= 0, "dvt_logmel_examples: negative R or L");
  DVT_REQUIRE(variant == DVT_LOGMEL_DFT || variant == DVT_LOGMEL_FFT, "dvt_logmel_examples: variant %d", variant);
  DVT_REQUIRE(dtype == DVT_F32 || dvt_is_16bit(dtype), "dvt_logmel_examples: dtype %d not supported", dtype);
  const int64_t E = num_examples(L);
  if (R == 0 || E == 0) return DVT_OK;
  DVT_REQUIRE(wave && tables && out, "dvt_logmel_examples: null wave / tables / out");
  DVT_REQUIRE(dvt_aligned16(tables), "dvt_logmel_examples: the tables must be 16-byte aligned");
  const int64_t blocks = R * E * (kExFrames / (variant == DVT_LOGMEL_DFT ? Shape<DVT_LOGMEL_DFT>::FPB : Shape<DVT_LOGMEL_FFT>::FPB));
  if (E >= ((int64_t)1 << 24) || blocks >= ((int64_t)1 << 31))
    DVT_UNSUPPORTED("dvt_logmel_examples: %lld clips of %lld examples: split the batch", (long long)R, (long long)E);
  hipStream_t st = (hipStream_t)stream;
  if (variant == DVT_LOGMEL_DFT) {
    DVT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((logmel_kernel<T, DVT_LOGMEL_DFT>), dim3((unsigned)blocks), dim3(256), 0, st,
                                                    wave, L, (int)E, tables, (T*)out));
  } else {
    DVT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((logmel_kernel<T, DVT_LOGMEL_FFT>), dim3((unsigned)blocks), dim3(256), 0, st,
                                                    wave, L, (int)E, tables, (T*)out));
  }
  DVT_LAUNCH_CHECK("dvt_logmel_examples");
  return DVT_OK;
}

int dvt_vggish_conv1_pool(const void* x, const float* w, const float* bias, void* y, int64_t N, int H, int W, int dtype,
                          dvt_stream_t stream) {
  DVT_REQUIRE(N >= 0 && H > 0 && W > 0, "dvt_vggish_conv1_pool: bad shape");
  if (W != kC1W || H % 2 != 0)
    DVT_UNSUPPORTED("dvt_vggish_conv1_pool: map %d x %d (takes an even height and width %d)", H, W, kC1W);
  DVT_REQUIRE(dtype == DVT_F32 || dvt_is_16bit(dtype), "dvt_vggish_conv1_pool: dtype %d not supported", dtype);
  if (N == 0) return DVT_OK;
  DVT_REQUIRE(x && w && bias && y, "dvt_vggish_conv1_pool: null pointer");
  DVT_REQUIRE(dvt_aligned16(y), "dvt_vggish_conv1_pool: y must be 16-byte aligned");
  const int64_t blocks = N * (H / 2);
  if (blocks >= ((int64_t)1 << 31)) DVT_UNSUPPORTED("dvt_vggish_conv1_pool: %lld images: split the batch", (long long)N);
  DVT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((vggish_conv1_pool_kernel<T>), dim3((unsigned)blocks), dim3(256), 0,
                                                  (hipStream_t)stream, (const T*)x, w, bias, (T*)y, H));
  DVT_LAUNCH_CHECK("dvt_vggish_conv1_pool");
  return DVT_OK;
}

}  // extern "C"
