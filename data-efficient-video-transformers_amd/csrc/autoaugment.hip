// autoaugment.hip -- torchvision's AutoAugment (PIL path) on uint8 frames that already live in HBM
// (reference: transforms.AutoAugment() in src/dataloaders/mmx/MMX_Frame_dl.py:63-71).
//
// One workgroup per sample, the image resident in LDS: the first operation of the sample's sub-policy reads the source
// frame from global memory and writes its uint8 result into LDS, the second reads that image and writes the destination
// with ToTensor + Normalize in its store.  No operation runs in place, so every pair works with the one buffer.  An
// operation that needs a statistic of its whole input (Equalize, AutoContrast: per-channel histograms; Contrast: the sum of
// the luma) first makes a counting pass over that input -- global for the first operation, LDS for the second -- into integer
// LDS counters, so the result cannot depend on the order of the additions.
//
// Arithmetic follows Pillow's C: integer luma, 16.16 fixed-point affine sampling, float32 blends with the product and the sum
// rounded separately, the AutoContrast table in double.  Neither the contraction pragma below nor __fmul_rn / __fadd_rn
// keeps the compiler from fusing a product into the sum that follows (the blend came out as v_fmac_f32 and truncated
// 14.999999 where Pillow truncates 15.0), so every product that Pillow rounds passes through aa_rounded() first.
#pragma clang fp contract(off)
#include "common.h"

#include <math.h>
#include <string.h>
#include <type_traits>

namespace {

constexpr int kAaThreads = 1024;                 // sixteen waves walk the pixels of one sample
constexpr int kAaChunk = 48;                     // samples whose slots travel as kernel arguments of one launch (64 bytes each)
constexpr int kAaSlot = 8;                       // {op, p0 .. p6}
constexpr int kAaOps = DVT_AA_INVERT + 1;
// LDS of a workgroup: int counters [3][256], byte tables [3][256], then the image [H, W, 3]
constexpr int kAaLut = 3 * 256 * (int)sizeof(int);
constexpr int kAaImage = kAaLut + 3 * 256;
constexpr int kAaLds = 160 * 1024;
constexpr int kAaImageBytes = kAaLds - kAaImage;
static_assert(kAaImage % 16 == 0 && 224 * 224 * 3 <= kAaImageBytes, "the reference's 224 x 224 image must fit");

struct AaRows { int v[kAaChunk][2][kAaSlot]; };
struct AaNorm { float m[3], d[3]; };
struct AaU8Hwc {};                               // destination tag: uint8 [N, H, W, 3], not normalised

__device__ __forceinline__ unsigned char* aa_lds() {
  extern __shared__ __attribute__((aligned(16))) unsigned char aa_lds_bytes[];
  return aa_lds_bytes;
}

// ---------------------------------------------------------------- where an operation reads and writes
struct AaSrcGlobal {
  const unsigned char* __restrict__ p;
  __device__ __forceinline__ void px(int i, int& r, int& g, int& b) const {
    const unsigned char* q = p + (int64_t)i * 3;
    r = q[0]; g = q[1]; b = q[2];
  }
};
struct AaSrcLds {
  __device__ __forceinline__ void px(int i, int& r, int& g, int& b) const {
    const unsigned char* q = aa_lds() + kAaImage + i * 3;
    r = q[0]; g = q[1]; b = q[2];
  }
};
struct AaDstLds {
  __device__ __forceinline__ void put(int i, int r, int g, int b) const {
    unsigned char* q = aa_lds() + kAaImage + i * 3;
    q[0] = (unsigned char)r; q[1] = (unsigned char)g; q[2] = (unsigned char)b;
  }
};
template <typename D>
struct AaDstOut {
  void* __restrict__ dst;                        // this sample's first element
  int plane;
  AaNorm nm;
  __device__ __forceinline__ void put(int i, int r, int g, int b) const {
    if constexpr (std::is_same<D, AaU8Hwc>::value) {
      unsigned char* o = (unsigned char*)dst + (int64_t)i * 3;
      o[0] = (unsigned char)r; o[1] = (unsigned char)g; o[2] = (unsigned char)b;
    } else {                                     // the epilogue of dvt_frames_augment, operation for operation
      const float v0 = __fdiv_rn(__fdiv_rn((float)r, 255.0f) - nm.m[0], nm.d[0]);
      const float v1 = __fdiv_rn(__fdiv_rn((float)g, 255.0f) - nm.m[1], nm.d[1]);
      const float v2 = __fdiv_rn(__fdiv_rn((float)b, 255.0f) - nm.m[2], nm.d[2]);
      D* o = (D*)dst + i;
      o[0] = from_f32<D>(v0); o[plane] = from_f32<D>(v1); o[2 * (int64_t)plane] = from_f32<D>(v2);
    }
  }
};

// ---------------------------------------------------------------- pixel arithmetic
// A value as the register holds it, opaque to the optimiser: a product that went through here is rounded, and cannot be
// fused with an addition on the other side.
template <typename T>
__device__ __forceinline__ T aa_rounded(T v) {
  asm volatile("" : "+v"(v));
  return v;
}

__device__ __forceinline__ int aa_clip8f(float v) { return v <= 0.0f ? 0 : (v >= 255.0f ? 255 : (int)v); }

__device__ __forceinline__ int aa_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend(degenerate, image, f): truncated when 0 <= f <= 1 (the value lies between the two), clipped otherwise
__device__ __forceinline__ int aa_blend(int deg, int v, float f, bool inside) {
  const float t = (float)deg + aa_rounded(f * (float)(v - deg));
  return inside ? (int)t : aa_clip8f(t);
}

// ImageFilter.SMOOTH at an interior pixel: weights 1 / 13 and 5 / 13 in float32; the sum starts at the rounding offset
// 0.5 and takes the row below, the row itself and the row above, each as ((left + centre) + right)
template <class S>
__device__ __forceinline__ void aa_smooth(const S& src, int i, int W, int& r, int& g, int& b) {
  const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
  float s0 = 0.5f, s1 = 0.5f, s2 = 0.5f;
#pragma unroll
  for (int dy = 1; dy >= -1; --dy) {
    const float km = dy == 0 ? k5 : k1;
    const int c = i + dy * W;
    int r0, g0, b0, r1, g1, b1, r2, g2, b2;
    src.px(c - 1, r0, g0, b0); src.px(c, r1, g1, b1); src.px(c + 1, r2, g2, b2);
    s0 += (aa_rounded((float)r0 * k1) + aa_rounded((float)r1 * km)) + aa_rounded((float)r2 * k1);
    s1 += (aa_rounded((float)g0 * k1) + aa_rounded((float)g1 * km)) + aa_rounded((float)g2 * k1);
    s2 += (aa_rounded((float)b0 * k1) + aa_rounded((float)b1 * km)) + aa_rounded((float)b2 * k1);
  }
  r = aa_clip8f(s0); g = aa_clip8f(s1); b = aa_clip8f(s2);
}

__device__ __forceinline__ int aa_wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The pixel loop of one kind of operation: OP is the operation, DVT_AA_ROTATE for every geometric one (they differ in their
// coefficients only) and DVT_AA_EQUALIZE for both table operations.  mean: the rounded mean luma (Contrast).
template <int OP, class S, class Dw>
__device__ __forceinline__ void aa_pixels(const int* s, const S src, const Dw dst, int H, int W, int mean) {
  constexpr bool blend = OP >= DVT_AA_BRIGHTNESS && OP <= DVT_AA_SHARPNESS;
  const int npx = H * W;
  const unsigned char* lut = aa_lds() + kAaLut;
  const float f = __int_as_float(s[1]);
  const bool inside = f >= 0.0f && f <= 1.0f;
#pragma unroll 4
  for (int i = threadIdx.x; i < npx; i += kAaThreads) {
    int r = 0, g = 0, b = 0;
    if constexpr (OP == DVT_AA_ROTATE) {
      const int y = i / W, x = i - y * W;
      const int64_t xin = ((int64_t)s[3] + (int64_t)s[2] * y + (int64_t)s[1] * x) >> 16;
      const int64_t yin = ((int64_t)s[6] + (int64_t)s[5] * y + (int64_t)s[4] * x) >> 16;
      if (xin >= 0 && xin < W && yin >= 0 && yin < H) src.px((int)yin * W + (int)xin, r, g, b);
    } else {
      src.px(i, r, g, b);
      if constexpr (blend) {
        int d0 = 0, d1 = 0, d2 = 0;              // Brightness: black
        if constexpr (OP == DVT_AA_COLOR) d0 = d1 = d2 = aa_luma(r, g, b);
        else if constexpr (OP == DVT_AA_CONTRAST) d0 = d1 = d2 = mean;
        else if constexpr (OP == DVT_AA_SHARPNESS) {
          const int y = i / W, x = i - y * W;
          d0 = r; d1 = g; d2 = b;                // the filter copies the one-pixel border
          if (y > 0 && y < H - 1 && x > 0 && x < W - 1) aa_smooth(src, i, W, d0, d1, d2);
        }
        r = aa_blend(d0, r, f, inside); g = aa_blend(d1, g, f, inside); b = aa_blend(d2, b, f, inside);
      } else if constexpr (OP == DVT_AA_POSTERIZE) {
        r &= s[1]; g &= s[1]; b &= s[1];
      } else if constexpr (OP == DVT_AA_SOLARIZE) {
        r = r < s[1] ? r : 255 - r; g = g < s[1] ? g : 255 - g; b = b < s[1] ? b : 255 - b;
      } else if constexpr (OP == DVT_AA_INVERT) {
        r = 255 - r; g = 255 - g; b = 255 - b;
      } else if constexpr (OP == DVT_AA_EQUALIZE) {
        r = lut[r]; g = lut[256 + g]; b = lut[512 + b];
      }
    }
    dst.put(i, r, g, b);
  }
}

// One operation over the whole image: slot s (wave-uniform), pixels read through src, results written through dst.  Ends
// with a barrier: the image written to LDS is complete, and the counters and tables may be used again.
template <class S, class Dw>
__device__ __forceinline__ void aa_apply(const int* s, const S src, const Dw dst, int H, int W) {
  const int op = s[0];
  const int npx = H * W;
  const int tid = threadIdx.x;
  int* hist = (int*)aa_lds();
  unsigned char* lut = aa_lds() + kAaLut;
  int mean = 0;
  if (op == DVT_AA_AUTOCONTRAST || op == DVT_AA_EQUALIZE) {
    for (int i = tid; i < 3 * 256; i += kAaThreads) hist[i] = 0;
    __syncthreads();
#pragma unroll 4
    for (int i = tid; i < npx; i += kAaThreads) {
      int r, g, b;
      src.px(i, r, g, b);
      atomicAdd(&hist[r], 1); atomicAdd(&hist[256 + g], 1); atomicAdd(&hist[512 + b], 1);
    }
    __syncthreads();
    if (tid < 3 * 256) {                         // thread (channel, value): one table entry from a scan of the channel's bins
      const int v = tid & 255;
      const int* h = hist + (tid & ~255);
      int total = 0, below = 0, bins = 0, last = 0, lo = 255, hi = 0;
      for (int j = 0; j < 256; ++j) {
        const int c = h[j];
        total += c;
        below += j < v ? c : 0;
        if (c) { ++bins; last = c; hi = j; lo = lo < j ? lo : j; }
      }
      int out = v;
      if (op == DVT_AA_EQUALIZE) {               // ImageOps.equalize
        const int step = (total - last) / 255;
        if (bins > 1 && step != 0) out = (step / 2 + below) / step;
      } else if (hi > lo) {                      // ImageOps.autocontrast, cutoff 0: Python's double arithmetic
        const double scale = 255.0 / (double)(hi - lo);
        const double offset = (double)(-lo) * scale;
        out = (int)(aa_rounded((double)v * scale) + offset);
      }
      lut[tid] = (unsigned char)(out < 0 ? 0 : (out > 255 ? 255 : out));
    }
    __syncthreads();
  } else if (op == DVT_AA_CONTRAST) {            // the degenerate image: the mean luma, rounded
    if (tid == 0) hist[0] = 0;
    __syncthreads();
    int sum = 0;                                 // at most 255 x 53,333 pixels of an image that fits: no overflow
#pragma unroll 4
    for (int i = tid; i < npx; i += kAaThreads) {
      int r, g, b;
      src.px(i, r, g, b);
      sum += aa_luma(r, g, b);
    }
    sum = aa_wave_sum_int(sum);
    if ((tid & 63) == 0) atomicAdd(&hist[0], sum);
    __syncthreads();
    mean = (int)((double)hist[0] / (double)npx + 0.5);
  }
  // the pixel loop, compiled once per kind of operation: a loop without the dispatch in it keeps four pixels' loads in flight
  switch (op) {
    case DVT_AA_SHEAR_X: case DVT_AA_SHEAR_Y: case DVT_AA_TRANSLATE_X: case DVT_AA_TRANSLATE_Y: case DVT_AA_ROTATE:
      aa_pixels<DVT_AA_ROTATE>(s, src, dst, H, W, mean); break;
    case DVT_AA_BRIGHTNESS: aa_pixels<DVT_AA_BRIGHTNESS>(s, src, dst, H, W, mean); break;
    case DVT_AA_COLOR: aa_pixels<DVT_AA_COLOR>(s, src, dst, H, W, mean); break;
    case DVT_AA_CONTRAST: aa_pixels<DVT_AA_CONTRAST>(s, src, dst, H, W, mean); break;
    case DVT_AA_SHARPNESS: aa_pixels<DVT_AA_SHARPNESS>(s, src, dst, H, W, mean); break;
    case DVT_AA_POSTERIZE: aa_pixels<DVT_AA_POSTERIZE>(s, src, dst, H, W, mean); break;
    case DVT_AA_SOLARIZE: aa_pixels<DVT_AA_SOLARIZE>(s, src, dst, H, W, mean); break;
    case DVT_AA_INVERT: aa_pixels<DVT_AA_INVERT>(s, src, dst, H, W, mean); break;
    case DVT_AA_AUTOCONTRAST: case DVT_AA_EQUALIZE: aa_pixels<DVT_AA_EQUALIZE>(s, src, dst, H, W, mean); break;
    default: aa_pixels<DVT_AA_IDENTITY>(s, src, dst, H, W, mean); break;
  }
  __syncthreads();
}

// Workgroup s of a launch: sample base + s.
template <typename D>
__global__ __launch_bounds__(kAaThreads) void autoaugment_kernel(const unsigned char* __restrict__ src, void* __restrict__ dst_,
                                                                 AaRows rows, int64_t base, int H, int W, AaNorm nm) {
  const int s = blockIdx.x;
  const int64_t n = base + s;
  const int npx = H * W;
  aa_apply(rows.v[s][0], AaSrcGlobal{src + n * npx * 3}, AaDstLds{}, H, W);
  char* out = (char*)dst_ + n * npx * 3 * (int64_t)(std::is_same<D, AaU8Hwc>::value ? 1 : sizeof(D));
  aa_apply(rows.v[s][1], AaSrcLds{}, AaDstOut<D>{out, npx, nm}, H, W);
}

template <typename D>
void aa_launch(int count, int lds, hipStream_t st, const void* src, void* dst, const AaRows& rows, int64_t base, int H, int W,
               const AaNorm& nm) {
  static DvtLdsAttr set;
  dvt_lds_attr(set, (const void*)autoaugment_kernel<D>, kAaLds);
  hipLaunchKernelGGL((autoaugment_kernel<D>), dim3((unsigned)count), dim3(kAaThreads), lds, st, (const unsigned char*)src, dst,
                     rows, base, H, W, nm);
}

}  // namespace

extern "C" {

int dvt_frames_autoaugment(const void* src, int64_t samples, int H, int W, const int32_t* table, void* dst, int dst_dtype,
                           const float* mean, const float* std, dvt_stream_t stream) {
  const bool u8 = dst_dtype == DVT_AUGMENT_U8_HWC;
  DVT_REQUIRE(src, "dvt_frames_autoaugment: src is null");
  DVT_REQUIRE(table, "dvt_frames_autoaugment: table is null");
  DVT_REQUIRE(dst, "dvt_frames_autoaugment: dst is null");
  DVT_REQUIRE(u8 || dst_dtype == DVT_F32 || dst_dtype == DVT_BF16 || dst_dtype == DVT_F16,
              "dvt_frames_autoaugment: dst_dtype %d is neither a dvt_dtype nor DVT_AUGMENT_U8_HWC", dst_dtype);
  DVT_REQUIRE(u8 || mean, "dvt_frames_autoaugment: mean is null");
  DVT_REQUIRE(u8 || std, "dvt_frames_autoaugment: std is null");
  DVT_REQUIRE(samples >= 0 && H >= 3 && W >= 3, "dvt_frames_autoaugment: samples %lld of %d x %d: needs samples >= 0 and H, W >= 3",
              (long long)samples, H, W);
  for (int64_t n = 0; n < samples; ++n)
    for (int k = 0; k < 2; ++k) {
      const int32_t* s = table + (n * 2 + k) * kAaSlot;
      DVT_REQUIRE(s[0] >= 0 && s[0] < kAaOps, "dvt_frames_autoaugment: sample %lld slot %d: op %d outside [0, %d)", (long long)n, k,
                  (int)s[0], kAaOps);
      if (s[0] == DVT_AA_POSTERIZE) {
        const int low = ~s[1] & 0xff;            // a valid mask keeps a run of high bits: its complement is 2^k - 1
        DVT_REQUIRE(s[1] >= 0 && s[1] <= 255 && (low & (low + 1)) == 0,
                    "dvt_frames_autoaugment: sample %lld slot %d: posterize mask %d is not a run of high bits of a byte",
                    (long long)n, k, (int)s[1]);
      } else if (s[0] == DVT_AA_SOLARIZE) {
        DVT_REQUIRE(s[1] >= 0 && s[1] <= 256, "dvt_frames_autoaugment: sample %lld slot %d: solarize threshold %d outside [0, 256]",
                    (long long)n, k, (int)s[1]);
      } else if (s[0] >= DVT_AA_BRIGHTNESS && s[0] <= DVT_AA_SHARPNESS) {
        float f;
        memcpy(&f, s + 1, sizeof(f));
        DVT_REQUIRE(isfinite(f), "dvt_frames_autoaugment: sample %lld slot %d: the blend factor is not finite", (long long)n, k);
      }
    }
  if (!u8) DVT_REQUIRE(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "dvt_frames_autoaugment: zero std");
  if ((int64_t)H * W * 3 > kAaImageBytes)
    DVT_UNSUPPORTED("dvt_frames_autoaugment: a %d x %d image is %lld bytes, more than the %d bytes of LDS a workgroup keeps its "
                    "image in (224 x 224 fits)", H, W, (long long)H * W * 3, kAaImageBytes);
  if (samples == 0) return DVT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int lds = kAaImage + ((H * W * 3 + 15) & ~15);
  AaNorm nm = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};
  if (!u8) nm = {{mean[0], mean[1], mean[2]}, {std[0], std[1], std[2]}};
  for (int64_t base = 0; base < samples; base += kAaChunk) {
    const int count = (int)(samples - base < kAaChunk ? samples - base : kAaChunk);
    AaRows rows;
    memset(&rows, 0, sizeof(rows));
    memcpy(rows.v, table + base * 2 * kAaSlot, sizeof(int) * 2 * kAaSlot * count);
    if (u8) aa_launch<AaU8Hwc>(count, lds, st, src, dst, rows, base, H, W, nm);
    else DVT_DISPATCH_DTYPE(dst_dtype, D, aa_launch<D>(count, lds, st, src, dst, rows, base, H, W, nm));
    DVT_LAUNCH_CHECK("dvt_frames_autoaugment");
  }
  return DVT_OK;
}

}  // extern "C"
