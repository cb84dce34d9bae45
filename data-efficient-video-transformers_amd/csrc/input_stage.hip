// input_stage.hip -- decoded uint8 RGB frames -> normalised clip tensor, on the device.
//
// Replaces the per-frame host pipeline of the reference's loader
//   transforms.Compose([Resize(S), CenterCrop(C), ToTensor(), Normalize(mean, std)])
// (src/dataloaders/mmx/MMX_Light_dl.py:203-217, applied frame by frame by 10 PIL workers at :161-162,270-273).
// Bit-exact with Pillow's 8-bit bilinear resample (ImagingResample): triangle filter of support max(scale, 1),
// weights normalised in double precision and rounded to 22-bit fixed point, horizontal pass then vertical pass
// through a uint8 intermediate.  Double-precision expressions must round exactly like the host C code, so
// floating-point contraction is disabled for this file.
#pragma clang fp contract(off)
#include "common.h"

#include <string.h>
#include <type_traits>

namespace {

constexpr int kPrec = 32 - 8 - 2;   // Pillow PRECISION_BITS
constexpr int kB = 256;

__device__ __forceinline__ int clip8(int v) {
  v >>= kPrec;                      // arithmetic shift, then the clip8 lookup of Pillow
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Pillow precompute_coeffs + normalize_coeffs_8bpc (bilinear, support 1) for output coordinate xx of an axis resampled
// from in_size to out_size: first tap `lo`, tap count `n`, fixed-point taps k[0 .. ksize) (zero past n).
__device__ __forceinline__ void resample_coeff_row(int in_size, int out_size, int xx, int ksize, int* __restrict__ k,
                                                   int& lo, int& n) {
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const double ss = 1.0 / filterscale;
  const double center = ((double)xx + 0.5) * scale;
  lo = (int)(center - support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(center + support + 0.5);
  if (hi > in_size) hi = in_size;
  n = hi - lo;
  double ww = 0.0;
  for (int x = 0; x < n; ++x) {
    double a = ((double)(x + lo) - center + 0.5) * ss;
    if (a < 0.0) a = -a;
    ww += a < 1.0 ? 1.0 - a : 0.0;
  }
  for (int x = 0; x < ksize; ++x) {
    int q = 0;
    if (x < n) {
      double a = ((double)(x + lo) - center + 0.5) * ss;
      if (a < 0.0) a = -a;
      double w = a < 1.0 ? 1.0 - a : 0.0;
      if (ww != 0.0) w = w / ww;
      q = w < 0.0 ? (int)(-0.5 + w * (double)(1 << kPrec)) : (int)(0.5 + w * (double)(1 << kPrec));
    }
    k[x] = q;
  }
}

// One thread per output coordinate of the one geometry every frame of dvt_frames_preprocess shares.
__global__ void resample_coeff_kernel(int in_size, int out_size, int ksize, int* __restrict__ xmin,
                                      int* __restrict__ cnt, int* __restrict__ kk) {
  const int xx = blockIdx.x * blockDim.x + threadIdx.x;
  if (xx >= out_size) return;
  int lo, n;
  resample_coeff_row(in_size, out_size, xx, ksize, kk + (int64_t)xx * ksize, lo, n);
  xmin[xx] = lo;
  cnt[xx] = n;
}

// Horizontal pass: src [F, H0, W0, 3] -> tmp [F, H0, Wc, 3] for the Wc resized columns [left, left + Wc).
__global__ void resample_h_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ tmp,
                                  const int* __restrict__ xmin, const int* __restrict__ cnt,
                                  const int* __restrict__ kk, int ksize, int64_t rows /* F*H0 */, int W0, int Wc,
                                  int left) {
  const int64_t total = rows * Wc;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % Wc);
    const int64_t r = i / Wc;
    const int xx = xo + left;
    const int lo = xmin[xx], n = cnt[xx];
    const int* k = kk + (int64_t)xx * ksize;
    const unsigned char* p = src + (r * W0 + lo) * 3;
    int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < n; ++x) {
      const int c = k[x];
      s0 += (int)p[3 * x + 0] * c;
      s1 += (int)p[3 * x + 1] * c;
      s2 += (int)p[3 * x + 2] * c;
    }
    unsigned char* o = tmp + i * 3;
    o[0] = (unsigned char)clip8(s0); o[1] = (unsigned char)clip8(s1); o[2] = (unsigned char)clip8(s2);
  }
}

// Vertical pass over tmp + centre crop + ToTensor (/255) + Normalize ((t - mean) / std), written as NCHW.
template <typename D>
__global__ void resample_v_norm_kernel(const unsigned char* __restrict__ tmp, D* __restrict__ dst,
                                       const int* __restrict__ ymin, const int* __restrict__ cnt,
                                       const int* __restrict__ kk, int ksize, int64_t F, int H0, int Wc, int Hc,
                                       int top, float m0, float m1, float m2, float d0, float d1, float d2) {
  const int64_t total = F * Hc * Wc;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % Wc), yo = (int)((i / Wc) % Hc);
    const int64_t f = i / ((int64_t)Wc * Hc);
    const int yy = yo + top;
    const int lo = ymin[yy], n = cnt[yy];
    const int* k = kk + (int64_t)yy * ksize;
    const unsigned char* p = tmp + ((f * H0 + lo) * Wc + xo) * 3;
    int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
    for (int y = 0; y < n; ++y) {
      const int c = k[y];
      const unsigned char* q = p + (int64_t)y * Wc * 3;
      s0 += (int)q[0] * c; s1 += (int)q[1] * c; s2 += (int)q[2] * c;
    }
    const float v0 = __fdiv_rn(__fdiv_rn((float)clip8(s0), 255.0f) - m0, d0);
    const float v1 = __fdiv_rn(__fdiv_rn((float)clip8(s1), 255.0f) - m1, d1);
    const float v2 = __fdiv_rn(__fdiv_rn((float)clip8(s2), 255.0f) - m2, d2);
    const int64_t plane = (int64_t)Hc * Wc;
    D* o = dst + f * 3 * plane + (int64_t)yo * Wc + xo;
    o[0] = from_f32<D>(v0); o[plane] = from_f32<D>(v1); o[2 * plane] = from_f32<D>(v2);
  }
}

struct Plan {
  int h, w, top, left, ks_h, ks_w;
  size_t off_xmin, off_xcnt, off_xk, off_ymin, off_ycnt, off_yk, off_tmp, bytes;
};

int ksize_of(int in_size, int out_size) {
  const double scale = (double)in_size / (double)out_size;
  const double support = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(support) * 2 + 1;
}

bool make_plan(int64_t frames, int H0, int W0, int resize, int crop, Plan* p) {
  // torchvision Resize(int): shorter side -> resize, longer -> int(resize * long / short)
  if (W0 <= H0) { p->w = resize; p->h = (int)((double)resize * H0 / W0); }
  else { p->h = resize; p->w = (int)((double)resize * W0 / H0); }
  if (p->h < crop || p->w < crop) return false;
  p->top = (int)lrint((p->h - crop) / 2.0);      // Python round(): half to even, like lrint in the default mode
  p->left = (int)lrint((p->w - crop) / 2.0);
  p->ks_w = ksize_of(W0, p->w);
  p->ks_h = ksize_of(H0, p->h);
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  size_t o = 0;
  p->off_xmin = o; o = al(o + sizeof(int) * p->w);
  p->off_xcnt = o; o = al(o + sizeof(int) * p->w);
  p->off_xk = o;   o = al(o + sizeof(int) * (size_t)p->w * p->ks_w);
  p->off_ymin = o; o = al(o + sizeof(int) * p->h);
  p->off_ycnt = o; o = al(o + sizeof(int) * p->h);
  p->off_yk = o;   o = al(o + sizeof(int) * (size_t)p->h * p->ks_h);
  p->off_tmp = o;  o = al(o + (size_t)frames * H0 * crop * 3);
  p->bytes = o;
  return true;
}

inline int grid_for(int64_t items) {
  int64_t b = dvt_cdiv(items, kB);
  const int64_t cap = (int64_t)dvt_num_cus() * 16;
  if (b > cap) b = cap;
  return (int)(b < 1 ? 1 : b);
}

// ---------------------------------------------------------------- per-sample crop -> resize -> flip -> normalise
constexpr int kAugFields = 7;        // table row: src_index, top, left, h, w, hflip, vflip
constexpr int kAugTabStride = 8;     // device copy of a row, padded to 32 bytes
constexpr int kAugChunk = 64;        // table rows that travel as kernel arguments of one coefficient launch
constexpr int kAugBand = 16;         // output rows per workgroup, fewer where the LDS budget asks for it
constexpr int kAugThreads = 1024;    // band kernel: sixteen waves share a band's input rows
constexpr int kAugLds = 64 * 1024;   // LDS budget of one band: the default dynamic limit
struct AugRows { int v[kAugChunk][kAugFields]; };

// One workgroup row (blockIdx.y) per sample of the chunk, one thread per output coordinate of either axis: the window's
// w -> out_w taps, then its h -> out_h taps -- the taps are those of the cropped image, i.e. clipped to the window.  Thread
// 0 also leaves the sample's table row in the workspace for the fused launch.
__global__ void augment_coeff_kernel(AugRows rows, int base, int out_h, int out_w, int ks_h, int ks_w,
                                     int* __restrict__ tab, int* __restrict__ xmin, int* __restrict__ xcnt,
                                     int* __restrict__ xk, int* __restrict__ ymin, int* __restrict__ ycnt,
                                     int* __restrict__ yk) {
  const int s = blockIdx.y;
  const int64_t n = (int64_t)base + s;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0) {
#pragma unroll
    for (int f = 0; f < kAugFields; ++f) tab[n * kAugTabStride + f] = rows.v[s][f];
  }
  if (j >= out_w + out_h) return;
  int lo, cnt;
  if (j < out_w) {
    const int64_t o = n * out_w + j;
    resample_coeff_row(rows.v[s][4], out_w, j, ks_w, xk + o * ks_w, lo, cnt);
    xmin[o] = lo;
    xcnt[o] = cnt;
  } else {
    const int64_t o = n * out_h + (j - out_w);
    resample_coeff_row(rows.v[s][3], out_h, j - out_w, ks_h, yk + o * ks_h, lo, cnt);
    ymin[o] = lo;
    ycnt[o] = cnt;
  }
}

struct AugNorm { float m[3], d[3]; };
struct U8Hwc {};                     // destination tag: uint8 [N, out_h, out_w, 3], not normalised

// Workgroup (band b, sample n): output rows [b * band, min(out_h, (b + 1) * band)) of sample n.  Phase 1 resamples the
// R input rows those output rows read (ymin of the first .. ymin + count of the last: both are monotone) horizontally
// into LDS as uint8 [R, out_w, 3]; phase 2 runs the vertical pass from LDS and writes the flipped destination pixel.
// Lanes walk xo, so global reads overlap between neighbours, LDS bytes are 3 apart (at most two lanes of a group in one
// dword, 24 distinct banks per 32 lanes: conflict-free) and each channel plane is written in whole runs of a row.
// R <= rmax by the host's bound (aug_rows_bound); the test is there so that a wrong bound could not write past the LDS.
template <typename D>
__global__ __launch_bounds__(kAugThreads) void augment_band_kernel(
    const unsigned char* __restrict__ src, void* __restrict__ dst_, const int* __restrict__ tab,
    const int* __restrict__ xmin, const int* __restrict__ xcnt, const int* __restrict__ xk, const int* __restrict__ ymin,
    const int* __restrict__ ycnt, const int* __restrict__ yk, int H0, int W0, int out_h, int out_w, int ks_h, int ks_w,
    int band, int rmax, AugNorm nm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char aug_rows[];
  const int64_t n = blockIdx.y;
  const int y0 = blockIdx.x * band;
  const int y1 = y0 + band < out_h ? y0 + band : out_h;
  const int* t = tab + n * kAugTabStride;
  const int frame = t[0], top = t[1], left = t[2], win_w = t[4], hflip = t[5], vflip = t[6];
  xmin += n * out_w; xcnt += n * out_w; xk += n * out_w * ks_w;
  ymin += n * out_h; ycnt += n * out_h; yk += n * out_h * ks_h;
  const int rlo = ymin[y0];
  const int R = ymin[y1 - 1] + ycnt[y1 - 1] - rlo;
  if (R > rmax) return;
  // the band's vertical taps, first rows and counts, behind the rows: phase 2 reads them once per tap and pixel
  int* yk_s = (int*)(aug_rows + ((rmax * out_w * 3 + 15) & ~15));
  int* ymin_s = yk_s + band * ks_h;
  int* ycnt_s = ymin_s + band;
  for (int i = threadIdx.x; i < (y1 - y0) * ks_h; i += kAugThreads) yk_s[i] = yk[(int64_t)y0 * ks_h + i];
  for (int i = threadIdx.x; i < y1 - y0; i += kAugThreads) {
    ymin_s[i] = ymin[y0 + i] - rlo;
    ycnt_s[i] = ycnt[y0 + i];
  }
  const unsigned char* win = src + (((int64_t)frame * H0 + top + rlo) * W0 + left) * 3;
  // Phase 1.  A thread keeps one output column and walks the band's input rows; the rows are split between
  // kAugThreads / out_w groups of threads.  A byte load is one address per lane and instruction and a tap loop waits once
  // per tap, so a column of up to 4 or 8 taps keeps its taps in registers and reads its K pixels of a row as 3 K / 4
  // unaligned dwords: one round of loads per row (40.6 -> 25.2 us at 28 x 360 x 640 -> 224^2).  The K pixels
  // start at min(lo, w - K), so they never leave the window (and so the frame); taps outside [lo, lo + cnt) weigh 0.
  // Windows narrower than K pixels and columns of more than 8 taps take the plain loop.
  const int cols = out_w < kAugThreads ? out_w : kAugThreads, groups = kAugThreads / cols, grp = threadIdx.x / cols;
  if (grp < groups) {
    for (int xo = threadIdx.x - grp * cols; xo < out_w; xo += cols) {
      const int lo = xmin[xo], cnt = xcnt[xo];
      const int* k = xk + (int64_t)xo * ks_w;
      auto column = [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        const int start = lo < win_w - K ? lo : win_w - K;
        int c[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const int t = j - (lo - start);
          c[j] = t >= 0 && t < cnt ? k[t] : 0;
        }
        const unsigned char* col = win + (int64_t)start * 3;
#pragma unroll 2
        for (int r = grp; r < R; r += groups) {
          unsigned v[3 * K / 4];
          __builtin_memcpy(v, col + (int64_t)r * W0 * 3, 3 * K);
          int s[3] = {1 << (kPrec - 1), 1 << (kPrec - 1), 1 << (kPrec - 1)};
#pragma unroll
          for (int b = 0; b < 3 * K; ++b) s[b % 3] += (int)((v[b >> 2] >> ((b & 3) * 8)) & 0xffu) * c[b / 3];
          unsigned char* o = aug_rows + (r * out_w + xo) * 3;
          o[0] = (unsigned char)clip8(s[0]); o[1] = (unsigned char)clip8(s[1]); o[2] = (unsigned char)clip8(s[2]);
        }
      };
      const unsigned char* col = win + (int64_t)lo * 3;
      if (cnt <= 4 && win_w >= 4) column(IntC<4>{});
      else if (cnt <= 8 && win_w >= 8) column(IntC<8>{});
      else {
        for (int r = grp; r < R; r += groups) {
          const unsigned char* p = col + (int64_t)r * W0 * 3;
          int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
          for (int x = 0; x < cnt; ++x) {
            const int c = k[x];
            s0 += (int)p[3 * x + 0] * c;
            s1 += (int)p[3 * x + 1] * c;
            s2 += (int)p[3 * x + 2] * c;
          }
          unsigned char* o = aug_rows + (r * out_w + xo) * 3;
          o[0] = (unsigned char)clip8(s0); o[1] = (unsigned char)clip8(s1); o[2] = (unsigned char)clip8(s2);
        }
      }
    }
  }
  __syncthreads();
  const int64_t plane = (int64_t)out_h * out_w;
  for (int i = threadIdx.x; i < (y1 - y0) * out_w; i += kAugThreads) {
    const int yb = i / out_w, xo = i - yb * out_w;
    const int yo = y0 + yb;
    const int cnt = ycnt_s[yb];
    const int* k = yk_s + yb * ks_h;
    const unsigned char* q = aug_rows + (ymin_s[yb] * out_w + xo) * 3;
    int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
    for (int y = 0; y < cnt; y += 4) {                 // four taps a round; past the count: weight 0 on the last row
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = y + j < cnt ? y + j : cnt - 1;
        const int c = y + j < cnt ? k[t] : 0;
        const unsigned char* qq = q + t * out_w * 3;
        s0 += (int)qq[0] * c; s1 += (int)qq[1] * c; s2 += (int)qq[2] * c;
      }
    }
    const int dy = vflip ? out_h - 1 - yo : yo, dx = hflip ? out_w - 1 - xo : xo;
    if constexpr (std::is_same<D, U8Hwc>::value) {
      unsigned char* o = (unsigned char*)dst_ + (n * plane + (int64_t)dy * out_w + dx) * 3;
      o[0] = (unsigned char)clip8(s0); o[1] = (unsigned char)clip8(s1); o[2] = (unsigned char)clip8(s2);
    } else {
      const float v0 = __fdiv_rn(__fdiv_rn((float)clip8(s0), 255.0f) - nm.m[0], nm.d[0]);
      const float v1 = __fdiv_rn(__fdiv_rn((float)clip8(s1), 255.0f) - nm.m[1], nm.d[1]);
      const float v2 = __fdiv_rn(__fdiv_rn((float)clip8(s2), 255.0f) - nm.m[2], nm.d[2]);
      D* o = (D*)dst_ + n * 3 * plane + (int64_t)dy * out_w + dx;
      o[0] = from_f32<D>(v0); o[plane] = from_f32<D>(v1); o[2 * plane] = from_f32<D>(v2);
    }
  }
}

// Input rows a band of `band` output rows can read when the window is the whole frame height (the largest scale, and the
// bound grows with the scale): last tap - first tap <= (c_last + support + 0.5) - (c_first - support + 0.5 - 1)
// = (band - 1) * scale + 2 * support + 1.
int aug_rows_bound(int H0, int out_h, int band) {
  const double scale = (double)H0 / (double)out_h;
  const double support = scale < 1.0 ? 1.0 : scale;
  const double r = ceil((double)(band - 1) * scale + 2.0 * support) + 1.0;
  return r < (double)H0 ? (int)r : H0;
}

// LDS of one band: its input rows resampled horizontally, uint8 [rmax, out_w, 3], then its vertical taps, first rows and counts
int64_t aug_lds_bytes(int rmax, int out_w, int band, int ks_h) {
  return (((int64_t)rmax * out_w * 3 + 15) & ~(int64_t)15) + (int64_t)sizeof(int) * band * (ks_h + 2);
}

struct AugPlan {
  int ks_h, ks_w, band, rmax, lds;
  size_t off_tab, off_xmin, off_xcnt, off_xk, off_ymin, off_ycnt, off_yk, bytes;
};

bool make_aug_plan(int64_t N, int H0, int W0, int out_h, int out_w, AugPlan* p) {
  p->ks_w = ksize_of(W0, out_w);     // the widest window is the frame
  p->ks_h = ksize_of(H0, out_h);
  p->band = 0;
  for (int b = out_h < kAugBand ? out_h : kAugBand; b >= 1 && !p->band; --b)
    if (aug_lds_bytes(aug_rows_bound(H0, out_h, b), out_w, b, p->ks_h) <= kAugLds) p->band = b;
  if (!p->band) return false;
  p->rmax = aug_rows_bound(H0, out_h, p->band);
  p->lds = (int)aug_lds_bytes(p->rmax, out_w, p->band, p->ks_h);
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t n = (size_t)N;
  size_t o = 0;
  p->off_tab = o;  o = al(o + sizeof(int) * n * kAugTabStride);
  p->off_xmin = o; o = al(o + sizeof(int) * n * out_w);
  p->off_xcnt = o; o = al(o + sizeof(int) * n * out_w);
  p->off_xk = o;   o = al(o + sizeof(int) * n * out_w * p->ks_w);
  p->off_ymin = o; o = al(o + sizeof(int) * n * out_h);
  p->off_ycnt = o; o = al(o + sizeof(int) * n * out_h);
  p->off_yk = o;   o = al(o + sizeof(int) * n * out_h * p->ks_h);
  p->bytes = o;
  return true;
}

// ---------------------------------------------------------------- random erasing
constexpr int kEraseChunk = 384;     // rectangles that travel as kernel arguments of one launch (8 bytes each)
struct EraseRows { unsigned tl[kEraseChunk], hw[kEraseChunk]; };   // top << 16 | left, h << 16 | w

// Workgroup (frame of the chunk, channel): fills the frame's rectangle in that channel plane, and nothing else.
template <typename D>
__global__ __launch_bounds__(kB) void erase_kernel(D* __restrict__ x, EraseRows rows, int64_t base, int H, int W, float v0,
                                                   float v1, float v2) {
  const int s = blockIdx.x, c = blockIdx.y;
  const int top = (int)(rows.tl[s] >> 16), left = (int)(rows.tl[s] & 0xffffu);
  const int h = (int)(rows.hw[s] >> 16), w = (int)(rows.hw[s] & 0xffffu);
  if (h == 0) return;
  const D v = from_f32<D>(c == 0 ? v0 : (c == 1 ? v1 : v2));
  D* o = x + (((base + s) * 3 + c) * H + top) * (int64_t)W + left;
  for (int i = threadIdx.x; i < h * w; i += kB) {
    const int ry = i / w, rx = i - ry * w;
    o[(int64_t)ry * W + rx] = v;
  }
}

}  // namespace

extern "C" {

size_t dvt_frames_preprocess_workspace_bytes(int64_t frames, int H0, int W0, int resize, int crop) {
  Plan p;
  if (frames < 0 || H0 <= 0 || W0 <= 0 || resize <= 0 || crop <= 0 || !make_plan(frames, H0, W0, resize, crop, &p))
    return 0;
  return p.bytes;
}

int dvt_frames_preprocess(const void* src, void* dst, int dst_dtype, int64_t frames, int H0, int W0, int resize,
                          int crop, const float* mean, const float* std, void* workspace, dvt_stream_t stream) {
  DVT_REQUIRE(src && dst && mean && std && workspace && frames >= 0 && H0 > 0 && W0 > 0 && resize > 0 && crop > 0,
              "dvt_frames_preprocess: bad arguments");
  Plan p;
  DVT_REQUIRE(make_plan(frames, H0, W0, resize, crop, &p),
              "dvt_frames_preprocess: crop %d exceeds the resized frame (%d x %d -> shorter side %d)", crop, H0, W0, resize);
  DVT_REQUIRE(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "dvt_frames_preprocess: zero std");
  if (frames == 0) return DVT_OK;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* xmin = (int*)(ws + p.off_xmin); int* xcnt = (int*)(ws + p.off_xcnt); int* xk = (int*)(ws + p.off_xk);
  int* ymin = (int*)(ws + p.off_ymin); int* ycnt = (int*)(ws + p.off_ycnt); int* yk = (int*)(ws + p.off_yk);
  unsigned char* tmp = (unsigned char*)(ws + p.off_tmp);
  hipLaunchKernelGGL(resample_coeff_kernel, dim3((unsigned)dvt_cdiv(p.w, 64)), dim3(64), 0, st, W0, p.w, p.ks_w, xmin,
                     xcnt, xk);
  hipLaunchKernelGGL(resample_coeff_kernel, dim3((unsigned)dvt_cdiv(p.h, 64)), dim3(64), 0, st, H0, p.h, p.ks_h, ymin,
                     ycnt, yk);
  DVT_LAUNCH_CHECK("dvt_frames_preprocess(coefficients)");
  hipLaunchKernelGGL(resample_h_kernel, dim3(grid_for(frames * H0 * crop)), dim3(kB), 0, st, (const unsigned char*)src,
                     tmp, xmin, xcnt, xk, p.ks_w, frames * H0, W0, crop, p.left);
  DVT_LAUNCH_CHECK("dvt_frames_preprocess(horizontal)");
  DVT_DISPATCH_DTYPE(dst_dtype, D, hipLaunchKernelGGL((resample_v_norm_kernel<D>), dim3(grid_for(frames * crop * crop)),
                                                      dim3(kB), 0, st, tmp, (D*)dst, ymin, ycnt, yk, p.ks_h, frames, H0,
                                                      crop, crop, p.top, mean[0], mean[1], mean[2], std[0], std[1],
                                                      std[2]));
  DVT_LAUNCH_CHECK("dvt_frames_preprocess(vertical)");
  return DVT_OK;
}

size_t dvt_frames_augment_workspace_bytes(int64_t samples, int H0, int W0, int out_h, int out_w) {
  AugPlan p;
  if (samples < 0 || H0 <= 0 || W0 <= 0 || out_h <= 0 || out_w <= 0 || !make_aug_plan(samples, H0, W0, out_h, out_w, &p))
    return 0;
  return p.bytes;
}

int dvt_frames_augment(const void* src, int64_t frames, int H0, int W0, const int32_t* table, int64_t samples, void* dst,
                       int dst_dtype, int out_h, int out_w, const float* mean, const float* std, void* workspace,
                       dvt_stream_t stream) {
  const bool u8 = dst_dtype == DVT_AUGMENT_U8_HWC;
  DVT_REQUIRE(src && dst && table && workspace && (u8 || (mean && std)) && frames >= 0 && samples >= 0 && H0 > 0 && W0 > 0 &&
                  out_h > 0 && out_w > 0,
              "dvt_frames_augment: bad arguments");
  DVT_REQUIRE(samples <= 65535 && (int64_t)H0 * W0 <= (1 << 28), "dvt_frames_augment: at most 65535 samples of 2^28 pixels");
  for (int64_t n = 0; n < samples; ++n) {
    const int32_t* r = table + n * kAugFields;
    DVT_REQUIRE(r[0] >= 0 && r[0] < frames, "dvt_frames_augment: table row %lld: src_index %d outside [0, %lld)",
                (long long)n, (int)r[0], (long long)frames);
    DVT_REQUIRE(r[3] >= 1 && r[4] >= 1 && r[1] >= 0 && r[2] >= 0 && r[3] <= H0 - r[1] && r[4] <= W0 - r[2],
                "dvt_frames_augment: table row %lld: window top %d left %d h %d w %d leaves the %d x %d frame",
                (long long)n, (int)r[1], (int)r[2], (int)r[3], (int)r[4], H0, W0);
    DVT_REQUIRE((r[5] == 0 || r[5] == 1) && (r[6] == 0 || r[6] == 1),
                "dvt_frames_augment: table row %lld: flips must be 0 or 1 (hflip %d, vflip %d)", (long long)n, (int)r[5],
                (int)r[6]);
  }
  if (!u8) DVT_REQUIRE(std[0] != 0.f && std[1] != 0.f && std[2] != 0.f, "dvt_frames_augment: zero std");
  AugPlan p;
  if (!make_aug_plan(samples, H0, W0, out_h, out_w, &p))
    DVT_UNSUPPORTED("dvt_frames_augment: one output row of a %d-row window resized to %d x %d needs %lld bytes of LDS, "
                    "more than the %d of a band",
                    H0, out_h, out_w, (long long)aug_lds_bytes(aug_rows_bound(H0, out_h, 1), out_w, 1, p.ks_h), kAugLds);
  if (samples == 0) return DVT_OK;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* tab = (int*)(ws + p.off_tab);
  int* xmin = (int*)(ws + p.off_xmin); int* xcnt = (int*)(ws + p.off_xcnt); int* xk = (int*)(ws + p.off_xk);
  int* ymin = (int*)(ws + p.off_ymin); int* ycnt = (int*)(ws + p.off_ycnt); int* yk = (int*)(ws + p.off_yk);
  for (int64_t base = 0; base < samples; base += kAugChunk) {
    const int count = (int)(samples - base < kAugChunk ? samples - base : kAugChunk);
    AugRows rows;
    memset(&rows, 0, sizeof(rows));
    memcpy(rows.v, table + base * kAugFields, sizeof(int) * kAugFields * count);
    hipLaunchKernelGGL(augment_coeff_kernel, dim3((unsigned)dvt_cdiv(out_w + out_h, 64), (unsigned)count), dim3(64), 0, st,
                       rows, (int)base, out_h, out_w, p.ks_h, p.ks_w, tab, xmin, xcnt, xk, ymin, ycnt, yk);
    DVT_LAUNCH_CHECK("dvt_frames_augment(coefficients)");
  }
  const dim3 grid((unsigned)dvt_cdiv(out_h, p.band), (unsigned)samples);
  AugNorm nm = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};
  if (!u8) nm = {{mean[0], mean[1], mean[2]}, {std[0], std[1], std[2]}};
#define DVT_AUG_LAUNCH(D)                                                                                              \
  hipLaunchKernelGGL((augment_band_kernel<D>), grid, dim3(kAugThreads), p.lds, st, (const unsigned char*)src, dst, tab, xmin, xcnt, \
                     xk, ymin, ycnt, yk, H0, W0, out_h, out_w, p.ks_h, p.ks_w, p.band, p.rmax, nm)
  if (u8) DVT_AUG_LAUNCH(U8Hwc);
  else DVT_DISPATCH_DTYPE(dst_dtype, D, DVT_AUG_LAUNCH(D));
#undef DVT_AUG_LAUNCH
  DVT_LAUNCH_CHECK("dvt_frames_augment(bands)");
  return DVT_OK;
}

int dvt_frames_erase(void* x, int dtype, int64_t frames, int H, int W, const int32_t* table, const float* value,
                     dvt_stream_t stream) {
  DVT_REQUIRE(x && table && value && frames >= 0 && H > 0 && W > 0 && H <= 65535 && W <= 65535,
              "dvt_frames_erase: bad arguments");
  for (int64_t f = 0; f < frames; ++f) {
    const int32_t* r = table + f * 4;
    DVT_REQUIRE(r[2] == 0 || (r[2] >= 1 && r[3] >= 1 && r[0] >= 0 && r[1] >= 0 && r[2] <= H - r[0] && r[3] <= W - r[1]),
                "dvt_frames_erase: table row %lld: rectangle top %d left %d h %d w %d leaves the %d x %d frame",
                (long long)f, (int)r[0], (int)r[1], (int)r[2], (int)r[3], H, W);
  }
  hipStream_t st = (hipStream_t)stream;
  for (int64_t base = 0; base < frames; base += kEraseChunk) {
    const int count = (int)(frames - base < kEraseChunk ? frames - base : kEraseChunk);
    EraseRows rows;
    memset(&rows, 0, sizeof(rows));
    bool any = false;
    for (int s = 0; s < count; ++s) {
      const int32_t* r = table + (base + s) * 4;
      if (r[2] == 0) continue;
      any = true;
      rows.tl[s] = (unsigned)r[0] << 16 | (unsigned)r[1];
      rows.hw[s] = (unsigned)r[2] << 16 | (unsigned)r[3];
    }
    if (!any) continue;
    DVT_DISPATCH_DTYPE(dtype, D, hipLaunchKernelGGL((erase_kernel<D>), dim3((unsigned)count, 3), dim3(kB), 0, st, (D*)x, rows,
                                                    base, H, W, value[0], value[1], value[2]));
    DVT_LAUNCH_CHECK("dvt_frames_erase");
  }
  return DVT_OK;
}

}  // extern "C"
