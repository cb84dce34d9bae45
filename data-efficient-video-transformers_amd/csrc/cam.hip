// cam.hip -- class-activation maps (Grad-CAM, Grad-CAM++, XGrad-CAM) of the R(2+1)D video encoder: what the reference does
// with the `pytorch_grad_cam` library at src/main.py:93-108 (GradCAM(model, [layer4[-1]]) on [N, 3, 12, 112, 112] chunks and
// show_cam_on_image on the frames).  That library does its arithmetic in numpy on the host; here it is three entry points:
//
//   dvt_cam_seed    logits [B][K] -> one-hot backward seed at category[b] or at the row's argmax (no host synchronisation);
//   dvt_cam_map     activation A and gradient G [N][P][C] (channels last, P = T' H' W') -> channel weights [N][C], the raw
//                   map relu(sum_c w A) [N][P] and the map scaled to [0, 1] per clip (the library's scale_cam_image);
//   dvt_cam_render  scaled [N][T'][H'][W'] -> trilinear mask [N][T][H][W] and, with frames, the JET overlay
//                   (show_cam_on_image) in the same launch.
//
// dvt_cam_map has two forms (dvt_cam_map_launches names the one a shape takes):
//   fused    one launch, one workgroup (8 waves) per clip: column sums over P (lane (cg, pr) owns 8 channels of every R-th
//            row, 16-byte loads; the R partial rows meet in LDS and are summed in row order), the weights stay in LDS, the map
//            re-reads A (L2), the row extrema and the scaling follow from the raw row held in LDS.  Taken where a workgroup
//            can own a clip's block: P <= DVT_CAM_FUSED_MAX_P, P * C <= DVT_CAM_FUSED_MAX_ELEMS (layer 4 at 98 x 512, layer 3
//            at 588 x 256).
//   general  three launches: weights (a workgroup per clip and 64-channel slab, the same code on a slab), map + extrema of
//            256-row chunks (weights from global memory, chunk extrema to the workspace), scaling in place.
// Every sum is fp32 in a fixed order, the extrema are order-free, nothing is atomic: identical calls give bitwise-equal
// results.  All pointers are the caller's; everything runs on the caller's stream.
#include "common.h"
#include "cam_scale.h"          // block_extrema and the scaling itself (shared with attn_rollout.hip)

#include <cmath>

namespace {

constexpr int kNT = 512;                          // threads of a map workgroup
constexpr int kWaves = kNT / 64;
constexpr int kMaxC = DVT_CAM_MAX_C;              // weights of a clip in LDS
constexpr int kSlab = 64;                         // channels per workgroup of the general form's weight launch
constexpr int kChunk = 256;                       // rows per workgroup of the general form's map and scaling launches
static_assert(DVT_CAM_FUSED_MAX_P % kChunk == 0 && kMaxC % 8 == 0 && kMaxC / 8 <= kNT, "map shapes");

struct MapLds {
  float part[kNT * 8];                            // [R][cw] partial column sums, R = kNT / (cw / 8)
  float wv[kMaxC];
  float sv[kMaxC];
  float red[2 * kWaves];
};

// sum of the R partial rows, in row order -> dst[0 .. cw)
__device__ __forceinline__ void col_reduce(MapLds& s, const float (&acc)[8], bool active, int cg, int pr, int cw, int R,
                                           float* dst) {
  if (active) {
#pragma unroll
    for (int i = 0; i < 8; ++i) s.part[pr * cw + cg * 8 + i] = acc[i];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < cw; c += kNT) {
    float t = 0.f;
    for (int r = 0; r < R; ++r) t += s.part[r * cw + c];
    dst[c] = t;
  }
  __syncthreads();
}

// channel weights of channels [0, cw) of one clip -> s.wv.  A, G point at the clip's first row (and the slab's first
// channel); ld is the row stride C.
template <typename T>
__device__ __forceinline__ void clip_weights(const T* __restrict__ A, const T* __restrict__ G, int P, int ld, int cw,
                                             int method, MapLds& s) {
  const int tid = threadIdx.x, cgw = cw >> 3, R = kNT / cgw, cg = tid % cgw, pr = tid / cgw;
  const bool active = pr < R;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float a[8], g[8];
  if (method == DVT_CAM_GRADCAM) {
    if (active)
      for (int p = pr; p < P; p += R) {
        load8<T>(G + (int64_t)p * ld + cg * 8, g);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += g[i];
      }
    col_reduce(s, acc, active, cg, pr, cw, R, s.wv);
    for (int c = tid; c < cw; c += kNT) s.wv[c] = s.wv[c] / (float)P;
  } else if (method == DVT_CAM_XGRADCAM) {
    float acc2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (active)
      for (int p = pr; p < P; p += R) {
        load8<T>(G + (int64_t)p * ld + cg * 8, g);
        load8<T>(A + (int64_t)p * ld + cg * 8, a);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          acc[i] = fmaf(g[i], a[i], acc[i]);
          acc2[i] += a[i];
        }
      }
    col_reduce(s, acc, active, cg, pr, cw, R, s.wv);
    col_reduce(s, acc2, active, cg, pr, cw, R, s.sv);
    for (int c = tid; c < cw; c += kNT) s.wv[c] = s.wv[c] / (s.sv[c] + 1e-7f);
  } else {                                        // Grad-CAM++
    if (active)
      for (int p = pr; p < P; p += R) {
        load8<T>(A + (int64_t)p * ld + cg * 8, a);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += a[i];
      }
    col_reduce(s, acc, active, cg, pr, cw, R, s.sv);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    if (active) {
      float S[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) S[i] = s.sv[cg * 8 + i];
      for (int p = pr; p < P; p += R) {
        load8<T>(G + (int64_t)p * ld + cg * 8, g);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          // max(G, 0) * a with a = G^2 / (2 G^2 + S G^3 + 1e-6): only G > 0 contributes (a is 0 where G == 0, max(G, 0) is
          // 0 where G < 0), so the quotient is formed there alone
          const float g2 = g[i] * g[i], den = 2.f * g2 + S[i] * (g2 * g[i]) + 1e-6f;
          acc[i] += g[i] > 0.f ? g[i] * (g2 / den) : 0.f;
        }
      }
    }
    col_reduce(s, acc, active, cg, pr, cw, R, s.wv);
  }
  __syncthreads();
}

// raw[p - p0] = max(sum_c w[c] A[p][c], 0) for rows p0 .. p1 - 1 of one clip (A: the clip's first row).  A group of
// g = min(64, pow2 >= C / 8) lanes owns a row; the butterfly leaves the same total in each of them.
template <typename T>
__device__ __forceinline__ void clip_rows(const T* __restrict__ A, int C, int p0, int p1, MapLds& s, float* rawv) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, cgs = C >> 3;
  int g = 1;
  while (g < cgs && g < 64) g <<= 1;
  const int rpw = 64 / g, sub = lane / g, cg0 = lane & (g - 1);
  for (int pb = p0; pb < p1; pb += kWaves * rpw) {
    const int p = pb + wid * rpw + sub;
    float v = 0.f;
    if (p < p1)
      for (int cg = cg0; cg < cgs; cg += g) {
        float a[8];
        load8<T>(A + (int64_t)p * C + cg * 8, a);
#pragma unroll
        for (int i = 0; i < 8; ++i) v = fmaf(s.wv[cg * 8 + i], a[i], v);
      }
    for (int o = g >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (p < p1 && cg0 == 0) rawv[p - p0] = fmaxf(v, 0.f);
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(kNT) void cam_map_fused_kernel(const T* __restrict__ A, const T* __restrict__ G, int P, int C,
                                                            int method, float* __restrict__ weights, float* __restrict__ raw,
                                                            float* __restrict__ scaled) {
  __shared__ __attribute__((aligned(16))) MapLds s;
  __shared__ float rawv[DVT_CAM_FUSED_MAX_P];
  const int64_t n = blockIdx.x, base = n * P * (int64_t)C;
  clip_weights<T>(A + base, G + base, P, C, C, method, s);
  if (weights)
    for (int c = threadIdx.x; c < C; c += kNT) weights[n * C + c] = s.wv[c];
  clip_rows<T>(A + base, C, 0, P, s, rawv);
  float mn = INFINITY, mx = -INFINITY;
  for (int p = threadIdx.x; p < P; p += kNT) { mn = fminf(mn, rawv[p]); mx = fmaxf(mx, rawv[p]); }
  block_extrema(mn, mx, s.red, kWaves);
  const float den = cam_scale_den(mn, mx);
  for (int p = threadIdx.x; p < P; p += kNT) {
    const float r = rawv[p];
    if (raw) raw[n * P + p] = r;
    scaled[n * P + p] = cam_scale_value(r, mn, den);
  }
}

// general form, launch 1: grid (N, slabs of kSlab channels)
template <typename T>
__global__ __launch_bounds__(kNT) void cam_weights_kernel(const T* __restrict__ A, const T* __restrict__ G, int P, int C,
                                                          int method, float* __restrict__ weights) {
  __shared__ __attribute__((aligned(16))) MapLds s;
  const int64_t n = blockIdx.x, base = n * P * (int64_t)C;
  const int c0 = blockIdx.y * kSlab, cw = min(kSlab, C - c0);
  clip_weights<T>(A + base + c0, G + base + c0, P, C, cw, method, s);
  for (int c = threadIdx.x; c < cw; c += kNT) weights[n * C + c0 + c] = s.wv[c];
}

// general form, launch 2: grid (N, chunks of kChunk rows): raw rows -> `scaled` (and `raw`), chunk extrema -> ext
template <typename T>
__global__ __launch_bounds__(kNT) void cam_rows_kernel(const T* __restrict__ A, const float* __restrict__ weights, int P,
                                                       int C, float* __restrict__ raw, float* __restrict__ scaled,
                                                       float* __restrict__ ext) {
  __shared__ __attribute__((aligned(16))) MapLds s;
  __shared__ float rawv[kChunk];
  const int64_t n = blockIdx.x;
  const int p0 = blockIdx.y * kChunk, p1 = min(P, p0 + kChunk);
  for (int c = threadIdx.x; c < C; c += kNT) s.wv[c] = weights[n * C + c];
  __syncthreads();
  clip_rows<T>(A + n * P * (int64_t)C, C, p0, p1, s, rawv);
  float mn = INFINITY, mx = -INFINITY;
  for (int p = p0 + threadIdx.x; p < p1; p += kNT) {
    const float r = rawv[p - p0];
    mn = fminf(mn, r); mx = fmaxf(mx, r);
    if (raw) raw[n * P + p] = r;
    scaled[n * P + p] = r;
  }
  block_extrema(mn, mx, s.red, kWaves);
  if (threadIdx.x == 0) {
    ext[(n * gridDim.y + blockIdx.y) * 2] = mn;
    ext[(n * gridDim.y + blockIdx.y) * 2 + 1] = mx;
  }
}

// general form, launch 3: grid (N, chunks), kChunk threads: the clip's extrema from the chunks', then the scaling in place
__global__ __launch_bounds__(kChunk) void cam_scale_kernel(const float* __restrict__ ext, int P, float* __restrict__ scaled) {
  __shared__ float red[2 * (kChunk / 64)];
  const int64_t n = blockIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  for (int ch = threadIdx.x; ch < (int)gridDim.y; ch += kChunk) {
    mn = fminf(mn, ext[(n * gridDim.y + ch) * 2]);
    mx = fmaxf(mx, ext[(n * gridDim.y + ch) * 2 + 1]);
  }
  block_extrema(mn, mx, red, kChunk / 64);
  const float den = cam_scale_den(mn, mx);
  const int p = blockIdx.y * kChunk + threadIdx.x;
  if (p < P) scaled[n * P + p] = cam_scale_value(scaled[n * P + p], mn, den);
}

inline bool fused_form(int64_t P, int64_t C) { return P <= DVT_CAM_FUSED_MAX_P && P * C <= DVT_CAM_FUSED_MAX_ELEMS; }
inline int64_t chunks_of(int64_t P) { return dvt_cdiv(P, kChunk); }

// ---------------------------------------------------------------- seed
// a wave per row: lane-strided scan with a strict compare (the lowest index of a lane's maximum), then a butterfly whose
// ties go to the lower index -- numpy.argmax's rule
template <typename T>
__global__ __launch_bounds__(256) void cam_seed_kernel(const T* __restrict__ logits, const int32_t* __restrict__ category,
                                                       T* __restrict__ seed, int64_t B, int K) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  int cat = category ? category[row] : -1;
  if (cat < 0) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int k = lane; k < K; k += 64) {
      const float v = to_f32<T>(logits[row * K + k]);
      if (v > best || bi == 0x7fffffff) { best = v; bi = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
    }
    cat = __shfl(bi, 0, 64);                      // one answer for the row, whatever a NaN did to the compares
  }
  for (int k = lane; k < K; k += 64) seed[row * K + k] = from_f32<T>(k == cat ? 1.f : 0.f);
}

// ---------------------------------------------------------------- render
struct Axis { int i0, i1; float l0, l1; };
// half-pixel centres: src = (o + 0.5) I / O - 0.5 clamped to [0, I - 1]; taps floor(src) and min(floor(src) + 1, I - 1)
__device__ __forceinline__ Axis axis_src(int o, int I, float scale) {
  const float src = fminf(fmaxf((o + 0.5f) * scale - 0.5f, 0.f), (float)(I - 1));
  Axis a;
  a.i0 = (int)src;
  a.i1 = min(a.i0 + 1, I - 1);
  a.l1 = src - (float)a.i0;
  a.l0 = 1.f - a.l1;
  return a;
}

template <typename F> __device__ __forceinline__ float frame_value(F v);
template <> __device__ __forceinline__ float frame_value<uint8_t>(uint8_t v) { return (float)v / 255.f; }
template <> __device__ __forceinline__ float frame_value<float>(float v) { return v; }

// One workgroup per output frame (n, t).  With frames the blend is evaluated twice -- once for the frame's maximum, once to
// write -- and never stored.
template <typename F>
__global__ __launch_bounds__(256) void cam_render_kernel(const float* __restrict__ src, int Ti, int Hi, int Wi, int T, int H,
                                                         int W, float st, float sh, float sw, float* __restrict__ mask,
                                                         const F* __restrict__ frames, const uint8_t* __restrict__ jet,
                                                         uint8_t* __restrict__ overlay, float image_weight, int use_rgb) {
  __shared__ float jt[768];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int64_t frame = blockIdx.x, n = frame / T;
  const int t = (int)(frame % T), HW = H * W;
  const Axis at = axis_src(t, Ti, st);
  const float* __restrict__ s0 = src + (n * Ti + at.i0) * (int64_t)(Hi * Wi);
  const float* __restrict__ s1 = src + (n * Ti + at.i1) * (int64_t)(Hi * Wi);
  auto sample = [&](int i) {
    const Axis ah = axis_src(i / W, Hi, sh), aw = axis_src(i % W, Wi, sw);
    const float f0 = ah.l0 * (aw.l0 * s0[ah.i0 * Wi + aw.i0] + aw.l1 * s0[ah.i0 * Wi + aw.i1]) +
                     ah.l1 * (aw.l0 * s0[ah.i1 * Wi + aw.i0] + aw.l1 * s0[ah.i1 * Wi + aw.i1]);
    const float f1 = ah.l0 * (aw.l0 * s1[ah.i0 * Wi + aw.i0] + aw.l1 * s1[ah.i0 * Wi + aw.i1]) +
                     ah.l1 * (aw.l0 * s1[ah.i1 * Wi + aw.i0] + aw.l1 * s1[ah.i1 * Wi + aw.i1]);
    return at.l0 * f0 + at.l1 * f1;
  };
  if (frames == nullptr) {
    for (int i = tid; i < HW; i += 256) mask[frame * HW + i] = sample(i);
    return;
  }
  for (int i = tid; i < 768; i += 256) jt[i] = (float)jet[i] / 255.f;
  __syncthreads();
  const F* __restrict__ img = frames + frame * HW * 3;
  // show_cam_on_image: heat = JET[(int)(255 mask)] / 255, blend = (1 - image_weight) heat + image_weight img
  auto blend = [&](float m, int i, float (&b)[3]) {
    const int idx = (int)fminf(fmaxf(255.f * m, 0.f), 255.f);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      b[ch] = (1.f - image_weight) * jt[idx * 3 + (use_rgb ? ch : 2 - ch)] + image_weight * frame_value<F>(img[(int64_t)i * 3 + ch]);
  };
  float mx = 0.f, b[3];
  for (int i = tid; i < HW; i += 256) {
    const float m = sample(i);
    if (mask) mask[frame * HW + i] = m;
    blend(m, i, b);
    mx = fmaxf(mx, fmaxf(b[0], fmaxf(b[1], b[2])));
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  uint8_t* __restrict__ dst = overlay + frame * HW * 3;
  for (int i = tid; i < HW; i += 256) {
    blend(sample(i), i, b);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      dst[(int64_t)i * 3 + ch] = mx > 0.f ? (uint8_t)(int)fminf(fmaxf(255.f * b[ch] / mx, 0.f), 255.f) : (uint8_t)0;
  }
}

}  // namespace

extern "C" {

int dvt_cam_seed(const void* logits, const int32_t* category, void* seed, int64_t B, int64_t K, int dtype,
                 dvt_stream_t stream) {
  DVT_REQUIRE(B >= 0 && K > 0, "dvt_cam_seed: bad shape [%lld][%lld]", (long long)B, (long long)K);
  DVT_REQUIRE(dtype == DVT_F32 || dvt_is_16bit(dtype), "dvt_cam_seed: dtype %d not supported", dtype);
  if (K >= ((int64_t)1 << 31) - 1 || B >= ((int64_t)1 << 32))
    DVT_UNSUPPORTED("dvt_cam_seed: [%lld][%lld] logits: split the batch", (long long)B, (long long)K);
  if (B == 0) return DVT_OK;
  DVT_REQUIRE(logits && seed, "dvt_cam_seed: null logits / seed");
  DVT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((cam_seed_kernel<T>), dim3((unsigned)dvt_cdiv(B, 4)), dim3(256), 0,
                                                  (hipStream_t)stream, (const T*)logits, category, (T*)seed, B, (int)K));
  DVT_LAUNCH_CHECK("dvt_cam_seed");
  return DVT_OK;
}

int dvt_cam_map_launches(int64_t P, int64_t C) { return (P <= 0 || C <= 0) ? 0 : (fused_form(P, C) ? 1 : 3); }

size_t dvt_cam_map_workspace_bytes(int64_t N, int64_t P, int64_t C) {
  if (N <= 0 || P <= 0 || C <= 0 || fused_form(P, C)) return 0;
  return (size_t)(N * C + 2 * N * chunks_of(P)) * sizeof(float);
}

int dvt_cam_map(const void* A, const void* G, int64_t N, int64_t P, int64_t C, int dtype, int method, float* weights,
                float* raw, float* scaled, void* workspace, size_t workspace_bytes, dvt_stream_t stream) {
  DVT_REQUIRE(N >= 0 && P > 0 && C > 0, "dvt_cam_map: bad shape [%lld][%lld][%lld]", (long long)N, (long long)P, (long long)C);
  DVT_REQUIRE(C % 8 == 0, "dvt_cam_map: C = %lld is not a multiple of 8 (16-byte channel loads)", (long long)C);
  DVT_REQUIRE(method == DVT_CAM_GRADCAM || method == DVT_CAM_GRADCAMPP || method == DVT_CAM_XGRADCAM,
              "dvt_cam_map: unknown method %d", method);
  DVT_REQUIRE(dtype == DVT_F32 || dvt_is_16bit(dtype), "dvt_cam_map: dtype %d not supported", dtype);
  const int64_t chunks = chunks_of(P);
  if (C > kMaxC || P >= ((int64_t)1 << 31) - kChunk || chunks > 65535 || N >= ((int64_t)1 << 31))
    DVT_UNSUPPORTED("dvt_cam_map: [%lld][%lld][%lld]: at most %d channels and 65535 x %d positions per clip", (long long)N,
                    (long long)P, (long long)C, kMaxC, kChunk);
  if (N == 0) return DVT_OK;
  DVT_REQUIRE(A && G && scaled, "dvt_cam_map: null A / G / scaled");
  DVT_REQUIRE(dvt_aligned16(A) && dvt_aligned16(G), "dvt_cam_map: A and G must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (fused_form(P, C)) {
    DVT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((cam_map_fused_kernel<T>), dim3((unsigned)N), dim3(kNT), 0, st, (const T*)A,
                                                    (const T*)G, (int)P, (int)C, method, weights, raw, scaled));
    DVT_LAUNCH_CHECK("dvt_cam_map (fused)");
    return DVT_OK;
  }
  DVT_REQUIRE(workspace && workspace_bytes >= dvt_cam_map_workspace_bytes(N, P, C),
              "dvt_cam_map: the general form needs a workspace of dvt_cam_map_workspace_bytes");
  float* ws = (float*)workspace;
  float* w = weights ? weights : ws;
  float* ext = ws + N * C;
  const dim3 gw((unsigned)N, (unsigned)dvt_cdiv(C, kSlab)), gr((unsigned)N, (unsigned)chunks);
  DVT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((cam_weights_kernel<T>), gw, dim3(kNT), 0, st, (const T*)A, (const T*)G,
                                                  (int)P, (int)C, method, w));
  DVT_LAUNCH_CHECK("dvt_cam_map (weights)");
  DVT_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((cam_rows_kernel<T>), gr, dim3(kNT), 0, st, (const T*)A, (const float*)w,
                                                  (int)P, (int)C, raw, scaled, ext));
  DVT_LAUNCH_CHECK("dvt_cam_map (rows)");
  hipLaunchKernelGGL(cam_scale_kernel, gr, dim3(kChunk), 0, st, (const float*)ext, (int)P, scaled);
  DVT_LAUNCH_CHECK("dvt_cam_map (scale)");
  return DVT_OK;
}

int dvt_cam_jet_table(uint8_t* dst, size_t bytes) {
  DVT_REQUIRE(dst && bytes >= 768, "dvt_cam_jet_table: needs a host buffer of 768 bytes");
  for (int i = 0; i < 256; ++i) {
    const double x = i / 255.0;
    const double v[3] = {1.5 - std::fabs(4.0 * x - 3.0), 1.5 - std::fabs(4.0 * x - 2.0), 1.5 - std::fabs(4.0 * x - 1.0)};
    for (int ch = 0; ch < 3; ++ch) dst[i * 3 + ch] = (uint8_t)std::floor(255.0 * std::fmin(std::fmax(v[ch], 0.0), 1.0) + 0.5);
  }
  return DVT_OK;
}

int dvt_cam_render(const float* scaled, int64_t N, int Ti, int Hi, int Wi, int T, int H, int W, float* mask,
                   const void* frames, int frames_f32, const uint8_t* jet, uint8_t* overlay, float image_weight, int use_rgb,
                   dvt_stream_t stream) {
  DVT_REQUIRE(N >= 0 && Ti > 0 && Hi > 0 && Wi > 0 && T > 0 && H > 0 && W > 0, "dvt_cam_render: bad shape");
  DVT_REQUIRE(image_weight >= 0.f && image_weight <= 1.f, "dvt_cam_render: image_weight %g is outside [0, 1]", (double)image_weight);
  if ((int64_t)Hi * Wi >= ((int64_t)1 << 24) || (int64_t)H * W >= ((int64_t)1 << 28) || N * T >= ((int64_t)1 << 31))
    DVT_UNSUPPORTED("dvt_cam_render: %lld clips of %d x %d x %d: split the batch", (long long)N, T, H, W);
  if (N == 0) return DVT_OK;
  DVT_REQUIRE(scaled, "dvt_cam_render: null scaled");
  DVT_REQUIRE(frames ? (jet && overlay) : (mask != nullptr),
              "dvt_cam_render: frames need jet and overlay; without frames a mask must be asked for");
  const float st = (float)Ti / (float)T, sh = (float)Hi / (float)H, sw = (float)Wi / (float)W;
  const dim3 grid((unsigned)(N * T));
  if (frames && frames_f32)
    hipLaunchKernelGGL((cam_render_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, scaled, Ti, Hi, Wi, T, H, W, st, sh,
                       sw, mask, (const float*)frames, jet, overlay, image_weight, use_rgb);
  else
    hipLaunchKernelGGL((cam_render_kernel<uint8_t>), grid, dim3(256), 0, (hipStream_t)stream, scaled, Ti, Hi, Wi, T, H, W, st,
                       sh, sw, mask, (const uint8_t*)frames, jet, overlay, image_weight, use_rgb);
  DVT_LAUNCH_CHECK("dvt_cam_render");
  return DVT_OK;
}

}  // extern "C"
