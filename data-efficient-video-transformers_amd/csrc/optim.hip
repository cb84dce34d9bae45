// optim.hip -- every optimizer step: AdamW (host step, device step, fused flat-buffer step with mirror, loss-scaled),
// torch.optim.Adam with coupled decay, SGD, Adagrad -- streaming kernels over fp32 master weights -- LARS, whose
// per-tensor norms make it a reduction over a table of segments followed by the scaled momentum update, and the global
// gradient norm with its in-place clip over the same kind of table.
//
// The Adam update, its bias correction, the step-counter ticket and the mirror dispatch are each stated once, in
// adam_update.h (shared with optim_groups.hip); the kernels differ only in their launch contract (scalar grid-stride or
// four elements per thread, mirror, ticket, the found_inf early-out).
#include "adam_update.h"
#include <type_traits>

namespace {

constexpr int kBlock = 256;

// ------------------------------------------------------------------ AdamW
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                             float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                             float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt) {
  const AdamCoef c = adam_coef(lr, b1, b2, eps, wd, BiasCorr{bc1, bc2_sqrt});
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam_update<false>(pi, g[i], mi, vi, c);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
}

__global__ void adamw_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                 float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                 float b1, float b2, float eps, float wd,
                                 const int64_t* __restrict__ step_dev, const uint8_t* __restrict__ skip) {
  const AdamCoef c = adam_coef(lr, b1, b2, eps, wd, bias_corr_dev(b1, b2, step_dev[0]));
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (skip && skip[i >> 6]) continue;               // parameter without a gradient this step: untouched (torch: grad None)
    float pi = p[i], mi = m[i], vi = v[i];
    adam_update<false>(pi, g[i], mi, vi, c);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
}

__global__ void inc_step_kernel(int64_t* step_dev) { step_dev[0] += 1; }

// The flat-buffer step of the training loop in ONE launch: AdamW on four elements per thread (16-byte accesses), the
// 16-bit mirror of the updated weights that the next step's GEMMs read (M = bf16 / f16; float: no mirror), and the step
// counter (publish_step).
template <typename M>
__global__ __launch_bounds__(256) void adamw_fused_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                          float b1, float b2, float eps, float wd, int64_t* step_dev,
                                                          const uint8_t* __restrict__ skip, M* __restrict__ mirror) {
  const int64_t steps = step_dev[0];
  const AdamCoef c = adam_coef(lr, b1, b2, eps, wd, bias_corr_dev(b1, b2, steps));
  const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const int64_t e = i << 2;
    f32x4 pv = *reinterpret_cast<const f32x4*>(p + e);
    if (!(skip && skip[e >> 6])) {                     // parameter without a gradient this step: untouched (torch: grad None)
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + e);
      f32x4 mv = *reinterpret_cast<const f32x4*>(m + e), vv = *reinterpret_cast<const f32x4*>(v + e);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pi = pv[k], mi = mv[k], vi = vv[k];
        adam_update<false>(pi, gv[k], mi, vi, c);
        pv[k] = pi; mv[k] = mi; vv[k] = vi;
      }
      *reinterpret_cast<f32x4*>(p + e) = pv;
      *reinterpret_cast<f32x4*>(m + e) = mv;
      *reinterpret_cast<f32x4*>(v + e) = vv;
    }
    if (!std::is_same<M, float>::value) {
      typedef M m4 __attribute__((ext_vector_type(4)));
      m4 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (M)pv[k];
      *reinterpret_cast<m4*>(mirror + e) = o;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {       // tail of a buffer whose length is not a multiple of 4
    const int64_t i = (n4 << 2) + threadIdx.x;
    float pi = p[i];
    if (!(skip && skip[i >> 6])) {
      float mi = m[i], vi = v[i];
      adam_update<false>(pi, g[i], mi, vi, c);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
    if (!std::is_same<M, float>::value) mirror[i] = (M)pi;
  }
  publish_step(step_dev, steps);
}

// torch.optim.Adam (amsgrad off, coupled decay) over a flat buffer, one launch: lr from the device; step counter and
// mirror as adamw_fused_kernel.
template <typename M>
__global__ __launch_bounds__(256) void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                       const float* __restrict__ lr_dev, float b1, float b2, float eps,
                                                       float wd, int64_t* step_dev, const uint8_t* __restrict__ skip,
                                                       M* __restrict__ mirror) {
  const int64_t steps = step_dev[0];
  const BiasCorr bc = bias_corr_dev(b1, b2, steps);   // the counter is read before the rate
  const AdamCoef c = adam_coef(lr_dev[0], b1, b2, eps, wd, bc);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float pi = p[i];
    if (!(skip && skip[i >> 6])) {                     // parameter without a gradient this step: untouched (torch: grad None)
      float mi = m[i], vi = v[i];
      adam_update<true>(pi, g[i], mi, vi, c);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
    if (!std::is_same<M, float>::value) mirror[i] = (M)pi;
  }
  publish_step(step_dev, steps);
}

// ---- fp16 loss scaling (BASELINE configs[4]: "fp16 + loss scaling"), all state on the device so the step stays
// hipGraph-capturable: scale[0], found_inf[0] (int32), good_steps[0] (int32), loss_grad[0] = scale * base.
__global__ void check_finite_kernel(const float* __restrict__ g, int64_t n, int* __restrict__ found_inf) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = g[i];
    bad |= !(fabsf(v) <= 3.402823466e38f);          // inf or nan
  }
  if (bad) atomicOr(found_inf, 1);
}

__global__ void adamw_scaled_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                    float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                                    const int64_t* __restrict__ step_dev, const float* __restrict__ scale,
                                    const int* __restrict__ found_inf, const uint8_t* __restrict__ skip) {
  if (found_inf[0]) return;                           // overflow: skip the whole update
  const float inv_scale = 1.0f / scale[0];
  const AdamCoef c = adam_coef(lr, b1, b2, eps, wd, bias_corr_dev(b1, b2, step_dev[0]));
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (skip && skip[i >> 6]) continue;
    float pi = p[i], mi = m[i], vi = v[i];
    adam_update<false>(pi, g[i] * inv_scale, mi, vi, c);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
}

// after the step: step counter, dynamic scale (torch.cuda.amp.GradScaler rule), flag reset, next loss gradient
__global__ void loss_scale_update_kernel(int64_t* step_dev, float* scale, int* found_inf, int* good_steps,
                                         int growth_interval, float growth, float backoff, float* loss_grad,
                                         float base) {
  if (found_inf[0]) {
    scale[0] *= backoff;
    good_steps[0] = 0;
  } else {
    step_dev[0] += 1;
    if (++good_steps[0] >= growth_interval) { scale[0] *= growth; good_steps[0] = 0; }
  }
  found_inf[0] = 0;
  loss_grad[0] = scale[0] * base;
}

// torch.optim.SGD (dampening 0, no nesterov): d = g + wd p; buf = mu buf + d; p -= lr buf   (buf starts at 0,
// which reproduces torch's "first step: buf = d" rule).  mu == 0: plain p -= lr d, buf untouched.
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                           int64_t n, float lr, float mu, float wd, const uint8_t* __restrict__ skip) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (skip && skip[i >> 6]) continue;
    const float pi = p[i];
    float d = fmaf(wd, pi, g[i]);
    if (mu != 0.f) {
      d = fmaf(mu, buf[i], d);
      buf[i] = d;
    }
    p[i] = pi - lr * d;
  }
}

// torch.optim.Adagrad: d = g + wd p; sum += d^2; p -= clr d / (sqrt(sum) + eps)
__global__ void adagrad_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sum,
                               int64_t n, float clr, float eps, float wd, const uint8_t* __restrict__ skip) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (skip && skip[i >> 6]) continue;
    const float pi = p[i];
    const float d = fmaf(wd, pi, g[i]);
    const float si = fmaf(d, d, sum[i]);
    sum[i] = si;
    p[i] = pi - clr * (d / (sqrtf(si) + eps));
  }
}

// ------------------------------------------------------------------ LARS (pl_bolts.optimizers.lars.LARS.step)
// A device table of segments (dvt_lars_seg, one per tensor with a gradient), cut into chunks of kLarsChunk elements: a
// chunk lies in one segment, segment s owns the chunks [chunk_begin[s], chunk_begin[s] + cdiv(numel, kLarsChunk)), and one
// block works on one chunk in both kernels.  Inside a chunk thread t owns the quads t, t + 256, ... (elements 4q .. 4q + 3),
// read as one 16-byte access when every pointer of the segment allows it and as four scalars otherwise; the last
// len & 3 elements go to the threads 0 .. 2.  Ownership, and with it the order of every sum, depends on numel alone.
constexpr int kLarsChunk = 8192;
constexpr int kLarsBlock = 256;

// The segment that owns chunk `c`: the last one whose chunk_begin is <= c (chunk_begin ascends strictly).
__device__ __forceinline__ int lars_find_segment(const dvt_lars_seg* __restrict__ table, int n, int64_t c) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].chunk_begin <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Elements of the chunk that begins at `start`.  A block past the table's last chunk (the caller's `chunks` larger than
// the table's own total) resolves to the last segment with start >= numel: it gets 0, so it reads and writes no element.
__device__ __forceinline__ int lars_chunk_len(int64_t numel, int64_t start) {
  const int64_t left = numel - start;
  return left <= 0 ? 0 : (int)(left < kLarsChunk ? left : kLarsChunk);
}

// The table holds device addresses: they are read as global memory (a generic pointer would compile to FLAT accesses).
#define DVT_GLOBAL __attribute__((address_space(1)))
typedef DVT_GLOBAL float gfloat;
template <typename T>
__device__ __forceinline__ DVT_GLOBAL T* lars_global(const void* p) { return (DVT_GLOBAL T*)(uintptr_t)p; }

template <bool kVec>
__device__ __forceinline__ f32x4 lars_load4(const gfloat* p) {
  if (kVec) return *(const DVT_GLOBAL f32x4*)p;
  return f32x4{p[0], p[1], p[2], p[3]};
}

template <bool kVec>
__device__ __forceinline__ void lars_store4(gfloat* p, f32x4 v) {
  if (kVec) *(DVT_GLOBAL f32x4*)p = v;
  else { p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3]; }
}

// Sum of (a, b) over the block in a fixed order: the xor butterfly inside each wave, then the waves in index order.
// Every thread returns the same pair.
__device__ __forceinline__ f32x2 lars_block_sum(float a, float b) {
  __shared__ float red[2][kLarsBlock / DVT_WAVE];
#pragma unroll
  for (int off = DVT_WAVE / 2; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, DVT_WAVE);
    b += __shfl_xor(b, off, DVT_WAVE);
  }
  __syncthreads();                                      // the previous use of `red` is over
  if ((threadIdx.x & (DVT_WAVE - 1)) == 0) {
    red[0][threadIdx.x / DVT_WAVE] = a;
    red[1][threadIdx.x / DVT_WAVE] = b;
  }
  __syncthreads();
  a = red[0][0]; b = red[1][0];
#pragma unroll
  for (int w = 1; w < kLarsBlock / DVT_WAVE; ++w) { a += red[0][w]; b += red[1][w]; }
  return f32x2{a, b};
}

template <bool kVec>
__device__ __forceinline__ void lars_chunk_sumsq(const gfloat* __restrict__ p, const gfloat* __restrict__ g, int len,
                                                 float& sp, float& sg) {
  const int n4 = len >> 2;
  for (int q = threadIdx.x; q < n4; q += kLarsBlock) {
    const f32x4 pv = lars_load4<kVec>(p + 4 * q), gv = lars_load4<kVec>(g + 4 * q);
#pragma unroll
    for (int k = 0; k < 4; ++k) { sp = fmaf(pv[k], pv[k], sp); sg = fmaf(gv[k], gv[k], sg); }
  }
  if ((int)threadIdx.x < (len & 3)) {
    const float pi = p[4 * n4 + threadIdx.x], gi = g[4 * n4 + threadIdx.x];
    sp = fmaf(pi, pi, sp); sg = fmaf(gi, gi, sg);
  }
}

// partial[c] = (sum p^2, sum g^2) of chunk c.
__global__ __launch_bounds__(kLarsBlock) void lars_norms_kernel(const dvt_lars_seg* __restrict__ table, int n,
                                                                f32x2* __restrict__ partial) {
  const int64_t c = blockIdx.x;
  const dvt_lars_seg s = table[lars_find_segment(table, n, c)];
  const int64_t start = (c - s.chunk_begin) * kLarsChunk;
  const int len = lars_chunk_len(s.numel, start);
  const gfloat* p = lars_global<float>(s.param) + start;
  const gfloat* g = lars_global<float>(s.grad) + start;
  float sp = 0.f, sg = 0.f;
  if ((((uintptr_t)p | (uintptr_t)g) & 15u) == 0) lars_chunk_sumsq<true>(p, g, len, sp, sg);
  else lars_chunk_sumsq<false>(p, g, len, sp, sg);
  const f32x2 r = lars_block_sum(sp, sg);
  if (threadIdx.x == 0) partial[c] = r;
}

// (sum p^2, sum g^2) of a whole segment from its chunks' partials: thread t adds the partials t, t + 256, ... in that
// order, lars_block_sum adds the threads.  The one statement of this sum: dvt_lars_sumsq reports what dvt_lars_step uses.
__device__ __forceinline__ f32x2 lars_segment_sumsq(const f32x2* __restrict__ partial, const dvt_lars_seg& s) {
  const int64_t chunks = (s.numel + kLarsChunk - 1) / kLarsChunk;
  float sp = 0.f, sg = 0.f;
  for (int64_t i = threadIdx.x; i < chunks; i += kLarsBlock) {
    const f32x2 v = partial[s.chunk_begin + i];
    sp += v[0]; sg += v[1];
  }
  return lars_block_sum(sp, sg);
}

__global__ __launch_bounds__(kLarsBlock) void lars_reduce_kernel(const dvt_lars_seg* __restrict__ table,
                                                                 const f32x2* __restrict__ partial, f32x2* __restrict__ out) {
  const f32x2 r = lars_segment_sumsq(partial, table[blockIdx.x]);
  if (threadIdx.x == 0) out[blockIdx.x] = r;
}

struct LarsCoef {
  float q, wd, mu, keep, lr;          // d = q (g + wd p); buf = mu buf + keep d
  bool scaled, first, nesterov;
};

// One element of LARS.  Without trust scaling (weight_decay == 0 or a zero norm) d is the raw gradient: no decay either.
// `first`: buf = d itself, not (1 - dampening) d.
__device__ __forceinline__ void lars_update(float& p, float g, float& buf, const LarsCoef& c) {
  float d = c.scaled ? c.q * fmaf(c.wd, p, g) : g;
  if (c.mu != 0.f) {
    buf = c.first ? d : fmaf(c.mu, buf, c.keep * d);
    d = c.nesterov ? fmaf(c.mu, buf, d) : buf;
  }
  p -= c.lr * d;
}

template <bool kVec, typename M>
__device__ __forceinline__ void lars_chunk_update(gfloat* __restrict__ p, const gfloat* __restrict__ g,
                                                  gfloat* __restrict__ buf, DVT_GLOBAL M* __restrict__ mirror, int len,
                                                  const LarsCoef& c) {
  typedef M m4 __attribute__((ext_vector_type(4)));
  constexpr bool kMirror = !std::is_same<M, float>::value;
  const bool mom = c.mu != 0.f;
  const int n4 = len >> 2;
  for (int q = threadIdx.x; q < n4; q += kLarsBlock) {
    const int e = 4 * q;
    f32x4 pv = lars_load4<kVec>(p + e), bv = {0.f, 0.f, 0.f, 0.f};
    const f32x4 gv = lars_load4<kVec>(g + e);
    if (mom && !c.first) bv = lars_load4<kVec>(buf + e);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pi = pv[k], bi = bv[k];
      lars_update(pi, gv[k], bi, c);
      pv[k] = pi; bv[k] = bi;
    }
    lars_store4<kVec>(p + e, pv);
    if (mom) lars_store4<kVec>(buf + e, bv);
    if (kMirror) {
      if (kVec) {
        m4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (M)pv[k];
        *(DVT_GLOBAL m4*)(mirror + e) = o;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) mirror[e + k] = (M)pv[k];
      }
    }
  }
  if ((int)threadIdx.x < (len & 3)) {
    const int i = 4 * n4 + threadIdx.x;
    float pi = p[i], bi = (mom && !c.first) ? buf[i] : 0.f;
    lars_update(pi, g[i], bi, c);
    p[i] = pi;
    if (mom) buf[i] = bi;
    if (kMirror) mirror[i] = (M)pi;
  }
}

// The update of one chunk: its segment's norms from the partials, q, then the rule.  lr and the step counter (int64[2],
// publish_step) are read on the device; the counter only tells the first step from the later ones.
template <typename M>
__global__ __launch_bounds__(kLarsBlock) void lars_update_kernel(const dvt_lars_seg* __restrict__ table, int n,
                                                                 const f32x2* __restrict__ partial,
                                                                 const float* __restrict__ lr_dev, float mu, float dampening,
                                                                 int nesterov, float trust, float eps, int64_t* step_dev,
                                                                 M* /* tag: the mirrors' type */) {
  const int64_t steps = step_dev[0];
  const int64_t c = blockIdx.x;
  const dvt_lars_seg s = table[lars_find_segment(table, n, c)];
  const f32x2 ss = lars_segment_sumsq(partial, s);
  const float pn = sqrtf(ss[0]), gn = sqrtf(ss[1]);
  LarsCoef k;
  k.scaled = s.weight_decay != 0.f && pn != 0.f && gn != 0.f;
  k.q = k.scaled ? trust * pn / (gn + s.weight_decay * pn + eps) : 1.f;
  k.wd = s.weight_decay; k.mu = mu; k.keep = 1.f - dampening; k.lr = lr_dev[0];
  k.first = steps == 0; k.nesterov = nesterov != 0;
  const int64_t start = (c - s.chunk_begin) * kLarsChunk;
  const int len = lars_chunk_len(s.numel, start);
  gfloat* p = lars_global<float>(s.param) + start;
  const gfloat* g = lars_global<float>(s.grad) + start;
  gfloat* buf = mu != 0.f ? lars_global<float>(s.buf) + start : nullptr;
  DVT_GLOBAL M* mirror = std::is_same<M, float>::value ? nullptr : lars_global<M>(s.mirror) + start;
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15u) == 0 && ((uintptr_t)mirror & 7u) == 0;
  if (vec) lars_chunk_update<true, M>(p, g, buf, mirror, len, k);
  else lars_chunk_update<false, M>(p, g, buf, mirror, len, k);
  publish_step(step_dev, steps);
}

// ------------------------------------------------------------------ global gradient norm and in-place clip
// (Lightning's gradient_clip_val = torch.nn.utils.clip_grad_norm_ over all gradients.)  The segment table, the chunks and
// their ownership are LARS's; only `grad` and `numel` of a row are read.  One float per chunk: the sum of g^2 (kind 2) or
// max |g| (kind inf), and ONE total over the whole table.  Every sum and maximum is taken in an order that numel alone
// fixes -- under data parallelism every rank forms the coefficient from the same all-reduced gradient, and a total that
// depended on the arrival order of the blocks would let the ranks' weights drift apart.
enum { kNormTwo = 0, kNormInf = 1 };

// max that keeps a NaN (fmaxf drops it): the clip must see a non-finite gradient under either norm.
__device__ __forceinline__ float grad_max(float a, float b) { return (a != a || a > b) ? a : b; }

template <int kKind>
__device__ __forceinline__ float grad_join(float a, float b) { return kKind == kNormTwo ? a + b : grad_max(a, b); }

// lars_block_sum for one value under either join: the xor butterfly inside each wave, then the waves in index order.
template <int kKind>
__device__ __forceinline__ float grad_block_join(float a) {
  __shared__ float red[kLarsBlock / DVT_WAVE];
#pragma unroll
  for (int off = DVT_WAVE / 2; off > 0; off >>= 1) a = grad_join<kKind>(a, __shfl_xor(a, off, DVT_WAVE));
  __syncthreads();                                      // the previous use of `red` is over
  if ((threadIdx.x & (DVT_WAVE - 1)) == 0) red[threadIdx.x / DVT_WAVE] = a;
  __syncthreads();
  a = red[0];
#pragma unroll
  for (int w = 1; w < kLarsBlock / DVT_WAVE; ++w) a = grad_join<kKind>(a, red[w]);
  return a;
}

template <int kKind, bool kVec>
__device__ __forceinline__ float grad_chunk_partial(const gfloat* __restrict__ g, int len) {
  float acc = 0.f;
  const int n4 = len >> 2;
  for (int q = threadIdx.x; q < n4; q += kLarsBlock) {
    const f32x4 gv = lars_load4<kVec>(g + 4 * q);
#pragma unroll
    for (int k = 0; k < 4; ++k) acc = kKind == kNormTwo ? fmaf(gv[k], gv[k], acc) : grad_max(acc, fabsf(gv[k]));
  }
  if ((int)threadIdx.x < (len & 3)) {
    const float gi = g[4 * n4 + threadIdx.x];
    acc = kKind == kNormTwo ? fmaf(gi, gi, acc) : grad_max(acc, fabsf(gi));
  }
  return acc;
}

// The total over all `chunks` partials: thread t joins the partials t, t + 256, ... in that order, then the block.
template <int kKind>
__device__ __forceinline__ float grad_total(const float* __restrict__ partial, int64_t chunks) {
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < chunks; i += kLarsBlock) acc = grad_join<kKind>(acc, partial[i]);
  return grad_block_join<kKind>(acc);
}

template <int kKind>
__device__ __forceinline__ float grad_norm_of(float total) { return kKind == kNormTwo ? sqrtf(total) : total; }

// partial[c] of chunk c.
template <int kKind>
__global__ __launch_bounds__(kLarsBlock) void grad_norm_kernel(const dvt_lars_seg* __restrict__ table, int n,
                                                               float* __restrict__ partial) {
  const int64_t c = blockIdx.x;
  const dvt_lars_seg s = table[lars_find_segment(table, n, c)];
  const int64_t start = (c - s.chunk_begin) * kLarsChunk;
  const int len = lars_chunk_len(s.numel, start);
  const gfloat* g = lars_global<float>(s.grad) + start;
  const float acc = ((uintptr_t)g & 15u) == 0 ? grad_chunk_partial<kKind, true>(g, len)
                                              : grad_chunk_partial<kKind, false>(g, len);
  const float r = grad_block_join<kKind>(acc);
  if (threadIdx.x == 0) partial[c] = r;
}

// out = {norm, total} from the partials: one block.  (A last-block ticket inside grad_norm_kernel would save this launch,
// but its release / acquire pair per block -- the L2s of the XCDs are not coherent with each other without it -- cost
// 75 us at 3521 chunks, four times the two launches together.)
template <int kKind>
__global__ __launch_bounds__(kLarsBlock) void grad_total_kernel(const float* __restrict__ partial, int64_t chunks,
                                                                float* __restrict__ out) {
  const float total = grad_total<kKind>(partial, chunks);
  if (threadIdx.x == 0) {
    out[0] = grad_norm_of<kKind>(total);
    out[1] = total;
  }
}

// g *= coef in place, coef = min(1, max_norm / (norm * inv_scale + 1e-6)) -- torch.nn.utils.clip_grad_norm_'s rule on the
// UNSCALED norm.  Every block forms the same total from the partials.  A non-finite total leaves the gradient as it is
// (the loss-scaled step's own found_inf check must still see the values that overflowed), and so does coef == 1, which
// saves the pass.  Block 0 reports norm * inv_scale.
template <int kKind>
__global__ __launch_bounds__(kLarsBlock) void grad_clip_kernel(const dvt_lars_seg* __restrict__ table, int n,
                                                               const float* __restrict__ partial, int64_t chunks,
                                                               float max_norm, const float* __restrict__ scale_dev,
                                                               int scale_is_inverse, float* __restrict__ out) {
  const float norm = grad_norm_of<kKind>(grad_total<kKind>(partial, chunks));
  const float inv_scale = !scale_dev ? 1.f : (scale_is_inverse ? scale_dev[0] : 1.0f / scale_dev[0]);
  const float unscaled = norm * inv_scale;
  if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = unscaled;
  if (!(fabsf(norm) <= 3.402823466e38f)) return;        // inf or nan
  const float coef = fminf(1.0f, max_norm / (unscaled + 1e-6f));
  if (coef == 1.0f) return;
  const int64_t c = blockIdx.x;
  const dvt_lars_seg s = table[lars_find_segment(table, n, c)];
  const int64_t start = (c - s.chunk_begin) * kLarsChunk;
  const int len = lars_chunk_len(s.numel, start);
  gfloat* g = lars_global<float>(const_cast<float*>(s.grad)) + start;
  const int n4 = len >> 2;
  if (((uintptr_t)g & 15u) == 0) {
    for (int q = threadIdx.x; q < n4; q += kLarsBlock) lars_store4<true>(g + 4 * q, lars_load4<true>(g + 4 * q) * coef);
  } else {
    for (int q = threadIdx.x; q < n4; q += kLarsBlock) lars_store4<false>(g + 4 * q, lars_load4<false>(g + 4 * q) * coef);
  }
  if ((int)threadIdx.x < (len & 3)) g[4 * n4 + threadIdx.x] *= coef;
}

#define DVT_LAUNCH_NORM_KIND(KERNEL, kind, grid, block, st, ...)                                           \
  do {                                                                                                     \
    if ((kind) == DVT_NORM_INF) hipLaunchKernelGGL((KERNEL<kNormInf>), grid, block, 0, st, __VA_ARGS__);   \
    else hipLaunchKernelGGL((KERNEL<kNormTwo>), grid, block, 0, st, __VA_ARGS__);                          \
  } while (0)

inline int64_t lars_total_chunks(const int64_t* numel, int n, int64_t* chunk_begin) {
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    if (chunk_begin) chunk_begin[i] = total;
    total += dvt_cdiv(numel[i], kLarsChunk);
  }
  if (chunk_begin) chunk_begin[n] = total;
  return total;
}

}  // namespace

extern "C" {

int dvt_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                   dvt_stream_t stream) {
  if (n == 0) return DVT_OK;   // empty tensors carry null pointers: nothing to validate, nothing to launch
  DVT_REQUIRE(param && grad && exp_avg && exp_avg_sq && n >= 0 && step >= 1,
              "dvt_adamw_step: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(adamw_kernel, dim3(dvt_grid(n)), dim3(kBlock), 0, st, param, grad, exp_avg,
                     exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, (float)bc1,
                     (float)sqrt(bc2));
  DVT_LAUNCH_CHECK("dvt_adamw_step");
  return DVT_OK;
}

int dvt_adamw_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                       float lr, float beta1, float beta2, float eps, float weight_decay,
                       int64_t* step_dev, const uint8_t* skip64, dvt_stream_t stream) {
  if (n == 0) return DVT_OK;   // empty tensors carry null pointers: nothing to validate, nothing to launch
  DVT_REQUIRE(param && grad && exp_avg && exp_avg_sq && step_dev && n >= 0, "dvt_adamw_step_dev: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adamw_dev_kernel, dim3(dvt_grid(n)), dim3(kBlock), 0, st, param, grad, exp_avg,
                     exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, (const int64_t*)step_dev, skip64);
  hipLaunchKernelGGL(inc_step_kernel, dim3(1), dim3(1), 0, st, step_dev);
  DVT_LAUNCH_CHECK("dvt_adamw_step_dev");
  return DVT_OK;
}

int dvt_adamw_step_fused(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int64_t* step_dev2,
                         const uint8_t* skip64, void* mirror, int mirror_dtype, dvt_stream_t stream) {
  if (n == 0) return DVT_OK;
  DVT_REQUIRE(param && grad && exp_avg && exp_avg_sq && step_dev2 && n >= 0, "dvt_adamw_step_fused: bad arguments");
  DVT_REQUIRE(dvt_aligned16(param) && dvt_aligned16(grad) && dvt_aligned16(exp_avg) && dvt_aligned16(exp_avg_sq),
              "dvt_adamw_step_fused: buffers must be 16-byte aligned");
  DVT_REQUIRE(!mirror || (dvt_is_16bit(mirror_dtype) && ((uintptr_t)mirror & 7u) == 0),
              "dvt_adamw_step_fused: mirror must be bf16 / f16 and 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(dvt_grid((n >> 2) + 1)), block(256);
  DVT_LAUNCH_MIRRORED(adamw_fused_kernel, mirror, mirror_dtype, grid, block, st, param, grad, exp_avg, exp_avg_sq, n, lr,
                      beta1, beta2, eps, weight_decay, step_dev2, skip64);
  DVT_LAUNCH_CHECK("dvt_adamw_step_fused");
  return DVT_OK;
}

int dvt_adamw_step_scaled(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int64_t* step_dev, float* scale,
                          int32_t* found_inf, int32_t* good_steps, int growth_interval, float growth, float backoff,
                          float* loss_grad, float loss_grad_base, const uint8_t* skip64, dvt_stream_t stream) {
  // empty tensors carry null pointers: the scaler state still moves (a clean step), nothing else is launched
  DVT_REQUIRE((n == 0 || (param && grad && exp_avg && exp_avg_sq)) && step_dev && scale && found_inf && good_steps &&
                  loss_grad && n >= 0 && growth_interval > 0 && growth >= 1.f && backoff > 0.f && backoff <= 1.f,
              "dvt_adamw_step_scaled: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) {
    hipLaunchKernelGGL(check_finite_kernel, dim3(dvt_grid(n)), dim3(kBlock), 0, st, grad, n, (int*)found_inf);
    hipLaunchKernelGGL(adamw_scaled_kernel, dim3(dvt_grid(n)), dim3(kBlock), 0, st, param, grad, exp_avg, exp_avg_sq, n,
                       lr, beta1, beta2, eps, weight_decay, (const int64_t*)step_dev, (const float*)scale,
                       (const int*)found_inf, skip64);
  }
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(1), 0, st, step_dev, scale, (int*)found_inf,
                     (int*)good_steps, growth_interval, growth, backoff, loss_grad, loss_grad_base);
  DVT_LAUNCH_CHECK("dvt_adamw_step_scaled");
  return DVT_OK;
}

int dvt_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* lr_dev,
                      float beta1, float beta2, float eps, float weight_decay, int64_t* step_dev2, const uint8_t* skip64,
                      void* mirror, int mirror_dtype, dvt_stream_t stream) {
  DVT_REQUIRE(n >= 0, "dvt_adam_step_dev: negative size");
  if (n == 0) return DVT_OK;
  DVT_REQUIRE(param && grad && exp_avg && exp_avg_sq && lr_dev && step_dev2, "dvt_adam_step_dev: bad arguments");
  DVT_REQUIRE(!mirror || dvt_is_16bit(mirror_dtype), "dvt_adam_step_dev: mirror must be bf16 / f16");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(dvt_cdiv(n, 256) < 4096 ? dvt_cdiv(n, 256) : 4096)), block(256);
  DVT_LAUNCH_MIRRORED(adam_dev_kernel, mirror, mirror_dtype, grid, block, st, param, grad, exp_avg, exp_avg_sq, n, lr_dev,
                      beta1, beta2, eps, weight_decay, step_dev2, skip64);
  DVT_LAUNCH_CHECK("dvt_adam_step_dev");
  return DVT_OK;
}

int dvt_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                 float weight_decay, const uint8_t* skip64, dvt_stream_t stream) {
  if (n == 0) return DVT_OK;   // empty tensors carry null pointers: nothing to validate, nothing to launch
  DVT_REQUIRE(param && grad && n >= 0 && (momentum == 0.f || momentum_buf), "dvt_sgd_step: bad arguments");
  hipLaunchKernelGGL(sgd_kernel, dim3(dvt_grid(n)), dim3(kBlock), 0, (hipStream_t)stream, param, grad, momentum_buf,
                     n, lr, momentum, weight_decay, skip64);
  DVT_LAUNCH_CHECK("dvt_sgd_step");
  return DVT_OK;
}

int dvt_adagrad_step(float* param, const float* grad, float* state_sum, int64_t n, float lr, float lr_decay,
                     float eps, float weight_decay, int64_t step, const uint8_t* skip64, dvt_stream_t stream) {
  if (n == 0) return DVT_OK;   // empty tensors carry null pointers: nothing to validate, nothing to launch
  DVT_REQUIRE(param && grad && state_sum && n >= 0 && step >= 1, "dvt_adagrad_step: bad arguments");
  const float clr = (float)((double)lr / (1.0 + (double)(step - 1) * (double)lr_decay));
  hipLaunchKernelGGL(adagrad_kernel, dim3(dvt_grid(n)), dim3(kBlock), 0, (hipStream_t)stream, param, grad, state_sum,
                     n, clr, eps, weight_decay, skip64);
  DVT_LAUNCH_CHECK("dvt_adagrad_step");
  return DVT_OK;
}

int dvt_lars_plan(const int64_t* numel, int n, dvt_lars_plan_info* info, int64_t* chunk_begin) {
  DVT_REQUIRE(info && n >= 0 && (numel || n == 0), "dvt_lars_plan: bad arguments");
  for (int i = 0; i < n; ++i) DVT_REQUIRE(numel[i] > 0, "dvt_lars_plan: every segment needs at least one element");
  const int64_t total = lars_total_chunks(numel, n, chunk_begin);
  DVT_REQUIRE(total <= 0x7fffffffll, "dvt_lars_plan: more chunks than one grid holds");
  info->chunk = kLarsChunk;
  info->blocks = total;
  info->grid_cap = 0;                              // one block per chunk, no grid-stride loop
  info->workspace_bytes = total * (int64_t)sizeof(f32x2);
  return DVT_OK;
}

int dvt_lars_sumsq(const dvt_lars_seg* table, int n, int64_t chunks, float* workspace, float* sumsq,
                   dvt_stream_t stream) {
  DVT_REQUIRE(n >= 0 && chunks >= 0 && chunks <= 0x7fffffffll, "dvt_lars_sumsq: bad sizes");
  if (n == 0) return DVT_OK;
  DVT_REQUIRE(table && workspace && sumsq && chunks >= n, "dvt_lars_sumsq: bad arguments");
  DVT_REQUIRE(((uintptr_t)workspace & 7u) == 0 && ((uintptr_t)sumsq & 7u) == 0, "dvt_lars_sumsq: buffers must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lars_norms_kernel, dim3((unsigned)chunks), dim3(kLarsBlock), 0, st, table, n, (f32x2*)workspace);
  hipLaunchKernelGGL(lars_reduce_kernel, dim3((unsigned)n), dim3(kLarsBlock), 0, st, table, (const f32x2*)workspace,
                     (f32x2*)sumsq);
  DVT_LAUNCH_CHECK("dvt_lars_sumsq");
  return DVT_OK;
}

int dvt_lars_step(const dvt_lars_seg* table, int n, int64_t chunks, float* workspace, const float* lr_dev, float momentum,
                  float dampening, int nesterov, float trust_coefficient, float eps, int64_t* step_dev2, int mirror,
                  int mirror_dtype, dvt_stream_t stream) {
  DVT_REQUIRE(n >= 0 && chunks >= 0 && chunks <= 0x7fffffffll, "dvt_lars_step: bad sizes");
  if (n == 0) return DVT_OK;
  DVT_REQUIRE(table && workspace && lr_dev && step_dev2 && chunks >= n, "dvt_lars_step: bad arguments");
  DVT_REQUIRE(((uintptr_t)workspace & 7u) == 0, "dvt_lars_step: workspace must be 8-byte aligned");
  DVT_REQUIRE(!mirror || dvt_is_16bit(mirror_dtype), "dvt_lars_step: mirror must be bf16 / f16");
  DVT_REQUIRE(momentum >= 0.f && (!nesterov || (momentum > 0.f && dampening == 0.f)),
              "dvt_lars_step: nesterov needs momentum > 0 and dampening == 0");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)chunks), block(kLarsBlock);
  hipLaunchKernelGGL(lars_norms_kernel, grid, block, 0, st, table, n, (f32x2*)workspace);
  void* tag = mirror ? (void*)workspace : nullptr;      // non-null selects the 16-bit instantiation; never dereferenced
  DVT_LAUNCH_MIRRORED(lars_update_kernel, tag, mirror_dtype, grid, block, st, table, n, (const f32x2*)workspace, lr_dev,
                      momentum, dampening, nesterov, trust_coefficient, eps, step_dev2);
  DVT_LAUNCH_CHECK("dvt_lars_step");
  return DVT_OK;
}

int dvt_grad_norm(const dvt_lars_seg* table, int n, int64_t chunks, float* workspace, int norm_kind, float* out2,
                  dvt_stream_t stream) {
  DVT_REQUIRE(n >= 0 && chunks >= 0 && chunks <= 0x7fffffffll, "dvt_grad_norm: bad sizes");
  DVT_REQUIRE(norm_kind == DVT_NORM_2 || norm_kind == DVT_NORM_INF, "dvt_grad_norm: norm_kind must be DVT_NORM_2 or DVT_NORM_INF");
  if (n == 0) return DVT_OK;
  DVT_REQUIRE(table && workspace && out2 && chunks >= n, "dvt_grad_norm: bad arguments");
  DVT_REQUIRE(((uintptr_t)workspace & 3u) == 0 && ((uintptr_t)out2 & 3u) == 0, "dvt_grad_norm: buffers must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  DVT_LAUNCH_NORM_KIND(grad_norm_kernel, norm_kind, dim3((unsigned)chunks), dim3(kLarsBlock), st, table, n, workspace);
  DVT_LAUNCH_NORM_KIND(grad_total_kernel, norm_kind, dim3(1), dim3(kLarsBlock), st, (const float*)workspace, chunks, out2);
  DVT_LAUNCH_CHECK("dvt_grad_norm");
  return DVT_OK;
}

int dvt_grad_clip(const dvt_lars_seg* table, int n, int64_t chunks, float* workspace, int norm_kind, float max_norm,
                  const float* scale_dev, int scale_is_inverse, float* norm_out, dvt_stream_t stream) {
  DVT_REQUIRE(n >= 0 && chunks >= 0 && chunks <= 0x7fffffffll, "dvt_grad_clip: bad sizes");
  DVT_REQUIRE(norm_kind == DVT_NORM_2 || norm_kind == DVT_NORM_INF, "dvt_grad_clip: norm_kind must be DVT_NORM_2 or DVT_NORM_INF");
  DVT_REQUIRE(max_norm >= 0.f, "dvt_grad_clip: max_norm must be >= 0");
  if (n == 0) return DVT_OK;
  DVT_REQUIRE(table && workspace && norm_out && chunks >= n, "dvt_grad_clip: bad arguments");
  DVT_REQUIRE(((uintptr_t)workspace & 3u) == 0 && ((uintptr_t)norm_out & 3u) == 0, "dvt_grad_clip: buffers must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)chunks), block(kLarsBlock);
  DVT_LAUNCH_NORM_KIND(grad_norm_kernel, norm_kind, grid, block, st, table, n, workspace);
  DVT_LAUNCH_NORM_KIND(grad_clip_kernel, norm_kind, grid, block, st, table, n, (const float*)workspace, chunks, max_norm,
                       scale_dev, scale_is_inverse, norm_out);
  DVT_LAUNCH_CHECK("dvt_grad_clip");
  return DVT_OK;
}

}  // extern "C"
