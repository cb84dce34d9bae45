// patchify.hip -- the patch gather of the tokenisers and its adjoint: the one place that knows the index map.
//
// The reference tokenises one frame at a time: 'b t c (h p1) (w p2) -> b t (h w) (p1 p2 c)' + Linear
// (src/models/vit.py:89-92).  A tubelet (the ViViT paper's 3-D patch) is a pt x P x P patch across pt consecutive frames.
// For x [frames, C, H, W], frames = b t, t % pt == 0, nh = H / P, nw = W / P and f = tau' pt + k (tau' = bi (t / pt) + tau):
//     out[(tau' nh + ph) nw + pw, ((k P + p1) P + p2) C + c] = x[tau' pt + k, c, ph P + p1, pw P + p2]
// i.e. 'b (tau k) c (h p1) (w p2) -> (b tau h w) (k p1 p2 c)': k slowest, c fastest, so an output row is the pt per-frame
// patch vectors of the reference order, concatenated.  The per-frame gather is pt == 1 (k = 0, tau' = f): dvt_patchify and
// dvt_patchify_bwd are the tubelet entry at pt = 1, the same kernels and launches.  The operation is a permutation: the
// adjoint is the inverse (the same index map with source and destination exchanged).
//
//   patchify_p16_fwd_kernel   forward, P = 16, C = 3, 16-bit patch vectors (the metric shape).
//       Lane mapping: the work list is the per-frame patch list (frame f, ph, pw) at every pt;
//       lane = (patch & 3) * 16 + p1, a wave owns four consecutive patches of (normally) one frame.  The lane's 96 output
//       bytes (one patch row: 16 pixels x 3 channels) go through a wave-private LDS patch and leave as six 1-KiB store
//       instructions; the per-lane form below stores 16-byte pieces at a 1,536-byte stride (one 64-byte segment per
//       piece: 3.3 TB/s).  pt moves only the destination: the patch vector of frame tau' pt + k lands at byte k * 1536 of
//       the pt * 1536-byte row (tau', ph, pw), so the wave's four vectors are four 1.5 KiB runs at a pt * 1536-byte stride
//       (at pt = 1: 6 KiB of contiguous output).
//       Why: (read side) the four patches are neighbours in pw, so per channel and image row the wave reads one
//       contiguous span of 64 pixels at every pt.  Giving a wave the pt vectors of ONE output row instead (6 KiB
//       contiguous out at pt = 4) would read 16-pixel spans from pt different frames: 32 bytes of a 64-byte segment each
//       in 16 bits.  (write side) 1536 = 24 * 64, the rows start 16-byte aligned at multiples of
//       1536: every run is whole 64-byte segments.  The six 1-KiB store instructions of the wave cover the runs as
//       1024 | 512 + 512 | 1024 | 1024 | 512 + 512 | 1024 bytes, so a store instruction writes one or two contiguous pieces
//       of at least 512 bytes.  The four run addresses are wave-uniform values read from lanes 0, 16, 32, 48.
//       A wave usually lives for ONE group (12,544 groups on 3,136 workgroups at the metric clip), so its set-up is on the
//       critical path: the patch / frame / tubelet indices are 32-bit, the tubelet split f / pt is computed behind the
//       issued loads, and a whole group issues its six LDS reads together and stores without a branch.  pt is a run-time
//       value: at pt = 1 this kernel measured 26.26 us against 26.34 us for the per-frame kernel it replaced, whose
//       destination was g * 4 * 1536 + off in 64-bit arithmetic (profiles/patch_gather.md).
//       Fewer than 2^31 patches; more go to the vector form (2^31 patch vectors are 3.3 TB, more than the device holds).
//   patchify_vec_kernel       P in {8, 16}, C = 3, any dtype pair, both directions: a lane moves one patch row
//       (C runs of P pixels <-> P C contiguous vector elements) with 16-byte accesses; pw is the fastest index.
//   patchify_scalar_kernel    any P, C and alignment, both directions, one element per lane and step.
// The direction is a template parameter and a kernel takes exactly one pixel and one vector pointer: no pointer is
// selected at run time.  Grid-stride loops, 64-bit offsets.
#include "common.h"

#include <type_traits>

namespace {

constexpr int kBlock = 256;

// const T* when the kernel reads the tensor, T* when it writes it
template <bool READS, typename T> using ptr_t = typename std::conditional<READS, const T*, T*>::type;

// LDS operations of one wave complete in order; this only keeps the compiler from moving them across the point
__device__ __forceinline__ void wave_lds_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// the 64-bit value lane L holds, as a wave-uniform value (all lanes active)
template <int L>
__device__ __forceinline__ int64_t value_of_lane(int64_t v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(uint32_t)v, L);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), L);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

template <typename S, typename D>
__global__ __launch_bounds__(256) void patchify_p16_fwd_kernel(const S* __restrict__ x, D* __restrict__ out, unsigned npatches,
                                                               int H, int W, unsigned nw, unsigned npf, unsigned pt) {
  constexpr int P = 16, C = 3, ROWB = P * C * 2;              // 96 bytes per patch row
  constexpr int VECB = P * ROWB;                              // 1536 bytes per patch vector
  static_assert(sizeof(D) == 2, "16-bit patch vectors");
  __shared__ __attribute__((aligned(16))) char lds[4][64 * ROWB];
  typedef D v8 __attribute__((ext_vector_type(8)));
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  // npatches < 2^31 (the launcher sends anything larger to the vector form): patch, frame and tubelet indices are 32-bit,
  // so the index divisions are the short unsigned ones; only byte and element offsets are 64-bit
  const unsigned ngroups = (npatches + 3) >> 2, nwaves = gridDim.x * 4;
  char* mine = lds[wid];
  for (unsigned g = blockIdx.x * 4 + wid; g < ngroups; g += nwaves) {
    const unsigned patch = min(g * 4 + (lane >> 4), npatches - 1);  // per-frame patch list; the tail repeats the last one
    const int p1 = lane & 15;
    const unsigned f = patch / npf;
    const unsigned sp = patch - f * npf;                      // ph * nw + pw
    const unsigned ph = sp / nw, pw = sp - ph * nw;
    const int64_t xoff = (((int64_t)f * C) * H + (int64_t)(ph * P + p1)) * W + (int64_t)(pw * P);
    float pix[C][P];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int q = 0; q < P / 8; ++q) {
        float t[8];
        load8<S>(x + xoff + (int64_t)c * H * W + q * 8, t);
#pragma unroll
        for (int e = 0; e < 8; ++e) pix[c][q * 8 + e] = t[e];
      }
#pragma unroll
    for (int q = 0; q < P * C / 8; ++q) {
      v8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int e = q * 8 + j;                                // e = p2 * C + c
        o[j] = (D)pix[e % C][e / C];
      }
      *reinterpret_cast<v8*>(mine + lane * ROWB + q * 16) = o;
    }
    // byte offset of this lane's patch vector in out; the four of the wave sit in lanes 0, 16, 32, 48
    const unsigned tau = f / pt, k = f - tau * pt;
    const int64_t vbase = (((int64_t)tau * npf + sp) * pt + k) * (int64_t)VECB;
    const int64_t b0 = value_of_lane<0>(vbase), b1 = value_of_lane<16>(vbase), b2 = value_of_lane<32>(vbase),
                  b3 = value_of_lane<48>(vbase);
    wave_lds_fence();
    const unsigned have = npatches - g * 4;                    // patch vectors of this group that exist (>= 1)
    v8 o[P * C / 8];
    int64_t dst[P * C / 8];
#pragma unroll
    for (int q = 0; q < P * C / 8; ++q) {
      const int off = (q * 64 + lane) * 16;
      const int s = off / VECB;                                 // which of the four vectors; two values per q at most
      dst[q] = (s == 0 ? b0 : s == 1 ? b1 : s == 2 ? b2 : b3) + (off - s * VECB);
      o[q] = *reinterpret_cast<const v8*>(mine + off);
    }
    // A whole group (all but the last one) stores without a branch, so the six LDS reads are issued together; under a
    // per-store condition each read sits in its own branch (measured: no difference on its own at six waves per SIMD).
    if (have >= 4) {
#pragma unroll
      for (int q = 0; q < P * C / 8; ++q) *reinterpret_cast<v8*>(reinterpret_cast<char*>(out) + dst[q]) = o[q];
    } else {
#pragma unroll
      for (int q = 0; q < P * C / 8; ++q)
        if ((unsigned)((q * 64 + lane) * 16 / VECB) < have) *reinterpret_cast<v8*>(reinterpret_cast<char*>(out) + dst[q]) = o[q];
    }
    wave_lds_fence();
  }
}

// Work item = one patch row (frame, ph, p1, pw): C runs of P contiguous pixels on the pixel side, one run of P*C
// contiguous elements on the vector side.  pw is the fastest index so a wave touches 64 adjacent pixel runs.
template <int P, int C, typename S, typename D, bool FWD>
__global__ void patchify_vec_kernel(ptr_t<FWD, S> __restrict__ pixp, ptr_t<!FWD, D> __restrict__ vecp, int64_t frames, int H,
                                    int W, int pt) {
  const int nh = H / P, nw = W / P;
  const int64_t items = frames * nh * P * nw;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  constexpr int64_t pd = (int64_t)P * P * C;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const int pw = (int)(it % nw);
    int64_t r = it / nw;
    const int p1 = (int)(r % P);
    r /= P;
    const int ph = (int)(r % nh);
    const int64_t f = r / nh;
    const int64_t tau = f / pt;
    const int k = (int)(f - tau * pt);
    const int64_t orow = (tau * nh + ph) * nw + pw;
    const int64_t ooff = (orow * pt + k) * pd + (int64_t)p1 * P * C;
    const int64_t xoff = ((f * C) * H + (int64_t)ph * P + p1) * W + (int64_t)pw * P;
    float vec[P * C];
    if constexpr (FWD) {
      float pix[C][P];
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int q = 0; q < P / 8; ++q) {
          float t[8];
          load8<S>(pixp + xoff + (int64_t)c * H * W + q * 8, t);
#pragma unroll
          for (int e = 0; e < 8; ++e) pix[c][q * 8 + e] = t[e];
        }
#pragma unroll
      for (int p2 = 0; p2 < P; ++p2)
#pragma unroll
        for (int c = 0; c < C; ++c) vec[p2 * C + c] = pix[c][p2];
#pragma unroll
      for (int q = 0; q < P * C / 8; ++q) {
        float t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = vec[q * 8 + e];
        store8<D>(vecp + ooff + q * 8, t);
      }
    } else {
#pragma unroll
      for (int q = 0; q < P * C / 8; ++q) {
        float t[8];
        load8<D>(vecp + ooff + q * 8, t);
#pragma unroll
        for (int e = 0; e < 8; ++e) vec[q * 8 + e] = t[e];
      }
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int q = 0; q < P / 8; ++q) {
          float t[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) t[e] = vec[(q * 8 + e) * C + c];
          store8<S>(pixp + xoff + (int64_t)c * H * W + q * 8, t);
        }
    }
  }
}

// Any P, C, alignment: a workgroup walks output rows (grid-stride, the one 64-bit division), its lanes the pt*P*P*C
// elements of the row (32-bit index arithmetic; the launcher refuses a row of 2^31 elements or more).
template <typename S, typename D, bool FWD>
__global__ void patchify_scalar_kernel(ptr_t<FWD, S> __restrict__ pixp, ptr_t<!FWD, D> __restrict__ vecp, int64_t rows,
                                       int C, int H, int W, int P, int pt) {
  const unsigned nw = W / P, npf = (H / P) * nw;
  const unsigned pd = (unsigned)P * P * C;                     // one frame's share of a row
  const unsigned rowlen = pd * pt, pc = (unsigned)P * C;
  for (int64_t orow = blockIdx.x; orow < rows; orow += gridDim.x) {
    const int64_t tub = orow / npf;                            // b * (t / pt) + tau
    const unsigned sp = (unsigned)(orow - tub * npf);
    const unsigned ph = sp / nw, pw = sp - ph * nw;
    for (unsigned col = threadIdx.x; col < rowlen; col += blockDim.x) {
      const unsigned k = col / pd, e = col - k * pd;
      const unsigned p1 = e / pc, r = e - p1 * pc;
      const unsigned p2 = r / C, c = r - p2 * C;
      const int64_t f = tub * pt + k;
      const int64_t xi = ((f * C + c) * H + (int64_t)(ph * P + p1)) * W + (int64_t)(pw * P + p2);
      const int64_t oi = orow * rowlen + col;
      if constexpr (FWD) vecp[oi] = from_f32<D>(to_f32<S>(pixp[xi]));
      else pixp[xi] = from_f32<S>(to_f32<D>(vecp[oi]));
    }
  }
}

template <typename S, typename D, bool FWD>
int patchify_dispatch(ptr_t<FWD, void> pix, ptr_t<!FWD, void> vec, int64_t frames, int C, int H, int W, int P, int pt,
                      hipStream_t st, const char* name) {
  const int nh = H / P, nw = W / P;
  const int64_t items = frames * nh * P * nw;
  const bool vec_ok = (W % 8 == 0) && (P % 8 == 0) && ((P * C) % 8 == 0) && dvt_aligned16(pix) && dvt_aligned16(vec) &&
                      ((int64_t)H * W % 8 == 0);
  auto pixp = (ptr_t<FWD, S>)pix;
  auto vecp = (ptr_t<!FWD, D>)vec;
  if constexpr (FWD && sizeof(D) == 2) {
    const int64_t npatches = frames * nh * nw;
    if (vec_ok && P == 16 && C == 3 && npatches < ((int64_t)1 << 31)) {
      int64_t blocks = dvt_cdiv(dvt_cdiv(npatches, 4), 4);
      const int64_t cap = (int64_t)dvt_num_cus() * 16;
      if (blocks > cap) blocks = cap;
      hipLaunchKernelGGL((patchify_p16_fwd_kernel<S, D>), dim3((unsigned)blocks), dim3(256), 0, st, pixp, vecp,
                         (unsigned)npatches, H, W, (unsigned)nw, (unsigned)(nh * nw), (unsigned)pt);
      DVT_LAUNCH_CHECK(name);
      return DVT_OK;
    }
  }
  if (vec_ok && P == 16 && C == 3) {
    hipLaunchKernelGGL((patchify_vec_kernel<16, 3, S, D, FWD>), dim3(dvt_grid(items)), dim3(kBlock), 0, st, pixp, vecp,
                       frames, H, W, pt);
  } else if (vec_ok && P == 8 && C == 3) {
    hipLaunchKernelGGL((patchify_vec_kernel<8, 3, S, D, FWD>), dim3(dvt_grid(items)), dim3(kBlock), 0, st, pixp, vecp,
                       frames, H, W, pt);
  } else {
    if ((int64_t)P * P * C * pt >= ((int64_t)1 << 31)) DVT_UNSUPPORTED("%s: a row of pt*P*P*C >= 2^31 elements", name);
    const int64_t rows = frames / pt * nh * nw;
    hipLaunchKernelGGL((patchify_scalar_kernel<S, D, FWD>), dim3(dvt_grid(rows * kBlock)), dim3(kBlock), 0, st, pixp, vecp,
                       rows, C, H, W, P, pt);
  }
  DVT_LAUNCH_CHECK(name);
  return DVT_OK;
}

// pix: x (forward, read) / dx (adjoint, written); vec: out (forward, written) / dout (adjoint, read)
template <bool FWD>
int patchify_entry(ptr_t<FWD, void> pix, int pix_dtype, ptr_t<!FWD, void> vec, int vec_dtype, int64_t frames, int C, int H,
                   int W, int P, int pt, dvt_stream_t stream, const char* name) {
  DVT_REQUIRE(pix && vec, "%s: null pointer", name);
  DVT_REQUIRE(pt >= 1, "%s: tubelet length %d < 1", name, pt);
  DVT_REQUIRE(frames >= 0 && C > 0 && H > 0 && W > 0 && P > 0, "%s: bad sizes", name);
  DVT_REQUIRE(frames % pt == 0, "%s: %lld frames are not whole tubelets of %d", name, (long long)frames, pt);
  DVT_REQUIRE(H % P == 0 && W % P == 0, "%s: image %dx%d not divisible by patch %d", name, H, W, P);
  if (frames == 0) return DVT_OK;
  hipStream_t st = (hipStream_t)stream;
#define DVT_PATCHIFY_CASE(PD, S, VD, D) \
  if (pix_dtype == PD && vec_dtype == VD) return patchify_dispatch<S, D, FWD>(pix, vec, frames, C, H, W, P, pt, st, name);
  DVT_PATCHIFY_CASE(DVT_F32, float, DVT_F32, float)
  DVT_PATCHIFY_CASE(DVT_F32, float, DVT_BF16, bf16)
  DVT_PATCHIFY_CASE(DVT_F32, float, DVT_F16, f16)
  DVT_PATCHIFY_CASE(DVT_BF16, bf16, DVT_BF16, bf16)
  DVT_PATCHIFY_CASE(DVT_F16, f16, DVT_F16, f16)
  DVT_PATCHIFY_CASE(DVT_BF16, bf16, DVT_F32, float)
  DVT_PATCHIFY_CASE(DVT_F16, f16, DVT_F32, float)
#undef DVT_PATCHIFY_CASE
  DVT_UNSUPPORTED("%s: dtype pair (%d, %d) not supported", name, pix_dtype, vec_dtype);
}
}  // namespace

extern "C" {

// the per-frame pair: the entry at pt = 1, under its own names
int dvt_patchify(const void* x, int x_dtype, void* out, int out_dtype, int64_t frames, int C, int H, int W, int P,
                 dvt_stream_t stream) {
  return patchify_entry<true>(x, x_dtype, out, out_dtype, frames, C, H, W, P, 1, stream, "dvt_patchify");
}

int dvt_patchify_bwd(const void* dout, int dout_dtype, void* dx, int dx_dtype, int64_t frames, int C, int H, int W, int P,
                     dvt_stream_t stream) {
  return patchify_entry<false>(dx, dx_dtype, dout, dout_dtype, frames, C, H, W, P, 1, stream, "dvt_patchify_bwd");
}

int dvt_tubelet_patchify(const void* x, int x_dtype, void* out, int out_dtype, int64_t frames, int C, int H, int W, int P,
                         int pt, dvt_stream_t stream) {
  return patchify_entry<true>(x, x_dtype, out, out_dtype, frames, C, H, W, P, pt, stream, "dvt_tubelet_patchify");
}

int dvt_tubelet_patchify_bwd(const void* dout, int dout_dtype, void* dx, int dx_dtype, int64_t frames, int C, int H, int W,
                             int P, int pt, dvt_stream_t stream) {
  return patchify_entry<false>(dx, dx_dtype, dout, dout_dtype, frames, C, H, W, P, pt, stream, "dvt_tubelet_patchify_bwd");
}

}  // extern "C"
