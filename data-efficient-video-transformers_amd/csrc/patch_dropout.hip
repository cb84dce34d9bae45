// patch_dropout.hip -- patch dropout of the ViViT tokeniser (src/models/vit.py:110-116 on a kept subset of the patch tokens).
//
// A clip [b, t, C, H, W] at patch P and tubelet pt has S = b (t / pt) sequences of n = (H/P)(W/P) positions.  A sequence keeps
// k of them: keep [S, k] (int32, strictly ascending per row) and its inverse slot [S, n] (int32, -1 = dropped).  The space
// stack then runs k + 1 rows per sequence instead of n + 1.
//
//   keep_kernel<DRAW>          one workgroup per key row, keys in LDS.  Position i is kept iff fewer than k positions j have
//                              (key_j, j) < (key_i, i) in signed order (the first k of a stable argsort).  The output index
//                              of a kept position is the number of kept positions below it (wave ballots + popcounts), so
//                              keep comes out ascending without a sort.  DRAW: the keys are Philox words of the dropout
//                              generator (rng_state read on the device: a replayed graph draws a new subset per step).
//                              Integer work only, no atomics, no waiting between workgroups.
//   slots_kernel               slot from a caller's keep (one workgroup per sequence, the row in LDS).
//   gather_keep_p16_fwd_kernel the patch gather of csrc/patchify.hip (its LDS-staged P = 16 form, forward into 16-bit vectors; its
//   gather_keep_vec_kernel     vector and scalar forms, both directions) through the index: forward reads the kept
//   gather_keep_scalar_kernel  patches only; the adjoint walks EVERY pixel of dx once (kept: from row slot; dropped: zero),
//                              so it needs no pre-zeroing launch and no atomics.  The element order is the tubelet gather's:
//                                out[s k + i, ((kf P + p1) P + p2) C + c] = x[s pt + kf, c, ph P + p1, pw P + p2],
//                                (ph, pw) = keep[s, i] / nw, keep[s, i] % nw.
//   tokens_keep_fwd_kernel     out[s, 0] = cls + pos[s % T, 0];  out[s, 1 + i] = emb[s k + i] + pos[s % T, 1 + keep[s, i]].
//   tokens_keep_bwd_kernel     dpos[tau, 1 + j] (+)= sum over b, ascending, of dout[(b, tau), 1 + slot] where slot >= 0 (a fixed
//                              order: deterministic, no float atomics); the same pass writes demb (each kept row of dout is
//                              read exactly once).  A position nobody kept gets 0 when overwriting and is not touched when
//                              accumulating.
//   rows0_sum_kernel           dcls (+)= sum_s dout[s, 0].
//
// Index safety: an entry of keep outside [0, n) or of slot outside [0, k) is treated as dropped -- compared as unsigned
// against the bound before any address is formed from it.
#include "common.h"

#include <type_traits>

namespace {

constexpr int kBlock = 256;
constexpr int kMaxN = 1024;                                   // positions per sequence the selection holds in LDS

template <bool READS, typename T> using ptr_t = typename std::conditional<READS, const T*, T*>::type;

// key of (row r, position i): word (e & 3) of Philox block base + e / 4, e = r n + i -- dvt_dropout's counter use
__device__ __forceinline__ int32_t drawn_key(uint64_t seed, uint64_t base, uint64_t e) {
  const uint64_t ctr = base + (e >> 2);
  uint32_t r[4];
  philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  return (int32_t)r[e & 3];
}

template <bool DRAW>
__global__ __launch_bounds__(256) void keep_kernel(const int32_t* __restrict__ keys, const uint64_t* __restrict__ state,
                                                   uint64_t call_offset, int n, int k, int rows_per,
                                                   int32_t* __restrict__ keep, int32_t* __restrict__ slot,
                                                   int32_t* __restrict__ keys_out) {
  __shared__ int32_t sk[kMaxN];
  __shared__ unsigned long long masks[kMaxN / 64];
  const int tid = threadIdx.x;
  const int64_t r = blockIdx.x;
  uint64_t seed = 0, base = 0;
  if constexpr (DRAW) { seed = state[0]; base = state[1] + call_offset; }
  for (int i = tid; i < n; i += kBlock) {
    int32_t v;
    if constexpr (DRAW) v = drawn_key(seed, base, (uint64_t)(r * n + i));
    else v = keys[r * n + i];
    sk[i] = v;
    if (keys_out) keys_out[r * n + i] = v;
  }
  if (!keep) return;                                          // keys only (uniform)
  __syncthreads();
  bool kept[kMaxN / kBlock];
#pragma unroll
  for (int c = 0; c < kMaxN / kBlock; ++c) {
    kept[c] = false;
    if (c * kBlock < n) {                                     // uniform: every lane of a live chunk takes part in the ballot
      const int i = c * kBlock + tid;
      if (i < n) {
        const int32_t ki = sk[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {                         // every lane reads the same word: an LDS broadcast
          const int32_t kj = sk[j];
          rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
        }
        kept[c] = rank < k;
      }
      const unsigned long long m = __ballot(kept[c]);
      if ((tid & 63) == 0) masks[i >> 6] = m;                 // i <= 1023: word 0 .. 15
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kMaxN / kBlock; ++c) {
    const int i = c * kBlock + tid;
    if (i < n) {
      int idx = -1;
      if (kept[c]) {
        idx = __popcll(masks[i >> 6] & ((1ull << (i & 63)) - 1ull));
        for (int w = 0; w < (i >> 6); ++w) idx += __popcll(masks[w]);
      }
      // exactly k positions have rank < k (the order is total), so 0 <= idx < k
      for (int q = 0; q < rows_per; ++q) {
        const int64_t row = r * rows_per + q;
        slot[row * n + i] = idx;
        if (idx >= 0) keep[row * k + idx] = i;
      }
    }
  }
}

__global__ __launch_bounds__(256) void slots_kernel(const int32_t* __restrict__ keep, int n, int k, int32_t* __restrict__ slot) {
  __shared__ int32_t sl[kMaxN];
  const int64_t s = blockIdx.x;
  for (int i = threadIdx.x; i < n; i += kBlock) sl[i] = -1;
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += kBlock) {
    const int32_t p = keep[s * k + i];
    if ((unsigned)p < (unsigned)n) sl[p] = i;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += kBlock) slot[s * n + i] = sl[i];
}

// ------------------------------------------------------------------ kept gather and its adjoint
// Work item = one patch row: C runs of P contiguous pixels on the pixel side, one run of P*C contiguous elements on the vector
// side, 16-byte accesses.  Forward: the kept patch rows (s, kf, p1, i), i fastest -- ascending kept positions are neighbours
// in pw more often than not.  Adjoint: every patch row of the clip (f, ph, p1, pw), pw fastest, as in the full gather.
template <int P, int C, typename S, typename D, bool FWD>
__global__ void gather_keep_vec_kernel(ptr_t<FWD, S> __restrict__ pixp, ptr_t<!FWD, D> __restrict__ vecp,
                                       const int32_t* __restrict__ index, int64_t seqs, int H, int W, int pt, int k) {
  const int nh = H / P, nw = W / P, n = nh * nw;
  constexpr int64_t pd = (int64_t)P * P * C;
  const int64_t items = FWD ? seqs * pt * P * k : seqs * pt * nh * P * nw;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    int64_t s, orow;
    int kf, p1, ph, pw;
    bool live;
    if constexpr (FWD) {
      const int i = (int)(it % k);
      int64_t r = it / k;
      p1 = (int)(r % P);
      r /= P;
      kf = (int)(r % pt);
      s = r / pt;
      orow = s * k + i;
      const int32_t pos = index[orow];                         // keep[s, i]
      live = (unsigned)pos < (unsigned)n;
      const int sp = live ? pos : 0;
      ph = sp / nw;
      pw = sp - ph * nw;
    } else {
      pw = (int)(it % nw);
      int64_t r = it / nw;
      p1 = (int)(r % P);
      r /= P;
      ph = (int)(r % nh);
      const int64_t f = r / nh;
      s = f / pt;
      kf = (int)(f - s * pt);
      const int32_t sl = index[s * n + ph * nw + pw];          // slot[s, position]
      live = (unsigned)sl < (unsigned)k;
      orow = s * k + (live ? sl : 0);
    }
    const int64_t ooff = (orow * pt + kf) * pd + (int64_t)p1 * P * C;
    const int64_t xoff = (((s * pt + kf) * C) * H + (int64_t)ph * P + p1) * W + (int64_t)pw * P;
    float vec[P * C];
    if constexpr (FWD) {
      float pix[C][P];
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int q = 0; q < P / 8; ++q) {
          float t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
          if (live) load8<S>(pixp + xoff + (int64_t)c * H * W + q * 8, t);
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
        float t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (live) load8<D>(vecp + ooff + q * 8, t);
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

// Forward at P = 16, C = 3 into 16-bit patch vectors (the metric shape): csrc/patchify.hip's LDS-staged form on the kept
// patch list.  The work list is (frame f, kept index i), i fastest; lane = (patch & 3) * 16 + p1, so a wave owns four
// consecutive kept patches of (normally) one frame.  A lane's 96 output bytes (one patch row) go through a wave-private LDS
// patch and leave as six 1-KiB store instructions over the wave's four 1.5-KiB vectors, which sit at a pt * 1536-byte stride
// (contiguous at pt = 1) -- whole 64-byte segments, where the per-lane form below stores 16-byte pieces at a 1,536-byte
// stride.  The read side is what the kept set makes it: 32-byte runs (16-bit source), neighbours only where neighbours are kept.
template <typename S, typename D>
__global__ __launch_bounds__(256) void gather_keep_p16_fwd_kernel(const S* __restrict__ x, D* __restrict__ out,
                                                                  const int32_t* __restrict__ keep, unsigned npatches, int H,
                                                                  int W, unsigned nw, unsigned n, unsigned pt, unsigned k) {
  constexpr int P = 16, C = 3, ROWB = P * C * 2;              // 96 bytes per patch row
  constexpr int VECB = P * ROWB;                              // 1536 bytes per patch vector
  static_assert(sizeof(D) == 2, "16-bit patch vectors");
  __shared__ __attribute__((aligned(16))) char lds[4][64 * ROWB];
  typedef D v8 __attribute__((ext_vector_type(8)));
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned ngroups = (npatches + 3) >> 2, nwaves = gridDim.x * 4;   // npatches = frames * k < 2^31 (the launcher)
  char* mine = lds[wid];
  for (unsigned g = blockIdx.x * 4 + wid; g < ngroups; g += nwaves) {
    const unsigned patch = min(g * 4 + (lane >> 4), npatches - 1);        // the tail repeats the last one
    const int p1 = lane & 15;
    const unsigned f = patch / k, i = patch - f * k;
    const unsigned tau = f / pt, kf = f - tau * pt;
    const int32_t pos = keep[(int64_t)tau * k + i];
    const bool live = (unsigned)pos < n;
    const unsigned sp = live ? (unsigned)pos : 0u;
    const unsigned ph = sp / nw, pw = sp - ph * nw;
    const int64_t xoff = (((int64_t)f * C) * H + (int64_t)(ph * P + p1)) * W + (int64_t)(pw * P);
    float pix[C][P];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int q = 0; q < P / 8; ++q) {
        float t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (live) load8<S>(x + xoff + (int64_t)c * H * W + q * 8, t);
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
    const int64_t vbase = ((((int64_t)tau * k + i) * pt) + kf) * (int64_t)VECB;
    const int64_t b0 = value_of_lane<0>(vbase), b1 = value_of_lane<16>(vbase), b2 = value_of_lane<32>(vbase),
                  b3 = value_of_lane<48>(vbase);
    wave_lds_fence();
    const unsigned have = npatches - g * 4;                    // patch vectors of this group that exist (>= 1)
#pragma unroll
    for (int q = 0; q < P * C / 8; ++q) {
      const int off = (q * 64 + lane) * 16;
      const int s = off / VECB;                                 // which of the four vectors
      const int64_t dst = (s == 0 ? b0 : s == 1 ? b1 : s == 2 ? b2 : b3) + (off - s * VECB);
      const v8 o = *reinterpret_cast<const v8*>(mine + off);
      if ((unsigned)s < have) *reinterpret_cast<v8*>(reinterpret_cast<char*>(out) + dst) = o;
    }
    wave_lds_fence();
  }
}

// Any P, C and alignment.  A workgroup walks rows (grid-stride), its lanes the pt*P*P*C elements of the row: forward the kept
// rows [S k], adjoint every row [S n] of the full gather (the pixels of a dropped one get zero).
template <typename S, typename D, bool FWD>
__global__ void gather_keep_scalar_kernel(ptr_t<FWD, S> __restrict__ pixp, ptr_t<!FWD, D> __restrict__ vecp,
                                          const int32_t* __restrict__ index, int64_t seqs, int C, int H, int W, int P, int pt,
                                          int k) {
  const unsigned nw = W / P, n = (H / P) * nw;
  const unsigned pd = (unsigned)P * P * C;
  const unsigned rowlen = pd * pt, pc = (unsigned)P * C;
  const int64_t rows = seqs * (FWD ? (int64_t)k : (int64_t)n);
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    int64_t s, orow;
    unsigned sp;
    bool live;
    if constexpr (FWD) {
      s = row / k;
      orow = row;
      const int32_t pos = index[row];
      live = (unsigned)pos < n;
      sp = live ? (unsigned)pos : 0u;
    } else {
      s = row / n;
      sp = (unsigned)(row - s * n);
      const int32_t sl = index[row];
      live = (unsigned)sl < (unsigned)k;
      orow = s * k + (live ? sl : 0);
    }
    const unsigned ph = sp / nw, pw = sp - ph * nw;
    for (unsigned col = threadIdx.x; col < rowlen; col += blockDim.x) {
      const unsigned kf = col / pd, e = col - kf * pd;
      const unsigned p1 = e / pc, r = e - p1 * pc;
      const unsigned p2 = r / C, c = r - p2 * C;
      const int64_t f = s * pt + kf;
      const int64_t xi = ((f * C + c) * H + (int64_t)(ph * P + p1)) * W + (int64_t)(pw * P + p2);
      const int64_t oi = orow * rowlen + col;
      if constexpr (FWD) vecp[oi] = live ? from_f32<D>(to_f32<S>(pixp[xi])) : from_f32<D>(0.f);
      else pixp[xi] = live ? from_f32<S>(to_f32<D>(vecp[oi])) : from_f32<S>(0.f);
    }
  }
}

template <typename S, typename D, bool FWD>
int gather_keep_dispatch(ptr_t<FWD, void> pix, ptr_t<!FWD, void> vec, const int32_t* index, int64_t frames, int C, int H,
                         int W, int P, int pt, int k, hipStream_t st, const char* name) {
  const int nh = H / P, nw = W / P;
  const int64_t seqs = frames / pt;
  const bool vec_ok = (W % 8 == 0) && (P % 8 == 0) && ((P * C) % 8 == 0) && dvt_aligned16(pix) && dvt_aligned16(vec) &&
                      ((int64_t)H * W % 8 == 0);
  auto pixp = (ptr_t<FWD, S>)pix;
  auto vecp = (ptr_t<!FWD, D>)vec;
  const int64_t items = FWD ? seqs * pt * P * k : frames * nh * P * nw;
  if constexpr (FWD && sizeof(D) == 2) {
    const int64_t npatches = frames * k;
    if (vec_ok && P == 16 && C == 3 && npatches < ((int64_t)1 << 31)) {
      int64_t blocks = dvt_cdiv(dvt_cdiv(npatches, 4), 4);
      const int64_t cap = (int64_t)dvt_num_cus() * 16;
      if (blocks > cap) blocks = cap;
      hipLaunchKernelGGL((gather_keep_p16_fwd_kernel<S, D>), dim3((unsigned)blocks), dim3(256), 0, st, pixp, vecp, index,
                         (unsigned)npatches, H, W, (unsigned)nw, (unsigned)(nh * nw), (unsigned)pt, (unsigned)k);
      DVT_LAUNCH_CHECK(name);
      return DVT_OK;
    }
  }
  if (vec_ok && P == 16 && C == 3) {
    hipLaunchKernelGGL((gather_keep_vec_kernel<16, 3, S, D, FWD>), dim3(dvt_grid(items)), dim3(kBlock), 0, st, pixp, vecp,
                       index, seqs, H, W, pt, k);
  } else if (vec_ok && P == 8 && C == 3) {
    hipLaunchKernelGGL((gather_keep_vec_kernel<8, 3, S, D, FWD>), dim3(dvt_grid(items)), dim3(kBlock), 0, st, pixp, vecp,
                       index, seqs, H, W, pt, k);
  } else {
    if ((int64_t)P * P * C * pt >= ((int64_t)1 << 31)) DVT_UNSUPPORTED("%s: a row of pt*P*P*C >= 2^31 elements", name);
    const int64_t rows = seqs * (FWD ? (int64_t)k : (int64_t)nh * nw);
    hipLaunchKernelGGL((gather_keep_scalar_kernel<S, D, FWD>), dim3(dvt_grid(rows * kBlock)), dim3(kBlock), 0, st, pixp,
                       vecp, index, seqs, C, H, W, P, pt, k);
  }
  DVT_LAUNCH_CHECK(name);
  return DVT_OK;
}

// pix: x (forward, read) / dx (adjoint, written); vec: out (forward, written) / dout (adjoint, read); index: keep / slot
template <bool FWD>
int gather_keep_entry(ptr_t<FWD, void> pix, int pix_dtype, ptr_t<!FWD, void> vec, int vec_dtype, const int32_t* index,
                      int64_t frames, int C, int H, int W, int P, int pt, int k, dvt_stream_t stream, const char* name) {
  DVT_REQUIRE(pix && vec && index, "%s: null pointer", name);
  DVT_REQUIRE(pt >= 1, "%s: tubelet length %d < 1", name, pt);
  DVT_REQUIRE(frames >= 0 && C > 0 && H > 0 && W > 0 && P > 0, "%s: bad sizes", name);
  DVT_REQUIRE(frames % pt == 0, "%s: %lld frames are not whole tubelets of %d", name, (long long)frames, pt);
  DVT_REQUIRE(H % P == 0 && W % P == 0, "%s: image %dx%d not divisible by patch %d", name, H, W, P);
  DVT_REQUIRE((int64_t)(H / P) * (W / P) < ((int64_t)1 << 31), "%s: 2^31 positions or more per frame", name);
  DVT_REQUIRE(k >= 1 && k <= (H / P) * (W / P), "%s: k = %d outside 1 .. n = %d", name, k, (H / P) * (W / P));
  if (frames == 0) return DVT_OK;
  hipStream_t st = (hipStream_t)stream;
#define DVT_KEEP_CASE(PD, S, VD, D) \
  if (pix_dtype == PD && vec_dtype == VD) \
    return gather_keep_dispatch<S, D, FWD>(pix, vec, index, frames, C, H, W, P, pt, k, st, name);
  DVT_KEEP_CASE(DVT_F32, float, DVT_F32, float)
  DVT_KEEP_CASE(DVT_F32, float, DVT_BF16, bf16)
  DVT_KEEP_CASE(DVT_F32, float, DVT_F16, f16)
  DVT_KEEP_CASE(DVT_BF16, bf16, DVT_BF16, bf16)
  DVT_KEEP_CASE(DVT_F16, f16, DVT_F16, f16)
  DVT_KEEP_CASE(DVT_BF16, bf16, DVT_F32, float)
  DVT_KEEP_CASE(DVT_F16, f16, DVT_F32, float)
#undef DVT_KEEP_CASE
  DVT_UNSUPPORTED("%s: dtype pair (%d, %d) not supported", name, pix_dtype, vec_dtype);
}

// ------------------------------------------------------------------ token assembly on kept rows
template <typename T>
__global__ void tokens_keep_fwd_kernel(const T* __restrict__ emb, const float* __restrict__ cls, const float* __restrict__ pos,
                                       const int32_t* __restrict__ keep, T* __restrict__ out, int64_t S, int64_t Tn, int n,
                                       int k, int64_t d, int64_t pos_rows) {
  const int64_t dv = d >> 3;
  const int64_t items = S * (k + 1) * dv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const int64_t c = (it % dv) << 3;
    const int64_t row = it / dv;
    const int64_t j = row % (k + 1);
    const int64_t s = row / (k + 1);
    float v[8], p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (j == 0) {
      load8<float>(cls + c, v);
      load8<float>(pos + ((s % Tn) * pos_rows) * d + c, p);
    } else {
      load8<T>(emb + (s * k + (j - 1)) * d + c, v);
      const int32_t q = keep[s * k + (j - 1)];
      if ((unsigned)q < (unsigned)n) load8<float>(pos + ((s % Tn) * pos_rows + 1 + q) * d + c, p);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += p[e];
    store8<T>(out + row * d + c, v);
  }
}

// item = 8 columns of one positional row (tau, j); j >= 1 walks the b sequences of tau in ascending order
template <typename T>
__global__ void tokens_keep_bwd_kernel(const T* __restrict__ dout, const int32_t* __restrict__ slot, float* __restrict__ dpos,
                                       T* __restrict__ demb, int64_t S, int64_t Tn, int n, int k, int64_t d,
                                       int64_t pos_rows, int accumulate) {
  const int64_t dv = d >> 3;
  const int64_t items = Tn * pos_rows * dv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t B = S / Tn;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const int64_t c = (it % dv) << 3;
    const int64_t row = it / dv;
    const int64_t j = row % pos_rows;
    const int64_t t = row / pos_rows;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool any = false;
    if (j <= n) {
      for (int64_t b = 0; b < B; ++b) {
        const int64_t s = b * Tn + t;
        int64_t src = 0;                                       // row of dout[s]
        if (j >= 1) {
          const int32_t sl = slot[s * n + (j - 1)];
          if ((unsigned)sl >= (unsigned)k) continue;
          src = 1 + sl;
        }
        float v[8];
        load8<T>(dout + (s * (k + 1) + src) * d + c, v);
        if (demb && j >= 1) store8<T>(demb + (s * k + src - 1) * d + c, v);
        any = true;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += v[e];
      }
    }
    float* o = dpos + row * d + c;
    if (accumulate) {
      if (!any) continue;                                      // nobody kept this position: the row stays as it is
      float p[8];
      load8<float>(o, p);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += p[e];
    }
    store8<float>(o, acc);
  }
}

// out[c] (+)= sum_{s < S} dout[s * row_stride + c]: one workgroup per 8-column chunk, a fixed order of additions
template <typename T>
__global__ __launch_bounds__(256) void rows0_sum_kernel(const T* __restrict__ dout, int64_t row_stride, int64_t S,
                                                        float* __restrict__ out, int accumulate) {
  __shared__ float red[8][kBlock / 64];
  const int64_t c = (int64_t)blockIdx.x << 3;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t r = threadIdx.x; r < S; r += kBlock) {
    float v[8];
    load8<T>(dout + r * row_stride + c, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += v[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float s = wave_sum(acc[e]);
    if ((threadIdx.x & 63) == 0) red[e][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    float t = 0.f;
    for (int i = 0; i < kBlock / 64; ++i) t += red[threadIdx.x][i];
    float* o = out + c + threadIdx.x;
    *o = accumulate ? *o + t : t;
  }
}

int keep_args(const char* name, int64_t R, int n, int k, int rows_per) {
  DVT_REQUIRE(R >= 0 && R < ((int64_t)1 << 31), "%s: %lld key rows", name, (long long)R);
  DVT_REQUIRE(n >= 1 && n <= kMaxN, "%s: n = %d outside 1 .. %d", name, n, kMaxN);
  DVT_REQUIRE(k >= 1 && k <= n, "%s: k = %d outside 1 .. n = %d", name, k, n);
  DVT_REQUIRE(rows_per >= 1, "%s: rows_per = %d < 1", name, rows_per);
  return DVT_OK;
}
}  // namespace

extern "C" {

int dvt_keep_select(const int32_t* keys, int64_t R, int n, int k, int rows_per, int32_t* keep, int32_t* slot,
                    dvt_stream_t stream) {
  DVT_REQUIRE(keys && keep && slot, "dvt_keep_select: null pointer");
  if (int rc = keep_args("dvt_keep_select", R, n, k, rows_per)) return rc;
  if (R == 0) return DVT_OK;
  hipLaunchKernelGGL((keep_kernel<false>), dim3((unsigned)R), dim3(kBlock), 0, (hipStream_t)stream, keys,
                     (const uint64_t*)nullptr, (uint64_t)0, n, k, rows_per, keep, slot, (int32_t*)nullptr);
  DVT_LAUNCH_CHECK("dvt_keep_select");
  return DVT_OK;
}

int dvt_keep_draw(const uint64_t* rng_state, uint64_t call_offset, int64_t R, int n, int k, int rows_per, int32_t* keep,
                  int32_t* slot, int32_t* keys_out, dvt_stream_t stream) {
  DVT_REQUIRE(rng_state, "dvt_keep_draw: null rng_state");
  DVT_REQUIRE((keep && slot) || (!keep && !slot && keys_out), "dvt_keep_draw: keep and slot together, or keys_out alone");
  if (int rc = keep_args("dvt_keep_draw", R, n, k, rows_per)) return rc;
  if (R == 0) return DVT_OK;
  hipLaunchKernelGGL((keep_kernel<true>), dim3((unsigned)R), dim3(kBlock), 0, (hipStream_t)stream, (const int32_t*)nullptr,
                     rng_state, call_offset, n, k, rows_per, keep, slot, keys_out);
  DVT_LAUNCH_CHECK("dvt_keep_draw");
  return DVT_OK;
}

int dvt_keep_slots(const int32_t* keep, int64_t S, int n, int k, int32_t* slot, dvt_stream_t stream) {
  DVT_REQUIRE(keep && slot, "dvt_keep_slots: null pointer");
  if (int rc = keep_args("dvt_keep_slots", S, n, k, 1)) return rc;
  if (S == 0) return DVT_OK;
  hipLaunchKernelGGL(slots_kernel, dim3((unsigned)S), dim3(kBlock), 0, (hipStream_t)stream, keep, n, k, slot);
  DVT_LAUNCH_CHECK("dvt_keep_slots");
  return DVT_OK;
}

int dvt_patchify_keep(const void* x, int x_dtype, void* out, int out_dtype, const int32_t* keep, int64_t frames, int C, int H,
                      int W, int P, int pt, int k, dvt_stream_t stream) {
  return gather_keep_entry<true>(x, x_dtype, out, out_dtype, keep, frames, C, H, W, P, pt, k, stream, "dvt_patchify_keep");
}

int dvt_patchify_keep_bwd(const void* dout, int dout_dtype, void* dx, int dx_dtype, const int32_t* slot, int64_t frames, int C,
                          int H, int W, int P, int pt, int k, dvt_stream_t stream) {
  return gather_keep_entry<false>(dx, dx_dtype, dout, dout_dtype, slot, frames, C, H, W, P, pt, k, stream,
                                  "dvt_patchify_keep_bwd");
}

int dvt_tokens_assemble_keep_fwd(const void* emb, const float* cls, const float* pos, const int32_t* keep, void* out,
                                 int64_t S, int64_t T, int n, int k, int64_t d, int64_t pos_rows, int dtype,
                                 dvt_stream_t stream) {
  DVT_REQUIRE(emb && cls && pos && keep && out, "dvt_tokens_assemble_keep_fwd: null pointer");
  DVT_REQUIRE(S >= 0 && T > 0 && n >= 1 && d > 0 && S % T == 0, "dvt_tokens_assemble_keep_fwd: bad sizes");
  DVT_REQUIRE(k >= 1 && k <= n, "dvt_tokens_assemble_keep_fwd: k = %d outside 1 .. n = %d", k, n);
  DVT_REQUIRE(pos_rows >= (int64_t)n + 1, "dvt_tokens_assemble_keep_fwd: positional table has %lld rows < n+1 = %d",
              (long long)pos_rows, n + 1);
  DVT_REQUIRE(d % 8 == 0, "dvt_tokens_assemble_keep_fwd: d = %lld must be a multiple of 8", (long long)d);
  DVT_REQUIRE(dvt_aligned16(emb) && dvt_aligned16(cls) && dvt_aligned16(pos) && dvt_aligned16(out),
              "dvt_tokens_assemble_keep_fwd: buffers must be 16-byte aligned");
  if (S == 0) return DVT_OK;
  const int64_t items = S * (k + 1) * (d >> 3);
  DVT_DISPATCH_DTYPE(dtype, Tt,
                     hipLaunchKernelGGL((tokens_keep_fwd_kernel<Tt>), dim3(dvt_grid(items)), dim3(kBlock), 0,
                                        (hipStream_t)stream, (const Tt*)emb, cls, pos, keep, (Tt*)out, S, T, n, k, d,
                                        pos_rows));
  DVT_LAUNCH_CHECK("dvt_tokens_assemble_keep_fwd");
  return DVT_OK;
}

int dvt_tokens_assemble_keep_bwd(const void* dout, const int32_t* slot, void* demb, float* dcls, float* dpos, int64_t S,
                                 int64_t T, int n, int k, int64_t d, int64_t pos_rows, int dtype, int accumulate,
                                 dvt_stream_t stream) {
  DVT_REQUIRE(dout && slot && demb && dcls && dpos, "dvt_tokens_assemble_keep_bwd: null pointer");
  DVT_REQUIRE(S > 0 && T > 0 && n >= 1 && d > 0 && S % T == 0, "dvt_tokens_assemble_keep_bwd: bad sizes");
  DVT_REQUIRE(k >= 1 && k <= n, "dvt_tokens_assemble_keep_bwd: k = %d outside 1 .. n = %d", k, n);
  DVT_REQUIRE(pos_rows >= (int64_t)n + 1 && d % 8 == 0, "dvt_tokens_assemble_keep_bwd: bad pos_rows / d");
  DVT_REQUIRE(dvt_aligned16(dout) && dvt_aligned16(demb) && dvt_aligned16(dcls) && dvt_aligned16(dpos),
              "dvt_tokens_assemble_keep_bwd: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t dv = d >> 3;
  DVT_DISPATCH_DTYPE(dtype, Tt, {
    hipLaunchKernelGGL((tokens_keep_bwd_kernel<Tt>), dim3(dvt_grid(T * pos_rows * dv)), dim3(kBlock), 0, st,
                       (const Tt*)dout, slot, dpos, (Tt*)demb, S, T, n, k, d, pos_rows, accumulate);
    hipLaunchKernelGGL((rows0_sum_kernel<Tt>), dim3((unsigned)dv), dim3(kBlock), 0, st, (const Tt*)dout,
                       (int64_t)(k + 1) * d, S, dcls, accumulate);
  });
  DVT_LAUNCH_CHECK("dvt_tokens_assemble_keep_bwd");
  return DVT_OK;
}

}  // extern "C"
