// drop_path.hip -- stochastic depth (timm's DropPath on `x = fn(x) + x`, src/models/vit.py:73-74) on whole sequences.
//
// A stack holds S sequences, each one contiguous row of L = N d elements of a [S, N, d] tensor.  A residual branch runs on a
// subset of them (DINOv2's "efficient stochastic depth"): gather the kept rows, run the branch on those, add the result back
// scaled.  The two streaming kernels are each other's adjoints and serve both directions:
//
//   seq_gather_kernel        y[j]   = alpha x[idx[j]]                where 0 <= idx[j] < S, else a row of zeros
//   seq_scatter_add_kernel   out[s] = fmaf(alpha, y[slot[s]], res[s]) where 0 <= slot[s] < k, else res[s]
//
//   forward    xg = gather(x, keep, 1);  yb = branch(xg);  out = scatter_add(x, yb, slot, S/k)
//   backward   dyb = gather(g, keep, S/k);  dxg = branch'(dyb);  dx = scatter_add(g, dxg, slot, 1)
//
// Work item = a tile of kTile 16-byte slots of one row (a scalar form takes one element per slot when the row length or a
// base pointer does not allow 16-byte accesses); workgroups walk the (row, tile) list grid-stride.  The row index is read
// once per tile (wave-uniform) and compared as unsigned against its bound before any address is formed from it.  A lane
// issues every load of its slots before its first store.  Every output row is written exactly once, by the tiles of that
// row: no atomics, no zero-filled intermediate, bitwise repeatable.  In scatter_add a lane reads a slot of `res` before it
// writes the same slot of `out` and no other lane touches that slot, so out may alias res.
//
//   drop_path_draw_kernel    m[s] = s with probability 1 - p, else -1: Philox word (s & 3) of block base + s / 4 of the
//                            dropout generator's device state (a replayed graph draws anew on every step).  With
//                            idx = slot = m and k = S the two kernels above are timm's per-sample rule.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kUnroll = 2;                        // slots per lane in flight (scatter_add: two loads each)
constexpr int kTile = kBlock * kUnroll;           // slots of one workgroup pass over a row

template <typename T, int VE> struct SlotVec { typedef T type __attribute__((ext_vector_type(VE))); };
template <typename T> struct SlotVec<T, 1> { typedef T type; };

template <typename T, int VE>
__device__ __forceinline__ T lane_of(const typename SlotVec<T, VE>::type& v, int j) {
  if constexpr (VE == 1) return v;
  else return v[j];
}
template <typename T, int VE>
__device__ __forceinline__ void set_lane(typename SlotVec<T, VE>::type& v, int j, T e) {
  if constexpr (VE == 1) v = e;
  else v[j] = e;
}

// VE elements per slot: 16 / sizeof(T) (vector form) or 1 (scalar form).  slots = L / VE.
template <typename T, int VE>
__global__ __launch_bounds__(kBlock) void seq_gather_kernel(const T* __restrict__ x, const int32_t* __restrict__ idx,
                                                            T* __restrict__ y, int64_t S, int64_t k, int64_t L,
                                                            int64_t slots, int64_t tiles, float alpha) {
  typedef typename SlotVec<T, VE>::type vec;
  const int64_t work = k * tiles;
  for (int64_t w = blockIdx.x; w < work; w += gridDim.x) {
    const int64_t j = w / tiles, tile = w - j * tiles;
    const int32_t src = idx[j];
    const bool live = (uint64_t)(int64_t)src < (uint64_t)S;          // negative values wrap above any S
    const vec* xs = reinterpret_cast<const vec*>(x + (live ? (int64_t)src : 0) * L);
    vec* yd = reinterpret_cast<vec*>(y + j * L);
    const int64_t s0 = tile * kTile + threadIdx.x;
    vec v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t s = s0 + u * kBlock;
      if (live && s < slots) v[u] = xs[s];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t s = s0 + u * kBlock;
      if (s >= slots) continue;
      vec r;
#pragma unroll
      for (int e = 0; e < VE; ++e)
        set_lane<T, VE>(r, e, from_f32<T>(live ? alpha * to_f32<T>(lane_of<T, VE>(v[u], e)) : 0.f));
      yd[s] = r;
    }
  }
}

// res / out carry no __restrict__: they may be the same buffer
template <typename T, int VE>
__global__ __launch_bounds__(kBlock) void seq_scatter_add_kernel(const T* res, const T* __restrict__ y,
                                                                 const int32_t* __restrict__ slot, T* out, int64_t S,
                                                                 int64_t k, int64_t L, int64_t slots, int64_t tiles,
                                                                 float alpha) {
  typedef typename SlotVec<T, VE>::type vec;
  const int64_t work = S * tiles;
  for (int64_t w = blockIdx.x; w < work; w += gridDim.x) {
    const int64_t row = w / tiles, tile = w - row * tiles;
    const int32_t sl = slot[row];
    const bool live = (uint64_t)(int64_t)sl < (uint64_t)k;
    const vec* rs = reinterpret_cast<const vec*>(res + row * L);
    const vec* ys = reinterpret_cast<const vec*>(y + (live ? (int64_t)sl : 0) * L);
    vec* od = reinterpret_cast<vec*>(out + row * L);
    const int64_t s0 = tile * kTile + threadIdx.x;
    vec a[kUnroll], b[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t s = s0 + u * kBlock;
      if (s < slots) {
        a[u] = rs[s];
        if (live) b[u] = ys[s];
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t s = s0 + u * kBlock;
      if (s >= slots) continue;
      vec r = a[u];
      if (live) {
#pragma unroll
        for (int e = 0; e < VE; ++e)
          set_lane<T, VE>(r, e, from_f32<T>(fmaf(alpha, to_f32<T>(lane_of<T, VE>(b[u], e)),
                                                 to_f32<T>(lane_of<T, VE>(a[u], e)))));
      }
      od[s] = r;
    }
  }
}

__global__ __launch_bounds__(kBlock) void drop_path_draw_kernel(const uint64_t* __restrict__ state, uint64_t call_offset,
                                                                int64_t S, uint32_t threshold, int32_t* __restrict__ m) {
  const uint64_t seed = state[0], base = state[1] + call_offset;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += stride)
    m[s] = dvt_dropout_keep(seed, base, (uint64_t)s, threshold) ? (int32_t)s : -1;
}

// (rows of work) x (tiles per row) workgroup passes, at most CUs x 8 workgroups
int seq_grid(int64_t rows, int64_t tiles) {
  const int64_t work = rows * tiles, cap = (int64_t)dvt_num_cus() * 8;
  return (int)(work < 1 ? 1 : (work > cap ? cap : work));
}

int seq_args(const char* name, int64_t S, int64_t k, int64_t L) {
  DVT_REQUIRE(S >= 1 && S < ((int64_t)1 << 31), "%s: S = %lld outside 1 .. 2^31 - 1", name, (long long)S);
  DVT_REQUIRE(k >= 1 && k < ((int64_t)1 << 31), "%s: k = %lld outside 1 .. 2^31 - 1", name, (long long)k);
  DVT_REQUIRE(L >= 1 && L < ((int64_t)1 << 40), "%s: row length L = %lld outside 1 .. 2^40 - 1", name, (long long)L);
  return DVT_OK;
}

template <typename T>
bool vec_ok(int64_t L, const void* a, const void* b, const void* c) {
  return (L * (int64_t)sizeof(T)) % 16 == 0 && dvt_aligned16(a) && dvt_aligned16(b) && dvt_aligned16(c);
}

}  // namespace

extern "C" {

int dvt_seq_gather(const void* x, const int32_t* idx, void* y, int64_t S, int64_t k, int64_t L, float alpha, int dtype,
                   dvt_stream_t stream) {
  DVT_REQUIRE(x && idx && y, "dvt_seq_gather: null pointer");
  if (int rc = seq_args("dvt_seq_gather", S, k, L)) return rc;
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T, {
    constexpr int VE = 16 / (int)sizeof(T);
    if (vec_ok<T>(L, x, y, y)) {
      const int64_t slots = L / VE, tiles = dvt_cdiv(slots, kTile);
      hipLaunchKernelGGL((seq_gather_kernel<T, VE>), dim3(seq_grid(k, tiles)), dim3(kBlock), 0, st, (const T*)x, idx, (T*)y,
                         S, k, L, slots, tiles, alpha);
    } else {
      const int64_t tiles = dvt_cdiv(L, kTile);
      hipLaunchKernelGGL((seq_gather_kernel<T, 1>), dim3(seq_grid(k, tiles)), dim3(kBlock), 0, st, (const T*)x, idx, (T*)y,
                         S, k, L, L, tiles, alpha);
    }
  });
  DVT_LAUNCH_CHECK("dvt_seq_gather");
  return DVT_OK;
}

int dvt_seq_scatter_add(const void* res, const void* y, const int32_t* slot, void* out, int64_t S, int64_t k, int64_t L,
                        float alpha, int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(res && y && slot && out, "dvt_seq_scatter_add: null pointer");
  if (int rc = seq_args("dvt_seq_scatter_add", S, k, L)) return rc;
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T, {
    constexpr int VE = 16 / (int)sizeof(T);
    if (vec_ok<T>(L, res, y, out)) {
      const int64_t slots = L / VE, tiles = dvt_cdiv(slots, kTile);
      hipLaunchKernelGGL((seq_scatter_add_kernel<T, VE>), dim3(seq_grid(S, tiles)), dim3(kBlock), 0, st, (const T*)res,
                         (const T*)y, slot, (T*)out, S, k, L, slots, tiles, alpha);
    } else {
      const int64_t tiles = dvt_cdiv(L, kTile);
      hipLaunchKernelGGL((seq_scatter_add_kernel<T, 1>), dim3(seq_grid(S, tiles)), dim3(kBlock), 0, st, (const T*)res,
                         (const T*)y, slot, (T*)out, S, k, L, L, tiles, alpha);
    }
  });
  DVT_LAUNCH_CHECK("dvt_seq_scatter_add");
  return DVT_OK;
}

int dvt_drop_path_draw(const uint64_t* rng_state, uint64_t call_offset, int64_t S, float p, int32_t* m,
                       dvt_stream_t stream) {
  DVT_REQUIRE(rng_state && m, "dvt_drop_path_draw: null pointer");
  DVT_REQUIRE(S >= 1 && S < ((int64_t)1 << 31), "dvt_drop_path_draw: S = %lld outside 1 .. 2^31 - 1", (long long)S);
  DVT_REQUIRE(p >= 0.f && p < 1.f, "dvt_drop_path_draw: p = %g outside [0, 1)", (double)p);
  // keep iff word >= threshold, threshold = round(p * 2^32): dvt_dropout's rule
  const double th = (double)p * 4294967296.0;
  const uint32_t threshold = th >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)(th + 0.5);
  hipLaunchKernelGGL(drop_path_draw_kernel, dim3(dvt_grid(S)), dim3(kBlock), 0, (hipStream_t)stream, rng_state, call_offset, S,
                     threshold, m);
  DVT_LAUNCH_CHECK("dvt_drop_path_draw");
  return DVT_OK;
}

}  // extern "C"
