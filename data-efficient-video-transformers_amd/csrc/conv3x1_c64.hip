// conv3x1_c64.hip -- the (3, 1, 1) temporal convolution 64 -> 64 of R(2+1)D-18's STEM (torchvision r2plus1d_18 as used by
// frame_transformer.py:64-74: Conv3d(45, 64, (3, 1, 1), pad (1, 0, 0)) behind the (1, 7, 7) spatial half; the 45 mid planes
// are stored zero-padded to 64) and, with the data-gradient pack of its weights, that layer's data gradient.
//
//   z[n, t, p, co] = sum over kt, ci of x[n, t + kt - 1, p, ci] * W[co][kt * 64 + ci]
//
// The implicit GEMM (gemm256.hip) gathers every pixel of the map once per temporal tap: 130 us per launch at 28 clips of
// 12 x 56^2 for 270 MB of input + output (2 TB/s).  Same scheme as conv3x1_fwd.hip (144 -> 64), with what 64-channel pixels
// change:
//   * window image: the 64-channel format of conv3x1_window.h (144-byte rows); a segment of 16 pixels over T + 2 frames is
//     32 KiB at 12 frames, two of them + the output staging fit with room to spare, so a tile is 16 pixels x all frames
//     (192 positions at 12 frames: half the tiles of the 144-channel kernel per pixel);
//   * eight waves = 4 output-channel blocks of 16 x 2 halves of the tile's position blocks (up to 6 each); a wave's weights
//     (16 output channels x 192: six 16-byte fragments) stay in registers for the whole launch;
//   * 64 channels per tap = two 16x16x32 steps, no 16x16x16 tail;
//   * epilogue as in conv3x1_fwd.hip (out64_tile, conv3x1_window.h): LDS staging image, whole 128-byte pixel rows stored,
//     the BatchNorm column sums of the STORED values carried per thread over the workgroup's tile sequence (optional: the
//     data gradient has no use for them).
#include "conv3x1_window.h"

namespace {

using dvt_window::Window;
using dvt_window::Form;
using F = dvt_window::Fmt64;
constexpr int kC = F::kC, kNW = dvt_window::kNW;
constexpr int kXRow = F::kRow;               // bytes per window position: 8 data slots + 1 padding slot
constexpr int kMaxXP = 5;                    // window DMA pieces (1 KiB) per wave: window <= 40 KiB
constexpr int kMaxPB = 6;                    // 16-position blocks per wave (tile <= 192 positions)

struct TcParams {
  const void* x;        // [N, T, L, 64]
  const void* w;        // [64][ldw] k-major, k = tap * 64 + ci
  void* y;              // [N, T, L, 64]
  float* bn_partial;    // [grid][2][64] or nullptr
  Window w_;
  int ntiles, ldw;
};

template <typename E, int NPB>
__global__ __launch_bounds__(kNW * 64) void conv3x1_c64_kernel(const TcParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using V8 = typename Elem16<E>::v8;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, li = lane & 15;
  const Window& w = p.w_;
  const int S = w.S;
  char* stage = smem + 2 * w.x_bytes;                                            // [KP][64] outputs of a tile, 128-byte rows
  const E* xg = (const E*)p.x;
  unsigned xq[kMaxXP];
  dvt_window::window_coords<F, kNW>(w, wid, lane, xq);
  auto load_tile = [&](int tile, int b) {
    const int n = tile / w.segs, sg = tile - n * w.segs;
    dvt_window::window_load<F, kNW>(w, xg, (int64_t)n * w.T * w.L + (int64_t)sg * S, xq, wid, smem + b * w.x_bytes);
  };

  // ---- this wave: output channels [16 u, 16 u + 16), position blocks pb0 .. pb0 + NPB - 1
  const int u = wid & 3, half = wid >> 2;
  const int pb0 = half * NPB;                                                    // (KP == 32 NPB)
  V8 wf[3][2];                                     // lane (g, li) <-> weight row 16 u + li, k = tap * 64 + 32 kk + 8 g
  {
    const E* wrow = (const E*)p.w + (int64_t)(16 * u + li) * p.ldw;
#pragma unroll
    for (int kt = 0; kt < 3; ++kt)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) wf[kt][kk] = *reinterpret_cast<const V8*>(wrow + kt * kC + kk * 32 + g * 8);
  }
  // byte offset of this lane's x fragments inside a window, per tap: row = position 16 pb0 + li + S kt, slot 4 kk + g
  int xo[3];
#pragma unroll
  for (int kt = 0; kt < 3; ++kt) xo[kt] = (pb0 * 16 + li + kt * S) * kXRow + (g << 4);

  float bs[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int nst = dvt_window::out64_stores(w, wid);
  int tile = blockIdx.x;
  if (tile < p.ntiles) load_tile(tile, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int it = 0; tile < p.ntiles; ++it, tile += gridDim.x) {
    const int cxo = (it & 1) * w.x_bytes;
    if (tile + (int)gridDim.x < p.ntiles) load_tile(tile + gridDim.x, (it + 1) & 1);
    f32x4 acc[NPB];
#pragma unroll
    for (int b = 0; b < NPB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    V8 xf[2][NPB];                                 // (two sets: the next step's reads under this step's MFMAs)
    auto rdx = [&](int st, V8* dst) {              // st = 2 kt + kk
#pragma unroll
      for (int b = 0; b < NPB; ++b)
        dst[b] = *reinterpret_cast<const V8*>(smem + cxo + xo[st >> 1] + b * (16 * kXRow) + (st & 1) * 64);
    };
    rdx(0, xf[0]);
#pragma unroll
    for (int st = 0; st < 6; ++st) {
      if (st + 1 < 6) rdx(st + 1, xf[(st + 1) & 1]);
#pragma unroll
      for (int b = 0; b < NPB; ++b) acc[b] = Elem16<E>::mma(wf[st >> 1][st & 1], xf[st & 1][b], acc[b]);
    }
    {
      const int n = tile / w.segs, sg = tile - n * w.segs;
      dvt_window::out64_tile<E, NPB>(w, stage, acc, u, g, li, pb0, (E*)p.y, (int64_t)n * w.T * w.L + (int64_t)sg * S,
                                     p.bn_partial != nullptr, bs, bq, nst);
    }
    __syncthreads();                                              // everybody is done with this tile's window and staging
  }
  if (p.bn_partial) dvt_window::out64_reduce(reinterpret_cast<float*>(smem), bs, bq, p.bn_partial);      // (over the images)
}

template <typename E, int NPB>
void tc_launch(const TcParams& p, int grid, int lds, hipStream_t st) {
  static DvtLdsAttr set;
  dvt_lds_attr(set, (const void*)conv3x1_c64_kernel<E, NPB>, 160 * 1024);
  hipLaunchKernelGGL((conv3x1_c64_kernel<E, NPB>), dim3(grid), dim3(kNW * 64), lds, st, p);
}

}  // namespace

namespace dvt_internal {

// the launcher's choice: two windows + the output staging [KP][64]; inst = position blocks per wave, the template parameter of
// conv3x1_c64_kernel (KP is a multiple of 32, at most 32 kMaxPB)
Form conv3x1_c64_form(int64_t N, int T, int L) {
  Window q;
  if (N <= 0 || !dvt_window::window_plan<F>(T, L, &q, 0, 128, 2, kNW * kMaxXP, 4096, 32 * kMaxPB)) return Form{};
  int lds = 2 * q.x_bytes + q.KP * 128;
  if (lds < 2 * kNW * 64 * 8 * 4) lds = 2 * kNW * 64 * 8 * 4;      // (the statistics scratch [2][512][8] overlays the images)
  return dvt_window::window_form(N, q, 0, q.KP >> 5, lds);
}

// (arguments checked by dvt_conv3x1_fwd; f = conv3x1_c64_form of the same geometry, launchable)
void conv3x1_c64_fwd(const Form& f, const void* x, const void* w, int64_t ldw, void* y, float* stats_partial, int64_t N, int dtype,
                    hipStream_t st) {
  TcParams p{};
  p.w_ = f.w;
  p.x = x; p.w = w; p.y = y; p.bn_partial = stats_partial; p.ldw = (int)ldw;
  p.ntiles = (int)(N * p.w_.segs);
  const bool h = dtype == DVT_F16;
  switch (f.inst) {
    case 1: h ? tc_launch<f16, 1>(p, f.grid, f.lds, st) : tc_launch<bf16, 1>(p, f.grid, f.lds, st); break;
    case 2: h ? tc_launch<f16, 2>(p, f.grid, f.lds, st) : tc_launch<bf16, 2>(p, f.grid, f.lds, st); break;
    case 3: h ? tc_launch<f16, 3>(p, f.grid, f.lds, st) : tc_launch<bf16, 3>(p, f.grid, f.lds, st); break;
    case 4: h ? tc_launch<f16, 4>(p, f.grid, f.lds, st) : tc_launch<bf16, 4>(p, f.grid, f.lds, st); break;
    case 5: h ? tc_launch<f16, 5>(p, f.grid, f.lds, st) : tc_launch<bf16, 5>(p, f.grid, f.lds, st); break;
    default: h ? tc_launch<f16, 6>(p, f.grid, f.lds, st) : tc_launch<bf16, 6>(p, f.grid, f.lds, st); break;
  }
}

}  // namespace dvt_internal
