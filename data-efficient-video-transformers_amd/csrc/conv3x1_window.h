// conv3x1_window.h -- the LDS "window" of the (3, 1, 1) temporal convolutions of R(2+1)D-18 (video_resnet.py:30-31), stated
// once for the whole family: the forward 144 -> 64 (conv3x1_fwd.hip) and its weight gradient (conv3x1_wgrad.hip) on the
// 144-plane map, the stem's 64 -> 64 (conv3x1_c64.hip) and the data gradient 64 -> 144 (conv3x1_dbn.hip) on a 64-plane map.
//
// A workgroup owns a segment of S pixels of one clip over ALL its T frames and stages the (T + 2) x S x C window of the
// C-plane map once (frames -1 and T are zero rows); the three taps are the position offsets 0 / S / 2S into it.  The image
// comes in two formats (Fmt144, Fmt64 below: a format is its row and the channel each 16-byte slot of a row holds):
//   * Fmt144: [position][144 channels] in rows of TEN 32-byte units (320 bytes): nine channel blocks of 16 plus one unit of
//     padding, block cb of position k stored at unit cb + ((k >> 3) & 1).  A 32-lane half of ds_read_b64_tr_b16 touches the
//     positions {q, 8 + q} + 4 hf: 320-byte rows put positions q = 0 .. 3 on banks 0 / 16 / 32 / 48 (+ 8 each) and the
//     one-unit shift moves positions 8 + q to banks 8 / 24 / 40 / 56 -- the eight 8-bank groups of one LDS cycle.  (No
//     linear pitch does that: positions k and k + 8 are 8 rows apart, a multiple of 256 bytes for every 32-byte-multiple
//     pitch.)  The same image serves ds_read_b128 row fragments (16 positions x 16 bytes: four 16-lane access groups, each
//     over 64 distinct banks).  The DMA is lane-linear, so the layout lives on the per-lane source address: slot = 16
//     bytes, 20 slots per position, two of them zero padding.
//   * Fmt64: [position][64 channels] as eight 16-byte slots + one slot of padding = 144-byte rows (9 is odd: the sixteen
//     positions of a ds_read_b128 access group land on sixteen different 16-byte bank groups).
//   * optional "virtual" BatchNorm: the map in HBM is the convolution output z of the layer in front;
//     the normalised activation y = relu(z * s + t) -- the formula and the rounding of dvt_bn_apply_fwd (BnAffine::apply,
//     conv.hip) -- is formed in the staged window, once per tile, by window_transform; the two zero rows stay zero.
#pragma once
#include "common.h"

namespace dvt_window {

// ---- the two formats: channels per pixel of the map, bytes and 16-byte slots per window position, and the channel whose
// 16-byte chunk slot h of position pos holds (-1: a padding slot, never loaded)
struct Fmt144 {
  static constexpr int kC = 144, kRow = 320, kSlots = 20;
  static constexpr int kCB = kC / 16;                                  // 9 channel blocks, block cb at unit cb + ((pos >> 3) & 1)
  static __host__ __device__ __forceinline__ int channel(int pos, int h) {
    const int cb = (h >> 1) - ((pos >> 3) & 1);
    return cb >= 0 && cb < kCB ? cb * 16 + (h & 1) * 8 : -1;
  }
};
struct Fmt64 {
  static constexpr int kC = 64, kRow = 144, kSlots = 9;
  static __host__ __device__ __forceinline__ int channel(int, int h) { return h < 8 ? h * 8 : -1; }
};

constexpr int kCI = Fmt144::kC, kCO = 64, kNW = 8;
constexpr int kCB = Fmt144::kCB;             // 9 input-channel blocks
constexpr int kXU = kCB + 1;                 // 32-byte units per position (one of padding)
constexpr int kXRow = Fmt144::kRow;          // 320 bytes
constexpr int kMaxXP = 6;                    // window DMA pieces (1 KiB) per wave: window <= 48 KiB
constexpr int kNoCap = 1 << 30;

// geometry of a launch (host: window_plan); the same for both formats
struct Window {
  int T, L, S, segs;    // frames, pixels per frame, pixels per segment, segments per frame
  int KP;               // T * S: positions of an output / gradient tile (multiple of 32)
  int xpos;             // (T + 2) * S: positions of a window
  int x_bytes;          // window image size (multiple of 1 KiB)
};

// the BatchNorm (+ ReLU) in front of the map, or mean == nullptr (the map already holds the normalised activation)
struct Affine {
  const float* mean;
  const float* invstd;
  const float* gamma;
  const float* beta;
  int c_valid, relu;
};

// The one segment search: the longest S <= 16 that divides L, makes the tile a multiple of 32 positions (at most max_kp) and
// fits the caller's LDS plan -- nbuf windows, extra_bytes_per_buffer / extra_bytes_once further bytes per tile position,
// `reserve` bytes kept free -- with a window of at most max_pieces 1 KiB DMA pieces (what the carrying waves take between them).
template <typename F>
inline int window_plan(int T, int L, Window* q, int extra_bytes_per_buffer, int extra_bytes_once, int nbuf, int max_pieces,
                       int reserve = 4096, int max_kp = kNoCap) {
  if (T < 1 || L < 1 || T + 2 > 2047) return 0;
  for (int S = 16; S >= 2; --S) {
    if (L % S || (T * S) % 32) continue;
    const int KP = T * S, xpos = (T + 2) * S;
    if (KP > max_kp) continue;
    const int xbytes = (xpos * F::kRow + 1023) & ~1023;
    if (nbuf * (xbytes + extra_bytes_per_buffer * KP) + extra_bytes_once * KP + reserve > 160 * 1024) continue;
    if ((xbytes >> 10) > max_pieces) continue;
    q->T = T; q->L = L; q->S = S; q->segs = L / S; q->KP = KP; q->xpos = xpos; q->x_bytes = xbytes;
    return 1;
  }
  return 0;
}

// persistent grid: one workgroup per CU, or per tile where there are fewer
inline int window_grid(int64_t N, const Window& q) {
  const int64_t ntiles = N * q.segs;
  return (int)(ntiles < dvt_num_cus() ? ntiles : dvt_num_cus());
}

// What a launcher has chosen for (N, T, L): every query of an operator (*_supported, *_plan, *_parts, *_workspace_bytes) and
// its launch read ONE of these, so that statistics rows and workspace bytes cannot disagree with the launch.
struct Form {
  Window w;
  int taken;            // N > 0 and a segment length exists (grid, lds, inst, pipelined are then set)
  int addressable;      // tile and element counts stay below 2^31
  int pipelined;        // the form with helper waves
  int inst;             // the kernel's instantiation parameter (position blocks per wave / per tile); 0 where it has none
  int grid, lds;
  bool launchable(int dtype) const { return taken && addressable && dvt_is_16bit(dtype); }
};
// (elems_per_pixel: what the kernel's 32-bit offsets count per pixel of the map)
inline Form window_form(int64_t N, const Window& q, int pipelined, int inst, int lds, int elems_per_pixel = 1) {
  Form f{};
  f.w = q; f.taken = 1; f.pipelined = pipelined; f.inst = inst; f.lds = lds;
  f.grid = window_grid(N, q);
  f.addressable = N * q.segs < ((int64_t)1 << 31) && N * q.T * q.L * elems_per_pixel < ((int64_t)1 << 31);
  return f;
}

#ifdef __HIPCC__
__device__ __attribute__((aligned(16))) static unsigned int window_zero16[4] = {0u, 0u, 0u, 0u};

// per-lane coordinates of this wave's window DMA pieces (fixed for the launch; wid: the wave's index among the NWAVES that
// carry the DMA): frame row << 20 | pixel of the segment << 8 | channel (multiple of 8) of the 16-byte chunk, bit 31 = never
// loaded (padding slot / past the window)
template <typename F, int NWAVES, int MAXP>
__device__ __forceinline__ void window_coords(const Window& w, int wid, int lane, unsigned (&xq)[MAXP]) {
  const int xp = w.x_bytes >> 10;
#pragma unroll
  for (int i = 0; i < MAXP; ++i) {
    const int piece = wid + NWAVES * i;
    const int sl = piece * 64 + lane;
    const int pos = sl / F::kSlots, h = sl - pos * F::kSlots;
    const int c = F::channel(pos, h);
    const int tt = pos / w.S, sx = pos - tt * w.S;
    const bool ok = piece < xp && pos < w.xpos && c >= 0;
    xq[i] = ok ? ((unsigned)tt << 20) | ((unsigned)sx << 8) | (unsigned)c : 0x80000000u;
  }
}

// request this wave's pieces of the window of (clip pixel base pix0 = frame 0, first pixel of the segment)
template <typename F, int NWAVES, typename E, int MAXP>
__device__ __forceinline__ void window_load(const Window& w, const E* xg, int64_t pix0, const unsigned (&xq)[MAXP], int wid,
                                            char* dst) {
  const int xp = w.x_bytes >> 10;
#pragma unroll
  for (int i = 0; i < MAXP; ++i) {
    const int piece = wid + NWAVES * i;
    if (piece < xp) {                            // wave-uniform
      const int frame = (int)((xq[i] >> 20) & 0x7FF) - 1;
      const bool ok = (int)xq[i] >= 0 && (unsigned)frame < (unsigned)w.T;
      const E* src = ok ? xg + (pix0 + (int64_t)frame * w.L + ((xq[i] >> 8) & 0xFFF)) * F::kC + (xq[i] & 0xFF)
                        : reinterpret_cast<const E*>(window_zero16);
      dvt_dma16(src, dst + piece * 1024);
    }
  }
}

// ---- the 64-channel output epilogue of the forward kernels without helper waves (conv3x1_fwd_kernel, conv3x1_c64_kernel:
// eight waves = 4 output-channel blocks u x 2 halves of the tile's position blocks, pb0 = the wave's first block).
// out64_tile: lane (g, li) holds z[position (pb0 + b) * 16 + li][16 u + 4 g .. + 3] in acc[b]; the tile goes through the
// XOR-swizzled staging image [KP][64] (128-byte rows) and leaves as whole 128-byte pixel rows, the BatchNorm column sums /
// sums of squares of the STORED values carried per thread (a thread always stores the same 8 channels).  One barrier inside
// (staging complete); the barriers around it are the caller's.
template <typename E, int NPB>
__device__ __forceinline__ void out64_tile(const Window& w, char* stage, const f32x4 (&acc)[NPB], int u, int g, int li, int pb0,
                                           E* yg, int64_t pix0, bool stats, float (&bs)[8], float (&bq)[8], int nst) {
  using V8 = typename Elem16<E>::v8;
  using V4 = typename Elem16<E>::v4;
#pragma unroll
  for (int b = 0; b < NPB; ++b) {
    V4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (E)acc[b][r];
    const int pos = (pb0 + b) * 16 + li;
    *reinterpret_cast<V4*>(stage + pos * 128 + (((2 * u + (g >> 1)) ^ (pos & 7)) << 4) + ((g & 1) << 3)) = o;
  }
  __syncthreads();                               // staging complete
  {
    const int c = threadIdx.x & 7;               // this thread's 8 channels, the same for every tile
    for (int r = threadIdx.x >> 3; r < w.KP; r += (kNW * 64) >> 3) {
      const V8 v = *reinterpret_cast<const V8*>(stage + r * 128 + ((c ^ (r & 7)) << 4));
      const int t = r / w.S, sx = r - t * w.S;
      *reinterpret_cast<V8*>(yg + (pix0 + (int64_t)t * w.L + sx) * kCO + c * 8) = v;
      if (stats) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float f = (float)v[k];
          bs[k] += f;
          bq[k] = fmaf(f, f, bq[k]);
        }
      }
    }
  }
  // the next window has landed; this tile's stores (issued behind its requests, nst <= 3 per thread: vmcnt counts in
  // issue order) stay in flight -- waiting for them as well cost ~3 us per tile, 130 us per launch
  dvt_wait_vm_upto<3>(nst);
}
// output rows (= stores) per thread and tile of out64_tile, wave-uniform
__device__ __forceinline__ int out64_stores(const Window& w, int wid) { return wid * 8 < w.KP ? (w.KP - wid * 8 + 63) >> 6 : 0; }

// the carried sums -> this workgroup's partial row [2][64]: threads with equal (tid & 7) hold the same 8 channels, summed in
// a fixed order through red = [2][512][8] floats (32 KiB of LDS that nobody reads any more)
__device__ __forceinline__ void out64_reduce(float* red, const float (&bs)[8], const float (&bq)[8], float* bn_partial) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    red[(0 * kNW * 64 + threadIdx.x) * 8 + k] = bs[k];
    red[(1 * kNW * 64 + threadIdx.x) * 8 + k] = bq[k];
  }
  __syncthreads();
  if (threadIdx.x < 2 * kCO) {
    const int stat = threadIdx.x >> 6, ch = threadIdx.x & 63, c = ch >> 3, k = ch & 7;
    float t = 0.f;
    for (int j = 0; j < (kNW * 64) >> 3; ++j) t += red[(stat * kNW * 64 + j * 8 + c) * 8 + k];
    bn_partial[((int64_t)blockIdx.x * 2 + stat) * kCO + ch] = t;
  }
}

// The virtual BatchNorm of a staged window: y = relu?(z * s + t) with s = invstd * gamma, t = beta - mean * s (the folded
// affine of BnAffine::init, conv.hip) on every live 16-byte slot.  A thread owns ONE channel group for the whole launch
// (thread = 18 q + slot: channel block slot >> 1, half slot & 1; positions q, q + 28, q + 56 ...), so its 8 scales / shifts
// sit in registers and a pass is one LDS read, 8 fma / max, one LDS write -- the first form (any thread, any slot: two
// integer divisions and four table reads per slot) cost ~50 us of a 157 us launch.
constexpr int kTfSlots = 2 * kCB;                       // 18 live 16-byte slots per position
constexpr int kTfPos = (kNW * 64) / kTfSlots;           // 28 positions per pass (504 of the 512 threads)
struct AffineRegs {
  float s[8], t[8];
  int pos0, slot_off;                                    // first position (>= xpos: idle thread); byte offset of the slot in a row
};
// (tid: the thread's index among the kNW * 64 threads that transform -- threadIdx.x, or its index among the helper waves of
//  the pipelined forward)
__device__ __forceinline__ void window_affine_regs(const Affine& a, AffineRegs& r, int tid = -1) {
  if (tid < 0) tid = threadIdx.x;
  const int q = tid / kTfSlots, slot = tid - q * kTfSlots;
  const int c0 = (slot >> 1) * 16 + (slot & 1) * 8;
  r.pos0 = q < kTfPos ? q : (1 << 30);
  r.slot_off = slot * 16;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = c0 + k;
    const float g = c < a.c_valid ? a.gamma[c] : 0.f, b = c < a.c_valid ? a.beta[c] : 0.f;
    r.s[k] = a.invstd[c] * g;
    r.t[k] = fmaf(-a.mean[c], r.s[k], b);
  }
}

// (all threads; barriers are the caller's; the zero rows of frames -1 and T stay zero)
// Four positions per thread in flight; the arithmetic as packed pairs (v_pk_fma_f32) and the ReLU on the ROUNDED 16-bit
// pairs as a signed-integer maximum with zero (v_pk_max_i16: rounding keeps the sign, so relu(round(y)) == round(relu(y))
// bit for bit, -0 included): ~20 vector instructions per slot instead of ~45.  The launch did not get shorter for it
// (160 us either way in tools/dev/tf_probe.py): with the parts of the forward kernel switched off one at a time the phases of
// a tile ADD UP -- 27 us loop + barriers, 30 transform, 58 fragment reads + MFMAs, 28 epilogue, 28 exposed window requests
// of a 170 us launch -- i.e. a phase costs its barrier-to-barrier latency chain (LDS round trip, drain, barrier) rather than
// its instruction count, and one workgroup per CU has nothing to overlap it with.
template <typename E>
__device__ __forceinline__ void window_transform(const Window& w, char* img_, const AffineRegs& r, int relu) {
  using V8 = typename Elem16<E>::v8;
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef short i16x8 __attribute__((ext_vector_type(8)));
  typedef __attribute__((address_space(3))) char lds_char;     // (callers pick the buffer at run time: keep the accesses ds_*)
  typedef __attribute__((address_space(3))) V8 lds_v8;
  lds_char* const img = (lds_char*)img_;
  const int lo = w.S, hi = (w.T + 1) * w.S;
  constexpr int kU = 4;
  for (int pos0 = r.pos0; pos0 < hi; pos0 += kU * kTfPos) {
    V8 v[kU];
    lds_v8* at[kU];
    bool live[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int pos = pos0 + u * kTfPos;
      live[u] = pos >= lo && pos < hi;
      at[u] = (lds_v8*)(img + pos * kXRow + (((pos >> 3) & 1) << 5) + r.slot_off);
      if (live[u]) v[u] = *at[u];
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      if (!live[u]) continue;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const f32x2 x = {(float)v[u][2 * k], (float)v[u][2 * k + 1]};
        const f32x2 y = __builtin_elementwise_fma(x, f32x2{r.s[2 * k], r.s[2 * k + 1]}, f32x2{r.t[2 * k], r.t[2 * k + 1]});
        v[u][2 * k] = (E)y[0];
        v[u][2 * k + 1] = (E)y[1];
      }
      if (relu) v[u] = __builtin_bit_cast(V8, __builtin_elementwise_max(__builtin_bit_cast(i16x8, v[u]), i16x8{0, 0, 0, 0, 0, 0, 0, 0}));
      *at[u] = v[u];
    }
  }
}
#endif  // __HIPCC__

}  // namespace dvt_window

namespace dvt_internal {
// conv3x1_c64.hip: the 64 -> 64 form of the (3, 1, 1) window convolution, behind dvt_conv3x1_fwd (conv3x1_fwd.hip);
// inst = position blocks per wave (1 .. 6)
dvt_window::Form conv3x1_c64_form(int64_t N, int T, int L);
void conv3x1_c64_fwd(const dvt_window::Form& f, const void* x, const void* w, int64_t ldw, void* y, float* stats_partial, int64_t N,
                     int dtype, hipStream_t st);
// conv3x1_dbn.hip: the temporal data gradient 64 -> 144 + mid-plane BatchNorm backward as a window kernel with helper waves
// (behind dvt_conv3x1_stream_bn_bwd, conv3x3_stream.hip); inst = position blocks per tile (2, 4, 6); one partial row per
// workgroup.  mode 1: the sums -> partial [grid][2][144]; mode 2: the corrected gradient -> dz (loc = the reduced sums)
dvt_window::Form conv3x1_dbn_form(int64_t N, int T, int L);
void conv3x1_dbn_pass(const dvt_window::Form& f, int mode, const void* dy, const void* w, int64_t ldw, const void* z,
                      const float* mean, const float* invstd, const float* gamma, const float* beta, int relu, int training,
                      float* partial, const float* loc, void* dz, int64_t N, int dtype, hipStream_t st);
}
