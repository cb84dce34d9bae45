// mix.hip -- Mixup / CutMix of clip batches, the mixed targets, and the cross-entropy that accepts them.
//
//   * timm.data.Mixup (mixup_alpha / cutmix_alpha; for clips the VideoMix form: one box for every frame and channel of a
//     sample), a stage the loaders' transform chain src/dataloaders/mmx/MMX_Frame_dl.py:63-88 does not have; the random
//     draws are the caller's (input_stage.Mixup)                                                  dvt_clips_mix
//   * timm's mixup_target: smoothed one-hot (or multi-hot) rows mixed with the partner's          dvt_targets_mix
//   * timm.loss.SoftTargetCrossEntropy, and with it nn.CrossEntropyLoss(label_smoothing=) of
//     src/models/basicmlp.py:38                                                                   dvt_ce_soft_*
//
// dvt_clips_mix is one kernel.  The launcher cuts the work into rows: a row names two samples a and b, a region of a sample
// (n0 x n1 x n2 runs of `len` contiguous elements, strides C H W / H W / W -- a full-width box merges its runs into longer
// ones, a whole sample is one run) and what each side receives there: nothing, lam * own + (1 - lam) * other, the other's
// value, or (out of place) its own.  Every lane takes 16-byte slots of a run: both sides are loaded, then both are stored, so
// in place a pair of samples is exchanged correctly without any ordering between lanes, waves or workgroups -- no address
// is touched by two lanes.  Rows travel by value in the kernel arguments; there is no device table and no copy.
// The stores are ordinary ones: non-temporal stores were measured at the metric clip (profiles/mixup.md) and changed the
// mixup by less than the spread of the repeats and made the CutMix box 10 % slower.
// The loss kernels keep their reductions in a fixed order with no atomics: two identical calls give bitwise-equal results.
#include <math.h>
#include <string.h>

#include "common.h"

namespace {

// ------------------------------------------------------------------ clips
constexpr int kMixRows = DVT_MIX_ROWS_PER_LAUNCH;
constexpr int kMixThreads = 256;
constexpr int kMixUnroll = 4;          // 16-byte slots per lane and side in flight
constexpr int kMixMaxBlocks = 4096;    // workgroups of one launch: 16 per CU

enum MixMode { kNone = 0, kMix = 1, kOther = 2, kSelf = 3 };

struct MixRows {
  int ia[kMixRows], ib[kMixRows];
  unsigned modes[kMixRows];                 // mode of side a | mode of side b << 4
  unsigned off0[kMixRows], nruns[kMixRows]; // first element of the region inside a sample; n0 * n1 * n2
  int n1[kMixRows], n2[kMixRows], len[kMixRows];
  float lam_a[kMixRows], oml_a[kMixRows], lam_b[kMixRows], oml_b[kMixRows];
};
static_assert(sizeof(MixRows) <= 3584, "MixRows travels in the kernel arguments");

template <typename D>
__device__ __forceinline__ D mix1(float lam, float oml, D own, D other) {
  return from_f32<D>(fmaf(lam, to_f32<D>(own), oml * to_f32<D>(other)));
}

template <typename D>
__global__ __launch_bounds__(kMixThreads) void clips_mix_kernel(const D* x, D* out, MixRows rows, int64_t S, int s0, int s1,
                                                                int s2) {
  constexpr int VE = 16 / (int)sizeof(D);
  typedef D vec __attribute__((ext_vector_type(VE)));
  const int e = blockIdx.y;
  const int ma = (int)(rows.modes[e] & 15u), mb = (int)(rows.modes[e] >> 4);
  const int len = rows.len[e], n1 = rows.n1[e], n2 = rows.n2[e];
  const unsigned nruns = rows.nruns[e];
  const float la = rows.lam_a[e], oa = rows.oml_a[e], lb = rows.lam_b[e], ob = rows.oml_b[e];
  const bool use_a = ma == kMix || ma == kSelf || mb != kNone;
  const bool use_b = ma == kMix || ma == kOther || mb == kMix;
  const D* pa = x + (int64_t)rows.ia[e] * S + rows.off0[e];
  const D* pb = x + (int64_t)rows.ib[e] * S + rows.off0[e];
  D* qa = out + (int64_t)rows.ia[e] * S + rows.off0[e];
  D* qb = out + (int64_t)rows.ib[e] * S + rows.off0[e];
  // slots per run: enough for any start inside a 16-byte line (a run that starts on a line needs one fewer: its last is empty)
  const unsigned spr = ((unsigned)len + 2u * VE - 2u) / VE;
  const int64_t slots = (int64_t)nruns * spr;
  const int64_t tiles = (slots + kMixThreads * kMixUnroll - 1) / (kMixThreads * kMixUnroll);

  // A lane's four slots of a tile lie kMixThreads apart: the first is split into (run, slot of the run) and the run into its
  // three indices by division, the others follow by adding the split of kMixThreads (the same for every lane) with carries.
  const unsigned un1 = (unsigned)n1, un2 = (unsigned)n2;
  const unsigned step_run = kMixThreads / spr, step_k = kMixThreads - step_run * spr;
  const unsigned step_r2 = step_run % un2, step_t = step_run / un2;
  const unsigned step_r1 = step_t % un1, step_r0 = step_t / un1;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int64_t off[kMixUnroll];
    int lo[kMixUnroll], hi[kMixUnroll];
    bool whole[kMixUnroll];
    vec va[kMixUnroll], vb[kMixUnroll];
    const int64_t g0 = tile * (kMixThreads * kMixUnroll) + threadIdx.x;
    unsigned k = (unsigned)g0, r0 = 0, r1 = 0, r2 = 0;       // slots < 2^32: the launcher holds a sample below 2^30 elements
    if (nruns > 1) {
      const unsigned run = (unsigned)g0 / spr;
      k = (unsigned)g0 - run * spr;
      const unsigned t = run / un2;
      r2 = run - t * un2;
      r0 = t / un1;
      r1 = t - r0 * un1;
    }
#pragma unroll
    for (int u = 0; u < kMixUnroll; ++u) {
      const int64_t g = g0 + u * kMixThreads;
      lo[u] = hi[u] = 0;
      off[u] = 0;
      whole[u] = false;
      const int64_t o = (int64_t)r0 * s0 + (int64_t)r1 * s1 + (int64_t)r2 * s2;
      const unsigned kk = k;
      if (nruns > 1) {                                       // the next slot of this lane; each index carries at most once
        k += step_k;
        unsigned c = k >= spr ? 1u : 0u;
        k -= c * spr;
        r2 += step_r2 + c;
        c = r2 >= un2 ? 1u : 0u;
        r2 -= c * un2;
        r1 += step_r1 + c;
        c = r1 >= un1 ? 1u : 0u;
        r1 -= c * un1;
        r0 += step_r0 + c;
      } else {
        k += kMixThreads;
      }
      if (g >= slots) continue;
      // the pointers this row uses must sit at the same place of their 16-byte lines for a slot to be one access each
      const unsigned ref = (unsigned)(reinterpret_cast<uintptr_t>((ma != kNone ? qa : qb) + o) & 15u);
      const bool same = (!use_a || (reinterpret_cast<uintptr_t>(pa + o) & 15u) == ref) &&
                        (!use_b || (reinterpret_cast<uintptr_t>(pb + o) & 15u) == ref) &&
                        (ma == kNone || (reinterpret_cast<uintptr_t>(qa + o) & 15u) == ref) &&
                        (mb == kNone || (reinterpret_cast<uintptr_t>(qb + o) & 15u) == ref);
      const int pad = same ? (int)(ref / sizeof(D)) : 0;      // elements of the first line in front of the run
      const int first = (int)kk * VE - pad;
      lo[u] = first < 0 ? 0 : first;
      hi[u] = first + VE > len ? len : first + VE;
      if (hi[u] < lo[u]) hi[u] = lo[u];
      off[u] = o;
      whole[u] = same && hi[u] - lo[u] == VE;
      if (whole[u]) {
        if (use_a) va[u] = *reinterpret_cast<const vec*>(pa + o + lo[u]);
        if (use_b) vb[u] = *reinterpret_cast<const vec*>(pb + o + lo[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kMixUnroll; ++u) {
      const int64_t o = off[u];
      if (whole[u]) {
        if (ma != kNone) {
          vec r = ma == kOther ? vb[u] : va[u];
          if (ma == kMix) {
#pragma unroll
            for (int j = 0; j < VE; ++j) r[j] = mix1<D>(la, oa, va[u][j], vb[u][j]);
          }
          *reinterpret_cast<vec*>(qa + o + lo[u]) = r;
        }
        if (mb != kNone) {
          vec r = va[u];
          if (mb == kMix) {
#pragma unroll
            for (int j = 0; j < VE; ++j) r[j] = mix1<D>(lb, ob, vb[u][j], va[u][j]);
          }
          *reinterpret_cast<vec*>(qb + o + lo[u]) = r;
        }
      } else if (hi[u] > lo[u]) {
        // the head or tail of a run, or lines that do not match: at most VE elements, every load issued before a store
        D ea[VE], eb[VE];
#pragma unroll
        for (int j = 0; j < VE; ++j) {
          const bool in = lo[u] + j < hi[u];
          ea[j] = use_a && in ? pa[o + lo[u] + j] : from_f32<D>(0.f);
          eb[j] = use_b && in ? pb[o + lo[u] + j] : from_f32<D>(0.f);
        }
#pragma unroll
        for (int j = 0; j < VE; ++j) {
          if (lo[u] + j >= hi[u]) continue;
          if (ma != kNone) qa[o + lo[u] + j] = ma == kMix ? mix1<D>(la, oa, ea[j], eb[j]) : (ma == kOther ? eb[j] : ea[j]);
          if (mb != kNone) qb[o + lo[u] + j] = mb == kMix ? mix1<D>(lb, ob, eb[j], ea[j]) : ea[j];
        }
      }
    }
  }
}

// what the table asks for sample i once the rows that change nothing are taken out
struct MixWant {
  int mode;                       // kNone, kMix or kOther (inside the box)
  int t0, t1, y0, y1, x0, x1;
};

static MixWant mix_want(const int32_t* r, int64_t i, float lam, int T, int H, int W) {
  MixWant w = {kNone, 0, 0, 0, 0, 0, 0};
  if (r[0] == i) return w;
  if (r[1] == 1 && lam != 1.0f) w = {kMix, 0, T, 0, H, 0, W};
  if (r[1] == 2 && r[3] > r[2] && r[5] > r[4] && r[7] > r[6]) w = {kOther, r[2], r[3], r[4], r[5], r[6], r[7]};
  return w;
}

struct MixLauncher {
  hipStream_t st;
  const void* x;
  void* out;
  int dtype, C, H, W;
  int64_t S;
  MixRows rows;
  int count;
  int64_t max_tiles;

  void add(int64_t ia, int64_t ib, int ma, int mb, float la, float lb, int t0, int t1, int y0, int y1, int x0, int x1) {
    int64_t n0 = t1 - t0, n1 = C, n2 = y1 - y0, len = x1 - x0;
    if (len == W) {
      len *= n2; n2 = 1;
      if (len == (int64_t)H * W) { len *= n1 * n0; n1 = 1; n0 = 1; }
    }
    const int k = count++;
    rows.ia[k] = (int)ia; rows.ib[k] = (int)ib;
    rows.modes[k] = (unsigned)ma | (unsigned)mb << 4;
    rows.off0[k] = (unsigned)(((int64_t)t0 * C * H + y0) * W + x0);
    rows.nruns[k] = (unsigned)(n0 * n1 * n2);
    rows.n1[k] = (int)n1; rows.n2[k] = (int)n2; rows.len[k] = (int)len;
    rows.lam_a[k] = la; rows.oml_a[k] = 1.0f - la;
    rows.lam_b[k] = lb; rows.oml_b[k] = 1.0f - lb;
    const int ve = 16 / (int)dvt_dtype_size(dtype);
    const int64_t slots = n0 * n1 * n2 * ((len + 2 * ve - 2) / ve);
    const int64_t tiles = dvt_cdiv(slots, kMixThreads * kMixUnroll);
    if (tiles > max_tiles) max_tiles = tiles;
  }
  bool full() const { return count == kMixRows; }

  int flush() {
    if (count == 0) return DVT_OK;
    int64_t gx = kMixMaxBlocks / count;
    if (gx > max_tiles) gx = max_tiles;
    if (gx < 1) gx = 1;
    const dim3 grid((unsigned)gx, (unsigned)count);
    DVT_DISPATCH_DTYPE(dtype, D, hipLaunchKernelGGL((clips_mix_kernel<D>), grid, dim3(kMixThreads), 0, st, (const D*)x, (D*)out,
                                                    rows, S, C * H * W, H * W, W));
    DVT_LAUNCH_CHECK("dvt_clips_mix");
    count = 0;
    max_tiles = 0;
    return DVT_OK;
  }
};

// ------------------------------------------------------------------ targets
constexpr int kTargetRows = 256;
struct TargetRows { int partner[kTargetRows]; float lam[kTargetRows], oml[kTargetRows]; };

__device__ __forceinline__ float target_value(const float* __restrict__ y, const int64_t* __restrict__ labels, int64_t r,
                                              int64_t c, int64_t Ccls, float off, float on) {
  if (y) return y[r * Ccls + c];
  const int64_t l = labels[r];
  if (l < 0 || l >= Ccls) return NAN;
  return c == l ? on : off;
}

// out[base + s][c] = lam * t(base + s, c) + oml * t(partner, c); a row with oml == 0 is its own target, whatever the partner's
__global__ __launch_bounds__(256) void targets_mix_kernel(const float* __restrict__ y, const int64_t* __restrict__ labels,
                                                          float* __restrict__ out, TargetRows rows, int64_t base,
                                                          int64_t Ccls, float off, float on) {
  const int s = blockIdx.y;
  const int64_t r = base + s, p = rows.partner[s];
  const float lam = rows.lam[s], oml = rows.oml[s];
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < Ccls; c += (int64_t)gridDim.x * 256) {
    float v = lam * target_value(y, labels, r, c, Ccls, off, on);
    if (oml != 0.f) v = fmaf(oml, target_value(y, labels, p, c, Ccls, off, on), v);
    out[r * Ccls + c] = v;
  }
}

// ------------------------------------------------------------------ soft-target cross-entropy
constexpr int kSoftWaves = 16;

// One workgroup: wave w takes rows w, w + 16, ...; per row the log-sum-exp (max, then sum of exp), sum_c t_c (lse - x_c) and
// sum_c t_c, each butterfly-reduced; the wave adds its rows in row order, lane 0 of the workgroup the 16 waves in wave order.
template <typename T>
__global__ __launch_bounds__(kSoftWaves * DVT_WAVE) void ce_soft_fwd_kernel(const T* __restrict__ x, int64_t ld,
                                                                          const float* __restrict__ t,
                                                                          float* __restrict__ loss, float* __restrict__ lse,
                                                                          int64_t M, int64_t C) {
  __shared__ float part[kSoftWaves];
  const int lane = threadIdx.x % DVT_WAVE, wv = threadIdx.x / DVT_WAVE;
  float acc = 0.f;
  for (int64_t r = wv; r < M; r += kSoftWaves) {
    const T* row = x + r * ld;
    const float* trow = t + r * C;
    float mx = -INFINITY;
    for (int64_t c = lane; c < C; c += DVT_WAVE) mx = fmaxf(mx, to_f32<T>(row[c]));
    mx = wave_max(mx);
    float se = 0.f;
    for (int64_t c = lane; c < C; c += DVT_WAVE) se += expf(to_f32<T>(row[c]) - mx);
    se = wave_sum(se);
    const float l = mx + logf(se);
    float nll = 0.f, ts = 0.f;
    for (int64_t c = lane; c < C; c += DVT_WAVE) {
      const float tc = trow[c];
      nll = fmaf(tc, l - to_f32<T>(row[c]), nll);
      ts += tc;
    }
    nll = wave_sum(nll);
    ts = wave_sum(ts);
    if (lane == 0) { lse[r] = l; lse[M + r] = ts; }
    acc += nll;
  }
  if (lane == 0) part[wv] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < kSoftWaves; ++w) s += part[w];
    loss[0] = s / (float)M;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ce_soft_bwd_kernel(const T* __restrict__ x, int64_t ld, const float* __restrict__ t,
                                                          const float* __restrict__ lse, const float* __restrict__ gloss,
                                                          T* __restrict__ dx, int64_t lddx, int64_t M, int64_t C) {
  const int64_t r = blockIdx.x;
  const T* row = x + r * ld;
  const float* trow = t + r * C;
  T* drow = dx + r * lddx;
  const float scale = gloss[0] / (float)M, l = lse[r], ts = lse[M + r];
  for (int64_t c = threadIdx.x; c < C; c += blockDim.x)
    drow[c] = from_f32<T>(scale * fmaf(expf(to_f32<T>(row[c]) - l), ts, -trow[c]));
}

static bool lam_ok(float v) { return v >= 0.f && v <= 1.f; }          // false for NaN

}  // namespace

extern "C" {

int dvt_clips_mix(void* x, void* out, int dtype, int64_t B, int T, int C, int H, int W, const int32_t* table,
                  const float* lam, dvt_stream_t stream) {
  DVT_REQUIRE(x && table && lam, "dvt_clips_mix: null pointer (x %p, table %p, lam %p)", x, (const void*)table,
              (const void*)lam);
  DVT_REQUIRE(dtype == DVT_F32 || dvt_is_16bit(dtype), "dvt_clips_mix: dtype %d is not f32, bf16 or f16", dtype);
  DVT_REQUIRE(B >= 1 && B < (1ll << 31) && T > 0 && C > 0 && H > 0 && W > 0, "dvt_clips_mix: bad shape [%lld, %d, %d, %d, %d]",
              (long long)B, T, C, H, W);
  const int64_t S = (int64_t)T * C * H * W;
  DVT_REQUIRE((double)T * C * H * W < 1073741824.0, "dvt_clips_mix: a sample of %d x %d x %d x %d elements is 2^30 or more", T, C, H,
              W);
  const size_t es = dvt_dtype_size(dtype);
  const bool in_place = out == nullptr || out == x;
  if (in_place) out = x;
  DVT_REQUIRE(reinterpret_cast<uintptr_t>(x) % es == 0 && reinterpret_cast<uintptr_t>(out) % es == 0,
              "dvt_clips_mix: x and out must be aligned to their element size");
  if (!in_place) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(x), b = reinterpret_cast<uintptr_t>(out), n = (uintptr_t)(B * S) * es;
    DVT_REQUIRE(a + n <= b || b + n <= a, "dvt_clips_mix: out overlaps x without being x");
  }
  for (int64_t i = 0; i < B; ++i) {
    const int32_t* r = table + i * 8;
    DVT_REQUIRE(r[1] >= 0 && r[1] <= 2, "dvt_clips_mix: table row %lld: kind %d is not 0 (leave), 1 (mixup) or 2 (cutmix)",
                (long long)i, (int)r[1]);
    DVT_REQUIRE(r[0] >= 0 && r[0] < B, "dvt_clips_mix: table row %lld: partner %d outside [0, %lld)", (long long)i, (int)r[0],
                (long long)B);
    DVT_REQUIRE(lam_ok(lam[i]), "dvt_clips_mix: table row %lld: lam %g outside [0, 1]", (long long)i, (double)lam[i]);
    DVT_REQUIRE(r[1] != 2 || (0 <= r[2] && r[2] <= r[3] && r[3] <= T && 0 <= r[4] && r[4] <= r[5] && r[5] <= H && 0 <= r[6] &&
                              r[6] <= r[7] && r[7] <= W),
                "dvt_clips_mix: table row %lld: box t %d..%d y %d..%d x %d..%d leaves the %d x %d x %d clip", (long long)i,
                (int)r[2], (int)r[3], (int)r[4], (int)r[5], (int)r[6], (int)r[7], T, H, W);
  }
  if (in_place)
    for (int64_t i = 0; i < B; ++i)
      DVT_REQUIRE(table[table[i * 8] * 8] == i,
                  "dvt_clips_mix: table row %lld: in place the partner map must be an involution, but partner[%d] = %d",
                  (long long)i, (int)table[i * 8], (int)table[table[i * 8] * 8]);

  MixLauncher L;
  L.st = (hipStream_t)stream; L.x = x; L.out = out; L.dtype = dtype; L.C = C; L.H = H; L.W = W; L.S = S;
  L.count = 0; L.max_tiles = 0;
  memset(&L.rows, 0, sizeof(L.rows));
  int rc = DVT_OK;
  if (!in_place) {
    // first every sample whole (mixed, or copied), then, behind those launches on the stream, the boxes
    for (int pass = 0; pass < 2; ++pass) {
      for (int64_t i = 0; i < B; ++i) {
        const MixWant w = mix_want(table + i * 8, i, lam[i], T, H, W);
        if (pass == 0) L.add(i, table[i * 8], w.mode == kMix ? kMix : kSelf, kNone, lam[i], 1.f, 0, T, 0, H, 0, W);
        else if (w.mode == kOther) L.add(i, table[i * 8], kOther, kNone, 1.f, 1.f, w.t0, w.t1, w.y0, w.y1, w.x0, w.x1);
        else continue;
        if (L.full() && (rc = L.flush()) != DVT_OK) return rc;
      }
      if ((rc = L.flush()) != DVT_OK) return rc;
    }
    return DVT_OK;
  }
  // in place: pairs i < partner[i].  The two boxes (a mixup's is the whole sample) cut each axis into at most five
  // intervals; inside a cell of that grid both members want one thing, so a cell is a row.
  for (int64_t i = 0; i < B; ++i) {
    const int64_t p = table[i * 8];
    if (p <= i) continue;
    const MixWant wa = mix_want(table + i * 8, i, lam[i], T, H, W), wb = mix_want(table + p * 8, p, lam[p], T, H, W);
    if (wa.mode == kNone && wb.mode == kNone) continue;
    int cut[3][6], ncut[3];
    const int full[3] = {T, H, W};
    const int ea[3][2] = {{wa.t0, wa.t1}, {wa.y0, wa.y1}, {wa.x0, wa.x1}}, eb[3][2] = {{wb.t0, wb.t1}, {wb.y0, wb.y1}, {wb.x0, wb.x1}};
    for (int ax = 0; ax < 3; ++ax) {
      int v[6] = {0, full[ax], 0, 0, 0, 0}, n = 2;
      if (wa.mode != kNone) { v[n++] = ea[ax][0]; v[n++] = ea[ax][1]; }
      if (wb.mode != kNone) { v[n++] = eb[ax][0]; v[n++] = eb[ax][1]; }
      for (int a = 1; a < n; ++a)                                  // insertion sort of at most six
        for (int b = a; b > 0 && v[b] < v[b - 1]; --b) { const int t = v[b]; v[b] = v[b - 1]; v[b - 1] = t; }
      int m = 0;
      for (int a = 0; a < n; ++a) if (m == 0 || v[a] != cut[ax][m - 1]) cut[ax][m++] = v[a];
      ncut[ax] = m;
    }
    for (int a = 0; a + 1 < ncut[0]; ++a)
      for (int b = 0; b + 1 < ncut[1]; ++b)
        for (int c = 0; c + 1 < ncut[2]; ++c) {
          const int t0 = cut[0][a], t1 = cut[0][a + 1], y0 = cut[1][b], y1 = cut[1][b + 1], x0 = cut[2][c], x1 = cut[2][c + 1];
          const bool in_a = wa.mode != kNone && t0 >= wa.t0 && t1 <= wa.t1 && y0 >= wa.y0 && y1 <= wa.y1 && x0 >= wa.x0 && x1 <= wa.x1;
          const bool in_b = wb.mode != kNone && t0 >= wb.t0 && t1 <= wb.t1 && y0 >= wb.y0 && y1 <= wb.y1 && x0 >= wb.x0 && x1 <= wb.x1;
          if (!in_a && !in_b) continue;
          L.add(i, p, in_a ? wa.mode : kNone, in_b ? wb.mode : kNone, lam[i], lam[p], t0, t1, y0, y1, x0, x1);
          if (L.full() && (rc = L.flush()) != DVT_OK) return rc;
        }
  }
  return L.flush();
}

int dvt_targets_mix(const float* y, const int64_t* labels, float* out, int64_t B, int64_t Ccls, const int32_t* table,
                    const float* lam, float smoothing, dvt_stream_t stream) {
  DVT_REQUIRE(out && table && lam, "dvt_targets_mix: null pointer (out %p, table %p, lam %p)", (void*)out, (const void*)table,
              (const void*)lam);
  DVT_REQUIRE((y != nullptr) != (labels != nullptr), "dvt_targets_mix: exactly one of y and labels is given");
  DVT_REQUIRE(B >= 1 && B < (1ll << 31) && Ccls >= 1, "dvt_targets_mix: bad shape [%lld, %lld]", (long long)B, (long long)Ccls);
  DVT_REQUIRE(smoothing >= 0.f && smoothing < 1.f, "dvt_targets_mix: smoothing %g outside [0, 1)", (double)smoothing);
  for (int64_t i = 0; i < B; ++i) {
    DVT_REQUIRE(table[i * 8] >= 0 && table[i * 8] < B, "dvt_targets_mix: table row %lld: partner %d outside [0, %lld)",
                (long long)i, (int)table[i * 8], (long long)B);
    DVT_REQUIRE(lam_ok(lam[i]), "dvt_targets_mix: table row %lld: lam %g outside [0, 1]", (long long)i, (double)lam[i]);
  }
  const float off = smoothing / (float)Ccls, on = 1.0f - smoothing + off;
  hipStream_t st = (hipStream_t)stream;
  const unsigned gx = (unsigned)(dvt_cdiv(Ccls, 256) < 64 ? dvt_cdiv(Ccls, 256) : 64);
  for (int64_t base = 0; base < B; base += kTargetRows) {
    const int count = (int)(B - base < kTargetRows ? B - base : kTargetRows);
    TargetRows rows;
    memset(&rows, 0, sizeof(rows));
    for (int s = 0; s < count; ++s) {
      rows.partner[s] = table[(base + s) * 8];
      rows.lam[s] = lam[base + s];
      rows.oml[s] = 1.0f - lam[base + s];
    }
    hipLaunchKernelGGL(targets_mix_kernel, dim3(gx, (unsigned)count), dim3(256), 0, st, y, labels, out, rows, base, Ccls, off, on);
    DVT_LAUNCH_CHECK("dvt_targets_mix");
  }
  return DVT_OK;
}

int dvt_ce_soft_fwd(const void* logits, int64_t ld, const float* targets, float* loss, float* lse, int64_t M, int64_t C,
                    int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(logits && targets && loss && lse, "dvt_ce_soft_fwd: null pointer (logits %p, targets %p, loss %p, lse %p)", logits,
              (const void*)targets, (void*)loss, (void*)lse);
  DVT_REQUIRE(M >= 1 && C >= 1 && ld >= C && (dtype == DVT_F32 || dvt_is_16bit(dtype)),
              "dvt_ce_soft_fwd: bad arguments (M %lld, C %lld, ld %lld, dtype %d)", (long long)M, (long long)C, (long long)ld, dtype);
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((ce_soft_fwd_kernel<T>), dim3(1), dim3(kSoftWaves * DVT_WAVE), 0, st, (const T*)logits,
                                        ld, targets, loss, lse, M, C));
  DVT_LAUNCH_CHECK("dvt_ce_soft_fwd");
  return DVT_OK;
}

int dvt_ce_soft_bwd(const void* logits, int64_t ld, const float* targets, const float* lse, const float* gloss, void* dlogits,
                    int64_t lddl, int64_t M, int64_t C, int dtype, dvt_stream_t stream) {
  DVT_REQUIRE(logits && targets && lse && gloss && dlogits,
              "dvt_ce_soft_bwd: null pointer (logits %p, targets %p, lse %p, gloss %p, dlogits %p)", logits, (const void*)targets,
              (const void*)lse, (const void*)gloss, dlogits);
  DVT_REQUIRE(M >= 1 && M < (1ll << 31) && C >= 1 && ld >= C && lddl >= C && (dtype == DVT_F32 || dvt_is_16bit(dtype)),
              "dvt_ce_soft_bwd: bad arguments (M %lld, C %lld, ld %lld, lddl %lld, dtype %d)", (long long)M, (long long)C,
              (long long)ld, (long long)lddl, dtype);
  hipStream_t st = (hipStream_t)stream;
  DVT_DISPATCH_DTYPE(dtype, T,
                     hipLaunchKernelGGL((ce_soft_bwd_kernel<T>), dim3((unsigned)M), dim3(256), 0, st, (const T*)logits, ld,
                                        targets, lse, gloss, (T*)dlogits, lddl, M, C));
  DVT_LAUNCH_CHECK("dvt_ce_soft_bwd");
  return DVT_OK;
}

}  // extern "C"
