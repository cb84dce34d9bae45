// eval_metrics.hip -- every evaluation metric on the device, one translation unit.  None of it is on a training step's
// path: clarity over speed, integer counts and fixed-order f64 sums, no floating-point atomic, so two identical calls
// give bitwise-equal results.  What the reference computes on the host with scikit-learn / torchmetrics:
//   thresholded   samples-averaged F1 at a sweep of thresholds (src/callbacks/callbacks.py:36-47), the counts behind the
//                 test epoch's classification_report (callbacks.py:67-82) and SSLOnlineEval's sweep (callbacks.py:249-274)
//   ranked        average precision (callbacks.py:48-55) and AUROC (src/models/frame_transformer.py:8,114-115,276-343,
//                 src/models/basicmlp.py:20) from ONE descending sort per class and a parallel, tie-aware rank pass
//   counts        confusion matrix, multilabel TP / FP / FN / TN and the MITEval accuracy count (callbacks.py:14,85-98)
//
// Rank pass.  A sorted column (segment) of L elements is cut into blocks of kRankBlock elements; grid = blocks x segments.
//   tp[i]   inclusive count of positives; element i is a group END when i == L-1 or s[i+1] != s[i] (-0.0 == +0.0)
//   S[i]    tp at the last END before i (0 if none), G[i] tp at the first END at or after i.  tp never decreases, so S is
//           a running maximum over the ENDs and G a running minimum from the right: two ordinary scans.
//   2U   =  sum over negatives of S + G           (exact, int64)
//   AP   =  sum over ENDs e of ((tp[e] - S[e]) / P) (tp[e] / (e + 1))      (float64, fixed order)
// Launch 1 writes three integers per block (positives, block-relative tp at the first and at the last END, -1 without
// one); launch 2 has every block read the aggregates of its own column for its carries and reduce its elements into one
// (2U, AP) partial; launch 3 (one workgroup: rank_final_kernel, or ap_final_kernel for dvt_average_precision) adds the
// partials in a fixed order and forms the ratios and averages.  The only ordering between workgroups is the launch
// boundary: nothing waits, spins or takes a ticket inside a launch.  The micro average is the same pass over all N C
// elements as one segment.  NaN scores are undefined behaviour of the metric.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <type_traits>

#include "common.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace {

constexpr int kMaxRowClasses = 64;   // classes per sample of the per-row ("samples") kernels (19 / 15 in the reference)
constexpr int kMaxThresholds = 16;   // dvt_f1_samples
constexpr int kRowThreads = 128;     // per-row AP / AUROC: a thread sorts one row
constexpr int kReportThreads = 256;
constexpr int kReportRowBlocks = 64;
constexpr int kCountThreads = 256;

// ---------------------------------------------------------------- the helpers every kernel below shares
// Block sum of K values per thread by the fixed halving tree: red[k][0] holds the sums afterwards.
template <typename T, int K, int NT>
__device__ __forceinline__ void block_tree_sum(T (&red)[K][NT], const T (&v)[K]) {
  const int t = threadIdx.x;
  for (int k = 0; k < K; ++k) red[k][t] = v[k];
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < K; ++k) red[k][t] += red[k][t + s];
    __syncthreads();
  }
}

// Second stage of a two-stage sum: column j of the per-block partials part[nblocks][stride], added in block order.
template <typename T>
__device__ __forceinline__ T ordered_sum(const T* __restrict__ part, int nblocks, int stride, int j) {
  T s = 0;
  for (int b = 0; b < nblocks; ++b) s += part[(int64_t)b * stride + j];
  return s;
}

// out[j] = scale * (the ordered sum of column j), j < T
template <typename Out>
__global__ void ordered_sum_kernel(const double* __restrict__ part, int nblocks, int T, double scale, Out* __restrict__ out) {
  const int j = threadIdx.x;
  if (j < T) out[j] = (Out)(ordered_sum(part, nblocks, T, j) * scale);
}

// The rows of a two-stage sum: about `want` blocks of `rpb` consecutive rows, none empty.
struct RowSplit { int nblocks; int64_t rpb; };
inline RowSplit row_split(int64_t N, int64_t want) {
  const int64_t rpb = dvt_cdiv(N, want);
  return {(int)dvt_cdiv(N, rpb), rpb};
}
inline RowSplit mean_split(int64_t N) { return row_split(N, std::min<int64_t>(std::max<int64_t>(N / 4096, 1), 1024)); }
inline int64_t report_blocks(int64_t N) { return std::min<int64_t>(kReportRowBlocks, dvt_cdiv(N, kReportThreads)); }

// One row's C <= kMaxRowClasses scores into s[] in descending order (insertion sort), their labels into l[]; returns
// the row's positives.
__device__ __forceinline__ int sort_row_desc(const float* __restrict__ probs, const unsigned char* __restrict__ labels, int C,
                                             float* s, unsigned char* l) {
  int total = 0;
  for (int c = 0; c < C; ++c) {
    const float v = probs[c];
    const unsigned char y = labels[c] != 0;
    total += y;
    int i = c;
    while (i > 0 && s[i - 1] < v) { s[i] = s[i - 1]; l[i] = l[i - 1]; --i; }
    s[i] = v; l[i] = y;
  }
  return total;
}

inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---------------------------------------------------------------- thresholded metrics
struct Thresholds { float t[kMaxThresholds]; };

// per-row F1 at every threshold: f[n, j] = 2 |P & T| / (|P| + |T|), 0 if both empty
__global__ void f1_rows_kernel(const float* __restrict__ probs, const unsigned char* __restrict__ labels, int64_t N,
                               int C, Thresholds th, int T, float* __restrict__ f) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  for (int j = 0; j < T; ++j) {
    int tp = 0, den = 0;
    for (int c = 0; c < C; ++c) {
      const int p = probs[n * C + c] > th.t[j], l = labels[n * C + c] != 0;
      tp += p & l;
      den += p + l;
    }
    f[n * T + j] = den > 0 ? (float)(2.0 * tp / den) : 0.f;
  }
}

// first stage of the column sums of a [N, T] f32 matrix: thread j walks column j over the block's rows
__global__ void colsum_partial_kernel(const float* __restrict__ x, int64_t N, int T, int64_t rows_per_block,
                                      double* __restrict__ part) {
  const int j = threadIdx.x;
  if (j >= T) return;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(N, r0 + rows_per_block);
  double s = 0.0;
  for (int64_t r = r0; r < r1; ++r) s += (double)x[r * T + j];
  part[(int64_t)blockIdx.x * T + j] = s;
}

// out[j] = the mean over the rows of column j of x [N, T], T <= kMaxThresholds; part: mean_split(N).nblocks * T doubles
void col_means(hipStream_t st, const float* x, int64_t N, int T, double* part, float* out) {
  const RowSplit sp = mean_split(N);
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(sp.nblocks), dim3(kMaxThresholds), 0, st, x, N, T, sp.rpb, part);
  hipLaunchKernelGGL(ordered_sum_kernel<float>, dim3(1), dim3(kMaxThresholds), 0, st, (const double*)part, sp.nblocks, T,
                     1.0 / (double)N, out);
}

// block (class, threshold): TP / FP / FN of `probs > threshold` over every row into counts[threshold][3][C]; the blocks of
// threshold 0 also write the class's support.  `thresholds` on the device, or null for the one threshold `th0`.
__global__ __launch_bounds__(kReportThreads) void class_counts_kernel(const float* __restrict__ probs,
                                                                     const unsigned char* __restrict__ labels, int64_t N,
                                                                     int C, const float* __restrict__ thresholds, float th0,
                                                                     int64_t* __restrict__ counts,
                                                                     int64_t* __restrict__ support) {
  __shared__ int64_t red[4][kReportThreads];
  const int c = blockIdx.x, ti = blockIdx.y, t = threadIdx.x;
  const float th = thresholds ? thresholds[ti] : th0;
  int64_t v[4] = {0, 0, 0, 0};                               // TP, FP, FN, support
  for (int64_t n = t; n < N; n += kReportThreads) {
    const int p = probs[n * C + c] > th, l = labels[n * C + c] != 0;
    v[0] += p & l;
    v[1] += p & !l;
    v[2] += !p & l;
    v[3] += l;
  }
  block_tree_sum(red, v);
  if (t < 3) counts[((int64_t)ti * 3 + t) * C + c] = red[t][0];
  if (t == 3 && ti == 0) support[c] = red[3][0];
}

// per-row precision / recall / F1 (0 where the denominator is 0), summed in f64 over a fixed row range per block
__global__ __launch_bounds__(kReportThreads) void report_rows_partial_kernel(const float* __restrict__ probs,
                                                                            const unsigned char* __restrict__ labels,
                                                                            int64_t N, int C, float th, int64_t rpb,
                                                                            double* __restrict__ part) {
  __shared__ double red[3][kReportThreads];
  const int t = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(N, r0 + rpb);
  double v[3] = {0.0, 0.0, 0.0};
  for (int64_t n = r0 + t; n < r1; n += kReportThreads) {
    int tp = 0, np = 0, nt = 0;
    for (int c = 0; c < C; ++c) {
      const int p = probs[n * C + c] > th, l = labels[n * C + c] != 0;
      tp += p & l;
      np += p;
      nt += l;
    }
    v[0] += np > 0 ? (double)tp / np : 0.0;
    v[1] += nt > 0 ? (double)tp / nt : 0.0;
    v[2] += np + nt > 0 ? 2.0 * tp / (np + nt) : 0.0;
  }
  block_tree_sum(red, v);
  if (t < 3) part[(int64_t)blockIdx.x * 3 + t] = red[t][0];
}

// ---------------------------------------------------------------- per-row ("samples") AP and AUROC
// AP of one sample over its C class scores, written to ap_rows[n]
__global__ void ap_rows_kernel(const float* __restrict__ probs, const unsigned char* __restrict__ labels, int64_t N,
                               int C, float* __restrict__ ap_rows) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float s[kMaxRowClasses];
  unsigned char l[kMaxRowClasses];
  const int total = sort_row_desc(probs + n * C, labels + n * C, C, s, l);
  double ap = 0.0, r_prev = 0.0;
  int tp = 0;
  if (total > 0) {
    for (int i = 0; i < C; ++i) {
      tp += l[i];
      if (i == C - 1 || s[i + 1] != s[i]) {
        const double r = (double)tp / total;
        ap += (r - r_prev) * ((double)tp / (i + 1));
        r_prev = r;
      }
    }
  }
  ap_rows[n] = (float)ap;
}

// AUROC of one row over its C class scores; a block's valid rows are summed in a fixed order into row_part[block], their
// number into row_cnt[block]
__global__ __launch_bounds__(kRowThreads) void auroc_rows_kernel(const float* __restrict__ probs,
                                                                const unsigned char* __restrict__ labels, int64_t N, int C,
                                                                double* __restrict__ row_part, int* __restrict__ row_cnt) {
  __shared__ double red[1][kRowThreads];
  __shared__ int cnt[1][kRowThreads];
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double val[1] = {0.0};
  int ok[1] = {0};
  if (n < N) {
    float s[kMaxRowClasses];
    unsigned char l[kMaxRowClasses];
    const int P = sort_row_desc(probs + n * C, labels + n * C, C, s, l);
    if (P > 0 && P < C) {
      int tp = 0, tp_prev = 0, b = 0, u = 0;
      for (int i = 0; i < C; ++i) {
        tp += l[i];
        if (i == C - 1 || s[i + 1] != s[i]) {
          const int pos = tp - tp_prev, neg = (i - b + 1) - pos;
          u += neg * (2 * tp_prev + pos);
          tp_prev = tp;
          b = i + 1;
        }
      }
      val[0] = (double)u / (2.0 * (double)P * (double)(C - P));
      ok[0] = 1;
    }
  }
  block_tree_sum(red, val);
  block_tree_sum(cnt, ok);
  if (threadIdx.x == 0) { row_part[blockIdx.x] = red[0][0]; row_cnt[blockIdx.x] = cnt[0][0]; }
}

// ---------------------------------------------------------------- class-major layout ahead of the per-class sort
// [N, C] -> class-major keys [C, N] (f32) and labels [C, N] (u8)
__global__ void to_class_major_kernel(const float* __restrict__ probs, const unsigned char* __restrict__ labels,
                                      int64_t N, int C, float* __restrict__ keys, unsigned char* __restrict__ vals) {
  const int64_t total = N * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i / C;
    const int c = (int)(i % C);
    keys[(int64_t)c * N + n] = probs[i];
    vals[(int64_t)c * N + n] = labels[i] != 0;
  }
}

__global__ void offsets_kernel(int* __restrict__ off, int C, int64_t N) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c <= C) off[c] = (int)(c * N);
}

// ---------------------------------------------------------------- the rank pass
constexpr int kRankThreads = 256;
constexpr int kRankItems = 8;
constexpr int kRankBlock = kRankThreads * kRankItems;      // elements of a column per workgroup
constexpr int kRankWaves = kRankThreads / DVT_WAVE;

// LDS image of a block's keys: one pad word per 32, so that lanes 8 words apart fall on distinct banks
__device__ __forceinline__ int kpad(int i) { return i + (i >> 5); }
constexpr int kKeyWords = kRankBlock + 1 + (kRankBlock + 1) / 32 + 1;

// ---- fixed-order block collectives (256 threads).  `buf` holds one slot per wave; a trailing barrier frees it for reuse.
template <typename T, typename Op>
__device__ __forceinline__ T wave_all(T v, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}
template <typename T, typename Op>
__device__ __forceinline__ T block_all(T v, Op op, T* buf) {
  v = wave_all(v, op);
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = buf[0];
#pragma unroll
  for (int w = 1; w < kRankWaves; ++w) r = op(r, buf[w]);
  __syncthreads();
  return r;
}
// exclusive scan over the threads in thread order; `id` is the operator's identity
template <typename Op>
__device__ __forceinline__ int block_scan_excl(int v, Op op, int id, int* buf) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc = op(u, inc);
  }
  if (lane == 63) buf[wv] = inc;
  int ex = __shfl_up(inc, 1, 64);
  if (lane == 0) ex = id;
  __syncthreads();
  int carry = id;
  for (int w = 0; w < wv; ++w) carry = op(carry, buf[w]);
  __syncthreads();
  return op(carry, ex);
}
// exclusive scan from the right (thread 255 first)
template <typename Op>
__device__ __forceinline__ int block_scan_excl_rev(int v, Op op, int id, int* buf) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_down(inc, o, 64);
    if (lane + o < 64) inc = op(inc, u);
  }
  if (lane == 0) buf[wv] = inc;
  int ex = __shfl_down(inc, 1, 64);
  if (lane == 63) ex = id;
  __syncthreads();
  int carry = id;
  for (int w = kRankWaves - 1; w > wv; --w) carry = op(buf[w], carry);
  __syncthreads();
  return op(ex, carry);
}

struct OpAdd { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct OpMax { template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct OpMin { template <typename T> __device__ T operator()(T a, T b) const { return a < b ? a : b; } };

struct RankLds {
  float key[kKeyWords];
  unsigned char lab[kRankBlock];
  int iw[kRankWaves];
  int64_t lw[kRankWaves];
  double dw[kRankWaves];
};

// What a thread knows of its kRankItems consecutive elements once the block is staged: labels, END flags and the
// block-relative inclusive tp of each.  Elements past the column's end are neither positive nor an END.
struct RankItems {
  int tp[kRankItems];
  unsigned pos, end, live;       // bit j: element j is positive / an END / inside the column
};

__device__ __forceinline__ RankItems rank_stage(const float* __restrict__ s, const unsigned char* __restrict__ l, int64_t L,
                                                int64_t b0, RankLds& lds) {
  const int t = threadIdx.x;
  const int n = (int)min((int64_t)kRankBlock, L - b0);           // elements of this block
  for (int i = t; i < n; i += kRankThreads) {
    lds.key[kpad(i)] = s[b0 + i];
    lds.lab[i] = l[b0 + i];
  }
  if (t == 0 && b0 + n < L) lds.key[kpad(n)] = s[b0 + n];         // the next block's first key decides this block's last END
  __syncthreads();
  RankItems it;
  it.pos = it.end = it.live = 0u;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < kRankItems; ++j) {
    const int i = t * kRankItems + j;
    if (i < n) {
      it.live |= 1u << j;
      if (lds.lab[i]) { it.pos |= 1u << j; ++cnt; }
      if (b0 + i == L - 1 || lds.key[kpad(i + 1)] != lds.key[kpad(i)]) it.end |= 1u << j;
    }
    it.tp[j] = cnt;
  }
  const int before = block_scan_excl(cnt, OpAdd(), 0, lds.iw);
#pragma unroll
  for (int j = 0; j < kRankItems; ++j) it.tp[j] += before;
  return it;
}

// launch 1: agg[(seg * nb + blk) * 3 + {0, 1, 2}] = positives, tp at the first END, tp at the last END (block-relative, -1: none)
__global__ __launch_bounds__(kRankThreads) void rank_aggregate_kernel(const float* __restrict__ keys,
                                                                     const unsigned char* __restrict__ vals, int64_t L,
                                                                     int nb, int* __restrict__ agg) {
  __shared__ RankLds lds;
  const int seg = blockIdx.y, blk = blockIdx.x;
  const RankItems it = rank_stage(keys + (int64_t)seg * L, vals + (int64_t)seg * L, L, (int64_t)blk * kRankBlock, lds);
  int first = INT_MAX, last = -1;
#pragma unroll
  for (int j = 0; j < kRankItems; ++j)
    if (it.end >> j & 1u) { first = min(first, it.tp[j]); last = max(last, it.tp[j]); }
  const int pos = block_all((int)__popc(it.pos), OpAdd(), lds.iw);
  first = block_all(first, OpMin(), lds.iw);
  last = block_all(last, OpMax(), lds.iw);
  if (threadIdx.x == 0) {
    int* a = agg + ((int64_t)seg * nb + blk) * 3;
    a[0] = pos;
    a[1] = last < 0 ? -1 : first;
    a[2] = last;
  }
}

// launch 2: part_u[seg * nb + blk] = the block's share of 2U, part_ap[...] its share of AP; seg_pos[seg] = P (block 0)
__global__ __launch_bounds__(kRankThreads) void rank_pass_kernel(const float* __restrict__ keys,
                                                                const unsigned char* __restrict__ vals, int64_t L, int nb,
                                                                const int* __restrict__ agg, int64_t* __restrict__ part_u,
                                                                double* __restrict__ part_ap, int64_t* __restrict__ seg_pos) {
  __shared__ RankLds lds;
  const int seg = blockIdx.y, blk = blockIdx.x, t = threadIdx.x;
  const int* a = agg + (int64_t)seg * nb * 3;
  // carries from the column's other blocks: the nearest block with an END on either side, then the positives before
  // this block, before those two and in all (integer sums: any order gives the same value)
  int jl = -1, jr = INT_MAX;
  for (int j = t; j < nb; j += kRankThreads)
    if (a[j * 3 + 2] >= 0) {
      if (j < blk) jl = max(jl, j);
      if (j > blk) jr = min(jr, j);
    }
  jl = block_all(jl, OpMax(), lds.iw);
  jr = block_all(jr, OpMin(), lds.iw);
  int64_t base = 0, base_l = 0, base_r = 0, P = 0;
  for (int j = t; j < nb; j += kRankThreads) {
    const int64_t p = a[j * 3];
    P += p;
    if (j < blk) base += p;
    if (j < jl) base_l += p;
    if (j < jr) base_r += p;
  }
  base = block_all(base, OpAdd(), lds.lw);
  base_l = block_all(base_l, OpAdd(), lds.lw);
  base_r = block_all(base_r, OpAdd(), lds.lw);
  P = block_all(P, OpAdd(), lds.lw);
  const int64_t S_in = jl >= 0 ? base_l + a[jl * 3 + 2] : 0;                  // tp at the last END before this block
  const int64_t G_in = jr != INT_MAX ? base_r + a[jr * 3 + 1] : 0;            // tp at the first END after it (the column's
                                                                              // last element is an END: unused when absent)
  const int64_t b0 = (int64_t)blk * kRankBlock;
  const RankItems it = rank_stage(keys + (int64_t)seg * L, vals + (int64_t)seg * L, L, b0, lds);
  int tmax = -1, tmin = INT_MAX;
#pragma unroll
  for (int j = 0; j < kRankItems; ++j)
    if (it.end >> j & 1u) { tmax = max(tmax, it.tp[j]); tmin = min(tmin, it.tp[j]); }
  const int s_before = block_scan_excl(tmax, OpMax(), -1, lds.iw);            // block-relative, -1: take S_in
  const int g_after = block_scan_excl_rev(tmin, OpMin(), INT_MAX, lds.iw);    // block-relative, INT_MAX: take G_in
  int64_t G[kRankItems];
  int64_t g = g_after == INT_MAX ? G_in : base + g_after;
#pragma unroll
  for (int j = kRankItems - 1; j >= 0; --j) {
    if (it.end >> j & 1u) g = base + it.tp[j];
    G[j] = g;
  }
  int64_t S = s_before < 0 ? S_in : base + s_before;
  int64_t u = 0;
  double ap = 0.0;
#pragma unroll
  for (int j = 0; j < kRankItems; ++j) {
    if (!(it.live >> j & 1u)) continue;
    const int64_t tp = base + it.tp[j];
    if (!(it.pos >> j & 1u)) u += S + G[j];
    if (it.end >> j & 1u) {
      if (P > 0) ap += ((double)(tp - S) / (double)P) * ((double)tp / (double)(b0 + t * kRankItems + j + 1));
      S = tp;
    }
  }
  u = block_all(u, OpAdd(), lds.lw);
  ap = block_all(ap, OpAdd(), lds.dw);
  if (t == 0) {
    part_u[(int64_t)seg * nb + blk] = u;
    part_ap[(int64_t)seg * nb + blk] = ap;
    if (blk == 0) seg_pos[seg] = P;
  }
}

struct RankOut {
  double* auroc; double* ap; int64_t* positives; int64_t* two_u;     // [C] each
  double* averages;                                                  // [DVT_RANK_N_AVERAGES]
  int64_t* counts;                                                   // [DVT_RANK_N_COUNTS]
};

// strided per-thread partial in index order, then the fixed tree of block_all
template <typename T>
__device__ __forceinline__ T block_sum_of(const T* __restrict__ p, int n, T* buf) {
  T s = 0;
  for (int j = threadIdx.x; j < n; j += kRankThreads) s += p[j];
  return block_all(s, OpAdd(), buf);
}

// launch 3, one workgroup: per-class totals and ratios, then the averages over the classes in class order
__global__ __launch_bounds__(kRankThreads) void rank_final_kernel(int64_t N, int C, int nb, const int64_t* __restrict__ part_u,
                                                                 const double* __restrict__ part_ap,
                                                                 const int64_t* __restrict__ seg_pos, int nb_micro,
                                                                 const int64_t* __restrict__ micro_u,
                                                                 const int64_t* __restrict__ micro_pos, int row_blocks,
                                                                 const double* __restrict__ row_part,
                                                                 const int* __restrict__ row_cnt, RankOut o) {
  __shared__ RankLds lds;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int c = 0; c < C; ++c) {
    const int64_t u = block_sum_of(part_u + (int64_t)c * nb, nb, lds.lw);
    const double ap = block_sum_of(part_ap + (int64_t)c * nb, nb, lds.dw);
    if (threadIdx.x == 0) {
      const int64_t P = seg_pos[c], Nn = N - P;
      o.two_u[c] = u;
      o.positives[c] = P;
      o.ap[c] = P > 0 ? ap : 0.0;
      o.auroc[c] = P > 0 && Nn > 0 ? (double)u / (2.0 * (double)P * (double)Nn) : nan;
    }
  }
  int64_t mu = -1, mp = -1;
  if (nb_micro > 0) { mu = block_sum_of(micro_u, nb_micro, lds.lw); mp = micro_pos[0]; }
  double rsum = nan;
  int64_t rcnt = -1;
  if (row_blocks > 0) {
    rcnt = block_sum_of(row_cnt, row_blocks, lds.iw);      // fewer than 2^31 rows; integers: any order
    if (threadIdx.x == 0) rsum = ordered_sum(row_part, row_blocks, 1, 0);   // thread 0 alone (the only one to use it)
  }
  __syncthreads();                                         // this workgroup's own stores to o.auroc / o.positives
  if (threadIdx.x != 0) return;
  double macro = 0.0, wsum = 0.0;
  int64_t valid = 0, support = 0;
  for (int c = 0; c < C; ++c) {
    const int64_t P = o.positives[c];
    if (P > 0 && P < N) {
      macro += o.auroc[c];
      wsum += o.auroc[c] * (double)P;
      support += P;
      ++valid;
    }
  }
  o.averages[DVT_RANK_AVG_MACRO] = valid > 0 ? macro / (double)valid : nan;
  o.averages[DVT_RANK_AVG_WEIGHTED] = valid > 0 ? wsum / (double)support : nan;
  const int64_t total = N * C;
  o.averages[DVT_RANK_AVG_MICRO] = mp > 0 && mp < total ? (double)mu / (2.0 * (double)mp * (double)(total - mp)) : nan;
  o.averages[DVT_RANK_AVG_SAMPLES_SUM] = rsum;
  o.counts[DVT_RANK_CNT_VALID_CLASSES] = valid;
  o.counts[DVT_RANK_CNT_VALID_ROWS] = rcnt;
  o.counts[DVT_RANK_CNT_MICRO_TWO_U] = mu;
  o.counts[DVT_RANK_CNT_MICRO_POSITIVES] = mp;
}

// launch 3 of dvt_average_precision, one workgroup: the class's AP as rank_final_kernel adds it, rounded to f32 (0 without
// positives), and the support-weighted mean of those f32 values
__global__ __launch_bounds__(kRankThreads) void ap_final_kernel(int C, int nb, const double* __restrict__ part_ap,
                                                               const int64_t* __restrict__ seg_pos,
                                                               float* __restrict__ out_per_class,
                                                               float* __restrict__ out_weighted) {
  __shared__ double dw[kRankWaves];
  double num = 0.0, den = 0.0;                             // thread 0's
  for (int c = 0; c < C; ++c) {
    const double ap = block_sum_of(part_ap + (int64_t)c * nb, nb, dw);
    if (threadIdx.x == 0) {
      const int64_t P = seg_pos[c];
      const float a = P > 0 ? (float)ap : 0.f;
      out_per_class[c] = a;
      num += (double)a * (double)P;
      den += (double)P;
    }
  }
  if (threadIdx.x == 0) out_weighted[0] = den > 0 ? (float)(num / den) : 0.f;
}

struct RankPlan {
  size_t off_keys_in, off_keys_out, off_vals_in, off_vals_out, off_offsets, off_agg, off_part_u, off_part_ap, off_seg_pos,
      off_micro_u, off_micro_ap, off_micro_pos, off_row_part, off_row_cnt, off_temp, temp_seg, temp_all, bytes;
  int nb, nb_micro, row_blocks;
};

bool rank_plan(int64_t N, int C, int flags, RankPlan* p) {
  if (N <= 0 || C <= 0 || N * C >= (int64_t)1 << 31) return false;
  const int64_t total = N * C;
  p->temp_seg = p->temp_all = 0;
  if (rocprim::segmented_radix_sort_pairs_desc(nullptr, p->temp_seg, (const float*)nullptr, (float*)nullptr,
                                               (const unsigned char*)nullptr, (unsigned char*)nullptr, (unsigned)total,
                                               (unsigned)C, (const int*)nullptr, (const int*)nullptr, 0, 32,
                                               (hipStream_t)0) != hipSuccess)
    return false;
  if ((flags & DVT_RANK_MICRO) &&
      rocprim::radix_sort_pairs_desc(nullptr, p->temp_all, (const float*)nullptr, (float*)nullptr,
                                     (const unsigned char*)nullptr, (unsigned char*)nullptr, (size_t)total, 0, 32,
                                     (hipStream_t)0) != hipSuccess)
    return false;
  p->nb = (int)dvt_cdiv(N, kRankBlock);
  p->nb_micro = (flags & DVT_RANK_MICRO) ? (int)dvt_cdiv(total, kRankBlock) : 0;
  p->row_blocks = (flags & DVT_RANK_SAMPLES) ? (int)dvt_cdiv(N, kRowThreads) : 0;
  const size_t nagg = (size_t)(p->nb_micro > (int64_t)p->nb * C ? p->nb_micro : (int64_t)p->nb * C);
  size_t o = 0;
  p->off_keys_in = o;   o = al256(o + sizeof(float) * total);
  p->off_keys_out = o;  o = al256(o + sizeof(float) * total);
  p->off_vals_in = o;   o = al256(o + (size_t)total);
  p->off_vals_out = o;  o = al256(o + (size_t)total);
  p->off_offsets = o;   o = al256(o + sizeof(int) * (C + 1));
  p->off_agg = o;       o = al256(o + sizeof(int) * 3 * nagg);            // the micro pass reuses it after the class pass
  p->off_part_u = o;    o = al256(o + sizeof(int64_t) * (size_t)p->nb * C);
  p->off_part_ap = o;   o = al256(o + sizeof(double) * (size_t)p->nb * C);
  p->off_seg_pos = o;   o = al256(o + sizeof(int64_t) * C);
  p->off_micro_u = o;   o = al256(o + sizeof(int64_t) * (size_t)p->nb_micro);
  p->off_micro_ap = o;  o = al256(o + sizeof(double) * (size_t)p->nb_micro);
  p->off_micro_pos = o; o = al256(o + sizeof(int64_t));
  p->off_row_part = o;  o = al256(o + sizeof(double) * (size_t)p->row_blocks);
  p->off_row_cnt = o;   o = al256(o + sizeof(int) * (size_t)p->row_blocks);
  p->off_temp = o;      o = al256(o + (p->temp_seg > p->temp_all ? p->temp_seg : p->temp_all));
  p->bytes = o;
  return true;
}

inline const char* phase(char (&buf)[64], const char* who, const char* what) {
  snprintf(buf, sizeof(buf), "%s(%s)", who, what);
  return buf;
}

// The per-class half of a ranked metric for the entry point `who`: class-major layout, one descending sort per class
// (rocPRIM segmented radix sort, stable), then launches 1 and 2 of the rank pass into the plan's part_u / part_ap / seg_pos.
int rank_classes(const char* who, hipStream_t st, const RankPlan& p, char* ws, const float* probs, const unsigned char* labels,
                 int64_t N, int C) {
  char buf[64];
  float* keys_in = (float*)(ws + p.off_keys_in);
  float* keys_out = (float*)(ws + p.off_keys_out);
  unsigned char* vals_in = (unsigned char*)(ws + p.off_vals_in);
  unsigned char* vals_out = (unsigned char*)(ws + p.off_vals_out);
  int* offsets = (int*)(ws + p.off_offsets);
  int* agg = (int*)(ws + p.off_agg);
  const int64_t total = N * C;
  hipLaunchKernelGGL(to_class_major_kernel, dim3((unsigned)(dvt_cdiv(total, 256) < 4096 ? dvt_cdiv(total, 256) : 4096)),
                     dim3(256), 0, st, probs, labels, N, C, keys_in, vals_in);
  hipLaunchKernelGGL(offsets_kernel, dim3((unsigned)dvt_cdiv(C + 1, 64)), dim3(64), 0, st, offsets, C, N);
  DVT_LAUNCH_CHECK(phase(buf, who, "layout"));
  size_t temp = p.temp_seg;
  const hipError_t e = rocprim::segmented_radix_sort_pairs_desc(
      (void*)(ws + p.off_temp), temp, (const float*)keys_in, keys_out, (const unsigned char*)vals_in, vals_out,
      (unsigned)total, (unsigned)C, (const int*)offsets, (const int*)(offsets + 1), 0, 32, st);
  DVT_REQUIRE(e == hipSuccess, "%s: segmented sort failed: %s", who, hipGetErrorString(e));
  hipLaunchKernelGGL(rank_aggregate_kernel, dim3((unsigned)p.nb, (unsigned)C), dim3(kRankThreads), 0, st,
                     (const float*)keys_out, (const unsigned char*)vals_out, N, p.nb, agg);
  hipLaunchKernelGGL(rank_pass_kernel, dim3((unsigned)p.nb, (unsigned)C), dim3(kRankThreads), 0, st, (const float*)keys_out,
                     (const unsigned char*)vals_out, N, p.nb, (const int*)agg, (int64_t*)(ws + p.off_part_u),
                     (double*)(ws + p.off_part_ap), (int64_t*)(ws + p.off_seg_pos));
  DVT_LAUNCH_CHECK(phase(buf, who, "classes"));
  return DVT_OK;
}

// dvt_average_precision's workspace: the rank plan without flags, then the per-row APs and their per-block sums
struct ApTail { size_t off_ap_rows, off_part, bytes; };
inline ApTail ap_tail(const RankPlan& p, int64_t N) {
  ApTail t;
  t.off_ap_rows = p.bytes;
  t.off_part = t.off_ap_rows + al256(sizeof(float) * (size_t)N);
  t.bytes = t.off_part + al256(sizeof(double) * (size_t)mean_split(N).nblocks);
  return t;
}

// ---------------------------------------------------------------- counts
constexpr int kCmLdsClasses = 64;          // a [C][C] table up to this C is privatised in LDS (16 KB of int32)
constexpr int kMlLdsClasses = 1024;

// the class of a row: argmax over C logits by a group of G lanes, the lowest index among equal maxima (numpy / torch)
template <typename T, int G>
__device__ __forceinline__ int row_argmax(const T* __restrict__ row, int C, int sub) {
  float best = 0.f;
  int arg = INT_MAX;
  for (int c = sub; c < C; c += G) {
    const float v = to_f32<T>(row[c]);
    if (arg == INT_MAX || v > best) { best = v; arg = c; }
  }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(arg, o, 64);
    if (oa != INT_MAX && (arg == INT_MAX || ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
  }
  return arg;
}

// cm[target][prediction] += 1 over a block's share of the rows; T = void: predictions are int64 class indices.
// LDS: the table is gathered per workgroup in int32 (a workgroup sees fewer than 2^31 rows) and added to `cm` once.
template <typename T, int G, bool LDS>
__global__ __launch_bounds__(kCountThreads) void confusion_kernel(const void* __restrict__ pred, const int64_t* __restrict__ target,
                                                                 int64_t N, int C, unsigned long long* __restrict__ cm,
                                                                 unsigned long long* __restrict__ ignored) {
  __shared__ int hist[LDS ? kCmLdsClasses * kCmLdsClasses : 1];
  __shared__ int skipped;
  const int t = threadIdx.x;
  if (LDS)
    for (int i = t; i < C * C; i += kCountThreads) hist[i] = 0;
  if (t == 0) skipped = 0;
  __syncthreads();
  const int sub = t % G;
  const int64_t groups = (int64_t)gridDim.x * (kCountThreads / G);
  for (int64_t n = (int64_t)blockIdx.x * (kCountThreads / G) + t / G; n < N; n += groups) {
    int64_t p;
    if constexpr (std::is_void<T>::value) p = ((const int64_t*)pred)[n];
    else p = row_argmax<T, G>((const T*)pred + n * C, C, sub);
    if (sub != 0) continue;
    const int64_t y = target[n];
    if (y < 0 || y >= C || p < 0 || p >= C) { atomicAdd(&skipped, 1); continue; }
    if (LDS) atomicAdd(&hist[(int)y * C + (int)p], 1);
    else atomicAdd(&cm[y * C + p], 1ull);
  }
  __syncthreads();
  if (LDS)
    for (int i = t; i < C * C; i += kCountThreads)
      if (hist[i]) atomicAdd(&cm[i], (unsigned long long)hist[i]);
  if (t == 0 && skipped) atomicAdd(ignored, (unsigned long long)skipped);
}

template <typename T, int G>
void confusion_launch(hipStream_t st, const void* pred, const int64_t* target, int64_t N, int C, int64_t* cm,
                      int64_t* ignored) {
  const int64_t rows_per_block = (int64_t)(kCountThreads / G) * 16;
  const unsigned grid = (unsigned)std::min<int64_t>(dvt_cdiv(N, rows_per_block), 2048);
  if (C <= kCmLdsClasses)
    hipLaunchKernelGGL((confusion_kernel<T, G, true>), dim3(grid), dim3(kCountThreads), 0, st, pred, target, N, C,
                       (unsigned long long*)cm, (unsigned long long*)ignored);
  else
    hipLaunchKernelGGL((confusion_kernel<T, G, false>), dim3(grid), dim3(kCountThreads), 0, st, pred, target, N, C,
                       (unsigned long long*)cm, (unsigned long long*)ignored);
}

template <typename T>
void confusion_logits(hipStream_t st, const void* logits, const int64_t* target, int64_t N, int C, int64_t* cm,
                      int64_t* ignored) {
  if (C <= 4) confusion_launch<T, 4>(st, logits, target, N, C, cm, ignored);
  else if (C <= 16) confusion_launch<T, 16>(st, logits, target, N, C, cm, ignored);
  else confusion_launch<T, 64>(st, logits, target, N, C, cm, ignored);
}

// state[0..3][c] += TP, FP, FN, TN of `probs > th` over rows [r0, r1) of a block: TP / FP / FN gathered in LDS, TN the rest
__global__ __launch_bounds__(kCountThreads) void multilabel_counts_kernel(const float* __restrict__ probs,
                                                                         const unsigned char* __restrict__ labels,
                                                                         int64_t N, int C, float th, int64_t rpb,
                                                                         unsigned long long* __restrict__ state) {
  __shared__ int hist[3 * kMlLdsClasses];
  const int t = threadIdx.x;
  for (int i = t; i < 3 * C; i += kCountThreads) hist[i] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(N, r0 + rpb);
  const int64_t e1 = r1 * C;
  for (int64_t e = r0 * C + t; e < e1; e += kCountThreads) {
    const int p = probs[e] > th, l = labels[e] != 0;
    if (p | l) atomicAdd(&hist[(p & l ? 0 : p ? 1 : 2) * C + (int)(e % C)], 1);
  }
  __syncthreads();
  for (int c = t; c < C; c += kCountThreads) {
    const int tp = hist[c], fp = hist[C + c], fn = hist[2 * C + c];
    if (tp) atomicAdd(&state[c], (unsigned long long)tp);
    if (fp) atomicAdd(&state[(int64_t)C + c], (unsigned long long)fp);
    if (fn) atomicAdd(&state[2 * (int64_t)C + c], (unsigned long long)fn);
    atomicAdd(&state[3 * (int64_t)C + c], (unsigned long long)((r1 - r0) - tp - fp - fn));
  }
}

// out[0] += the number of i with a[i] == b[i] (MITEval's `running_logits == running_labels`); T = int64_t or float
template <typename T>
__global__ __launch_bounds__(kCountThreads) void count_equal_kernel(const T* __restrict__ a, const T* __restrict__ b, int64_t n,
                                                                   unsigned long long* __restrict__ out) {
  __shared__ int red[1][kCountThreads];
  int c[1] = {0};                                             // a thread sees fewer than 2^31 elements (grid >= n / 2^20)
  for (int64_t i = (int64_t)blockIdx.x * kCountThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCountThreads)
    c[0] += a[i] == b[i];
  block_tree_sum(red, c);
  if (threadIdx.x == 0 && red[0][0]) atomicAdd(out, (unsigned long long)red[0][0]);
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- thresholded metrics
size_t dvt_f1_samples_workspace_bytes(int64_t N, int T) {
  if (N <= 0 || T <= 0 || T > kMaxThresholds) return 0;
  return al256(sizeof(float) * (size_t)N * T) + al256(sizeof(double) * 1024 * kMaxThresholds);
}

int dvt_f1_samples(const float* probs, const unsigned char* labels, int64_t N, int C, const float* thresholds, int T,
                   float* out, void* workspace, dvt_stream_t stream) {
  DVT_REQUIRE(probs && labels && thresholds && out && workspace && N > 0 && C > 0, "dvt_f1_samples: bad arguments");
  DVT_REQUIRE(T > 0 && T <= kMaxThresholds, "dvt_f1_samples: 1..%d thresholds", kMaxThresholds);
  hipStream_t st = (hipStream_t)stream;
  Thresholds th;
  for (int j = 0; j < kMaxThresholds; ++j) th.t[j] = j < T ? thresholds[j] : 0.f;
  float* f = (float*)workspace;
  double* part = (double*)((char*)workspace + al256(sizeof(float) * (size_t)N * T));
  hipLaunchKernelGGL(f1_rows_kernel, dim3((unsigned)dvt_cdiv(N, 256)), dim3(256), 0, st, probs, labels, N, C, th, T, f);
  col_means(st, f, N, T, part, out);
  DVT_LAUNCH_CHECK("dvt_f1_samples");
  return DVT_OK;
}

size_t dvt_multilabel_report_workspace_bytes(int64_t N) {
  if (N <= 0) return 0;
  return sizeof(double) * 3 * (size_t)report_blocks(N);
}

int dvt_multilabel_report(const float* probs, const unsigned char* labels, int64_t N, int C, float threshold,
                          int64_t* counts, double* row_sums, void* workspace, dvt_stream_t stream) {
  DVT_REQUIRE(probs && labels && counts && row_sums && workspace && N > 0 && C > 0,
              "dvt_multilabel_report: bad arguments");
  DVT_REQUIRE(N * (int64_t)C < ((int64_t)1 << 62), "dvt_multilabel_report: N*C too large");
  hipStream_t st = (hipStream_t)stream;
  // counts [4][C]: the sweep's [1][3][C] with the support as its fourth row
  hipLaunchKernelGGL(class_counts_kernel, dim3((unsigned)C, 1), dim3(kReportThreads), 0, st, probs, labels, N, C,
                     (const float*)nullptr, threshold, counts, counts + 3 * (int64_t)C);
  const RowSplit sp = row_split(N, report_blocks(N));
  double* part = (double*)workspace;
  hipLaunchKernelGGL(report_rows_partial_kernel, dim3(sp.nblocks), dim3(kReportThreads), 0, st, probs, labels, N, C,
                     threshold, sp.rpb, part);
  hipLaunchKernelGGL(ordered_sum_kernel<double>, dim3(1), dim3(64), 0, st, (const double*)part, sp.nblocks, 3, 1.0, row_sums);
  DVT_LAUNCH_CHECK("dvt_multilabel_report");
  return DVT_OK;
}

int dvt_multilabel_sweep_counts(const float* probs, const unsigned char* labels, int64_t N, int C, const float* thresholds,
                                int T, int64_t* counts, int64_t* support, dvt_stream_t stream) {
  DVT_REQUIRE(probs && labels && thresholds && counts && support && N > 0 && C > 0 && T >= 1 && T <= 64,
              "dvt_multilabel_sweep_counts: bad arguments (1 <= T <= 64)");
  DVT_REQUIRE(N * (int64_t)C < ((int64_t)1 << 62), "dvt_multilabel_sweep_counts: N*C too large");
  hipLaunchKernelGGL(class_counts_kernel, dim3((unsigned)C, (unsigned)T), dim3(kReportThreads), 0, (hipStream_t)stream, probs,
                     labels, N, C, thresholds, 0.f, counts, support);
  DVT_LAUNCH_CHECK("dvt_multilabel_sweep_counts");
  return DVT_OK;
}

// ---------------------------------------------------------------- ranked metrics
size_t dvt_average_precision_workspace_bytes(int64_t N, int C) {
  RankPlan p;
  return rank_plan(N, C, 0, &p) ? ap_tail(p, N).bytes : 0;
}

int dvt_average_precision(const float* probs, const unsigned char* labels, int64_t N, int C, float* out_samples,
                          float* out_weighted, float* out_per_class, void* workspace, dvt_stream_t stream) {
  DVT_REQUIRE(probs && labels && out_samples && out_weighted && out_per_class && workspace && N > 0 && C > 0,
              "dvt_average_precision: bad arguments");
  DVT_REQUIRE(C <= kMaxRowClasses, "dvt_average_precision: at most %d classes", kMaxRowClasses);
  RankPlan p;
  DVT_REQUIRE(rank_plan(N, C, 0, &p), "dvt_average_precision: N*C too large");
  const ApTail tail = ap_tail(p, N);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* ap_rows = (float*)(ws + tail.off_ap_rows);
  // "samples": per-row AP, then the mean over rows
  hipLaunchKernelGGL(ap_rows_kernel, dim3((unsigned)dvt_cdiv(N, kRowThreads)), dim3(kRowThreads), 0, st, probs, labels, N, C,
                     ap_rows);
  col_means(st, ap_rows, N, 1, (double*)(ws + tail.off_part), out_samples);
  DVT_LAUNCH_CHECK("dvt_average_precision(samples)");
  // per class and "weighted": the rank pass, then its AP partials in rank_final_kernel's order
  const int rc = rank_classes("dvt_average_precision", st, p, ws, probs, labels, N, C);
  if (rc != DVT_OK) return rc;
  hipLaunchKernelGGL(ap_final_kernel, dim3(1), dim3(kRankThreads), 0, st, C, p.nb, (const double*)(ws + p.off_part_ap),
                     (const int64_t*)(ws + p.off_seg_pos), out_per_class, out_weighted);
  DVT_LAUNCH_CHECK("dvt_average_precision(final)");
  return DVT_OK;
}

int dvt_rank_metrics_block(void) { return kRankBlock; }

size_t dvt_rank_metrics_workspace_bytes(int64_t N, int C, int flags) {
  RankPlan p;
  return rank_plan(N, C, flags, &p) ? p.bytes : 0;
}

int dvt_rank_metrics(const float* probs, const unsigned char* labels, int64_t N, int C, int flags, double* auroc, double* ap,
                     int64_t* positives, int64_t* two_u, double* averages, int64_t* counts, void* workspace,
                     dvt_stream_t stream) {
  DVT_REQUIRE(probs && labels && auroc && ap && positives && two_u && averages && counts && workspace && N > 0 && C > 0,
              "dvt_rank_metrics: bad arguments");
  DVT_REQUIRE((flags & ~(DVT_RANK_MICRO | DVT_RANK_SAMPLES)) == 0, "dvt_rank_metrics: unknown flag bits in %d", flags);
  DVT_REQUIRE(!(flags & DVT_RANK_SAMPLES) || C <= kMaxRowClasses, "dvt_rank_metrics: the per-row part takes at most %d classes",
              kMaxRowClasses);
  RankPlan p;
  DVT_REQUIRE(rank_plan(N, C, flags, &p), "dvt_rank_metrics: N*C too large");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int64_t* micro_u = (int64_t*)(ws + p.off_micro_u);
  int64_t* micro_pos = (int64_t*)(ws + p.off_micro_pos);
  double* row_part = (double*)(ws + p.off_row_part);
  int* row_cnt = (int*)(ws + p.off_row_cnt);
  if (flags & DVT_RANK_SAMPLES) {
    hipLaunchKernelGGL(auroc_rows_kernel, dim3((unsigned)p.row_blocks), dim3(kRowThreads), 0, st, probs, labels, N, C, row_part,
                       row_cnt);
    DVT_LAUNCH_CHECK("dvt_rank_metrics(rows)");
  }
  const int rc = rank_classes("dvt_rank_metrics", st, p, ws, probs, labels, N, C);
  if (rc != DVT_OK) return rc;
  if (flags & DVT_RANK_MICRO) {                              // the same pass over every element as one column
    const int64_t total = N * C;
    float* keys_out = (float*)(ws + p.off_keys_out);
    unsigned char* vals_out = (unsigned char*)(ws + p.off_vals_out);
    int* agg = (int*)(ws + p.off_agg);
    size_t temp = p.temp_all;
    const hipError_t e = rocprim::radix_sort_pairs_desc((void*)(ws + p.off_temp), temp, (const float*)(ws + p.off_keys_in),
                                                        keys_out, (const unsigned char*)(ws + p.off_vals_in), vals_out,
                                                        (size_t)total, 0, 32, st);
    DVT_REQUIRE(e == hipSuccess, "dvt_rank_metrics: sort failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(rank_aggregate_kernel, dim3((unsigned)p.nb_micro, 1), dim3(kRankThreads), 0, st,
                       (const float*)keys_out, (const unsigned char*)vals_out, total, p.nb_micro, agg);
    hipLaunchKernelGGL(rank_pass_kernel, dim3((unsigned)p.nb_micro, 1), dim3(kRankThreads), 0, st, (const float*)keys_out,
                       (const unsigned char*)vals_out, total, p.nb_micro, (const int*)agg, micro_u,
                       (double*)(ws + p.off_micro_ap), micro_pos);
    DVT_LAUNCH_CHECK("dvt_rank_metrics(micro)");
  }
  RankOut o{auroc, ap, positives, two_u, averages, counts};
  hipLaunchKernelGGL(rank_final_kernel, dim3(1), dim3(kRankThreads), 0, st, N, C, p.nb, (const int64_t*)(ws + p.off_part_u),
                     (const double*)(ws + p.off_part_ap), (const int64_t*)(ws + p.off_seg_pos), p.nb_micro,
                     (const int64_t*)micro_u, (const int64_t*)micro_pos, p.row_blocks, (const double*)row_part,
                     (const int*)row_cnt, o);
  DVT_LAUNCH_CHECK("dvt_rank_metrics(final)");
  return DVT_OK;
}

// ---------------------------------------------------------------- counts
int dvt_confusion_matrix(const void* logits, int dtype, const int64_t* preds, const int64_t* target, int64_t N, int C,
                         int accumulate, int64_t* cm, int64_t* cm_ignored, dvt_stream_t stream) {
  DVT_REQUIRE(target && cm && cm_ignored && N >= 0 && C > 0 && C <= 32768, "dvt_confusion_matrix: bad arguments");
  DVT_REQUIRE((logits != nullptr) != (preds != nullptr), "dvt_confusion_matrix: give logits or preds, not both");
  DVT_REQUIRE(!logits || N * (int64_t)C < ((int64_t)1 << 62), "dvt_confusion_matrix: N*C too large");
  hipStream_t st = (hipStream_t)stream;
  if (!accumulate) {
    hipError_t e = hipMemsetAsync(cm, 0, sizeof(int64_t) * (size_t)C * C, st);
    if (e == hipSuccess) e = hipMemsetAsync(cm_ignored, 0, sizeof(int64_t), st);
    if (e != hipSuccess) return dvt_fail_hip(e, "dvt_confusion_matrix(zero)");
  }
  if (N == 0) return DVT_OK;
  if (preds) confusion_launch<void, 1>(st, preds, target, N, C, cm, cm_ignored);
  else DVT_DISPATCH_DTYPE(dtype, T, confusion_logits<T>(st, logits, target, N, C, cm, cm_ignored));
  DVT_LAUNCH_CHECK("dvt_confusion_matrix");
  return DVT_OK;
}

int dvt_count_equal(const void* a, const void* b, int64_t n, int is_int64, int accumulate, int64_t* out, dvt_stream_t stream) {
  DVT_REQUIRE(out && n >= 0 && (n == 0 || (a && b)), "dvt_count_equal: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (!accumulate) {
    const hipError_t e = hipMemsetAsync(out, 0, sizeof(int64_t), st);
    if (e != hipSuccess) return dvt_fail_hip(e, "dvt_count_equal(zero)");
  }
  if (n == 0) return DVT_OK;
  // 4096 elements per block, at most 2048 blocks; a block's int32 partial holds fewer than 2^31 matches up to n = 2^42
  const unsigned grid = (unsigned)std::min<int64_t>(dvt_cdiv(n, (int64_t)kCountThreads * 16), 2048);
  DVT_REQUIRE(n < ((int64_t)1 << 42), "dvt_count_equal: n too large");
  if (is_int64)
    hipLaunchKernelGGL(count_equal_kernel<int64_t>, dim3(grid), dim3(kCountThreads), 0, st, (const int64_t*)a,
                       (const int64_t*)b, n, (unsigned long long*)out);
  else
    hipLaunchKernelGGL(count_equal_kernel<float>, dim3(grid), dim3(kCountThreads), 0, st, (const float*)a, (const float*)b, n,
                       (unsigned long long*)out);
  DVT_LAUNCH_CHECK("dvt_count_equal");
  return DVT_OK;
}

int dvt_multilabel_counts(const float* probs, const unsigned char* labels, int64_t N, int C, float threshold, int accumulate,
                          int64_t* state, dvt_stream_t stream) {
  DVT_REQUIRE(probs && labels && state && N >= 0 && C > 0, "dvt_multilabel_counts: bad arguments");
  DVT_REQUIRE(C <= kMlLdsClasses, "dvt_multilabel_counts: at most %d classes", kMlLdsClasses);
  DVT_REQUIRE(N * (int64_t)C < ((int64_t)1 << 62), "dvt_multilabel_counts: N*C too large");
  hipStream_t st = (hipStream_t)stream;
  if (!accumulate) {
    const hipError_t e = hipMemsetAsync(state, 0, sizeof(int64_t) * 4 * (size_t)C, st);
    if (e != hipSuccess) return dvt_fail_hip(e, "dvt_multilabel_counts(zero)");
  }
  if (N == 0) return DVT_OK;
  // a block's rows: at least 16 threads' worth of elements each, at most 2048 blocks (and fewer than 2^31 elements)
  int64_t rpb = std::max<int64_t>(dvt_cdiv((int64_t)kCountThreads * 16, C), dvt_cdiv(N, 2048));
  const unsigned grid = (unsigned)dvt_cdiv(N, rpb);
  DVT_REQUIRE(rpb * C < ((int64_t)1 << 31), "dvt_multilabel_counts: N*C too large for 2048 blocks");
  hipLaunchKernelGGL(multilabel_counts_kernel, dim3(grid), dim3(kCountThreads), 0, st, probs, labels, N, C, threshold, rpb,
                     (unsigned long long*)state);
  DVT_LAUNCH_CHECK("dvt_multilabel_counts");
  return DVT_OK;
}

}  // extern "C"
