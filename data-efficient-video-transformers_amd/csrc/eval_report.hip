// eval_report.hip -- the counts behind the test epoch's classification_report (src/callbacks/callbacks.py:67-82) on the
// device: per class TP / FP / FN / support of `probs > threshold` against multilabel targets, and the sums over rows of
// the per-row precision / recall / F1 (the "samples" average).  Integer counts and fixed-order f64 sums (no atomics);
// not on the training hot path.  Also the per-threshold counts of SSLOnlineEval's sweep (callbacks.py:249-274).  A translation unit of its own, so that the code objects of eval_metrics.hip stay as
// they are.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kReportThreads = 256;
constexpr int kReportRowBlocks = 64;

// one block per class: TP / FP / FN / support over every row; int64 partials, fixed-order tree in LDS
__global__ __launch_bounds__(kReportThreads) void report_class_kernel(const float* __restrict__ probs,
                                                                     const unsigned char* __restrict__ labels, int64_t N,
                                                                     int C, float th, int64_t* __restrict__ counts) {
  __shared__ int64_t red[4][kReportThreads];
  const int c = blockIdx.x, t = threadIdx.x;
  int64_t tp = 0, fp = 0, fn = 0, sup = 0;
  for (int64_t n = t; n < N; n += kReportThreads) {
    const int p = probs[n * C + c] > th, l = labels[n * C + c] != 0;
    tp += p & l;
    fp += p & !l;
    fn += !p & l;
    sup += l;
  }
  red[0][t] = tp; red[1][t] = fp; red[2][t] = fn; red[3][t] = sup;
  __syncthreads();
  for (int s = kReportThreads / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int j = 0; j < 4; ++j) red[j][t] += red[j][t + s];
    __syncthreads();
  }
  if (t < 4) counts[(int64_t)t * C + c] = red[t][0];
}

// per-row precision / recall / F1 (0 where the denominator is 0), summed in f64 over a fixed row range per block
__global__ __launch_bounds__(kReportThreads) void report_rows_partial_kernel(const float* __restrict__ probs,
                                                                            const unsigned char* __restrict__ labels,
                                                                            int64_t N, int C, float th, int64_t rpb,
                                                                            double* __restrict__ part) {
  __shared__ double red[3][kReportThreads];
  const int t = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(N, r0 + rpb);
  double sp = 0.0, sr = 0.0, sf = 0.0;
  for (int64_t n = r0 + t; n < r1; n += kReportThreads) {
    int tp = 0, np = 0, nt = 0;
    for (int c = 0; c < C; ++c) {
      const int p = probs[n * C + c] > th, l = labels[n * C + c] != 0;
      tp += p & l;
      np += p;
      nt += l;
    }
    sp += np > 0 ? (double)tp / np : 0.0;
    sr += nt > 0 ? (double)tp / nt : 0.0;
    sf += np + nt > 0 ? 2.0 * tp / (np + nt) : 0.0;
  }
  red[0][t] = sp; red[1][t] = sr; red[2][t] = sf;
  __syncthreads();
  for (int s = kReportThreads / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int j = 0; j < 3; ++j) red[j][t] += red[j][t + s];
    __syncthreads();
  }
  if (t < 3) part[(int64_t)blockIdx.x * 3 + t] = red[t][0];
}

__global__ void report_rows_final_kernel(const double* __restrict__ part, int nblocks, double* __restrict__ sums) {
  const int j = threadIdx.x;
  if (j >= 3) return;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += part[(int64_t)b * 3 + j];
  sums[j] = s;
}

// block (class, threshold): TP / FP / FN of `probs > thresholds[t]` over every row; the blocks of threshold 0 also write the
// class's support.  int64 partials, fixed-order tree in LDS.
__global__ __launch_bounds__(kReportThreads) void sweep_counts_kernel(const float* __restrict__ probs,
                                                                     const unsigned char* __restrict__ labels, int64_t N,
                                                                     int C, const float* __restrict__ thresholds,
                                                                     int64_t* __restrict__ counts,
                                                                     int64_t* __restrict__ support) {
  __shared__ int64_t red[4][kReportThreads];
  const int c = blockIdx.x, ti = blockIdx.y, t = threadIdx.x;
  const float th = thresholds[ti];
  int64_t tp = 0, fp = 0, fn = 0, sup = 0;
  for (int64_t n = t; n < N; n += kReportThreads) {
    const int p = probs[n * C + c] > th, l = labels[n * C + c] != 0;
    tp += p & l;
    fp += p & !l;
    fn += !p & l;
    sup += l;
  }
  red[0][t] = tp; red[1][t] = fp; red[2][t] = fn; red[3][t] = sup;
  __syncthreads();
  for (int s = kReportThreads / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int j = 0; j < 4; ++j) red[j][t] += red[j][t + s];
    __syncthreads();
  }
  if (t < 3) counts[((int64_t)ti * 3 + t) * C + c] = red[t][0];
  if (t == 3 && ti == 0) support[c] = red[3][0];
}

inline int report_row_blocks(int64_t N) { return (int)std::min<int64_t>(kReportRowBlocks, dvt_cdiv(N, kReportThreads)); }

}  // namespace

extern "C" {

size_t dvt_multilabel_report_workspace_bytes(int64_t N) {
  if (N <= 0) return 0;
  return sizeof(double) * 3 * (size_t)report_row_blocks(N);
}

int dvt_multilabel_report(const float* probs, const unsigned char* labels, int64_t N, int C, float threshold,
                          int64_t* counts, double* row_sums, void* workspace, dvt_stream_t stream) {
  DVT_REQUIRE(probs && labels && counts && row_sums && workspace && N > 0 && C > 0,
              "dvt_multilabel_report: bad arguments");
  DVT_REQUIRE(N * (int64_t)C < ((int64_t)1 << 62), "dvt_multilabel_report: N*C too large");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(report_class_kernel, dim3((unsigned)C), dim3(kReportThreads), 0, st, probs, labels, N, C, threshold,
                     counts);
  int nblocks = report_row_blocks(N);
  const int64_t rpb = dvt_cdiv(N, nblocks);
  nblocks = (int)dvt_cdiv(N, rpb);
  double* part = (double*)workspace;
  hipLaunchKernelGGL(report_rows_partial_kernel, dim3(nblocks), dim3(kReportThreads), 0, st, probs, labels, N, C,
                     threshold, rpb, part);
  hipLaunchKernelGGL(report_rows_final_kernel, dim3(1), dim3(64), 0, st, (const double*)part, nblocks, row_sums);
  DVT_LAUNCH_CHECK("dvt_multilabel_report");
  return DVT_OK;
}

int dvt_multilabel_sweep_counts(const float* probs, const unsigned char* labels, int64_t N, int C, const float* thresholds,
                                int T, int64_t* counts, int64_t* support, dvt_stream_t stream) {
  DVT_REQUIRE(probs && labels && thresholds && counts && support && N > 0 && C > 0 && T >= 1 && T <= 64,
              "dvt_multilabel_sweep_counts: bad arguments (1 <= T <= 64)");
  DVT_REQUIRE(N * (int64_t)C < ((int64_t)1 << 62), "dvt_multilabel_sweep_counts: N*C too large");
  hipLaunchKernelGGL(sweep_counts_kernel, dim3((unsigned)C, (unsigned)T), dim3(kReportThreads), 0, (hipStream_t)stream, probs,
                     labels, N, C, thresholds, counts, support);
  DVT_LAUNCH_CHECK("dvt_multilabel_sweep_counts");
  return DVT_OK;
}

}  // extern "C"
