/*
 * dvt_hip.h -- C ABI of libdvt_hip.so: the MI355X (gfx950) kernels behind the
 * video-clip forward/backward hot path of data-efficient-video-transformers.
 *
 * The reference has no native layer: every entry point below replaces a
 * third-party PyTorch operator at the reference call site cited next to it
 * (paths relative to the reference repository root).  INTEGRATION.md shows the
 * ctypes binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - Plain C: raw device pointers, int64 sizes / element strides, enums as int.
 *   - Every function is asynchronous on `stream` (a hipStream_t passed as
 *     void*; NULL = the legacy default stream), never synchronises, never
 *     allocates or retains memory: the caller owns all buffers and workspaces.
 *   - Return value: 0 (DVT_OK) or a negative dvt_status; the message for the
 *     last failure on the calling thread is dvt_last_error().  No C++
 *     exception crosses the boundary.
 *   - Activations are `dtype` (DVT_BF16 or DVT_F32 ...); LayerNorm scale/shift,
 *     biases, positional tables, statistics and all parameter gradients are
 *     float32.  Accumulation is always float32.
 *   - Matrices are row-major with the last dimension contiguous unless an
 *     element stride says otherwise.
 */
#ifndef DVT_HIP_H
#define DVT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a descriptor struct changes layout (fields are only ever appended) or an entry point changes
 * signature.  v2: dvt_gemm_desc / dvt_conv_desc gained defer_reduce / pending / carry, dvt_splitk_pending and the
 * head-wise / folded-attention descriptors were added.  Callers MUST zero-initialise every descriptor (memset / = {0})
 * before filling it: a zero in a field this header adds later means "feature off".  v5: the `aux` matrix of DVT_EPI_GELU /
 * DVT_EPI_DGELU holds the activation's DERIVATIVE (was the pre-activation): a meaning changed, no layout. */
#define DVT_ABI_VERSION 5

typedef void* dvt_stream_t; /* hipStream_t */

enum dvt_dtype { DVT_F32 = 0, DVT_BF16 = 1, DVT_F16 = 2 };

enum dvt_status {
  DVT_OK = 0,
  DVT_ERR_BAD_ARG = -1,     /* null pointer, negative size, misaligned buffer ... */
  DVT_ERR_UNSUPPORTED = -2, /* shape / dtype this build has no kernel for */
  DVT_ERR_HIP = -3          /* a HIP runtime call or launch failed */
};

int dvt_version(void);
const char* dvt_last_error(void);
/* Fills compute-unit count, LDS bytes per CU and the gcnArchName of the
 * current device. */
int dvt_device_info(int* cu_count, int* lds_bytes, char* arch, int arch_len);

/* ---------------------------------------------------------------- casts / adds
 * dst[i] = (dst_dtype) src[i].  Replaces tensor.to(dtype) on the path (bf16
 * compute copies of the fp32 master weights, clip tensors). */
int dvt_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n,
             dvt_stream_t stream);
/* out = a + b (residual adds `attn(x) + x`, `ff(x) + x`: src/models/vit.py:73-74
 * when the producing GEMM is not the one fusing it). */
int dvt_add(const void* a, const void* b, void* out, int64_t n, int dtype, dvt_stream_t stream);
/* out[r, :] = x[r, :] + table[r / rows_per_entry, :]  -- sinusoidal PositionalEncoding on
 * seq-first [L, B, E] activations: `x + self.pe[:x.size(0)]`, frame_transformer.py:32-34
 * (rows_per_entry = B).  table: [rows / rows_per_entry, d] f32. */
int dvt_add_rowtable(const void* x, const float* table, void* out, int64_t rows, int64_t d,
                     int64_t rows_per_entry, int dtype, dvt_stream_t stream);
/* Strided 2-D copy: dst[r*dst_ld + c] = src[r*src_ld + c], r < rows, c < cols (elements).
 * src_ld == 0 broadcasts one row.  Used for the per-sample CLS-clip concatenation
 * (frame_transformer.py:194-197) and sequence slices. */
int dvt_copy2d(const void* src, void* dst, int64_t rows, int64_t cols, int64_t src_ld, int64_t dst_ld,
               int dtype, dvt_stream_t stream);
/* out[c] (+)= sum_{r<rows} src[r*row_stride + c]   (f32 out; gradient of a broadcast). */
int dvt_rows_sum(const void* src, int64_t row_stride, int64_t rows, int64_t cols, float* out,
                 int dtype, int accumulate, dvt_stream_t stream);
/* [A, B, C] -> [B, A, C]   ('b s d -> s b d', frame_transformer.py:205; transformer.py:76). */
int dvt_permute_021(const void* src, void* dst, int64_t A, int64_t B, int64_t C, int dtype,
                    dvt_stream_t stream);
/* dst(f32)[i] = beta * dst[i] + alpha * src[i]  (gradient accumulation). */
int dvt_axpby_f32(const void* src, int src_dtype, float alpha, float* dst, float beta, int64_t n,
                  dvt_stream_t stream);

/* Stand-alone activations (the 3-layer GELU head, src/models/frame_transformer.py:106,
 * where no GEMM epilogue is worth fusing into).  act: 1 = GELU(erf), 2 = ReLU, 3 = sigmoid (TPN.py:99).
 * fwd: y = act(x);  bwd: dx = dy * act'(x). */
int dvt_act_fwd(const void* x, void* y, int64_t n, int act, int dtype, dvt_stream_t stream);
int dvt_act_bwd(const void* dy, const void* x, void* dx, int64_t n, int act, int dtype,
                dvt_stream_t stream);

/* Measurement aid: occupies the stream for `microseconds` (<= 1 s) with a single spinning lane, so that the host can
 * enqueue a whole step behind it and HIP-event brackets around individual launches then measure device time only
 * (bench.py's roofline pass). */
int dvt_device_delay(uint64_t microseconds, dvt_stream_t stream);
/* Asynchronous zero fill (a memset node inside a captured graph): the rows a gather's adjoint does not write --
 * `x[:, 0]` at src/models/vit.py:120,126 has a zero gradient on every other row. */
int dvt_zero(void* dst, size_t nbytes, dvt_stream_t stream);

/* ---------------------------------------------------------------- dropout
 * nn.Dropout(p) in training mode (frame_transformer.py:22,41-44 p = 0.5; TPN.py:92,95; vit.py:23,25,43,104):
 * y[i] = keep_i ? x[i] / (1 - p) : 0.  keep_i comes from Philox4x32-10 word (i & 3) of counter
 * rng_state[1] + call_offset + i / 4 under key rng_state[0]; rng_state is a device array {seed, step base offset}.
 * The same call with dy in place of x is the backward pass (no mask is stored).  call_offset separates the dropout
 * sites of one step (advance it by ceil(n / 4) per site); dvt_rng_advance moves the base once per step on the
 * device, so a captured hipGraph draws new masks on every replay.  torch's own generator stream is not reproduced. */
int dvt_dropout(const void* x, void* y, int64_t n, float p, const uint64_t* rng_state, uint64_t call_offset, int dtype,
                dvt_stream_t stream);
/* The same mask fused with its neighbours in nn.TransformerEncoderLayer's training-mode forward (frame_transformer.py:39-47:
 * x + dropout1(sa), dropout(relu(linear1 x)), x + dropout2(ff)):  y = residual? + keep * relu?(x) / (1 - p), residual nullable,
 * relu 0 / 1, mask drawn exactly like dvt_dropout at (rng_state, call_offset).  With rng_state == NULL and `gate` given (the
 * backward of the relu form, gate = the forward's output): y = gate != 0 ? x / (1 - p) : 0 -- no mask is re-drawn, an element
 * the mask dropped and one the ReLU zeroed both pass no gradient.  Exactly one of rng_state and gate is non-NULL.  The
 * backward of the residual form is dvt_dropout on dy (and dy itself for the residual). */
int dvt_dropout_fused(const void* x, const void* residual, const void* gate, void* y, int64_t n, float p,
                      const uint64_t* rng_state, uint64_t call_offset, int relu, int dtype, dvt_stream_t stream);
int dvt_rng_advance(uint64_t* rng_state, uint64_t delta, dvt_stream_t stream);

/* ---------------------------------------------------------------- patchify
 * Rearrange 'b t c (h p1) (w p2) -> b t (h w) (p1 p2 c)'  (src/models/vit.py:90).
 * x: [frames, C, H, W] in x_dtype; out: [frames * (H/P) * (W/P), P*P*C] in
 * out_dtype (patch-vector index = (p1*P + p2)*C + c).  This pair is the tubelet pair below at pt = 1: one
 * implementation (csrc/patchify.hip), the same argument checks, error texts under its own names. */
int dvt_patchify(const void* x, int x_dtype, void* out, int out_dtype, int64_t frames, int C,
                 int H, int W, int P, dvt_stream_t stream);
/* Adjoint of dvt_patchify (scatter back to pixel layout): needed when the clip
 * itself carries a gradient (learnable pixel-space CLS clip,
 * src/models/frame_transformer.py:105,195). */
int dvt_patchify_bwd(const void* dout, int dout_dtype, void* dx, int dx_dtype, int64_t frames,
                     int C, int H, int W, int P, dvt_stream_t stream);
/* Tubelet embedding gather: the 3-D counterpart of the per-frame Rearrange + Linear tokeniser of
 * src/models/vit.py:89-92 (the ViViT paper's own embedding; the reference builds the per-frame one only).
 * 'b (tau k) c (h p1) (w p2) -> (b tau h w) (k p1 p2 c)':  x: [frames, C, H, W] in x_dtype, frames = b * t flattened,
 * every pt consecutive frames form a tubelet (the caller guarantees t % pt == 0); out: [(frames / pt) * (H/P) * (W/P),
 * pt*P*P*C] in out_dtype,
 *   out[((bi*(t/pt) + tau)*nh + ph)*nw + pw, ((k*P + p1)*P + p2)*C + c] = x[bi, tau*pt + k, c, ph*P + p1, pw*P + p2]
 * with nh = H/P, nw = W/P: k slowest, c fastest -- a row is the pt per-frame patch vectors of dvt_patchify's order,
 * concatenated; pt == 1 is dvt_patchify itself (the same launch).  DVT_ERR_BAD_ARG for a null pointer, pt < 1, frames % pt != 0,
 * H % P != 0 or W % P != 0, before any HIP call. */
int dvt_tubelet_patchify(const void* x, int x_dtype, void* out, int out_dtype, int64_t frames, int C, int H, int W, int P,
                         int pt, dvt_stream_t stream);
/* Adjoint (= inverse: the gather is a permutation) of dvt_tubelet_patchify, the scatter back to [frames, C, H, W]:
 *   dx[bi, tau*pt + k, c, ph*P + p1, pw*P + p2] = dout[((bi*(t/pt) + tau)*nh + ph)*nw + pw, ((k*P + p1)*P + p2)*C + c]
 * (src/models/vit.py:89-92 in backward, when the clip itself carries a gradient).  Same argument checks. */
int dvt_tubelet_patchify_bwd(const void* dout, int dout_dtype, void* dx, int dx_dtype, int64_t frames, int C, int H, int W,
                             int P, int pt, dvt_stream_t stream);

/* ---------------------------------------------------------------- token assembly
 * ViViT.forward token plumbing, src/models/vit.py:113-115:
 *   out[s, 0, :]   = cls[:]            + pos[s % T, 0, :]
 *   out[s, 1+j, :] = emb[s*n + j, :]   + pos[s % T, 1+j, :]
 * emb: [S*n, d] dtype; cls: [d] f32; pos: [T, pos_rows, d] f32 (pos_rows >= n+1);
 * out: [S, n+1, d] dtype.  */
int dvt_tokens_assemble_fwd(const void* emb, const float* cls, const float* pos, void* out,
                            int64_t S, int64_t T, int64_t n, int64_t d, int64_t pos_rows,
                            int dtype, dvt_stream_t stream);
/* demb = dout[:, 1:, :]; dcls (+)= sum_s dout[s,0,:]; dpos[t,j,:] (+)= sum_{s%T==t} dout[s,j,:].
 * `accumulate` != 0 adds into dcls/dpos instead of overwriting. */
int dvt_tokens_assemble_bwd(const void* dout, void* demb, float* dcls, float* dpos, int64_t S,
                            int64_t T, int64_t n, int64_t d, int64_t pos_rows, int dtype,
                            int accumulate, dvt_stream_t stream);

/* ---------------------------------------------------------------- patch dropout (csrc/patch_dropout.hip)
 * The tokeniser of src/models/vit.py:110-116 on a kept subset of the patch tokens (tube masking as in VideoMAE, or drawn
 * per frame as in PatchDropout; the reference has neither).  A clip [b, t, C, H, W] at patch P and tubelet pt has
 * S = b * (t / pt) sequences of n = (H/P) * (W/P) positions; a sequence keeps k of them:
 *   keep [S, k] int32, strictly ascending per row;  slot [S, n] int32, the inverse map, -1 for a dropped position.
 * The kernels that read keep / slot treat an entry of keep outside [0, n) or of slot outside [0, k) as dropped: no address
 * is formed from it.
 *
 * Selection (specialises the row choice of vit.py:110-116): keys [R, n] int32; position i of a row is kept iff fewer than k
 * positions j have (key_j, j) < (key_i, i) in signed order, ties to the lower position -- the first k of a stable argsort;
 * the output index of a kept position is the number of kept positions below it.  Every key row is written rows_per times
 * (rows r * rows_per .. of keep / slot): tube masking is R = b, rows_per = t / pt; per frame R = b * t / pt, rows_per = 1.
 * DVT_ERR_BAD_ARG before any launch unless 1 <= n <= 1024, 1 <= k <= n, rows_per >= 1.  Integer work, no atomics. */
int dvt_keep_select(const int32_t* keys, int64_t R, int n, int k, int rows_per, int32_t* keep, int32_t* slot,
                    dvt_stream_t stream);
/* The same selection, in one launch, on keys drawn on the device (vit.py:110-116 in training mode): key(r, i) is, as int32,
 * Philox4x32-10 word (e & 3) of counter rng_state[1] + call_offset + e / 4 under key rng_state[0], e = r * n + i -- the
 * generator and the device state {seed, step base} of dvt_dropout (a site takes ceil(R * n / 4) blocks), so a captured
 * hipGraph draws a new subset on every replay once dvt_rng_advance has moved the base.  keys_out (nullable, [R, n]) receives
 * the keys; keep and slot are given together, or both NULL with keys_out (keys only). */
int dvt_keep_draw(const uint64_t* rng_state, uint64_t call_offset, int64_t R, int n, int k, int rows_per, int32_t* keep,
                  int32_t* slot, int32_t* keys_out, dvt_stream_t stream);
/* slot [S, n] of a caller's keep [S, k] (vit.py:110-116 with the rows chosen by the caller); same argument ranges. */
int dvt_keep_slots(const int32_t* keep, int64_t S, int n, int k, int32_t* slot, dvt_stream_t stream);
/* Kept gather (the Rearrange of vit.py:110 on the kept patches): dvt_tubelet_patchify's element order, kept rows only,
 *   out[s*k + i, ((kf*P + p1)*P + p2)*C + c] = x[s*pt + kf, c, ph*P + p1, pw*P + p2],  ph*nw + pw = keep[s, i];
 * out: [(frames / pt) * k, pt*P*P*C].  Reads only the kept patches.  Same argument checks and dtype pairs as
 * dvt_tubelet_patchify, and 1 <= k <= n. */
int dvt_patchify_keep(const void* x, int x_dtype, void* out, int out_dtype, const int32_t* keep, int64_t frames, int C, int H,
                      int W, int P, int pt, int k, dvt_stream_t stream);
/* Its adjoint (vit.py:110 in backward): writes EVERY pixel of dx [frames, C, H, W] exactly once -- a pixel of a kept patch
 * from row s*k + slot[s, position] of dout, a pixel of a dropped patch zero.  No pre-zeroing, no atomics. */
int dvt_patchify_keep_bwd(const void* dout, int dout_dtype, void* dx, int dx_dtype, const int32_t* slot, int64_t frames, int C,
                          int H, int W, int P, int pt, int k, dvt_stream_t stream);
/* Token assembly on kept rows (vit.py:113-115):
 *   out[s, 0, :]   = cls[:]           + pos[s % T, 0, :]
 *   out[s, 1+i, :] = emb[s*k + i, :]  + pos[s % T, 1 + keep[s, i], :]
 * emb: [S*k, d] dtype; cls: [d] f32; pos: [T, pos_rows, d] f32 (pos_rows >= n+1); out: [S, k+1, d] dtype. */
int dvt_tokens_assemble_keep_fwd(const void* emb, const float* cls, const float* pos, const int32_t* keep, void* out,
                                 int64_t S, int64_t T, int n, int k, int64_t d, int64_t pos_rows, int dtype,
                                 dvt_stream_t stream);
/* Backward of the above (vit.py:113-115): demb [S*k, d] = dout[:, 1:, :]; dcls (+)= sum_s dout[s, 0, :];
 * dpos[tau, 0, :] (+)= sum_b dout[b*T + tau, 0, :]; dpos[tau, 1+j, :] (+)= the sum, over those b with
 * slot[b*T + tau, j] >= 0 in ascending b, of dout[b*T + tau, 1 + slot, :] -- a fixed order, no float atomics.  A row of dpos
 * whose position nobody kept (and every row above n) gets exactly zero when overwriting and is not touched when
 * `accumulate` != 0.  slot must be the inverse of a keep [S, k]: demb is written from the rows slot names. */
int dvt_tokens_assemble_keep_bwd(const void* dout, const int32_t* slot, void* demb, float* dcls, float* dpos, int64_t S,
                                 int64_t T, int n, int k, int64_t d, int64_t pos_rows, int dtype, int accumulate,
                                 dvt_stream_t stream);

/* ---------------------------------------------------------------- stochastic depth (csrc/drop_path.hip)
 * timm's DropPath on the residual lines `x = attn(x) + x`, `x = ff(x) + x` (src/models/vit.py:73-74; the reference has no
 * drop path), in the form that runs the branch on the kept sequences only.  A "sequence" is one contiguous row of
 * L = N * d elements of a [S, N, d] tensor; input and output share one element type (f32, bf16, f16), arithmetic is fp32
 * with one rounding on the store.  16-byte accesses when L * sizeof(T) is a multiple of 16 and every base pointer is
 * 16-byte aligned, a scalar form otherwise.  An index read from device memory is compared against its bound before any
 * address is formed from it.  DVT_ERR_BAD_ARG before any launch on a null pointer or S, k, L < 1 (S, k < 2^31).
 *
 * Gather (replaces DropPath on vit.py:73-74: the rows the branch runs on; in backward the rows of the gradient it sees):
 *   y[j, :] = alpha * x[idx[j], :]  where 0 <= idx[j] < S;  a row of zeros otherwise (-1 is the "dropped" value).
 * x: [S, L]; idx: [k] int32; y: [k, L]. */
int dvt_seq_gather(const void* x, const int32_t* idx, void* y, int64_t S, int64_t k, int64_t L, float alpha, int dtype,
                   dvt_stream_t stream);
/* Scatter-add, the adjoint of the gather (replaces DropPath's `+ x` on vit.py:73-74, and in backward the sum of the
 * shortcut's and the branch's gradient):
 *   out[s, :] = res[s, :] + alpha * y[slot[s], :]  (one fmaf) where 0 <= slot[s] < k;  out[s, :] = res[s, :] otherwise.
 * res, out: [S, L]; y: [k, L]; slot: [S] int32.  Every row of out is written exactly once; no atomics, no zero-filled
 * intermediate, bitwise repeatable.  out MAY ALIAS res (in place): a lane reads a piece of res before it writes the same
 * piece of out and nobody else touches it.  out must not overlap y. */
int dvt_seq_scatter_add(const void* res, const void* y, const int32_t* slot, void* out, int64_t S, int64_t k, int64_t L,
                        float alpha, int dtype, dvt_stream_t stream);
/* Per-sequence Bernoulli draw (replaces the random tensor of DropPath on vit.py:73-74):  m[s] = s with probability 1 - p,
 * else -1 -- usable as idx and as slot of the two kernels above at k = S.  Sequence s is kept iff word (s & 3) of
 * Philox4x32-10 block rng_state[1] + call_offset + s / 4 under key rng_state[0] is >= round(p * 2^32): dvt_dropout's
 * generator, device state and rule (a site takes ceil(S / 4) blocks), so a captured hipGraph draws anew on every replay.
 * 0 <= p < 1. */
int dvt_drop_path_draw(const uint64_t* rng_state, uint64_t call_offset, int64_t S, float p, int32_t* m,
                       dvt_stream_t stream);

/* ---------------------------------------------------------------- masked-autoencoder pre-training (csrc/mae.hip)
 * Additions within ABI v5: new entry points only.  MAE / MAE-ST / VideoMAE on the tokeniser of src/models/vit.py:110-116 (the
 * reference has no self-supervised clip model): the space stack encodes the k kept tokens of every sequence (the patch
 * dropout entries above), a decoder reconstructs the pixels of the n - k dropped patches.  keep [S, k] / slot [S, n] as above;
 * an entry of slot outside [0, k) counts as dropped, an entry of keep outside [0, n) yields a zero row.  fp32 arithmetic, one
 * rounding per output element, every output element written exactly once, no float atomics, bitwise repeatable.
 *
 * Restore (what vit.py:113-115 is to the encoder, for the decoder): the encoded kept rows back at their positions, the
 * learned mask token everywhere else, plus the decoder's positional table (no CLS row):
 *   out[s, j, :] = (0 <= slot[s, j] < k ? y[s, skip + slot[s, j], :] : mask[:]) + pos[s % T, j, :]
 * y: [S, skip + k, d] dtype (the `skip` leading rows of a sequence -- the CLS row -- are not restored); mask: [d] f32;
 * pos: [T, n, d] f32; out: [S, n, d] dtype.  DVT_ERR_BAD_ARG before any launch unless d % 8 == 0, 1 <= k <= n, skip >= 0,
 * S % T == 0 and every buffer is 16-byte aligned. */
int dvt_tokens_restore_fwd(const void* y, const float* mask, const float* pos, const int32_t* slot, void* out, int64_t S,
                           int64_t T, int n, int k, int skip, int64_t d, int dtype, dvt_stream_t stream);
/* Its adjoint: dy [S, skip + k, d]: dy[s, skip + i] = dout[s, keep[s, i]], the skip leading rows exactly zero;
 * dmask [d] (+)= the sum of dout[s, j] over all dropped (s, j); dpos[tau, j] (+)= sum_b dout[b*T + tau, j] in ascending b, over
 * every position, kept or not.  Fixed orders: dmask is reduced from `partial` [T * n, d] f32 (scratch the caller owns, written
 * whole by the same pass that sums dpos) by one workgroup per 8 columns.  `accumulate` != 0 adds into dmask / dpos instead
 * of overwriting; dmask is exactly zero (or untouched in value) when k == n. */
int dvt_tokens_restore_bwd(const void* dout, const int32_t* keep, const int32_t* slot, void* dy, float* dmask, float* dpos,
                           float* partial, int64_t S, int64_t T, int n, int k, int skip, int64_t d, int dtype, int accumulate,
                           dvt_stream_t stream);
/* Masked patch loss: the mean over the M = S * (n - k) dropped patches (S = frames / pt) of the mean over D = pt*P*P*C of
 * (pred - target)^2.  The target of a dropped (s, j) is row (s, j) of dvt_tubelet_patchify(clip), read from the clip:
 *   target[((kf*P + p1)*P + p2)*C + c] = clip[s*pt + kf, c, ph*P + p1, pw*P + p2],  ph*nw + pw = j;
 * with norm_pix != 0 it is (x - mean) / sqrt(var + eps), mean and UNBIASED variance (divisor D - 1) over the D values of the
 * patch, the variance as a sum of squared deviations from the mean.  pred: [S, n, D] pred_dtype; clip: [frames, C, H, W]
 * clip_dtype (any pair of f32 / bf16 / f16); per_patch: [S, n] f32, exactly 0 at kept positions; stats: [S, n, 2] f32
 * {mean, rstd} (required with norm_pix, zeros at kept positions; else ignored, may be NULL); loss: one f32, written by a
 * second launch that sums per_patch and divides by M in double.  k is an argument, not counted on the device.
 * DVT_ERR_BAD_ARG before any launch unless 1 <= k < n (M == 0 is refused), frames % pt == 0, P divides H and W. */
int dvt_mae_loss_fwd(const void* pred, int pred_dtype, const void* clip, int clip_dtype, const int32_t* slot, float* per_patch,
                     float* stats, float* loss, int64_t frames, int C, int H, int W, int P, int pt, int k, int norm_pix,
                     float eps, dvt_stream_t stream);
/* dpred[s, j, :] = gloss[0] * 2 / (M * D) * (pred - target) at dropped positions, exactly 0 at kept ones; pred_dtype.  gloss is
 * a DEVICE f32 scalar; the target is recomputed from the clip with the forward's stats.  The clip gets no gradient. */
int dvt_mae_loss_bwd(const void* pred, int pred_dtype, const void* clip, int clip_dtype, const int32_t* slot,
                     const float* stats, const float* gloss, void* dpred, int64_t frames, int C, int H, int W, int P, int pt,
                     int k, int norm_pix, dvt_stream_t stream);

/* Row gather with an optional leading token (vit.py:120-123, x[:, 0] then
 * cat(temporal_token, .)):  out[b, 0, :] = tok (if tok != NULL, then lead = 1)
 * out[b, lead + t, :] = src[(b*T + t) * src_row_stride : + d].  */
int dvt_rows_gather_fwd(const void* src, int64_t src_row_stride, const float* tok, void* out,
                        int64_t B, int64_t T, int64_t d, int dtype, dvt_stream_t stream);
/* dsrc rows (same addressing) = dout[b, lead+t, :]; dtok (+)= sum_b dout[b,0,:].
 * Rows of dsrc that are not gathered are NOT touched (caller zero-fills). */
int dvt_rows_gather_bwd(const void* dout, void* dsrc, int64_t src_row_stride, float* dtok,
                        int64_t B, int64_t T, int64_t d, int dtype, int accumulate,
                        dvt_stream_t stream);

/* Scaled sum over the middle dimension: out[b, :] = scale * sum_j x[b, j, :].  scale = 1/L is
 * `x.mean(dim=1)` (pool == 'mean', src/models/vit.py:126) and the global AvgPool2d of the feature
 * pyramid (src/models/TPN.py:6,20,33); scale = 1 is `sum_group` (TPN.py:64-72).
 * bwd: dx[b, j, :] = scale * dout[b, :]. */
int dvt_mean_rows_fwd(const void* x, void* out, int64_t B, int64_t L, int64_t d, float scale, int dtype,
                      dvt_stream_t stream);
int dvt_mean_rows_bwd(const void* dout, void* dx, int64_t B, int64_t L, int64_t d, float scale, int dtype,
                      dvt_stream_t stream);

/* ---------------------------------------------------------------- LayerNorm
 * nn.LayerNorm(d), eps 1e-5, affine: src/models/vit.py:11,64,105;
 * src/models/frame_transformer.py:117; torch TransformerEncoderLayer norm1/2.
 * Rows are indexed (i0, i1), i0 < n0, i1 < n1; row (i0,i1) of x starts at element
 * i0*xs0 + i1*xs1, of y at i0*ys0 + i1*ys1 (dense: n0 = rows, n1 = 1, xs0 = ys0 = d).
 * mean/rstd: [n0*n1] f32, written by fwd, read by bwd. */
int dvt_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean,
                      float* rstd, int64_t n0, int64_t n1, int64_t d, int64_t xs0, int64_t xs1,
                      int64_t ys0, int64_t ys1, float eps, int dtype, dvt_stream_t stream);
size_t dvt_layernorm_bwd_workspace_bytes(int64_t d);
/* dy uses the y strides; x, dx and dx_add use the x strides.  dx = LN'(dy) (+ dx_add
 * when dx_add != NULL: the residual-branch gradient of `fn(LN(x)) + x`, vit.py:73-74,
 * so that the two gradient paths into x are summed inside this kernel).
 * dgamma/dbeta: [d] f32, overwritten (accumulate == 0) or added to.  workspace: at
 * least dvt_layernorm_bwd_workspace_bytes(d) bytes of device memory. */
int dvt_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean,
                      const float* rstd, const void* dx_add, void* dx, float* dgamma,
                      float* dbeta, void* workspace,
                      int64_t n0, int64_t n1, int64_t d, int64_t xs0, int64_t xs1, int64_t ys0,
                      int64_t ys1, int dtype, int accumulate, dvt_stream_t stream);
/* The same with (a) two more operands that enter only the FIRST row of each group (i1 == 0), indexed by i0:
 * dy_first is added to dy before the backward (a second gradient path into LN(x)[:, 0]: the query projection
 * of a block whose output is read at the CLS row only, src/models/vit.py:119-120 `x[:, 0]`), dx_first is added
 * to dx (the residual path of that row); either may be NULL; and (b) separate accumulate flags for dgamma and
 * dbeta (the two may sit in different gradient buckets). */
int dvt_layernorm_bwd_first(const void* dy, const void* x, const float* gamma, const float* mean,
                            const float* rstd, const void* dx_add, void* dx, float* dgamma, float* dbeta,
                            void* workspace,
                            int64_t n0, int64_t n1, int64_t d, int64_t xs0, int64_t xs1, int64_t ys0,
                            int64_t ys1, const void* dy_first, int64_t dy_first_stride,
                            const void* dx_first, int64_t dx_first_stride, int dtype,
                            int accumulate_gamma, int accumulate_beta, dvt_stream_t stream);

/* The general forms.  _fwd_mixed: x and y may differ in element type -- fp32 on exactly one side, a 16-bit type on the
 * other: the launch-bound zone of the path (the 33-token temporal encoder of vit.py:122-128, 264 rows at B = 8) keeps its
 * residual stream and its row gradients in fp32 (there single rows carry whole gradients; storage there costs no
 * bandwidth), while the GEMM operands stay 16-bit.  _bwd_ex: dy / x / dx element types separately (all equal; or dy 16-bit,
 * x and dx fp32, plus dx_lp, a 16-bit copy of dx for the GEMMs behind; or dy fp32, x and dx 16-bit: the seam where the fp32
 * stream meets the space stack's rows); defer_reduce leaves the dgamma / dbeta reduce of the per-workgroup partial rows
 * undone and describes it in *pending -- dvt_layernorm_reduce_group then performs up to 32 of them in ONE launch (the zone
 * has a dozen LayerNorms whose reduces were a launch of ~5 us each).  The partial rows live in `workspace`
 * (>= dvt_layernorm_bwd_partial_bytes(rows, d)), which must stay untouched until that launch. */
typedef struct dvt_ln_pending {
  const float* partial;   /* [nparts][2][d] */
  int32_t nparts, d;
  float* dgamma;
  float* dbeta;
  int32_t accumulate;     /* bit 0: dgamma +=, bit 1: dbeta += */
  int32_t valid;
} dvt_ln_pending;
typedef struct dvt_ln_bwd_desc {
  const void* dy; int32_t dy_dtype;
  const void* x; int32_t x_dtype;
  const float* gamma; const float* mean; const float* rstd;
  const void* dx_add;                    /* dx_dtype, x strides; may be NULL */
  void* dx; int32_t dx_dtype;
  void* dx_lp; int32_t dx_lp_dtype;      /* optional second copy of dx, x strides */
  float* dgamma; float* dbeta; void* workspace;
  int64_t n0, n1, d, xs0, xs1, ys0, ys1;
  const void* dy_first; int64_t dy_first_stride;   /* dy_dtype */
  const void* dx_first; int64_t dx_first_stride;   /* dx_dtype */
  int32_t accumulate_gamma, accumulate_beta;
  int32_t defer_reduce;
  dvt_ln_pending* pending;
} dvt_ln_bwd_desc;
int dvt_layernorm_fwd_mixed(const void* x, int x_dtype, const float* gamma, const float* beta, void* y, int y_dtype, float* mean,
                            float* rstd, int64_t n0, int64_t n1, int64_t d, int64_t xs0, int64_t xs1,
                            int64_t ys0, int64_t ys1, float eps, dvt_stream_t stream);
size_t dvt_layernorm_bwd_partial_bytes(int64_t rows, int64_t d);
int dvt_layernorm_bwd_ex(const dvt_ln_bwd_desc* desc, dvt_stream_t stream);
int dvt_layernorm_reduce_group(const dvt_ln_pending* list, int count, dvt_stream_t stream);

/* ---------------------------------------------------------------- GEMM family
 * C[M,N] = epilogue( sum_k A(m,k) * B(k,n) ).  One kernel family serves
 *   forward  Linear        y = x W^T          (A k-major, B = W[N,K] k-major)
 *   dgrad                  dx = dy W          (A k-major, B = W[K=N_out, N=K_in] mn-major)
 *   wgrad                  dW = dy^T x        (A, B mn-major; reduction over rows)
 * and so replaces nn.Linear at src/models/vit.py:20-25,39-43,91,106 and inside
 * torch's TransformerEncoderLayer (frame_transformer.py:41-44).
 *   a_kmajor: element (m,k) at A[m*lda + k]  else at A[k*lda + m]
 *   b_kmajor: element (k,n) at B[n*ldb + k]  else at B[k*ldb + n]
 */
enum dvt_epilogue {
  DVT_EPI_NONE = 0,          /* C = acc (+ bias) */
  DVT_EPI_GELU = 1,          /* C = gelu_erf(acc + bias); aux (if != NULL) = gelu_erf'(acc + bias), what DVT_EPI_DGELU takes */
  DVT_EPI_RELU = 2,          /* C = relu(acc + bias) */
  DVT_EPI_RESIDUAL = 3,      /* C = acc + bias + residual */
  DVT_EPI_DGELU = 4,         /* C = acc * aux          (aux = the derivative saved by DVT_EPI_GELU) */
  DVT_EPI_DRELU = 5          /* C = acc * (aux > 0)    (aux = saved post-activation) */
};

/* A split-K reduction that a dvt_gemm call left undone (desc.defer_reduce): C (+)= sum_z slab[z] in slice order, and
 * the fused bias gradient's partial rows.  It is handed to the NEXT dvt_gemm call of the same stream (desc.carry) --
 * the data gradient of the same Linear, src/models/vit.py:20-25,39-43 backward --, whose launch performs it in extra
 * workgroups at the END of its grid: a data-gradient launch is 1.5-6 rounds of tiles and leaves CUs idle in its last
 * round, which is where a reduce that reads 64 MB of slabs then runs instead of as a launch of its own.  A call that
 * cannot carry it (not the LDS-DMA kernel) launches it stand-alone first; dvt_splitk_reduce_pending does so explicitly.
 * The slabs live in the deferring call's workspace: it must stay untouched until the carrying call has been enqueued. */
typedef struct dvt_splitk_pending {
  const float* slab;       /* [splits][M][N] f32 */
  int32_t splits, valid;   /* valid == 0: nothing pending (the deferring call did not split K) */
  int64_t M, N;
  float* C;                /* f32 [M, ldc] */
  int64_t ldc;
  int32_t accumulate;
  int32_t cs_accumulate;
  const float* cs_slab;    /* [splits][M] f32 or NULL */
  float* cs_out;           /* [M] f32 */
  /* conv_taps > 0: the product is the weight gradient of a convolution, rows m = tap * conv_cin + ci, columns n = co, and
   * the reduce scatters it straight into the parameter's own layout C[co][ci][tap] (f32 [N][conv_cin][conv_taps], ldc
   * unused): no packed intermediate, no scatter launch behind the reduce. */
  int32_t conv_cin, conv_taps;
  /* channel-padded layers: only n < conv_cout_l and ci < conv_cin_l exist in the parameter f32 [conv_cout_l][conv_cin_l]
   * [conv_taps] (0: the GEMM's own N / conv_cin) */
  int32_t conv_cin_l, conv_cout_l;
} dvt_splitk_pending;

typedef struct dvt_gemm_desc {
  const void* A;
  const void* B;
  void* C;
  int64_t M, N, K;
  int64_t lda, ldb, ldc;
  int32_t a_kmajor, b_kmajor;
  int32_t in_dtype;     /* dtype of A, B, residual, aux */
  int32_t out_dtype;    /* dtype of C: in_dtype, or DVT_F32 (weight gradients) */
  int32_t epilogue;     /* enum dvt_epilogue */
  int32_t accumulate;   /* out_dtype == DVT_F32 only: C += result instead of C = result */
  const float* bias;    /* [N] f32 or NULL */
  const void* residual; /* [M, ldr] or NULL */
  int64_t ldr;
  void* aux;            /* [M, ldaux] or NULL */
  int64_t ldaux;
  float alpha;          /* result scale applied to acc before the epilogue (1.0f default) */
  int32_t split_k;      /* 0 = library chooses; >1 forces that many K slices */
  void* workspace;      /* >= dvt_gemm_workspace_bytes(desc) bytes (may be NULL if that is 0) */
  /* Optional, mn-major A only (weight gradients, A = dY): colsum_out[m] (+)= sum_k A(m,k),
   * i.e. the bias gradient, produced by the same pass over dY (an extra MFMA against an
   * all-ones fragment) instead of a separate reduction.  NULL = off. */
  float* colsum_out;
  int32_t colsum_accumulate;
  /* Optional (both may be NULL / 0).  defer_reduce: when this call splits K with the plain f32 reduce behind it
   * (weight gradients), leave the reduce undone and describe it in *pending (pending->valid = 0 when there is none).
   * carry: a pending reduce of an earlier call to perform with this call (see dvt_splitk_pending). */
  int32_t defer_reduce;
  dvt_splitk_pending* pending;
  const dvt_splitk_pending* carry;
  /* RESIDUAL epilogue with an fp32 residual [M, ldr] (and out_dtype DVT_F32): y32 = x W^T + b + r32 -- the residual stream of
   * the launch-bound zone (the 33-token temporal encoder) is kept in fp32 while the GEMM operands stay 16-bit.  Served by
   * the panel-streaming kernel (launch-bound shapes) only; other shapes report DVT_ERR_UNSUPPORTED. */
  int32_t residual_f32;
} dvt_gemm_desc;

size_t dvt_gemm_workspace_bytes(const dvt_gemm_desc* desc);
int dvt_gemm(const dvt_gemm_desc* desc, dvt_stream_t stream);
/* Which kernel family dvt_gemm would take for desc (no launch): 0 = the panel-streaming kernel of the launch-bound shapes
 * (the only one that serves residual_f32), 1 = the LDS-DMA / register-staged MFMA kernels, 2 = the generic fp32 kernel. */
int dvt_gemm_route(const dvt_gemm_desc* desc);
/* What dvt_gemm would launch for desc, taken from the same decisions the launcher makes (ABI v5 addition; host only, runs
 * without a device: the CU-count dependent thresholds then assume the MI355X's 256).  The workspace, defer_reduce and
 * carry fields of desc count: a planned split with no workspace runs unsplit on the 128x128 kernel, and `carry` reports
 * what becomes of a valid desc->carry.  Returns what dvt_gemm returns for a descriptor it refuses, else DVT_OK. */
enum dvt_gemm_kernel {
  DVT_GEMM_K_NONE = 0,         /* nothing to launch (M == 0 or N == 0) */
  DVT_GEMM_K_SMALL = 1,        /* gemm_small_kernel (panel streaming, tile_m rows per tile) */
  DVT_GEMM_K_SMALL_PAIR = 2,   /* gemm_small_pair_kernel (dvt_gemm_pair_plan only) */
  DVT_GEMM_K_DMA = 3,          /* gemm_dma_kernel, 256-row tiles, configuration cfg */
  DVT_GEMM_K_DMA224 = 4,       /* gemm_dma_kernel, configuration 8 (224-row tiles) */
  DVT_GEMM_K_MFMA128 = 5,      /* gemm_mfma_kernel (128x128 register-staged) */
  DVT_GEMM_K_GENERIC64 = 6,    /* gemm_generic_kernel (64x64 FMA tiles) */
  DVT_GEMM_K_TINY_WAVE = 7,    /* gemm_tiny_kernel, one wave per output */
  DVT_GEMM_K_TINY_THREAD = 8   /* gemm_tiny_kernel, one thread per output */
};
enum dvt_gemm_reduce {         /* what sums the split-K slabs */
  DVT_GEMM_R_NONE = 0,         /* no split */
  DVT_GEMM_R_PLAIN = 1,        /* splitk_reduce_kernel (with the fused bias gradient's rows where colsum is FUSED) */
  DVT_GEMM_R_EPILOGUE = 2,     /* splitk_reduce_epi_kernel (bias / alpha / activation / residual after the sum) */
  DVT_GEMM_R_DEFERRED = 3      /* left undone in *desc->pending */
};
enum dvt_gemm_colsum {         /* how colsum_out is produced */
  DVT_GEMM_CS_NONE = 0,
  DVT_GEMM_CS_FUSED = 1,       /* by the GEMM launch itself (panel kernel; LDS-DMA slabs summed by the reduce) */
  DVT_GEMM_CS_ALONE = 2        /* by dvt_colsum, a launch of its own */
};
enum dvt_gemm_carry {          /* what becomes of a valid desc->carry */
  DVT_GEMM_CARRY_NONE = 0,
  DVT_GEMM_CARRY_TAIL = 1,     /* rides in the grid tail of this call's LDS-DMA launch */
  DVT_GEMM_CARRY_ALONE = 2,    /* launched on its own first: splitk_reduce_kernel */
  DVT_GEMM_CARRY_WIDE = 3,     /* launched on its own first: splitk_reduce_wide_kernel (>= 64 slices, M*N <= 2^20) */
  DVT_GEMM_CARRY_CONV = 4      /* launched on its own first: a convolution-scatter reduce */
};
typedef struct dvt_gemm_plan_info {
  int32_t route;        /* as dvt_gemm_route */
  int32_t kernel;       /* enum dvt_gemm_kernel */
  int32_t cfg;          /* LDS-DMA configuration (DMA / DMA224), else -1 */
  int32_t split;        /* K slices (1: none) */
  int32_t k_per_split;  /* DMA / MFMA128: K per slice, a multiple of 64; else 0 */
  int32_t tile_m;       /* SMALL / SMALL_PAIR: rows per tile (32 or 64); else 0 */
  int32_t reduce;       /* enum dvt_gemm_reduce */
  int32_t colsum;       /* enum dvt_gemm_colsum */
  int32_t carry;        /* enum dvt_gemm_carry */
  /* the instantiation launched: operand layouts, epilogue (DVT_EPI_NONE where the reduce applies it: LDS-DMA slabs) and
   * output form (0 = in_dtype, 1 = f32, 2 = f32 split-K slabs) */
  int32_t a_kmajor, b_kmajor, epilogue, out_form;
} dvt_gemm_plan_info;
int dvt_gemm_plan(const dvt_gemm_desc* desc, dvt_gemm_plan_info* info);
/* dvt_gemm_pair's launches: both SMALL_PAIR when they are one launch (dvt_gemm_pair_fused), else dvt_gemm_plan of each. */
int dvt_gemm_pair_plan(const dvt_gemm_desc* wgrad, const dvt_gemm_desc* dgrad, dvt_gemm_plan_info* wgrad_info,
                       dvt_gemm_plan_info* dgrad_info);
/* The two products of one Linear's backward (src/models/vit.py:20-25,39-43: dW = dy^T x with both operands mn-major,
 * dx = dy W with A k-major / B mn-major) as ONE launch when both are launch-bound shapes (the 33-token temporal encoder,
 * the CLS-row layers: a few hundred rows): they are independent, each fills a fraction of the chip, and between dependent
 * launches of a few microseconds the launch itself is the cost.  Any other pair: the two dvt_gemm calls one after the
 * other.  dvt_gemm_pair_fused tells which (1 = one launch). */
int dvt_gemm_pair_fused(const dvt_gemm_desc* wgrad, const dvt_gemm_desc* dgrad);
int dvt_gemm_pair(const dvt_gemm_desc* wgrad, const dvt_gemm_desc* dgrad, dvt_stream_t stream);
/* Performs a pending split-K reduction as a launch of its own. */
int dvt_splitk_reduce_pending(const dvt_splitk_pending* pending, dvt_stream_t stream);

/* out[n] (+)= sum_m x[m*ldx + n]  -- bias gradients. workspace >=
 * dvt_colsum_workspace_bytes(M, N). */
size_t dvt_colsum_workspace_bytes(int64_t M, int64_t N);
int dvt_colsum(const void* x, int64_t ldx, float* out, void* workspace, int64_t M, int64_t N,
               int dtype, int accumulate, dvt_stream_t stream);

/* ---------------------------------------------------------------- attention
 * o = softmax(q k^T * scale) v per (batch, head): src/models/vit.py:51-55, and
 * the core of nn.MultiheadAttention inside TransformerEncoderLayer
 * (frame_transformer.py:41-44).  Lq != Lk gives the cross-modal form
 * (frame_transformer.py:225-226 joint video/image tokens; BASELINE config 4).
 * Element (b, h, l, e) of q sits at q[b*q_sb + h*q_sh + l*q_sl + e]; likewise
 * k, v, o.  do/dq/dk/dv reuse the strides of o/q/k/v.  lse: [B, H, Lq] f32
 * (log-sum-exp of the scaled scores), written by fwd and read by bwd.
 * Scores are never materialised in HBM. */
typedef struct dvt_attn_desc {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  float* lse;
  const void* d_o; /* bwd only */
  void* dq;        /* bwd only */
  void* dk;
  void* dv;
  int64_t B, H, Lq, Lk, dh;
  int64_t q_sb, q_sh, q_sl;
  int64_t k_sb, k_sh, k_sl;
  int64_t v_sb, v_sh, v_sl;
  int64_t o_sb, o_sh, o_sl;
  float scale;
  int32_t dtype;
  void* workspace; /* bwd only: >= dvt_attention_bwd_workspace_bytes(desc) bytes (may be NULL if 0): holds
                    * delta = rowsum(dO * O), written by the dq pass and read by the dk/dv pass */
  /* Attention-probability dropout, nn.MultiheadAttention(dropout=p) in training mode (frame_transformer.py:41-44):
   * o = (softmax(s) * keep / (1 - p)) v, keep(b,h,i,j) drawn like dvt_dropout from rng_state (device {seed, base})
   * at rng_offset + (((b*H + h)*Lq + i)*Lk + j) / 4.  0 = off.  Served by the generic (non-MFMA) kernels. */
  float dropout_p;
  const uint64_t* rng_state;
  uint64_t rng_offset;
  /* bwd, 16-bit dh = 64 kernels: sequences whose two lengths pad to the same multiple of 32 <= 224 (the 197-token frames,
   * the 33-token clips) run as ONE pass -- Q, dO, K staged once, dK / dV kept in registers by key-owner waves, dQ formed by
   * a dedicated wave from 16-bit dS strips in LDS (5 MFMA products and 8 units of traffic instead of the 7 and 13 of the
   * dq + dk/dv pair).  bwd_two_pass != 0 forces the pair (longer sequences always use it). */
  int32_t bwd_two_pass;
} dvt_attn_desc;

size_t dvt_attention_bwd_workspace_bytes(const dvt_attn_desc* desc);
int dvt_attention_fwd(const dvt_attn_desc* desc, dvt_stream_t stream);
int dvt_attention_bwd(const dvt_attn_desc* desc, dvt_stream_t stream);
/* What dvt_attention_fwd (bwd == 0) or dvt_attention_bwd (bwd != 0) would launch for desc, taken from the same decisions
 * the launchers make (ABI v5 addition; host only, runs without a device).  The workspace pointer is not required: the
 * `workspace` field says whether the launch would use it.  Returns what the launcher returns for a descriptor it refuses,
 * else DVT_OK (family NONE when B == 0). */
enum dvt_attn_family {
  DVT_ATTN_F_NONE = 0,
  DVT_ATTN_F_Q1 = 1,        /* fwd: attn_fwd_q1_kernel (Lq == 1, dh == 64) */
  DVT_ATTN_F_RES = 2,       /* fwd: attn_fwd_mfma_res_kernel<E, count> (whole score row in registers, <= 352 keys) */
  DVT_ATTN_F_ONLINE = 3,    /* fwd: attn_fwd_mfma_kernel (online softmax over 32-key steps) */
  DVT_ATTN_F_SMALL = 4,     /* fwd: attn_small_fwd_kernel (both lengths <= 32) */
  DVT_ATTN_F_GENERIC = 5,   /* fwd: attn_fwd_generic_kernel (one wave per query row) */
  DVT_ATTN_B_Q1 = 6,        /* bwd: attn_bwd_q1_kernel */
  DVT_ATTN_B_FUSED = 7,     /* bwd: attn_bwd_fused_kernel<E, count> (one pass) */
  DVT_ATTN_B_PAIR = 8,      /* bwd: attn_bwd_dq_mfma_kernel<E, count> then attn_bwd_dkv_mfma_kernel<E, count2> */
  DVT_ATTN_B_SMALL = 9,     /* bwd: attn_small_bwd_kernel */
  DVT_ATTN_B_GENERIC = 10   /* bwd: attn_delta_kernel, attn_bwd_dq_generic_kernel, attn_bwd_dkv_generic_kernel */
};
typedef struct dvt_attn_plan_info {
  int32_t family;     /* enum dvt_attn_family */
  int32_t count;      /* template count of the (first) launch: RES NKP, FUSED NP, PAIR the dq kernel's NKP (0 = rolled) */
  int32_t count2;     /* PAIR: the dk/dv kernel's NQP (0 = rolled); else 0 */
  int32_t waves;      /* waves per block of the (first) launch */
  int32_t waves2;     /* PAIR / GENERIC bwd: of the dk/dv launch; else 0 */
  int32_t patch;      /* RES / ONLINE / PAIR dq: 1 = output tiles stored as whole rows through LDS patches, 0 = per lane;
                       * -1 for families without the choice */
  int32_t patch2;     /* PAIR: the same for the dk/dv launch; else -1 */
  int32_t workspace;  /* 1 if the launch reads and writes desc->workspace */
  int64_t lds;        /* dynamic LDS bytes of the (first) launch */
  int64_t lds2;       /* of the dk/dv launch (PAIR, GENERIC bwd); else 0 */
} dvt_attn_plan_info;
int dvt_attention_plan(const dvt_attn_desc* desc, int bwd, dvt_attn_plan_info* info);

/* Streamed MFMA attention: the same computation on the same descriptor for sequences of any length (csrc/attention.hip,
 * attn_long_*).  A workgroup owns a block of query rows (forward, dq) or key rows (dk/dv) of one (batch, head) and the other
 * side passes through LDS in double-buffered chunks, so neither length is bounded by LDS; lse keeps its definition, so
 * either backward can follow either forward.  16-bit types, dh == 64, dropout_p == 0, scale > 0, strides that are multiples
 * of 8 and 16-byte aligned pointers: dvt_attention_long_supported (host only; bwd != 0 includes the gradient pointers)
 * returns 1 for such a descriptor and 0 otherwise, and the launchers refuse what it refuses with DVT_ERR_UNSUPPORTED.  The
 * backward is two launches (dq, which writes delta = rowsum(dO * O) to the workspace, then dk/dv), without atomics, bitwise
 * reproducible; bwd_two_pass is ignored.  dvt_attention_long_plan (host only) reports the launchers' decisions. */
typedef struct dvt_attn_long_plan_info {
  int32_t q_block;    /* fwd / dq launch: query rows per workgroup */
  int32_t k_chunk;    /* fwd / dq launch: keys per LDS chunk (a multiple of 32) */
  int32_t waves;      /* fwd / dq launch: waves per workgroup */
  int32_t ring;       /* fwd / dq launch: chunk buffers in LDS */
  int32_t patch;      /* fwd / dq launch: 1 = output tiles stored as whole rows through LDS patches */
  int32_t k_block;    /* bwd, dk/dv launch: key rows per workgroup; else 0 */
  int32_t q_chunk;    /* bwd, dk/dv launch: queries per LDS chunk; else 0 */
  int32_t waves2;     /* bwd, dk/dv launch; else 0 */
  int32_t ring2;      /* bwd, dk/dv launch; else 0 */
  int32_t patch2;     /* bwd, dk/dv launch; else -1 */
  int32_t workspace;  /* 1 if the launch reads and writes desc->workspace */
  int32_t chunks;     /* fwd / dq launch: chunks each workgroup streams */
  int32_t chunks2;    /* bwd, dk/dv launch; else 0 */
  int64_t grid;       /* workgroups of the fwd / dq launch */
  int64_t grid2;      /* of the dk/dv launch; else 0 */
  int64_t lds;        /* dynamic LDS bytes of the fwd / dq launch */
  int64_t lds2;       /* of the dk/dv launch; else 0 */
} dvt_attn_long_plan_info;
int dvt_attention_long_supported(const dvt_attn_desc* desc, int bwd);
size_t dvt_attention_long_bwd_workspace_bytes(const dvt_attn_desc* desc);
int dvt_attention_long_fwd(const dvt_attn_desc* desc, dvt_stream_t stream);
int dvt_attention_long_bwd(const dvt_attn_desc* desc, dvt_stream_t stream);
int dvt_attention_long_plan(const dvt_attn_desc* desc, int bwd, dvt_attn_long_plan_info* info);

/* ---------------------------------------------------------------- single-query attention with folded K / V projections
 * The reference reads only row 0 of the space transformer's output (src/models/vit.py:119-120; :126 for the temporal
 * one under pool == 'cls'), so the attention of a stack's LAST layer (vit.py:46-58) has ONE query per (sequence, head),
 * and with one query the key / value projections of to_qkv (vit.py:39,48) commute with the attention sums:
 *     s_jh = scale q_h . (Wk_h LN(x_j)) = r_h . LN(x_j),   r_h = scale Wk_h^T q_h   (dvt_heads_expand)
 *     o_h  = sum_j p_jh Wv_h LN(x_j)    = Wv_h m_h,         m_h = sum_j p_jh LN(x_j) (dvt_heads_contract)
 * -- neither K, V nor LN(x) of the rows that are never read again is materialised: dvt_attn_cls_fwd is one pass over
 * the raw rows x[S][N][d] (LayerNorm statistics, H scores and H weighted sums per row), dvt_attn_cls_bwd one more, which
 * also is the LayerNorm backward of those rows (the gradient of row 0's own query / residual paths is added by a
 * dvt_layernorm_bwd call on the S first rows).  Row (s, j) of x sits at x + s*xs0 + j*xs1 (elements); dx uses the same
 * strides.  All [S, H, d] arrays are f32.  With n_j = (x_j - mean_j) rstd_j, LN(x_j) = gamma n_j + beta:
 *   fwd:  R -> A[s,h,:] = sum_j p_jh n_j (so m_h = gamma A_h + beta), lse[S,H], the probabilities P[S,N,8] (head h of row
 *         j at P[(s*N + j)*8 + h]; kept for the backward), mean / rstd [S*N]
 *   bwd:  dM (gradient of m) -> dx, G[s,h,:] = sum_j ds_jh n_j (so dr_h = gamma G_h), dgamma / dbeta (+= when the
 *         accumulate flags are set; workspace >= dvt_attn_cls_bwd_workspace_bytes holds one partial row per sequence).
 * 16-bit dtypes, d % 8 == 0, d <= 512, H <= 8, N <= 400 (sequences of more than 200 rows -- the 325-token frames of a 288^2
 * clip -- are walked in two chunks per pass); dvt_attn_cls_supported tells (callers keep the unfolded
 * dvt_layernorm_fwd -> dvt_gemm -> dvt_attention_fwd sequence otherwise). */
typedef struct dvt_attn_cls_desc {
  const void* x;
  int64_t xs0, xs1;
  const float* gamma;
  const float* beta;
  float eps;
  int64_t S, N, d, H;
  int32_t dtype;
  const float* R;
  float* A;
  float* lse;
  float* P;
  float* mean;
  float* rstd;
  /* backward only */
  const float* dM;
  void* dx;
  float* G;
  float* dgamma;
  float* dbeta;
  int32_t accumulate_gamma, accumulate_beta;
  void* workspace;
} dvt_attn_cls_desc;

int dvt_attn_cls_supported(const dvt_attn_cls_desc* desc);
size_t dvt_attn_cls_bwd_workspace_bytes(const dvt_attn_cls_desc* desc);
int dvt_attn_cls_fwd(const dvt_attn_cls_desc* desc, dvt_stream_t stream);
int dvt_attn_cls_bwd(const dvt_attn_cls_desc* desc, dvt_stream_t stream);
/* The head-wise products on either side of it, over S rows only; W is a row range of the packed to_qkv weight
 * (vit.py:39; [H*dh, ldw] in the 16-bit compute dtype), the [S, H, d] operands are f32 and, when gamma / beta are
 * given, enter as gamma * v + beta (either may be NULL):
 *   expand:   out[s, h, c]     = alpha sum_e in[s, h*dh + e] W[h*dh + e, c]                (q -> r, do -> dm)
 *   contract: out[s, h*dh + e] = alpha sum_c v[s, h, c] W[h*dh + e, c]                      (m -> o, dr -> dq)
 *   outer:    dW[h*dh + e, c] (+)= alpha sum_s a[s, h*dh + e] v[s, h, c]                    (weight gradients of Wv, Wk) */
int dvt_heads_expand(const void* in, int64_t ld_in, const void* W, int64_t ldw, float* out, int64_t S, int64_t H,
                     int64_t dh, int64_t d, float alpha, int dtype, dvt_stream_t stream);
int dvt_heads_contract(const float* in, const float* gamma, const float* beta, const void* W, int64_t ldw, void* out,
                       int64_t ld_out, int64_t S, int64_t H, int64_t dh, int64_t d, float alpha, int dtype,
                       dvt_stream_t stream);
int dvt_heads_outer(const void* a, int64_t lda, const float* b, const float* gamma, const float* beta, float* dW,
                    int64_t ldw, int64_t S, int64_t H, int64_t dh, int64_t d, float alpha, int accumulate, int dtype,
                    dvt_stream_t stream);
/* The backward runs them in two independent pairs, one launch each (workgroups of the first member in front):
 *   expand_outer:    out = alpha_out expand(in, W);          dW (+)= alpha_dw outer(in, gamma v + beta)     (dm and dWv from do)
 *   contract_outer:  out = alpha_out contract(gamma v, W);   dW (+)= alpha_dw outer(a, gamma v)             (dq and dWk from G) */
int dvt_heads_expand_outer(const void* in, int64_t ld_in, const void* W, int64_t ldw, float* out, float alpha_out,
                           const float* v, const float* gamma, const float* beta, float* dW, int64_t ld_dw, float alpha_dw,
                           int accumulate, int64_t S, int64_t H, int64_t dh, int64_t d, int dtype, dvt_stream_t stream);
int dvt_heads_contract_outer(const float* v, const float* gamma, const void* W, int64_t ldw, void* out, int64_t ld_out,
                             float alpha_out, const void* a, int64_t lda, float* dW, int64_t ld_dw, float alpha_dw,
                             int accumulate, int64_t S, int64_t H, int64_t dh, int64_t d, int dtype, dvt_stream_t stream);

/* ---------------------------------------------------------------- on-device input stage
 * transforms.Compose([Resize(resize), CenterCrop(crop), ToTensor(), Normalize(mean, std)]) of the reference's loader
 * (src/dataloaders/mmx/MMX_Light_dl.py:203-217; val_transform :195-201) applied to decoded uint8 RGB frames
 * src[F, H0, W0, 3] already resident in HBM; dst[F, 3, crop, crop] (f32: bit-exact with PIL + torch; bf16: that
 * value rounded to nearest even).  Resize = Pillow 8-bit bilinear resample (antialiased triangle filter, 22-bit fixed
 * point, horizontal then vertical pass through a uint8 intermediate in the workspace).  mean/std are host arrays of 3. */
size_t dvt_frames_preprocess_workspace_bytes(int64_t frames, int H0, int W0, int resize, int crop);
int dvt_frames_preprocess(const void* src, void* dst, int dst_dtype, int64_t frames, int H0, int W0, int resize,
                          int crop, const float* mean, const float* std, void* workspace, dvt_stream_t stream);
/* Addition within ABI v5: the random training augmentations of the frame loader, with the random draws made by the caller.
 *   image branch  RandomResizedCrop(224) -> RandomHorizontalFlip(0.3) -> RandomVerticalFlip(0.3) -> AutoAugment ->
 *                 ToTensor -> Normalize   (src/dataloaders/mmx/MMX_Frame_dl.py:63-71, live at :154)
 *   video branch  Resize(120) -> CenterCrop(112) -> ToTensor -> Normalize -> RandomErasing()   (:81-88, live at :152-153)
 * dvt_frames_augment: sample n of `samples` reads frame table[n].src_index of src[frames, H0, W0, 3] (uint8, device) and is
 *   img.crop((left, top, left + w, top + h)).resize((out_w, out_h), BILINEAR), transpose(FLIP_LEFT_RIGHT) if hflip,
 *   transpose(FLIP_TOP_BOTTOM) if vflip, then ToTensor + Normalize -- Pillow's 8-bit resample as above, its taps clipped to
 *   the crop window (not to the frame).  table: HOST array of samples x 7 int32 rows {src_index, top, left, h, w, hflip,
 *   vflip}, validated whole before any launch (0 <= src_index < frames; h, w >= 1; window inside the frame; flips 0 / 1): a
 *   bad row returns DVT_ERR_BAD_ARG and dvt_last_error() names it.  dst_dtype: a dvt_dtype -> dst[samples, 3, out_h, out_w]
 *   normalised; DVT_AUGMENT_U8_HWC -> dst[samples, out_h, out_w, 3] uint8, not normalised (mean / std unused; the
 *   input of dvt_frames_autoaugment).  One coefficient launch per 64 samples and one fused launch: a workgroup resamples the
 *   input rows of a band of output rows horizontally into LDS (uint8) and runs the vertical pass from there; no
 *   intermediate image in HBM.  The band height is chosen so that the band of a full-height window fits 64 KiB of LDS;
 *   a geometry whose single output row does not fit is refused (DVT_ERR_UNSUPPORTED; workspace_bytes returns 0).
 * dvt_frames_erase: RandomErasing with a constant fill, in place on x[frames, 3, H, W] (dtype): table is a HOST array of
 *   frames x 4 int32 rows {top, left, h, w}; h == 0 leaves the frame alone, otherwise h, w >= 1 and the rectangle lies inside
 *   the frame (H, W <= 65535).  value: host array of 3 (one fill per channel).  Writes the rectangles only. */
enum dvt_augment_dst { DVT_AUGMENT_U8_HWC = 8 };
size_t dvt_frames_augment_workspace_bytes(int64_t samples, int H0, int W0, int out_h, int out_w);
int dvt_frames_augment(const void* src, int64_t frames, int H0, int W0, const int32_t* table, int64_t samples, void* dst,
                       int dst_dtype, int out_h, int out_w, const float* mean, const float* std, void* workspace,
                       dvt_stream_t stream);
int dvt_frames_erase(void* x, int dtype, int64_t frames, int H, int W, const int32_t* table, const float* value,
                     dvt_stream_t stream);
/* Addition within ABI v5: Mixup / CutMix across the batch (timm.data.Mixup; for clips the VideoMix form, one box for all
 * frames and channels of a sample), a stage behind the transform chains above (MMX_Frame_dl.py:63-88 has none), the mixed
 * targets (timm's mixup_target) and the loss that accepts them (timm.loss.SoftTargetCrossEntropy; with a smoothed one-hot
 * target it is nn.CrossEntropyLoss(label_smoothing=) of src/models/basicmlp.py:38).  The random draws are the caller's.
 * Every argument is validated on the host before any HIP call; a bad table row returns DVT_ERR_BAD_ARG and
 * dvt_last_error() names it.
 * dvt_clips_mix: x[B, T, C, H, W] (dtype, contiguous).  table: HOST array of B x 8 int32 rows {partner, kind, t0, t1, y0, y1,
 *   x0, x1}, kind 0 = leave alone, 1 = mixup, 2 = cutmix with the half-open box (read for kind 2 only) shared by every
 *   channel; lam: HOST array of B floats in [0, 1].
 *     kind 1   out[i] = fmaf(lam_i, x[i], (1.0f - lam_i) * x[partner_i]) in fp32, rounded once to dtype
 *     kind 2   out[i][box] = x[partner_i][box], a copy; the rest of out[i] is x[i]
 *   Kind 0, partner_i == i, an empty box and kind 1 with lam_i == 1 leave sample i bit for bit as it is.  out == NULL or
 *   out == x: in place; the partner map must then be an involution (partner[partner[i]] == i, refused otherwise), pairs
 *   i < partner_i are taken together -- a lane loads the same elements of both members, then stores both -- and no byte of
 *   an unchanged sample or outside a box is written; the result equals the out-of-place one bit for bit.  out disjoint
 *   from x: any partner map; every sample is written.  The work travels to the kernel by value, DVT_MIX_ROWS_PER_LAUNCH
 *   rows (a pair or sample and one region of it) per launch; launches with nothing to do are not made.  16-byte accesses
 *   wherever the addresses a row uses sit alike in their 16-byte lines, element accesses for the head and tail of a run
 *   and where they do not.  T x C x H x W < 2^30.
 * dvt_targets_mix: out[B, Ccls] f32 = lam_i * t_i + (1.0f - lam_i) * t_partner(i) with partner = column 0 of the same table
 *   and lam the target's lambda (for cutmix 1 - box volume / (T H W)); exactly one of y (f32 [B, Ccls], taken as it is) and
 *   labels (int64 [B]) is non-null; a label row is smoothing / Ccls everywhere and 1 - smoothing + smoothing / Ccls at the
 *   label.  A label outside [0, Ccls) is never used as an index: its row (and a row that mixes it in) is NaN.  A row with
 *   lam_i == 1 is its own target exactly.
 * dvt_ce_soft_fwd: loss[0] = mean over the M rows of sum_c -t_rc (x_rc - lse_r), fp32 arithmetic, fixed order; logits
 *   [M][ld] dtype, targets f32 [M][C]; lse f32 [2 M] receives the per-row log-sum-exp and, at [M + r], sum_c t_rc (rows need
 *   not sum to 1).  dvt_ce_soft_bwd: dlogits[r] = gloss[0] / M * (softmax(x_r) * sum_c t_rc - t_r).  No gradient to targets. */
#define DVT_MIX_ROWS_PER_LAUNCH 64
int dvt_clips_mix(void* x, void* out, int dtype, int64_t B, int T, int C, int H, int W, const int32_t* table,
                  const float* lam, dvt_stream_t stream);
int dvt_targets_mix(const float* y, const int64_t* labels, float* out, int64_t B, int64_t Ccls, const int32_t* table,
                    const float* lam, float smoothing, dvt_stream_t stream);
int dvt_ce_soft_fwd(const void* logits, int64_t ld, const float* targets, float* loss, float* lse, int64_t M, int64_t C,
                    int dtype, dvt_stream_t stream);
int dvt_ce_soft_bwd(const void* logits, int64_t ld, const float* targets, const float* lse, const float* gloss, void* dlogits,
                    int64_t lddl, int64_t M, int64_t C, int dtype, dvt_stream_t stream);
/* Addition within ABI v5: the AutoAugment stage of the image branch above (torchvision's AutoAugment on its PIL path, the
 * random draws made by the caller).  dvt_frames_autoaugment: sample n of src[samples, H, W, 3] (uint8, device) takes the
 *   two operations of table[n] in order.  table: HOST array of samples x 2 slots x 8 int32 {op, p0 .. p6}, validated whole
 *   before any HIP call (op in range; a posterize mask is a run of high bits; a blend factor is finite; a solarize threshold
 *   lies in [0, 256]): a bad slot returns DVT_ERR_BAD_ARG and dvt_last_error() names it; so are null pointers, by name.
 *     geometric (SHEAR_X .. ROTATE)       p0 .. p5 = a0 .. a5, Pillow's 16.16 fixed-point inverse affine matrix, a2 and a5 with
 *                                         the half-pixel offset: xin = (a2 + a1 y + a0 x) >> 16, yin = (a5 + a4 y + a3 x) >> 16,
 *                                         nearest, 0 outside the image (Image.transform(AFFINE, NEAREST), Image.rotate)
 *     blend (BRIGHTNESS .. SHARPNESS)     p0 = the bits of the float32 factor f: deg + f (img - deg) in float32, the product and
 *                                         the sum rounded separately, truncated for 0 <= f <= 1 and clipped otherwise
 *                                         (ImageEnhance); deg = 0 / luma / the rounded mean luma of the image / ImageFilter.SMOOTH
 *     POSTERIZE  p0 = the byte mask;  SOLARIZE  p0 = ceil(threshold): v < p0 ? v : 255 - v;  INVERT;  IDENTITY
 *     AUTOCONTRAST, EQUALIZE              per channel, from the channel's 256-bin histogram (ImageOps, cutoff 0)
 *   dst_dtype: DVT_AUGMENT_U8_HWC -> dst[samples, H, W, 3] uint8; a dvt_dtype -> dst[samples, 3, H, W] after ToTensor +
 *   Normalize in the float32 arithmetic of dvt_frames_augment (two IDENTITY slots give the bits of that entry point; mean / std
 *   unused for uint8).  One launch per 48 samples, one workgroup per sample: the first operation reads src and leaves its
 *   result in LDS as uint8, the second reads that image and writes dst; an operation that needs a statistic of its whole
 *   input (histograms, the luma sum: integer counts) makes a counting pass over that input first.  No workspace.  H, W >= 3,
 *   and 3 H W bytes must fit the LDS image of a workgroup (160,000 bytes: 224 x 224 fits); a larger image returns
 *   DVT_ERR_UNSUPPORTED. */
enum dvt_autoaugment_op { DVT_AA_IDENTITY = 0, DVT_AA_SHEAR_X = 1, DVT_AA_SHEAR_Y = 2, DVT_AA_TRANSLATE_X = 3,
  DVT_AA_TRANSLATE_Y = 4, DVT_AA_ROTATE = 5, DVT_AA_BRIGHTNESS = 6, DVT_AA_COLOR = 7, DVT_AA_CONTRAST = 8,
  DVT_AA_SHARPNESS = 9, DVT_AA_POSTERIZE = 10, DVT_AA_SOLARIZE = 11, DVT_AA_AUTOCONTRAST = 12, DVT_AA_EQUALIZE = 13,
  DVT_AA_INVERT = 14 };
int dvt_frames_autoaugment(const void* src, int64_t samples, int H, int W, const int32_t* table, void* dst, int dst_dtype,
                           const float* mean, const float* std, dvt_stream_t stream);

/* ---------------------------------------------------------------- multi-modal gating + contrastive loss
 * F.normalize(x) (collabgating.py:70) and the normaliser of F.cosine_similarity (ntxent.py:63):
 * y = x / max(||x||_2, eps) per row of [rows, D]; inv_norm[rows] is kept for backward. */
int dvt_l2norm_rows_fwd(const void* x, void* y, float* inv_norm, int64_t rows, int D, float eps, int dtype,
                        dvt_stream_t stream);
int dvt_l2norm_rows_bwd(const void* dy, const void* y, const float* inv_norm, void* dx, int64_t rows, int D, float eps,
                        int dtype, dvt_stream_t stream);
/* nn.CosineSimilarity(dim=1)(a, b) (frame_transformer.py:121, logged at :257): out[r] f32, no gradient. */
int dvt_cosine_rows(const void* a, const void* b, float* out, int64_t rows, int D, float eps, int dtype,
                    dvt_stream_t stream);
/* ContextGating: F.glu(cat(x, x + x1), -1) = x * sigmoid(x + x1) (collabgating.py:83-86): y = a * sigmoid(b). */
int dvt_gate_fwd(const void* a, const void* b, void* y, int64_t n, int dtype, dvt_stream_t stream);
int dvt_gate_bwd(const void* dy, const void* a, const void* b, void* da, void* db, int64_t n, int dtype,
                 dvt_stream_t stream);
/* ContrastiveLoss.forward on the cosine-similarity matrix sim[M, M] f32, M = 2 * batch (ntxent.py:63-75):
 * loss = mean_k( log sum_{j != k} exp(sim_kj / T) - sim_{k, (k + M/2) mod M} / T ).  row_lse[M], row_loss[M]: scratch /
 * saved for backward.  bwd: dsim = dloss/dsim scaled by gloss[0]. */
int dvt_contrastive_fwd(const float* sim, int M, float temperature, float* loss, float* row_lse, float* row_loss,
                        dvt_stream_t stream);
int dvt_contrastive_bwd(const float* sim, const float* row_lse, int M, float temperature, const float* gloss,
                        float* dsim, dvt_stream_t stream);

/* ---------------------------------------------------------------- evaluation reductions
 * scikit-learn calls of src/callbacks/callbacks.py:36-55 on running_logits / running_labels, on the device.
 * probs [N, C] f32 (sigmoid outputs, frame_transformer.py:331), labels [N, C] u8 (0 / non-zero).
 * dvt_f1_samples: out[j] = f1_score(labels, probs > thresholds[j], average="samples", zero_division=0);
 * thresholds is a host array of T <= 16 values (callbacks.py:38: 0, 0.1 .. 0.8).
 * dvt_average_precision: average_precision_score(labels, probs, average="samples" / "weighted" / None) ->
 * out_samples[1], out_weighted[1], out_per_class[C] (device f32); C <= 64.  The per-class values are the rank pass of
 * dvt_rank_metrics (its f64 AP rounded to f32), the weighted one their support-weighted mean. */
size_t dvt_f1_samples_workspace_bytes(int64_t N, int T);
int dvt_f1_samples(const float* probs, const unsigned char* labels, int64_t N, int C, const float* thresholds, int T,
                   float* out, void* workspace, dvt_stream_t stream);
size_t dvt_average_precision_workspace_bytes(int64_t N, int C);
int dvt_average_precision(const float* probs, const unsigned char* labels, int64_t N, int C, float* out_samples,
                          float* out_weighted, float* out_per_class, void* workspace, dvt_stream_t stream);
/* Addition within ABI v5: classification_report(labels, probs > threshold) of callbacks.py:67-82 (the test epoch), as
 * exact counts.  counts int64 [4, C] (device): rows TP, FP, FN, support per class.  row_sums f64 [3] (device): the sums
 * over the N rows of the per-row precision, recall and F1 (each 0 where its denominator is 0, zero_division=0), in a
 * fixed order.  Integer counts and fixed-order f64 sums, no atomics: two identical calls are bitwise equal.
 * workspace >= dvt_multilabel_report_workspace_bytes(N). */
size_t dvt_multilabel_report_workspace_bytes(int64_t N);
int dvt_multilabel_report(const float* probs, const unsigned char* labels, int64_t N, int C, float threshold,
                          int64_t* counts, double* row_sums, void* workspace, dvt_stream_t stream);

/* ---------------------------------------------------------------- per-frame CNN encoder
 * src/models/custom_resnet.py:19-153 (conv3x3 / 7x7 stem / 1x1 downsample, BatchNorm2d, ReLU,
 * MaxPool2d(3,2,1), residual adds).  Feature maps are NHWC = [N*H*W, C] matrices, so a
 * convolution is  dvt_im2col -> dvt_gemm -> [N*Ho*Wo, Cout];  weights nn.Conv2d [Cout,Cin,kh,kw]. */
/* out[(n,ho,wo), (ki*kw+kj)*C + c] = x[n, ho*sh-ph+ki, wo*sw-pw+kj, c] (0 outside); columns
 * [kh*kw*C, ld) are zero padding.  x is NCHW when x_nchw != 0 (the raw clip frames), else NHWC.
 * Rectangular kernels / strides / paddings also serve the factorised R(2+1)D convolutions
 * (frame_transformer.py:67): (1,3,3) spatial = per-frame 2-D conv; (3,1,1) temporal = a (3,1) conv over
 * the [T, H*W] view of each clip. */
int dvt_im2col(const void* x, int x_dtype, int x_nchw, void* out, int out_dtype, int64_t N, int C, int H,
               int W, int kh, int kw, int sh, int sw, int ph, int pw, int64_t ld, dvt_stream_t stream);
/* Raw NCHW frames x[N, C, H, W] (custom_resnet.py:138: the stem reads the clip frames) -> NHWC matrix y[N*H*W, Cpad] with
 * the channels C .. Cpad-1 zero.  Cpad = 8: one 16-byte chunk per pixel (C <= 8).  Cpad = 4 (C <= 4, W even): one chunk per
 * pair of horizontally adjacent pixels, i.e. the [N, H, W/2, 8] view in which a stride-2 stem (custom_resnet.py:100,
 * frame_transformer.py:67) is a stride-(sh, 1) convolution over pixel pairs with the weights of dvt_conv_weight_pairs --
 * 28 instead of 49 gathered chunks per output pixel (7 rows x 4 pixel pairs) and half the zero padding of the C = 8 form. */
int dvt_nchw_to_nhwc_pad(const void* x, int x_dtype, void* y, int y_dtype, int64_t N, int C, int H, int W, int Cpad,
                         dvt_stream_t stream);
/* Stem weights for the pixel-pair view: w[Cout, Cin <= 4, kh, kw] f32 -> wp[Cout, 8, kh, kwp] f32 with
 * wp[co, px*4 + c, ki, p] = w[co, c, ki, 2p - (pw & 1) + px], zero outside the kernel / beyond Cin (pw = the horizontal
 * padding of the stride-2 convolution; the pair convolution has kernel (kh, kwp), stride (sh, 1), padding
 * (ph, (pw + (pw & 1)) / 2)).  _bwd: the adjoint gather of the weight gradient (+= when accumulate). */
int dvt_conv_weight_pairs(const float* w, float* wp, int Cout, int Cin, int kh, int kw, int pw, int kwp, dvt_stream_t stream);
int dvt_conv_weight_pairs_bwd(const float* dwp, float* dw, int Cout, int Cin, int kh, int kw, int pw, int kwp, int accumulate,
                              dvt_stream_t stream);
/* Adjoint gather (data gradient of the convolution), NHWC.  Optional second gradient path into the same map, summed in
 * the same pass (a residual block's shortcut joining its first convolution's data gradient, custom_resnet.py:38-54):
 * add [N*H*W, C] when add_stride == 0; else the COMPACT gradient [N*ceil(H/s)*ceil(W/s), C] of the map's stride-s
 * subsampling (the input of a strided 1x1 downsample convolution), added at the pixels with h % s == 0 and w % s == 0. */
int dvt_col2im(const void* dcol, void* dx, int64_t N, int C, int H, int W, int kh, int kw, int sh, int sw,
               int ph, int pw, int64_t ld, const void* add, int add_stride, int dtype, dvt_stream_t stream);
/* Same adjoint written in NCHW order and in the clip's own dtype: the gradient of the stem w.r.t. the raw
 * frames (needed by the learnable pixel-space CLS clip, frame_transformer.py:105,195). */
int dvt_col2im_nchw(const void* dcol, int dtype, void* dx, int dx_dtype, int64_t N, int C, int H, int W, int kh,
                    int kw, int sh, int sw, int ph, int pw, int64_t ld, dvt_stream_t stream);
/* Implicit-GEMM convolution: y[N*Ho*Wo, Cout] = sum_{ki,kj,c} x[n, ho*sh-ph+ki, wo*sw-pw+kj, c] * w[co, (ki*kw+kj)*C + c]
 * with the gather fused into the GEMM's A-operand LDS-DMA -- no column matrix in HBM (nn.Conv2d of
 * custom_resnet.py:19-22,128; the (1,3,3)/(3,1,1) convolutions of R(2+1)D).  x NHWC, w = dvt_conv_weight_pack(...,
 * ld = kh*kw*C).  The data gradient of a stride-1 convolution is the same call on dz with the 180-degree-rotated,
 * channel-transposed weights and padding k-1-p.  16-bit dtypes, C % 64 == 0 (C % 32 == 0 when Cout <= 128),
 * Cout % 8 == 0; dvt_conv2d_implicit_supported tells (callers fall back to dvt_im2col + dvt_gemm otherwise). */
/* Channel padding of f32 parameter arrays viewed as [A, B, K] (conv weights: A = Cout, B = Cin, K = kh*kw; BatchNorm
 * vectors: B = K = 1): dst[Ap, Bp, K] = src zero-extended; dvt_unpad3_f32 is the adjoint slice (+= when accumulate).
 * Lets layers whose channel counts are not multiples of 8 (R(2+1)D mid planes 45 / 230 / 460 / 921,
 * frame_transformer.py:67) run on the MFMA kernels with exactly-zero padded channels. */
int dvt_pad3_f32(const float* src, float* dst, int A, int B, int K, int Ap, int Bp, dvt_stream_t stream);
int dvt_unpad3_f32(const float* src, float* dst, int A, int B, int K, int Bp, int accumulate, dvt_stream_t stream);
/* w[Cout,Cin,kh,kw] f32 -> dst[Cin, (kh*kw)*Cout]: taps rotated by 180 degrees, channels transposed (the weight
 * operand of the data-gradient convolution, see dvt_conv2d_implicit). */
int dvt_conv_weight_pack_dgrad(const float* w, void* dst, int dst_dtype, int Cout, int Cin, int kh, int kw,
                               dvt_stream_t stream);
/* Both packed forms of many convolution weights in ONE launch -- the weights change once per optimizer step, so a training
 * step needs one such launch instead of two per layer -- with the zero extension of channel-padded layers (cout_p >= cout_l,
 * cin_p >= cin_l) folded in.  kind 0: dvt_conv_weight_pack's layout dst[cout_p][ld] (column (ki*kw+kj)*cin_p + ci, zeros
 * beyond); kind 1: dvt_conv_weight_pack_dgrad's dst[cin_p][kh*kw*cout_p] (rotated taps, transposed channels). */
typedef struct dvt_pack_entry {
  const float* src;      /* f32 [cout_l][cin_l][kh*kw] */
  void* dst;
  int32_t cout_l, cin_l, kh, kw, cout_p, cin_p, ld, kind, dtype;
  /* kind 2 (ABI v4): the data-gradient operand of ONE parity class of a strided convolution -- dst[cin_p][nth*ntw*cout_p]
   * holding only the taps ki = cls_rh + j * cls_sh (j < nth = ceil((kh - cls_rh) / cls_sh)), kj likewise, in DECREASING
   * ki / kj order (so that tap t of the class reads dz row hq + t - pad'), channels transposed as in kind 1.  The class of
   * input pixels hi % sh == a uses cls_rh = (a + ph) % sh. */
  int32_t cls_sh, cls_sw, cls_rh, cls_rw;
} dvt_pack_entry;
int dvt_conv_weight_pack_group(const dvt_pack_entry* entries, int count, dvt_stream_t stream);
typedef struct dvt_conv_desc {
  const void* x;
  const void* w;
  void* y;
  int64_t N;
  int32_t H, W, C, Cout, kh, kw, sh, sw, ph, pw;
  int32_t dtype;
  void* workspace;   /* weight gradient; forward / data gradient when dvt_conv2d_implicit_workspace_bytes(desc) > 0 */
  /* forward only, optional: the BatchNorm that follows the convolution (custom_resnet.py:30,33,104: conv -> bn) needs the
   * column sums and sums of squares of y; when stats_partial != NULL (>= dvt_conv2d_implicit_stats_bytes(desc)) the GEMM
   * epilogue leaves them here from its fp32 accumulators, per 128-row block: [parts][2][Cout] f32 with
   * parts = dvt_conv2d_implicit_stats_parts(desc); dvt_bn_stats_from_partials turns them into mean / invstd.  Saves the
   * separate statistics pass over y. */
  float* stats_partial;
  /* output columns dropped at the right edge: Wo = (W + 2*pw - kw)/sw + 1 - trim_w (0: the usual convolution).  The
   * pixel-pair stem (dvt_conv_weight_pairs) pads two pair columns on the left and needs only one on the right. */
  int32_t trim_w;
  /* Optional, like the same three fields of the GEMM descriptor: the weight gradient (dvt_conv2d_implicit_wgrad) leaves its split-K
   * reduce undone when defer_reduce != 0 and describes it in *pending; the data gradient of the same layer
   * (dvt_conv2d_implicit on dz with the rotated weights) performs a pending reduce handed to it as `carry` in extra
   * workgroups at the end of its grid.  The weight-gradient scatter (dvt_conv_weight_unpack_grad_t) goes behind the carrier. */
  int32_t defer_reduce;
  dvt_splitk_pending* pending;
  const dvt_splitk_pending* carry;
  /* forward / data gradient, optional: y = conv(x) + residual, residual [N*Ho*Wo, Cout] in the map's dtype, added on the fp32
   * accumulators (the shortcut's gradient joining a block input's gradient, custom_resnet.py:38-54: no add kernel). */
  const void* residual;
  /* weight gradient, optional: y is the parameter's own gradient f32 [Cout][C][kh][kw] (+= when wgrad_accumulate) instead
   * of the packed dWt -- the split-K reduce scatters into it (dvt_splitk_pending.conv_taps). */
  int32_t wgrad_master_layout, wgrad_accumulate;
  int32_t wgrad_cout_l, wgrad_cin_l;   /* channel-padded layers: the parameter's own channel counts (0: Cout / C) */
  /* forward / data gradient, optional (ABI v4).  The data gradient of a STRIDED convolution (custom_resnet.py:19-22 with
   * stride 2, the 1 x 1 / 2 downsample of :124-130; R(2+1)D's strided halves) as implicit launches: the input pixels
   * (hi, wi) fall into sh x sw parity classes (hi % sh, wi % sw), and the gradient of one class is a stride-1 convolution of
   * dz with the class's taps (1 / 2 / 2 / 4 of a 3 x 3 / 2 filter: dvt_pack_entry kind 2), whose output rows are SCATTERED
   * into the full-size gradient.  out_h / out_w (> 0): the launch computes out_h x out_w output pixels per image instead of
   * the usual (H + 2 ph - kh) / sh + 1 (taps that fall outside the map read zeros, as padding does).  out_rows (int32
   * [N * out_h * out_w]): row m of the launch is row out_rows[m] of y (and of `residual`, unless residual_compact: then
   * residual row m joins -- the compact gradient of a strided 1 x 1 shortcut, which touches one class only).  No column
   * matrix, no col2im pass. */
  int32_t out_h, out_w;
  const int32_t* out_rows;
  int32_t residual_compact;
} dvt_conv_desc;
/* 3x3 / stride 1 / pad 1 convolution with 64 input and 64 output channels (layer 1 of ResNet-18, custom_resnet.py:19-22,
 * 109; also its data gradient, with the rotated weights of dvt_conv_weight_pack_dgrad) from an LDS-resident halo patch: a
 * workgroup stages the (R + 2) x (W + 2) input patch of R whole output rows once and the nine taps read it from LDS, the
 * 64 x 576 weights stay resident (the implicit GEMM gathers every input element nine times from L2).  x, y NHWC
 * [N*H*W, 64], w [64][576] (dvt_conv_weight_pack, ld = 576).  stats_partial (optional): [dvt_conv3x3_c64_stats_parts + 64]
 * [2][64] f32 partial column sums for dvt_bn_stats_from_partials.  _supported: 16-bit dtype and W <= 56-ish (two patches
 * must fit beside the weights in 160 KiB); callers fall back to dvt_conv2d_implicit otherwise. */
int dvt_conv3x3_c64_supported(int64_t N, int H, int W, int dtype);
/* Weight gradient of the same layer from LDS-resident halo patches: a workgroup of the persistent grid stages the input
 * patch and the gradient tile of R output rows once each (the implicit form gathers the input nine times), accumulates
 * [co 64][tap * 64 + ci] over its tile sequence in registers and leaves ONE fp32 partial per workgroup in `workspace`
 * (dvt_conv3x3_c64_wgrad_workspace_bytes); the split-K reduce of the family sums the partials into the parameter's own
 * layout dw f32 [64][64][3][3] (+= when accumulate) -- right away, or (defer_reduce) described in *pending for a later
 * dvt_splitk_reduce_pending / a carrying launch.  x, dz NHWC [N*H*W, 64]. */
int dvt_conv3x3_c64_wgrad_supported(int64_t N, int H, int W, int dtype);
size_t dvt_conv3x3_c64_wgrad_workspace_bytes(int64_t N, int H, int W);
int dvt_conv3x3_c64_wgrad(const void* x, const void* dz, float* dw, void* workspace, int64_t N, int H, int W, int accumulate,
                          int defer_reduce, dvt_splitk_pending* pending, int dtype, dvt_stream_t stream);
/* The same with Cout output channels (>= 64 in steps of 16: the 64 -> 144 spatial half of R(2+1)D-18's layer-1 Conv2Plus1D,
 * video_resnet.py:25): the kernel runs once per group of dz channels -- groups of 64, the last one up to 80 wide (144 = 64 +
 * 80: a 16-channel launch of its own would re-stage every input patch for a ninth of the work) --, each group's partials
 * summed into its rows of dw f32 [Cout][64][3][3] before the next launch reuses the workspace (the size
 * dvt_conv3x3_c64_wgrad_workspace_bytes reports covers the widest group); defer_reduce defers the LAST group's reduce. */
int dvt_conv3x3_c64_wgrad_wide(const void* x, const void* dz, float* dw, void* workspace, int64_t N, int H, int W, int Cout,
                               int accumulate, int defer_reduce, dvt_splitk_pending* pending, int dtype, dvt_stream_t stream);
/* The launches of dvt_conv3x3_c64_wgrad (Cout = 64) / _wide (host only): launch i takes the dz channels [c0[i], c0[i] + width[i])
 * on conv3x3_c64_wgrad_kernel<., mb[i]> (mb = 5: an 80-wide last group, 4: up to 64 channels, 1: a 16-channel tail) in tiles
 * of rows[i] whole output rows of a frame.  Returns the number of launches -- the first max_launches are written --, 0 where
 * the call is refused. */
int dvt_conv3x3_c64_wgrad_plan(int64_t N, int H, int W, int Cout, int dtype, int max_launches, int* c0, int* width, int* mb,
                               int* rows);
/* The temporal half of R(2+1)D-18's layer-1 Conv2Plus1D (torchvision r2plus1d_18 as used by frame_transformer.py:64-74: a
 * (3, 1, 1) convolution, 144 mid planes -> 64, stride 1, pad 1) from LDS-resident sliding windows: a workgroup stages a
 * segment of S pixels of one clip over all T + 2 frames once and the three taps read it at three position offsets.
 * x [N, T, L, 144] (L = H * W pixels per frame), w [64][ldw] (dvt_conv_weight_pack, column kt * 144 + ci), y / dz
 * [N, T, L, 64], dw f32 [64][144][3] (the Conv3d parameter's own layout; += when accumulate).
 * x_affine (optional, both entry points): x is the OUTPUT z of the spatial convolution in front and the BatchNorm (+ ReLU)
 * between the two halves -- y = relu(z * invstd * gamma + (beta - mean * invstd * gamma)), the formula and rounding of
 * dvt_bn_apply_fwd -- is applied to the staged window: the normalised 144-plane activation never exists in HBM.
 * stats_partial (forward): [dvt_conv3x1_fwd_stats_parts + 64][2][64] f32 partial column sums of the stored output for
 * dvt_bn_stats_from_partials.  workspace / defer_reduce / pending (weight gradient) as dvt_conv3x3_c64_wgrad.
 * The forward also takes Cin = 64 (since ABI v5): the temporal half of the STEM, Conv3d(45, 64, (3, 1, 1)) with its 45 mid
 * planes stored zero-padded to 64 -- x [N, T, L, 64], w [64][ldw] with column kt * 64 + ci, no x_affine -- and, given the
 * data-gradient pack of the weights (dvt_conv_weight_pack_dgrad), that layer's data gradient. */
typedef struct dvt_bn_affine {
  const float* mean;     /* [C] */
  const float* invstd;   /* [C] */
  const float* gamma;    /* [c_valid] */
  const float* beta;     /* [c_valid] */
  int32_t c_valid;       /* channels gamma / beta have (0: all) */
  int32_t relu;
} dvt_bn_affine;
int dvt_conv3x1_fwd_supported(int64_t N, int T, int L, int Cin, int Cout, int dtype);
int64_t dvt_conv3x1_fwd_stats_parts(int64_t N, int T, int L, int Cin);
/* Which kernel dvt_conv3x1_fwd launches for the 144 -> 64 form (host only, no HIP call): *npb = 16-position blocks per wave
 * (1 .. 6, the template parameter of conv3x1_fwd_kernel / conv3x1_fwd_pipe_kernel), *pipelined = 1 for the form with helper
 * waves.  Returns 1, or 0 (both outputs 0) where dvt_conv3x1_fwd_supported refuses the geometry or Cin != 144 (since ABI v5). */
int dvt_conv3x1_fwd_plan(int64_t N, int T, int L, int Cin, int Cout, int dtype, int* npb, int* pipelined);
/* The same for the 64 -> 64 form (conv3x1_c64_kernel): *npb = 16-position blocks per wave (1 .. 6).  Returns 1, or 0 (*npb 0)
 * where the geometry is not taken. */
int dvt_conv3x1_c64_plan(int64_t N, int T, int L, int dtype, int* npb);
int dvt_conv3x1_fwd(const void* x, const dvt_bn_affine* x_affine, const void* w, int64_t ldw, void* y, float* stats_partial,
                    int64_t N, int T, int L, int Cin, int dtype, dvt_stream_t stream);
int dvt_conv3x1_wgrad_supported(int64_t N, int T, int L, int Cin, int Cout, int dtype);
/* Which kernel dvt_conv3x1_wgrad launches (host only): *pipelined = 1 for conv3x1_wgrad_pipe_kernel (three buffer pairs, helper
 * waves), 0 for conv3x1_wgrad_kernel.  Returns 1, or 0 where dvt_conv3x1_wgrad_supported refuses the geometry. */
int dvt_conv3x1_wgrad_plan(int64_t N, int T, int L, int Cin, int Cout, int dtype, int* pipelined);
size_t dvt_conv3x1_wgrad_workspace_bytes(int64_t N, int T, int L);
int dvt_conv3x1_wgrad(const void* x, const dvt_bn_affine* x_affine, const void* dz, float* dw, void* workspace, int64_t N, int T,
                      int L, int accumulate, int defer_reduce, dvt_splitk_pending* pending, int dtype, dvt_stream_t stream);
/* The 7x7 / stride 2 / pad 3 stem on 3-channel frames, 64 output channels (reference custom_resnet.py:100 `conv1`; the
 * (1, 7, 7) spatial half of torchvision's R(2+1)D stem behind frame_transformer.py:64-74, its 45 planes zero-extended to 64),
 * from an LDS halo patch with the weights in registers.  x_pairs: the pixel-pair map [N, H, Wp = W / 2, 8] of
 * dvt_nchw_to_nhwc_pad(.., 4); w: [64][ldw] with column (ki * 4 + kj) * 8 + c8 (dvt_conv_weight_pairs + dvt_conv_weight_pack,
 * ldw >= 224); y: [N * (H / 2) * Wp, 64] -- the same result as dvt_conv2d_implicit with the pair geometry (kernel (7, 4),
 * stride (2, 1), pad (3, 2), trim_w 1).  stats_partial: [dvt_conv_stem7_stats_parts + 64][2][64] or NULL. */
int dvt_conv_stem7_supported(int64_t N, int H, int Wp, int dtype);
int64_t dvt_conv_stem7_stats_parts(int64_t N, int H, int Wp);
int dvt_conv_stem7(const void* x_pairs, const void* w, int64_t ldw, void* y, float* stats_partial, int64_t N, int H, int Wp,
                   int dtype, dvt_stream_t stream);
int64_t dvt_conv3x3_c64_stats_parts(int64_t N, int H, int W);
int dvt_conv3x3_c64(const void* x, const void* w, void* y, float* stats_partial, const void* residual, int64_t N, int H, int W,
                    int dtype, dvt_stream_t stream);   /* residual (optional): added to the output rows, like dvt_conv_desc.residual */
/* The same convolution where one side has 144 channels -- the spatial half of R(2+1)D-18's layer-1 Conv2Plus1D
 * (video_resnet.py: 64 -> 144 mid planes forward, 144 -> 64 as the data gradient with the rotated weights): the weights
 * (162 KiB) cannot stay in LDS, so they stream through a ring of 18 KiB stages issued by a producer wave while seven
 * compute waves run the taps of the staged patch (per 48-channel chunk at 144 input channels).  (Cin, Cout) = (64, 144)
 * or (144, 64) -- and (128, 288) / (288, 128), the same pair in layer 2, as one launch per 144- / 64-wide group of output
 * channels; x [N*H*W, Cin], w [Cout][9 * Cin] (k = tap * Cin + c), y [N*H*W, Cout].  stats_partial: only with
 * Cout = 144 / 288, [dvt_conv3x3_stream_stats_parts + 64][2][Cout]; residual: only with Cout = 64 / 128. */
int dvt_conv3x3_stream_supported(int64_t N, int H, int W, int Cin, int Cout, int dtype);
int64_t dvt_conv3x3_stream_stats_parts(int64_t N, int H, int W, int Cin, int Cout);
/* Which instantiation dvt_conv3x3_stream launches (host only): conv3x3_stream_kernel<., *ci, *co, 9, 0>, once per group of
 * *co output channels (*groups launches: 2 for the layer-2 pairs).  Returns 1, or 0 (all outputs 0) where
 * dvt_conv3x3_stream_supported refuses the call. */
int dvt_conv3x3_stream_plan(int64_t N, int H, int W, int Cin, int Cout, int dtype, int* ci, int* co, int* groups);
int dvt_conv3x3_stream(const void* x, const void* w, void* y, float* stats_partial, const void* residual, int64_t N, int H, int W,
                       int Cin, int Cout, int dtype, dvt_stream_t stream);
/* The (3, 1) sibling over the [T, L] view of N clips (L = H * W pixels per frame; rows of the "image" are L pixels apart): the
 * temporal half of the same Conv2Plus1D as its data gradient, 64 -> 144 channels, stride 1, pad (1, 0).  x [N*T*L, 64],
 * w [144][3 * 64], y [N*T*L, 144].  A tile is R frames of one column segment (a divisor of L); three weight stages per tile. */
int dvt_conv3x1_stream_supported(int64_t N, int T, int L, int Cin, int Cout, int dtype);
int dvt_conv3x1_stream(const void* x, const void* w, void* y, int64_t N, int T, int L, int Cin, int Cout, int dtype,
                       dvt_stream_t stream);
/* The same data gradient with the backward of the BatchNorm (+ ReLU) in FRONT of the temporal half fused in (the mid-plane
 * BatchNorm of Conv2Plus1D, video_resnet.py:30-31 of torchvision's layout; reference frame_transformer.py:64-74): dy [N*T*L, 64]
 * is the temporal convolution's output gradient, z [N*T*L, 144] the spatial half's output that `bn` normalised, dz [N*T*L, 144]
 * receives gamma * invstd * (d - sum d / rows - xhat * sum d xhat / rows) with d = (dy (*) w) under the ReLU mask recomputed
 * from z (training == 0: gamma * invstd * d); dgamma / dbeta [144] overwritten or accumulated.  The data gradient itself is
 * never stored: it is computed twice (sums, then the corrected gradient), which replaces a write and two reads of a
 * 144-plane map by one read of the 64-plane dy.  Same geometry as dvt_conv3x1_stream (dvt_conv3x1_stream_supported). */
size_t dvt_conv3x1_stream_bn_bwd_workspace_bytes(int64_t N, int T, int L);
int dvt_conv3x1_stream_bn_bwd(const void* dy, const void* w, const void* z, const dvt_bn_affine* bn, void* dz, float* dgamma,
                              float* dbeta, void* workspace, int64_t N, int T, int L, int training, int accumulate, int dtype,
                              dvt_stream_t stream);
/* Which kernel pair takes dvt_conv3x1_stream_bn_bwd (host only): the window kernel with helper waves
 * conv3x1_dbn_kernel<., *nb, 1 | 2> where it takes the geometry (*nb = 16-position blocks per tile: 2, 4 or 6), else the
 * streamed-weight kernel conv3x3_stream_kernel<., 64, 144, 3, 1 | 2> (*nb = 0).  Returns 1, or 0 (kernel NONE) where
 * dvt_conv3x1_stream_supported refuses the geometry. */
enum dvt_conv3x1_bn_bwd_kernel {
  DVT_CONV3X1_BN_BWD_NONE = 0,
  DVT_CONV3X1_BN_BWD_WINDOW = 1,
  DVT_CONV3X1_BN_BWD_STREAM = 2
};
int dvt_conv3x1_stream_bn_bwd_plan(int64_t N, int T, int L, int dtype, int* kernel, int* nb);
int dvt_conv2d_implicit_supported(const dvt_conv_desc* desc);
/* Row length K of the packed weights w[Cout][K] the forward call expects: kh*kw*C -- rounded up to the kernel's k-tile in
 * the stem form C == 8 (the columns past kh*kw*8 must be zero: dvt_conv_weight_pack with ld = K writes them so). */
int64_t dvt_conv2d_implicit_k(const dvt_conv_desc* desc);
/* Scratch a forward / data-gradient launch of this descriptor needs (0 for most shapes): launches with few output rows and a
 * deep reduction (R(2+1)D layers 3 - 4) split K over workgroups into fp32 slabs in desc->workspace and sum them in a second
 * launch that also rounds, adds `residual` and leaves the BatchNorm partial sums (same contract as the one-launch form). */
size_t dvt_conv2d_implicit_workspace_bytes(const dvt_conv_desc* desc);
int dvt_conv2d_implicit(const dvt_conv_desc* desc, dvt_stream_t stream);
int64_t dvt_conv2d_implicit_stats_parts(const dvt_conv_desc* desc);
size_t dvt_conv2d_implicit_stats_bytes(const dvt_conv_desc* desc);
/* Weight gradient without a column matrix: with x = the layer input (NHWC), w = dz [N*Ho*Wo, Cout] and
 * y = dWt f32 [kh*kw*C, Cout] (overwritten): dWt[(ki*kw+kj)*C + c, co] = sum_rows gather(x)[row, .] * dz[row, co];
 * split-K over the rows with a fixed-order reduction (reproducible).  C % 8 == 0, Cout % 8 == 0, any number of output
 * pixels (rows past the end of the last k-tile are read as zeros).  dvt_conv_weight_unpack_grad_t scatters dWt into the
 * [Cout, Cin, kh, kw] master; or see wgrad_master_layout below. */
int dvt_conv2d_implicit_wgrad_supported(const dvt_conv_desc* desc);
size_t dvt_conv2d_implicit_wgrad_workspace_bytes(const dvt_conv_desc* desc);
int dvt_conv2d_implicit_wgrad(const dvt_conv_desc* desc, dvt_stream_t stream);
/* What dvt_conv2d_implicit (wgrad == 0) or dvt_conv2d_implicit_wgrad (wgrad != 0) would launch for desc, taken from the
 * same decisions the launchers make (ABI v5 addition; host only, runs without a device: the CU-count dependent thresholds
 * then assume the MI355X's 256).  The operand pointers x / w / y are not looked at; every other field counts -- a split
 * launch without desc->workspace is refused as the launcher refuses it, and `carry` reports what becomes of a valid
 * desc->carry.  Returns what the launcher returns for a descriptor it refuses, else DVT_OK. */
enum dvt_conv_reduce {             /* the kernel that sums split-K slabs, as a launch of its own */
  DVT_CONV_R_NONE = 0,             /* forward / data gradient in one slice: no slabs */
  DVT_CONV_R_SPLIT = 1,            /* conv_split_reduce_kernel (forward: rounds, adds `residual`, leaves the BatchNorm partials) */
  DVT_CONV_R_PLAIN = 2,            /* splitk_reduce_kernel<float> (the packed dWt) */
  DVT_CONV_R_WIDE = 3,             /* splitk_reduce_wide_kernel (>= 64 slices, at most 2^20 entries) */
  DVT_CONV_R_SCATTER = 4,          /* splitk_reduce_pending_kernel scattering into the parameter's layout */
  DVT_CONV_R_SCATTER_TILED = 5     /* splitk_reduce_conv_tiled_kernel (the same through LDS tiles: 2^20 entries and more) */
};
enum dvt_conv_carry {              /* what becomes of a valid desc->carry */
  DVT_CONV_CARRY_NONE = 0,
  DVT_CONV_CARRY_TAIL = 1,         /* rides in the grid tail of the one-slice launch */
  DVT_CONV_CARRY_ALONE = 2         /* launched on its own first (a split launch carries nothing): carry_reduce tells the kernel */
};
typedef struct dvt_conv_plan_info {
  int32_t cfg;            /* LDS-DMA configuration of the gemm_dma_kernel<..., true> launch */
  int32_t split;          /* slices of the reduction (blockIdx.z); 1: none */
  int32_t k_per_split;    /* reduction length per slice: channels x taps (forward), output pixels (weight gradient) */
  int32_t epilogue;       /* DVT_EPI_NONE or DVT_EPI_RESIDUAL of that launch (NONE where the reduce adds the residual) */
  int32_t out_form;       /* 0 = the map in desc->dtype, 2 = fp32 split-K slabs */
  int32_t reduce;         /* enum dvt_conv_reduce */
  int32_t deferred;       /* 1: the reduce is left undone in *desc->pending (`reduce`: what dvt_splitk_reduce_pending would run) */
  int32_t carry;          /* enum dvt_conv_carry */
  int32_t carry_reduce;   /* CARRY_ALONE: enum dvt_conv_reduce of the carried reduce's own launch; else NONE */
} dvt_conv_plan_info;
int dvt_conv2d_implicit_plan(const dvt_conv_desc* desc, int wgrad, dvt_conv_plan_info* info);
int dvt_conv_weight_unpack_grad_t(const float* gt, float* dw, int Cout, int Cin, int kh, int kw, int accumulate,
                                  dvt_stream_t stream);
/* w[Cout,Cin,kh,kw] f32 -> dst[Cout, ld] (column order (ki,kj,ci), zero padded) in dst_dtype, and the
 * inverse for the fp32 weight gradient (dw (+)= g re-ordered). */
int dvt_conv_weight_pack(const float* w, void* dst, int dst_dtype, int Cout, int Cin, int kh, int kw, int64_t ld,
                         dvt_stream_t stream);
int dvt_conv_weight_unpack_grad(const float* g, float* dw, int Cout, int Cin, int kh, int kw, int64_t ld,
                                int accumulate, dvt_stream_t stream);
/* nn.BatchNorm2d over the rows of x[rows, C] (custom_resnet.py:30,33,104).  Training: batch mean and
 * biased variance -> mean / invstd, running statistics updated with `momentum` (unbiased variance),
 * as torch does.  Eval: dvt_bn_eval_invstd from running_var.  workspace >= dvt_bn_workspace_bytes. */
size_t dvt_bn_workspace_bytes(int64_t rows, int C);
/* c_valid (every BatchNorm entry that takes it): the channels the parameter-side arrays really have -- gamma, beta, the
 * running statistics, dgamma, dbeta are [c_valid]; mean / invstd and the maps are [C] wide, C >= c_valid.  The layers of
 * R(2+1)D whose plane counts (45, 230, 460, 921) are zero-extended to multiples of 64 run at the padded width without
 * padded copies of their BatchNorm vectors: channels >= c_valid behave as gamma = beta = 0.  c_valid <= 0 means C. */
int dvt_bn_stats(const void* x, float* mean, float* invstd, float* running_mean, float* running_var,
                 void* workspace, int64_t rows, int C, int c_valid, float eps, float momentum, int dtype, dvt_stream_t stream);
/* Same result from the per-block partial sums a convolution left behind (dvt_conv_desc.stats_partial, a buffer of
 * dvt_conv2d_implicit_stats_bytes = parts + 64 rows of 2 * C floats: with more than 256 partial rows the call WRITES
 * the 64-row tail -- it folds the partial rows into it before the final sum, hence the non-const pointer). */
int dvt_bn_stats_from_partials(float* partial, int64_t parts, float* mean, float* invstd, float* running_mean,
                               float* running_var, int64_t rows, int C, int c_valid, float eps, float momentum,
                               dvt_stream_t stream);
int dvt_bn_eval_invstd(const float* running_var, float* invstd, int C, float eps, dvt_stream_t stream);
/* y = relu?((x-mean)*invstd*gamma + beta (+ residual)): `out += residual; relu` fused (custom_resnet.py:51-52).
 * relu_mask (optional, C % 8 == 0): uint8 [rows][C/8], bit k of byte (r, g) = y[r, 8g + k] > 0 -- the ReLU mask the backward
 * of a layer WITH a residual branch needs (its output cannot be recomputed from x alone); dvt_bn_bwd reads these bytes
 * (1/16 of the traffic) instead of the output y in both of its passes. */
int dvt_bn_apply_fwd(const void* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                     const void* residual, void* y, void* relu_mask, int64_t rows, int C, int c_valid, int relu, int dtype,
                     dvt_stream_t stream);
/* dz = dy*(relu mask); dres = dz (if dres != NULL); dgamma/dbeta (+)=; dx by the batch-statistics formula (training) or
 * gamma*invstd*dz (eval).  The ReLU mask comes from relu_mask (dvt_bn_apply_fwd's bytes) when given, else from the
 * forward output y, else -- a ReLU layer without a residual branch -- it is recomputed from x as
 * (x - mean)*invstd*gamma + beta > 0 (beta required). */
int dvt_bn_bwd(const void* dy, const void* x, const void* y, const void* relu_mask, const float* mean, const float* invstd,
               const float* gamma, const float* beta, void* dx, void* dres, float* dgamma, float* dbeta, void* workspace,
               int64_t rows, int C, int c_valid, int relu, int training, int accumulate, int dtype, dvt_stream_t stream);
/* The ResNet stem's bn1 -> relu -> maxpool(3, 2, 1) (custom_resnet.py:100-105,138-142) without the normalised map in HBM:
 * _fwd reads the convolution output z once and writes the pooled map y[N*Ho*Wo, C] and the argmax taps idx (same values
 * and taps as dvt_bn_apply_fwd followed by dvt_maxpool_fwd); dvt_bn_bwd_pooled is dvt_bn_bwd whose incoming gradient
 * is gathered from the pooled gradient dy_pool and idx on the fly (the ReLU mask is recomputed from z), so neither the
 * max-pool's input gradient nor the BatchNorm output exist as tensors.  C % 8 == 0. */
int dvt_bn_relu_maxpool_fwd(const void* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                            void* y, void* idx, int64_t N, int C, int H, int W, int relu, int dtype, dvt_stream_t stream);
int dvt_bn_bwd_pooled(const void* dy_pool, const void* idx, const void* x, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, void* dx, float* dgamma, float* dbeta, void* workspace, int64_t N,
                      int C, int H, int W, int relu, int training, int accumulate, int dtype, dvt_stream_t stream);
/* nn.MaxPool2d(k, stride, pad) on NHWC; idx: uint8 [N*Ho*Wo*C] window position of the (first) maximum. */
int dvt_maxpool_fwd(const void* x, void* y, void* idx, int64_t N, int C, int H, int W, int k, int stride, int pad,
                    int dtype, dvt_stream_t stream);
int dvt_maxpool_bwd(const void* dy, const void* idx, void* dx, int64_t N, int C, int H, int W, int k, int stride,
                    int pad, int dtype, dvt_stream_t stream);
/* [B, R, C] -> [B, C, R]  (NHWC <-> NCHW at the module boundary). */
int dvt_transpose_last2(const void* src, void* dst, int64_t B, int R, int Cc, int dtype, dvt_stream_t stream);

/* ---------------------------------------------------------------- losses
 * nn.BCEWithLogitsLoss() (mean): src/models/frame_transformer.py:89,263,268,273.
 * z: [n] dtype, target: [n] f32, loss: [1] f32. */
int dvt_bce_logits_fwd(const void* z, const float* target, float* loss, int64_t n, int dtype,
                       dvt_stream_t stream);
/* dz = gscale * (sigmoid(z) - target) / n */
int dvt_bce_logits_bwd(const void* z, const float* target, const float* gloss, void* dz,
                       int64_t n, int dtype, dvt_stream_t stream);
/* The classification head and its loss in ONE launch (vit.py:97-100 mlp_head = LayerNorm + Linear on the pooled CLS row,
 * :126-128; behind the temporal Transformer's final LayerNorm of :43, which commutes with the CLS pooling; the caller's
 * nn.BCEWithLogitsLoss() mean):  h1 = LN(x; g1, b1) (skipped when g1 == NULL), h2 = LN(h1; g2, b2), z = h2 W^T + c,
 * loss = mean BCE(z, target) -- eight rows at the metric shape, where the five launches this replaces (and the six of
 * their backward) cost ~5 us each and compute nothing to speak of.  All arithmetic fp32 on the fp32 parameters.
 * The same launch leaves d(loss)/d(everything) for an upstream gradient of 1 in `grads` (f32, dvt_head_bce_grads_elems
 * elements: [dx rows*d][dg1 d][db1 d][dg2 d][db2 d][dW classes*d][dc classes], then scratch); the backward pass is then
 * dvt_scaled_emit_group: scale by the incoming gradient of the loss and store / accumulate into the gradient buffers.
 * Limits: rows <= 32, d / 64 in {1, 2, 3, 4, 6, 8, 12, 16}, classes <= 64, classes * d <= 12288 (dvt_head_bce_supported). */
typedef struct dvt_head_bce_desc {
  const void* x;          /* [rows, d] f32 or 16-bit (x_dtype) */
  const float* g1;        /* first LayerNorm (NULL: none) */
  const float* b1;
  const float* g2;        /* second LayerNorm */
  const float* b2;
  const float* w;         /* [classes, d] */
  const float* c;         /* [classes] or NULL */
  const float* target;    /* [rows, classes] */
  float* logits;          /* [rows, classes] out */
  float* loss;            /* [1] out */
  float* grads;           /* out, see above */
  int32_t rows, d, classes, x_dtype;
  float eps1, eps2;
} dvt_head_bce_desc;
int dvt_head_bce_supported(int rows, int d, int classes);
int64_t dvt_head_bce_grads_elems(int rows, int d, int classes);
int dvt_head_bce_fwd(const dvt_head_bce_desc* desc, dvt_stream_t stream);
/* dst[i] = scale[0] * src[i] (+ dst[i] when accumulate), optionally also a 16-bit copy of the RESULT (dst_lp); dst may be
 * NULL when only the copy is wanted.  Up to 16 entries per launch; scale is a device scalar. */
typedef struct dvt_emit_entry {
  const float* src;
  float* dst;
  void* dst_lp;
  int64_t n;
  int32_t accumulate, lp_dtype;
} dvt_emit_entry;
int dvt_scaled_emit_group(const float* scale, const dvt_emit_entry* entries, int count, dvt_stream_t stream);
/* Hard-label distillation CE(student, argmax(teacher)), mean over rows:
 * src/models/frame_transformer.py:90,250.  student/teacher: [rows, C]. */
int dvt_ce_argmax_fwd(const void* student, const void* teacher, float* loss, int64_t rows,
                      int64_t C, int dtype, dvt_stream_t stream);
int dvt_ce_argmax_bwd(const void* student, const void* teacher, const float* gloss, void* dstudent,
                      int64_t rows, int64_t C, int dtype, dvt_stream_t stream);

/* ---------------------------------------------------------------- optimizer
 * torch.optim.AdamW step over a flat fp32 buffer (frame_transformer.py:127-129). */
int dvt_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                   dvt_stream_t stream);
/* Same update with the step counter in device memory (*step_dev is the number of steps
 * already taken; it is incremented by the call), so that the launch can be captured in
 * a hipGraph and replayed.
 * skip64 (nullable; here and in the three flat-buffer forms below): one byte per 64-element block of the flat
 * buffer; blocks whose byte is non-zero are left untouched -- parameter, moments and all.  torch's optimizers skip
 * parameters whose .grad is None (frame_transformer.py:123-134 hands every parameter to the optimizer, and the frozen
 * image encoder :59 / unused members never get a gradient): without the mask a flat-buffer step would still weight-
 * decay them.
 * The bias correction uses the ONE step counter of the flat buffer, where torch keeps a counter per parameter: the two
 * agree when the set of masked (gradient-less) parameters is the same in every step of a run -- a frozen encoder, an
 * unused member --, which is what the path's models do; a parameter that receives a gradient only in some steps would
 * see a larger step number here than under torch.optim.AdamW (same for dvt_adagrad_step's decayed learning rate). */
int dvt_adamw_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                       float lr, float beta1, float beta2, float eps, float weight_decay,
                       int64_t* step_dev, const uint8_t* skip64, dvt_stream_t stream);
/* The whole flat-buffer optimizer step of the training loop in one launch: the dvt_adamw_step_dev update, the 16-bit
 * mirror of the updated weights that the next step's GEMMs read (mirror nullable; mirror_dtype DVT_BF16 / DVT_F16) and
 * the step counter.  step_dev2: int64[2] = {steps already taken, 0}: element 1 is a ticket the launch uses to let its
 * last workgroup store the increment (it is 0 again when the launch has finished). */
int dvt_adamw_step_fused(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int64_t* step_dev2,
                         const uint8_t* skip64, void* mirror, int mirror_dtype, dvt_stream_t stream);
/* AdamW under dynamic loss scaling (BASELINE configs[4]: fp16 + loss scaling; torch.cuda.amp.GradScaler rule).
 * grad holds the gradient of (scale * loss).  On the device, in stream order: found_inf |= any non-finite grad;
 * unless found_inf: the dvt_adamw_step_dev update with grad / scale and step_dev += 1; then
 * found_inf ? scale *= backoff : (every growth_interval clean steps: scale *= growth); found_inf = 0;
 * loss_grad[0] = scale * loss_grad_base (the seed of the next backward, e.g. base = 1 / world).  No host sync.
 * n == 0: the four tensors may be NULL; the scaler state alone moves, as after a clean step. */
int dvt_adamw_step_scaled(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int64_t* step_dev, float* scale,
                          int32_t* found_inf, int32_t* good_steps, int growth_interval, float growth, float backoff,
                          float* loss_grad, float loss_grad_base, const uint8_t* skip64, dvt_stream_t stream);
/* torch.optim.SGD(lr, momentum, weight_decay) (frame_transformer.py:124-126; config.yaml momentum 0.005):
 * d = g + wd*p; buf = momentum*buf + d; p -= lr*buf.  momentum_buf starts zeroed (may be NULL when momentum == 0). */
int dvt_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                 float weight_decay, const uint8_t* skip64, dvt_stream_t stream);
/* torch.optim.Adagrad(lr, weight_decay) (frame_transformer.py:130-132): d = g + wd*p; sum += d*d;
 * p -= lr/(1+(step-1)*lr_decay) * d / (sqrt(sum) + eps); step counts from 1. */
int dvt_adagrad_step(float* param, const float* grad, float* state_sum, int64_t n, float lr, float lr_decay,
                     float eps, float weight_decay, int64_t step, const uint8_t* skip64, dvt_stream_t stream);

/* ---------------------------------------------------------------- LSTM (the LSTMRegressor baseline)
 * Additions within ABI v5: new entry points only, no existing layout or meaning changed.
 * The recurrent chain of one nn.LSTM(batch_first=True) layer over a whole sequence (src/models/LSTM.py:32-38 builds it,
 * :40-45 runs it), gate order i, f, g, o; h0 = c0 = 0.  The input projection G = x W_ih^T [B, T, 4H] (dtype, no bias)
 * is computed before the call and the parameter / input gradients after the backward call, on the GEMM entry points;
 * only h_{t-1} W_hh^T and the cell update are in the chain, one launch per step on `stream`.  Gates, c and dc are f32
 * in every dtype; h and the gate gradients are dtype.  No atomics: two identical calls give bitwise-equal results.
 * Limits: H a multiple of 16 (else DVT_ERR_UNSUPPORTED); dtype F32, BF16 or F16.
 *
 * Forward.  b_ih, b_hh [4H] f32 (either may be NULL); w_hh [4H, H] dtype.  Outputs: h_out [B, T, H] = h_t;
 * h_prev [B, T, H] = h_{t-1} (zeros at t = 0: the operand of dW_hh = dG^T h_prev, and the chain's own input);
 * gates [B, T, 4H] f32 = sigmoid(i), sigmoid(f), tanh(g), sigmoid(o); c [B, T, H] f32 = c_t; h_last [B, H] = h_{T-1}
 * (NULL: not written). */
int dvt_lstm_seq_fwd(const void* G, const float* b_ih, const float* b_hh, const void* w_hh, void* h_prev, void* h_out,
                     float* gates, float* c, void* h_last, int64_t B, int64_t T, int64_t H, int dtype, dvt_stream_t stream);
/* Backward through time (LSTM.py:32-38).  gates, c: the forward's outputs.  The gradient arriving at h_t is
 * dh_seq[:, t] (dtype [B, T, H], NULL: none) plus, at t = T-1, dh_last (dtype [B, H], NULL: none); at least one is given.
 * Output dG [B, T, 4H] dtype: the gradient of the pre-activation gates (= of G, of b_ih and of b_hh per row), from which
 * dW_ih = dG^T x, dW_hh = dG^T h_prev, db = colsum(dG) and dx = dG W_ih are ordinary GEMMs.
 * workspace: dvt_lstm_seq_bwd_workspace_bytes(B, H, dtype) bytes, 16-byte aligned. */
size_t dvt_lstm_seq_bwd_workspace_bytes(int64_t B, int64_t H, int dtype);
int dvt_lstm_seq_bwd(const void* w_hh, const float* gates, const float* c, const void* dh_seq, const void* dh_last,
                     void* dG, void* workspace, int64_t B, int64_t T, int64_t H, int dtype, dvt_stream_t stream);
/* The LSTMRegressor criterion nn.BCELoss()(torch.sigmoid(z), y) (LSTM.py:55-57), mean over n; each log term clamped at
 * -100 as BCELoss does (this is not BCEWithLogits: a saturated logit gives loss 100, not its magnitude).
 * z [n] dtype, target [n] f32, loss [1] f32, prob [n] f32 = sigmoid(z) (NULL: not written). */
int dvt_sigmoid_bce_fwd(const void* z, const float* target, float* loss, float* prob, int64_t n, int dtype,
                        dvt_stream_t stream);
/* dz = gloss[0] / n * (p - y) / max(p (1 - p), 1e-12) * p (1 - p) with p = sigmoid(z): BCELoss's backward, then sigmoid's. */
int dvt_sigmoid_bce_bwd(const void* z, const float* target, const float* gloss, void* dz, int64_t n, int dtype,
                        dvt_stream_t stream);

/* ---------------------------------------------------------------- 3-D convolution (the r3d_18 video expert)
 * Additions within ABI v5: new entry points only, no existing layout or meaning changed.
 * Full kt x kh x kw convolution forward as an implicit GEMM, for inference (torchvision r3d_18: Conv3DSimple, BasicStem and
 * the 1x1x1 strided downsamples, behind the reference's EmbeddingExtractor, src/models/pretrained/models.py).
 * x NDHWC [N*T*H*W, C] in dtype, C a multiple of 8 (zero-extend fewer channels: the stem's 3 planes run as 8);
 * w [Cout][K] with K = dvt_conv3d_implicit_k(desc) = kt*kh*kw*C rounded up to 32, column ((dt*kh + dh)*kw + dw)*C + c,
 * zero beyond (dvt_conv3d_weight_pack writes it so); y [N*To*Ho*Wo, Cout] in dtype, To = (T + 2 pt - kt) / st + 1 etc.
 * Epilogue on the fp32 accumulators, every part optional (NULL / 0: off):
 *   y = relu ? max(0, acc * scale[co] + shift[co] + residual[m, co]) : acc * scale[co] + shift[co] + residual[m, co]
 * scale / shift f32 [Cout] (an eval-mode BatchNorm folded by dvt_bn_fold), residual [M, Cout] in dtype.
 * dtype BF16 / F16 (fp32 accumulation) or F32 (exact fp32 MFMA).  Geometries with few output tiles and a deep K split the
 * reduction into fp32 slabs in `workspace` (dvt_conv3d_implicit_workspace_bytes(desc) bytes, 16-byte aligned; 0: none
 * needed) summed in a fixed order by a second launch.  No atomics: two identical calls give bitwise-equal results.
 * x and w must each be < 2 GiB (else DVT_ERR_UNSUPPORTED: split the batch).  The caller zero-initialises the descriptor. */
typedef struct dvt_conv3d_desc {
  const void* x;
  const void* w;
  void* y;
  int64_t N;
  int32_t T, H, W, C, Cout;
  int32_t kt, kh, kw, st, sh, sw, pt, ph, pw;
  int32_t dtype;
  const float* scale;
  const float* shift;
  const void* residual;
  int32_t relu;
  void* workspace;
} dvt_conv3d_desc;
int dvt_conv3d_implicit_supported(const dvt_conv3d_desc* desc);   /* 1: dvt_conv3d_implicit takes the geometry */
int64_t dvt_conv3d_implicit_k(const dvt_conv3d_desc* desc);         /* row length of the packed weights; -1: unsupported */
size_t dvt_conv3d_implicit_workspace_bytes(const dvt_conv3d_desc* desc);
int dvt_conv3d_implicit(const dvt_conv3d_desc* desc, dvt_stream_t stream);
/* Addition within ABI v5: the layer-1 halves of R(2+1)D-18 at inference, with the same descriptor, packed weights and
 * epilogue as dvt_conv3d_implicit: 64 -> 144 (1,3,3) / 1 / (0,1,1) and 144 -> 64 (3,1,1) / 1 / (1,0,0), bf16 / fp16, any
 * N, T, H, W whose map stays below 2 GiB.  No workspace, no atomics.  _supported: 1 if the descriptor is one of them. */
int dvt_conv2p1d_l1_supported(const dvt_conv3d_desc* desc);
int dvt_conv2p1d_l1(const dvt_conv3d_desc* desc, dvt_stream_t stream);
/* w f32 [Cout][Cin][kt][kh][kw] (nn.Conv3d.weight) -> dst [Cout][ld] in dst_dtype, column ((dt*kh + dh)*kw + dw)*Cp + c,
 * zero for c >= Cin and for columns >= kt*kh*kw*Cp.  Cp >= Cin, ld >= kt*kh*kw*Cp. */
int dvt_conv3d_weight_pack(const float* w, void* dst, int dst_dtype, int Cout, int Cin, int kt, int kh, int kw, int Cp,
                           int64_t ld, dvt_stream_t stream);
/* Eval-mode BatchNorm as a per-channel affine: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale
 * (gamma / beta NULL: 1 / 0).  All f32 [C]. */
int dvt_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                float* scale, float* shift, int C, dvt_stream_t stream);

/* ---------------------------------------------------------------- the MLP baselines on expert embeddings
 * Additions within ABI v5: new entry points only, no existing layout or meaning changed.
 * SpatioTemporalContrastiveModel (src/models/contrastivemodel.py) and BasicMLP (src/models/basicmlp.py); their GEMMs run on
 * dvt_gemm.  No atomics in any reduction: two identical calls give bitwise-equal results.  dtype F32, BF16 or F16.
 *
 * y = BatchNorm1d(relu(z)) on S * B rows of C columns (S = 1 or 2 segments of B rows, each with its own batch statistics:
 * two views in one launch).  z [S*B][ldz], y [S*B][ldy] in dtype; gamma, beta, running_mean, running_var f32 [C].
 * training: mean and biased variance per segment (centred two-pass form), save_mean / save_invstd f32 [S, C]; the running
 * statistics (NULL: not tracked) take momentum * (mean, unbiased variance) segment 0 first, then segment 1, and
 * *num_batches_tracked (NULL: none) += S -- exactly S successive nn.BatchNorm1d calls.  B = 1 is refused, as torch does.
 * eval: the affine form from the running statistics; save_mean / save_invstd (optional) f32 [C] receive running_mean and
 * 1 / sqrt(running_var + eps). */
int dvt_bn1d_relu_fwd(const void* z, int64_t ldz, void* y, int64_t ldy, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save_mean,
                      float* save_invstd, int64_t B, int64_t C, int S, float eps, float momentum, int training, int dtype,
                      dvt_stream_t stream);
/* Backward of dvt_bn1d_relu_fwd: dz = [z > 0] * d/dx BN(x) (the ReLU of the prologue applied in the same pass).
 * save_mean / save_invstd: the forward's ([S, C] training, [C] eval).  dgamma / dbeta f32 [C] (NULL: not wanted) are the
 * sums over the segments in order, added to the buffers when `accumulate`. */
int dvt_bn1d_relu_bwd(const void* dy, int64_t lddy, const void* z, int64_t ldz, const float* gamma, const float* save_mean,
                      const float* save_invstd, void* dz, int64_t lddz, float* dgamma, float* dbeta, int accumulate,
                      int64_t B, int64_t C, int S, int training, int dtype, dvt_stream_t stream);
/* torch.optim.Adam (amsgrad off, coupled L2 decay: g += weight_decay * p before the moments) over n f32 elements, the
 * learning rate read from the device scalar lr_dev[0] (a captured step sees a new value without re-capture).
 * step_dev2, skip64 and mirror as dvt_adamw_step_fused. */
int dvt_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* lr_dev,
                      float beta1, float beta2, float eps, float weight_decay, int64_t* step_dev2, const uint8_t* skip64,
                      void* mirror, int mirror_dtype, dvt_stream_t stream);
/* nn.CrossEntropyLoss() on integer labels: loss[0] = mean over the rows whose label != ignore_index of
 * logsumexp(x_r) - x_r[label_r], fp32 arithmetic.  logits [M][ld] dtype, labels int64 [M]; lse f32 [M + 1] receives the
 * per-row log-sum-exp and, at [M], the number of counted rows.  A label outside [0, C) is never used as an index: the
 * loss (and that row's gradient) become NaN. */
int dvt_ce_labels_fwd(const void* logits, int64_t ld, const int64_t* labels, float* loss, float* lse, int64_t M, int64_t C,
                      int64_t ignore_index, int dtype, dvt_stream_t stream);
/* dlogits[r] = gloss[0] / count * (softmax(x_r) - onehot(label_r)); zero rows for ignore_index. */
int dvt_ce_labels_bwd(const void* logits, int64_t ld, const int64_t* labels, const float* lse, const float* gloss,
                      void* dlogits, int64_t lddl, int64_t M, int64_t C, int64_t ignore_index, int dtype,
                      dvt_stream_t stream);
/* out[r][0:D] = concatenation of `parts` source rows, cast to dtype; columns past the sources' total width are zero.
 * table: int64 [rows][parts][3] on the device, {address, width, source dtype} per entry. */
int dvt_gather_rows_ptr(const int64_t* table, int64_t rows, int parts, void* out, int64_t ldo, int64_t D, int dtype,
                        dvt_stream_t stream);

/* ---------------------------------------------------------------- the online probe of the contrastive model
 * Additions within ABI v5: new entry points and one new descriptor, no existing layout or meaning changed.
 * SSLOnlineEval (src/callbacks/callbacks.py:147-300) trains pl_bolts' SSLEvaluator after every training batch:
 *   Dropout(p) -> Linear(D, H, no bias) -> BatchNorm1d(H) -> ReLU -> Dropout(p) -> Linear(H, C) -> sigmoid -> nn.BCELoss()
 * followed by torch.optim.SGD(lr, no momentum, no decay).  One step is three launches, in this order:
 *   dvt_probe_fwd       per slab of 16 hidden columns: z = drop(x) W1^T, BatchNorm (training: batch statistics, the running
 *                       statistics and *num_batches_tracked moved exactly as nn.BatchNorm1d moves them; eval: the running
 *                       statistics), ReLU, second dropout; writes h, z (training), save_mean / save_invstd (training) and
 *                       the slab's partial logits into `workspace` (f32 [H / 16][B][C], dvt_probe_workspace_bytes).
 *   dvt_probe_loss      sums the partials in slab order, adds the bias; prob = sigmoid (f32), loss[0] = the mean BCE with
 *                       each log clamped at -100; training: dlogits, the bias gradient and its SGD update.  Without a
 *                       target (training = 0 in this call's descriptor) it only writes `logits`.
 *   dvt_probe_bwd_step  (training) per slab: the gradients of W2[:, slab] (from W2 before its update), gamma, beta and
 *                       W1[slab, :] with the dropout masks of the forward (the first regenerated from the Philox stream, the
 *                       second and the ReLU read from h != 0), then SGD on those parameters.
 * Gradients live in the persistent f32 buffers g_*: overwritten, or added to when `accumulate` (a probe whose gradients
 * are never zeroed).  The SGD update is p - lr * g with both operations rounded in fp32, g the buffer's new content.
 * Parameters are f32 masters, rounded to `dtype` where a matrix instruction reads them; fp32 is exact fp32 arithmetic.
 * Dropout (training, p > 0): rng_state {seed, step base} on the device as for dvt_dropout; the first mask takes the
 * (B D + 3) / 4 Philox blocks from call offset rng_offset on, the second the (B H + 3) / 4 blocks after them.
 * No atomics, no host synchronisation, every reduction in a fixed order: two identical calls from the same state give
 * bitwise-equal results, and the three calls may be captured in a hipGraph (lr is a plain argument).
 * _supported: 1 <= B <= 1024 (B = 1 refused in training, as torch does), 1 <= D <= 4096, H a multiple of 16 up to 2048,
 * 1 <= C <= 32, dtype F32 / BF16 / F16. */
typedef struct dvt_probe_desc {
  const void* x;                 /* [B][D] dtype */
  const float* target;           /* [B][C] f32 (loss) */
  float* w1;                     /* [H][D] block_forward.2.weight */
  float* gamma;                  /* [H] block_forward.3.weight */
  float* beta;                   /* [H] block_forward.3.bias */
  float* running_mean;           /* [H] (training: NULL = not tracked) */
  float* running_var;            /* [H] */
  int64_t* num_batches_tracked;  /* [1] or NULL */
  float* w2;                     /* [C][H] block_forward.6.weight */
  float* b2;                     /* [C] block_forward.6.bias */
  float* g_w1;                   /* gradient buffers, the parameters' shapes (training) */
  float* g_gamma;
  float* g_beta;
  float* g_w2;
  float* g_b2;
  void* h;                       /* [B][H] dtype: the second Linear's input */
  float* z;                      /* [B][H] f32: the first Linear's output (training) */
  float* save_mean;              /* [H] (training) */
  float* save_invstd;            /* [H] (training) */
  float* logits;                 /* [B][C] f32, optional: the pre-sigmoid output (target NULL: the only output) */
  float* prob;                   /* [B][C] f32 */
  float* loss;                   /* [1] f32 */
  float* dlogits;                /* [B][C] f32 (training) */
  void* workspace;               /* dvt_probe_workspace_bytes */
  const uint64_t* rng_state;     /* {seed, step base} on the device (training, p > 0) */
  uint64_t rng_offset;
  int64_t B;
  int32_t D, H, C, dtype, training, accumulate;
  float p, eps, momentum, lr;
} dvt_probe_desc;
int dvt_probe_supported(int64_t B, int D, int H, int C, int dtype);
size_t dvt_probe_workspace_bytes(int64_t B, int H, int C);
int dvt_probe_fwd(const dvt_probe_desc* desc, dvt_stream_t stream);
int dvt_probe_loss(const dvt_probe_desc* desc, dvt_stream_t stream);
int dvt_probe_bwd_step(const dvt_probe_desc* desc, dvt_stream_t stream);
/* SSLOnlineEval.on_shared_end: per class and per threshold the TP / FP / FN counts of `probs > thresholds[t]` (strict,
 * compared in fp32) against multilabel targets, in ONE launch: counts int64 [T][3][C], support int64 [C].  probs f32 [N][C],
 * labels u8 [N][C], thresholds f32 [T] on the device, 1 <= T <= 64.  Integer counts, fixed-order sums, no atomics. */
int dvt_multilabel_sweep_counts(const float* probs, const unsigned char* labels, int64_t N, int C, const float* thresholds,
                                int T, int64_t* counts, int64_t* support, dvt_stream_t stream);

/* ---------------------------------------------------------------- LARS (layer-wise adaptive rate scaling)
 * Additions within ABI v5.  pl_bolts.optimizers.lars.LARS, which the reference imports for its contrastive model
 * (contrastivemodel.py:8, :64-70).  Per tensor with a gradient, all in fp32:
 *   d = g
 *   if weight_decay != 0 and |p| != 0 and |g| != 0:  d = trust_coefficient |p| / (|g| + weight_decay |p| + eps) * (g + weight_decay p)
 *   if momentum != 0:  buf = d on the first step, momentum buf + (1 - dampening) d afterwards;  d = d + momentum buf (nesterov) or buf
 *   p = p - lr d
 * The tensors are the entries of a table ON THE DEVICE (pointers, so that separate allocations and slices of one flat buffer
 * take the same path); a tensor without a gradient this step is not in the table and stays untouched.  Each segment is cut
 * into chunks of dvt_lars_plan_info.chunk elements, one block per chunk; chunk_begin is the index of the segment's first
 * chunk (dvt_lars_plan fills it), ascending over the table.  `workspace` (caller-owned, workspace_bytes, 8-byte aligned,
 * no initial content required) receives the per-chunk sums of p^2 and g^2; a segment's sums are added from them in a fixed
 * order that depends on numel alone.  No atomics on floats, no host synchronisation: identical calls from the same state
 * give bitwise-equal results and may be captured in a hipGraph. */
typedef struct dvt_lars_seg {
  float* param;                  /* [numel] f32 */
  const float* grad;             /* [numel] f32 */
  float* buf;                    /* [numel] f32 momentum buffer (momentum == 0: unused, may be NULL) */
  void* mirror;                  /* [numel] bf16 / f16 copy of the updated parameter (`mirror` == 0: unused) */
  int64_t numel;                 /* >= 1 */
  int64_t chunk_begin;
  float weight_decay;
  int32_t reserved;
} dvt_lars_seg;
typedef struct dvt_lars_plan_info {
  int64_t chunk;                 /* elements per chunk */
  int64_t blocks;                /* blocks per launch = the total number of chunks, sum of ceil(numel / chunk) */
  int64_t grid_cap;              /* 0: no cap, every chunk has a block of its own */
  int64_t workspace_bytes;
} dvt_lars_plan_info;
/* Host only.  numel [n] on the host; chunk_begin (optional) receives n + 1 values, the last one the total. */
int dvt_lars_plan(const int64_t* numel, int n, dvt_lars_plan_info* info, int64_t* chunk_begin);
/* sumsq f32 [n][2] on the device = {sum p^2, sum g^2} per segment, the values dvt_lars_step uses.  `chunks`: the plan's
 * `blocks` for this table (the table is on the device, so the host cannot check it against chunk_begin); `workspace`
 * holds `chunks` pairs.  A larger value only launches idle blocks, which touch no tensor.  Two launches. */
int dvt_lars_sumsq(const dvt_lars_seg* table, int n, int64_t chunks, float* workspace, float* sumsq, dvt_stream_t stream);
/* One LARS step over the table in two launches (norms, update).  lr_dev f32 [1] and step_dev2 int64 [2] {steps taken,
 * launch ticket} on the device, as dvt_adam_step_dev; the counter only tells the first step (buf = d) from later ones.
 * mirror != 0: every segment's `mirror` is written, mirror_dtype DVT_BF16 / DVT_F16.  n == 0: nothing is launched. */
int dvt_lars_step(const dvt_lars_seg* table, int n, int64_t chunks, float* workspace, const float* lr_dev, float momentum,
                  float dampening, int nesterov, float trust_coefficient, float eps, int64_t* step_dev2, int mirror,
                  int mirror_dtype, dvt_stream_t stream);

/* ---------------------------------------------------------------- global gradient norm and clipping
 * Additions within ABI v5.  The reference's trainer line, pl.Trainer(..., accumulate_grad_batches=8, precision=16, ...)
 * (src/main.py:85), is a transformer run under Lightning, whose other knob for such runs is gradient_clip_val:
 * torch.nn.utils.clip_grad_norm_ over all gradients between backward and the optimizer step.  csrc/optim.hip.
 * Both entry points take a dvt_lars_seg table (dvt_lars_plan's chunks and chunk_begin) and read `grad` and `numel` of a row
 * only: `param`, `buf` and `mirror` may be NULL, so the parameters cost no bytes.  ONE norm over the whole table.
 * norm_kind DVT_NORM_2: total = sum g^2, norm = sqrt(total); DVT_NORM_INF: total = norm = max |g| (a NaN is kept).
 * `workspace`: the plan's workspace_bytes, 4-byte aligned, no initial content required; it receives one partial per chunk.
 * No atomics at all: every sum and maximum is taken in an order that numel alone fixes, so identical calls give
 * bitwise-equal results on every rank and in a hipGraph replay.  No host synchronisation.  n == 0: nothing is launched.
 *   dvt_grad_norm: TWO launches (partials; one block for the total).  out2 f32 [2] on the device = {norm, total}.
 *   dvt_grad_clip: TWO launches (partials; scale -- every block forms the total from the partials itself).  coef = min(1, max_norm / (norm * inv_scale + 1e-6)), grad *= coef in
 *     place, norm_out f32 [1] = norm * inv_scale (the norm before clipping).  inv_scale = 1 when scale_dev is NULL, else
 *     scale_dev[0] (scale_is_inverse != 0) or 1 / scale_dev[0] (the loss scale itself, as dvt_adamw_step_scaled reads it): the
 *     threshold applies to the unscaled gradient.  Deviation from torch: a non-finite norm leaves the gradient exactly
 *     as it is (torch would multiply it by NaN), so that dvt_adamw_step_scaled's own found_inf check still sees the values
 *     that overflowed and skips the step; norm_out then holds the non-finite value.  coef == 1 writes nothing either. */
enum dvt_norm_kind { DVT_NORM_2 = 0, DVT_NORM_INF = 1 };
int dvt_grad_norm(const dvt_lars_seg* table, int n, int64_t chunks, float* workspace, int norm_kind, float* out2,
                  dvt_stream_t stream);
int dvt_grad_clip(const dvt_lars_seg* table, int n, int64_t chunks, float* workspace, int norm_kind, float max_norm,
                  const float* scale_dev, int scale_is_inverse, float* norm_out, dvt_stream_t stream);

/* ---------------------------------------------------------------- grouped AdamW and weight EMA (csrc/optim_groups.hip)
 * Additions within ABI v5.  The fine-tuning recipe of a pre-trained ViT (MAE's param_groups_lrd, timm's ModelEmaV2) on
 * the flat buffer: the dvt_adamw_step_fused launch with the learning rate and the weight decay chosen per 64-element
 * block.  group64: one byte per 64 elements (ceil(n / 64) bytes, the granularity of skip64) naming a row of group_table,
 * f32 [ngroups][2] = {lr_scale, weight_decay} on the device, 1 <= ngroups <= 255; a block's rate is
 * lr_dev[0] * lr_scale (fp32), lr_dev an f32 device scalar as in dvt_adam_step_dev.  The map is on the device, so the
 * entry cannot check that every byte is below ngroups: the caller does (ops.adamw_group_table).  step_dev2, skip64 and
 * mirror as dvt_adamw_step_fused.  ema (nullable) f32 [n]: after the update, ema = d ema + (1 - d) param with
 * d = ema_decay_dev[0], for EVERY element -- blocks that skip64 masks included, as ModelEmaV2 averages every entry
 * whether or not the optimizer touched it.  One launch, no host synchronisation, no allocation. */
int dvt_adamw_groups_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                          const float* lr_dev, float beta1, float beta2, float eps, const uint8_t* group64,
                          const float* group_table, int ngroups, int64_t* step_dev2, const uint8_t* skip64, void* mirror,
                          int mirror_dtype, float* ema, const float* ema_decay_dev, dvt_stream_t stream);
/* ema = d ema + (1 - d) param over n f32 elements, d = ema_decay_dev[0]: the same statement as a launch of its own,
 * for use after any other optimizer step.  Both buffers 16-byte aligned. */
int dvt_ema_update(float* ema, const float* param, int64_t n, const float* ema_decay_dev, dvt_stream_t stream);

/* ---------------------------------------------------------------- VGGish audio expert: log-mel front end, first layer
 * Additions within ABI v5.  The audio network the reference names at pretrained/models.py:13 (torchvggish, commented out:
 * torch.hub needs the network) and calls at :55-57.  csrc/audio.hip; the definition of the front end (16 kHz mono, frames
 * of 400 every 160, periodic Hann, |rfft_512|, 64 HTK mel bands 125 .. 7500 Hz with a zero DC row, log(mel + 0.01), examples
 * of 96 frames every 96) is stated once, at the top of that file.
 *   dvt_logmel_num_examples(L): examples E a row of L samples yields (0 below 15 600).  Host only.
 *   dvt_logmel_tables: the window, the FFT twiddles, the windowed DFT table and the mel matrix, computed in float64 and
 *     rounded once, written to a HOST buffer of dvt_logmel_examples_workspace_bytes() bytes; the caller uploads it once and
 *     passes the device copy (16-byte aligned) as `tables`.
 *   dvt_logmel_examples: wave f32 [R][L] in [-1, 1] -> out [R * E][96][64] of `dtype` (the NHWC map of a one-channel image,
 *     H = time, W = mel), fp32 arithmetic, one rounding at the store.  E == 0 or R == 0: nothing is launched.  `variant`
 *     picks the spectrum: a radix-2 FFT in LDS (the form the Python side uses) or a table DFT on v_mfma_f32_16x16x4_f32 (kept
 *     for the comparison of the two; its 400-term sums are less accurate); both leave their magnitudes to the same mel product.  No atomics: identical calls give bitwise-equal results.
 *   dvt_vggish_conv1_pool: Conv2d(1, 64, 3, padding 1) + bias + ReLU + MaxPool2d(2, 2) in one launch.  x [N][H][64] of
 *     `dtype`, w f32 [64][9] (nn.Conv2d's [64, 1, 3, 3]), bias f32 [64] -> y NHWC [N * H/2 * 32][64] of `dtype`; H even. */
enum dvt_logmel_variant { DVT_LOGMEL_DFT = 0, DVT_LOGMEL_FFT = 1 };
int64_t dvt_logmel_num_examples(int64_t L);
size_t dvt_logmel_examples_workspace_bytes(void);
int dvt_logmel_tables(float* dst, size_t bytes);
int dvt_logmel_examples(const float* wave, int64_t R, int64_t L, const float* tables, void* out, int dtype, int variant,
                        dvt_stream_t stream);
int dvt_vggish_conv1_pool(const void* x, const float* w, const float* bias, void* y, int64_t N, int H, int W, int dtype,
                          dvt_stream_t stream);

/* ---------------------------------------------------------------- class-activation maps (Grad-CAM) of the video encoder
 * Additions within ABI v5.  What the reference does with the pytorch_grad_cam library at src/main.py:93-108, on the device;
 * csrc/cam.hip.  All three entry points run asynchronously on `stream`, use only the caller's buffers, sum in fp32 in a fixed
 * order without atomics (identical calls give bitwise-equal results) and launch nothing for N == 0 (B == 0).
 *   dvt_cam_seed: logits [B][K] of `dtype` -> seed [B][K] of `dtype`, one-hot at category[b] (device int32 [B]), or at the
 *     row's argmax (ties to the lowest index, as numpy.argmax) where `category` is NULL or the entry negative; an entry >= K
 *     leaves the row zero.  No host synchronisation.
 *   dvt_cam_map: activation A and gradient G [N][P][C] of `dtype`, channels last, P = T' H' W', C a multiple of 8 and at most
 *     DVT_CAM_MAX_C, both 16-byte aligned -> weights f32 [N][C] (optional), raw f32 [N][P] (optional), scaled f32 [N][P].
 *       DVT_CAM_GRADCAM    w = (1 / P) sum_p G
 *       DVT_CAM_XGRADCAM   w = sum_p G A / (sum_p A + 1e-7)
 *       DVT_CAM_GRADCAMPP  w = sum_p max(G, 0) a,  a = G^2 / (2 G^2 + S G^3 + 1e-6) (0 where G == 0),  S = sum_p A
 *     raw = max(sum_c w A, 0);  scaled = (raw - min_p raw) / (1e-7 + max_p (raw - min_p raw)) per clip (the library's
 *     scale_cam_image); an all-zero raw row gives an all-zero scaled row.
 *     Launches: ONE, one workgroup per clip, where P <= DVT_CAM_FUSED_MAX_P and P * C <= DVT_CAM_FUSED_MAX_ELEMS (layer 4 at
 *     2*7*7 x 512, layer 3 at 3*14*14 x 256); otherwise THREE (weights per 64-channel slab; map and chunk extrema; scaling)
 *     and a workspace of dvt_cam_map_workspace_bytes(N, P, C) bytes (0 for the one-launch form).  dvt_cam_map_launches(P, C)
 *     names the form.  Host only, both.
 *   dvt_cam_jet_table: the 256 x 3 byte JET table in RGB order, built in float64 (x = i / 255: r = clamp(1.5 - |4x - 3|),
 *     g = clamp(1.5 - |4x - 2|), b = clamp(1.5 - |4x - 1|), entries floor(255 v + 0.5)), written to a HOST buffer.
 *   dvt_cam_render: scaled f32 [N][Ti][Hi][Wi] -> mask f32 [N][T][H][W] (optional when frames are given): separable linear
 *     interpolation with half-pixel centres, per axis src = (o + 0.5) I / O - 0.5 clamped to [0, I - 1], taps floor(src) and
 *     min(floor(src) + 1, I - 1) (torch's interpolate(mode="trilinear", align_corners=False); Ti == T == 1 is the bilinear
 *     case).  With `frames` ([N][T][H][W][3], uint8, or f32 in [0, 1] when frames_f32) it also writes `overlay` uint8
 *     [N][T][H][W][3], the library's show_cam_on_image per frame: heat = jet[(int)(255 mask)] / 255 (RGB if use_rgb, else
 *     BGR; the index clamped to 0 .. 255), blend = (1 - image_weight) heat + image_weight img, out = (uint8)(255 blend /
 *     max over the frame of blend), zeros where that maximum is 0.  `jet`: a device copy of dvt_cam_jet_table's bytes.  One
 *     workgroup per output frame evaluates the blend twice (maximum, then write) and stores no intermediate. */
#define DVT_CAM_MAX_C 2048
#define DVT_CAM_FUSED_MAX_P 4096
#define DVT_CAM_FUSED_MAX_ELEMS 262144
enum dvt_cam_method { DVT_CAM_GRADCAM = 0, DVT_CAM_GRADCAMPP = 1, DVT_CAM_XGRADCAM = 2 };
int dvt_cam_seed(const void* logits, const int32_t* category, void* seed, int64_t B, int64_t K, int dtype,
                 dvt_stream_t stream);
int dvt_cam_map_launches(int64_t P, int64_t C);
size_t dvt_cam_map_workspace_bytes(int64_t N, int64_t P, int64_t C);
int dvt_cam_map(const void* A, const void* G, int64_t N, int64_t P, int64_t C, int dtype, int method, float* weights,
                float* raw, float* scaled, void* workspace, size_t workspace_bytes, dvt_stream_t stream);
int dvt_cam_jet_table(uint8_t* dst, size_t bytes);
int dvt_cam_render(const float* scaled, int64_t N, int Ti, int Hi, int Wi, int T, int H, int W, float* mask,
                   const void* frames, int frames_f32, const uint8_t* jet, uint8_t* overlay, float image_weight, int use_rgb,
                   dvt_stream_t stream);

/* ---------------------------------------------------------------- rank metrics and counts (AUROC, AP, F1, confusion matrix)
 * Additions within ABI v5: new entry points only, no existing layout or meaning changed.  What the reference names next to
 * AveragePrecision: `from torchmetrics import AUROC, F1, AveragePrecision` (src/models/frame_transformer.py:8; val_auroc /
 * train_auroc at :114-115, the log lines at :276-343), torchmetrics.F1(num_classes=22) (src/models/basicmlp.py:20), and
 * scikit-learn's confusion_matrix with the MITEval accuracy callback (src/callbacks/callbacks.py:14, :85-98; attached to every
 * MIT run at src/main.py:46-50).  csrc/eval_metrics.hip.  Everything runs asynchronously on `stream` with no host
 * synchronisation; integer results are exact and floating-point sums go in a fixed order without atomics, so identical calls
 * give bitwise-equal results.
 *
 *   dvt_rank_metrics: probs f32 [N][C], labels u8 [N][C] (non-zero = positive), N * C < 2^31.  One class-major layout and ONE
 *     descending segmented radix sort per call (as dvt_average_precision), then a tie-aware parallel reduction of every sorted
 *     column in blocks of dvt_rank_metrics_block() elements (host only; three launches: per-block aggregates, the pass with
 *     carries read from the aggregates, the totals -- no workgroup waits on another inside a launch).  A tie group is a
 *     maximal run of equal scores (-0.0 == +0.0); with tp the inclusive count of positives, P the positives and Nn = N - P,
 *     per group g = [b, e]: pos_g = tp[e] - tp[b-1], neg_g = (e - b + 1) - pos_g,
 *         two_u[c]  = sum_g neg_g (2 tp[b-1] + pos_g)                  (int64, exact)
 *         auroc[c]  = two_u / (2 P Nn) in float64; NaN for a class without positives or without negatives
 *         ap[c]     = sum_g (pos_g / P) (tp[e] / (e + 1)) in float64; 0 for a class without positives
 *     (roc_auc_score / average_precision_score of scikit-learn with average=None, to about 1e-16).
 *     averages f64 [DVT_RANK_N_AVERAGES], indexed by dvt_rank_average: macro and support-weighted AUROC over the VALID
 *     classes (both kinds present; NaN when there is none), micro AUROC (the same pass over all N C elements as one column:
 *     only with DVT_RANK_MICRO, else NaN), and with DVT_RANK_SAMPLES (C <= 64 then) the fixed-order SUM of the per-row AUROC
 *     over the valid rows, else NaN.  counts int64 [DVT_RANK_N_COUNTS], indexed by dvt_rank_count: valid classes, valid rows,
 *     the micro column's 2U and positives (-1 where the flag is off).  Scikit-learn and torchmetrics raise on a column
 *     without both kinds; raising needs a host read, hence NaN.  NaN scores are undefined behaviour of the metric.
 *     workspace >= dvt_rank_metrics_workspace_bytes(N, C, flags) (0: empty input or N * C >= 2^31).
 *   dvt_confusion_matrix: cm int64 [C][C], rows = target, columns = prediction.  Predictions are `logits` [N][C] of `dtype`
 *     (the row's argmax, the lowest index among equal maxima) or `preds` int64 [N]; exactly one of the two is non-NULL.
 *     target int64 [N].  accumulate != 0 ADDS to cm and cm_ignored, 0 overwrites them.  A row whose target (or integer
 *     prediction) is outside [0, C) is skipped and counted in cm_ignored[1].  N == 0 is allowed.
 *   dvt_multilabel_counts: state int64 [4][C] = TP, FP, FN, TN per class of `probs > threshold` (strict, compared in fp32 as
 *     dvt_multilabel_sweep_counts does) against labels u8 [N][C]; same `accumulate`; C <= 1024; N == 0 is allowed.
 *   dvt_count_equal: out int64 [1] = the number of i < n with a[i] == b[i], both int64 (is_int64 != 0) or both f32: the
 *     `torch.sum(running_logits == running_labels)` of MITEval (callbacks.py:91); same `accumulate`; n == 0 is allowed. */
enum dvt_rank_flags { DVT_RANK_MICRO = 1, DVT_RANK_SAMPLES = 2 };
enum dvt_rank_average { DVT_RANK_AVG_MACRO = 0, DVT_RANK_AVG_WEIGHTED = 1, DVT_RANK_AVG_MICRO = 2, DVT_RANK_AVG_SAMPLES_SUM = 3 };
enum dvt_rank_count { DVT_RANK_CNT_VALID_CLASSES = 0, DVT_RANK_CNT_VALID_ROWS = 1, DVT_RANK_CNT_MICRO_TWO_U = 2,
                      DVT_RANK_CNT_MICRO_POSITIVES = 3 };
#define DVT_RANK_N_AVERAGES 4
#define DVT_RANK_N_COUNTS 4
int dvt_rank_metrics_block(void);
size_t dvt_rank_metrics_workspace_bytes(int64_t N, int C, int flags);
int dvt_rank_metrics(const float* probs, const unsigned char* labels, int64_t N, int C, int flags, double* auroc, double* ap,
                     int64_t* positives, int64_t* two_u, double* averages, int64_t* counts, void* workspace,
                     dvt_stream_t stream);
int dvt_confusion_matrix(const void* logits, int dtype, const int64_t* preds, const int64_t* target, int64_t N, int C,
                         int accumulate, int64_t* cm, int64_t* cm_ignored, dvt_stream_t stream);
int dvt_multilabel_counts(const float* probs, const unsigned char* labels, int64_t N, int C, float threshold, int accumulate,
                          int64_t* state, dvt_stream_t stream);
int dvt_count_equal(const void* a, const void* b, int64_t n, int is_int64, int accumulate, int64_t* out, dvt_stream_t stream);

/* ---------------------------------------------------------------- attention rollout (Abnar & Zuidema, 2020)
 * Additions within ABI v5: new entry points only.  What a transformer attends to, from the attention the model already
 * computes at src/models/vit.py:51-53 (P = softmax(scale q k^T) per head; nn.MultiheadAttention inside
 * nn.TransformerEncoderLayer for the FrameTransformer, frame_transformer.py:41-44); csrc/attn_rollout.hip.  With
 * A_l = rho I + (1 - rho) mean_h P_l^h the rollout of a start vector r0 is r0^T A_L ... A_1: only that ROW is formed, one
 * vector-matrix product per layer, and no N x N tensor exists anywhere:
 *     r_out[s, j] = rho r_in[s, j] + (1 - rho) / H sum_h sum_i r_in[s, i] exp(scale q_i . k_j - lse[s, h, i])
 * Probabilities and r are fp32 throughout (nothing is rounded to 16 bits after the exponential); every sum has a fixed
 * order and nothing is atomic, so identical calls give bitwise-equal results.  Everything runs asynchronously on `stream`
 * with the caller's buffers; S == 0 launches nothing.
 *   dvt_rollout_step: q [S][H][Lq][dh] and k [S][H][N][dh] as strided views (element (s, h, l, e) at q[s*q_sb + h*q_sh +
 *     l*q_sl + e], the fields of dvt_attn_desc), lse f32 [S][H][Lq] as dvt_attention_fwd wrote it, r_in f32 [S][N] or NULL,
 *     r_out f32 [S][N] (not r_in).  r_in == NULL stands for a start vector that is never stored: the one-hot of token
 *     `query` (>= 0), or the uniform vector 1 / N (query == DVT_ROLLOUT_UNIFORM: the mean-pooled temporal stack).  Lq is N,
 *     or 1 for a layer that ran for one query only (dvt_attention_fwd with Lq == 1: row 0 of q IS token `query`; r_in must be
 *     NULL and query >= 0 then).  Two forms (dvt_rollout_plan names the one a descriptor takes):
 *       MFMA     16-bit dtypes, dh == 64, N <= 512, Lq == N, a stored or uniform r_in, 16-byte aligned q / k and strides that
 *                are multiples of 8: one workgroup per sequence, S^T = K Q^T on mfma_f32_16x16x32 with the query on the lane;
 *       GENERIC  any dtype, dh and N that fits LDS, on the fp32 FMA; every one-hot start (one query row) takes it.
 *     What neither form takes is refused (DVT_ERR_UNSUPPORTED), never computed wrongly.
 *   dvt_rollout_from_probs: the start of the recurrence where the last layer ran on the folded single-query path: P f32
 *     [S][N][8] as dvt_attn_cls_fwd returns it (normalised probabilities of the CLS query, head h of key j at P[(s*N + j)*8
 *     + h]) -> r_out[s, j] = rho [j == query] + (1 - rho) / H sum_h P[s, j, h].
 *   dvt_rollout_video: r_space f32 [B*T][n + 1] (sequence b*T + f: frame f of clip b) and r_time f32 [B][T + 1], both with
 *     the CLS entry first -> raw[b, f, p] = r_time[b, 1 + f] r_space[b*T + f, 1 + p] (optional) and `scaled`, the same map
 *     scaled per clip exactly as dvt_cam_map scales its maps; both f32 [B][T][n].  One launch, one workgroup per clip. */
#define DVT_ROLLOUT_UNIFORM -1
#define DVT_ROLLOUT_MFMA_MAX_N 512
typedef struct dvt_rollout_desc {
  const void* q;
  const void* k;
  const float* lse;
  const float* r_in;
  float* r_out;
  int64_t S, H, N, Lq, dh;
  int64_t q_sb, q_sh, q_sl;
  int64_t k_sb, k_sh, k_sl;
  int64_t query;
  float rho;
  float scale;
  int32_t dtype;
} dvt_rollout_desc;
enum dvt_rollout_form { DVT_ROLLOUT_F_NONE = 0, DVT_ROLLOUT_F_MFMA = 1, DVT_ROLLOUT_F_GENERIC = 2 };
typedef struct dvt_rollout_plan_info {
  int32_t form;       /* enum dvt_rollout_form; NONE when S == 0 */
  int32_t waves;      /* waves per workgroup */
  int32_t key_steps;  /* MFMA: 32-key steps, one per wave column; else 0 */
  int32_t query_parts; /* MFMA: wave rows the 16-query tiles are dealt to; else 0 */
  int64_t lds;        /* dynamic LDS bytes */
} dvt_rollout_plan_info;
/* What dvt_rollout_step would launch for desc, from the launcher's own decisions (host only, runs without a device; the
 * pointers are looked at for NULL-ness and alignment only).  Returns what the launcher returns for a descriptor it refuses. */
int dvt_rollout_plan(const dvt_rollout_desc* desc, dvt_rollout_plan_info* info);
int dvt_rollout_step(const dvt_rollout_desc* desc, dvt_stream_t stream);
int dvt_rollout_from_probs(const float* P, int64_t S, int64_t N, int64_t H, int64_t query, float rho, float* r_out,
                           dvt_stream_t stream);
int dvt_rollout_video(const float* r_space, const float* r_time, int64_t B, int64_t T, int64_t n, float* raw, float* scaled,
                      dvt_stream_t stream);

/* ---------------------------------------------------------------- data-parallel gradient exchange
 * The reference is single-GPU (pl.Trainer(gpus=1), src/main.py:87); north_star partitions the clips of the global
 * batch over the 8 GPUs of a node, and the only exchange of the path is the SUM of the parameter gradients.  RCCL over
 * xGMI behind the ABI, one process per GPU:
 *   rank 0 calls dvt_comm_unique_id and hands the 128 bytes to every rank (any side channel: torch.distributed's
 *   store, MPI, a file); every rank calls dvt_comm_init (a collective: ncclCommInitRank on the calling thread's current
 *   device); dvt_comm_allreduce / dvt_comm_broadcast ENQUEUE an in-place collective on `stream` (no host sync: they may
 *   be captured in a hipGraph next to the backward kernels they overlap with); dvt_comm_destroy frees the communicator.
 * dtype: DVT_F32, or DVT_BF16 / DVT_F16 for half-width gradient buckets.  RCCL is bound at run time (the instance the
 * process has already loaded, e.g. PyTorch's, else the ROCm installation's); DVT_ERR_UNSUPPORTED when none is found. */
#define DVT_COMM_ID_BYTES 128
typedef void* dvt_comm_t;
int dvt_comm_unique_id(void* id_out /* DVT_COMM_ID_BYTES */);
int dvt_comm_init(dvt_comm_t* comm_out, const void* unique_id, int world, int rank);
int dvt_comm_allreduce(dvt_comm_t comm, void* buf, int64_t count, int dtype, dvt_stream_t stream);
int dvt_comm_broadcast(dvt_comm_t comm, void* buf, int64_t count, int dtype, int root, dvt_stream_t stream);
int dvt_comm_destroy(dvt_comm_t comm);

#ifdef __cplusplus
}
#endif
#endif /* DVT_HIP_H */
