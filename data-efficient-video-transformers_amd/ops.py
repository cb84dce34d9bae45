"""Raw (autograd-free) Python wrappers over the C ABI.

Every function launches hand-written HIP kernels from libdvt_hip.so on the
current torch stream; torch is used only to own device memory.  Nothing here
falls back to torch arithmetic.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib as L

Tensor = torch.Tensor

_DT = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}
_TORCH_DT = {L.F32: torch.float32, L.BF16: torch.bfloat16, L.F16: torch.float16}


def dt(t: Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"dtype {t.dtype} is not supported by libdvt_hip (float32 / bfloat16)")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need_cuda(*ts: Optional[Tensor]) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("libdvt_hip operators need tensors on the GPU (HIP device); "
                               "there is no CPU path")


_ws = {}

# Optional live profiler (bench.py): an object with begin(key, flops) / end(key) that
# records HIP events on the current stream around selected launches.
_profiler = None


def set_profiler(p) -> None:
    global _profiler
    _profiler = p


class _timed:
    """``with _timed(key, units):`` -- bracket a launch with the profiler's events when one is installed
    (units = algorithmic bytes for the HBM-bound kernels, flops for GEMMs)."""

    __slots__ = ("key", "units", "prof")

    def __init__(self, key, units):
        self.key, self.units, self.prof = key, units, _profiler

    def __enter__(self):
        if self.prof is not None:
            self.prof.begin(self.key, self.units)

    def __exit__(self, *exc):
        if self.prof is not None:
            self.prof.end(self.key)
        return False



def workspace(nbytes: int, device, slot: str = "main") -> Optional[Tensor]:
    """Grow-only scratch buffer per (device, stream, slot).  Kernels on one stream run in
    order, so consecutive operators on it may share the buffer; another stream gets its own."""
    if nbytes <= 0:
        return None
    key = (str(device), slot, _stream())
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=device)
        _ws[key] = buf
    return buf


_live_deferred = {}      # (device, stream) -> the SplitKPending whose slabs occupy the "deferred" scratch slot


def _deferred_workspace(nbytes: int, device, pending) -> Optional[Tensor]:
    """Scratch slot for the slabs of a deferred split-K reduce.  One slot per (device, stream): a second deferral while an
    earlier pending reduce is still outstanding would overwrite that one's slabs -- refuse it instead of producing a
    silently wrong weight gradient (callers resolve a pending reduce -- ``carry=`` / ``splitk_reduce_pending`` -- before
    they defer the next)."""
    key = (str(device), _stream())
    prev = _live_deferred.get(key)
    if prev is not None and prev.valid:
        raise RuntimeError("a deferred split-K reduce is still pending on this stream: carry it (carry=) or call "
                           "ops.splitk_reduce_pending before deferring another one")
    _live_deferred[key] = pending
    return workspace(nbytes, device, slot="deferred")


# ------------------------------------------------------------------ elementwise
def cast(src: Tensor, dtype: torch.dtype) -> Tensor:
    _need_cuda(src)
    src = src.contiguous()
    out = torch.empty(src.shape, dtype=dtype, device=src.device)
    L.check(L.load().dvt_cast(src.data_ptr(), dt(src), out.data_ptr(), _DT[dtype], src.numel(), _stream()),
            "dvt_cast")
    return out


def zeros(shape, dtype: torch.dtype, device) -> Tensor:
    """A zero-filled tensor without an ATen fill kernel (hipMemsetAsync on the launch stream)."""
    t = torch.empty(shape, dtype=dtype, device=device)
    if not t.is_cuda:
        raise RuntimeError("dvt_amd ops have no CPU path")
    L.check(L.load().dvt_zero(t.data_ptr(), t.numel() * t.element_size(), _stream()), "dvt_zero")
    return t


def add(a: Tensor, b: Tensor) -> Tensor:
    _need_cuda(a, b)
    assert a.shape == b.shape and a.dtype == b.dtype
    a = a.contiguous(); b = b.contiguous()
    out = torch.empty_like(a)
    L.check(L.load().dvt_add(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), dt(a), _stream()), "dvt_add")
    return out


def add_rowtable(x: Tensor, table: Tensor, rows_per_entry: int) -> Tensor:
    """out[r] = x[r] + table[r // rows_per_entry]; x [rows, d], table [rows/rows_per_entry, d] f32."""
    _need_cuda(x, table)
    assert x.is_contiguous() and table.is_contiguous() and table.dtype == torch.float32
    d = x.shape[-1]
    rows = x.numel() // d
    assert table.shape[-1] == d and table.numel() // d * rows_per_entry >= rows
    out = torch.empty_like(x)
    L.check(L.load().dvt_add_rowtable(x.data_ptr(), table.data_ptr(), out.data_ptr(), rows, d, rows_per_entry,
                                      dt(x), _stream()), "dvt_add_rowtable")
    return out


def copy_(dst: Tensor, src: Tensor) -> Tensor:
    """Contiguous device copy (optionally converting dtype) through dvt_cast."""
    _need_cuda(dst, src)
    assert dst.is_contiguous() and src.is_contiguous() and dst.numel() == src.numel()
    L.check(L.load().dvt_cast(src.data_ptr(), dt(src), dst.data_ptr(), dt(dst), src.numel(), _stream()), "dvt_cast")
    return dst


def copy2d(src: Tensor, dst: Tensor, rows: int, cols: int, src_ld: int, dst_ld: int) -> None:
    """dst[r*dst_ld + c] = src[r*src_ld + c] on the raw storages starting at the tensors' data pointers."""
    _need_cuda(src, dst)
    assert src.dtype == dst.dtype
    L.check(L.load().dvt_copy2d(src.data_ptr(), dst.data_ptr(), rows, cols, src_ld, dst_ld, dt(src), _stream()),
            "dvt_copy2d")


def rows_sum(src: Tensor, row_stride: int, rows: int, cols: int, *, out: Optional[Tensor] = None,
             accumulate: bool = False) -> Tensor:
    _need_cuda(src)
    if out is None:
        assert not accumulate
        out = torch.empty((cols,), dtype=torch.float32, device=src.device)
    L.check(L.load().dvt_rows_sum(src.data_ptr(), row_stride, rows, cols, out.data_ptr(), dt(src), int(accumulate),
                                  _stream()), "dvt_rows_sum")
    return out


def permute_021(x: Tensor) -> Tensor:
    """[A, B, C] -> [B, A, C] (contiguous)."""
    _need_cuda(x)
    x = x.contiguous()
    A, B, Cc = x.shape
    out = torch.empty((B, A, Cc), dtype=x.dtype, device=x.device)
    L.check(L.load().dvt_permute_021(x.data_ptr(), out.data_ptr(), A, B, Cc, dt(x), _stream()), "dvt_permute_021")
    return out


def axpby_f32_(dst: Tensor, src: Tensor, alpha: float = 1.0, beta: float = 1.0) -> Tensor:
    """dst(f32) = beta*dst + alpha*src."""
    _need_cuda(dst, src)
    assert dst.dtype == torch.float32 and dst.is_contiguous() and src.is_contiguous()
    assert dst.numel() == src.numel()
    L.check(L.load().dvt_axpby_f32(src.data_ptr(), dt(src), alpha, dst.data_ptr(), beta, dst.numel(), _stream()),
            "dvt_axpby_f32")
    return dst


ACT_GELU, ACT_RELU, ACT_SIGMOID = 1, 2, 3


def act_fwd(x: Tensor, act: int) -> Tensor:
    _need_cuda(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    L.check(L.load().dvt_act_fwd(x.data_ptr(), y.data_ptr(), x.numel(), act, dt(x), _stream()), "dvt_act_fwd")
    return y


def act_bwd(dy: Tensor, x: Tensor, act: int) -> Tensor:
    _need_cuda(dy, x)
    dy = dy.contiguous()
    dx = torch.empty_like(x)
    L.check(L.load().dvt_act_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(), act, dt(x), _stream()),
            "dvt_act_bwd")
    return dx


def _tubelet_geometry(shape, patch: int, tubelet: int, what: str):
    """(frames, C, H, W) of a clip shape [..., t, C, H, W] whose t frames split into whole tubelets."""
    if len(shape) < 4:
        raise ValueError(f"{what}: expected a clip [..., t, C, H, W], got shape {tuple(shape)}")
    if int(tubelet) != tubelet or tubelet < 1:
        raise ValueError(f"{what}: tubelet must be an integer >= 1, got {tubelet!r}")
    t, Cc, H, W = (int(s) for s in shape[-4:])
    if t % tubelet:
        raise ValueError(f"{what}: {t} frames per clip are not whole tubelets of {tubelet}")
    frames = 1
    for s in shape[:-3]:
        frames *= int(s)
    return frames, Cc, H, W


def _patch_gather(what: str, src: Tensor, shape, patch: int, tubelet: Optional[int], dtype: torch.dtype) -> Tensor:
    """The one caller of the patch gather (csrc/patchify.hip) in both directions: allocate, time, launch dvt_<what>.
    ``shape`` is the clip's; ``src`` is the clip (forward) or dout (``what`` ends in _bwd).  ``tubelet`` None is the
    per-frame pair: the entry points without a pt argument, a clip [..., C, H, W] that needs no frame axis."""
    _need_cuda(src)
    if tubelet is None:
        frames, Cc, H, W = _tubelet_geometry((1, *shape), patch, 1, what)
    else:
        frames, Cc, H, W = _tubelet_geometry(shape, patch, tubelet, what)
    pt = () if tubelet is None else (tubelet,)
    src = src.contiguous()
    if what.endswith("_bwd"):
        if src.numel() != frames * Cc * H * W:
            raise ValueError(f"{what}: dout {tuple(src.shape)} does not hold a clip of shape {tuple(shape)}")
        dst = torch.empty(tuple(shape), dtype=dtype, device=src.device)
    else:
        rows = frames // (tubelet or 1) * (H // patch) * (W // patch)
        dst = torch.empty((rows, (tubelet or 1) * patch * patch * Cc), dtype=dtype, device=src.device)
    with _timed(("hbm", what, src.numel()), src.numel() * src.element_size() + dst.numel() * dst.element_size()):
        L.check(getattr(L.load(), "dvt_" + what)(src.data_ptr(), dt(src), dst.data_ptr(), _DT[dtype], frames, Cc, H, W, patch,
                                                 *pt, _stream()), "dvt_" + what)
    return dst


def patchify(x: Tensor, patch: int, out_dtype: torch.dtype) -> Tensor:
    """[..., C, H, W] -> [frames * n, P*P*C]  (vit.py:90 ordering): the tubelet gather at pt = 1 under its own name."""
    return _patch_gather("patchify", x, x.shape, patch, None, out_dtype)


def patchify_bwd(dout: Tensor, shape, patch: int, dx_dtype: torch.dtype) -> Tensor:
    return _patch_gather("patchify_bwd", dout, shape, patch, None, dx_dtype)


def tubelet_patchify(x: Tensor, patch: int, tubelet: int, out_dtype: torch.dtype) -> Tensor:
    """[..., t, C, H, W] -> [(frames / tubelet) * n, tubelet*P*P*C]: 'b (tau k) c (h p1) (w p2) -> (b tau h w) (k p1 p2 c)'
    (tubelet == 1 is ``patchify``)."""
    return _patch_gather("tubelet_patchify", x, x.shape, patch, tubelet, out_dtype)


def tubelet_patchify_bwd(dout: Tensor, shape, patch: int, tubelet: int, dx_dtype: torch.dtype) -> Tensor:
    """The adjoint (inverse) of ``tubelet_patchify``: dout [(frames / tubelet) * n, tubelet*P*P*C] -> dx of ``shape``."""
    return _patch_gather("tubelet_patchify_bwd", dout, shape, patch, tubelet, dx_dtype)


# ------------------------------------------------------------------ patch dropout (csrc/patch_dropout.hip)
def _index_table(what: str, t: Tensor, rows: Optional[int] = None, cols: Optional[int] = None) -> Tensor:
    """An int32 device matrix (keys, keep or slot) as the kernels take it; ValueError otherwise."""
    if not isinstance(t, Tensor) or t.dtype != torch.int32 or t.dim() != 2:
        raise ValueError(f"{what}: expected a 2-D int32 tensor, got {getattr(t, 'dtype', type(t))} "
                         f"of shape {tuple(getattr(t, 'shape', ()))}")
    if (rows is not None and t.shape[0] != rows) or (cols is not None and t.shape[1] != cols):
        raise ValueError(f"{what}: shape {tuple(t.shape)} where [{'*' if rows is None else rows}, "
                         f"{'*' if cols is None else cols}] is expected")
    _need_cuda(t)
    return t.contiguous()


def keep_select(keys: Tensor, k: int, rows_per: int = 1) -> Tuple[Tensor, Tensor]:
    """keys [R, n] int32 -> (keep [R*rows_per, k] ascending, slot [R*rows_per, n], -1 = dropped): position i is kept iff
    fewer than k positions j have (key_j, j) < (key_i, i) -- the first k of a stable argsort; every row written rows_per
    times (tube masking: R = b, rows_per = t')."""
    keys = _index_table("keep_select: keys", keys)
    R, n = keys.shape
    keep = torch.empty((R * rows_per, k), dtype=torch.int32, device=keys.device)
    slot = torch.empty((R * rows_per, n), dtype=torch.int32, device=keys.device)
    L.check(L.load().dvt_keep_select(keys.data_ptr(), R, n, k, rows_per, keep.data_ptr(), slot.data_ptr(), _stream()),
            "dvt_keep_select")
    return keep, slot


def keep_draw(R: int, n: int, k: int, rng_state: Tensor, call_offset: int, rows_per: int = 1) -> Tuple[Tensor, Tensor]:
    """``keep_select`` on keys that are a pure function of (rng_state on the device, call_offset, row, position): one launch.
    A site takes ceil(R*n / 4) Philox blocks (``functional._rng.take(R * n)``)."""
    _need_cuda(rng_state)
    keep = torch.empty((R * rows_per, k), dtype=torch.int32, device=rng_state.device)
    slot = torch.empty((R * rows_per, n), dtype=torch.int32, device=rng_state.device)
    L.check(L.load().dvt_keep_draw(rng_state.data_ptr(), call_offset, R, n, k, rows_per, keep.data_ptr(), slot.data_ptr(),
                                   None, _stream()), "dvt_keep_draw")
    return keep, slot


def keep_keys(R: int, n: int, rng_state: Tensor, call_offset: int) -> Tensor:
    """The keys [R, n] int32 ``keep_draw`` selects on at the same (rng_state, call_offset)."""
    _need_cuda(rng_state)
    keys = torch.empty((R, n), dtype=torch.int32, device=rng_state.device)
    L.check(L.load().dvt_keep_draw(rng_state.data_ptr(), call_offset, R, n, 1, 1, None, None, keys.data_ptr(), _stream()),
            "dvt_keep_draw")
    return keys


def keep_slots(keep: Tensor, n: int) -> Tensor:
    """slot [S, n] int32 of a caller's keep [S, k]: slot[s, keep[s, i]] = i, -1 elsewhere."""
    keep = _index_table("keep_slots: keep", keep)
    S, k = keep.shape
    slot = torch.empty((S, n), dtype=torch.int32, device=keep.device)
    L.check(L.load().dvt_keep_slots(keep.data_ptr(), S, n, k, slot.data_ptr(), _stream()), "dvt_keep_slots")
    return slot


def patchify_keep(x: Tensor, patch: int, tubelet: int, keep: Tensor, out_dtype: torch.dtype) -> Tensor:
    """[..., t, C, H, W], keep [S, k] -> [S*k, tubelet*P*P*C]: the rows ``keep`` names of ``tubelet_patchify``, read from
    the kept patches only."""
    frames, Cc, H, W = _tubelet_geometry(x.shape, patch, tubelet, "patchify_keep")
    keep = _index_table("patchify_keep: keep", keep, rows=frames // tubelet)
    _need_cuda(x)
    x = x.contiguous()
    k = keep.shape[1]
    out = torch.empty((keep.shape[0] * k, tubelet * patch * patch * Cc), dtype=out_dtype, device=x.device)
    nbytes = out.numel() * (x.element_size() + out.element_size())
    with _timed(("hbm", "patchify_keep", out.numel()), nbytes):
        L.check(L.load().dvt_patchify_keep(x.data_ptr(), dt(x), out.data_ptr(), _DT[out_dtype], keep.data_ptr(), frames, Cc, H,
                                           W, patch, tubelet, k, _stream()), "dvt_patchify_keep")
    return out


def patchify_keep_bwd(dout: Tensor, shape, patch: int, tubelet: int, slot: Tensor, dx_dtype: torch.dtype) -> Tensor:
    """The adjoint of ``patchify_keep``: dout [S*k, tubelet*P*P*C], slot [S, n] -> dx of ``shape``, every pixel written once
    (zero where the patch was dropped)."""
    _need_cuda(dout)
    frames, Cc, H, W = _tubelet_geometry(shape, patch, tubelet, "patchify_keep_bwd")
    if H % patch or W % patch:
        raise ValueError(f"patchify_keep_bwd: image {H}x{W} is not divisible by patch {patch}")
    slot = _index_table("patchify_keep_bwd: slot", slot, rows=frames // tubelet, cols=(H // patch) * (W // patch))
    dout = dout.contiguous()
    cols = tubelet * patch * patch * Cc
    if dout.dim() != 2 or dout.shape[1] != cols or dout.shape[0] % slot.shape[0] or dout.shape[0] == 0:
        raise ValueError(f"patchify_keep_bwd: dout {tuple(dout.shape)} is not [S*k, {cols}] for S = {slot.shape[0]}")
    k = dout.shape[0] // slot.shape[0]
    dx = torch.empty(tuple(shape), dtype=dx_dtype, device=dout.device)
    nbytes = dout.numel() * dout.element_size() + dx.numel() * dx.element_size()
    with _timed(("hbm", "patchify_keep_bwd", dout.numel()), nbytes):
        L.check(L.load().dvt_patchify_keep_bwd(dout.data_ptr(), dt(dout), dx.data_ptr(), _DT[dx_dtype], slot.data_ptr(), frames,
                                               Cc, H, W, patch, tubelet, k, _stream()), "dvt_patchify_keep_bwd")
    return dx


def tokens_assemble_keep_fwd(emb: Tensor, cls: Tensor, pos: Tensor, keep: Tensor) -> Tensor:
    """emb [S*k, d]; cls [d] f32; pos [T, rows >= n+1, d] f32; keep [S, k] -> [S, k+1, d]:
    out[s, 0] = cls + pos[s % T, 0], out[s, 1+i] = emb[s*k + i] + pos[s % T, 1 + keep[s, i]]."""
    _need_cuda(emb, cls, pos)
    keep = _index_table("tokens_assemble_keep_fwd: keep", keep)
    S, k = keep.shape
    d = emb.shape[-1]
    assert emb.is_contiguous() and cls.is_contiguous() and pos.is_contiguous()
    assert cls.dtype == torch.float32 and pos.dtype == torch.float32 and pos.dim() == 3
    if emb.numel() != S * k * d:
        raise ValueError(f"tokens_assemble_keep_fwd: emb {tuple(emb.shape)} does not hold [S*k, d] for keep {tuple(keep.shape)}")
    T, pos_rows = pos.shape[0], pos.shape[1]
    out = torch.empty((S, k + 1, d), dtype=emb.dtype, device=emb.device)
    with _timed(("hbm", "tokens_assemble_keep_fwd", emb.numel()), (emb.numel() + 2 * out.numel()) * emb.element_size()):
        L.check(L.load().dvt_tokens_assemble_keep_fwd(emb.data_ptr(), cls.data_ptr(), pos.data_ptr(), keep.data_ptr(),
                                                      out.data_ptr(), S, T, pos_rows - 1, k, d, pos_rows, dt(emb), _stream()),
                "dvt_tokens_assemble_keep_fwd")
    return out


def tokens_assemble_keep_bwd(dout: Tensor, T: int, pos_rows: int, slot: Tensor, *, dcls: Optional[Tensor] = None,
                             dpos: Optional[Tensor] = None, accumulate: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """dout [S, k+1, d], slot [S, n] -> (demb [S*k, d], dcls [d], dpos [T, pos_rows, d]); dcls / dpos may be caller-owned
    fp32 destinations (gradient sinks).  A positional row nobody kept gets exactly zero when overwriting and stays as it is
    when accumulating.  Deterministic: the sum over the clips of a position runs in ascending clip order."""
    _need_cuda(dout)
    dout = dout.contiguous()
    S, k1, d = dout.shape
    k = k1 - 1
    slot = _index_table("tokens_assemble_keep_bwd: slot", slot, rows=S)
    n = slot.shape[1]
    if pos_rows < n + 1:
        raise ValueError(f"tokens_assemble_keep_bwd: the positional table has {pos_rows} rows < n + 1 = {n + 1}")
    demb = torch.empty((S * k, d), dtype=dout.dtype, device=dout.device)
    if dcls is None:
        assert not accumulate
        dcls = torch.empty((d,), dtype=torch.float32, device=dout.device)
    if dpos is None:
        assert not accumulate
        dpos = torch.empty((T, pos_rows, d), dtype=torch.float32, device=dout.device)
    assert dcls.is_contiguous() and dpos.is_contiguous() and dcls.numel() == d and dpos.numel() == T * pos_rows * d
    L.check(L.load().dvt_tokens_assemble_keep_bwd(dout.data_ptr(), slot.data_ptr(), demb.data_ptr(), dcls.data_ptr(),
                                                  dpos.data_ptr(), S, T, n, k, d, pos_rows, dt(dout), int(accumulate),
                                                  _stream()), "dvt_tokens_assemble_keep_bwd")
    return demb, dcls, dpos


# ------------------------------------------------------------------ stochastic depth (csrc/drop_path.hip)
DROP_PATH_MAX_SEQS = 1024          # sequences a fixed-size subset is drawn from: keep_draw holds the selection in LDS


def _seq_index(what: str, t: Tensor, count: Optional[int], like: Tensor) -> Tensor:
    """A 1-D int32 device vector of sequence indices (idx, slot or a Bernoulli draw); ValueError otherwise."""
    if not isinstance(t, Tensor) or t.dtype != torch.int32 or t.dim() != 1 or t.numel() < 1:
        raise ValueError(f"{what}: expected a non-empty 1-D int32 tensor, got {getattr(t, 'dtype', type(t))} "
                         f"of shape {tuple(getattr(t, 'shape', ()))}")
    if count is not None and t.numel() != count:
        raise ValueError(f"{what}: {t.numel()} entries where {count} are expected")
    if t.device != like.device:
        raise ValueError(f"{what}: on {t.device}, the data on {like.device}")
    return t.contiguous()


def _seq_rows(what: str, x: Tensor) -> Tuple[int, int]:
    if not isinstance(x, Tensor) or x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"{what}: expected [S, ...] with at least two dimensions and no empty one, got "
                         f"{tuple(getattr(x, 'shape', ()))}")
    if x.dtype not in _DT:
        raise ValueError(f"{what}: dtype {x.dtype} is not float32, bfloat16 or float16")
    return x.shape[0], x.numel() // x.shape[0]


def seq_gather(x: Tensor, idx: Tensor, alpha: float = 1.0) -> Tensor:
    """x [S, ...], idx [k] int32 -> y [k, ...]: y[j] = alpha * x[idx[j]] where 0 <= idx[j] < S, a row of zeros otherwise
    (-1 = dropped)."""
    S, L_ = _seq_rows("seq_gather: x", x)
    idx = _seq_index("seq_gather: idx", idx, None, x)
    _need_cuda(x, idx)
    x = x.contiguous()
    k = idx.numel()
    y = torch.empty((k,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    with _timed(("hbm", "seq_gather", y.numel()), 2 * y.numel() * y.element_size()):
        L.check(L.load().dvt_seq_gather(x.data_ptr(), idx.data_ptr(), y.data_ptr(), S, k, L_, float(alpha), dt(x), _stream()),
                "dvt_seq_gather")
    return y


def seq_scatter_add(res: Tensor, y: Tensor, slot: Tensor, alpha: float = 1.0, out: Optional[Tensor] = None) -> Tensor:
    """res [S, ...], y [k, ...], slot [S] int32 -> out [S, ...]: out[s] = res[s] + alpha * y[slot[s]] where
    0 <= slot[s] < k, res[s] otherwise.  The adjoint of ``seq_gather``.  ``out`` may be ``res`` itself (in place)."""
    S, L_ = _seq_rows("seq_scatter_add: res", res)
    k, Ly = _seq_rows("seq_scatter_add: y", y)
    if Ly != L_ or y.dtype != res.dtype or y.device != res.device:
        raise ValueError(f"seq_scatter_add: y {tuple(y.shape)} {y.dtype} on {y.device} does not hold rows of res "
                         f"{tuple(res.shape)} {res.dtype} on {res.device}")
    slot = _seq_index("seq_scatter_add: slot", slot, S, res)
    if out is not None and (not isinstance(out, Tensor) or out.shape != res.shape or out.dtype != res.dtype
                            or out.device != res.device or not out.is_contiguous() or not res.is_contiguous()):
        raise ValueError("seq_scatter_add: out must be a contiguous tensor of res's shape, dtype and device "
                         "(and res contiguous)")
    _need_cuda(res, y, slot)
    if out is None:
        res = res.contiguous()
        out = torch.empty_like(res)
    y = y.contiguous()
    nbytes = (2 * res.numel() + y.numel()) * res.element_size()
    with _timed(("hbm", "seq_scatter_add", res.numel()), nbytes):
        L.check(L.load().dvt_seq_scatter_add(res.data_ptr(), y.data_ptr(), slot.data_ptr(), out.data_ptr(), S, k, L_,
                                             float(alpha), dt(res), _stream()), "dvt_seq_scatter_add")
    return out


def drop_path_draw(S: int, p: float, rng_state: Tensor, call_offset: int) -> Tensor:
    """m [S] int32: m[s] = s with probability 1 - p, else -1 -- a pure function of (rng_state on the device, call_offset,
    s).  A site takes ceil(S / 4) Philox blocks (``functional._rng.take(S)``)."""
    if isinstance(S, bool) or not isinstance(S, int) or S < 1:
        raise ValueError(f"drop_path_draw: S must be an integer >= 1, got {S!r}")
    if not 0.0 <= p < 1.0:
        raise ValueError(f"drop_path_draw: p must be in [0, 1), got {p!r}")
    _need_cuda(rng_state)
    m = torch.empty((S,), dtype=torch.int32, device=rng_state.device)
    with _timed(("hbm", "drop_path_draw", S), 4 * S):
        L.check(L.load().dvt_drop_path_draw(rng_state.data_ptr(), call_offset, S, float(p), m.data_ptr(), _stream()),
                "dvt_drop_path_draw")
    return m


# ------------------------------------------------------------------ masked-autoencoder pre-training (csrc/mae.hip)
def _restore_geometry(what: str, t: Tensor, slot: Tensor, rows: Optional[int]):
    """(S, n, d) of a row tensor [S, rows or any, d] against slot [S, n]; ValueError on a mismatch or d % 8 != 0."""
    if not isinstance(t, Tensor) or t.dim() != 3 or t.dtype not in _DT or t.numel() == 0:
        raise ValueError(f"{what}: expected a non-empty [S, rows, d] tensor in float32 / bfloat16 / float16, got "
                         f"{getattr(t, 'dtype', type(t))} of shape {tuple(getattr(t, 'shape', ()))}")
    S, r, d = t.shape
    if d % 8:
        raise ValueError(f"{what}: d = {d} must be a multiple of 8")
    slot = _index_table(f"{what}: slot", slot, rows=S)
    if rows is not None and r != rows:
        raise ValueError(f"{what}: {r} rows per sequence where {rows} are expected")
    return S, slot.shape[1], d, slot


def tokens_restore_fwd(y: Tensor, mask: Tensor, pos: Tensor, slot: Tensor, k: int, skip: int = 1) -> Tensor:
    """y [S, skip + k, d]; mask [d] f32; pos [T, n, d] f32; slot [S, n] -> out [S, n, d] in y's type:
    out[s, j] = (y[s, skip + slot[s, j]] if slot[s, j] >= 0 else mask) + pos[s % T, j]."""
    S, n, d, slot = _restore_geometry("tokens_restore_fwd", y, slot, None)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= n or skip < 0 or y.shape[1] != skip + k:
        raise ValueError(f"tokens_restore_fwd: y {tuple(y.shape)} does not hold skip + k = {skip} + {k} rows per sequence "
                         f"with 1 <= k <= n = {n}")
    if (mask.dtype != torch.float32 or pos.dtype != torch.float32 or mask.numel() != d or pos.dim() != 3
            or tuple(pos.shape[1:]) != (n, d) or S % pos.shape[0]):
        raise ValueError(f"tokens_restore_fwd: mask {tuple(mask.shape)} {mask.dtype} / pos {tuple(pos.shape)} {pos.dtype} "
                         f"where float32 [{d}] and [T, {n}, {d}] with T dividing S = {S} are expected")
    _need_cuda(y, mask, pos)
    assert y.is_contiguous() and mask.is_contiguous() and pos.is_contiguous()
    out = torch.empty((S, n, d), dtype=y.dtype, device=y.device)
    nbytes = (S * k * d + out.numel()) * y.element_size() + (pos.numel() + d) * 4 + slot.numel() * 4
    with _timed(("hbm", "tokens_restore_fwd", out.numel()), nbytes):
        L.check(L.load().dvt_tokens_restore_fwd(y.data_ptr(), mask.data_ptr(), pos.data_ptr(), slot.data_ptr(), out.data_ptr(),
                                                S, pos.shape[0], n, k, skip, d, dt(y), _stream()), "dvt_tokens_restore_fwd")
    return out


def tokens_restore_bwd(dout: Tensor, keep: Tensor, slot: Tensor, T: int, skip: int = 1, *, dmask: Optional[Tensor] = None,
                       dpos: Optional[Tensor] = None, accumulate: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """dout [S, n, d], keep [S, k], slot [S, n] -> (dy [S, skip + k, d], dmask [d], dpos [T, n, d]); dmask / dpos may be
    caller-owned fp32 destinations (gradient sinks).  dy[s, skip + i] = dout[s, keep[s, i]] with zero skip rows; dmask sums
    the dropped rows, dpos every row of its position in ascending clip order.  Deterministic."""
    S, n, d, slot = _restore_geometry("tokens_restore_bwd", dout, slot, None)
    if dout.shape[1] != n:
        raise ValueError(f"tokens_restore_bwd: dout {tuple(dout.shape)} for slot {tuple(slot.shape)}")
    keep = _index_table("tokens_restore_bwd: keep", keep, rows=S)
    k = keep.shape[1]
    if not 1 <= k <= n or skip < 0 or T < 1 or S % T:
        raise ValueError(f"tokens_restore_bwd: k = {k}, n = {n}, skip = {skip}, T = {T}, S = {S}")
    _need_cuda(dout)
    dout = dout.contiguous()
    dy = torch.empty((S, skip + k, d), dtype=dout.dtype, device=dout.device)
    if dmask is None:
        assert not accumulate
        dmask = torch.empty((d,), dtype=torch.float32, device=dout.device)
    if dpos is None:
        assert not accumulate
        dpos = torch.empty((T, n, d), dtype=torch.float32, device=dout.device)
    assert dmask.is_contiguous() and dpos.is_contiguous() and dmask.numel() == d and dpos.numel() == T * n * d
    assert dmask.dtype == torch.float32 and dpos.dtype == torch.float32
    partial = workspace(T * n * d * 4, dout.device, slot="mae")
    nbytes = (dout.numel() + dy.numel()) * dout.element_size() + (3 + int(accumulate)) * T * n * d * 4 + slot.numel() * 4
    with _timed(("hbm", "tokens_restore_bwd", dout.numel()), nbytes):
        L.check(L.load().dvt_tokens_restore_bwd(dout.data_ptr(), keep.data_ptr(), slot.data_ptr(), dy.data_ptr(),
                                                dmask.data_ptr(), dpos.data_ptr(), partial.data_ptr(), S, T, n, k, skip, d,
                                                dt(dout), int(accumulate), _stream()), "dvt_tokens_restore_bwd")
    return dy, dmask, dpos


MAE_EPS = 1e-6                     # the epsilon of the per-patch normalised target (MAE / MAE-ST)


def _mae_geometry(what: str, pred: Tensor, clip: Tensor, slot: Tensor, k: int, patch: int, tubelet: int):
    frames, Cc, H, W = _tubelet_geometry(clip.shape, patch, tubelet, what)
    if isinstance(patch, bool) or not isinstance(patch, int) or patch < 1 or H % patch or W % patch:
        raise ValueError(f"{what}: image {H}x{W} is not divisible by patch {patch!r}")
    S, n, D = frames // tubelet, (H // patch) * (W // patch), tubelet * patch * patch * Cc
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k < n:
        raise ValueError(f"{what}: k = {k!r} must satisfy 1 <= k < n = {n}: no masked patch (M == 0) or no kept one")
    if (not isinstance(pred, Tensor) or pred.dtype not in _DT or clip.dtype not in _DT or pred.numel() != S * n * D
            or pred.shape[-1] != D):
        raise ValueError(f"{what}: pred {tuple(getattr(pred, 'shape', ()))} {getattr(pred, 'dtype', type(pred))} does not "
                         f"hold [{S}, {n}, {D}] for a clip {tuple(clip.shape)} {clip.dtype}")
    slot = _index_table(f"{what}: slot", slot, rows=S, cols=n)
    _need_cuda(pred, clip)
    return frames, Cc, H, W, S, n, D, slot


def mae_loss_fwd(pred: Tensor, clip: Tensor, slot: Tensor, k: int, patch: int, tubelet: int, norm_pix: bool,
                 eps: float = MAE_EPS):
    """pred [S, n, D], clip [b, t, C, H, W] (its own dtype), slot [S, n] -> (loss f32 [1], per_patch f32 [S, n], stats f32
    [S, n, 2] or None): the mean over the S (n - k) dropped patches of mean_D (pred - target)^2, the target read from the
    clip in the tubelet gather's order (per-patch normalised, unbiased variance, under ``norm_pix``)."""
    frames, Cc, H, W, S, n, D, slot = _mae_geometry("mae_loss_fwd", pred, clip, slot, k, patch, tubelet)
    pred, clip = pred.contiguous(), clip.contiguous()
    per_patch = torch.empty((S, n), dtype=torch.float32, device=pred.device)
    stats = torch.empty((S, n, 2), dtype=torch.float32, device=pred.device) if norm_pix else None
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    masked = S * (n - k) * D
    nbytes = masked * (pred.element_size() + clip.element_size()) + S * n * (8 + (8 if norm_pix else 0))
    with _timed(("hbm", "mae_loss_fwd", masked), nbytes):
        L.check(L.load().dvt_mae_loss_fwd(pred.data_ptr(), dt(pred), clip.data_ptr(), dt(clip), slot.data_ptr(),
                                          per_patch.data_ptr(), _p(stats), loss.data_ptr(), frames, Cc, H, W, patch, tubelet, k,
                                          int(bool(norm_pix)), float(eps), _stream()), "dvt_mae_loss_fwd")
    return loss, per_patch, stats


def mae_loss_bwd(pred: Tensor, clip: Tensor, slot: Tensor, k: int, patch: int, tubelet: int, stats: Optional[Tensor],
                 gloss: Tensor) -> Tensor:
    """dpred [S, n, D] in pred's type = gloss * 2 / (M D) * (pred - target) at dropped positions, exact zeros at kept ones;
    ``gloss`` is a device f32 scalar, ``stats`` the forward's (None without norm_pix)."""
    frames, Cc, H, W, S, n, D, slot = _mae_geometry("mae_loss_bwd", pred, clip, slot, k, patch, tubelet)
    _need_cuda(gloss)
    assert gloss.dtype == torch.float32 and gloss.numel() == 1
    assert stats is None or (stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == 2 * S * n)
    pred, clip = pred.contiguous(), clip.contiguous()
    dpred = torch.empty((S, n, D), dtype=pred.dtype, device=pred.device)
    masked = S * (n - k) * D
    nbytes = (masked + S * n * D) * pred.element_size() + masked * clip.element_size() + S * n * (4 + (8 if stats is not None else 0))
    with _timed(("hbm", "mae_loss_bwd", masked), nbytes):
        L.check(L.load().dvt_mae_loss_bwd(pred.data_ptr(), dt(pred), clip.data_ptr(), dt(clip), slot.data_ptr(), _p(stats),
                                          gloss.data_ptr(), dpred.data_ptr(), frames, Cc, H, W, patch, tubelet, k,
                                          int(stats is not None), _stream()), "dvt_mae_loss_bwd")
    return dpred


def tokens_assemble_fwd(emb: Tensor, cls: Tensor, pos: Tensor, S: int, T: int, n: int) -> Tensor:
    """emb [S*n, d]; cls [d] f32; pos [T, rows>=n+1, d] f32 -> [S, n+1, d]."""
    _need_cuda(emb, cls, pos)
    d = emb.shape[-1]
    assert emb.is_contiguous() and cls.is_contiguous() and pos.is_contiguous()
    assert cls.dtype == torch.float32 and pos.dtype == torch.float32
    out = torch.empty((S, n + 1, d), dtype=emb.dtype, device=emb.device)
    with _timed(("hbm", "tokens_assemble_fwd", emb.numel()), (emb.numel() + out.numel()) * emb.element_size() + pos.numel() * 4):
        L.check(L.load().dvt_tokens_assemble_fwd(emb.data_ptr(), cls.data_ptr(), pos.data_ptr(), out.data_ptr(), S, T,
                                                 n, d, pos.shape[-2], dt(emb), _stream()), "dvt_tokens_assemble_fwd")
    return out


def tokens_assemble_bwd(dout: Tensor, T: int, pos_rows: int, *, dcls: Optional[Tensor] = None,
                        dpos: Optional[Tensor] = None, accumulate: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """dcls / dpos may be caller-owned fp32 destinations (gradient sinks)."""
    _need_cuda(dout)
    dout = dout.contiguous()
    S, n1, d = dout.shape
    n = n1 - 1
    demb = torch.empty((S * n, d), dtype=dout.dtype, device=dout.device)
    if dcls is None:
        assert not accumulate
        dcls = torch.empty((d,), dtype=torch.float32, device=dout.device)
    if dpos is None:
        assert not accumulate
        dpos = torch.empty((T, pos_rows, d), dtype=torch.float32, device=dout.device)
    assert dcls.is_contiguous() and dpos.is_contiguous() and dcls.numel() == d and dpos.numel() == T * pos_rows * d
    L.check(L.load().dvt_tokens_assemble_bwd(dout.data_ptr(), demb.data_ptr(), dcls.data_ptr(), dpos.data_ptr(), S,
                                             T, n, d, pos_rows, dt(dout), int(accumulate), _stream()),
            "dvt_tokens_assemble_bwd")
    return demb, dcls, dpos


def rows_gather_fwd(src: Tensor, row_stride: int, tok: Optional[Tensor], B: int, T: int, d: int) -> Tensor:
    _need_cuda(src, tok)
    lead = 0 if tok is None else 1
    out = torch.empty((B, T + lead, d), dtype=src.dtype, device=src.device)
    L.check(L.load().dvt_rows_gather_fwd(src.data_ptr(), row_stride, _p(tok), out.data_ptr(), B, T, d, dt(src),
                                         _stream()), "dvt_rows_gather_fwd")
    return out


def rows_gather_bwd(dout: Tensor, dsrc: Tensor, row_stride: int, want_tok: bool, B: int, T: int,
                    d: int, *, dtok: Optional[Tensor] = None, accumulate: bool = False) -> Optional[Tensor]:
    """Scatters dout rows into ``dsrc`` (pre-zeroed by the caller where needed)."""
    _need_cuda(dout, dsrc)
    dout = dout.contiguous()
    if want_tok and dtok is None:
        assert not accumulate
        dtok = torch.empty((d,), dtype=torch.float32, device=dout.device)
    if not want_tok:
        dtok = None
    L.check(L.load().dvt_rows_gather_bwd(dout.data_ptr(), dsrc.data_ptr(), row_stride, _p(dtok), B, T, d, dt(dout),
                                         int(accumulate), _stream()), "dvt_rows_gather_bwd")
    return dtok


def mean_rows_fwd(x: Tensor, scale: Optional[float] = None) -> Tensor:
    """[B, L, d] -> [B, d]: scale * sum over L (default scale 1/L = mean)."""
    _need_cuda(x)
    x = x.contiguous()
    B, Ln, d = x.shape
    out = torch.empty((B, d), dtype=x.dtype, device=x.device)
    sc = 1.0 / Ln if scale is None else scale
    L.check(L.load().dvt_mean_rows_fwd(x.data_ptr(), out.data_ptr(), B, Ln, d, sc, dt(x), _stream()),
            "dvt_mean_rows_fwd")
    return out


def mean_rows_bwd(dout: Tensor, Ln: int, scale: Optional[float] = None) -> Tensor:
    _need_cuda(dout)
    dout = dout.contiguous()
    B, d = dout.shape
    dx = torch.empty((B, Ln, d), dtype=dout.dtype, device=dout.device)
    sc = 1.0 / Ln if scale is None else scale
    L.check(L.load().dvt_mean_rows_bwd(dout.data_ptr(), dx.data_ptr(), B, Ln, d, sc, dt(dout), _stream()),
            "dvt_mean_rows_bwd")
    return dx


# ------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x: Tensor, gamma: Tensor, beta: Tensor, eps: float = 1e-5, *, rows=None,
                  out: Optional[Tensor] = None, out_rows=None, out_dtype: Optional[torch.dtype] = None
                  ) -> Tuple[Tensor, Tensor, Tensor]:
    """Dense (rows is None): x [..., d] contiguous -> y like x.
    Strided: rows = (n0, n1, xs0, xs1) selects row (i0,i1) of ``x`` at element
    i0*xs0 + i1*xs1; the output row goes to ``out`` at i0*ys0 + i1*ys1 with
    out_rows = (ys0, ys1) (default: a dense [n0*n1, d] tensor).
    out_dtype: element type of y when it differs from x's (fp32 stream <-> 16-bit GEMM operand, see dvt_layernorm_fwd_mixed)."""
    _need_cuda(x, gamma, beta)
    d = x.shape[-1]
    ydt = x.dtype if out_dtype is None else out_dtype
    if rows is None:
        assert x.is_contiguous()
        n0, n1, xs0, xs1 = x.numel() // d, 1, d, 0
        if out is None:
            out = torch.empty(x.shape, dtype=ydt, device=x.device)
        ys0, ys1 = d, 0
    else:
        n0, n1, xs0, xs1 = rows
        if out is None:
            out = torch.empty((n0 * n1, d), dtype=ydt, device=x.device)
        ys0, ys1 = out_rows if out_rows is not None else (n1 * d, d)
    assert out.dtype == ydt
    nrows = n0 * n1
    mean = torch.empty((nrows,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((nrows,), dtype=torch.float32, device=x.device)
    with _timed(("hbm", "layernorm_fwd", nrows), nrows * (d * (x.element_size() + out.element_size()) + 8)):
        L.check(L.load().dvt_layernorm_fwd_mixed(x.data_ptr(), dt(x), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                                                 dt(out), mean.data_ptr(), rstd.data_ptr(), n0, n1, d, xs0, xs1, ys0, ys1,
                                                 eps, _stream()), "dvt_layernorm_fwd")
    return out, mean, rstd


# dgamma / dbeta reduces left undone by layernorm_bwd(defer=...): (pending descriptor, callback) pairs, performed by ONE
# launch in layernorm_flush() -- the launch-bound zone of the step has a dozen LayerNorms whose reduces were a launch each
_ln_deferred = []
LN_DEFER_MAX = 24


def layernorm_flush() -> None:
    """Perform every deferred dgamma / dbeta reduce (one launch per 32) and run their completion callbacks."""
    global _ln_deferred
    if not _ln_deferred:
        return
    todo, _ln_deferred = _ln_deferred, []
    arr = (L.LnPending * len(todo))(*[pn for pn, _ in todo])
    L.check(L.load().dvt_layernorm_reduce_group(arr, len(todo), _stream()), "dvt_layernorm_reduce_group")
    for pn, done in todo:
        pn.valid = 0
        if done is not None:
            done()


def layernorm_bwd(dy: Tensor, x: Tensor, gamma: Tensor, mean: Tensor, rstd: Tensor, *,
                  dx_add: Optional[Tensor] = None, rows=None, dy_rows=None,
                  dx: Optional[Tensor] = None, dg: Optional[Tensor] = None, db: Optional[Tensor] = None,
                  accumulate: bool = False, accumulate_beta: Optional[bool] = None,
                  dy_first: Optional[Tensor] = None, dx_first: Optional[Tensor] = None,
                  dx_dtype: Optional[torch.dtype] = None, dx_lp: Optional[torch.dtype] = None, defer=None):
    """``accumulate`` applies to dgamma (and to dbeta unless ``accumulate_beta`` is given).
    ``dy_first`` / ``dx_first`` [n0, d] (row stride free): added to dy / dx of row (i0, 0) only.
    Element types: dy's, x's and dx's (``dx_dtype``, default x's) may differ as dvt_layernorm_bwd_ex allows; ``dx_lp``: also
    return a copy of dx in that 16-bit type (-> (dx, dg, db, dx_copy)).  ``defer``: a callable (or True): the dgamma / dbeta
    reduce is left to ``layernorm_flush()`` (one launch for many layers), which calls it when dg / db are final."""
    _need_cuda(dy, x, gamma, mean, rstd, dx_add, dy_first, dx_first)
    d = x.shape[-1]
    if rows is None:
        assert x.is_contiguous() and dy.is_contiguous()
        n0, n1, xs0, xs1 = x.numel() // d, 1, d, 0
        ys0, ys1 = d, 0
    else:
        n0, n1, xs0, xs1 = rows
        ys0, ys1 = dy_rows if dy_rows is not None else (d * n1, d)
    dxt = x.dtype if dx_dtype is None else dx_dtype
    assert dy_first is None or (dy_first.dim() == 2 and dy_first.shape == (n0, d) and dy_first.stride(1) == 1 and dy_first.dtype == dy.dtype)
    assert dx_first is None or (dx_first.dim() == 2 and dx_first.shape == (n0, d) and dx_first.stride(1) == 1 and dx_first.dtype == dxt)
    if dx is None:
        dx = torch.empty(x.shape, dtype=dxt, device=x.device)
    assert dx.dtype == dxt and (dx_add is None or dx_add.dtype == dxt)
    if dg is None or db is None:
        assert not accumulate and not accumulate_beta and dg is None and db is None
        dg = torch.empty((d,), dtype=torch.float32, device=x.device)
        db = torch.empty((d,), dtype=torch.float32, device=x.device)
    acc_b = accumulate if accumulate_beta is None else accumulate_beta
    lib = L.load()
    q = L.LnBwdDesc()
    q.dy, q.dy_dtype, q.x, q.x_dtype = dy.data_ptr(), dt(dy), x.data_ptr(), dt(x)
    q.gamma, q.mean, q.rstd = gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr()
    q.dx_add, q.dx, q.dx_dtype = _p(dx_add), dx.data_ptr(), _DT[dxt]
    lp = None
    if dx_lp is not None:
        lp = torch.empty(x.shape, dtype=dx_lp, device=x.device)
        q.dx_lp, q.dx_lp_dtype = lp.data_ptr(), _DT[dx_lp]
    q.dgamma, q.dbeta = dg.data_ptr(), db.data_ptr()
    q.n0, q.n1, q.d, q.xs0, q.xs1, q.ys0, q.ys1 = n0, n1, d, xs0, xs1, ys0, ys1
    q.dy_first, q.dy_first_stride = _p(dy_first), dy_first.stride(0) if dy_first is not None else 0
    q.dx_first, q.dx_first_stride = _p(dx_first), dx_first.stride(0) if dx_first is not None else 0
    q.accumulate_gamma, q.accumulate_beta = int(accumulate), int(acc_b)
    pending = None
    if defer:
        # the partial rows must outlive this call: a buffer of their own, kept alive by the pending record
        ws = torch.empty((lib.dvt_layernorm_bwd_partial_bytes(n0 * n1, d),), dtype=torch.uint8, device=x.device)
        pending = L.LnPending()
        pending._keep = (ws, dg, db)
        q.defer_reduce, q.pending = 1, C.pointer(pending)
    else:
        ws = workspace(lib.dvt_layernorm_bwd_workspace_bytes(d), x.device)
    q.workspace = ws.data_ptr()
    nb = n0 * n1 * (d * (dy.element_size() + x.element_size() + dx.element_size() * (1 + (dx_add is not None))) + 8)
    with _timed(("hbm", "layernorm_bwd", n0 * n1), nb):
        L.check(lib.dvt_layernorm_bwd_ex(C.byref(q), _stream()), "dvt_layernorm_bwd")
    if defer:
        _ln_deferred.append((pending, defer if callable(defer) else None))
        if len(_ln_deferred) >= LN_DEFER_MAX:
            layernorm_flush()
    return (dx, dg, db) if dx_lp is None else (dx, dg, db, lp)


# ------------------------------------------------------------------ GEMM family
def _gemm_desc(A: Tensor, B: Tensor, M: int, N: int, K: int, *, a_kmajor: bool, b_kmajor: bool, lda: int, ldb: int,
               out: Optional[Tensor] = None, out_dtype: Optional[torch.dtype] = None, epilogue: int = L.EPI_NONE,
               bias: Optional[Tensor] = None, residual: Optional[Tensor] = None, aux: Optional[Tensor] = None,
               accumulate: bool = False, alpha: float = 1.0, split_k: int = 0, colsum_out: Optional[Tensor] = None,
               colsum_accumulate: bool = False, _launch: bool = True):
    """-> (dvt_gemm_desc, out): argument checks, output allocation and descriptor of one product (``_launch`` False: for
    a plan query, tensors on any device)."""
    if _launch:
        _need_cuda(A, B, bias, residual, aux)
    assert A.dtype == B.dtype
    if out_dtype is None:
        out_dtype = A.dtype
    if out is None:
        assert not accumulate
        out = torch.empty((M, N), dtype=out_dtype, device=A.device)
    assert out.dtype == out_dtype and out.stride(-1) == 1
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == N
    d = L.GemmDesc()
    if residual is not None and residual.dtype != A.dtype:      # fp32 residual stream behind 16-bit operands (dvt_gemm_desc.residual_f32)
        assert residual.dtype == torch.float32 and out_dtype == torch.float32 and epilogue == L.EPI_RESIDUAL
        d.residual_f32 = 1
    d.A, d.B, d.C = A.data_ptr(), B.data_ptr(), out.data_ptr()
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = lda, ldb, out.stride(0) if out.dim() == 2 else N
    d.a_kmajor, d.b_kmajor = int(a_kmajor), int(b_kmajor)
    d.in_dtype, d.out_dtype = dt(A), _DT[out_dtype]
    d.epilogue, d.accumulate = epilogue, int(accumulate)
    d.bias = _p(bias)
    d.residual = _p(residual)
    d.ldr = residual.stride(0) if residual is not None else 0
    d.aux = _p(aux)
    d.ldaux = aux.stride(0) if aux is not None else 0
    d.alpha = alpha
    d.split_k = split_k
    if colsum_out is not None:
        assert colsum_out.dtype == torch.float32 and colsum_out.numel() == M and colsum_out.is_contiguous()
    d.colsum_out = _p(colsum_out)
    d.colsum_accumulate = int(colsum_accumulate)
    return d, out


def gemm(A: Tensor, B: Tensor, M: int, N: int, K: int, *, a_kmajor: bool, b_kmajor: bool,
         lda: int, ldb: int, out: Optional[Tensor] = None, out_dtype: Optional[torch.dtype] = None,
         epilogue: int = L.EPI_NONE, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
         aux: Optional[Tensor] = None, accumulate: bool = False, alpha: float = 1.0,
         split_k: int = 0, colsum_out: Optional[Tensor] = None, colsum_accumulate: bool = False,
         defer_reduce: bool = False, carry=None):
    """defer_reduce: a split-K reduce this call would launch is left undone and returned as a pending descriptor --
    (out, pending) -- for the ``carry=`` argument of the NEXT gemm call on this stream (the data gradient of the same
    Linear), which performs it in the idle tail of its own launch; ``out`` is complete only after that call."""
    d, out = _gemm_desc(A, B, M, N, K, a_kmajor=a_kmajor, b_kmajor=b_kmajor, lda=lda, ldb=ldb, out=out, out_dtype=out_dtype,
                        epilogue=epilogue, bias=bias, residual=residual, aux=aux, accumulate=accumulate, alpha=alpha,
                        split_k=split_k, colsum_out=colsum_out, colsum_accumulate=colsum_accumulate)
    out_dtype = out.dtype
    pending = None
    if defer_reduce:
        pending = L.SplitKPending()
        pending._keep = (out, colsum_out)          # the descriptor names their storage
        d.defer_reduce = 1
        d.pending = C.pointer(pending)
    if carry is not None:
        d.carry = C.pointer(carry)
    lib = L.load()
    # the slabs of a deferred reduce must survive the next call: they get a scratch slot of their own
    nws = lib.dvt_gemm_workspace_bytes(C.byref(d))
    ws = _deferred_workspace(nws, A.device, pending) if defer_reduce else workspace(nws, A.device)
    d.workspace = _p(ws)
    if defer_reduce:
        pending._keep += (ws,)
    prof = _profiler
    if prof is not None:
        # algorithmic bytes of the launch: both operands once, every output once, every extra epilogue operand once
        esz, osz = A.element_size(), out.element_size()
        nbytes = esz * (M * K + N * K) + osz * M * N * (2 if accumulate else 1)
        nbytes += esz * M * N * ((residual is not None) + (aux is not None))
        key = ("gemm", int(a_kmajor), int(b_kmajor), M, N, K, epilogue, nbytes)
        prof.begin(key, 2.0 * M * N * K)
        L.check(lib.dvt_gemm(C.byref(d), _stream()), "dvt_gemm")
        prof.end(key)
        return (out, pending) if defer_reduce else out
    L.check(lib.dvt_gemm(C.byref(d), _stream()), "dvt_gemm")
    return (out, pending) if defer_reduce else out


class GemmPlan(NamedTuple):
    """What one dvt_gemm call launches (dvt_gemm_plan): the kernel family, its LDS-DMA configuration (-1: none), the K
    slices and K per slice, the panel kernel's tile rows, what sums the slabs, how colsum_out is produced and what becomes
    of a carried reduce; then the instantiation: operand layouts, epilogue and output form ("in" = the operands' type,
    "f32", "slab" = fp32 split-K partials).  Names: GEMM_KERNELS, GEMM_REDUCES, GEMM_COLSUMS, GEMM_CARRIES, GEMM_OUTS."""
    kernel: str
    cfg: int = -1
    split: int = 1
    k_per_split: int = 0
    tile_m: int = 0
    reduce: str = "none"
    colsum: str = "none"
    carry: str = "none"
    a_kmajor: bool = True
    b_kmajor: bool = True
    epilogue: int = L.EPI_NONE
    out: str = "in"


def _enum_names(enum: str, prefix: str) -> Tuple[str, ...]:
    """The enumerators of a dvt_hip.h enum as lower-cased names without ``prefix`` (a regular expression), indexed by value."""
    names = {v: re.fullmatch(prefix + r"(\w+)", k).group(1).lower() for k, v in L.ENUMS[enum].items()}
    return tuple(names[i] for i in range(len(names)))


GEMM_OUTS = ("in", "f32", "slab")                     # dvt_gemm_plan_info.out_form (no enum in the header)
GEMM_KERNELS = _enum_names("dvt_gemm_kernel", "DVT_GEMM_K_")
GEMM_REDUCES = _enum_names("dvt_gemm_reduce", "DVT_GEMM_R_")
GEMM_COLSUMS = _enum_names("dvt_gemm_colsum", "DVT_GEMM_CS_")
GEMM_CARRIES = _enum_names("dvt_gemm_carry", "DVT_GEMM_CARRY_")


def _plan_tuple(q) -> GemmPlan:
    return GemmPlan(GEMM_KERNELS[q.kernel], q.cfg, q.split, q.k_per_split, q.tile_m, GEMM_REDUCES[q.reduce],
                    GEMM_COLSUMS[q.colsum], GEMM_CARRIES[q.carry], bool(q.a_kmajor), bool(q.b_kmajor), q.epilogue,
                    GEMM_OUTS[q.out_form])


def _plan_desc(A: Tensor, B: Tensor, M: int, N: int, K: int, *, defer_reduce: bool = False, carry=None, **kw):
    """the descriptor ``gemm`` would pass for these arguments, with a stand-in workspace address where it would pass one"""
    d, out = _gemm_desc(A, B, M, N, K, _launch=False, **kw)
    keep = [out]
    if defer_reduce:
        keep.append(L.SplitKPending())
        d.defer_reduce, d.pending = 1, C.pointer(keep[-1])
    if carry is not None:
        d.carry = C.pointer(carry)
    d.workspace = 256 if L.load().dvt_gemm_workspace_bytes(C.byref(d)) > 0 else None
    return d, keep


def gemm_plan(A: Tensor, B: Tensor, M: int, N: int, K: int, **kw) -> GemmPlan:
    """What ``gemm`` launches for the same arguments (dvt_gemm_plan: the launcher's own decisions, no launch, no device
    needed -- the tensors may live anywhere, only their addresses, strides and types count)."""
    d, _keep = _plan_desc(A, B, M, N, K, **kw)
    q = L.GemmPlanInfo()
    L.check(L.load().dvt_gemm_plan(C.byref(d), C.byref(q)), "dvt_gemm_plan")
    return _plan_tuple(q)


def gemm_pair_plan(wgrad: dict, dgrad: dict) -> Tuple[GemmPlan, GemmPlan]:
    """dvt_gemm_pair's launches for two products, each given as the keyword arguments of ``gemm`` (A, B, M, N, K, ...)."""
    wd, _kw = _plan_desc(**wgrad)
    gd, _kg = _plan_desc(**dgrad)
    qw, qg = L.GemmPlanInfo(), L.GemmPlanInfo()
    L.check(L.load().dvt_gemm_pair_plan(C.byref(wd), C.byref(gd), C.byref(qw), C.byref(qg)), "dvt_gemm_pair_plan")
    return _plan_tuple(qw), _plan_tuple(qg)


def gemm_is_launch_bound(M: int, N: int, K: int, dtype: torch.dtype, *, a_kmajor: bool = True, b_kmajor: bool = True) -> bool:
    """Does dvt_gemm take the panel-streaming kernel of the launch-bound shapes for this product (no launch)?"""
    if dtype not in (torch.bfloat16, torch.float16):
        return False
    d = L.GemmDesc()
    d.A = d.B = d.C = 16                              # (non-null, aligned: the route depends on shapes and layouts only)
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = (K if a_kmajor else M), (K if b_kmajor else N), N
    d.a_kmajor, d.b_kmajor = int(a_kmajor), int(b_kmajor)
    d.in_dtype = d.out_dtype = _DT[dtype]
    d.alpha = 1.0
    return L.load().dvt_gemm_route(C.byref(d)) == 0


def splitk_reduce_pending(pending) -> None:
    """Perform a deferred split-K reduce as a launch of its own (no data-gradient launch followed to carry it)."""
    if pending is not None and pending.valid:
        L.check(L.load().dvt_splitk_reduce_pending(C.byref(pending), _stream()), "dvt_splitk_reduce_pending")
        pending.valid = 0


def linear_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, *, epilogue: int = L.EPI_NONE,
               residual: Optional[Tensor] = None, aux: Optional[Tensor] = None,
               out_dtype: Optional[torch.dtype] = None) -> Tensor:
    """y[M,N] = epi(x[M,K] @ w[N,K]^T + bias).  out_dtype float32 with an fp32 residual: the fp32 residual stream."""
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and x.stride(1) == 1 and w.is_contiguous()
    return gemm(x, w, M, N, K, a_kmajor=True, b_kmajor=True, lda=x.stride(0), ldb=K, epilogue=epilogue,
                bias=bias, residual=residual, aux=aux, out_dtype=out_dtype)


def linear_dgrad(dy: Tensor, w: Tensor, *, epilogue: int = L.EPI_NONE, aux: Optional[Tensor] = None,
                 carry=None) -> Tensor:
    """dx[M,K] = epi(dy[M,N] @ w[N,K])   (epilogue DGELU / DRELU multiplies by act'(aux)).
    carry: the pending split-K reduce of the weight gradient launched just before (linear_wgrad(defer_reduce=True))."""
    M, N = dy.shape
    K = w.shape[1]
    assert w.shape[0] == N and dy.stride(1) == 1 and w.is_contiguous()
    out = gemm(dy, w, M, K, N, a_kmajor=True, b_kmajor=False, lda=dy.stride(0), ldb=K, epilogue=epilogue,
               aux=aux, carry=carry)
    if carry is not None:
        carry.valid = 0                              # performed by this call, one way or the other
    return out


def linear_wgrad(dy: Tensor, x: Tensor, *, out: Optional[Tensor] = None, accumulate: bool = False,
                 bias_out: Optional[Tensor] = None, bias_accumulate: bool = False, defer_reduce: bool = False):
    """dW[N,K] (f32) = dy[M,N]^T @ x[M,K]; optionally also the bias gradient
    bias_out[N] (+)= sum_m dy[m, :] from the same pass over dy.  defer_reduce: -> (dW, pending), see ``gemm``."""
    M, N = dy.shape
    K = x.shape[1]
    assert x.shape[0] == M and dy.stride(1) == 1 and x.stride(1) == 1
    return gemm(dy, x, N, K, M, a_kmajor=False, b_kmajor=False, lda=dy.stride(0), ldb=x.stride(0), out=out,
                out_dtype=torch.float32, accumulate=accumulate, colsum_out=bias_out,
                colsum_accumulate=bias_accumulate, defer_reduce=defer_reduce)


PAIR_LAUNCH = True        # A/B switch (bench.py --no-pair-launch): weight + data gradient of a launch-bound Linear in one launch


def linear_backward(dy: Tensor, x: Tensor, w: Tensor, *, out: Optional[Tensor] = None, accumulate: bool = False,
                    bias_out: Optional[Tensor] = None, bias_accumulate: bool = False, epilogue: int = L.EPI_NONE,
                    aux: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Both gradients of y = x w^T (+ bias) from dy [M,N]: (dW [N,K] f32 (+ bias_out), dx [M,K] = epi(dy w)).
    Launch-bound shapes (a few hundred rows: the temporal encoder, the CLS-row layers): ONE launch (dvt_gemm_pair) --
    the two products are independent.  Otherwise the weight gradient with its split-K reduce deferred, then the data
    gradient carrying that reduce in its grid tail."""
    M, N = dy.shape
    K = x.shape[1]
    assert x.shape[0] == M and dy.stride(1) == 1 and x.stride(1) == 1 and w.shape == (N, K) and w.is_contiguous()
    wd, out = _gemm_desc(dy, x, N, K, M, a_kmajor=False, b_kmajor=False, lda=dy.stride(0), ldb=x.stride(0), out=out,
                         out_dtype=torch.float32, accumulate=accumulate, colsum_out=bias_out,
                         colsum_accumulate=bias_accumulate)
    gd, _ = _gemm_desc(dy, w, M, K, N, a_kmajor=True, b_kmajor=False, lda=dy.stride(0), ldb=K, out=dy[:, :0].new_empty((0, K)),
                       epilogue=epilogue, aux=aux)
    gd.C, gd.ldc = dy.data_ptr(), K                     # a valid address for the shape test; the real one below
    lib = L.load()
    if PAIR_LAUNCH and lib.dvt_gemm_pair_fused(C.byref(wd), C.byref(gd)):
        dx = torch.empty((M, K), dtype=dy.dtype, device=dy.device)
        gd.C, gd.ldc = dx.data_ptr(), K
        L.check(lib.dvt_gemm_pair(C.byref(wd), C.byref(gd), _stream()), "dvt_gemm_pair")
        return out, dx
    _, pend = linear_wgrad(dy, x, out=out, accumulate=accumulate, bias_out=bias_out, bias_accumulate=bias_accumulate,
                           defer_reduce=True)
    return out, linear_dgrad(dy, w, epilogue=epilogue, aux=aux, carry=pend)


def colsum(x: Tensor, *, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """f32 [N] = sum over rows of x[M,N] (bias gradients)."""
    _need_cuda(x)
    M, N = x.shape
    assert x.stride(1) == 1
    if out is None:
        assert not accumulate
        out = torch.empty((N,), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.numel() == N and out.is_contiguous()
    lib = L.load()
    ws = workspace(lib.dvt_colsum_workspace_bytes(M, N), x.device)
    L.check(lib.dvt_colsum(x.data_ptr(), x.stride(0), out.data_ptr(), _p(ws), M, N, dt(x), int(accumulate),
                           _stream()), "dvt_colsum")
    return out


# ------------------------------------------------------------------ attention
def _attn_desc(q: Tensor, k: Tensor, v: Tensor, o: Tensor, lse: Tensor, scale: float, dropout=None) -> L.AttnDesc:
    """q,k,v,o are 4-D views [B, H, L, dh] with unit stride in the last dim."""
    for t in (q, k, v, o):
        assert t.dim() == 4 and t.stride(3) == 1, "attention operands must be [B,H,L,dh] views, dh contiguous"
    B, H, Lq, dh = q.shape
    Lk = k.shape[2]
    assert k.shape == (B, H, Lk, dh) and v.shape == (B, H, Lk, dh) and o.shape == (B, H, Lq, dh)
    d = L.AttnDesc()
    d.q, d.k, d.v, d.o, d.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr()
    d.B, d.H, d.Lq, d.Lk, d.dh = B, H, Lq, Lk, dh
    d.q_sb, d.q_sh, d.q_sl = q.stride(0), q.stride(1), q.stride(2)
    d.k_sb, d.k_sh, d.k_sl = k.stride(0), k.stride(1), k.stride(2)
    d.v_sb, d.v_sh, d.v_sl = v.stride(0), v.stride(1), v.stride(2)
    d.o_sb, d.o_sh, d.o_sl = o.stride(0), o.stride(1), o.stride(2)
    d.scale = scale
    d.dtype = dt(q)
    if dropout is not None:                      # (p, rng_state tensor, site offset): attention-probability dropout
        d.dropout_p, d.rng_state, d.rng_offset = float(dropout[0]), dropout[1].data_ptr(), int(dropout[2])
    return d


def attention_fwd(q: Tensor, k: Tensor, v: Tensor, o: Tensor, scale: float, dropout=None,
                  lse: Optional[Tensor] = None) -> Tensor:
    """Writes o (a [B,H,Lq,dh] view of caller-owned memory); returns lse [B,H,Lq] f32 (written into `lse` if given: a
    contiguous f32 tensor of B*H*Lq elements)."""
    _need_cuda(q, k, v, o)
    B, H, Lq, _ = q.shape
    if lse is None:
        lse = torch.empty((B, H, Lq), dtype=torch.float32, device=q.device)
    else:
        assert lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() == B * H * Lq and lse.device == q.device
    d = _attn_desc(q, k, v, o, lse, scale, dropout)
    nb = (2 * q.numel() + k.numel() + v.numel()) * q.element_size()          # read q, k, v; write o
    with _timed(("hbm", "attention_fwd", q.numel(), 4.0 * q.numel() * k.shape[2]), nb):   # key carries the MFMA flops
        L.check(L.load().dvt_attention_fwd(C.byref(d), _stream()), "dvt_attention_fwd")
    return lse


ATTN_BWD_TWO_PASS = False      # A/B switch (bench.py --attn-two-pass): the dq + dk/dv kernel pair instead of the one-pass backward


def attention_bwd(q: Tensor, k: Tensor, v: Tensor, o: Tensor, lse: Tensor, do: Tensor, dq: Tensor,
                  dk: Tensor, dv: Tensor, scale: float, dropout=None, two_pass: Optional[bool] = None,
                  ws: Optional[Tensor] = None) -> None:
    """do must share o's strides; dq/dk/dv must share q/k/v's strides (views of
    caller-owned memory, fully overwritten).  ws: caller-owned workspace of at least
    dvt_attention_bwd_workspace_bytes (default: the shared scratch buffer)."""
    _need_cuda(q, k, v, o, do, dq, dk, dv)
    for a, b in ((do, o), (dq, q), (dk, k), (dv, v)):
        assert a.shape == b.shape and all(sa == sb for sa, sb, n in zip(a.stride(), b.stride(), a.shape) if n > 1), \
            "gradient views must share the layout of their primal"
    d = _attn_desc(q, k, v, o, lse, scale, dropout)
    d.d_o, d.dq, d.dk, d.dv = do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    d.bwd_two_pass = int(ATTN_BWD_TWO_PASS if two_pass is None else two_pass)
    lib = L.load()
    need = lib.dvt_attention_bwd_workspace_bytes(C.byref(d))
    if ws is None:
        ws = workspace(need, q.device)
    else:
        assert ws.device == q.device and ws.numel() * ws.element_size() >= need
    d.workspace = _p(ws)
    # algorithmic bytes: q, k, v, o, dO read once, dq, dk, dv written once (the one-pass form moves exactly that; the
    # two-kernel form re-reads q, k, v, dO: 13 units through the memory pipeline for these 8)
    nb = (4 * q.numel() + 2 * k.numel() + 2 * v.numel()) * q.element_size()
    with _timed(("hbm", "attention_bwd", q.numel(), 10.0 * q.numel() * k.shape[2]), nb):  # 5 products of 2*L*L*dh
        L.check(lib.dvt_attention_bwd(C.byref(d), _stream()), "dvt_attention_bwd")


class AttnPlan(NamedTuple):
    """What one dvt_attention_fwd / _bwd call launches (dvt_attention_plan): the kernel family (ATTN_FAMILIES), the
    template count of the (first) launch and of the dk/dv launch (0 = rolled loop / not templated), waves per block of
    each, whether each stores output tiles as whole rows through LDS patches (True), per lane (False) or has no such
    choice (None), whether the workspace is used, and the dynamic LDS bytes of each launch."""
    family: str
    count: int = 0
    count2: int = 0
    waves: int = 0
    waves2: int = 0
    patch: Optional[bool] = None
    patch2: Optional[bool] = None
    workspace: bool = False
    lds: int = 0
    lds2: int = 0


ATTN_FAMILIES = _enum_names("dvt_attn_family", "DVT_ATTN_[FB]_")


def attention_plan(q: Tensor, k: Tensor, v: Tensor, o: Tensor, *, bwd: bool = False, do: Optional[Tensor] = None,
                   dq: Optional[Tensor] = None, dk: Optional[Tensor] = None, dv: Optional[Tensor] = None,
                   dropout_p: float = 0.0, two_pass: Optional[bool] = None, scale: Optional[float] = None) -> AttnPlan:
    """What ``attention_fwd`` (or, bwd=True, ``attention_bwd``) launches for the same views (dvt_attention_plan: the
    launchers' own decisions, no launch, no device needed -- only shapes, strides, addresses, types and the sign of
    `scale` count; default dh^-1/2, the model's).  The gradient views default to their primals' (same strides and
    alignment)."""
    d = _attn_desc(q, k, v, o, o, q.shape[3] ** -0.5 if scale is None else float(scale))
    if dropout_p:
        d.dropout_p, d.rng_state = float(dropout_p), 256
    if bwd:
        do, dq, dk, dv = (o if do is None else do), (q if dq is None else dq), (k if dk is None else dk), (v if dv is None else dv)
        d.d_o, d.dq, d.dk, d.dv = do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
        d.bwd_two_pass = int(ATTN_BWD_TWO_PASS if two_pass is None else two_pass)
    r = L.AttnPlanInfo()
    L.check(L.load().dvt_attention_plan(C.byref(d), int(bwd), C.byref(r)), "dvt_attention_plan")
    opt = lambda x: None if x < 0 else bool(x)
    return AttnPlan(ATTN_FAMILIES[r.family], r.count, r.count2, r.waves, r.waves2, opt(r.patch), opt(r.patch2),
                    bool(r.workspace), r.lds, r.lds2)


# ------------------------------------------------------------------ streamed attention (attn_long_*: any length, dh = 64)
def _attn_long_desc(q, k, v, o, lse, scale, do=None, dq=None, dk=None, dv=None) -> L.AttnDesc:
    d = _attn_desc(q, k, v, o, lse, scale)
    if do is not None:
        d.d_o, d.dq, d.dk, d.dv = do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    return d


def attention_long_supported(q: Tensor, k: Tensor, v: Tensor, o: Tensor, *, scale: Optional[float] = None,
                             dropout_p: float = 0.0, do: Optional[Tensor] = None, dq: Optional[Tensor] = None,
                             dk: Optional[Tensor] = None, dv: Optional[Tensor] = None) -> bool:
    """Do the streamed kernels take these views (dvt_attention_long_supported: 16-bit, dh == 64, no dropout, scale > 0,
    strides multiples of 8, 16-byte aligned)?  With `do` the gradient views count too (default: their primals')."""
    d = _attn_desc(q, k, v, o, o, q.shape[3] ** -0.5 if scale is None else float(scale))
    if dropout_p:
        d.dropout_p, d.rng_state = float(dropout_p), 256
    bwd = do is not None
    if bwd:
        dq, dk, dv = (q if dq is None else dq), (k if dk is None else dk), (v if dv is None else dv)
        d.d_o, d.dq, d.dk, d.dv = do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    return bool(L.load().dvt_attention_long_supported(C.byref(d), int(bwd)))


def attention_long_fwd(q: Tensor, k: Tensor, v: Tensor, o: Tensor, scale: float, lse: Optional[Tensor] = None) -> Tensor:
    """``attention_fwd`` on the streamed kernels: writes o, returns lse [B,H,Lq] f32 (the same definition)."""
    _need_cuda(q, k, v, o)
    B, H, Lq, _ = q.shape
    if lse is None:
        lse = torch.empty((B, H, Lq), dtype=torch.float32, device=q.device)
    else:
        assert lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() == B * H * Lq and lse.device == q.device
    d = _attn_long_desc(q, k, v, o, lse, scale)
    nb = (2 * q.numel() + k.numel() + v.numel()) * q.element_size()
    with _timed(("hbm", "attention_long_fwd", q.numel(), 4.0 * q.numel() * k.shape[2]), nb):
        L.check(L.load().dvt_attention_long_fwd(C.byref(d), _stream()), "dvt_attention_long_fwd")
    return lse


def attention_long_bwd(q: Tensor, k: Tensor, v: Tensor, o: Tensor, lse: Tensor, do: Tensor, dq: Tensor,
                       dk: Tensor, dv: Tensor, scale: float, ws: Optional[Tensor] = None) -> None:
    """``attention_bwd`` on the streamed kernels (dq launch, then dk/dv; the same layout rules)."""
    _need_cuda(q, k, v, o, do, dq, dk, dv)
    for a, b in ((do, o), (dq, q), (dk, k), (dv, v)):
        assert a.shape == b.shape and all(sa == sb for sa, sb, n in zip(a.stride(), b.stride(), a.shape) if n > 1), \
            "gradient views must share the layout of their primal"
    d = _attn_long_desc(q, k, v, o, lse, scale, do, dq, dk, dv)
    lib = L.load()
    need = lib.dvt_attention_long_bwd_workspace_bytes(C.byref(d))
    if ws is None:
        ws = workspace(need, q.device)
    else:
        assert ws.device == q.device and ws.numel() * ws.element_size() >= need
    d.workspace = _p(ws)
    nb = (4 * q.numel() + 2 * k.numel() + 2 * v.numel()) * q.element_size()
    with _timed(("hbm", "attention_long_bwd", q.numel(), 10.0 * q.numel() * k.shape[2]), nb):
        L.check(lib.dvt_attention_long_bwd(C.byref(d), _stream()), "dvt_attention_long_bwd")


class AttnLongPlan(NamedTuple):
    """What one dvt_attention_long_fwd / _bwd call launches (dvt_attention_long_plan).  Of the forward or dq launch: query
    rows per workgroup, keys per LDS chunk, waves, chunk buffers, chunks streamed, workgroups, dynamic LDS bytes and whether
    tiles go out as whole rows through LDS patches; of the dk/dv launch (backward only, else 0 / None): key rows per
    workgroup, queries per chunk and the same."""
    q_block: int
    k_chunk: int
    waves: int
    ring: int
    chunks: int
    grid: int
    lds: int
    patch: bool
    k_block: int = 0
    q_chunk: int = 0
    waves2: int = 0
    ring2: int = 0
    chunks2: int = 0
    grid2: int = 0
    lds2: int = 0
    patch2: Optional[bool] = None
    workspace: bool = False


def attention_long_plan(q: Tensor, k: Tensor, v: Tensor, o: Tensor, *, bwd: bool = False, do: Optional[Tensor] = None,
                        dq: Optional[Tensor] = None, dk: Optional[Tensor] = None, dv: Optional[Tensor] = None,
                        dropout_p: float = 0.0, scale: Optional[float] = None) -> AttnLongPlan:
    """What ``attention_long_fwd`` (or, bwd=True, ``attention_long_bwd``) launches for these views; raises what the
    launcher raises for views it refuses.  No launch, no device needed."""
    d = _attn_desc(q, k, v, o, o, q.shape[3] ** -0.5 if scale is None else float(scale))
    if dropout_p:
        d.dropout_p, d.rng_state = float(dropout_p), 256
    if bwd:
        do, dq, dk, dv = (o if do is None else do), (q if dq is None else dq), (k if dk is None else dk), (v if dv is None else dv)
        d.d_o, d.dq, d.dk, d.dv = do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    r = L.AttnLongPlanInfo()
    L.check(L.load().dvt_attention_long_plan(C.byref(d), int(bwd), C.byref(r)), "dvt_attention_long_plan")
    opt = lambda x: None if x < 0 else bool(x)
    return AttnLongPlan(r.q_block, r.k_chunk, r.waves, r.ring, r.chunks, r.grid, r.lds, bool(r.patch), r.k_block, r.q_chunk,
                        r.waves2, r.ring2, r.chunks2, r.grid2, r.lds2, opt(r.patch2), bool(r.workspace))


# ------------------------------------------------------------------ single-query attention, K / V projections folded
def _attn_cls_desc(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, H: int) -> L.AttnClsDesc:
    """x [S, N, d] (16-bit), last dim contiguous."""
    assert x.dim() == 3 and x.stride(2) == 1
    q = L.AttnClsDesc()
    q.x, q.xs0, q.xs1 = x.data_ptr(), x.stride(0), x.stride(1)
    q.gamma, q.beta, q.eps = gamma.data_ptr(), beta.data_ptr(), eps
    q.S, q.N, q.d = x.shape
    q.H, q.dtype = H, dt(x)
    return q


def attn_cls_supported(x: Tensor, H: int, dh: Optional[int] = None) -> bool:
    """Shape / dtype test of the folded single-query path (no launch): the row-pass kernels (dvt_attn_cls_supported) and,
    when ``dh`` is given, the head-wise products on either side of them (dvt_heads_expand_outer: dh <= 384;
    dvt_heads_contract*: d % 8 == 0, d <= 512) -- so that a shape accepted here cannot fail later inside backward."""
    if not x.is_cuda or x.dim() != 3 or x.stride(2) != 1:
        return False
    if dh is not None and not (0 < dh <= 384 and x.shape[2] % 8 == 0 and x.shape[2] <= 512):
        return False
    q = L.AttnClsDesc()
    q.xs0, q.xs1 = x.stride(0), x.stride(1)
    q.S, q.N, q.d = x.shape
    q.H, q.dtype = H, dt(x)
    return bool(L.load().dvt_attn_cls_supported(C.byref(q)))


def attn_cls_fwd(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, R: Tensor):
    """x [S,N,d], R [S,H,d] f32 -> (A [S,H,d] f32, lse [S,H], P [S,N,8], mean [S*N], rstd [S*N])."""
    _need_cuda(x, gamma, beta, R)
    S, N, d = x.shape
    H = R.shape[1]
    assert R.shape == (S, H, d) and R.dtype == torch.float32 and R.is_contiguous()
    q = _attn_cls_desc(x, gamma, beta, eps, H)
    f32 = dict(dtype=torch.float32, device=x.device)
    A, lse, P = torch.empty((S, H, d), **f32), torch.empty((S, H), **f32), torch.empty((S, N, 8), **f32)
    mean, rstd = torch.empty((S * N,), **f32), torch.empty((S * N,), **f32)
    q.R, q.A, q.lse, q.P = R.data_ptr(), A.data_ptr(), lse.data_ptr(), P.data_ptr()
    q.mean, q.rstd = mean.data_ptr(), rstd.data_ptr()
    with _timed(("hbm", "attn_cls_fwd", S * N), S * N * d * x.element_size() + 2 * S * H * d * 4):
        L.check(L.load().dvt_attn_cls_fwd(C.byref(q), _stream()), "dvt_attn_cls_fwd")
    return A, lse, P, mean, rstd


def attn_cls_bwd(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, R: Tensor, A: Tensor, lse: Tensor, P: Tensor,
                 mean: Tensor, rstd: Tensor, dM: Tensor, *, dx: Optional[Tensor] = None, dg: Optional[Tensor] = None,
                 db: Optional[Tensor] = None, accumulate: bool = False, accumulate_beta: Optional[bool] = None):
    """-> (dx like x, G [S,H,d] f32, dgamma, dbeta)."""
    _need_cuda(x, gamma, beta, R, A, lse, P, mean, rstd, dM)
    S, N, d = x.shape
    H = R.shape[1]
    assert dM.shape == (S, H, d) and dM.dtype == torch.float32 and dM.is_contiguous() and P.shape == (S, N, 8)
    q = _attn_cls_desc(x, gamma, beta, eps, H)
    if dx is None:
        dx = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
    assert dx.stride() == x.stride()
    if dg is None or db is None:
        assert not accumulate and not accumulate_beta and dg is None and db is None
        dg = torch.empty((d,), dtype=torch.float32, device=x.device)
        db = torch.empty((d,), dtype=torch.float32, device=x.device)
    G = torch.empty((S, H, d), dtype=torch.float32, device=x.device)
    q.R, q.A, q.lse, q.P = R.data_ptr(), A.data_ptr(), lse.data_ptr(), P.data_ptr()
    q.mean, q.rstd = mean.data_ptr(), rstd.data_ptr()
    q.dM, q.dx, q.G, q.dgamma, q.dbeta = dM.data_ptr(), dx.data_ptr(), G.data_ptr(), dg.data_ptr(), db.data_ptr()
    q.accumulate_gamma = int(accumulate)
    q.accumulate_beta = int(accumulate if accumulate_beta is None else accumulate_beta)
    lib = L.load()
    ws = workspace(lib.dvt_attn_cls_bwd_workspace_bytes(C.byref(q)), x.device)
    q.workspace = _p(ws)
    with _timed(("hbm", "attn_cls_bwd", S * N), 2 * S * N * d * x.element_size() + 4 * S * H * d * 4):
        L.check(lib.dvt_attn_cls_bwd(C.byref(q), _stream()), "dvt_attn_cls_bwd")
    return dx, G, dg, db


def heads_expand(a: Tensor, W: Tensor, H: int, alpha: float = 1.0) -> Tensor:
    """a [S, H*dh] (16-bit, row stride free), W [H*dh, d] rows of a 16-bit weight -> out[s,h,:] = alpha a[s,h,:] W_h (f32)."""
    _need_cuda(a, W)
    S, inner = a.shape
    d = W.shape[1]
    assert W.shape[0] == inner and a.stride(1) == 1 and W.stride(1) == 1 and a.dtype == W.dtype and inner % H == 0
    out = torch.empty((S, H, d), dtype=torch.float32, device=a.device)
    L.check(L.load().dvt_heads_expand(a.data_ptr(), a.stride(0), W.data_ptr(), W.stride(0), out.data_ptr(), S, H,
                                      inner // H, d, alpha, dt(a), _stream()), "dvt_heads_expand")
    return out


def heads_contract(v: Tensor, W: Tensor, alpha: float = 1.0, gamma: Optional[Tensor] = None,
                   beta: Optional[Tensor] = None) -> Tensor:
    """v [S,H,d] f32 (entering as gamma*v+beta), W [H*dh, d] 16-bit -> out [S, H*dh] = alpha W_h v_h in W's dtype."""
    _need_cuda(v, W, gamma, beta)
    S, H, d = v.shape
    inner = W.shape[0]
    assert W.shape[1] == d and W.stride(1) == 1 and v.is_contiguous() and v.dtype == torch.float32 and inner % H == 0
    out = torch.empty((S, inner), dtype=W.dtype, device=v.device)
    L.check(L.load().dvt_heads_contract(v.data_ptr(), _p(gamma), _p(beta), W.data_ptr(), W.stride(0), out.data_ptr(),
                                        inner, S, H, inner // H, d, alpha, dt(W), _stream()), "dvt_heads_contract")
    return out


def heads_outer(a: Tensor, v: Tensor, out: Tensor, alpha: float = 1.0, gamma: Optional[Tensor] = None,
                beta: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """out[h*dh+e, c] (+)= alpha sum_s a[s, h*dh+e] (gamma*v+beta)[s,h,c]; a [S, H*dh] 16-bit, v [S,H,d] f32,
    out [H*dh, d] f32 (row stride free): the weight gradient of a row range of the packed to_qkv."""
    _need_cuda(a, v, out, gamma, beta)
    S, H, d = v.shape
    inner = a.shape[1]
    assert out.shape == (inner, d) and out.stride(1) == 1 and out.dtype == torch.float32 and a.stride(1) == 1
    assert v.is_contiguous() and v.dtype == torch.float32 and inner % H == 0
    L.check(L.load().dvt_heads_outer(a.data_ptr(), a.stride(0), v.data_ptr(), _p(gamma), _p(beta), out.data_ptr(),
                                     out.stride(0), S, H, inner // H, d, alpha, int(accumulate), dt(a), _stream()),
            "dvt_heads_outer")
    return out


def heads_expand_outer(a: Tensor, W: Tensor, H: int, v: Tensor, dW: Tensor, *, alpha_out: float = 1.0, alpha_dw: float = 1.0,
                       gamma: Optional[Tensor] = None, beta: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """One launch: ``heads_expand(a, W, H, alpha_out)`` (returned) and ``heads_outer(a, v, dW, alpha_dw, gamma, beta)``."""
    _need_cuda(a, W, v, dW, gamma, beta)
    S, inner = a.shape
    d = W.shape[1]
    assert W.shape[0] == inner and a.stride(1) == 1 and W.stride(1) == 1 and a.dtype == W.dtype and inner % H == 0
    assert v.shape == (S, H, d) and v.is_contiguous() and v.dtype == torch.float32
    assert dW.shape == (inner, d) and dW.stride(1) == 1 and dW.dtype == torch.float32
    out = torch.empty((S, H, d), dtype=torch.float32, device=a.device)
    L.check(L.load().dvt_heads_expand_outer(a.data_ptr(), a.stride(0), W.data_ptr(), W.stride(0), out.data_ptr(), alpha_out,
                                            v.data_ptr(), _p(gamma), _p(beta), dW.data_ptr(), dW.stride(0), alpha_dw,
                                            int(accumulate), S, H, inner // H, d, dt(a), _stream()), "dvt_heads_expand_outer")
    return out


def heads_contract_outer(v: Tensor, gamma: Tensor, W: Tensor, a: Tensor, dW: Tensor, *, alpha_out: float = 1.0,
                         alpha_dw: float = 1.0, accumulate: bool = False) -> Tensor:
    """One launch: ``heads_contract(v, W, alpha_out, gamma)`` (returned) and ``heads_outer(a, v, dW, alpha_dw, gamma)``."""
    _need_cuda(v, gamma, W, a, dW)
    S, H, d = v.shape
    inner = W.shape[0]
    assert W.shape[1] == d and W.stride(1) == 1 and v.is_contiguous() and v.dtype == torch.float32 and inner % H == 0
    assert a.shape == (S, inner) and a.stride(1) == 1 and a.dtype == W.dtype
    assert dW.shape == (inner, d) and dW.stride(1) == 1 and dW.dtype == torch.float32
    out = torch.empty((S, inner), dtype=W.dtype, device=v.device)
    L.check(L.load().dvt_heads_contract_outer(v.data_ptr(), gamma.data_ptr(), W.data_ptr(), W.stride(0), out.data_ptr(), inner,
                                              alpha_out, a.data_ptr(), a.stride(0), dW.data_ptr(), dW.stride(0), alpha_dw,
                                              int(accumulate), S, H, inner // H, d, dt(W), _stream()),
            "dvt_heads_contract_outer")
    return out


# ------------------------------------------------------------------ losses
def bce_logits_fwd(z: Tensor, target: Tensor) -> Tensor:
    _need_cuda(z, target)
    assert z.is_contiguous() and target.is_contiguous() and target.dtype == torch.float32
    loss = torch.empty((1,), dtype=torch.float32, device=z.device)
    L.check(L.load().dvt_bce_logits_fwd(z.data_ptr(), target.data_ptr(), loss.data_ptr(), z.numel(), dt(z),
                                        _stream()), "dvt_bce_logits_fwd")
    return loss


def head_bce_supported(rows: int, d: int, classes: int) -> bool:
    return bool(L.load().dvt_head_bce_supported(int(rows), int(d), int(classes)))


def head_bce_fwd(x: Tensor, g1, b1, eps1: float, g2: Tensor, b2: Tensor, eps2: float, w: Tensor, c, target: Tensor):
    """LN -> LN -> Linear -> mean BCE in one launch (dvt_head_bce_fwd) -> (loss [1], logits [rows, C], grads): grads maps
    "x", "g1", "b1", "g2", "b2", "w", "c" to fp32 views holding d(loss)/d(.) for an upstream gradient of 1."""
    _need_cuda(x, g2, b2, w, target)
    rows, d = x.shape
    Cc = w.shape[0]
    assert x.is_contiguous() and w.is_contiguous() and w.shape[1] == d and target.shape == (rows, Cc)
    for t in (g1, b1, g2, b2, w, c, target):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    lib = L.load()
    n = lib.dvt_head_bce_grads_elems(rows, d, Cc)
    if n < 0:
        raise ValueError(f"head_bce_fwd: unsupported shape rows={rows} d={d} classes={Cc}")
    G = torch.empty((n,), dtype=torch.float32, device=x.device)
    logits = torch.empty((rows, Cc), dtype=torch.float32, device=x.device)
    loss = torch.empty((1,), dtype=torch.float32, device=x.device)
    desc = L.HeadBceDesc()
    desc.x, desc.x_dtype = x.data_ptr(), dt(x)
    desc.g1, desc.b1 = (g1.data_ptr(), b1.data_ptr()) if g1 is not None else (None, None)
    desc.g2, desc.b2, desc.w, desc.c = g2.data_ptr(), b2.data_ptr(), w.data_ptr(), (c.data_ptr() if c is not None else None)
    desc.target, desc.logits, desc.loss, desc.grads = target.data_ptr(), logits.data_ptr(), loss.data_ptr(), G.data_ptr()
    desc.rows, desc.d, desc.classes, desc.eps1, desc.eps2 = rows, d, Cc, float(eps1), float(eps2)
    L.check(lib.dvt_head_bce_fwd(C.byref(desc), _stream()), "dvt_head_bce_fwd")
    o, grads = 0, {}
    for name, cnt in (("x", rows * d), ("g1", d), ("b1", d), ("g2", d), ("b2", d), ("w", Cc * d), ("c", (Cc + 63) // 64 * 64)):
        grads[name] = G[o:o + (Cc if name == "c" else cnt)]
        o += cnt
    grads["x"] = grads["x"].view(rows, d)
    grads["w"] = grads["w"].view(Cc, d)
    return loss, logits, grads


def scaled_emit_group(scale: Tensor, entries) -> None:
    """dst = scale * src (+ dst), optional 16-bit copy of the result; entries: (src f32, dst f32 or None, accumulate,
    dst_lp 16-bit or None).  One launch (dvt_scaled_emit_group)."""
    if not entries:
        return
    _need_cuda(scale)
    assert scale.dtype == torch.float32 and scale.numel() == 1
    arr = (L.EmitEntry * len(entries))()
    for i, (src, dst, acc, lp) in enumerate(entries):
        _need_cuda(src)
        assert src.dtype == torch.float32 and src.is_contiguous()
        assert dst is None or (dst.dtype == torch.float32 and dst.is_contiguous() and dst.numel() == src.numel())
        assert lp is None or (lp.is_contiguous() and lp.numel() == src.numel())
        e = arr[i]
        e.src, e.dst, e.dst_lp = src.data_ptr(), (dst.data_ptr() if dst is not None else None), (lp.data_ptr() if lp is not None else None)
        e.n, e.accumulate, e.lp_dtype = src.numel(), int(bool(acc)), (dt(lp) if lp is not None else 0)
    L.check(L.load().dvt_scaled_emit_group(scale.data_ptr(), arr, len(entries), _stream()),
            "dvt_scaled_emit_group")


def bce_logits_bwd(z: Tensor, target: Tensor, gloss: Tensor) -> Tensor:
    _need_cuda(z, target, gloss)
    dz = torch.empty_like(z)
    L.check(L.load().dvt_bce_logits_bwd(z.data_ptr(), target.data_ptr(), gloss.data_ptr(), dz.data_ptr(), z.numel(),
                                        dt(z), _stream()), "dvt_bce_logits_bwd")
    return dz


def sigmoid_bce_fwd(z: Tensor, target: Tensor, want_prob: bool = False):
    """nn.BCELoss()(sigmoid(z), target) (mean, log terms clamped at -100) -> loss [1] f32 (, sigmoid(z) f32)."""
    _need_cuda(z, target)
    assert z.is_contiguous() and target.is_contiguous() and target.dtype == torch.float32 and target.numel() == z.numel()
    loss = torch.empty((1,), dtype=torch.float32, device=z.device)
    prob = torch.empty(z.shape, dtype=torch.float32, device=z.device) if want_prob else None
    L.check(L.load().dvt_sigmoid_bce_fwd(z.data_ptr(), target.data_ptr(), loss.data_ptr(), _p(prob), z.numel(), dt(z),
                                         _stream()), "dvt_sigmoid_bce_fwd")
    return (loss, prob) if want_prob else loss


def sigmoid_bce_bwd(z: Tensor, target: Tensor, gloss: Tensor) -> Tensor:
    _need_cuda(z, target, gloss)
    dz = torch.empty_like(z)
    L.check(L.load().dvt_sigmoid_bce_bwd(z.data_ptr(), target.data_ptr(), gloss.data_ptr(), dz.data_ptr(), z.numel(),
                                         dt(z), _stream()), "dvt_sigmoid_bce_bwd")
    return dz


def ce_argmax_fwd(student: Tensor, teacher: Tensor) -> Tensor:
    _need_cuda(student, teacher)
    assert student.is_contiguous() and teacher.is_contiguous() and student.dtype == teacher.dtype
    rows, Cn = student.shape
    loss = torch.empty((1,), dtype=torch.float32, device=student.device)
    L.check(L.load().dvt_ce_argmax_fwd(student.data_ptr(), teacher.data_ptr(), loss.data_ptr(), rows, Cn,
                                       dt(student), _stream()), "dvt_ce_argmax_fwd")
    return loss


def ce_argmax_bwd(student: Tensor, teacher: Tensor, gloss: Tensor) -> Tensor:
    rows, Cn = student.shape
    ds = torch.empty_like(student)
    L.check(L.load().dvt_ce_argmax_bwd(student.data_ptr(), teacher.data_ptr(), gloss.data_ptr(), ds.data_ptr(), rows,
                                       Cn, dt(student), _stream()), "dvt_ce_argmax_bwd")
    return ds


def frames_preprocess(frames: Tensor, resize: int, crop: int, mean, std, out_dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """uint8 RGB frames [F, H0, W0, 3] -> [F, 3, crop, crop]: Resize(resize) + CenterCrop(crop) + ToTensor +
    Normalize(mean, std), bit-exact with PIL / torch in fp32 (MMX_Light_dl.py:203-217)."""
    _need_cuda(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 [F, H0, W0, 3]")
    frames = frames.contiguous()
    Fr, H0, W0, _ = frames.shape
    lib = L.load()
    nbytes = lib.dvt_frames_preprocess_workspace_bytes(Fr, H0, W0, resize, crop)
    if nbytes == 0:
        raise ValueError(f"crop {crop} exceeds the frame resized to shorter side {resize} ({H0}x{W0})")
    ws = workspace(nbytes, frames.device)
    out = torch.empty((Fr, 3, crop, crop), dtype=out_dtype, device=frames.device)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    sd = (C.c_float * 3)(*[float(v) for v in std])
    L.check(lib.dvt_frames_preprocess(frames.data_ptr(), out.data_ptr(), _DT[out_dtype], Fr, H0, W0, resize, crop,
                                      C.cast(m, C.c_void_p), C.cast(sd, C.c_void_p), ws.data_ptr(),
                                      _stream()), "dvt_frames_preprocess")
    return out


def _host_table(table, cols: int, what: str) -> Tensor:
    """A parameter table as a contiguous int32 CPU tensor [rows, cols]: the launchers validate it on the host before any launch."""
    if isinstance(table, Tensor) and table.is_cuda:
        raise ValueError(f"{what}: the table is a host array (validated before any launch), got a device tensor")
    t = torch.as_tensor(table, dtype=torch.int32).contiguous()
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError(f"{what}: the table must be [rows, {cols}], got {tuple(t.shape)}")
    return t


def frames_augment(frames: Tensor, table, out_hw, mean=None, std=None, out_dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """uint8 RGB frames [F, H0, W0, 3] + host table [N, 7] int32 (src_index, top, left, h, w, hflip, vflip) ->
    [N, 3, out_h, out_w] in ``out_dtype``: per sample crop -> Pillow bilinear resize -> flips -> ToTensor -> Normalize
    (MMX_Frame_dl.py:63-71), bit-exact in fp32.  ``out_dtype=torch.uint8`` -> [N, out_h, out_w, 3] bytes, not normalised."""
    if not isinstance(frames, Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 [F, H0, W0, 3]")
    tab = _host_table(table, 7, "frames_augment")
    if out_dtype != torch.uint8 and out_dtype not in _DT:
        raise ValueError(f"frames_augment: no kernel writes {out_dtype}")
    _need_cuda(frames)
    frames = frames.contiguous()
    Fr, H0, W0, _ = frames.shape
    out_h, out_w = (int(v) for v in ((out_hw, out_hw) if isinstance(out_hw, int) else out_hw))
    N = tab.shape[0]
    lib = L.load()
    nbytes = lib.dvt_frames_augment_workspace_bytes(N, H0, W0, out_h, out_w)
    if nbytes == 0:
        raise ValueError(f"frames_augment: one output row of a {H0}x{W0} frame resized to {out_h}x{out_w} does not fit "
                         "the LDS band of the kernel")
    ws = workspace(nbytes, frames.device)
    u8 = out_dtype == torch.uint8
    out = torch.empty((N, out_h, out_w, 3) if u8 else (N, 3, out_h, out_w), dtype=out_dtype, device=frames.device)
    m = sd = None
    if not u8:
        m = C.cast((C.c_float * 3)(*[float(v) for v in mean]), C.c_void_p)
        sd = C.cast((C.c_float * 3)(*[float(v) for v in std]), C.c_void_p)
    L.check(lib.dvt_frames_augment(frames.data_ptr(), Fr, H0, W0, tab.data_ptr(), N, out.data_ptr(),
                                   L.ENUMS["dvt_augment_dst"]["DVT_AUGMENT_U8_HWC"] if u8 else _DT[out_dtype], out_h, out_w,
                                   m, sd, ws.data_ptr(), _stream()), "dvt_frames_augment")
    return out


def frames_erase(x: Tensor, table, value=(0, 0, 0)) -> Tensor:
    """RandomErasing with a constant fill, in place on x [F, 3, H, W]: host table [F, 4] int32 (top, left, h, w), h == 0
    leaves the frame alone (MMX_Frame_dl.py:87).  Only the rectangles are written.  Returns x."""
    if not isinstance(x, Tensor) or x.dim() != 4 or x.shape[1] != 3 or x.dtype not in _DT:
        raise ValueError("x must be a floating-point tensor [F, 3, H, W]")
    tab = _host_table(table, 4, "frames_erase")
    if tab.shape[0] != x.shape[0]:
        raise ValueError(f"frames_erase: {tab.shape[0]} table rows for {x.shape[0]} frames")
    _need_cuda(x)
    if not x.is_contiguous():
        raise ValueError("frames_erase works in place and needs a contiguous tensor")
    v = (C.c_float * 3)(*[float(c) for c in value])
    L.check(L.load().dvt_frames_erase(x.data_ptr(), dt(x), x.shape[0], x.shape[2], x.shape[3], tab.data_ptr(),
                                      C.cast(v, C.c_void_p), _stream()), "dvt_frames_erase")
    return x


# ------------------------------------------------------------------ Mixup / CutMix and soft targets (csrc/mix.hip)
MIX_ROWS_PER_LAUNCH = L.MACROS["DVT_MIX_ROWS_PER_LAUNCH"]      # rows (a pair or sample and one region) per clips_mix launch


def _host_lam(lam, rows: int, what: str) -> Tensor:
    """The lambdas as a contiguous float32 CPU tensor [rows]: validated on the host like the table."""
    if isinstance(lam, Tensor) and lam.is_cuda:
        raise ValueError(f"{what}: lam is a host array (validated before any launch), got a device tensor")
    t = torch.as_tensor(lam, dtype=torch.float32).contiguous()
    if t.dim() != 1 or t.shape[0] != rows:
        raise ValueError(f"{what}: lam must be [{rows}], got {tuple(t.shape)}")
    return t


def clips_mix(x: Tensor, table, lam, out: Optional[Tensor] = None) -> Tensor:
    """Mixup / CutMix across the batch of x [B, ..., C, H, W] (the dimensions between B and C fold into T): host table [B, 8]
    int32 (partner, kind, t0, t1, y0, y1, x0, x1), kind 0 = leave alone, 1 = mixup ``fmaf(lam, x[i], (1 - lam) x[partner])``,
    2 = cutmix ``out[i][box] = x[partner][box]``; host lam [B] float32.  ``out=None`` (or x): in place, the partner map must be
    an involution and only what changes is written; otherwise ``out`` (same shape and dtype, disjoint from x) receives every
    sample and any partner map goes.  One launch per ``MIX_ROWS_PER_LAUNCH`` rows (a pair, or out of place a sample, and one
    region of it).  Returns the tensor written."""
    if not isinstance(x, Tensor) or x.dim() < 4 or x.dtype not in _DT:
        raise ValueError("x must be a floating-point tensor [B, ..., C, H, W]")
    tab = _host_table(table, 8, "clips_mix")
    B = x.shape[0]
    if tab.shape[0] != B:
        raise ValueError(f"clips_mix: {tab.shape[0]} table rows for {B} samples")
    lm = _host_lam(lam, B, "clips_mix")
    if not x.is_contiguous():
        raise ValueError("clips_mix needs a contiguous tensor")
    if out is not None and out is not x:
        if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
            raise ValueError("clips_mix: out must be contiguous with the shape, dtype and device of x")
    in_place = out is None or out is x or out.data_ptr() == x.data_ptr()
    partner = tab[:, 0].tolist()
    if in_place and any(not (0 <= p < B and partner[p] == i) for i, p in enumerate(partner)):
        raise ValueError("clips_mix: in place the partner map must be an involution (partner[partner[i]] == i); pass out= "
                         "for any other map")
    _need_cuda(x, out)
    Cc, H, W = x.shape[-3:]
    T = 1
    for n in x.shape[1:-3]:
        T *= int(n)
    if x.numel() == 0:
        return x if in_place else out
    L.check(L.load().dvt_clips_mix(x.data_ptr(), None if in_place else out.data_ptr(), dt(x), B, T, Cc, H, W,
                                   tab.data_ptr(), lm.data_ptr(), _stream()), "dvt_clips_mix")
    return x if in_place else out


def targets_mix(table, lam, y: Optional[Tensor] = None, labels: Optional[Tensor] = None, num_classes: Optional[int] = None,
                smoothing: float = 0.0) -> Tensor:
    """Mixed targets f32 [B, C]: ``lam_i t_i + (1 - lam_i) t_partner(i)`` with the partner of column 0 of the host table
    [B, 8] and the host lam [B] (the target's lambda).  Exactly one of ``y`` (float32 [B, C], mixed as it is) and ``labels``
    (int64 [B], with ``num_classes``: rows ``smoothing / C`` everywhere and ``1 - smoothing + smoothing / C`` at the label; a
    label outside [0, C) gives a NaN row)."""
    if (y is None) == (labels is None):
        raise ValueError("targets_mix: exactly one of y and labels")
    tab = _host_table(table, 8, "targets_mix")
    src = y if y is not None else labels
    B = src.shape[0]
    if tab.shape[0] != B:
        raise ValueError(f"targets_mix: {tab.shape[0]} table rows for {B} samples")
    lm = _host_lam(lam, B, "targets_mix")
    if y is not None:
        if y.dim() != 2 or y.dtype != torch.float32:
            raise ValueError("targets_mix: y must be float32 [B, C]")
        Cc = y.shape[1]
    else:
        if labels.dim() != 1 or labels.dtype != torch.int64:
            raise ValueError("targets_mix: labels must be int64 [B]")
        if num_classes is None:
            raise ValueError("targets_mix: integer labels need num_classes")
        Cc = int(num_classes)
    _need_cuda(src)
    src = src.contiguous()
    out = torch.empty((B, Cc), dtype=torch.float32, device=src.device)
    L.check(L.load().dvt_targets_mix(_p(src) if y is not None else None, _p(src) if y is None else None, out.data_ptr(), B, Cc,
                                     tab.data_ptr(), lm.data_ptr(), float(smoothing), _stream()), "dvt_targets_mix")
    return out


def ce_soft_fwd(logits: Tensor, targets: Tensor):
    """Soft-target cross-entropy: mean over the rows of ``sum_c -t_c log_softmax(x)_c`` -> (loss f32 [1], lse f32 [2 M]: the
    per-row log-sum-exp, then the per-row sums of the targets)."""
    _need_cuda(logits, targets)
    M, Cc = logits.shape
    assert logits.stride(1) == 1
    assert targets.dtype == torch.float32 and targets.is_contiguous() and targets.shape == (M, Cc)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    lse = torch.empty(2 * M, dtype=torch.float32, device=logits.device)
    L.check(L.load().dvt_ce_soft_fwd(logits.data_ptr(), logits.stride(0), targets.data_ptr(), loss.data_ptr(), lse.data_ptr(), M,
                                     Cc, dt(logits), _stream()), "dvt_ce_soft_fwd")
    return loss, lse


def ce_soft_bwd(logits: Tensor, targets: Tensor, lse: Tensor, gloss: Tensor) -> Tensor:
    _need_cuda(logits, targets, lse, gloss)
    M, Cc = logits.shape
    assert logits.stride(1) == 1 and gloss.dtype == torch.float32 and lse.numel() == 2 * M
    assert targets.dtype == torch.float32 and targets.is_contiguous() and targets.shape == (M, Cc)
    d = torch.empty((M, Cc), dtype=logits.dtype, device=logits.device)
    L.check(L.load().dvt_ce_soft_bwd(logits.data_ptr(), logits.stride(0), targets.data_ptr(), lse.data_ptr(), gloss.data_ptr(),
                                     d.data_ptr(), Cc, M, Cc, dt(logits), _stream()), "dvt_ce_soft_bwd")
    return d


def frames_autoaugment(frames_u8: Tensor, table, mean=None, std=None, out_dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """uint8 RGB frames [N, H, W, 3] + host table [N, 2, 8] int32 (two slots {op, p0 .. p6} per sample, applied in order;
    ``input_stage.AutoAugment.draw`` makes one) -> [N, 3, H, W] in ``out_dtype``: torchvision's AutoAugment operations as its
    PIL path computes them, then ToTensor -> Normalize (MMX_Frame_dl.py:63-71), bit-exact in fp32, in one launch per 48
    samples.  ``out_dtype=torch.uint8`` -> [N, H, W, 3] bytes, not normalised."""
    if not isinstance(frames_u8, Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise ValueError("frames_u8 must be uint8 [N, H, W, 3]")
    if isinstance(table, Tensor) and table.is_cuda:
        raise ValueError("frames_autoaugment: table is a host array (validated before any launch), got a device tensor")
    tab = torch.as_tensor(table, dtype=torch.int32).contiguous()
    N, H, W, _ = frames_u8.shape
    if tuple(tab.shape) not in ((N, 2, 8), (N, 16)):
        raise ValueError(f"frames_autoaugment: table must be [{N}, 2, 8] for {N} frames, got {tuple(tab.shape)}")
    u8 = out_dtype == torch.uint8
    if not u8 and out_dtype not in _DT:
        raise ValueError(f"frames_autoaugment: out_dtype: no kernel writes {out_dtype}")
    if not u8 and (mean is None or std is None or len(mean) != 3 or len(std) != 3):
        raise ValueError("frames_autoaugment: mean and std must hold one number per channel")
    _need_cuda(frames_u8)
    frames_u8 = frames_u8.contiguous()
    out = torch.empty((N, H, W, 3) if u8 else (N, 3, H, W), dtype=out_dtype, device=frames_u8.device)
    m = sd = None
    if not u8:
        m = C.cast((C.c_float * 3)(*[float(v) for v in mean]), C.c_void_p)
        sd = C.cast((C.c_float * 3)(*[float(v) for v in std]), C.c_void_p)
    L.check(L.load().dvt_frames_autoaugment(frames_u8.data_ptr(), N, H, W, tab.data_ptr(), out.data_ptr(),
                                            L.ENUMS["dvt_augment_dst"]["DVT_AUGMENT_U8_HWC"] if u8 else _DT[out_dtype], m, sd,
                                            _stream()), "dvt_frames_autoaugment")
    return out


def _scores_and_mask(name: str, probs: Tensor, labels: Tensor) -> Tuple[Tensor, Tensor]:
    """The dtype plumbing of every metrics wrapper: a 16-bit score is cast to f32 (exact, so ties stay ties), a label mask
    becomes u8."""
    _need_cuda(probs, labels)
    if probs.dim() != 2 or tuple(labels.shape) != tuple(probs.shape):
        raise ValueError(f"{name}: probs {tuple(probs.shape)} and labels {tuple(labels.shape)} must be the same [N, C]")
    probs = probs.contiguous() if probs.dtype == torch.float32 else cast(probs.contiguous(), torch.float32)
    lab = labels.contiguous()
    if lab.dtype != torch.uint8:
        lab = (lab != 0).to(torch.uint8)
    return probs, lab


def f1_samples(probs: Tensor, labels: Tensor, thresholds) -> Tensor:
    """samples-averaged F1 of ``probs > t`` for every t (callbacks.py:38-41) -> f32 [T] on the device."""
    probs, lab = _scores_and_mask("f1_samples", probs, labels)
    N, Cn = probs.shape
    th = [float(t) for t in thresholds]
    lib = L.load()
    ws = workspace(lib.dvt_f1_samples_workspace_bytes(N, len(th)), probs.device)
    out = torch.empty((len(th),), dtype=torch.float32, device=probs.device)
    arr = (C.c_float * len(th))(*th)
    L.check(lib.dvt_f1_samples(probs.data_ptr(), lab.data_ptr(), N, Cn, C.cast(arr, C.c_void_p), len(th),
                               out.data_ptr(), ws.data_ptr(), _stream()), "dvt_f1_samples")
    return out


def average_precision(probs: Tensor, labels: Tensor):
    """-> (samples-averaged AP [1], support-weighted AP [1], per-class AP [C]) f32 device tensors
    (``average_precision_score`` of callbacks.py:48-54)."""
    probs, lab = _scores_and_mask("average_precision", probs, labels)
    N, Cn = probs.shape
    lib = L.load()
    nbytes = lib.dvt_average_precision_workspace_bytes(N, Cn)
    if nbytes == 0:
        raise ValueError("average_precision: empty input or N*C >= 2^31")
    ws = workspace(nbytes, probs.device)
    out = torch.empty((2 + Cn,), dtype=torch.float32, device=probs.device)
    L.check(lib.dvt_average_precision(probs.data_ptr(), lab.data_ptr(), N, Cn, out.data_ptr(), out[1:].data_ptr(),
                                      out[2:].data_ptr(), ws.data_ptr(), _stream()), "dvt_average_precision")
    return out[0:1], out[1:2], out[2:]


def multilabel_report_counts(probs: Tensor, labels: Tensor, threshold: float):
    """``classification_report(labels, probs > threshold)`` as exact counts (dvt_multilabel_report) -> (counts int64 [4, C]:
    TP / FP / FN / support per class, row_sums f64 [3]: the sums over rows of the per-row precision / recall / F1)."""
    probs, lab = _scores_and_mask("multilabel_report_counts", probs, labels)
    N, Cn = probs.shape
    lib = L.load()
    ws = workspace(lib.dvt_multilabel_report_workspace_bytes(N), probs.device)
    counts = torch.empty((4, Cn), dtype=torch.int64, device=probs.device)
    sums = torch.empty((3,), dtype=torch.float64, device=probs.device)
    L.check(lib.dvt_multilabel_report(probs.data_ptr(), lab.data_ptr(), N, Cn, float(threshold), counts.data_ptr(),
                                      sums.data_ptr(), _p(ws), _stream()), "dvt_multilabel_report")
    return counts, sums


def l2norm_rows_fwd(x: Tensor, eps: float):
    _need_cuda(x)
    x = x.contiguous()
    rows, D = x.shape
    y = torch.empty_like(x)
    inv = torch.empty((rows,), dtype=torch.float32, device=x.device)
    L.check(L.load().dvt_l2norm_rows_fwd(x.data_ptr(), y.data_ptr(), inv.data_ptr(), rows, D, eps, dt(x), _stream()),
            "dvt_l2norm_rows_fwd")
    return y, inv


def l2norm_rows_bwd(dy: Tensor, y: Tensor, inv: Tensor, eps: float) -> Tensor:
    dy = dy.contiguous()
    rows, D = y.shape
    dx = torch.empty_like(y)
    L.check(L.load().dvt_l2norm_rows_bwd(dy.data_ptr(), y.data_ptr(), inv.data_ptr(), dx.data_ptr(), rows, D, eps, dt(y),
                                         _stream()), "dvt_l2norm_rows_bwd")
    return dx


def cosine_rows(a: Tensor, b: Tensor, eps: float = 1e-8) -> Tensor:
    """nn.CosineSimilarity(dim=1): [rows, D] x [rows, D] -> f32 [rows] (no gradient):
    <a, b> / (max(||a||, eps) * max(||b||, eps)), each norm clamped on its own as torch does."""
    _need_cuda(a, b)
    a, b = a.detach().contiguous(), b.detach().contiguous()
    assert a.shape == b.shape and a.dim() == 2 and a.dtype == b.dtype
    out = torch.empty((a.shape[0],), dtype=torch.float32, device=a.device)
    L.check(L.load().dvt_cosine_rows(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.shape[0], a.shape[1], eps, dt(a),
                                     _stream()), "dvt_cosine_rows")
    return out


def gate_fwd(a: Tensor, b: Tensor) -> Tensor:
    _need_cuda(a, b)
    a, b = a.contiguous(), b.contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype
    y = torch.empty_like(a)
    L.check(L.load().dvt_gate_fwd(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), dt(a), _stream()), "dvt_gate_fwd")
    return y


def gate_bwd(dy: Tensor, a: Tensor, b: Tensor):
    dy = dy.contiguous()
    da, db = torch.empty_like(a), torch.empty_like(b)
    L.check(L.load().dvt_gate_bwd(dy.data_ptr(), a.data_ptr(), b.data_ptr(), da.data_ptr(), db.data_ptr(), a.numel(), dt(a),
                                  _stream()), "dvt_gate_bwd")
    return da, db


def contrastive_fwd(sim: Tensor, temperature: float):
    _need_cuda(sim)
    M = sim.shape[0]
    assert sim.dtype == torch.float32 and sim.is_contiguous() and sim.shape == (M, M)
    buf = torch.empty((2 * M + 1,), dtype=torch.float32, device=sim.device)
    L.check(L.load().dvt_contrastive_fwd(sim.data_ptr(), M, temperature, buf[2 * M:].data_ptr(), buf.data_ptr(),
                                         buf[M:].data_ptr(), _stream()), "dvt_contrastive_fwd")
    return buf[2 * M:].view(()), buf[:M]                     # loss, row_lse


def contrastive_bwd(sim: Tensor, row_lse: Tensor, temperature: float, gloss: Tensor) -> Tensor:
    M = sim.shape[0]
    dsim = torch.empty_like(sim)
    L.check(L.load().dvt_contrastive_bwd(sim.data_ptr(), row_lse.data_ptr(), M, temperature, gloss.data_ptr(),
                                         dsim.data_ptr(), _stream()), "dvt_contrastive_bwd")
    return dsim


def device_delay(microseconds: int) -> None:
    """Keep the current stream busy for a while (measurement aid, see dvt_device_delay)."""
    L.check(L.load().dvt_device_delay(int(microseconds), _stream()), "dvt_device_delay")


def dropout(x: Tensor, p: float, rng_state: Tensor, call_offset: int) -> Tensor:
    """y = x * keep / (1 - p); keep is a pure function of (rng_state on the device, call_offset, element index)."""
    _need_cuda(x, rng_state)
    x = x.contiguous()
    y = torch.empty_like(x)
    L.check(L.load().dvt_dropout(x.data_ptr(), y.data_ptr(), x.numel(), p, rng_state.data_ptr(), call_offset, dt(x),
                                 _stream()), "dvt_dropout")
    return y


def dropout_fused(x: Tensor, p: float, rng_state: Optional[Tensor], call_offset: int, *, residual: Optional[Tensor] = None,
                  relu: bool = False, gate: Optional[Tensor] = None) -> Tensor:
    """y = residual? + keep * relu?(x) / (1 - p) with the mask of ``dropout`` at (rng_state, call_offset); or, with ``gate``
    (the forward's output) and no rng_state, the backward of the relu form: gate != 0 ? x / (1 - p) : 0 (dvt_dropout_fused)."""
    _need_cuda(x, residual, gate, rng_state)
    x = x.contiguous()
    assert (rng_state is None) != (gate is None)
    for t in (residual, gate):
        assert t is None or (t.shape == x.shape and t.dtype == x.dtype and t.is_contiguous())
    y = torch.empty_like(x)
    L.check(L.load().dvt_dropout_fused(x.data_ptr(), _p(residual), _p(gate), y.data_ptr(), x.numel(), p, _p(rng_state),
                                       call_offset, int(relu), dt(x), _stream()), "dvt_dropout_fused")
    return y


def rng_advance_(rng_state: Tensor, delta: int) -> None:
    L.check(L.load().dvt_rng_advance(rng_state.data_ptr(), delta, _stream()), "dvt_rng_advance")


# ------------------------------------------------------------------ optimizer steps (csrc/optim.hip)
def _flat_f32(param: Tensor, grad: Tensor, *state: Optional[Tensor]):
    """What every optimizer step asks of ``param``, ``grad`` and the state tensors it is given: on the device, fp32,
    contiguous, one size.  Returns the leading arguments of its entry point: their pointers, then the element count."""
    _need_cuda(param, grad, *state)
    for t in (param, grad, *state):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == param.numel())
    return (*map(_p, (param, grad, *state)), param.numel())


def _skip(skip: Optional[Tensor], param: Tensor):
    """Pointer of the optional 64-element-block skip mask of the flat-buffer optimizer steps."""
    if skip is None:
        return None
    _need_cuda(skip)
    assert skip.dtype == torch.uint8 and skip.is_contiguous() and skip.numel() * 64 >= param.numel()
    return skip.data_ptr()


def _mirror(mirror: Optional[Tensor], param: Tensor):
    """(pointer, dtype code) of the optional 16-bit mirror that a one-launch step writes the updated weights into."""
    if mirror is None:
        return None, 0
    _need_cuda(mirror)
    assert mirror.numel() == param.numel() and mirror.is_contiguous() and mirror.dtype in (torch.bfloat16, torch.float16)
    return mirror.data_ptr(), _DT[mirror.dtype]


def adamw_step_(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, *, lr: float, beta1: float,
                beta2: float, eps: float, weight_decay: float, step: int) -> None:
    L.check(L.load().dvt_adamw_step(*_flat_f32(param, grad, exp_avg, exp_avg_sq), lr, beta1, beta2, eps, weight_decay,
                                    step, _stream()), "dvt_adamw_step")


def adamw_step_dev_(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, step_dev: Tensor, *,
                    lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
                    skip: Optional[Tensor] = None) -> None:
    """AdamW with the step counter on the device (hipGraph-capturable)."""
    _need_cuda(step_dev)
    assert step_dev.dtype == torch.int64 and step_dev.numel() == 1
    L.check(L.load().dvt_adamw_step_dev(*_flat_f32(param, grad, exp_avg, exp_avg_sq), lr, beta1, beta2, eps, weight_decay,
                                        step_dev.data_ptr(), _skip(skip, param), _stream()), "dvt_adamw_step_dev")


def adamw_step_fused_(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, step_dev2: Tensor, *,
                      lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
                      skip: Optional[Tensor] = None, mirror: Optional[Tensor] = None) -> None:
    """AdamW + the 16-bit weight mirror + the device step counter (int64[2]: steps, ticket) in one launch."""
    _need_cuda(step_dev2)
    assert step_dev2.dtype == torch.int64 and step_dev2.numel() == 2
    L.check(L.load().dvt_adamw_step_fused(*_flat_f32(param, grad, exp_avg, exp_avg_sq), lr, beta1, beta2, eps, weight_decay,
                                          step_dev2.data_ptr(), _skip(skip, param), *_mirror(mirror, param), _stream()),
            "dvt_adamw_step_fused")


def adamw_step_scaled_(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, step_dev: Tensor, scale: Tensor,
                       found_inf: Tensor, good_steps: Tensor, loss_grad: Tensor, *, lr: float, beta1: float, beta2: float,
                       eps: float, weight_decay: float, growth_interval: int, growth: float, backoff: float,
                       loss_grad_base: float, skip: Optional[Tensor] = None) -> None:
    """AdamW under dynamic loss scaling, all scaler state on the device (hipGraph-capturable)."""
    _need_cuda(step_dev, scale, found_inf, good_steps, loss_grad)
    assert found_inf.dtype == torch.int32 and good_steps.dtype == torch.int32 and step_dev.dtype == torch.int64
    L.check(L.load().dvt_adamw_step_scaled(*_flat_f32(param, grad, exp_avg, exp_avg_sq), lr, beta1, beta2, eps, weight_decay,
                                           step_dev.data_ptr(), scale.data_ptr(), found_inf.data_ptr(), good_steps.data_ptr(),
                                           growth_interval, growth, backoff, loss_grad.data_ptr(), loss_grad_base,
                                           _skip(skip, param), _stream()), "dvt_adamw_step_scaled")


def adam_step_dev_(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, step_dev2: Tensor, lr_dev: Tensor, *,
                   beta1: float, beta2: float, eps: float, weight_decay: float, skip: Optional[Tensor] = None,
                   mirror: Optional[Tensor] = None) -> None:
    """torch.optim.Adam (coupled L2 decay) + optional 16-bit mirror + device step counter (int64[2]) in one launch; the
    learning rate is read from the device scalar ``lr_dev`` (f32)."""
    _need_cuda(step_dev2, lr_dev)
    assert step_dev2.dtype == torch.int64 and step_dev2.numel() == 2 and lr_dev.dtype == torch.float32
    L.check(L.load().dvt_adam_step_dev(*_flat_f32(param, grad, exp_avg, exp_avg_sq), lr_dev.data_ptr(), beta1, beta2, eps,
                                       weight_decay, step_dev2.data_ptr(), _skip(skip, param), *_mirror(mirror, param),
                                       _stream()), "dvt_adam_step_dev")


def sgd_step_(param: Tensor, grad: Tensor, momentum_buf: Optional[Tensor], *, lr: float, momentum: float,
              weight_decay: float, skip: Optional[Tensor] = None) -> None:
    L.check(L.load().dvt_sgd_step(*_flat_f32(param, grad, momentum_buf), lr, momentum, weight_decay, _skip(skip, param),
                                  _stream()), "dvt_sgd_step")


def adagrad_step_(param: Tensor, grad: Tensor, state_sum: Tensor, *, lr: float, lr_decay: float, eps: float,
                  weight_decay: float, step: int, skip: Optional[Tensor] = None) -> None:
    L.check(L.load().dvt_adagrad_step(*_flat_f32(param, grad, state_sum), lr, lr_decay, eps, weight_decay, step,
                                      _skip(skip, param), _stream()), "dvt_adagrad_step")


LarsSeg = L.STRUCTS["dvt_lars_seg"]
LarsPlanInfo = L.STRUCTS["dvt_lars_plan_info"]


class LarsPlan(NamedTuple):
    chunk: int                # elements per chunk
    blocks: int               # blocks per launch: sum of ceil(numel / chunk)
    grid_cap: int             # 0: none
    workspace_bytes: int
    chunk_begin: Tuple[int, ...]      # first chunk of every segment, then the total


def lars_plan(numels) -> LarsPlan:
    """How ``dvt_lars_sumsq`` / ``dvt_lars_step`` cut tensors of these sizes into chunks (host only, no GPU needed)."""
    numels = [int(n) for n in numels]
    arr, begin, info = (C.c_int64 * len(numels))(*numels), (C.c_int64 * (len(numels) + 1))(), LarsPlanInfo()
    L.check(L.load().dvt_lars_plan(C.cast(arr, C.c_void_p), len(numels), C.byref(info), C.cast(begin, C.c_void_p)),
            "dvt_lars_plan")
    return LarsPlan(info.chunk, info.blocks, info.grid_cap, info.workspace_bytes, tuple(begin))


class LarsTable:
    """The device segment table of one LARS call, its plan and its workspace.  Holds the tensors it points into, and the
    host rows in pinned memory, so that ``set_grads`` can point the same table at other gradient tensors."""

    def __init__(self, rows, pinned: Tensor, plan: LarsPlan, keep, mirror_dtype: int, device):
        self.rows, self.pinned, self.plan, self.keep, self.mirror_dtype = rows, pinned, plan, keep, mirror_dtype
        self.n = len(plan.chunk_begin) - 1
        self.has_buf = all(k[2] is not None for k in keep)
        self.table = torch.empty(pinned.numel(), dtype=torch.uint8, device=device)
        self.workspace = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=device)
        self._uploaded = None
        self._upload()

    def _upload(self):
        """Host rows -> device table on the current stream, without waiting for it.  The rows are pinned memory that the
        copy reads later, so they are written again only after the previous copy is over (an event that has long fired
        by the next step; no other wait)."""
        self.table.copy_(self.pinned, non_blocking=True)
        self._uploaded = torch.cuda.Event()
        self._uploaded.record()

    def grad_ptrs(self):
        return tuple(k[1].data_ptr() for k in self.keep)

    def set_grads(self, grads) -> None:
        """The same segments with other gradient tensors (torch's ``zero_grad(set_to_none=True)`` gives every step fresh
        ones): only the gradient pointers change; table, workspace and plan stay, and the former gradients are let go."""
        grads = list(grads)
        assert len(grads) == self.n
        self._uploaded.synchronize()
        for r, k, g in zip(self.rows, self.keep, grads):
            _, r.grad, _ = _flat_f32(g if k[0] is None else k[0], g)      # (k[0] None: a row of ``grad_table``)
        self.keep = [(k[0], g, k[2], k[3]) for k, g in zip(self.keep, grads)]
        self._upload()


def lars_table(segments) -> LarsTable:
    """segments: (param, grad, momentum_buf or None, mirror or None, weight_decay) per tensor with a gradient; empty tensors
    are left out.  Every tensor obeys the optimizer steps' contract (``_flat_f32``, ``_mirror``); mirrors are given for all
    segments or for none, in one dtype.  The table is built on the host and copied to the device once."""
    segments = [s for s in segments if s[0].numel() > 0]
    if not segments:
        raise ValueError("lars_table: no segments")
    _need_cuda(*(t for s in segments for t in s[:4]))
    plan = lars_plan(s[0].numel() for s in segments)
    pinned = torch.empty(C.sizeof(LarsSeg) * len(segments), dtype=torch.uint8, pin_memory=True)
    rows, keep, mdts = (LarsSeg * len(segments)).from_address(pinned.data_ptr()), [], set()
    for r, (p, g, buf, mirror, wd), begin in zip(rows, segments, plan.chunk_begin):
        r.param, r.grad, r.buf, r.numel = _flat_f32(p, g, buf)
        r.mirror, mdt = _mirror(mirror, p)
        r.chunk_begin, r.weight_decay, r.reserved = begin, float(wd), 0
        mdts.add(mdt)
        keep.append((p, g, buf, mirror))
    if len(mdts) != 1:
        raise ValueError("lars_table: give a 16-bit mirror of one dtype for every segment, or for none")
    return LarsTable(rows, pinned, plan, keep, mdts.pop(), segments[0][0].device)


def lars_sumsq(t: LarsTable) -> Tensor:
    """-> f32 [segments, 2]: sum of p^2 and of g^2 per segment, the values ``lars_step_`` forms its norms from."""
    out = torch.empty((t.n, 2), dtype=torch.float32, device=t.table.device)
    L.check(L.load().dvt_lars_sumsq(C.cast(t.table.data_ptr(), C.POINTER(LarsSeg)), t.n, t.plan.blocks,
                                    t.workspace.data_ptr(), out.data_ptr(), _stream()), "dvt_lars_sumsq")
    return out


def lars_step_(t: LarsTable, lr_dev: Tensor, step_dev2: Tensor, *, momentum: float = 0.0, dampening: float = 0.0,
               nesterov: bool = False, trust_coefficient: float = 0.001, eps: float = 1e-8) -> None:
    """One LARS step over the table's segments in two launches (norms, update); the learning rate is read from the
    device scalar ``lr_dev`` (f32), the first-step rule from the device counter ``step_dev2`` (int64[2])."""
    _need_cuda(step_dev2, lr_dev)
    assert step_dev2.dtype == torch.int64 and step_dev2.numel() == 2 and lr_dev.dtype == torch.float32
    if momentum != 0 and not t.has_buf:
        raise ValueError("lars_step_: momentum != 0 needs a momentum buffer for every segment")
    L.check(L.load().dvt_lars_step(C.cast(t.table.data_ptr(), C.POINTER(LarsSeg)), t.n, t.plan.blocks,
                                   t.workspace.data_ptr(), lr_dev.data_ptr(), momentum, dampening, int(bool(nesterov)),
                                   trust_coefficient, eps, step_dev2.data_ptr(), int(t.mirror_dtype != 0), t.mirror_dtype,
                                   _stream()), "dvt_lars_step")


# ------------------------------------------------------------------ global gradient norm and clip (csrc/optim.hip)
def grad_table(grads) -> LarsTable:
    """A segment table over gradients alone, for ``grad_norm`` / ``grad_clip_``: the rows, plan, workspace and upload of
    ``lars_table`` with no parameter, buffer or mirror pointer (those kernels read ``grad`` and ``numel`` only).  Empty
    tensors are left out."""
    grads = [g for g in grads if g.numel() > 0]
    if not grads:
        raise ValueError("grad_table: no gradients")
    _need_cuda(*grads)
    plan = lars_plan(g.numel() for g in grads)
    pinned = torch.empty(C.sizeof(LarsSeg) * len(grads), dtype=torch.uint8, pin_memory=True)
    rows, keep = (LarsSeg * len(grads)).from_address(pinned.data_ptr()), []
    for r, g, begin in zip(rows, grads, plan.chunk_begin):
        _, r.grad, r.numel = _flat_f32(g, g)
        r.param, r.buf, r.mirror = None, None, None
        r.chunk_begin, r.weight_decay, r.reserved = begin, 0.0, 0
        keep.append((None, g, None, None))
    return LarsTable(rows, pinned, plan, keep, 0, grads[0].device)


def norm_kind(norm_type) -> int:
    """``norm_type`` of torch.nn.utils.clip_grad_norm_ -> dvt_norm_kind; 2 and inf have kernels."""
    if isinstance(norm_type, (int, float)) and float(norm_type) == 2.0:
        return L.ENUMS["dvt_norm_kind"]["DVT_NORM_2"]
    if isinstance(norm_type, (int, float)) and float(norm_type) == float("inf"):
        return L.ENUMS["dvt_norm_kind"]["DVT_NORM_INF"]
    raise NotImplementedError(f"norm_type={norm_type!r}: the gradient norm kernels compute the 2-norm and the inf-norm")


def grad_norm(t: LarsTable, norm_type=2.0, *, raw: bool = False) -> Tensor:
    """-> f32 [1] on the device: the ``norm_type`` norm (2 or inf) of all gradients of the table taken as one vector, in
    two launches (partials, total).  ``raw``: the reduced total itself instead -- the sum of squares for norm_type 2 (the maximum either way
    for inf)."""
    out = torch.empty(2, dtype=torch.float32, device=t.table.device)
    L.check(L.load().dvt_grad_norm(C.cast(t.table.data_ptr(), C.POINTER(LarsSeg)), t.n, t.plan.blocks,
                                   t.workspace.data_ptr(), norm_kind(norm_type), out.data_ptr(), _stream()),
            "dvt_grad_norm")
    return out[1:2] if raw else out[0:1]


def grad_clip_(t: LarsTable, max_norm: float, norm_type=2.0, inv_scale: Optional[Tensor] = None, *,
               scale: Optional[Tensor] = None) -> Tensor:
    """torch.nn.utils.clip_grad_norm_ over the table's gradients in two launches: g *= min(1, max_norm / (norm * s + 1e-6))
    in place, s = ``inv_scale[0]`` or ``1 / scale[0]`` (device fp32 scalars; give at most one -- ``scale`` is the loss scale
    as ``adamw_step_scaled_`` holds it) or 1.  -> f32 [1] on the device: norm * s, the norm before clipping.  A non-finite
    norm leaves the gradients as they are (``dvt_grad_clip`` in include/dvt_hip.h)."""
    if inv_scale is not None and scale is not None:
        raise ValueError("grad_clip_: give inv_scale or scale, not both")
    s = inv_scale if inv_scale is not None else scale
    if s is not None:
        _need_cuda(s)
        assert s.dtype == torch.float32 and s.numel() == 1
    out = torch.empty(1, dtype=torch.float32, device=t.table.device)
    L.check(L.load().dvt_grad_clip(C.cast(t.table.data_ptr(), C.POINTER(LarsSeg)), t.n, t.plan.blocks,
                                   t.workspace.data_ptr(), norm_kind(norm_type), float(max_norm), _p(s),
                                   int(inv_scale is not None), out.data_ptr(), _stream()), "dvt_grad_clip")
    return out


# ------------------------------------------------------------------ grouped AdamW and weight EMA (csrc/optim_groups.hip)
class AdamwGroupTable:
    """The device side of a parameter grouping: ``group64`` (uint8, one byte per 64 elements, the row each block takes)
    and ``table`` (f32 [ngroups, 2] = {lr_scale, weight_decay}).  Built by ``adamw_group_table``."""

    def __init__(self, group64: Tensor, table: Tensor):
        self.group64, self.table, self.ngroups = group64, table, int(table.shape[0])


def adamw_group_table(group64, lr_scales, weight_decays) -> AdamwGroupTable:
    """group64: uint8 [ceil(n / 64)] (any device; it is validated on the host and copied to the GPU), one row index per
    64-element block; lr_scales / weight_decays: one value per group.  Every map byte must be below the number of groups:
    the kernel cannot refuse a bad one, so this is checked here, once.  Not to be built inside a hipGraph capture."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("adamw_group_table builds its device map and table when it is called; make that call in a "
                           "warm-up step, not inside a hipGraph capture")
    lr_scales, weight_decays = [float(s) for s in lr_scales], [float(w) for w in weight_decays]
    ngroups = len(lr_scales)
    if len(weight_decays) != ngroups:
        raise ValueError(f"adamw_group_table: {ngroups} lr_scales for {len(weight_decays)} weight_decays")
    if not 1 <= ngroups <= 255:
        raise ValueError(f"adamw_group_table: ngroups must be in 1 .. 255, got {ngroups}")
    g = torch.as_tensor(group64)
    if g.dtype != torch.uint8 or g.dim() != 1:
        raise TypeError("adamw_group_table: group64 must be a one-dimensional uint8 tensor")
    host = g.cpu()
    if host.numel() and int(host.max()) >= ngroups:
        bad = int((host >= ngroups).nonzero()[0])
        raise ValueError(f"adamw_group_table: map byte {int(host[bad])} at block {bad} is not below ngroups = {ngroups}")
    if not torch.cuda.is_available():
        raise RuntimeError("libdvt_hip operators need tensors on the GPU (HIP device); there is no CPU path")
    dev = g.device if g.is_cuda else torch.device("cuda", torch.cuda.current_device())
    table = torch.tensor(list(zip(lr_scales, weight_decays)), dtype=torch.float32).reshape(ngroups, 2)
    return AdamwGroupTable(host.contiguous().to(dev), table.to(dev))


def adamw_groups_step_(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, step_dev2: Tensor, lr_dev: Tensor,
                       table: AdamwGroupTable, *, beta1: float, beta2: float, eps: float, skip: Optional[Tensor] = None,
                       mirror: Optional[Tensor] = None, ema: Optional[Tensor] = None,
                       ema_decay: Optional[Tensor] = None) -> None:
    """AdamW with the rate ``lr_dev[0] * lr_scale`` and the weight decay of each 64-element block's group + the 16-bit
    mirror + the device step counter (int64[2]) in one launch; with ``ema`` (f32, the size of ``param``) the weight EMA
    under the device scalar ``ema_decay`` as well, for every element."""
    _need_cuda(step_dev2, lr_dev, table.group64, table.table, ema, ema_decay)
    assert step_dev2.dtype == torch.int64 and step_dev2.numel() == 2 and lr_dev.dtype == torch.float32
    assert table.group64.numel() * 64 >= param.numel()
    assert ema is None or (ema.dtype == torch.float32 and ema.is_contiguous() and ema.numel() == param.numel())
    assert ema_decay is None or ema_decay.dtype == torch.float32
    L.check(L.load().dvt_adamw_groups_step(*_flat_f32(param, grad, exp_avg, exp_avg_sq), lr_dev.data_ptr(), beta1, beta2, eps,
                                           table.group64.data_ptr(), table.table.data_ptr(), table.ngroups,
                                           step_dev2.data_ptr(), _skip(skip, param), *_mirror(mirror, param), _p(ema),
                                           _p(ema_decay), _stream()), "dvt_adamw_groups_step")


def ema_update_(ema: Tensor, param: Tensor, decay_dev: Tensor) -> None:
    """ema = d ema + (1 - d) param in place, d = ``decay_dev[0]`` (f32 device scalar): one streaming launch."""
    _need_cuda(ema, param, decay_dev)
    assert ema.dtype == param.dtype == decay_dev.dtype == torch.float32 and ema.is_contiguous() and param.is_contiguous()
    assert ema.numel() == param.numel()
    L.check(L.load().dvt_ema_update(ema.data_ptr(), param.data_ptr(), param.numel(), decay_dev.data_ptr(), _stream()),
            "dvt_ema_update")


# ------------------------------------------------------------------ per-frame CNN encoder (csrc/conv.hip)
def _pair(v):
    return (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))


def conv_out_hw(H: int, W: int, k, stride, pad) -> Tuple[int, int]:
    (kh, kw), (sh, sw), (ph, pw) = _pair(k), _pair(stride), _pair(pad)
    return (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1


def im2col(x: Tensor, nchw: bool, N: int, Cc: int, H: int, W: int, k, stride, pad, ld: int,
           out_dtype: torch.dtype) -> Tensor:
    """k / stride / pad: int or (h, w) pair."""
    _need_cuda(x)
    assert x.is_contiguous()
    (kh, kw), (sh, sw), (ph, pw) = _pair(k), _pair(stride), _pair(pad)
    Ho, Wo = conv_out_hw(H, W, k, stride, pad)
    out = torch.empty((N * Ho * Wo, ld), dtype=out_dtype, device=x.device)
    L.check(L.load().dvt_im2col(x.data_ptr(), dt(x), int(nchw), out.data_ptr(), _DT[out_dtype], N, Cc, H, W, kh, kw,
                                sh, sw, ph, pw, ld, _stream()), "dvt_im2col")
    return out


def col2im(dcol: Tensor, N: int, Cc: int, H: int, W: int, k, stride, pad, *, add: Optional[Tensor] = None,
           add_stride: int = 0) -> Tensor:
    """add: a second gradient path into the same map, summed in the same pass -- [N*H*W, C] (add_stride 0), or the compact
    gradient of the map's stride-``add_stride`` subsampling, added at the pixels that subsampling reads."""
    _need_cuda(dcol, add)
    assert dcol.is_contiguous()
    (kh, kw), (sh, sw), (ph, pw) = _pair(k), _pair(stride), _pair(pad)
    dx = torch.empty((N * H * W, Cc), dtype=dcol.dtype, device=dcol.device)
    if add is not None:
        s_ = add_stride
        rows = N * H * W if s_ == 0 else N * ((H + s_ - 1) // s_) * ((W + s_ - 1) // s_)
        assert add.is_contiguous() and add.dtype == dcol.dtype and tuple(add.shape) == (rows, Cc)
    L.check(L.load().dvt_col2im(dcol.data_ptr(), dx.data_ptr(), N, Cc, H, W, kh, kw, sh, sw, ph, pw, dcol.shape[1],
                                _p(add), add_stride, dt(dcol), _stream()), "dvt_col2im")
    return dx


def col2im_nchw(dcol: Tensor, N: int, Cc: int, H: int, W: int, k, stride, pad, dx_dtype: torch.dtype) -> Tensor:
    """Adjoint gather written as an NCHW tensor [N, C, H, W] in ``dx_dtype`` (stem input gradient)."""
    _need_cuda(dcol)
    assert dcol.is_contiguous()
    (kh, kw), (sh, sw), (ph, pw) = _pair(k), _pair(stride), _pair(pad)
    dx = torch.empty((N, Cc, H, W), dtype=dx_dtype, device=dcol.device)
    L.check(L.load().dvt_col2im_nchw(dcol.data_ptr(), dt(dcol), dx.data_ptr(), _DT[dx_dtype], N, Cc, H, W, kh, kw, sh,
                                     sw, ph, pw, dcol.shape[1], _stream()), "dvt_col2im_nchw")
    return dx


def _conv_desc(x: Tensor, wp: Tensor, y, N, Cc, H, W, Cout, k, stride, pad, trim_w: int = 0):
    (kh, kw), (sh, sw), (ph, pw) = _pair(k), _pair(stride), _pair(pad)
    d = L.ConvDesc()
    d.x, d.w, d.y = x.data_ptr(), wp.data_ptr(), (y.data_ptr() if y is not None else 1 << 4)
    d.N, d.H, d.W, d.C, d.Cout = N, H, W, Cc, Cout
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw = kh, kw, sh, sw, ph, pw
    d.dtype = dt(x)
    d.trim_w = trim_w
    return d


def conv2d_implicit_k(Cc: int, Cout: int, k) -> int:
    """Row length of the packed weights the implicit forward expects (kh*kw*C; rounded up to the k-tile for C == 8)."""
    (kh, kw) = _pair(k)
    d = L.ConvDesc()
    d.C, d.Cout, d.kh, d.kw = Cc, Cout, kh, kw
    return int(L.load().dvt_conv2d_implicit_k(C.byref(d)))


def conv2d_implicit_supported(x: Tensor, wp: Tensor, N, Cc, H, W, Cout, k, stride, pad, trim_w: int = 0) -> bool:
    if not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float16) or wp.dtype != x.dtype:
        return False
    if not (x.is_contiguous() and wp.is_contiguous() and wp.shape == (Cout, conv2d_implicit_k(Cc, Cout, k))):
        return False
    return bool(L.load().dvt_conv2d_implicit_supported(C.byref(_conv_desc(x, wp, None, N, Cc, H, W, Cout, k, stride, pad, trim_w))))


def nchw_to_nhwc_pad(x: Tensor, dtype: torch.dtype, cpad: int = 8) -> Tensor:
    """Raw frames [N, C, H, W] -> the stem's input form in ``dtype``: cpad 8 = NHWC matrix [N*H*W, 8] (channels C.. zero);
    cpad 4 (C <= 4, W even) = [N*H*(W/2), 8], one row per pair of horizontally adjacent pixels (4 channels each)."""
    _need_cuda(x)
    x = x.contiguous()
    N, Cc, H, W = x.shape
    y = torch.empty((N * H * W * cpad // 8, 8), dtype=dtype, device=x.device)
    L.check(L.load().dvt_nchw_to_nhwc_pad(x.data_ptr(), dt(x), y.data_ptr(), _DT[dtype], N, Cc, H, W, cpad, _stream()),
            "dvt_nchw_to_nhwc_pad")
    return y


def conv_weight_pairs(w: Tensor, Cout: int, Cin: int, kh: int, kw: int, pw: int, kwp: int) -> Tensor:
    """Stem weights f32 [Cout, Cin <= 4, kh, kw] -> pixel-pair form f32 [Cout, 8, kh, kwp] (dvt_conv_weight_pairs)."""
    _need_cuda(w)
    w = w.detach().contiguous()
    assert w.dtype == torch.float32 and w.numel() == Cout * Cin * kh * kw
    out = torch.empty((Cout, 8, kh, kwp), dtype=torch.float32, device=w.device)
    L.check(L.load().dvt_conv_weight_pairs(w.data_ptr(), out.data_ptr(), Cout, Cin, kh, kw, pw, kwp, _stream()),
            "dvt_conv_weight_pairs")
    return out


def conv_weight_pairs_bwd(dwp: Tensor, Cout: int, Cin: int, kh: int, kw: int, pw: int, kwp: int, *,
                          out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """Adjoint: f32 [Cout, 8, kh, kwp] -> f32 [Cout, Cin, kh, kw] (+= into ``out`` when accumulate)."""
    _need_cuda(dwp)
    assert dwp.dtype == torch.float32 and dwp.is_contiguous() and dwp.numel() == Cout * 8 * kh * kwp
    if out is None:
        assert not accumulate
        out = torch.empty((Cout, Cin, kh, kw), dtype=torch.float32, device=dwp.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == Cout * Cin * kh * kw
    L.check(L.load().dvt_conv_weight_pairs_bwd(dwp.data_ptr(), out.data_ptr(), Cout, Cin, kh, kw, pw, kwp, int(accumulate),
                                               _stream()), "dvt_conv_weight_pairs_bwd")
    return out


def conv_stem7_supported(xp: Tensor, wp: Tensor, N: int, H: int, Wp: int) -> bool:
    """Does dvt_conv_stem7 take this stem?  xp: the pixel-pair map [N*H*Wp, 8] (nchw_to_nhwc_pad(.., 4)), wp [64, >= 224]."""
    if not xp.is_cuda or xp.dtype not in (torch.bfloat16, torch.float16) or wp.dtype != xp.dtype:
        return False
    if not (xp.is_contiguous() and wp.is_contiguous() and xp.numel() == N * H * Wp * 8 and wp.dim() == 2 and wp.shape[0] == 64
            and wp.shape[1] >= 224 and wp.shape[1] % 8 == 0):
        return False
    return bool(L.load().dvt_conv_stem7_supported(N, H, Wp, dt(xp)))


def conv_stem7(xp: Tensor, wp: Tensor, N: int, H: int, Wp: int, want_stats: bool = False):
    """The 7x7 / 2 / 3 stem on the pixel-pair map from an LDS halo patch, weights in registers (dvt_conv_stem7): same result
    and statistics contract as conv2d_implicit with the pair geometry ((7, 4) / (2, 1) / (3, 2), trim_w = 1).
    -> z [N * (H/2) * Wp, 64] (, partial, parts)."""
    _need_cuda(xp, wp)
    Ho = H // 2
    y = torch.empty((N * Ho * Wp, 64), dtype=xp.dtype, device=xp.device)
    lib = L.load()
    partial, parts = None, 0
    if want_stats:
        parts = int(lib.dvt_conv_stem7_stats_parts(N, H, Wp))
        partial = workspace((parts + 64) * 2 * 64 * 4, xp.device, slot="bn_partial")
    nb = (xp.numel() + y.numel() + wp.numel()) * xp.element_size()
    with _timed(("conv", "stem7", N * Ho * Wp, 64, 224, nb), 2.0 * N * Ho * Wp * 64 * 224):
        L.check(lib.dvt_conv_stem7(xp.data_ptr(), wp.data_ptr(), wp.shape[1], y.data_ptr(), _p(partial), N, H, Wp, dt(xp),
                                   _stream()), "dvt_conv_stem7")
    return (y, partial, parts) if want_stats else y


def conv3x3_c64_supported(x: Tensor, wp: Tensor, N: int, H: int, W: int) -> bool:
    if not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float16) or wp.dtype != x.dtype:
        return False
    if not (x.is_contiguous() and wp.is_contiguous() and tuple(wp.shape) == (64, 576) and x.shape == (N * H * W, 64)):
        return False
    return bool(L.load().dvt_conv3x3_c64_supported(N, H, W, dt(x)))


def conv3x3_c64(x: Tensor, wp: Tensor, N: int, H: int, W: int, want_stats: bool = False, residual: Optional[Tensor] = None):
    """3x3 / 1 / 1 convolution, 64 -> 64 channels, from an LDS-resident halo patch (dvt_conv3x3_c64); same contract as
    conv2d_implicit (residual: added to the output)."""
    _need_cuda(x, wp, residual)
    y = torch.empty((N * H * W, 64), dtype=x.dtype, device=x.device)
    if residual is not None:
        assert residual.is_contiguous() and residual.dtype == x.dtype and residual.shape == y.shape
    lib = L.load()
    partial, parts = None, 0
    if want_stats:
        parts = int(lib.dvt_conv3x3_c64_stats_parts(N, H, W))
        partial = workspace((parts + 64) * 2 * 64 * 4, x.device, slot="bn_partial")
    with _timed(("conv", "halo3x3_c64", N * H * W, 64, 576, (2 * x.numel() + wp.numel()) * x.element_size()), 2.0 * N * H * W * 64 * 576):
        L.check(lib.dvt_conv3x3_c64(x.data_ptr(), wp.data_ptr(), y.data_ptr(), _p(partial), _p(residual), N, H, W, dt(x),
                                    _stream()), "dvt_conv3x3_c64")
    return (y, partial, parts) if want_stats else y


_STREAM_PAIRS = ((64, 144), (144, 64), (128, 288), (288, 128))


def conv3x3_stream_supported(x: Tensor, wp: Tensor, N: int, H: int, W: int, Cin: int, Cout: int) -> bool:
    if not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float16) or wp.dtype != x.dtype:
        return False
    if (Cin, Cout) not in _STREAM_PAIRS:
        return False
    if not (x.is_contiguous() and wp.is_contiguous() and tuple(wp.shape) == (Cout, 9 * Cin) and x.shape == (N * H * W, Cin)):
        return False
    return bool(L.load().dvt_conv3x3_stream_supported(N, H, W, Cin, Cout, dt(x)))


def conv3x3_stream_geometry(N: int, H: int, W: int, Cin: int, Cout: int, dtype: torch.dtype) -> bool:
    """Whether dvt_conv3x3_stream takes this (frames, map, channel pair): what a model needs to know before it decides the
    channel padding of the layer (no tensors yet)."""
    if dtype not in (torch.bfloat16, torch.float16):
        return False
    return bool(L.load().dvt_conv3x3_stream_supported(N, H, W, Cin, Cout, _DT[dtype]))


def conv3x3_stream(x: Tensor, wp: Tensor, N: int, H: int, W: int, Cin: int, Cout: int, want_stats: bool = False,
                   residual: Optional[Tensor] = None):
    """3x3 / 1 / 1 convolution 64 -> 144 / 144 -> 64 (layer 1 of R(2+1)D-18) or 128 -> 288 / 288 -> 128 (layer 2) from LDS halo
    patches with streamed weights (dvt_conv3x3_stream); same contract as conv3x3_c64 (statistics with the 144- / 288-wide
    output, residual with the 64- / 128-wide one)."""
    _need_cuda(x, wp, residual)
    y = torch.empty((N * H * W, Cout), dtype=x.dtype, device=x.device)
    if residual is not None:
        assert residual.is_contiguous() and residual.dtype == x.dtype and residual.shape == y.shape
    lib = L.load()
    partial, parts = None, 0
    if want_stats:
        parts = int(lib.dvt_conv3x3_stream_stats_parts(N, H, W, Cin, Cout))
        partial = workspace((parts + 64) * 2 * Cout * 4, x.device, slot="bn_partial")
    nb = (x.numel() + y.numel() + wp.numel()) * x.element_size()
    with _timed(("conv", "halo3x3_stream", N * H * W, Cout, 9 * Cin, nb), 2.0 * N * H * W * Cout * 9 * Cin):
        L.check(lib.dvt_conv3x3_stream(x.data_ptr(), wp.data_ptr(), y.data_ptr(), _p(partial), _p(residual), N, H, W, Cin, Cout,
                                       dt(x), _stream()), "dvt_conv3x3_stream")
    return (y, partial, parts) if want_stats else y


def conv3x1_stream_supported(x: Tensor, wp: Tensor, N: int, T: int, HW: int, Cin: int, Cout: int) -> bool:
    if not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float16) or wp.dtype != x.dtype or (Cin, Cout) != (64, 144):
        return False
    if not (x.is_contiguous() and wp.is_contiguous() and tuple(wp.shape) == (Cout, 3 * Cin) and x.shape == (N * T * HW, Cin)):
        return False
    return bool(L.load().dvt_conv3x1_stream_supported(N, T, HW, Cin, Cout, dt(x)))


def conv3x1_stream(x: Tensor, wp: Tensor, N: int, T: int, HW: int, Cin: int, Cout: int) -> Tensor:
    """(3, 1) / 1 / (1, 0) convolution 64 -> 144 over the [T, HW] view of N clips (dvt_conv3x1_stream): the temporal half of
    R(2+1)D's layer-1 Conv2Plus1D as its data gradient."""
    _need_cuda(x, wp)
    y = torch.empty((N * T * HW, Cout), dtype=x.dtype, device=x.device)
    nb = (x.numel() + y.numel() + wp.numel()) * x.element_size()
    with _timed(("conv", "halo3x3_stream", N * T * HW, Cout, 3 * Cin, nb), 2.0 * N * T * HW * Cout * 3 * Cin):
        L.check(L.load().dvt_conv3x1_stream(x.data_ptr(), wp.data_ptr(), y.data_ptr(), N, T, HW, Cin, Cout, dt(x), _stream()),
                 "dvt_conv3x1_stream")
    return y


def conv3x1_stream_bn_bwd(dy: Tensor, wp: Tensor, z: Tensor, affine, N: int, T: int, HW: int, training: bool, *,
                          dgamma: Optional[Tensor] = None, dbeta: Optional[Tensor] = None, accumulate: bool = False):
    """Data gradient of the (3, 1) temporal convolution 144 -> 64 (as ``conv3x1_stream``) with the backward of the BatchNorm
    (+ ReLU) in front of that layer fused in (dvt_conv3x1_stream_bn_bwd): dy [N*T*HW, 64], z [N*T*HW, 144] the spatial half's
    output, affine = (mean, invstd, gamma, beta, c_valid, relu) of the BatchNorm that normalised it
    -> (dz [N*T*HW, 144], dgamma, dbeta).  The 144-plane data gradient is never stored (computed twice instead)."""
    _need_cuda(dy, wp, z)
    assert dy.dtype == z.dtype and z.shape == (N * T * HW, 144) and dy.shape == (N * T * HW, 64)
    aff, keep = _bn_affine(affine)
    if dgamma is None:
        assert not accumulate
        dgamma = torch.empty((144,), dtype=torch.float32, device=z.device)
        dbeta = torch.empty((144,), dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z)
    lib = L.load()
    ws = workspace(lib.dvt_conv3x1_stream_bn_bwd_workspace_bytes(N, T, HW), z.device)
    esz = z.element_size()
    nb = 2 * (dy.numel() + z.numel() + wp.numel()) * esz + dz.numel() * esz
    with _timed(("conv", "stream3x1_bn_bwd", N * T * HW, 144, 3 * 64, nb), 2 * 2.0 * N * T * HW * 144 * 3 * 64):
        L.check(lib.dvt_conv3x1_stream_bn_bwd(dy.data_ptr(), wp.data_ptr(), z.data_ptr(), C.byref(aff), dz.data_ptr(),
                                              dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), N, T, HW, int(training),
                                              int(accumulate), dt(z), _stream()), "dvt_conv3x1_stream_bn_bwd")
    return dz, dgamma, dbeta


def conv3x3_c64_wgrad_supported(x: Tensor, dz: Tensor, N: int, H: int, W: int, Cout: int = 64) -> bool:
    if not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float16) or dz.dtype != x.dtype:
        return False
    if Cout < 64 or Cout % 16:
        return False
    if not (x.is_contiguous() and dz.is_contiguous() and x.shape == (N * H * W, 64) and dz.shape == (N * H * W, Cout)):
        return False
    return bool(L.load().dvt_conv3x3_c64_wgrad_supported(N, H, W, dt(x)))


def conv3x3_c64_wgrad(x: Tensor, dz: Tensor, N: int, H: int, W: int, master: Tensor, *, accumulate: bool = False,
                      defer_reduce: bool = False, Cout: int = 64):
    """Weight gradient of the 64 -> 64 3x3 / 1 / 1 convolution from LDS halo patches (dvt_conv3x3_c64_wgrad), summed into
    ``master`` (the parameter's own gradient f32 [64, 64, 3, 3]; += when accumulate).  defer_reduce: -> pending, for
    ``splitk_reduce_pending`` / a carrying launch (the workgroups' partials live in the deferred-reduce scratch slot)."""
    _need_cuda(x, dz, master)
    assert master.dtype == torch.float32 and master.is_contiguous() and master.numel() == Cout * 64 * 9
    lib = L.load()
    pend = L.SplitKPending()
    nbytes = int(lib.dvt_conv3x3_c64_wgrad_workspace_bytes(N, H, W))
    ws = _deferred_workspace(nbytes, x.device, pend) if defer_reduce else workspace(nbytes, x.device, slot="conv3_wgrad")
    nb = (x.numel() + dz.numel()) * x.element_size() + master.numel() * 4
    with _timed(("conv", "halo3x3_c64_wgrad", 576, Cout, N * H * W, nb), 2.0 * N * H * W * Cout * 576):
        if Cout == 64:
            L.check(lib.dvt_conv3x3_c64_wgrad(x.data_ptr(), dz.data_ptr(), master.data_ptr(), ws.data_ptr(), N, H, W,
                                              int(accumulate), int(defer_reduce), C.byref(pend), dt(x), _stream()),
                    "dvt_conv3x3_c64_wgrad")
        else:       # (one launch + reduce per 64-channel group of dz over the same workspace; the last reduce deferred)
            L.check(lib.dvt_conv3x3_c64_wgrad_wide(x.data_ptr(), dz.data_ptr(), master.data_ptr(), ws.data_ptr(), N, H, W, Cout,
                                                   int(accumulate), int(defer_reduce), C.byref(pend), dt(x), _stream()),
                    "dvt_conv3x3_c64_wgrad_wide")
    if defer_reduce:
        pend._keep = (ws, master)
        return pend
    return None


def conv3x1_wgrad_supported(x: Tensor, dz: Tensor, N: int, T: int, Lp: int, Cin: int, Cout: int) -> bool:
    if not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float16) or dz.dtype != x.dtype:
        return False
    if not (x.is_contiguous() and dz.is_contiguous() and x.shape == (N * T * Lp, Cin) and dz.shape == (N * T * Lp, Cout)):
        return False
    return bool(L.load().dvt_conv3x1_wgrad_supported(N, T, Lp, Cin, Cout, dt(x)))


def _bn_affine(affine):
    """affine = (mean, invstd, gamma, beta, c_valid, relu) of the BatchNorm in front of a map, or None -> (struct, keep-alive)."""
    if affine is None:
        return None, None
    mean, invstd, gamma, beta, c_valid, relu = affine[:6]
    _need_cuda(mean, invstd, gamma, beta)
    for t in (mean, invstd, gamma, beta):
        assert t.dtype == torch.float32 and t.is_contiguous()
    a = L.BnAffine()
    a.mean, a.invstd, a.gamma, a.beta = mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    a.c_valid, a.relu = int(c_valid or 0), int(bool(relu))
    return a, (mean, invstd, gamma, beta)


def conv3x1_wgrad(x: Tensor, dz: Tensor, N: int, T: int, Lp: int, master: Tensor, *, accumulate: bool = False,
                  defer_reduce: bool = False, affine=None):
    """Weight gradient of the (3, 1) temporal convolution 144 -> 64 over the [T, H*W] view of N clips from LDS-resident
    sliding windows (dvt_conv3x1_wgrad), summed into ``master`` (f32 [64, 144, 3(, 1, 1)]; += when accumulate).
    affine: x is the convolution output in front of the BatchNorm (+ ReLU) whose (mean, invstd, gamma, beta, c_valid, relu)
    this is; the normalised activation is formed in the staged window.  defer_reduce: -> pending, as ``conv3x3_c64_wgrad``."""
    _need_cuda(x, dz, master)
    assert master.dtype == torch.float32 and master.is_contiguous() and master.numel() == 64 * 144 * 3
    lib = L.load()
    pend = L.SplitKPending()
    aff, keep = _bn_affine(affine)
    nbytes = int(lib.dvt_conv3x1_wgrad_workspace_bytes(N, T, Lp))
    ws = _deferred_workspace(nbytes, x.device, pend) if defer_reduce else workspace(nbytes, x.device, slot="conv3_wgrad")
    nb = (x.numel() + dz.numel()) * x.element_size() + master.numel() * 4
    with _timed(("conv", "window3x1_wgrad", 432, 64, N * T * Lp, nb), 2.0 * N * T * Lp * 64 * 432):
        L.check(lib.dvt_conv3x1_wgrad(x.data_ptr(), None if aff is None else C.byref(aff), dz.data_ptr(), master.data_ptr(),
                                      ws.data_ptr(), N, T, Lp, int(accumulate), int(defer_reduce), C.byref(pend), dt(x), _stream()),
                "dvt_conv3x1_wgrad")
    if defer_reduce:
        pend._keep = (ws, master, keep)
        return pend
    return None


def conv3x1_window_geometry(N: int, T: int, Lp: int, Cin: int, Cout: int, dtype: torch.dtype) -> bool:
    """Do BOTH window kernels of the (3, 1) temporal convolution (forward and weight gradient) take this geometry?  (No
    tensors needed: models/video_resnet.py asks before it decides to keep a BatchNorm virtual.)"""
    if dtype not in (torch.bfloat16, torch.float16):
        return False
    lib = L.load()
    return bool(lib.dvt_conv3x1_fwd_supported(N, T, Lp, Cin, Cout, _DT[dtype])) and \
        bool(lib.dvt_conv3x1_wgrad_supported(N, T, Lp, Cin, Cout, _DT[dtype]))


def conv3x1_fwd_plan(N: int, T: int, Lp: int, dtype: torch.dtype):
    """(position blocks per wave, pipelined) of the 144 -> 64 window forward dvt_conv3x1_fwd launches for this geometry, i.e.
    which conv3x1_fwd_kernel / conv3x1_fwd_pipe_kernel instantiation runs; None where it does not take it.  Host only."""
    if dtype not in (torch.bfloat16, torch.float16):
        return None
    npb, pipe = C.c_int(), C.c_int()
    rc = L.load().dvt_conv3x1_fwd_plan(N, T, Lp, 144, 64, _DT[dtype], C.byref(npb), C.byref(pipe))
    L.check(min(rc, 0), "dvt_conv3x1_fwd_plan")
    return (npb.value, bool(pipe.value)) if rc == 1 else None


def conv3x1_c64_plan(N: int, T: int, Lp: int, dtype: torch.dtype) -> Optional[int]:
    """Position blocks per wave (the NPB of conv3x1_c64_kernel) dvt_conv3x1_fwd launches for the 64 -> 64 form; None where it
    does not take the geometry.  Host only."""
    if dtype not in (torch.bfloat16, torch.float16):
        return None
    npb = C.c_int()
    rc = L.load().dvt_conv3x1_c64_plan(N, T, Lp, _DT[dtype], C.byref(npb))
    L.check(min(rc, 0), "dvt_conv3x1_c64_plan")
    return npb.value if rc == 1 else None


def conv3x1_wgrad_plan(N: int, T: int, Lp: int, dtype: torch.dtype) -> Optional[bool]:
    """Whether dvt_conv3x1_wgrad launches the pipelined kernel (conv3x1_wgrad_pipe_kernel) for this geometry; None where it
    does not take it.  Host only."""
    if dtype not in (torch.bfloat16, torch.float16):
        return None
    pipe = C.c_int()
    rc = L.load().dvt_conv3x1_wgrad_plan(N, T, Lp, 144, 64, _DT[dtype], C.byref(pipe))
    L.check(min(rc, 0), "dvt_conv3x1_wgrad_plan")
    return bool(pipe.value) if rc == 1 else None


class BnBwdPlan(NamedTuple):
    kernel: str      # "window": conv3x1_dbn_kernel<., nb, 1 | 2>; "stream": conv3x3_stream_kernel<., 64, 144, 3, 1 | 2>
    nb: int          # window: 16-position blocks per tile (2, 4, 6); stream: 0


def conv3x1_stream_bn_bwd_plan(N: int, T: int, HW: int, dtype: torch.dtype) -> Optional[BnBwdPlan]:
    """Which kernel pair takes dvt_conv3x1_stream_bn_bwd for this geometry; None where it is refused.  Host only."""
    if dtype not in (torch.bfloat16, torch.float16):
        return None
    kern, nb = C.c_int(), C.c_int()
    rc = L.load().dvt_conv3x1_stream_bn_bwd_plan(N, T, HW, _DT[dtype], C.byref(kern), C.byref(nb))
    L.check(min(rc, 0), "dvt_conv3x1_stream_bn_bwd_plan")
    names = {v: k[len("DVT_CONV3X1_BN_BWD_"):].lower() for k, v in L.ENUMS["dvt_conv3x1_bn_bwd_kernel"].items()}
    return BnBwdPlan(names[kern.value], nb.value) if rc == 1 else None


def conv3x3_c64_wgrad_plan(N: int, H: int, W: int, Cout: int, dtype: torch.dtype, *, rows: bool = False):
    """The launches of conv3x3_c64_wgrad: ((first dz channel, channels, MB of conv3x3_c64_wgrad_kernel), ...) -- with
    ``rows``, a fourth entry: the output rows of a frame per tile --; None where the call is refused.  Host only."""
    if dtype not in (torch.bfloat16, torch.float16):
        return None
    lib = L.load()
    n = int(lib.dvt_conv3x3_c64_wgrad_plan(N, H, W, Cout, _DT[dtype], 0, None, None, None, None))
    L.check(min(n, 0), "dvt_conv3x3_c64_wgrad_plan")
    if n == 0:
        return None
    c0, cv, mb, r = ((C.c_int * n)() for _ in range(4))
    assert int(lib.dvt_conv3x3_c64_wgrad_plan(N, H, W, Cout, _DT[dtype], n, c0, cv, mb, r)) == n
    return tuple(zip(c0, cv, mb, r)) if rows else tuple(zip(c0, cv, mb))


class StreamPlan(NamedTuple):
    ci: int          # conv3x3_stream_kernel<., ci, co, 9, 0>
    co: int
    groups: int      # launches (groups of co output channels)


def conv3x3_stream_plan(N: int, H: int, W: int, Cin: int, Cout: int, dtype: torch.dtype) -> Optional[StreamPlan]:
    """The instantiation dvt_conv3x3_stream launches and how many times; None where the call is refused.  Host only."""
    if dtype not in (torch.bfloat16, torch.float16):
        return None
    ci, co, groups = C.c_int(), C.c_int(), C.c_int()
    rc = L.load().dvt_conv3x3_stream_plan(N, H, W, Cin, Cout, _DT[dtype], C.byref(ci), C.byref(co), C.byref(groups))
    L.check(min(rc, 0), "dvt_conv3x3_stream_plan")
    return StreamPlan(ci.value, co.value, groups.value) if rc == 1 else None


def conv3x1_fwd_supported(x: Tensor, wp: Tensor, N: int, T: int, Lp: int, Cin: int, Cout: int) -> bool:
    if not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float16) or wp.dtype != x.dtype:
        return False
    if not (x.is_contiguous() and wp.is_contiguous() and x.shape == (N * T * Lp, Cin) and wp.dim() == 2 and wp.shape[0] == Cout
            and wp.shape[1] >= 3 * Cin and wp.shape[1] % 8 == 0):
        return False
    return bool(L.load().dvt_conv3x1_fwd_supported(N, T, Lp, Cin, Cout, dt(x)))


def conv3x1_fwd(x: Tensor, wp: Tensor, N: int, T: int, Lp: int, want_stats: bool = False, affine=None):
    """(3, 1) temporal convolution 144 -> 64 (or 64 -> 64: the stem's temporal half / its data gradient) over the [T, H*W] view
    of N clips from LDS-resident sliding windows (dvt_conv3x1_fwd): x [N*T*Lp, Cin], wp [64, >= 3 * Cin] (column kt * Cin + ci)
    -> [N*T*Lp, 64]; want_stats: also the partial column sums for ``bn_stats_from_partials``; affine (144 channels only) as
    ``conv3x1_wgrad``."""
    _need_cuda(x, wp)
    lib = L.load()
    Cin = x.shape[1]
    y = torch.empty((N * T * Lp, 64), dtype=x.dtype, device=x.device)
    aff, _keep = _bn_affine(affine)
    partial, parts = None, 0
    if want_stats:
        parts = int(lib.dvt_conv3x1_fwd_stats_parts(N, T, Lp, Cin))
        partial = workspace((parts + 64) * 2 * 64 * 4, x.device, slot="bn_partial")
    nb = (x.numel() + wp.numel() + y.numel()) * x.element_size()
    with _timed(("conv", "window3x1_fwd" if Cin == 144 else "window3x1_c64", N * T * Lp, 64, 3 * Cin, nb), 2.0 * N * T * Lp * 64 * 3 * Cin):
        L.check(lib.dvt_conv3x1_fwd(x.data_ptr(), None if aff is None else C.byref(aff), wp.data_ptr(), wp.shape[1], y.data_ptr(),
                                    _p(partial), N, T, Lp, Cin, dt(x), _stream()), "dvt_conv3x1_fwd")
    return (y, partial, parts) if want_stats else y


def conv2d_implicit(x: Tensor, wp: Tensor, N: int, Cc: int, H: int, W: int, Cout: int, k, stride, pad,
                    want_stats: bool = False, trim_w: int = 0, carry=None, residual: Optional[Tensor] = None,
                    out: Optional[Tensor] = None, out_hw=None, out_rows: Optional[Tensor] = None, residual_compact: bool = False):
    """NHWC matrix x [N*H*W, C], packed weights wp [Cout, kh*kw*C] -> [N*Ho*Wo, Cout]; gather fused into the GEMM.
    want_stats: also returns (partial, parts), the per-block column sums / sums of squares of the output that the GEMM
    epilogue leaves for the BatchNorm behind the convolution (bn_stats_from_partials).
    out / out_hw / out_rows / residual_compact: one parity class of a strided convolution's data gradient
    (dvt_conv_desc.out_h / out_w / out_rows): the launch computes out_hw pixels per image and writes row m of its product
    to row out_rows[m] of ``out`` (a full-size map the classes fill between them)."""
    _need_cuda(x, wp)
    Ho, Wo = conv_out_hw(H, W, k, stride, pad)
    Wo -= trim_w                                  # columns dropped at the right edge (dvt_conv_desc.trim_w)
    if out_hw is not None:
        Ho, Wo = out_hw
    if out_rows is not None:
        assert out is not None and out.is_contiguous() and out.dtype == x.dtype and out.shape[1] == Cout and not want_stats
        assert out_rows.dtype == torch.int32 and out_rows.is_contiguous() and out_rows.numel() == N * Ho * Wo
        y = out
    else:
        assert out is None and not residual_compact
        y = torch.empty((N * Ho * Wo, Cout), dtype=x.dtype, device=x.device)
    d = _conv_desc(x, wp, y, N, Cc, H, W, Cout, k, stride, pad, trim_w)
    if out_hw is not None:
        d.out_h, d.out_w = Ho, Wo
    if out_rows is not None:
        d.out_rows, d.residual_compact = out_rows.data_ptr(), int(residual_compact)
    if residual is not None:                          # a second gradient path joining this one: added on the accumulators
        assert residual.is_contiguous() and residual.dtype == x.dtype and not want_stats
        assert residual.shape == ((N * Ho * Wo, Cout) if (residual_compact or out_rows is None) else y.shape)
        d.residual = residual.data_ptr()
    lib = L.load()
    partial, parts = None, 0
    if want_stats:
        parts = int(lib.dvt_conv2d_implicit_stats_parts(C.byref(d)))
        partial = workspace(lib.dvt_conv2d_implicit_stats_bytes(C.byref(d)), x.device, slot="bn_partial")
        d.stats_partial = _p(partial)
    (kh, kw) = _pair(k)
    rows = N * Ho * Wo
    nb = (x.numel() + wp.numel() + rows * Cout * (2 if residual is not None else 1)) * x.element_size()    # implicit GEMM: the image is read once, not kh*kw times
    if carry is not None and carry.valid:             # the layer's weight-gradient reduce rides in this launch's grid tail
        d.carry = C.pointer(carry)
    wsb = int(lib.dvt_conv2d_implicit_workspace_bytes(C.byref(d)))
    if wsb:                                           # few output rows x deep K: split-K slabs (dvt_conv2d_implicit_workspace_bytes)
        d.workspace = workspace(wsb, x.device, slot="conv_split").data_ptr()
    with _timed(("conv", "implicit", rows, Cout, kh * kw * Cc, nb), 2.0 * rows * Cout * kh * kw * Cc):
        L.check(lib.dvt_conv2d_implicit(C.byref(d), _stream()), "dvt_conv2d_implicit")
    if carry is not None:
        carry.valid = 0
    return (y, partial, parts) if want_stats else y


_CLASS_ROWS = {}


def strided_class_rows(N: int, H: int, W: int, sh: int, sw: int, a: int, b: int, device) -> Tensor:
    """int32 [N * Hq * Wq]: the row of the full-size NHWC map [N*H*W, C] that pixel (n, hq, wq) of parity class (a, b) --
    input pixel (sh * hq + a, sw * wq + b) -- names.  Static per geometry: built once on the host, cached on the device."""
    key = (N, H, W, sh, sw, a, b, str(device))
    t = _CLASS_ROWS.get(key)
    if t is None:
        import numpy as np
        hq = np.arange(a, H, sh, dtype=np.int64)
        wq = np.arange(b, W, sw, dtype=np.int64)
        rows = (np.arange(N, dtype=np.int64)[:, None, None] * (H * W) + hq[None, :, None] * W + wq[None, None, :]).reshape(-1)
        assert rows.size == 0 or rows.max() < (1 << 31)
        t = torch.from_numpy(rows.astype(np.int32)).to(device)
        _CLASS_ROWS[key] = t
    return t


def strided_dgrad_classes(k, stride, pad, H: int, W: int):
    """The parity classes of the data gradient of a (k, stride, pad) convolution over an H x W input, or None when the
    decomposition does not apply (a class without a tap -- e.g. a strided 1 x 1 -- or with taps above / left of the map).
    -> [(a, b, (nth, ntw), (ph', pw'), (rh, rw), (Hq, Wq))]: class (a, b) = input pixels (hi % sh, wi % sw); its gradient is the
    stride-1 convolution of dz with the nth x ntw taps ki = rh + j * sh (decreasing), padded by (ph', pw') in front."""
    (kh, kw), (sh, sw), (ph, pw) = _pair(k), _pair(stride), _pair(pad)
    if sh == 1 and sw == 1:
        return None
    out = []
    for a in range(sh):
        for b in range(sw):
            dims = []
            for (kk, s, p, r0, ext) in ((kh, sh, ph, a, H), (kw, sw, pw, b, W)):
                r = (r0 + p) % s
                nt = (kk - r + s - 1) // s if r < kk else 0
                padq = (nt - 1) - (r0 + p) // s
                q = (ext - r0 + s - 1) // s if ext > r0 else 0
                dims.append((nt, padq, r, q))
            (nth, pph, rh, Hq), (ntw, ppw, rw, Wq) = dims
            if Hq == 0 or Wq == 0:
                continue
            if nth == 0 or ntw == 0 or pph < 0 or ppw < 0:
                return None
            out.append((a, b, (nth, ntw), (pph, ppw), (rh, rw), (Hq, Wq)))
    return out


def bn_stats_from_partials(partial: Tensor, parts: int, rows: int, Cc: int, running_mean: Optional[Tensor],
                           running_var: Optional[Tensor], eps: float, momentum: float, c_valid: int = 0):
    """mean / invstd (and the running statistics update) from the partial sums of conv2d_implicit(want_stats=True).
    c_valid: channels the running statistics really have (channel-padded layers; 0 = Cc)."""
    mean = torch.empty((Cc,), dtype=torch.float32, device=partial.device)
    invstd = torch.empty((Cc,), dtype=torch.float32, device=partial.device)
    L.check(L.load().dvt_bn_stats_from_partials(partial.data_ptr(), parts, mean.data_ptr(), invstd.data_ptr(),
                                               _p(running_mean), _p(running_var), rows, Cc, c_valid, eps, momentum,
                                               _stream()), "dvt_bn_stats_from_partials")
    return mean, invstd


def conv2d_implicit_wgrad_supported(x: Tensor, dz: Tensor, N, Cc, H, W, Cout, k, stride, pad, trim_w: int = 0) -> bool:
    if not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float16) or dz.dtype != x.dtype:
        return False
    if not (x.is_contiguous() and dz.is_contiguous()):
        return False
    return bool(L.load().dvt_conv2d_implicit_wgrad_supported(C.byref(_conv_desc(x, dz, None, N, Cc, H, W, Cout, k, stride, pad, trim_w))))


def conv2d_implicit_wgrad(x: Tensor, dz: Tensor, N: int, Cc: int, H: int, W: int, Cout: int, k, stride, pad,
                          trim_w: int = 0, defer_reduce: bool = False, master: Optional[Tensor] = None,
                          accumulate: bool = False, logical: Optional[Tuple[int, int]] = None):
    """-> dWt f32 [kh*kw*C, Cout] = gather(x)^T dz, the column matrix never materialised.
    defer_reduce: -> (dWt, pending): the split-K reduce is left to the data-gradient launch of the same layer
    (``conv2d_implicit(..., carry=pending)`` / ``linear_dgrad(..., carry=pending)``) or ``splitk_reduce_pending``.
    master: the parameter's own gradient f32 [Cout, C, kh, kw] (+= when accumulate): the reduce scatters into it directly
    and it is what is returned in dWt's place (no packed intermediate, no scatter launch)."""
    _need_cuda(x, dz, master)
    (kh, kw) = _pair(k)
    cout_l, cin_l = logical if logical is not None else (Cout, Cc)       # channel-padded layers: the parameter's own counts
    if master is not None:
        assert master.dtype == torch.float32 and master.is_contiguous() and master.numel() == cout_l * cin_l * kh * kw
        assert cout_l <= Cout and cin_l <= Cc
        out = master
    else:
        assert not accumulate
        out = torch.empty((kh * kw * Cc, Cout), dtype=torch.float32, device=x.device)
    d = _conv_desc(x, dz, out, N, Cc, H, W, Cout, k, stride, pad, trim_w)
    d.wgrad_master_layout, d.wgrad_accumulate = int(master is not None), int(accumulate)
    d.wgrad_cout_l, d.wgrad_cin_l = (cout_l, cin_l) if master is not None else (0, 0)
    lib = L.load()
    pending = L.SplitKPending() if defer_reduce else None
    nws = lib.dvt_conv2d_implicit_wgrad_workspace_bytes(C.byref(d))
    ws = _deferred_workspace(nws, x.device, pending) if defer_reduce else workspace(nws, x.device)
    d.workspace = _p(ws)
    if defer_reduce:
        pending._keep = (out, ws)
        d.defer_reduce = 1
        d.pending = C.pointer(pending)
    rows = dz.shape[0]
    nb = (x.numel() + dz.numel()) * x.element_size() + out.numel() * out.element_size()
    with _timed(("conv", "wgrad", kh * kw * Cc, Cout, rows, nb), 2.0 * rows * Cout * kh * kw * Cc):
        L.check(lib.dvt_conv2d_implicit_wgrad(C.byref(d), _stream()), "dvt_conv2d_implicit_wgrad")
    return (out, pending) if defer_reduce else out


class ConvPlan(NamedTuple):
    """What one dvt_conv2d_implicit / dvt_conv2d_implicit_wgrad call launches (dvt_conv2d_implicit_plan): the LDS-DMA
    configuration of its gemm_dma_kernel<..., true>, the slices of the reduction and its length per slice, the launch's
    epilogue and output form ("map" = the 16-bit map, "slab" = fp32 split-K partials), the kernel that sums the slabs as a
    launch of its own (CONV_REDUCES) and whether that reduce is left in a pending descriptor, and what becomes of a
    carried reduce (CONV_CARRIES; carry_reduce: its kernel when it is launched on its own)."""
    cfg: int
    split: int = 1
    k_per_split: int = 0
    epilogue: int = L.EPI_NONE
    out: str = "map"
    reduce: str = "none"
    deferred: bool = False
    carry: str = "none"
    carry_reduce: str = "none"


CONV_OUTS = {0: "map", 2: "slab"}                     # dvt_conv_plan_info.out_form
CONV_REDUCES = _enum_names("dvt_conv_reduce", "DVT_CONV_R_")
CONV_CARRIES = _enum_names("dvt_conv_carry", "DVT_CONV_CARRY_")


def conv2d_implicit_plan(N: int, Cc: int, H: int, W: int, Cout: int, k, stride, pad, dtype: torch.dtype, *,
                         wgrad: bool = False, trim_w: int = 0, residual: bool = False, want_stats: bool = False, carry=None,
                         out_hw=None, out_rows: bool = False, residual_compact: bool = False, defer_reduce: bool = False,
                         master: bool = False, accumulate: bool = False, logical: Optional[Tuple[int, int]] = None,
                         workspace: Optional[bool] = None) -> ConvPlan:
    """What ``conv2d_implicit`` (or, wgrad=True, ``conv2d_implicit_wgrad``) launches for the same geometry and options
    (dvt_conv2d_implicit_plan: the launcher's own decisions, no launch, no device, no tensors -- the options that name
    tensors there are flags here).  workspace: None = given where the launcher's size query asks for one; False = withheld."""
    (kh, kw), (sh, sw), (ph, pw) = _pair(k), _pair(stride), _pair(pad)
    d = L.ConvDesc()
    d.x = d.w = d.y = 1 << 4                          # (stand-ins: the size queries look at them, the plan does not)
    d.N, d.H, d.W, d.C, d.Cout = N, H, W, Cc, Cout
    d.kh, d.kw, d.sh, d.sw, d.ph, d.pw = kh, kw, sh, sw, ph, pw
    d.dtype, d.trim_w = _DT[dtype], trim_w
    keep = []
    if out_hw is not None:
        d.out_h, d.out_w = out_hw
    if out_rows:
        d.out_rows, d.residual_compact = 1 << 4, int(residual_compact)
    if residual:
        d.residual = 1 << 4
    if want_stats:
        d.stats_partial = 1 << 4
    if carry is not None:
        d.carry = C.pointer(carry)
    if wgrad:
        d.wgrad_master_layout, d.wgrad_accumulate = int(master), int(accumulate)
        d.wgrad_cout_l, d.wgrad_cin_l = logical if (master and logical is not None) else (0, 0)
        if defer_reduce:
            keep.append(L.SplitKPending())
            d.defer_reduce, d.pending = 1, C.pointer(keep[-1])
    lib = L.load()
    need = lib.dvt_conv2d_implicit_wgrad_workspace_bytes(C.byref(d)) if wgrad else lib.dvt_conv2d_implicit_workspace_bytes(C.byref(d))
    d.workspace = 256 if (need > 0 and workspace is not False) else None
    q = L.ConvPlanInfo()
    L.check(lib.dvt_conv2d_implicit_plan(C.byref(d), int(wgrad), C.byref(q)), "dvt_conv2d_implicit_plan")
    return ConvPlan(q.cfg, q.split, q.k_per_split, q.epilogue, CONV_OUTS[q.out_form], CONV_REDUCES[q.reduce], bool(q.deferred),
                    CONV_CARRIES[q.carry], CONV_REDUCES[q.carry_reduce])


def conv_weight_unpack_grad_t(gt: Tensor, shape, *, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    Cout, Cin, kh, kw = shape
    if out is None:
        assert not accumulate
        out = torch.empty(tuple(shape), dtype=torch.float32, device=gt.device)
    L.check(L.load().dvt_conv_weight_unpack_grad_t(gt.data_ptr(), out.data_ptr(), Cout, Cin, kh, kw, int(accumulate),
                                                   _stream()), "dvt_conv_weight_unpack_grad_t")
    return out


def pad3_f32(src: Tensor, A: int, B: int, K: int, Ap: int, Bp: int) -> Tensor:
    """f32 [A, B, K] -> zero-extended [Ap, Bp, K]."""
    _need_cuda(src)
    src = src.detach().contiguous()
    assert src.dtype == torch.float32 and src.numel() == A * B * K
    dst = torch.empty((Ap, Bp, K), dtype=torch.float32, device=src.device)
    L.check(L.load().dvt_pad3_f32(src.data_ptr(), dst.data_ptr(), A, B, K, Ap, Bp, _stream()), "dvt_pad3_f32")
    return dst


def unpad3_f32(src: Tensor, A: int, B: int, K: int, Bp: int, *, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """slice [:A, :B, :] of f32 [Ap, Bp, K] (+= into ``out`` when accumulate)."""
    _need_cuda(src)
    assert src.dtype == torch.float32 and src.is_contiguous()
    if out is None:
        assert not accumulate
        out = torch.empty((A, B, K), dtype=torch.float32, device=src.device)
    L.check(L.load().dvt_unpad3_f32(src.data_ptr(), out.data_ptr(), A, B, K, Bp, int(accumulate), _stream()), "dvt_unpad3_f32")
    return out


def conv_weight_pack_group(entries) -> None:
    """Both packed forms of many convolution weights in one launch.  entries: (src f32 [cout_l, cin_l, kh*kw] contiguous,
    dst tensor, cout_l, cin_l, kh, kw, cout_p, cin_p, ld, kind[, (sh, sw, rh, rw)]) with kind 0 = forward operand [cout_p, ld],
    1 = data-gradient operand [cin_p, kh*kw*cout_p], 2 = the data-gradient operand of one parity class of a strided
    convolution [cin_p, nth*ntw*cout_p] (dvt_pack_entry.cls_*)."""
    if not entries:
        return
    arr = (L.PackEntry * len(entries))()
    for i, ent in enumerate(entries):
        (src, dst, cout_l, cin_l, kh, kw, cout_p, cin_p, ld, kind), cls = ent[:10], (ent[10] if len(ent) > 10 else None)
        _need_cuda(src, dst)
        assert src.dtype == torch.float32 and src.is_contiguous() and src.numel() == cout_l * cin_l * kh * kw
        e = arr[i]
        ntaps = kh * kw
        if kind == 2:                                  # one parity class of a strided convolution's data gradient
            e.cls_sh, e.cls_sw, e.cls_rh, e.cls_rw = cls
            ntaps = ((kh - cls[2] + cls[0] - 1) // cls[0]) * ((kw - cls[3] + cls[1] - 1) // cls[1])
        assert dst.is_contiguous() and dst.numel() == (cout_p * ld if kind == 0 else cin_p * ntaps * cout_p)
        e.src, e.dst = src.data_ptr(), dst.data_ptr()
        e.cout_l, e.cin_l, e.kh, e.kw, e.cout_p, e.cin_p, e.ld, e.kind, e.dtype = cout_l, cin_l, kh, kw, cout_p, cin_p, ld, kind, dt(dst)
    L.check(L.load().dvt_conv_weight_pack_group(arr, len(entries), _stream()), "dvt_conv_weight_pack_group")


def conv_weight_pack(w: Tensor, ld: int, dtype: torch.dtype) -> Tensor:
    _need_cuda(w)
    w = w.detach().contiguous()
    assert w.dtype == torch.float32 and w.dim() == 4
    Cout, Cin, kh, kw = w.shape
    out = torch.empty((Cout, ld), dtype=dtype, device=w.device)
    L.check(L.load().dvt_conv_weight_pack(w.data_ptr(), out.data_ptr(), _DT[dtype], Cout, Cin, kh, kw, ld, _stream()),
            "dvt_conv_weight_pack")
    return out


def conv_weight_pack_dgrad(w: Tensor, dtype: torch.dtype) -> Tensor:
    """[Cout, Cin, kh, kw] f32 -> [Cin, kh*kw*Cout]: rotated taps, transposed channels (data-gradient operand)."""
    _need_cuda(w)
    w = w.detach().contiguous()
    Cout, Cin, kh, kw = w.shape
    out = torch.empty((Cin, kh * kw * Cout), dtype=dtype, device=w.device)
    L.check(L.load().dvt_conv_weight_pack_dgrad(w.data_ptr(), out.data_ptr(), _DT[dtype], Cout, Cin, kh, kw, _stream()),
            "dvt_conv_weight_pack_dgrad")
    return out


def conv_weight_unpack_grad(g: Tensor, shape, *, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    _need_cuda(g)
    Cout, Cin, kh, kw = shape
    if out is None:
        assert not accumulate
        out = torch.empty(tuple(shape), dtype=torch.float32, device=g.device)
    L.check(L.load().dvt_conv_weight_unpack_grad(g.data_ptr(), out.data_ptr(), Cout, Cin, kh, kw, g.shape[1],
                                                 int(accumulate), _stream()), "dvt_conv_weight_unpack_grad")
    return out


def bn_stats(z: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor], eps: float,
             momentum: float, c_valid: int = 0) -> Tuple[Tensor, Tensor]:
    _need_cuda(z)
    rows, Cc = z.shape
    mean = torch.empty((Cc,), dtype=torch.float32, device=z.device)
    invstd = torch.empty((Cc,), dtype=torch.float32, device=z.device)
    lib = L.load()
    ws = workspace(lib.dvt_bn_workspace_bytes(rows, Cc), z.device)
    with _timed(("hbm", "bn_stats", rows * Cc), z.numel() * z.element_size()):
        L.check(lib.dvt_bn_stats(z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _p(running_mean), _p(running_var),
                                 ws.data_ptr(), rows, Cc, c_valid, eps, momentum, dt(z), _stream()), "dvt_bn_stats")
    return mean, invstd


def bn_eval_invstd(running_var: Tensor, eps: float) -> Tensor:
    out = torch.empty_like(running_var)
    L.check(L.load().dvt_bn_eval_invstd(running_var.data_ptr(), out.data_ptr(), running_var.numel(), eps, _stream()),
            "dvt_bn_eval_invstd")
    return out


def bn_apply_fwd(z: Tensor, mean: Tensor, invstd: Tensor, gamma: Tensor, beta: Tensor, residual: Optional[Tensor],
                 relu: bool, want_mask: bool = False, c_valid: int = 0):
    """want_mask: -> (y, mask) with mask uint8 [rows, C/8], the ReLU mask bits for bn_bwd (layers with a residual branch)."""
    rows, Cc = z.shape
    y = torch.empty_like(z)
    mask = torch.empty((rows, Cc // 8), dtype=torch.uint8, device=z.device) if want_mask else None
    nb = z.numel() * z.element_size() * (2 + (residual is not None)) + (rows * (Cc // 8) if want_mask else 0)
    with _timed(("hbm", "bn_apply_fwd", rows * Cc), nb):
        L.check(L.load().dvt_bn_apply_fwd(z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                                          beta.data_ptr(), _p(residual), y.data_ptr(), _p(mask), rows, Cc, c_valid, int(relu),
                                          dt(z), _stream()), "dvt_bn_apply_fwd")
    return (y, mask) if want_mask else y


def bn_bwd(dy: Tensor, z: Tensor, y: Optional[Tensor], mean: Tensor, invstd: Tensor, gamma: Tensor, relu: bool,
           training: bool, want_dres: bool, *, dgamma: Optional[Tensor] = None, dbeta: Optional[Tensor] = None,
           accumulate: bool = False, beta: Optional[Tensor] = None, mask: Optional[Tensor] = None, c_valid: int = 0):
    """ReLU mask: ``mask`` (bn_apply_fwd(want_mask=True)) if given, else ``y``, else recomputed from z (``beta`` given, no
    residual branch)."""
    rows, Cc = z.shape
    dz = torch.empty_like(z)
    dres = torch.empty_like(z) if want_dres else None
    if dgamma is None:
        assert not accumulate
        dgamma = torch.empty((c_valid or Cc,), dtype=torch.float32, device=z.device)
        dbeta = torch.empty((c_valid or Cc,), dtype=torch.float32, device=z.device)
    if mask is not None:
        assert mask.dtype == torch.uint8 and mask.is_contiguous() and mask.numel() == rows * (Cc // 8)
        y = None
    lib = L.load()
    ws = workspace(lib.dvt_bn_workspace_bytes(rows, Cc), z.device)
    # train-mode BatchNorm backward is two passes by construction (the sums over the batch, then the input gradient):
    # each reads dy and z (and the mask bytes, or y when the mask cannot be recomputed), the second writes dz (and the
    # shortcut's gradient)
    esz = z.element_size()
    per_pass = z.numel() * esz * (2 + (y is not None)) + (mask.numel() if mask is not None else 0)
    nb = 2 * per_pass + z.numel() * esz * (1 + int(want_dres))
    with _timed(("hbm", "bn_bwd", rows * Cc), nb):
        L.check(lib.dvt_bn_bwd(dy.data_ptr(), z.data_ptr(), _p(y), _p(mask), mean.data_ptr(), invstd.data_ptr(),
                               gamma.data_ptr(), _p(beta), dz.data_ptr(), _p(dres), dgamma.data_ptr(), dbeta.data_ptr(),
                               ws.data_ptr(), rows, Cc, c_valid, int(relu), int(training), int(accumulate), dt(z), _stream()),
                "dvt_bn_bwd")
    return dz, dres, dgamma, dbeta


def bn_relu_maxpool_fwd(z: Tensor, mean: Tensor, invstd: Tensor, gamma: Tensor, beta: Tensor, N: int, Cc: int, H: int, W: int,
                        relu: bool):
    """BatchNorm (+ ReLU) + max-pool(3, 2, 1) of the NHWC map z in one pass -> (pooled [N*Ho*Wo, C], argmax taps)."""
    Ho, Wo = conv_out_hw(H, W, 3, 2, 1)
    y = torch.empty((N * Ho * Wo, Cc), dtype=z.dtype, device=z.device)
    idx = torch.empty((N * Ho * Wo * Cc,), dtype=torch.uint8, device=z.device)
    L.check(L.load().dvt_bn_relu_maxpool_fwd(z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                             y.data_ptr(), idx.data_ptr(), N, Cc, H, W, int(relu), dt(z), _stream()),
            "dvt_bn_relu_maxpool_fwd")
    return y, idx


def bn_bwd_pooled(dy_pool: Tensor, idx: Tensor, z: Tensor, mean: Tensor, invstd: Tensor, gamma: Tensor, beta: Tensor, N: int,
                  H: int, W: int, relu: bool, training: bool, *, dgamma: Optional[Tensor] = None,
                  dbeta: Optional[Tensor] = None, accumulate: bool = False):
    """bn_bwd with the incoming gradient gathered from the gradient of the max-pool(3, 2, 1) that follows the layer."""
    rows, Cc = z.shape
    assert rows == N * H * W
    dz = torch.empty_like(z)
    if dgamma is None:
        assert not accumulate
        dgamma = torch.empty((Cc,), dtype=torch.float32, device=z.device)
        dbeta = torch.empty((Cc,), dtype=torch.float32, device=z.device)
    lib = L.load()
    ws = workspace(lib.dvt_bn_workspace_bytes(rows, Cc), z.device)
    L.check(lib.dvt_bn_bwd_pooled(dy_pool.data_ptr(), idx.data_ptr(), z.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                  gamma.data_ptr(), beta.data_ptr(), dz.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                  ws.data_ptr(), N, Cc, H, W, int(relu), int(training), int(accumulate), dt(z), _stream()),
            "dvt_bn_bwd_pooled")
    return dz, dgamma, dbeta


def maxpool_fwd(x: Tensor, N: int, Cc: int, H: int, W: int, k: int, stride: int, pad: int):
    Ho, Wo = conv_out_hw(H, W, k, stride, pad)
    y = torch.empty((N * Ho * Wo, Cc), dtype=x.dtype, device=x.device)
    idx = torch.empty((N * Ho * Wo * Cc,), dtype=torch.uint8, device=x.device)
    L.check(L.load().dvt_maxpool_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(), N, Cc, H, W, k, stride, pad, dt(x),
                                     _stream()), "dvt_maxpool_fwd")
    return y, idx


def maxpool_bwd(dy: Tensor, idx: Tensor, N: int, Cc: int, H: int, W: int, k: int, stride: int, pad: int) -> Tensor:
    dx = torch.empty((N * H * W, Cc), dtype=dy.dtype, device=dy.device)
    L.check(L.load().dvt_maxpool_bwd(dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), N, Cc, H, W, k, stride, pad,
                                     dt(dy), _stream()), "dvt_maxpool_bwd")
    return dx


def transpose_last2(x: Tensor) -> Tensor:
    """[B, R, C] -> [B, C, R] contiguous."""
    _need_cuda(x)
    x = x.contiguous()
    B, R, Cc = x.shape
    out = torch.empty((B, Cc, R), dtype=x.dtype, device=x.device)
    L.check(L.load().dvt_transpose_last2(x.data_ptr(), out.data_ptr(), B, R, Cc, dt(x), _stream()),
            "dvt_transpose_last2")
    return out


# ------------------------------------------------------------------ LSTM recurrent chain
def lstm_seq_fwd(G: Tensor, w_hh: Tensor, b_ih: Optional[Tensor], b_hh: Optional[Tensor], B: int, T: int,
                 want_last: bool = False):
    """The recurrent chain of one nn.LSTM layer (dvt_lstm_seq_fwd).  G [B*T, 4H] = x W_ih^T (no bias), w_hh [4H, H] in
    G's dtype, biases f32.  -> (h_out [B, T, H], h_prev [B, T, H] (h shifted one step, zeros first), gates [B, T, 4H] f32,
    c [B, T, H] f32, h_last [B, H] or None)."""
    _need_cuda(G, w_hh, b_ih, b_hh)
    H = w_hh.shape[1]
    assert G.is_contiguous() and w_hh.is_contiguous() and w_hh.dtype == G.dtype and w_hh.shape == (4 * H, H)
    assert G.numel() == B * T * 4 * H
    for b in (b_ih, b_hh):
        assert b is None or (b.dtype == torch.float32 and b.is_contiguous() and b.numel() == 4 * H)
    dev = G.device
    h_out = torch.empty((B, T, H), dtype=G.dtype, device=dev)
    h_prev = torch.empty((B, T, H), dtype=G.dtype, device=dev)
    gates = torch.empty((B, T, 4 * H), dtype=torch.float32, device=dev)
    c = torch.empty((B, T, H), dtype=torch.float32, device=dev)
    h_last = torch.empty((B, H), dtype=G.dtype, device=dev) if want_last else None
    L.check(L.load().dvt_lstm_seq_fwd(G.data_ptr(), _p(b_ih), _p(b_hh), w_hh.data_ptr(), h_prev.data_ptr(),
                                      h_out.data_ptr(), gates.data_ptr(), c.data_ptr(), _p(h_last), B, T, H, dt(G),
                                      _stream()), "dvt_lstm_seq_fwd")
    return h_out, h_prev, gates, c, h_last


def lstm_seq_bwd(w_hh: Tensor, gates: Tensor, c: Tensor, dh_seq: Optional[Tensor], dh_last: Optional[Tensor]) -> Tensor:
    """Backward through time of ``lstm_seq_fwd`` (dvt_lstm_seq_bwd) -> dG [B*T, 4H] in w_hh's dtype, the gradient of the
    pre-activation gates."""
    _need_cuda(w_hh, gates, c, dh_seq, dh_last)
    B, T, H = c.shape
    for t in (dh_seq, dh_last):
        assert t is None or (t.dtype == w_hh.dtype and t.is_contiguous())
    assert dh_seq is None or dh_seq.numel() == B * T * H
    assert dh_last is None or dh_last.numel() == B * H
    lib = L.load()
    dG = torch.empty((B * T, 4 * H), dtype=w_hh.dtype, device=w_hh.device)
    ws = workspace(lib.dvt_lstm_seq_bwd_workspace_bytes(B, H, dt(w_hh)), w_hh.device)
    L.check(lib.dvt_lstm_seq_bwd(w_hh.data_ptr(), gates.data_ptr(), c.data_ptr(), _p(dh_seq), _p(dh_last),
                                 dG.data_ptr(), _p(ws), B, T, H, dt(w_hh), _stream()), "dvt_lstm_seq_bwd")
    return dG


# ------------------------------------------------------------------ 3-D convolution (inference; the r3d_18 video expert)
def conv3d_desc(x: Tensor, w: Optional[Tensor], geom, Cout: int, k, stride, pad, *, dtype: Optional[torch.dtype] = None,
                y: Optional[Tensor] = None) -> L.Conv3dDesc:
    """geom = (N, T, H, W); k / stride / pad = (t, h, w) triples.  x NDHWC [N*T*H*W, C] (C % 8 == 0)."""
    N, T, H, W = geom
    d = L.Conv3dDesc()
    d.x, d.w, d.y = _p(x), _p(w), _p(y)
    d.N, d.T, d.H, d.W, d.C, d.Cout = N, T, H, W, x.shape[1], Cout
    d.kt, d.kh, d.kw = k
    d.st, d.sh, d.sw = stride
    d.pt, d.ph, d.pw = pad
    d.dtype = _DT[dtype if dtype is not None else x.dtype]
    return d


def conv3d_out(geom, k, stride, pad):
    """(To, Ho, Wo) of a 3-D convolution."""
    return tuple((n + 2 * p - kk) // s + 1 for n, kk, s, p in zip(geom[1:], k, stride, pad))


def conv3d_implicit_k(x: Tensor, geom, Cout: int, k, stride, pad) -> int:
    """Row length of the packed weights dvt_conv3d_implicit expects for this geometry."""
    d = conv3d_desc(x, None, geom, Cout, k, stride, pad)
    K = L.load().dvt_conv3d_implicit_k(C.byref(d))
    if K < 0:
        L.check(-2, "dvt_conv3d_implicit_k")          # DVT_ERR_UNSUPPORTED, with the library's message
    return int(K)


def conv3d_weight_pack(w: Tensor, Cp: int, ld: int, dtype: torch.dtype) -> Tensor:
    """nn.Conv3d weight f32 [Cout, Cin, kt, kh, kw] -> packed [Cout, ld] in dtype (column ((dt*kh+dh)*kw+dw)*Cp + c)."""
    _need_cuda(w)
    w = w.detach().float().contiguous()
    Cout, Cin, kt, kh, kw = w.shape
    out = torch.empty((Cout, ld), dtype=dtype, device=w.device)
    L.check(L.load().dvt_conv3d_weight_pack(w.data_ptr(), out.data_ptr(), _DT[dtype], Cout, Cin, kt, kh, kw, Cp, ld,
                                            _stream()), "dvt_conv3d_weight_pack")
    return out


def bn_fold(gamma: Optional[Tensor], beta: Optional[Tensor], running_mean: Tensor, running_var: Tensor, eps: float):
    """Eval-mode BatchNorm -> (scale, shift) f32 [C]: y = x * scale + shift."""
    f = lambda t: None if t is None else t.detach().float().contiguous()      # noqa: E731
    gamma, beta, mean, var = f(gamma), f(beta), f(running_mean), f(running_var)
    _need_cuda(gamma, beta, mean, var)
    Cc = mean.numel()
    scale = torch.empty(Cc, dtype=torch.float32, device=mean.device)
    shift = torch.empty_like(scale)
    L.check(L.load().dvt_bn_fold(_p(gamma), _p(beta), mean.data_ptr(), var.data_ptr(), float(eps), scale.data_ptr(),
                                 shift.data_ptr(), Cc, _stream()), "dvt_bn_fold")
    return scale, shift


def conv3d_implicit(x: Tensor, w: Tensor, geom, Cout: int, k, stride, pad, *, scale: Optional[Tensor] = None,
                    shift: Optional[Tensor] = None, residual: Optional[Tensor] = None, relu: bool = False) -> Tensor:
    """y [N*To*Ho*Wo, Cout] = relu?(conv3d(x, w) * scale + shift + residual) in x's dtype (dvt_conv3d_implicit).
    x NDHWC [N*T*H*W, C], w packed [Cout, conv3d_implicit_k(..)] (conv3d_weight_pack)."""
    _need_cuda(x, w, scale, shift, residual)
    x = x.contiguous()
    if w.dtype != x.dtype:
        raise TypeError(f"conv3d_implicit: weights {w.dtype} != map {x.dtype}")
    To, Ho, Wo = conv3d_out(geom, k, stride, pad)
    M = geom[0] * To * Ho * Wo
    if residual is not None:
        residual = residual.contiguous()
        if residual.dtype != x.dtype or residual.numel() != M * Cout:
            raise ValueError("conv3d_implicit: residual must be [N*To*Ho*Wo, Cout] in the map's dtype")
    y = torch.empty((M, Cout), dtype=x.dtype, device=x.device)
    d = conv3d_desc(x, w, geom, Cout, k, stride, pad, y=y)
    lib = L.load()
    K = lib.dvt_conv3d_implicit_k(C.byref(d))
    if K > 0 and tuple(w.shape) != (Cout, K):
        raise ValueError(f"conv3d_implicit: packed weights {tuple(w.shape)} != ({Cout}, {K})")
    d.scale, d.shift, d.residual, d.relu = _p(scale), _p(shift), _p(residual), int(relu)
    ws = workspace(lib.dvt_conv3d_implicit_workspace_bytes(C.byref(d)), x.device, slot="conv3d")
    d.workspace = _p(ws)
    with _timed("conv3d_implicit", 2 * M * Cout * x.shape[1] * k[0] * k[1] * k[2]):
        L.check(lib.dvt_conv3d_implicit(C.byref(d), _stream()), "dvt_conv3d_implicit")
    return y


def conv2p1d_l1_supported(x: Tensor, geom, Cout: int, k, stride, pad) -> bool:
    """Is this convolution one of the layer-1 halves dvt_conv2p1d_l1 takes?"""
    d = conv3d_desc(x, None, geom, Cout, k, stride, pad)
    return bool(L.load().dvt_conv2p1d_l1_supported(C.byref(d)))


def conv2p1d_l1(x: Tensor, w: Tensor, geom, Cout: int, k, stride, pad, *, scale: Optional[Tensor] = None,
                shift: Optional[Tensor] = None, residual: Optional[Tensor] = None, relu: bool = False) -> Tensor:
    """conv3d_implicit's contract for the layer-1 halves of R(2+1)D-18 (csrc/conv2p1d_l1.hip): x NDHWC [N*T*H*W, C], w packed
    [Cout, conv3d_implicit_k(..)] (conv3d_weight_pack) -> y [N*T*H*W, Cout] = relu?(conv3d(x, w) * scale + shift + residual)."""
    _need_cuda(x, w, scale, shift, residual)
    x = x.contiguous()
    if w.dtype != x.dtype:
        raise TypeError(f"conv2p1d_l1: weights {w.dtype} != map {x.dtype}")
    M = geom[0] * geom[1] * geom[2] * geom[3]
    if residual is not None:
        residual = residual.contiguous()
        if residual.dtype != x.dtype or residual.numel() != M * Cout:
            raise ValueError("conv2p1d_l1: residual must be [N*T*H*W, Cout] in the map's dtype")
    for t in (scale, shift):
        if t is not None and (t.dtype != torch.float32 or t.numel() != Cout):
            raise ValueError("conv2p1d_l1: scale / shift must be f32 [Cout]")
    y = torch.empty((M, Cout), dtype=x.dtype, device=x.device)
    d = conv3d_desc(x, w, geom, Cout, k, stride, pad, y=y)
    lib = L.load()
    K = lib.dvt_conv3d_implicit_k(C.byref(d))
    if tuple(w.shape) != (Cout, K) or x.shape[0] != M:
        raise ValueError(f"conv2p1d_l1: packed weights {tuple(w.shape)} != ({Cout}, {K}) or map rows {x.shape[0]} != {M}")
    d.scale, d.shift, d.residual, d.relu = _p(scale), _p(shift), _p(residual), int(relu)
    with _timed("conv2p1d_l1", 2 * M * Cout * x.shape[1] * k[0] * k[1] * k[2]):
        L.check(lib.dvt_conv2p1d_l1(C.byref(d), _stream()), "dvt_conv2p1d_l1")
    return y


# ------------------------------------------------------------------ MLP baselines on expert embeddings (csrc/embed_mlp.hip)
def _ld(t: Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1
    return t.stride(0)


def bn1d_relu_fwd(z: Tensor, gamma: Tensor, beta: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor],
                  num_batches_tracked: Optional[Tensor], *, segments: int, training: bool, eps: float, momentum: float):
    """y = BatchNorm1d(relu(z)) on z [S*B, C] (S = segments, each with its own batch statistics) -> (y, mean, invstd):
    mean / invstd f32 [S, C] in training, [C] (from the running statistics) in eval."""
    _need_cuda(z, gamma, beta, running_mean, running_var, num_batches_tracked)
    R, Cc = z.shape
    if R % segments:
        raise ValueError(f"bn1d_relu: {R} rows do not split into {segments} segments")
    B = R // segments
    for t in (gamma, beta, running_mean, running_var):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == Cc)
    assert num_batches_tracked is None or num_batches_tracked.dtype == torch.int64
    y = torch.empty((R, Cc), dtype=z.dtype, device=z.device)
    shape = (segments, Cc) if training else (Cc,)
    mean = torch.empty(shape, dtype=torch.float32, device=z.device)
    invstd = torch.empty(shape, dtype=torch.float32, device=z.device)
    L.check(L.load().dvt_bn1d_relu_fwd(z.data_ptr(), _ld(z), y.data_ptr(), Cc, gamma.data_ptr(), beta.data_ptr(),
                                       _p(running_mean), _p(running_var), _p(num_batches_tracked), mean.data_ptr(),
                                       invstd.data_ptr(), B, Cc, segments, eps, momentum, int(training), dt(z), _stream()),
            "dvt_bn1d_relu_fwd")
    return y, mean, invstd


def bn1d_relu_bwd(dy: Tensor, z: Tensor, gamma: Tensor, mean: Tensor, invstd: Tensor, *, segments: int, training: bool,
                  dgamma: Optional[Tensor] = None, dbeta: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """dz = [z > 0] * dBN/dx (one launch); dgamma / dbeta f32 [C] written (or added to, ``accumulate``) when given."""
    _need_cuda(dy, z, gamma, mean, invstd, dgamma, dbeta)
    R, Cc = z.shape
    assert dy.shape == z.shape and dy.dtype == z.dtype
    for t in (dgamma, dbeta):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == Cc)
    dz = torch.empty((R, Cc), dtype=z.dtype, device=z.device)
    L.check(L.load().dvt_bn1d_relu_bwd(dy.data_ptr(), _ld(dy), z.data_ptr(), _ld(z), gamma.data_ptr(), mean.data_ptr(),
                                       invstd.data_ptr(), dz.data_ptr(), Cc, _p(dgamma), _p(dbeta), int(accumulate),
                                       R // segments, Cc, segments, int(training), dt(z), _stream()), "dvt_bn1d_relu_bwd")
    return dz


CE_IGNORE_INDEX = -100


def ce_labels_fwd(logits: Tensor, labels: Tensor, ignore_index: int = CE_IGNORE_INDEX):
    """nn.CrossEntropyLoss() (mean, ignore_index) -> (loss f32 [1], lse f32 [M + 1]: per-row log-sum-exp, then the count)."""
    _need_cuda(logits, labels)
    M, Cc = logits.shape
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == M
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    lse = torch.empty(M + 1, dtype=torch.float32, device=logits.device)
    L.check(L.load().dvt_ce_labels_fwd(logits.data_ptr(), _ld(logits), labels.data_ptr(), loss.data_ptr(), lse.data_ptr(),
                                       M, Cc, ignore_index, dt(logits), _stream()), "dvt_ce_labels_fwd")
    return loss, lse


def ce_labels_bwd(logits: Tensor, labels: Tensor, lse: Tensor, gloss: Tensor,
                  ignore_index: int = CE_IGNORE_INDEX) -> Tensor:
    _need_cuda(logits, labels, lse, gloss)
    M, Cc = logits.shape
    assert gloss.dtype == torch.float32 and lse.numel() == M + 1
    d = torch.empty((M, Cc), dtype=logits.dtype, device=logits.device)
    L.check(L.load().dvt_ce_labels_bwd(logits.data_ptr(), _ld(logits), labels.data_ptr(), lse.data_ptr(), gloss.data_ptr(),
                                       d.data_ptr(), Cc, M, Cc, ignore_index, dt(logits), _stream()), "dvt_ce_labels_bwd")
    return d


def gather_rows_ptr(rows, D: int, dtype: torch.dtype, device) -> Tensor:
    """rows: a list (one per output row) of lists of GPU tensors, each holding one row of ``numel()`` elements ->
    [len(rows), D] in ``dtype``, row r = cat(rows[r]) (zero past the parts' total width), in ONE launch.  The pointer
    table is built on the host and copied to the device once."""
    R, P = len(rows), len(rows[0])
    out = torch.empty((R, D), dtype=dtype, device=device)
    tab = torch.empty((R, P, 3), dtype=torch.int64)
    keep = []
    for r, parts in enumerate(rows):
        if len(parts) != P:
            raise ValueError("gather_rows_ptr: every row needs the same number of parts")
        if sum(t.numel() for t in parts) != D:
            raise ValueError(f"gather_rows_ptr: row {r} has {sum(t.numel() for t in parts)} elements, expected {D}")
        for j, t in enumerate(parts):
            _need_cuda(t)
            if t.device != out.device or not t.is_contiguous():
                raise ValueError("gather_rows_ptr: parts must be contiguous tensors on the output's device")
            tab[r, j, 0], tab[r, j, 1], tab[r, j, 2] = t.data_ptr(), t.numel(), dt(t)
            keep.append(t)
    table = tab.to(out.device)
    L.check(L.load().dvt_gather_rows_ptr(table.data_ptr(), R, P, out.data_ptr(), D, D, _DT[dtype], _stream()),
            "dvt_gather_rows_ptr")
    return out


# ------------------------------------------------------------------ the online probe (csrc/probe.hip)
ProbeDesc = L.STRUCTS["dvt_probe_desc"]
PROBE_LIMITS = "2 <= B <= 1024 in training (1 <= B in eval), D <= 4096, H a multiple of 16 up to 2048, C <= 32, fp32 / bf16 / fp16"


def probe_supported(B: int, D: int, H: int, Cn: int, dtype: torch.dtype, training: bool = True) -> bool:
    """The range of the probe-step kernels (dvt_probe_supported; B = 1 is refused in training as torch's BatchNorm1d does)."""
    if dtype not in _DT or (training and B < 2):
        return False
    return bool(L.load().dvt_probe_supported(B, D, H, Cn, _DT[dtype]))


def probe_desc(x: Tensor, w1: Tensor, gamma: Tensor, beta: Tensor, running_mean: Tensor, running_var: Tensor,
               num_batches_tracked: Optional[Tensor], w2: Tensor, b2: Tensor, *, training: bool, p: float = 0.0,
               eps: float = 1e-5, momentum: float = 0.1, rng_state: Optional[Tensor] = None, rng_offset: int = 0):
    """-> (descriptor, the tensors it points to) for one pass of the probe on x [B, D]: the forward's outputs h / z /
    save_mean / save_invstd and the partial-logit workspace are allocated here; target, prob, loss, dlogits, logits, the
    gradient buffers, lr and accumulate are filled in by ``probe_loss`` / ``probe_bwd_step``."""
    _need_cuda(x, w1, gamma, beta, running_mean, running_var, num_batches_tracked, w2, b2, rng_state)
    B, D = x.shape
    H, Cn = w1.shape[0], w2.shape[0]
    if not probe_supported(B, D, H, Cn, x.dtype, training):
        raise NotImplementedError(f"probe step: B={B} D={D} H={H} C={Cn} {x.dtype} is outside the kernels' range "
                                  f"({PROBE_LIMITS})")
    assert x.is_contiguous() and tuple(w1.shape) == (H, D) and tuple(w2.shape) == (Cn, H) and b2.numel() == Cn
    for t in (w1, gamma, beta, running_mean, running_var, w2, b2):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert gamma.numel() == beta.numel() == running_mean.numel() == running_var.numel() == H
    assert num_batches_tracked is None or num_batches_tracked.dtype == torch.int64
    dev = x.device
    lib = L.load()
    keep = dict(x=x, h=torch.empty((B, H), dtype=x.dtype, device=dev),
                ws=torch.empty((lib.dvt_probe_workspace_bytes(B, H, Cn),), dtype=torch.uint8, device=dev))
    d = ProbeDesc()
    d.x, d.w1, d.gamma, d.beta, d.w2, d.b2 = (t.data_ptr() for t in (x, w1, gamma, beta, w2, b2))
    d.running_mean, d.running_var, d.num_batches_tracked = running_mean.data_ptr(), running_var.data_ptr(), _p(num_batches_tracked)
    d.h, d.workspace = keep["h"].data_ptr(), keep["ws"].data_ptr()
    if training:
        keep.update(z=torch.empty((B, H), dtype=torch.float32, device=dev),
                    stats=torch.empty((2, H), dtype=torch.float32, device=dev))
        d.z, d.save_mean, d.save_invstd = keep["z"].data_ptr(), keep["stats"][0].data_ptr(), keep["stats"][1].data_ptr()
        if p > 0.0:
            assert rng_state is not None and rng_state.dtype == torch.int64
            keep["rng"] = rng_state
            d.rng_state, d.rng_offset = rng_state.data_ptr(), int(rng_offset)
    d.B, d.D, d.H, d.C, d.dtype, d.training = B, D, H, Cn, dt(x), int(training)
    d.p, d.eps, d.momentum = (float(p) if training else 0.0), float(eps), float(momentum)
    return d, keep


def probe_fwd(d, keep) -> Tensor:
    """Launch 1: Dropout -> Linear -> BatchNorm1d -> ReLU -> Dropout and the slabs' partial logits -> h [B, H]."""
    L.check(L.load().dvt_probe_fwd(C.byref(d), _stream()), "dvt_probe_fwd")
    return keep["h"]


def probe_logits(d, keep) -> Tensor:
    """Launch 2 without a target: the logits [B, C] f32 of the forward just run."""
    out = torch.empty((d.B, d.C), dtype=torch.float32, device=keep["x"].device)
    e = ProbeDesc.from_buffer_copy(d)
    e.logits, e.training, e.target = out.data_ptr(), 0, None
    L.check(L.load().dvt_probe_loss(C.byref(e), _stream()), "dvt_probe_loss")
    return out


def probe_loss(d, keep, target: Tensor, g_b2: Optional[Tensor] = None, *, lr: float = 0.0, accumulate: bool = False):
    """Launch 2: sigmoid + nn.BCELoss() -> (loss 0-dim f32, prob [B, C] f32); in a training descriptor also dlogits and the
    SGD update of the bias through its gradient buffer g_b2."""
    _need_cuda(target, g_b2)
    assert target.dtype == torch.float32 and target.is_contiguous() and tuple(target.shape) == (d.B, d.C)
    dev = target.device
    keep.update(target=target, prob=torch.empty((d.B, d.C), dtype=torch.float32, device=dev),
                loss=torch.empty((1,), dtype=torch.float32, device=dev))
    d.target, d.prob, d.loss = target.data_ptr(), keep["prob"].data_ptr(), keep["loss"].data_ptr()
    if d.training:
        assert g_b2 is not None and g_b2.dtype == torch.float32 and g_b2.numel() == d.C
        keep["dlogits"] = torch.empty((d.B, d.C), dtype=torch.float32, device=dev)
        d.dlogits, d.g_b2, d.lr, d.accumulate = keep["dlogits"].data_ptr(), g_b2.data_ptr(), float(lr), int(accumulate)
    L.check(L.load().dvt_probe_loss(C.byref(d), _stream()), "dvt_probe_loss")
    return keep["loss"].view(()), keep["prob"]


def probe_bwd_step(d, keep, g_w1: Tensor, g_gamma: Tensor, g_beta: Tensor, g_w2: Tensor) -> None:
    """Launch 3: the gradients of W1, gamma, beta, W2 into their buffers (added when the descriptor accumulates) and SGD."""
    _need_cuda(g_w1, g_gamma, g_beta, g_w2)
    for g, n in ((g_w1, d.H * d.D), (g_gamma, d.H), (g_beta, d.H), (g_w2, d.C * d.H)):
        assert g.dtype == torch.float32 and g.is_contiguous() and g.numel() == n
    d.g_w1, d.g_gamma, d.g_beta, d.g_w2 = (g.data_ptr() for g in (g_w1, g_gamma, g_beta, g_w2))
    L.check(L.load().dvt_probe_bwd_step(C.byref(d), _stream()), "dvt_probe_bwd_step")


def multilabel_sweep_counts(probs: Tensor, labels: Tensor, thresholds) -> Tuple[Tensor, Tensor]:
    """TP / FP / FN per class of ``probs > t`` for every t of ``thresholds`` in one launch (dvt_multilabel_sweep_counts)
    -> (counts int64 [T, 3, C], support int64 [C])."""
    probs, lab = _scores_and_mask("multilabel_sweep_counts", probs, labels)
    N, Cn = probs.shape
    th = torch.tensor([float(t) for t in thresholds], dtype=torch.float32).to(probs.device)
    counts = torch.empty((th.numel(), 3, Cn), dtype=torch.int64, device=probs.device)
    support = torch.empty((Cn,), dtype=torch.int64, device=probs.device)
    L.check(L.load().dvt_multilabel_sweep_counts(probs.data_ptr(), lab.data_ptr(), N, Cn, th.data_ptr(), th.numel(),
                                                 counts.data_ptr(), support.data_ptr(), _stream()),
            "dvt_multilabel_sweep_counts")
    return counts, support


# ------------------------------------------------------------------ rank metrics and counts (csrc/eval_metrics.hip)
class RankMetrics(NamedTuple):
    """What ``rank_metrics`` returns: device tensors, no host synchronisation.  ``micro`` / ``micro_two_u`` /
    ``micro_positives`` are NaN / -1 / -1 without ``micro=True``; ``samples_sum`` / ``valid_rows`` NaN / -1 without
    ``samples=True``."""
    auroc: Tensor              # f64 [C], NaN for a class without both kinds
    ap: Tensor                 # f64 [C], 0 for a class without positives
    positives: Tensor          # int64 [C]
    two_u: Tensor              # int64 [C]: twice the Mann-Whitney U of the class (ties count half)
    macro: Tensor              # f64 []: mean AUROC over the valid classes
    weighted: Tensor           # f64 []: support-weighted AUROC over the valid classes
    micro: Tensor              # f64 []: AUROC of all N C elements as one column
    samples_sum: Tensor        # f64 []: sum over the valid rows of the per-row AUROC
    valid_classes: Tensor      # int64 []
    valid_rows: Tensor         # int64 []
    micro_two_u: Tensor        # int64 []
    micro_positives: Tensor    # int64 []


RANK_BLOCK = None


def rank_metrics_block() -> int:
    """Elements of a sorted column that one workgroup of the rank pass reduces (dvt_rank_metrics_block)."""
    global RANK_BLOCK
    if RANK_BLOCK is None:
        RANK_BLOCK = int(L.load().dvt_rank_metrics_block())
    return RANK_BLOCK


def rank_metrics(probs: Tensor, labels: Tensor, micro: bool = False, samples: bool = False) -> RankMetrics:
    """AUROC and average precision per class from one descending sort and a parallel tie-aware rank pass
    (dvt_rank_metrics), with the macro / weighted averages and, on request, the micro AUROC and the per-row ("samples",
    C <= 64) sum."""
    probs, lab = _scores_and_mask("rank_metrics", probs, labels)
    N, Cn = probs.shape
    lib = L.load()
    flags = (L.ENUMS["dvt_rank_flags"]["DVT_RANK_MICRO"] if micro else 0) | (
        L.ENUMS["dvt_rank_flags"]["DVT_RANK_SAMPLES"] if samples else 0)
    nbytes = lib.dvt_rank_metrics_workspace_bytes(N, Cn, flags)
    if nbytes == 0:
        raise ValueError("rank_metrics: empty input or N*C >= 2^31")
    ws = workspace(nbytes, probs.device)
    na, nc = L.MACROS["DVT_RANK_N_AVERAGES"], L.MACROS["DVT_RANK_N_COUNTS"]
    f = torch.empty((2 * Cn + na,), dtype=torch.float64, device=probs.device)
    i = torch.empty((2 * Cn + nc,), dtype=torch.int64, device=probs.device)
    L.check(lib.dvt_rank_metrics(probs.data_ptr(), lab.data_ptr(), N, Cn, flags, f.data_ptr(), f[Cn:].data_ptr(),
                                 i.data_ptr(), i[Cn:].data_ptr(), f[2 * Cn:].data_ptr(), i[2 * Cn:].data_ptr(),
                                 ws.data_ptr(), _stream()), "dvt_rank_metrics")
    A, K = L.ENUMS["dvt_rank_average"], L.ENUMS["dvt_rank_count"]
    avg, cnt = f[2 * Cn:], i[2 * Cn:]
    return RankMetrics(f[:Cn], f[Cn:2 * Cn], i[:Cn], i[Cn:2 * Cn], avg[A["DVT_RANK_AVG_MACRO"]],
                       avg[A["DVT_RANK_AVG_WEIGHTED"]], avg[A["DVT_RANK_AVG_MICRO"]], avg[A["DVT_RANK_AVG_SAMPLES_SUM"]],
                       cnt[K["DVT_RANK_CNT_VALID_CLASSES"]], cnt[K["DVT_RANK_CNT_VALID_ROWS"]],
                       cnt[K["DVT_RANK_CNT_MICRO_TWO_U"]], cnt[K["DVT_RANK_CNT_MICRO_POSITIVES"]])


def confusion_matrix(preds: Tensor, target: Tensor, num_classes: int, cm: Optional[Tensor] = None,
                     ignored: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """cm int64 [C, C] (rows = target, columns = prediction) and the count of skipped rows, int64 [1]
    (dvt_confusion_matrix).  ``preds``: logits [N, C] (f32 / bf16 / fp16; the row's argmax, lowest index among equal
    maxima) or integer classes [N].  With ``cm`` and ``ignored`` given the counts are ADDED to them in place."""
    _need_cuda(preds, target)
    Cn = int(num_classes)
    target = target.contiguous().to(torch.int64)
    N = target.shape[0]
    if target.dim() != 1:
        raise ValueError(f"confusion_matrix: target {tuple(target.shape)} must be [N]")
    logits = None
    if preds.dim() == 2:
        if tuple(preds.shape) != (N, Cn) or preds.dtype not in _DT:
            raise ValueError(f"confusion_matrix: logits {tuple(preds.shape)} {preds.dtype} for N = {N}, C = {Cn}")
        logits = preds.contiguous()
    elif preds.dim() == 1 and preds.shape[0] == N and not preds.is_floating_point():
        preds = preds.contiguous().to(torch.int64)
    else:
        raise ValueError(f"confusion_matrix: preds {tuple(preds.shape)} {preds.dtype} must be [N, C] logits or [N] integers")
    if (cm is None) != (ignored is None):
        raise ValueError("confusion_matrix: give both cm and ignored, or neither")
    accumulate = cm is not None
    if accumulate:
        if (cm.dtype, ignored.dtype) != (torch.int64, torch.int64) or tuple(cm.shape) != (Cn, Cn) or ignored.numel() != 1 \
                or not (cm.is_contiguous() and cm.is_cuda and ignored.is_cuda):
            raise ValueError("confusion_matrix: cm must be a contiguous int64 [C, C] and ignored an int64 [1] on the device")
    else:
        cm = torch.empty((Cn, Cn), dtype=torch.int64, device=target.device)
        ignored = torch.empty((1,), dtype=torch.int64, device=target.device)
    if N == 0:                                                    # nothing to count (an empty tensor has no address)
        return (cm, ignored) if accumulate else (zeros((Cn, Cn), torch.int64, target.device),
                                                 zeros((1,), torch.int64, target.device))
    L.check(L.load().dvt_confusion_matrix(_p(logits), dt(logits) if logits is not None else L.F32,
                                          None if logits is not None else preds.data_ptr(), target.data_ptr(), N, Cn,
                                          int(accumulate), cm.data_ptr(), ignored.data_ptr(), _stream()),
            "dvt_confusion_matrix")
    return cm, ignored


def multilabel_counts(probs: Tensor, labels: Tensor, threshold: float, state: Optional[Tensor] = None) -> Tensor:
    """state int64 [4, C] = TP / FP / FN / TN per class of ``probs > threshold`` (strict, compared in f32) against the
    multilabel targets (dvt_multilabel_counts).  With ``state`` given the counts are ADDED to it in place."""
    probs, lab = _scores_and_mask("multilabel_counts", probs, labels)
    N, Cn = probs.shape
    accumulate = state is not None
    if accumulate:
        if state.dtype != torch.int64 or tuple(state.shape) != (4, Cn) or not (state.is_contiguous() and state.is_cuda):
            raise ValueError("multilabel_counts: state must be a contiguous int64 [4, C] on the device")
    else:
        state = torch.empty((4, Cn), dtype=torch.int64, device=probs.device)
    if N == 0:
        return state if accumulate else zeros((4, Cn), torch.int64, probs.device)
    L.check(L.load().dvt_multilabel_counts(probs.data_ptr(), lab.data_ptr(), N, Cn, float(threshold), int(accumulate),
                                           state.data_ptr(), _stream()), "dvt_multilabel_counts")
    return state


def count_equal(a: Tensor, b: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """int64 [1]: the number of positions where ``a == b`` (dvt_count_equal); integer tensors are compared as int64,
    anything else as f32.  With ``out`` given the count is ADDED to it in place."""
    _need_cuda(a, b)
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"count_equal: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    ints = not (a.is_floating_point() or b.is_floating_point())
    if ints:
        a, b = a.contiguous().to(torch.int64), b.contiguous().to(torch.int64)
    else:
        a, b = (t.contiguous() if t.dtype == torch.float32 else
                (cast(t.contiguous(), torch.float32) if t.dtype in _DT else t.contiguous().to(torch.float32)) for t in (a, b))
    accumulate = out is not None
    if accumulate:
        if out.dtype != torch.int64 or out.numel() != 1 or not out.is_cuda:
            raise ValueError("count_equal: out must be an int64 [1] on the device")
    else:
        out = torch.empty((1,), dtype=torch.int64, device=a.device)
    n = a.numel()
    L.check(L.load().dvt_count_equal(a.data_ptr() if n else None, b.data_ptr() if n else None, n, int(ints), int(accumulate),
                                     out.data_ptr(), _stream()), "dvt_count_equal")
    return out


# ------------------------------------------------------------------ VGGish audio expert (csrc/audio.hip)
LOGMEL_VARIANTS = {name[len("DVT_LOGMEL_"):].lower(): v for name, v in L.ENUMS["dvt_logmel_variant"].items()}
# The spectrum dvt_logmel_examples computes by default; DESIGN 4.16 has the grounds and both forms' measured times and errors.
# "dft" stays selectable for that comparison (tools/bench_audio.py); its accuracy is pinned to a looser, stated bound.
LOGMEL_VARIANT = "fft"
LOGMEL_FRAMES, LOGMEL_BANDS = 96, 64          # an example's shape, as csrc/audio.hip states it (kExFrames, kMel): the output's trailing dims
_logmel_tables = {}


def logmel_num_examples(L_: int) -> int:
    """Examples a waveform row of L_ samples yields (dvt_logmel_num_examples; host only)."""
    return int(L.load().dvt_logmel_num_examples(int(L_)))


def logmel_tables_host() -> Tensor:
    """The front end's tables as dvt_logmel_tables builds them (float64 on the host, rounded once) -> f32 CPU tensor."""
    lib = L.load()
    t = torch.empty(lib.dvt_logmel_examples_workspace_bytes() // 4, dtype=torch.float32)
    L.check(lib.dvt_logmel_tables(t.data_ptr(), t.numel() * 4), "dvt_logmel_tables")
    return t


def logmel_examples(wave: Tensor, out_dtype: torch.dtype = torch.float32, variant: Optional[str] = None) -> Tensor:
    """wave f32 [R, L] (mono, 16 kHz, in [-1, 1]) -> log-mel examples [R * E, 96, 64] in out_dtype (dvt_logmel_examples);
    E = logmel_num_examples(L), an empty result when the row is shorter than one example.  The tables are uploaded once per
    device."""
    _need_cuda(wave)
    if wave.dim() != 2 or wave.dtype != torch.float32:
        raise TypeError("logmel_examples: expected an f32 waveform [R, L]")
    wave = wave.contiguous()
    R, L_ = wave.shape
    E = logmel_num_examples(L_)
    out = torch.empty((R * E, LOGMEL_FRAMES, LOGMEL_BANDS), dtype=out_dtype, device=wave.device)
    if out.numel() == 0:
        return out
    tab = _logmel_tables.get(wave.device)
    if tab is None:
        tab = _logmel_tables[wave.device] = logmel_tables_host().to(wave.device)
    v = LOGMEL_VARIANTS[LOGMEL_VARIANT if variant is None else variant]
    with _timed("logmel_examples", wave.numel() * 4 + out.numel() * out.element_size()):
        L.check(L.load().dvt_logmel_examples(wave.data_ptr(), R, L_, tab.data_ptr(), out.data_ptr(), _DT[out_dtype], v,
                                             _stream()), "dvt_logmel_examples")
    return out


def vggish_conv1_pool(x: Tensor, w: Tensor, bias: Tensor) -> Tensor:
    """Conv2d(1, 64, 3, padding=1) + bias + ReLU + MaxPool2d(2, 2) in one launch (dvt_vggish_conv1_pool).  x [N, H, 64] in the
    compute dtype, w f32 [64, 1, 3, 3], bias f32 [64] -> NHWC [N * H/2 * 32, 64] in x's dtype."""
    _need_cuda(x, w, bias)
    if x.dim() != 3 or w.dtype != torch.float32 or bias.dtype != torch.float32 or w.numel() != 576 or bias.numel() != 64:
        raise TypeError("vggish_conv1_pool: expected x [N, H, 64], w f32 [64, 1, 3, 3], bias f32 [64]")
    x, w, bias = x.contiguous(), w.contiguous(), bias.contiguous()
    N, H, W = x.shape
    y = torch.empty((N * (H // 2) * (W // 2), 64), dtype=x.dtype, device=x.device)
    with _timed("vggish_conv1_pool", x.numel() * x.element_size() + y.numel() * y.element_size()):
        L.check(L.load().dvt_vggish_conv1_pool(x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), N, H, W, dt(x),
                                               _stream()), "dvt_vggish_conv1_pool")
    return y


# ------------------------------------------------------------------ class-activation maps (csrc/cam.hip)
CAM_METHODS = {"gradcam": L.ENUMS["dvt_cam_method"]["DVT_CAM_GRADCAM"],
               "gradcam++": L.ENUMS["dvt_cam_method"]["DVT_CAM_GRADCAMPP"],
               "xgradcam": L.ENUMS["dvt_cam_method"]["DVT_CAM_XGRADCAM"]}
_cam_jet = {}


def cam_seed(logits: Tensor, category: Optional[Tensor] = None) -> Tensor:
    """logits [B, K] -> the backward seed [B, K] in the logits' dtype (dvt_cam_seed): one-hot at category[b] (device int32 [B])
    or at the row's argmax where category is None or the entry negative (ties to the lowest index).  No host synchronisation."""
    _need_cuda(logits, category)
    if logits.dim() != 2 or logits.shape[1] == 0:
        raise TypeError("cam_seed: expected logits [B, K]")
    if category is not None and (category.dtype != torch.int32 or category.dim() != 1 or category.shape[0] != logits.shape[0]):
        raise TypeError("cam_seed: category must be an int32 tensor [B]")
    logits = logits.contiguous()
    category = None if category is None else category.contiguous()
    B, K = logits.shape
    seed = torch.empty_like(logits)
    L.check(L.load().dvt_cam_seed(logits.data_ptr(), _p(category), seed.data_ptr(), B, K, dt(logits), _stream()), "dvt_cam_seed")
    return seed


def cam_map_launches(P: int, C: int) -> int:
    """Launches dvt_cam_map takes at P positions of C channels: 1 (a workgroup owns a clip's block) or 3.  Host only."""
    return int(L.load().dvt_cam_map_launches(int(P), int(C)))


def cam_map(A: Tensor, G: Tensor, method: str = "gradcam", want_weights: bool = False, want_raw: bool = False):
    """Activation A and gradient G [N, P, C] (channels last, one dtype, C a multiple of 8) -> (scaled [N, P], raw [N, P] or
    None, weights [N, C] or None), all f32 (dvt_cam_map).  method: one of CAM_METHODS."""
    if method not in CAM_METHODS:
        raise ValueError(f"cam_map: unknown method {method!r} (one of {sorted(CAM_METHODS)})")
    _need_cuda(A, G)
    if A.dim() != 3 or A.shape != G.shape or A.dtype != G.dtype:
        raise TypeError("cam_map: expected A and G [N, P, C] of one shape and dtype")
    if A.shape[2] % 8 != 0:
        raise ValueError("cam_map: the channel count must be a multiple of 8")
    A, G = A.contiguous(), G.contiguous()
    N, P, C = A.shape
    scaled = torch.empty((N, P), dtype=torch.float32, device=A.device)
    raw = torch.empty((N, P), dtype=torch.float32, device=A.device) if want_raw else None
    weights = torch.empty((N, C), dtype=torch.float32, device=A.device) if want_weights else None
    if N == 0 or P == 0:
        return scaled, raw, weights
    lib = L.load()
    nbytes = int(lib.dvt_cam_map_workspace_bytes(N, P, C))
    ws = workspace(nbytes, A.device)
    with _timed("cam_map", 2 * A.numel() * A.element_size()):
        L.check(lib.dvt_cam_map(A.data_ptr(), G.data_ptr(), N, P, C, dt(A), CAM_METHODS[method], _p(weights), _p(raw),
                                scaled.data_ptr(), _p(ws), nbytes, _stream()), "dvt_cam_map")
    return scaled, raw, weights


def cam_jet_table_host() -> Tensor:
    """The JET colour table as dvt_cam_jet_table builds it (float64 on the host) -> uint8 CPU tensor [256, 3], RGB."""
    t = torch.empty((256, 3), dtype=torch.uint8)
    L.check(L.load().dvt_cam_jet_table(t.data_ptr(), t.numel()), "dvt_cam_jet_table")
    return t


def cam_render(scaled: Tensor, size, frames: Optional[Tensor] = None, use_rgb: bool = False, image_weight: float = 0.5,
               want_mask: bool = True):
    """scaled f32 [N, T', H', W'] -> (mask f32 [N, T, H, W] or None, overlay uint8 [N, T, H, W, 3] or None) with size =
    (T, H, W) (dvt_cam_render): trilinear upsample with half-pixel centres and, with frames ([N, T, H, W, 3], uint8, or f32
    in [0, 1]), the JET overlay of show_cam_on_image in the same launch.  The table is uploaded once per device."""
    _need_cuda(scaled, frames)
    if scaled.dim() != 4 or scaled.dtype != torch.float32:
        raise TypeError("cam_render: expected f32 maps [N, T', H', W']")
    T, H, W = (int(v) for v in size)
    N, Ti, Hi, Wi = scaled.shape
    if min(T, H, W) <= 0:
        raise ValueError("cam_render: size must be positive (T, H, W)")
    if frames is None and not want_mask:
        raise ValueError("cam_render: nothing to compute (no frames and no mask)")
    scaled = scaled.contiguous()
    mask = torch.empty((N, T, H, W), dtype=torch.float32, device=scaled.device) if want_mask else None
    overlay = jet = None
    if frames is not None:
        if frames.dtype not in (torch.uint8, torch.float32) or tuple(frames.shape) != (N, T, H, W, 3):
            raise TypeError(f"cam_render: frames must be uint8 or f32 [N, T, H, W, 3] = {(N, T, H, W, 3)}")
        frames = frames.contiguous()
        overlay = torch.empty((N, T, H, W, 3), dtype=torch.uint8, device=scaled.device)
        jet = _cam_jet.get(scaled.device)
        if jet is None:
            jet = _cam_jet[scaled.device] = cam_jet_table_host().to(scaled.device)
    if N == 0 or min(Ti, Hi, Wi) == 0:
        return mask, overlay
    with _timed("cam_render", scaled.numel() * 4 + N * T * H * W * (4 + (6 if frames is not None else 0))):
        L.check(L.load().dvt_cam_render(scaled.data_ptr(), N, Ti, Hi, Wi, T, H, W, _p(mask), _p(frames),
                                        int(frames is not None and frames.dtype == torch.float32), _p(jet), _p(overlay),
                                        float(image_weight), int(bool(use_rgb)), _stream()), "dvt_cam_render")
    return mask, overlay


# ------------------------------------------------------------------ attention rollout (csrc/attn_rollout.hip)
ROLLOUT_FORMS = _enum_names("dvt_rollout_form", "DVT_ROLLOUT_F_")
ROLLOUT_UNIFORM = L.MACROS["DVT_ROLLOUT_UNIFORM"]


class RolloutPlan(NamedTuple):
    """What one dvt_rollout_step call launches (dvt_rollout_plan): the form (ROLLOUT_FORMS), waves per workgroup, the MFMA
    form's 32-key steps and query parts (0 otherwise) and the dynamic LDS bytes."""
    form: str
    waves: int = 0
    key_steps: int = 0
    query_parts: int = 0
    lds: int = 0


def _rollout_desc(q: Tensor, k: Tensor, lse: Optional[Tensor], r_in: Optional[Tensor], r_out: Optional[Tensor],
                  query: int, residual: float, scale: Optional[float]):
    """q [S, H, Lq, dh] and k [S, H, N, dh]: strided views with unit stride in the last dim, one dtype; Lq is N or 1."""
    if q.dim() != 4 or k.dim() != 4 or q.stride(3) != 1 or k.stride(3) != 1 or q.dtype != k.dtype:
        raise TypeError("rollout_step: q and k must be [S, H, L, dh] views of one dtype, dh contiguous")
    S, H, Lq, dh = q.shape
    N = k.shape[2]
    if tuple(k.shape) != (S, H, N, dh) or Lq not in (N, 1):
        raise TypeError(f"rollout_step: q {tuple(q.shape)} and k {tuple(k.shape)} do not pair (Lq is N or 1)")
    if lse is not None and (lse.dtype != torch.float32 or lse.numel() != S * H * Lq or not lse.is_contiguous()):
        raise TypeError("rollout_step: lse must be a contiguous f32 tensor [S, H, Lq]")
    if r_in is not None and (r_in.dtype != torch.float32 or tuple(r_in.shape) != (S, N) or not r_in.is_contiguous()):
        raise TypeError("rollout_step: r_in must be a contiguous f32 tensor [S, N]")
    if r_in is None and not (query == ROLLOUT_UNIFORM or 0 <= query < N):
        raise ValueError(f"rollout_step: without r_in, query = {query} must be a token index below {N} or ROLLOUT_UNIFORM")
    if r_in is not None and Lq == 1:
        raise ValueError("rollout_step: a layer with one query row takes the one-hot start (r_in None, query >= 0)")
    if not 0.0 <= residual <= 1.0:
        raise ValueError(f"rollout_step: residual = {residual} is outside [0, 1]")
    d = L.RolloutDesc()
    d.q, d.k, d.lse, d.r_in, d.r_out = q.data_ptr(), k.data_ptr(), _p(lse), _p(r_in), _p(r_out)
    d.S, d.H, d.N, d.Lq, d.dh = S, H, N, Lq, dh
    d.q_sb, d.q_sh, d.q_sl = q.stride(0), q.stride(1), q.stride(2)
    d.k_sb, d.k_sh, d.k_sl = k.stride(0), k.stride(1), k.stride(2)
    d.query, d.rho, d.scale, d.dtype = int(query), float(residual), float(dh ** -0.5 if scale is None else scale), dt(q)
    return d


def rollout_plan(q: Tensor, k: Tensor, r_in: Optional[Tensor] = None, *, query: int = 0, residual: float = 0.5,
                 scale: Optional[float] = None) -> RolloutPlan:
    """What ``rollout_step`` launches for the same views (dvt_rollout_plan: the launcher's own decisions, no launch, no
    device needed -- shapes, strides, addresses and types count; CPU tensors are fine).  Raises where the launcher refuses."""
    d = _rollout_desc(q, k, None, r_in, None, query, residual, scale)
    d.lse = d.r_out = 256                       # looked at for NULL-ness only
    r = L.RolloutPlanInfo()
    L.check(L.load().dvt_rollout_plan(C.byref(d), C.byref(r)), "dvt_rollout_plan")
    return RolloutPlan(ROLLOUT_FORMS[r.form], r.waves, r.key_steps, r.query_parts, r.lds)


def rollout_step(q: Tensor, k: Tensor, lse: Tensor, r_in: Optional[Tensor] = None, *, query: int = 0,
                 residual: float = 0.5, scale: Optional[float] = None) -> Tensor:
    """One layer of the rollout recurrence (dvt_rollout_step): r_out[s, j] = residual r_in[s, j] + (1 - residual) / H
    sum_h sum_i r_in[s, i] softmax(scale q k^T)[s, h, i, j], with q [S, H, Lq, dh] / k [S, H, N, dh] the strided views and
    lse [S, H, Lq] the log-sum-exp ``attention_fwd`` took and returned.  r_in f32 [S, N], or None for a start vector that is
    never stored: the one-hot of token ``query``, or 1 / N with query = ROLLOUT_UNIFORM.  Lq == 1: a layer that ran for token
    ``query`` alone (r_in None).  scale defaults to dh^-1/2, the model's.  -> r_out f32 [S, N]."""
    _need_cuda(q, k, lse, r_in)
    if lse is None:
        raise TypeError("rollout_step: lse is required")
    r_out = torch.empty((q.shape[0], k.shape[2]), dtype=torch.float32, device=q.device)
    d = _rollout_desc(q, k, lse, r_in, r_out, query, residual, scale)
    with _timed("rollout_step", (q.numel() + k.numel()) * q.element_size()):
        L.check(L.load().dvt_rollout_step(C.byref(d), _stream()), "dvt_rollout_step")
    return r_out


def rollout_from_probs(P: Tensor, heads: int, *, query: int = 0, residual: float = 0.5) -> Tensor:
    """The start of the recurrence from the folded single-query layer (dvt_rollout_from_probs): P f32 [S, N, 8] as
    ``attn_cls_fwd`` returns it (normalised probabilities of the query, head h of key j at P[s, j, h]) ->
    r f32 [S, N] = residual e_query + (1 - residual) mean over the first ``heads`` heads."""
    _need_cuda(P)
    if P.dim() != 3 or P.shape[2] != 8 or P.dtype != torch.float32:
        raise TypeError("rollout_from_probs: expected P f32 [S, N, 8]")
    S, N, _ = P.shape
    if not 1 <= heads <= 8:
        raise ValueError(f"rollout_from_probs: heads = {heads} is outside 1 .. 8")
    if not 0 <= query < max(N, 1):
        raise ValueError(f"rollout_from_probs: query = {query} is no token index below {N}")
    if not 0.0 <= residual <= 1.0:
        raise ValueError(f"rollout_from_probs: residual = {residual} is outside [0, 1]")
    P = P.contiguous()
    r = torch.empty((S, N), dtype=torch.float32, device=P.device)
    if S == 0 or N == 0:
        return r
    L.check(L.load().dvt_rollout_from_probs(P.data_ptr(), S, N, int(heads), int(query), float(residual), r.data_ptr(),
                                            _stream()), "dvt_rollout_from_probs")
    return r


def rollout_video(r_space: Tensor, r_time: Tensor, want_raw: bool = True):
    """r_space f32 [B*T, n + 1] (sequence b*T + f) and r_time f32 [B, T + 1], CLS entries first -> (raw, scaled) f32
    [B, T, n]: raw[b, f, p] = r_time[b, 1 + f] r_space[b*T + f, 1 + p] (None unless want_raw) and the same scaled per clip as
    ``cam_map`` scales its maps (dvt_rollout_video, one launch)."""
    _need_cuda(r_space, r_time)
    if r_space.dim() != 2 or r_time.dim() != 2 or r_space.dtype != torch.float32 or r_time.dtype != torch.float32:
        raise TypeError("rollout_video: expected f32 r_space [B*T, n + 1] and r_time [B, T + 1]")
    B, T, n = r_time.shape[0], r_time.shape[1] - 1, r_space.shape[1] - 1
    if T <= 0 or n <= 0 or r_space.shape[0] != B * T:
        raise ValueError(f"rollout_video: r_space {tuple(r_space.shape)} is not B*T rows for r_time {tuple(r_time.shape)}")
    r_space, r_time = r_space.contiguous(), r_time.contiguous()
    scaled = torch.empty((B, T, n), dtype=torch.float32, device=r_space.device)
    raw = torch.empty((B, T, n), dtype=torch.float32, device=r_space.device) if want_raw else None
    if B == 0:
        return raw, scaled
    L.check(L.load().dvt_rollout_video(r_space.data_ptr(), r_time.data_ptr(), B, T, n, _p(raw), scaled.data_ptr(), _stream()),
            "dvt_rollout_video")
    return raw, scaled
