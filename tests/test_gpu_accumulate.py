"""Global gradient norm, in-place clipping and gradient accumulation on the real kernels.

Exact part: gradients of small integers make every sum of squares an exact fp32 integer, so ``dvt_grad_norm`` must
reproduce numpy's integer sums bit for bit whatever order it adds in -- at every length at which the chunking takes
another path (below one quad, around one chunk of 8192, more than 256 chunks so that one thread of the total joins two
partials), on 16-byte-aligned gradients and on views offset by one element (the scalar path)."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 8192
LENGTHS = (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 257 * CHUNK + 5)


@pytest.fixture(scope="module")
def int_grads():
    rng = np.random.default_rng(20)
    return [rng.integers(-2, 3, size=n).astype(np.float32) for n in LENGTHS]


@pytest.fixture(scope="module")
def normal_grads():
    rng = np.random.default_rng(21)
    return [rng.standard_normal(n).astype(np.float32) for n in LENGTHS]


def _on_device(arrays, offset):
    """Device copies; ``offset`` 1: each a view one element into its allocation, i.e. 4 bytes off 16-byte alignment."""
    out = []
    for a in arrays:
        base = torch.zeros(a.size + offset, dtype=torch.float32, device="cuda")
        t = base[offset:]
        t.copy_(torch.from_numpy(a))
        assert t.data_ptr() % 16 == 4 * offset and t.is_contiguous()
        out.append(t)
    return out


@pytest.mark.parametrize("offset", [0, 1])
def test_norms_of_integer_gradients_are_exact(device, int_grads, offset):
    from dvt_amd import ops
    assert ops.lars_plan(LENGTHS).chunk == CHUNK
    dev = _on_device(int_grads, offset)
    sets = [list(range(len(LENGTHS)))] + [[i] for i in range(len(LENGTHS))]
    for idx in sets:
        table = ops.grad_table([dev[i] for i in idx])
        want_sq = sum(int((int_grads[i].astype(np.int64) ** 2).sum()) for i in idx)
        want_max = max(float(np.abs(int_grads[i]).max()) for i in idx)
        assert want_sq < 1 << 24
        for _ in range(2):                                   # the workspace is reused as it was left
            raw = float(ops.grad_norm(table, 2.0, raw=True))
            nrm = float(ops.grad_norm(table, 2.0))
            mx = float(ops.grad_norm(table, float("inf")))
            print(f"[exact] offset {offset} segments {idx}: sumsq {raw} (want {want_sq}), max {mx} (want {want_max})")
            assert raw == float(want_sq), (idx, raw, want_sq)
            assert abs(nrm - np.sqrt(want_sq)) <= 1e-6 * np.sqrt(want_sq)
            assert mx == want_max


@pytest.mark.parametrize("offset", [0, 1])
def test_a_single_nonzero_is_found_at_every_boundary(device, offset):
    """One 3.0 among zeros: at the last element of each segment and on each side of every chunk boundary it has."""
    from dvt_amd import ops
    dev = _on_device([np.zeros(n, dtype=np.float32) for n in LENGTHS], offset)
    table = ops.grad_table(dev)
    assert float(ops.grad_norm(table, 2.0)) == 0.0 and float(ops.grad_norm(table, float("inf"))) == 0.0
    for t in dev:
        n = t.numel()
        spots = {n - 1}
        for b in range(CHUNK, n, CHUNK):
            if b < 3 * CHUNK or b > n - 2 * CHUNK:           # the first and the last boundaries of the long segment
                spots |= {b - 1, b}
        for i in sorted(spots):
            t[i] = -3.0
            raw, mx = float(ops.grad_norm(table, 2.0, raw=True)), float(ops.grad_norm(table, float("inf")))
            t[i] = 0.0
            assert raw == 9.0 and mx == 3.0, (n, i, raw, mx)


class _Bag(torch.nn.Module):
    def __init__(self, lengths):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.ones(n)) for n in lengths])


def _flat_with(grads, **scaling):
    from dvt_amd.dp import FlatParameters
    flat = FlatParameters(_Bag([g.numel() for g in grads]).cuda(), compute_dtype=None)
    if scaling:
        flat.enable_loss_scaling(**scaling)
    flat.zero_grad()
    for s, g in zip(flat.sinks, grads):
        s.buf.copy_(g)
        s.mark_written()
    flat.finish_backward()
    return flat


def _norm64(arrays, norm_type):
    if norm_type == 2.0:
        return float(np.sqrt(sum((a.astype(np.float64) ** 2).sum() for a in arrays)))
    return float(max(np.abs(a).max() for a in arrays))


def _check_clipped(got, arrays, norm64, max_norm):
    coef = min(1.0, max_norm / (norm64 + 1e-6))
    for g, a in zip(got, arrays):
        want = a.astype(np.float64) * coef
        err = np.abs(g.double().cpu().numpy() - want)
        assert (err <= 1e-5 * np.abs(want)).all(), float((err / np.maximum(np.abs(want), 1e-300)).max())


@pytest.mark.parametrize("norm_type", [2.0, float("inf")])
def test_flat_clip_against_torchs_definition(device, normal_grads, norm_type):
    dev = _on_device(normal_grads, 0)
    flat = _flat_with(dev)
    norm64 = _norm64(normal_grads, norm_type)
    before = flat.grad.clone()
    got = flat.clip_grad_norm_(1e30, norm_type)               # the coefficient clamps to 1: nothing may change
    print(f"[clip flat] norm_type {norm_type}: norm {float(got)} float64 {norm64}")
    assert abs(float(got) - norm64) <= 1e-5 * norm64
    assert torch.equal(flat.grad, before)
    got = flat.clip_grad_norm_(1.0, norm_type)
    assert abs(float(got) - norm64) <= 1e-5 * norm64          # the norm BEFORE clipping
    _check_clipped([p.grad for p in flat.params], normal_grads, norm64, 1.0)
    after = float(flat.clip_grad_norm_(1.0, norm_type))
    assert abs(after - 1.0) <= 2e-5


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("norm_type", [2.0, float("inf")])
def test_optim_clip_against_torchs_definition(device, normal_grads, norm_type, offset):
    from dvt_amd import optim
    params = [torch.nn.Parameter(torch.ones(n, device="cuda")) for n in LENGTHS]
    for p, g in zip(params, _on_device(normal_grads, offset)):
        p.grad = g
    idle = torch.nn.Parameter(torch.ones(7, device="cuda"))   # no gradient: left out, like grad None
    norm64 = _norm64(normal_grads, norm_type)
    before = [p.grad.clone() for p in params]
    got = optim.clip_grad_norm_(params + [idle], 1e30, norm_type)
    assert abs(float(got) - norm64) <= 1e-5 * norm64
    assert all(torch.equal(p.grad, b) for p, b in zip(params, before))
    got = optim.clip_grad_norm_(params + [idle], 0.5, norm_type)
    print(f"[clip optim] norm_type {norm_type} offset {offset}: norm {float(got)} float64 {norm64}")
    assert abs(float(got) - norm64) <= 1e-5 * norm64 and idle.grad is None
    _check_clipped([p.grad for p in params], normal_grads, norm64, 0.5)
    assert len(optim._clip_tables) >= 1
    n_tables = len(optim._clip_tables)
    optim.clip_grad_norm_(params + [idle], 0.5, norm_type)    # the same gradient tensors: the cached table
    assert len(optim._clip_tables) == n_tables


def test_clip_under_loss_scaling(device, normal_grads):
    """scale 1024 and gradient 1024 g: a power of two commutes with every rounding, so the result is 1024 * (clip of g
    without scaling), bit for bit.  One inf: gradient untouched, norm non-finite, and the scaled step skips and halves."""
    plain = _flat_with(_on_device(normal_grads, 0))
    scaled = _flat_with(_on_device([a * np.float32(1024) for a in normal_grads], 0), init_scale=1024.0)
    n0, n1 = plain.clip_grad_norm_(1.0), scaled.clip_grad_norm_(1.0)
    assert float(n0) == float(n1) and float(n0) > 1.0         # the returned norm is the unscaled one
    assert torch.equal(scaled.grad, plain.grad * 1024.0)
    assert not torch.equal(plain.grad, _flat_with(_on_device(normal_grads, 0)).grad)      # it did clip

    scaled = _flat_with(_on_device([a * np.float32(1024) for a in normal_grads], 0), init_scale=1024.0)
    scaled.params[6].grad[CHUNK] = float("inf")
    before, weights = scaled.grad.clone(), scaled.data.clone()
    for norm_type in (2.0, float("inf")):
        got = scaled.clip_grad_norm_(1.0, norm_type)
        assert not np.isfinite(float(got))
        assert torch.equal(scaled.grad, before)               # bitwise untouched (inf == inf)
    scaled.adamw_step(lr=1e-2)
    assert torch.equal(scaled.data, weights) and float(scaled.scale_dev) == 512.0 and int(scaled.step_dev[0]) == 0
    scaled.params[6].grad[CHUNK] = float("nan")               # a NaN must not be dropped by the maximum
    assert np.isnan(float(scaled.clip_grad_norm_(1.0, float("inf"))))


# ------------------------------------------------------------------ accumulation on the real backward kernels
def _model():
    from dvt_amd.models.vit import ViViT
    torch.manual_seed(1130)
    return ViViT(32, 8, 19, 3, dim=64, depth=2, heads=2, dim_head=32, compute_dtype=torch.float32)   # dropout 0, no BatchNorm


def _data(n):
    g = torch.Generator().manual_seed(5)
    return torch.randn(n, 3, 3, 32, 32, generator=g).cuda(), (torch.rand(n, 19, generator=g) < 0.3).float().cuda()


def _window(net, flat, xs, ys, seed):
    """One accumulation window over the micro-batches (xs[j], ys[j])."""
    k = len(xs)
    flat.zero_grad()
    for j in range(k):
        with (flat.no_sync() if j < k - 1 else contextlib.nullcontext()):
            net.loss(xs[j], ys[j])[0].backward(seed)
            flat.finish_backward()


def test_two_micro_batches_equal_one_batch_of_four(device):
    from dvt_amd.dp import Communicator, FlatParameters
    x, y = _data(4)
    ref_net = _model().cuda()
    ref = FlatParameters(ref_net, compute_dtype=None)
    _window(ref_net, ref, [x], [y], torch.full((), ref.loss_scale, device="cuda"))
    ref_grad = ref.grad.clone()
    ref.adamw_step(lr=1e-3, weight_decay=0.09)
    comm = Communicator(1, 0, Communicator.unique_id())
    try:
        net = _model().cuda()
        flat = FlatParameters(net, bucket_mb=0.1, compute_dtype=None, comm=comm)
        assert len(flat.bucket_ranges) >= 2 and flat.accumulation_scale(2) == 0.5
        calls = []
        plain = flat._all_reduce
        flat._all_reduce = lambda t, via=None: (calls.append(flat._no_sync), plain(t, via))[1]
        for _ in range(2):                                    # the second window overwrites the first one's sums
            calls.clear()
            _window(net, flat, [x[:2], x[2:]], [y[:2], y[2:]], torch.full((), flat.accumulation_scale(2), device="cuda"))
            # one collective per bucket (and per late side buffer), every one of them outside no_sync
            assert not any(calls) and len(calls) == len(flat.bucket_ranges) + sum(s.late_written for s in flat.sinks)
        torch.cuda.synchronize()
        scale = ref_grad.abs().max()
        err = float((flat.grad - ref_grad).abs().max() / scale)
        print(f"[accumulate] gradient error {err:.3g} of the largest entry")
        assert err < 2e-5
        assert flat.skip_mask is None and ref.skip_mask is None
        flat.adamw_step(lr=1e-3, weight_decay=0.09)
        assert float((flat.data - ref.data).abs().max()) < 1e-5
    finally:
        comm.destroy()


K = 3


def _accumulated(mode, scaling, comm):
    """Two warm-up windows on the static inputs as they stand, then two windows whose micro-batches are copied in."""
    from dvt_amd.dp import FlatParameters
    from dvt_amd.graph import capture_accumulated_step
    x, y = _data(2 * K)
    net = _model().cuda()
    flat = FlatParameters(net, bucket_mb=0.1, compute_dtype=None, comm=comm)
    if scaling:
        seed = flat.enable_loss_scaling(init_scale=1024.0, growth_interval=2, accumulate=K)
    else:
        seed = torch.full((), flat.accumulation_scale(K), device="cuda")
    sx, sy = x[:2].clone(), y[:2].clone()
    norms = []

    def micro():
        loss = net.loss(sx, sy)[0]
        loss.backward(seed)
        flat.finish_backward()
        return loss

    def update():
        norms.append(flat.clip_grad_norm_(1e-3))
        flat.adamw_step(lr=1e-3, weight_decay=0.09)

    def load(j):
        sx.copy_(x[2 * j:2 * j + 2])
        sy.copy_(y[2 * j:2 * j + 2])

    losses = []
    if mode == "eager":
        for w in range(2 + 2):
            flat.zero_grad()
            for j in range(K):
                if w >= 2:
                    load(j)
                with (flat.no_sync() if j < K - 1 else contextlib.nullcontext()):
                    loss = micro()
            update()
            if w >= 2:
                losses.append(float(loss.detach()))
    else:
        replay, out = capture_accumulated_step(micro, update, flat, K, warmup=2)
        for w in range(2):
            for j in range(K):
                load(j)
                replay(j)
            losses.append(float(out.detach()))
    torch.cuda.synchronize()
    state = [flat.data.clone(), flat.exp_avg.clone(), flat.exp_avg_sq.clone(), flat.step_dev.clone(), flat.grad.clone(),
             norms[-1].clone()]
    if scaling:
        state += [flat.scale_dev.clone(), flat.loss_grad.clone().reshape(1)]
    return losses, state


@pytest.mark.parametrize("scaling", [False, True])
def test_three_graphs_replay_the_eager_accumulated_step_bit_for_bit(device, scaling):
    from dvt_amd.dp import Communicator
    comm = Communicator(1, 0, Communicator.unique_id())
    try:
        eager = _accumulated("eager", scaling, comm)
        graph = _accumulated("graph", scaling, comm)
    finally:
        comm.destroy()
    print(f"[graphs] scaling {scaling}: losses {eager[0]} / {graph[0]}, pre-clip norm {float(eager[1][5])}, "
          f"steps {int(eager[1][3][0])}")
    assert float(eager[1][5]) > 1e-3                           # the clip was active
    assert int(eager[1][3][0]) == 4
    assert eager[0] == graph[0]
    for a, b in zip(eager[1], graph[1]):
        assert torch.equal(a, b)
    if scaling:
        assert float(eager[1][6]) == 4096.0                   # grown twice in four steps: the captured scalars moved


def test_changed_set_of_unwritten_parameters_raises_inside_the_capture(device):
    from dvt_amd.dp import FlatParameters
    from dvt_amd.graph import capture_accumulated_step
    x, y = _data(2)
    net = _model().cuda()
    net.register_parameter("probe", torch.nn.Parameter(torch.ones(300, device="cuda")))
    flat = FlatParameters(net, compute_dtype=None)
    seed = torch.full((), flat.accumulation_scale(2), device="cuda")
    passes = []

    def micro():
        loss = net.loss(x, y)[0]
        loss.backward(seed)
        if len(passes) < 2:                                   # the warm-up window writes the probe, the captured one does not
            s = net.probe._dvt_sink
            s.buf.fill_(1.0) if s.fresh else s.buf.add_(1.0)
            s.mark_written()
        passes.append(1)
        flat.finish_backward()
        return loss

    with pytest.raises(RuntimeError, match="set of parameters without a gradient changed"):
        capture_accumulated_step(micro, lambda: flat.adamw_step(lr=1e-3), flat, 2, warmup=1)
    torch.cuda.synchronize()
