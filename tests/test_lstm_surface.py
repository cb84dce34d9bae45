"""CPU-side checks of the LSTM baseline (src/models/LSTM.py): the LSTMRegressor surface and state dict match the
reference's, and the chain entry points of the C ABI validate their arguments before touching the GPU."""
import inspect

import pytest
import torch
from torch import nn

# LSTMRegressor.__init__ of the reference (src/models/LSTM.py:13-21), in order
REFERENCE_PARAMS = ["n_features", "hidden_size", "seq_len", "batch_size", "num_layers", "dropout", "learning_rate",
                    "criterion"]


def _model(**kw):
    from dvt_amd.models.LSTM import LSTMRegressor
    args = dict(seq_len=200, batch_size=64, criterion=nn.BCELoss(), n_features=4608, hidden_size=512, num_layers=4,
                dropout=0.2, learning_rate=5e-5)
    args.update(kw)
    return LSTMRegressor(**args)


def test_constructor_parameters_equal_the_reference():
    from dvt_amd.models.LSTM import LSTMRegressor
    assert list(inspect.signature(LSTMRegressor.__init__).parameters)[1:] == REFERENCE_PARAMS


def test_attributes_of_the_reference():
    m = _model()
    for name in ("lstm", "linear", "criterion", "running_logits", "running_labels", "learning_rate", "n_features",
                 "hidden_size", "seq_len", "batch_size", "num_layers", "dropout"):
        assert hasattr(m, name), name
    assert m.running_logits == [] and m.running_labels == [] and m.learning_rate == 5e-5
    assert isinstance(m.criterion, nn.BCELoss)


def test_state_dict_equals_nn_lstm_plus_linear_and_loads():
    m = _model()
    ref = nn.Module()
    ref.lstm = nn.LSTM(input_size=4608, hidden_size=512, batch_first=True, num_layers=4, dropout=0.2)
    ref.linear = nn.Linear(512, 15)
    ours, theirs = m.state_dict(), ref.state_dict()
    assert list(ours) == list(theirs)
    for k in theirs:
        assert ours[k].shape == theirs[k].shape, k
    res = m.load_state_dict(theirs, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.state_dict()["lstm.weight_hh_l3"], theirs["lstm.weight_hh_l3"])


def test_initialisation_draws_like_nn_lstm():
    from dvt_amd.models.LSTM import LSTM
    torch.manual_seed(7)
    ref = nn.LSTM(64, 32, 2, batch_first=True)
    torch.manual_seed(7)
    ours = LSTM(64, 32, 2)
    for k, v in ref.state_dict().items():
        assert torch.equal(ours.state_dict()[k], v), k


def test_other_criterion_is_refused():
    with pytest.raises(NotImplementedError, match="BCELoss"):
        _model(criterion=nn.MSELoss())
    with pytest.raises(NotImplementedError, match="BCELoss"):
        _model(criterion=nn.BCELoss(reduction="sum"))


def test_optimizer_is_adam_arithmetic():
    from dvt_amd import optim
    opt = _model(n_features=64, hidden_size=32, num_layers=2).configure_optimizers()
    assert isinstance(opt, optim.AdamW)
    g = opt.param_groups[0]
    assert g["lr"] == 5e-5 and g["weight_decay"] == 0


def test_lstm_entry_points_validate_before_any_hip_call():
    import dvt_amd
    lib = dvt_amd._lib.load()
    p = 256                                            # any non-null, 16-byte aligned address: never dereferenced here
    rc = lib.dvt_lstm_seq_fwd(None, None, None, p, p, p, p, p, None, 4, 16, 32, 1, None)
    assert rc == -1 and b"dvt_lstm_seq_fwd" in lib.dvt_last_error()
    rc = lib.dvt_lstm_seq_bwd(p, p, p, None, p, None, p, 4, 16, 32, 1, None)
    assert rc == -1 and b"dvt_lstm_seq_bwd" in lib.dvt_last_error()
    rc = lib.dvt_lstm_seq_bwd(p, p, p, None, None, p, p, 4, 16, 32, 1, None)        # no incoming gradient at all
    assert rc == -1 and b"dvt_lstm_seq_bwd" in lib.dvt_last_error()
    # unsupported shapes / dtypes: -2 with a message, never a fallback
    rc = lib.dvt_lstm_seq_fwd(p, None, None, p, p, p, p, p, None, 4, 16, 24, 1, None)
    assert rc == -2 and b"multiple of 16" in lib.dvt_last_error()
    rc = lib.dvt_lstm_seq_bwd(p, p, p, p, None, p, p, 4, 16, 40, 0, None)
    assert rc == -2 and b"dvt_lstm_seq_bwd" in lib.dvt_last_error()
    rc = lib.dvt_lstm_seq_fwd(p, None, None, p, p, p, p, p, None, 4, 16, 32, 7, None)
    assert rc == -2
    rc = lib.dvt_lstm_seq_fwd(p, None, None, p, p, p, p, p, None, 0, 16, 32, 1, None)
    assert rc == -1
    assert lib.dvt_lstm_seq_bwd_workspace_bytes(64, 512, 1) >= 4 * 512 * 512 * 2 + 64 * 512 * 4
    rc = lib.dvt_sigmoid_bce_fwd(None, p, p, None, 15, 0, None)
    assert rc == -1 and b"dvt_sigmoid_bce_fwd" in lib.dvt_last_error()
    rc = lib.dvt_sigmoid_bce_bwd(p, p, p, None, 15, 0, None)
    assert rc == -1 and b"dvt_sigmoid_bce_bwd" in lib.dvt_last_error()


def test_lstm_regressor_has_no_cpu_path():
    m = _model(n_features=64, hidden_size=32, num_layers=2, dropout=0.0)
    batch = {"experts": [torch.randn(1, 16, 64) for _ in range(2)], "label": [torch.zeros(1, 15) for _ in range(2)]}
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.training_step(batch, 0)
