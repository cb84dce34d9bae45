"""Patch dropout without a GPU: the entry points of csrc/patch_dropout.hip in include/dvt_hip.h and the derived binding,
``ViViT(patch_dropout=, patch_dropout_mode=)`` and ``keep=``: argument errors, the rule k = n - floor(p n), state-dict keys,
and the argument checks the launchers make before any HIP call."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(dim=64, depth=2, heads=2, dim_head=32)
ENTRY_POINTS = ["dvt_keep_select", "dvt_keep_draw", "dvt_keep_slots", "dvt_patchify_keep", "dvt_patchify_keep_bwd",
                "dvt_tokens_assemble_keep_fwd", "dvt_tokens_assemble_keep_bwd"]


def test_header_declares_the_entry_points_and_the_binding_follows():
    from dvt_amd import _lib
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dvt_hip.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        (params,) = re.findall(rf"\bint\s+{name}\s*\(([^()]*)\)\s*;", code)
        res, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == params.count(",") + 1 and None not in argtypes, name
        assert "dvt_stream_t stream" in params.split(",")[-1], name
    # each cites the call site it specialises
    text = open(os.path.join(ROOT, "include", "dvt_hip.h")).read()
    section = text[text.index("patch dropout (csrc/patch_dropout.hip)"):text.index("dvt_tokens_assemble_keep_bwd(")]
    assert section.count("vit.py:110") + section.count("vit.py:113-115") >= len(ENTRY_POINTS)
    assert os.path.exists(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "patch_dropout.hip"))


def test_launchers_refuse_bad_ranges_before_any_launch():
    from dvt_amd import _lib
    lib = _lib.load()
    one = 16                                   # any non-null address: the arguments are refused before it is used
    assert lib.dvt_keep_select(None, 1, 16, 4, 1, one, one, None) == -1 and b"dvt_keep_select" in lib.dvt_last_error()
    for n, k, rows_per in ((0, 1, 1), (1025, 4, 1), (16, 0, 1), (16, 17, 1), (16, 4, 0)):
        assert lib.dvt_keep_select(one, 1, n, k, rows_per, one, one, None) == -1, (n, k, rows_per)
        assert lib.dvt_keep_draw(one, 0, 1, n, k, rows_per, one, one, None, None) == -1, (n, k, rows_per)
    assert lib.dvt_keep_draw(one, 0, 1, 16, 4, 1, one, None, None, None) == -1
    assert lib.dvt_keep_slots(one, 1, 16, 17, one, None) == -1
    assert lib.dvt_patchify_keep(one, 0, one, 0, one, 4, 3, 32, 32, 8, 2, 17, None) == -1        # k > n = 16
    assert lib.dvt_patchify_keep(one, 0, one, 0, one, 3, 3, 32, 32, 8, 2, 4, None) == -1         # 3 frames, pt = 2
    assert lib.dvt_patchify_keep_bwd(one, 0, one, 0, None, 4, 3, 32, 32, 8, 2, 4, None) == -1
    assert lib.dvt_tokens_assemble_keep_fwd(one, one, one, one, one, 4, 2, 16, 17, 64, 17, 0, None) == -1
    assert lib.dvt_tokens_assemble_keep_fwd(one, one, one, one, one, 4, 2, 16, 4, 64, 16, 0, None) == -1   # pos_rows < n + 1
    assert lib.dvt_tokens_assemble_keep_bwd(one, one, one, one, one, 4, 3, 16, 4, 64, 17, 0, 0, None) == -1  # S % T
    assert b"dvt_tokens_assemble_keep_bwd" in lib.dvt_last_error()


def test_constructor_arguments_and_errors():
    from dvt_amd.models.vit import ViViT
    params = inspect.signature(ViViT.__init__).parameters
    for name, default in (("patch_dropout", 0.0), ("patch_dropout_mode", "tube")):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default
    assert list(inspect.signature(ViViT.forward).parameters) == ["self", "x", "keep"]
    assert list(inspect.signature(ViViT.loss).parameters) == ["self", "x", "target", "keep"]
    net = ViViT(32, 8, 19, 4, patch_dropout=0.5, patch_dropout_mode="frame", **CFG)
    assert net.patch_dropout == 0.5 and net.patch_dropout_mode == "frame"
    assert ViViT(32, 8, 19, 4, **CFG).patch_dropout == 0.0
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="patch_dropout"):
            ViViT(32, 8, 19, 4, patch_dropout=bad, **CFG)
    with pytest.raises(ValueError, match="patch_dropout_mode"):
        ViViT(32, 8, 19, 4, patch_dropout=0.5, patch_dropout_mode="block", **CFG)


def test_the_number_kept_is_n_minus_floor_p_n():
    from dvt_amd.models.vit import ViViT

    def k(image, patch, p):
        return ViViT(image, patch, 19, 4, patch_dropout=p, **CFG).num_kept((image // patch) ** 2)

    # n = 16: floor(0.7 * 16) = 11, floor(0.5 * 16) = 8, floor(0.99 * 16) = 15
    assert k(32, 8, 0.7) == 5 and k(32, 8, 0.5) == 8 and k(32, 8, 0.99) == 1 and k(32, 8, 0.0) == 16
    assert k(32, 8, 0.999) == 1                      # floor(15.984) = 15: one position is always left below p = 1
    assert k(224, 16, 0.5) == 98 and k(224, 16, 0.75) == 49 and k(224, 16, 0.9) == 196 - 176
    with pytest.raises(ValueError, match="patch_dropout"):
        k(32, 8, 1.0)


def test_state_dict_keys_are_those_of_a_default_model():
    from dvt_amd.models.vit import ViViT
    a = ViViT(32, 8, 19, 4, patch_dropout=0.5, **CFG).state_dict()
    b = ViViT(32, 8, 19, 4, **CFG).state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)


def test_a_keep_of_wrong_dtype_shape_or_device_is_refused_on_the_host():
    from dvt_amd.models.vit import ViViT
    net = ViViT(32, 8, 19, 4, patch_dropout=0.5, **CFG)
    x = torch.zeros(2, 4, 3, 32, 32)
    good = torch.arange(5, dtype=torch.int32).repeat(8, 1)
    for keep in (good.long(), good.float(), good[:7], good[0], torch.zeros(8, 0, dtype=torch.int32),
                 torch.arange(17, dtype=torch.int32).repeat(8, 1), good.tolist()):
        with pytest.raises(ValueError, match="keep"):
            net(x, keep=keep)
        with pytest.raises(ValueError, match="keep"):
            net.loss(x, torch.zeros(2, 19), keep=keep)
    with pytest.raises(ValueError, match="keep is on"):
        net(x, keep=good.to("meta"))
    with pytest.raises(RuntimeError, match="no CPU path"):        # a well-formed keep reaches the device operators
        net(x, keep=good)
    net.eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(x)


def test_ops_check_their_index_tables():
    from dvt_amd import functional as F
    from dvt_amd import ops
    keys = torch.zeros(2, 16, dtype=torch.int32)
    with pytest.raises(ValueError, match="int32"):
        ops.keep_select(keys.long(), 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.keep_select(keys, 4)
    with pytest.raises(ValueError, match="shape"):
        ops.patchify_keep(torch.zeros(1, 4, 3, 32, 32), 8, 2, torch.zeros(3, 5, dtype=torch.int32), torch.float32)
    assert list(inspect.signature(F.patch_embed_keep).parameters) == ["clip", "w", "b", "patch", "dtype", "tubelet", "keep", "slot"]
    assert list(inspect.signature(F.tokens_assemble_keep).parameters) == ["emb", "cls", "pos", "keep", "slot", "S", "T"]
