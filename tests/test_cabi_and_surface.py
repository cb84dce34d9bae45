"""CPU-side checks: the C-ABI library builds/loads and exports every symbol of
include/dvt_hip.h (no compute calls without a GPU); the module mirror keeps the
reference's surface; the product path refuses to run without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "dvt_hip.h")).read()


def _declared():
    return sorted(set(re.findall(r"\b(dvt_[a-z0-9_]+)\s*\(", _header())))


def test_library_exports_every_declared_symbol():
    import dvt_amd
    dvt_amd.build_extension(verbose=False)
    lib = ctypes.CDLL(dvt_amd._lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/dvt_hip.h but not exported"
    # the ctypes table covers exactly the header
    assert sorted(dvt_amd._lib.SIGNATURES) == names
    # ... with one argument type per parameter, counted here (commas of the prototype) and not by the binding's parser
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    for n in names:
        (params,) = re.findall(rf"\b{n}\s*\(([^()]*)\)\s*;", code)
        argtypes = dvt_amd._lib.SIGNATURES[n][1]
        assert len(argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), n
        assert None not in argtypes, n


def test_descriptor_layouts_match_the_c_compiler(tmp_path):
    """sizeof of every descriptor struct and offsetof / size of every field, as the host C compiler lays out
    include/dvt_hip.h, against the ctypes Structures the binding derives from the same header."""
    from dvt_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler (cc / gcc / clang) on PATH")
    assert len(_lib.STRUCTS) == len(re.findall(r"\btypedef\s+struct\b", _header())) >= 14
    lines = ['#include <stdio.h>', '#include "dvt_hip.h"', 'int main(void) {']
    for name, st in _lib.STRUCTS.items():
        lines.append(f'  printf("{name} - %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name} {f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f, _ in st._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    compiled = [tuple(line.split()) for line in out.splitlines()]
    derived = []
    for name, st in _lib.STRUCTS.items():
        derived.append((name, "-", str(ctypes.sizeof(st))))
        derived += [(name, f, str(getattr(st, f).offset), str(getattr(st, f).size)) for f, _ in st._fields_]
    assert len(compiled) > 14 and compiled == derived


def test_no_kernel_of_the_library_lost_an_address_space():
    """FLAT loads / stores are what the compiler emits for a pointer whose address space it could not prove (an LDS buffer
    picked from a run-time-indexed pointer array): they count on vmcnt AND lgkmcnt, so every LDS fragment wait also waits for
    the outstanding global loads.  The halo convolution's main loop ran that way for two rounds; tools/check_flat_ops.py
    disassembles the built code object so that it cannot come back unseen."""
    import importlib.util
    import dvt_amd
    dvt_amd.build_extension(verbose=False)
    spec = importlib.util.spec_from_file_location("check_flat_ops", os.path.join(ROOT, "tools", "check_flat_ops.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    gen = {}
    ops = mod.flat_ops(dvt_amd._lib.LIB_PATH, gen)
    assert len(ops) > 300                                                   # the disassembly found the kernels
    bad = {k: v for k, v in ops.items() if v and not any(a in k for a in mod.ALLOWED)}
    assert not bad, f"kernels with FLAT memory instructions: {bad}"
    # the milder form: ds_* accesses whose address is a generic pointer converted (null check + select) per access
    badg = {k: v for k, v in gen.items() if v > mod.GENERIC_LIMIT and not any(a in k for a in mod.ALLOWED)}
    assert not badg, f"kernels converting generic pointers to LDS addresses in bulk: {badg}"


def test_version_and_error_channel_without_gpu():
    import dvt_amd
    lib = dvt_amd._lib.load()
    assert lib.dvt_version() == 5
    # argument validation happens before any HIP call: safe on a CPU-only box
    rc = lib.dvt_cast(None, 0, None, 1, 8, None)
    assert rc == -1
    assert b"dvt_cast" in lib.dvt_last_error()
    rc = lib.dvt_layernorm_fwd(None, None, None, None, None, None, 1, 1, 64, 64, 0, 64, 0, 1e-5, 1, None)
    assert rc == -1


def test_window_convolution_plan_queries_answer_without_a_gpu():
    """dvt_conv3x1_c64_plan, dvt_conv3x1_wgrad_plan, dvt_conv3x1_stream_bn_bwd_plan, dvt_conv3x3_c64_wgrad_plan and
    dvt_conv3x3_stream_plan: host-only, declared in the header, wrapped in ops as tuples; they report the layer-1 workload's
    instantiations and refuse what the launchers refuse (tests/test_window_conv_coverage.py sweeps them)."""
    import dvt_amd
    from dvt_amd import ops
    declared = _declared()
    for n in ("dvt_conv3x1_c64_plan", "dvt_conv3x1_wgrad_plan", "dvt_conv3x1_stream_bn_bwd_plan", "dvt_conv3x3_c64_wgrad_plan",
              "dvt_conv3x3_stream_plan"):
        assert n in declared and n in dvt_amd._lib.SIGNATURES
    assert dvt_amd._lib.ENUMS["dvt_conv3x1_bn_bwd_kernel"] == {"DVT_CONV3X1_BN_BWD_NONE": 0, "DVT_CONV3X1_BN_BWD_WINDOW": 1,
                                                               "DVT_CONV3X1_BN_BWD_STREAM": 2}
    bf = torch.bfloat16
    # R(2+1)D-18 layer 1 at 28 clips of 12 x 56 x 56, ResNet-18 layer 1 at 256 frames of 56 x 56
    assert ops.conv3x1_c64_plan(28, 12, 3136, bf) == 6
    assert ops.conv3x1_stream_bn_bwd_plan(28, 12, 3136, bf) == ops.BnBwdPlan("window", 6)
    assert ops.conv3x1_wgrad_plan(28, 12, 3136, bf) is True
    assert ops.conv3x3_c64_wgrad_plan(256, 56, 56, 64, bf) == ((0, 64, 4),)
    assert ops.conv3x3_c64_wgrad_plan(336, 56, 56, 144, bf) == ((0, 64, 4), (64, 80, 5))
    assert ops.conv3x3_stream_plan(336, 56, 56, 64, 144, bf) == ops.StreamPlan(64, 144, 1)
    assert ops.conv3x3_stream_plan(336, 28, 28, 288, 128, bf) == ops.StreamPlan(288, 64, 2)
    for plan in (ops.conv3x1_c64_plan(3, 5, 32, bf), ops.conv3x1_wgrad_plan(3, 5, 32, bf), ops.conv3x1_stream_bn_bwd_plan(2, 2, 32, bf),
                 ops.conv3x3_c64_wgrad_plan(2, 13, 20, 72, bf), ops.conv3x3_stream_plan(2, 13, 20, 64, 64, bf),
                 ops.conv3x1_c64_plan(28, 12, 3136, torch.float32)):
        assert plan is None


def test_vivit_surface_matches_reference_state_dict():
    from dvt_amd.models.vit import ViViT, Transformer, Attention, FeedForward, PreNorm
    from tests.util import golden
    g = golden("vivit_tiny.npz")
    net = ViViT(32, 8, 19, 3, dim=64, depth=2, heads=2, dim_head=32)
    ref_keys = [k[2:] for k in g.files if k.startswith("w:")]
    assert [k for k, _ in net.named_parameters()] == ref_keys
    for k, p in net.named_parameters():
        assert tuple(p.shape) == g["w:" + k].shape, k
    # default constructor arguments of the reference (vit.py:80-81)
    d = ViViT(224, 16, 100, 16)
    assert d.pos_embedding.shape == (1, 16, 197, 192) and d.pool == "cls"
    assert isinstance(Attention(64, heads=1, dim_head=64).to_out, torch.nn.Identity)


def test_product_path_has_no_cpu_fallback():
    from dvt_amd.models.vit import ViViT
    net = ViViT(32, 8, 19, 3, dim=64, depth=1, heads=2, dim_head=32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(torch.randn(1, 3, 3, 32, 32))


def test_product_code_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "data-efficient-video-transformers_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("# oracle", ""), os.path.join(dirpath, f)


def test_frame_transformer_vid_mode_has_the_reference_state_dict_keys():
    """frame_transformer.py:83-121 as executed (image branch commented out): a model="vid" mirror must expose exactly
    position_encoder.pe, vid_model.backbone.* (torchvision R(2+1)D names, fc.0.*), distil_transformer.transformer.layers.*,
    vid_cls, img_mlp_head.{0,2,4}.*, norm.* -- so reference checkpoints load with strict=True."""
    import torch
    from dvt_amd.models.frame_transformer import FrameTransformer
    net = FrameTransformer(batch_size=2, seq_len=13, cls=1, model="vid", opt="adamW", learning_rate=5e-6, weight_decay=0.09,
                           momentum=0.005)
    keys = list(net.state_dict().keys())
    tops = sorted({k.split(".")[0] for k in keys})
    assert tops == ["distil_transformer", "img_mlp_head", "norm", "position_encoder", "vid_cls", "vid_model"], tops
    sd = net.state_dict()
    assert sd["vid_cls"].shape == (1, 12, 3, 112, 112) and sd["position_encoder.pe"].shape[2] == 896
    assert sd["distil_transformer.transformer.layers.0.self_attn.in_proj_weight"].shape == (2688, 896)
    assert sd["distil_transformer.transformer.layers.3.linear1.weight"].shape == (512, 896)
    assert sd["vid_model.backbone.fc.0.weight"].shape == (896, 512)
    assert sd["vid_model.backbone.stem.0.weight"].shape == (45, 3, 1, 7, 7)
    assert sd["vid_model.backbone.layer2.0.conv1.0.0.weight"].shape == (230, 64, 1, 3, 3)
    assert {k for k in keys if k.startswith("img_mlp_head")} == {f"img_mlp_head.{i}.{n}" for i in (0, 2, 4) for n in ("weight", "bias")}
    # the image-branch modes add the members the reference left commented out
    net2 = FrameTransformer(batch_size=2, seq_len=13, cls=1, model="sum", opt="adamW", learning_rate=5e-6, weight_decay=0.09,
                            momentum=0.005)
    assert {"img_model", "scene_transformer", "img_cls"} <= {k.split(".")[0] for k in net2.state_dict()}


def test_src_layout_shim_resolves_the_drivers_imports(tmp_path):
    """with ``shim/src`` on PYTHONPATH the driver's ``from models.frame_transformer import
    FrameTransformer`` / ``from models.transformer import SimpleTransformer`` (main.py:14-15) resolve to the build's
    classes from a ``src/``-style working directory whose own ``models/`` holds the modules the build does not
    replace (``models.LSTM``, main.py:13) -- emulated in a temp directory; the reference tree is not read."""
    import inspect
    import subprocess
    import sys
    src = tmp_path / "src"
    (src / "models").mkdir(parents=True)                       # like the reference: no __init__.py in src/models
    (src / "models" / "LSTM.py").write_text("class LSTMRegressor:\n    origin = 'reference tree'\n")
    (src / "models" / "vit.py").write_text("raise RuntimeError('the reference file must be shadowed by the shim')\n")
    (src / "main.py").write_text(
        "from models.LSTM import LSTMRegressor\n"
        "from models.transformer import SimpleTransformer\n"
        "from models.frame_transformer import FrameTransformer\n"
        "from models.vit import ViViT\n"
        "from models.custom_resnet import resnet18\n"
        "from models.TPN import TPN, Reasoning\n"
        "from models.losses.ntxent import ContrastiveLoss\n"
        "import dvt_amd.models.frame_transformer as B, dvt_amd.models.transformer as Tm, dvt_amd.models.vit as V\n"
        "assert FrameTransformer is B.FrameTransformer and SimpleTransformer is Tm.SimpleTransformer and ViViT is V.ViViT\n"
        "assert LSTMRegressor.origin == 'reference tree'\n"
        "print('SHIM-OK')\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "shim", "src"))
    r = subprocess.run([sys.executable, "main.py"], cwd=str(src), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SHIM-OK" in r.stdout, r.stderr[-2000:]
    # constructor signatures the driver relies on: Model(**config) (main.py:38,44) and ViViT's positional order (vit.py:80-81)
    from dvt_amd.models.frame_transformer import FrameTransformer
    from dvt_amd.models.transformer import SimpleTransformer
    from dvt_amd.models.vit import ViViT
    for cls in (FrameTransformer, SimpleTransformer):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert params[-1].kind is inspect.Parameter.VAR_KEYWORD, cls
    names = list(inspect.signature(ViViT.__init__).parameters)
    assert names[1:14] == ["image_size", "patch_size", "num_classes", "num_frames", "dim", "depth", "heads", "pool",
                           "in_channels", "dim_head", "dropout", "emb_dropout", "scale_dim"]
