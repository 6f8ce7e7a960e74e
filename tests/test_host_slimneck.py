"""CPU: the slim-neck blocks GSConv, GSBottleneck and VoVGSCSP (reference nn/extra_modules/block.py:886-967) -- the float64
restatement of the shuffle entries (tests/slimneck_ref.py) against the reference's reshape / permute form and autograd; the modules,
the parser, the YAML against what the reference builds from it (parameter count, state-dict layout, the fresh BatchNorm buffers with
``res.bn`` never run), every refusal of the supported set, the declared unused parameters, the header and the checkpoints."""
import os

import pytest
import torch
import yaml

import slimneck_ref as R
import slimneck_util as U
from conftest import CFG_DIR, ROOT

SMALL = [g for g in U.KERNEL_CASES if g != U.BIG] + [U.SLICED]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


# ----------------------------------------------------------------------------- the restatement against the reference's form
@pytest.mark.parametrize("n", [16, 48, 32, 64, 128])
def test_shuffle_is_even_channels_then_odd_channels(n):
    """The reference's reshape / permute / reshape / cat lines (block.py:902-908) == cat(x2[:, 0::2], x2[:, 1::2]) == the restatement,
    for n = 2 c_ channels (16 and 48: one straddling group alone, and one in the middle)."""
    x2 = torch.randn(2, n, 3, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(n))
    want = R.reference_form(x2)
    assert torch.equal(want, torch.cat((x2[:, 0::2], x2[:, 1::2]), 1))
    got = R.forward(_nhwc(x2[:, :n // 2]), _nhwc(x2[:, n // 2:]))
    assert torch.equal(_nchw(got), want)


@pytest.mark.parametrize("geom", SMALL, ids=[U.case_id(g) for g in SMALL])
def test_inverse_is_autograd_of_the_reference_form(geom):
    N, H, W, c = geom
    t = U.normal_inputs(geom, 2)
    x1 = _nchw(t["x1"].double()).clone().requires_grad_(True)
    d = _nchw(t["d"].double()).clone().requires_grad_(True)
    y = R.reference_form(torch.cat((x1, d), 1))
    assert torch.equal(_nhwc(y.detach()), R.forward(t["x1"].double(), t["d"].double()))
    y.backward(_nchw(t["dy"].double()))
    g1, gd = R.backward(t["dy"].double())
    assert torch.equal(_nhwc(x1.grad), g1) and torch.equal(_nhwc(d.grad), gd)
    # a permutation: the inverse of the forward, and every element of dy lands exactly once
    b1, bd = R.backward(R.forward(t["x1"], t["d"]))
    assert torch.equal(b1, t["x1"]) and torch.equal(bd, t["d"])


# ----------------------------------------------------------------------------- modules
def _model(name=U.MODEL):
    from ultralytics.nn.tasks import DetectionModel
    return DetectionModel(os.path.join(CFG_DIR, name + ".yaml"), ch=3, verbose=False)


def _build(case):
    from ultralytics.nn.extra_modules import block as B
    cls, args, H, W = U.MODULE_CASES[case]
    return getattr(B, cls)(*args)


def test_module_keys_class_paths_and_attributes(golden):
    import torch.nn as nn
    from ultralytics.nn.extra_modules.block import GSBottleneck, GSConv, VoVGSCSP
    from ultralytics.nn.modules import Conv
    G = golden("slimneck")
    for cls in (GSConv, GSBottleneck, VoVGSCSP):
        assert cls.__module__ == "ultralytics.nn.extra_modules.block"
    m = GSConv(16, 32, 3, 2)
    assert isinstance(m.cv1, Conv) and isinstance(m.cv2, Conv)
    assert (m.cv1.conv.in_channels, m.cv1.conv.out_channels, m.cv1.conv.kernel_size, m.cv1.conv.stride, m.cv1.conv.groups) == (16, 16, (3, 3), (2, 2), 1)
    assert (m.cv2.conv.in_channels, m.cv2.conv.out_channels, m.cv2.conv.kernel_size, m.cv2.conv.stride, m.cv2.conv.padding, m.cv2.conv.groups) == \
        (16, 16, (5, 5), (1, 1), (2, 2), 16)
    assert m.out_hw(15, 17) == (8, 9) and GSConv(32, 16, 1, 1).out_hw(16, 16) == (16, 16)
    # ``act`` is accepted and ignored: both Convs keep SiLU
    g = GSConv(16, 32, 3, 1, act=False)
    assert isinstance(g.cv1.act, nn.SiLU) and isinstance(g.cv2.act, nn.SiLU)
    b = GSBottleneck(32, 32, k=7, s=2, e=1.0)  # k and s are ignored
    assert isinstance(b.conv_lighting, nn.Sequential) and len(b.conv_lighting) == 2
    assert b.conv_lighting[0].cv1.conv.kernel_size == (1, 1) and b.conv_lighting[1].cv1.conv.kernel_size == (3, 3)
    assert b.conv_lighting[1].cv1.conv.stride == (1, 1) and isinstance(b.conv_lighting[1].cv1.act, nn.SiLU)
    assert isinstance(b.shortcut.act, nn.Identity) and b.shortcut.conv.kernel_size == (1, 1)
    v = VoVGSCSP(32, 32, 2, False, 4)  # shortcut and g are ignored
    assert len(v.gsb) == 2 and isinstance(v.res.act, nn.Identity) and v.res.conv.kernel_size == (3, 3)
    assert (v.cv3.conv.in_channels, v.cv3.conv.out_channels) == (32, 32)
    for case in U.MODULE_CASES:
        want = U.layout(G, f"mod/{case}")
        got = {k: tuple(t.shape) for k, t in _build(case).state_dict().items()}
        assert got == want and list(got) == list(want), case


def test_unused_parameters_are_exactly_res(golden):
    """What VoVGSCSP declares as never read is what the reference's backward leaves without a gradient."""
    G = golden("slimneck")
    m = _model()
    unrun = {id(s) for mod in m.modules() if hasattr(mod, "unused_modules") for u in mod.unused_modules() for s in u.modules()}
    names = [f"{mn}.{pn}" for mn, mod in m.named_modules() if id(mod) in unrun for pn, _ in mod.named_parameters(recurse=False)]
    assert names == [str(k) for k in G[f"{U.MODEL}/unused"]]
    assert names == [f"model.{i}.res.{s}" for i in U.VOV_LAYERS for s in ("conv.weight", "bn.weight", "bn.bias")]
    assert all(dict(m.named_parameters())[k].requires_grad for k in names)  # as in the reference
    case = "vov_32_32"
    assert [str(k) for k in G[f"mod/{case}/nograd"]] == ["res.conv.weight", "res.bn.weight", "res.bn.bias"]
    assert [str(k) for k in G["mod/gs_32_16_k1/nograd"]] == [""]
    from ultralytics.nn.extra_modules.block import GSConv
    assert GSConv(16, 16).unused_modules() == ()


def test_flat_mask_covers_exactly_the_res_tensors():
    """The flat layout on the host (as tests/test_host_any_nc.py builds it): the frozen mask is set on exactly the ``res.*`` slices (and
    the padding behind every tensor), their ``.grad`` is None as in the reference, every other parameter's is its flat view."""
    from types import SimpleNamespace
    from ultralytics.hip.runtime import PAD, Runtime
    m = _model()
    rt = object.__new__(Runtime)
    rt.root, rt.eng = m, SimpleNamespace(device=torch.device("cpu"))
    rt._flatten()
    names = rt.unused_parameter_names()
    assert sorted(names) == sorted(f"model.{i}.res.{s}" for i in U.VOV_LAYERS for s in ("conv.weight", "bn.weight", "bn.bias"))
    want = torch.zeros_like(rt.frozen)
    for n, p in m.named_parameters():
        o, k = rt.param_off[n], p.numel()
        want[o + k:o + (k + PAD - 1) // PAD * PAD] = 1
        if n in names:
            want[o:o + k] = 1
            assert p.grad is None and p.requires_grad and not rt.updates(p), n
        elif not p.requires_grad:  # (Detect's DFL weights are built frozen)
            assert ".dfl." in n
            want[o:o + k] = 1
        else:
            assert p.grad.data_ptr() == rt.flat_g[o:].data_ptr() and rt.updates(p), n
    assert torch.equal(rt.frozen, want)
    d = _model("yolov8n-ASF-P2P2")
    rd = object.__new__(Runtime)
    rd.root, rd.eng = d, SimpleNamespace(device=torch.device("cpu"))
    rd._flatten()
    assert rd.unused_parameter_names() == [] and rd.unused_mods == set()


GS_BAD = [dict(c1=12, c2=32), dict(c1=16, c2=24), dict(c1=16, c2=8), dict(c1=16, c2=32, k=5), dict(c1=16, c2=32, k=1, s=2), dict(c1=16, c2=32, k=3, s=3),
          dict(c1=16, c2=32, k=3, s=1, p=1), dict(c1=16, c2=32, g=2), dict(c1=16, c2=32, k=3, d=2)]


@pytest.mark.parametrize("kw", GS_BAD, ids=["-".join(f"{k}{v}" for k, v in kw.items()) for kw in GS_BAD])
def test_gsconv_constructor_refuses_by_name(kw):
    from ultralytics.nn.extra_modules.block import GSConv
    full = dict(dict(k=1, s=1, p=None, g=1, d=1), **kw)
    text = rf"GSConv\(c1={full['c1']}, c2={full['c2']}, k={full['k']}, s={full['s']}, p={full['p']}, g={full['g']}, d={full['d']}\) is outside the HIP hot path " \
           r"\(supported: GSConv with c1 % 8 == 0, c2 % 16 == 0"
    with pytest.raises(NotImplementedError, match=text):
        GSConv(**kw)


@pytest.mark.parametrize("cls,c1,c2,e", [("VoVGSCSP", 32, 48, 0.5), ("VoVGSCSP", 12, 32, 0.5), ("VoVGSCSP", 32, 32, 0.25), ("GSBottleneck", 32, 48, 0.5),
                                         ("GSBottleneck", 32, 16, 0.5)])
def test_block_constructors_refuse_by_name(cls, c1, c2, e):
    from ultralytics.nn.extra_modules import block as B
    with pytest.raises(NotImplementedError, match=rf"{cls}\(c1={c1}, c2={c2}, e={e}\) is outside the HIP hot path .*int\(c2 \* e\) % 16 == 0"):
        getattr(B, cls)(c1, c2, e=e)


@pytest.mark.parametrize("n", [0, -1])
def test_vovgscsp_without_a_bottleneck_is_refused(n):
    from ultralytics.nn.extra_modules.block import VoVGSCSP
    with pytest.raises(NotImplementedError, match=rf"VoVGSCSP\(c1=32, c2=32, n={n}\) is outside the HIP hot path .*n >= 1"):
        VoVGSCSP(32, 32, n)


def _custom(rows, nc=6):
    return {"nc": nc, "scales": {"n": [1.0, 1.0, 1024]}, "scale": "n", "backbone": rows, "head": [[[-1], 1, "Detect", ["nc"]]]}


def test_parser_refuses_by_layer():
    from ultralytics.nn.tasks import DetectionModel
    with pytest.raises(NotImplementedError, match=r"layer 1 \(GSConv\)\(c1=32, c2=24, k=3, s=2, p=None, g=1, d=1\) is outside the HIP hot path"):
        DetectionModel(_custom([[-1, 1, "Conv", [32, 3, 2]], [-1, 1, "GSConv", [24, 3, 2]]]), verbose=False)
    with pytest.raises(NotImplementedError, match=r"layer 1 \(GSConv\)\(c1=32, c2=32, k=5, s=1, p=None, g=1, d=1\) is outside the HIP hot path"):
        DetectionModel(_custom([[-1, 1, "Conv", [32, 3, 2]], [-1, 1, "GSConv", [32, 5, 1]]]), verbose=False)
    with pytest.raises(NotImplementedError, match=r"layer 1 \(VoVGSCSP\)\(c1=32, c2=48, e=0.5\) is outside the HIP hot path"):
        DetectionModel(_custom([[-1, 1, "Conv", [32, 3, 2]], [-1, 3, "VoVGSCSP", [48]]]), verbose=False)
    with pytest.raises(NotImplementedError, match=r"layer 1 \(GSConv\) reads layer 0, which is 12 channels wide"):
        DetectionModel(_custom([[-1, 1, "Conv", ["nc", 3, 2]], [-1, 1, "GSConv", [32]]], nc=12), verbose=False)
    with pytest.raises(NotImplementedError, match=r"layer 1 \(VoVGSCSP\) would be 12 channels wide"):
        DetectionModel(_custom([[-1, 1, "Conv", [32, 3, 2]], [-1, 1, "VoVGSCSP", ["nc"]]], nc=12), verbose=False)
    for name in ("GSConvns", "VoVGSCSPns", "VoVGSCSPC"):
        with pytest.raises(NotImplementedError, match=rf"module '{name}' is outside the DEAL-YOLO hot path"):
            DetectionModel(_custom([[-1, 1, "Conv", [32, 3, 2]], [-1, 1, name, [32]]]), verbose=False)
    # ... and supported rows build: the repeat count goes into VoVGSCSP as for C2f, a GSConv row down-samples by its s
    m = DetectionModel(_custom([[-1, 1, "Conv", [32, 3, 2]], [-1, 1, "GSConv", [64, 3, 2]], [-1, 3, "VoVGSCSP", [32]]]), verbose=False)
    assert m._cout[:3] == [32, 64, 32] and m.stride.tolist() == [4.0] and len(m.model[2].gsb) == 3


def test_graph_builds_like_the_reference(golden):
    from ultralytics.nn.extra_modules.block import GSConv, VoVGSCSP
    G = golden("slimneck")
    m = _model()
    assert [type(m.model[i]) for i in U.VOV_LAYERS] == [VoVGSCSP] * 4 and [type(m.model[i]) for i in U.GS_LAYERS] == [GSConv] * 2
    assert [(m.model[i].cv1.conv.in_channels, m.model[i].cv3.conv.out_channels) for i in U.VOV_LAYERS] == list(U.VOV_WIDTHS.values())
    assert [(m.model[i].cv1.conv.in_channels, 2 * m.model[i].cv1.conv.out_channels) for i in U.GS_LAYERS] == list(U.GS_WIDTHS.values())
    assert sum(q.numel() for q in m.parameters()) == int(G[f"{U.MODEL}/n_params"]) == 947538
    assert m.stride.tolist() == G[f"{U.MODEL}/stride"].tolist() == [4.0, 8.0, 16.0]
    want = U.layout(G, U.MODEL)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want) and got == want
    assert [m._cout[i] for i in U.VOV_LAYERS + U.GS_LAYERS] == [c2 for _, c2 in list(U.VOV_WIDTHS.values()) + list(U.GS_WIDTHS.values())]
    assert m.model[12].type == "ultralytics.nn.extra_modules.block.VoVGSCSP" and m.model[18].type == "ultralytics.nn.extra_modules.block.GSConv"
    assert m.model[12].np == sum(q.numel() for q in m.model[12].parameters())  # (res counted)
    head = open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2-SlimNeck.yaml")).read().split("nc:")[0]
    flat = " ".join(head.replace("#", " ").split())
    assert "project's own reading" in flat and "ship no YAML" in flat
    a = yaml.safe_load(open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2-SlimNeck.yaml")))
    d = yaml.safe_load(open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2.yaml")))
    for i, (ra, rd) in enumerate(zip(a["backbone"] + a["head"], d["backbone"] + d["head"])):
        if i in U.VOV_LAYERS:
            assert ra == [rd[0], rd[1], "VoVGSCSP", [rd[3][0]]] and rd[2] == "C2f", i
        elif i in U.GS_LAYERS:
            assert ra == [rd[0], rd[1], "GSConv", rd[3]] and rd[2] == "Conv" and rd[3][1:] == [3, 2], i
        else:
            assert ra == rd, i


def test_fresh_batchnorm_buffers_are_the_references(golden):
    """The stride probe's side effect reaches every BatchNorm a forward runs -- and never ``res.bn``, which keeps (0, 1, 0)."""
    G = golden("slimneck")
    sd = _model().state_dict()
    names = [str(k) for k in G[f"{U.MODEL}/fresh_names"]]
    assert len(names) > 100 and sum(".res.bn." in k for k in names) == 3 * len(U.VOV_LAYERS)
    for k, lo, hi in zip(names, G[f"{U.MODEL}/fresh_min"], G[f"{U.MODEL}/fresh_max"]):
        assert float(sd[k].min()) == pytest.approx(float(lo), abs=1e-7) and float(sd[k].max()) == pytest.approx(float(hi), abs=1e-7), k
    for i in U.VOV_LAYERS:
        bn = f"model.{i}.res.bn."
        assert float(sd[bn + "running_mean"].abs().max()) == 0.0 and torch.equal(sd[bn + "running_var"], torch.ones_like(sd[bn + "running_var"]))
        assert int(sd[bn + "num_batches_tracked"]) == 0 and int(sd[f"model.{i}.cv3.bn.num_batches_tracked"]) == 1
        assert float(sd[f"model.{i}.gsb.0.shortcut.bn.running_var"][0]) == pytest.approx(0.9)


def test_fuse_folds_every_conv_res_included():
    m = _model().eval()
    m.fuse()
    from ultralytics.nn.modules import Conv
    convs = [c for i in U.VOV_LAYERS + U.GS_LAYERS for c in m.model[i].modules() if isinstance(c, Conv)]
    assert len(convs) == 4 * 9 + 2 * 2  # VoVGSCSP: cv1, cv2, cv3, res, the shortcut and two GSConvs of two Convs each
    for cv in convs:
        assert not hasattr(cv, "bn") and cv.conv.bias is not None
    assert m.model[12].res.conv.bias is not None


def test_freeze_names_cover_the_blocks():
    from ultralytics.engine.trainer import frozen_parameter_names
    names = [k for k, _ in _model().named_parameters()]
    frozen = set(frozen_parameter_names(names, [18]))
    assert {"model.18.cv1.conv.weight", "model.18.cv2.conv.weight", "model.18.cv2.bn.bias"} <= frozen and "model.17.cv3.conv.weight" not in frozen
    frozen = set(frozen_parameter_names(names, 13))
    assert {"model.12.res.conv.weight", "model.12.gsb.0.shortcut.bn.weight"} <= frozen and "model.13.conv.weight" not in frozen


# ----------------------------------------------------------------------------- header and binding
def test_header_declares_and_the_library_binds_the_entry_points():
    import ctypes as C
    from ultralytics.hip import SIGNATURES, lib
    txt = open(os.path.join(ROOT, "include", "dealyolo_hip.h")).read()
    for name, nargs in (("dy_gs_shuffle_forward", 11), ("dy_gs_shuffle_backward", 13)):
        assert f"int {name}(" in txt
        res, args = SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
        assert getattr(lib(), name).argtypes == list(args)
    assert "block.py:896-908" in txt  # the reference lines the entries replace
    assert "gsconv.hip" in open(os.path.join(ROOT, "experiment-yolo_amd", "csrc", "Makefile")).read()
    L = lib()
    # refusals need no device: nothing is launched (host numbers stand in for pointers)
    ARG, ALIGN = -1, -3
    base = dict(x1=4096, ld1=16, d=8192, ldd=16, y=16384, ldy=32, n=1, H=4, W=4, c=16)

    def fwd(**kw):
        v = dict(base, **kw)
        return L.dy_gs_shuffle_forward(v["x1"], v["ld1"], v["d"], v["ldd"], v["y"], v["ldy"], v["n"], v["H"], v["W"], v["c"], None)

    def bwd(**kw):
        v = dict(base, **kw)  # (x1, d stand for dx1, dd; y for dy)
        return L.dy_gs_shuffle_backward(v["y"], v["ldy"], v["x1"], v["ld1"], 0, v["d"], v["ldd"], 0, v["n"], v["H"], v["W"], v["c"], None)

    for f in (fwd, bwd):
        assert f(y=0) == ARG and f(n=0) == ARG and f(H=0) == ARG and f(W=0) == ARG and f(c=0) == ARG and f(c=4) == ARG
        assert f(ld1=8) == ARG and f(ldd=8) == ARG and f(ldy=24) == ARG                       # pitches below the width
        assert f(c=12) == ALIGN and f(ld1=20) == ALIGN and f(ldd=20) == ALIGN and f(ldy=36) == ALIGN
        assert f(x1=4104) == ALIGN and f(d=8200) == ALIGN and f(y=16392) == ALIGN
    assert fwd(x1=0) == ARG and fwd(d=0) == ARG
    assert bwd(x1=0, d=0) == 0                                # both destinations null: nothing to launch
    assert bwd(x1=0, ld1=3, d=0, ldd=5) == 0                  # (a null destination's pitch is not looked at)


# ----------------------------------------------------------------------------- checkpoints
def test_reference_written_checkpoint_rebuilds(golden):
    """tests/golden/ref_ckpt_slimneck.pt: a whole-module fp16 pickle written by the REFERENCE's classes; its module paths
    ultralytics.nn.extra_modules.block.{GSConv, GSBottleneck, VoVGSCSP} resolve to this package's classes; strict=True."""
    from ultralytics.nn.extra_modules.block import GSBottleneck, GSConv, VoVGSCSP
    from ultralytics.nn.tasks import DetectionModel, _rebuild, attempt_load_weights, torch_safe_load
    G = golden("slimneck")
    ckpt, _ = torch_safe_load(U.CKPT)
    obj = ckpt["model"]
    assert [type(obj.model[i]) for i in U.VOV_LAYERS] == [VoVGSCSP] * 4 and [type(obj.model[i]) for i in U.GS_LAYERS] == [GSConv] * 2
    assert type(obj.model[12].gsb[0]) is GSBottleneck
    m = _rebuild(obj, ckpt)
    assert isinstance(m, DetectionModel)
    assert [m.model[i].cv3.conv.out_channels for i in U.VOV_LAYERS] == G["ckpt/vov_channels"].tolist() == [32, 32, 32, 32]
    assert sum(q.numel() for q in m.parameters()) == int(G["ckpt/n_params"])
    want = U.state(G, "ckpt")
    got = m.state_dict()
    assert list(want) == list(got)
    for k, v in want.items():
        assert torch.equal(got[k].float(), (v.half().float() if v.is_floating_point() else v.float())), k
    assert not attempt_load_weights(U.CKPT).training


def test_checkpoint_roundtrip_in_the_reference_format(tmp_path):
    """``reference_module_copy`` (through save_reference_format) and back."""
    from ultralytics.nn.extra_modules.block import GSConv, VoVGSCSP
    from ultralytics.nn.tasks import attempt_load_weights, reference_module_copy, save_reference_format, torch_safe_load
    m = _model()
    cp = reference_module_copy(m)
    assert next(cp.parameters()).dtype == torch.float16 and list(cp.state_dict()) == list(m.state_dict())
    path = save_reference_format(str(tmp_path / "last.pt"), m, updates=4, epoch=1, train_args={"imgsz": 64})
    obj = torch_safe_load(path)[0]["model"]
    assert next(obj.parameters()).dtype == torch.float16 and all("rt" not in mod.__dict__ for mod in obj.modules())
    assert [type(obj.model[i]) for i in U.VOV_LAYERS] == [VoVGSCSP] * 4 and [type(obj.model[i]) for i in U.GS_LAYERS] == [GSConv] * 2
    back = attempt_load_weights(path)
    for (k, a), (_, b) in zip(m.state_dict().items(), back.state_dict().items()):
        assert torch.equal(a.half().float() if a.is_floating_point() else a, b.float() if a.is_floating_point() else b), k
