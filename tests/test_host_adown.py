"""CPU: ADown (reference nn/extra_modules/block.py:4685-4698) -- the float64 restatement of the pool entries (tests/adown_ref.py)
against torch's avg_pool2d / max_pool2d and autograd, tie cases included; the golden module cases against that restatement; an fp32
emulation of the orders csrc/adown.hip documents against the bounds tests/test_gpu_adown.py asserts; the module, the parser, the
YAML, the header and the checkpoints."""
import glob
import os

import pytest
import torch
import torch.nn.functional as F
import yaml

import adown_ref as R
import adown_util as U
from conftest import CFG_DIR, ROOT
from golden.cases import rnd

IDS = [U.case_id(g) for g in U.KERNEL_CASES]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _torch_forward(x):
    """torch's own forward on the NHWC float64 ``x`` -> (x leaf, averaged map, first half, pooled second half, flat arg-max indices)."""
    xt = _nchw(x).clone().requires_grad_(True)
    av = F.avg_pool2d(xt, 2, 1, 0, False, True)
    x1, x2 = av.chunk(2, 1)
    p, idx = F.max_pool2d(x2, 3, 2, 1, return_indices=True)
    return xt, av, x1, p, idx


def _codes(idx, H, W):
    """ATen's flat index into the (H-1) x (W-1) map -> the tap code 3 ky + kx of the window that holds it (NHWC)."""
    oy, ox = torch.arange(H // 2).view(1, 1, -1, 1), torch.arange(W // 2).view(1, 1, 1, -1)
    iy, ix = idx // (W - 1), idx % (W - 1)
    return _nhwc(3 * (iy - (2 * oy - 1)) + (ix - (2 * ox - 1))).to(torch.uint8)


# ----------------------------------------------------------------------------- the restatement against torch
@pytest.mark.parametrize("geom", U.KERNEL_CASES, ids=IDS)
@pytest.mark.parametrize("kind", ["exact", "tie"])
def test_restatement_equals_torch_on_the_exact_grids(geom, kind):
    """On both grids every average is an fp16 number (asserted), so the rounding inside the restatement is the identity and a, p, the
    arg-max (ATen's index, ties included) and the gradient through both halves must EQUAL torch's in float64."""
    N, H, W, C = geom
    x, da, dp = U.exact_inputs(geom, 1) if kind == "exact" else U.tie_inputs(geom)
    f = R.forward(x)
    xt, av, x1, p, idx = _torch_forward(x)
    assert torch.equal(av.detach().half().double(), av.detach())
    xh = _nchw(x).half()
    assert torch.equal(F.avg_pool2d(xh.float(), 2, 1, 0, False, True).half().double(), av.detach())  # fp32 / fp16 agree with float64
    assert torch.equal(_nhwc(x1.detach()), f["a"][:, :H - 1, :W - 1])
    assert float(f["a"][:, H - 1:].abs().sum()) == 0 and float(f["a"][:, :, W - 1:].abs().sum()) == 0
    assert f["a"].shape == (N, 2 * (H // 2), 2 * (W // 2), C // 2)
    assert torch.equal(_nhwc(p.detach()), f["p"])
    assert torch.equal(_codes(idx, H, W), f["arg"])
    ((x1 * _nchw(da[:, :H - 1, :W - 1])).sum() + (p * _nchw(dp)).sum()).backward()
    b = R.backward(da, dp, f["arg"], H, W)
    assert torch.equal(_nhwc(xt.grad), b["dx"])  # (every sum is exact in float64 on these grids)


@pytest.mark.parametrize("geom", U.TIE_CASES, ids=[U.case_id(g) for g in U.TIE_CASES])
def test_the_tie_inputs_tie(geom):
    f = R.forward(U.tie_inputs(geom)[0])
    print(geom, f"windows with a tied maximum: {100 * f['ties']:.1f} %")
    assert f["ties"] >= 0.10


def test_all_zero_map_sends_its_gradients_to_the_first_tap():
    """The rule by the example ATen gives: an all-zero 4x4 averaged map sends its four window gradients to (0,0), (0,1), (1,0), (1,1)."""
    z = torch.zeros(1, 1, 4, 4, dtype=torch.float64, requires_grad=True)
    F.max_pool2d(z, 3, 2, 1).sum().backward()
    assert sorted((int(i), int(j)) for _, _, i, j in z.grad.nonzero()) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    f = R.forward(torch.zeros(1, 5, 5, 16, dtype=torch.float64))
    assert f["arg"][0, :, :, 0].tolist() == [[4, 3], [1, 0]]  # windows (0,0), (0,1), (1,0), (1,1): taps (1,1), (1,0), (0,1), (0,0)


@pytest.mark.parametrize("geom", U.KERNEL_CASES, ids=IDS)
def test_restatement_vs_autograd_on_normal_inputs(geom):
    """Normal inputs: the restatement WITHOUT its fp16 rounding is torch's float64 forward; with it, the backward on its own arg-max
    is autograd's through a max over the rounded averages."""
    N, H, W, C = geom
    x, da, dp = U.normal_inputs(geom, 2)
    f = R.forward(x, round16=False)
    xt, av, x1, p, idx = _torch_forward(x)
    assert float((_nhwc(x1.detach()) - f["a"][:, :H - 1, :W - 1]).abs().max()) < 1e-15
    assert float((_nhwc(p.detach()) - f["p"]).abs().max()) < 1e-15
    assert torch.equal(_codes(idx, H, W), f["arg"])
    ((x1 * _nchw(da[:, :H - 1, :W - 1])).sum() + (p * _nchw(dp)).sum()).backward()
    b = R.backward(da, dp, f["arg"], H, W)
    assert float((_nhwc(xt.grad) - b["dx"]).abs().max()) < 1e-13
    assert bool((b["mag"] + 1e-15 >= b["dx"].abs()).all())


# ----------------------------------------------------------------------------- the kernel's orders in fp32 against the GPU bounds
@pytest.mark.parametrize("geom", U.KERNEL_CASES, ids=IDS)
def test_fp32_emulation_of_the_documented_orders_meets_the_bounds(geom):
    """What tests/test_gpu_adown.py asserts of the kernels, asserted here of an fp32 emulation of their summation orders: equality on
    the exact grid, the one-rounding bound of the forward and the counted bound of the backward on normal inputs."""
    N, H, W, C = geom
    x, da, dp = U.exact_inputs(geom, 1)
    f = R.forward(x)
    a, p = U.emulate_forward(x)
    assert torch.equal(a, f["a"]) and torch.equal(p, f["p"])
    b = R.backward(da, dp, f["arg"], H, W)
    assert torch.equal(U.emulate_backward(da, dp, f["arg"], H, W), b["dx"].half().double())
    old = U.exact_inputs(geom, 3)[0]
    assert torch.equal(U.emulate_backward(da, dp, f["arg"], H, W, old=old.numpy()), (b["dx"] + old).half().double())
    x, da, dp = U.normal_inputs(geom, 2)
    f = R.forward(x, round16=False)
    a, p = U.emulate_forward(x)
    U.check("a", a, f["a"], torch.zeros_like(a), 0)
    U.check("p", p, f["p"], torch.zeros_like(p), 0)
    arg = R.forward(x)["arg"]
    b = R.backward(da, dp, arg, H, W)
    k32 = U.backward_k32(C)
    U.check("dx", U.emulate_backward(da, dp, arg, H, W), b["dx"], b["mag"] * k32, 1)
    old = U.normal_inputs(geom, 4)[0]
    U.check("dx (add)", U.emulate_backward(da, dp, arg, H, W, old=old.numpy()), b["dx"] + old, (b["mag"] + old.abs()) * (k32 + 0.5), 1)


# ----------------------------------------------------------------------------- the golden module cases against the restatement
@pytest.mark.parametrize("case", list(U.MODULE_CASES))
def test_golden_module_cases_vs_the_restatement(golden, case):
    """The reference module's stored fp32 output and input gradient against ADown rebuilt from the float64 restatement (R.forward
    without its fp16 rounding, R.backward) around torch's float64 Conv + BatchNorm + SiLU with the same state: 1e-5 (fp32 values)."""
    G = golden("adown")
    c1, c2, H, W = U.MODULE_CASES[case]
    p_ = f"mod/{case}"
    seed = int(G[f"{p_}/seed"])
    sd = {k: v.double() for k, v in U.state(G, p_).items()}
    x, gy = rnd(10 * seed, 2, c1, H, W).double(), rnd(10 * seed + 1, 2, c2, H // 2, W // 2).double()
    f = R.forward(_nhwc(x), round16=False)
    a = _nchw(f["a"][:, :H - 1, :W - 1]).clone().requires_grad_(True)
    p = _nchw(f["p"]).clone().requires_grad_(True)

    def conv_bn(t, name, k, s):
        z = F.conv2d(t, sd[f"{name}.conv.weight"], None, s, k // 2)
        return F.silu(F.batch_norm(z, None, None, sd[f"{name}.bn.weight"], sd[f"{name}.bn.bias"], True, 0.0, 1e-3))

    y = torch.cat((conv_bn(a, "cv1", 3, 2), conv_bn(p, "cv2", 1, 1)), 1)
    y.backward(gy)
    da = torch.zeros(2, 2 * (H // 2), 2 * (W // 2), c1 // 2, dtype=torch.float64)
    da[:, :H - 1, :W - 1] = _nhwc(a.grad)
    gx = _nchw(R.backward(da, _nhwc(p.grad), f["arg"], H, W)["dx"])
    ey, ex = float((y.detach() - G.t(f"{p_}/y")).abs().max()), float((gx - G.t(f"{p_}/gx")).abs().max())
    print(case, f"y {ey:.2e} gx {ex:.2e}")
    assert ey < 1e-5 and ex < 1e-5 * max(1.0, float(G.t(f"{p_}/gx").abs().max()))
    # the bordered even buffer under the 3x3 s2 p1 convolution is the odd map under it, bit for bit
    w = sd["cv1.conv.weight"]
    assert torch.equal(F.conv2d(_nchw(f["a"]), w, None, 2, 1), F.conv2d(_nchw(f["a"][:, :H - 1, :W - 1]), w, None, 2, 1))


# ----------------------------------------------------------------------------- module, parser, YAML
def _model(name=U.MODEL):
    from ultralytics.nn.tasks import DetectionModel
    return DetectionModel(os.path.join(CFG_DIR, name + ".yaml"), ch=3, verbose=False)


def test_module_keys_class_path_and_attributes(golden):
    from ultralytics.nn.extra_modules.block import ADown
    from ultralytics.nn.modules import Conv
    G = golden("adown")
    assert ADown.__module__ == "ultralytics.nn.extra_modules.block"
    m = ADown(32, 64)
    assert m.c == 32 and isinstance(m.cv1, Conv) and isinstance(m.cv2, Conv)
    assert (m.cv1.conv.in_channels, m.cv1.conv.out_channels, m.cv1.conv.kernel_size, m.cv1.conv.stride, m.cv1.conv.padding) == (16, 32, (3, 3), (2, 2), (1, 1))
    assert (m.cv2.conv.in_channels, m.cv2.conv.out_channels, m.cv2.conv.kernel_size, m.cv2.conv.stride, m.cv2.conv.padding) == (16, 32, (1, 1), (1, 1), (0, 0))
    assert m.out_hw(9, 7) == (4, 3)
    for case, (c1, c2, _, _) in U.MODULE_CASES.items():
        want = U.layout(G, f"mod/{case}")
        assert {k: tuple(v.shape) for k, v in ADown(c1, c2).state_dict().items()} == want and list(ADown(c1, c2).state_dict()) == list(want)


@pytest.mark.parametrize("c1,c2", [(24, 32), (32, 40), (12, 32), (8, 16), (16, 8)])
def test_constructor_refuses_by_name(c1, c2):
    from ultralytics.nn.extra_modules.block import ADown
    with pytest.raises(NotImplementedError, match=rf"ADown\(c1={c1}, c2={c2}\) is outside the HIP hot path \(supported: c1 % 16 == 0 and c2 % 16 == 0"):
        ADown(c1, c2)


def _custom(rows, nc=6):
    return {"nc": nc, "scales": {"n": [1.0, 1.0, 1024]}, "scale": "n", "backbone": rows, "head": [[[-1], 1, "Detect", ["nc"]]]}


def test_parser_refuses_by_layer():
    from ultralytics.nn.tasks import DetectionModel
    with pytest.raises(NotImplementedError, match=r"layer 1 \(ADown\)\(c1=24, c2=32\) is outside the HIP hot path"):
        DetectionModel(_custom([[-1, 1, "Conv", [24, 3, 2]], [-1, 1, "ADown", [32]]]), verbose=False)
    with pytest.raises(NotImplementedError, match=r"layer 1 \(ADown\)\(c1=32, c2=40\) is outside the HIP hot path"):
        DetectionModel(_custom([[-1, 1, "Conv", [32, 3, 2]], [-1, 1, "ADown", [40]]]), verbose=False)
    # a 12-channel input can only come from a ``Conv [nc, ...]`` row: the parser names the reader and the width
    with pytest.raises(NotImplementedError, match=r"layer 1 \(ADown\) reads layer 0, which is 12 channels wide"):
        DetectionModel(_custom([[-1, 1, "Conv", ["nc", 3, 2]], [-1, 1, "ADown", [32]]], nc=12), verbose=False)
    m = DetectionModel(_custom([[-1, 1, "Conv", [32, 3, 2]], [-1, 1, "ADown", [48]]]), verbose=False)  # ... and a supported row builds
    assert m._cout[:2] == [32, 48] and m.stride.tolist() == [4.0]


def test_graph_builds_like_the_reference(golden):
    from ultralytics.nn.extra_modules.block import ADown
    G = golden("adown")
    m = _model()
    assert [type(m.model[i]) for i in U.ADOWN_LAYERS] == [ADown] * 5
    assert [(2 * m.model[i].cv1.conv.in_channels, 2 * m.model[i].c) for i in U.ADOWN_LAYERS] == list(U.ADOWN_WIDTHS.values())
    assert sum(q.numel() for q in m.parameters()) == int(G[f"{U.MODEL}/n_params"]) == 894034
    assert m.stride.tolist() == G[f"{U.MODEL}/stride"].tolist() == [4.0, 8.0, 16.0]
    want = U.layout(G, U.MODEL)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want) and got == want
    assert [m._cout[i] for i in U.ADOWN_LAYERS] == [c2 for _, c2 in U.ADOWN_WIDTHS.values()]
    assert all(mod.type == "ultralytics.nn.extra_modules.block.ADown" for mod in (m.model[i] for i in U.ADOWN_LAYERS))
    head = open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2-ADown.yaml")).read().split("nc:")[0]
    flat = " ".join(head.replace("#", " ").split())  # (however the comment wraps)
    assert "project's own reading" in flat and "ship no YAML" in flat
    # the same rows as the dense graph, the five stride-2 rows apart
    a = yaml.safe_load(open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2-ADown.yaml")))
    d = yaml.safe_load(open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2.yaml")))
    for i, (ra, rd) in enumerate(zip(a["backbone"] + a["head"], d["backbone"] + d["head"])):
        if i in U.ADOWN_LAYERS:
            assert ra == [rd[0], rd[1], "ADown", [rd[3][0]]] and rd[2] == "Conv" and rd[3][1:] == [3, 2], i
        else:
            assert ra == rd, i


def test_fuse_folds_both_convs():
    m = _model().eval()
    m.fuse()
    for i in U.ADOWN_LAYERS:
        for cv in (m.model[i].cv1, m.model[i].cv2):
            assert not hasattr(cv, "bn") and cv.conv.bias is not None


def test_other_shipped_yamls_hold_no_adown_row():
    files = sorted(glob.glob(os.path.join(CFG_DIR, "*.yaml")))
    assert len(files) > 5
    with_rows = [os.path.basename(f) for f in files
                 if any(row[2] == "ADown" for row in (lambda d: d["backbone"] + d["head"])(yaml.safe_load(open(f))))]
    assert with_rows == ["yolov8-ASF-P2P2-ADown.yaml"]


def test_freeze_names_cover_both_convs():
    from ultralytics.engine.trainer import frozen_parameter_names
    names = [k for k, _ in _model().named_parameters()]
    frozen = set(frozen_parameter_names(names, 4))
    assert {"model.1.cv1.conv.weight", "model.1.cv2.bn.bias", "model.3.cv2.conv.weight"} <= frozen and "model.5.cv1.conv.weight" not in frozen


# ----------------------------------------------------------------------------- header and binding
def test_header_declares_and_the_library_binds_the_entry_points():
    import ctypes as C
    from ultralytics.hip import SIGNATURES, lib
    txt = open(os.path.join(ROOT, "include", "dealyolo_hip.h")).read()
    for name, nargs in (("dy_adown_pool", 12), ("dy_adown_pool_backward", 13)):
        assert f"int {name}(" in txt
        res, args = SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
        assert getattr(lib(), name).argtypes == list(args)
    assert "block.py:4685-4698" in txt  # the reference lines the entries replace
    L = lib()
    # refusals need no device: nothing is launched (host numbers stand in for pointers)
    ARG, ALIGN = -1, -3
    base = dict(x=4096, ldx=32, a=8192, lda=16, p=16384, ldp=16, arg=32768, n=1, H=4, W=4, C=32)

    def fwd(**kw):
        v = dict(base, **kw)
        return L.dy_adown_pool(v["x"], v["ldx"], v["a"], v["lda"], v["p"], v["ldp"], v["arg"], v["n"], v["H"], v["W"], v["C"], None)

    def bwd(**kw):
        v = dict(base, **kw)  # (a, p stand for da, dp; x for dx)
        return L.dy_adown_pool_backward(v["a"], v["lda"], v["p"], v["ldp"], v["arg"], v["x"], v["ldx"], 0, v["n"], v["H"], v["W"], v["C"], None)

    for f in (fwd, bwd):
        assert f(x=0) == ARG and f(a=0) == ARG and f(p=0) == ARG and f(n=0) == ARG and f(H=1) == ARG and f(W=1) == ARG
        assert f(ldx=24) == ARG and f(lda=8) == ARG and f(ldp=8) == ARG                                  # pitches below the width
        assert f(C=24) == ALIGN and f(C=8) == ALIGN and f(ldx=36) == ALIGN and f(lda=20) == ALIGN and f(ldp=20) == ALIGN
        assert f(x=4104) == ALIGN and f(a=8200) == ALIGN and f(p=16392) == ALIGN and f(arg=32776) == ALIGN
    assert bwd(arg=0) == ARG  # (the forward takes a null arg-max: inference)


# ----------------------------------------------------------------------------- checkpoints
def test_reference_written_checkpoint_rebuilds(golden):
    """tests/golden/ref_ckpt_adown.pt: a whole-module fp16 pickle written by the REFERENCE's classes; its module path
    ultralytics.nn.extra_modules.block.ADown resolves to this package's class."""
    from ultralytics.nn.extra_modules.block import ADown
    from ultralytics.nn.tasks import DetectionModel, _rebuild, attempt_load_weights, torch_safe_load
    G = golden("adown")
    ckpt, _ = torch_safe_load(U.CKPT)
    obj = ckpt["model"]
    assert [type(obj.model[i]) for i in U.ADOWN_LAYERS] == [ADown] * 5
    assert sum(1 for row in obj.yaml["backbone"] + obj.yaml["head"] if row[2] == "ADown") == 5
    m = _rebuild(obj, ckpt)
    assert isinstance(m, DetectionModel)
    assert [2 * m.model[i].cv1.conv.in_channels for i in U.ADOWN_LAYERS] == G["ckpt/adown_channels"].tolist() == [16, 32, 32, 32, 32]
    want = U.state(G, "ckpt")
    got = m.state_dict()
    assert list(want) == list(got)
    for k, v in want.items():
        assert torch.equal(got[k].float(), (v.half().float() if v.is_floating_point() else v.float())), k
    assert not attempt_load_weights(U.CKPT).training


def test_checkpoint_roundtrip_in_the_reference_format(tmp_path):
    from ultralytics.nn.extra_modules.block import ADown
    from ultralytics.nn.tasks import attempt_load_weights, save_reference_format, torch_safe_load
    m = _model()
    path = save_reference_format(str(tmp_path / "last.pt"), m, updates=4, epoch=1, train_args={"imgsz": 64})
    obj = torch_safe_load(path)[0]["model"]
    assert next(obj.parameters()).dtype == torch.float16 and all("rt" not in mod.__dict__ for mod in obj.modules())
    assert [type(obj.model[i]) for i in U.ADOWN_LAYERS] == [ADown] * 5
    back = attempt_load_weights(path)
    for (k, a), (_, b) in zip(m.state_dict().items(), back.state_dict().items()):
        assert torch.equal(a.half().float() if a.is_floating_point() else a, b.float() if a.is_floating_point() else b), k
