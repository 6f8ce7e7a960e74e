"""CPU: DySample (learned dynamic up-sampling, reference nn/extra_modules/block.py:3819-3892) without a GPU -- the float64
restatement of tests/dysample_ref.py against the reference's autograd values (tests/golden/dysample_kernel.npz, dysample_big_*.npz:
1e-11), the init_pos formula against the reference's buffer, the new graph's layout and parameter count against the reference's
DetectionModel on this package's YAML, the refusals of what the HIP path does not take, the bound entry points, and the layouts of
the graphs that existed before."""
import os

import pytest
import torch

import dysample_ref as R
from conftest import CFG_DIR, ROOT
from dysample_util import (BIG, BOUNDED_CASES, CKPT, DYSAMPLE_LAYERS, GROUPS, KERNEL_CASES, MODEL, MODULE_CASES, ZERO_CASE, dysample_state,
                           fetch, init_pos, kernel_inputs, layout, state)
from golden.cases import rnd

ALL_MODULE_CASES = {**MODULE_CASES, ZERO_CASE: MODULE_CASES["ds_32_s2"]}


def _maxerr(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max())


def kernel_case(G, name):
    """Inputs of a kernel case (drawn again from the stored seed; equal to the stored ones where they are stored)."""
    C, s, H, W = {**KERNEL_CASES, **BOUNDED_CASES}[name]
    x, off, dy = kernel_inputs(C, s, H, W, int(G[f"ker/{name}/seed"]), bounded=name in BOUNDED_CASES)
    if f"ker/{name}/x" in G:
        assert torch.equal(x.float(), G.t(f"ker/{name}/x")) and torch.equal(off, G.t(f"ker/{name}/off")) and torch.equal(dy.float(), G.t(f"ker/{name}/dy"))
    return x, off, dy, s


# ----------------------------------------------------------------------------- the restatement against the reference's autograd
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_restatement_vs_kernel_golden(golden, name):
    G = golden("dysample_kernel")
    x, off, dy, s = kernel_case(G, name)
    fw, bw = R.forward(x, off, s, GROUPS), R.backward(x, off, dy, s, GROUPS)
    errs = dict(y=_maxerr(fw["y"], fetch(G, f"ker/{name}/y")), dx=_maxerr(bw["dx"], fetch(G, f"ker/{name}/dx")),
                doff=_maxerr(bw["doff"], fetch(G, f"ker/{name}/doff")))
    print(name, errs)
    assert max(errs.values()) < 1e-11
    # the magnitudes bound the values they belong to, and the term count the dx bound is counted for holds
    assert bool((fw["mag"] >= fw["y"].abs() - 1e-12).all()) and bool((bw["dx_mag"] >= bw["dx"].abs() - 1e-12).all())
    assert bool((bw["doff_mag"] >= bw["doff"].abs() - 1e-12).all())
    assert int(bw["dx_terms"].max()) == int(G[f"ker/{name}/dx_terms_max"]) <= 120


@pytest.mark.parametrize("name", list(ALL_MODULE_CASES))
def test_restatement_vs_module_golden(golden, name):
    """Offset convolution + sampler + both backward halves in float64 against the reference module run in float64."""
    G, G64 = golden("dysample"), golden("dysample_kernel")
    C, s, H, W = ALL_MODULE_CASES[name]
    p, q = f"mod/{name}", f"mod64/{name}"
    seed = int(G[f"{p}/seed"])
    x, gy = rnd(10 * seed, 2, C, H, W), rnd(10 * seed + 1, 2, C, s * H, s * W)
    if f"{p}/x" in G:
        assert torch.equal(x, G.t(f"{p}/x")) and torch.equal(gy, G.t(f"{p}/gy"))
    sd = state(G, p)
    w, b = sd["offset.weight"].double().reshape(-1, C), sd["offset.bias"].double()
    xh = R.nhwc(x.double())
    off = R.offset_conv(xh, w, b)
    if name == ZERO_CASE:
        assert float(off.abs().max()) == 0.0
    fw, bw = R.forward(xh, off, s, GROUPS), R.backward(xh, off, R.nhwc(gy.double()), s, GROUPS)
    doff = bw["doff"].reshape(-1, off.shape[-1])
    gx = R.nchw(bw["dx"] + bw["doff"] @ w)
    errs = dict(gx=_maxerr(gx, fetch(G64, f"{q}/gx")), gw=_maxerr((doff.t() @ xh.reshape(-1, C)).reshape(G64[f"{q}/gw"].shape), G64.t(f"{q}/gw")),
                gb=_maxerr(doff.sum(0), G64.t(f"{q}/gb")))
    if not name.endswith(BIG):
        errs["y"] = _maxerr(R.nchw(fw["y"]), G64.t(f"{q}/y"))
    print(name, errs)
    assert max(errs.values()) < 1e-11
    # and the fp32 run the GPU tests compare with is that float64 run up to fp32 rounding (isolated kink flips: Frobenius)
    y32 = fetch(G, f"{p}/y")
    assert float((R.nchw(fw["y"]) - y32.double()).norm() / y32.double().norm()) < 1e-5


# ----------------------------------------------------------------------------- init_pos
@pytest.mark.parametrize("name", list(ALL_MODULE_CASES))
def test_init_pos_formula_vs_the_reference_buffer(golden, name):
    from ultralytics.nn.extra_modules import DySample
    G = golden("dysample")
    C, s, _, _ = ALL_MODULE_CASES[name]
    ref = G.t(f"mod/{name}/init_pos")
    assert torch.equal(init_pos(s, GROUPS), ref)
    assert torch.equal(R.init_pos(s, GROUPS).float().view(1, -1, 1, 1), ref)
    assert torch.equal(DySample(C, s).init_pos, ref)
    t = {2: [-0.25, 0.25], 4: [-0.375, -0.125, 0.125, 0.375]}[s]
    n = GROUPS * s * s
    for g in range(GROUPS):
        for i in range(s):
            for j in range(s):
                assert float(ref[0, g * s * s + i * s + j]) == t[j] and float(ref[0, n + g * s * s + i * s + j]) == t[i]


# ----------------------------------------------------------------------------- module, parser, graph
def _model(name=MODEL):
    from ultralytics.nn.tasks import DetectionModel
    return DetectionModel(os.path.join(CFG_DIR, name + ".yaml"), ch=3, verbose=False)


def test_module_keys_init_and_class_path():
    import ultralytics.nn.extra_modules as X
    import ultralytics.nn.extra_modules.block as B
    assert "DySample" in X.__all__ and "DySample" in B.__all__ and X.DySample is B.DySample
    assert B.DySample.__module__ == "ultralytics.nn.extra_modules.block"
    torch.manual_seed(0)
    m = B.DySample(64, 2, "lp", 4)
    assert list(m.state_dict()) == ["init_pos", "offset.weight", "offset.bias"]
    assert tuple(m.offset.weight.shape) == (32, 64, 1, 1) and tuple(m.init_pos.shape) == (1, 32, 1, 1)
    assert [k for k, _ in m.named_parameters()] == ["offset.weight", "offset.bias"]
    assert float(m.offset.bias.detach().abs().max()) == 0.0 and 5e-4 < float(m.offset.weight.detach().std()) < 2e-3  # normal, std 0.001
    assert (m.scale, m.style, m.groups) == (2, "lp", 4) and m.out_hw(5, 7) == (10, 14)
    assert tuple(B.DySample(32, 4).offset.weight.shape) == (128, 32, 1, 1)


def test_graph_builds_like_the_reference(golden):
    from ultralytics.nn.extra_modules import DySample
    G = golden("dysample")
    m = _model()
    want = layout(G, MODEL)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want) and got == want
    assert sum(p.numel() for p in m.parameters()) == int(G[f"{MODEL}/n_params"])
    assert m.stride.tolist() == [4.0, 8.0, 16.0] == G[f"{MODEL}/stride"].tolist()
    assert [i for i, mod in enumerate(m.model) if isinstance(mod, DySample)] == list(DYSAMPLE_LAYERS)
    assert [m.model[i].offset.in_channels for i in DYSAMPLE_LAYERS] == [64, 32]  # scale n
    assert all(m.model[i].type == "ultralytics.nn.extra_modules.block.DySample" for i in DYSAMPLE_LAYERS)
    assert [m._cout[i] for i in DYSAMPLE_LAYERS] == [64, 32]
    base = _model("yolov8n-ASF-P2P2")  # two layers of a few thousand parameters on top of DEAL-YOLO-N
    extra = sum(p.numel() for p in m.parameters()) - sum(p.numel() for p in base.parameters())
    assert extra == (64 * 32 + 32) + (32 * 32 + 32)
    m.load_state_dict(state(G, MODEL), strict=True)


def test_optimizer_groups_of_the_offset_convolution():
    """offset.weight goes with the decayed weights and offset.bias with the biases (reference build_optimizer: 'bias' in the name ->
    g[2], a norm layer's weight -> g[1], else g[0]); hip/runtime.py sorts by the same rule."""
    import torch.nn as nn
    m = _model()
    norm = tuple(v for k, v in nn.__dict__.items() if "Norm" in k and isinstance(v, type))
    for i in DYSAMPLE_LAYERS:
        mod = m.model[i]
        assert not isinstance(mod.offset, norm)
        names = [f"model.{i}.offset.weight", f"model.{i}.offset.bias"]
        assert [n for n, _ in m.named_parameters() if n.startswith(f"model.{i}.")] == names
        assert ["bias" in n for n in names] == [False, True]
    assert "model.9.init_pos" in dict(m.named_buffers())


@pytest.mark.parametrize("row,what", [([2, "pl"], "style"), ([2, "lp", 4, True], "dyscope"), ([3, "lp"], "scale")])
def test_unsupported_arguments_raise(row, what):
    import yaml
    d = yaml.safe_load(open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2-DySample.yaml")))
    d["head"][1][3] = row
    d["scale"] = "n"
    from ultralytics.nn.tasks import DetectionModel
    with pytest.raises(NotImplementedError, match="supported"):
        DetectionModel(d, ch=3, verbose=False)


def test_layer_on_24_channels_raises():
    import yaml
    from ultralytics.nn.tasks import DetectionModel
    d = yaml.safe_load(open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2-DySample.yaml")))
    d["head"][0][3] = [96, 1, 1]  # layer 8 at scale n: 24 channels in front of the DySample of layer 9
    d["scale"] = "n"
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        DetectionModel(d, ch=3, verbose=False)
    from ultralytics.nn.extra_modules import DySample
    with pytest.raises(NotImplementedError, match="in_channels=24"):
        DySample(24)


def test_dynamic_scalseq_stays_outside():
    import yaml
    from ultralytics.nn.tasks import DetectionModel
    d = yaml.safe_load(open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2-DySample.yaml")))
    d["head"][16][2] = "DynamicScalSeq"
    d["scale"] = "n"
    with pytest.raises(NotImplementedError, match="'DynamicScalSeq' is outside the DEAL-YOLO hot path"):
        DetectionModel(d, ch=3, verbose=False)


@pytest.mark.parametrize("name", ["yolov8n-ASF-P2P2", "yolov8n-ASF-P2", "yolov8n-ASF", "yolov8n-LD-P2", "yolov8n-p2"])
def test_existing_graphs_keep_their_layouts(name):
    from oracle import graph as og
    want = og.state_layout(og.build_graph(og.load_yaml(os.path.join(CFG_DIR, name + ".yaml"))))
    got = {k: tuple(v.shape) for k, v in _model(name).state_dict().items()}
    assert list(got) == list(want) and got == {k: tuple(v) for k, v in want.items()}


@pytest.mark.parametrize("name", ["yolov8n-ASF-P2P2-SPD", "yolov8n-LD-P2-SPD"])
def test_existing_spd_graphs_keep_their_layouts(golden, name):
    from spd_util import layout as spd_layout
    want = spd_layout(golden("spd"), name)
    got = {k: tuple(v.shape) for k, v in _model(name).state_dict().items()}
    assert list(got) == list(want) and got == want


# ----------------------------------------------------------------------------- checkpoints
def test_reference_written_checkpoint_rebuilds(golden):
    """tests/golden/ref_ckpt_dysample.pt: a whole-module fp16 pickle written by the REFERENCE's classes; its module path
    ultralytics.nn.extra_modules.block.DySample resolves to this package's class."""
    from ultralytics.nn.extra_modules import DySample
    from ultralytics.nn.tasks import DetectionModel, _rebuild, attempt_load_weights, torch_safe_load
    ckpt, _ = torch_safe_load(CKPT)
    obj = ckpt["model"]
    assert [type(obj.model[i]) for i in DYSAMPLE_LAYERS] == [DySample] * 2
    assert sum(1 for row in obj.yaml["backbone"] + obj.yaml["head"] if row[2] == "DySample") == 2
    m = _rebuild(obj, ckpt)
    assert isinstance(m, DetectionModel)
    want = state(golden("dysample"), "ckpt")
    got = m.state_dict()
    assert list(want) == list(got)
    for k, v in want.items():
        assert torch.equal(got[k].float(), (v.half().float() if v.is_floating_point() else v.float())), k
    assert not attempt_load_weights(CKPT).training


def test_checkpoint_roundtrip_in_the_reference_format(tmp_path):
    from ultralytics.nn.extra_modules import DySample
    from ultralytics.nn.tasks import attempt_load_weights, save_reference_format, torch_safe_load
    m = _model()
    path = save_reference_format(str(tmp_path / "last.pt"), m, updates=4, epoch=1, train_args={"imgsz": 64})
    obj = torch_safe_load(path)[0]["model"]
    assert next(obj.parameters()).dtype == torch.float16 and all("rt" not in mod.__dict__ for mod in obj.modules())
    assert [type(obj.model[i]) for i in DYSAMPLE_LAYERS] == [DySample] * 2
    back = attempt_load_weights(path)
    for (k, a), (_, b) in zip(m.state_dict().items(), back.state_dict().items()):
        assert torch.equal(a.half().float() if a.is_floating_point() else a, b.float() if a.is_floating_point() else b), k


# ----------------------------------------------------------------------------- header and binding
def test_header_declares_and_the_library_binds_the_entry_points():
    import ctypes as C
    from ultralytics.hip import SIGNATURES, lib
    txt = open(os.path.join(ROOT, "include", "dealyolo_hip.h")).read()
    for name, nargs in (("dy_dysample_supported", 3), ("dy_dysample", 13), ("dy_dysample_backward", 21)):
        assert f"int {name}(" in txt
        res, args = SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
        assert getattr(lib(), name).argtypes == list(args)
    assert "block.py:3856-3879" in txt  # the reference lines the entries replace
    L = lib()
    ok = [(32, 4, 2), (64, 4, 2), (32, 4, 4), (64, 1, 2), (96, 4, 2), (8, 1, 4)]
    bad = [(24, 4, 2), (32, 4, 3), (32, 4, 1), (32, 0, 2), (36, 4, 2), (16, 4, 2), (0, 1, 2), (32, 4, 8)]
    assert all(L.dy_dysample_supported(*a) == 1 for a in ok) and all(L.dy_dysample_supported(*a) == 0 for a in bad)
    # refusals need no device: nothing is launched
    DY_ERR_ARG, DY_ERR_ALIGN = -1, -3
    base = dict(x=4096, ldx=32, off=8192, ldoff=32, y=16384, ldy=32, n=1, H=4, W=4, C=32, G=4, s=2)

    def rc(**kw):
        a = dict(base, **kw)
        return L.dy_dysample(a["x"], a["ldx"], a["off"], a["ldoff"], a["y"], a["ldy"], a["n"], a["H"], a["W"], a["C"], a["G"], a["s"], None)

    assert rc(s=3) == DY_ERR_ARG and rc(C=24, ldx=24, ldy=24) == DY_ERR_ARG and rc(x=0) == DY_ERR_ARG and rc(off=0) == DY_ERR_ARG
    assert rc(y=0) == DY_ERR_ARG and rc(ldoff=16) == DY_ERR_ARG and rc(ldx=24) == DY_ERR_ARG
    assert rc(ldx=36) == DY_ERR_ALIGN and rc(ldy=34) == DY_ERR_ALIGN and rc(x=4104) == DY_ERR_ALIGN and rc(y=16392) == DY_ERR_ALIGN
