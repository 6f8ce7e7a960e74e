"""CPU: CARAFE (content-aware up-sampling, reference nn/extra_modules/block.py:3898-3936) without a GPU -- the float64 restatement
of tests/carafe_ref.py against the reference's own float64 values (tests/golden/carafe_kernel.npz, carafe_big_*.npz: 1e-11 on
every element, forward and both gradients), the new graph's layout, parameter count and strides against the reference's
DetectionModel on this package's YAML, the module's keys and class path, the refusals of what the HIP path does not take, the bound
entry points, and a reference-written checkpoint."""
import os

import pytest
import torch

import carafe_ref as R
from carafe_util import CARAFE_LAYERS, CKPT, KERNEL_CASES, MODEL, fetch, kernel_inputs, layout, state
from conftest import CFG_DIR, ROOT


def _maxerr(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max())


# ----------------------------------------------------------------------------- the restatement against the reference's autograd
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_restatement_vs_kernel_golden(golden, name):
    G = golden("carafe_kernel")
    C, H, W, gain = KERNEL_CASES[name]
    x, lg, dy = kernel_inputs(C, H, W, int(G[f"ker/{name}/seed"]), gain)
    fw, bw = R.forward(x, lg), R.backward(x, lg, dy)
    errs = dict(y=_maxerr(fw["y"], fetch(G, f"ker/{name}/y")), dx=_maxerr(bw["dx"], fetch(G, f"ker/{name}/dx")),
                dlogits=_maxerr(bw["dlogits"], fetch(G, f"ker/{name}/dlogits")))
    print(name, errs)
    assert max(errs.values()) < 1e-11
    # the magnitudes bound the values they belong to
    assert bool((fw["mag"] >= fw["y"].abs() - 1e-12).all()) and bool((bw["dx_mag"] >= bw["dx"].abs() - 1e-12).all())
    assert bool((bw["dlogits_mag"] >= bw["dlogits"].abs() - 1e-12).all())


def test_the_hot_case_needs_the_stable_softmax(golden):
    """|logit| reaches about 200 there: exp of it overflows fp32 (and fp64's softmax without the maximum would too), weights near one-hot."""
    C, H, W, gain = KERNEL_CASES["k_32_hot"]
    _, lg, _ = kernel_inputs(C, H, W, int(golden("carafe_kernel")["ker/k_32_hot/seed"]), gain)
    assert float(lg.abs().max()) > 150 and float(R.weights(lg).max()) > 0.999999
    assert not bool(torch.isfinite(torch.exp(lg.float())).all())


# ----------------------------------------------------------------------------- module, parser, graph
def _model(name=MODEL):
    from ultralytics.nn.tasks import DetectionModel
    return DetectionModel(os.path.join(CFG_DIR, name + ".yaml"), ch=3, verbose=False)


def test_module_keys_and_class_path():
    import ultralytics.nn.extra_modules as X
    import ultralytics.nn.extra_modules.block as B
    from ultralytics.nn.modules import Conv
    assert "CARAFE" in X.__all__ and "CARAFE" in B.__all__ and X.CARAFE is B.CARAFE
    assert B.CARAFE.__module__ == "ultralytics.nn.extra_modules.block"
    m = B.CARAFE(64)
    keys = [f"{c}.{k}" for c in ("comp", "enc") for k in ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var",
                                                          "bn.num_batches_tracked")]
    assert list(m.state_dict()) == keys and not [k for k, _ in m.named_buffers() if ".bn." not in k]
    assert isinstance(m.comp, Conv) and isinstance(m.enc, Conv)
    assert tuple(m.comp.conv.weight.shape) == (64, 64, 1, 1) and tuple(m.enc.conv.weight.shape) == (100, 64, 3, 3)
    assert isinstance(m.enc.act, torch.nn.Identity) and isinstance(m.comp.act, torch.nn.SiLU)
    assert m.out_hw(5, 7) == (10, 14)
    assert tuple(B.CARAFE(32, 1, 5, 16).enc.conv.weight.shape) == (100, 16, 1, 1)


def test_graph_builds_like_the_reference(golden):
    G = golden("carafe")
    m = _model()  # (before this layer existed: "module 'CARAFE' is outside the DEAL-YOLO hot path")
    from ultralytics.nn.extra_modules import CARAFE
    want = layout(G, MODEL)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want) and got == want
    assert sum(p.numel() for p in m.parameters()) == int(G[f"{MODEL}/n_params"]) == 1028002
    assert m.stride.tolist() == [4.0, 8.0, 16.0] == G[f"{MODEL}/stride"].tolist()
    assert [i for i, mod in enumerate(m.model) if isinstance(mod, CARAFE)] == list(CARAFE_LAYERS)
    assert [m.model[i].comp.conv.in_channels for i in CARAFE_LAYERS] == [64, 32]  # scale n
    assert [m.model[i].comp.conv.out_channels for i in CARAFE_LAYERS] == [16, 16]
    assert [m.model[i].enc.conv.out_channels for i in CARAFE_LAYERS] == [100, 100]
    assert all(m.model[i].type == "ultralytics.nn.extra_modules.block.CARAFE" for i in CARAFE_LAYERS)
    assert [m._cout[i] for i in CARAFE_LAYERS] == [64, 32]
    m.load_state_dict(state(G, MODEL), strict=True)


def test_module_defaults_build_the_reference_parameter_count(golden):
    import yaml
    from ultralytics.nn.tasks import DetectionModel
    d = yaml.safe_load(open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2-CARAFE.yaml")))
    d["scale"] = "n"
    for row in d["head"]:
        if row[2] == "CARAFE":
            row[3] = []
    n = sum(p.numel() for p in DetectionModel(d, ch=3, verbose=False).parameters())
    assert n == int(golden("carafe")[f"{MODEL}/n_params_default_args"]) == 1119202


@pytest.mark.parametrize("kw,what", [(dict(c=32, k_up=3), "k_up=3"), (dict(c=32, scale=4), "scale=4"), (dict(c=12), "c=12")])
def test_unsupported_arguments_raise(kw, what):
    from ultralytics.nn.extra_modules import CARAFE
    with pytest.raises(NotImplementedError, match="supported: k_up=5, scale=2") as e:
        CARAFE(**kw)
    assert what in str(e.value)


def test_unsupported_row_raises_in_the_parser():
    import yaml
    from ultralytics.nn.tasks import DetectionModel
    d = yaml.safe_load(open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2-CARAFE.yaml")))
    d["head"][1][3] = [3, 7, 16]
    d["scale"] = "n"
    with pytest.raises(NotImplementedError, match="k_up=7"):
        DetectionModel(d, ch=3, verbose=False)


# ----------------------------------------------------------------------------- checkpoints
def test_reference_written_checkpoint_rebuilds(golden):
    """tests/golden/ref_ckpt_carafe.pt: a whole-module fp16 pickle written by the REFERENCE's classes; its module path
    ultralytics.nn.extra_modules.block.CARAFE resolves to this package's class."""
    from ultralytics.nn.extra_modules import CARAFE
    from ultralytics.nn.tasks import DetectionModel, _rebuild, attempt_load_weights, torch_safe_load
    G = golden("carafe")
    ckpt, _ = torch_safe_load(CKPT)
    obj = ckpt["model"]
    assert [type(obj.model[i]) for i in CARAFE_LAYERS] == [CARAFE] * 2
    assert sum(1 for row in obj.yaml["backbone"] + obj.yaml["head"] if row[2] == "CARAFE") == 2
    m = _rebuild(obj, ckpt)
    assert isinstance(m, DetectionModel)
    assert [m.model[i].comp.conv.in_channels for i in CARAFE_LAYERS] == G["ckpt/carafe_channels"].tolist() == [32, 16]
    want = state(G, "ckpt")
    got = m.state_dict()
    assert list(want) == list(got)
    for k, v in want.items():
        assert torch.equal(got[k].float(), (v.half().float() if v.is_floating_point() else v.float())), k
    assert not attempt_load_weights(CKPT).training


def test_checkpoint_roundtrip_in_the_reference_format(tmp_path):
    from ultralytics.nn.extra_modules import CARAFE
    from ultralytics.nn.tasks import attempt_load_weights, save_reference_format, torch_safe_load
    m = _model()
    path = save_reference_format(str(tmp_path / "last.pt"), m, updates=4, epoch=1, train_args={"imgsz": 64})
    obj = torch_safe_load(path)[0]["model"]
    assert next(obj.parameters()).dtype == torch.float16 and all("rt" not in mod.__dict__ for mod in obj.modules())
    assert [type(obj.model[i]) for i in CARAFE_LAYERS] == [CARAFE] * 2
    back = attempt_load_weights(path)
    for (k, a), (_, b) in zip(m.state_dict().items(), back.state_dict().items()):
        assert torch.equal(a.half().float() if a.is_floating_point() else a, b.float() if a.is_floating_point() else b), k


# ----------------------------------------------------------------------------- header and binding
def test_header_declares_and_the_library_binds_the_entry_points():
    import ctypes as C
    from ultralytics.hip import SIGNATURES, lib
    txt = open(os.path.join(ROOT, "include", "dealyolo_hip.h")).read()
    for name, nargs in (("dy_carafe_supported", 3), ("dy_carafe", 11), ("dy_carafe_backward", 16)):
        assert f"int {name}(" in txt
        res, args = SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
        assert getattr(lib(), name).argtypes == list(args)
    assert "block.py:3926-3935" in txt  # the reference lines the entries replace
    L = lib()
    ok = [(8, 5, 2), (32, 5, 2), (64, 5, 2), (72, 5, 2), (256, 5, 2)]
    bad = [(12, 5, 2), (0, 5, 2), (4, 5, 2), (32, 3, 2), (32, 5, 4), (32, 7, 2), (-8, 5, 2)]
    assert all(L.dy_carafe_supported(*a) == 1 for a in ok) and all(L.dy_carafe_supported(*a) == 0 for a in bad)
    # refusals need no device: nothing is launched
    DY_ERR_ARG, DY_ERR_ALIGN = -1, -3
    base = dict(x=4096, ldx=32, lg=8192, ldl=104, y=16384, ldy=32, n=1, H=4, W=4, C=32)

    def rc(**kw):
        a = dict(base, **kw)
        return L.dy_carafe(a["x"], a["ldx"], a["lg"], a["ldl"], a["y"], a["ldy"], a["n"], a["H"], a["W"], a["C"], None)

    def rcb(dx=32768, lddx=32, dl=65536, lddl=104, **kw):
        a = dict(base, **kw)
        return L.dy_carafe_backward(a["x"], a["ldx"], a["lg"], a["ldl"], a["y"], a["ldy"], dx, lddx, 0, dl, lddl, a["n"], a["H"], a["W"],
                                    a["C"], None)

    assert rc(C=12, ldx=16, ldy=16) == DY_ERR_ARG and rc(x=0) == DY_ERR_ARG and rc(lg=0) == DY_ERR_ARG and rc(y=0) == DY_ERR_ARG
    assert rc(H=0) == DY_ERR_ARG and rc(W=0) == DY_ERR_ARG and rc(n=0) == DY_ERR_ARG
    assert rc(ldl=96) == DY_ERR_ARG and rc(ldx=24) == DY_ERR_ARG and rc(ldy=24) == DY_ERR_ARG        # pitches below the width
    assert rc(ldl=100) == DY_ERR_ALIGN and rc(ldx=36) == DY_ERR_ALIGN and rc(ldy=34) == DY_ERR_ALIGN  # pitches off the granule
    assert rc(x=4104) == DY_ERR_ALIGN and rc(y=16392) == DY_ERR_ALIGN and rc(lg=8200) == DY_ERR_ALIGN
    assert rc(n=1 << 15, H=1 << 8, W=1 << 7) == DY_ERR_ARG  # 4 n H W = 2^32
    assert rcb(dl=0) == DY_ERR_ARG and rcb(C=12, ldx=16, ldy=16) == DY_ERR_ARG and rcb(lddl=96) == DY_ERR_ARG and rcb(lddx=24) == DY_ERR_ARG
    assert rcb(lddl=100) == DY_ERR_ALIGN and rcb(dl=65544) == DY_ERR_ALIGN and rcb(dx=32776) == DY_ERR_ALIGN and rcb(lddx=36) == DY_ERR_ALIGN
