"""CPU: SPDConv (space-to-depth convolution, reference nn/extra_modules/block.py:2497-2507) in the model plumbing -- the two SPD
graphs build on a host without a GPU with the reference's parameter counts, strides and state_dict layout (tests/golden/spd.npz,
taken from the reference's own DetectionModel on this package's YAML files), a reference-written SPD checkpoint rebuilds, and the
kernel's entry point is bound."""
import os

import pytest
import torch

from conftest import CFG_DIR
from spd_util import CKPT, MODELS, N_PARAMS, SPD_LAYERS, layout


def _model(name):
    from ultralytics.nn.tasks import DetectionModel
    return DetectionModel(os.path.join(CFG_DIR, name + ".yaml"), ch=3, verbose=False)


@pytest.mark.parametrize("name", MODELS)
def test_spd_graphs_build_like_the_reference(golden, name):
    from ultralytics.nn.extra_modules import SPDConv
    G = golden("spd")
    m = _model(name)
    assert sum(p.numel() for p in m.parameters()) == N_PARAMS[name] == int(G[f"{name}/n_params"])
    assert m.yaml["nc"] == 6 and m.stride.tolist() == [4.0, 8.0, 16.0] == G[f"{name}/stride"].tolist()
    assert [i for i, mod in enumerate(m.model) if isinstance(mod, SPDConv)] == list(SPD_LAYERS)
    for i in SPD_LAYERS:
        assert m.model[i].type == "ultralytics.nn.extra_modules.block.SPDConv" and m.model[i].d == 1
        assert m.model[i].conv.conv.in_channels == 4 * m._cout[i - 1] and m.model[i].conv.conv.kernel_size == (3, 3)
        assert m.model[i].conv.conv.stride == (1, 1) and m.model[i].out_hw(12, 20) == (6, 10)
    if "ASF" in name:  # the five SPD convolutions of the issue: 64>32, 128>64, 256>128, 128>32, 256>64
        assert [(m.model[i].conv.conv.in_channels, m.model[i].conv.conv.out_channels) for i in SPD_LAYERS] == [
            (64, 32), (128, 64), (256, 128), (128, 32), (256, 64)]


@pytest.mark.parametrize("name", MODELS)
def test_state_dict_layout_is_the_reference_s(golden, name):
    want = layout(golden("spd"), name)
    got = {k: tuple(v.shape) for k, v in _model(name).state_dict().items()}
    assert list(got) == list(want), [k for k in got if k not in want][:5] + [k for k in want if k not in got][:5]
    assert got == want
    assert all(f"model.{i}.conv.conv.weight" in got and f"model.{i}.conv.bn.running_var" in got for i in SPD_LAYERS)


def test_scale_letter_resolves():
    m = _model("yolov8s-ASF-P2P2-SPD")
    assert m.yaml["scale"] == "s" and m.model[1].conv.conv.in_channels == 4 * 32 and m.model[1].conv.conv.out_channels == 64
    assert m.stride.tolist() == [4.0, 8.0, 16.0]


def test_module_is_exported_under_the_reference_s_class_path():
    import ultralytics.nn.extra_modules as X
    import ultralytics.nn.extra_modules.block as B
    assert "SPDConv" in X.__all__ and "SPDConv" in B.__all__ and X.SPDConv is B.SPDConv
    assert B.SPDConv.__module__ == "ultralytics.nn.extra_modules.block"
    m = B.SPDConv(16, 32)
    assert list(m.state_dict()) == ["conv.conv.weight", "conv.bn.weight", "conv.bn.bias", "conv.bn.running_mean", "conv.bn.running_var",
                                    "conv.bn.num_batches_tracked"]
    assert tuple(m.conv.conv.weight.shape) == (32, 64, 3, 3) and m.d == 1


@pytest.mark.parametrize("hw", [(13, 20), (12, 21), (1, 8)])
def test_odd_map_is_refused_by_name(hw):
    """The reference's torch.cat of the four parity views raises on an odd map; here the layer says which one it is and what it got,
    before anything is launched (the check needs no device)."""
    from types import SimpleNamespace
    m = _model("yolov8n-ASF-P2P2-SPD").model[3]
    x = SimpleNamespace(N=2, H=hw[0], W=hw[1], C=32)
    with pytest.raises(ValueError) as e:
        m.forward_act(x)
    assert "layer 3" in str(e.value) and f"{hw[0]}x{hw[1]}" in str(e.value)


def test_reference_written_spd_checkpoint_rebuilds(golden):
    """tests/golden/ref_ckpt_spd.pt: a whole-module fp16 pickle written by the REFERENCE's classes whose YAML names SPDConv."""
    from spd_util import state
    from ultralytics.nn.extra_modules import SPDConv
    from ultralytics.nn.tasks import DetectionModel, _rebuild, attempt_load_weights, torch_safe_load
    ckpt, _ = torch_safe_load(CKPT)
    assert ckpt["epoch"] == 3 and ckpt["ema"] is None
    obj = ckpt["model"]
    assert [type(obj.model[i]) for i in SPD_LAYERS] == [SPDConv] * 5, "the pickled class path does not resolve to this package's SPDConv"
    assert any(row[2] == "SPDConv" for row in obj.yaml["backbone"] + obj.yaml["head"])
    m = _rebuild(obj, ckpt)
    assert isinstance(m, DetectionModel)
    pickled, got = obj.state_dict(), m.state_dict()
    assert list(got) == list(pickled)
    for k, v in pickled.items():
        assert got[k].dtype == (torch.float32 if v.is_floating_point() else v.dtype)
        assert torch.equal(got[k].float(), v.float()), k
    want = state(golden("spd"), "ckpt")  # the state the generator filled in, as the reference's .half() stored it
    assert list(want) == list(got)
    for k, v in want.items():
        assert torch.equal(got[k].float(), (v.half().float() if v.is_floating_point() else v.float())), k
    assert not attempt_load_weights(CKPT).training


def test_spd_checkpoint_roundtrip_in_the_reference_format(tmp_path):
    from ultralytics.nn.extra_modules import SPDConv
    from ultralytics.nn.tasks import attempt_load_weights, save_reference_format, torch_safe_load
    m = _model("yolov8n-ASF-P2P2-SPD")
    path = save_reference_format(str(tmp_path / "last.pt"), m, updates=4, epoch=1, train_args={"imgsz": 64})
    ckpt, _ = torch_safe_load(path)
    obj = ckpt["model"]
    assert next(obj.parameters()).dtype == torch.float16 and all("rt" not in mod.__dict__ for mod in obj.modules())
    assert [type(obj.model[i]) for i in SPD_LAYERS] == [SPDConv] * 5 and obj.model[1].type == "ultralytics.nn.extra_modules.block.SPDConv"
    back = attempt_load_weights(path)
    for (k, a), (_, b) in zip(m.state_dict().items(), back.state_dict().items()):
        assert torch.equal(a.half().float() if a.is_floating_point() else a, b.float() if a.is_floating_point() else b), k


def test_entry_point_is_bound():
    import ctypes as C
    from ultralytics.hip import SIGNATURES, lib
    res, args = SIGNATURES["dy_space_to_depth"]
    assert res is C.c_int and len(args) == 11 and args[0] is C.c_void_p and args[2] is C.c_void_p
    L = lib()
    assert L.dy_space_to_depth.argtypes == list(args)
    # refusals need no device: nothing is launched
    DY_ERR_ARG, DY_ERR_ALIGN = -1, -3  # include/dealyolo_hip.h
    ok = dict(x=4096, ldx=16, y=8192, ldy=64, n=1, h=4, w=4, C=16)

    def rc(**kw):
        a = dict(ok, **kw)
        return L.dy_space_to_depth(a["x"], a["ldx"], a["y"], a["ldy"], a["n"], a["h"], a["w"], a["C"], 0, 0, None)

    assert rc(h=5) == DY_ERR_ARG and rc(w=3) == DY_ERR_ARG and rc(h=0) == DY_ERR_ARG and rc(w=1) == DY_ERR_ARG
    assert rc(x=0) == DY_ERR_ARG and rc(y=0) == DY_ERR_ARG
    assert rc(C=12) == DY_ERR_ALIGN and rc(ldx=20) == DY_ERR_ALIGN and rc(ldy=68) == DY_ERR_ALIGN
    assert rc(x=4104) == DY_ERR_ALIGN and rc(y=8200) == DY_ERR_ALIGN
