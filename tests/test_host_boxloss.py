"""CPU: the box-loss menu's public interface (WiseIouLoss, BboxLoss.iou_type / iou_variant, the cfg keys) and its encoding into the
argument block of dy_detection_loss (include/dealyolo_hip.h DY_BOX_*), and the coverage of the fixture tests/golden/boxloss_*.npz."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the package on sys.path)
from golden.boxloss_modes import BBOX_TYPES, SUBSET, SUBSET_CASES, FULL_CASES, STEP_MODES, WISE_LTYPES, boxloss_modes

LEGACY = (0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)


def _bl():
    from ultralytics.utils.loss import BboxLoss
    s = torch.zeros(16)
    s[4] = 1.0
    return BboxLoss(15, True, s), s


def test_wise_iou_loss_signature_and_validation():
    from ultralytics.utils.metrics import WiseIouLoss
    w = WiseIouLoss()
    assert (w.ltype, w.monotonous, w.inner_iou, w.focaler_iou) == ("WIoU", False, False, False)
    assert (WiseIouLoss.momentum, WiseIouLoss.alpha, WiseIouLoss.delta) == (1e-2, 1.7, 2.7)
    assert float(w.iou_mean) == 1.0
    for lt in WISE_LTYPES:
        WiseIouLoss(lt, None, True, False)
    with pytest.raises(AssertionError):
        WiseIouLoss("AlphaIoU")
    with pytest.raises(NotImplementedError, match="criterion"):
        w(torch.zeros(1, 4), torch.zeros(1, 4))


def test_bbox_loss_validation():
    bl, _ = _bl()
    for name, bad in (("iou_type", "WIoU"), ("iou_type", "ciou"), ("iou_variant", "Inner"), ("iou_variant", ""), ("inner_ratio", 0.0),
                      ("focaler_u", float("nan")), ("piou_lambda", "1.3"), ("wiou_loss", object())):
        with pytest.raises(ValueError):
            setattr(bl, name, bad)
    bl.iou_variant, bl.focaler_d, bl.focaler_u = "focaler", 0.5, 0.5
    with pytest.raises(ValueError):
        bl.mode_fields()


def test_defaults_encode_the_legacy_modes():
    """All-zero new fields: what the four legacy modes (use_wiseiou x nwd_loss) always sent."""
    from ultralytics.utils.metrics import WiseIouLoss
    bl, _ = _bl()
    assert (bl.iou_type, bl.iou_variant) == ("CIoU", None)
    assert (bl.inner_ratio, bl.focaler_d, bl.focaler_u, bl.shape_scale, bl.piou_lambda) == (0.7, 0.0, 0.95, 0.0, 1.3)
    for wise in (False, True):
        for nwd in (False, True):
            bl.use_wiseiou, bl.nwd_loss = wise, nwd
            assert bl.mode_fields() == LEGACY
    bl.use_wiseiou = True
    bl.wiou_loss = WiseIouLoss("WIoU", False, False, False)  # the reference's default object is the legacy WIoU v3
    assert bl.mode_fields() == LEGACY
    bl.use_wiseiou = False
    bl.iou_type, bl.iou_variant = "CIoU", None
    assert bl.mode_fields() == LEGACY


def test_encoding_of_the_menu():
    from ultralytics.utils.metrics import WiseIouLoss
    bl, _ = _bl()
    bl.use_wiseiou = True
    bl.wiou_loss = WiseIouLoss("SIoU", None, False, True)
    assert bl.mode_fields()[:4] == (1, 6, 1, 2)
    bl.wiou_loss = WiseIouLoss("MPDIoU", True, True, True)  # inner wins over focaler, as in utils/metrics.py:618
    assert bl.mode_fields()[:4] == (1, 10, 2, 1)
    bl.wiou_loss = WiseIouLoss("WIoU", False, True, False)
    assert bl.mode_fields()[:4] == (1, 1, 3, 1)
    bl.use_wiseiou = False
    bl.iou_type, bl.iou_variant, bl.shape_scale = "ShapeIoU", "inner", 0.5
    assert bl.mode_fields() == (2, 7, 0, 1, 0.7, 0.0, 0.95, 0.5, 1.3)
    bl.iou_type, bl.iou_variant = "CIoU", "focaler"
    assert bl.mode_fields()[:4] == (2, 5, 0, 2)


def test_assigning_a_fresh_wise_iou_loss_restarts_the_mean():
    from ultralytics.utils.metrics import WiseIouLoss
    bl, s = _bl()
    s[4] = 0.37  # a running mean left by earlier calls
    w = WiseIouLoss("EIoU")
    bl.wiou_loss = w
    assert float(s[4]) == 1.0 and float(bl.wiou_loss.iou_mean) == 1.0
    w.iou_mean = 0.5  # afterwards the object reads and writes the criterion's scalar
    assert float(s[4]) == 0.5
    s[4] = 0.25
    assert float(w.iou_mean) == 0.25


def test_cfg_keys_and_trainer_mapping():
    from types import SimpleNamespace
    from ultralytics.cfg import DEFAULT_CFG_DICT, get_cfg
    from ultralytics.utils.metrics import WiseIouLoss
    d = DEFAULT_CFG_DICT
    assert (d["iou_type"], d["iou_variant"], d["wiou_ltype"], d["wiou_monotonous"], d["wiou_inner"], d["wiou_focaler"]) == \
        ("CIoU", None, "WIoU", False, False, False)
    a = get_cfg(d, dict(wiou=True, wiou_ltype="SIoU", wiou_monotonous=None, wiou_focaler=True))
    with pytest.raises(TypeError):
        get_cfg(d, dict(wiou_inner="yes"))
    # the trainer's mapping (engine/trainer.py): the defaults keep today's modes
    bl, _ = _bl()
    bl.use_wiseiou = bool(d["wiou"])
    bl.configure_from_cfg(get_cfg(d))
    assert bl.mode_fields() == LEGACY
    bl.use_wiseiou = True
    bl.configure_from_cfg(a)
    assert isinstance(bl.wiou_loss, WiseIouLoss) and bl.mode_fields()[:4] == (1, 6, 1, 2)
    bl.use_wiseiou = False
    bl.configure_from_cfg(SimpleNamespace(iou_type="MPDIoU", iou_variant="inner"))
    assert bl.mode_fields()[:4] == (2, 10, 0, 1)
    with pytest.raises(ValueError):
        bl.configure_from_cfg(SimpleNamespace(iou_type="AlphaIoU", iou_variant=None))


def test_argument_block_carries_the_mode():
    import ctypes as C
    from ultralytics.hip import DyLossArgs
    names = [f[0] for f in DyLossArgs._fields_]
    tail = ["box_family", "box_ltype", "box_fm", "box_modifier", "inner_ratio", "focaler_d", "focaler_u", "shape_scale", "piou_lambda"]
    assert names[-len(tail):] == tail  # appended: the offsets of every earlier field are unchanged
    assert DyLossArgs.box_in_coef.offset + DyLossArgs.box_in_coef.size <= DyLossArgs.box_family.offset
    a = DyLossArgs()
    assert all(getattr(a, n) == 0 for n in tail)
    assert C.sizeof(DyLossArgs) >= DyLossArgs.piou_lambda.offset + 4


def test_fixture_covers_the_menu(golden):
    modes = boxloss_modes()
    assert len(modes) == 76
    assert list(golden("boxloss_0")["modes"]) == list(modes)
    specs = list(modes.values())
    for lt in WISE_LTYPES:
        for v in (None, "inner", "focaler"):
            assert any(s["wise"] and s["ltype"] == lt and s["variant"] == v and s["mono"] is False for s in specs), (lt, v)
    for lt in ("WIoU", "CIoU", "SIoU", "MPDIoU"):
        for mono in (None, True):
            assert any(s["wise"] and s["ltype"] == lt and s["mono"] is mono and s["variant"] is None for s in specs)
    for t in BBOX_TYPES:
        for v in (None, "inner", "focaler"):
            assert any(not s["wise"] and s["ltype"] == t and s["variant"] == v for s in specs), (t, v)
    assert sum(s["nwd"] for s in specs) == 3 and any("scale" in s for s in specs) and any("d" in s for s in specs)
    assert all(m in modes for m in SUBSET) and len(SUBSET) == 12
    for i, (m, s) in enumerate(modes.items()):
        G = golden(f"boxloss_{i % 3}")
        for case in FULL_CASES + (SUBSET_CASES if m in SUBSET else ()):
            tag = f"{case}/{m}" + ("/call2" if s["wise"] and case == "random5" else "")
            assert np.isfinite(G[f"{tag}/loss"]) and np.isfinite(G[f"{tag}/items"]).all()
            assert G[f"{case}/{m}/gbox"].shape[1] == 64
    G0 = golden("boxloss_0")
    for m in STEP_MODES:
        assert len(G0[f"step/{m}/grad_names"]) == len(G0[f"step/{m}/grad_l2"]) > 100
