"""-m gpu: the reference's box-loss menu in dy_detection_loss (box_loss_kernel<true>) against tests/golden/boxloss_*.npz -- every
WiseIouLoss ltype x {plain, Inner, Focaler} (v3, and v1 / v2 for four of them), every bbox_iou-family flag x {plain, Inner, Focaler},
NWD blends and non-default parameters -- through the public criterion and through a whole StepPlan step of DEAL-YOLO-N.

Bounds: tests/test_gpu_loss.py's for the same quantities (loss 1e-4 relative + 1e-5, items 1e-4, gradients 2e-3 of the largest entry
as they are emitted in fp16, iou_mean 1e-5) and tests/test_gpu_model.py's for the N step (fp16 activations).  The reference's own fp32
rounding on these inputs (fp32 vs fp64 over the whole matrix) is at most 3.9e-6 on the gradients, 2.7e-7 on the items and 1.3e-7 on
iou_mean: every bound has at least 25x headroom over it."""
import os

import numpy as np
import pytest
import torch

from conftest import CFG_DIR
from golden.boxloss_modes import STEP_MODES, apply_mode, boxloss_modes, cases_of, n_calls, step_spec
from gpu_util import relerr
from oracle import graph as og

pytestmark = pytest.mark.gpu
MODES = boxloss_modes()
MODE_NAMES = list(MODES)
PAIRS = [(case, mode) for mode in MODES for case in cases_of(mode)]


def _shard(golden, mode):
    return golden(f"boxloss_{MODE_NAMES.index(mode) % 3}")


def _headout(L, case):
    from ultralytics.nn.modules.head import HeadOut
    box, cls = [], []
    for l in range(3):
        f = L.t(f"{case}/feat{l}").cuda().permute(0, 2, 3, 1).contiguous()
        box.append(f[..., :64].contiguous())
        c = torch.zeros(*f.shape[:3], 8, device="cuda")
        c[..., :6] = f[..., 64:]
        cls.append(c)
    ho = HeadOut(box, cls, 6, [4.0, 8.0, 16.0])
    ho.alloc_grads()
    for d in ho.dbox:
        d.fill_(1.0)  # every row must be written: foreground rows by the loss, the rest zeroed
    return ho


class _M:  # minimal stand-in exposing what v8DetectionLoss reads from a model
    class _Det:
        stride = torch.tensor([4.0, 8.0, 16.0])
        nc, no, reg_max = 6, 70, 16

    def __init__(self):
        self.model = [self._Det()]
        self._p = torch.zeros(1, device="cuda")

    def parameters(self):
        yield self._p


def _check_call(crit, ho, L, G, case, mode, call, last):
    from ultralytics.utils.metrics import WiseIouLoss  # noqa: F401
    spec = MODES[mode]
    batch = {k: L.t(f"{case}/{k}") for k in ("batch_idx", "cls", "bboxes")}
    loss, items = crit(ho, batch)
    torch.cuda.synchronize()
    tag = f"{case}/{mode}" + (f"/call{call}" if n_calls(spec, case) > 1 else "")
    ref_loss = float(G[f"{tag}/loss"])
    e_items = relerr(items, G.t(f"{tag}/items"))
    msg = f"{tag}: loss {float(loss):.7g} vs {ref_loss:.7g}, items relerr {e_items:.2e}"
    if spec["wise"]:
        d_mean = abs(float(crit.bbox_loss.wiou_loss.iou_mean) - float(G[f"{tag}/iou_mean"]))
        msg += f", iou_mean diff {d_mean:.2e}"
    print(msg)
    assert abs(float(loss) - ref_loss) <= 1e-4 * abs(ref_loss) + 1e-5, msg
    assert e_items < 1e-4, msg
    if spec["wise"]:
        assert d_mean < 1e-5, msg
    if not last:
        return
    fg = L.t(f"{case}/fg_mask").bool()
    got = torch.cat([d.float().flatten(1, 2) for d in ho.dbox], 1).cpu()  # (B, A, 64), level-major
    assert float(got[~fg].abs().max()) == 0.0, "background box-logit rows"
    ref = G.t(f"{case}/{mode}/gbox")
    if ref.shape[0]:
        e = relerr(got[fg], ref)
        print(f"  foreground box-logit gradient relerr {e:.2e} ({ref.shape[0]} rows)")
        assert e < 2e-3
    for l in range(3):
        refc = L.t(f"{case}/ciou/gfeat{l}").permute(0, 2, 3, 1)[..., 64:]
        gotc = ho.dcls[l][..., :6].float().cpu()
        if float(refc.abs().max()) == 0:
            assert float(gotc.abs().max()) == 0
        else:
            assert relerr(gotc, refc) < 2e-3, f"class gradient level {l}"


@pytest.mark.parametrize("case,mode", PAIRS, ids=[f"{c}-{m}" for c, m in PAIRS])
def test_criterion_vs_golden(golden, case, mode):
    from ultralytics.utils.loss import v8DetectionLoss
    from ultralytics.utils.metrics import WiseIouLoss
    L, G = golden("loss"), _shard(golden, mode)
    crit = v8DetectionLoss(_M())
    apply_mode(crit.bbox_loss, MODES[mode], WiseIouLoss)
    n = n_calls(MODES[mode], case)
    for call in range(n):
        _check_call(crit, _headout(L, case), L, G, case, mode, call, call == n - 1)


def test_switching_modes_on_one_criterion(golden):
    """Modes change between calls of one criterion; assigning a fresh WiseIouLoss restarts the running mean at 1."""
    from ultralytics.utils.loss import v8DetectionLoss
    from ultralytics.utils.metrics import WiseIouLoss
    L = golden("loss")
    case = "random5"
    crit = v8DetectionLoss(_M())
    seq = [("w_SIoU_v3_plain", 0), ("w_SIoU_v3_plain", 1), ("b_DIoU_inner", 0), ("w_SIoU_v3_plain", 0), ("w_PIoU2_v3_focaler", 0),
           ("b_CIoU_plain", 0), ("w_MPDIoU_v1_plain", 0), ("b_ShapeIoU_focaler", 0)]
    for mode, call in seq:
        if call == 0:
            apply_mode(crit.bbox_loss, MODES[mode], WiseIouLoss)
        _check_call(crit, _headout(L, case), L, _shard(golden, mode), case, mode, call, True)
    # the legacy toggles still select the legacy modes on the same criterion
    crit.bbox_loss.use_wiseiou, crit.bbox_loss.nwd_loss = False, False
    crit.bbox_loss.iou_type, crit.bbox_loss.iou_variant = "CIoU", None
    loss, items = crit(_headout(L, case), {k: L.t(f"{case}/{k}") for k in ("batch_idx", "cls", "bboxes")})
    assert relerr(items, L.t(f"{case}/ciou/items")) < 1e-4


def _build_n():
    from ultralytics.nn.tasks import DetectionModel
    name = "yolov8n-ASF-P2P2"
    m = DetectionModel(os.path.join(CFG_DIR, name + ".yaml"), ch=3, verbose=False)
    g = og.build_graph(og.load_yaml(os.path.join(CFG_DIR, name + ".yaml")))
    m.load_state_dict(og.fill_state(og.state_layout(g), 7), strict=True)
    return m.cuda().train()


def _batch(golden):
    M = golden("models")
    return {k: M.t(f"yolov8n-ASF-P2P2/{k}") for k in ("img", "batch_idx", "cls", "bboxes")}


@pytest.mark.parametrize("mode", STEP_MODES)
def test_step_plan_vs_golden(golden, mode):
    """DEAL-YOLO-N 64x64, batch 2, under an extended mode: tests/test_gpu_model.py's bounds for N (fp16 activation storage)."""
    from ultralytics.hip.train import StepPlan
    from ultralytics.utils.metrics import WiseIouLoss
    G = golden("boxloss_0")
    m = _build_n()
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    apply_mode(plan.crit.bbox_loss, step_spec(mode), WiseIouLoss)
    assert plan.crit.bbox_loss.mode_fields()[0] != 0
    plan.forward_backward(_batch(golden))
    torch.cuda.synchronize()
    s = plan.crit.scalars.cpu()
    ref_items = G.t(f"step/{mode}/items")
    per_item = float(((s[5:8] - ref_items).abs() / ref_items.abs()).max())
    d_loss = abs(float(s[8]) - float(G[f"step/{mode}/loss"])) / float(G[f"step/{mode}/loss"])
    names = list(G[f"step/{mode}/grad_names"])
    params = dict(m.named_parameters())
    scale = float(plan.state[0])
    l2 = torch.stack([params[k].grad.float().norm() / scale for k in names]).cpu()
    ref = G.t(f"step/{mode}/grad_l2")
    rel = ((l2 - ref).abs() / (ref.abs() + 1e-3 * ref.abs().max())).numpy()
    print(f"{mode}: items {s[5:8].tolist()} vs {ref_items.tolist()} worst per-item {per_item:.2e}, loss {d_loss:.2e}, "
          f"grad-l2 median {np.median(rel):.2e} max {rel.max():.2e} ({names[int(rel.argmax())]})")
    assert per_item < 1.2e-2
    assert d_loss < 5e-3
    assert np.median(rel) < 4e-3 and rel.max() < 4e-2


def test_graph_replay_under_an_extended_mode(golden):
    """A replayed hipGraph step reproduces the traced step bit for bit under an extended mode, and a replay after the extended mode
    changed raises instead of replaying the old loss; the legacy toggles keep their behaviour."""
    from ultralytics.hip.train import StepPlan
    from ultralytics.utils.metrics import WiseIouLoss
    batch = _batch(golden)
    m = _build_n()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0, use_graph=True)
    apply_mode(plan.crit.bbox_loss, step_spec("b_EIoU_inner"), WiseIouLoss)
    plan.forward_backward(batch)
    torch.cuda.synchronize()
    assert plan.graph_fb is not None
    g1, s1 = plan.rt.flat_g.clone(), plan.crit.scalars.clone()
    m.load_state_dict(sd0)
    plan.forward_backward(batch)  # graph replay
    torch.cuda.synchronize()
    assert torch.equal(plan.crit.scalars[5:9], s1[5:9])
    assert torch.equal(plan.rt.flat_g, g1)
    plan.crit.bbox_loss.iou_variant = "focaler"
    with pytest.raises(RuntimeError, match="captured"):
        plan.forward_backward(batch)
    plan.crit.bbox_loss.iou_type, plan.crit.bbox_loss.iou_variant = "CIoU", None  # legacy CIoU: differs from the captured mode too
    with pytest.raises(RuntimeError, match="captured"):
        plan.forward_backward(batch)
    plan.crit.bbox_loss.iou_type, plan.crit.bbox_loss.iou_variant = "EIoU", "inner"
    plan.forward_backward(batch)
    torch.cuda.synchronize()
    # legacy capture: the legacy toggles replay frozen, as before; switching to an extended mode raises
    plan2 = StepPlan(_build_n(), 2, 64, nmax=8, init_scale=1024.0, use_graph=True)
    plan2.forward_backward(batch)
    plan2.crit.bbox_loss.nwd_loss = True
    plan2.forward_backward(batch)
    plan2.crit.bbox_loss.nwd_loss = False
    plan2.crit.bbox_loss.use_wiseiou = True
    plan2.crit.bbox_loss.wiou_loss = WiseIouLoss("SIoU")
    with pytest.raises(RuntimeError, match="captured"):
        plan2.forward_backward(batch)
    torch.cuda.synchronize()


def test_trainer_applies_the_cfg_keys(tmp_path):
    """``YOLO(...).train(wiou=True, wiou_ltype=...)`` / ``train(iou_type=..., iou_variant=...)``: the keys reach the criterion before the
    first trace, so the recorded (hipGraph) step runs the chosen box loss."""
    from golden.cases import write_dataset
    from ultralytics import YOLO
    from ultralytics.utils.metrics import WiseIouLoss
    root = str(tmp_path / "ds")
    write_dataset(root)
    common = dict(data=os.path.join(root, "data.yaml"), batch=4, imgsz=64, epochs=1, optimizer="SGD", workers=2, hipgraph=True, val=False)
    y = YOLO("yolov8n-ASF-P2P2.yaml")
    hist = y.train(wiou=True, wiou_ltype="SIoU", wiou_monotonous=None, wiou_focaler=True, nwd=True, **common)
    plan = y.trainer.plan
    assert isinstance(plan.crit.bbox_loss.wiou_loss, WiseIouLoss) and plan.crit.bbox_loss.wiou_loss.ltype == "SIoU"
    assert plan._box_mode[:4] == (1, 6, 1, 2) and plan.crit._args.box_family == 1 and plan.crit._args.use_nwd == 1
    assert np.isfinite(np.asarray(hist, dtype=np.float64)).all()
    y = YOLO("yolov8n-ASF-P2P2.yaml")
    hist = y.train(iou_type="MPDIoU", iou_variant="focaler", **common)
    plan = y.trainer.plan
    assert plan._box_mode[:4] == (2, 10, 0, 2) and plan.crit._args.box_ltype == 10
    assert np.isfinite(np.asarray(hist, dtype=np.float64)).all()
