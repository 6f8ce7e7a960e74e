"""-m gpu: test-time augmentation, ``model(x, augment=True)`` (csrc/tta.hip, ultralytics/hip/tta.py; reference nn/tasks.py:335-371,
utils/torch_utils.py:355-366, engine/predictor.py:140, engine/validator.py:109, double_inference.py:231-235).

What is pinned: dy_scale_img against F.interpolate + F.pad on the same device; dy_tta_merge against the torch restatement of
_descale_pred + _clip_augmented + cat, bit for bit; the augmented forward against the reference's (tests/golden/tta.npz); the
recorded plans against the walked launches, bit for bit; the plan registry; and the public entry points that pass ``augment``."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import CFG_DIR
from gpu_util import relerr

pytestmark = pytest.mark.gpu


def _model(name, seed=7, fuse=False):
    from oracle import graph as og
    from ultralytics.nn.tasks import DetectionModel
    p = os.path.join(CFG_DIR, name + ".yaml")
    m = DetectionModel(p, ch=3, verbose=False)
    g = og.build_graph(og.load_yaml(p))
    m.load_state_dict(og.fill_state(og.state_layout(g), seed), strict=True)
    m = m.cuda().eval()
    return m.fuse() if fuse else m


def _scale(x, flip, Ho, Wo, Hp, Wp):
    from ultralytics.hip.tta import scale_into
    out = torch.full((x.shape[0], 3, Hp, Wp), float("nan"), device=x.device)
    return scale_into(x, dict(flip=flip, Ho=Ho, Wo=Wo, Hp=Hp, Wp=Wp), out)


@pytest.mark.parametrize("gs", [16, 32])
@pytest.mark.parametrize("flip", [0, 2, 3])
def test_scale_img_kernel_matches_interpolate_and_pad(gs, flip):
    torch.manual_seed(gs + flip)
    exact = []
    for B, H, W in [(2, 64, 64), (3, 37, 53), (1, 160, 96), (2, 101, 211)]:
        x = torch.rand(B, 3, H, W, device="cuda")
        xi = x.flip(flip) if flip else x
        for r in (0.83, 0.67, 0.5):
            Ho, Wo = int(H * r), int(W * r)
            Hp, Wp = math.ceil(H * r / gs) * gs, math.ceil(W * r / gs) * gs
            want = F.pad(F.interpolate(xi, size=(Ho, Wo), mode="bilinear", align_corners=False), [0, Wp - Wo, 0, Hp - Ho], value=0.447)
            got = _scale(x, flip, Ho, Wo, Hp, Wp)
            torch.cuda.synchronize()
            d = float((got[:, :, :Ho, :Wo] - want[:, :, :Ho, :Wo]).abs().max())
            assert d <= 2.4e-7, (B, H, W, r, d)
            exact.append(torch.equal(got[:, :, :Ho, :Wo], want[:, :, :Ho, :Wo]))
            pad = torch.tensor(0.447, dtype=torch.float32).item()
            assert (got[:, :, Ho:, :] == pad).all() and (got[:, :, :, Wo:] == pad).all()
    print(f"dy_scale_img bit-exact to F.interpolate in {sum(exact)} of {len(exact)} cases (gs {gs}, flip {flip})")
    # ratio 1 with a flip: scale_img returns the flipped tensor itself
    x = torch.rand(2, 3, 37, 52, device="cuda")
    for f in (2, 3):
        assert torch.equal(_scale(x, f, 37, 52, 37, 52), x.flip(f))


def _restated_merge(ys, geo, H, W):
    """_descale_pred + _clip_augmented + torch.cat as the reference writes them (on the host, where ATen divides)."""
    out = []
    for y, p in zip(ys, geo):
        q = y.cpu().clone()
        q[:, :4] /= p["scale"]
        x_, y_, wh, cls = q.split((1, 1, 2, q.shape[1] - 4), 1)
        if p["flip"] == 2:
            y_ = H - y_
        elif p["flip"] == 3:
            x_ = W - x_
        q = torch.cat((x_, y_, wh, cls), 1)
        lo, hi = p["cols"]
        out.append(q[..., lo:hi])
    return torch.cat(out, -1)


@pytest.mark.parametrize("nl,no,B,As,H,W", [(3, 10, 2, (336, 336, 189), 64, 64), (4, 84, 1, (340, 340, 340), 64, 64),
                                             (3, 7, 3, (1008, 735, 630), 96, 128), (3, 12, 1, (20, 21, 40), 33, 17)])
def test_merge_kernel_is_descale_clip_cat_bit_for_bit(nl, no, B, As, H, W):
    from ultralytics.hip.tta import kept_columns, merge
    g = torch.Generator().manual_seed(sum(As))
    ys = [(torch.randn(B, no, A, generator=g) * 300).cuda() for A in As]
    for flips in ([0, 3, 0], [2, 0, 3]):
        geo = [dict(scale=s, flip=f, cols=c) for s, f, c in zip((1, 0.83, 0.67), flips, kept_columns(list(As), nl))]
        got = merge(ys, geo, H, W)
        want = _restated_merge(ys, geo, H, W)
        assert got.shape == want.shape and torch.equal(got.cpu(), want), float((got.cpu() - want).abs().max())


@pytest.mark.parametrize("case,fuse", [("asf_p2p2_64", False), ("asf_p2p2_96x128", False), ("asf_p2p2_160", False),
                                       ("asf_p2p2_96x128_fused", True), ("p2_64", False)])
def test_augmented_forward_matches_reference(golden, case, fuse):
    g = golden("tta")
    m = _model("yolov8n-p2" if case.startswith("p2") else "yolov8n-ASF-P2P2", fuse=fuse)
    x = (torch.from_numpy(g["img/" + str(g[case + "/img"])]).float() / 255).cuda()
    want = g.t(case + "/y")
    for _ in range(3):  # walked, recorded, replayed
        y, second = m(x, augment=True)
        assert second is None and tuple(y.shape) == tuple(want.shape)
        eb, ec = relerr(y[:, :4], want[:, :4]), relerr(y[:, 4:], want[:, 4:])
        print(f"{case}: box relerr {eb:.2e}, class relerr {ec:.2e}")
        assert eb <= 1e-3 and ec <= 1e-3
    if case == "asf_p2p2_96x128":  # the third pass's image against the reference's scale_img
        from ultralytics.hip.tta import tta_geometry
        p = tta_geometry(96, 128, 16, 3)[2]
        got = _scale(x, p["flip"], p["Ho"], p["Wo"], p["Hp"], p["Wp"])
        assert float((got.cpu() - g.t(case + "/scaled2")).abs().max()) <= 1e-6


def test_plan_replays_the_walked_forward_bit_for_bit():
    from ultralytics.hip import infer as I
    m = _model("yolov8n-ASF-P2P2", fuse=True)
    x = torch.rand(2, 3, 96, 128, device="cuda")
    ys = [m(x, augment=True)[0] for _ in range(3)]  # walk, record, replay
    st = m._tta_plans
    assert set(st["plans"]) == {(2, 3, 96, 128)}
    assert all(p.rec is not None for p in st["plans"][(2, 3, 96, 128)].plans)
    I.INFER_PLAN = False
    try:
        ys.append(m(x, augment=True)[0])
    finally:
        I.INFER_PLAN = True
    for y in ys[1:]:
        assert torch.equal(y, ys[0])
    assert ys[1].data_ptr() != ys[2].data_ptr()  # the caller's own tensor


def test_plan_registries_are_separate():
    m = _model("yolov8n-ASF-P2P2")
    x = torch.rand(1, 3, 64, 64, device="cuda")
    for _ in range(2):
        m(x, augment=True)
        m(x)
    single, tta = m._infer_plans["plans"][(1, 3, 64, 64)], m._tta_plans["plans"][(1, 3, 64, 64)]
    recs = [single.rec] + [p.rec for p in tta.plans]
    ya, yb = m(x, augment=True)[0], m(x)[0]
    for _ in range(3):
        assert torch.equal(m(x, augment=True)[0], ya) and torch.equal(m(x)[0], yb)
    assert m._infer_plans["plans"][(1, 3, 64, 64)] is single and m._tta_plans["plans"][(1, 3, 64, 64)] is tta
    assert [single.rec] + [p.rec for p in tta.plans] == recs  # nothing re-recorded
    assert ya.shape[-1] != yb.shape[-1]


def test_predict_passes_augment():
    from ultralytics import YOLO
    from ultralytics.utils import ops
    y = YOLO("yolov8n-ASF-P2P2.yaml")
    from oracle import graph as og
    p = os.path.join(CFG_DIR, "yolov8n-ASF-P2P2.yaml")
    y.model.load_state_dict(og.fill_state(og.state_layout(og.build_graph(og.load_yaml(p))), 7), strict=True)
    x = torch.rand(2, 3, 64, 96)
    res = y.predict(x, augment=True, conf=0.001)
    pred, _ = y.model(x.cuda(), augment=True)
    want = ops.non_max_suppression(pred, 0.001, 0.7, max_det=300)
    for r, w in zip(res, want):
        w[:, :4] = ops.scale_boxes((64, 96), w[:, :4], (64, 96, 3))  # equal shapes: the clip
        assert len(w) > 0 and torch.equal(r.boxes.data.cpu(), w.cpu())
    single = y.predict(x, augment=False, conf=0.001)
    assert any(not torch.equal(a.boxes.data, b.boxes.data) for a, b in zip(res, single))


def test_validator_runs_tta_when_asked(monkeypatch):
    from ultralytics.hip import tta
    from ultralytics.models.yolo.detect import DetectionValidator
    m = _model("yolov8n-ASF-P2P2")
    calls = []
    real = tta.forward_tta

    def spy(model, x):
        calls.append(tuple(x.shape))
        return real(model, x)

    monkeypatch.setattr(tta, "forward_tta", spy)
    rng = np.random.default_rng(3)
    B, nb = 2, 3

    def batch():
        return dict(img=torch.from_numpy(rng.random((B, 3, 64, 64), dtype=np.float32)), batch_idx=torch.arange(B).repeat_interleave(nb).float(),
                    cls=torch.from_numpy(rng.integers(0, 6, (B * nb, 1)).astype(np.float32)),
                    bboxes=torch.from_numpy(np.concatenate([rng.random((B * nb, 2)) * 0.6 + 0.2, rng.random((B * nb, 2)) * 0.3 + 0.05], 1).astype(np.float32)))
    data = [batch(), batch()]
    DetectionValidator(dataloader=[dict(b) for b in data], args={"augment": False})(model=m)
    assert calls == []
    stats = DetectionValidator(dataloader=[dict(b) for b in data], args={"augment": True})(model=m)
    assert calls == [(B, 3, 64, 64)] * 2 and isinstance(stats, dict)


def test_double_inference_second_stage_with_augment(monkeypatch):
    from ultralytics.hip import tta
    from ultralytics.utils import double_inference as di
    m = _model("yolov8n-ASF-P2P2")
    calls, stages = [], []
    real, real_stage = tta.forward_tta, di._second_stage
    monkeypatch.setattr(tta, "forward_tta", lambda model, x: calls.append(tuple(x.shape)) or real(model, x))

    def stage(*a, **k):
        stages.append((k.get("augment", False), real_stage(*a, **k)))
        return stages[-1][1]

    monkeypatch.setattr(di, "_second_stage", stage)
    rng = np.random.default_rng(5)
    H, W = 240, 320
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    dets = [{"bbox": [40.0, 30.0, 120.0, 110.0], "score": 0.5, "category_id": 1},
            {"bbox": [150.0, 60.0, 260.0, 200.0], "score": 0.4, "category_id": 2}]
    out, dt = di.perform_batch_double_inference(img, m, dets, use_augment=True, conf=0.001, return_aligned=True)
    assert calls and len(out) == len(dets) and dt >= 0
    (augment, preds), = stages
    assert augment and len(preds) == len(dets) and any(len(p) for p in preds) and all(p.shape[1] == 6 for p in preds)
    assert all(o is None or len(o["bbox"]) == 4 for o in out)
