"""CPU: the host half of test-time augmentation (ultralytics/hip/tta.py; reference nn/tasks.py:335-371, utils/torch_utils.py:355-366).

The pass geometry -- scaled size, padded size, the columns _clip_augmented keeps -- is pinned against a literal restatement of the
reference's arithmetic and against what the reference recorded in tests/golden/tta.npz; ``augment=True`` outside eval mode raises."""
import math
import os

import pytest
import torch

from conftest import CFG_DIR


def _restated(H, W, gs, nl, As):
    """scale_img / _clip_augmented as the reference writes them, on shapes only."""
    out = []
    for si in (1, 0.83, 0.67):
        if si == 1.0:
            out.append((H, W, H, W))
            continue
        s = (int(H * si), int(W * si))
        h, w = (math.ceil(x * si / gs) * gs for x in (H, W))
        out.append((s[0], s[1], h, w))
    y = [torch.zeros(A) for A in As]
    idx = [torch.arange(A) for A in As]
    g = sum(4 ** x for x in range(nl))
    i = (y[0].shape[-1] // g) * sum(4 ** x for x in range(1))
    idx[0] = idx[0][..., :-i]
    i = (y[-1].shape[-1] // g) * sum(4 ** (nl - 1 - x) for x in range(1))
    idx[-1] = idx[-1][..., i:]
    cols = [(int(t[0]), int(t[-1]) + 1) if len(t) else (0, 0) for t in idx]
    return out, cols


def _anchors(Hp, Wp, strides):
    return sum((Hp // s) * (Wp // s) for s in strides)


@pytest.mark.parametrize("gs,nl,strides", [(16, 3, (4, 8, 16)), (32, 4, (4, 8, 16, 32)), (32, 3, (8, 16, 32))])
def test_geometry_matches_reference_arithmetic(gs, nl, strides):
    from ultralytics.hip.tta import tta_geometry
    sizes = [(640, 640), (1280, 1280), (480, 640), (64, 64), (96, 128), (160, 160), (17, 33), (331, 517), (100, 37), (1, 5), (47, 641)]
    for H, W in sizes:
        geo = tta_geometry(H, W, gs, nl)
        As = [_anchors(p["Hp"], p["Wp"], strides) for p in geo]
        want, cols = _restated(H, W, gs, nl, As)
        geo = tta_geometry(H, W, gs, nl, As)
        assert [(p["Ho"], p["Wo"], p["Hp"], p["Wp"]) for p in geo] == want, (H, W)
        assert [p["cols"] for p in geo] == cols, (H, W, As)
        assert [(p["scale"], p["flip"]) for p in geo] == [(1, 0), (0.83, 3), (0.67, 0)]
    # the issue's worked example: 640 -> 531 padded to 544 (gs 16 and 32), 428 padded to 432 (gs 16) or 448 (gs 32)
    geo = tta_geometry(640, 640, gs, nl)
    assert (geo[1]["Ho"], geo[1]["Hp"]) == (531, 544)
    assert (geo[2]["Ho"], geo[2]["Hp"]) == (428, 432 if gs == 16 else 448)


def test_kept_columns_is_a_count_not_a_level():
    """_clip_augmented slices by column counts: with fewer than g anchors the first pass keeps NOTHING (``[..., :-0]``), and the
    last pass's cut may exceed what a level holds."""
    from ultralytics.hip.tta import kept_columns
    assert kept_columns([20, 20, 20], 3) == [(0, 0), (0, 20), (0, 20)]
    assert kept_columns([336, 336, 189], 3) == [(0, 320), (0, 336), (144, 189)]
    assert kept_columns([340, 340, 340], 4) == [(0, 336), (0, 340), (256, 340)]
    assert kept_columns([85, 85, 170], 4) == [(0, 84), (0, 85), (128, 170)]


def test_geometry_matches_fixture(golden):
    from ultralytics.hip.tta import tta_geometry
    g = golden("tta")
    cases = sorted({k.split("/")[0] for k in g.keys() if not k.startswith("img/")})
    assert len(cases) == 5
    for c in cases:
        B, _, H, W = g["img/" + str(g[c + "/img"])].shape
        gs, nl, A = int(g[c + "/gs"]), int(g[c + "/nl"]), [int(a) for a in g[c + "/A"]]
        geo = tta_geometry(H, W, gs, nl, A)
        assert [[p["Hp"], p["Wp"]] for p in geo] == g[c + "/hw"].tolist(), c
        assert [list(p["cols"]) for p in geo] == g[c + "/cols"].tolist(), c
        assert g[c + "/y"].shape == (B, g[c + "/y"].shape[1], sum(hi - lo for lo, hi in g[c + "/cols"].tolist())), c
    assert int(g["asf_p2p2_64/gs"]) == 16 and int(g["p2_64/gs"]) == 32


def test_augment_in_training_mode_raises():
    from ultralytics.nn.tasks import DetectionModel
    m = DetectionModel(os.path.join(CFG_DIR, "yolov8n-ASF-P2P2.yaml"), ch=3, verbose=False)
    m.train()
    with pytest.raises(NotImplementedError, match="eval"):
        m(torch.zeros(1, 3, 64, 64), augment=True)
    with pytest.raises(NotImplementedError, match="eval"):
        m.predict(torch.zeros(1, 3, 64, 64), augment=True)
