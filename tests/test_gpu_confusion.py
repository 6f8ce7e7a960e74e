"""-m gpu: the evaluation kernels of csrc/confusion.hip (dy_confusion_matrix, dy_count_fp) against tests/golden/confusion.npz -- the
REFERENCE's ConfusionMatrix.process_batch and gt_fails.count_fp -- directly, through ``ConfusionMatrix.process_batch``, through
``DetectionValidator`` and through ``ultralytics.utils.gt_fails.count_fp`` with a stub model.  Integer counts: every comparison is exact.
(The fixture's cases keep every IoU 1e-4 from its threshold: tests/golden/make_confusion_golden.py.)"""
import os

import numpy as np
import pytest
import torch

from test_host_confusion import CM_CASES, cm_case

pytestmark = pytest.mark.gpu


def t(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def launch(c, skip, matrix=None, native=True):
    """One dy_confusion_matrix launch on a fixture case: native xyxy labels (no geometry table) or the collate-format labels with the
    identity geometry of a 640 x 640 image."""
    from ultralytics.hip import lib
    B, nc = len(c["pred_off"]) - 1, c["nc"]
    keep = [t(c["predn"]), t(c["pred_off"], torch.int32), t(c["t_bidx"]), t(c["t_cls"]), t(c["t_xyxy"] if native else c["t_xywhn"]),
            t(np.tile(np.array([1, 0, 0, 640, 640], np.float32), (B, 1)))]
    matrix = torch.zeros((nc + 1, nc + 1), dtype=torch.int32, device="cuda") if matrix is None else matrix
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ptr = lambda x: x.data_ptr() if x.numel() else 0
    rc = lib().dy_confusion_matrix(ptr(keep[0]), keep[1].data_ptr(), len(c["predn"]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), len(c["t_cls"]),
                                   0 if native else keep[5].data_ptr(), B, 640, 640, nc, 0.25, 0.45, skip, matrix.data_ptr(), status.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return matrix, int(status.item())


@pytest.mark.parametrize("case", CM_CASES)
def test_kernel_matches_the_reference_matrices(golden, case):
    c = cm_case(golden("confusion"), case)
    for native in (True, False):
        for skip in (0, 1):
            m, st = launch(c, skip, native=native)
            print(case, "native" if native else "collate", "skip", skip, "differing cells", int((m.cpu().numpy() != c[f"matrix_skip{skip}"]).sum()))
            assert st == 0 and (m.cpu().numpy() == c[f"matrix_skip{skip}"]).all()


def test_second_launch_adds_to_the_same_matrix(golden):
    c = cm_case(golden("confusion"), "six")
    m, _ = launch(c, 1)
    m, st = launch(c, 1, matrix=m)
    assert st == 0 and (m.cpu().numpy() == 2 * c["matrix_skip1"]).all()


@pytest.mark.parametrize("case", ["six", "nc80"])
def test_process_batch_image_by_image_equals_the_batched_launch(golden, case):
    from ultralytics.utils.metrics import ConfusionMatrix
    c = cm_case(golden("confusion"), case)
    cm = ConfusionMatrix(nc=c["nc"], conf=0.001)  # the validator's default confidence: means 0.25
    for i in range(len(c["pred_off"]) - 1):
        det, sel = c["predn"][c["pred_off"][i]:c["pred_off"][i + 1]], c["t_bidx"] == i
        one = ConfusionMatrix(nc=c["nc"])
        for obj in (cm, one):
            obj.process_batch(t(det) if len(det) else None, t(c["t_xyxy"][sel]).reshape(-1, 4), t(c["t_cls"][sel]))
        assert (one.matrix == c["per_image"][i]).all(), f"image {i}"
    batched, _ = launch(c, 0)
    assert cm.matrix.dtype == np.float64 and (cm.matrix == batched.cpu().numpy()).all() and (cm.matrix == c["matrix_skip0"]).all()
    tp, fp = cm.tp_fp()
    assert (tp == np.diag(c["matrix_skip0"])[:-1]).all() and (fp == (c["matrix_skip0"].sum(1) - np.diag(c["matrix_skip0"]))[:-1]).all()


def _validator(plots, nc):
    from ultralytics.models.yolo.detect import DetectionValidator
    v = DetectionValidator(args=dict(plots=plots))
    v.device = torch.device("cuda:0")

    class _Model:
        names = {i: str(i) for i in range(nc)}

    v.init_metrics(_Model())
    return v


def _batch(c):
    tb = dict(batch_idx=t(c["t_bidx"]), cls=t(c["t_cls"]).reshape(-1, 1), bboxes=t(c["t_xywhn"]))
    tb["img"] = torch.zeros(len(c["pred_off"]) - 1, 3, 640, 640, device="cuda")
    return tb


def test_validator_fills_the_confusion_matrix_and_leaves_tp_alone(golden):
    """The six-image batch at 640 x 640 without letterbox padding: the network-input predictions ARE the native ones."""
    c = cm_case(golden("confusion"), "six")
    preds = [t(c["predn"][c["pred_off"][i]:c["pred_off"][i + 1]]) for i in range(6)]
    on, off = _validator(True, 3), _validator(False, 3)
    tp_on, tp_off = on.update_metrics(preds, _batch(c)), off.update_metrics(preds, _batch(c))
    assert torch.equal(tp_on, tp_off) and torch.equal(on.last_predn, off.last_predn) and on.seen == off.seen == 6
    for k in on.stats:
        assert torch.equal(on.stats[k][0], off.stats[k][0])
    res_on, res_off = on.get_stats(), off.get_stats()
    assert res_on == res_off
    assert on.metrics.confusion_matrix is on.confusion_matrix and (on.metrics.confusion_matrix.matrix == c["matrix_skip1"]).all()
    assert not off.metrics.confusion_matrix.matrix.any()  # plots=False: created, never filled
    on.update_metrics(preds, _batch(c))  # the counter persists over the run ...
    assert (on.confusion_matrix.matrix == 2 * c["matrix_skip1"]).all()
    on.init_metrics(type("M", (), {"names": {i: str(i) for i in range(3)}})())  # ... and a new run starts from zero
    assert not on.confusion_matrix.matrix.any()


def test_more_than_1024_labels_in_one_image_raises():
    from ultralytics.utils.metrics import ConfusionMatrix
    rng = np.random.default_rng(3)
    n = 1025
    xy = rng.uniform(0, 600, (n, 2)).astype(np.float32)
    box = np.concatenate([xy, xy + 20], 1)
    cm = ConfusionMatrix(nc=2)
    cm.process_batch(t(np.array([[0, 0, 20, 20, 0.9, 1]])), t(box), t(rng.integers(0, 2, n)))
    with pytest.raises(RuntimeError, match="1024 labels"):
        cm.matrix
    ok = ConfusionMatrix(nc=2)
    ok.process_batch(t(np.array([[0, 0, 20, 20, 0.9, 1]])), t(box[:1024]), t(np.zeros(1024)))
    assert ok.matrix.sum() >= 1024
    # the validator: labels only (no detection, so dy_match_predictions does not run), get_stats raises
    v = _validator(True, 2)
    lab = np.concatenate([(xy + 10) / 640, np.full((n, 2), 20 / 640, np.float32)], 1)
    tb = dict(batch_idx=t(np.zeros(n)), cls=t(rng.integers(0, 2, (n, 1))), bboxes=t(lab), img=torch.zeros(1, 3, 640, 640, device="cuda"))
    v.update_metrics([torch.zeros((0, 6), device="cuda")], tb)
    with pytest.raises(RuntimeError, match="1024 labels"):
        v.get_stats()
    bad = ConfusionMatrix(nc=2)
    bad.process_batch(t(np.array([[0, 0, 20, 20, 0.9, 2]])), t(box[:0]).reshape(-1, 4), t(np.zeros(0)))  # class 2 of 2
    with pytest.raises(RuntimeError, match="outside"):
        bad.matrix


def _count_fp_kernel(G, order=None):
    from ultralytics.hip import lib
    doff, loff = G["fp/det_off"], G["fp/lab_off"]
    B = len(G["fp/count"])
    keep = [t(G["fp/dets"]), t(doff, torch.int32), t(G["fp/labels"], torch.float64), t(loff, torch.int32), t(G["fp/wh"], torch.int32)]
    fp = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = lib().dy_count_fp(*[k.data_ptr() for k in keep], B, 0.25, 0.5, fp.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return fp.cpu().numpy(), int(status.item())


def test_count_fp_kernel_matches_the_reference(golden):
    G = golden("confusion")
    fp, st = _count_fp_kernel(G)
    print("fp", fp.tolist(), "reference", G["fp/count"].tolist())
    assert st == 0 and (fp == G["fp/count"]).all()
    assert fp[4] == 1 and fp[5] == 0  # first fit: the order of the detections decides


def test_count_fp_more_than_1024_labels_sets_the_flag():
    from ultralytics.hip import lib
    lab = np.tile(np.array([[0, 0.5, 0.5, 0.1, 0.1]]), (1025, 1))
    keep = [t(np.array([[10, 10, 20, 20, 0.9, 0]])), t([0, 1], torch.int32), t(lab, torch.float64), t([0, 1025], torch.int32), t([[640, 480]], torch.int32)]
    fp, status = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib().dy_count_fp(*[k.data_ptr() for k in keep], 1, 0.25, 0.5, fp.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert int(status.item()) == 1 and int(fp.item()) == 1


def test_count_fp_through_a_stub_model(golden, tmp_path):
    """``count_fp`` on a folder of (empty) image files with label files written from the fixture; the stub's ``predict`` returns the canned
    detections as device-resident ``Results``.  Batches of 3: three launches, one read-back."""
    from ultralytics.engine.results import Results
    from ultralytics.utils.gt_fails import count_fp
    G = golden("confusion")
    doff, loff, wh = G["fp/det_off"], G["fp/lab_off"], G["fp/wh"]
    B = len(G["fp/count"])
    os.makedirs(tmp_path / "images"), os.makedirs(tmp_path / "labels")
    canned = {}
    for i in range(B):
        f = str(tmp_path / "images" / f"im{i:02d}.jpg")
        open(f, "w").close()
        rows = G["fp/labels"][loff[i]:loff[i + 1]]
        if len(rows):  # image 0 has no label file
            with open(tmp_path / "labels" / f"im{i:02d}.txt", "w") as fh:
                fh.writelines(f"{int(r[0])} {r[1]!r} {r[2]!r} {r[3]!r} {r[4]!r}\n" for r in rows.tolist())
        canned[f] = (np.zeros((int(wh[i, 1]), int(wh[i, 0]), 3), np.uint8), t(G["fp/dets"][doff[i]:doff[i + 1]]).reshape(-1, 6))
    (tmp_path / "images" / "notes.png").write_bytes(b"")  # not a *.jpg: ignored, as by the script

    class Stub:
        calls = []

        def predict(self, source, conf, batch, verbose=False):
            self.calls.append((len(source), conf, batch))
            return [Results(canned[f][0], path=f, names={}, boxes=canned[f][1]) for f in source]

    total, per_image = count_fp(Stub(), str(tmp_path / "images"), str(tmp_path / "labels"), batch=3)
    assert total == int(G["fp/total"]) and list(per_image) == sorted(canned)
    assert [per_image[f] for f in sorted(canned)] == G["fp/count"].tolist()
    assert Stub.calls == [(3, 0.25, 3), (3, 0.25, 3), (2, 0.25, 2)]
    assert count_fp(Stub(), str(tmp_path / "labels"), str(tmp_path / "labels")) == (0, {})
