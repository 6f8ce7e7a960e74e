"""CPU: the two evaluation kernels of csrc/confusion.hip from the host side -- header, ctypes table and library agree on both symbols,
bad arguments come back as DY_ERR_ARG before any launch -- and a plain numpy restatement of the two rules (``confusion_rule``,
``count_fp_rule``: also the host loop tools/confusion_bench.py times) that reproduces every case of tests/golden/confusion.npz, the
REFERENCE's ConfusionMatrix.process_batch and gt_fails.count_fp.  That pins the fixture and the rule the kernels implement."""
import os
import re

import numpy as np
import pytest

CM_CASES = ("six", "big", "nc1", "nc80")


def box_iou32(lab, det):
    """(n,4) x (m,4) xyxy -> (n,m) in fp32 with the evaluation order of the reference's box_iou."""
    a, b = lab.astype(np.float32)[:, None, :], det.astype(np.float32)[None, :, :]
    iw = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), np.float32(0))
    ih = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), np.float32(0))
    inter = iw * ih
    return inter / ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter + np.float32(1e-7))


def confusion_rule(det, lab, lcls, nc, conf=0.25, iou_thres=0.45, skip_unlabelled=False):
    """One image -> (nc+1, nc+1) counts, [predicted, true], nc = background."""
    m = np.zeros((nc + 1, nc + 1), np.int64)
    det = det[det[:, 4] > np.float32(conf)]
    dcls = det[:, 5].astype(int)
    if len(lcls) == 0:
        if not skip_unlabelled:
            np.add.at(m, (dcls, nc), 1)
        return m
    winner = np.full(len(lcls), -1)
    if len(det):
        iou = box_iou32(lab, det)
        best = np.where(iou > np.float32(iou_thres), iou, -1).argmax(0)  # argmax: the lower label index on a tie
        chose = iou[best, np.arange(len(det))] > np.float32(iou_thres)
        for g in range(len(lcls)):
            cand = np.flatnonzero(chose & (best == g))
            if len(cand):
                winner[g] = cand[iou[g, cand].argmax()]  # the lower detection index on a tie
    for g, c in enumerate(lcls.astype(int)):
        m[dcls[winner[g]] if winner[g] >= 0 else nc, c] += 1
    if (winner >= 0).any():
        lost = np.setdiff1d(np.arange(len(det)), winner[winner >= 0])
        np.add.at(m, (dcls[lost], nc), 1)
    return m


def count_fp_rule(det, labels, w, h, conf=0.25, iou_thr=0.5):
    """One image: detections (n,6) fp32 in stored order, label rows cls xc yc w h (fp64) in file order -> false positives."""
    used, fp = np.zeros(len(labels), bool), 0
    g = np.stack([labels[:, 1] * w - labels[:, 3] * w / 2, labels[:, 2] * h - labels[:, 4] * h / 2, labels[:, 1] * w + labels[:, 3] * w / 2,
                  labels[:, 2] * h + labels[:, 4] * h / 2], 1).reshape(-1, 4)
    gcls = labels[:, 0].astype(int)
    for p in det[det[:, 4] >= np.float32(conf)].astype(np.float64):
        iw = np.maximum(0, np.minimum(p[2], g[:, 2]) - np.maximum(p[0], g[:, 0]))
        ih = np.maximum(0, np.minimum(p[3], g[:, 3]) - np.maximum(p[1], g[:, 1]))
        inter = iw * ih
        iou = inter / (max(0, (p[2] - p[0]) * (p[3] - p[1])) + np.maximum(0, (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])) - inter + 1e-6)
        fit = np.flatnonzero(~used & (gcls == p[5]) & (iou >= iou_thr))
        if len(fit):
            used[fit[0]] = True  # first fit
        else:
            fp += 1
    return fp


def cm_case(G, case):
    return {k: G[f"{case}/{k}"] for k in ("predn", "pred_off", "t_bidx", "t_cls", "t_xywhn", "t_xyxy", "per_image", "matrix_skip0", "matrix_skip1")} | \
        {"nc": int(G[f"{case}/nc"])}


@pytest.mark.parametrize("case", CM_CASES)
def test_numpy_rule_reproduces_the_reference_matrices(golden, case):
    c = cm_case(golden("confusion"), case)
    B, nc = len(c["pred_off"]) - 1, c["nc"]
    tot0, tot1 = np.zeros((nc + 1, nc + 1), np.int64), np.zeros((nc + 1, nc + 1), np.int64)
    for i in range(B):
        det, sel = c["predn"][c["pred_off"][i]:c["pred_off"][i + 1]], c["t_bidx"] == i
        got = confusion_rule(det, c["t_xyxy"][sel], c["t_cls"][sel], nc)
        assert (got == c["per_image"][i]).all(), f"image {i}"
        tot0 += got
        tot1 += confusion_rule(det, c["t_xyxy"][sel], c["t_cls"][sel], nc, skip_unlabelled=True)
    assert (tot0 == c["matrix_skip0"]).all() and (tot1 == c["matrix_skip1"]).all()


def test_fixture_holds_the_situations_it_was_built_for(golden):
    G = golden("confusion")
    c = cm_case(G, "six")
    n_lab = np.bincount(c["t_bidx"].astype(int), minlength=6)
    n_det = np.diff(c["pred_off"])
    assert n_lab[0] > 0 and n_det[0] == 0 and n_lab[1] == 0 and n_det[1] > 0 and c["nc"] == 3
    assert (c["matrix_skip0"] != c["matrix_skip1"]).any() and (c["matrix_skip0"] - c["matrix_skip1"])[:, :3].sum() == 0
    p = c["per_image"]
    assert p[2, :3, :].sum() == 0 and p[2, 3, 1] == 1                      # labels and detections, no pair: no false positive
    assert p[3, 0, 0] == 1 and p[3, 0, 3] == 1                            # the loser of two detections on one label
    assert p[3, 1, 1] == 1 and p[3, 3, 2] == 1                            # one detection over two labels: the larger IoU
    assert p[4, 1, 0] == 1 and p[4, 3, 2] == 1 and p[4, 2, 3] == 1 and p[4].sum() == 3  # off the diagonal; below 0.25 ignored
    big = cm_case(G, "big")
    assert len(big["predn"]) == 300 and len(big["t_cls"]) == 70 and big["matrix_skip0"][:3, :3].sum() > 20
    assert (big["predn"][256:, 4] > 0.25).any()  # kept detections in the block's second pass
    assert cm_case(G, "nc1")["nc"] == 1 and cm_case(G, "nc80")["nc"] == 80
    assert np.diff(G["fp/lab_off"]).tolist() == [0, 2, 1, 1, 2, 2, 70, 130] and G["fp/count"][4] == 1 and G["fp/count"][5] == 0


def test_numpy_rule_reproduces_the_reference_false_positive_counts(golden):
    G = golden("confusion")
    doff, loff = G["fp/det_off"], G["fp/lab_off"]
    got = [count_fp_rule(G["fp/dets"][doff[i]:doff[i + 1]], G["fp/labels"][loff[i]:loff[i + 1]], *G["fp/wh"][i].tolist())
           for i in range(len(G["fp/count"]))]
    assert got == G["fp/count"].tolist() and sum(got) == int(G["fp/total"])


def test_header_binding_and_library_agree():
    import ctypes as C
    from conftest import ROOT
    from ultralytics.hip import SIGNATURES, lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dealyolo_hip.h")).read(), flags=re.S)
    L = lib()
    for name in ("dy_confusion_matrix", "dy_count_fp"):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert decl, f"{name} is not declared"
        params = [p.strip() for p in decl.group(1).split(",")]
        res, args = SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params) and hasattr(L, name)
        for p, a in zip(params, args):
            want = C.c_void_p if ("*" in p or p.startswith("hipStream_t")) else {"int": C.c_int, "float": C.c_float, "double": C.c_double}[p.split()[0]]
            assert a is want, (name, p, a)


def test_entry_points_reject_bad_arguments_without_a_launch():
    from ultralytics.hip import lib
    L = lib()
    cm = lambda predn=8, off=8, n=4, bidx=8, cls=8, box=8, nt=2, geom=8, B=2, nc=3, conf=0.25, iou=0.45, mat=8, st=8: \
        L.dy_confusion_matrix(predn, off, n, bidx, cls, box, nt, geom, B, 640, 640, nc, conf, iou, 1, mat, st, None)
    assert cm(B=0) == -1 and cm(nc=0) == -1 and cm(n=-1) == -1 and cm(nt=-1) == -1
    assert cm(mat=None) == -1 and cm(st=None) == -1
    assert cm(predn=None) == -1 and cm(cls=None) == -1 and cm(box=None) == -1  # detections / labels without their arrays
    assert cm(off=None) == -1 and cm(bidx=None) == -1                          # a batch without offsets / image indices
    assert cm(iou=-0.1) == -1 and cm(iou=float("nan")) == -1 and cm(conf=float("nan")) == -1
    fp = lambda dets=8, doff=8, lab=8, loff=8, wh=8, B=2, conf=0.25, iou=0.5, out=8, st=8: \
        L.dy_count_fp(dets, doff, lab, loff, wh, B, conf, iou, out, st, None)
    assert fp(B=0) == -1 and fp(doff=None) == -1 and fp(loff=None) == -1 and fp(wh=None) == -1 and fp(out=None) == -1 and fp(st=None) == -1
    assert fp(conf=float("nan")) == -1 and fp(iou=float("nan")) == -1


def test_confusion_matrix_object_on_the_host():
    from ultralytics.utils.metrics import ConfusionMatrix
    cm = ConfusionMatrix(nc=3, conf=0.001)
    assert cm.conf == 0.25 and ConfusionMatrix(3, conf=None).conf == 0.25 and ConfusionMatrix(3, conf=0.4).conf == 0.4 and cm.iou_thres == 0.45
    assert cm.matrix.shape == (4, 4) and cm.matrix.dtype == np.float64 and not cm.matrix.any()
    tp, fp = cm.tp_fp()
    assert tp.shape == fp.shape == (3,)
    with pytest.raises(NotImplementedError):
        ConfusionMatrix(nc=3, task="classify")
    with pytest.raises(NotImplementedError):
        cm.plot()
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cm.process_batch(torch.zeros(1, 6), torch.zeros(1, 4), torch.zeros(1))
