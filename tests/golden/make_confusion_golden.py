"""Generate tests/golden/confusion.npz from the REFERENCE implementation: ``ConfusionMatrix.process_batch`` (reference
ultralytics/utils/metrics.py:935-986) image by image, and ``count_fp`` of the reference's gt_fails.py (:35-84).

Run in the build container only (needs the reference tree, which ``_refimport`` locates):

    python tests/golden/make_confusion_golden.py

gt_fails.py runs a Kaggle evaluation when imported, so it is read with ``ast``: only its function definitions and its two numeric
constants are executed, in a namespace where ``YOLO`` is a stand-in whose results are the case's canned boxes; its ``glob`` and label
files point into a temporary directory.  Nothing of the reference's text is stored here.

Confusion cases ``<case>/``: ``predn`` (Ntot, 6) fp32 native-space x1 y1 x2 y2 conf cls, ``pred_off`` (B + 1), the labels as the collate
function gives them (``t_bidx``, ``t_cls``, ``t_xywhn`` fp32, image size 640 x 640, no letterbox padding) and moved to native space with the
validator's fp32 formulas (``t_xyxy``: what the reference was given), ``nc``, and the reference's answers: ``per_image`` (B, nc+1, nc+1),
``matrix_skip0`` (their sum: what direct ``process_batch`` calls give) and ``matrix_skip1`` (the sum over labelled images: what the reference
validator accumulates, val.py:131-152).

  six    one batch of six images, nc = 3: labels without detections; detections without labels; labels and detections with no pair above
         0.45 (no false positive may be counted); two detections on one label (the loser goes to the background column) and one detection
         above 0.45 on two labels (it goes to the larger IoU, the other label to the background row); a wrong-class match (off the
         diagonal) with detections below 0.25 mixed in, one of them exactly on a label; a random image
  big    one image, 300 detections, 70 labels: more than one pass of the 256-thread block, more than one wave of labels
  nc1, nc80   three random images each

False-positive case ``fp/``: ``dets`` (Ntot, 6) fp32, ``det_off``, ``labels`` (Ltot, 5) fp64 rows cls xc yc w h in file order, ``lab_off``, ``wh``
(B, 2) image width and height, ``count`` (B) = the reference's count_fp on each image alone, ``total`` = on all of them.  Images: no label
file; no detections; a class mismatch; a detection at confidence 0.2502 (kept) beside one at 0.2498; first fit against best fit (A
overlaps labels 1 and 2, B only label 1: one false positive) and the same pair in reverse order (none); 70 labels with the only fitting
one in the second chunk of 64; 130 labels with repeated detections on the same label.

Conditions the generator asserts (the reference is undefined otherwise, and the device arithmetic differs from it in the last bits): every
IoU that takes part in a decision is at least 1e-4 from its threshold; within an image all IoUs above 0.3 are pairwise at least 1e-4
apart; every confidence is at least 1e-4 from the confidence threshold.  Random images are redrawn until they meet them.
"""
import ast
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

IMGSZ = 640
MARGIN = 1e-4
CONF, IOU = 0.25, 0.45
FP_CONF, FP_IOU = 0.25, 0.5


# ---- confusion-matrix cases ------------------------------------------------------------------------------------------------------------
def xywhn(boxes_px):
    """Pixel (cx, cy, w, h) rows -> normalised fp32 rows."""
    return (np.asarray(boxes_px, np.float64).reshape(-1, 4) / IMGSZ).astype(np.float32)


def to_native(t):
    """The validator's fp32 formulas at gain 1, padding 0, 640 x 640: xywh2xyxy, * (w, h, w, h), scale_boxes, clip_boxes."""
    t = t.astype(np.float32)
    s, half = np.float32(IMGSZ), np.float32(2)
    dw, dh = t[:, 2] / half, t[:, 3] / half
    out = np.stack([(t[:, 0] - dw) * s, (t[:, 1] - dh) * s, (t[:, 0] + dw) * s, (t[:, 1] + dh) * s], 1)
    return np.clip(out, np.float32(0), s).astype(np.float32)


def det(x1, y1, x2, y2, conf, cls):
    return [x1, y1, x2, y2, conf, cls]


def random_image(rng, n_lab, n_near, n_far, nc):
    """Labels on a jittered grid (they do not overlap), ``n_near`` detections jittered off random labels, ``n_far`` anywhere."""
    cols = int(np.ceil(np.sqrt(max(n_lab, 1) * 1.3)))
    cell = IMGSZ / cols
    cells = rng.permutation(cols * cols)[:n_lab]
    cx = (cells % cols + 0.5) * cell + rng.uniform(-0.1, 0.1, n_lab) * cell
    cy = (cells // cols + 0.5) * cell + rng.uniform(-0.1, 0.1, n_lab) * cell
    w, h = rng.uniform(0.45, 0.75, n_lab) * cell, rng.uniform(0.45, 0.75, n_lab) * cell
    lab = xywhn(np.stack([cx, cy, w, h], 1))
    lcls = rng.integers(0, nc, n_lab).astype(np.float32)
    nat = to_native(lab)
    rows = []
    for _ in range(n_near if n_lab else 0):
        j = int(rng.integers(0, n_lab))
        bw, bh = nat[j, 2] - nat[j, 0], nat[j, 3] - nat[j, 1]
        b = nat[j] + rng.normal(0, 0.09, 4) * np.array([bw, bh, bw, bh])
        c = lcls[j] if rng.random() < 0.7 else rng.integers(0, nc)
        rows.append(det(*b, rng.uniform(0.02, 1.0), c))
    for _ in range(n_far):
        x, y = rng.uniform(0, IMGSZ - 40, 2)
        rows.append(det(x, y, x + rng.uniform(8, 40), y + rng.uniform(8, 40), rng.uniform(0.02, 1.0), rng.integers(0, nc)))
    d = np.array(rows, np.float32).reshape(-1, 6)
    d[:, :4] = np.clip(d[:, :4], 0, IMGSZ)
    d = d[rng.permutation(len(d))]
    return lab, lcls, d


def case_six(rng):
    imgs = []
    # 0: labels, no detections
    imgs.append((xywhn([[120, 90, 60, 40], [400, 300, 100, 120]]), [0, 2], []))
    # 1: detections, no labels
    imgs.append((xywhn([]), [], [det(50, 60, 150, 160, 0.9, 0), det(300, 310, 420, 400, 0.5, 2), det(10, 10, 90, 70, 0.1, 1)]))
    # 2: labels and detections, no pair above 0.45 (IoU 1/3 and 0)
    imgs.append((xywhn([[200, 200, 100, 100]]), [1], [det(200, 150, 300, 250, 0.9, 1), det(500, 500, 560, 580, 0.8, 0)]))
    # 3: two detections on label 0 (IoU 0.905 beats 0.667); one detection on labels 1 (0.778) and 2 (0.6)
    imgs.append((xywhn([[100, 100, 80, 80], [300, 100, 80, 80], [330, 100, 80, 80]]), [0, 1, 2],
                 [det(76, 60, 156, 140, 0.8, 0), det(64, 60, 144, 140, 0.9, 0), det(270, 60, 350, 140, 0.7, 1)]))
    # 4: a wrong-class match; a detection exactly on label 1 but below 0.25; a far one above and a far one below 0.25
    imgs.append((xywhn([[100, 100, 80, 80], [400, 400, 100, 60]]), [0, 2],
                 [det(66, 60, 146, 140, 0.7, 1), det(350, 370, 450, 430, 0.1, 2), det(500, 100, 560, 160, 0.6, 2), det(20, 500, 90, 560, 0.2, 0)]))
    # 5: random
    imgs.append(random_image(rng, 5, 6, 3, 3))
    return imgs, 3


def case_big(rng):
    return [random_image(rng, 70, 45, 255, 3)], 3


def case_nc1(rng):
    return [random_image(rng, 4, 5, 2, 1), random_image(rng, 1, 2, 1, 1), random_image(rng, 6, 4, 4, 1)], 1


def case_nc80(rng):
    return [random_image(rng, 9, 8, 3, 80), random_image(rng, 3, 5, 1, 80), random_image(rng, 12, 10, 5, 80)], 80


CM_CASES = {"six": case_six, "big": case_big, "nc1": case_nc1, "nc80": case_nc80}


def confusion_conditions(ref_metrics, torch, nat, d):
    """False when the reference's answer for this image is not defined with the margins of the module docstring."""
    d = np.asarray(d, np.float32).reshape(-1, 6)
    if len(d) and (np.abs(d[:, 4].astype(np.float64) - CONF) < MARGIN).any():
        return False
    kept = d[d[:, 4] > CONF]
    if not len(kept) or not len(nat):
        return True
    iou = ref_metrics.box_iou(torch.from_numpy(nat), torch.from_numpy(kept[:, :4])).numpy().astype(np.float64)
    if (np.abs(iou - IOU) < MARGIN).any():
        return False
    high = np.sort(iou[iou > 0.3])
    return not (len(high) > 1 and np.diff(high).min() < MARGIN)


def build_confusion(ref_metrics, torch, name, make):
    for attempt in range(200):
        rng = np.random.default_rng([len(name), ord(name[0]), attempt])
        imgs, nc = make(rng)
        if all(confusion_conditions(ref_metrics, torch, to_native(lab), d) for lab, _, d in imgs):
            break
    else:
        raise AssertionError(f"{name}: no draw met the margins")
    B = len(imgs)
    per = np.zeros((B, nc + 1, nc + 1), np.int64)
    for i, (lab, lcls, d) in enumerate(imgs):
        d = np.asarray(d, np.float32).reshape(-1, 6)
        assert confusion_conditions(ref_metrics, torch, to_native(lab), d)
        cm = ref_metrics.ConfusionMatrix(nc=nc, conf=CONF, iou_thres=IOU)
        cm.process_batch(torch.from_numpy(d) if len(d) else None, torch.from_numpy(to_native(lab)), torch.tensor(lcls, dtype=torch.float32))
        per[i] = cm.matrix.astype(np.int64)
        assert (per[i] == cm.matrix).all()
    labelled = np.array([len(lcls) > 0 for _, lcls, _ in imgs])
    out = dict(predn=np.concatenate([np.asarray(d, np.float32).reshape(-1, 6) for _, _, d in imgs], 0),
               pred_off=np.cumsum([0] + [len(d) for _, _, d in imgs]).astype(np.int32),
               t_bidx=np.concatenate([np.full(len(lcls), i, np.float32) for i, (_, lcls, _) in enumerate(imgs)]),
               t_cls=np.concatenate([np.asarray(lcls, np.float32) for _, lcls, _ in imgs]),
               t_xywhn=np.concatenate([lab for lab, _, _ in imgs], 0), nc=np.int32(nc), per_image=per,
               matrix_skip0=per.sum(0), matrix_skip1=per[labelled].sum(0), attempt=np.int32(attempt))
    out["t_xyxy"] = to_native(out["t_xywhn"])
    return out


# ---- false-positive cases -------------------------------------------------------------------------------------------------------------------
def lab_rows(boxes_px, cls, w, h):
    """Pixel x1 y1 x2 y2 rows -> label-file rows cls xc yc w h (fp64)."""
    b = np.asarray(boxes_px, np.float64).reshape(-1, 4)
    return np.stack([np.asarray(cls, np.float64), (b[:, 0] + b[:, 2]) / 2 / w, (b[:, 1] + b[:, 3]) / 2 / h, (b[:, 2] - b[:, 0]) / w,
                     (b[:, 3] - b[:, 1]) / h], 1)


def grid_labels(rng, n, w, h, nc):
    cols = int(np.ceil(np.sqrt(n * 1.3)))
    cw, ch = w / cols, h / cols
    cells = rng.permutation(cols * cols)[:n]
    x1, y1 = (cells % cols + 0.2) * cw, (cells // cols + 0.2) * ch
    return np.stack([x1, y1, x1 + 0.6 * cw, y1 + 0.6 * ch], 1), rng.integers(0, nc, n)


def fp_images():
    rng = np.random.default_rng(77)
    A, Bx = det(115, 100, 215, 200, 0.9, 1), det(80, 100, 180, 200, 0.8, 1)
    two = lab_rows([[100, 100, 200, 200], [120, 100, 220, 200]], [1, 1], 640, 480)
    imgs = [
        ((640, 480), None, [det(10, 10, 100, 100, 0.9, 0), det(200, 200, 300, 280, 0.1, 0), det(400, 100, 500, 220, 0.5, 1)]),
        ((640, 480), lab_rows([[10, 10, 100, 100], [300, 300, 400, 380]], [0, 1], 640, 480), []),
        ((1280, 720), lab_rows([[100, 100, 300, 260]], [2], 1280, 720), [det(100, 100, 300, 260, 0.9, 1)]),
        ((640, 480), lab_rows([[500, 300, 600, 400]], [0], 640, 480), [det(50, 50, 150, 150, 0.2502, 0), det(200, 50, 300, 150, 0.2498, 0)]),
        ((640, 480), two, [A, Bx]),
        ((640, 480), two, [Bx, A]),
    ]
    # 70 labels: the detection sits on label 66; a label of another class lies under it in the first chunk
    box, cls = grid_labels(rng, 70, 1280, 720, 3)
    cls[66] = 1
    box[5], cls[5] = box[66], 2
    d = [det(*(box[66] + [1, -1, 2, 1]), 0.8, 1), det(*(box[66] + [2, 1, -1, 0]), 0.7, 1), det(*(box[20] + [1, 1, 1, 1]), 0.6, (cls[20] + 1) % 3)]
    imgs.append(((1280, 720), lab_rows(box, cls, 1280, 720), d))
    # 130 labels, 60 detections off random labels (repeats find their label used), a third of them of another class
    box, cls = grid_labels(rng, 130, 1280, 720, 4)
    rows = []
    for _ in range(60):
        j = int(rng.integers(0, 130))
        bw, bh = box[j, 2] - box[j, 0], box[j, 3] - box[j, 1]
        c = cls[j] if rng.random() < 0.67 else (cls[j] + 1) % 4
        rows.append(det(*(box[j] + rng.normal(0, 0.07, 4) * [bw, bh, bw, bh]), rng.uniform(0.05, 1.0), c))
    imgs.append(((1280, 720), lab_rows(box, cls, 1280, 720), rows))
    return imgs


def fp_conditions(wh, labels, d):
    d = np.asarray(d, np.float32).reshape(-1, 6)
    assert not len(d) or (np.abs(d[:, 4].astype(np.float64) - FP_CONF) >= MARGIN).all(), "a confidence at the threshold"
    if labels is None or not len(d):
        return
    w, h = wh
    g = np.stack([labels[:, 1] * w - labels[:, 3] * w / 2, labels[:, 2] * h - labels[:, 4] * h / 2, labels[:, 1] * w + labels[:, 3] * w / 2,
                  labels[:, 2] * h + labels[:, 4] * h / 2], 1)
    p = d[:, None, :4].astype(np.float64)
    iw = np.clip(np.minimum(p[..., 2], g[None, :, 2]) - np.maximum(p[..., 0], g[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(p[..., 3], g[None, :, 3]) - np.maximum(p[..., 1], g[None, :, 1]), 0, None)
    inter = iw * ih
    iou = inter / ((p[..., 2] - p[..., 0]) * (p[..., 3] - p[..., 1]) + ((g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]))[None] - inter + 1e-6)
    same = d[:, 5:6].astype(np.float64) == labels[None, :, 0]
    assert (np.abs(iou[same] - FP_IOU) >= MARGIN).all(), "an IoU at the threshold"


def reference_count_fp():
    """The reference's functions, compiled from its file without the module-level evaluation run."""
    import _refimport
    import glob
    tree = ast.parse(open(os.path.join(_refimport.REF, "gt_fails.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) or
            (isinstance(n, ast.Assign) and isinstance(n.value, ast.Constant) and isinstance(n.value.value, (int, float)))]
    ns = {"os": os, "glob": glob, "np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "<reference gt_fails functions>", "exec"), ns)
    assert ns["CONF_THRESH"] == FP_CONF and ns["IOU_THRESH"] == FP_IOU
    return ns


def build_fp(torch):
    ns = reference_count_fp()
    imgs = fp_images()
    canned = {}

    class _Boxes:
        def __init__(self, d):
            t = torch.from_numpy(d)
            self.xyxy, self.conf, self.cls = t[:, :4], t[:, 4], t[:, 5]

    class _Result:
        def __init__(self, wh, d):
            self.orig_shape, self.boxes = (wh[1], wh[0]), _Boxes(d)

    class _Model:
        def __init__(self, path):
            pass

        def __call__(self, img_path, verbose=False):
            return [canned[os.path.basename(img_path)]]

    ns["YOLO"] = _Model
    counts = []
    with tempfile.TemporaryDirectory() as tmp:
        everything = os.path.join(tmp, "all")
        os.makedirs(os.path.join(everything, "images")), os.makedirs(os.path.join(everything, "labels"))
        for i, (wh, labels, d) in enumerate(imgs):
            d = np.asarray(d, np.float32).reshape(-1, 6)
            fp_conditions(wh, labels, d)
            canned[f"im{i:02d}.jpg"] = _Result(wh, d)
            for root in (os.path.join(tmp, f"one{i}"), everything):
                os.makedirs(os.path.join(root, "images"), exist_ok=True), os.makedirs(os.path.join(root, "labels"), exist_ok=True)
                open(os.path.join(root, "images", f"im{i:02d}.jpg"), "w").close()
                if labels is not None:
                    with open(os.path.join(root, "labels", f"im{i:02d}.txt"), "w") as f:
                        f.writelines(f"{int(r[0])} {r[1]!r} {r[2]!r} {r[3]!r} {r[4]!r}\n" for r in labels.tolist())
            counts.append(ns["count_fp"]("stand-in.pt", os.path.join(tmp, f"one{i}", "images"), os.path.join(tmp, f"one{i}", "labels")))
        total = ns["count_fp"]("stand-in.pt", os.path.join(everything, "images"), os.path.join(everything, "labels"))
    assert total == sum(counts)
    labs = [np.zeros((0, 5)) if l is None else l for _, l, _ in imgs]
    return dict(dets=np.concatenate([np.asarray(d, np.float32).reshape(-1, 6) for _, _, d in imgs], 0),
                det_off=np.cumsum([0] + [len(d) for _, _, d in imgs]).astype(np.int32), labels=np.concatenate(labs, 0).astype(np.float64),
                lab_off=np.cumsum([0] + [len(l) for l in labs]).astype(np.int32), wh=np.array([wh for wh, _, _ in imgs], np.int32),
                count=np.array(counts, np.int32), total=np.int32(total))


def main():
    import _refimport
    _refimport.install()
    import torch
    from ultralytics.utils import metrics as ref_metrics
    assert ref_metrics.__file__.startswith(_refimport.REF)
    arrs = {}
    for name, make in CM_CASES.items():
        c = build_confusion(ref_metrics, torch, name, make)
        for k, v in c.items():
            arrs[f"{name}/{k}"] = v
        print(name, "images", len(c["pred_off"]) - 1, "detections", len(c["predn"]), "labels", len(c["t_cls"]), "draw", int(c["attempt"]),
              "counts", int(c["matrix_skip0"].sum()), "matched", int(c["matrix_skip0"][:-1, :-1].sum()))
        if int(c["nc"]) <= 3:
            print(c["matrix_skip0"], c["matrix_skip1"], sep="\n")
    f = build_fp(torch)
    for k, v in f.items():
        arrs[f"fp/{k}"] = v
    print("fp", "count", f["count"].tolist(), "total", int(f["total"]))
    path = os.path.join(HERE, "confusion.npz")
    np.savez_compressed(path, **arrs)
    assert os.path.getsize(path) < 1 << 20
    print(f"confusion.npz  {os.path.getsize(path) / 1024:.1f} KiB  ({len(arrs)} arrays)")


if __name__ == "__main__":
    main()
