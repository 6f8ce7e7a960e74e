"""Generate tests/golden/two_stage_eval.npz from the REFERENCE script's own evaluation functions.

Run where the reference tree exists (the build container; _refimport.REF, overridden by DEALYOLO_REFERENCE):

    python tests/golden/make_two_stage_eval_golden.py

In the manner of make_golden.py:gen_two_stage: double_inference.py is a Kaggle script whose import has side effects, so only the
definitions of calculate_iou_tensor, calculate_metrics_optimized, load_ground_truth and load_image_predictions are compiled -- read from
the reference tree at generation time with their decorators stripped (@torch.jit.script: same arithmetic, eager), nothing is copied --
and called on seeded inputs.  The fixture holds those inputs and the recorded outputs only.
"""
import ast
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, ROOT]
import _refimport  # noqa: E402  (only for the location of the reference tree; nothing of it is imported)
from oracle import two_stage as ots  # noqa: E402

REF = _refimport.REF
WANT = {"calculate_iou_tensor", "calculate_metrics_optimized", "load_ground_truth", "load_image_predictions"}
CASES = ((0, 3), (4, 0), (1, 1), (7, 5), (40, 12), (300, 60))  # (predictions, labels)
THRESHOLDS = (0.25, 0.45, 0.5)  # refinement filter, NMS, match: no IoU of the fixture may come near one of them
MARGIN = 1e-4
W, H = 900, 600


def reference_functions():
    tree = ast.parse(open(os.path.join(REF, "double_inference.py")).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANT]
    assert {f.name for f in fns} == WANT
    for f in fns:
        f.decorator_list = []
    ns = {"torch": torch, "np": np, "os": os, "json": json}
    exec(compile(ast.Module(body=fns, type_ignores=[]), "double_inference.py", "exec"), ns)
    return ns


def pair_ious(a, b):
    """All IoUs of (n,4) x (m,4) in float32, calculate_iou_tensor's formula vectorised: only to keep every IoU away from the thresholds."""
    a, b = a.astype(np.float32)[:, None], b.astype(np.float32)[None]
    iw = np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0])
    ih = np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1])
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0).astype(np.float32)
    union = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1), 0)


def greedy_case(rng, n_pred, n_lab):
    """Labels of 10-80 px; predictions = jittered copies (sigma 6 px) of the labels in turn, class wrong with probability 0.2; one pair
    of identical predictions and one pair of identical labels (equal IoU to whatever meets them: the tie goes to the first)."""
    c = np.stack([rng.uniform(60, W - 60, n_lab), rng.uniform(60, H - 60, n_lab)], 1)
    wh = rng.uniform(10, 80, (n_lab, 2))
    lab_boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    lab_cls = rng.integers(0, 3, n_lab)
    if n_lab >= 5:
        lab_boxes[3], lab_cls[3] = lab_boxes[1], lab_cls[1]
    if n_lab:
        src = np.arange(n_pred) % n_lab
        boxes = (lab_boxes[src] + rng.normal(0, 6, (n_pred, 4))).astype(np.float32)
        cls = np.where(rng.random(n_pred) < 0.2, (lab_cls[src] + 1) % 3, lab_cls[src])
    else:
        c = np.stack([rng.uniform(60, W - 60, n_pred), rng.uniform(60, H - 60, n_pred)], 1)
        wh = rng.uniform(10, 80, (n_pred, 2))
        boxes, cls = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32), rng.integers(0, 3, n_pred)
    scores = rng.uniform(0.25, 1, n_pred).astype(np.float32)
    if n_pred >= 7:
        boxes[5], cls[5] = boxes[2], cls[2]
    return boxes, scores, cls.astype(np.int64), lab_boxes, lab_cls.astype(np.int64)


def clear_of_thresholds(boxes, lab_boxes):
    ious = np.concatenate([pair_ious(boxes, lab_boxes).ravel(), pair_ious(boxes, boxes).ravel()])
    return all((np.abs(ious - t) > MARGIN).all() for t in THRESHOLDS)


def main():
    ns = reference_functions()
    arrs = {"greedy/n": len(CASES), "greedy/sizes": np.array(CASES)}
    seed = 31
    for k, (n_pred, n_lab) in enumerate(CASES):
        while True:
            case = greedy_case(np.random.default_rng(seed), n_pred, n_lab)
            seed += 1
            if clear_of_thresholds(case[0], case[3]):
                break
        boxes, scores, cls, lab_boxes, lab_cls = case
        assert clear_of_thresholds(boxes, lab_boxes), "an IoU of the fixture lies within 1e-4 of a threshold"
        t = lambda a, dt=torch.float32: torch.tensor(a, dtype=dt)  # noqa: E731
        counts = ns["calculate_metrics_optimized"](t(boxes), t(scores), t(cls, torch.int64), t(lab_boxes), t(lab_cls, torch.int64), 0.5)
        keep = np.array(ots.nms_per_class(boxes, scores, cls, 0.45), np.int64)
        kept = ns["calculate_metrics_optimized"](t(boxes[keep]), t(scores[keep]), t(cls[keep], torch.int64), t(lab_boxes), t(lab_cls, torch.int64), 0.5)
        arrs.update({f"greedy/{k}/boxes": boxes, f"greedy/{k}/scores": scores, f"greedy/{k}/labels": cls, f"greedy/{k}/lab_boxes": lab_boxes,
                     f"greedy/{k}/lab_cls": lab_cls, f"greedy/{k}/counts": np.array([int(v) for v in counts]),
                     f"greedy/{k}/keep": keep, f"greedy/{k}/counts_kept": np.array([int(v) for v in kept])})
        print(f"case {k} ({n_pred}, {n_lab}): tp fp fn {[int(v) for v in counts]}; after NMS {len(keep)} rows {[int(v) for v in kept]}")
    # label files: a short line, a blank line, an empty file, a missing file
    label_files = {"a": "0 0.5 0.5 0.2 0.1\n1 0.25 0.75 0.1 0.3\n", "b": "2 0.1 0.2 0.05 0.07\n0 0.3 0.3\n\n1 0.9 0.8 0.15 0.25\n", "c": ""}
    sizes = {"a": (640, 480), "b": (53, 37), "c": (100, 100), "missing": (64, 64)}  # (width, height)
    with tempfile.TemporaryDirectory() as tmp:
        for stem, txt in label_files.items():
            with open(os.path.join(tmp, stem + ".txt"), "w") as f:
                f.write(txt)
        for stem, (w, h) in sizes.items():
            boxes, labels = ns["load_ground_truth"](os.path.join(tmp, stem + ".txt"), w, h)
            arrs[f"labels/{stem}/text"] = np.array(label_files.get(stem, ""))
            arrs[f"labels/{stem}/wh"] = np.array([w, h])
            arrs[f"labels/{stem}/boxes"] = np.array(boxes, np.float64).reshape(-1, 4)
            arrs[f"labels/{stem}/boxes_f32"] = torch.tensor(boxes).reshape(-1, 4).numpy()  # what main builds its targets from
            arrs[f"labels/{stem}/labels"] = np.array(labels, np.int64)
        # predictions JSON: a record below the threshold, an image with records only below it
        records = [{"image_id": "a", "category_id": 0, "bbox": [10.5, 20.25, 30.0, 40.125], "score": 0.9},
                   {"image_id": "a", "category_id": 2, "bbox": [100.0, 50.0, 12.5, 8.0], "score": 0.1},
                   {"image_id": "b", "category_id": 1, "bbox": [1.0, 2.0, 3.0, 4.0], "score": 0.05},
                   {"image_id": "b", "category_id": 1, "bbox": [5.0, 6.0, 7.0, 8.0], "score": 0.2},
                   {"image_id": "a", "category_id": 1, "bbox": [0.0, 0.0, 639.999, 479.5], "score": 0.25},
                   {"image_id": "c", "category_id": 0, "bbox": [33.333, 44.444, 5.555, 6.666], "score": 0.31234}]
        path = os.path.join(tmp, "predictions.json")
        with open(path, "w") as f:
            json.dump(records, f)
        parsed = ns["load_image_predictions"](path, 0.25)
    arrs["json/text"] = np.array(json.dumps(records))
    arrs["json/stems"] = np.array(list(parsed))
    for stem, p in parsed.items():
        arrs[f"json/{stem}/boxes"] = np.array(p["boxes"], np.float64).reshape(-1, 4)
        arrs[f"json/{stem}/scores"] = np.array(p["scores"], np.float64)
        arrs[f"json/{stem}/labels"] = np.array(p["labels"], np.int64)
    out = os.path.join(HERE, "two_stage_eval.npz")
    np.savez_compressed(out, **arrs)
    print(f"two_stage_eval.npz  {os.path.getsize(out) / 1024:.1f} KiB  ({len(arrs)} arrays)")


if __name__ == "__main__":
    main()
