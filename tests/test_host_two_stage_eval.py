"""CPU: the host half of the dataset-level two-stage evaluation (ultralytics/utils/double_inference.py: predictions JSON, label reader,
chunk bookkeeping, scoring rules) against tests/golden/two_stage_eval.npz -- outputs of the reference script's own functions
(tests/golden/make_two_stage_eval_golden.py) -- and the numpy restatement of dy_two_stage_merge that tests/test_gpu_two_stage_eval.py
measures the kernel with."""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

from oracle import two_stage as ots

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "two_stage_eval.npz"))


def merge_reference(rows, refined, found, slot_row, aligned, nms_iou, labels, match_iou):
    """What dy_two_stage_merge does for ONE image, step by step as process_image_optimized :430-444 and calculate_metrics_optimized
    :306-333 do it.  rows (n,6); refined (k,6) / found (k) per crop; slot_row (k) image-local row of each crop slot; labels (m,5)
    cls x1 y1 x2 y2.  -> (rows after the replacements, keep mask, (tp, fp, fn))."""
    rows = np.array(rows, np.float32).reshape(-1, 6).copy()
    labels = np.asarray(labels, np.float32).reshape(-1, 5)
    hits = [k for k in range(len(found)) if found[k]]
    for j, k in enumerate(hits):  # 1. apply: aligned -> the crop's own row; the script's zip -> the j-th found one takes slot j
        rows[slot_row[k if aligned else j]] = refined[k]
    keep = np.ones(len(rows), bool)  # 2. per-class greedy NMS
    if nms_iou >= 0 and len(rows):
        keep[:] = False
        keep[ots.nms_per_class(rows[:, :4], rows[:, 4], rows[:, 5].astype(int), nms_iou)] = True
    matched = np.zeros(len(labels), bool)  # 3. greedy count over the kept rows in stored order
    tp = 0
    for r in rows[keep]:
        best, best_j = 0.0, -1
        for j in range(len(labels)):
            if matched[j] or labels[j, 0] != r[5]:
                continue
            iou = ots.calculate_iou(r[:4], labels[j, 1:])
            if iou > best and iou >= match_iou:
                best, best_j = iou, j
        if best_j >= 0:
            tp += 1
            matched[best_j] = True
    return rows, keep, (tp, int(keep.sum()) - tp, len(labels) - tp)


def greedy_case(k):
    rows = np.concatenate([G[f"greedy/{k}/boxes"].reshape(-1, 4), G[f"greedy/{k}/scores"].reshape(-1, 1),
                           G[f"greedy/{k}/labels"].reshape(-1, 1).astype(np.float32)], 1).astype(np.float32)
    labels = np.concatenate([G[f"greedy/{k}/lab_cls"].reshape(-1, 1).astype(np.float32), G[f"greedy/{k}/lab_boxes"].reshape(-1, 4)], 1).astype(np.float32)
    return rows, labels


def test_merge_restatement_agrees_with_the_reference_counts():
    """Pins the yardstick of the GPU test: the restatement's greedy count equals calculate_metrics_optimized on every fixture case, on
    all rows and on the rows a 0.45 NMS keeps; the fixture's construction makes tp, fp and fn all non-trivial."""
    assert [tuple(s) for s in G["greedy/sizes"]] == [(0, 3), (4, 0), (1, 1), (7, 5), (40, 12), (300, 60)]
    none = np.zeros((0, 6), np.float32)
    for k in range(int(G["greedy/n"])):
        rows, labels = greedy_case(k)
        _, keep, counts = merge_reference(rows, none, [], [], True, -1.0, labels, 0.5)
        assert keep.all() and counts == tuple(G[f"greedy/{k}/counts"]), k
        _, keep, counts = merge_reference(rows, none, [], [], True, 0.45, labels, 0.5)
        assert np.array_equal(np.where(keep)[0], G[f"greedy/{k}/keep"]) and counts == tuple(G[f"greedy/{k}/counts_kept"]), k
    assert tuple(G["greedy/0/counts"]) == (0, 0, 3) and tuple(G["greedy/1/counts"]) == (0, 4, 0)  # the two early returns
    assert min(G["greedy/5/counts"]) > 0 and min(G["greedy/5/counts_kept"]) > 0


def test_load_image_predictions_matches_the_reference(tmp_path):
    from ultralytics.utils.double_inference import load_image_predictions
    path = tmp_path / "predictions.json"
    path.write_text(str(G["json/text"]))
    out = load_image_predictions(str(path), 0.25)
    assert list(out) == [str(s) for s in G["json/stems"]] == ["a", "b", "c"]
    for stem, p in out.items():
        assert np.array_equal(np.array(p["boxes"], np.float64).reshape(-1, 4), G[f"json/{stem}/boxes"])
        assert np.array_equal(np.array(p["scores"], np.float64), G[f"json/{stem}/scores"]) and p["labels"] == G[f"json/{stem}/labels"].tolist()
    assert len(out["a"]["scores"]) == 2          # the 0.1 record is dropped, the 0.25 one (>=) stays
    assert out["b"] == {"boxes": [], "scores": [], "labels": []}  # only records below the threshold: an empty entry
    try:
        load_image_predictions(str(tmp_path / "nothing.json"))
        raise AssertionError("a missing file must raise")
    except FileNotFoundError:
        pass


def test_label_reader_matches_the_reference(tmp_path):
    from ultralytics.utils.double_inference import ground_truth_rows, load_ground_truth
    for stem in ("a", "b", "c", "missing"):
        path = tmp_path / f"{stem}.txt"
        if stem != "missing":
            path.write_text(str(G[f"labels/{stem}/text"]))
        w, h = [int(v) for v in G[f"labels/{stem}/wh"]]
        boxes, labels = load_ground_truth(str(path), w, h)
        assert np.array_equal(np.array(boxes, np.float64).reshape(-1, 4), G[f"labels/{stem}/boxes"])  # float64, the script's operation order
        assert labels == G[f"labels/{stem}/labels"].tolist()
        rows = ground_truth_rows(str(path), w, h)
        assert rows.dtype == np.float32 and np.array_equal(rows[:, 1:], G[f"labels/{stem}/boxes_f32"]) and rows[:, 0].tolist() == labels
    assert len(G["labels/b/labels"]) == 2        # the three-field line and the blank line are skipped
    assert len(G["labels/c/labels"]) == 0 and len(G["labels/missing/labels"]) == 0


def test_predictions_json_round_trip(tmp_path):
    """predictions_to_json rounds the top-left xywh box to 3 decimals and the score to 5 (pred_to_json); load_image_predictions adds
    x + w back.  So x1, y1 return within 0.5e-3, x2, y2 within 1e-3 (two roundings) plus fp32 noise, scores within 0.5e-5; classes and
    the record order are exact, and a score that rounds below the threshold is the reader's to drop."""
    from ultralytics.utils.double_inference import load_image_predictions, predictions_to_json
    rng = np.random.default_rng(3)
    results, files, want = [], [], {}
    for i, n in enumerate((5, 0, 2)):
        xy = rng.uniform(0, 500, (n, 2))
        d = np.concatenate([xy, xy + rng.uniform(2, 100, (n, 2)), rng.uniform(0.3, 1, (n, 1)), rng.integers(0, 3, (n, 1))], 1).astype(np.float32)
        results.append(SimpleNamespace(boxes=SimpleNamespace(data=torch.from_numpy(d))))
        files.append(str(tmp_path / "images" / f"img_{i}.png"))
        want[f"img_{i}"] = d
    path = str(tmp_path / "p.json")
    records = predictions_to_json(results, files, path)
    assert records == json.load(open(path)) and len(records) == 7
    assert all(set(r) == {"image_id", "category_id", "bbox", "score"} and isinstance(r["category_id"], int) for r in records)
    back = load_image_predictions(path, 0.25)
    assert list(back) == ["img_0", "img_2"]  # an image without detections writes no record
    for stem, p in back.items():
        d = want[stem]
        b = np.array(p["boxes"]).reshape(-1, 4)
        assert np.abs(b[:, :2] - d[:, :2]).max() <= 0.5e-3 + 1e-4 and np.abs(b[:, 2:] - d[:, 2:4]).max() <= 1e-3 + 1e-4
        assert np.abs(np.array(p["scores"]) - d[:, 4]).max() <= 0.5e-5 + 1e-7 and p["labels"] == d[:, 5].astype(int).tolist()


def test_chunk_bookkeeping():
    """Three images: one whose detections all lie below the threshold, one whose crops are all degenerate (boxes beside the image),
    one with a degenerate crop between two good ones."""
    from ultralytics.utils.double_inference import calculate_optimal_crop_batch, crop_geometry, pad_forwards, plan_two_stage_chunk
    beside = [150.0, 10.0, 170.0, 30.0]  # right of a 100-wide image: the crop's x2 clamps below its x1
    preds = [{"boxes": [[10.0, 10.0, 50.0, 40.0], [20.0, 20.0, 60.0, 60.0]], "scores": [0.2, 0.1], "labels": [0, 1]},
             {"boxes": [beside, [160.0, 20.0, 190.0, 60.0]], "scores": [0.9, 0.8], "labels": [1, 1]},
             {"boxes": [[5.0, 5.0, 45.0, 30.0], [30.0, 30.0, 35.0, 33.0], beside, [60.5, 20.25, 99.0, 70.0]], "scores": [0.5, 0.24, 0.7, 0.3], "labels": [2, 0, 0, 1]}]
    sizes = [(80, 100), (80, 100), (80, 100)]
    p = plan_two_stage_chunk(preds, sizes, 0.25)
    assert p["row_off"].tolist() == [0, 2, 4, 8] and p["crop_off"].tolist() == [0, 0, 0, 2]
    assert p["crop_img"].tolist() == [2, 2] and p["crop_row"].tolist() == [4, 7]
    assert p["zip_row"].tolist() == [4, 6]  # the script zips with ALL candidates: slot 1 is the degenerate candidate's row
    assert p["rows"].shape == (8, 6) and p["rows"].dtype == np.float32 and p["rows"][7].tolist() == [60.5, 20.25, 99.0, 70.0, np.float32(0.3), 1.0]
    for j, i in enumerate((0, 3)):
        c = calculate_optimal_crop_batch([{"bbox": preds[2]["boxes"][i]}], 100, 80)[0]
        g = crop_geometry(c)
        assert p["rects"][j].tolist() == [c["x1"], c["y1"], c["x2"], c["y2"]]
        assert p["geom"][j].tolist() == [*g["new_size"], g["pad_x"], g["pad_y"]]
        assert p["scale"][j].tolist() == [np.float32(g["ratio"]), g["pad_x"], g["pad_y"]]
        assert p["orig"][j].tolist() == p["rows"][p["crop_row"][j]].tolist()
    for k in ("crop_img", "crop_row", "zip_row", "rects", "geom", "row_off", "crop_off"):
        assert p[k].dtype == np.int32
    empty = plan_two_stage_chunk([], [])
    assert empty["rows"].shape == (0, 6) and empty["row_off"].tolist() == [0] and empty["rects"].shape == (0, 4)
    assert [pad_forwards(k, 64) for k in (0, 1, 64, 65, 128)] == [(0, 0), (1, 63), (1, 0), (2, 63), (2, 0)]


def test_scoring_rules():
    from ultralytics.utils.double_inference import precision_recall, scored_mask
    box = {"boxes": [[0, 0, 1, 1]], "scores": [0.5], "labels": [0]}
    none = {"boxes": [], "scores": [], "labels": []}
    lab, nolab = np.zeros((2, 5), np.float32), np.zeros((0, 5), np.float32)
    preds, labels = [box, none, box, none], [lab, lab, nolab, nolab]
    assert scored_mask(preds, labels) == [True, False, False, False]  # :535: a box AND a label
    assert scored_mask(preds, labels, skip_empty=False) == [True] * 4
    tp, fp, fn = [int(v) for v in G["greedy/5/counts_kept"]]
    assert precision_recall(tp, fp, fn) == (tp / (tp + fp), tp / (tp + fn))
    assert precision_recall(0, 0, 0) == (0.0, 0.0) and precision_recall(0, 0, 7) == (0.0, 0.0)  # / max(1, ...)
