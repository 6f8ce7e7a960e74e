#!/usr/bin/env python3
"""Sliced (tiled) inference over a directory of large frames, next to the letterboxed single pass (ultralytics/utils/tiled.py, DESIGN.md
section 27; the workflow of the reference's docs/en/guides/sahi-tiled-inference.md):

    python sliced_inference.py <weights.pt | model.yaml> <images_dir> [labels_dir] [--tile 640] [--overlap 0.2] [--json out.json]

Per image the number of detections of the single pass and of the sliced pass, then the totals; with a label directory the script-style
greedy TP / FP / FN (double_inference.py's calculate_metrics_optimized) and mAP@0.5 (the package's validator arithmetic) of both.
``--json`` writes the sliced detections in the predictions format ``double_inference.py`` reads.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "experiment-yolo_amd"))
from ultralytics import YOLO  # noqa: E402
from ultralytics.utils import double_inference as di  # noqa: E402


def run(model, images_dir, labels_dir=None, tile=640, overlap=0.2, conf=di.CONF_THRESHOLD, batch=16, json_path=None, chunk=16, log=print):
    """-> {'single': m, 'sliced': m, 'images'} with m = {'detections', and with labels 'tp', 'fp', 'fn', 'precision', 'recall', 'map_50'}."""
    files = sorted(f for f in os.listdir(images_dir) if os.path.splitext(f)[1].lower() in di.IMG_EXTENSIONS)
    net = model.model
    stages = {s: {"detections": 0, "tp": 0, "fp": 0, "fn": 0, "entries": []} for s in ("single", "sliced")}
    kept = []
    for lo in range(0, len(files), chunk):
        names = files[lo:lo + chunk]
        paths = [os.path.join(images_dir, f) for f in names]
        res = {"single": model.predict(source=paths, conf=conf, batch=len(paths), verbose=False),
               "sliced": model.predict(source=paths, conf=conf, batch=batch, tile=tile, tile_overlap=overlap, verbose=False)}
        kept += res["sliced"]
        preds = {s: [di._results_to_prediction(r) for r in rs] for s, rs in res.items()}
        for i, f in enumerate(names):
            log(f"{f}: single {len(preds['single'][i]['boxes'])} sliced {len(preds['sliced'][i]['boxes'])}")
        dev = next(net.parameters()).device  # predict has moved the model
        if labels_dir:
            stems = [os.path.splitext(f)[0] for f in names]
            shapes = [r.orig_shape for r in res["single"]]
            raw = [di.read_label_rows(os.path.join(labels_dir, s + ".txt")) for s in stems]
            labs = [di.ground_truth_rows(os.path.join(labels_dir, s + ".txt"), w, h) for s, (h, w) in zip(stems, shapes)]
        for s, st in stages.items():
            st["detections"] += sum(len(p["boxes"]) for p in preds[s])
            if labels_dir:
                cnt = di.greedy_counts(preds[s], labs, device=dev)
                st["tp"], st["fp"], st["fn"] = st["tp"] + int(cnt[:, 0].sum()), st["fp"] + int(cnt[:, 1].sum()), st["fn"] + int(cnt[:, 2].sum())
                st["entries"] += list(zip(preds[s], raw, shapes))
    nc = int(getattr(net, "nc", 0) or net.model[-1].nc)
    cls_names = model.names if isinstance(model.names, dict) else dict(enumerate(model.names))
    for s, st in stages.items():
        entries = st.pop("entries")
        line = f"[{s}] detections: {st['detections']}"
        if labels_dir:
            st["precision"], st["recall"] = di.precision_recall(st["tp"], st["fp"], st["fn"])
            st["map_50"], _ = di.map50_by_validator(entries, nc, cls_names, dev)
            line += f" tp {st['tp']} fp {st['fp']} fn {st['fn']} precision {st['precision']:.4f} recall {st['recall']:.4f} mAP@0.5 {st['map_50']:.4f}"
        else:
            for k in ("tp", "fp", "fn"):
                st.pop(k)
        log(line)
    if json_path:
        di.predictions_to_json(kept, files, json_path)
    return {**stages, "images": len(files)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("weights")
    ap.add_argument("images_dir")
    ap.add_argument("labels_dir", nargs="?")
    ap.add_argument("--tile", type=int, default=640)
    ap.add_argument("--overlap", type=float, default=0.2)
    ap.add_argument("--conf", type=float, default=di.CONF_THRESHOLD)
    ap.add_argument("--batch", type=int, default=16, help="tiles per forward")
    ap.add_argument("--json")
    a = ap.parse_args()
    run(YOLO(a.weights), a.images_dir, a.labels_dir, a.tile, a.overlap, a.conf, a.batch, a.json)
