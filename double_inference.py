#!/usr/bin/env python3
"""Entry script with the reference's shape (reference double_inference.py:494-560 without its Kaggle paths, JSON dumps, metric
tables and drawings): first-stage detections of one image, then the two-stage refinement + per-class NMS on the GPU.

    python double_inference.py <weights.pt | model.yaml> <image> [conf=0.25]

With a directory in place of the image, the script's ``main`` (:509-562) over a whole split -- two-stage inference in batched launches,
scored against the label files, for the single-stage and the refined detections:

    python double_inference.py <weights.pt | model.yaml> <images_dir> <labels_dir> [predictions.json]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "experiment-yolo_amd"))
from ultralytics import YOLO  # noqa: E402
from ultralytics.utils.double_inference import CONF_THRESHOLD, double_inference, evaluate_two_stage  # noqa: E402


def evaluate(model, images_dir, labels_dir, predictions=None):
    """The closing lines of the script's main (:552-556), for both stages."""
    import time
    t0 = time.time()
    res = evaluate_two_stage(model, images_dir, labels_dir, predictions=predictions)
    total = time.time() - t0
    for stage in ("single", "refined"):
        m = res[stage]
        print(f"[{stage}] mAP@0.5: {m['map_50']:.4f}")
        print(f"[{stage}] Precision: {m['precision']:.4f}")
        print(f"[{stage}] Recall: {m['recall']:.4f}")
        print(f"[{stage}] tp {m['tp']} fp {m['fp']} fn {m['fn']} over {m['scored_images']} of {res['images']} images")
    print(f"Processing time: {total:.2f} seconds")
    print(f"Average extra inference time per image: {res['extra_seconds'] / max(1, res['images']):.4f} seconds")
    return res


if __name__ == "__main__":
    from PIL import Image
    model = YOLO(sys.argv[1] if len(sys.argv) > 1 else "yolov8n-ASF-P2P2.yaml")
    if len(sys.argv) > 2 and os.path.isdir(sys.argv[2]):
        if len(sys.argv) < 4:
            sys.exit("usage: double_inference.py <weights.pt | model.yaml> <images_dir> <labels_dir> [predictions.json]")
        evaluate(model, sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None)
        sys.exit(0)
    conf = float(sys.argv[3]) if len(sys.argv) > 3 else CONF_THRESHOLD
    img = np.asarray(Image.open(sys.argv[2]).convert("RGB")) if len(sys.argv) > 2 else np.random.default_rng(0).integers(0, 256, (720, 1280, 3), dtype=np.uint8)
    # first stage: model.predict on the image (letterbox, forward, soft-NMS, boxes mapped back: detect/predict.py:23-43)
    det = model.predict(source=np.ascontiguousarray(img[..., ::-1]), imgsz=640, conf=conf, iou=0.7)[0].boxes.data.cpu().numpy()
    single = {"boxes": det[:, :4].tolist(), "scores": det[:, 4].tolist(), "labels": det[:, 5].astype(int).tolist()}
    refined, dt = double_inference(torch.from_numpy(img), model.model, single, conf_threshold=conf)
    print(f"single stage: {len(single['boxes'])} detections; double stage: {len(refined['boxes'])} after refinement + NMS "
          f"({dt * 1e3:.1f} ms extra)")
