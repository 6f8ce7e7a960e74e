#!/usr/bin/env python3
"""Entry script with the reference's shape (reference gt_fails.py:35-94 without its Kaggle paths): the false positives of a model on
a labelled image folder -- detections with confidence >= 0.25 that find no unused label of their class with IoU >= 0.5.

    python gt_fails.py <weights.pt | model.yaml> <images_dir> <labels_dir>
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "experiment-yolo_amd"))
from ultralytics import YOLO  # noqa: E402
from ultralytics.utils.gt_fails import count_fp  # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) != 4:
        sys.exit(__doc__)
    total, _ = count_fp(YOLO(sys.argv[1]), sys.argv[2], sys.argv[3])
    print(f"Correct FP count: {total}")
