"""False-positive count of a model on a labelled image folder (reference gt_fails.py:35-84) with the matching on the device.

The reference script calls the model once per image and matches in a triple Python loop: the detections with confidence >= 0.25, in
the order the model returns them, each take the first unused label (file order) of the same class with IoU >= 0.5; a detection that
finds none is a false positive.  Here ``model.predict`` runs on batches of images, the detections (``Results.boxes.data``) stay on the
device, ONE dy_count_fp launch per batch does the matching (csrc/confusion.hip: one wave per image) and the counts are read back once at
the end.  The script evaluates its IoU in a mix of float32 and float64; the kernel in float64: the counts agree unless an
IoU lies within rounding of the threshold."""
import glob
import os

import numpy as np
import torch

from ..hip import check, lib

CONF_THRESH = 0.25  # gt_fails.py:6-7
IOU_THRESH = 0.5


def load_labels(label_file):
    """Rows ``cls xc yc w h`` of a YOLO label file as (n, 5) float64 in file order; a missing file has none (gt_fails.py:9-16)."""
    if not os.path.exists(label_file):
        return np.zeros((0, 5), np.float64)
    with open(label_file) as f:
        rows = [[float(v) for v in line.split()] for line in f if line.strip()]
    if any(len(r) != 5 for r in rows):
        raise ValueError(f"{label_file}: every label row must be 'cls xc yc w h'")
    return np.asarray(rows, np.float64).reshape(-1, 5)


def count_fp_batch(results, labels, fp_out, status, conf=CONF_THRESH, iou=IOU_THRESH):
    """One launch: ``results`` (the batch's ``Results``, boxes on the device), ``labels`` (their (n, 5) float64 arrays) -> ``fp_out`` (B)
    int32 on the device.  No synchronisation."""
    dev = fp_out.device
    B = len(results)
    boxes = [r.boxes.data.reshape(-1, 6).float() for r in results]
    doff = np.zeros(B + 1, np.int32)
    doff[1:] = np.cumsum([b.shape[0] for b in boxes])
    loff = np.zeros(B + 1, np.int32)
    loff[1:] = np.cumsum([len(l) for l in labels])
    dets = torch.cat(boxes, 0).contiguous() if doff[-1] else torch.zeros((0, 6), device=dev)
    if dets.device != dev:
        raise RuntimeError("count_fp: HIP path only (the model's detections must be on the device)")
    wh = np.array([[r.orig_shape[1], r.orig_shape[0]] for r in results], np.int32)
    host = np.concatenate([doff, loff, wh.reshape(-1)])  # one copy for the three integer tables
    tab = torch.from_numpy(host).to(dev)
    lab = torch.from_numpy(np.concatenate(labels, 0).reshape(-1, 5)).to(dev) if loff[-1] else None
    check(lib().dy_count_fp(dets.data_ptr() if doff[-1] else 0, tab.data_ptr(), lab.data_ptr() if lab is not None else 0,
                            tab.data_ptr() + 4 * (B + 1), tab.data_ptr() + 8 * (B + 1), B, conf, iou, fp_out.data_ptr(), status.data_ptr(),
                            torch.cuda.current_stream(dev).cuda_stream), "dy_count_fp")


def count_fp(model, images_dir, labels_dir, conf=CONF_THRESH, iou=IOU_THRESH, batch=16):
    """-> (total, per_image): the false positives of ``model`` over the sorted ``*.jpg`` files of ``images_dir`` against the label files
    of the same names in ``labels_dir``.  ``model``: a ``YOLO`` (or anything whose ``predict(source=[files], conf=, batch=, verbose=)``
    returns ``Results`` with device-resident ``boxes.data`` and ``orig_shape``)."""
    files = sorted(glob.glob(os.path.join(images_dir, "*.jpg")))
    if not files:
        return 0, {}
    dev = torch.device("cuda", torch.cuda.current_device())
    fp = torch.zeros(len(files), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for lo in range(0, len(files), batch):
        chunk = files[lo:lo + batch]
        labels = [load_labels(os.path.join(labels_dir, os.path.splitext(os.path.basename(f))[0] + ".txt")) for f in chunk]
        results = model.predict(source=chunk, conf=conf, batch=len(chunk), verbose=False)
        if len(results) != len(chunk):
            raise RuntimeError(f"predict returned {len(results)} results for {len(chunk)} images")
        count_fp_batch(results, labels, fp[lo:lo + len(chunk)], status, conf, iou)
    host = torch.cat([fp, status]).cpu().numpy()  # the one read-back
    if host[-1] & 1:
        raise RuntimeError("an image carried more than 1024 labels (dy_count_fp capacity)")
    per_image = {f: int(n) for f, n in zip(files, host[:-1])}
    return int(host[:-1].sum()), per_image
