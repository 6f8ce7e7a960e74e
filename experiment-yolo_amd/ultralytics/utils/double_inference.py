"""Two-stage ("double") inference (drop-in for the numeric part of reference double_inference.py:98-305; SURVEY.md section
8f row 4): every first-stage detection is cut out of the image with 20 % padding, letterboxed to 640x640, sent through the
model again, and replaced when the second look finds the same class with a higher confidence close to the original box;
a per-class hard NMS merges the result.

The reference does this one detection at a time on the host (PIL crop, cv2 resize, ``model.predict`` per crop, numpy / Python
loops).  Here the image is uploaded once; ``dy_crop_letterbox_u8`` cuts all crops in one launch, the second pass runs as
batched forwards + the soft-NMS kernel, ``dy_refine_select`` picks the replacements for all detections in one launch and
``dy_nms_hard`` does the merge.  Function names and argument meaning follow the reference script; file / JSON handling,
torchmetrics scoring and the visualisations of that script are control plane.

One reference quirk is kept behind a switch: ``process_image_optimized`` zips the list of *successful* refinements with the
list of *all* refined indices (:437-441), so the k-th success overwrites the k-th candidate detection, not the one it was
computed for.  ``aligned=False`` reproduces that; ``aligned=True`` (default here) applies each refinement to its own
detection."""
from __future__ import annotations

import os
import time

import numpy as np
import torch

from ..hip import check, lib
from . import ops
from ..hip.engine import dev_empty

CONF_THRESHOLD = 0.25       # double_inference.py:25
NMS_IOU_THRESHOLD = 0.45    # :27
CROP_SIZE = 640


def calculate_optimal_crop_batch(detections, img_width, img_height, pad_factor=0.2):
    """:98-126 (Python int/float arithmetic kept: int() truncates toward zero)."""
    crops = []
    for detection in detections:
        x1, y1, x2, y2 = detection["bbox"]
        sw, sh = max(1, x2 - x1), max(1, y2 - y1)
        cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
        crop_w, crop_h = sw + 2 * (sw * pad_factor), sh + 2 * (sh * pad_factor)
        nx1, ny1 = max(0, int(cx - crop_w / 2)), max(0, int(cy - crop_h / 2))
        nx2, ny2 = min(img_width, int(cx + crop_w / 2)), min(img_height, int(cy + crop_h / 2))
        if nx2 - nx1 < 10 or ny2 - ny1 < 10:
            m = 32
            nx1, ny1 = max(0, int(cx - m / 2)), max(0, int(cy - m / 2))
            nx2, ny2 = min(img_width, int(cx + m / 2)), min(img_height, int(cy + m / 2))
        crops.append({"x1": nx1, "y1": ny1, "x2": nx2, "y2": ny2})
    return crops


def crop_geometry(crop_info, size=CROP_SIZE):
    """The letterbox bookkeeping of prepare_cropped_image_cv2 (:129-149), or None for an empty crop."""
    w, h = crop_info["x2"] - crop_info["x1"], crop_info["y2"] - crop_info["y1"]
    if w <= 0 or h <= 0:
        return None
    ratio = min(size / w, size / h)
    new_size = (int(w * ratio), int(h * ratio))
    return {"original_size": (w, h), "new_size": new_size, "pad_x": (size - new_size[0]) // 2, "pad_y": (size - new_size[1]) // 2,
            "ratio": ratio}


def prepare_cropped_images(image, crop_infos, size=CROP_SIZE):
    """image: (H,W,3) uint8 tensor on the device.  -> ((K,size,size,3) uint8 batch, [geometry dict per crop])."""
    H, W = image.shape[:2]
    geos = [crop_geometry(c, size) for c in crop_infos]
    assert all(g is not None and g["new_size"][0] > 0 and g["new_size"][1] > 0 for g in geos), "filter empty crops first"
    K = len(crop_infos)
    out = dev_empty((K, size, size, 3), torch.uint8, image.device)
    if K:
        rects = torch.tensor([[c["x1"], c["y1"], c["x2"], c["y2"]] for c in crop_infos], dtype=torch.int32).to(image.device)
        geom = torch.tensor([[g["new_size"][0], g["new_size"][1], g["pad_x"], g["pad_y"]] for g in geos], dtype=torch.int32).to(image.device)
        check(lib().dy_crop_letterbox_u8(image.data_ptr(), H, W, rects.data_ptr(), geom.data_ptr(), K, size, out.data_ptr(),
                                         torch.cuda.current_stream(image.device).cuda_stream), "dy_crop_letterbox_u8")
    return out, geos


def scale_boxes_vectorized(boxes, pad_x, pad_y, crop_info, ratio):
    """:152-161 (host copy for callers of the reference API; the device path does this inside dy_refine_select)."""
    if boxes.size == 0:
        return np.array([])
    scaled = boxes.copy()
    scaled[:, [0, 2]] -= pad_x
    scaled[:, [1, 3]] -= pad_y
    scaled /= ratio
    scaled[:, [0, 2]] += crop_info["x1"]
    scaled[:, [1, 3]] += crop_info["y1"]
    return scaled


def _second_stage(model, crops, conf, iou, batch_size, augment=False):
    """model.predict on every crop: forward (test-time augmented with ``augment``, :231/:235) + decode + soft-NMS, boxes clipped to
    the crop canvas (ops.scale_boxes with equal shapes = clip_boxes)."""
    model.eval()
    preds = []
    with torch.no_grad():
        for i in range(0, crops.shape[0], batch_size):
            x = crops[i:i + batch_size].permute(0, 3, 1, 2).float() / 255
            y, _ = model(x, augment=augment)
            for p in ops.non_max_suppression(y, conf, iou, max_det=300):
                p[:, :4].clamp_(0, crops.shape[1])
                preds.append(p)
    return preds


def perform_batch_double_inference(image, model, detections, use_augment=False, conf=0.25, iou=0.7, batch_size=64,
                                   return_aligned=False):
    """:206-260.  image: (H,W,3) uint8 RGB (tensor | ndarray); detections: [{'bbox': [x1,y1,x2,y2], 'score', 'category_id'}].
    Returns ([refined dicts], seconds) like the reference -- only the successful refinements, in detection order -- or, with
    ``return_aligned``, one entry (dict | None) per detection."""
    t0 = time.time()
    dev = next(model.parameters()).device
    image = torch.as_tensor(image).to(dev).contiguous()
    H, W = image.shape[:2]
    crop_infos = calculate_optimal_crop_batch(detections, W, H)
    valid = [k for k, c in enumerate(crop_infos) if c["x2"] > c["x1"] and c["y2"] > c["y1"]
             and min(crop_geometry(c)["new_size"]) > 0]
    aligned = [None] * len(detections)
    if valid:
        cinfo = [crop_infos[k] for k in valid]
        crops, geos = prepare_cropped_images(image, cinfo)
        args = (model, crops, conf, iou, batch_size)
        preds = _second_stage(*args, augment=True) if use_augment else _second_stage(*args)
        K = len(valid)
        counts = [int(p.shape[0]) for p in preds]
        off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=dev)
        dets = torch.cat([p.reshape(-1, 6).float() for p in preds], 0).contiguous() if sum(counts) else torch.zeros((0, 6), device=dev)
        orig = torch.tensor([[*detections[k]["bbox"], detections[k]["score"], detections[k]["category_id"]] for k in valid],
                            dtype=torch.float32, device=dev)
        rects = torch.tensor([[c["x1"], c["y1"], c["x2"], c["y2"]] for c in cinfo], dtype=torch.int32, device=dev)
        scale = torch.tensor([[g["ratio"], g["pad_x"], g["pad_y"]] for g in geos], dtype=torch.float32, device=dev)
        out = torch.zeros((K, 6), dtype=torch.float32, device=dev)
        found = torch.zeros(K, dtype=torch.int32, device=dev)
        check(lib().dy_refine_select(dets.data_ptr(), off.data_ptr(), orig.data_ptr(), rects.data_ptr(), scale.data_ptr(), K,
                                     float(W), float(H), out.data_ptr(), found.data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream), "dy_refine_select")
        out_h, found_h = out.cpu().numpy(), found.cpu().numpy()
        for j, k in enumerate(valid):
            if found_h[j]:
                aligned[k] = {"bbox": out_h[j, :4].tolist(), "score": float(out_h[j, 4]), "category_id": int(out_h[j, 5])}
    dt = time.time() - t0
    return (aligned, dt) if return_aligned else ([r for r in aligned if r is not None], dt)


def torchvision_nms(boxes, scores, labels, iou_threshold=NMS_IOU_THRESHOLD, device=None):
    """:164-203: per-class greedy NMS; returns the kept (boxes, scores, labels) as lists in their original order."""
    if not boxes or len(boxes) == 0:
        return [], [], []
    dev = torch.device(device or "cuda:0")
    b = torch.tensor(boxes, dtype=torch.float32, device=dev).reshape(-1, 4).contiguous()
    s = torch.tensor(scores, dtype=torch.float32, device=dev).contiguous()
    lab = torch.tensor(labels, dtype=torch.int64)
    lf = lab.to(dev).float().contiguous()
    keep = torch.zeros(b.shape[0], dtype=torch.uint8, device=dev)
    check(lib().dy_nms_hard(b.data_ptr(), s.data_ptr(), lf.data_ptr(), b.shape[0], float(iou_threshold), keep.data_ptr(),
                            torch.cuda.current_stream(dev).cuda_stream), "dy_nms_hard")
    k = keep.bool().cpu()
    return b.cpu()[k].tolist(), s.cpu()[k].tolist(), lab[k].tolist()


def double_inference(image, model, predictions, conf_threshold=CONF_THRESHOLD, nms_iou=NMS_IOU_THRESHOLD, aligned=True):
    """The per-image flow of process_image_optimized (:404-449) without its file handling: ``predictions`` =
    {'boxes': [[x1,y1,x2,y2]], 'scores': [...], 'labels': [...]} (first stage); returns the refined dict + seconds spent."""
    cur = {k: list(v) for k, v in predictions.items()}
    idxs = [i for i, s in enumerate(cur["scores"]) if s >= conf_threshold]
    dets = [{"bbox": cur["boxes"][i], "score": cur["scores"][i], "category_id": cur["labels"][i]} for i in idxs]
    res, dt = perform_batch_double_inference(image, model, dets, return_aligned=True)
    pairs = zip(res, idxs) if aligned else zip([r for r in res if r is not None], idxs)
    for refined, i in pairs:
        if refined is not None:
            cur["boxes"][i], cur["scores"][i], cur["labels"][i] = refined["bbox"], refined["score"], refined["category_id"]
    if cur["boxes"]:
        cur["boxes"], cur["scores"], cur["labels"] = torchvision_nms(cur["boxes"], cur["scores"], cur["labels"], nms_iou,
                                                                     device=next(model.parameters()).device)
    return cur, dt


# ---- the same flow for many images at once, and the script's main (:509-562) -------------------------------------------------
# double_inference handles one image: its crops are one launch, its second pass a forward of however many detections the image has,
# and its results come back in three copies.  Below, the crops of a whole chunk of images are one dy_crop_letterbox_u8_multi launch,
# the second pass runs in forwards of exactly (batch_size, 3, 640, 640) -- the last one filled up with grey canvases, so that every
# forward replays one recorded plan (hip/infer.py keys its plans by shape) -- and dy_refine_select_multi + dy_two_stage_merge leave
# the refined rows, the NMS mask and the script's greedy TP/FP/FN counts in one buffer that is read back once.
SECOND_CONF, SECOND_IOU = 0.25, 0.7   # what double_inference passes to the second pass (perform_batch_double_inference's defaults)
MATCH_IOU = 0.5                       # double_inference.py:26 IOU_THRESHOLD
MERGE_MAX_ROWS, MERGE_MAX_LABELS = 2048, 1024  # csrc/two_stage_batch.hip
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp")


def plan_two_stage_chunk(predictions, sizes, conf_threshold=CONF_THRESHOLD, size=CROP_SIZE):
    """The host bookkeeping of a chunk (pure: no device).  ``predictions``: the first-stage dict of every image, ``sizes``: their
    (H, W).  Every prediction becomes a row of ``rows`` (M, 6) x1 y1 x2 y2 score label with ``row_off`` (N+1); every row with score >=
    ``conf_threshold`` whose crop is not degenerate (the rule of perform_batch_double_inference) becomes a crop: ``crop_img`` /
    ``crop_row`` (K) = its image / its row in ``rows``, ``crop_off`` (N+1), ``rects`` / ``geom`` (K, 4), ``scale`` (K, 3), ``orig``
    (K, 6).  ``zip_row`` (K) is the table of the reference's zip (``aligned=False``): slot j of an image holds the row of its j-th
    CANDIDATE (score >= threshold, degenerate or not); it equals ``crop_row`` whenever no crop was dropped."""
    rows, row_off, crop_off = [], [0], [0]
    crop_img, crop_row, zip_row, rects, geom, scale, orig = [], [], [], [], [], [], []
    for b, (pred, (H, W)) in enumerate(zip(predictions, sizes)):
        base = row_off[-1]
        n = len(pred["scores"])
        for i in range(n):
            rows.append([*pred["boxes"][i], pred["scores"][i], pred["labels"][i]])
        idxs = [i for i in range(n) if pred["scores"][i] >= conf_threshold]
        dets = [{"bbox": pred["boxes"][i]} for i in idxs]
        kept = 0
        for i, c in zip(idxs, calculate_optimal_crop_batch(dets, W, H)):
            g = crop_geometry(c, size) if c["x2"] > c["x1"] and c["y2"] > c["y1"] else None
            if g is None or min(g["new_size"]) <= 0:
                continue
            kept += 1
            crop_img.append(b)
            crop_row.append(base + i)
            rects.append([c["x1"], c["y1"], c["x2"], c["y2"]])
            geom.append([g["new_size"][0], g["new_size"][1], g["pad_x"], g["pad_y"]])
            scale.append([g["ratio"], g["pad_x"], g["pad_y"]])
            orig.append([*pred["boxes"][i], pred["scores"][i], pred["labels"][i]])
        zip_row.extend(base + i for i in idxs[:kept])
        row_off.append(base + n)
        crop_off.append(crop_off[-1] + kept)
    i32 = lambda a, *s: np.asarray(a, np.int32).reshape(-1, *s)  # noqa: E731
    f32 = lambda a, *s: np.asarray(a, np.float32).reshape(-1, *s)  # noqa: E731
    return {"rows": f32(rows, 6), "row_off": i32(row_off), "crop_off": i32(crop_off), "crop_img": i32(crop_img), "crop_row": i32(crop_row),
            "zip_row": i32(zip_row), "rects": i32(rects, 4), "geom": i32(geom, 4), "scale": f32(scale, 3), "orig": f32(orig, 6)}


def pad_forwards(n_crops, batch_size):
    """-> (forwards, pad canvases): the second pass of ``n_crops`` crops in forwards of exactly ``batch_size``."""
    forwards = -(-n_crops // batch_size)
    return forwards, forwards * batch_size - n_crops


def image_pool(images, device):
    """(H, W, 3) uint8 images of any sizes -> (one uint8 device tensor holding them back to back, byte offsets (N) int64, sizes
    [(H, W)]).  Host arrays are joined on the host and uploaded in one copy."""
    sizes, flat = [], []
    for im in images:
        if tuple(im.shape[2:]) != (3,) or str(im.dtype).split(".")[-1] != "uint8":
            raise ValueError(f"images must be (H, W, 3) uint8, got {tuple(im.shape)} {im.dtype}")
        sizes.append((int(im.shape[0]), int(im.shape[1])))
        flat.append(im.contiguous().reshape(-1) if isinstance(im, torch.Tensor) else np.ascontiguousarray(im).reshape(-1))
    off = np.zeros(len(images), np.int64)
    off[1:] = np.cumsum([h * w * 3 for h, w in sizes])[:-1]
    if flat and all(isinstance(f, torch.Tensor) and f.device == device for f in flat):
        pool = torch.cat(flat)
    else:
        host = [f.cpu().numpy() if isinstance(f, torch.Tensor) else f for f in flat]
        pool = torch.from_numpy(np.concatenate(host) if host else np.zeros(0, np.uint8)).to(device)
    return pool, off, sizes


def crop_letterbox_multi(pool, img_off, sizes, crop_img, rects, geom, out, size=CROP_SIZE):
    """One dy_crop_letterbox_u8_multi launch: the K crops into ``out[:K]`` ((>= K, size, size, 3) uint8 on the pool's device).
    The tables are host arrays and are checked here -- the kernel trusts them."""
    img_off, crop_img = np.asarray(img_off, np.int64).reshape(-1), np.asarray(crop_img, np.int32).reshape(-1)
    rects, geom = np.asarray(rects, np.int32).reshape(-1, 4), np.asarray(geom, np.int32).reshape(-1, 4)
    hw = np.asarray(sizes, np.int32).reshape(-1, 2)
    K, N = len(crop_img), len(hw)
    if K == 0:
        return
    if len(rects) != K or len(geom) != K or crop_img.min() < 0 or crop_img.max() >= N or len(img_off) != N:
        raise ValueError("crop tables do not match")
    h, w = hw[crop_img, 0], hw[crop_img, 1]
    if (rects[:, 0] < 0).any() or (rects[:, 1] < 0).any() or (rects[:, 2] > w).any() or (rects[:, 3] > h).any() \
            or (rects[:, 2] <= rects[:, 0]).any() or (rects[:, 3] <= rects[:, 1]).any():
        raise ValueError("a crop rectangle is empty or leaves its image")
    if (geom[:, :2] <= 0).any() or (geom[:, 2:] < 0).any() or (geom[:, :2] + geom[:, 2:] > size).any():
        raise ValueError("a crop does not fit its canvas")
    if (img_off < 0).any() or (img_off + hw[:, 0].astype(np.int64) * hw[:, 1] * 3 > pool.numel()).any():
        raise ValueError("an image leaves the pool")
    if out.dtype != torch.uint8 or out.shape[0] < K or tuple(out.shape[1:]) != (size, size, 3) or not out.is_contiguous():
        raise ValueError("out must be a contiguous (>= K, size, size, 3) uint8 tensor")
    dev = pool.device
    offs = torch.from_numpy(img_off).to(dev)
    tab = torch.from_numpy(np.concatenate([hw.reshape(-1), crop_img, rects.reshape(-1), geom.reshape(-1)])).to(dev)
    p = tab.data_ptr()
    check(lib().dy_crop_letterbox_u8_multi(pool.data_ptr(), offs.data_ptr(), p, p + 4 * 2 * N, p + 4 * (2 * N + K), p + 4 * (2 * N + 5 * K),
                                           K, size, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
          "dy_crop_letterbox_u8_multi")


def two_stage_merge(rows, row_off, refined, found, crop_row, crop_off, labels, lab_off, aligned, nms_iou, match_iou, device):
    """One dy_two_stage_merge launch and ONE read-back.  Host arrays ``rows`` (M, 6), ``row_off`` / ``crop_off`` / ``lab_off`` (N+1),
    ``crop_row`` (K), ``labels`` (L, 5) cls x1 y1 x2 y2; ``refined`` (K, 6) / ``found`` (K) device tensors (or None with K = 0).
    -> (rows with the replacements applied (M, 6), keep (M) bool, counts (N, 3) tp fp fn) as numpy arrays.  ``nms_iou`` < 0: no NMS.
    Raises when an image exceeds the kernel's 2,048 rows or 1,024 labels."""
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 6)
    labels = np.ascontiguousarray(labels, np.float32).reshape(-1, 5)
    ints = [np.asarray(a, np.int32).reshape(-1) for a in (row_off, crop_off, lab_off, crop_row)]
    N, M, K, L = len(ints[0]) - 1, len(rows), len(ints[3]), len(labels)
    if len(ints[1]) != N + 1 or len(ints[2]) != N + 1 or ints[0][-1] != M or ints[1][-1] != K or ints[2][-1] != L:
        raise ValueError("offset tables do not match")
    if N == 0:
        return rows, np.zeros(0, bool), np.zeros((0, 3), np.int32)
    itab = torch.from_numpy(np.concatenate(ints)).to(device)
    ftab = torch.from_numpy(np.concatenate([rows.reshape(-1), labels.reshape(-1), np.zeros(1, np.float32)])).to(device)
    # one output buffer: rows (M, 6) fp32 | counts (N, 3) int32 | status int32 | keep (M) bytes
    o_cnt, o_st, o_keep = 24 * M, 24 * M + 12 * N, 24 * M + 12 * N + 4
    outb = torch.zeros(o_keep + M, dtype=torch.uint8, device=device)
    if M:
        outb[:o_cnt].view(torch.float32).copy_(ftab[:6 * M])
    ip, op = itab.data_ptr(), outb.data_ptr()
    check(lib().dy_two_stage_merge(op, ip, refined.data_ptr() if K else 0, found.data_ptr() if K else 0, ip + 4 * 3 * (N + 1),
                                   ip + 4 * (N + 1), int(bool(aligned)), float(nms_iou), ftab.data_ptr() + 4 * 6 * M, ip + 4 * 2 * (N + 1),
                                   float(match_iou), N, op + o_keep, op + o_cnt, op + o_st,
                                   torch.cuda.current_stream(device).cuda_stream), "dy_two_stage_merge")
    host = outb.cpu().numpy()  # the one read-back
    if host[o_st:o_keep].view(np.int32)[0] & 1:
        raise RuntimeError(f"an image carried more than {MERGE_MAX_ROWS} detections or {MERGE_MAX_LABELS} labels (dy_two_stage_merge capacity)")
    return host[:o_cnt].view(np.float32).reshape(-1, 6), host[o_keep:].astype(bool), host[o_cnt:o_st].view(np.int32).reshape(-1, 3)


def _label_tables(labels, N):
    if labels is None:
        return np.zeros((0, 5), np.float32), np.zeros(N + 1, np.int32)
    labs = [np.asarray(l, np.float32).reshape(-1, 5) for l in labels]
    if len(labs) != N:
        raise ValueError("one label array per image")
    off = np.zeros(N + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in labs])
    return (np.concatenate(labs, 0) if N else np.zeros((0, 5), np.float32)), off


def _rows_to_predictions(rows, keep, row_off):
    out = []
    for b in range(len(row_off) - 1):
        r = rows[row_off[b]:row_off[b + 1]][keep[row_off[b]:row_off[b + 1]]]
        out.append({"boxes": r[:, :4].tolist(), "scores": r[:, 4].tolist(), "labels": r[:, 5].astype(np.int64).tolist()})
    return out


def double_inference_batch(images, model, predictions, labels=None, conf_threshold=CONF_THRESHOLD, nms_iou=NMS_IOU_THRESHOLD,
                           match_iou=MATCH_IOU, aligned=True, use_augment=False, batch_size=64):
    """``double_inference`` for a chunk of images in batched launches.  ``images``: [(H, W, 3) uint8 RGB array | tensor] of any
    sizes; ``predictions``: their first-stage dicts; ``labels``: per image an (n, 5) array ``cls x1 y1 x2 y2`` in native pixels, or
    None.  -> (refined dicts, counts, seconds): per image what ``double_inference`` returns for it alone given the same second-stage
    rows, and ``counts`` (N, 3) = the script's greedy tp, fp, fn of the refined set against the labels (None without labels)."""
    t0 = time.time()
    dev = next(model.parameters()).device
    N = len(images)
    if len(predictions) != N:
        raise ValueError("one first-stage dict per image")
    pool, img_off, sizes = image_pool(images, dev)
    plan = plan_two_stage_chunk(predictions, sizes, conf_threshold)
    lab, lab_off = _label_tables(labels, N)
    K = len(plan["crop_img"])
    refined = found = None
    if K:
        forwards, _ = pad_forwards(K, batch_size)
        crops = torch.full((forwards * batch_size, CROP_SIZE, CROP_SIZE, 3), 114, dtype=torch.uint8, device=dev)  # pad canvases: grey
        crop_letterbox_multi(pool, img_off, sizes, plan["crop_img"], plan["rects"], plan["geom"], crops)
        args = (model, crops, SECOND_CONF, SECOND_IOU, batch_size)
        preds = _second_stage(*args, augment=True) if use_augment else _second_stage(*args)
        if len(preds) != crops.shape[0]:
            raise RuntimeError(f"the second stage returned {len(preds)} results for {crops.shape[0]} canvases")
        preds = preds[:K]  # whatever the pad canvases produced ends here
        counts = [int(p.shape[0]) for p in preds]
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        dets = torch.cat([p.reshape(-1, 6).float() for p in preds], 0).contiguous() if off[-1] else torch.zeros((0, 6), device=dev)
        hw = np.asarray(sizes, np.int32).reshape(-1)
        itab = torch.from_numpy(np.concatenate([off, plan["rects"].reshape(-1), plan["crop_img"], hw])).to(dev)
        ftab = torch.from_numpy(np.concatenate([plan["orig"].reshape(-1), plan["scale"].reshape(-1)])).to(dev)
        refined = torch.zeros((K, 6), dtype=torch.float32, device=dev)
        found = torch.zeros(K, dtype=torch.int32, device=dev)
        ip, fp = itab.data_ptr(), ftab.data_ptr()
        check(lib().dy_refine_select_multi(dets.data_ptr(), ip, fp, ip + 4 * (K + 1), fp + 4 * 6 * K, ip + 4 * (5 * K + 1), ip + 4 * (6 * K + 1),
                                           K, refined.data_ptr(), found.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
              "dy_refine_select_multi")
    rows, keep, cnt = two_stage_merge(plan["rows"], plan["row_off"], refined, found, plan["crop_row"] if aligned else plan["zip_row"],
                                      plan["crop_off"], lab, lab_off, aligned, nms_iou, match_iou, dev)
    out = _rows_to_predictions(rows, keep, plan["row_off"])
    return out, (cnt if labels is not None else None), time.time() - t0


def greedy_counts(predictions, labels, match_iou=MATCH_IOU, device=None):
    """calculate_metrics_optimized (:306-333) of every image in one launch: ``predictions`` as they stand (no refinement, no NMS)
    against ``labels`` -> (N, 3) tp fp fn."""
    dev = torch.device(device or "cuda:0")
    N = len(predictions)
    plan = plan_two_stage_chunk(predictions, [(0, 0)] * N, conf_threshold=float("inf"))
    lab, lab_off = _label_tables(labels, N)
    return two_stage_merge(plan["rows"], plan["row_off"], None, None, plan["crop_row"], plan["crop_off"], lab, lab_off, True, -1.0,
                           match_iou, dev)[2]


def load_image_predictions(predictions_path, conf_threshold=CONF_THRESHOLD):
    """:473-489.  Records ``{image_id: stem, category_id, bbox: [x, y, w, h] top-left, score}`` -> {stem: first-stage dict}; an
    image whose every record lies below the threshold keeps an empty entry."""
    import json
    if not os.path.exists(predictions_path):
        raise FileNotFoundError(f"Predictions file not found at {predictions_path}")
    with open(predictions_path) as f:
        records = json.load(f)
    out = {}
    for rec in records:
        entry = out.setdefault(rec["image_id"], {"boxes": [], "scores": [], "labels": []})
        if rec["score"] >= conf_threshold:
            x, y, w, h = rec["bbox"]
            entry["boxes"].append([x, y, x + w, y + h])
            entry["scores"].append(rec["score"])
            entry["labels"].append(rec["category_id"])
    return out


def predictions_to_json(results, files, path):
    """The writer ``load_image_predictions`` reads: the records of the reference validator's ``pred_to_json``
    (models/yolo/detect/val.py:261-275: top-left xywh rounded to 3 decimals, score to 5, the file stem as image id) for a list of
    ``Results`` and their files.  Returns the records."""
    import json
    records = []
    for r, f in zip(results, files):
        stem = os.path.splitext(os.path.basename(str(f)))[0]
        predn = torch.as_tensor(r.boxes.data).reshape(-1, 6).float().cpu()
        box = ops.xyxy2xywh(predn[:, :4])
        box[:, :2] -= box[:, 2:] / 2
        for p, b in zip(predn.tolist(), box.tolist()):
            records.append({"image_id": stem, "category_id": int(p[5]), "bbox": [round(x, 3) for x in b], "score": round(p[4], 5)})
    with open(path, "w") as f:
        json.dump(records, f)
    return records


def read_label_rows(label_path):
    """The lines of a YOLO label file the script accepts (:496-499: at least 5 fields) as (n, 5) float64 ``cls xc yc w h``; a missing
    file has none.  A line with more than 5 fields does not unpack in the script either."""
    rows = []
    if os.path.exists(label_path):
        with open(label_path) as f:
            for line in f.readlines():
                parts = line.strip().split()
                if len(parts) >= 5:
                    if len(parts) > 5:
                        raise ValueError(f"{label_path}: a label row must be 'cls xc yc w h'")
                    rows.append([float(v) for v in parts])
    return np.asarray(rows, np.float64).reshape(-1, 5)


def load_ground_truth(label_path, img_width, img_height):
    """:492-506 -> (boxes [[x1, y1, x2, y2]] in pixels as Python floats (float64 arithmetic, the script's operation order), labels)."""
    boxes, labels = [], []
    for class_id, xc, yc, w, h in read_label_rows(label_path).tolist():
        boxes.append([(xc - w / 2) * img_width, (yc - h / 2) * img_height, (xc + w / 2) * img_width, (yc + h / 2) * img_height])
        labels.append(int(class_id))
    return boxes, labels


def ground_truth_rows(label_path, img_width, img_height):
    """``load_ground_truth`` as the (n, 5) fp32 ``cls x1 y1 x2 y2`` rows the merge kernel takes (what ``torch.tensor`` of the script's
    Python floats holds)."""
    boxes, labels = load_ground_truth(label_path, img_width, img_height)
    return np.concatenate([np.asarray(labels, np.float32).reshape(-1, 1), np.asarray(boxes, np.float32).reshape(-1, 4)], 1)


def scored_mask(predictions, labels, skip_empty=True):
    """:535: an image enters the scores only with at least one box AND at least one label; ``skip_empty=False`` scores all."""
    return [not skip_empty or (len(p["boxes"]) > 0 and len(l) > 0) for p, l in zip(predictions, labels)]


def precision_recall(tp, fp, fn):
    """:351-352."""
    return tp / max(1, tp + fp), tp / max(1, tp + fn)


def map50_by_validator(entries, nc, names, device):
    """mAP@0.5 by the package's validator arithmetic (NOT torchmetrics' COCO AP: DESIGN.md section 26).  ``entries``: per scored image
    (prediction dict, (n, 5) ``cls xc yc w h`` normalised label rows, (H, W)).  One dy_match_predictions launch (gain 1, pad 0) per
    group of equally sized images, then ap_per_class.  -> (map_50, {class: AP@0.5})."""
    from ..models.yolo.detect.val import DetectionValidator
    v = DetectionValidator()
    v.device, v.nc, v.plots_gate = device, nc, False
    v.names = names
    v.metrics.names = names
    groups = {}
    for e in entries:
        groups.setdefault(tuple(e[2]), []).append(e)
    for (H, W), group in groups.items():
        preds = [torch.from_numpy(np.concatenate([np.asarray(p["boxes"], np.float32).reshape(-1, 4), np.asarray(p["scores"], np.float32).reshape(-1, 1),
                                                  np.asarray(p["labels"], np.float32).reshape(-1, 1)], 1)).to(device) for p, _, _ in group]
        labs = [np.asarray(l, np.float32).reshape(-1, 5) for _, l, _ in group]
        cat = np.concatenate(labs, 0)
        batch = {"img": torch.empty((0, 3, H, W)), "cls": torch.from_numpy(cat[:, 0].copy()).to(device),
                 "bboxes": torch.from_numpy(cat[:, 1:].copy()).to(device), "ori_shape": [(H, W)] * len(group),
                 "batch_idx": torch.from_numpy(np.repeat(np.arange(len(group)), [len(l) for l in labs]).astype(np.float32)).to(device)}
        v.update_metrics(preds, batch)
    if not groups:
        return 0.0, {}
    v.get_stats()
    box = v.metrics.box
    return float(box.map50), {int(c): float(a) for c, a in zip(box.ap_class_index, box.ap50)}


def _results_to_prediction(r):
    d = r.boxes.data.reshape(-1, 6).float().cpu().numpy()
    return {"boxes": d[:, :4].tolist(), "scores": d[:, 4].tolist(), "labels": d[:, 5].astype(np.int64).tolist()}


def evaluate_two_stage(model, images_dir, labels_dir, predictions=None, conf=CONF_THRESHOLD, nms_iou=NMS_IOU_THRESHOLD, match_iou=MATCH_IOU,
                       use_augment=True, aligned=True, chunk=16, skip_empty=True):
    """The script's ``main`` (:509-562): two-stage inference over the images of ``images_dir`` against the label files of the same
    stems in ``labels_dir``.  ``model``: a ``YOLO`` (``model.model`` runs the second stage).  ``predictions``: a predictions JSON
    (``load_image_predictions``), a loaded {stem: first-stage dict}, or None = run the first stage here with ``model.predict`` on
    chunks; with predictions given only the images they name are processed (:516-517).
    -> {'single': m, 'refined': m, 'images', 'extra_seconds'} with m = {'map_50', 'precision', 'recall', 'tp', 'fp', 'fn',
    'per_class_ap', 'scored_images', 'predictions': {stem: dict}}; precision / recall from the device counts by the script's
    formulas, map_50 by ``map50_by_validator``."""
    from PIL import Image
    net = getattr(model, "model", model)
    dev = next(net.parameters()).device
    if isinstance(predictions, (str, os.PathLike)):
        predictions = load_image_predictions(predictions, conf)
    files = sorted(f for f in os.listdir(images_dir) if os.path.splitext(f)[1].lower() in IMG_EXTENSIONS)
    if predictions is not None:
        files = [f for f in files if os.path.splitext(f)[0] in predictions]
    stages = {s: {"tp": 0, "fp": 0, "fn": 0, "scored_images": 0, "predictions": {}, "entries": []} for s in ("single", "refined")}
    extra = 0.0
    for lo in range(0, len(files), chunk):
        names = files[lo:lo + chunk]
        paths = [os.path.join(images_dir, f) for f in names]
        stems = [os.path.splitext(f)[0] for f in names]
        images = [np.asarray(Image.open(p).convert("RGB")) for p in paths]
        if predictions is None:
            results = model.predict(source=paths, conf=conf, batch=len(paths), verbose=False)
            if len(results) != len(paths):
                raise RuntimeError(f"predict returned {len(results)} results for {len(paths)} images")
            first = [_results_to_prediction(r) for r in results]
        else:
            first = [predictions[s] for s in stems]
        raw = [read_label_rows(os.path.join(labels_dir, s + ".txt")) for s in stems]
        labs = [ground_truth_rows(os.path.join(labels_dir, s + ".txt"), im.shape[1], im.shape[0]) for s, im in zip(stems, images)]
        refined, cnt, dt = double_inference_batch(images, net, first, labs, conf, nms_iou, match_iou, aligned, use_augment)
        extra += dt
        for stage, preds, counts in (("single", first, greedy_counts(first, labs, match_iou, dev)), ("refined", refined, cnt)):
            st = stages[stage]
            for i, ok in enumerate(scored_mask(preds, labs, skip_empty)):
                st["predictions"][stems[i]] = preds[i]
                if ok:
                    st["tp"], st["fp"], st["fn"] = st["tp"] + int(counts[i, 0]), st["fp"] + int(counts[i, 1]), st["fn"] + int(counts[i, 2])
                    st["scored_images"] += 1
                    st["entries"].append((preds[i], raw[i], images[i].shape[:2]))
    nc = int(getattr(net, "nc", 0) or net.model[-1].nc)
    cls_names = getattr(model, "names", None) or {i: str(i) for i in range(nc)}
    cls_names = dict(enumerate(cls_names)) if isinstance(cls_names, (list, tuple)) else cls_names
    out = {"images": len(files), "extra_seconds": extra}
    for stage, st in stages.items():
        st["precision"], st["recall"] = precision_recall(st["tp"], st["fp"], st["fn"])
        st["map_50"], st["per_class_ap"] = map50_by_validator(st.pop("entries"), nc, cls_names, dev)
        out[stage] = st
    return out
