"""Sliced (tiled) inference for frames much larger than the model input (the workflow of the reference's
docs/en/guides/sahi-tiled-inference.md, without the SAHI package): the frame is cut into overlapping ``tile`` x ``tile`` windows, every
window goes through the model at native resolution -- so an animal a few dozen pixels wide in a 4K frame reaches the stem as it was
filmed -- and the detections of all windows, plus those of one letterboxed pass over the whole frame, are mapped into the frame and
merged by a greedy NMS across windows.

The frame is uploaded once as uint8.  ``dy_tile_gather_f32`` writes all windows of a group of frames straight into the fp32 planar
batch the forward reads (3 bytes in, 12 out per pixel; no host slice, no host letterbox, no float upload, no permute / convert pass);
the forwards all have the shape ``(batch, 3, tile, tile)``, so they replay one recorded plan; ``dy_tile_merge`` maps and merges the
rows of every frame of the group in one launch that is read back once."""
from __future__ import annotations

import numpy as np
import torch

from ..hip import check, lib
from ..hip.engine import dev_empty
from . import ops
from .double_inference import image_pool, pad_forwards

MERGE_MAX_ROWS = 8192  # DY_TILE_MERGE_MAX_ROWS
GROUP = 16             # images per pool upload
METRICS = {"iou": 0, "ios": 1}


def _origins(L, tile, step):
    if L <= tile:
        return [0]
    out, o = [], 0
    while o + tile < L:
        out.append(o)
        o += step
    out.append(L - tile)  # the first window that would reach or cross the edge is shifted back instead of padded
    return out


def tile_grid(H, W, tile, overlap):
    """-> [(x1, y1, x2, y2)] with exclusive x2 / y2, row-major.  Per axis: windows every ``tile - int(overlap * tile)`` pixels while
    they end inside the image; the one that would reach the edge sits at ``L - tile``.  An axis shorter than ``tile`` has one window."""
    H, W, tile = int(H), int(W), int(tile)
    if H <= 0 or W <= 0 or tile <= 0:
        raise ValueError(f"tile_grid needs positive sizes, got H={H} W={W} tile={tile}")
    if not 0 <= overlap < 1:
        raise ValueError(f"overlap must lie in [0, 1), got {overlap}")
    step = tile - int(overlap * tile)
    return [(x, y, min(x + tile, W), min(y + tile, H)) for y in _origins(H, tile, step) for x in _origins(W, tile, step)]


def check_tile(tile, stride=32):
    """``tile`` must be a positive multiple of the predictor's stride (max(model stride, 32), as DetectionPredictor.setup_model)."""
    if isinstance(tile, bool) or not isinstance(tile, (int, np.integer)) or tile <= 0 or tile % int(stride):
        raise ValueError(f"tile={tile!r} must be a positive multiple of the stride {int(stride)}")
    return int(tile)


def model_stride(model):
    return max(int(max(float(s) for s in model.stride)), 32) if hasattr(model, "stride") else 32


def full_pass_record(H, W, tile):
    """The letterboxed whole-image record: (rect, geom, map-back row)."""
    r = min(tile / H, tile / W)
    new_w, new_h = max(1, round(W * r)), max(1, round(H * r))
    pad_x, pad_y = (tile - new_w) // 2, (tile - new_h) // 2
    return (0, 0, W, H), (new_w, new_h, pad_x, pad_y), _map_row(0, 0, pad_x, pad_y, r)


def _map_row(x1, y1, pad_x, pad_y, r):
    r32 = np.float32(r)
    return np.array([x1, y1, pad_x, pad_y, r32, np.float32(1) / r32], np.float32)


def plan_tiles(sizes, tile, overlap, full_image=True):
    """The records of a group of images (pure: no device).  ``sizes``: [(H, W)].  -> dict of ``tile_img`` (K) int32, ``rects`` (K, 4)
    int32, ``geom`` (K, 4) int32 new_w new_h pad_x pad_y, ``maps`` (K, 6) fp32 x1 y1 pad_x pad_y r 1/r, ``rec_off`` (N+1): the records
    of image i are rec_off[i]:rec_off[i+1], its windows in row-major order, then the whole-image pass unless the grid is one window."""
    tile_img, rects, geom, maps, rec_off = [], [], [], [], [0]
    for b, (H, W) in enumerate(sizes):
        grid = tile_grid(H, W, tile, overlap)
        for x1, y1, x2, y2 in grid:
            tile_img.append(b), rects.append((x1, y1, x2, y2)), geom.append((x2 - x1, y2 - y1, 0, 0)), maps.append(_map_row(x1, y1, 0, 0, 1.0))
        if full_image and len(grid) > 1:
            rc, g, m = full_pass_record(H, W, tile)
            tile_img.append(b), rects.append(rc), geom.append(g), maps.append(m)
        rec_off.append(len(tile_img))
    return {"tile_img": np.asarray(tile_img, np.int32).reshape(-1), "rects": np.asarray(rects, np.int32).reshape(-1, 4),
            "geom": np.asarray(geom, np.int32).reshape(-1, 4), "maps": np.asarray(maps, np.float32).reshape(-1, 6),
            "rec_off": np.asarray(rec_off, np.int32)}


_LUT = {}


def byte_table(device):
    """(256) fp32 on ``device``: what ``uint8_tensor.float() / 255`` gives for every byte on that device, computed there once."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _LUT:
        _LUT[key] = (torch.arange(256, dtype=torch.int32, device=device).to(torch.uint8).float() / 255).contiguous()
    return _LUT[key]


def tile_gather(pool, img_off, sizes, tile_img, rects, geom, out, size):
    """One dy_tile_gather_f32 launch: K records into ``out[:K]`` ((>= K, 3, size, size) fp32, contiguous, on the pool's device).
    ``tile_img[k] < 0`` is a pad canvas (114 / 255 everywhere; its rect and geom are ignored).  The tables are host arrays and are
    checked here -- the kernel trusts them."""
    img_off, tile_img = np.asarray(img_off, np.int64).reshape(-1), np.asarray(tile_img, np.int32).reshape(-1)
    rects, geom = np.asarray(rects, np.int32).reshape(-1, 4).copy(), np.asarray(geom, np.int32).reshape(-1, 4).copy()
    hw = np.asarray(sizes, np.int32).reshape(-1, 2)
    K, N = len(tile_img), len(hw)
    if K == 0:
        return
    if len(rects) != K or len(geom) != K or tile_img.max() >= N or len(img_off) != N:
        raise ValueError("tile tables do not match")
    real = tile_img >= 0
    rects[~real], geom[~real] = 0, 0
    h, w = hw[tile_img[real], 0], hw[tile_img[real], 1]
    rc, gm = rects[real], geom[real]
    if (rc[:, 0] < 0).any() or (rc[:, 1] < 0).any() or (rc[:, 2] > w).any() or (rc[:, 3] > h).any() \
            or (rc[:, 2] <= rc[:, 0]).any() or (rc[:, 3] <= rc[:, 1]).any():
        raise ValueError("a tile rectangle is empty or leaves its image")
    if (gm[:, :2] <= 0).any() or (gm[:, 2:] < 0).any() or (gm[:, :2] + gm[:, 2:] > size).any():
        raise ValueError("a tile does not fit its canvas")
    if (img_off < 0).any() or (img_off + hw[:, 0].astype(np.int64) * hw[:, 1] * 3 > pool.numel()).any():
        raise ValueError("an image leaves the pool")
    if pool.dtype != torch.uint8 or not pool.is_contiguous():
        raise ValueError("the pool must be a contiguous uint8 tensor")
    if out.dtype != torch.float32 or out.dim() != 4 or out.shape[0] < K or tuple(out.shape[1:]) != (3, size, size) or not out.is_contiguous() \
            or out.device != pool.device:
        raise ValueError("out must be a contiguous (>= K, 3, size, size) fp32 tensor on the pool's device")
    dev = pool.device
    offs = torch.from_numpy(img_off).to(dev)
    tab = torch.from_numpy(np.concatenate([hw.reshape(-1), tile_img, rects.reshape(-1), geom.reshape(-1)])).to(dev)
    p = tab.data_ptr()
    check(lib().dy_tile_gather_f32(pool.data_ptr(), offs.data_ptr(), p, p + 4 * 2 * N, p + 4 * (2 * N + K), p + 4 * (2 * N + 5 * K),
                                   byte_table(dev).data_ptr(), K, size, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
          "dy_tile_gather_f32")


def tile_merge(rows, row_off, row_tile, maps, sizes, thr, metric="ios", agnostic=False):
    """One dy_tile_merge launch and ONE read-back.  ``rows`` (M, 6) device tensor (x1 y1 x2 y2 score label in canvas coordinates,
    packed image-major); host arrays ``row_off`` (N+1), ``row_tile`` (M) -> ``maps`` (Kt, 6), ``sizes`` [(H, W)].
    -> (mapped rows (M, 6) device tensor, order (M) int32 device tensor, nkeep (N) numpy): the kept rows of image i, in descending
    score, are ``mapped[order[row_off[i]:row_off[i] + nkeep[i]]]``.  Raises when an image has more than 8,192 rows."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    row_off, row_tile = np.asarray(row_off, np.int32).reshape(-1), np.asarray(row_tile, np.int32).reshape(-1)
    maps = np.ascontiguousarray(maps, np.float32).reshape(-1, 6)
    hw = np.asarray(sizes, np.int32).reshape(-1, 2)
    N, M, Kt = len(hw), int(rows.shape[0]), len(maps)
    dev = rows.device
    if rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] != 6 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous (M, 6) fp32 tensor")
    if len(row_off) != N + 1 or row_off[0] != 0 or row_off[-1] != M or (np.diff(row_off) < 0).any() or len(row_tile) != M:
        raise ValueError("offset tables do not match")
    if M and (row_tile.min() < 0 or row_tile.max() >= Kt):
        raise ValueError("a row names a record that does not exist")
    mapped = dev_empty((M, 6), torch.float32, dev)
    ints = torch.zeros(M + N + 1, dtype=torch.int32, device=dev)  # order (M) | nkeep (N) | status
    if N == 0:
        return mapped, ints[:M], np.zeros(0, np.int32)
    max_rows = int(np.diff(row_off).max())
    itab = torch.from_numpy(np.concatenate([row_off, row_tile, hw.reshape(-1)])).to(dev)
    ftab = torch.from_numpy(np.concatenate([maps.reshape(-1), np.zeros(1, np.float32)])).to(dev)
    ip, op = itab.data_ptr(), ints.data_ptr()
    rc = lib().dy_tile_merge(rows.data_ptr(), ip, ip + 4 * (N + 1), ftab.data_ptr(), ip + 4 * (N + 1 + M), N, Kt, max_rows, float(thr),
                             METRICS[metric], int(bool(agnostic)), mapped.data_ptr(), op, op + 4 * M, op + 4 * (M + N),
                             torch.cuda.current_stream(dev).cuda_stream)
    if rc == -4:
        raise RuntimeError(f"an image carried {max_rows} detections, more than {MERGE_MAX_ROWS} (dy_tile_merge capacity)")
    check(rc, "dy_tile_merge")
    tail = ints[M:].cpu().numpy()  # the one read-back
    if tail[N] & 1:
        raise RuntimeError(f"an image carried more than {MERGE_MAX_ROWS} detections (dy_tile_merge capacity)")
    if tail[N] & 2:
        raise RuntimeError("dy_tile_merge: a row names a record that does not exist")
    return mapped, ints[:M], tail[:N].copy()


def _detect_tiles(model, x, conf, iou, classes=None, agnostic=False, max_det=300, augment=False):
    """One forward of (batch, 3, tile, tile) canvases -> [(k, 6)] x1 y1 x2 y2 score label per canvas, in canvas coordinates: the calls
    ``DetectionPredictor`` makes for a batch, so a native tile is predicted as ``predict`` would predict it as an image of its own."""
    y = model(x, augment=augment)
    return ops.non_max_suppression(y, conf, iou, classes=classes, agnostic=agnostic, max_det=max_det)


@torch.no_grad()
def tiled_predict(images, model, tile=640, overlap=0.2, conf=0.25, iou=0.7, merge_iou=0.5, metric="ios", full_image=True, batch=64,
                  agnostic=False, classes=None, max_det=300, augment=False):
    """Sliced inference.  ``images``: [(H, W, 3) uint8 RGB array | tensor] of any sizes; ``model``: an eval-mode detection model on
    the GPU.  -> one (k, 6) device tensor ``x1 y1 x2 y2 score label`` per image, native pixels, descending score.

    ``conf`` / ``iou`` / ``classes`` / ``agnostic`` / ``max_det`` / ``augment`` are those of the per-tile prediction; ``merge_iou`` and
    ``metric`` ('ios': intersection over the smaller box, which also removes the truncated piece a neighbouring tile reports of an
    object; 'iou') those of the merge across tiles; ``full_image`` adds one letterboxed pass over the whole frame (large objects no
    tile holds); ``batch`` = tiles per forward."""
    tile = check_tile(tile, model_stride(model))
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    dev = next(model.parameters()).device
    results = []
    for lo in range(0, len(images), GROUP):
        pool, img_off, sizes = image_pool(images[lo:lo + GROUP], dev)
        plan = plan_tiles(sizes, tile, overlap, full_image)
        K = len(plan["tile_img"])
        forwards, pads = pad_forwards(K, batch)
        x = dev_empty((forwards * batch, 3, tile, tile), torch.float32, dev)
        fill = lambda a, v: np.concatenate([a, np.full((pads,) + a.shape[1:], v, a.dtype)])  # noqa: E731
        tile_gather(pool, img_off, sizes, fill(plan["tile_img"], -1), fill(plan["rects"], 0), fill(plan["geom"], 0), x, tile)
        dets = []
        for f in range(forwards):
            out = _detect_tiles(model, x[f * batch:(f + 1) * batch], conf, iou, classes=classes, agnostic=agnostic, max_det=max_det, augment=augment)
            if len(out) != batch:
                raise RuntimeError(f"the tile forward returned {len(out)} results for {batch} canvases")
            dets += list(out)
        dets = dets[:K]  # whatever the pad canvases produced ends here
        counts = np.asarray([int(d.shape[0]) for d in dets], np.int64)
        per_rec = np.concatenate([[0], np.cumsum(counts)])
        row_off = per_rec[plan["rec_off"]].astype(np.int32)
        row_tile = np.repeat(np.arange(K, dtype=np.int32), counts)
        rows = torch.cat([d.reshape(-1, 6).float() for d in dets], 0).contiguous() if per_rec[-1] else torch.zeros((0, 6), device=dev)
        mapped, order, nkeep = tile_merge(rows, row_off, row_tile, plan["maps"], sizes, merge_iou, metric, agnostic)
        for i in range(len(sizes)):
            results.append(mapped[order[int(row_off[i]):int(row_off[i]) + int(nkeep[i])].long()])
    return results
