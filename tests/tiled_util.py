"""Shared by tests/test_host_tiled.py and tests/test_gpu_tiled.py: the numpy statement of dy_tile_merge (every operation in
np.float32, one rounding each) and the planted generator of merge cases."""
import numpy as np

f32 = np.float32


def metric_to_all(box, others, ios):
    """iou_plain (csrc/two_stage_iou.h) / its intersection-over-smaller variant of one box against (n, 4) boxes, fp32 throughout."""
    x1, y1 = np.maximum(box[0], others[:, 0]), np.maximum(box[1], others[:, 1])
    x2, y2 = np.minimum(box[2], others[:, 2]), np.minimum(box[3], others[:, 3])
    inter = (x2 - x1) * (y2 - y1)
    a1, a2 = (box[2] - box[0]) * (box[3] - box[1]), (others[:, 2] - others[:, 0]) * (others[:, 3] - others[:, 1])
    den = np.minimum(a1, a2) if ios else a1 + a2 - inter
    ok = (x2 > x1) & (y2 > y1) & (a1 > 0) & (a2 > 0) & (den > 0)
    return np.where(ok, inter / np.where(ok, den, f32(1)), f32(0)).astype(f32)


def merge_reference(rows, row_tile, maps, H, W, thr, ios=True, agnostic=False):
    """One image.  rows (n, 6) canvas coordinates, row_tile (n) -> maps (Kt, 6) x1 y1 pad_x pad_y r 1/r.
    -> (mapped rows (n, 6) fp32, kept row indices in sweep order, rows that entered the sweep)."""
    rows = np.asarray(rows, f32).reshape(-1, 6)
    m = np.asarray(maps, f32).reshape(-1, 6)[np.asarray(row_tile, np.int64).reshape(-1)]
    out = rows.copy()
    for c, (org, pad, lim) in enumerate(((0, 2, W), (1, 3, H), (0, 2, W), (1, 3, H))):
        out[:, c] = np.clip((rows[:, c] - m[:, pad]).astype(f32) / m[:, 4] + m[:, org], f32(0), f32(lim))
    valid = np.flatnonzero((out[:, 2] - out[:, 0] > 0) & (out[:, 3] - out[:, 1] > 0))
    idx = np.asarray(sorted(valid.tolist(), key=lambda i: (-out[i, 4], i)), np.int64)
    alive, keep = np.ones(len(idx), bool), []
    for t, i in enumerate(idx):
        if not alive[t]:
            continue
        keep.append(int(i))
        later = idx[t + 1:]
        hit = metric_to_all(out[i, :4], out[later, :4], ios) > f32(thr)
        if not agnostic:
            hit &= out[later, 5] == out[i, 5]
        alive[t + 1:] &= ~hit
    return out, keep, len(idx)


def planted_case(seed, H=100, W=150, tile=64, overlap=0.25, n_obj=14):
    """A frame with planted objects as its tiles and the whole-image pass would report them.  -> (rows (n, 6) fp32 in canvas
    coordinates, row_tile (n), maps (Kt, 6), (H, W)).  Every tile reports, with probability 0.85, its part of every object that is at
    least 2 px wide and high there (jittered by up to 1 px); the whole-image pass reports all of them scaled (jittered by up to 0.5);
    scores are sixteenths, so ties are common."""
    from ultralytics.utils.tiled import plan_tiles
    rng = np.random.default_rng(seed)
    plan = plan_tiles([(H, W)], tile, overlap, True)
    half = rng.integers(3, 15, (n_obj, 2)).astype(np.float64)
    cxy = np.stack([rng.uniform(0, W, n_obj), rng.uniform(0, H, n_obj)], 1)
    boxes = np.concatenate([cxy - half, cxy + half], 1).clip(0, [W, H, W, H])
    labels = rng.integers(0, 3, n_obj)
    rows, row_tile = [], []
    for k, ((x1, y1, x2, y2), (nw, nh, px, py)) in enumerate(zip(plan["rects"].tolist(), plan["geom"].tolist())):
        full = k == len(plan["rects"]) - 1
        for b, l in zip(boxes, labels):
            score = rng.integers(4, 17) / 16
            if full:
                r = float(plan["maps"][k, 4])
                box = b * r + [px, py, px, py] + rng.uniform(-0.5, 0.5, 4)
            else:
                part = np.array([max(b[0], x1), max(b[1], y1), min(b[2], x2), min(b[3], y2)])
                if part[2] - part[0] < 2 or part[3] - part[1] < 2 or rng.random() >= 0.85:
                    continue
                box = part - [x1, y1, x1, y1] + rng.uniform(-1, 1, 4)
            rows.append([*box, score, l])
            row_tile.append(k)
    return np.asarray(rows, f32).reshape(-1, 6), np.asarray(row_tile, np.int32), plan["maps"], (H, W)
