#!/usr/bin/env python3
"""Sliced inference (ultralytics/utils/tiled.py) measured on one MI355X, written as a markdown report.

  gather   dy_tile_gather_f32 on the records of 8 frames of 3840x2160 (tile 640, overlap 0.2: 32 tiles + the whole-frame pass each, 264
           records), device events around ``reps`` launches after a warm-up; bytes = 15 per output pixel (3 read, 12 written), as a share
           of the 8.0 TB/s HBM peak.  Beside it, alternating: dy_crop_letterbox_u8_multi on the same records and the ATen
           ``permute().float() / 255`` pass over its output -- what fed the forward before.
  merge    dy_tile_merge at 300 / 2,000 / 8,192 rows per image for 1 and 8 images: disjoint boxes (every row survives, so every step of
           the sweep is a pivot: the sequential worst case) and clusters of four duplicates (three rows in four suppressed).
  flow     ``tiled_predict`` per frame against the same job through the public interface as it was before this module: tiles cut on
           the host, ``YOLO.predict`` on them (imgsz 640, the same batch) plus one ``predict`` of the whole frame, boxes moved to frame
           coordinates on the host, ``torchvision_nms`` per frame.  Alternating in one process, host clock around passes that end in a
           device synchronise, once with a fresh model (no detections: the cost of moving pixels and of the forwards) and once with
           the class biases zeroed (every anchor a candidate: the NMS of every tile at its worst).  The gather's share of the flow
           closes each table.

usage: tiled_bench.py [--out profiles/r14_tiled.md] [--frames 2] [--batch 16] [--rounds 3] [--passes 2] [--reps 20]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "experiment-yolo_amd"))
import numpy as np  # noqa: E402

H, W, TILE, OVERLAP = 2160, 3840, 640, 0.2
HBM_PEAK = 8.0e12
MAX_DET = 50  # per tile: 33 records stay under dy_nms_hard's 2,048 rows, which the baseline's merge goes through


def events(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us


def med(a):
    return float(np.median(a))


def leg_gather(o):
    import torch
    from ultralytics.hip import check, lib
    from ultralytics.utils import double_inference as di, tiled
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8)]
    pool, off, sizes = di.image_pool(images, dev)
    plan = tiled.plan_tiles(sizes, TILE, OVERLAP)
    K = len(plan["tile_img"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    offs, hw, timg, rects, geom = t(off), t(np.asarray(sizes, np.int32)), t(plan["tile_img"]), t(plan["rects"]), t(plan["geom"])
    out = torch.empty((K, 3, TILE, TILE), device=dev)
    u8 = torch.empty((K, TILE, TILE, 3), dtype=torch.uint8, device=dev)
    lut, stream = tiled.byte_table(dev), torch.cuda.current_stream().cuda_stream

    def gather():
        check(lib().dy_tile_gather_f32(pool.data_ptr(), offs.data_ptr(), hw.data_ptr(), timg.data_ptr(), rects.data_ptr(), geom.data_ptr(),
                                       lut.data_ptr(), K, TILE, out.data_ptr(), stream), "dy_tile_gather_f32")

    def crop():
        check(lib().dy_crop_letterbox_u8_multi(pool.data_ptr(), offs.data_ptr(), hw.data_ptr(), timg.data_ptr(), rects.data_ptr(), geom.data_ptr(),
                                               K, TILE, u8.data_ptr(), stream), "dy_crop_letterbox_u8_multi")

    def convert():
        torch.div(u8.permute(0, 3, 1, 2).float(), 255, out=out)

    gather(), crop()
    same = torch.equal(out, u8.permute(0, 3, 1, 2).float() / 255)
    ts = {"gather": [], "crop": [], "convert": []}
    for _ in range(o.rounds):
        for name, fn in (("gather", gather), ("crop", crop), ("convert", convert)):
            ts[name].append(events(fn, o.reps))
    nbytes = 15 * K * TILE * TILE
    g = med(ts["gather"])
    bw = nbytes / (g * 1e-6)
    lines = [f"## gather: {K} records of 8 frames {W}x{H}, tile {TILE}, overlap {OVERLAP}; {o.rounds} rounds of {o.reps} launches, alternating", "",
             "| pass | median us | range over rounds |", "|---|---|---|"]
    for name, label in (("gather", "dy_tile_gather_f32 (pool -> fp32 planar)"), ("crop", "dy_crop_letterbox_u8_multi (pool -> uint8 HWC)"),
                        ("convert", "ATen permute().float() / 255 of that (uint8 HWC -> fp32 planar)")):
        lines.append(f"| {label} | {med(ts[name]):.1f} | {min(ts[name]):.1f} .. {max(ts[name]):.1f} |")
    lines += ["", f"gather output equals crop + convert bit for bit: {same}",
              f"gather: {nbytes / 1e9:.3f} GB (15 bytes per output pixel) in {g:.1f} us = {bw / 1e12:.2f} TB/s = {bw / HBM_PEAK:.2f} of the {HBM_PEAK / 1e12:.1f} TB/s HBM peak; "
              f"crop + convert together {med(ts['crop']) + med(ts['convert']):.1f} us ({(med(ts['crop']) + med(ts['convert'])) / g:.2f}x)"]
    return lines, g / K


def merge_rows(n, clustered, rng):
    side = 4
    cells = n // 4 if clustered else n
    cols = 256
    cell = np.arange(n) // 4 if clustered else np.arange(n)
    xy = np.stack([(cell % cols) * side, (cell // cols) * side], 1).astype(np.float32)
    rows = np.concatenate([xy, xy + 3, rng.integers(1, 4097, (n, 1)) / 4096, rng.integers(0, 3, (n, 1)) if not clustered else (cell % 3).reshape(-1, 1)], 1)
    return rows.astype(np.float32), (int(cells // cols + 1) * side + 4, cols * side)


def leg_merge(o):
    import torch
    from ultralytics.hip import check, lib
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"## merge: dy_tile_merge, IoS 0.5, per class; {o.rounds} rounds of {o.reps} launches", "",
             "| rows per image | images | boxes | kept per image | median us | range over rounds |", "|---|---|---|---|---|---|"]
    for n in (300, 2000, 8192):
        for N in (1, 8):
            for clustered in (False, True):
                rows, size = merge_rows(n, clustered, rng)
                r = torch.from_numpy(np.tile(rows, (N, 1))).to(dev)
                itab = torch.from_numpy(np.concatenate([np.arange(N + 1) * n, np.zeros(N * n), np.tile(size, N)]).astype(np.int32)).to(dev)
                maps = torch.tensor([0, 0, 0, 0, 1, 1], dtype=torch.float32, device=dev)
                outr = torch.empty((N * n, 6), device=dev)
                ints = torch.zeros(N * n + N + 1, dtype=torch.int32, device=dev)
                ip, op = itab.data_ptr(), ints.data_ptr()

                def merge():
                    check(lib().dy_tile_merge(r.data_ptr(), ip, ip + 4 * (N + 1), maps.data_ptr(), ip + 4 * (N + 1 + N * n), N, 1, n, 0.5, 1, 0,
                                              outr.data_ptr(), op, op + 4 * N * n, op + 4 * (N * n + N), stream), "dy_tile_merge")

                ts = [events(merge, o.reps) for _ in range(o.rounds)]
                kept = ints[N * n:N * n + N].cpu().tolist()
                lines.append(f"| {n} | {N} | {'clusters of 4' if clustered else 'disjoint'} | {kept[0]} | {med(ts):.1f} | {min(ts):.1f} .. {max(ts):.1f} |")
    return lines


def leg_flow(o, gather_us_per_record, saturated):
    import torch
    from ultralytics import YOLO
    from ultralytics.utils import double_inference as di, tiled
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(o.frames)]  # RGB for tiled_predict, read as BGR by predict: same cost
    torch.manual_seed(0)
    yolo = YOLO("yolov8n-ASF-P2P2.yaml")
    if saturated:  # class scores near 0.5: every anchor is a candidate and every tile reports its max_det rows -- the NMS's worst case
        for seq in yolo.model.model[-1].cv3:
            torch.nn.init.zeros_(seq[-1].bias)
    yolo.predict([frames[0][:TILE, :TILE]], imgsz=TILE, batch=1)  # moves the model to the device
    net = yolo.model
    grid = tiled.tile_grid(H, W, TILE, OVERLAP)

    def sliced():
        return tiled.tiled_predict(frames, net, tile=TILE, overlap=OVERLAP, batch=o.batch, max_det=MAX_DET)

    def baseline():
        out = []
        for f in frames:
            tiles = [np.ascontiguousarray(f[y1:y2, x1:x2]) for x1, y1, x2, y2 in grid]
            res = yolo.predict(tiles, imgsz=TILE, batch=o.batch, max_det=MAX_DET)
            parts = [r.boxes.data.cpu().numpy() + np.array([x1, y1, x1, y1, 0, 0], np.float32) for r, (x1, y1, _, _) in zip(res, grid)]
            parts.append(yolo.predict([f], imgsz=TILE, batch=1, max_det=MAX_DET)[0].boxes.data.cpu().numpy())
            rows = np.concatenate(parts, 0)
            out.append(di.torchvision_nms(rows[:, :4].tolist(), rows[:, 4].tolist(), rows[:, 5].astype(int).tolist(), 0.5, device="cuda:0"))
        return out

    a, b = sliced(), baseline()
    sliced(), baseline()  # second warm-up: the plans of both flows' shapes are recorded on the second forward of a shape
    ts = {"sliced": [], "baseline": []}
    for _ in range(o.rounds):
        for name, fn in (("sliced", sliced), ("baseline", baseline)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(o.passes):
                fn()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3 / (o.passes * o.frames))
    records = len(grid) + 1
    gather_ms = gather_us_per_record * records * 1e-3
    s, bl = med(ts["sliced"]), med(ts["baseline"])
    what = "class biases zeroed: every anchor a candidate, every tile reports max_det rows" if saturated else "fresh model: no anchor reaches conf 0.25, nothing to merge"
    return [f"## flow ({what}): {o.frames} frames of {W}x{H} per pass, {records} records per frame, {o.batch} tiles per forward, max_det {MAX_DET} per tile; "
            f"{o.rounds} rounds of {o.passes} passes, alternating", "",
            "| flow | median ms per frame | range over rounds | boxes on the first frame |", "|---|---|---|---|",
            f"| tiled_predict (IoS 0.5 merge on the device) | {s:.1f} | {min(ts['sliced']):.1f} .. {max(ts['sliced']):.1f} | {len(a[0])} |",
            f"| host tiles + YOLO.predict + host map-back + torchvision_nms (IoU 0.5) | {bl:.1f} | {min(ts['baseline']):.1f} .. {max(ts['baseline']):.1f} | {len(b[0][0])} |",
            "", f"baseline / tiled_predict = {bl / s:.2f}x",
            f"gather share of the flow: {records} records x {gather_us_per_record:.2f} us = {gather_ms:.3f} ms of {s:.1f} ms per frame = {gather_ms / s:.4f}", ""]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_tiled.md"))
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    o = ap.parse_args()
    lines = ["# Sliced inference: gather, merge and the whole flow (tools/tiled_bench.py)", ""]

    def flush():
        with open(o.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    g_lines, per_record = leg_gather(o)
    lines += g_lines + [""]
    flush()
    lines += leg_merge(o) + [""]
    flush()
    for saturated in (False, True):
        lines += leg_flow(o, per_record, saturated)
        flush()
    print("\n".join(lines))
