#!/usr/bin/env python3
"""The per-image two-stage loop next to the batched, dataset-level flow (ultralytics/utils/double_inference.py) on
64 synthetic 1920x1080 images with 8 seeded first-stage detections each, the same model and first-stage predictions for both.

  flows     ``double_inference`` called per image  vs  ``double_inference_batch`` on chunks of 16 images (what ``evaluate_two_stage``
            runs), alternating in one process after a warm-up of both; host clock around ``passes`` passes over all images that end in a device
            synchronise; the second-stage forwards and their distinct input shapes are counted with a forward hook in a pass of their
            own, and the results of the two flows are compared
  kernels   device events around ``reps`` launches: dy_two_stage_merge on one chunk's tables; dy_crop_letterbox_u8_multi on one chunk's
            crops beside dy_crop_letterbox_u8 launched once per image for the same crops

Each leg runs in a child process of its own under a time limit; the parent never opens the device.

usage: two_stage_eval_bench.py [--out profiles/r13_two_stage_eval.md] [--images 64] [--dets 8] [--chunk 16] [--rounds 5] [--passes 5] [--reps 50]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "experiment-yolo_amd"))
import numpy as np  # noqa: E402

H, W = 1080, 1920
LEG_SECONDS = {"flows": 420, "kernels": 120}


def synth(n_img, n_det, seed=0):
    rng = np.random.default_rng(seed)
    images, preds, labels = [], [], []
    for _ in range(n_img):
        images.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        c = np.stack([rng.uniform(60, W - 60, n_det), rng.uniform(60, H - 60, n_det)], 1)
        wh = rng.uniform(10, 100, (n_det, 2))
        boxes = np.concatenate([c - wh / 2, c + wh / 2], 1)
        cls = rng.integers(0, 6, n_det)
        preds.append({"boxes": boxes.tolist(), "scores": rng.uniform(0.3, 0.8, n_det).tolist(), "labels": cls.tolist()})
        labels.append(np.concatenate([cls.reshape(-1, 1), boxes + rng.normal(0, 3, boxes.shape)], 1).astype(np.float32))
    return images, preds, labels


def timed_launches(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def med(a):
    return float(np.median(a))


def spread(a):
    return f"{min(a):.4f} .. {max(a):.4f}"


def leg_flows(o):
    import torch
    from ultralytics.nn.tasks import DetectionModel
    from ultralytics.utils import double_inference as di
    images, preds, labels = synth(o.images, o.dets)
    dev_images = [torch.from_numpy(im).cuda() for im in images]  # both flows start from device-resident images
    torch.manual_seed(0)
    model = DetectionModel("yolov8n-ASF-P2P2.yaml", verbose=False).cuda().eval()
    model.fuse()

    def per_image():
        return [di.double_inference(dev_images[i], model, preds[i])[0] for i in range(o.images)]

    def batched():
        out = []
        for lo in range(0, o.images, o.chunk):
            sl = slice(lo, lo + o.chunk)
            out += di.double_inference_batch(dev_images[sl], model, preds[sl], labels[sl])[0]
        return out

    shapes = {}
    for name, fn in (("per image", per_image), ("batched", batched)):
        fn()  # warm-up: records the plans of every shape the flow uses
        seen = []
        hook = model.register_forward_pre_hook(lambda m, args: seen.append(tuple(args[0].shape)))
        res = fn()
        hook.remove()
        shapes[name] = (len(seen), len(set(seen)), res)
    a, b = shapes["per image"][2], shapes["batched"][2]
    same = sum(len(x["boxes"]) == len(y["boxes"]) and x["labels"] == y["labels"]
               and (not x["boxes"] or (np.abs(np.array(x["boxes"]) - np.array(y["boxes"])).max() <= 1e-3
                                       and np.abs(np.array(x["scores"]) - np.array(y["scores"])).max() <= 1e-6)) for x, y in zip(a, b))
    t = {"per image": [], "batched": []}
    for _ in range(o.rounds):
        for name, fn in (("per image", per_image), ("batched", batched)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(o.passes):
                fn()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) / (o.passes * o.images))
    lines = [f"flows: {o.images} images of {W}x{H}, {o.dets} first-stage detections each, chunks of {o.chunk}; {o.rounds} rounds of {o.passes} passes, alternating",
             "", "| flow | median s per image | range over rounds | second-stage forwards per pass | distinct input shapes |", "|---|---|---|---|---|"]
    for name in ("per image", "batched"):
        lines.append(f"| {name} | {med(t[name]):.5f} | {min(t[name]):.5f} .. {max(t[name]):.5f} | {shapes[name][0]} | {shapes[name][1]} |")
    lines += ["", f"images whose refined detections agree between the flows (boxes 1e-3, scores 1e-6, labels exact): {same} of {o.images}"]
    return lines


def leg_kernels(o):
    import torch
    from ultralytics.hip import check, lib
    from ultralytics.utils import double_inference as di
    images, preds, labels = synth(o.chunk, o.dets)
    dev = torch.device("cuda:0")
    pool, img_off, sizes = di.image_pool(images, dev)
    plan = di.plan_two_stage_chunk(preds, sizes)
    K = len(plan["crop_img"])
    out = torch.zeros((K, 640, 640, 3), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    offs, hw, cimg, rects, geom = t(img_off), t(np.asarray(sizes, np.int32)), t(plan["crop_img"]), t(plan["rects"]), t(plan["geom"])
    dev_images = [t(im) for im in images]
    co = plan["crop_off"]

    def crop_multi():
        check(lib().dy_crop_letterbox_u8_multi(pool.data_ptr(), offs.data_ptr(), hw.data_ptr(), cimg.data_ptr(), rects.data_ptr(), geom.data_ptr(), K,
                                               640, out.data_ptr(), stream), "dy_crop_letterbox_u8_multi")

    def crop_single():
        for b in range(o.chunk):
            if co[b + 1] > co[b]:
                check(lib().dy_crop_letterbox_u8(dev_images[b].data_ptr(), H, W, rects.data_ptr() + 16 * int(co[b]), geom.data_ptr() + 16 * int(co[b]),
                                                 int(co[b + 1] - co[b]), 640, out.data_ptr() + 640 * 640 * 3 * int(co[b]), stream), "dy_crop_letterbox_u8")

    crop_multi()
    ref = out.clone()
    out.zero_()
    crop_single()
    same = bool((out == ref).all())
    k_multi, k_single = [], []
    for _ in range(o.rounds):
        k_multi.append(timed_launches(crop_multi, o.reps))
        k_single.append(timed_launches(crop_single, o.reps))
    # the merge kernel on the chunk's tables: every crop found, refined = the label box at a higher score
    lab = np.concatenate(labels, 0)
    refined = t(np.concatenate([lab[plan["crop_row"], 1:], np.full((K, 1), 0.9, np.float32), lab[plan["crop_row"], :1]], 1).astype(np.float32))
    found = torch.ones(K, dtype=torch.int32, device=dev)
    N, M = o.chunk, len(plan["rows"])
    lab_off = np.arange(N + 1, dtype=np.int32) * o.dets
    itab = t(np.concatenate([plan["row_off"], plan["crop_off"], lab_off, plan["crop_row"]]))
    rows0, rows, labd = t(plan["rows"]), t(plan["rows"]), t(lab)
    keep = torch.zeros(M, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(3 * N + 1, dtype=torch.int32, device=dev)
    ip = itab.data_ptr()

    def merge():
        check(lib().dy_two_stage_merge(rows.data_ptr(), ip, refined.data_ptr(), found.data_ptr(), ip + 12 * (N + 1), ip + 4 * (N + 1), 1, 0.45,
                                       labd.data_ptr(), ip + 8 * (N + 1), 0.5, N, keep.data_ptr(), cnt.data_ptr(), cnt.data_ptr() + 12 * N, stream),
              "dy_two_stage_merge")

    merge()
    k_merge = [timed_launches(merge, o.reps) for _ in range(o.rounds)]
    rows.copy_(rows0)
    merge()
    c = cnt.cpu().numpy()
    return [f"kernels: one chunk of {o.chunk} images, {K} crops of 640x640; {o.rounds} rounds of {o.reps} launches, device events", "",
            "| leg | median ms | range over rounds |", "|---|---|---|",
            f"| dy_crop_letterbox_u8_multi, one launch for the chunk | {med(k_multi):.4f} | {spread(k_multi)} |",
            f"| dy_crop_letterbox_u8, one launch per image ({o.chunk} launches) | {med(k_single):.4f} | {spread(k_single)} |",
            f"| dy_two_stage_merge, one launch for the chunk ({M} rows, {len(lab)} labels) | {med(k_merge):.4f} | {spread(k_merge)} |", "",
            f"crops of the two kernels byte-equal: {same}; merge counts tp {int(c[0:3 * N:3].sum())} fp {int(c[1:3 * N:3].sum())} "
            f"fn {int(c[2:3 * N:3].sum())}, status {int(c[-1])}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_two_stage_eval.md"))
    ap.add_argument("--leg", choices=sorted(LEG_SECONDS))
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--dets", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    o = ap.parse_args()
    if o.leg is None:  # the driver: one child per leg, each under its own limit; the first failure ends the run
        for leg, limit in LEG_SECONDS.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg] + sys.argv[1:], timeout=limit)
            if r.returncode != 0:
                sys.exit(f"leg {leg} failed with status {r.returncode}")
        return
    import torch
    assert torch.cuda.is_available(), "two_stage_eval_bench.py measures on the GPU"
    lines = (leg_flows if o.leg == "flows" else leg_kernels)(o)
    print("\n".join(lines))
    if o.out:
        with open(o.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
