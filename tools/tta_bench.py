#!/usr/bin/env python3
"""Single-scale vs test-time augmented eval forward, get_FPS.py protocol (warm-up, then timed ``model(x)`` bracketed by a device
synchronise), both in one process and alternating round by round; fused DEAL-YOLO-N at 640x640, batch 64 by default.

    python tools/tta_bench.py [--weights yolov8n-ASF-P2P2.yaml] [--batch 64] [--imgs 640 640] [--rounds 10] [--iters 20]
    python tools/tta_bench.py --tta-only 50      # only augmented forwards after the warm-up (a rocprofv3 --kernel-trace run)

Prints one JSON line: images/s of both, their ratio, and the device time of each stage of one augmented forward (events)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ultralytics import YOLO  # noqa: E402
from ultralytics.hip import tta  # noqa: E402


def timed(fn, n):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def stages(model, x):
    """Device time (ms) of each stage of one recorded augmented forward: scale_img / forward per pass, then the merge."""
    plan = tta.tta_plan_for(model, x)
    assert plan is not None, "no recorded TTA plan yet"
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
    names, k = [], 0
    ev[k].record()
    ys = []
    with torch.no_grad():
        for i, (p, ip) in enumerate(zip(plan.geo, plan.plans)):
            if tta._is_identity(p):
                ys.append(ip(x))
            else:
                tta.scale_into(x, p, ip.img)
                k += 1
                ev[k].record()
                names.append(f"scale_img{i} ({p['Hp']}x{p['Wp']})")
                ys.append(ip(ip.img))
            k += 1
            ev[k].record()
            names.append(f"forward{i} ({p['Hp']}x{p['Wp']})")
        tta.merge(ys, plan.geo, x.shape[2], x.shape[3])
        k += 1
        ev[k].record()
        names.append("merge")
    torch.cuda.synchronize()
    return {n: round(ev[i].elapsed_time(ev[i + 1]), 4) for i, n in enumerate(names)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", default="yolov8n-ASF-P2P2.yaml")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--imgs", nargs=2, type=int, default=[640, 640])
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tta-only", type=int, default=0)
    opt = ap.parse_args()
    torch.manual_seed(0)
    model = YOLO(opt.weights).model.cuda().eval()
    model.fuse()
    x = torch.rand(opt.batch, 3, *opt.imgs, device="cuda")
    single = lambda: model(x)  # noqa: E731
    aug = lambda: model(x, augment=True)  # noqa: E731
    with torch.no_grad():
        if opt.tta_only:
            timed(aug, opt.warmup)
            t = timed(aug, opt.tta_only)
            print(json.dumps({"tta_ms": round(1e3 * float(np.mean(t)), 4), "forwards": opt.tta_only}))
            return
        timed(single, opt.warmup)
        timed(aug, opt.warmup)
        ts, ta = [], []
        for _ in range(opt.rounds):
            ts += timed(single, opt.iters)
            ta += timed(aug, opt.iters)
        st = stages(model, x)
    fs, fa = opt.batch / float(np.mean(ts)), opt.batch / float(np.mean(ta))
    print(json.dumps({"weights": opt.weights, "batch": opt.batch, "imgs": opt.imgs, "fused": True,
                      "single_ms": round(1e3 * float(np.mean(ts)), 4), "tta_ms": round(1e3 * float(np.mean(ta)), 4),
                      "single_fps": round(fs, 1), "tta_fps": round(fa, 1), "ratio": round(fa / fs, 4), "target_ratio": 0.40,
                      "stages_ms": st, "timed_forwards": len(ts) + len(ta)}))


if __name__ == "__main__":
    main()
