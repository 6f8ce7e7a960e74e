#!/usr/bin/env python3
"""Training-step time of DEAL-YOLO-N (yolov8n-ASF-P2P2) at 640x640, batch 64, hipGraph, under the default box loss (wiou+nwd, the
legacy box_loss_kernel<false>) and under extended modes of the box-loss menu (box_loss_kernel<true>), and the time of
dy_detection_loss alone in each mode.

    python tools/boxloss_bench.py [--modes default w_SIoU_v3_focaler b_EIoU_inner w_MPDIoU_v2_nwd] [--steps 30] [--loss-iters 50]

Each mode gets its own model and StepPlan (a captured graph freezes its box loss).  The step is bench.py's: synthetic batch in the
plan's input buffer, SGD, warm-up, then settling until the loss-scale search has stopped skipping steps.  ``dy_detection_loss alone``
re-issues the plan's own loss launch (its argument block as the step left it) between events.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

# mode name -> BboxLoss settings; "default" is bench.py's north-star wiou+nwd (legacy modes only: runs on trees without the menu)
MODES = {
    "default": dict(use_wiseiou=True, nwd_loss=True),
    "w_SIoU_v3_focaler": dict(use_wiseiou=True, nwd_loss=False, wise=("SIoU", False, False, True)),
    "b_EIoU_inner": dict(use_wiseiou=False, nwd_loss=False, iou_type="EIoU", iou_variant="inner"),
    "w_MPDIoU_v2_nwd": dict(use_wiseiou=True, nwd_loss=True, wise=("MPDIoU", True, False, False)),
}


def synth_batch(seed, B, S, nc, n_per=8):
    g = torch.Generator().manual_seed(seed)
    n = B * n_per
    return dict(img=torch.rand(B, 3, S, S, generator=g), batch_idx=torch.arange(B).repeat_interleave(n_per).float(),
                cls=torch.randint(0, nc, (n, 1), generator=g).float(),
                bboxes=torch.cat([torch.rand(n, 2, generator=g) * 0.7 + 0.15, torch.rand(n, 2, generator=g) * 0.3 + 0.05], 1))


def set_mode(bl, spec):
    bl.use_wiseiou, bl.nwd_loss = spec["use_wiseiou"], spec["nwd_loss"]
    if "wise" in spec:
        from ultralytics.utils.metrics import WiseIouLoss
        bl.wiou_loss = WiseIouLoss(*spec["wise"])
    if "iou_type" in spec:
        bl.iou_type, bl.iou_variant = spec["iou_type"], spec["iou_variant"]


def run_mode(name, a):
    from ultralytics.hip import lib
    from ultralytics.hip.train import StepPlan
    from ultralytics.nn.tasks import DetectionModel
    torch.manual_seed(0)
    model = DetectionModel(os.path.join(ROOT, "experiment-yolo_amd/ultralytics/cfg/models/yolov8n-ASF-P2P2.yaml"), verbose=False).cuda().train()
    for k, v in model.named_parameters():
        v.requires_grad = ".dfl" not in k
    plan = StepPlan(model, a.batch, a.imgsz, nmax=8, optimizer="SGD", use_graph=True)
    set_mode(plan.crit.bbox_loss, MODES[name])
    batch = {k: v.cuda() for k, v in synth_batch(1, a.batch, a.imgsz, 6).items()}
    plan.img.copy_(batch["img"])
    batch["img"] = plan.img
    lr, mom, wd = [0.01] * 3, 0.937, [0.0, 0.0005, 0.0]

    def one_step():
        plan.set_hyper(lr, mom, wd)
        plan.forward_backward(batch)
        plan.optimizer_step()

    for _ in range(a.warmup):
        one_step()
    settle, still, last = 0, 0, float(plan.state[6])
    while still < 8 and settle < 100:
        one_step()
        settle += 1
        now = float(plan.state[6])
        still, last = (still + 1, last) if now == last else (0, now)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        one_step()
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) / a.steps * 1e3
    assert bool(torch.isfinite(plan.crit.scalars[5:9]).all()), f"{name}: non-finite loss"
    # dy_detection_loss alone: the plan's own launch, re-issued on the current stream
    fn, args = lib().dy_detection_loss, C.byref(plan.crit._args)
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(5):
        fn(args, stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.loss_iters):
        fn(args, stream)
    e1.record()
    torch.cuda.synchronize()
    loss_ms = e0.elapsed_time(e1) / a.loss_iters
    out = {"step_ms": round(step_ms, 4), "images_per_s": round(a.batch / step_ms * 1e3, 1), "loss_call_ms": round(loss_ms, 4),
           "box_family": int(getattr(plan.crit._args, "box_family", 0))}
    del plan, model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=list(MODES))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--loss-iters", type=int, default=50)
    a = ap.parse_args()
    res = {m: run_mode(m, a) for m in a.modes}
    print(json.dumps({"workload": f"yolov8n-ASF-P2P2 train step {a.imgsz}x{a.imgsz} batch {a.batch}, hipGraph", "steps": a.steps,
                      "modes": res}))


if __name__ == "__main__":
    main()
