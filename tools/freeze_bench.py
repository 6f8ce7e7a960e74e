#!/usr/bin/env python3
"""The bench.py step (DEAL-YOLO-N 640x640, batch 64, hipGraph, wiou+nwd, SGD) under freeze = None / 8 / [12, 20], alternating on one box.

All configurations are built first (one model + one captured step each, in this process), warmed up and settled like bench.py does;
then ROUNDS rounds time STEPS steps of each configuration in turn (A B C A B C ...), so that clock / thermal drift hits all of them
alike.  Reported per configuration: the median round and the min-max spread, the launches recorded behind the loss, and -- with
--profile -- the event-timed device time of the backward launches that name a layer-0..7 buffer in the UNFROZEN list: the saving
freeze=8 can reach at best (its target).
usage: freeze_bench.py [--rounds 7] [--steps 20] [--batch 64] [--imgsz 640] [--profile] [--out freeze_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
import torch  # noqa: E402

from bench import CFG, synth_batch  # noqa: E402
from ultralytics.engine.trainer import frozen_parameter_names  # noqa: E402
from ultralytics.hip.train import StepPlan  # noqa: E402
from ultralytics.nn.tasks import DetectionModel  # noqa: E402

CONFIGS = [("none", None), ("8", 8), ("12_20", [12, 20])]


def build(freeze, a, dev):
    torch.manual_seed(0)
    model = DetectionModel(CFG, verbose=False).to(dev).train()
    frozen = set(frozen_parameter_names([k for k, _ in model.named_parameters()], freeze))
    for k, v in model.named_parameters():
        v.requires_grad = k not in frozen
    plan = StepPlan(model, a.batch, a.imgsz, nmax=8, optimizer="SGD", use_graph=True)
    plan.crit.bbox_loss.use_wiseiou, plan.crit.bbox_loss.nwd_loss = True, True
    batch = {k: v.to(dev) for k, v in synth_batch(1, a.batch, a.imgsz, 6).items()}
    plan.img.copy_(batch["img"])
    batch["img"] = plan.img

    def one_step():
        plan.set_hyper([0.01] * 3, 0.937, [0.0, 0.0005, 0.0])
        plan.forward_backward(batch)
        plan.optimizer_step()

    for _ in range(5):
        one_step()
    settle, still, last = 0, 0, float(plan.state[6])
    while still < 8 and settle < 100:  # bench.py: until the loss-scale search has stopped skipping steps
        one_step()
        settle += 1
        now = float(plan.state[6])
        still, last = (still + 1, last) if now == last else (0, now)
    return model, plan, batch, one_step


def prefix_backward_ms(model, plan, batch, layers=range(8)):
    """Device ms (HIP events, un-captured replay) of the backward launches that name a buffer of a convolution in ``layers``."""
    rt = plan.rt
    ptrs = set()
    for i in layers:
        for mod in model.model[i].modules():
            sp = rt.specs.get(id(mod))
            if sp is not None:
                ptrs |= {t.data_ptr() for t in (sp.weight, sp.wpack, sp.wpack_t, sp.coef, sp.acc_b, sp.gweight, sp.gbn_w) if t is not None}
    back = {id(op[1]) for op in plan.rec_fb.ops[plan.fb_split:] if op[0] is not None}
    tot, n = 0.0, 0
    for name, args, ms in plan.profile_ops(3):
        if id(args) in back and any(isinstance(v, int) and v in ptrs for v in args):
            tot, n = tot + ms, n + 1
    return tot, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    built = {tag: build(fr, a, dev) for tag, fr in CONFIGS}
    times = {tag: [] for tag, _ in CONFIGS}
    for _ in range(a.rounds):
        for tag, _fr in CONFIGS:  # alternating: every round times every configuration once
            one_step = built[tag][3]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                one_step()
            torch.cuda.synchronize()
            times[tag].append((time.perf_counter() - t0) / a.steps * 1e3)
    out = {"batch": a.batch, "imgsz": a.imgsz, "rounds": a.rounds, "steps": a.steps, "configs": {}}
    for tag, fr in CONFIGS:
        model, plan, batch, _ = built[tag]
        plan.check_progress()
        t = times[tag]
        ops = [op for op in plan.rec_fb.ops if op[0] is not None]
        out["configs"][tag] = {"freeze": fr, "ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                               "ms_rounds": [round(v, 4) for v in t], "launches": len(ops),
                               "backward_launches": len([op for op in plan.rec_fb.ops[plan.fb_split:] if op[0] is not None]),
                               "dgrad_only_launches": sum(op[2] == "dy_conv1x1_dgrad_bn" for op in ops),
                               "weight_gradient_reductions": len(plan.wgrad_specs)}
        print(f"freeze={fr}: {statistics.median(t):.3f} ms/step (min {min(t):.3f}, max {max(t):.3f}), {len(ops)} launches", flush=True)
    if a.profile:
        model, plan, batch, _ = built["none"]
        ms, n = prefix_backward_ms(model, plan, batch)
        out["target_ms_layers_0_7_backward"] = round(ms, 4)
        out["target_launches"] = n
        base = out["configs"]["none"]["ms_median"]
        print(f"target for freeze=8: {ms:.3f} ms in {n} backward launches of layers 0-7 (event-timed, unfrozen list); "
              f"measured saving {base - out['configs']['8']['ms_median']:.3f} ms", flush=True)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
