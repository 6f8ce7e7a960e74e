#!/usr/bin/env python3
"""One validation pass inside training, timed three ways, DEAL-YOLO-N at 640x640 on synthetic planted-rectangle data held on the device:

  (a) fresh ema.ema + validator    what the trainer did for its one validation after the last epoch: a new DetectionModel from the YAML,
                                   every tensor through the host, a new Runtime, new weight packs, new InferPlans (validator(model=...));
                                   the loss comes from model.loss(batch, preds) with the logits materialised
  (b) persistent + materialize()   ModelEMA.eval_model() refreshed from the flat EMA buffers, the plain fused Detect tail, the logits
                                   written by two eager conv launches per level when the loss asks (DY_HEAD_INFER_LOGITS=0)
  (c) persistent + fused logits    the same model, the Detect tail writes y and the logits in its one launch (the default)

The legs alternate (a, b, c, a, b, c, ...) in one process after one untimed pass each; every leg is the host clock around the whole pass
(model refresh or construction, all batches, NMS, matching, get_stats) ending in a device synchronise.  (b) and (c) must return the same
numbers.  Then the two head entry points stand-alone at the same geometry (B x 160^2 / 80^2 / 40^2 / 20^2 pixels at 640x640, nc 6): device
events around ``reps`` launches, legs alternating, plus the two eager final convs per level that materialize() issues.

usage: val_epoch_bench.py [--out profiles/r12_val_epoch.md] [--rounds 5] [--batches 8] [--batch 16] [--imgsz 640] [--reps 50]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

MODEL = os.path.join(ROOT, "experiment-yolo_amd", "ultralytics", "cfg", "models", "yolov8n-ASF-P2P2.yaml")


def device_batches(n, B, S, nc):
    from golden.cases import planted_batches
    out = []
    for b in planted_batches(7, n, B, S, nc):
        out.append({k: torch.from_numpy(v).cuda() for k, v in b.items()})
    return out


def fmt(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    from ultralytics.engine.trainer import DetectionTrainer
    from ultralytics.models.yolo.detect import DetectionValidator
    from ultralytics.nn.modules import head
    from ultralytics.nn.tasks import DetectionModel
    nc = 6
    torch.manual_seed(0)
    model = DetectionModel(MODEL, nc=nc, verbose=False)
    tr = DetectionTrainer(model, overrides=dict(optimizer="SGD", amp=False, epochs=1, val_period=1, plots=False, nmax=8))
    data = device_batches(a.batches, a.batch, a.imgsz, nc)
    tr.setup(len(data), a.batch, a.imgsz)
    for i, b in enumerate(data[:4]):  # a few optimizer steps: the EMA differs from the initial weights
        tr.train_step(b, i, 0)
    torch.cuda.synchronize()
    tr.epoch, tr.save_dir = 0, None
    tr._begin_val_loop()
    v = DetectionValidator(dataloader=data, args=tr.args)

    def leg_a():
        m = tr.ema.ema
        loss = torch.zeros(3, device="cuda")
        v.device = torch.device("cuda:0")
        m.to(v.device).eval()
        m.args = tr.args
        v.init_metrics(m)
        v.plots_gate = None
        with torch.no_grad():
            for batch in data:
                batch = v.preprocess(dict(batch))
                preds = m(batch["img"])
                loss += m.loss(batch, preds)[1]
                v.update_metrics(v.postprocess(preds), batch)
        stats = v.get_stats()
        return stats, (loss.cpu() / len(data)).tolist()

    def leg_persistent(fused):
        head.HEAD_INFER_LOGITS = fused
        res = v(trainer=tr)
        return res, [res[k] for k in ("val/box_loss", "val/cls_loss", "val/dfl_loss")]

    legs = [("(a) fresh ema.ema + validator", leg_a), ("(b) persistent + materialize()", lambda: leg_persistent(False)),
            ("(c) persistent + fused logits", lambda: leg_persistent(True))]
    import io
    from contextlib import redirect_stdout
    times, results = {n: [] for n, _ in legs}, {}
    for rnd in range(a.rounds + 1):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with redirect_stdout(io.StringIO()):
                results[name] = fn()
            torch.cuda.synchronize()
            if rnd:  # round 0: untimed (library loading, first plans of (b) / (c))
                times[name].append((time.perf_counter() - t0) * 1e3)
    head.HEAD_INFER_LOGITS = True
    rb, rc = results[legs[1][0]], results[legs[2][0]]
    assert rb == rc, "the fused-logits pass and the materialize() pass disagree"
    lines = ["# One validation pass inside training: fresh model, persistent model, fused logits; one MI355X", "",
             f"`python tools/val_epoch_bench.py --rounds {a.rounds} --batches {a.batches} --batch {a.batch} --imgsz {a.imgsz} --reps {a.reps}`: "
             f"DEAL-YOLO-N, {a.batches} batches of {a.batch} images {a.imgsz}x{a.imgsz} resident on the device, nc {nc}; legs alternating in one process, "
             "one untimed pass each first; host clock around the whole pass, ms, median (min .. max).", "",
             "| leg | ms per validation pass |", "|---|---|"]
    for name, _ in legs:
        lines.append(f"| {name} | {fmt(times[name])} |")
    lines += ["", f"val losses (b) = (c): {rc[1]}; (a): {[round(x, 5) for x in results[legs[0][0]][1]]}", ""]

    # ---- the head stand-alone
    m = tr.ema.eval_model()
    x = data[0]["img"].float()
    with torch.no_grad():
        m(x), m(x)
        plan = m._infer_plans["plans"][tuple(x.shape)]
        ho = plan.ho

    def ev(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.reps * 1e3

    y = ho.infer()

    def plain_then_fill():
        ho.infer(y)
        ho.logits_current = False
        ho.fill_box()

    hlegs = [("dy_head_infer_levels (y only)", lambda: ho.infer(y)), ("dy_head_infer_levels_logits (y + logits)", lambda: ho.infer(y, logits=True)),
             ("dy_head_infer_levels + materialize() (1 + 2 x nl launches)", plain_then_fill)]
    ht = {n: [] for n, _ in hlegs}
    for rnd in range(a.rounds + 1):
        for name, fn in hlegs:
            t = ev(fn)
            if rnd:
                ht[name].append(t)
    A = y.shape[2]
    lines += [f"## The Detect tail stand-alone (batch {a.batch}, {A} anchors per image, device events around {a.reps} launches, us per call)", "",
              "| leg | us |", "|---|---|"]
    for name, _ in hlegs:
        lines.append(f"| {name} | {fmt(ht[name])} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
