#!/usr/bin/env python3
"""What optimizer='SOAP' adds to a training step, measured: the bench.py configuration (DEAL-YOLO-N 640x640, batch 64, WIoU+NWD)
under three settings in one process, alternating round by round:

    soap_host   optimizer='SOAP', DY_SOAP_HIP=0   the host-driven restatement (ultralytics/hip/soap.py, class Soap)
    soap_hip    optimizer='SOAP', DY_SOAP_HIP=1   the grouped HIP kernels (csrc/soap.hip, class SoapHip)
    sgd         optimizer='SGD'                   the same launch lists, run eagerly like the SOAP plans (SOAP steps are not captured)

usage: soap_bench.py [--rounds 5] [--batch 64] [--imgsz 640] [--lr 0.001] [--out FILE]

SOAP refreshes its eigenbases every tenth step, so a round times, per setting, two cycles of: the nine steady steps after a refresh
as one window (host clock around work that ends in a device synchronise, divided by nine), then the refresh step alone.  A row is
the median over the rounds, its spread max - min over the rounds; "adds" is a SOAP row minus the SGD row of the same kind.  The SOAP
part alone (``StepPlan._soap_step`` between two synchronisations, steady steps) is timed afterwards, and the device path's launches
per steady step are read from its counter.  The float64 QR of a refresh is timed batched per matrix size, as the optimizer calls
it, and matrix by matrix.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
import ultralytics.hip  # noqa: E402,F401
import torch  # noqa: E402


def build(setting, a):
    from bench import CFG, synth_batch
    from ultralytics.hip.train import StepPlan
    from ultralytics.nn.tasks import DetectionModel
    os.environ["DY_SOAP_HIP"] = "0" if setting == "soap_host" else "1"  # read when the optimizer object is built (first step)
    torch.manual_seed(0)
    model = DetectionModel(CFG, verbose=False).cuda().train()
    for k, v in model.named_parameters():
        v.requires_grad = ".dfl" not in k
    soap = setting != "sgd"
    plan = StepPlan(model, a.batch, a.imgsz, nmax=8, optimizer="SOAP" if soap else "SGD", use_graph=False)
    plan.crit.bbox_loss.use_wiseiou, plan.crit.bbox_loss.nwd_loss = True, True
    batch = {k: v.cuda() for k, v in synth_batch(1, a.batch, a.imgsz, 6).items()}
    plan.img.copy_(batch["img"])
    batch["img"] = plan.img
    lr = [a.lr if soap else 0.01] * 3

    def step():
        plan.set_hyper(lr, 0.937, [0.0, 0.0005, 0.0])
        plan.forward_backward(batch)
        plan.optimizer_step()

    step()  # builds the optimizer object under this setting's switch
    still, last, n = 0, float(plan.state[6]), 0
    while still < 8 and n < 100:  # the loss-scale search, as bench.py lets it settle
        step()
        n += 1
        now = float(plan.state[6])
        still, last = (still + 1, last) if now == last else (0, now)
    return plan, step


def soap_t(plan):
    so = getattr(plan, "_soap", None)
    if so is None:
        return None
    return so.t if hasattr(so, "t") else so.state[0].step


def cycle(plan, step):
    """(ms per steady step over the nine steps after a refresh, ms of the refresh step), None where a step was skipped."""
    while soap_t(plan) is not None and soap_t(plan) % 10 != 0:
        step()
    torch.cuda.synchronize()
    skipped = float(plan.state[6])
    t0 = time.perf_counter()
    for _ in range(9):
        step()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if float(plan.state[6]) != skipped:
        return None
    return (t1 - t0) / 9 * 1e3, (t2 - t1) * 1e3


def soap_part(plan):
    """ms of the SOAP part of a steady step alone, and (device path) its launches."""
    so, g = plan._soap, plan.rt.flat_g
    ts, launches = [], None
    while soap_t(plan) % 10 != 0:
        plan._soap_step(g)
    for _ in range(8):
        before = getattr(so, "launches", None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan._soap_step(g)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        if before is not None:
            launches = so.launches - before
    return statistics.median(ts), launches


def qr_compare(plan):
    """The float64 QR of one refresh of the device path's pools, batched per matrix size (what ``SoapHip._refresh_bases`` calls) and
    matrix by matrix: ms each, whether the two agree bit for bit and the batched call with itself; and one whole refresh, in ms."""
    so = plan._soap
    mats = []
    for n, gg, q, _ in so._pools():
        est = torch.diagonal(q.transpose(1, 2) @ gg @ q, dim1=1, dim2=2)
        idx = torch.argsort(est, dim=1, descending=True, stable=True)
        mats.append((gg @ torch.gather(q, 2, idx[:, None, :].expand_as(q))).double())
    forms = {"batched": lambda m: torch.linalg.qr(m)[0], "loop": lambda m: torch.stack([torch.linalg.qr(a)[0] for a in m])}
    ms, res = {}, {}
    for name, form in (("batched", "batched"), ("loop", "loop"), ("batched_again", "batched")):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = [forms[form](m) for m in mats]
        torch.cuda.synchronize()
        ms[name] = (time.perf_counter() - t0) * 1e3
        res[name] = torch.cat([o.reshape(-1) for o in out])
    keep = [t.clone() for t in (so.basis, so.v, so.order)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    so._refresh_bases()
    torch.cuda.synchronize()
    whole = (time.perf_counter() - t0) * 1e3
    for dst, src in zip((so.basis, so.v, so.order), keep):
        dst.copy_(src)
    return {"batched_ms": ms["batched"], "loop_ms": ms["loop"], "batched_repeat_ms": ms["batched_again"], "whole_refresh_ms": whole,
            "matrices": sum(m.shape[0] for m in mats),
            "batched_is_deterministic": bool(torch.equal(res["batched"], res["batched_again"])),
            "batched_equals_loop_bitwise": bool(torch.equal(res["batched"], res["loop"])),
            "batched_vs_loop_max_abs": float((res["batched"] - res["loop"]).abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--lr", type=float, default=0.001, help="SOAP's learning rate (timing does not depend on it)")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "soap_bench.py measures on the GPU"
    names = ["soap_host", "soap_hip", "sgd"]
    plans = {}
    for s in names:
        plans[s] = build(s, a)
        print(f"[soap_bench] {s} ready", file=sys.stderr, flush=True)
    rows = {s: {"steady": [], "refresh": []} for s in names}
    dropped = 0
    for r in range(a.rounds):
        for s in (names if r % 2 == 0 else names[::-1]):
            for _ in range(2):
                c = cycle(*plans[s])
                if c is None:
                    dropped += 1
                    continue
                rows[s]["steady"].append(c[0])
                rows[s]["refresh"].append(c[1])
        print(f"[soap_bench] round {r + 1}/{a.rounds}: " + ", ".join(f"{s} {rows[s]['steady'][-1]:.2f} / {rows[s]['refresh'][-1]:.2f} ms" for s in names if rows[s]["steady"]),
              file=sys.stderr, flush=True)
    med = lambda v: statistics.median(v) if v else None  # noqa: E731
    res = {"config": f"yolov8n-ASF-P2P2 train step {a.imgsz}x{a.imgsz} batch {a.batch}, wiou+nwd, eager launch lists", "rounds": a.rounds,
           "cycles_dropped_for_skipped_steps": dropped, "ms": {}}
    for s in names:
        res["ms"][s] = {k: {"median": med(v), "min": min(v, default=None), "max": max(v, default=None), "n": len(v)} for k, v in rows[s].items()}
    for s in names[:2]:
        res["ms"][s]["adds"] = {k: (res["ms"][s][k]["median"] - res["ms"]["sgd"][k]["median"]) if rows[s][k] and rows["sgd"][k] else None for k in ("steady", "refresh")}
        part, launches = soap_part(plans[s][0])
        res["ms"][s]["soap_part_steady"] = part
        res["ms"][s]["launches_per_steady_step"] = launches
    res["qr"] = qr_compare(plans["soap_hip"][0])
    for s in names:
        plans[s][0].check_progress()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
