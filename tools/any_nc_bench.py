#!/usr/bin/env python3
"""What a class count outside the multiples of 16 costs: yolov8n-ASF-P2P2 at nc = 32, 37, 40, 48, 100 on one box.

(a) the bench.py protocol's training step (640x640, batch 64, SGD, WIoU + NWD, hipGraph replay): every shape is built and warmed first,
    then the shapes are timed in turn, round after round, so that drift of the box hits all of them alike;
(b) the fused inference forward (model.fuse(), eval, the recorded inference plan) of the same shapes, the same way;
(c) which launches make the difference: device time per entry point of one recorded step (StepPlan.profile_ops), nc = 37 / 40 / 100
    against nc = 32 and nc = 48;
(d) the three class-branch layers of the 160x160 level -- Conv(32, c3, 3) -> Conv(c3, c3, 3) -> nn.Conv2d(c3, nc, 1) -- stand-alone,
    forward + backward through the engine tape, beside the nc = 32 and nc = 48 layers.

nc = 32 and 48 take the accumulator-statistics fast paths (c3 = 32 / 48); 37 and 100 (c3 = 100) have a ragged last 8-channel granule
and 40 a width that is no multiple of 16: the three-launch BatchNorm form, no BatchNorm inside the weight-gradient kernel.

usage: any_nc_bench.py [--batch 64] [--imgsz 640] [--rounds 5] [--steps 10] [--nc 32,37,40,48,100] [--skip-layers]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
import torch  # noqa: E402

NEIGHBOURS = (32, 48)


def build_plan(nc, B, S):
    from bench import CFG, synth_batch
    from ultralytics.hip.train import StepPlan
    from ultralytics.nn.tasks import DetectionModel
    torch.manual_seed(0)
    model = DetectionModel(CFG, nc=nc, verbose=False).cuda().train()
    for k, v in model.named_parameters():
        v.requires_grad = ".dfl" not in k
    plan = StepPlan(model, B, S, nmax=8, optimizer="SGD", use_graph=True)
    plan.crit.bbox_loss.use_wiseiou, plan.crit.bbox_loss.nwd_loss = True, True
    batch = {k: v.cuda() for k, v in synth_batch(1, B, S, min(nc, 6)).items()}
    plan.img.copy_(batch["img"])
    batch["img"] = plan.img

    def step():
        plan.set_hyper([0.01] * 3, 0.937, [0.0, 5e-4, 0.0])
        plan.forward_backward(batch)
        plan.optimizer_step()
    return model, plan, step


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def alternate(fns, rounds, steps):
    """{key: [ms per call, one per round]}: the callables timed in turn, round after round."""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            out[k].append(timed(f, steps))
    return out


def table(title, ms, ncs):
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    base = sum(mean[k] for k in NEIGHBOURS if k in mean) / max(1, sum(1 for k in NEIGHBOURS if k in mean))
    print(title)
    print("| nc | c3 | ms (mean of rounds) | min .. max | ratio to the mean of nc = 32 and nc = 48 |")
    print("|---|---|---|---|---|")
    for nc in ncs:
        print(f"| {nc} | {max(32, min(nc, 100))} | {mean[nc]:.3f} | {min(ms[nc]):.3f} .. {max(ms[nc]):.3f} | {mean[nc] / base:.3f} |")


def layer_part(ncs, B):
    """cv3 of the 160x160 level on its own: forward + backward of the three layers through the engine tape, eager launches."""
    from ultralytics.hip.engine import Storage
    from ultralytics.nn.modules import Detect
    from ultralytics.nn.tasks import initialize_weights
    print("(d) class branch of the 160x160 level stand-alone (forward + backward, eager launches, ms per pass)")
    print("| nc | Conv(32, c3, 3) -> Conv(c3, c3, 3) -> Conv2d(c3, nc, 1) | ms |")
    print("|---|---|---|")
    for nc in ncs:
        torch.manual_seed(0)
        det = Detect(nc, (32, 64, 128))
        det.stride = torch.tensor([4.0, 8.0, 16.0])
        initialize_weights(det)
        det.cuda().train()
        rt = det._runtime(torch.device("cuda", 0))
        eng = rt.eng
        rt.pack_all(True)
        st = Storage(eng, B, 160, 160, 32)
        st.buf.normal_()
        ncp = (nc + 7) // 8 * 8
        out = torch.zeros((B, 160, 160, ncp), dtype=torch.float32, device="cuda")
        dout = torch.randn((B, 160, 160, ncp), device="cuda").half()
        dout[..., nc:] = 0
        spec = rt.specs[(id(det), "cv3", 0)]

        def one():
            eng.training, eng.tape = True, []
            x = st.act()
            st.gbuf, st.gwritten = None, []
            c = det.cv3[0][1].forward_act(det.cv3[0][0].forward_act(x))
            eng.conv_bias(spec, c, out.data_ptr(), ncp, True, lambda: (dout.data_ptr(), ncp))
            eng.zero_backward_acc()
            for f in reversed(eng.tape):
                f()
            eng.tape = None
        one()
        ms = min(timed(one, 5) for _ in range(3))
        c3 = det.cv3[0][0].conv.out_channels
        print(f"| {nc} | c3 = {c3} | {ms:.3f} |")
        del det, rt, st, out, dout
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--nc", default="32,37,40,48,100")
    ap.add_argument("--skip-layers", action="store_true")
    a = ap.parse_args()
    ncs = [int(v) for v in a.nc.split(",")]
    B, S = a.batch, a.imgsz
    print(f"yolov8n-ASF-P2P2, batch {B}, {S}x{S}; {a.rounds} rounds x {a.steps} calls per shape, shapes taken in turn")

    plans, steps = {}, {}
    for nc in ncs:
        plans[nc] = build_plan(nc, B, S)
        steps[nc] = plans[nc][2]
        for _ in range(12):  # trace, capture, and let the dynamic loss scale settle
            steps[nc]()
    table("(a) training step", alternate(steps, a.rounds, a.steps), ncs)

    prof = {}
    for nc in ncs:
        rows = plans[nc][1].profile_ops(3)
        agg = {}
        for name, _, ms in rows:
            agg[name] = agg.get(name, (0, 0.0))
            agg[name] = (agg[name][0] + 1, agg[name][1] + ms)
        prof[nc] = (agg, sum(ms for _, _, ms in rows), len(rows))
    print("(c) device time per entry point of one recorded forward + backward (event-timed replay), ms; launches in brackets")
    names = sorted({n for nc in ncs for n in prof[nc][0]}, key=lambda n: -max(prof[nc][0].get(n, (0, 0.0))[1] for nc in ncs))
    print("| entry point | " + " | ".join(f"nc = {nc}" for nc in ncs) + " |")
    print("|---|" + "---|" * len(ncs))
    shown = 0
    for n in names:
        vals = [prof[nc][0].get(n, (0, 0.0)) for nc in ncs]
        if max(v[1] for v in vals) - min(v[1] for v in vals) < 0.02 and len({v[0] for v in vals}) == 1:
            continue  # the same launches at the same cost in every shape
        print(f"| {n} | " + " | ".join(f"{v[1]:.3f} ({v[0]})" for v in vals) + " |")
        shown += 1
    print("| all launches | " + " | ".join(f"{prof[nc][1]:.3f} ({prof[nc][2]})" for nc in ncs) + " |")
    del plans, steps
    torch.cuda.empty_cache()

    from bench import CFG
    from ultralytics.nn.tasks import DetectionModel
    infer = {}
    x = torch.rand(B, 3, S, S, device="cuda")
    for nc in ncs:
        torch.manual_seed(0)
        m = DetectionModel(CFG, nc=nc, verbose=False).cuda()
        m.fuse().eval()

        def fwd(m=m):
            with torch.no_grad():
                m(x)
        for _ in range(4):
            fwd()
        infer[nc] = fwd
    table("(b) fused inference forward", alternate(infer, a.rounds, a.steps), ncs)
    del infer
    torch.cuda.empty_cache()
    if not a.skip_layers:
        layer_part(ncs, min(B, 16))


if __name__ == "__main__":
    main()
