#!/usr/bin/env python3
"""DySample's sampler (csrc/dysample.hip) measured: (a) forward and backward stand-alone at the two DEAL-YOLO-N 640x640 batch-64
shapes (64 channels 40^2 -> 80^2, 32 channels 80^2 -> 160^2), beside ``dy_upsample2x`` forward and backward at the same shape -- existing
code that writes the same bytes -- and beside a plain copy of the byte floor (the output write plus the offsets read), the variants
alternating in one process; (b) the sampler launches' share of a training step of yolov8n-ASF-P2P2-DySample (event-timed replay of
the recorded launch list, as tools/op_profile.py times it); (c) ``bench.py --model`` for that graph and for yolov8n-ASF-P2P2, each in
a fresh child process, alternating.

usage: dysample_bench.py [--kernel] [--step] [--bench] [--batch 64] [--rounds 5]     (all parts when none is named)

Every timed loop walks a ring of buffer sets of at least 1 GiB, so a kernel never finds its operands resident from its previous
repetition.  Offsets: ``init`` = what a freshly initialised layer predicts (std(0.25 o) = 2.5e-4 px: the gather radius is 1) and
``spread`` = std(0.25 o) = 0.5 px as in the golden state (4.5 % of the samples take the atomic side pass, the gather radius is 2).
A row is the median over the rounds of the mean time of 20 launches; its spread is max - min over the rounds."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
import torch  # noqa: E402

SHAPES = [(64, 40, 40, 64), (64, 80, 80, 32)]  # inputs of layers 9 and 14 of yolov8n-ASF-P2P2-DySample at 640x640, batch 64
RING_BYTES = 1 << 30
G, S = 4, 2


def timeit(fns, reps=20):
    """Mean ms per call of the callables in ``fns`` taken in turn (one per ring slot)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_part(batch, rounds):
    from ultralytics.hip import check, lib
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731

    def call(name, *a):
        check(getattr(L, name)(*a, st), name)

    print("(a) stand-alone, fp16 NHWC; us per launch (median of the rounds, spread = max - min), TB/s of the byte floor")
    for N, H, W, C in [(batch, h, w, c) for _, h, w, c in SHAPES]:
        nch = 2 * G * S * S
        e_in, e_out = N * H * W * C, N * H * W * C * S * S
        floor = 2 * e_out + 4 * N * H * W * nch  # the output write plus the offsets read
        ring = max(2, -(-RING_BYTES // (4 * e_out + 2 * e_in)))
        xs = [torch.randn(N, H, W, C, device="cuda").half() for _ in range(ring)]
        ys = [torch.randn(N, S * H, S * W, C, device="cuda").half() for _ in range(ring)]
        dxs = [torch.empty(N, H, W, C, dtype=torch.float16, device="cuda") for _ in range(ring)]
        doffs = [torch.empty(N, H, W, nch, dtype=torch.float16, device="cuda") for _ in range(ring)]
        offs = {"init": [torch.randn(N, H, W, nch, device="cuda") * 1e-3 for _ in range(ring)],
                "spread": [torch.randn(N, H, W, nch, device="cuda") * 2.0 for _ in range(ring)]}
        cp_src = [torch.empty(floor // 2, dtype=torch.uint8, device="cuda") for _ in range(ring)]
        cp_dst = [torch.empty(floor // 2, dtype=torch.uint8, device="cuda") for _ in range(ring)]
        dx32, scratch = torch.empty(e_in, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
        variants = {}
        for kind, off in offs.items():
            variants[f"dysample forward ({kind})"] = [lambda x=x, o=o, y=y: call("dy_dysample", p(x), C, p(o), nch, p(y), C, N, H, W, C, G, S)
                                                      for x, o, y in zip(xs, off, ys)]
            variants[f"dysample backward dx + d(o) ({kind})"] = [
                lambda x=x, o=o, y=y, d=d, q=q: call("dy_dysample_backward", p(x), C, p(o), nch, p(y), C, p(d), C, 0, p(dx32), p(q), nch, p(scratch),
                                                     2, N, H, W, C, G, S) for x, o, y, d, q in zip(xs, off, ys, dxs, doffs)]
            variants[f"dysample backward d(o) only ({kind})"] = [
                lambda x=x, o=o, y=y, q=q: call("dy_dysample_backward", p(x), C, p(o), nch, p(y), C, 0, 0, 0, 0, p(q), nch, 0, 2, N, H, W, C, G, S)
                for x, o, y, q in zip(xs, off, ys, doffs)]
            variants[f"dysample backward dx only ({kind})"] = [
                lambda x=x, o=o, y=y, d=d: call("dy_dysample_backward", p(x), C, p(o), nch, p(y), C, p(d), C, 0, p(dx32), 0, 0, p(scratch), 2,
                                                N, H, W, C, G, S) for x, o, y, d in zip(xs, off, ys, dxs)]
        variants["upsample2x forward (same output)"] = [lambda x=x, y=y: call("dy_upsample2x", p(x), C, p(y), C, N, H, W, C, 0, 0) for x, y in zip(xs, ys)]
        variants["upsample2x backward (same input)"] = [lambda d=d, y=y: call("dy_upsample2x", p(y), C, p(d), C, N, H, W, C, 1, 0) for d, y in zip(dxs, ys)]
        variants["torch copy_ of the byte floor"] = [lambda a=a, b=b: b.copy_(a) for a, b in zip(cp_src, cp_dst)]
        for fns in variants.values():  # warm up every variant on every ring slot
            for f in fns:
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(rounds):  # the variants alternate inside every round
            for k, fns in variants.items():
                times[k].append(timeit(fns))
        print(f"x = ({N}, {H}, {W}, {C}) -> ({N}, {S * H}, {S * W}, {C}): output {2 * e_out / 1e6:.0f} MB, offsets {4 * N * H * W * nch / 1e6:.0f} MB, "
              f"byte floor {floor / 1e6:.0f} MB, ring of {ring}, {rounds} rounds")
        for k, ts in times.items():
            med = statistics.median(ts)
            print(f"  {k:44s} {med * 1e3:8.1f} us  (spread {(max(ts) - min(ts)) * 1e3:5.1f})  {floor / med / 1e9:5.2f} TB/s of the floor")
        del xs, ys, dxs, doffs, offs, cp_src, cp_dst, variants
        torch.cuda.empty_cache()


def step_part(model_name, B):
    from bench import CFG, synth_batch
    from ultralytics.hip.train import StepPlan
    from ultralytics.nn.tasks import DetectionModel
    torch.manual_seed(0)
    model = DetectionModel(os.path.join(os.path.dirname(CFG), model_name + ".yaml"), verbose=False).cuda().train()
    plan = StepPlan(model, B, 640, nmax=8)
    batch = {k: v.cuda() for k, v in synth_batch(1, B, 640, 6).items()}
    plan.set_hyper([0.01] * 3, 0.937, [0, 5e-4, 0])
    for _ in range(3):
        plan.forward_backward(batch)
        plan.optimizer_step()
    prof = plan.profile_ops(5)
    total = sum(ms for _, _, ms in prof)
    ds = [(name, a, ms) for name, a, ms in prof if name in ("dy_dysample", "dy_dysample_backward")]
    print(f"(b) {model_name}, batch {B}, 640x640: {len(prof)} launches in forward + backward, {total:.3f} ms of device time")
    for name, a, ms in ds:
        n, h, w, c = (a[6], a[7], a[8], a[9]) if name == "dy_dysample" else (a[14], a[15], a[16], a[17])
        floor = n * h * w * (2 * c * S * S + 4 * 2 * G * S * S)
        print(f"  {name:22s} ({n}, {h}, {w}, {c})  {ms * 1e3:8.1f} us  {floor / ms / 1e9:5.2f} TB/s of the byte floor")
    dsum = sum(ms for _, _, ms in ds)
    print(f"  {len(ds)} sampler launches: {dsum:.3f} ms = {100 * dsum / total:.2f} % of the step's device time (the two offset convolutions "
          "and their gradients are not in this figure)")


def bench_part(rounds):
    """bench.py (unchanged) on both graphs, each run a fresh child process, alternating."""
    models = ["yolov8n-ASF-P2P2-DySample", "yolov8n-ASF-P2P2"]
    res = {m: [] for m in models}
    for _ in range(rounds):
        for m in models:
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "8", "--no-cpu",
                                  "--probe", "0", "--secondary", "0", "--model", m], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise RuntimeError(f"bench.py --model {m} failed:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
            res[m].append(json.loads(line))
    print(f"(c) bench.py --steps 30 --warmup 8 --no-cpu --probe 0 --secondary 0, {rounds} runs per model, alternating")
    for m, rs in res.items():
        print(f"  {m}: " + "; ".join(json.dumps({k: v for k, v in r.items() if isinstance(v, (int, float)) and not isinstance(v, bool)}) for r in rs))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--model", default="yolov8n-ASF-P2P2-DySample")
    a = ap.parse_args()
    every = not (a.kernel or a.step or a.bench)
    if not torch.cuda.is_available():
        raise SystemExit("dysample_bench.py measures on the GPU; there is none here")
    if a.kernel or every:
        kernel_part(a.batch, a.rounds)
    if a.step or every:
        step_part(a.model, a.batch)
    if a.bench or every:
        bench_part(2)
