#!/usr/bin/env python3
"""Fusion's kernels (csrc/fusion.hip) measured: (a) dy_fusion_forward and dy_fusion_backward (+ dy_fusion_wgrad_finish) stand-alone at
the three layer shapes of yolov8n-ASF-P2P2-BiFPN at 640x640, batch 64 -- rows 11 (80 x 80 x 64, one operand stored at 40 x 40),
16 (160 x 160 x 32, one operand at 80 x 80) and 25 (160 x 160 x 32, both operands plain) -- each beside dy_add over the same number
of operands (all at full resolution: it cannot read through an un-executed up-sampling) and beside dy_copy_slice moving the SAME
number of bytes as the fusion launch, the byte floor as this library reaches it; all alternating under device events in one
process; (b) the dy_fusion_* launches' share of a training step of that graph; (c) ``--bench``: ``python bench.py --model ...`` on
the BiFPN graph and on the default graph (and the default graph from a built checkout of the parent commit, ``--parent DIR``),
each run a fresh child process, alternating.

usage: bifpn_bench.py [--kernel] [--step] [--bench [--parent DIR]] [--batch 64] [--rounds 5]     (parts (a) and (b) when none is named)

Every timed loop walks a ring of buffer sets of at least 1 GiB, so a kernel never finds its operands resident from its previous
repetition.  Bytes (fp16): the forward reads every operand once (a half-resolution operand is a quarter of the map) and writes y;
the backward reads dy and every operand and writes every dx at full resolution.  A row is the median over the rounds of the mean
time of 20 launches; its spread is max - min; the ratio is the entry's time over the copy's."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
import torch  # noqa: E402

SHAPES = {11: (80, 80, 64, True), 16: (160, 160, 32, True), 25: (160, 160, 32, False)}  # row -> (H, W, C, second operand at half resolution)
RING_BYTES = 1 << 30
MODEL = "yolov8n-ASF-P2P2-BiFPN"
COPY_C = 64  # the copy's row width in channels


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

    print("(a) stand-alone, fp16 NHWC, two operands; us per launch (median of the rounds, spread = max - min), TB/s of the entry's own bytes")
    for row, (H, W, C, up) in SHAPES.items():
        N = batch
        full, low = 2 * N * H * W * C, 2 * N * (H // 2) * (W // 2) * C
        fwd_bytes = full + (low if up else full) + full
        bwd_bytes = full + full + (low if up else full) + 2 * full
        ring = max(2, -(-RING_BYTES // bwd_bytes))
        half = lambda *s: torch.randn(*s, device="cuda").half()  # noqa: E731
        x0 = [half(N, H, W, C) for _ in range(ring)]
        x1 = [half(N, H // 2, W // 2, C) if up else half(N, H, W, C) for _ in range(ring)]
        x1f = [half(N, H, W, C) for _ in range(ring)] if up else x1
        ys = [torch.empty(N, H, W, C, dtype=torch.float16, device="cuda") for _ in range(ring)]
        d0 = [torch.empty(N, H, W, C, dtype=torch.float16, device="cuda") for _ in range(ring)]
        d1 = [torch.empty(N, H, W, C, dtype=torch.float16, device="cuda") for _ in range(ring)]
        w = torch.tensor([1.3, 0.6], dtype=torch.float32, device="cuda")
        gw = torch.zeros(8, dtype=torch.float32, device="cuda")
        parts = L.dy_fusion_num_partials(N * H * W, C)
        ws = torch.zeros(3 * parts, dtype=torch.float32, device="cuda")
        u = int(up)

        def copy_of(nbytes):
            npix = nbytes // 4 // COPY_C  # the copy reads npix x COPY_C fp16 and writes as many: nbytes in all
            src = [half(npix, COPY_C) for _ in range(ring)]
            dst = [torch.empty(npix, COPY_C, dtype=torch.float16, device="cuda") for _ in range(ring)]
            return [lambda s=s, d=d: call("dy_copy_slice", p(s), COPY_C, p(d), COPY_C, npix, COPY_C) for s, d in zip(src, dst)]

        def bwd(a, b, y, da, db, wsp):
            call("dy_fusion_backward", p(y), C, p(a), C, 0, p(da), C, 0, p(b), C, u, p(db), C, 0, 0, 0, 0, 0, 0, 0, p(w), wsp, 2, N, H, W, C)
            if wsp:
                call("dy_fusion_wgrad_finish", wsp, parts, p(w), p(gw), 2, 0)

        variants = {
            "dy_fusion_forward": ([lambda a=a, b=b, y=y: call("dy_fusion_forward", p(a), C, 0, p(b), C, u, 0, 0, 0, p(w), p(y), C, 2, N, H, W, C)
                                   for a, b, y in zip(x0, x1, ys)], fwd_bytes),
            "dy_add, two operands": ([lambda a=a, b=b, y=y: call("dy_add", p(a), C, p(b), C, 0, 0, p(y), C, N * H * W, C)
                                      for a, b, y in zip(x0, x1f, ys)], 3 * full),
            "dy_copy_slice, forward's bytes": (copy_of(fwd_bytes), fwd_bytes),
            "dy_fusion_backward + finish": ([lambda a=a, b=b, y=y, da=da, db=db: bwd(a, b, y, da, db, p(ws))
                                             for a, b, y, da, db in zip(x0, x1, ys, d0, d1)], bwd_bytes),
            "dy_fusion_backward, frozen": ([lambda a=a, b=b, y=y, da=da, db=db: bwd(a, b, y, da, db, 0)
                                            for a, b, y, da, db in zip(x0, x1, ys, d0, d1)], 3 * full),
            "dy_copy_slice, backward's bytes": (copy_of(bwd_bytes), bwd_bytes),
        }
        for fns, _ in variants.values():
            for f in fns:
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(rounds):  # the variants alternate inside every round
            for k, (fns, _) in variants.items():
                times[k].append(timeit(fns))
        print(f"row {row}: ({N}, {H}, {W}, {C}), second operand {'at ' + str(H // 2) + ' x ' + str(W // 2) if up else 'plain'}: forward "
              f"{fwd_bytes / 1e6:.0f} MB, backward {bwd_bytes / 1e6:.0f} MB; {parts} partials; ring of {ring}, {rounds} rounds")
        med = {k: statistics.median(ts) for k, ts in times.items()}
        floor = {"dy_fusion_forward": "dy_copy_slice, forward's bytes", "dy_add, two operands": "dy_copy_slice, forward's bytes",
                 "dy_fusion_backward + finish": "dy_copy_slice, backward's bytes", "dy_fusion_backward, frozen": "dy_copy_slice, backward's bytes"}
        for k, ts in times.items():
            nbytes = variants[k][1]
            ratio = ""
            if k in floor:  # time per byte against the copy's time per byte
                ratio = f"  {(med[k] / nbytes) / (med[floor[k]] / variants[floor[k]][1]):.2f}x the copy's time per byte"
            print(f"  {k:34s} {med[k] * 1e3:8.1f} us  (spread {(max(ts) - min(ts)) * 1e3:5.1f})  {nbytes / med[k] / 1e9:5.2f} TB/s{ratio}")
        del x0, x1, x1f, ys, d0, d1, variants
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
    fu = [(name, a, ms) for name, a, ms in prof if name.startswith("dy_fusion")]
    print(f"(b) {model_name}, batch {B}, 640x640: {len(prof)} launches in forward + backward, {total:.3f} ms of device time")
    for name, a, ms in fu:
        print(f"  {name:24s} {ms * 1e3:8.1f} us")
    dsum = sum(ms for _, _, ms in fu)
    print(f"  {len(fu)} fusion launches: {dsum:.3f} ms = {100 * dsum / total:.2f} % of the step's device time")


def bench_part(parent, rounds):
    """bench.py (unchanged) in fresh child processes, alternating: the default graph and the BiFPN graph from this tree, and the
    default graph from the parent's tree when one is given."""
    runs = {"this tree, default graph": (ROOT, []), f"this tree, {MODEL}": (ROOT, ["--model", MODEL])}
    if parent:
        runs = {"parent, default graph": (os.path.abspath(parent), []), **runs}
    res = {k: [] for k in runs}
    for _ in range(rounds):
        for k, (root, extra) in runs.items():
            out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "8", "--no-cpu",
                                  "--probe", "0", "--secondary", "0", *extra], capture_output=True, text=True, timeout=600, cwd=root)
            if out.returncode != 0:
                raise RuntimeError(f"bench.py in {root} failed:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
            res[k].append(json.loads(line))
    print(f"(c) bench.py --steps 30 --warmup 8 --no-cpu --probe 0 --secondary 0, {rounds} runs each, alternating")
    for k, rs in res.items():
        print(f"  {k}: " + "; ".join(json.dumps({n: v for n, v in r.items() if isinstance(v, (int, float)) and not isinstance(v, bool)}) for r in rs))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--parent", help="a built checkout of the parent commit (part (c))")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--model", default=MODEL)
    a = ap.parse_args()
    every = not (a.kernel or a.step or a.bench)
    if not torch.cuda.is_available():
        raise SystemExit("bifpn_bench.py measures on the GPU; there is none here")
    if a.kernel or every:
        kernel_part(a.batch, a.rounds)
    if a.step or every:
        step_part(a.model, a.batch)
    if a.bench:
        bench_part(a.parent, 3)
