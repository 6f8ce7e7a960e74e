#!/usr/bin/env python3
"""SimAM's kernels (csrc/simam.hip) measured: (a) dy_simam_forward and dy_simam_backward (stored and accumulating) stand-alone at the
three layer shapes of yolov8n-ASF-P2P2-SimAM at 640x640, batch 64 -- rows 26 (160 x 160 x 32), 27 (80 x 80 x 64) and 28
(40 x 40 x 128) -- each beside dy_copy_slice moving the SAME number of bytes as the entry, the byte floor as this library reaches
it; all alternating under device events in one process; (b) the dy_simam_* launches' share of a training step of that graph;
(c) ``--bench``: ``python bench.py --model ...`` on the SimAM graph and on the default graph (and the default graph from a built
checkout of the parent commit, ``--parent DIR``), each run a fresh child process, alternating.

usage: simam_bench.py [--kernel] [--step] [--bench [--parent DIR]] [--batch 64] [--rounds 5]     (parts (a) and (b) when none is named)

Every timed loop walks a ring of buffer sets of at least 1 GiB, so a kernel never finds its operands resident from its previous
repetition.  Bytes (fp16; each entry is two launches): the forward reads x twice (statistics pass, apply pass) and writes y: 3 maps;
the backward reads dy and x twice and writes dx: 5 maps, 6 when it adds to a stored dx.  The fp64 partials and the fp32 statistics
are a few hundred KB and not counted.  A row is the median over the rounds of the mean time of 20 calls; its spread is max - min; the
ratio is the entry's time per byte over the copy's."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
import torch  # noqa: E402

SHAPES = {26: (160, 160, 32), 27: (80, 80, 64), 28: (40, 40, 128)}  # row -> (H, W, C)
RING_BYTES = 1 << 30
MODEL = "yolov8n-ASF-P2P2-SimAM"
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

    print("(a) stand-alone, fp16 NHWC; us per call of an entry (two launches; median of the rounds, spread = max - min), TB/s of the entry's own bytes")
    for row, (H, W, C) in SHAPES.items():
        N = batch
        full = 2 * N * H * W * C
        fwd_bytes, bwd_bytes, acc_bytes = 3 * full, 5 * full, 6 * full
        ring = max(2, -(-RING_BYTES // (4 * full)))
        half = lambda *s: torch.randn(*s, device="cuda").half()  # noqa: E731
        xs = [half(N, H, W, C) for _ in range(ring)]
        gs = [half(N, H, W, C) for _ in range(ring)]
        ys = [torch.empty(N, H, W, C, dtype=torch.float16, device="cuda") for _ in range(ring)]
        ds = [torch.zeros(N, H, W, C, dtype=torch.float16, device="cuda") for _ in range(ring)]
        parts = L.dy_simam_num_partials(H * W, C)
        ws = torch.zeros(N * parts * 2 * C, dtype=torch.float64, device="cuda")
        stats = torch.zeros(N * 2 * C, dtype=torch.float32, device="cuda")
        call("dy_simam_forward", p(xs[0]), C, p(ys[0]), C, p(stats), p(ws), 1e-4, N, H, W, C)  # (the backward reads stats: any plane's will do for timing)

        def copy_of(nbytes):
            npix = nbytes // 4 // COPY_C  # the copy reads npix x COPY_C fp16 and writes as many: nbytes in all
            src = [half(npix, COPY_C) for _ in range(ring)]
            dst = [torch.empty(npix, COPY_C, dtype=torch.float16, device="cuda") for _ in range(ring)]
            return [lambda s=s, d=d: call("dy_copy_slice", p(s), COPY_C, p(d), COPY_C, npix, COPY_C) for s, d in zip(src, dst)]

        variants = {
            "dy_simam_forward": ([lambda x=x, y=y: call("dy_simam_forward", p(x), C, p(y), C, p(stats), p(ws), 1e-4, N, H, W, C)
                                  for x, y in zip(xs, ys)], fwd_bytes),
            "dy_copy_slice, forward's bytes": (copy_of(fwd_bytes), fwd_bytes),
            "dy_simam_backward, stored": ([lambda x=x, g=g, d=d: call("dy_simam_backward", p(g), C, p(x), C, p(stats), p(d), C, 0, p(ws), N, H, W, C)
                                           for x, g, d in zip(xs, gs, ds)], bwd_bytes),
            "dy_copy_slice, backward's bytes": (copy_of(bwd_bytes), bwd_bytes),
            "dy_simam_backward, added": ([lambda x=x, g=g, d=d: call("dy_simam_backward", p(g), C, p(x), C, p(stats), p(d), C, 1, p(ws), N, H, W, C)
                                          for x, g, d in zip(xs, gs, ys)], acc_bytes),
        }
        for fns, _ in variants.values():
            for f in fns:
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(rounds):  # the variants alternate inside every round
            for k, (fns, _) in variants.items():
                times[k].append(timeit(fns))
        print(f"row {row}: ({N}, {H}, {W}, {C}): forward {fwd_bytes / 1e6:.0f} MB, backward {bwd_bytes / 1e6:.0f} MB ({acc_bytes / 1e6:.0f} MB adding); "
              f"{parts} runs per image; ring of {ring}, {rounds} rounds")
        med = {k: statistics.median(ts) for k, ts in times.items()}
        floor = {"dy_simam_forward": "dy_copy_slice, forward's bytes", "dy_simam_backward, stored": "dy_copy_slice, backward's bytes",
                 "dy_simam_backward, added": "dy_copy_slice, backward's bytes"}
        for k, ts in times.items():
            nbytes = variants[k][1]
            ratio = ""
            if k in floor:  # time per byte against the copy's time per byte
                ratio = f"  {(med[k] / nbytes) / (med[floor[k]] / variants[floor[k]][1]):.2f}x the copy's time per byte"
            print(f"  {k:34s} {med[k] * 1e3:8.1f} us  (spread {(max(ts) - min(ts)) * 1e3:5.1f})  {nbytes / med[k] / 1e9:5.2f} TB/s{ratio}")
        del xs, gs, ys, ds, variants
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
    sa = [(name, a, ms) for name, a, ms in prof if name.startswith("dy_simam")]
    print(f"(b) {model_name}, batch {B}, 640x640: {len(prof)} calls in forward + backward, {total:.3f} ms of device time")
    for name, a, ms in sa:
        print(f"  {name:24s} {ms * 1e3:8.1f} us")
    dsum = sum(ms for _, _, ms in sa)
    print(f"  {len(sa)} SimAM calls: {dsum:.3f} ms = {100 * dsum / total:.2f} % of the step's device time")


def bench_part(parent, rounds):
    """bench.py (unchanged) in fresh child processes, alternating: the default graph and the SimAM graph from this tree, and the
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
        raise SystemExit("simam_bench.py measures on the GPU; there is none here")
    if a.kernel or every:
        kernel_part(a.batch, a.rounds)
    if a.step or every:
        step_part(a.model, a.batch)
    if a.bench:
        bench_part(a.parent, 3)
