#!/usr/bin/env python3
"""GSConv's shuffle entries (csrc/gsconv.hip) measured: (a) dy_gs_shuffle_forward and dy_gs_shuffle_backward (both destinations
stored, as the graph runs it, and both accumulated) stand-alone at the GSConv shapes of yolov8n-ASF-P2P2-SlimNeck at 640x640,
batch 64, each beside dy_copy_slice moving the same number of bytes, the variants alternating under device events in one process;
(b) the dy_gs_* launches' share of a training step of that graph (event-timed replay of the recorded launch list, as
tools/op_profile.py times it); (c) ``--bench``: ``python bench.py --model ...`` on the slim-neck graph and on the dense default graph
(and the default graph from a built checkout of the parent commit, ``--parent DIR``), each run a fresh child process, alternating.

usage: gsconv_bench.py [--kernel] [--step] [--bench [--parent DIR]] [--batch 64] [--rounds 5]     (parts (a) and (b) when none is named)

Every timed loop walks a ring of buffer sets of at least 1 GiB, so a kernel never finds its operands resident from its previous
repetition.  Bytes of an entry: it reads 2 c_ channels per pixel and writes 2 c_ (fp16): 8 c_ bytes per pixel; the accumulating
backward reads its destinations too, 12 c_.  The copy reads half of the stored entry's bytes and writes half.  A row is the median
over the rounds of the mean time of 20 launches; its spread is max - min."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
import torch  # noqa: E402

# (H, W, c_) of the shuffled maps at 640x640, scale n, and the GSConvs that have them: rows 18 and 21 themselves, and the two GSConvs
# inside the GSBottleneck of the VoVGSCSP rows 12, 17, 20, 23
SHAPES = {(160, 160, 8): "row 17 (x 2)", (80, 80, 16): "rows 18, 12 (x 2), 20 (x 2)", (40, 40, 32): "rows 21, 23 (x 2)"}
RING_BYTES = 1 << 30
MODEL = "yolov8n-ASF-P2P2-SlimNeck"
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

    print("(a) stand-alone, fp16 NHWC; us per launch (median of the rounds, spread = max - min), TB/s of the stored entry's bytes")
    for (H, W, c), where in SHAPES.items():
        N = batch
        nbytes = 8 * c * N * H * W
        ring = max(2, -(-RING_BYTES // nbytes))
        half = lambda *s: torch.randn(*s, device="cuda").half()  # noqa: E731
        x1s, ds, ys = [half(N, H, W, c) for _ in range(ring)], [half(N, H, W, c) for _ in range(ring)], [half(N, H, W, 2 * c) for _ in range(ring)]
        g1s, gds = [half(N, H, W, c) for _ in range(ring)], [half(N, H, W, c) for _ in range(ring)]
        npix = nbytes // 4 // COPY_C  # the copy reads npix x COPY_C fp16 and writes as many: nbytes in all
        cp = ([half(npix, COPY_C) for _ in range(ring)], [torch.empty(npix, COPY_C, dtype=torch.float16, device="cuda") for _ in range(ring)])
        geom = (N, H, W, c)
        variants = {
            "dy_gs_shuffle_forward": [lambda a=a, b=b, y=y: call("dy_gs_shuffle_forward", p(a), c, p(b), c, p(y), 2 * c, *geom) for a, b, y in zip(x1s, ds, ys)],
            "dy_gs_shuffle_backward (stored)": [lambda y=y, a=a, b=b: call("dy_gs_shuffle_backward", p(y), 2 * c, p(a), c, 0, p(b), c, 0, *geom)
                                                for y, a, b in zip(ys, g1s, gds)],
            "dy_gs_shuffle_backward (added)": [lambda y=y, a=a, b=b: call("dy_gs_shuffle_backward", p(y), 2 * c, p(a), c, 1, p(b), c, 1, *geom)
                                               for y, a, b in zip(ys, g1s, gds)],
            "dy_copy_slice, the same bytes": [lambda s=s, d=d: call("dy_copy_slice", p(s), COPY_C, p(d), COPY_C, npix, COPY_C) for s, d in zip(*cp)],
        }
        for fns in variants.values():  # warm up every variant on every ring slot
            for f in fns:
                f()
        for g in g1s + gds:  # (the accumulating variant adds dy on every call: start it from zero, the values stay finite)
            g.zero_()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(rounds):  # the variants alternate inside every round
            for k, fns in variants.items():
                times[k].append(timeit(fns))
        print(f"x1, d = ({N}, {H}, {W}, {c}) -> y ({N}, {H}, {W}, {2 * c}) [{where}]: {nbytes / 1e6:.0f} MB per stored entry; ring of {ring}, {rounds} rounds")
        med = {k: statistics.median(ts) for k, ts in times.items()}
        for k, ts in times.items():
            nb = nbytes * 3 // 2 if "added" in k else nbytes
            print(f"  {k:34s} {med[k] * 1e3:8.1f} us  (spread {(max(ts) - min(ts)) * 1e3:5.1f})  {nb / med[k] / 1e9:5.2f} TB/s")
        cpy = med["dy_copy_slice, the same bytes"]
        print("  against the copy: " + ", ".join(f"{k} {med[k] / cpy:.2f}x" for k in med if k.startswith("dy_gs")))
        del x1s, ds, ys, g1s, gds, cp, variants
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
    gs = [(name, a, ms) for name, a, ms in prof if name.startswith("dy_gs_")]
    dw = [(name, a, ms) for name, a, ms in prof if name.startswith("dy_dwconv")]
    print(f"(b) {model_name}, batch {B}, 640x640: {len(prof)} launches in forward + backward, {total:.3f} ms of device time")
    for name, a, ms in gs:
        print(f"  {name:24s} (n, H, W, c_) = {tuple(a[-4:])}  {ms * 1e3:8.1f} us")
    gsum, dsum = sum(ms for _, _, ms in gs), sum(ms for _, _, ms in dw)
    print(f"  {len(gs)} shuffle launches: {gsum:.3f} ms = {100 * gsum / total:.2f} % of the step's device time; the {len(dw)} depthwise launches of the "
          f"GSConvs' cv2: {dsum:.3f} ms = {100 * dsum / total:.2f} %")


def bench_part(parent, rounds):
    """bench.py (unchanged) in fresh child processes, alternating: the default graph and the slim-neck graph from this tree, and the
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
        raise SystemExit("gsconv_bench.py measures on the GPU; there is none here")
    if a.kernel or every:
        kernel_part(a.batch, a.rounds)
    if a.step or every:
        step_part(a.model, a.batch)
    if a.bench:
        bench_part(a.parent, 3)
