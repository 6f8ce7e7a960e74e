#!/usr/bin/env python3
"""CARAFE's reassembly (csrc/carafe.hip) measured: (a) forward and each backward half stand-alone at the two DEAL-YOLO-N 640x640
batch-64 shapes (64 channels 40^2 -> 80^2, 32 channels 80^2 -> 160^2), beside a plain copy of the same bytes and beside
``dy_upsample2x`` and ``dy_dysample`` at the same shapes, the variants alternating in one process; (b) the four launches' share of a
training step of yolov8n-ASF-P2P2-CARAFE (event-timed replay of the recorded launch list, as tools/op_profile.py times it);
(c) ``bench.py`` on the default graph from this tree and from a checkout of the parent commit (``--parent DIR``, built), each run a
fresh child process, alternating.

usage: carafe_bench.py [--kernel] [--step] [--bench --parent DIR] [--batch 64] [--rounds 5]     (parts (a) and (b) when none is named)

Every timed loop walks a ring of buffer sets of at least 1 GiB, so a kernel never finds its operands resident from its previous
repetition.  Byte floors: forward = X read + 104 logit lanes read + Y written; dlogits = X + logits + dY read, 104 lanes written;
dx = logits + dY read, dX written.  A row is the median over the rounds of the mean time of 20 launches; its spread is max - min
over the rounds."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
import torch  # noqa: E402

SHAPES = [(64, 40, 40, 64), (64, 80, 80, 32)]  # inputs of layers 9 and 14 of yolov8n-ASF-P2P2-CARAFE at 640x640, batch 64
RING_BYTES = 1 << 30
LP = 104  # the logits' pitch


def timeit(fns, reps=20):
    """Mean ms per call of the callables in ``fns`` taken in turn (one per ring slot)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def floors(N, H, W, C):
    px = N * H * W
    return dict(fwd=2 * px * (C + LP + 4 * C), dl=2 * px * (C + LP + 4 * C + LP), dx=2 * px * (LP + 4 * C + C))


def kernel_part(batch, rounds):
    from ultralytics.hip import check, lib
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731

    def call(name, *a):
        check(getattr(L, name)(*a, st), name)

    print("(a) stand-alone, fp16 NHWC; us per launch (median of the rounds, spread = max - min), TB/s of the row's own byte floor")
    for N, H, W, C in [(batch, h, w, c) for _, h, w, c in SHAPES]:
        fl = floors(N, H, W, C)
        e_in, e_out, e_lg = N * H * W * C, 4 * N * H * W * C, N * H * W * LP
        ring = max(2, -(-RING_BYTES // (2 * (2 * e_out + 2 * e_in + 2 * e_lg))))
        xs = [torch.randn(N, H, W, C, device="cuda").half() for _ in range(ring)]
        lgs = [torch.randn(N, H, W, LP, device="cuda").half() for _ in range(ring)]
        ys = [torch.randn(N, 2 * H, 2 * W, C, device="cuda").half() for _ in range(ring)]
        dxs = [torch.empty(N, H, W, C, dtype=torch.float16, device="cuda") for _ in range(ring)]
        dls = [torch.empty(N, H, W, LP, dtype=torch.float16, device="cuda") for _ in range(ring)]
        offs = [torch.randn(N, H, W, 32, device="cuda") * 1e-3 for _ in range(ring)]  # DySample, 4 groups, freshly initialised
        cp = {k: ([torch.empty(v // 2, dtype=torch.uint8, device="cuda") for _ in range(ring)],
                  [torch.empty(v // 2, dtype=torch.uint8, device="cuda") for _ in range(ring)]) for k, v in fl.items()}
        variants = {
            "carafe forward": ("fwd", [lambda x=x, g=g, y=y: call("dy_carafe", p(x), C, p(g), LP, p(y), C, N, H, W, C) for x, g, y in zip(xs, lgs, ys)]),
            "carafe backward dlogits only": ("dl", [lambda x=x, g=g, y=y, q=q: call("dy_carafe_backward", p(x), C, p(g), LP, p(y), C, 0, 0, 0, p(q), LP,
                                                                                     N, H, W, C) for x, g, y, q in zip(xs, lgs, ys, dls)]),
            "carafe backward dlogits + dx": ("dl+dx", [lambda x=x, g=g, y=y, d=d, q=q: call("dy_carafe_backward", p(x), C, p(g), LP, p(y), C, p(d), C, 0,
                                                                                             p(q), LP, N, H, W, C)
                                                       for x, g, y, d, q in zip(xs, lgs, ys, dxs, dls)]),
            "torch copy_ of the forward's bytes": ("fwd", [lambda a=a, b=b: b.copy_(a) for a, b in zip(*cp["fwd"])]),
            "torch copy_ of the dlogits half's bytes": ("dl", [lambda a=a, b=b: b.copy_(a) for a, b in zip(*cp["dl"])]),
            "torch copy_ of the dx half's bytes": ("dx", [lambda a=a, b=b: b.copy_(a) for a, b in zip(*cp["dx"])]),
            "upsample2x forward (same output)": ("fwd", [lambda x=x, y=y: call("dy_upsample2x", p(x), C, p(y), C, N, H, W, C, 0, 0) for x, y in zip(xs, ys)]),
            "upsample2x backward (same input)": ("dx", [lambda d=d, y=y: call("dy_upsample2x", p(y), C, p(d), C, N, H, W, C, 1, 0) for d, y in zip(dxs, ys)]),
            "dysample forward (init offsets)": ("fwd", [lambda x=x, o=o, y=y: call("dy_dysample", p(x), C, p(o), 32, p(y), C, N, H, W, C, 4, 2)
                                                        for x, o, y in zip(xs, offs, ys)]),
        }
        for _, fns in variants.values():  # warm up every variant on every ring slot
            for f in fns:
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(rounds):  # the variants alternate inside every round
            for k, (_, fns) in variants.items():
                times[k].append(timeit(fns))
        fl["dl+dx"] = fl["dl"] + fl["dx"]
        print(f"x = ({N}, {H}, {W}, {C}) -> ({N}, {2 * H}, {2 * W}, {C}): byte floors forward {fl['fwd'] / 1e6:.0f} MB, dlogits {fl['dl'] / 1e6:.0f} MB, "
              f"dx {fl['dx'] / 1e6:.0f} MB; {100 * C * N * H * W / 1e9:.2f} G multiply-adds each; ring of {ring}, {rounds} rounds")
        med = {k: statistics.median(ts) for k, ts in times.items()}
        for k, ts in times.items():
            f = fl[variants[k][0]]
            print(f"  {k:42s} {med[k] * 1e3:8.1f} us  (spread {(max(ts) - min(ts)) * 1e3:5.1f})  {f / med[k] / 1e9:5.2f} TB/s of {f / 1e6:.0f} MB")
        fw, both, dl_only = med["carafe forward"], med["carafe backward dlogits + dx"], med["carafe backward dlogits only"]
        cpy, ups, dys = med["torch copy_ of the forward's bytes"], med["upsample2x forward (same output)"], med["dysample forward (init offsets)"]
        print(f"  dx half by difference: {(both - dl_only) * 1e3:.1f} us; forward / its copy {fw / cpy:.2f}x, / upsample2x {fw / ups:.2f}x, "
              f"/ dysample {fw / dys:.2f}x")
        del xs, lgs, ys, dxs, dls, offs, cp, variants
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
    cf = [(name, a, ms) for name, a, ms in prof if name in ("dy_carafe", "dy_carafe_backward")]
    print(f"(b) {model_name}, batch {B}, 640x640: {len(prof)} launches in forward + backward, {total:.3f} ms of device time")
    for name, a, ms in cf:
        n, h, w, c = (a[6], a[7], a[8], a[9]) if name == "dy_carafe" else (a[11], a[12], a[13], a[14])
        fl = floors(n, h, w, c)
        f = fl["fwd"] if name == "dy_carafe" else fl["dl"] + fl["dx"]
        print(f"  {name:20s} ({n}, {h}, {w}, {c})  {ms * 1e3:8.1f} us  {f / ms / 1e9:5.2f} TB/s of its byte floor")
    csum = sum(ms for _, _, ms in cf)
    print(f"  {len(cf)} reassembly launches: {csum:.3f} ms = {100 * csum / total:.2f} % of the step's device time (comp, enc and their "
          "gradients are not in this figure)")


def bench_part(parent, rounds):
    """bench.py (unchanged) on the default graph from two trees, each run a fresh child process, alternating."""
    trees = {"parent": os.path.abspath(parent), "this tree": ROOT}
    res = {k: [] for k in trees}
    for _ in range(rounds):
        for k, root in trees.items():
            out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "8", "--no-cpu",
                                  "--probe", "0", "--secondary", "0"], capture_output=True, text=True, timeout=600, cwd=root)
            if out.returncode != 0:
                raise RuntimeError(f"bench.py in {root} failed:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
            res[k].append(json.loads(line))
    print(f"(c) bench.py --steps 30 --warmup 8 --no-cpu --probe 0 --secondary 0 on the default graph, {rounds} runs per tree, alternating")
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
    ap.add_argument("--model", default="yolov8n-ASF-P2P2-CARAFE")
    a = ap.parse_args()
    every = not (a.kernel or a.step or a.bench)
    if not torch.cuda.is_available():
        raise SystemExit("carafe_bench.py measures on the GPU; there is none here")
    if a.bench and not a.parent:
        raise SystemExit("--bench needs --parent DIR")
    if a.kernel or every:
        kernel_part(a.batch, a.rounds)
    if a.step or every:
        step_part(a.model, a.batch)
    if a.bench:
        bench_part(a.parent, 4)
