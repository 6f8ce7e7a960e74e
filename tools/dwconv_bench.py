#!/usr/bin/env python3
"""The depthwise convolution kernels (csrc/dwconv.hip) measured: (a) forward (statistics epilogue), input gradient and weight gradient
stand-alone at the five layer shapes of yolov8n-ASF-P2P2-DW at 640x640, batch 64, each beside a plain copy of the same bytes (the byte
floor) and beside the dense 3x3 launch the layer replaces (dy_conv_forward, its transposed form, dy_conv_wgrad with its reduction),
the variants alternating in one process; (b) the dy_dwconv_* launches' share of a training step of yolov8n-ASF-P2P2-DW (event-timed
replay of the recorded launch list, as tools/op_profile.py times it); (c) ``bench.py --model yolov8n-ASF-P2P2-DW`` beside the default
graph, and the default graph from a checkout of the parent commit (``--parent DIR``, built), each run a fresh child process, alternating.

usage: dwconv_bench.py [--kernel] [--step] [--bench [--parent DIR]] [--batch 64] [--rounds 5]     (parts (a) and (b) when none is named)

Every timed loop walks a ring of buffer sets of at least 1 GiB, so a kernel never finds its operands resident from its previous
repetition.  Byte floors (the weights and slabs are noise): forward = X read + Y written; input gradient = d(raw) read + dX written;
weight gradient = X + d(raw) read.  A row is the median over the rounds of the mean time of 20 launches; its spread is max - min."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
import torch  # noqa: E402

# (H, W, c1, m) of rows 1, 3, 5, 18, 21 at 640x640, scale n; k 3, s 2
SHAPES = [(320, 320, 16, 2), (160, 160, 32, 2), (80, 80, 64, 2), (160, 160, 32, 1), (80, 80, 64, 1)]
K, S = 3, 2
RING_BYTES = 1 << 30
MODEL = "yolov8n-ASF-P2P2-DW"


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
    from ultralytics.hip import DY_EPI_STATS, check, lib
    from ultralytics.nn.modules import Conv
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731

    def call(name, *a):
        check(getattr(L, name)(*a, st), name)

    print("(a) stand-alone, fp16 NHWC, k 3, s 2; us per launch (median of the rounds, spread = max - min), TB/s of the row's own byte floor")
    for H, W, c1, m in SHAPES:
        N, c2, Ho, Wo = batch, c1 * m, H // 2, W // 2
        geom = (N, H, W, c1, m, K, S)
        e_in, e_out = N * H * W * c1, N * Ho * Wo * c2
        fl = dict(fwd=2 * (e_in + e_out), dgrad=2 * (e_in + e_out), wgrad=2 * (e_in + e_out))
        ring = max(2, -(-RING_BYTES // (2 * (e_in + e_out))))
        xs = [torch.randn(N, H, W, c1, device="cuda").half() for _ in range(ring)]
        ys = [torch.randn(N, Ho, Wo, c2, device="cuda").half() for _ in range(ring)]
        dxs = [torch.empty(N, H, W, c1, dtype=torch.float16, device="cuda") for _ in range(ring)]
        w = torch.randn(c2, 1, K, K, device="cuda") / 3
        dw = torch.empty_like(w)
        part = torch.empty(L.dy_dwconv_num_partials(*geom) * 2 * c2 + 1024, device="cuda")
        slabs = torch.empty(L.dy_dwconv_wgrad_slabs(*geom) * c2 * K * K, device="cuda")
        # (a copy reads and writes: half the floor's bytes each way)
        cp = ([torch.empty((e_in + e_out) // 2, dtype=torch.float16, device="cuda") for _ in range(ring)],
              [torch.empty((e_in + e_out) // 2, dtype=torch.float16, device="cuda") for _ in range(ring)])
        # the dense layer this one replaces: Conv(c1, c2, 3, 2) through its own spec (packs, geometry)
        dense = Conv(c1, c2, K, S).cuda()
        rt = dense._runtime(torch.device("cuda", 0))
        sp = rt.spec(dense)
        rt.pack_all(True)
        dpart = torch.empty(L.dy_conv_num_partials(N, H, W, sp.cin_phys, c2, K, S, 1) * 2 * ((c2 + 15) // 16 * 16) + 1024, device="cuda")
        ns, se = C.c_int(), C.c_long()
        L.dy_wgrad_workspace(N, H, W, c1, c2, K, S, C.byref(ns), C.byref(se))
        dslabs = torch.empty(ns.value * se.value, device="cuda")
        gw = torch.empty(c2, c1, K, K, device="cuda")
        variants = {
            "dwconv forward + statistics": ("fwd", [lambda x=x, y=y: call("dy_dwconv_forward", p(x), c1, p(w), 0, p(y), c2, p(part), *geom, DY_EPI_STATS)
                                                    for x, y in zip(xs, ys)]),
            "dwconv input gradient": ("dgrad", [lambda y=y, d=d: call("dy_dwconv_input_grad", p(y), c2, p(w), p(d), c1, 0, *geom) for y, d in zip(ys, dxs)]),
            "dwconv weight gradient": ("wgrad", [lambda x=x, y=y: call("dy_dwconv_wgrad", p(x), c1, p(y), c2, p(slabs), p(dw), 0, *geom) for x, y in zip(xs, ys)]),
            "torch copy_ of the same bytes": ("fwd", [lambda a=a, b=b: b.copy_(a) for a, b in zip(*cp)]),
            "dense 3x3 forward + statistics": ("fwd", [lambda x=x, y=y: call("dy_conv_forward", p(x), c1, p(sp.wpack), 0, p(y), c2, p(dpart), N, H, W, c1, c2, K, S,
                                                                             1, 0, 0, DY_EPI_STATS, None) for x, y in zip(xs, ys)]),
            "dense 3x3 input gradient": ("dgrad", [lambda y=y, d=d: call("dy_conv_forward", p(y), c2, p(sp.wpack_t), 0, p(d), c1, 0, N, Ho, Wo, c2, c1, K, 1, S,
                                                                         H, W, 0, None) for y, d in zip(ys, dxs)]),
            "dense 3x3 weight gradient": ("wgrad", [lambda x=x, y=y: call("dy_conv_wgrad", p(x), c1, p(y), c2, p(dslabs), p(gw), N, H, W, c1, c2, K, S, 0)
                                                    for x, y in zip(xs, ys)]),
        }
        for _, fns in variants.values():  # warm up every variant on every ring slot
            for f in fns:
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(rounds):  # the variants alternate inside every round
            for k, (_, fns) in variants.items():
                times[k].append(timeit(fns))
        print(f"x = ({N}, {H}, {W}, {c1}) -> ({N}, {Ho}, {Wo}, {c2}), m = {m}: byte floor {fl['fwd'] / 1e6:.0f} MB; "
              f"{9 * e_out / 1e9:.2f} G multiply-adds (dense: {9 * c1 * e_out / 1e9:.1f}); ring of {ring}, {rounds} rounds")
        med = {k: statistics.median(ts) for k, ts in times.items()}
        for k, ts in times.items():
            f = fl[variants[k][0]]
            print(f"  {k:34s} {med[k] * 1e3:8.1f} us  (spread {(max(ts) - min(ts)) * 1e3:5.1f})  {f / med[k] / 1e9:5.2f} TB/s of {f / 1e6:.0f} MB")
        cpy = med["torch copy_ of the same bytes"]
        print("  against the copy: " + ", ".join(f"{k.split('dwconv ')[1]} {med[k] / cpy:.2f}x" for k in med if k.startswith("dwconv")))
        del xs, ys, dxs, cp, variants, dense, rt, sp
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
    dw = [(name, a, ms) for name, a, ms in prof if name.startswith("dy_dwconv")]
    print(f"(b) {model_name}, batch {B}, 640x640: {len(prof)} launches in forward + backward, {total:.3f} ms of device time")
    for name, a, ms in dw:
        print(f"  {name:22s} (n, H, W, c1, m, k, s) = {tuple(a[-7:]) if name != 'dy_dwconv_forward' else tuple(a[-8:-1])}  {ms * 1e3:8.1f} us")
    dsum = sum(ms for _, _, ms in dw)
    print(f"  {len(dw)} depthwise launches: {dsum:.3f} ms = {100 * dsum / total:.2f} % of the step's device time (their BatchNorm launches are "
          "not in this figure)")


def bench_part(parent, rounds):
    """bench.py (unchanged) in fresh child processes, alternating: the default graph and the depthwise graph from this tree, and the
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
        raise SystemExit("dwconv_bench.py measures on the GPU; there is none here")
    if a.kernel or every:
        kernel_part(a.batch, a.rounds)
    if a.step or every:
        step_part(a.model, a.batch)
    if a.bench:
        bench_part(a.parent, 3)
