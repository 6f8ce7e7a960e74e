#!/usr/bin/env python3
"""Stand-alone A/B of one tensor_ops launch of the training step at the step's shape (DEAL-YOLO-N, batch 64, 640 x 640): the kernel behind
DY_TENSOR_OPS_V1=1 against the default one, alternating in ONE process, --reps timed repetitions after --warmup.  A repetition launches
the kernel once on each of --sets buffer sets (together larger than the 256 MiB Infinity Cache, so no launch finds its inputs cached by the
launch before) between two device events.  Prints one JSON line; run one process per kernel:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/tensor_ops_bench.py --kernel scalseq0|scalseq1|sppf_fwd|sppf_bwd

The kernel durations of the trace are the measurement (profiles/r15_tensor_ops.md).  The event times in the JSON line are a first look
only: they include the host's launch rate, which bounds them for the short SPPF launches (one ctypes call per launch).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", required=True, choices=["scalseq0", "scalseq1", "sppf_fwd", "sppf_bwd"])
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--sets", type=int, default=3)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()

from ultralytics.hip.engine import Engine  # noqa: E402

L = Engine("cuda:0").L
s = torch.cuda.current_stream().cuda_stream
N = args.batch
g = torch.Generator(device="cuda").manual_seed(1)


def h16(*shape):
    return torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32).half()


if args.kernel.startswith("scalseq"):
    H = W = 160
    Cc = 32
    mode = int(args.kernel[-1])
    sets = []
    for _ in range(args.sets):
        r = [h16(N, H >> l, W >> l, Cc) for l in range(3)]
        dy = h16(N, H, W, Cc)
        dr = [torch.empty_like(t) for t in r] if mode else [None] * 3
        sets.append((r, dy, dr))
    coef = torch.stack([torch.rand(Cc, device="cuda") + 0.5, 0.3 * torch.randn(Cc, device="cuda"), 0.2 * torch.randn(Cc, device="cuda"),
                        torch.rand(Cc, device="cuda") + 0.5]).contiguous()
    bw = (0.05 * torch.randn(2, Cc, device="cuda")).contiguous()
    part = torch.zeros(2048 * 2 * Cc, device="cuda")
    n = C.c_int(0)
    own = (sum(t.numel() for t in sets[0][0]) + sets[0][1].numel()) * 2 * (2 if mode else 1) - (sets[0][1].numel() * 2 if mode else 0)

    def launch(k):
        r, dy, dr = sets[k]
        p = lambda t: t.data_ptr() if t is not None else 0  # noqa: E731
        rc = L.dy_scalseq_tail_backward_all(r[0].data_ptr(), Cc, r[1].data_ptr(), Cc, r[2].data_ptr(), Cc, dy.data_ptr(), Cc, p(dr[0]), Cc, p(dr[1]), Cc,
                                            p(dr[2]), Cc, coef.data_ptr(), bw.data_ptr() if mode else 0, 0 if mode else part.data_ptr(), 2048, N, H, W,
                                            Cc, mode, None if mode else C.byref(n), s)
        assert rc == 0, rc
else:
    H = W = 40
    Cc = 64  # SPPF's hidden width in DEAL-YOLO-N: 64 images x 4 groups of 16 channels = 256 workgroups
    assert L.dy_sppf_pool3_supported(H, W, Cc)
    sets = []
    for _ in range(args.sets * 4):  # the maps are small: more sets to get past the cache
        cat = h16(N, H, W, 4 * Cc)
        arg = [torch.zeros(N * H * W * Cc, dtype=torch.uint8, device="cuda") for _ in range(3)]
        L.dy_sppf_pool3(cat.data_ptr(), 4 * Cc, Cc, arg[0].data_ptr(), arg[1].data_ptr(), arg[2].data_ptr(), N, H, W, s)  # valid arg maps
        sets.append((cat, arg, h16(N, H, W, 4 * Cc)))
    fwd = args.kernel == "sppf_fwd"
    own = N * H * W * Cc * ((2 * 4 + 3) if fwd else (2 * 5 + 3))

    def launch(k):
        cat, arg, gcat = sets[k]
        if fwd:
            rc = L.dy_sppf_pool3(cat.data_ptr(), 4 * Cc, Cc, arg[0].data_ptr(), arg[1].data_ptr(), arg[2].data_ptr(), N, H, W, s)
        else:
            rc = L.dy_sppf_pool3_backward(gcat.data_ptr(), 4 * Cc, Cc, arg[0].data_ptr(), arg[1].data_ptr(), arg[2].data_ptr(), N, H, W, 1, 1, 1, s)
        assert rc == 0, rc


def timed(v1):
    if v1:
        os.environ["DY_TENSOR_OPS_V1"] = "1"
    else:
        os.environ.pop("DY_TENSOR_OPS_V1", None)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(len(sets)):
        launch(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / len(sets)


out = {"old": [], "new": []}
for i in range(args.warmup + args.reps):
    for name, v1 in (("old", True), ("new", False)):
        t = timed(v1)
        if i >= args.warmup:
            out[name].append(t)
os.environ.pop("DY_TENSOR_OPS_V1", None)
res = {"kernel": args.kernel, "reps": args.reps, "own_MB": round(own / 1e6, 1)}
for name, v in out.items():
    m = statistics.mean(v)
    res[name] = {"mean_us": round(m, 2), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                 "stdev_us": round(statistics.stdev(v), 2), "TBps": round(own / m / 1e6, 2)}
res["speedup"] = round(res["old"]["mean_us"] / res["new"]["mean_us"], 3)
print(json.dumps(res))
