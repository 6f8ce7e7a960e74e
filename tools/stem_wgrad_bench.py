#!/usr/bin/env python3
"""Stand-alone A/B of the stem launches and of the wide 3x3 weight gradient at the training step's shapes (DEAL-YOLO-N, batch 64,
640 x 640): the kernel behind the switch (DY_STEM_V1=1: the plain stem kernels; DY_WGRAD_WIDE=0 / 1: four / eight waves per workgroup of the 64 x 64 block)
against the other one, alternating in ONE process, --reps timed repetitions after --warmup.  A repetition launches the kernel once on
each of --sets buffer sets (together larger than the 256 MiB Infinity Cache) between two device events.  Prints one JSON line; run one
process per kernel:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/stem_wgrad_bench.py --kernel stem_fwd|stem_eval|stem_wgrad|wgrad160|wgrad80|wgrad40

The kernel durations of the trace are the measurement (profiles/r18_stream_rate.md); the event times in the JSON line are a first look.
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
ap.add_argument("--kernel", required=True, choices=["stem_fwd", "stem_eval", "stem_wgrad", "wgrad160", "wgrad80", "wgrad40"])
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--sets", type=int, default=2)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()

from ultralytics.hip import DY_BN_COPIES  # noqa: E402
from ultralytics.hip.engine import Engine  # noqa: E402

L = Engine("cuda:0").L
s = torch.cuda.current_stream().cuda_stream
N = args.batch
g = torch.Generator(device="cuda").manual_seed(1)


def h16(*shape):
    return torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32).half()


def coef_of(c):
    return torch.cat([torch.rand(c, device="cuda") + 0.5, 0.3 * torch.randn(c, device="cuda"), 0.2 * torch.randn(c, device="cuda"),
                      torch.rand(c, device="cuda") + 0.5]).contiguous()


if args.kernel.startswith("stem"):
    H = W = 640 if args.kernel != "stem_eval" else 1280
    if args.kernel == "stem_eval":
        N = min(N, 32)  # yolov8n-p2 at 1280 x 1280, batch 32
    Ho, Wo = H // 2, W // 2
    SWITCH, OLD, NEW = "DY_STEM_V1", "1", None
    w = (torch.randn(16, 3, 3, 3, device="cuda") / 27 ** 0.5).contiguous()
    bias = torch.randn(16, device="cuda")
    coef = coef_of(16)
    acc = torch.zeros(DY_BN_COPIES * 2 * 16, dtype=torch.float64, device="cuda")
    sets = []
    for _ in range(args.sets):
        img = torch.rand(N, 3, H, W, generator=g, device="cuda")
        raw = h16(N, Ho, Wo, 16)
        dy = h16(N, Ho, Wo, 16) if args.kernel == "stem_wgrad" else None
        sets.append((img, raw, dy))
    slabs = torch.zeros(L.dy_stem_grid(N, H, W) * 9 * 16 * 16, device="cuda")
    dg, db = torch.zeros(16, device="cuda"), torch.zeros(16, device="cuda")
    own = N * 3 * H * W * 4 + N * Ho * Wo * 16 * 2 * (2 if args.kernel == "stem_wgrad" else 1)

    def launch(k):
        img, raw, dy = sets[k]
        if args.kernel == "stem_fwd":
            rc = L.dy_stem_forward(img.data_ptr(), w.data_ptr(), raw.data_ptr(), 16, acc.data_ptr(), N, H, W, 1.0, s)
        elif args.kernel == "stem_eval":
            rc = L.dy_stem_forward_eval(img.data_ptr(), w.data_ptr(), bias.data_ptr(), raw.data_ptr(), 16, N, H, W, 1.0, 1, s)
        else:
            rc = L.dy_stem_wgrad_bn(img.data_ptr(), dy.data_ptr(), 16, raw.data_ptr(), 16, coef.data_ptr(), acc.data_ptr(), dg.data_ptr(),
                                    db.data_ptr(), float(N * Ho * Wo), slabs.data_ptr(), N, H, W, 1.0, s)
        assert rc == 0, rc
else:
    H = W = int(args.kernel[5:])
    cin, cout = (128, 64) if H == 40 else (64, 64)  # the step's launches of the 64 x 64 block: 160 x 160, Detect's at 80 x 80, 128 -> 64 at 40 x 40
    SWITCH, OLD, NEW = "DY_WGRAD_WIDE", "0", "1"
    buf = C.create_string_buffer(128)
    assert L.dy_wgrad_kernel_name_at(N, H, W, cin, cout, 3, 1, buf, 128) == 0 and b"<3, 1, 4, 4, 0>" in buf.value, buf.value
    ns, se = C.c_int(0), C.c_long(0)
    assert L.dy_wgrad_workspace(N, H, W, cin, cout, 3, 1, C.byref(ns), C.byref(se)) == 0
    coef = coef_of(cout)
    acc = torch.zeros(DY_BN_COPIES * 2 * cout, dtype=torch.float64, device="cuda")
    dg, db = torch.zeros(cout, device="cuda"), torch.zeros(cout, device="cuda")
    sets = [(h16(N, H, W, cin), h16(N, H, W, cout), h16(N, H, W, cout), torch.empty(N, H, W, cout, dtype=torch.float16, device="cuda"),
             torch.zeros(ns.value * se.value, device="cuda")) for _ in range(args.sets * (1 if H == 160 else 4))]
    own = N * H * W * (cin + 3 * cout) * 2 + ns.value * se.value * 4

    def launch(k):
        x, dy, raw, draw, slabs = sets[k]
        rc = L.dy_conv_wgrad_bn(x.data_ptr(), cin, dy.data_ptr(), cout, raw.data_ptr(), cout, draw.data_ptr(), coef.data_ptr(), acc.data_ptr(),
                                dg.data_ptr(), db.data_ptr(), float(N * H * W), slabs.data_ptr(), None, N, H, W, cin, cout, 3, 1, 0, s)
        assert rc == 0, rc


def timed(value):
    if value is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = value
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(len(sets)):
        launch(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / len(sets)


out = {"old": [], "new": []}
for i in range(args.warmup + args.reps):
    for name, value in (("old", OLD), ("new", NEW)):
        t = timed(value)
        if i >= args.warmup:
            out[name].append(t)
os.environ.pop(SWITCH, None)
res = {"kernel": args.kernel, "reps": args.reps, "own_MB": round(own / 1e6, 1)}
for name, v in out.items():
    m = statistics.mean(v)
    res[name] = {"mean_us": round(m, 2), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                 "stdev_us": round(statistics.stdev(v), 2), "TBps": round(own / m / 1e6, 2)}
res["speedup"] = round(res["old"]["mean_us"] / res["new"]["mean_us"], 3)
print(json.dumps(res))
