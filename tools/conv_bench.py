#!/usr/bin/env python3
"""Micro-benchmark of single dy_conv_forward / dy_conv_wgrad launches (algorithmic GB/s and TFLOP/s).
usage: conv_bench.py [fwd|wgrad] cin cout ks stride H W [N] [reps]
       conv_bench.py pair cin cout H W [N] [reps]     the backward of one 1x1 Conv + BatchNorm + SiLU stand-alone: the two-launch pair
           (dy_conv_wgrad_bn / _segs, then the input gradient) against the fused launch (dy_conv1x1_wgrad_dgrad_bn / _segs); cin = 64
           times dX stored and accumulated, cin = 32+32+32 (concatenation members) times the segmented form, members adding alternately
       conv_bench.py frozen cin cout H W [N] [reps]   the backward of one FROZEN 1x1 Conv + BatchNorm + SiLU stand-alone: the two-launch form
           (dy_bn_act_bwd_apply_acc, then the input gradient) against the launch that forms the input gradient alone (dy_conv1x1_dgrad_bn)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
import torch  # noqa: E402

from ultralytics.hip.engine import ConvSpec, Engine, Storage  # noqa: E402



def pair_bench(argv):
    import ctypes as C
    from ultralytics.hip import DY_BN_COPIES, DY_EPI_ACCUM, DySegs
    parts = tuple(map(int, argv[0].split("+")))
    cout, H, W = map(int, argv[1:4])
    N = int(argv[4]) if len(argv) > 4 else 64
    reps = int(argv[5]) if len(argv) > 5 else 20
    seg, cin, npix = len(parts) > 1, sum(parts), N * H * W
    eng = Engine("cuda:0")
    L = eng.L
    if not L.dy_conv1x1_wgrad_dgrad_supported(N, H, W, cin, cout):
        sys.exit(f"pair {cin}->{cout} @{H}x{W} n={N}: no fused form for this geometry (dy_conv1x1_wgrad_dgrad_supported)")
    w = torch.randn(cout, cin, 1, 1, device="cuda") / cin ** 0.5
    sp = ConvSpec("b", w, None, None, 1, 1, 0)
    eng.prepare_conv(sp)
    eng.pack(sp)
    half = lambda *sh: torch.randn(*sh, device="cuda").half()  # noqa: E731
    xt, gt = [half(N, H, W, c) for c in parts], [half(N, H, W, c) for c in parts]
    dy, raw, draw = half(N, H, W, cout) * 0.05, half(N, H, W, cout), half(N, H, W, cout)
    coef = torch.cat([torch.rand(cout) + 0.5, torch.randn(cout) * 0.1, torch.randn(cout) * 0.1, torch.rand(cout) + 0.5]).cuda()
    acc = torch.randn(DY_BN_COPIES, 2, cout, dtype=torch.float64, device="cuda") * npix * 1e-3
    ns, se = C.c_int(), C.c_long()
    L.dy_wgrad_workspace(N, H, W, cin, cout, 1, 1, C.byref(ns), C.byref(se))
    slabs = torch.zeros(ns.value * se.value, device="cuda")
    dw, dg, db = torch.zeros_like(w), torch.zeros(cout, device="cuda"), torch.zeros(cout, device="cuda")
    bn = (coef.data_ptr(), acc.data_ptr(), dg.data_ptr(), db.data_ptr(), float(npix), slabs.data_ptr(), dw.data_ptr())
    tail = (N, H, W, cin, cout, 0)
    wt = sp.wpack_t.data_ptr()

    def table(tens, accs):
        t, end = DySegs(), 0
        t.nseg = len(parts)
        for i, c in enumerate(parts):
            end += c
            t.c_end[i], t.ld[i], t.ptr[i], t.acc[i] = end, c, tens[i].data_ptr(), accs[i]
        return t

    def timed(f):
        for _ in range(3):
            f()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            f()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps * 1e3

    xs = table(xt, [0] * len(parts))
    forms = [("segmented", [i % 2 for i in range(len(parts))])] if seg else [("store", 0), ("accumulate", 1)]
    for tag, a in forms:
        if seg:
            dxs = table(gt, a)
            two = lambda: (eng.call("dy_conv1x1_wgrad_bn_segs", C.byref(xs), dy.data_ptr(), cout, raw.data_ptr(), cout, draw.data_ptr(), *bn, *tail),  # noqa: E731
                           eng.call("dy_conv1x1_input_grad_segs", draw.data_ptr(), cout, wt, C.byref(dxs), N, H, W, cout, cin))
            one = lambda: eng.call("dy_conv1x1_wgrad_dgrad_bn_segs", C.byref(xs), dy.data_ptr(), cout, raw.data_ptr(), cout, *bn, wt, C.byref(dxs), *tail)  # noqa: E731
            old = sum(c for c, f in zip(parts, a) if f)
        else:
            two = lambda: (eng.call("dy_conv_wgrad_bn", xt[0].data_ptr(), cin, dy.data_ptr(), cout, raw.data_ptr(), cout, draw.data_ptr(), *bn,  # noqa: E731
                                    N, H, W, cin, cout, 1, 1, 0),
                           eng.call("dy_conv_forward", draw.data_ptr(), cout, wt, 0, gt[0].data_ptr(), cin, 0, N, H, W, cout, cin, 1, 1, 1, H, W,
                                    DY_EPI_ACCUM if a else 0, None))
            one = lambda: eng.call("dy_conv1x1_wgrad_dgrad_bn", xt[0].data_ptr(), cin, dy.data_ptr(), cout, raw.data_ptr(), cout, *bn, wt,  # noqa: E731
                                   gt[0].data_ptr(), cin, a, *tail)
            old = cin if a else 0
        t2, t1 = timed(two), timed(one)
        b2, b1 = npix * (2 * cin + 4 * cout + old) * 2, npix * (2 * cin + 2 * cout + old) * 2  # own bytes: the pair also writes and reads d(raw)
        print(f"pair {argv[0]}->{cout} @{H}x{W} n={N} {tag}: two launches {t2:.1f} us ({b2 / t2 / 1e6:.2f} TB/s)  fused {t1:.1f} us ({b1 / t1 / 1e6:.2f} TB/s)  "
              f"saved {t2 - t1:.1f} us")


def frozen_bench(argv):
    import ctypes as C
    from ultralytics.hip import DY_ACT_SILU, DY_BN_COPIES, DY_EPI_ACCUM, DySegs
    parts = tuple(map(int, argv[0].split("+")))
    cout, H, W = map(int, argv[1:4])
    N = int(argv[4]) if len(argv) > 4 else 64
    reps = int(argv[5]) if len(argv) > 5 else 20
    seg, cin, npix = len(parts) > 1, sum(parts), N * H * W
    eng = Engine("cuda:0")
    L = eng.L
    if not L.dy_conv1x1_dgrad_bn_supported(N, H, W, cin, cout):
        sys.exit(f"frozen {cin}->{cout} @{H}x{W} n={N}: no input-gradient-only form for this geometry (dy_conv1x1_dgrad_bn_supported)")
    w = torch.randn(cout, cin, 1, 1, device="cuda") / cin ** 0.5
    sp = ConvSpec("b", w, None, None, 1, 1, 0)
    eng.prepare_conv(sp)
    eng.pack(sp)
    half = lambda *sh: torch.randn(*sh, device="cuda").half()  # noqa: E731
    gt = [half(N, H, W, c) for c in parts]
    dy, raw, draw = half(N, H, W, cout) * 0.05, half(N, H, W, cout), half(N, H, W, cout)
    coef = torch.cat([torch.rand(cout) + 0.5, torch.randn(cout) * 0.1, torch.randn(cout) * 0.1, torch.rand(cout) + 0.5]).cuda()
    acc = torch.randn(DY_BN_COPIES, 2, cout, dtype=torch.float64, device="cuda") * npix * 1e-3
    dg, db = torch.zeros(cout, device="cuda"), torch.zeros(cout, device="cuda")
    wt = sp.wpack_t.data_ptr()

    def timed(f):
        for _ in range(3):
            f()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            f()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps * 1e3

    apply = lambda: eng.call("dy_bn_act_bwd_apply_acc", dy.data_ptr(), cout, raw.data_ptr(), cout, draw.data_ptr(), cout, coef.data_ptr(),  # noqa: E731
                             acc.data_ptr(), dg.data_ptr(), db.data_ptr(), npix, cout, DY_ACT_SILU, float(npix))
    forms = [("segmented", [i % 2 for i in range(len(parts))])] if seg else [("store", 0), ("accumulate", 1)]
    for tag, a in forms:
        if seg:
            dxs, end = DySegs(), 0
            dxs.nseg = len(parts)
            for i, c in enumerate(parts):
                end += c
                dxs.c_end[i], dxs.ld[i], dxs.ptr[i], dxs.acc[i] = end, c, gt[i].data_ptr(), a[i]
            two = lambda: (apply(), eng.call("dy_conv1x1_input_grad_segs", draw.data_ptr(), cout, wt, C.byref(dxs), N, H, W, cout, cin))  # noqa: E731
            one = lambda: eng.call("dy_conv1x1_dgrad_bn", dy.data_ptr(), 0, cout, 0, raw.data_ptr(), cout, coef.data_ptr(), acc.data_ptr(), float(npix),  # noqa: E731
                                   wt, 0, 0, 0, C.byref(dxs), N, H, W, cin, cout)
            old = sum(c for c, f in zip(parts, a) if f)
        else:
            two = lambda: (apply(), eng.call("dy_conv_forward", draw.data_ptr(), cout, wt, 0, gt[0].data_ptr(), cin, 0, N, H, W, cout, cin, 1, 1, 1,  # noqa: E731
                                             H, W, DY_EPI_ACCUM if a else 0, None))
            one = lambda: eng.call("dy_conv1x1_dgrad_bn", dy.data_ptr(), 0, cout, 0, raw.data_ptr(), cout, coef.data_ptr(), acc.data_ptr(), float(npix),  # noqa: E731
                                   wt, gt[0].data_ptr(), cin, a, None, N, H, W, cin, cout)
            old = cin if a else 0
        t2, t1 = timed(two), timed(one)
        b2, b1 = npix * (cin + 4 * cout + old) * 2, npix * (cin + 2 * cout + old) * 2  # own bytes: the pair also writes and reads d(raw)
        print(f"frozen {argv[0]}->{cout} @{H}x{W} n={N} {tag}: apply + input gradient {t2:.1f} us ({b2 / t2 / 1e6:.2f} TB/s)  one launch {t1:.1f} us "
              f"({b1 / t1 / 1e6:.2f} TB/s)  saved {t2 - t1:.1f} us", flush=True)


if sys.argv[1] == "pair":
    pair_bench(sys.argv[2:])
    sys.exit(0)
if sys.argv[1] == "frozen":
    frozen_bench(sys.argv[2:])
    sys.exit(0)
mode, cin, cout, ks, s, H, W = sys.argv[1], *map(int, sys.argv[2:8])
N = int(sys.argv[8]) if len(sys.argv) > 8 else 64
reps = int(sys.argv[9]) if len(sys.argv) > 9 else 20
eng = Engine("cuda:0")
w = torch.randn(cout, cin, ks, ks, device="cuda") / (cin * ks * ks) ** 0.5
sp = ConvSpec("b", w, None, None, ks, s, 0)
sp.gweight = torch.zeros_like(w)
eng.prepare_conv(sp)
eng.pack(sp)
cp = (cin + 7) // 8 * 8
x = Storage(eng, N, H, W, cp)
x.buf.copy_(torch.randn_like(x.buf))
xa = x.act()
Ho, Wo = eng.out_hw(sp, xa)
y = Storage(eng, N, Ho, Wo, (cout + 7) // 8 * 8)
y.buf.copy_(torch.randn_like(y.buf))
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
EPI = int(os.environ.get("DY_EPI", "0"))  # 16 = accumulate, 33 = BatchNorm sums into an fp64 accumulator (DY_EPI_STATS | DY_EPI_STATS_ACC)
ACC = torch.zeros(16 * 2 * ((cout + 15) // 16 * 16), dtype=torch.float64, device="cuda")


def run():
    if mode == "fwd":
        eng._conv_raw(sp, xa, y.buf.data_ptr(), y.C, EPI, ACC.data_ptr() if EPI & 1 else 0)
    else:
        eng._conv_bwd(sp, Storage.act(x) if False else xa, y.buf.data_ptr(), y.C, Ho, Wo)


xa.needs_grad = False
for _ in range(3):
    run()
torch.cuda.synchronize()
ev[0].record()
for _ in range(reps):
    run()
ev[1].record()
torch.cuda.synchronize()
ms = ev[0].elapsed_time(ev[1]) / reps
by = N * H * W * cp * 2 + N * Ho * Wo * cout * 2
fl = 2 * N * Ho * Wo * cout * cin * ks * ks
print(f"{mode} {cin}->{cout} k{ks} s{s} @{H}x{W} n={N}: {ms*1e3:.1f} us  {by/ms/1e6:.0f} GB/s  {fl/ms/1e9:.1f} TFLOP/s  (v1={'DY_CONV_V1' in os.environ})")
if os.environ.get("DY_TIMING"):
    import ctypes as C
    from ultralytics.hip import lib
    L = lib()
    out = (C.c_ulonglong * 8)()
    L.dy_conv_timing_fetch(out, 1)
    run(); torch.cuda.synchronize()
    L.dy_conv_timing_fetch(out, 1)
    n = max(out[7], 1)
    names = ["loop-top", "k_loop", "epilogue N-tiles", "stage_write(+vmcnt)", "prefetch_issue", "barrier", "epilogue setup (+slot idle)"]
    tot = sum(out[i] for i in range(7))
    for i, nm in enumerate(names):
        print(f"  {nm:22s} {out[i]/n:10.0f} cycles/wave  {100*out[i]/tot:5.1f}%")
    print(f"  total {tot/n:.0f} cycles per wave0, {n} workgroups")
