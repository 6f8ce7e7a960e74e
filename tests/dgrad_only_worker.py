"""Runs the backward of FROZEN 1x1 Conv + BatchNorm + SiLU layers through the C ABI and saves the results: tests/test_gpu_dgrad_only.py
compares, per case, the dX of the fused weight + input gradient launch (dy_conv1x1_wgrad_dgrad_bn / _segs / _planes, csrc/conv_wgrad.hip
BNF 5 / 7) with the dX of the launch that forms the input gradient alone (dy_conv1x1_dgrad_bn, BNF 13 / 15) on the same operands and the
same old dX values.  The new entry has no X argument at all: the kernel runs with a null X pointer, so nothing of X can be read.
The caller starts this process with DY_WGRAD_SPLIT=0: the weight-gradient geometry then keeps every output channel in one workgroup
block on small maps too, which is where both launches exist (dy_conv1x1_wgrad_dgrad_supported) -- the instantiations are those of the
training step's large maps, the maps stay small.
usage: dgrad_only_worker.py <out.pt>"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "experiment-yolo_amd")
sys.path[:0] = [ROOT, PKG, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from ultralytics.hip import DY_BN_COPIES, DySegs  # noqa: E402
from ultralytics.hip.engine import ConvSpec, Engine  # noqa: E402

# name, (N, H, W), input channels (an int: one tensor; a tuple: concatenation members), cout, dY in two planes, index of an up-sampled member,
# store / accumulate of dX per member (a plain input runs both).  Maps of at most 40x40 at batch 2: 12-25 tiles, several workgroups.
CASES = [
    ("16_16", (2, 40, 40), 16, 16, False, None, None),                 # one k-step of 16 real channels
    ("32_32", (2, 40, 40), 32, 32, False, None, None),
    ("64_64", (2, 40, 40), 64, 64, False, None, None),
    ("64_32", (2, 32, 32), 64, 32, False, None, None),
    ("128_64", (2, 20, 20), 128, 64, False, None, None),               # two Cin chunks: grid rows that repeat the d(raw) arithmetic
    ("128_32", (2, 20, 20), 128, 32, False, None, None),
    ("64_48", (2, 40, 40), 64, 48, False, None, None),                 # three k-steps of 16 real channels
    ("3x16_32", (2, 40, 40), (16, 16, 16), 32, False, None, (0, 1, 0)),    # 16-channel members, store and add side by side
    ("64up+32_64", (2, 40, 40), (64, 32), 64, False, 0, (1, 0)),       # an up-sampled member: its gradient tensor is full-resolution
    ("planes_64_64", (2, 40, 40), 64, 64, True, None, None),           # C2f.cv1: the output gradient in two planes
    ("planes_2x32_64", (2, 40, 40), (32, 32), 64, True, None, (1, 0)),
    ("ragged_32_32", (1, 13, 7), 32, 32, False, None, None),           # 91 pixels: less than one tile, no multiple of 16
    ("ragged_planes_64_64", (1, 13, 7), 64, 64, True, None, None),
    ("ragged_2x32_32", (2, 13, 7), (32, 32), 32, False, None, (0, 1)),
    ("batch1_64_64", (1, 40, 40), 64, 64, False, None, None),
    ("loop_16_16", (2, 320, 320), 16, 16, False, None, None),          # 800 tiles for 768 resident workgroups: the persistent loop takes a second tile
]
ORACLE = ("64_64", "128_32", "64_48")  # cases whose operands are saved too: the test rebuilds dX in fp32


def main(out):
    assert os.environ.get("DY_WGRAD_SPLIT") == "0", "start this worker with DY_WGRAD_SPLIT=0 (see the module docstring)"
    eng = Engine("cuda:0")
    L = eng.L
    res, names = {}, {}

    def rnd(gen, *shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).half().cuda()

    for name, (N, H, W), cin_s, cout, planes, up, accs in CASES:
        seg = isinstance(cin_s, tuple)
        parts = cin_s if seg else (cin_s,)
        cin, npix = sum(parts), N * H * W
        assert L.dy_conv1x1_wgrad_dgrad_supported(N, H, W, cin, cout) == 1, name
        assert L.dy_conv1x1_dgrad_bn_supported(N, H, W, cin, cout) == 1, name
        gen = torch.Generator().manual_seed(sum(map(ord, name)) * 7 + cin + cout)
        w = (torch.randn(cout, cin, 1, 1, generator=gen) / cin ** 0.5).cuda()
        sp = ConvSpec("c", w, None, None, 1, 1, 0)
        eng.prepare_conv(sp)
        eng.pack(sp)
        xt, xs = [], DySegs()
        xs.nseg, end = len(parts), 0
        for i, c in enumerate(parts):
            end += c
            ld = c + 8 * ((i + 1) % 2)
            t = rnd(gen, N, H // 2, W // 2, ld) if up == i else rnd(gen, N, H, W, ld)
            xt.append(t)
            xs.c_end[i], xs.ld[i], xs.ptr[i], xs.acc[i] = end, ld, t.data_ptr(), (2 if up == i else 0)
        if planes:
            cs = cout // 2
            dy = rnd(gen, 2, N, H, W, cs, scale=0.05)
            dyp, dyp2, lddy = dy.data_ptr(), dy[1].data_ptr(), cs
        else:
            lddy = cout + 16
            dy = rnd(gen, N, H, W, lddy, scale=0.05)
            dyp, dyp2 = dy.data_ptr(), 0
        raw = rnd(gen, N, H, W, cout)
        coef = torch.cat([torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen) * 0.1, torch.randn(cout, generator=gen) * 0.1,
                          torch.rand(cout, generator=gen) * 1.5 + 0.5]).float().cuda()
        acc = torch.zeros(DY_BN_COPIES, 2, cout, dtype=torch.float64)
        acc[:3] = torch.randn(3, 2, cout, generator=gen).double() * npix * 0.003
        acc = acc.cuda()
        ns, se = C.c_int(), C.c_long()
        L.dy_wgrad_workspace(N, H, W, cin, cout, 1, 1, C.byref(ns), C.byref(se))
        buf = C.create_string_buffer(128)
        assert L.dy_dgrad_only_kernel_name(N, H, W, cin, cout, int(seg), buf, 128) == 0
        names[name] = buf.value.decode()
        if name in ORACLE:
            src = torch.cat([dy[0], dy[1]], dim=-1) if planes else dy[..., :cout]
            res[f"oracle/{name}"] = dict(dy=src.contiguous().cpu(), raw=raw.cpu(), coef=coef.cpu(), acc=acc.cpu(), w=w.cpu())

        for mode in ((accs,) if seg else ((1,) if name.startswith("loop") else (0, 1))):  # (the large map: one mode, to keep the file small)
            tag = name + ("/" + "".join(map(str, mode)) if seg else ("/accumulate" if mode else "/store"))
            for form in ("fused", "only"):
                gen2 = torch.Generator().manual_seed(cin * 3 + cout + H)  # the same old dX values for both forms
                gt, dxs = [], DySegs()
                dxs.nseg, end = len(parts), 0
                for i, c in enumerate(parts):
                    end += c
                    ld = c + 8 * (i % 2) if seg else c + 8
                    t = rnd(gen2, N, H, W, ld)
                    gt.append(t)
                    dxs.c_end[i], dxs.ld[i], dxs.ptr[i], dxs.acc[i] = end, ld, t.data_ptr(), (mode[i] if seg else 0)
                if form == "fused":
                    for i, t in enumerate(gt):
                        res[f"{tag}/old{i}"] = t.cpu()
                dx = (0, 0, 0) if seg else (gt[0].data_ptr(), dxs.ld[0], int(mode))
                wt = sp.wpack_t.data_ptr()
                if form == "fused":
                    slabs = torch.zeros(ns.value * se.value, dtype=torch.float32, device="cuda")
                    dw = torch.zeros(cout, cin, 1, 1, dtype=torch.float32, device="cuda")
                    dgam, dbet = torch.zeros(cout, device="cuda"), torch.zeros(cout, device="cuda")
                    bnargs = (coef.data_ptr(), acc.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), float(npix), slabs.data_ptr(), dw.data_ptr())
                    x0, ld0 = (0, 0) if seg else (xt[0].data_ptr(), xs.ld[0])
                    if planes:
                        eng.call("dy_conv1x1_wgrad_dgrad_bn_planes", C.byref(xs) if seg else None, x0, ld0, dyp, dyp2, lddy, cout // 2, raw.data_ptr(),
                                 cout, *bnargs, wt, *dx, C.byref(dxs) if seg else None, N, H, W, cin, cout, 0)
                    elif seg:
                        eng.call("dy_conv1x1_wgrad_dgrad_bn_segs", C.byref(xs), dyp, lddy, raw.data_ptr(), cout, *bnargs, wt, C.byref(dxs), N, H, W,
                                 cin, cout, 0)
                    else:
                        eng.call("dy_conv1x1_wgrad_dgrad_bn", x0, ld0, dyp, lddy, raw.data_ptr(), cout, *bnargs, wt, *dx, N, H, W, cin, cout, 0)
                else:
                    eng.call("dy_conv1x1_dgrad_bn", dyp, dyp2, lddy, cout // 2 if planes else 0, raw.data_ptr(), cout, coef.data_ptr(), acc.data_ptr(),
                             float(npix), wt, *dx, C.byref(dxs) if seg else None, N, H, W, cin, cout)
                torch.cuda.synchronize()
                for i, t in enumerate(gt):
                    res[f"{tag}/{form}/dx{i}"] = t.cpu()  # the whole buffers: the stride padding behind a member must keep its old values
    torch.save({"res": res, "names": names, "parts": {c[0]: (c[2] if isinstance(c[2], tuple) else (c[2],)) for c in CASES}}, out)


if __name__ == "__main__":
    main(sys.argv[1])
