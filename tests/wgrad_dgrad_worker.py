"""Runs the backward of 1x1 Conv + BatchNorm + SiLU layers through the C ABI and saves the results: tests/test_gpu_wgrad_dgrad.py compares
the files of two processes, DY_WGRAD_DGRAD=0 (two launches: dy_conv_wgrad_bn / _segs / _planes, which write d(raw), then the input
gradient through dy_conv_forward over the transposed pack or dy_conv1x1_input_grad_segs) and anything else (ONE launch:
dy_conv1x1_wgrad_dgrad_bn / _segs / _planes, csrc/conv_wgrad.hip BNF 5 / 7).  Inputs, BatchNorm coefficients and the backward sums are
drawn on the CPU from fixed seeds, so both processes see the same bits.
usage: wgrad_dgrad_worker.py <out.pt>"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "experiment-yolo_amd")
sys.path[:0] = [ROOT, PKG, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from ultralytics.hip import DY_BN_COPIES, DY_EPI_ACCUM, DySegs  # noqa: E402
from ultralytics.hip.engine import ConvSpec, Engine  # noqa: E402

FUSED = os.environ.get("DY_WGRAD_DGRAD", "1") != "0"

# name, (N, H, W), input channels (an int: one tensor; a tuple: concatenation members), cout, dY in two planes, index of an up-sampled member,
# store / accumulate of dX (per member for a concatenation; a plain input runs both).  Every map is large enough for wgrad_geometry to keep
# all output channels in one workgroup block (the worker asserts that the helper says yes).
CASES = [
    ("32_32@160", (2, 160, 160), 32, 32, False, None, None),          # the step's shapes
    ("64_64@80", (6, 80, 80), 64, 64, False, None, None),
    ("64_32@80", (4, 80, 80), 64, 32, False, None, None),
    ("128_64@40", (16, 40, 40), 128, 64, False, None, None),
    ("128_32@40", (16, 40, 40), 128, 32, False, None, None),
    ("3x16_32@160", (1, 160, 160), (16, 16, 16), 32, False, None, (0, 1, 0)),    # 16-channel members, batch 1
    ("3x32_64@80", (4, 80, 80), (32, 32, 32), 64, False, None, (1, 0, 1)),
    ("64up+32_64@80", (4, 80, 80), (64, 32), 64, False, 0, (0, 0)),
    ("planes_64_64@80", (6, 80, 80), 64, 64, True, None, None),        # C2f.cv1: the output gradient in two planes
    ("planes_2x32_64@80", (6, 80, 80), (32, 32), 64, True, None, (1, 1)),
    ("ragged_32_32", (1, 161, 159), 32, 32, False, None, None),        # 25599 (39999) pixels: no multiple of a 128- or 256-pixel tile
    ("ragged_planes_64_64", (1, 201, 199), 64, 64, True, None, None),
    ("ragged_2x32_32", (1, 161, 159), (32, 32), 32, False, None, (0, 1)),
    ("batch1_64_64@200", (1, 200, 200), 64, 64, False, None, None),
    ("16_16@160", (1, 160, 160), 16, 16, False, None, None),           # one k-step of 16 real channels
    ("32_16@160", (1, 160, 160), 32, 16, False, None, None),
    ("64_48@80", (4, 80, 80), 64, 48, False, None, None),              # three k-steps of 16 real channels
    ("96_48@80", (4, 80, 80), 96, 48, False, None, None),
]
ORACLE = ("64_64@80", "128_32@40", "64_48@80")  # cases whose operands are saved too: the test rebuilds dX in fp32


def main(out):
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
        gen = torch.Generator().manual_seed(sum(map(ord, name)) * 7 + cin + cout)
        w = (torch.randn(cout, cin, 1, 1, generator=gen) / cin ** 0.5).cuda()
        sp = ConvSpec("c", w, None, None, 1, 1, 0)
        eng.prepare_conv(sp)
        eng.pack(sp)
        # operands: X (members with pixel strides of their own, one possibly at half resolution), dY, raw, coefficients, backward sums
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
        assert L.dy_wgrad_dgrad_kernel_name(N, H, W, cin, cout, int(seg), buf, 128) == 0
        names[name] = buf.value.decode()
        if name in ORACLE:
            res[f"oracle/{name}"] = dict(dy=dy[..., :cout].contiguous().cpu(), raw=raw.cpu(), coef=coef.cpu(), acc=acc.cpu(), w=w.cpu())

        # dX targets: members' gradient tensors (full resolution, strides of their own) or one tensor; old values are random
        for mode in ((accs,) if seg else (0, 1)):
            gen2 = torch.Generator().manual_seed(cin * 3 + cout + H)
            gt, dxs = [], DySegs()
            dxs.nseg, end = len(parts), 0
            for i, c in enumerate(parts):
                end += c
                ld = c + 8 * (i % 2) if seg else c + 8
                t = rnd(gen2, N, H, W, ld)
                gt.append(t)
                dxs.c_end[i], dxs.ld[i], dxs.ptr[i], dxs.acc[i] = end, ld, t.data_ptr(), (mode[i] if seg else 0)
            slabs = torch.zeros(ns.value * se.value, dtype=torch.float32, device="cuda")
            dw = torch.zeros(cout, cin, 1, 1, dtype=torch.float32, device="cuda")
            dgam, dbet = torch.zeros(cout, device="cuda"), torch.zeros(cout, device="cuda")
            bnargs = (coef.data_ptr(), acc.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), float(npix), slabs.data_ptr(), dw.data_ptr())
            x0, ld0 = (0, 0) if seg else (xt[0].data_ptr(), xs.ld[0])
            wt = sp.wpack_t.data_ptr()
            if FUSED:
                dx = (0, 0, 0) if seg else (gt[0].data_ptr(), dxs.ld[0], int(mode))
                if planes:
                    eng.call("dy_conv1x1_wgrad_dgrad_bn_planes", C.byref(xs) if seg else None, x0, ld0, dyp, dyp2, lddy, cout // 2, raw.data_ptr(), cout,
                             *bnargs, wt, *dx, C.byref(dxs) if seg else None, N, H, W, cin, cout, 0)
                elif seg:
                    eng.call("dy_conv1x1_wgrad_dgrad_bn_segs", C.byref(xs), dyp, lddy, raw.data_ptr(), cout, *bnargs, wt, C.byref(dxs), N, H, W, cin, cout, 0)
                else:
                    eng.call("dy_conv1x1_wgrad_dgrad_bn", x0, ld0, dyp, lddy, raw.data_ptr(), cout, *bnargs, wt, *dx, N, H, W, cin, cout, 0)
            else:
                draw = torch.zeros(N, H, W, cout, dtype=torch.float16, device="cuda")
                head = (raw.data_ptr(), cout, draw.data_ptr())
                if planes:
                    eng.call("dy_conv1x1_wgrad_bn_planes", C.byref(xs) if seg else None, x0, ld0, dyp, dyp2, lddy, cout // 2, *head, *bnargs,
                             N, H, W, cin, cout, 0)
                elif seg:
                    eng.call("dy_conv1x1_wgrad_bn_segs", C.byref(xs), dyp, lddy, *head, *bnargs, N, H, W, cin, cout, 0)
                else:
                    eng.call("dy_conv_wgrad_bn", x0, ld0, dyp, lddy, *head, *bnargs, N, H, W, cin, cout, 1, 1, 0)
                if seg:
                    eng.call("dy_conv1x1_input_grad_segs", draw.data_ptr(), cout, wt, C.byref(dxs), N, H, W, sp.cout_phys, cin)
                else:
                    eng.call("dy_conv_forward", draw.data_ptr(), cout, wt, 0, gt[0].data_ptr(), dxs.ld[0], 0, N, H, W, sp.cout_phys, cin, 1, 1, 1,
                             H, W, DY_EPI_ACCUM if mode else 0, None)
                if name in ORACLE and not mode:
                    res[f"oracle/{name}"]["draw"] = draw.cpu()
            torch.cuda.synchronize()
            tag = name + ("/" + "".join(map(str, mode)) if seg else ("/accumulate" if mode else "/store"))
            for i, c in enumerate(parts):
                # the whole buffers: channels past the member's own (the stride padding) must keep their old values
                res[f"{tag}/dx{i}"] = gt[i].cpu()
            res[f"{tag}/dw"], res[f"{tag}/dgamma"], res[f"{tag}/dbeta"] = dw.cpu(), dgam.cpu(), dbet.cpu()
    torch.save({"res": res, "names": names, "fused": FUSED}, out)


if __name__ == "__main__":
    main(sys.argv[1])
