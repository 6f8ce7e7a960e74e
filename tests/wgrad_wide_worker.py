"""Runs the weight gradient of the wide 3x3 blocks (64 x 64 channels per workgroup: csrc/conv_wgrad.hip) through dy_conv_wgrad,
dy_conv_wgrad_bn and dy_conv_wgrad_bias and saves what they wrote.  tests/test_gpu_wgrad_wide.py compares the files of two processes
started with DY_WGRAD_WIDE=0 (four waves per workgroup) and =1 (eight waves), both with DY_WGRAD_SPLIT=0 so that maps this small still
launch the 64 x 64 block.
usage: wgrad_wide_worker.py <out.pt>"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "experiment-yolo_amd")
sys.path[:0] = [ROOT, PKG, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

BLOCKS = [(64, 64), (128, 64)]  # (cin, cout): one and two Cin chunks of the 64 x 64 block
# (N, H, W): two tile columns, the second one pixel wide; several tiles per column with a ragged last row; one tile, so that some
# workgroups' prefetch has no second tile; the 40 x 40 map of the step's 128 -> 64 launch
SHAPES = [(2, 9, 33), (2, 24, 40), (1, 4, 32), (3, 40, 40)]


def inputs(cin, cout, N, H, W):
    g = torch.Generator().manual_seed(cin * 7 + cout + N * 1000 + H * 31 + W)
    x = torch.randn(N, H, W, cin, generator=g).half()
    dy = torch.randn(N, H, W, cout, generator=g).half()
    raw = (torch.randn(N, H, W, cout, generator=g) * 1.5 + 0.2).half()
    coef = torch.cat([torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3, torch.randn(cout, generator=g) * 0.2,
                      torch.rand(cout, generator=g) + 0.5])
    sums = torch.randn(2, cout, generator=g).double() * (N * H * W) ** 0.5  # sums of g and g * xhat over the pixels
    return x, dy, raw, coef, sums


def main(out):
    from ultralytics.hip import DY_BN_COPIES
    from ultralytics.hip.engine import Engine
    eng = Engine("cuda:0")
    L = eng.L
    res = {}
    for cin, cout in BLOCKS:
        for N, H, W in SHAPES:
            key = f"{cin}_{cout}_{N}x{H}x{W}"
            x, dy, raw, coef, sums = [t.cuda().contiguous() for t in inputs(cin, cout, N, H, W)]
            buf = C.create_string_buffer(128)
            assert L.dy_wgrad_kernel_name_at(N, H, W, cin, cout, 3, 1, buf, 128) == 0
            res[key + "/name"] = buf.value.decode()
            ns, se = C.c_int(0), C.c_long(0)
            assert L.dy_wgrad_workspace(N, H, W, cin, cout, 3, 1, C.byref(ns), C.byref(se)) == 0
            acc = torch.zeros(DY_BN_COPIES, 2, cout, dtype=torch.float64, device="cuda")
            acc[0] = sums
            for form in ("plain", "bn", "bias"):
                slabs = torch.full((ns.value * se.value,), float("nan"), device="cuda")
                dw = torch.zeros(cout, cin, 3, 3, device="cuda")
                tail = (N, H, W, cin, cout, 3, 1, 0)
                if form == "plain":
                    eng.call("dy_conv_wgrad", x.data_ptr(), cin, dy.data_ptr(), cout, slabs.data_ptr(), dw.data_ptr(), *tail)
                elif form == "bn":
                    draw = torch.full_like(raw, float("nan"))
                    dg, db = torch.zeros(cout, device="cuda"), torch.zeros(cout, device="cuda")
                    eng.call("dy_conv_wgrad_bn", x.data_ptr(), cin, dy.data_ptr(), cout, raw.data_ptr(), cout, draw.data_ptr(), coef.data_ptr(),
                             acc.data_ptr(), dg.data_ptr(), db.data_ptr(), float(N * H * W), slabs.data_ptr(), dw.data_ptr(), *tail)
                    res[f"{key}/bn/draw"], res[f"{key}/bn/dgamma"], res[f"{key}/bn/dbeta"] = draw, dg, db
                else:
                    bacc = torch.zeros(DY_BN_COPIES, cout, dtype=torch.float64, device="cuda")
                    eng.call("dy_conv_wgrad_bias", x.data_ptr(), cin, dy.data_ptr(), cout, bacc.data_ptr(), slabs.data_ptr(), dw.data_ptr(), *tail)
                    res[f"{key}/bias/sum"] = bacc.sum(0)
                res[f"{key}/{form}/slabs"], res[f"{key}/{form}/dw"] = slabs, dw
    torch.cuda.synchronize()
    torch.save({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in res.items()}, out)


if __name__ == "__main__":
    main(sys.argv[1])
