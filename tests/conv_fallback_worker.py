"""Runs convolution cases of tests/conv_ref.py through the C entry points the way tests/test_gpu_kernels.py drives them and returns /
saves what they left, whole buffers with their canary: tests/test_gpu_conv_fallback.py calls ``run`` in its own process, and starts
this file as a worker where a switch that csrc/conv.hip reads once per process has to differ:
    conv_fallback_worker.py v1 <out.pt>     (under DY_CONV_V1=1)      the FORCED_V1 shapes on conv_mfma_kernel
    conv_fallback_worker.py nodg2 <out.pt>  (under DY_CONV_NO_DG2=1)  the input gradients of the stride-2 cases on their base family"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd"), os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

import conv_ref as R  # noqa: E402
from ultralytics.hip import (DY_BN_COPIES, DY_EPI_ACCUM, DY_EPI_BIAS, DY_EPI_F32OUT, DY_EPI_SILU, DY_EPI_STATS,  # noqa: E402
                             DY_EPI_STATS_ACC)
from ultralytics.hip.engine import ConvSpec, Engine, Storage  # noqa: E402

EPIS = {"y0": 0, "y_stats": DY_EPI_STATS, "y_acc_stats": DY_EPI_STATS | DY_EPI_STATS_ACC, "y_silu": DY_EPI_BIAS | DY_EPI_SILU,
        "y32": DY_EPI_F32OUT | DY_EPI_BIAS, "y16_accum": DY_EPI_ACCUM, "y32_accum": DY_EPI_F32OUT | DY_EPI_ACCUM}


def _name(fn, *a):
    buf = C.create_string_buffer(128)
    rc = fn(*a, buf, 128)
    assert rc == 0, (fn.__name__, a, rc)
    return buf.value.decode()


def kernel_names(L, case, nhw):
    """What the planning helpers say the launches of this case run: forward per epilogue, and the input gradient."""
    N, H, W = nhw
    Ho, Wo = R.out_hw(case, H, W)
    n = {"fwd": _name(L.dy_conv_kernel_name, case.cin, case.cout, case.ks, case.s)}
    for k, e in EPIS.items():
        n[k] = (_name(L.dy_conv1x1_kernel_name_live, case.cin, case.cout, N, H, W, e, None, None) if case.ks == 1 else
                _name(L.dy_conv_kernel_name_at, case.cin, case.cout, case.ks, case.s, Wo, 1, e))
    coutp = R.round8(case.cout)
    n["dgrad"] = _name(L.dy_conv_kernel_name_at, coutp, case.cin, case.ks, 1, W, case.s, 0)
    g = [C.c_int() for _ in range(8)]
    assert L.dy_conv_geometry(coutp, case.cin, case.ks, 1, *[C.byref(v) for v in g]) == 0
    dg2 = R.dg2_takes(case, g[2].value, g[4].value, g[3].value) and not any(os.environ.get(k) for k in ("DY_CONV_NO_DG2", "DY_CONV_V1"))
    n["dgrad_ran"] = f"conv_mfma_dg2_kernel<{g[2].value}, {g[4].value}>" if dg2 else n["dgrad"]
    return n


def _pitched(t, dtype=torch.float16):
    return R.pitched(t, dtype=dtype).cuda()


def _canary(shape, dtype=torch.float16):
    return torch.full(shape, R.CANARY, dtype=dtype, device="cuda")


def _setup(eng, case, nhw, only=None):
    N, H, W = nhw
    d = R.inputs(case, nhw, only)
    sp = ConvSpec("t", d["w"].float().cuda().contiguous(), d["b"].float().cuda(), None, case.ks, case.s, 0)
    sp.gweight = torch.zeros_like(sp.weight)
    sp.gbias = torch.zeros(R.round8(case.cout), device="cuda")
    eng.prepare_conv(sp)
    eng.pack(sp, transposed=True)
    xst = Storage(eng, N, H, W, R.round8(case.cin) + 8)
    xst.buf.copy_(_pitched(d["x"]))
    return d, sp, xst


def run(case, nhw, fwd=True, bwd=True):
    """Every epilogue of the forward, then weight + input gradient stored and accumulated -> {what: CPU tensor}, "names", "unchanged"."""
    assert DY_BN_COPIES == R.BN_COPIES
    eng = Engine("cuda:0")
    N, H, W = nhw
    Ho, Wo = R.out_hw(case, H, W)
    cin, cout, cinp, coutp, ctot = case.cin, case.cout, R.round8(case.cin), R.round8(case.cout), R.round16(case.cout)
    d, sp, xst = _setup(eng, case, nhw)
    xa = xst.act(0, cin)
    x0, w0, b0 = xst.buf.clone(), sp.weight.clone(), sp.bias.clone()
    res = {"names": kernel_names(eng.L, case, nhw)}
    ld = coutp + 8
    if fwd:
        nparts = eng.L.dy_conv_num_partials(N, H, W, cinp, cout, case.ks, case.s, 1)
        part = _canary((nparts + 2, 2, ctot), torch.float32)
        acc = torch.zeros(DY_BN_COPIES, 2, ctot, dtype=torch.float64, device="cuda")
        bufs = {k: _canary((N, Ho, Wo, ld), torch.float32 if e & DY_EPI_F32OUT else torch.float16) for k, e in EPIS.items()}
        bufs["y16_accum"] = _pitched(d["old16"])
        bufs["y32_accum"] = _pitched(d["old32"], torch.float32)
        told = C.c_int(-1)
        for k, e in EPIS.items():
            if k == "y32":  # Detect's final convolution, as the engine launches it
                eng.conv_bias(sp, xa, bufs[k].data_ptr(), ld, True)
                continue
            p = part.data_ptr() if k == "y_stats" else (acc.data_ptr() if k == "y_acc_stats" else 0)
            eng.call("dy_conv_forward", xa.ptr, xa.ld, sp.wpack.data_ptr(), sp.bias.data_ptr() if e & DY_EPI_BIAS else 0, bufs[k].data_ptr(), ld,
                     p, N, H, W, cinp, cout, case.ks, case.s, 1, 0, 0, e, C.byref(told) if k == "y_stats" else None)
        torch.cuda.synchronize()
        assert told.value == nparts, f"dy_conv_forward reports {told.value} partial rows, dy_conv_num_partials {nparts}"
        res.update({k: v.cpu() for k, v in bufs.items()}, part=part.cpu(), acc=acc.cpu(), nparts=nparts)
    unchanged = True
    if bwd:
        dyst = Storage(eng, N, Ho, Wo, ld)
        dyst.buf.copy_(_pitched(d["dy"]))
        dy0 = dyst.buf.clone()
        dya = dyst.act(0, cout)
        xst.gbuf = _canary(tuple(xst.buf.shape))
        xa.needs_grad = cin % 8 == 0  # (the 3-channel image gets no gradient)
        for acc_w, sfx in ((0, ""), (1, "2")):
            eng._conv_bwd(sp, xa, dya.ptr, dya.ld, Ho, Wo, accumulate_w=acc_w)
            torch.cuda.synchronize()
            res["dw" + sfx] = sp.gweight.cpu().clone()
            if xa.needs_grad:
                res["dx" + sfx] = xst.gbuf.cpu().clone()
        unchanged = torch.equal(dyst.buf, dy0)
    torch.cuda.synchronize()
    res["unchanged"] = unchanged and torch.equal(xst.buf, x0) and torch.equal(sp.weight, w0) and torch.equal(sp.bias, b0)
    return res


def run_persistent(case, nhw):
    """DY_EPI_STATS forward of a map of more than 512 tiles -> the stored output (N, Ho, Wo, cout + 8), the partial rows and the input."""
    eng = Engine("cuda:0")
    N, H, W = nhw
    Ho, Wo = R.out_hw(case, H, W)
    d, sp, xst = _setup(eng, case, nhw, only="forward")
    ld, ctot = case.cout + 8, R.round16(case.cout)
    nparts = eng.L.dy_conv_num_partials(N, H, W, case.cin, case.cout, case.ks, case.s, 1)
    part = _canary((nparts + 2, 2, ctot), torch.float32)
    y = _canary((N, Ho, Wo, ld))
    eng.call("dy_conv_forward", xst.buf.data_ptr(), xst.C, sp.wpack.data_ptr(), 0, y.data_ptr(), ld, part.data_ptr(), N, H, W, case.cin, case.cout,
             case.ks, case.s, 1, 0, 0, DY_EPI_STATS, None)
    torch.cuda.synchronize()
    return dict(y=y.cpu(), part=part.cpu(), nparts=nparts, x=d["x"], w=d["w"], names=kernel_names(eng.L, case, nhw))


def main(mode, out):
    res = {}
    if mode == "v1":
        assert os.environ.get("DY_CONV_V1")
        for case in R.FORCED_V1:
            res[case.id] = run(case, case.maps[0])
    elif mode == "nodg2":
        assert os.environ.get("DY_CONV_NO_DG2")
        for case in R.CASES:
            if case.s == 2:
                for nhw in case.maps:
                    res[f"{case.id}/{nhw}"] = run(case, nhw, fwd=False)
    else:
        raise SystemExit(f"unknown mode {mode}")
    torch.save(res, out)


if __name__ == "__main__":
    main(*sys.argv[1:3])
