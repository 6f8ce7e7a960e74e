"""Runs the three stem launches (csrc/stem.hip: dy_stem_forward, dy_stem_forward_eval, dy_stem_wgrad_bn) on seeded inputs and saves what
they wrote: tests/test_gpu_stem_pipeline.py compares the files of two processes, one started with DY_STEM_V1=1 (the plain kernels) and one
without it (the pipelined kernels with the aligned staging wherever the width allows it).
usage: stem_pipeline_worker.py <out.pt>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "experiment-yolo_amd")
sys.path[:0] = [ROOT, PKG, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

# (N, H, W, mul): Ho 17 / Wo 35 = partial tiles both ways and W % 4 != 0 (the old load loop); the aligned path with a partial last
# tile; the smallest legal input; 2,400 tiles against the forward grid of 2,048 and the weight-gradient grid of 1,024 (a second and a
# third tile per workgroup: the persistent loop and the prefetch); uint8-valued pixels scaled by 1 / 255
CASES = [(2, 34, 70, 1.0), (2, 36, 72, 1.0), (1, 2, 2, 1.0), (6, 640, 640, 1.0), (2, 36, 72, 1.0 / 255)]


def inputs(N, H, W, mul):
    """The same tensors in the workers and in the test: image, weight, bias, output gradient, BatchNorm affine."""
    g = torch.Generator().manual_seed(N * 1000 + H * 7 + W + (1 if mul != 1.0 else 0))
    img = torch.rand(N, 3, H, W, generator=g)
    if mul != 1.0:
        img = (img * 255).round()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w = (torch.randn(16, 3, 3, 3, generator=g) / 27 ** 0.5).half().float()
    bias = torch.randn(16, generator=g) * 0.2
    dy = torch.randn(N, Ho, Wo, 16, generator=g).half()
    gamma, beta = torch.rand(16, generator=g) + 0.5, torch.randn(16, generator=g) * 0.2
    return img, w, bias, dy, gamma, beta


def main(out):
    from ultralytics.hip import DY_BN_COPIES
    from ultralytics.hip.engine import Engine
    eng = Engine("cuda:0")
    res = {}
    for N, H, W, mul in CASES:
        key = f"{N}x{H}x{W}_{'255' if mul != 1.0 else '1'}"
        img, w, bias, dy, gamma, beta = [t.cuda().contiguous() for t in inputs(N, H, W, mul)]
        Ho, Wo = dy.shape[1:3]
        npix = N * Ho * Wo
        res[key + "/pipelined"] = eng.L.dy_stem_pipelined(img.data_ptr(), W)
        raw = torch.zeros(N, Ho, Wo, 16, dtype=torch.float16, device="cuda")
        af = torch.zeros(DY_BN_COPIES * 2 * 16, dtype=torch.float64, device="cuda")
        eng.call("dy_stem_forward", img.data_ptr(), w.data_ptr(), raw.data_ptr(), 16, af.data_ptr(), N, H, W, mul)
        acc = af.clone()  # the fp64 statistic accumulator after a zeroed start
        y_fused, y_plain = torch.zeros_like(raw), torch.zeros_like(raw)
        eng.call("dy_stem_forward_eval", img.data_ptr(), w.data_ptr(), bias.data_ptr(), y_fused.data_ptr(), 16, N, H, W, mul, 1)
        eng.call("dy_stem_forward_eval", img.data_ptr(), w.data_ptr(), 0, y_plain.data_ptr(), 16, N, H, W, mul, 0)
        # BatchNorm forward (coefficients) and the first backward pass (sums of g, g * xhat): the same launches in both processes
        y = torch.zeros_like(raw)
        rm, rv, coef = torch.zeros(16, device="cuda"), torch.ones(16, device="cuda"), torch.zeros(64, device="cuda")
        ab = torch.zeros_like(af)
        eng.call("dy_bn_act_apply_acc", raw.data_ptr(), 16, 0, 0, y.data_ptr(), 16, af.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                 rm.data_ptr(), rv.data_ptr(), coef.data_ptr(), npix, 16, 1, float(npix), 1e-3, 0.03)
        eng.call("dy_bn_act_bwd_reduce_acc", dy.data_ptr(), 16, raw.data_ptr(), 16, coef.data_ptr(), ab.data_ptr(), npix, 16, 1, 0, 0, 0)
        ns = eng.L.dy_stem_grid(N, H, W)
        slabs = torch.zeros(ns, 9, 16, 16, device="cuda")  # the kernel writes cin 0..2 only
        dg, db = torch.zeros(16, device="cuda"), torch.zeros(16, device="cuda")
        eng.call("dy_stem_wgrad_bn", img.data_ptr(), dy.data_ptr(), 16, raw.data_ptr(), 16, coef.data_ptr(), ab.data_ptr(), dg.data_ptr(),
                 db.data_ptr(), float(npix), slabs.data_ptr(), N, H, W, mul)
        torch.cuda.synchronize()
        for name, t in (("raw", raw), ("acc", acc), ("y_fused", y_fused), ("y_plain", y_plain), ("slabs", slabs), ("dgamma", dg), ("dbeta", db),
                        ("coef", coef)):
            res[f"{key}/{name}"] = t.cpu()
    torch.save(res, out)


if __name__ == "__main__":
    main(sys.argv[1])
