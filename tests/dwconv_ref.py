"""Float64 reference of the depthwise convolution kernels (csrc/dwconv.hip): forward, input gradient and weight gradient through
``torch.nn.functional.conv2d(groups=c1)`` and ``torch.nn.grad`` in float64, on the fp16 activations and fp32 weights the kernels
see, NHWC in and out.  Every function also returns ``mag``, the sum of the absolute values of the terms of each element: what the
per-element bound  |got - ref| <= k16 2^-11 |ref| + k32 2^-23 mag + 2^-24  of tests/test_gpu_dwconv.py scales its fp32 part by.
tests/test_host_dwconv.py ties these to autograd at 1e-11 and runs an fp32 emulation of the kernels' summation orders against the
bounds."""
import numpy as np
import torch
import torch.nn.functional as F


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def out_hw(H, W, k, s):
    p = k // 2
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def forward(x, w, s):
    """x (N,H,W,C1) fp16, w (C2,1,k,k) fp32 -> dict(y, mag) float64 (N,Ho,Wo,C2)."""
    k, c1 = w.shape[-1], x.shape[-1]
    xd, wd = nchw(x.double()), w.double()
    return dict(y=nhwc(F.conv2d(xd, wd, None, s, k // 2, 1, c1)), mag=nhwc(F.conv2d(xd.abs(), wd.abs(), None, s, k // 2, 1, c1)))


def input_grad(dy, w, s, H, W, m):
    """dy (N,Ho,Wo,C2) fp16, channel multiplier m (c1 = c2 / m) -> dict(dx, mag) float64 (N,H,W,C1)."""
    k, c1 = w.shape[-1], w.shape[0] // m
    shape = (dy.shape[0], c1, H, W)
    g, wd = nchw(dy.double()), w.double()
    return dict(dx=nhwc(torch.nn.grad.conv2d_input(shape, wd, g, s, k // 2, 1, c1)),
                mag=nhwc(torch.nn.grad.conv2d_input(shape, wd.abs(), g.abs(), s, k // 2, 1, c1)))


def weight_grad(x, dy, k, s):
    """-> dict(dw, mag) float64 (C2,1,k,k)."""
    c1, c2 = x.shape[-1], dy.shape[-1]
    xd, g = nchw(x.double()), nchw(dy.double())
    shape = (c2, 1, k, k)
    return dict(dw=torch.nn.grad.conv2d_weight(xd, shape, g, s, k // 2, 1, c1),
                mag=torch.nn.grad.conv2d_weight(xd.abs(), shape, g.abs(), s, k // 2, 1, c1))


def inputs(N, H, W, C1, m, k, s, seed):
    """The seeded operands of a kernel case: x fp16 (N,H,W,C1), w fp32 (C1 m,1,k,k), dy fp16 (N,Ho,Wo,C1 m), bias fp32 (C1 m)."""
    rng = np.random.default_rng(seed)
    Ho, Wo = out_hw(H, W, k, s)
    x = torch.from_numpy(rng.standard_normal((N, H, W, C1)).astype(np.float16))
    w = torch.from_numpy((rng.standard_normal((C1 * m, 1, k, k)) / k).astype(np.float32))
    dy = torch.from_numpy(rng.standard_normal((N, Ho, Wo, C1 * m)).astype(np.float16))
    bias = torch.from_numpy(rng.standard_normal(C1 * m).astype(np.float32))
    return x, w, dy, bias
