"""The eight-wave form of the weight gradient's wide 3x3 blocks (csrc/conv_wgrad.hip: 64 x 64 channels per workgroup, the 36
(ci tile, tap) columns dealt to eight waves instead of four) against the four-wave form: the same bits, and both inside the suite's
weight-gradient tolerance against float64."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from gpu_util import relerr
from wgrad_wide_worker import BLOCKS, SHAPES, inputs

pytestmark = pytest.mark.gpu
CASES = [(cin, cout, *shape) for cin, cout in BLOCKS for shape in SHAPES]


@pytest.fixture(scope="module")
def outs(tmp_path_factory):
    """tests/wgrad_wide_worker.py under DY_WGRAD_WIDE=0 and =1, both with DY_WGRAD_SPLIT=0 (read once per process)."""
    d = tmp_path_factory.mktemp("wgrad_wide")
    got = {}
    for wide in ("0", "1"):
        f = d / f"wide_{wide}.pt"
        env = dict(os.environ, DY_WGRAD_WIDE=wide, DY_WGRAD_SPLIT="0")
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "wgrad_wide_worker.py"), str(f)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        got[wide] = torch.load(f)
    return got


@pytest.mark.parametrize("cin,cout,N,H,W", CASES)
def test_the_wide_block_is_what_runs_and_the_name_says_which_form(outs, cin, cout, N, H, W):
    """Every case launches the (4, 4) block of 3x3 stride 1, and dy_wgrad_kernel_name_at names two different kernels for the two forms:
    the default one as before, the other with 16 added to the last template argument."""
    k = f"{cin}_{cout}_{N}x{H}x{W}/name"
    names = {outs["0"][k], outs["1"][k]}
    assert names == {"conv_wgrad_kernel<3, 1, 4, 4, 0>", "conv_wgrad_kernel<3, 1, 4, 4, 16>"}, names


@pytest.mark.parametrize("cin,cout,N,H,W", CASES)
def test_eight_waves_give_the_bits_of_four(outs, cin, cout, N, H, W):
    """Every accumulator is fed by the same k-steps of the same tiles in the same order: slabs and reduced dW of all three entry points,
    d(raw), dgamma and dbeta are EQUAL.  The bias sums are fp32 per thread over other granules with 512 threads, then fp64: at most
    4,800 fp32 additions per channel, each off by at most 2^-25 of a partial sum below ~50, is 7e-3 absolute in the worst case against
    column sums whose largest is ~170 (sqrt(4,800) x 2.5): 4e-5, rounded up to 1e-4."""
    k = f"{cin}_{cout}_{N}x{H}x{W}"
    for name in ("plain/slabs", "plain/dw", "bn/slabs", "bn/dw", "bn/draw", "bn/dgamma", "bn/dbeta", "bias/slabs", "bias/dw"):
        a, b = outs["0"][f"{k}/{name}"], outs["1"][f"{k}/{name}"]
        assert bool(torch.isfinite(a.double()).all()), name
        assert torch.equal(a, b), (name, int((a != b).sum()))
    assert relerr(outs["1"][k + "/bias/sum"], outs["0"][k + "/bias/sum"]) < 1e-4
    assert float(outs["1"][k + "/bn/draw"].float().abs().max()) > 0


@pytest.mark.parametrize("cin,cout,N,H,W", CASES)
def test_wide_weight_gradient_against_float64(outs, cin, cout, N, H, W):
    """dW of dy_conv_wgrad (and of dy_conv_wgrad_bias, with its bias sums) against autograd in float64; 3e-4 is the weight-gradient bound
    of tests/test_gpu_kernels.py."""
    x, dy, _raw, _coef, _sums = inputs(cin, cout, N, H, W)
    xd, dyd = x.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2)
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xd, w, None, 1, 1).backward(dyd)
    k = f"{cin}_{cout}_{N}x{H}x{W}"
    for wide in ("0", "1"):
        assert relerr(outs[wide][k + "/plain/dw"], w.grad) < 3e-4, wide
        assert relerr(outs[wide][k + "/bias/dw"], w.grad) < 3e-4, wide
        assert relerr(outs[wide][k + "/bias/sum"], dyd.sum((0, 2, 3))) < 1e-4, wide
