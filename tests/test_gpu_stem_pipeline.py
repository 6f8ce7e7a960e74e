"""The pipelined stem kernels (csrc/stem.hip: next tile's patch prefetched into registers, aligned 16-byte image loads, the weight
gradient's patch staged per kx) against the plain kernels that DY_STEM_V1=1 still launches: the same bits everywhere, and both inside
the stem's bound against a float64 convolution."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from gpu_util import relerr
from stem_pipeline_worker import CASES, inputs

pytestmark = pytest.mark.gpu


def key_of(N, H, W, mul):
    return f"{N}x{H}x{W}_{'255' if mul != 1.0 else '1'}"


@pytest.fixture(scope="module")
def outs(tmp_path_factory):
    """tests/stem_pipeline_worker.py in a process of its own per switch setting."""
    d = tmp_path_factory.mktemp("stem_pipeline")
    got = {}
    for mode in ("old", "new"):
        f = d / f"stem_{mode}.pt"
        env = dict(os.environ)
        env.pop("DY_STEM_V1", None)
        if mode == "old":
            env["DY_STEM_V1"] = "1"
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "stem_pipeline_worker.py"), str(f)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        got[mode] = torch.load(f)
    return got


@pytest.mark.parametrize("N,H,W,mul", CASES)
def test_the_switch_selects_the_kernels(outs, N, H, W, mul):
    """DY_STEM_V1=1 launches the plain kernels at every width; without it the pipelined ones run exactly where W % 4 == 0."""
    k = key_of(N, H, W, mul)
    assert outs["old"][k + "/pipelined"] == 0
    assert outs["new"][k + "/pipelined"] == (1 if W % 4 == 0 else 0)


@pytest.mark.parametrize("N,H,W,mul", CASES)
def test_pipelined_stem_gives_the_bits_of_the_plain_kernels(outs, N, H, W, mul):
    """Same tiles, same LDS values, same MFMAs in the same order: raw, the eval outputs (fused bias + SiLU and plain), the fp64 statistic
    accumulator after a zeroed start, the weight-gradient slabs, dgamma and dbeta are EQUAL."""
    k = key_of(N, H, W, mul)
    for name in ("raw", "y_fused", "y_plain", "acc", "coef", "slabs", "dgamma", "dbeta"):
        a, b = outs["old"][f"{k}/{name}"], outs["new"][f"{k}/{name}"]
        assert bool(torch.isfinite(a.double()).all()), name
        assert torch.equal(a, b), (name, int((a != b).sum()))
    assert float(outs["new"][k + "/raw"].float().abs().max()) > 0 and float(outs["new"][k + "/slabs"].abs().max()) > 0


@pytest.mark.parametrize("N,H,W,mul", CASES)
def test_stem_against_float64(outs, N, H, W, mul):
    """Both forms against F.conv2d in float64 on the fp16-rounded img * mul, with the stem's bound of tests/test_gpu_kernels.py (1e-3 of
    the largest output: fp16 storage of the output is 4.9e-4)."""
    img, w, bias, _dy, _gamma, _beta = inputs(N, H, W, mul)
    x = (img * torch.tensor(mul, dtype=torch.float32)).half().double()
    ref = F.conv2d(x, w.double(), None, 2, 1).permute(0, 2, 3, 1)
    k = key_of(N, H, W, mul)
    for mode in ("old", "new"):
        assert relerr(outs[mode][k + "/raw"], ref) < 1e-3, mode
        assert relerr(outs[mode][k + "/y_plain"], ref) < 1e-3, mode
        assert relerr(outs[mode][k + "/y_fused"], F.silu(ref + bias.double())) < 1e-3, mode
