"""The input-gradient-only form of the fused 1x1 backward (csrc/conv_wgrad.hip, BNF 13 / 15, dy_conv1x1_dgrad_bn: what a FROZEN
1x1 Conv + BatchNorm + SiLU runs when its input needs a gradient) against the fused weight + input gradient launch (BNF 5 / 7) on the
same operands, and against an fp32 reference."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from gpu_util import relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def outs(tmp_path_factory):
    """tests/dgrad_only_worker.py in a fresh process with a time limit of its own (DY_WGRAD_SPLIT=0: see the worker)."""
    f = tmp_path_factory.mktemp("dgrad_only") / "dgrad_only.pt"
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "dgrad_only_worker.py"), str(f)],
                       env=dict(os.environ, DY_WGRAD_SPLIT="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(f)


def test_input_gradient_alone_gives_the_bits_of_the_fused_launch(outs):
    """dX -- stored, accumulated onto non-zero old values, every member of a segmented target (store and add side by side, an
    up-sampled member, 16-channel members), dY in one tensor and in two planes, a ragged pixel count, batch 1, a map large enough for
    the persistent loop -- must be EQUAL to the dX of the BNF 5 / 7 launch; the stride padding behind a member keeps its old values.
    X is absent: dy_conv1x1_dgrad_bn takes no X argument and the kernel runs with a null X pointer."""
    res, parts = outs["res"], outs["parts"]
    n = 0
    for k, a in res.items():
        if "/fused/" not in k:
            continue
        b = res[k.replace("/fused/", "/only/")]
        assert torch.isfinite(a.float()).all() and float(a.float().abs().max()) > 0, k
        assert torch.equal(a, b), f"{k}: max diff {float((a.float() - b.float()).abs().max()):.3e} ({outs['names'][k.split('/')[0]]})"
        case, i = k.split("/")[0], int(k.rsplit("dx", 1)[1])
        c = parts[case][i]
        old = res[k.replace("/fused/dx", "/old")]
        assert torch.equal(b[..., c:], old[..., c:]), f"{k}: the padding behind the member's channels was written"
        assert not torch.equal(b[..., :c], old[..., :c]), k
        n += 1
    print(n, sorted(set(outs["names"].values())))
    cases = {k.split("/")[0] for k in res if not k.startswith("oracle/")}
    for need in ("16_16", "32_32", "64_64", "64_32", "128_64", "128_32", "64_48", "3x16_32", "64up+32_64", "planes_64_64", "planes_2x32_64",
                 "ragged_32_32", "ragged_planes_64_64", "ragged_2x32_32", "batch1_64_64", "loop_16_16"):
        assert need in cases, need
    for case in cases:
        if len(parts[case]) == 1 and not case.startswith("loop"):
            assert f"{case}/store/only/dx0" in res and f"{case}/accumulate/only/dx0" in res, case
    assert n >= 32, n
    kinds = {v.rsplit(", ", 1)[1] for v in outs["names"].values()}
    assert kinds == {"13>", "15>"}, kinds  # both the plain and the segmented instantiation ran


@pytest.mark.parametrize("case", ["64_64", "128_32", "64_48"])
def test_input_gradient_alone_against_fp32(outs, case):
    """The formula and the bound of tests/test_gpu_wgrad_dgrad.py::test_fused_input_gradient_against_fp32: d(raw) rebuilt in fp32
    (dx = sc*g - (kb*x + kc), g = dy * silu'(sc*x + sh)), rounded to fp16 as the kernel stages it, times W in fp32; 2e-3."""
    o = outs["res"][f"oracle/{case}"]
    dy, raw, coef, acc, w = o["dy"].float(), o["raw"].float(), o["coef"], o["acc"], o["w"]
    cout, cin = w.shape[:2]
    npix = float(dy.numel() // cout)
    sc, sh, mean, inv = coef.view(4, cout)
    s = acc.sum(0)
    mg, mgx = (s[0] / npix).float(), (s[1] / npix).float()
    kb = sc * inv * mgx
    kc = sc * mg - kb * mean
    z = raw * sc + sh
    sig = torch.sigmoid(z)
    g = dy * (sig + z * sig * (1 - sig))
    draw = (sc * g - (kb * raw + kc)).half().float()
    ref = F.conv_transpose2d(draw.permute(0, 3, 1, 2), w.half().float())
    got = outs["res"][f"{case}/store/only/dx0"][..., :cin].float().permute(0, 3, 1, 2)
    e = relerr(got, ref)
    print(f"{case}: dX of the input-gradient-only launch against fp32 {e:.3e}")
    assert e < 2e-3
