"""The fused 1x1 backward (csrc/conv_wgrad.hip, BNF 5 / 7: weight gradient and input gradient in one launch, d(raw) never leaves LDS)
against the two-launch form it replaces on the training step, and against an fp32 reference."""
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
    """tests/wgrad_dgrad_worker.py under DY_WGRAD_DGRAD=0 and =1, a fresh process each."""
    d = tmp_path_factory.mktemp("wgrad_dgrad")
    got = {}
    for mode in ("0", "1"):
        f = d / f"wgrad_dgrad_{mode}.pt"
        env = dict(os.environ, DY_WGRAD_DGRAD=mode)
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "wgrad_dgrad_worker.py"), str(f)], env=env,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        got[mode] = torch.load(f)
    assert got["0"]["fused"] is False and got["1"]["fused"] is True
    return got


def test_fused_backward_gives_the_bits_of_the_two_launch_form(outs):
    """dX -- stored, accumulated onto non-zero old values, and every member of a segmented target (store and accumulate side by side,
    an up-sampled member, 16-channel members, the padding behind a member's channels untouched) -- the reduced dW, dgamma and dbeta
    must be EQUAL to what dy_conv_wgrad_bn / _segs / _planes followed by the input-gradient launch give: the step's shapes, ragged
    pixel counts, batch 1, Cout 16 and 48, dY in one tensor and in two planes."""
    a_all, b_all = outs["0"]["res"], outs["1"]["res"]
    assert a_all.keys() == b_all.keys()
    n = {"dx": 0, "dw": 0, "dgamma": 0, "dbeta": 0}
    for k, a in a_all.items():
        if k.startswith("oracle/"):
            continue
        b = b_all[k]
        assert torch.isfinite(a.float()).all() and float(a.float().abs().max()) > 0, k
        assert torch.equal(a, b), f"{k}: max diff {float((a.float() - b.float()).abs().max()):.3e} ({outs['1']['names'][k.split('/')[0]]})"
        kind = k.rsplit("/", 1)[1]
        n["dx" if kind.startswith("dx") else kind] += 1
    print(n, sorted(set(outs["1"]["names"].values())))
    assert n["dx"] >= 36 and n["dw"] == n["dgamma"] == n["dbeta"] >= 29, n
    cases = {k.split("/")[0] for k in a_all if not k.startswith("oracle/")}
    for need in ("32_32@160", "64_64@80", "64_32@80", "128_64@40", "128_32@40", "3x16_32@160", "3x32_64@80", "64up+32_64@80", "planes_64_64@80",
                 "planes_2x32_64@80", "ragged_32_32", "ragged_planes_64_64", "ragged_2x32_32", "batch1_64_64@200", "16_16@160", "32_16@160",
                 "64_48@80", "96_48@80"):
        assert need in cases, need
    for case in cases:
        if "x" in case.split("_")[0] or "+" in case or "2x32" in case:
            continue
        assert f"{case}/store/dx0" in a_all and f"{case}/accumulate/dx0" in a_all, case
    # both segmented and plain instantiations ran
    kinds = {v.rsplit(", ", 1)[1] for v in outs["1"]["names"].values()}
    assert kinds == {"5>", "7>"}, kinds


@pytest.mark.parametrize("case", ["64_64@80", "128_32@40", "64_48@80"])
def test_fused_input_gradient_against_fp32(outs, case):
    """Not a self-comparison: d(raw) rebuilt in fp32 from the kernel's formula (dx = sc*g - (kb*x + kc), g = dy * silu'(sc*x + sh)), rounded
    to fp16 as the kernel stages it, times W in fp32 (conv_transpose2d of a 1x1 kernel) -- at the 2e-3 bound tests/test_gpu_conv1x1_stream.py
    applies to the fp16 output of the input-gradient launch.  The two-launch form's d(raw) is checked against the same formula."""
    o = outs["1"]["res"][f"oracle/{case}"]
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
    two = outs["0"]["res"][f"oracle/{case}"]["draw"].float()
    e0 = relerr(two, draw)
    ref = F.conv_transpose2d(draw.permute(0, 3, 1, 2), w.half().float())
    got = outs["1"]["res"][f"{case}/store/dx0"][..., :cin].float().permute(0, 3, 1, 2)
    e = relerr(got, ref)
    print(f"{case}: d(raw) of the two-launch form {e0:.3e}, fused dX {e:.3e}")
    assert e0 < 2e-3
    assert e < 2e-3
    # dbeta / dgamma are the sums themselves
    assert relerr(outs["1"]["res"][f"{case}/store/dbeta"], s[0].float()) < 1e-6
    assert relerr(outs["1"]["res"][f"{case}/store/dgamma"], s[1].float()) < 1e-6
