"""The streaming 1x1 convolution kernel (csrc/conv1x1_stream.hip) against the ping-pong kernel's 1x1 branch it replaces on the training
step, and against fp32 F.conv2d."""
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
    """tests/stream1x1_worker.py under DY_CONV1X1_STREAM=0 and =force (the switch is read once per process)."""
    d = tmp_path_factory.mktemp("stream1x1")
    got = {}
    for mode in ("0", "force"):
        f = d / f"stream_{mode}.pt"
        env = dict(os.environ, DY_CONV1X1_STREAM=mode)
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "stream1x1_worker.py"), str(f)], env=env,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        got[mode] = torch.load(f)
    return got


def test_stream_kernel_gives_the_bits_of_the_ping_pong_kernel(outs):
    """Same MFMA, same GEMM orientation, same k order: every convolution output -- plain store, accumulate onto non-zero old values,
    the tensor stored beside the statistics, segmented inputs (16- / 32- / 64-channel members, one up-sampled), segmented outputs that
    mix store and accumulate, pixel strides larger than the channel count, ragged pixel counts, padded cout groups -- must be EQUAL to
    the ping-pong kernel's; the BatchNorm sums to 1e-6 relative (and, because the launches with sums keep the ping-pong kernel's pixel map, to fp64 noise).  Only cases
    the stream kernel really ran (dy_conv1x1_kernel_name_live under force) count, and there must be at least 40 of them."""
    a_all, b_all = outs["0"], outs["force"]
    assert a_all["pairs"] == b_all["pairs"] and len(a_all["pairs"]) >= 8, a_all["pairs"]
    assert a_all["res"].keys() == b_all["res"].keys()
    compared, pairs_hit = 0, set()
    for k, a in a_all["res"].items():
        if k.startswith("oracle/"):
            continue
        b = b_all["res"][k]
        assert not a_all["live"][k].startswith("conv1x1_stream_kernel"), (k, a_all["live"][k])
        ran_stream = b_all["live"][k].startswith("conv1x1_stream_kernel<")
        assert torch.isfinite(a.float()).all() and float(a.float().abs().max()) > 0, k
        assert torch.isfinite(b.float()).all() and float(b.float().abs().max()) > 0, k
        if k.endswith("stats_acc"):
            e = relerr(b, a)
            assert e < 1e-6, f"{k}: {e:.3e}"
            # launches with sums run on the ping-pong kernel's pixel map and reduce as it does: each workgroup adds the same fp32 partial
            # sums, so only the order of the fp64 atomic adds is left (2^-53 per add); a training run then keeps its trajectory
            if ran_stream:
                assert e < 1e-12, f"{k}: {e:.3e} -- the statistics no longer have the ping-pong kernel's fp32 partial sums"
        else:
            assert torch.equal(a, b), f"{k}: max diff {float((a.float() - b.float()).abs().max()):.3e} ({b_all['live'][k]})"
        if ran_stream:
            compared += 1
            if k[0].isdigit():
                pairs_hit.add(k.split("_")[0] + "_" + k.split("_")[1])
    print(f"{compared} cases ran the stream kernel, {len(pairs_hit)} model (cin, cout) pairs among them: {sorted(pairs_hit)}")
    assert compared >= 40, compared
    for fam in ("segx_", "segy_", "/accum", "/stats_acc", "_up"):
        assert any(fam in k and b_all["live"][k].startswith("conv1x1_stream_kernel<") for k in b_all["res"] if not k.startswith("oracle/")), fam
    assert any("_48_" in k and b_all["live"][k].startswith("conv1x1_stream_kernel<") for k in b_all["res"] if not k.startswith("oracle/")), \
        "no padded cout group among the cases the stream kernel ran"
    # the steady state (a wave walks several tiles): plain, accumulate, statistics, one and two cout groups, 64- and 32-pixel wave tiles,
    # segmented outputs -- compared through position-weighted sums of the bit patterns
    big = [k for k in b_all["res"] if k.startswith("big_") and b_all["live"][k].startswith("conv1x1_stream_kernel<")]
    for need in ("big_64_64_", "big_128_64_", "big_64_128_", "big_segy_"):
        assert any(k.startswith(need) for k in big), need
    assert sum(k.endswith("/accum") for k in big) >= 3 and sum(k.endswith("/plain") for k in big) >= 3, big


@pytest.mark.parametrize("cin,cout", [(64, 64), (128, 64), (32, 48)])
def test_stream_kernel_against_fp32_conv2d(outs, cin, cout):
    """Not a self-comparison: three shapes of the forced run against fp32 F.conv2d on the same fp16 inputs, at the bounds of
    test_conv_forward_dgrad_wgrad -- 2e-3 for the fp16 output, 5e-4 for the BatchNorm sums."""
    r, live = outs["force"]["res"], outs["force"]["live"]
    key = f"{cin}_{cout}_3x40x40"
    assert live[key + "/plain"].startswith("conv1x1_stream_kernel<"), live[key + "/plain"]
    x, w = r[f"oracle/{cin}_{cout}/x"].float(), r[f"oracle/{cin}_{cout}/w"].float().cpu()
    ref = F.conv2d(x.permute(0, 3, 1, 2), w.half().float())
    e = relerr(r[key + "/plain"].float().permute(0, 3, 1, 2), ref)
    print(f"{key}: fp16 output {e:.3e}")
    assert e < 2e-3
    e = relerr(r[key + "/stats_y"].float().permute(0, 3, 1, 2), ref)
    assert e < 2e-3
    e1 = relerr(r[key + "/stats_acc"][0], ref.sum((0, 2, 3)))
    e2 = relerr(r[key + "/stats_acc"][1], (ref * ref).sum((0, 2, 3)))
    print(f"{key}: sums {e1:.3e} {e2:.3e}")
    assert e1 < 5e-4 and e2 < 5e-4
