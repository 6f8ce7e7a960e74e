"""-m gpu: the fallback convolution kernels of csrc/conv.hip -- conv_mfma_wlds_kernel ("v3") and conv_mfma_kernel ("v1"), which take
every shape whose weights and two tiles do not fit LDS beside the ping-pong kernel -- per element against the float64 reference and the
DERIVED bounds of tests/conv_ref.py (validated without a GPU by tests/test_host_conv_ref.py), through the C entry points as
tests/test_gpu_kernels.py drives them (tests/conv_fallback_worker.py).  Every case asserts the kernel instantiation it means to
run; test_coverage_equals_the_fixture ties the set of v3 / v1 instantiations run here to the one tests/golden/conv_select.json.gz
names, so a change of the selection cannot silently empty the coverage.  Also here: the one-row forms of the ping-pong kernel that
CONV_CASES misses, v3's persistent tile loop (513 tiles), conv_mfma_kernel forced by DY_CONV_V1 (tools/conv_bench.py's A/B
baseline) and three Conv modules at scale-s widths.

Outputs live in canary-filled buffers of pitch round8(cout) + 8: what lies behind the written channels, and every input, must be
bit-unchanged.

How to read a failure: conv_ref.check prints "worst |got - ref| / bound" for every output and, when it raises, the worst element with
every term of its bound.  A ratio a little above 1 with "K 2^-23 S" or "2^-11 |ref|" dominating would be arithmetic (an accumulation
or rounding the derivation did not allow for); a ratio of tens or thousands is a wrong tap, mask, tile or index -- the element's
position (border pixel, last tile row, channel >= 128, second image) says which."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
from gpu_util import relerr, run_fwd_bwd

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ALL = [(c, nhw) for c in R.CASES for nhw in c.maps]
IDS = [f"{c.id}-{'x'.join(map(str, nhw))}" for c, nhw in ALL]
S2 = [(c, nhw) for c, nhw in ALL if c.s == 2]
RATIOS = {}  # (family, output) -> worst ratio seen in this session (printed by the last test: the DESIGN 4.1 table)


def _family(name):
    return "v3" if name.startswith("conv_mfma_wlds") else ("v1" if name.startswith("conv_mfma_kernel") else name.split("_kernel")[0].replace("conv_mfma_", ""))


def _note(log, fwd_name, dgrad_name):
    for what, v in log.items():
        out = what.split(" ", 2)[2]
        fam = _family(dgrad_name if out.startswith("dX") else ("conv_wgrad" if out.startswith("dW") else fwd_name))
        RATIOS[(fam, out)] = max(RATIOS.get((fam, out), 0.0), v)


def _worker(mode, env, tmp_path_factory):
    out = tmp_path_factory.mktemp(mode) / "out.pt"
    e = {k: v for k, v in os.environ.items() if not k.startswith(("DY_CONV", "DY_PP"))}
    r = subprocess.run([sys.executable, os.path.join(HERE, "conv_fallback_worker.py"), mode, str(out)], env=dict(e, **env), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out)


@pytest.fixture(scope="module")
def nodg2(tmp_path_factory):
    return _worker("nodg2", {"DY_CONV_NO_DG2": "1"}, tmp_path_factory)


@pytest.fixture(scope="module")
def forced_v1(tmp_path_factory):
    return _worker("v1", {"DY_CONV_V1": "1"}, tmp_path_factory)


@pytest.mark.parametrize("case,nhw", ALL, ids=IDS)
def test_every_epilogue_and_both_gradients(case, nhw):
    """Plain store, STATS (partial rows and fp64 accumulator), BIAS | SILU, F32OUT | BIAS, ACCUM (fp16 and fp32), then dW and dX stored
    and accumulated, on the instantiation the case names."""
    import conv_fallback_worker as WK
    res = WK.run(case, nhw)
    n = res["names"]
    assert n["fwd"] == case.kernel and all(n[k] == case.kernel for k in WK.EPIS), n
    assert n["dgrad"] == case.dgrad, n
    print(f"{case.id}: forward {n['fwd']}; input gradient {n['dgrad_ran']}")
    log = R.compare(res, case, nhw, fwd_pp=not R.is_fallback(n["fwd"]), dgrad_pp=not R.is_fallback(n["dgrad_ran"]))
    assert len(log) == 15 and res["unchanged"], "an input changed"
    _note(log, n["fwd"], n["dgrad_ran"])


@pytest.mark.parametrize("case,nhw", S2, ids=[i for i, (c, _) in zip(IDS, ALL) if c.s == 2])
def test_stride2_input_gradient_on_the_base_family(case, nhw, nodg2):
    """DY_CONV_NO_DG2=1 (read once per process: a worker): the dil == 2 staging of the base family is what forms dX."""
    res = nodg2[f"{case.id}/{nhw}"]
    assert res["names"]["dgrad_ran"] == res["names"]["dgrad"] == case.dgrad, res["names"]
    print(f"{case.id}: input gradient {case.dgrad} with dil = 2")
    log = R.compare(res, case, nhw)
    assert len(log) == 4 and res["unchanged"]
    _note(log, case.kernel, case.dgrad)


@pytest.mark.parametrize("case", R.FORCED_V1, ids=[c.id for c in R.FORCED_V1])
def test_forced_v1_computes_the_same_convolution(case, forced_v1):
    """DY_CONV_V1=1 puts ping-pong shapes on conv_mfma_kernel; with and without the switch the results sit in the same bounds."""
    import conv_fallback_worker as WK
    nhw = case.maps[0]
    res = forced_v1[case.id]
    assert all(res["names"][k] == case.kernel for k in ("fwd", *WK.EPIS)), res["names"]
    want = 15 if case.cin % 8 == 0 else 13  # (the 3-channel image takes no gradient)
    log = R.compare(res, case, nhw)  # (under the switch the input gradient is a conv_mfma_kernel launch too)
    assert len(log) == want and res["unchanged"] and R.is_fallback(res["names"]["dgrad_ran"])
    _note(log, case.kernel, res["names"]["dgrad_ran"])
    here = WK.run(case, nhw)
    assert all(here["names"][k] == case.pp for k in ("fwd", *WK.EPIS)), here["names"]
    assert len(R.compare(here, case, nhw, fwd_pp=True, dgrad_pp=not R.is_fallback(here["names"]["dgrad_ran"]))) == want and here["unchanged"]


def test_coverage_equals_the_fixture():
    """The v3 / v1 instantiations the cases above assert (forward and input gradient) are exactly those the fixture's run "unset"
    names under name/...: 19 today, plus the three one-row ping-pong forms."""
    from golden.make_conv_select_golden import labels_sha, load, sweep
    gold, _, shas = load()
    pairs = sweep("unset")
    assert labels_sha(pairs) == shas["unset"] and len(pairs) == len(gold["unset"])
    named = {v for (k, _), v in zip(pairs, gold["unset"]) if k.startswith("name/") and isinstance(v, str) and R.is_fallback(v)}
    ran = {n for c in R.CASES for n in (c.kernel, c.dgrad) if R.is_fallback(n)}
    print(f"{len(ran)} v3 / v1 instantiations run, {len(named)} named by the fixture")
    assert ran == named, (sorted(ran - named), sorted(named - ran))
    assert len(named) == 19 and {c.kernel for c in R.FALLBACK_CASES} == named
    assert {c.kernel for c in R.PP_ONE_ROW_CASES} == {R.PP % a for a in ("64, 4, 1, 1, 1", "64, 2, 3, 1, 1", "64, 1, 3, 1, 1")}


def _band(x, w, case, a, b, H):
    """Output rows [a, b) of the float64 convolution and of its absolute-value form, from the input rows they read."""
    s, pad, ks = case.s, case.ks // 2, case.ks
    lo, hi = a * s - pad, (b - 1) * s + pad + 1
    xs = F.pad(x[:, :, max(lo, 0):min(hi, H)], (pad, pad, max(-lo, 0), max(hi - H, 0)))
    return F.conv2d(xs, w, None, s), F.conv2d(xs.abs(), w.abs(), None, s)


@pytest.mark.parametrize("case,nhw,th", R.PERSISTENT, ids=[c.id for c, _, _ in R.PERSISTENT])
def test_v3_persistent_tile_loop(case, nhw, th):
    """513 tiles on 512 workgroups: workgroup 0 runs a second tile, whose first chunk it prefetched during the last k-loop of its first.
    Row bands (first tiles, tiles 511...513, the last rows) against float64; the STATS rows against the sums of the stored output --
    over the whole map, and per workgroup (tiles r and r + 512), which is where sums carried across tiles wrongly would show."""
    import conv_fallback_worker as WK
    N, H, W = nhw
    Ho, Wo = R.out_hw(case, H, W)
    res = WK.run_persistent(case, nhw)
    assert res["names"]["y_stats"] == case.kernel and res["nparts"] == 512 and -(-Ho // th) == 513 and Wo <= 32
    y, cout, K = res["y"], case.cout, case.cin * case.ks ** 2
    R.check_canary(y, cout, f"{case.id} persistent")
    for a, b in ((0, 2 * th), (510 * th, Ho)):
        ref, S = (R.nhwc(t) for t in _band(res["x"], res["w"], case, a, b, H))
        R.check(y[:, a:b, :, :cout], ref, R.b16(ref, R.b32(ref, S, K)), f"{case.id} rows {a}...{b}")
    part, yd = res["part"], y[0, :, :, :cout].double()
    assert bool((part[512:] == R.CANARY).all())
    ps = part[:512].double().sum(0)
    R.check_sums(ps[0, :cout], ps[1, :cout], yd.reshape(-1, cout), f"{case.id} whole map")
    rows = yd[:512 * th].reshape(512, th * Wo, cout)
    extra = yd[512 * th:].reshape(-1, cout)
    P = torch.full((512, 1), float(th * Wo), dtype=torch.float64)
    P[0] += extra.shape[0]
    for which, f in ((0, lambda t: t), (1, lambda t: t * t)):
        ref = f(rows).sum(1)
        mag = f(rows).abs().sum(1)
        ref[0] += f(extra).sum(0)
        mag[0] += f(extra).abs().sum(0)
        R.check(part[:512, which, :cout], ref, {"(P + 1) 2^-23 sum": (P + which) * R.EPS32 * mag, "2^-126": torch.full_like(ref, 2.0 ** -126)},
                f"{case.id} per workgroup sum y{'^2' if which else ''}")


@pytest.mark.parametrize("cin,cout,k,s", [(128, 256, 3, 1), (96, 160, 3, 1), (80, 64, 3, 2)])
def test_conv_modules_at_scale_s_widths(cin, cout, k, s):
    """Conv (conv + BatchNorm + SiLU, training mode) on v1 (128 -> 256), v3 (96 -> 160) and stride-2 v3 (80 -> 64) through the engine
    tape against oracle.nn.conv_bn_silu in float64; TOL["Conv"] of tests/test_gpu_modules.py, running statistics 2e-3."""
    import ctypes as C
    import oracle.nn as onn
    from ultralytics.hip import lib
    from ultralytics.nn.modules import Conv
    L, buf = lib(), C.create_string_buffer(128)
    assert L.dy_conv_kernel_name(cin, cout, k, s, buf, 128) == 0 and R.is_fallback(buf.value.decode()), buf.value
    g = torch.Generator().manual_seed(cin + cout)
    r = lambda *sh: torch.randn(*sh, generator=g)  # noqa: E731
    x = r(2, cin, 12, 20).half().float()
    Ho, Wo = (12 + 2 - 3) // s + 1, (20 + 2 - 3) // s + 1
    gy = r(2, cout, Ho, Wo).half().float()
    sd = {"conv.weight": r(cout, cin, k, k) / (cin * k * k) ** 0.5, "bn.weight": torch.rand(cout, generator=g) + 0.5, "bn.bias": r(cout) * 0.2,
          "bn.running_mean": r(cout) * 0.3, "bn.running_var": torch.rand(cout, generator=g) + 0.5, "bn.num_batches_tracked": torch.tensor(3)}
    m = Conv(cin, cout, k, s)
    m.load_state_dict(sd, strict=True)
    y, gxs, rt = run_fwd_bwd(m, [x], gy)
    # no reduce rides a dgrad epilogue here: the helper refuses the stride-1 shapes in both orientations, and the engine took none
    if s == 1:
        assert L.dy_conv_red_supported(cin, cout, k) == 0 and L.dy_conv_red_supported(cout, cin, k) == 0
    assert not rt.eng._reduced
    rsd = {"cv." + n: (v.double().clone().requires_grad_("running" not in n) if v.is_floating_point() else v.clone()) for n, v in sd.items()}
    xr = x.double().requires_grad_(True)
    ry = onn.conv_bn_silu(rsd, "cv", xr, k, s, True)
    (ry * gy.double()).sum().backward()
    e = {"y": relerr(y, ry.detach()), "gx": relerr(gxs[0], xr.grad)}
    params, bufs = dict(m.named_parameters()), dict(m.named_buffers())
    for n in ("conv.weight", "bn.weight", "bn.bias"):
        e[n] = relerr(params[n].grad.cpu(), rsd["cv." + n].grad)
    for n in ("bn.running_mean", "bn.running_var"):
        e[n] = relerr(bufs[n].cpu(), rsd["cv." + n].detach())
    print(f"Conv({cin}, {cout}, {k}, {s}):", {n: f"{v:.2e}" for n, v in e.items()})
    assert e["y"] < 3e-3 and e["gx"] < 6e-3 and all(e[n] < 4e-3 for n in ("conv.weight", "bn.weight", "bn.bias")), e
    assert e["bn.running_mean"] < 2e-3 and e["bn.running_var"] < 2e-3, e


def test_print_the_worst_ratios():
    """Informational (the bounds are derived; nothing here asserts a ratio): the table of DESIGN section 4.1."""
    for (fam, out), v in sorted(RATIOS.items()):
        print(f"{fam:12s} {out:28s} {v:.3f}")
