"""tests/conv_ref.py without a GPU: the float64 reference and the derived bounds that tests/test_gpu_conv_fallback.py holds the
fallback convolution kernels to.  The reference alone passes (the kernels' arithmetic emulated in IEEE fp32, in two accumulation
orders, sits inside every bound with room), the bounds have teeth (each listed mutation of the float64 result is rejected), and the
autograd gradients equal the direct transposed-convolution / correlation formulas."""
import pytest
import torch

import conv_ref as R

ALL = [(c, nhw) for c in R.CASES + R.FORCED_V1 for nhw in c.maps]
IDS = [f"{c.id}-{'x'.join(map(str, nhw))}" for c, nhw in ALL]


FP16_OUT = ("y0", "y_stats", "y_acc_stats", "y_silu", "y16_accum", "dX", "dX accumulate")


@pytest.mark.parametrize("case,nhw", ALL, ids=IDS)
def test_fp32_emulation_sits_inside_every_bound_with_room(case, nhw):
    """float32 F.conv2d of the same inputs with every epilogue as the kernels write it, and the same accumulated per tap and per
    32-channel k-step: everything is in bound, and the worst err / bound is < 0.5 for every output ``compare`` checks.  An fp16 output
    is measured BEFORE its rounding, against the fp32 part of its bound: a correct rounding alone uses up to the whole 2^-11 |ref| term
    (half an fp16 ulp IS 2^-11 |ref| at the bottom of a binade), so a stored value has no room to show, whatever computed it."""
    worst = {}
    for chunked in (False, True):
        # as the ping-pong / dg2 kernels accumulate and sum (two roundings, fp32 sums): in bound under their rule
        assert len(R.compare(R.emulate(case, nhw, chunked, pp=True), case, nhw, fwd_pp=True, dgrad_pp=True)) == 15
        res = R.emulate(case, nhw, chunked)
        log = R.compare(res, case, nhw)  # asserts <= 1 for every output, stored fp16 values included
        assert len(log) == 15
        log = {k: v for k, v in log.items() if not k.endswith(FP16_OUT)}
        exp, r, pre = R.expected(case, nhw), R.reference(case, nhw), res["pre"]
        for k in ("y0", "y_silu", "y16_accum"):
            log[k + " before rounding"] = R.check(pre[k], exp[k][0], R.fp32_part(exp[k][1]), f"{case.id} {k} before rounding")
        Kdx = R.round8(case.cout) * case.ks ** 2
        ref2 = R.nhwc_inv(res["dx"][..., :case.cin].double()) + r["dx"]
        log["dX before rounding"] = R.check(pre["dx"], r["dx"], R.b32(r["dx"], r["Sdx"], Kdx), f"{case.id} dX before rounding")
        log["dX accumulate before rounding"] = R.check(pre["dx2"], ref2, R.b32(ref2, r["Sdx"], Kdx), f"{case.id} dX accumulate before rounding")
        for k, v in log.items():
            worst[k] = max(worst.get(k, 0.0), v)
    k = max(worst, key=worst.get)
    print(f"{case.id} {nhw}: worst emulation err / bound = {worst[k]:.3f} ({k})")
    assert worst[k] < 0.5, (k, worst[k])


def _bound_y0(case, nhw):
    ref, terms = R.expected(case, nhw)["y0"]
    return ref, R.total(terms)


def _rejected(mut, ref, bnd):
    """The mutated float64 result, stored as the kernel stores it (fp16), is out of bound somewhere."""
    return bool(((mut.half().double() - ref).abs() > bnd).any())


MUT_CASES = [c for c in R.CASES if c.cin in (88, 144, 128, 1024, 264) and c.cout in (48, 144, 37)]


@pytest.mark.parametrize("case", MUT_CASES, ids=[c.id for c in MUT_CASES])
def test_bounds_reject_forward_mutations(case):
    nhw = case.maps[0]  # (2, 19, 37) / (2, 21, 39): two images
    r = R.reference(case, nhw)
    ref, bnd = _bound_y0(case, nhw)
    assert not _rejected(ref, ref, bnd)
    x, w, ks, s, pad = r["x"], r["w"], case.ks, case.s, case.ks // 2
    xp = torch.nn.functional.pad(x, (pad, pad, pad, pad))
    done = []

    def patch(n, oy, ox, c0, c1):  # the input window of output pixel (oy, ox), channels [c0, c1)
        return xp[n, c0:c1, oy * s:oy * s + ks, ox * s:ox * s + ks]

    # one tap (the centre one, which exists at every border) dropped at one border pixel only
    m = ref.clone()
    m[1, :, 0, 0] -= w[:, :, pad, pad] @ patch(1, 0, 0, 0, case.cin)[:, pad, pad]
    done.append(("tap at a border pixel", _rejected(m, ref, bnd)))
    # one 8-channel granule dropped at one pixel
    m = ref.clone()
    oy, ox = ref.shape[2] - 2, ref.shape[3] - 1
    m[0, :, oy, ox] -= torch.einsum("ockl,ckl->o", w[:, 8:16], patch(0, oy, ox, 8, 16))
    done.append(("8-channel granule at one pixel", _rejected(m, ref, bnd)))
    done.append(("images swapped", _rejected(ref.flip(0), ref, bnd)))
    m = ref.clone()
    m[:, :, :, 5] = ref[:, :, :, 6]
    done.append(("one output column shifted", _rejected(m, ref, bnd)))
    if case.cout == 144:
        m = ref.clone()
        m[:, 128:144] = 0
        done.append(("cout group 128...143 zeroed", _rejected(m, ref, bnd)))
    for what, rej in done:
        print(f"{case.id}: {what}: {'rejected' if rej else 'ACCEPTED'}")
    assert all(rej for _, rej in done), done
    assert case.cout != 144 or len(done) == 5


S2_CASES = [c for c in R.CASES if c.s == 2]


@pytest.mark.parametrize("case", S2_CASES, ids=[c.id for c in S2_CASES])
def test_bounds_reject_a_contribution_from_an_odd_parity_position(case):
    """dil = 2: the input gradient reads a zero-dilated map; a kernel whose parity predicate lets ONE odd position through (here with
    the value of its even neighbour) must be out of bound."""
    nhw = case.maps[0]
    N, H, W = nhw
    r = R.reference(case, nhw)
    Kdx = R.round8(case.cout) * 9
    bnd = R.total(R.b16(r["dx"], R.b32(r["dx"], r["Sdx"], Kdx)))
    v = R.dilate(r["dy"], 2)
    clean = R.dgrad_direct(v, r["w"], 3, H, W)
    assert not _rejected(clean, r["dx"], bnd)
    for oy, ox in ((1, 0), (0, 1), (3, 5)):
        m = v.clone()
        m[0, :, oy, ox] = v[0, :, oy - oy % 2, ox - ox % 2]
        assert _rejected(R.dgrad_direct(m, r["w"], 3, H, W), r["dx"], bnd), (oy, ox)
    print(f"{case.id}: odd-parity contributions rejected")


@pytest.mark.parametrize("case,nhw", [(c, c.maps[-1]) for c in R.CASES], ids=[c.id for c in R.CASES])
def test_autograd_equals_the_direct_formulas(case, nhw):
    """dX == the stride-1 convolution of the zero-dilated dY with the flipped, transposed kernel; dW == the correlation of x with dY."""
    N, H, W = nhw
    r = R.reference(case, nhw)
    dx = R.dgrad_direct(R.dilate(r["dy"], case.s), r["w"], case.ks, H, W)
    dw = R.wgrad_direct(r["x"], r["dy"], case.ks, case.s)
    assert float((dx - r["dx"]).abs().max()) < 1e-12 and float((dw - r["dw"]).abs().max()) < 1e-12
    # and the absolute-value forms are what the bounds take them for
    assert float((R.wgrad_direct(r["x"].abs(), r["dy"].abs(), case.ks, case.s) - r["Sdw"]).abs().max()) < 1e-12
    assert bool((r["S"] >= r["y"].abs() - 1e-12).all()) and bool((r["Sdx"] >= r["dx"].abs() - 1e-12).all())


def test_case_tables():
    """Every (case, map) is distinct, the persistent maps have 513 tiles, and the padded cout group / ragged widths are in."""
    assert len(set(ALL)) == len(ALL) and len(R.FALLBACK_CASES) == 19
    assert len({c.kernel for c in R.FALLBACK_CASES}) == 19 and all(R.is_fallback(c.kernel) for c in R.FALLBACK_CASES + R.RAGGED_CASES)
    for case, (N, H, W), th in R.PERSISTENT:
        Ho, Wo = R.out_hw(case, H, W)
        assert N * -(-Ho // th) * -(-Wo // 32) == 513
        assert N * -(-(Ho - 1) // th) * -(-Wo // 32) == 512 or case.s == 1  # stride 2: the smallest height with 513 tiles
    assert any(c.cout % 8 for c in R.RAGGED_CASES) and any(c.cout == 144 and c.cin == 128 for c in R.FALLBACK_CASES)
