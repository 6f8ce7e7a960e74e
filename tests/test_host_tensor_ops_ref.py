"""The float64 references of tests/tensor_ops_ref.py against ATen and autograd on the CPU: what tests/test_gpu_tensor_ops.py compares the
HIP kernels with is tied here to the operations of the reference modules, without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import tensor_ops_ref as R


@pytest.mark.parametrize("shape,neg", [((2, 8, 12, 24), False), ((1, 8, 8, 16), True), ((2, 4, 4, 8), True)])
def test_scalseq_closed_form_equals_autograd(shape, neg):
    """dr_l == r_l.grad, S1 == beta.grad, S2 == gamma.grad through interpolate(nearest) -> stack -> batch_norm(training) -> leaky_relu ->
    max_pool3d, with coef from the batch statistics and bwdcoef = S / (3NHW); negative gamma included."""
    N, H, W, C = shape
    g = R.gen(11 + C)
    r = [torch.randn(N, H >> l, W >> l, C, generator=g, dtype=torch.float64) for l in range(3)]
    dy = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    if neg:
        gamma[1::2] *= -1
    beta = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    grads, ggamma, gbeta, coef = R.scalseq_autograd(r, dy, gamma, beta)
    s = R.scalseq_backward(r, dy, coef)
    cnt = 3 * N * H * W
    out = R.scalseq_backward(r, dy, coef, torch.stack([s["S1"], s["S2"]]) / cnt)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    assert rel(s["S1"], gbeta) < 1e-8 and rel(s["S2"], ggamma) < 1e-8
    for l in range(3):
        assert rel(out["dr"][l], grads[l]) < 1e-8, l
    # and the forward: the same coefficients give the module's output
    rs = [t.permute(0, 3, 1, 2) for t in r]
    vol = torch.stack([rs[0], F.interpolate(rs[1], size=(H, W)), F.interpolate(rs[2], size=(H, W))], 2)
    y = F.max_pool3d(F.leaky_relu(F.batch_norm(vol, None, None, gamma, beta, True, 0.0, 1e-3), 0.1), (3, 1, 1)).squeeze(2)
    assert rel(R.scalseq_tail(r, coef)[0], y.permute(0, 2, 3, 1)) < 1e-12


def test_scalseq_tie_and_zero_rules_are_atens():
    """max_pool3d over the depth routes a tie to the first level and propagates a NaN; leaky_relu's slope at exactly 0 is 0.1: the
    rules scalseq_argmax / scalseq_backward write out."""
    v = torch.tensor([[1.0, 1.0, 0.0], [0.0, 2.0, 2.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -1.0]], dtype=torch.float64)  # (pos, level)
    vol = v.t().reshape(1, 1, 3, 4, 1).clone().requires_grad_(True)
    F.max_pool3d(vol, (3, 1, 1)).sum().backward()
    am_aten = vol.grad.view(3, 4).argmax(0)
    am, zb, gap = R.scalseq_argmax([v[:, l] for l in range(3)])
    assert am.tolist() == am_aten.tolist() == [0, 1, 0, 0]
    assert zb.tolist() == [1.0, 2.0, 0.0, -1.0] and gap.tolist() == [0.0, 0.0, 0.0, 0.0]
    z = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    F.leaky_relu(z, 0.1).sum().backward()
    assert z.grad.tolist() == [0.1, 0.1, 0.1]
    nan = torch.tensor([0.0, float("nan"), 1.0], dtype=torch.float64).view(1, 1, 3, 1, 1)
    assert bool(torch.isnan(F.max_pool3d(nan, (3, 1, 1))).all())
    r = [torch.zeros(1, 4 >> l, 4 >> l, 8, dtype=torch.float64) for l in range(3)]
    r[2][0, 0, 0, 3] = float("nan")
    y = R.scalseq_tail(r, torch.tensor([[1.0] * 8, [0.0] * 8]))[0]
    assert int(torch.isnan(y).sum()) == 16 and bool(torch.isnan(y[..., 3]).all())


@pytest.mark.parametrize("shape", R.SCALSEQ_FWD_SHAPES)
def test_scalseq_exact_regime_is_exact_in_fp32(shape):
    """The ties case: on the k/4 grid with dyadic coefficients the kernel's fp32 chain (emulated here in IEEE fp32) picks the level the
    float64 reference picks everywhere, ties are frequent, winners equal to 0 occur, and the fp16-rounded outputs coincide."""
    r, dy, coef = R.scalseq_inputs(R.seed_of(shape, True), *shape, exact=True)
    z64, _, _ = R.scalseq_levels(r, coef)
    am64, zb64, gap = R.scalseq_argmax(z64)
    z32 = []
    for l in range(3):
        up = r[l].float()
        for _ in range(l):
            up = R.upsample2x(up)
        p = up * coef[0] + coef[1]
        z32.append(torch.where(p > 0, p, torch.tensor(0.1, dtype=torch.float32) * p))
    am32, zb32, _ = R.scalseq_argmax(z32)
    assert torch.equal(am32, am64)
    assert torch.equal(zb32 > 0, zb64 > 0)
    ties, zeros = float((gap == 0).double().mean()), float((zb64 == 0).double().mean())
    print(f"{shape}: {100 * ties:.1f}% of positions tie for first place, {100 * zeros:.1f}% of winners are exactly 0")
    assert ties > 0.03 and zeros > 0.01
    assert float(gap[gap > 0].min()) > 0.012  # a grid step (1/8 with scale 0.5) through the 0.1 slope at the least: 0.0125
    res = R.randn16(R.gen(5), *shape)
    y, m, _ = R.scalseq_tail(r, coef)
    assert torch.equal(zb32.half(), m.half())
    assert torch.equal((zb32.half().float() + res.float()).half(), (R.h16(m) + res).half())


@pytest.mark.parametrize("shape,kernel", R.SCALSEQ_BWD_SHAPES)
def test_scalseq_realistic_regime_exempts_few_pixels(shape, kernel):
    N, H, W, C = shape
    assert R.scalseq_kernel(W, C) == kernel and H % 4 == 0 and W % 4 == 0
    r, dy, coef = R.scalseq_inputs(R.seed_of(shape, False), *shape, exact=False)
    s = R.scalseq_backward(r, dy, coef)
    shares = [float(e.double().mean()) for e in R.scalseq_exempt(s["gap"])]
    zmax = max(float(z.abs().max()) for z in R.scalseq_levels(r, coef)[0])
    print(f"{shape}: exempt shares {[f'{100 * v:.2f}%' for v in shares]}, max |z| {zmax:.2f}")
    assert all(v <= cap for v, cap in zip(shares, R.EXEMPT_CAPS)), shares
    assert zmax <= 8.0  # GAP = 1e-4 stays above 100 fp32 ulps of z


def _scan_pool(x):
    """5x5 pool by the row-major window scan: a larger value or a NaN replaces the running maximum."""
    H, W = x.shape
    y, code = torch.empty(H, W, dtype=torch.float64), torch.empty(H, W, dtype=torch.uint8)
    for oy in range(H):
        for ox in range(W):
            best, bc = -float("inf"), 0
            for dy in range(5):
                for dx in range(5):
                    yy, xx = oy + dy - 2, ox + dx - 2
                    if 0 <= yy < H and 0 <= xx < W:
                        f = float(x[yy, xx])
                        if f > best or f != f:
                            best, bc = f, dy * 5 + dx
            y[oy, ox], code[oy, ox] = best, bc
    return y, code


def test_maxpool5_reference_is_first_maximum_last_nan():
    ones = torch.ones(1, 4, 7, 8, dtype=torch.float64)
    y, code, flat = R.maxpool5(ones)
    assert int(flat[0, 0, 0, 0]) == 0 and int(code[0, 0, 0, 0]) == 12 and int(code[0, 3, 6, 0]) == 0 and int(code[0, 2, 3, 0]) == 0
    g = R.gen(2)
    x = R.coarse16(g, 1, 6, 7, 8)
    x[0, 1, 2, 0] = float("nan")
    x[0, 2, 4, 0] = float("nan")
    y, code, flat = R.maxpool5(x)
    for c in (0, 5):
        ys, cs = _scan_pool(x[0, :, :, c])
        R.same_bits(y[0, :, :, c].half(), ys.half(), "pool value")
        R.same_bits(code[0, :, :, c], cs, "pool code")
    assert int(flat[0, 2, 3, 0]) == 2 * 7 + 4  # both NaNs in the window: the last one in row-major order
    # the scatter is ATen's backward
    x = R.coarse16(g, 2, 5, 6, 8)
    dy = R.randn16(g, 2, 5, 6, 8)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(xr, 5, 1, 2).backward(dy.permute(0, 3, 1, 2))
    ref, mag = R.maxpool5_backward(dy, R.maxpool5(x)[2])
    assert float((ref - xr.grad.permute(0, 2, 3, 1)).abs().max()) < 1e-12 and bool((mag >= ref.abs() - 1e-12).all())


def test_zoom_pool_reference_routes_ties_to_the_first():
    x = torch.ones(1, 4, 6, 8, dtype=torch.float64)
    dy = torch.ones(1, 2, 3, 8, dtype=torch.float64)
    ref, _ = R.zoom_pool_backward(x, dy)
    assert torch.equal(ref[0, :2, :2, 0], torch.tensor([[1.25, 0.25], [0.25, 0.25]], dtype=torch.float64))
    y, mean = R.zoom_pool(x)
    assert torch.equal(y, torch.full_like(y, 2.0)) and torch.equal(mean, torch.ones_like(mean))


def test_upsample_and_add_references():
    g = R.gen(4)
    dy = R.randn16(g, 2, 6, 10, 8)
    xr = torch.zeros(2, 8, 3, 5, dtype=torch.float64, requires_grad=True)
    F.interpolate(xr, scale_factor=2.0, mode="nearest").backward(dy.permute(0, 3, 1, 2))
    ref, mag = R.upsample2x_backward(dy)
    assert float((ref - xr.grad.permute(0, 2, 3, 1)).abs().max()) < 1e-12
    x = R.randn16(g, 2, 3, 5, 8)
    assert torch.equal(R.upsample2x(x), F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest").permute(0, 2, 3, 1))
    a, b, c = (R.randn16(g, 7, 8).half() for _ in range(3))
    # the chain rounds twice: it is not the single rounding of the exact sum everywhere, and it is within its two-rounding bound
    v = R.add_f32_chain(a, b, c)
    exact = a.double() + b.double() + c.double()
    R.check(v, exact, R.bound(exact, k16=1, abs16=(a.double() + b.double()).abs()), "add chain")


def test_check_bites_at_one_element():
    ref = torch.full((4, 8), 1.0, dtype=torch.float64)
    got = ref.clone()
    got[2, 3] += 1.01 * (R.EPS16 + R.TINY)
    R.check(ref + 0.99 * R.EPS16, ref, R.bound(ref, k16=1), "inside")
    with pytest.raises(AssertionError, match=r"1 of 32 elements out of bound; worst at \(2, 3\)"):
        R.check(got, ref, R.bound(ref, k16=1), "one element off")
    with pytest.raises(AssertionError):
        R.same_bits(torch.tensor([0.0, float("nan")]).half(), torch.tensor([float("nan"), 0.0]).half())
