"""-m gpu: the kernels of csrc/tensor_ops.hip through their C entry points, each against the float64 reference of tests/tensor_ops_ref.py
(validated on the CPU by tests/test_host_tensor_ops_ref.py), compared PER ELEMENT:

    |got - ref| <= k16 * 2^-11 * |ref| + k32 * 2^-23 * mag + 2^-24

with k16 / k32 / mag written next to each comparison (tensor_ops_ref.py explains the terms).  Selections and copies must be bit-equal.
Every op runs on dense maps (ld == C) and on channel slices of wider buffers (pointer offset by 8 channels, pitch C + 8 or C + 16) that
were pre-filled with a canary: the bytes outside the slice, and every input, must be unchanged afterwards."""
import ctypes as C
import functools
import math

import pytest
import torch

import tensor_ops_ref as R

pytestmark = pytest.mark.gpu

CANARY = 777.0
LAYOUTS = ["dense", "slice"]


@pytest.fixture(scope="module")
def L():
    from ultralytics.hip.engine import Engine
    return Engine("cuda:0").L


def _s():
    return torch.cuda.current_stream().cuda_stream


class Map:
    """A (..., C) fp16 map in device memory: dense, or channels [8, 8 + C) of a canary-filled buffer of pitch C + pad."""

    def __init__(self, shape, data=None, layout="dense", pad=16, dtype=torch.float16):
        self.C = shape[-1]
        self.c0, self.ld = (8, self.C + pad) if layout == "slice" else (0, self.C)
        self.full = torch.full((*shape[:-1], self.ld), CANARY, dtype=dtype, device="cuda")
        if data is not None:
            self.view().copy_(data.to(dtype))
        self.before = self.full.clone()
        self.ptr = self.full.data_ptr() + self.c0 * self.full.element_size()

    def view(self):
        return self.full[..., self.c0:self.c0 + self.C]

    def get(self):
        torch.cuda.synchronize()
        return self.view().cpu()

    def outside_unchanged(self):
        torch.cuda.synchronize()
        a, b = self.full.clone(), self.before.clone()
        a[..., self.c0:self.c0 + self.C] = 0
        b[..., self.c0:self.c0 + self.C] = 0
        return torch.equal(a.view(torch.int16), b.view(torch.int16))

    def unchanged(self):
        torch.cuda.synchronize()
        return torch.equal(self.full.view(torch.int16), self.before.view(torch.int16))


def _dev(t):
    return t.float().contiguous().cuda()


# =====================================================================================================================================
# 1. ScalSeq tail forward
# =====================================================================================================================================
def _ss_forward(L, shape, r, coef, res, layout):
    N, H, W, Cc = shape
    rm = [Map((N, H >> l, W >> l, Cc), r[l], layout, pad=8 + 8 * l) for l in range(3)]
    resm = None if res is None else Map(shape, res, layout)
    y = Map(shape, None, layout)
    cd = _dev(coef)
    assert L.dy_scalseq_tail(rm[0].ptr, rm[0].ld, rm[1].ptr, rm[1].ld, rm[2].ptr, rm[2].ld, 0 if resm is None else resm.ptr,
                             0 if resm is None else resm.ld, y.ptr, y.ld, cd.data_ptr(), N, H, W, Cc, _s()) == 0
    got = y.get()
    assert y.outside_unchanged() and all(m.unchanged() for m in rm) and (resm is None or resm.unchanged())
    return got


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("shape", R.SCALSEQ_FWD_SHAPES)
def test_scalseq_tail_forward(L, shape, with_res, layout):
    """z_l = leaky(r_l_up * scale + shift), max over the levels by F.max_pool3d, + res; negative scales on every third channel."""
    r, _, coef = R.scalseq_inputs(R.seed_of(shape, False), *shape, exact=False)
    res = R.randn16(R.gen(5), *shape) if with_res else None
    ref, m, mag = R.scalseq_tail(r, coef, res)
    got = _ss_forward(L, shape, r, coef, res, layout)
    # scalseq_tail_kernel: z = v * coef + shift, 0.1f * z (k32 = 3 on mag = |v * coef| + |shift|); without res one rounding of the
    # maximum at the store (k16 = 1); with res the maximum is rounded first and the sum once more (k16 = 2: 2^-11 |m| + 2^-11 |y|)
    bnd = R.bound(ref, k16=1, k32=3, mag=mag, abs16=m.abs() if with_res else None)
    R.check(got, ref, bnd, f"scalseq_tail {shape} res={with_res} {layout}")


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("shape", R.SCALSEQ_FWD_SHAPES)
def test_scalseq_tail_forward_ties_are_exact(L, shape, with_res):
    """Inputs on the k/4 grid, scale in {0.5, 1, 2, -1}, shift a multiple of 1/4: z is exact in fp32, ~9% of the positions tie for first
    place and ~4% of the winners are exactly 0 (tests/test_host_tensor_ops_ref.py), so the output is the reference rounded to fp16."""
    r, _, coef = R.scalseq_inputs(R.seed_of(shape, True), *shape, exact=True)
    res = R.randn16(R.gen(5), *shape) if with_res else None
    _, m, _ = R.scalseq_tail(r, coef)
    want = m.half() if res is None else (R.h16(m) + res).half()
    R.same_bits(_ss_forward(L, shape, r, coef, res, "slice"), want, f"scalseq_tail ties {shape} res={with_res}")


def test_scalseq_tail_forward_propagates_nan(L):
    """One NaN in r1 and one in r2: NaN at every position they map to, as max_pool3d gives (eval-mode coefficients are fixed, so nothing
    else would show it); every other output stays within its bound."""
    shape = (2, 8, 12, 24)
    r, _, coef = R.scalseq_inputs(R.seed_of(shape, False), *shape, exact=False)
    r[1][1, 2, 3, 5] = float("nan")
    r[2][0, 1, 2, 17] = float("nan")
    r0 = [torch.nan_to_num(t, nan=0.0) for t in r]
    ref, _, mag = R.scalseq_tail(r0, coef)
    want_nan = torch.isnan(R.scalseq_tail(r, coef)[0])
    assert int(want_nan.sum()) == 4 + 16
    got = _ss_forward(L, shape, r, coef, None, "dense")
    assert torch.equal(torch.isnan(got), want_nan), (int(torch.isnan(got).sum()), int(want_nan.sum()))
    R.check(torch.where(want_nan, ref.half(), got), ref, R.bound(ref, k16=1, k32=3, mag=mag), "scalseq_tail beside the NaNs")


# =====================================================================================================================================
# 2. ScalSeq tail backward: dy_scalseq_tail_backward_all (both kernels) and the per-level dy_scalseq_tail_backward
# =====================================================================================================================================
BWD_CASES = [(shape, exact) for shape, _ in R.SCALSEQ_BWD_SHAPES for exact in (True, False)]
BWD_IDS = [f"{'x'.join(map(str, s))}-{'exact' if e else 'realistic'}" for s, e in BWD_CASES]
ENGINE_PARTIALS = 2048  # Engine._scalseq_bwd


@functools.lru_cache(maxsize=None)
def _ss_case(shape, exact):
    """Inputs and the closed-form reference of one case, computed once and shared (nothing below writes to them)."""
    N, H, W, Cc = shape
    assert H % 4 == 0 and W % 4 == 0
    assert dict(R.SCALSEQ_BWD_SHAPES)[shape] == R.scalseq_kernel(W, Cc)  # the kernel the case is listed for is the one it takes
    r, dy, coef = R.scalseq_inputs(R.seed_of(shape, exact), *shape, exact=exact)
    g = R.gen(99)
    bw = torch.stack([0.05 * torch.randn(Cc, generator=g), 0.05 * torch.randn(Cc, generator=g)]).float()  # not derived from the data
    ref = R.scalseq_backward(r, dy, coef, bw)
    if exact:  # the arg-max is deterministic, ties included: no position is exempt
        exempt = [torch.zeros_like(d, dtype=torch.bool) for d in ref["dr"]]
    else:
        exempt = R.scalseq_exempt(ref["gap"])
        shares = [float(e.double().mean()) for e in exempt]
        assert all(v <= cap for v, cap in zip(shares, R.EXEMPT_CAPS)), (shape, shares)  # on the reference, before the GPU runs
    # mode 0, realistic regime: a position fp32 may route to another level moves the channel's sums by at most |dy| (1 + |xhat|)
    n_ex = (ref["gap"] < R.GAP).double().sum((0, 1, 2)) if not exact else torch.zeros(Cc, dtype=torch.float64)
    widen = n_ex * float(dy.abs().max()) * (1 + ref["xhatmax"])
    return dict(r=r, dy=dy, coef=coef, bw=bw, ref=ref, exempt=exempt, widen=widen)


def _sum_depth(kind, shape, nparts, level=0):
    """fp32 additions on the longest path into one partial: a thread's accumulation over its grid-stride iterations (``per`` additions
    each, the g * xhat products and xhat's own two operations included), then the rows of the block's LDS reduce."""
    N, H, W, Cc = shape
    cpp = Cc // 8
    if kind == "cols":    # scalseq_bwd_cols_kernel: 4 wave items per block and iteration; per item 4 x (g0) + 2 x (2 gs1 + shuffle + ps) + (4 gs2 + 2 shuffles + ps)
        iters, per = math.ceil(N * (H // 4) * (W // (64 // cpp)) / (nparts * 4)), 4 + 2 * 4 + 7
    elif kind == "block":  # scalseq_bwd_all_kernel: 256 / cpp level-2 pixels per block and iteration; per pixel 16 x (g0) + 4 x (4 gs1 + ps) + (16 gs2 + ps)
        iters, per = math.ceil(N * (H // 4) * (W // 4) / (nparts * (256 // cpp))), 16 + 4 * 5 + 17
    else:                  # scalseq_bwd_kernel: 256 / cpp level-l pixels per block and iteration; per pixel s * s (gsum) + ps
        iters, per = math.ceil(N * (H >> level) * (W >> level) / (nparts * (256 // cpp))), (1 << level) ** 2 + 1
    return iters * (per + 3) + 256 // cpp


def _ss_maps(case, shape, layout):
    N, H, W, Cc = shape
    rm = [Map((N, H >> l, W >> l, Cc), case["r"][l], layout, pad=8) for l in range(3)]
    dym = Map(shape, case["dy"], layout, pad=8)
    rargs = (rm[0].ptr, rm[0].ld, rm[1].ptr, rm[1].ld, rm[2].ptr, rm[2].ld, dym.ptr, dym.ld)
    return rm + [dym], rargs


def _partials(Cc, blocks):
    return torch.full((blocks * 2 * Cc + 64,), CANARY, dtype=torch.float32, device="cuda")


def _sum_partials(part, n, Cc):
    torch.cuda.synchronize()
    assert bool((part[n * 2 * Cc:] == CANARY).all()), "partials written past nparts"
    return part[: n * 2 * Cc].view(n, 2, Cc).double().sum(0).cpu()


def _check_sums(got, case, shape, depth, what):
    ref = case["ref"]
    # S1: sum of g (k32 = depth additions on mag = sum |g|); S2: sum of g * xhat, xhat = (r - mean) * inv (mag = sum |g| (|r| + |mean|) |inv|)
    for i, (s, mag) in enumerate([("S1", "magS1"), ("S2", "magS2")]):
        R.check(got[i], ref[s], R.bound(ref[s], k32=depth, mag=ref[mag]) + case["widen"], f"{what} {s} (k32 = {depth})")


def _check_dr(got, case, l, what):
    ref = case["ref"]
    # mode 1: dr = scale * (sum_block g - cnt * mean_g - cnt * xhat * mean_gxhat): one fp16 rounding at the store (k16 = 1); in fp32 the
    # 4^l additions of the block sum, 0.1f * g, xhat's subtraction and product, xhat * mean_gxhat, two subtractions, the scale (4^l + 7)
    bnd = R.bound(ref["dr"][l], k16=1, k32=4 ** l + 7, mag=ref["magdr"][l])
    R.check(got, ref["dr"][l], bnd, f"{what} dr{l} ({int(case['exempt'][l].sum())} exempt)", mask=~case["exempt"][l])


@pytest.mark.parametrize("shape,exact", BWD_CASES, ids=BWD_IDS)
def test_scalseq_backward_all_statistics(L, shape, exact):
    """Mode 0 of dy_scalseq_tail_backward_all: the partials summed over nparts against S1 = sum g and S2 = sum g * xhat, with max_partials
    at the engine's value and at 1 and 3 (the grid-stride loops iterate)."""
    case = _ss_case(shape, exact)
    N, H, W, Cc = shape
    kind = R.scalseq_kernel(W, Cc)
    maps, rargs = _ss_maps(case, shape, "dense")
    cd = _dev(case["coef"])
    for maxp in (ENGINE_PARTIALS, 1, 3):
        part = _partials(Cc, ENGINE_PARTIALS)
        n = C.c_int(0)
        assert L.dy_scalseq_tail_backward_all(*rargs, 0, 0, 0, 0, 0, 0, cd.data_ptr(), 0, part.data_ptr(), maxp, N, H, W, Cc, 0,
                                              C.byref(n), _s()) == 0
        assert 1 <= n.value <= maxp
        _check_sums(_sum_partials(part, n.value, Cc), case, shape, _sum_depth(kind, shape, n.value), f"{kind} {shape} max_partials={maxp}")
    assert all(m.unchanged() for m in maps)


@pytest.mark.parametrize("shape,exact", BWD_CASES, ids=BWD_IDS)
def test_scalseq_backward_all_input_gradients(L, shape, exact):
    """Mode 1 of dy_scalseq_tail_backward_all against the closed form (first maximum over the levels, slope 0.1 at a winner equal to 0),
    with a random bwdcoef and random coef[2:4].  Realistic regime: a pixel is exempt when the reference's top-two gap at one of its
    positions is below 1e-4; measured shares of exempt level-0 / 1 / 2 pixels over the ten shapes: at most 0.07% / 0.29% / 1.17%
    (caps 0.5% / 1% / 3%, asserted on the reference)."""
    case = _ss_case(shape, exact)
    N, H, W, Cc = shape
    kind = R.scalseq_kernel(W, Cc)
    maps, rargs = _ss_maps(case, shape, "dense")
    cd, bd = _dev(case["coef"]), _dev(case["bw"])
    dr = [Map((N, H >> l, W >> l, Cc)) for l in range(3)]
    assert L.dy_scalseq_tail_backward_all(*rargs, dr[0].ptr, dr[0].ld, dr[1].ptr, dr[1].ld, dr[2].ptr, dr[2].ld, cd.data_ptr(), bd.data_ptr(),
                                          0, 0, N, H, W, Cc, 1, None, _s()) == 0
    for l in range(3):
        _check_dr(dr[l].get(), case, l, f"{kind} {shape}")
    assert all(m.unchanged() for m in maps)


@pytest.mark.parametrize("shape,exact", BWD_CASES, ids=BWD_IDS)
def test_scalseq_backward_per_level(L, shape, exact):
    """The per-level dy_scalseq_tail_backward (levels 0, 1, 2; still exported) on the same inputs against the same reference."""
    case = _ss_case(shape, exact)
    N, H, W, Cc = shape
    maps, rargs = _ss_maps(case, shape, "dense")
    cd, bd = _dev(case["coef"]), _dev(case["bw"])
    total, depth = torch.zeros(2, Cc, dtype=torch.float64), 0
    for l in range(3):
        part = _partials(Cc, 1024)
        n = C.c_int(0)
        assert L.dy_scalseq_tail_backward(*rargs, 0, 0, cd.data_ptr(), 0, part.data_ptr(), 1024, N, H, W, Cc, l, 0, C.byref(n), _s()) == 0
        assert 1 <= n.value <= 1024
        total += _sum_partials(part, n.value, Cc)
        depth += _sum_depth("level", shape, n.value, l)
        d = Map((N, H >> l, W >> l, Cc))
        assert L.dy_scalseq_tail_backward(*rargs, d.ptr, d.ld, cd.data_ptr(), bd.data_ptr(), 0, 0, N, H, W, Cc, l, 1, None, _s()) == 0
        _check_dr(d.get(), case, l, f"per-level {shape}")
    _check_sums(total, case, shape, depth, f"per-level {shape}")
    assert all(m.unchanged() for m in maps)


@pytest.mark.parametrize("shape,exact", BWD_CASES, ids=BWD_IDS)
def test_scalseq_backward_engine_chain(L, shape, exact):
    """What Engine._scalseq_bwd runs: partials -> dy_bn_bwd_finalize -> dgamma, dbeta, bwdcoef -> mode 1 with that bwdcoef."""
    case = _ss_case(shape, exact)
    N, H, W, Cc = shape
    kind = R.scalseq_kernel(W, Cc)
    maps, rargs = _ss_maps(case, shape, "dense")
    cd = _dev(case["coef"])
    part = _partials(Cc, ENGINE_PARTIALS)
    n = C.c_int(0)
    assert L.dy_scalseq_tail_backward_all(*rargs, 0, 0, 0, 0, 0, 0, cd.data_ptr(), 0, part.data_ptr(), ENGINE_PARTIALS, N, H, W, Cc, 0,
                                          C.byref(n), _s()) == 0
    dgamma, dbeta, bw = (torch.full((k * Cc,), CANARY, device="cuda") for k in (1, 1, 2))
    cnt = float(3 * N * H * W)
    assert L.dy_bn_bwd_finalize(part.data_ptr(), n.value, dgamma.data_ptr(), dbeta.data_ptr(), bw.data_ptr(), Cc, cnt, 0, _s()) == 0
    torch.cuda.synchronize()
    depth = _sum_depth(kind, shape, n.value) + 1  # bn_bwd_finalize_kernel adds the partials in fp64 and rounds to fp32 once
    _check_sums(torch.stack([dbeta, dgamma]).cpu(), case, shape, depth, f"finalize {shape}")
    _check_sums(bw.view(2, Cc).cpu() * cnt, case, shape, depth + 1, f"bwdcoef {shape}")
    # mode 1 with the chain's own bwdcoef: the reference takes the fp32 values the kernel reads
    chained = R.scalseq_backward(case["r"], case["dy"], case["coef"], bw.view(2, Cc).cpu())
    dr = [Map((N, H >> l, W >> l, Cc)) for l in range(3)]
    assert L.dy_scalseq_tail_backward_all(*rargs, dr[0].ptr, dr[0].ld, dr[1].ptr, dr[1].ld, dr[2].ptr, dr[2].ld, cd.data_ptr(), bw.data_ptr(),
                                          0, 0, N, H, W, Cc, 1, None, _s()) == 0
    for l in range(3):
        _check_dr(dr[l].get(), dict(case, ref=chained), l, f"chain {shape}")
    assert all(m.unchanged() for m in maps)


@pytest.mark.parametrize("shape", [(2, 8, 16, 32), (2, 8, 12, 24)], ids=["cols", "block"])
def test_scalseq_backward_on_slices(L, shape):
    """One cols and one block shape with strided r, dy and dr (ld = C + 8, channel offset 8) and canaries, both entry points."""
    case = _ss_case(shape, False)
    N, H, W, Cc = shape
    kind = R.scalseq_kernel(W, Cc)
    maps, rargs = _ss_maps(case, shape, "slice")
    cd, bd = _dev(case["coef"]), _dev(case["bw"])
    part = _partials(Cc, ENGINE_PARTIALS)
    n = C.c_int(0)
    assert L.dy_scalseq_tail_backward_all(*rargs, 0, 0, 0, 0, 0, 0, cd.data_ptr(), 0, part.data_ptr(), ENGINE_PARTIALS, N, H, W, Cc, 0,
                                          C.byref(n), _s()) == 0
    _check_sums(_sum_partials(part, n.value, Cc), case, shape, _sum_depth(kind, shape, n.value), f"{kind} slices {shape}")
    dr = [Map((N, H >> l, W >> l, Cc), None, "slice", pad=8) for l in range(3)]
    assert L.dy_scalseq_tail_backward_all(*rargs, dr[0].ptr, dr[0].ld, dr[1].ptr, dr[1].ld, dr[2].ptr, dr[2].ld, cd.data_ptr(), bd.data_ptr(),
                                          0, 0, N, H, W, Cc, 1, None, _s()) == 0
    for l in range(3):
        _check_dr(dr[l].get(), case, l, f"{kind} slices {shape}")
        assert dr[l].outside_unchanged()
        d = Map((N, H >> l, W >> l, Cc), None, "slice", pad=8)
        assert L.dy_scalseq_tail_backward(*rargs, d.ptr, d.ld, cd.data_ptr(), bd.data_ptr(), 0, 0, N, H, W, Cc, l, 1, None, _s()) == 0
        _check_dr(d.get(), case, l, f"per-level slices {shape}")
        assert d.outside_unchanged()
    assert all(m.unchanged() for m in maps)


# =====================================================================================================================================
# 3. 5x5 max-pool and the fused SPPF pools
# =====================================================================================================================================
POOL_SHAPES = [(8, 1, 1), (16, 2, 3), (8, 4, 7), (24, 11, 13)]  # C, H, W
POOL_N = 2


def _pool_input(Cc, H, W, variant):
    g = R.gen(100 * H + W + Cc)
    x = R.coarse16(g, POOL_N, H, W, Cc) if variant != "random" else R.randn16(g, POOL_N, H, W, Cc)
    if variant == "nan":
        x[1, H // 2, W // 2, 3] = float("nan")
    return g, x


def _arg_buffer(npix, Cc):
    return torch.full((npix * Cc + 64,), 99, dtype=torch.uint8, device="cuda")


def _arg_get(buf, shape):
    torch.cuda.synchronize()
    n = math.prod(shape)
    assert bool((buf[n:] == 99).all()), "arg-max map written past its end"
    return buf[:n].view(shape).cpu()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("variant", ["random", "ties", "nan"])
@pytest.mark.parametrize("Cc,H,W", POOL_SHAPES)
def test_maxpool5_forward_backward(L, Cc, H, W, variant, layout):
    """dy_maxpool5 against ATen's CPU max_pool2d (first maximum, last NaN): values and window codes bit-equal, on a coarse grid that
    forces ties and with a NaN in the map; dy_maxpool5_backward against the float64 scatter to ATen's arg-max, accumulate 0 and 1."""
    g, x = _pool_input(Cc, H, W, variant)
    shape = (POOL_N, H, W, Cc)
    yref, code, flat = R.maxpool5(x)
    xm, ym = Map(shape, x, layout), Map(shape, None, layout, pad=8)
    arg = _arg_buffer(POOL_N * H * W, Cc)
    assert L.dy_maxpool5(xm.ptr, xm.ld, ym.ptr, ym.ld, arg.data_ptr(), POOL_N, H, W, Cc, _s()) == 0
    R.same_bits(ym.get(), yref.half(), "maxpool5 values")
    R.same_bits(_arg_get(arg, shape), code, "maxpool5 arg-max codes")
    assert xm.unchanged() and ym.outside_unchanged()
    dy = R.randn16(g, *shape)
    old = R.randn16(g, *shape)
    dym = Map(shape, dy, layout)
    for acc in (0, 1):
        dxm = Map(shape, old, layout, pad=8)
        assert L.dy_maxpool5_backward(dym.ptr, dym.ld, arg.data_ptr(), dxm.ptr, dxm.ld, POOL_N, H, W, Cc, acc, _s()) == 0
        ref, mag = R.maxpool5_backward(dy, flat, old if acc else None)
        # maxpool5_bwd_kernel: up to 25 window gradients + the old content added in fp32 (k32 <= 26), one rounding at the store (k16 = 1)
        R.check(dxm.get(), ref, R.bound(ref, k16=1, k32=26, mag=mag), f"maxpool5 backward acc={acc}")
        assert dxm.outside_unchanged()
    assert dym.unchanged()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("variant", ["ties", "nan"])
@pytest.mark.parametrize("Cc,H,W", POOL_SHAPES)
def test_sppf_fused_pools_match_aten_chain_with_ties(L, Cc, H, W, variant, layout):
    """dy_sppf_pool3 / dy_sppf_pool3_backward against ATen's chain y1 = m(x), y2 = m(y1), y3 = m(y2) on tie-forcing inputs: y1..y3 and the
    three arg-max maps bit-equal, the chained backward within the bound its three roundings give."""
    assert L.dy_sppf_pool3_supported(H, W, Cc) in (8, 16)
    g, x = _pool_input(Cc, H, W, variant)
    shape, cshape = (POOL_N, H, W, Cc), (POOL_N, H, W, 4 * Cc)
    ys, codes, flats = [x], [], []
    for _ in range(3):
        y, code, flat = R.maxpool5(ys[-1])
        ys.append(y); codes.append(code); flats.append(flat)
    cat = Map(cshape, torch.cat([x, torch.full((POOL_N, H, W, 3 * Cc), CANARY, dtype=torch.float64)], -1), layout)
    args = [_arg_buffer(POOL_N * H * W, Cc) for _ in range(3)]
    assert L.dy_sppf_pool3(cat.ptr, cat.ld, Cc, args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), POOL_N, H, W, _s()) == 0
    R.same_bits(cat.get(), torch.cat(ys, -1).half(), "sppf y1..y3")
    for l in range(3):
        R.same_bits(_arg_get(args[l], shape), codes[l], f"sppf arg-max {l}")
    assert cat.outside_unchanged()
    dcat = R.randn16(g, *cshape)
    d = [dcat[..., l * Cc:(l + 1) * Cc] for l in range(4)]
    for acc in ((1, 1, 1), (0, 1, 1), (1, 0, 1)):
        gm = Map(cshape, dcat, layout)
        assert L.dy_sppf_pool3_backward(gm.ptr, gm.ld, Cc, args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), POOL_N, H, W, *acc, _s()) == 0
        # sppf_pool3_bwd_kernel: level l = poolbwd(level l + 1) (+ dcat_l when acc[l]), each level as maxpool5_bwd_kernel (k16 = 1,
        # k32 <= 26) and rounded to fp16 before the next one reads it: its bound travels through the next scatter with the values
        ref, bnd = d[3], torch.zeros_like(d[3])
        for l in (2, 1, 0):
            carried = R.scatter_bound(bnd, flats[l])
            ref, mag = R.maxpool5_backward(ref, flats[l], d[l] if acc[l] else None)
            bnd = R.bound(ref, k16=1, k32=26, mag=mag) + carried
        got = gm.get()
        R.check(got[..., :Cc], ref, bnd, f"sppf chained backward acc={acc}")
        R.same_bits(got[..., Cc:], dcat[..., Cc:].half(), "sppf backward leaves the gradients of y1..y3 alone")
        assert gm.outside_unchanged()


# =====================================================================================================================================
# 4. dy_upsample2x, dy_add, dy_copy_slice
# =====================================================================================================================================
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("Cc", [8, 24])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (6, 4)])
def test_upsample2x_forward_backward(L, H, W, Cc, layout):
    N = 2
    g = R.gen(10 * H + W + Cc)
    x = R.randn16(g, N, H, W, Cc)
    xm, ym = Map((N, H, W, Cc), x, layout), Map((N, 2 * H, 2 * W, Cc), None, layout, pad=8)
    assert L.dy_upsample2x(xm.ptr, xm.ld, ym.ptr, ym.ld, N, H, W, Cc, 0, 0, _s()) == 0
    R.same_bits(ym.get(), R.upsample2x(x).half(), "upsample2x forward")
    assert xm.unchanged() and ym.outside_unchanged()
    dy, old = R.randn16(g, N, 2 * H, 2 * W, Cc), R.randn16(g, N, H, W, Cc)
    dym = Map((N, 2 * H, 2 * W, Cc), dy, layout)
    for acc in (0, 1):
        dxm = Map((N, H, W, Cc), old, layout, pad=8)
        assert L.dy_upsample2x(dym.ptr, dym.ld, dxm.ptr, dxm.ld, N, H, W, Cc, 1, acc, _s()) == 0
        ref, mag = R.upsample2x_backward(dy, old if acc else None)
        # upsample2x_bwd_kernel: the old content + four gradients added in fp32 (k32 = 5), one rounding at the store (k16 = 1)
        R.check(dxm.get(), ref, R.bound(ref, k16=1, k32=5, mag=mag), f"upsample2x backward acc={acc}")
        assert dxm.outside_unchanged()
    assert dym.unchanged()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("npix", [1, 7, 300])
def test_add_two_three_inputs_and_in_place(L, npix, layout):
    """dy_add bit-equal to the same chain in IEEE fp32: ((a + b) -> f16) + c -> f16; each input with its own pitch; in place (y == a) as
    Engine.add's backward and conv_bias call it."""
    Cc = 24
    g = R.gen(npix)
    a, b, c = (R.randn16(g, npix, Cc).half() for _ in range(3))
    am, bm, cm = Map((npix, Cc), a, layout, pad=8), Map((npix, Cc), b, layout, pad=16), Map((npix, Cc), c, layout, pad=24)
    for third in (None, cm):
        ym = Map((npix, Cc), None, layout, pad=32)
        assert L.dy_add(am.ptr, am.ld, bm.ptr, bm.ld, 0 if third is None else cm.ptr, 0 if third is None else cm.ld, ym.ptr, ym.ld, npix, Cc, _s()) == 0
        R.same_bits(ym.get(), R.add_f32_chain(a, b, None if third is None else c), f"add {2 if third is None else 3} inputs")
        assert ym.outside_unchanged() and am.unchanged() and bm.unchanged() and cm.unchanged()
    assert L.dy_add(am.ptr, am.ld, bm.ptr, bm.ld, 0, 0, am.ptr, am.ld, npix, Cc, _s()) == 0
    R.same_bits(am.get(), R.add_f32_chain(a, b), "add in place")
    assert am.outside_unchanged() and bm.unchanged()


@pytest.mark.parametrize("npix", [1, 300])
def test_copy_slice_to_slice(L, npix):
    Cc = 24
    x = R.randn16(R.gen(npix), npix, Cc)
    xm, ym = Map((npix, Cc), x, "slice", pad=8), Map((npix, Cc), None, "slice", pad=16)
    assert L.dy_copy_slice(xm.ptr, xm.ld, ym.ptr, ym.ld, npix, Cc, _s()) == 0
    R.same_bits(ym.get(), x.half(), "copy_slice")
    assert ym.outside_unchanged() and xm.unchanged()
    dm = Map((npix, Cc))
    assert L.dy_copy_slice(xm.ptr, xm.ld, dm.ptr, dm.ld, npix, Cc, _s()) == 0
    R.same_bits(dm.get(), x.half(), "copy_slice to a dense map")


# =====================================================================================================================================
# 5. Zoom_cat's 2x2 max + mean pool
# =====================================================================================================================================
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("variant", ["random", "ties"])
@pytest.mark.parametrize("Cc", [8, 24])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (8, 8)])
def test_zoom_pool_forward_backward(L, H, W, Cc, variant, layout):
    """dy_zoom_pool against adaptive_max_pool2d + adaptive_avg_pool2d to half size in float64, dy_zoom_pool_backward against float64
    autograd of the same expression (the first arg-max takes a tie: the coarse grid makes many), accumulate 0 and 1."""
    N = 2
    g = R.gen(10 * H + W + Cc)
    x = (R.coarse16 if variant == "ties" else R.randn16)(g, N, 2 * H, 2 * W, Cc)
    xm, ym = Map((N, 2 * H, 2 * W, Cc), x, layout), Map((N, H, W, Cc), None, layout, pad=8)
    assert L.dy_zoom_pool(xm.ptr, xm.ld, ym.ptr, ym.ld, N, H, W, Cc, _s()) == 0
    ref, mean = R.zoom_pool(x)
    # zoom_pool_fwd_kernel: (f16)max is exact, the mean is rounded once and the sum once (k16 = 2: 2^-11 |mean| + 2^-11 |y|)
    R.check(ym.get(), ref, R.bound(ref, k16=1, abs16=mean.abs()), "zoom_pool forward")
    assert xm.unchanged() and ym.outside_unchanged()
    dy, old = R.randn16(g, N, H, W, Cc), R.randn16(g, N, 2 * H, 2 * W, Cc)
    dym = Map((N, H, W, Cc), dy, layout)
    for acc in (0, 1):
        dxm = Map((N, 2 * H, 2 * W, Cc), old, layout, pad=8)
        assert L.dy_zoom_pool_backward(xm.ptr, xm.ld, dym.ptr, dym.ld, dxm.ptr, dxm.ld, N, H, W, Cc, acc, _s()) == 0
        gref, mag = R.zoom_pool_backward(x, dy, old if acc else None)
        # zoom_pool_bwd_kernel: g * 0.25 or g * 1.25 is exact in fp32; one addition of the old content (k32 = 1), one rounding (k16 = 1)
        R.check(dxm.get(), gref, R.bound(gref, k16=1, k32=1, mag=mag), f"zoom_pool backward acc={acc}")
        assert dxm.outside_unchanged()
    assert xm.unchanged() and dym.unchanged()
