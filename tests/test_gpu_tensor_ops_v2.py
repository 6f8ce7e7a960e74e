"""-m gpu: the streaming ScalSeq backward kernel (scalseq_bwd_v2_kernel) and the integer-key SPPF forward kernel (sppf_pool3_fwd_v2_kernel)
of csrc/tensor_ops.hip against the kernels they replaced, which DY_TENSOR_OPS_V1=1 selects at every call: both run in this process on the
same buffers and every output must have the SAME BITS -- the partial sums (BatchNorm statistics: DESIGN 4.9), every written row of them
with a canary behind nparts, dr0 / dr1 / dr2; y1..y3 and the three arg-max maps.  The float64 / ATen references of
tests/test_gpu_tensor_ops.py keep checking the values; this file checks that the new kernels did not move a single bit."""
import ctypes as C
import functools
import math
import os

import pytest
import torch

import tensor_ops_ref as R
from test_gpu_tensor_ops import CANARY, ENGINE_PARTIALS, POOL_SHAPES, Map, _arg_buffer, _dev, _partials, _s

pytestmark = pytest.mark.gpu

SWITCH = "DY_TENSOR_OPS_V1"
COLS_SHAPES = [(2, 8, 16, 32), (2, 8, 48, 32), (2, 8, 64, 8), (2, 8, 32, 16), (2, 8, 16, 64), (2, 4, 4, 128)]
BLOCK_SHAPE = (2, 8, 12, 24)
VIRTUAL_SHAPE = (4, 16, 64, 32)  # 4 x 4 x 4 = 64 wave items -> 16 virtual blocks of 4 waves


@pytest.fixture(scope="module")
def L():
    from ultralytics.hip.engine import Engine
    return Engine("cuda:0").L


@pytest.fixture(autouse=True)
def _switch_off():
    """Every test starts and ends on the new path with the default grid."""
    os.environ.pop(SWITCH, None)
    yield
    os.environ.pop(SWITCH, None)


def _use_v1(on):
    if on:
        os.environ[SWITCH] = "1"  # os.environ writes through to the C environment the library reads
    else:
        os.environ.pop(SWITCH, None)


@functools.lru_cache(maxsize=None)
def _inputs(shape, exact):
    r, dy, coef = R.scalseq_inputs(R.seed_of(shape, exact), *shape, exact=exact)
    g = R.gen(99)
    bw = torch.stack([0.05 * torch.randn(shape[3], generator=g), 0.05 * torch.randn(shape[3], generator=g)]).float()
    return r, dy, coef, bw


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _run(L, shape, exact, maxp, layout, v1, cap=0):
    """Both modes of dy_scalseq_tail_backward_all on fresh canary-filled outputs: (nparts, partials buffer, the three dr buffers)."""
    N, H, W, Cc = shape
    r, dy, coef, bw = _inputs(shape, exact)
    rm = [Map((N, H >> l, W >> l, Cc), r[l], layout, pad=8) for l in range(3)]
    dym = Map(shape, dy, layout, pad=8)
    rargs = (rm[0].ptr, rm[0].ld, rm[1].ptr, rm[1].ld, rm[2].ptr, rm[2].ld, dym.ptr, dym.ld)
    cd, bd = _dev(coef), _dev(bw)
    part = _partials(Cc, ENGINE_PARTIALS)
    dr = [Map((N, H >> l, W >> l, Cc), None, layout, pad=8) for l in range(3)]
    n = C.c_int(0)
    _use_v1(v1)
    old = L.dy_scalseq_bwd_grid_cap(cap)
    try:
        assert L.dy_scalseq_tail_backward_all(*rargs, 0, 0, 0, 0, 0, 0, cd.data_ptr(), 0, part.data_ptr(), maxp, N, H, W, Cc, 0, C.byref(n), _s()) == 0
        assert L.dy_scalseq_tail_backward_all(*rargs, dr[0].ptr, dr[0].ld, dr[1].ptr, dr[1].ld, dr[2].ptr, dr[2].ld, cd.data_ptr(), bd.data_ptr(),
                                              0, 0, N, H, W, Cc, 1, None, _s()) == 0
        torch.cuda.synchronize()
    finally:
        L.dy_scalseq_bwd_grid_cap(old)
        _use_v1(False)
    assert all(m.unchanged() for m in rm) and dym.unchanged()
    assert 1 <= n.value <= maxp
    assert bool((part[n.value * 2 * Cc:] == CANARY).all()), "partials written past nparts"
    assert all(d.outside_unchanged() for d in dr)
    return n.value, part.cpu(), [d.full.cpu() for d in dr]


def _same(a, b, what):
    assert a[0] == b[0], f"{what}: nparts {a[0]} != {b[0]}"
    assert torch.equal(_bits(a[1]), _bits(b[1])), f"{what}: partials differ in {int((_bits(a[1]) != _bits(b[1])).sum())} words"
    for l in range(3):
        assert torch.equal(_bits(a[2][l]), _bits(b[2][l])), f"{what}: dr{l} differs in {int((_bits(a[2][l]) != _bits(b[2][l])).sum())} values"


@pytest.mark.parametrize("layout", ["dense", "slice"])
@pytest.mark.parametrize("maxp", [ENGINE_PARTIALS, 3, 1])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "realistic"])
@pytest.mark.parametrize("shape", COLS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scalseq_streaming_kernel_keeps_every_bit(L, shape, exact, maxp, layout):
    """Every width of the cols path (cpp = 1, 2, 4 -- the DPP path --, 8, 16), both input regimes, max_partials at the engine's value and
    at 3 and 1 (virtual blocks that iterate), dense maps and channel slices of wider buffers."""
    assert R.scalseq_kernel(shape[2], shape[3]) == "cols"
    new = _run(L, shape, exact, maxp, layout, v1=False)
    _same(new, _run(L, shape, exact, maxp, layout, v1=True), f"{shape} exact={exact} max_partials={maxp} {layout}")
    assert bool((new[1][: new[0] * 2 * shape[3]] != CANARY).all()), "a partial row below nparts was not written"


@pytest.mark.parametrize("cap", [1, 2, 5])
def test_scalseq_virtual_blocks_walked_by_one_workgroup(L, cap):
    """64 items = 16 virtual blocks; with the physical grid capped at 1, 2 and 5 workgroups one workgroup reduces several virtual blocks in
    turn (what the step's shape does about twice per workgroup): the same bits as the uncapped run and as the old kernel."""
    free = _run(L, VIRTUAL_SHAPE, False, ENGINE_PARTIALS, "dense", v1=False)
    assert free[0] == 16
    _same(_run(L, VIRTUAL_SHAPE, False, ENGINE_PARTIALS, "dense", v1=False, cap=cap), free, f"cap {cap} vs uncapped")
    _same(free, _run(L, VIRTUAL_SHAPE, False, ENGINE_PARTIALS, "dense", v1=True), "uncapped vs old kernel")
    # fewer partial rows than items / 4: a virtual block iterates as well
    _same(_run(L, VIRTUAL_SHAPE, True, 6, "dense", v1=False, cap=cap), _run(L, VIRTUAL_SHAPE, True, 6, "dense", v1=True), f"cap {cap}, 6 partial rows")


def test_scalseq_block_kernel_is_unchanged(L):
    """A shape the selection rule gives to scalseq_bwd_all_kernel: the switch changes nothing there."""
    assert R.scalseq_kernel(BLOCK_SHAPE[2], BLOCK_SHAPE[3]) == "block"
    for exact in (True, False):
        _same(_run(L, BLOCK_SHAPE, exact, ENGINE_PARTIALS, "slice", v1=False), _run(L, BLOCK_SHAPE, exact, ENGINE_PARTIALS, "slice", v1=True),
              f"block kernel exact={exact}")


@pytest.mark.parametrize("shape", [(2, 8, 16, 32), VIRTUAL_SHAPE], ids=["2x8x16x32", "4x16x64x32"])
def test_scalseq_streaming_kernel_replays_bitwise(L, shape):
    """The new kernel twice on the same inputs: bit-equal outputs (no atomics, no order that depends on scheduling)."""
    _same(_run(L, shape, False, ENGINE_PARTIALS, "dense", v1=False), _run(L, shape, False, ENGINE_PARTIALS, "dense", v1=False), f"replay {shape}")


# =====================================================================================================================================
# SPPF pools: dy_sppf_pool3 (new kernel) and dy_sppf_pool3_backward (unchanged, run after either forward) against the switch
# =====================================================================================================================================
SPPF_CASES = [(2, *c) for c in POOL_SHAPES] + [(1, 16, 40, 40), (1, 128, 40, 40), (1, 16, 44, 44)]  # N, C, H, W
SPPF_VARIANTS = ["ties", "nan", "zeros", "ninf", "partial", "random"]
NINF = float("-inf")


@functools.lru_cache(maxsize=None)
def _sppf_input(N, Cc, H, W, variant):
    g = R.gen(7 * H + 3 * W + Cc)
    if variant == "random":
        return R.randn16(g, N, H, W, Cc)
    x = R.coarse16(g, N, H, W, Cc)  # the tie-forcing grid
    if variant == "nan":  # two NaNs in one window, one on the border, one in a corner
        x[0, H // 2, W // 2, 3] = float("nan")
        x[0, H // 2, min(W // 2 + 1, W - 1), 3] = float("nan")
        x[N - 1, H - 1, W // 2, 0] = float("nan")
        x[0, 0, 0, Cc - 1] = float("nan")
    if variant == "zeros":  # +0, -0 and -inf: ties between the two zeros, windows that hold nothing but -inf (border and interior)
        pick = torch.randint(0, 5, x.shape, generator=g)
        x = torch.where(pick == 0, torch.zeros_like(x), x)
        x = torch.where(pick == 1, -torch.zeros_like(x), x)
        x = torch.where(pick == 2, torch.full_like(x, NINF), x)
        x[:, : (H + 1) // 2, : (W + 1) // 2, : Cc // 2] = NINF
        x[:, H - 1, W - 1, :] = -0.0
    if variant in ("ninf", "partial"):
        # -inf and +0 but no -0 and no NaN, so the workgroups stay on the key passes: -inf scattered among finite values (its key against
        # theirs, its inverse key), and a quadrant of nothing but -inf (windows on the border and in the interior: code 0)
        pick = torch.randint(0, 5, x.shape, generator=g)
        x = torch.where(pick == 0, torch.zeros_like(x), x)
        x = torch.where(pick == 2, torch.full_like(x, NINF), x)
        x[:, : (H + 1) // 2, : (W + 1) // 2, : Cc // 2] = NINF
        assert not bool(((x == 0) & torch.signbit(x)).any()) and not bool(torch.isnan(x).any())
        if variant == "partial":  # a -0 in ONE workgroup's tile (image 0, first 8 channels): the old passes and the key passes in one launch
            x[0, H - 1, W - 1, 0] = -0.0
    return x


def _sppf_run(L, case, variant, layout, v1, with_args=True):
    """Forward, then the backward with three settings of the accumulate flags: every buffer that was written, on the CPU."""
    N, Cc, H, W = case
    x = _sppf_input(N, Cc, H, W, variant)
    shape, cshape = (N, H, W, Cc), (N, H, W, 4 * Cc)
    cat = Map(cshape, torch.cat([x, torch.full((N, H, W, 3 * Cc), CANARY, dtype=torch.float64)], -1), layout)
    args = [_arg_buffer(N * H * W, Cc) for _ in range(3)]
    ap = [t.data_ptr() if with_args else 0 for t in args]
    g = R.gen(11)
    dcat = R.randn16(g, *cshape)
    _use_v1(v1)
    try:
        assert L.dy_sppf_pool3(cat.ptr, cat.ld, Cc, ap[0], ap[1], ap[2], N, H, W, _s()) == 0
        torch.cuda.synchronize()
        out = [cat.full.cpu()] + [t.cpu() for t in args]
        assert cat.outside_unchanged()
        n = math.prod(shape)
        assert all(bool((t[n:] == 99).all()) for t in out[1:]), "arg-max map written past its end"
        if with_args:
            for acc in ((1, 1, 1), (0, 1, 1), (1, 0, 1)):
                gm = Map(cshape, dcat, layout)
                assert L.dy_sppf_pool3_backward(gm.ptr, gm.ld, Cc, ap[0], ap[1], ap[2], N, H, W, *acc, _s()) == 0
                torch.cuda.synchronize()
                assert gm.outside_unchanged()
                out.append(gm.full.cpu())
        else:
            assert all(bool((t == 99).all()) for t in out[1:]), "a NULL arg-max map was written"
    finally:
        _use_v1(False)
    return out


def _same_list(a, b, what):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        ub, vb = (u.view(torch.int16), v.view(torch.int16)) if u.dtype == torch.float16 else (u, v)
        assert torch.equal(ub, vb), f"{what}: buffer {i} differs in {int((ub != vb).sum())} elements"


@pytest.mark.parametrize("variant", SPPF_VARIANTS)
@pytest.mark.parametrize("case", SPPF_CASES, ids=lambda c: "x".join(map(str, c)))
def test_sppf_new_kernels_keep_every_bit(L, case, variant):
    """y1..y3, the three arg-max maps and the chained backward (three settings of its accumulate flags) under both settings of the switch,
    on channel slices of a canary-filled buffer: POOL_SHAPES, the step's 40 x 40 map with one and with eight channel groups, and 44 x 44
    (16 channels per workgroup only in the old kernel's LDS layout, so that case compares the old kernel with itself).  Inputs: a
    tie-forcing grid; NaNs (two in one window, border, corner); +0 / -0 / -inf with windows of nothing but -inf ("zeros": every workgroup
    holds a -0 and runs the old passes); the same without any -0 ("ninf": every workgroup runs the key passes) and with a -0 in one
    workgroup's tile only ("partial"); random values."""
    N, Cc, H, W = case
    assert L.dy_sppf_pool3_supported(H, W, Cc) in (8, 16)
    new = _sppf_run(L, case, variant, "slice", v1=False)
    _same_list(new, _sppf_run(L, case, variant, "slice", v1=True), f"sppf {case} {variant}")
    if variant in ("zeros", "ninf", "partial"):  # what the "same bits" are worth: against ATen's chain on the same special values
        x = _sppf_input(N, Cc, H, W, variant)
        ys, codes = [x], []
        for _ in range(3):
            y, code, _ = R.maxpool5(ys[-1])
            ys.append(y); codes.append(code)
        got = new[0][..., 8:8 + 4 * Cc]
        R.same_bits(got, torch.cat(ys, -1).half(), f"sppf y1..y3 on {variant}")
        n = N * H * W * Cc
        for l in range(3):  # ATen's window code wherever the window holds a number; 0 where it holds nothing but -inf (dy_maxpool5's rule)
            got_code = new[1 + l][:n].view(N, H, W, Cc)
            empty = ys[l + 1] == NINF
            assert bool((~empty).any()) and (l > 0 or min(H, W) < 11 or bool(empty.any()))  # the -inf quadrant outlasts pool 0 on the larger maps
            assert torch.equal(got_code[~empty], codes[l][~empty].to(got_code.dtype)), f"sppf arg-max {l} on {variant}"
            assert bool((got_code[empty] == 0).all()), f"sppf arg-max {l}: an all -inf window must keep code 0"


@pytest.mark.parametrize("variant", ["ties", "nan"])
def test_sppf_forward_without_arg_maps(L, variant):
    """Eval (arg[l] == NULL): the same y1..y3, nothing written to the maps."""
    case = (2, 24, 11, 13)
    new = _sppf_run(L, case, variant, "dense", v1=False, with_args=False)
    _same_list(new, _sppf_run(L, case, variant, "dense", v1=True, with_args=False), f"sppf eval {variant}")
    _same_list(new[:1], _sppf_run(L, case, variant, "dense", v1=False)[:1], "sppf y1..y3 with and without arg maps")


def test_sppf_unsupported_map_gets_the_same_answer(L):
    """A map that does not fit in LDS: dy_sppf_pool3_supported says 0 (the engine then chains dy_maxpool5) and both entries refuse it,
    whatever the switch says."""
    H, W, Cc = 80, 80, 16
    assert L.dy_sppf_pool3_supported(H, W, Cc) == 0
    cat = Map((1, H, W, 4 * Cc), None, "dense")
    args = [_arg_buffer(H * W, Cc) for _ in range(3)]
    for v1 in (False, True):
        _use_v1(v1)
        try:
            rc = (L.dy_sppf_pool3(cat.ptr, cat.ld, Cc, *[t.data_ptr() for t in args], 1, H, W, _s()),
                  L.dy_sppf_pool3_backward(cat.ptr, cat.ld, Cc, *[t.data_ptr() for t in args], 1, H, W, 1, 1, 1, _s()))
        finally:
            _use_v1(False)
        assert rc[0] != 0 and rc[1] != 0
    assert cat.unchanged()


def test_sppf_new_forward_replays_bitwise(L):
    case = (1, 16, 40, 40)
    for variant in ("ties", "nan"):  # the key passes, and the workgroup that meets a NaN
        _same_list(_sppf_run(L, case, variant, "dense", v1=False), _sppf_run(L, case, variant, "dense", v1=False), f"sppf replay {variant}")
