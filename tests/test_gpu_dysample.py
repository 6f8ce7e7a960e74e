"""-m gpu: DySample (learned dynamic up-sampling, reference nn/extra_modules/block.py:3819-3892, style 'lp') on the HIP path.

1. the sampler kernels (csrc/dysample.hip) per element against the reference's float64 values (tests/golden/dysample_kernel.npz,
   dysample_big_*.npz), dense and on channel slices, under the rule of tests/tensor_ops_ref.py

       |got - ref| <= k16 * 2^-11 * |ref| + k32 * 2^-23 * mag + 2^-23 * 4 (W + H) * dcoord + 2^-24

   mag = the sum of |terms| of the element, dcoord = |d value / d coordinate| (both from tests/dysample_ref.py, which
   tests/test_host_dysample.py holds to the same float64 values): the coordinate term covers the fp32 ``w + (0.25 o + init)``, two
   roundings of at most 2^-24 (W + H) each.  k16 / k32 count the kernel's own roundings:
     forward   k16 = 1 (the fp16 store; x is exact)        k32 = 8: 1 - f (1), weight product (1), four products and three adds (<= 7,
                                                            fewer with fused multiply-adds), on terms each bounded by mag
     d(o)      k16 = 1 (the fp16 store)                    k32 = 16: per term 1 - f, two products, their sum and the product with dy
                                                            (<= 5 half-ulps of mag in total over the sum) + one add per channel of the
                                                            group (<= 16 channels here: 8 ulps) -- differences of fp16 values are exact
     dx        k16 = 1 (the fp16 store; with accumulate    k32 = 64: 1 - f, row weight, row * column (3) + one multiply-add per term,
               the old value joins mag)                     <= 120 terms per element (asserted by the generator): 60 ulps; the far
                                                            side pass adds the same terms in another order and one more add to fold in
2. the far path at rmax = 1 (every displaced sample goes through the atomics) and 2, and bit-repeatability of the bounded cases;
3. refusals; 4. the module against the reference at 4 x the generator's measured tolerances; 5. the graph: eval / fused eval /
InferPlan, one training step, captured = eager, freeze=, a reference-written checkpoint, augment=True, the public trainer -- at the
bounds tests/test_gpu_spd.py and tests/test_gpu_model.py apply to the LD graphs (DySample shares LDConv's piecewise-linear sampling,
and with it the isolated flips under fp16)."""
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

import dysample_ref as R
from conftest import CFG_DIR
from dysample_util import (BIG, BOUNDED_CASES, CKPT, DYSAMPLE_LAYERS, GROUPS, KERNEL_CASES, MODEL, MODULE_CASES, SLICE, ZERO_CASE, batch,
                           fetch, kernel_inputs, state)
from golden.cases import rnd
from gpu_util import l2err, relerr, run_fwd_bwd

pytestmark = pytest.mark.gpu
DY_ERR_ARG, DY_ERR_ALIGN = -1, -3  # include/dealyolo_hip.h
POISON = -1234.0  # exactly representable in fp16
K = dict(y=(1, 8), doff=(1, 16), dx=(1, 64))  # (k16, k32), counted in the docstring above
_REF = {}


# ----------------------------------------------------------------------------- helpers
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _store(t, extra=0, c0=0):
    """fp16 device storage (..., C + extra), POISON outside channels [c0, c0 + C), holding ``t`` inside."""
    C = t.shape[-1]
    s = torch.full((*t.shape[:-1], C + extra), POISON, dtype=torch.float16)
    s[..., c0:c0 + C] = t.half()
    return s.cuda()


def _outside_untouched(s, c0, C):
    return bool((s[..., :c0] == POISON).all()) and bool((s[..., c0 + C:] == POISON).all())


def _fwd(x, cx, off, y, cy, C, s, G=GROUPS):
    from ultralytics.hip import lib
    N, H, W = off.shape[:3]
    return lib().dy_dysample(x.data_ptr() + 2 * cx, x.shape[-1], off.data_ptr(), off.shape[-1], y.data_ptr() + 2 * cy, y.shape[-1],
                             N, H, W, C, G, s, _stream())


def _bwd(x, cx, off, dy, cy, dx, cdx, doff, C, s, accumulate=0, rmax=2, G=GROUPS, scratch=None, dx32=None):
    from ultralytics.hip import lib
    N, H, W = off.shape[:3]
    if dx is not None:
        dx32 = torch.full((N * H * W * C,), float("nan"), device="cuda") if dx32 is None else dx32  # need not be zeroed
        scratch = torch.full((4,), 0x7fffffff, dtype=torch.int32, device="cuda") if scratch is None else scratch
    rc = lib().dy_dysample_backward(x.data_ptr() + 2 * cx, x.shape[-1], off.data_ptr(), off.shape[-1], dy.data_ptr() + 2 * cy, dy.shape[-1],
                                    0 if dx is None else dx.data_ptr() + 2 * cdx, 0 if dx is None else dx.shape[-1], accumulate,
                                    0 if dx is None else dx32.data_ptr(), 0 if doff is None else doff.data_ptr(),
                                    0 if doff is None else doff.shape[-1], 0 if dx is None else scratch.data_ptr(), rmax,
                                    N, H, W, C, G, s, _stream())
    torch.cuda.synchronize()  # (keeps dx32 / scratch alive until the launches have run)
    return rc


def _case(golden, name):
    """Inputs, float64 reference values and bound magnitudes of a kernel case, computed once and shared."""
    if name not in _REF:
        G = golden("dysample_kernel")
        C, s, H, W = {**KERNEL_CASES, **BOUNDED_CASES}[name]
        x, off, dy = kernel_inputs(C, s, H, W, int(G[f"ker/{name}/seed"]), bounded=name in BOUNDED_CASES)
        fw, bw = R.forward(x, off, s, GROUPS), R.backward(x, off, dy, s, GROUPS)
        ref = dict(y=fw["y"], dx=bw["dx"], doff=bw["doff"])
        if name in KERNEL_CASES:  # the reference's own float64 values (the restatement equals them to 1e-11: tests/test_host_dysample.py)
            ref = {k: fetch(G, f"ker/{name}/{k}").double() for k in ref}
        mag = dict(y=(fw["mag"], fw["dcoord"]), dx=(bw["dx_mag"], bw["dx_dcoord"]), doff=(bw["doff_mag"], bw["doff_dcoord"]))
        _REF[name] = (x, off, dy, C, s, H, W, ref, mag)
    return _REF[name]


def _check(what, got, ref, mag, dcoord, H, W, extra=None):
    """The per-element bound of the module docstring; NO element is left out."""
    k16, k32 = K[what]
    got, ref = got.double().cpu(), ref.double()
    if extra is not None:  # accumulate: the old value is one more term
        ref, mag = ref + extra.double(), mag + extra.double().abs()
    bound = k16 * 2.0 ** -11 * ref.abs() + k32 * 2.0 ** -23 * mag + 2.0 ** -23 * 4 * (W + H) * dcoord + 2.0 ** -24
    err = (got - ref).abs()
    worst = float((err / bound).max())
    print(f"{what}: max err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, f"{what}: {int((err > bound).sum())} of {err.numel()} elements beyond the bound"


VARIANTS = {"dense": (0, 0, 0, 0), "sliced": (SLICE["x_off"], SLICE["x_extra"], SLICE["y_off"], SLICE["y_extra"])}


# ----------------------------------------------------------------------------- 1. the kernels, per element
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_forward_per_element(golden, name, variant):
    x, off, dy, C, s, H, W, ref, mag = _case(golden, name)
    cx, ex, cy, ey = VARIANTS[variant]
    xs, ys = _store(x, ex, cx), _store(torch.zeros(x.shape[0], s * H, s * W, C) + POISON, ey, cy)
    x0 = xs.clone()
    assert _fwd(xs, cx, off.cuda(), ys, cy, C, s) == 0
    torch.cuda.synchronize()
    _check("y", ys[..., cy:cy + C], ref["y"], *mag["y"], H, W)
    assert _outside_untouched(ys, cy, C) and torch.equal(xs, x0)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_backward_per_element(golden, name, variant):
    """dx and d(o) at the default rmax = 2; accumulate = 1 adds; dx == NULL and doff == NULL skip without touching the other output."""
    x, off, dy, C, s, H, W, ref, mag = _case(golden, name)
    cx, ex, cy, ey = VARIANTS[variant]
    nch = off.shape[-1]
    xs, dys, offd = _store(x, ex, cx), _store(dy, ey, cy), off.cuda()

    def outputs():
        return _store(torch.zeros_like(x.float()) + POISON, ex, cx), torch.full((*off.shape[:3], nch + 8), POISON, dtype=torch.float16, device="cuda")

    dxs, doff = outputs()
    assert _bwd(xs, cx, offd, dys, cy, dxs, cx, doff, C, s) == 0
    _check("dx", dxs[..., cx:cx + C], ref["dx"], *mag["dx"], H, W)
    _check("doff", doff[..., :nch], ref["doff"], *mag["doff"], H, W)
    assert _outside_untouched(dxs, cx, C) and bool((doff[..., nch:] == POISON).all())
    # accumulate = 1: one fp16 rounding of (old value + gradient); doff is written, not accumulated
    dxa, doffa = outputs()
    prev = torch.from_numpy(np.random.default_rng(7).standard_normal(tuple(x.shape)).astype(np.float16))
    dxa[..., cx:cx + C] = prev.cuda()
    assert _bwd(xs, cx, offd, dys, cy, dxa, cx, doffa, C, s, accumulate=1) == 0
    _check("dx", dxa[..., cx:cx + C], ref["dx"], *mag["dx"], H, W, extra=prev)
    assert torch.equal(doffa, doff) and _outside_untouched(dxa, cx, C)
    # dx == NULL: the offset gradient alone, the same bits;  doff == NULL: the input gradient alone, the same bits class
    dxn, doffn = outputs()
    assert _bwd(xs, cx, offd, dys, cy, None, 0, doffn, C, s) == 0
    assert torch.equal(doffn, doff) and bool((dxn == POISON).all())
    dxm, doffm = outputs()
    assert _bwd(xs, cx, offd, dys, cy, dxm, cx, None, C, s) == 0
    _check("dx", dxm[..., cx:cx + C], ref["dx"], *mag["dx"], H, W)
    assert bool((doffm == POISON).all()) and _outside_untouched(dxm, cx, C)


# ----------------------------------------------------------------------------- 2. far path and repeatability
@pytest.mark.parametrize("rmax", [1, 2])
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_far_path_meets_the_bound_at_either_radius(golden, name, rmax):
    """The displaced cases (a quarter of their samples have |0.25 o| > 1, all of them > 0): at rmax = 1 every sample takes the atomic side
    pass, at rmax = 2 the far quarter does.  The side accumulator arrives as NaN: the launch zeroes it itself."""
    x, off, dy, C, s, H, W, ref, mag = _case(golden, name)
    assert float(((0.25 * off).abs() > 1.0).float().mean()) > 0.01
    dxs = _store(torch.zeros_like(x.float()) + POISON)
    assert _bwd(_store(x), 0, off.cuda(), _store(dy), 0, dxs, 0, None, C, s, rmax=rmax) == 0
    _check("dx", dxs, ref["dx"], *mag["dx"], H, W)


@pytest.mark.parametrize("name", list(BOUNDED_CASES))
def test_bounded_offsets_repeat_bit_for_bit(golden, name):
    """|0.25 o| <= 0.9 <= rmax - 1: no far sample, so the side accumulator stays untouched and two calls give the same bits."""
    x, off, dy, C, s, H, W, ref, mag = _case(golden, name)
    assert float((0.25 * off).abs().max()) <= 0.9
    xs, dys, offd = _store(x), _store(dy), off.cuda()
    outs = []
    for _ in range(2):
        dxs = _store(torch.zeros_like(x.float()) + POISON)
        doff = torch.full(tuple(off.shape), POISON, dtype=torch.float16, device="cuda")
        dx32 = torch.full((x.numel(),), 3.0, device="cuda")
        assert _bwd(xs, 0, offd, dys, 0, dxs, 0, doff, C, s, dx32=dx32) == 0
        assert bool((dx32 == 3.0).all())
        outs.append((dxs.clone(), doff.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    _check("dx", outs[0][0], ref["dx"], *mag["dx"], H, W)
    _check("doff", outs[0][1], ref["doff"], *mag["doff"], H, W)
    ys = _store(torch.zeros_like(dy.float()) + POISON)
    assert _fwd(xs, 0, offd, ys, 0, C, s) == 0
    torch.cuda.synchronize()
    _check("y", ys, ref["y"], *mag["y"], H, W)


# ----------------------------------------------------------------------------- 3. refusals
def test_refusals_launch_nothing():
    from ultralytics.hip import lib
    L = lib()
    N, H, W, C, s = 1, 4, 4, 32, 2
    x = torch.full((N, H, W, C), POISON, dtype=torch.float16, device="cuda")
    off = torch.zeros(N, H, W, 2 * GROUPS * 9, device="cuda")
    y = torch.full((N, 4 * H, 4 * W, C), POISON, dtype=torch.float16, device="cuda")
    doff = torch.full((N, H, W, 2 * GROUPS * 9 + 8), POISON, dtype=torch.float16, device="cuda")
    dx32, scratch = torch.zeros(N * H * W * C, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    st = _stream()

    def fwd(xp=None, ldx=C, yp=None, ldy=C, C_=C, G=GROUPS, s_=s, ldoff=32):
        return L.dy_dysample(x.data_ptr() if xp is None else xp, ldx, off.data_ptr(), ldoff, y.data_ptr() if yp is None else yp, ldy, N, H, W,
                             C_, G, s_, st)

    def bwd(xp=None, ldx=C, dxp=None, lddx=C, doffp=None, lddoff=40, C_=C, G=GROUPS, s_=s, rmax=2, d32=None, scr=None):
        return L.dy_dysample_backward(x.data_ptr() if xp is None else xp, ldx, off.data_ptr(), 32, y.data_ptr(), C,
                                      x.data_ptr() if dxp is None else dxp, lddx, 0, dx32.data_ptr() if d32 is None else d32,
                                      doff.data_ptr() if doffp is None else doffp, lddoff, scratch.data_ptr() if scr is None else scr, rmax,
                                      N, H, W, C_, G, s_, st)

    assert fwd(s_=3, ldoff=72) == DY_ERR_ARG and bwd(s_=3) == DY_ERR_ARG                      # scale 3
    assert fwd(C_=24, ldx=24, ldy=24) == DY_ERR_ARG and bwd(C_=24, ldx=24, lddx=24) == DY_ERR_ARG  # 24 channels in 4 groups
    assert fwd(xp=0) == DY_ERR_ARG and fwd(yp=0) == DY_ERR_ARG and bwd(xp=0) == DY_ERR_ARG    # null pointers
    assert bwd(d32=0) == DY_ERR_ARG and bwd(scr=0) == DY_ERR_ARG and bwd(rmax=0) == DY_ERR_ARG and bwd(rmax=17) == DY_ERR_ARG
    assert fwd(ldx=C + 4) == DY_ERR_ALIGN and fwd(ldy=C + 1) == DY_ERR_ALIGN                  # odd pitches
    assert bwd(lddx=C + 4) == DY_ERR_ALIGN and bwd(lddoff=36) == DY_ERR_ALIGN and bwd(ldx=C + 2) == DY_ERR_ALIGN
    assert fwd(xp=x.data_ptr() + 8) == DY_ERR_ALIGN and fwd(yp=y.data_ptr() + 2) == DY_ERR_ALIGN  # pointers off a 16-byte boundary
    assert bwd(dxp=x.data_ptr() + 8) == DY_ERR_ALIGN and bwd(doffp=doff.data_ptr() + 4) == DY_ERR_ALIGN
    assert fwd(ldoff=24) == DY_ERR_ARG and bwd(lddoff=24) == DY_ERR_ARG                       # pitches below the channel count
    torch.cuda.synchronize()
    assert bool((x == POISON).all()) and bool((y == POISON).all()) and bool((doff == POISON).all())


def test_engine_op_rejects_an_unsupported_geometry():
    from ultralytics.hip.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        eng.dysample(None, 2, 4, eng.wrap_act(torch.zeros(1, 4, 4, 24, dtype=torch.float16, device="cuda")))


# ----------------------------------------------------------------------------- 4. the module against the reference
@pytest.mark.parametrize("case", list(MODULE_CASES) + [ZERO_CASE])
def test_module_vs_golden(golden, case):
    """l2err of y, gx and both parameter gradients below 4 x the tolerance the generator measured for the case (tol/<case>/...: the
    error of a float64 emulation of this path's fp16 storage against the same fp32 values).  The factor pays for another fp32
    summation order, not for another algorithm."""
    from ultralytics.nn.extra_modules import DySample
    G = golden("dysample")
    C, s, H, W = {**MODULE_CASES, ZERO_CASE: MODULE_CASES["ds_32_s2"]}[case]
    p = f"mod/{case}"
    seed = int(G[f"{p}/seed"])
    x, gy = rnd(10 * seed, 2, C, H, W), rnd(10 * seed + 1, 2, C, s * H, s * W)
    m = DySample(C, s, "lp", GROUPS)
    m.load_state_dict(state(G, p), strict=True)
    y, gxs, rt = run_fwd_bwd(m, [x], gy)
    got = dict(y=y, gx=gxs[0], gw=m.offset.weight.grad.float().cpu(), gb=m.offset.bias.grad.float().cpu())
    want = dict(y=fetch(G, f"{p}/y"), gx=fetch(G, f"{p}/gx"), gw=G.t(f"{p}/gp/offset.weight"), gb=G.t(f"{p}/gp/offset.bias"))
    errs = {k: l2err(got[k].reshape(want[k].shape), want[k]) for k in got}
    tols = {k: float(G[f"tol/{case}/{k}"]) for k in got}
    print(case, {k: f"{errs[k]:.2e} (4 x {tols[k]:.2e})" for k in errs})
    for k in errs:
        assert errs[k] < 4 * tols[k], k


# ----------------------------------------------------------------------------- 5. the graph against the reference
def _model(G):
    from ultralytics.nn.tasks import DetectionModel
    m = DetectionModel(os.path.join(CFG_DIR, MODEL + ".yaml"), ch=3, verbose=False)
    m.load_state_dict(state(G, MODEL), strict=True)
    return m.cuda()


def test_eval_and_fused_eval_vs_golden(golden):
    """2e-2 on boxes and on class scores (the eval bound of tests/test_gpu_spd.py for both of its graphs, LD included); the second call
    of a geometry is traced into an InferPlan, the third replays it: all three bit for bit, two dy_dysample launches in the list."""
    G = golden("dysample")
    m = _model(G).eval()
    x = G.t("batch/img").cuda()
    for key in ("y_eval", "y_eval_fused"):
        if key == "y_eval_fused":
            m.fuse()
        ref = G.t(f"{MODEL}/{key}")
        with torch.no_grad():
            y1, _ = m(x)   # walked
            assert not m._infer_plans["plans"]
            y2, _ = m(x)   # traced into a plan
            plan = m._infer_plans["plans"][(2, 3, 64, 64)]
            y3, _ = m(x)   # replayed
        torch.cuda.synchronize()
        assert sum(1 for o in plan.rec.ops if o[2] == "dy_dysample") == 2
        assert not any(o[2] == "dy_upsample2x" for o in plan.rec.ops)
        assert torch.equal(y1, y2) and torch.equal(y1, y3)
        assert y1.shape == ref.shape
        eb, ec = relerr(y1[:, :4].cpu(), ref[:, :4]), relerr(y1[:, 4:].cpu(), ref[:, 4:])
        print(f"{key}: box relerr {eb:.2e} cls relerr {ec:.2e}")
        assert eb < 2e-2 and ec < 2e-2


def test_train_step_vs_golden(golden):
    """One training step: the comparisons of tests/test_gpu_spd.py::test_train_step_vs_golden at its bounds for the LD graph."""
    from ultralytics.hip.train import StepPlan
    G = golden("dysample")
    m = _model(G).train()
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.forward_backward(batch(G))
    torch.cuda.synchronize()
    s = plan.crit.scalars.cpu()
    ref_items = G.t(f"{MODEL}/items")
    per_item = float(((s[5:8] - ref_items).abs() / ref_items.abs()).max())
    print("items", s[5:8].tolist(), ref_items.tolist(), f"worst per-item relative error {per_item:.2e}")
    assert per_item < 1.2e-2
    assert abs(float(s[8]) - float(G[f"{MODEL}/loss"])) < 5e-3 * float(G[f"{MODEL}/loss"])
    names = [str(k) for k in G[f"{MODEL}/grad_names"]]
    params = dict(m.named_parameters())
    assert all(f"model.{i}.offset.weight" in names and f"model.{i}.offset.bias" in names for i in DYSAMPLE_LAYERS)
    scale = float(plan.state[0])
    l2 = torch.stack([params[k].grad.float().norm() / scale for k in names]).cpu()
    ref = G.t(f"{MODEL}/grad_l2")
    rel = ((l2 - ref).abs() / (ref.abs() + 1e-3 * ref.abs().max())).numpy()
    print("grad-l2 rel err: median %.2e max %.2e (%s)" % (np.median(rel), rel.max(), names[int(rel.argmax())]))
    for i in DYSAMPLE_LAYERS:
        for k in (f"model.{i}.offset.weight", f"model.{i}.offset.bias"):
            print(k, f"l2 {float(l2[names.index(k)]):.4e} reference {float(ref[names.index(k)]):.4e}")
    assert np.median(rel) < 1e-2 and rel.max() < 0.2
    first = params[names[0]].grad.float().cpu() / scale
    ef = l2err(first, G.t(f"{MODEL}/grad_first"))
    print(f"grad_first err {ef:.3e}")
    assert ef < 0.15
    sd = m.state_dict()
    rm = [str(k) for k in G[f"{MODEL}/run_mean_names"]]
    assert relerr(torch.stack([sd[k].sum() for k in rm]).cpu(), G.t(f"{MODEL}/run_mean_sum")) < 5e-3
    assert relerr(torch.stack([sd[k.replace("mean", "var")].sum() for k in rm]).cpu(), G.t(f"{MODEL}/run_var_sum")) < 5e-3
    assert torch.isfinite(plan.rt.flat_g).all() and float(plan.state[2]) == 0.0


def test_captured_step_equals_the_eager_step(golden):
    """One StepPlan step replayed as a hipGraph against the eager tape step of another plan on the same state and batch: the same
    launches.  The golden state has far samples (|0.25 o| > 1), whose scatter adds with fp32 atomics: equal to their order, the
    bound of the LD graphs in tests/test_gpu_spd.py."""
    from ultralytics.hip.train import StepPlan
    G = golden("dysample")
    outs = []
    for graph in (False, True):
        m = _model(G).train()
        plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0, use_graph=graph)
        sd0 = {k: v.clone() for k, v in m.state_dict().items()}
        plan.forward_backward(batch(G))
        if graph:
            assert plan.graph_fb is not None
            m.load_state_dict(sd0)
            plan.forward_backward(batch(G))  # the captured graph's replay
        torch.cuda.synchronize()
        ops = [o[2] for o in plan.rec_fb.ops if o[0] is not None]
        assert ops.count("dy_dysample") == 2 and ops.count("dy_dysample_backward") == 2 and "dy_upsample2x" not in ops
        outs.append((plan.rt.flat_g.clone(), plan.crit.scalars.clone()))
    assert torch.isfinite(outs[0][0]).all() and float(outs[0][0].abs().max()) > 0
    assert relerr(outs[0][1][5:9], outs[1][1][5:9]) < 1e-6 and relerr(outs[0][0], outs[1][0]) < 1e-4


def _backward_ops(plan):
    return plan.rec_fb.ops[:plan.fb_split], plan.rec_fb.ops[plan.fb_split:]


def _frozen_step(G, frozen):
    from ultralytics.hip.train import StepPlan
    m = _model(G).train()
    for k, v in m.named_parameters():
        v.requires_grad = k not in frozen
    start = {k: v.detach().clone() for k, v in m.state_dict().items()}
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.set_hyper([0.01] * 3, 0.9, [0.0, 5e-4, 0.0])
    plan.forward_backward(batch(G))
    plan.optimizer_step()
    torch.cuda.synchronize()
    return m, plan, start


# argument positions of dy_dysample_backward (include/dealyolo_hip.h)
A_DX, A_DOFF, A_C = 6, 10, 17


def test_freeze_10_prunes_layer_9_and_keeps_layer_14(golden):
    """freeze=10 (layers 0-9): nothing trainable lies upstream of layer 9 and its own convolution is frozen, so it leaves nothing on the
    tape -- no sampler backward, no weight gradient, no buffer of its convolution named after the loss; layer 14 keeps both halves."""
    from ultralytics.engine.trainer import frozen_parameter_names
    G = golden("dysample")
    names = [k for k, _ in _model(G).named_parameters()]
    frozen = set(frozen_parameter_names(names, 10))
    assert {"model.9.offset.weight", "model.9.offset.bias"} <= frozen and "model.14.offset.weight" not in frozen
    m, plan, start = _frozen_step(G, frozen)
    rt = plan.rt
    sp9, sp14 = rt.specs[(id(m.model[9]), "offset")], rt.specs[(id(m.model[14]), "offset")]
    assert not sp9.trainable and sp14.trainable
    fwd, back = _backward_ops(plan)
    assert [o[2] for o in fwd].count("dy_dysample") == 2  # the forward keeps both
    ds_back = [o for o in back if o[2] == "dy_dysample_backward"]
    assert len(ds_back) == 1 and ds_back[0][1][A_C] == 32 and ds_back[0][1][A_DX] and ds_back[0][1][A_DOFF]
    ptrs = {t.data_ptr() for t in (sp9.weight, sp9.wpack, sp9.wpack_t, sp9.gweight, sp9.gbias) if t is not None}
    for fn, args, name, _sid in back:
        assert not [a for a in args if isinstance(a, int) and a in ptrs], f"{name} after the loss touches layer 9's convolution"
    ws = {id(sp) for sp in plan.wgrad_specs}
    assert id(sp9) not in ws and id(sp14) in ws
    sd = m.state_dict()
    for k in frozen:
        assert torch.equal(sd[k], start[k]), f"frozen parameter {k} moved"
    assert not torch.equal(sd["model.14.offset.weight"], start["model.14.offset.weight"])
    assert not torch.equal(sd["model.14.offset.bias"], start["model.14.offset.bias"])
    assert float(rt.flat_g[rt.frozen.bool()].abs().max()) == 0.0 and torch.isfinite(rt.flat_g).all()


def test_frozen_layer_with_a_trainable_prefix_keeps_its_input_gradient(golden):
    """Only layer 9's own parameters frozen, everything upstream trainable: its parameter gradients are pruned (no weight-gradient
    launch, nothing of its gradient views named), its input gradient is kept whole -- the sampler's dx AND W^T d(o), which is part of
    dX whatever the flags say, so d(o) is still computed."""
    G = golden("dysample")
    frozen = {"model.9.offset.weight", "model.9.offset.bias"}
    m, plan, start = _frozen_step(G, frozen)
    rt = plan.rt
    sp9 = rt.specs[(id(m.model[9]), "offset")]
    assert not sp9.trainable
    fwd, back = _backward_ops(plan)
    ds_back = [o for o in back if o[2] == "dy_dysample_backward"]
    assert sorted(o[1][A_C] for o in ds_back) == [32, 64] and all(o[1][A_DX] and o[1][A_DOFF] for o in ds_back)
    assert id(sp9) not in {id(sp) for sp in plan.wgrad_specs}
    gptrs = {t.data_ptr() for t in (sp9.gweight, sp9.gbias) if t is not None}
    for fn, args, name, _sid in back:
        assert not [a for a in args if isinstance(a, int) and a in gptrs], f"{name} writes a frozen parameter's gradient"
    doff9 = [o for o in ds_back if o[1][A_C] == 64][0][1][A_DOFF]
    assert any(o[2] == "dy_conv_forward" and o[1][0] == doff9 and o[1][2] == sp9.wpack_t.data_ptr() for o in back), "W^T d(o) is missing"
    sd = m.state_dict()
    for k in frozen:
        assert torch.equal(sd[k], start[k])
    # the gradient everything upstream receives equals the unfrozen step's: freezing the layer changes no dX
    m2, plan2, _ = _frozen_step(G, set())
    k0 = "model.8.conv.weight"
    g1, g2 = dict(m.named_parameters())[k0].grad.float(), dict(m2.named_parameters())[k0].grad.float()
    assert relerr(g1, g2) < 1e-3 and float(g2.abs().max()) > 0


def test_reference_written_checkpoint_runs(golden):
    """attempt_load_weights of tests/golden/ref_ckpt_dysample.pt (module path ultralytics.nn.extra_modules.block.DySample, two groups):
    the eval forward is the reference's (2e-2) and EQUALS that of a natively built model with the same fp16-rounded state."""
    from ultralytics.nn.tasks import DetectionModel, attempt_load_weights, torch_safe_load
    G = golden("dysample")
    a = attempt_load_weights(CKPT, device="cuda:0")
    cfg = deepcopy(torch_safe_load(CKPT)[0]["model"].yaml)
    b = DetectionModel(cfg, ch=3, verbose=False)
    b.load_state_dict({k: (v.half().float() if v.is_floating_point() else v) for k, v in state(G, "ckpt").items()}, strict=True)
    b.cuda().eval()
    x = G.t("batch/img").cuda()
    with torch.no_grad():
        ya, _ = a(x)
        yb, _ = b(x)
    assert torch.equal(ya, yb)
    ref = G.t("ckpt/y_eval")
    eb, ec = relerr(ya[:, :4].cpu(), ref[:, :4]), relerr(ya[:, 4:].cpu(), ref[:, 4:])
    print(f"checkpoint eval: box relerr {eb:.2e} cls relerr {ec:.2e}")
    assert eb < 2e-2 and ec < 2e-2


def test_augmented_forward_vs_golden(golden):
    """model(x, augment=True): walked, recorded, replayed; the bound of tests/test_gpu_tta.py (1e-3 on boxes and on class scores)."""
    G = golden("dysample")
    m = _model(G).eval()
    x = G.t("batch/img").cuda()
    want = G.t(f"{MODEL}/y_aug")
    ys = []
    for _ in range(3):
        y, second = m(x, augment=True)
        assert second is None and tuple(y.shape) == tuple(want.shape)
        eb, ec = relerr(y[:, :4], want[:, :4]), relerr(y[:, 4:], want[:, 4:])
        print(f"augment: box relerr {eb:.2e}, class relerr {ec:.2e}")
        assert eb <= 1e-3 and ec <= 1e-3
        ys.append(y.clone())
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


def test_two_epochs_through_the_public_trainer():
    from ultralytics import YOLO
    from ultralytics.data import SyntheticDetection
    torch.manual_seed(0)
    y = YOLO("yolov8n-ASF-P2P2-DySample.yaml")
    w0 = {k: v.detach().clone() for k, v in y.model.state_dict().items()}
    src = SyntheticDetection(n_batches=4, batch=4, imgsz=64, boxes_per_image=3, wh=(0.1, 0.4), seed=3)
    hist = y.train(data=src, batch=4, imgsz=64, epochs=2, optimizer="SGD", warmup_epochs=0.0, lr0=0.01, nbs=4, hipgraph=True, amp=False)
    hist = np.asarray([[float(v) for v in h] for h in hist], dtype=np.float64)
    assert hist.shape == (2, 3) and np.isfinite(hist).all()
    plan = y.trainer.plan
    st = plan.state.cpu().numpy()
    # every optimizer_step() the trainer issued took effect: none skipped at amp=False, the device counter advanced with the host's
    assert st[5] == 8 and st[6] == 0 and st[5] == plan.opt_calls and st[0] == 1.0, st.tolist()
    w1 = y.trainer.model.state_dict()
    ds = [k for k, _ in y.trainer.model.named_parameters() if any(k.startswith(f"model.{i}.") for i in DYSAMPLE_LAYERS)]
    assert ds == ["model.9.offset.weight", "model.9.offset.bias", "model.14.offset.weight", "model.14.offset.bias"]
    still = [k for k in ds if torch.equal(w1[k].cpu(), w0[k].cpu())]
    assert not still, f"DySample parameters that never moved: {still}"
    for i in DYSAMPLE_LAYERS:  # the buffer is no parameter: EMA, optimizer and checkpoints carry it unchanged
        assert torch.equal(w1[f"model.{i}.init_pos"].cpu(), w0[f"model.{i}.init_pos"].cpu())
    assert torch.isfinite(plan.rt.flat_g).all()


def test_multi_scale_over_one_arena():
    """multi_scale=True: one recorded launch list per drawn size, all over one arena (tests/test_gpu_trainer.py holds the default
    graph to the same): every optimizer step takes effect, and the run equals, bit for bit, one whose size plans keep separate buffers
    -- the sampler's offsets, d(o) and side buffers are step-local, and a freshly initialised layer has no far sample."""
    from ultralytics import YOLO
    from ultralytics.data import SyntheticDetection
    from ultralytics.engine.trainer import DetectionTrainer

    def run(share):
        torch.manual_seed(0)
        y = YOLO(os.path.join(CFG_DIR, MODEL + ".yaml"))
        src = SyntheticDetection(n_batches=8, batch=4, imgsz=64, boxes_per_image=3, wh=(0.1, 0.4), seed=3)
        DetectionTrainer.share_arena = share
        try:
            hist = y.train(data=src, batch=4, imgsz=64, epochs=1, optimizer="SGD", warmup_epochs=0.0, lr0=0.01, nbs=4, hipgraph=True,
                           multi_scale=True, amp=False)
        finally:
            DetectionTrainer.share_arena = True
        tr = y.trainer
        return hist, tr.plan.rt.flat_p.clone(), tr

    hist, p1, tr = run(True)
    sizes = sorted(k[1] for k in tr.plans if isinstance(k, tuple))
    assert len(sizes) >= 2 and all(torch.isfinite(torch.as_tensor(h)).all() for h in hist), sizes
    assert float(tr.plan.state[5]) == 8 and float(tr.plan.state[6]) == 0
    assert tr.arena is not None and 0 < tr.arena.peak <= tr.arena.cap
    _, p2, tr2 = run(False)
    assert torch.equal(p1, p2)


def test_flat_layout_puts_the_offset_convolution_in_the_head_segments(golden):
    """The six-segment flat layout (hip/runtime.py): offset.weight with the decayed weights, offset.bias with the biases, both in the
    neck + head half -- the first data-parallel gradient bucket -- and init_pos among the float buffers that EMA and checkpoints carry."""
    m = _model(golden("dysample"))
    rt = m._runtime(torch.device("cuda", 0))
    for i in DYSAMPLE_LAYERS:
        w, b = f"model.{i}.offset.weight", f"model.{i}.offset.bias"
        assert rt.param_group[w] == 1 and rt.param_group[b] == 0
        assert rt.param_off[b] < rt.seg_bounds[0] <= rt.param_off[w] < rt.seg_bounds[1] <= rt.bucket_split
        assert any(n == f"model.{i}.init_pos" for n, _ in rt.buffer_layout)
        p = dict(m.named_parameters())[w]
        assert p.data.data_ptr() == rt.flat_p.data_ptr() + 4 * rt.param_off[w] and p.grad.data_ptr() == rt.flat_g.data_ptr() + 4 * rt.param_off[w]
