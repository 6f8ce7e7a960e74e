"""-m gpu: Fusion in 'bifpn' mode (reference nn/extra_modules/block.py:453-490) on the HIP path.

1. the kernels (csrc/fusion.hip) per element against the float64 restatement tests/bifpn_ref.py (tests/test_host_bifpn.py ties it to
   the reference's stored values and to autograd), at the shapes of tests/bifpn_util.py::KERNEL_CASES, each with 2 and 3 operands, the
   half-resolution operand first, last and absent, gradients stored and accumulated:

   exact inputs (operands, dy and the stored gradients small integers; p = (1, 1), (1, 3), (1, 1, 2): every f a dyadic fraction; every
   dot product's sum of absolute values below 2^22, asserted): y and dx bit-equal to the float64 value rounded to fp16, g (the sum of
   the stage-one partials) and dL/dp bit-equal in fp32.

   the ReLU cut, p = (-0.5, 1.2): the cut operand's dx all zeros, its dL/dp exactly 0, the other operand's dx equal to dy.

   normal inputs: the bounds of tests/bifpn_util.py, counted from the orders the kernel file documents BEFORE the first GPU run:
   y and dx: U16 |ref| + 2^-25 + (f's n roundings + the product + the n - 1 additions (dx: the addition of the stored value) + 1) U32 mag;
   g: (2 x 8 x granules per work item + 6 shuffle levels + 3 wave additions + 1) U32 sum |dy x|;
   dL/dp: the g bounds carried through the Jacobian + its own fp32 operations (bound_dp); sum_j relu(p_j) dL/dp_j = 0 to that bound.

   two backward runs: the same bytes.  The frozen variant (null workspace): the full variant's dx bytes, the workspace and the
   gradient slice untouched; the finish with accumulate = 1 adds.  Nothing outside a slice is ever written (canaries around every buffer).
2. the module against the reference's fp32 values at 4 x the tolerance the generator measured (tol/<case>/...); the engine's refusals.
3. the graph yolov8n-ASF-P2P2-BiFPN at 64x64, batch 2, at 4 x the generator's measured tolerances: eval / fused eval / augmented eval /
   the checkpoint's eval; one training step with the three fusion_weight gradients in full and the updated vectors; captured = eager;
   SOAP and the six adaptive modes of the flat optimizer (RMSProp among them); freeze; launch lists without a forward dy_upsample2x; last.pt and EMA; multi_scale; the default graph launches no
   dy_fusion_* kernel."""
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

import bifpn_ref as R
import bifpn_util as U
from conftest import CFG_DIR
from golden.cases import rnd
from gpu_util import l2err, relerr, run_fwd_bwd

pytestmark = pytest.mark.gpu
POISON = -1234.0  # exactly representable in fp16
GUARD = 3         # canary pixels behind every written tensor
WS_POISON = -4321.0
VARIANTS = [(name, n, up) for name in U.KERNEL_CASES for n, up in U.variants(name)]
IDS = [f"{name}-{n}ops-up{'none' if up is None else up}" for name, n, up in VARIANTS]


# ----------------------------------------------------------------------------- helpers
def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """fp16 device storage of an (N, H, W, C) array at channel offset c0 of pitch ld, POISON everywhere else and in GUARD pixels
    behind it."""

    def __init__(self, a, c0, ld, fill=None):
        t = torch.as_tensor(np.asarray(a))
        self.shape, self.C, self.c0, self.ld = tuple(t.shape), t.shape[-1], c0, ld
        self.npix = int(np.prod(self.shape[:-1]))
        s = torch.full((self.npix + GUARD, ld), POISON, dtype=torch.float16)
        s[:self.npix, c0:c0 + self.C] = (t if fill is None else torch.full_like(t, fill)).reshape(self.npix, self.C).half()
        self.s = s.cuda()

    ptr = property(lambda b: b.s.data_ptr() + 2 * b.c0)

    def get(self):
        return self.s[:self.npix, self.c0:self.c0 + self.C].reshape(self.shape).cpu().double().numpy()

    def clean(self):
        """Nothing outside the slice was written."""
        return bool((self.s[self.npix:] == POISON).all()) and bool((self.s[:, :self.c0] == POISON).all()) and \
            bool((self.s[:, self.c0 + self.C:] == POISON).all())


def _run(name, n, up, xs, dy, p, old=None, frozen=False, need=None):
    """Forward, backward and finish of one case -> dict(y, dx, g, dp, raw=(dx buffers' bytes, gw bytes)).  ``old``: accumulate into
    these stored gradients; ``need``: which operands get a dx (default all)."""
    from ultralytics.hip import lib
    L = lib()
    N, H, W, C, c0, ld = U.KERNEL_CASES[name]
    need = [True] * n if need is None else need
    xb = [Buf(x, c0, ld) for x in xs]
    x0 = [b.s.clone() for b in xb]
    pb = torch.tensor(p, dtype=torch.float32, device="cuda")
    yb = Buf(np.zeros((N, H, W, C)), c0, ld, fill=POISON)
    ops = [v for i in range(n) for v in (xb[i].ptr, ld, int(i == up))] + [0, 0, 0] * (3 - n)
    assert L.dy_fusion_forward(*ops, pb.data_ptr(), yb.ptr, ld, n, N, H, W, C, _stream()) == 0
    dyb = Buf(dy, c0, ld)
    dxb = [Buf(old[i], c0, ld) if old is not None else Buf(np.zeros((N, H, W, C)), c0, ld, fill=POISON) for i in range(n)]
    parts = L.dy_fusion_num_partials(N * H * W, C)
    assert parts == U.num_partials(N * H * W, C)
    ws = torch.full((3 * parts + 16,), WS_POISON, dtype=torch.float32, device="cuda")
    gw = torch.full((8,), WS_POISON, dtype=torch.float32, device="cuda")
    bops = [v for i in range(n) for v in (xb[i].ptr, ld, int(i == up), dxb[i].ptr if need[i] else 0, ld, int(old is not None))]
    bops += [0, 0, 0, 0, 0, 0] * (3 - n)
    assert L.dy_fusion_backward(dyb.ptr, ld, *bops, pb.data_ptr(), 0 if frozen else ws.data_ptr(), n, N, H, W, C, _stream()) == 0
    if not frozen:
        assert L.dy_fusion_wgrad_finish(ws.data_ptr(), parts, pb.data_ptr(), gw.data_ptr(), n, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert yb.clean() and dyb.clean() and all(b.clean() for b in dxb) and all(torch.equal(b.s, s0) for b, s0 in zip(xb, x0))
    assert bool((ws[n * parts:] == WS_POISON).all()) and bool((gw[n:] == WS_POISON).all())
    if frozen:
        assert bool((ws == WS_POISON).all()) and bool((gw == WS_POISON).all())
    for i in range(n):
        if not need[i] and old is None:
            assert bool((dxb[i].s == POISON).all())
    g = ws[:n * parts].view(n, parts).double().sum(1).cpu().numpy()
    return dict(y=yb.get(), dx=[b.get() for b in dxb], g=g, dp=gw[:n].cpu().double().numpy(), parts=parts,
                raw=([b.s.clone() for b in dxb], gw.clone(), ws.clone()))


def _full(xs, up):
    return [R.up2(x) if i == up else x for i, x in enumerate(xs)]


def _f16(a):
    return np.asarray(a).astype(np.float16).astype(np.float64)


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


# ----------------------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("name,n,up", VARIANTS, ids=IDS)
def test_exact_inputs_equal_the_reference(name, n, up):
    for p in U.EXACT_P[n]:
        xs, dy, old = U.exact_inputs(name, n, up)
        f, b = R.forward(_full(xs, up), p), R.backward(_full(xs, up), p, dy)
        assert float(b["gmag"].max()) < 2 ** 22 < 2 ** 24  # every partial and every sum is an integer fp32 holds exactly
        got = _run(name, n, up, xs, dy, p)
        assert np.array_equal(got["y"], _f16(f["y"])) and np.array_equal(_f16(f["y"]), f["y"])
        for i in range(n):
            assert np.array_equal(got["dx"][i], _f16(b["dx"][i])), (p, i)
        assert np.array_equal(got["g"], b["g"]) and np.array_equal(_f32(b["g"]), b["g"])
        assert np.array_equal(got["dp"], _f32(b["dp"])) and np.array_equal(_f32(b["dp"]), b["dp"])
        acc = _run(name, n, up, xs, dy, p, old=old)
        for i in range(n):
            assert np.array_equal(acc["dx"][i], _f16(b["dx"][i] + old[i])), (p, i)
        assert np.array_equal(acc["dp"], got["dp"])


@pytest.mark.parametrize("name", ["one_granule", "slice", "partials"])
@pytest.mark.parametrize("up", [None, 0, 1])
def test_relu_cut(name, up):
    xs, dy, old = U.exact_inputs(name, 2, up, seed=3)
    got = _run(name, 2, up, xs, dy, U.CUT_P)
    assert not got["dx"][0].any() and got["dp"][0] == 0.0
    assert np.array_equal(got["dx"][1], dy) and np.array_equal(got["y"], _full(xs, up)[1])
    assert got["dp"][1] == 0.0  # (g1 - f1 g1) / s with f1 = 1
    xs, dy, old = U.normal_inputs(name, 2, up, seed=4)
    got = _run(name, 2, up, xs, dy, U.CUT_P)
    assert not got["dx"][0].any() and got["dp"][0] == 0.0 and np.array_equal(got["dx"][1], dy)


@pytest.mark.parametrize("name,n,up", VARIANTS, ids=IDS)
def test_normal_inputs_within_the_counted_bounds(name, n, up):
    N, H, W, C = U.KERNEL_CASES[name][:4]
    p = np.asarray(U.NORMAL_P[n], dtype=np.float32).astype(np.float64)
    xs, dy, old = U.normal_inputs(name, n, up)
    f, b = R.forward(_full(xs, up), p), R.backward(_full(xs, up), p, dy)

    def check(what, got, ref, bound):
        err = np.abs(got - ref)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{what}: max err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
        assert np.isfinite(got).all() and worst <= 1.0, what

    got = _run(name, n, up, xs, dy, p)
    check("y", got["y"], f["y"], U.bound_y(f["y"], f["mag"], n))
    for i in range(n):
        check(f"dx{i}", got["dx"][i], b["dx"][i], U.bound_dx(b["dx"][i], n))
    check("g", got["g"], b["g"], U.bound_g(b["gmag"], N * H * W, C))
    bd = U.bound_dp(p, b["g"], b["gmag"], N * H * W, C)
    check("dp", got["dp"], b["dp"], bd)
    ident = abs(float((np.maximum(p, 0) * got["dp"]).sum()))
    print(f"sum relu(p) dL/dp = {ident:.3e} (bound {float((np.maximum(p, 0) * bd).sum()):.3e})")
    assert ident <= float((np.maximum(p, 0) * bd).sum())
    acc = _run(name, n, up, xs, dy, p, old=old)
    for i in range(n):
        check(f"dx{i} (add)", acc["dx"][i], b["dx"][i] + old[i], U.bound_dx(b["dx"][i] + old[i], n, old=old[i]))


@pytest.mark.parametrize("name,n,up", [("odd_granules", 3, 0), ("partials", 2, 1), ("slice", 3, 2)])
def test_two_runs_give_the_same_bytes_and_the_frozen_variant_the_same_dx(name, n, up):
    p = U.NORMAL_P[n]
    xs, dy, old = U.normal_inputs(name, n, up)
    a, b = _run(name, n, up, xs, dy, p), _run(name, n, up, xs, dy, p)
    for u, v in zip(a["raw"][0] + [a["raw"][1], a["raw"][2]], b["raw"][0] + [b["raw"][1], b["raw"][2]]):
        assert torch.equal(u, v)
    fz = _run(name, n, up, xs, dy, p, frozen=True)  # (asserts in _run: the workspace and the gradient slice keep their canaries)
    for u, v in zip(a["raw"][0], fz["raw"][0]):
        assert torch.equal(u, v)
    aa, fa = _run(name, n, up, xs, dy, p, old=old), _run(name, n, up, xs, dy, p, old=old, frozen=True)
    for u, v in zip(aa["raw"][0], fa["raw"][0]):
        assert torch.equal(u, v)
    # an operand that needs no gradient: its dx is not written, the others' and the weight gradient are the same bytes
    need = [i != 0 for i in range(n)]
    nn_ = _run(name, n, up, xs, dy, p, need=need)
    assert all(torch.equal(u, v) for u, v in zip(a["raw"][0][1:], nn_["raw"][0][1:])) and torch.equal(a["raw"][1], nn_["raw"][1])


@pytest.mark.parametrize("name,n,up", [("one_granule", 2, 1), ("partials", 3, 0)])
def test_finish_accumulates_into_the_gradient_slice(name, n, up):
    """dy_fusion_wgrad_finish with accumulate = 1 adds to what the slice holds: on the exact inputs a second call over the same
    partials leaves 2 dL/dp, a third 3 dL/dp, bit for bit (small dyadic values: the sums are exact in fp32); a stored call in
    between starts over; nothing behind the n values is written."""
    from ultralytics.hip import lib
    L = lib()
    p = U.EXACT_P[n][-1]
    xs, dy, old = U.exact_inputs(name, n, up)
    b = R.backward(_full(xs, up), p, dy)
    got = _run(name, n, up, xs, dy, p)
    assert np.array_equal(got["dp"], b["dp"]) and np.abs(b["dp"]).max() > 0
    gw, ws = got["raw"][1].clone(), got["raw"][2]
    pb = torch.tensor(p, dtype=torch.float32, device="cuda")
    want = torch.tensor(b["dp"], dtype=torch.float32)
    for k, acc in ((2, 1), (3, 1), (1, 0), (2, 1)):
        assert L.dy_fusion_wgrad_finish(ws.data_ptr(), got["parts"], pb.data_ptr(), gw.data_ptr(), n, acc, _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(gw[:n].cpu(), k * want) and bool((gw[n:] == WS_POISON).all()), (k, acc)


def test_all_weights_nonpositive_give_nan():
    """The reference's 0 / 0, kept: no guard, no epsilon."""
    xs, dy, old = U.exact_inputs("one_granule", 2, None)
    got = _run("one_granule", 2, None, xs, dy, (-1.0, 0.0))
    assert np.isnan(got["y"]).all() and got["dp"].tolist() == [0.0, 0.0]


# ----------------------------------------------------------------------------- 2. the module against the reference
@pytest.mark.parametrize("case", list(U.MODULE_CASES))
def test_module_vs_golden(golden, case):
    """l2err of y, every gx and the parameter gradient below 4 x the tolerance the generator measured for the case (the error of a
    float64 emulation of this path's fp16 storage against the reference's fp32 values).  A tensor the reference has as all zeros
    (the cut operand's gradient) must be all zeros."""
    from ultralytics.nn.extra_modules.block import Fusion
    G = golden("bifpn")
    C, H, W, p = U.MODULE_CASES[case]
    seed, n = U.MODULE_SEEDS[case], len(p)
    m = Fusion([C] * n, "bifpn")
    with torch.no_grad():
        m.fusion_weight.copy_(torch.tensor(p))
    xs = [rnd(10 * seed + i, U.BATCH, C, H, W) for i in range(n)]
    gy = rnd(10 * seed + 9, U.BATCH, C, H, W)
    y, gxs, rt = run_fwd_bwd(m, xs, gy)
    got, want = dict(y=y, gp=m.fusion_weight.grad.float().cpu()), dict(y=G.t(f"mod/{case}/y"), gp=G.t(f"mod/{case}/gp"))
    for i in range(n):
        got[f"gx{i}"], want[f"gx{i}"] = gxs[i], G.t(f"mod/{case}/gx{i}")
    tols = {k: float(G[f"tol/{case}/{k}"]) for k in got}
    errs = {k: l2err(got[k].reshape(want[k].shape), want[k]) for k in got if float(want[k].abs().max()) > 0}
    print(case, {k: f"{errs[k]:.2e} (4 x {tols[k]:.2e})" for k in errs})
    for k in got:
        if k in errs:
            assert errs[k] < 4 * tols[k], k
        else:
            assert not bool(got[k].any()), k
    for j, pj in enumerate(p):
        if pj <= 0:
            assert float(got["gp"][j]) == 0.0


def test_engine_refuses_by_name():
    from ultralytics.hip.engine import FusionVec
    from ultralytics.nn.extra_modules.block import Fusion
    m = Fusion([16, 16]).cuda()
    rt = m._runtime(torch.device("cuda", 0))
    eng = rt.eng
    act = lambda c, h=4: eng.wrap_act(torch.zeros(1, h, 4, c, dtype=torch.float16, device="cuda"))  # noqa: E731
    pv = FusionVec(m.fusion_weight.data, rt.gviews[id(m.fusion_weight)], True)
    with pytest.raises(NotImplementedError, match=r"Fusion.*4 operands \(supported: 2 or 3 operands"):
        eng.fusion([act(16)] * 4, pv)
    with pytest.raises(NotImplementedError, match=r"Fusion.*supported: 2 or 3 operands of one shape"):
        eng.fusion([act(16), act(32)], pv)
    with pytest.raises(NotImplementedError, match=r"Fusion.*supported: 2 or 3 operands of one shape"):
        eng.fusion([act(16), act(16, 2)], pv)
    with pytest.raises(NotImplementedError, match=r"an input of width 12"):
        eng.fusion([act(16).sub(0, 12), act(16).sub(0, 12)], pv)
    y = eng.fusion([act(16), act(16)], pv)  # ... and the supported call runs
    torch.cuda.synchronize()
    assert (y.N, y.H, y.W, y.C) == (1, 4, 4, 16)


# ----------------------------------------------------------------------------- 3. the graph against the reference
def _model(G, name=U.MODEL):
    from ultralytics.nn.tasks import DetectionModel
    m = DetectionModel(os.path.join(CFG_DIR, name + ".yaml"), ch=3, verbose=False)
    if name == U.MODEL:
        m.load_state_dict(U.state(G, U.MODEL), strict=True)
    return m.cuda()


def _names(ops):
    return [o[2] for o in ops if o[0] is not None]


def _forward_upsamples(ops):
    """dy_upsample2x launches of a list that run FORWARD (argument 8, ``backward``, is 0)."""
    return [o for o in ops if o[0] is not None and o[2] == "dy_upsample2x" and o[1][8] == 0]


def test_eval_and_fused_eval_vs_golden(golden):
    """Box rows and class scores at 4 x the generator's measured tolerances; the second call of a geometry is traced into an
    InferPlan, the third replays it: all three bit for bit; three dy_fusion_forward launches in the list, two of them with a
    half-resolution operand, and no forward dy_upsample2x: rows 9 and 14 are never executed."""
    G = golden("bifpn")
    m = _model(G).eval()
    x = G.t("batch/img").cuda()
    for key in ("y_eval", "y_eval_fused"):
        if key == "y_eval_fused":
            m.fuse()
            assert not hasattr(m.model[1], "bn") and isinstance(m.model[11].fusion_weight, torch.nn.Parameter)
        ref = G.t(f"{U.MODEL}/{key}")
        with torch.no_grad():
            y1, _ = m(x)   # walked
            assert not m._infer_plans["plans"]
            y2, _ = m(x)   # traced into a plan
            plan = m._infer_plans["plans"][(2, 3, 64, 64)]
            y3, _ = m(x)   # replayed
        torch.cuda.synchronize()
        fus = [o for o in plan.rec.ops if o[0] is not None and o[2] == "dy_fusion_forward"]
        assert len(fus) == 3 and sorted(o[1][2] + o[1][5] for o in fus) == [0, 1, 1] and not _forward_upsamples(plan.rec.ops)
        assert torch.equal(y1, y2) and torch.equal(y1, y3)
        assert y1.shape == ref.shape
        eb, ec = relerr(y1[:, :4].cpu(), ref[:, :4]), relerr(y1[:, 4:].cpu(), ref[:, 4:])
        tb, tc = float(G[f"tol/{U.MODEL}/{key}_box"]), float(G[f"tol/{U.MODEL}/{key}_cls"])
        print(f"{key}: box relerr {eb:.2e} (4 x {tb:.2e}) cls relerr {ec:.2e} (4 x {tc:.2e})")
        assert eb < 4 * tb and ec < 4 * tc


def test_augmented_forward_vs_golden(golden):
    G = golden("bifpn")
    m = _model(G).eval()
    x = G.t("batch/img").cuda()
    want = G.t(f"{U.MODEL}/y_aug")
    ys = []
    for _ in range(3):
        y, second = m(x, augment=True)
        assert second is None and tuple(y.shape) == tuple(want.shape)
        ys.append(y.clone())
    eb, ec = relerr(ys[0][:, :4].cpu(), want[:, :4]), relerr(ys[0][:, 4:].cpu(), want[:, 4:])
    tb, tc = float(G[f"tol/{U.MODEL}/y_aug_box"]), float(G[f"tol/{U.MODEL}/y_aug_cls"])
    print(f"augment: box relerr {eb:.2e} (4 x {tb:.2e}), class relerr {ec:.2e} (4 x {tc:.2e})")
    assert eb < 4 * tb and ec < 4 * tc
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


def test_train_step_vs_golden(golden):
    """One training step: loss items, loss, gradient norms (median / max of the relative error), the first layer's gradient, the
    three fusion_weight gradients element by element and, after one clipped SGD-nesterov step, the norms of every tensor's change and
    the change of the three vectors, at 4 x the tolerances the generator measured for them (tol/<model>/...).  The traced list holds
    three forward, three backward and three finish launches and no forward dy_upsample2x."""
    from ultralytics.hip.train import StepPlan
    G = golden("bifpn")
    keys = ("items", "loss", "grad_l2_median", "grad_l2_max", "grad_first", "upd_l2_median", "upd_l2_max")
    tol = {k: float(G[f"tol/{U.MODEL}/{k}"]) for k in keys}
    m = _model(G).train()
    for k, v in m.named_parameters():
        v.requires_grad = ".dfl" not in k  # (the reference freezes it: engine/trainer.py:563)
    start = {k: v.detach().clone() for k, v in m.named_parameters()}
    plan = StepPlan(m, 2, 64, nmax=8, optimizer="SGD", init_scale=1024.0, dynamic_scale=False)
    plan.set_hyper([U.STEP_LR] * 3, U.STEP_MOM, [0.0] * 3, max_norm=10.0)
    plan.forward_backward(U.batch(G))
    torch.cuda.synchronize()
    ops = _names(plan.rec_fb.ops)
    assert [ops.count(k) for k in ("dy_fusion_forward", "dy_fusion_backward", "dy_fusion_wgrad_finish")] == [3, 3, 3]
    assert not _forward_upsamples(plan.rec_fb.ops) and ops.count("dy_upsample2x") >= 2  # (backward only: the folds of rows 9 and 14's gradients)
    s = plan.crit.scalars.cpu()
    ref_items = G.t(f"{U.MODEL}/items")
    per_item = float(((s[5:8] - ref_items).abs() / ref_items.abs()).max())
    eloss = abs(float(s[8]) - float(G[f"{U.MODEL}/loss"])) / float(G[f"{U.MODEL}/loss"])
    names = [str(k) for k in G[f"{U.MODEL}/grad_names"]]
    params = dict(m.named_parameters())
    scale = float(plan.state[0])
    l2 = torch.stack([params[k].grad.float().norm() / scale for k in names]).cpu()
    ref = G.t(f"{U.MODEL}/grad_l2")
    rel = ((l2 - ref).abs() / (ref.abs() + 1e-3 * ref.abs().max())).numpy()
    ef = l2err(params[names[0]].grad.float().cpu() / scale, G.t(f"{U.MODEL}/grad_first"))
    got = dict(items=per_item, loss=eloss, grad_l2_median=float(np.median(rel)), grad_l2_max=float(rel.max()), grad_first=ef)
    for k in U.FUSION_KEYS:
        g = params[k].grad.float().cpu() / scale
        got[f"grad/{k}"], tol[f"grad/{k}"] = l2err(g, G.t(f"{U.MODEL}/grad/{k}")), float(G[f"tol/{U.MODEL}/grad/{k}"])
        w = start[k].clamp(min=0).cpu()
        print(k, "gradient", g.tolist(), "reference", G.t(f"{U.MODEL}/grad/{k}").tolist(), "sum relu(p) g", float((w * g).sum()))
    sd = m.state_dict()
    rm = [str(k) for k in G[f"{U.MODEL}/run_mean_names"]]
    assert relerr(torch.stack([sd[k].sum() for k in rm]).cpu(), G.t(f"{U.MODEL}/run_mean_sum")) < 5e-3
    assert relerr(torch.stack([sd[k.replace("mean", "var")].sum() for k in rm]).cpu(), G.t(f"{U.MODEL}/run_var_sum")) < 5e-3
    assert torch.isfinite(plan.rt.flat_g).all() and float(plan.state[2]) == 0.0
    plan.optimizer_step()
    torch.cuda.synchronize()
    after = dict(m.named_parameters())
    upd = torch.stack([(after[k].detach() - start[k]).float().norm() for k in names]).cpu()
    ref_u = G.t(f"{U.MODEL}/upd_l2")
    relu = ((upd - ref_u).abs() / (ref_u.abs() + 1e-3 * ref_u.abs().max())).numpy()
    got.update(upd_l2_median=float(np.median(relu)), upd_l2_max=float(relu.max()))
    for k in U.FUSION_KEYS:
        d_got, d_ref = (after[k].detach() - start[k]).float().cpu(), G.t(f"{U.MODEL}/upd/{k}") - start[k].cpu()
        got[f"upd/{k}"], tol[f"upd/{k}"] = l2err(d_got, d_ref), float(G[f"tol/{U.MODEL}/upd/{k}"])
        assert float(d_got.abs().max()) > 0, k
    print("items", s[5:8].tolist(), ref_items.tolist())
    print({k: f"{got[k]:.2e} (4 x {tol[k]:.2e})" for k in got}, "worst gradient norm:", names[int(rel.argmax())])
    for k in got:
        assert got[k] < 4 * tol[k], k


def test_captured_step_equals_the_eager_step(golden):
    """One StepPlan step replayed as a hipGraph against the eager step of another plan on the same state and batch: the same
    launches, no atomics in the fusion kernels, so loss items and ALL gradients are EQUAL."""
    from ultralytics.hip.train import StepPlan
    G = golden("bifpn")
    outs = []
    for graph in (False, True):
        m = _model(G).train()
        plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0, use_graph=graph)
        sd0 = {k: v.clone() for k, v in m.state_dict().items()}
        plan.forward_backward(U.batch(G))
        if graph:
            assert plan.graph_fb is not None
            m.load_state_dict(sd0)
            plan.forward_backward(U.batch(G))  # the captured graph's replay
        torch.cuda.synchronize()
        assert _names(plan.rec_fb.ops).count("dy_fusion_backward") == 3
        outs.append((plan.rt.flat_g.clone(), plan.crit.scalars.clone()))
    assert torch.isfinite(outs[0][0]).all() and float(outs[0][0].abs().max()) > 0
    assert torch.equal(outs[0][1][5:9], outs[1][1][5:9]) and torch.equal(outs[0][0], outs[1][0])


def test_flat_layout_ema_and_clipping_see_the_vectors(golden):
    """The generic paths: the three vectors lie in the decayed group of the neck + head segment, their gradient views are slices of
    the flat gradient buffer (so the clip norm and a data-parallel bucket include them), one SGD step moves parameter and EMA, and
    weight decay acts on them (the decayed group)."""
    from ultralytics.hip.train import StepPlan
    G = golden("bifpn")
    moved = {}
    for wd in (0.0, 0.05):
        m = _model(G).train()
        plan = StepPlan(m, 2, 64, nmax=8, optimizer="SGD", init_scale=1024.0, dynamic_scale=False)
        rt = plan.rt
        params = dict(m.named_parameters())
        for k in U.FUSION_KEYS:
            o = rt.param_off[k]
            assert rt.param_group[k] == 1 and rt.seg_bounds[0] <= o < rt.seg_bounds[1] <= rt.bucket_split
            assert params[k].grad.data_ptr() == rt.flat_g[o:].data_ptr() and params[k].data.data_ptr() == rt.flat_p[o:].data_ptr()
        ema0 = plan.ema.clone()
        p0 = rt.flat_p.clone()
        plan.set_hyper([0.01] * 3, 0.9, [0.0, wd, 0.0], ema_decay=0.5)
        plan.forward_backward(U.batch(G))
        plan.optimizer_step()
        torch.cuda.synchronize()
        for k in U.FUSION_KEYS:
            o = rt.param_off[k]
            assert float(rt.flat_g[o:o + 2].abs().min()) > 0 and bool((rt.flat_g[o + 2:o + 8] == 0).all())
            assert not torch.equal(rt.flat_p[o:o + 2], p0[o:o + 2]) and not torch.equal(plan.ema[o:o + 2], ema0[o:o + 2])
            assert not torch.equal(plan.ema[o:o + 2], rt.flat_p[o:o + 2]) and torch.equal(rt.flat_p[o + 2:o + 8], p0[o + 2:o + 8])
        moved[wd] = torch.cat([rt.flat_p[rt.param_off[k]:rt.param_off[k] + 2] for k in U.FUSION_KEYS]).cpu()
    assert not torch.equal(moved[0.0], moved[0.05])


def test_soap_steps_the_vectors(golden, monkeypatch):
    """optimizer='SOAP': the grouped HIP step (SoapHip) against the host-driven Soap (DY_SOAP_HIP=0) and against Soap over float64
    tensors on the same gradients, three calls: on the three vectors the device path is within 4 x the host path's distance from
    float64 (the margin tests/test_gpu_soap.py allows) or 16 fp32 roundings of the parameter."""
    from ultralytics.hip.soap import Soap, SoapHip
    from ultralytics.hip.train import StepPlan
    G = golden("bifpn")
    LR, MOM, WD = [0.003] * 3, 0.937, [0.0, 5e-4, 0.0]
    res, grads, views, p0 = {}, None, None, None
    for hip in (True, False):
        monkeypatch.setenv("DY_SOAP_HIP", "1" if hip else "0")
        m = _model(G).train()
        plan = StepPlan(m, 2, 64, nmax=8, optimizer="SOAP", init_scale=1.0, dynamic_scale=False)
        rt = plan.rt
        if grads is None:
            p0 = rt.flat_p.clone()
            gen = torch.Generator(device="cpu").manual_seed(901)
            grads = [(torch.randn(rt.n_params_flat, generator=gen) * 0.01).cuda().masked_fill_(rt.frozen.bool(), 0.0) for _ in range(3)]
        for g in grads:
            rt.flat_g.copy_(g)
            plan.set_hyper(LR, MOM, WD)
            plan.optimizer_step()
        torch.cuda.synchronize()
        assert isinstance(plan._soap, SoapHip if hip else Soap)
        res[hip], views = rt.flat_p.clone(), plan._soap_views
        offs = {k: rt.param_off[k] for k in U.FUSION_KEYS}
    p64 = p0.double()
    opt = Soap([(p64[o:o + k].view(sh), g) for _, o, k, sh, g in views], beta1=MOM, beta2=0.95)
    for g in grads:
        g = g.double()
        coef = min(10.0 / (float(g.norm()) + 1e-6), 1.0)
        opt.step([g[o:o + k].view(sh) * coef for _, o, k, sh, _ in views], LR, WD)
    for k, o in offs.items():
        ref = p64[o:o + 2]
        e_hip, e_host = float((res[True][o:o + 2].double() - ref).abs().max()), float((res[False][o:o + 2].double() - ref).abs().max())
        moved = float((ref - p0[o:o + 2].double()).abs().max())
        print(k, f"SoapHip {e_hip:.3e}, Soap fp32 {e_host:.3e} from float64; moved by {moved:.3e}")
        assert moved > 0 and not torch.equal(res[True][o:o + 2], p0[o:o + 2])
        assert e_hip <= max(4 * e_host, 16 * 2.0 ** -24 * float(ref.abs().max()))
    monkeypatch.delenv("DY_SOAP_HIP", raising=False)


@pytest.mark.parametrize("optimizer", ["Adam", "AdamW", "RMSProp", "RAdam", "Adamax", "NAdam"])
def test_adaptive_optimizers_step_the_vectors(golden, optimizer):
    """One step of every adaptive mode of the flat optimizer kernel after a real forward + backward: the three vectors move, stay
    finite, and their padding does not move.  Size of a first step: the bias-corrected modes divide the gradient by its own
    magnitude, about one learning rate per element (NAdam's momentum schedule: below two); RMSProp has no bias correction, so its
    first step is lr g / (sqrt((1 - alpha) g^2) + eps) < lr / sqrt(1 - alpha) = 10 lr at alpha = 0.99, which eps keeps it under by
    parts in 10^5 only.  Asserted: below 10 lr plus 1 % for fp32 rounding."""
    from ultralytics.hip.train import StepPlan
    G = golden("bifpn")
    lr = 0.001
    m = _model(G).train()
    plan = StepPlan(m, 2, 64, nmax=8, optimizer=optimizer, init_scale=1024.0, dynamic_scale=False)
    rt = plan.rt
    p0 = rt.flat_p.clone()
    plan.set_hyper([lr] * 3, 0.9, [0.0, 5e-4, 0.0])
    plan.forward_backward(U.batch(G))
    plan.optimizer_step()
    torch.cuda.synchronize()
    assert float(plan.state[5]) == 1 and float(plan.state[6]) == 0  # the step was taken, not skipped
    for k in U.FUSION_KEYS:
        o = rt.param_off[k]
        d = (rt.flat_p[o:o + 2] - p0[o:o + 2]).abs()
        print(optimizer, k, "moved by", d.tolist())
        assert bool(torch.isfinite(rt.flat_p[o:o + 2]).all()) and float(d.min()) > 0 and float(d.max()) < 10 * lr * 1.01, k
        assert torch.equal(rt.flat_p[o + 2:o + 8], p0[o + 2:o + 8])


def _frozen_step(G, frozen):
    from ultralytics.hip.train import StepPlan
    m = _model(G).train()
    for k, v in m.named_parameters():
        v.requires_grad = k not in frozen
    start = {k: v.detach().clone() for k, v in m.state_dict().items()}
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.set_hyper([0.01] * 3, 0.9, [0.0, 5e-4, 0.0])
    plan.forward_backward(U.batch(G))
    plan.optimizer_step()
    torch.cuda.synchronize()
    return m, plan, start


def test_freeze_11_records_the_frozen_variant(golden):
    """freeze=[11]: model.11.fusion_weight keeps its bits; the list holds three backward launches, the one of row 11 with a null
    workspace, and two finish launches, none writing row 11's gradient slice; the gradients of the layers below equal the unfrozen
    run's byte for byte (the frozen variant writes the same dx)."""
    from ultralytics.engine.trainer import frozen_parameter_names
    G = golden("bifpn")
    names = [k for k, _ in _model(G).named_parameters()]
    frozen = set(frozen_parameter_names(names, [11]))
    assert "model.11.fusion_weight" in frozen and all(k.startswith("model.11.") for k in frozen if ".dfl" not in k)
    m, plan, start = _frozen_step(G, frozen)
    rt = plan.rt
    ops = [o for o in plan.rec_fb.ops if o[0] is not None]
    bwd = [o for o in ops if o[2] == "dy_fusion_backward"]
    fin = [o for o in ops if o[2] == "dy_fusion_wgrad_finish"]
    WS = 21  # argument position of ws (include/dealyolo_hip.h)
    assert len(bwd) == 3 and sorted(o[1][WS] == 0 for o in bwd) == [False, False, True] and len(fin) == 2
    p11 = m.model[11].fusion_weight
    assert [o for o in bwd if o[1][WS] == 0][0][1][WS - 1] == p11.data.data_ptr()  # (the frozen launch is row 11's: it reads its p)
    o11 = rt.param_off["model.11.fusion_weight"]
    slice11 = rt.flat_g[o11:].data_ptr()
    assert all(o[1][3] != slice11 for o in fin) and {o[1][3] for o in fin} == {rt.flat_g[rt.param_off[k]:].data_ptr() for k in U.FUSION_KEYS[1:]}
    sd = m.state_dict()
    for k in frozen:
        assert torch.equal(sd[k], start[k]), f"frozen parameter {k} moved"
    for k in U.FUSION_KEYS[1:]:
        assert not torch.equal(sd[k], start[k]), k
    assert float(rt.flat_g[rt.frozen.bool()].abs().max()) == 0.0 and torch.isfinite(rt.flat_g).all()
    m2, plan2, _ = _frozen_step(G, {k for k in frozen if ".dfl" in k})
    for k0 in ("model.10.conv.weight", "model.8.conv.weight", "model.8.bn.weight", "model.4.cv1.conv.weight", "model.0.conv.weight",
               "model.16.fusion_weight", "model.25.fusion_weight"):
        g1, g2 = dict(m.named_parameters())[k0].grad, dict(m2.named_parameters())[k0].grad
        assert torch.equal(g1, g2) and float(g2.abs().max()) > 0, k0
    assert float(dict(m2.named_parameters())["model.11.fusion_weight"].grad.abs().max()) > 0


def test_frozen_prefix_prunes_nothing_of_the_neck_but_a_frozen_model_prunes_the_layer(golden):
    """Nothing upstream and not the weight itself needing a gradient: no closure.  Layers 0..16 frozen: row 11 and row 16 leave no
    backward launch; row 25 (trainable, fed by the trainable row 17) keeps its own."""
    from ultralytics.engine.trainer import frozen_parameter_names
    G = golden("bifpn")
    names = [k for k, _ in _model(G).named_parameters()]
    frozen = set(frozen_parameter_names(names, 17))
    assert {"model.11.fusion_weight", "model.16.fusion_weight"} <= frozen and "model.25.fusion_weight" not in frozen
    m, plan, start = _frozen_step(G, frozen)
    ops = _names(plan.rec_fb.ops)
    assert [ops.count(k) for k in ("dy_fusion_forward", "dy_fusion_backward", "dy_fusion_wgrad_finish")] == [3, 1, 1]
    sd = m.state_dict()
    assert torch.equal(sd["model.11.fusion_weight"], start["model.11.fusion_weight"]) and not torch.equal(sd["model.25.fusion_weight"], start["model.25.fusion_weight"])


def test_reference_written_checkpoint_runs(golden):
    """attempt_load_weights of tests/golden/ref_ckpt_bifpn.pt (module path ultralytics.nn.extra_modules.block.Fusion): the eval
    forward is the reference's (4 x tol/ckpt/y_eval_*) and EQUALS that of a natively built model with the same fp16-rounded state."""
    from ultralytics.nn.tasks import DetectionModel, attempt_load_weights, torch_safe_load
    G = golden("bifpn")
    a = attempt_load_weights(U.CKPT, device="cuda:0")
    cfg = deepcopy(torch_safe_load(U.CKPT)[0]["model"].yaml)
    b = DetectionModel(cfg, ch=3, verbose=False)
    b.load_state_dict({k: (v.half().float() if v.is_floating_point() else v) for k, v in U.state(G, "ckpt").items()}, strict=True)
    b.cuda().eval()
    x = G.t("batch/img").cuda()
    with torch.no_grad():
        ya, _ = a(x)
        yb, _ = b(x)
    assert torch.equal(ya, yb)
    ref = G.t("ckpt/y_eval")
    eb, ec = relerr(ya[:, :4].cpu(), ref[:, :4]), relerr(ya[:, 4:].cpu(), ref[:, 4:])
    tb, tc = float(G["tol/ckpt/y_eval_box"]), float(G["tol/ckpt/y_eval_cls"])
    print(f"checkpoint eval: box relerr {eb:.2e} (4 x {tb:.2e}) cls relerr {ec:.2e} (4 x {tc:.2e})")
    assert eb < 4 * tb and ec < 4 * tc


def test_public_trainer_last_pt_and_ema(tmp_path):
    """Two epochs through the public trainer: the loss falls, every step is taken, the three vectors move; last.pt holds them (raw and
    EMA copies, which differ after a step) and reloads with them intact."""
    from ultralytics import YOLO
    from ultralytics.data import SyntheticDetection
    torch.manual_seed(0)
    y = YOLO("yolov8n-ASF-P2P2-BiFPN.yaml")
    src = SyntheticDetection(n_batches=4, batch=4, imgsz=64, boxes_per_image=3, wh=(0.1, 0.4), seed=3)
    hist = y.train(data=src, batch=4, imgsz=64, epochs=2, optimizer="SGD", warmup_epochs=0.0, lr0=0.01, nbs=4, hipgraph=True, amp=False,
                   project=str(tmp_path), name="run")
    hist = np.asarray([[float(v) for v in h] for h in hist], dtype=np.float64)
    print("loss items per epoch", hist.tolist())
    assert hist.shape == (2, 3) and np.isfinite(hist).all() and hist[-1].sum() < hist[0].sum()
    plan = y.trainer.plan
    st = plan.state.cpu().numpy()
    assert st[5] == 8 and st[6] == 0 and st[5] == plan.opt_calls, st.tolist()
    last = tmp_path / "run" / "weights" / "last.pt"
    ck = torch.load(last, map_location="cpu", weights_only=False)
    raw = y.trainer.model.state_dict()
    for k in U.FUSION_KEYS:
        assert torch.equal(ck["model"][k], raw[k].cpu()) and ck["model"][k].dtype == torch.float32 and tuple(ck["model"][k].shape) == (2,)
        assert not torch.equal(ck["model"][k], torch.ones(2)), f"{k} never moved"
        assert not torch.equal(ck["ema"][k].float(), ck["model"][k]), f"the EMA copy of {k} equals the raw one"
        assert float((ck["ema"][k].float() - 1).abs().max()) > 0
    back = YOLO(str(last)).model.state_dict()
    for k in U.FUSION_KEYS:
        assert any(torch.equal(back[k].cpu().float(), ck[w][k].float()) for w in ("ema", "model")), k


def test_multi_scale_over_one_arena():
    """multi_scale=True: one recorded launch list per drawn size, all over one arena, the dot products' workspace grown to the largest
    map: every optimizer step takes effect, and the run equals, bit for bit, one whose size plans keep separate buffers."""
    from ultralytics import YOLO
    from ultralytics.data import SyntheticDetection
    from ultralytics.engine.trainer import DetectionTrainer

    def run(share):
        torch.manual_seed(0)
        y = YOLO(os.path.join(CFG_DIR, U.MODEL + ".yaml"))
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


def test_default_graph_launches_no_fusion_kernel(golden):
    from ultralytics.hip.train import StepPlan
    G = golden("bifpn")
    m = _model(G, "yolov8n-ASF-P2P2").train()
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.forward_backward(U.batch(G))
    torch.cuda.synchronize()
    ops = _names(plan.rec_fb.ops)
    assert ops and not [n for n in ops if n.startswith("dy_fusion")]
