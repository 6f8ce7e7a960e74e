"""-m gpu: ADown (reference nn/extra_modules/block.py:4685-4698) on the HIP path.

1. the pool entries (csrc/adown.hip) against the float64 restatement of tests/adown_ref.py (tests/test_host_adown.py ties it to torch's
   avg_pool2d / max_pool2d and autograd, tie cases included), dense and with every operand a channel slice (pitch C + 8, offset 8):

   exact inputs (multiples of 2^-6, |x| < 4: every average is an fp16 number, every gradient sum exact in fp32) and tie inputs
   (multiples of 1/2 in [-2, 2]: at least 10 % of the windows tie, asserted of the input): a, its zero border, p, argmax and dx
   (stored and accumulated) EQUAL the reference; no element is left out.

   normal inputs: the forward within 2^-11 |ref| + 2^-24 of the un-rounded float64 value (one fp16 rounding); the backward against
   the restatement evaluated on the kernel's OWN argmax under

       |got - ref| <= 2^-11 |ref| + k32 2^-23 mag + 2^-24

   mag = the sum of the absolute values of the element's terms, k32 = half the additions on the longest path, counted from the
   orders the kernel file documents before the first GPU run: first half 4 additions (the <= 4 entries of da): k32 = 2; second
   half 4 additions: k32 = 2 (a window's recorded tap names ONE average, so each of the <= 4 windows that can hold one of the
   pixel's averages enters at most once; a kernel that walked averages x windows would have 16 additions, k32 = 8: the bound
   asserted here is the tighter one); + 0.5 for the addition of the stored value when accumulating (mag then includes |old|).
   tests/test_host_adown.py runs an fp32 emulation of the orders against the same bounds.

2. error codes with the canaries intact; each entry twice: the same bits.
3. the module against the reference's fp32 values at 4 x the tolerance the generator measured (tol/<case>/...: the error of a float64
   emulation of this path's storage against the same values); the engine's refusal of a 24-channel input.
4. the graph yolov8n-ASF-P2P2-ADown at 64x64, batch 2, everything at 4 x the tolerance the generator measured for the quantity with
   the same emulation over the whole graph: eval / fused eval / augmented eval / the checkpoint's eval (box rows and class rows), walked
   = traced = replayed; one training step, the ten ADown weight gradients element by element, the updated parameters; captured = eager;
   freeze; a reference-written checkpoint; augment=True; the public trainer; multi_scale; 5. the default graph launches no
   dy_adown_* kernel."""
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

import adown_ref as R
import adown_util as U
from conftest import CFG_DIR
from golden.cases import rnd
from gpu_util import l2err, relerr, run_fwd_bwd

pytestmark = pytest.mark.gpu
POISON = -1234.0  # exactly representable in fp16
GUARD = 3         # canary pixels behind every written tensor
VARIANTS = [(g, "dense") for g in U.KERNEL_CASES] + [(U.SLICED, "sliced")]
IDS = [f"{U.case_id(g)}-{v}" for g, v in VARIANTS]
_REF = {}


# ----------------------------------------------------------------------------- helpers
def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """fp16 device storage of an (N, H, W, C) tensor at channel offset c0 of pitch C + extra, POISON everywhere else and in GUARD
    pixels behind it."""

    def __init__(self, t, sliced, fill=None):
        self.shape, self.C = tuple(t.shape), t.shape[-1]
        self.c0, self.ld = (8, self.C + 8) if sliced else (0, self.C)
        self.npix = int(np.prod(self.shape[:-1]))
        s = torch.full((self.npix + GUARD, self.ld), POISON, dtype=torch.float16)
        s[:self.npix, self.c0:self.c0 + self.C] = (t if fill is None else torch.full_like(t, fill)).reshape(self.npix, self.C).half()
        self.s = s.cuda()

    ptr = property(lambda b: b.s.data_ptr() + 2 * b.c0)

    def get(self):
        return self.s[:self.npix, self.c0:self.c0 + self.C].reshape(self.shape).cpu().double()

    def clean(self):
        """Nothing outside the slice was written."""
        return bool((self.s[self.npix:] == POISON).all()) and bool((self.s[:, :self.c0] == POISON).all()) and \
            bool((self.s[:, self.c0 + self.C:] == POISON).all())


ARG_POISON = 0xEE


def _argbuf(shape):
    n = int(np.prod(shape))
    return torch.full((n + 64,), ARG_POISON, dtype=torch.uint8, device="cuda"), n


def _case(geom, kind):
    """Inputs and float64 references of a kernel case, computed once and shared."""
    key = (geom, kind)
    if key not in _REF:
        x, da, dp = dict(exact=lambda: U.exact_inputs(geom, 1), tie=lambda: U.tie_inputs(geom), normal=lambda: U.normal_inputs(geom, 2))[kind]()
        assert torch.equal(x.half().double(), x) and torch.equal(da.half().double(), da) and torch.equal(dp.half().double(), dp)
        _REF[key] = dict(x=x, da=da, dp=dp, f=R.forward(x), f64=R.forward(x, round16=False))
    return _REF[key]


def _pool(geom, xb, ab, pb, arg):
    from ultralytics.hip import lib
    rc = lib().dy_adown_pool(xb.ptr, xb.ld, ab.ptr, ab.ld, pb.ptr, pb.ld, 0 if arg is None else arg.data_ptr(), *geom, _stream())
    torch.cuda.synchronize()
    return rc


def _pool_bwd(geom, dab, dpb, arg, dxb, acc):
    from ultralytics.hip import lib
    rc = lib().dy_adown_pool_backward(dab.ptr, dab.ld, dpb.ptr, dpb.ld, arg.data_ptr(), dxb.ptr, dxb.ld, acc, *geom, _stream())
    torch.cuda.synchronize()
    return rc


def _run_forward(geom, c, sl, want_arg=True):
    N, H, W, C = geom
    xb = Buf(c["x"], sl)
    x0 = xb.s.clone()
    ab, pb = Buf(c["f"]["a"], sl, fill=POISON), Buf(c["f"]["p"], sl, fill=POISON)
    arg, n = _argbuf(c["f"]["arg"].shape)
    assert _pool(geom, xb, ab, pb, arg if want_arg else None) == 0
    assert ab.clean() and pb.clean() and torch.equal(xb.s, x0) and bool((arg[n:] == ARG_POISON).all())
    if not want_arg:
        assert bool((arg == ARG_POISON).all())
    return ab, pb, arg, n


def _forward_equal(geom, kind, sl):
    c = _case(geom, kind)
    f = c["f"]
    ab, pb, arg, n = _run_forward(geom, c, sl)
    a, p = ab.get(), pb.get()
    N, H, W, C = geom
    assert torch.equal(a, f["a"])
    assert float(a[:, H - 1:].abs().sum()) == 0 and float(a[:, :, W - 1:].abs().sum()) == 0  # the zero border (none on an odd side)
    assert not bool((a == POISON).any()) and not bool((p == POISON).any())
    assert torch.equal(p, f["p"])
    assert torch.equal(arg[:n].view(f["arg"].shape).cpu(), f["arg"])
    # inference: a null arg-max, the same a and p
    ab2, pb2, _, _ = _run_forward(geom, c, sl, want_arg=False)
    assert torch.equal(ab2.s, ab.s) and torch.equal(pb2.s, pb.s)
    return c, arg


def _backward_equal(geom, c, arg, sl):
    N, H, W, C = geom
    ref = R.backward(c["da"], c["dp"], c["f"]["arg"], H, W)["dx"]
    dab, dpb = Buf(c["da"], sl), Buf(c["dp"], sl)
    d0, p0, a0 = dab.s.clone(), dpb.s.clone(), arg.clone()
    dxb = Buf(ref, sl, fill=POISON)
    assert _pool_bwd(geom, dab, dpb, arg, dxb, 0) == 0
    assert torch.equal(dxb.get(), ref.half().double()) and dxb.clean()
    assert torch.equal(dab.s, d0) and torch.equal(dpb.s, p0) and torch.equal(arg, a0)
    old = U.exact_inputs(geom, 3)[0]
    dxa = Buf(old, sl)
    assert _pool_bwd(geom, dab, dpb, arg, dxa, 1) == 0
    assert torch.equal(dxa.get(), (ref + old).half().double()) and dxa.clean()


# ----------------------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("geom,variant", VARIANTS, ids=IDS)
def test_exact_inputs_equal_the_reference(geom, variant):
    sl = variant == "sliced"
    c, arg = _forward_equal(geom, "exact", sl)
    _backward_equal(geom, c, arg, sl)


@pytest.mark.parametrize("geom", U.TIE_CASES, ids=[U.case_id(g) for g in U.TIE_CASES])
def test_tie_inputs_equal_the_reference(geom):
    c = _case(geom, "tie")
    print(geom, f"windows with a tied maximum: {100 * c['f']['ties']:.1f} %")
    assert c["f"]["ties"] >= 0.10  # a condition on the input
    c, arg = _forward_equal(geom, "tie", False)
    _backward_equal(geom, c, arg, False)


@pytest.mark.parametrize("geom,variant", VARIANTS, ids=IDS)
def test_normal_inputs_within_the_counted_bounds(geom, variant):
    """Forward: one fp16 rounding of the float64 value.  Backward: on the kernel's own argmax, k32 = 2 for either half (4 additions
    each), + 0.5 when accumulating (module docstring)."""
    sl = variant == "sliced"
    N, H, W, C = geom
    c = _case(geom, "normal")
    ab, pb, arg, n = _run_forward(geom, c, sl)
    a, p = ab.get(), pb.get()
    U.check("a", a, c["f64"]["a"], torch.zeros_like(a), 0)
    U.check("p", p, c["f64"]["p"], torch.zeros_like(p), 0)
    got_arg = arg[:n].view(c["f"]["arg"].shape).cpu()
    assert int(got_arg.max()) <= 8
    flips = float((got_arg != c["f"]["arg"]).double().mean())
    print(f"argmax differs from the float64 restatement's on {100 * flips:.3f} % of the elements (fp32 sums before the fp16 rounding)")
    b = R.backward(c["da"], c["dp"], got_arg, H, W)
    k32 = U.backward_k32(C)
    dab, dpb = Buf(c["da"], sl), Buf(c["dp"], sl)
    dxb = Buf(b["dx"], sl, fill=POISON)
    assert _pool_bwd(geom, dab, dpb, arg, dxb, 0) == 0 and dxb.clean()
    U.check("dx", dxb.get(), b["dx"], b["mag"] * k32, 1)
    old = U.normal_inputs(geom, 4)[0]
    dxa = Buf(old, sl)
    assert _pool_bwd(geom, dab, dpb, arg, dxa, 1) == 0 and dxa.clean()
    U.check("dx (add)", dxa.get(), b["dx"] + old, (b["mag"] + old.abs()) * (k32 + 0.5), 1)


# ----------------------------------------------------------------------------- 2. refusals and repeat-equality
def test_refused_arguments_leave_the_outputs_alone():
    from ultralytics.hip import lib
    L = lib()
    geom = (2, 8, 8, 32)
    c = _case(geom, "exact")
    xb = Buf(c["x"], False)
    ab, pb = Buf(c["f"]["a"], False, fill=POISON), Buf(c["f"]["p"], False, fill=POISON)
    arg, n = _argbuf(c["f"]["arg"].shape)
    dxb = Buf(c["x"], False, fill=POISON)
    ARG, ALIGN = -1, -3

    def fwd(x=xb.ptr, ldx=32, a=ab.ptr, lda=16, p=pb.ptr, ldp=16, am=arg.data_ptr(), n_=2, H=8, W=8, C=32):
        return L.dy_adown_pool(x, ldx, a, lda, p, ldp, am, n_, H, W, C, _stream())

    def bwd(da=ab.ptr, ldda=16, dp=pb.ptr, lddp=16, am=arg.data_ptr(), dx=dxb.ptr, lddx=32, n_=2, H=8, W=8, C=32):
        return L.dy_adown_pool_backward(da, ldda, dp, lddp, am, dx, lddx, 0, n_, H, W, C, _stream())

    assert [fwd(x=0), fwd(a=0), fwd(p=0), fwd(n_=0), fwd(H=1), fwd(W=1), fwd(ldx=24), fwd(lda=8), fwd(ldp=8)] == [ARG] * 9
    assert [fwd(C=24), fwd(C=8), fwd(ldx=36), fwd(lda=20), fwd(ldp=20), fwd(x=xb.ptr + 8), fwd(a=ab.ptr + 8), fwd(p=pb.ptr + 8),
            fwd(am=arg.data_ptr() + 8)] == [ALIGN] * 9
    assert [bwd(da=0), bwd(dp=0), bwd(am=0), bwd(dx=0), bwd(n_=0), bwd(H=1), bwd(W=1), bwd(lddx=24), bwd(ldda=8), bwd(lddp=8)] == [ARG] * 10
    assert [bwd(C=24), bwd(C=8), bwd(lddx=36), bwd(ldda=20), bwd(lddp=20), bwd(da=ab.ptr + 8), bwd(dp=pb.ptr + 8), bwd(dx=dxb.ptr + 8),
            bwd(am=arg.data_ptr() + 8)] == [ALIGN] * 9
    torch.cuda.synchronize()
    for b in (ab, pb, dxb):
        assert bool((b.s == POISON).all())
    assert bool((arg == ARG_POISON).all())


@pytest.mark.parametrize("geom", [(2, 7, 9, 16), (2, 18, 66, 64)], ids=["2x7x9x16", "2x18x66x64"])
def test_two_launches_give_the_same_bits(geom):
    c = _case(geom, "normal")
    outs = []
    for _ in range(2):
        ab, pb, arg, n = _run_forward(geom, c, False)
        dab, dpb = Buf(c["da"], False), Buf(c["dp"], False)
        old = U.normal_inputs(geom, 4)[0]
        dxb, dxa = Buf(c["x"], False, fill=POISON), Buf(old, False)
        assert _pool_bwd(geom, dab, dpb, arg, dxb, 0) == 0 and _pool_bwd(geom, dab, dpb, arg, dxa, 1) == 0
        outs.append((ab.s, pb.s, arg, dxb.s, dxa.s))
    for u, v in zip(*outs):
        assert torch.equal(u, v)


def test_grid_stride_loop_repeats_the_small_case():
    """Both launches cap their grid at 8192 workgroups of 256 work items; beyond 2^21 items a work item walks on by the grid's size.
    Images are independent, so the (2, 18, 66, 64) case repeated 884 times along N (2.1 M forward items, 8.4 M backward items) must
    give the small case's outputs 884 times over: compared on the device, no large array on the host."""
    from ultralytics.hip import lib
    geom, rep = (2, 18, 66, 64), 884
    N, H, W, C = geom
    assert rep * N * (H // 2) * (W // 2) * (C // 16) > 8192 * 256
    c = _case(geom, "exact")
    ab, pb, arg, n = _run_forward(geom, c, False)
    dab, dpb = Buf(c["da"], False), Buf(c["dp"], False)
    dxb = Buf(c["x"], False, fill=POISON)
    assert _pool_bwd(geom, dab, dpb, arg, dxb, 0) == 0
    small = [ab.s[:ab.npix], pb.s[:pb.npix], arg[:n], dxb.s[:dxb.npix]]
    big = lambda b: b.s[:b.npix].repeat(rep, 1).contiguous()  # noqa: E731
    x, da, dp = big(Buf(c["x"], False)), big(dab), big(dpb)
    a, p, dx = torch.full_like(da, POISON), torch.full_like(dp, POISON), torch.full_like(x, POISON)
    am = torch.full((rep * n,), ARG_POISON, dtype=torch.uint8, device="cuda")
    L, g = lib(), (rep * N, H, W, C)
    assert L.dy_adown_pool(x.data_ptr(), C, a.data_ptr(), C // 2, p.data_ptr(), C // 2, am.data_ptr(), *g, _stream()) == 0
    assert L.dy_adown_pool_backward(da.data_ptr(), C // 2, dp.data_ptr(), C // 2, am.data_ptr(), dx.data_ptr(), C, 0, *g, _stream()) == 0
    torch.cuda.synchronize()
    for got, want in zip((a, p, am, dx), small):
        assert torch.equal(got.view(rep, *want.shape), want.unsqueeze(0).expand(rep, *want.shape))


# ----------------------------------------------------------------------------- 3. the module against the reference
@pytest.mark.parametrize("case", list(U.MODULE_CASES))
def test_module_vs_golden(golden, case):
    """l2err of y, gx and every parameter gradient below 4 x the tolerance the generator measured for the case.  The factor pays for
    another fp32 summation order and for fp32-against-float64 arithmetic, not for another algorithm.  Running statistics after the
    one forward: 2e-3, as tests/test_gpu_spd.py."""
    from ultralytics.nn.extra_modules.block import ADown
    G = golden("adown")
    c1, c2, H, W = U.MODULE_CASES[case]
    p = f"mod/{case}"
    seed = int(G[f"{p}/seed"])
    m = ADown(c1, c2)
    m.load_state_dict(U.state(G, p), strict=True)
    want = dict(y=G.t(f"{p}/y"), gx=G.t(f"{p}/gx"))
    x, gy = rnd(10 * seed, 2, c1, H, W), rnd(10 * seed + 1, *want["y"].shape)
    y, gxs, rt = run_fwd_bwd(m, [x], gy)
    got = dict(y=y, gx=gxs[0])
    for n, q in m.named_parameters():
        got[f"gp/{n}"], want[f"gp/{n}"] = q.grad.float().cpu(), G.t(f"{p}/gp/{n}")
    errs = {n: l2err(got[n].reshape(want[n].shape), want[n]) for n in got}
    tols = {n: float(G[f"tol/{case}/{n}"]) for n in got}
    print(case, {n: f"{errs[n]:.2e} (4 x {tols[n]:.2e})" for n in errs})
    for n in errs:
        assert errs[n] < 4 * tols[n], n
    bufs = dict(m.named_buffers())
    for n in G.keys(f"{p}/buf/"):
        assert relerr(bufs[n.split("/buf/")[1]], G.t(n)) < 2e-3, n


def test_engine_refuses_a_24_channel_input_by_name():
    from ultralytics.nn.extra_modules.block import ADown
    m = ADown(32, 32).cuda()
    rt = m._runtime(torch.device("cuda", 0))
    eng = rt.eng
    x = eng.wrap_act(torch.zeros(1, 4, 4, 32, dtype=torch.float16, device="cuda"))
    with pytest.raises(NotImplementedError, match=r"ADown.*an input of 24 channels.*supported: c1 % 16 == 0"):
        eng.adown(rt.spec(m.cv1), rt.spec(m.cv2), x.sub(0, 24))
    with pytest.raises(NotImplementedError, match=r"ADown.*on a 1x4 map"):
        eng.adown(rt.spec(m.cv1), rt.spec(m.cv2), eng.wrap_act(torch.zeros(1, 1, 4, 32, dtype=torch.float16, device="cuda")))
    rt.pack_all(True)
    y = eng.adown(rt.spec(m.cv1), rt.spec(m.cv2), x)  # ... and the supported call runs
    torch.cuda.synchronize()
    assert (y.N, y.H, y.W, y.C) == (1, 2, 2, 32)


# ----------------------------------------------------------------------------- 4. the graph against the reference
def _model(G, name=U.MODEL):
    from ultralytics.nn.tasks import DetectionModel
    m = DetectionModel(os.path.join(CFG_DIR, name + ".yaml"), ch=3, verbose=False)
    if name == U.MODEL:
        m.load_state_dict(U.state(G, U.MODEL), strict=True)
    return m.cuda()


def _names(ops):
    return [o[2] for o in ops if o[0] is not None]


def test_eval_and_fused_eval_vs_golden(golden):
    """Box rows and class scores at 4 x the generator's measured tolerances (tol/<model>/y_eval_*, y_eval_fused_*); the second call of
    a geometry is traced into an InferPlan, the third replays it: all three bit for bit, five dy_adown_pool launches in the list, each
    with a null arg-max."""
    G = golden("adown")
    m = _model(G).eval()
    x = G.t("batch/img").cuda()
    for key in ("y_eval", "y_eval_fused"):
        if key == "y_eval_fused":
            m.fuse()
            assert not hasattr(m.model[1].cv1, "bn")
        ref = G.t(f"{U.MODEL}/{key}")
        with torch.no_grad():
            y1, _ = m(x)   # walked
            assert not m._infer_plans["plans"]
            y2, _ = m(x)   # traced into a plan
            plan = m._infer_plans["plans"][(2, 3, 64, 64)]
            y3, _ = m(x)   # replayed
        torch.cuda.synchronize()
        pools = [o for o in plan.rec.ops if o[0] is not None and o[2] == "dy_adown_pool"]
        assert len(pools) == 5 and all(o[1][6] == 0 for o in pools)
        assert torch.equal(y1, y2) and torch.equal(y1, y3)
        assert y1.shape == ref.shape
        eb, ec = relerr(y1[:, :4].cpu(), ref[:, :4]), relerr(y1[:, 4:].cpu(), ref[:, 4:])
        tb, tc = float(G[f"tol/{U.MODEL}/{key}_box"]), float(G[f"tol/{U.MODEL}/{key}_cls"])
        print(f"{key}: box relerr {eb:.2e} (4 x {tb:.2e}) cls relerr {ec:.2e} (4 x {tc:.2e})")
        assert eb < 4 * tb and ec < 4 * tc


def test_train_step_vs_golden(golden):
    """One training step: loss items, loss, gradient norms (median / max of the relative error, tests/test_gpu_carafe.py's formula),
    the first layer's gradient, the gradients of the ten ADown convolution weights element by element (l2err: a norm does not see a
    wrong direction) and, after one clipped SGD-nesterov step, the norms of every tensor's change, at 4 x the tolerances the
    generator measured for them (tol/<model>/...)."""
    from ultralytics.hip.train import StepPlan
    G = golden("adown")
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
    assert ops.count("dy_adown_pool") == 5 and ops.count("dy_adown_pool_backward") == 5
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
    print("items", s[5:8].tolist(), ref_items.tolist())
    print({k: f"{got[k]:.2e} (4 x {tol[k]:.2e})" for k in got}, "worst gradient norm:", names[int(rel.argmax())])
    for i in U.ADOWN_LAYERS:
        for cv in ("cv1", "cv2"):
            j = names.index(f"model.{i}.{cv}.conv.weight")
            e, t = l2err(params[names[j]].grad.float().cpu() / scale, G.t(f"{U.MODEL}/grad/{names[j]}")), float(G[f"tol/{U.MODEL}/grad/{names[j]}"])
            got[f"grad/{names[j]}"], tol[f"grad/{names[j]}"] = e, t
            print(names[j], f"l2 {float(l2[j]):.4e} reference {float(ref[j]):.4e} rel {float(rel[j]):.2e}; l2err {e:.2e} (4 x {t:.2e})")
    for k in got:
        assert got[k] < 4 * tol[k], k


def test_captured_step_equals_the_eager_step(golden):
    """One StepPlan step replayed as a hipGraph against the eager tape step of another plan on the same state and batch: the same
    launches, no atomics in the pool kernels, so loss items and ALL gradients are EQUAL."""
    from ultralytics.hip.train import StepPlan
    G = golden("adown")
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
        ops = _names(plan.rec_fb.ops)
        assert ops.count("dy_adown_pool") == 5 and ops.count("dy_adown_pool_backward") == 5
        outs.append((plan.rt.flat_g.clone(), plan.crit.scalars.clone()))
    assert torch.isfinite(outs[0][0]).all() and float(outs[0][0].abs().max()) > 0
    assert torch.equal(outs[0][1][5:9], outs[1][1][5:9]) and torch.equal(outs[0][0], outs[1][0])


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


A_BWD_DX = 5  # argument position (include/dealyolo_hip.h): dx of dy_adown_pool_backward


def _specs(plan, m, i):
    return plan.rt.spec(m.model[i].cv1), plan.rt.spec(m.model[i].cv2)


def test_freeze_4_prunes_rows_1_and_3(golden):
    """freeze=4 (layers 0-3): rows 1 and 3 are frozen and nothing trainable lies upstream of them, so they leave nothing on the tape:
    no pool backward, no weight gradient, no arg-max map (their forward launches pass a null one), their parameters do not move;
    rows 5, 18, 21 keep everything."""
    from ultralytics.engine.trainer import frozen_parameter_names
    G = golden("adown")
    names = [k for k, _ in _model(G).named_parameters()]
    frozen = set(frozen_parameter_names(names, 4))
    assert {"model.1.cv1.conv.weight", "model.3.cv2.bn.bias"} <= frozen and "model.5.cv1.conv.weight" not in frozen
    m, plan, start = _frozen_step(G, frozen)
    rt = plan.rt
    for i in (1, 3):
        assert not any(sp.trainable for sp in _specs(plan, m, i))
    for i in (5, 18, 21):
        assert all(sp.trainable for sp in _specs(plan, m, i))
    ops = [o for o in plan.rec_fb.ops if o[0] is not None]
    pools = [o for o in ops if o[2] == "dy_adown_pool"]
    assert len(pools) == 5 and [o[1][6] != 0 for o in pools] == [False, False, True, True, True]
    assert _names(ops).count("dy_adown_pool_backward") == 3
    ws = {id(s) for s in plan.wgrad_specs}
    for i in (1, 3):
        assert not any(id(sp) in ws for sp in _specs(plan, m, i))
    for i in (5, 18, 21):
        assert all(id(sp) in ws for sp in _specs(plan, m, i))
    frozen_g = {sp.gweight.data_ptr() for i in (1, 3) for sp in _specs(plan, m, i)}
    for fn, args, name, _sid in ops:
        assert not [a for a in args if isinstance(a, int) and a in frozen_g], f"{name} writes a frozen weight's gradient"
    sd = m.state_dict()
    for k in frozen:
        assert torch.equal(sd[k], start[k]), f"frozen parameter {k} moved"
    for i in (5, 18, 21):
        for cv in ("cv1", "cv2"):
            assert not torch.equal(sd[f"model.{i}.{cv}.conv.weight"], start[f"model.{i}.{cv}.conv.weight"]), (i, cv)
    assert float(rt.flat_g[rt.frozen.bool()].abs().max()) == 0.0 and torch.isfinite(rt.flat_g).all()


def test_frozen_row_with_a_trainable_prefix_keeps_its_input_gradient(golden):
    """freeze=[3], layer 2 trainable: row 3's two weight-gradient launches are pruned, its two input gradients and its pool backward
    run, and the gradient everything upstream receives equals the unfrozen step's."""
    from ultralytics.engine.trainer import frozen_parameter_names
    G = golden("adown")
    names = [k for k, _ in _model(G).named_parameters()]
    frozen = set(frozen_parameter_names(names, [3]))
    assert frozen and all(k.startswith("model.3.") for k in frozen if ".dfl" not in k)
    m, plan, start = _frozen_step(G, frozen)
    sp3 = _specs(plan, m, 3)
    assert not any(sp.trainable for sp in sp3)
    ops = [o for o in plan.rec_fb.ops if o[0] is not None]
    assert _names(ops).count("dy_adown_pool") == 5 and _names(ops).count("dy_adown_pool_backward") == 5
    ws = {id(s) for s in plan.wgrad_specs}
    assert not any(id(sp) in ws for sp in sp3)
    gptrs = {sp.gweight.data_ptr() for sp in sp3}
    for fn, args, name, _sid in ops:
        assert not [a for a in args if isinstance(a, int) and a in gptrs], f"{name} writes a frozen weight's gradient"
    sd = m.state_dict()
    for k in frozen:
        assert torch.equal(sd[k], start[k])
    m2, plan2, _ = _frozen_step(G, {k for k in frozen if ".dfl" in k})
    # the frozen row runs the same reduce, d(raw) and input-gradient launches on the same operands and hands them to the same pool
    # backward, all of them deterministic: EQUAL
    for k0 in ("model.2.cv1.conv.weight", "model.2.m.0.cv2.bn.weight", "model.1.cv1.conv.weight", "model.1.cv2.bn.bias", "model.0.conv.weight"):
        g1, g2 = dict(m.named_parameters())[k0].grad, dict(m2.named_parameters())[k0].grad
        assert torch.equal(g1, g2) and float(g2.abs().max()) > 0, k0


def test_reference_written_checkpoint_runs(golden):
    """attempt_load_weights of tests/golden/ref_ckpt_adown.pt (module path ultralytics.nn.extra_modules.block.ADown): the eval forward
    is the reference's (4 x tol/ckpt/y_eval_*) and EQUALS that of a natively built model with the same fp16-rounded state."""
    from ultralytics.nn.tasks import DetectionModel, attempt_load_weights, torch_safe_load
    G = golden("adown")
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


def test_augmented_forward_runs(golden):
    """model(x, augment=True): walked, recorded, replayed give the same bits; against the reference's augmented forward at 4 x the
    generator's measured tolerances (tol/<model>/y_aug_*).  The scaled passes run on odd-sized maps."""
    G = golden("adown")
    m = _model(G).eval()
    x = G.t("batch/img").cuda()
    want = G.t(f"{U.MODEL}/y_aug")
    ys = []
    for _ in range(3):
        y, second = m(x, augment=True)
        assert second is None and tuple(y.shape) == tuple(want.shape)
        ys.append(y.clone())
    eb, ec = relerr(ys[0][:, :4], want[:, :4]), relerr(ys[0][:, 4:], want[:, 4:])
    tb, tc = float(G[f"tol/{U.MODEL}/y_aug_box"]), float(G[f"tol/{U.MODEL}/y_aug_cls"])
    print(f"augment: box relerr {eb:.2e} (4 x {tb:.2e}), class relerr {ec:.2e} (4 x {tc:.2e})")
    assert eb < 4 * tb and ec < 4 * tc
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


def test_two_epochs_through_the_public_trainer():
    from ultralytics import YOLO
    from ultralytics.data import SyntheticDetection
    torch.manual_seed(0)
    y = YOLO("yolov8n-ASF-P2P2-ADown.yaml")
    w0 = {k: v.detach().clone() for k, v in y.model.state_dict().items()}
    src = SyntheticDetection(n_batches=4, batch=4, imgsz=64, boxes_per_image=3, wh=(0.1, 0.4), seed=3)
    hist = y.train(data=src, batch=4, imgsz=64, epochs=2, optimizer="SGD", warmup_epochs=0.0, lr0=0.01, nbs=4, hipgraph=True, amp=False)
    hist = np.asarray([[float(v) for v in h] for h in hist], dtype=np.float64)
    print("loss items per epoch", hist.tolist())
    assert hist.shape == (2, 3) and np.isfinite(hist).all()
    assert hist[-1].sum() < hist[0].sum()
    plan = y.trainer.plan
    st = plan.state.cpu().numpy()
    assert st[5] == 8 and st[6] == 0 and st[5] == plan.opt_calls, st.tolist()
    w1 = y.trainer.model.state_dict()
    keys = [f"model.{i}.{cv}.conv.weight" for i in U.ADOWN_LAYERS for cv in ("cv1", "cv2")]
    still = [k for k in keys if torch.equal(w1[k].cpu(), w0[k].cpu())]
    assert not still, f"ADown weights that never moved: {still}"
    assert torch.isfinite(plan.rt.flat_g).all()


def test_soap_steps_the_graph():
    """optimizer='SOAP' needs nothing new (the ADown weights are dense (c, c1 / 2, k, k) tensors): two epochs of four batches, every
    step taken, finite losses, every ADown weight moved."""
    from ultralytics import YOLO
    from ultralytics.data import SyntheticDetection
    torch.manual_seed(0)
    y = YOLO(os.path.join(CFG_DIR, U.MODEL + ".yaml"))
    w0 = {k: v.detach().clone() for k, v in y.model.state_dict().items()}
    src = SyntheticDetection(n_batches=4, batch=4, imgsz=64, boxes_per_image=3, wh=(0.1, 0.4), seed=3)
    hist = y.train(data=src, batch=4, imgsz=64, epochs=2, optimizer="SOAP", warmup_epochs=0.0, lr0=0.003, nbs=4, amp=False)
    plan = y.trainer.plan
    assert plan.soap and plan._soap is not None
    taken, skipped, _ = plan.check_progress()
    assert (taken, skipped) == (8, 0) and all(torch.isfinite(torch.as_tensor(h)).all() for h in hist)
    w1 = y.trainer.model.state_dict()
    keys = [f"model.{i}.{cv}.conv.weight" for i in U.ADOWN_LAYERS for cv in ("cv1", "cv2")]
    still = [k for k in keys if torch.equal(w1[k].cpu(), w0[k].cpu())]
    assert not still, f"ADown weights that never moved: {still}"


def test_multi_scale_over_one_arena():
    """multi_scale=True: one recorded launch list per drawn size (32 and 96 among them: other map sizes through every pool), all over
    one arena -- the arg-max maps are step-local and live there too: every optimizer step takes effect, and the run equals, bit for
    bit, one whose size plans keep separate buffers."""
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


# ----------------------------------------------------------------------------- 5. the default graph
def test_default_graph_launches_no_adown_kernel(golden):
    from ultralytics.hip.train import StepPlan
    G = golden("adown")
    m = _model(G, "yolov8n-ASF-P2P2").train()
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.forward_backward(U.batch(G))
    torch.cuda.synchronize()
    ops = _names(plan.rec_fb.ops)
    assert ops and not [n for n in ops if n.startswith("dy_adown")]
