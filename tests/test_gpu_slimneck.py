"""-m gpu: the slim-neck blocks GSConv / GSBottleneck / VoVGSCSP (reference nn/extra_modules/block.py:886-967) on the HIP path.

1. the shuffle entries (csrc/gsconv.hip) against the restatement of tests/slimneck_ref.py (tests/test_host_slimneck.py ties it to the
   reference's reshape / permute form and to autograd), per element, no element left out.  They are permutations, so everything
   stored is BIT-EQUAL to the reference: the forward, the stored backward, and the accumulating backward on exact inputs (multiples
   of 2^-6, |v| < 4: old + v is an fp16 number).  The accumulating backward on normal inputs is one fp32 addition and one fp16
   rounding: |got - ref| <= 2^-11 |ref| + 2^-24.  Each destination null in turn: the other's bytes as with both, the null side's
   buffer untouched.  One case runs with every operand a channel slice (pitch C + 8, offset 8) under POISON canaries; one case is
   larger than the capped grid, so a work item's grid-stride loop runs a second time.
2. error codes with the canaries intact; each entry twice: the same bits.
3. the modules against the reference's fp32 values at 4 x the tolerance the generator measured (tol/<case>/...: the error of a float64
   emulation of this path's storage against the same values).
4. the graph yolov8n-ASF-P2P2-SlimNeck at 64x64, batch 2, everything at 4 x the tolerance the generator measured for the quantity with
   the same emulation over the whole graph: eval / fused eval / augmented eval / the checkpoint's eval (box rows and class rows), walked
   = traced = replayed; one training step; captured = eager; freeze; multi_scale; the public trainer with weight decay, through which
   every ``res.*`` tensor keeps its bits; SOAP's refusal; 5. the default graph launches no dy_gs_* kernel."""
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

import slimneck_ref as R
import slimneck_util as U
from conftest import CFG_DIR
from golden.cases import rnd
from gpu_util import l2err, relerr, run_fwd_bwd

pytestmark = pytest.mark.gpu
POISON = -1234.0  # exactly representable in fp16
GUARD = 3         # canary pixels behind every written tensor
VARIANTS = [(g, "dense") for g in U.KERNEL_CASES] + [(U.SLICED, "sliced")]
IDS = [f"{U.case_id(g)}-{v}" for g, v in VARIANTS]
N_SHUFFLES = len(U.GS_LAYERS) + 2 * len(U.VOV_LAYERS)  # one per GSConv: the two rows and the two inside every GSBottleneck
_REF = {}


# ----------------------------------------------------------------------------- helpers
def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """fp16 device storage of an (N, H, W, C) tensor at channel offset c0 of pitch C + extra, POISON everywhere else and in GUARD
    pixels behind it.  Built and compared on the device (the large case stays there)."""

    def __init__(self, t, sliced, fill=None):
        self.shape, self.C = tuple(t.shape), t.shape[-1]
        self.c0, self.ld = (8, self.C + 8) if sliced else (0, self.C)
        self.npix = int(np.prod(self.shape[:-1]))
        self.s = torch.full((self.npix + GUARD, self.ld), POISON, dtype=torch.float16, device="cuda")
        if fill is None:
            self.s[:self.npix, self.c0:self.c0 + self.C] = t.reshape(self.npix, self.C).half().cuda()
        else:
            self.s[:self.npix, self.c0:self.c0 + self.C] = fill

    ptr = property(lambda b: b.s.data_ptr() + 2 * b.c0)

    def get(self):
        return self.s[:self.npix, self.c0:self.c0 + self.C].reshape(self.shape)

    def clean(self):
        """Nothing outside the slice was written."""
        return bool((self.s[self.npix:] == POISON).all()) and bool((self.s[:, :self.c0] == POISON).all()) and \
            bool((self.s[:, self.c0 + self.C:] == POISON).all())


def _case(geom, kind):
    """Inputs (fp16, on the device) and references of a kernel case, computed once, shared and left unchanged."""
    key = (geom, kind)
    if key not in _REF:
        t = {k: v.cuda() for k, v in (U.exact_inputs(geom, 1) if kind == "exact" else U.normal_inputs(geom, 2)).items()}
        t["y"] = R.forward(t["x1"], t["d"])
        t["g1"], t["gd"] = R.backward(t["dy"])
        _REF[key] = t
    return _REF[key]


def _fwd(geom, x1b, db, yb):
    from ultralytics.hip import lib
    rc = lib().dy_gs_shuffle_forward(x1b.ptr, x1b.ld, db.ptr, db.ld, yb.ptr, yb.ld, *geom, _stream())
    torch.cuda.synchronize()
    return rc


def _bwd(geom, dyb, g1b, acc1, gdb, accd):
    from ultralytics.hip import lib
    rc = lib().dy_gs_shuffle_backward(dyb.ptr, dyb.ld, 0 if g1b is None else g1b.ptr, 0 if g1b is None else g1b.ld, acc1,
                                      0 if gdb is None else gdb.ptr, 0 if gdb is None else gdb.ld, accd, *geom, _stream())
    torch.cuda.synchronize()
    return rc


def _within_one_rounding(what, got, ref64):
    """|got - ref| <= 2^-11 |ref| + 2^-24 on EVERY element (one fp32 addition of two fp16 numbers is exact or rounds far below it)."""
    got, ref64 = got.double(), ref64.double()
    bound = 2.0 ** -11 * ref64.abs() + 2.0 ** -24
    err = (got - ref64).abs()
    worst = float((err / bound).max())
    print(f"{what}: max err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, f"{what}: {int((err > bound).sum())} of {err.numel()} elements beyond the bound"


# ----------------------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("geom,variant", VARIANTS, ids=IDS)
def test_forward_equals_the_reference(geom, variant):
    sl = variant == "sliced"
    c = _case(geom, "normal")
    x1b, db = Buf(c["x1"], sl), Buf(c["d"], sl)
    x0, d0 = x1b.s.clone(), db.s.clone()
    yb = Buf(c["y"], sl, fill=POISON)
    assert _fwd(geom, x1b, db, yb) == 0
    assert torch.equal(yb.get(), c["y"]) and yb.clean()
    assert torch.equal(x1b.s, x0) and torch.equal(db.s, d0)


@pytest.mark.parametrize("geom,variant", VARIANTS, ids=IDS)
def test_backward_stored_equals_the_reference(geom, variant):
    sl = variant == "sliced"
    c = _case(geom, "normal")
    dyb = Buf(c["dy"], sl)
    dy0 = dyb.s.clone()
    g1b, gdb = Buf(c["g1"], sl, fill=POISON), Buf(c["gd"], sl, fill=POISON)
    assert _bwd(geom, dyb, g1b, 0, gdb, 0) == 0
    assert torch.equal(g1b.get(), c["g1"]) and torch.equal(gdb.get(), c["gd"]) and g1b.clean() and gdb.clean()
    assert torch.equal(dyb.s, dy0)
    # mixed flags: one destination stored, the other accumulated (exact inputs below cover both accumulated)
    e = _case(geom, "exact")
    dyb = Buf(e["dy"], sl)
    g1b, gdb = Buf(e["old1"], sl), Buf(e["gd"], sl, fill=POISON)
    assert _bwd(geom, dyb, g1b, 1, gdb, 0) == 0
    assert torch.equal(g1b.get(), (e["old1"].float() + e["g1"].float()).half()) and torch.equal(gdb.get(), e["gd"]) and g1b.clean() and gdb.clean()


@pytest.mark.parametrize("geom,variant", VARIANTS, ids=IDS)
def test_backward_accumulated_on_exact_inputs_is_bit_equal(geom, variant):
    sl = variant == "sliced"
    c = _case(geom, "exact")
    s1, sd = c["old1"].double() + c["g1"].double(), c["oldd"].double() + c["gd"].double()
    assert torch.equal(s1.half().double(), s1) and torch.equal(sd.half().double(), sd)  # a condition on the inputs: the sums are fp16 numbers
    dyb = Buf(c["dy"], sl)
    g1b, gdb = Buf(c["old1"], sl), Buf(c["oldd"], sl)
    assert _bwd(geom, dyb, g1b, 1, gdb, 1) == 0
    assert torch.equal(g1b.get(), s1.half()) and torch.equal(gdb.get(), sd.half()) and g1b.clean() and gdb.clean()


@pytest.mark.parametrize("geom,variant", VARIANTS, ids=IDS)
def test_backward_accumulated_on_normal_inputs_is_one_rounding(geom, variant):
    sl = variant == "sliced"
    c = _case(geom, "normal")
    dyb = Buf(c["dy"], sl)
    g1b, gdb = Buf(c["old1"], sl), Buf(c["oldd"], sl)
    assert _bwd(geom, dyb, g1b, 1, gdb, 1) == 0 and g1b.clean() and gdb.clean()
    _within_one_rounding("dx1 (add)", g1b.get(), c["old1"].double() + c["g1"].double())
    _within_one_rounding("dd (add)", gdb.get(), c["oldd"].double() + c["gd"].double())


@pytest.mark.parametrize("geom,variant", VARIANTS, ids=IDS)
def test_each_destination_null_in_turn(geom, variant):
    """A null destination is skipped: the other side's bytes are what a call with both gives, and the skipped side's buffer -- handed to
    nothing -- keeps every canary."""
    sl = variant == "sliced"
    c = _case(geom, "normal")
    dyb = Buf(c["dy"], sl)
    both1, bothd = Buf(c["old1"], sl), Buf(c["oldd"], sl)
    assert _bwd(geom, dyb, both1, 1, bothd, 0) == 0
    idle = Buf(c["g1"], sl, fill=POISON)
    only1 = Buf(c["old1"], sl)
    assert _bwd(geom, dyb, only1, 1, None, 0) == 0
    assert torch.equal(only1.s, both1.s) and bool((idle.s == POISON).all())
    onlyd = Buf(c["oldd"], sl)
    assert _bwd(geom, dyb, None, 1, onlyd, 0) == 0
    assert torch.equal(onlyd.s, bothd.s) and bool((idle.s == POISON).all())
    assert _bwd(geom, dyb, None, 0, None, 0) == 0  # both null: nothing is launched


# ----------------------------------------------------------------------------- 2. refusals and repeat-equality
def test_refused_arguments_leave_the_outputs_alone():
    from ultralytics.hip import lib
    L = lib()
    geom = (2, 4, 4, 16)
    c = _case(geom, "normal")
    x1b, db, dyb = Buf(c["x1"], False), Buf(c["d"], False), Buf(c["dy"], False)
    yb = Buf(c["y"], False, fill=POISON)
    g1b, gdb = Buf(c["g1"], False, fill=POISON), Buf(c["gd"], False, fill=POISON)
    ARG, ALIGN = -1, -3

    def fwd(x1=x1b.ptr, ld1=16, d=db.ptr, ldd=16, y=yb.ptr, ldy=32, n_=2, H=4, W=4, c_=16):
        return L.dy_gs_shuffle_forward(x1, ld1, d, ldd, y, ldy, n_, H, W, c_, _stream())

    def bwd(dy=dyb.ptr, ldy=32, dx1=g1b.ptr, ld1=16, dd=gdb.ptr, ldd=16, n_=2, H=4, W=4, c_=16):
        return L.dy_gs_shuffle_backward(dy, ldy, dx1, ld1, 0, dd, ldd, 0, n_, H, W, c_, _stream())

    assert [fwd(x1=0), fwd(d=0), fwd(y=0), fwd(n_=0), fwd(H=0), fwd(W=0), fwd(c_=0), fwd(c_=4), fwd(ld1=8), fwd(ldd=8), fwd(ldy=24)] == [ARG] * 11
    assert [fwd(c_=12), fwd(ld1=20), fwd(ldd=20), fwd(ldy=36), fwd(x1=x1b.ptr + 8), fwd(d=db.ptr + 8), fwd(y=yb.ptr + 8)] == [ALIGN] * 7
    assert [bwd(dy=0), bwd(n_=0), bwd(H=0), bwd(W=0), bwd(c_=0), bwd(c_=4), bwd(ld1=8), bwd(ldd=8), bwd(ldy=24)] == [ARG] * 9
    assert [bwd(c_=12), bwd(ld1=20), bwd(ldd=20), bwd(ldy=36), bwd(dy=dyb.ptr + 8), bwd(dx1=g1b.ptr + 8), bwd(dd=gdb.ptr + 8)] == [ALIGN] * 7
    torch.cuda.synchronize()
    for b in (yb, g1b, gdb):
        assert bool((b.s == POISON).all())


@pytest.mark.parametrize("geom", [(1, 2, 3, 24), (1, 5, 7, 32)], ids=["1x2x3x24", "1x5x7x32"])
def test_two_launches_give_the_same_bits(geom):
    c = _case(geom, "normal")
    outs = []
    for _ in range(2):
        x1b, db, dyb = Buf(c["x1"], False), Buf(c["d"], False), Buf(c["dy"], False)
        yb = Buf(c["y"], False, fill=POISON)
        g1b, gdb = Buf(c["g1"], False, fill=POISON), Buf(c["gd"], False, fill=POISON)
        a1b, adb = Buf(c["old1"], False), Buf(c["oldd"], False)
        assert _fwd(geom, x1b, db, yb) == 0 and _bwd(geom, dyb, g1b, 0, gdb, 0) == 0 and _bwd(geom, dyb, a1b, 1, adb, 1) == 0
        outs.append((yb.s, g1b.s, gdb.s, a1b.s, adb.s))
    for u, v in zip(*outs):
        assert torch.equal(u, v)


# ----------------------------------------------------------------------------- 3. the modules against the reference
def _build(case):
    from ultralytics.nn.extra_modules import block as B
    cls, args, H, W = U.MODULE_CASES[case]
    return getattr(B, cls)(*args), args[0], H, W


@pytest.mark.parametrize("case", list(U.MODULE_CASES))
def test_module_vs_golden(golden, case):
    """l2err of y, gx and every parameter gradient, and the relerr of every running statistic after the one forward, below 4 x the
    tolerance the generator measured for that quantity of the case (tol/<case>/..., tol/<case>/buf/...).  The factor pays for another
    fp32 summation order and for fp32-against-float64 arithmetic, not for another algorithm.  A gradient that is zero in exact
    arithmetic (tol/<case>/abs/gp/...: GSBottleneck's ``shortcut.bn.bias`` in front of ``cv3``'s training-mode BatchNorm) has a
    relative tolerance that says nothing (the reference's value is rounding noise), so its largest |value| is ALSO held below 4 x the
    largest |value| of the generator's emulation, which has the same fp16 storage noise.  VoVGSCSP's ``res``: no gradient, as in the
    reference, and its statistics untouched (measured tolerance 0: equal).
    Map sizes: batch 2 on 15 x 17, 16 x 16 and 12 x 10 maps -- what the graph's GSConv / VoVGSCSP rows see at a 64 x 64 input is
    16 x 16 and smaller; the reference's full y / gx of the three modules on 64 x 64 MAPS (4.4 MB of fp32) do not fit the 1 MiB limit
    of a committed fixture."""
    G = golden("slimneck")
    m, c1, H, W = _build(case)
    p = f"mod/{case}"
    seed = int(G[f"{p}/seed"])
    m.load_state_dict(U.state(G, p), strict=True)
    want = dict(y=G.t(f"{p}/y"), gx=G.t(f"{p}/gx"))
    x, gy = rnd(10 * seed, 2, c1, H, W), rnd(10 * seed + 1, *want["y"].shape)
    y, gxs, rt = run_fwd_bwd(m, [x], gy)
    got = dict(y=y, gx=gxs[0])
    nograd = [str(k) for k in G[f"{p}/nograd"] if str(k)]
    for n, q in m.named_parameters():
        if n in nograd:
            assert q.grad is None and float(rt.flat_g[rt.param_off[n]:rt.param_off[n] + q.numel()].abs().max()) == 0.0, n
        else:
            got[f"gp/{n}"], want[f"gp/{n}"] = q.grad.float().cpu(), G.t(f"{p}/gp/{n}")
    assert sorted(rt.unused_parameter_names()) == sorted(nograd)
    errs = {n: l2err(got[n].reshape(want[n].shape), want[n]) for n in got}
    tols = {n: float(G[f"tol/{case}/{n}"]) for n in got}
    print(case, {n: f"{errs[n]:.2e} (4 x {tols[n]:.2e})" for n in errs})
    for n in errs:
        assert errs[n] < 4 * tols[n], n
    for n in G.keys(f"tol/{case}/abs/gp/"):
        k = n.split("/abs/gp/")[1]
        a, t = float(got[f"gp/{k}"].abs().max()), float(G[n])
        other = float(got[f"gp/{k.replace('bias', 'weight')}"].abs().max())
        print(case, k, f"max |gradient| {a:.2e} (4 x {t:.2e}); the reference's {float(G[f'{p}/ref_abs/gp/{k}']):.2e}; max |gradient| of its gamma {other:.2e}")
        assert a < 4 * t, n
    bufs = dict(m.named_buffers())
    berr = {}
    for n in G.keys(f"{p}/buf/"):
        k = n.split("/buf/")[1]
        berr[k] = (relerr(bufs[k], G.t(n)), float(G[f"tol/{case}/buf/{k}"]))
    print(case, "running statistics", {k: f"{e:.2e} (4 x {t:.2e})" for k, (e, t) in berr.items()})
    for k, (e, t) in berr.items():
        assert e <= 4 * t, k
    if nograd:
        sd = U.state(G, p)
        for k in ("res.bn.running_mean", "res.bn.running_var", "res.conv.weight"):
            assert torch.equal(m.state_dict()[k].cpu(), sd[k]), k
        assert id(m.res) not in rt.specs and len(rt.specs) == 8  # no ConvSpec for res, so no pack and no launch


# ----------------------------------------------------------------------------- 4. the graph against the reference
def _model(G, name=U.MODEL):
    from ultralytics.nn.tasks import DetectionModel
    m = DetectionModel(os.path.join(CFG_DIR, name + ".yaml"), ch=3, verbose=False)
    if name == U.MODEL:
        m.load_state_dict(U.state(G, U.MODEL), strict=True)
    return m.cuda()


def _names(ops):
    return [o[2] for o in ops if o[0] is not None]


def _res_names(m):
    return [k for k in m.state_dict() if ".res." in k]


def test_eval_and_fused_eval_vs_golden(golden):
    """Box rows and class scores at 4 x the generator's measured tolerances (tol/<model>/y_eval_*, y_eval_fused_*); the second call of
    a geometry is traced into an InferPlan, the third replays it: all three bit for bit, ten shuffle launches in the list."""
    G = golden("slimneck")
    m = _model(G).eval()
    x = G.t("batch/img").cuda()
    for key in ("y_eval", "y_eval_fused"):
        if key == "y_eval_fused":
            m.fuse()
            assert not hasattr(m.model[18].cv2, "bn") and not hasattr(m.model[12].res, "bn")
        ref = G.t(f"{U.MODEL}/{key}")
        with torch.no_grad():
            y1, _ = m(x)   # walked
            assert not m._infer_plans["plans"]
            y2, _ = m(x)   # traced into a plan
            plan = m._infer_plans["plans"][(2, 3, 64, 64)]
            y3, _ = m(x)   # replayed
        torch.cuda.synchronize()
        assert _names(plan.rec.ops).count("dy_gs_shuffle_forward") == N_SHUFFLES
        assert torch.equal(y1, y2) and torch.equal(y1, y3)
        assert y1.shape == ref.shape
        eb, ec = relerr(y1[:, :4].cpu(), ref[:, :4]), relerr(y1[:, 4:].cpu(), ref[:, 4:])
        tb, tc = float(G[f"tol/{U.MODEL}/{key}_box"]), float(G[f"tol/{U.MODEL}/{key}_cls"])
        print(f"{key}: box relerr {eb:.2e} (4 x {tb:.2e}) cls relerr {ec:.2e} (4 x {tc:.2e})")
        assert eb < 4 * tb and ec < 4 * tc


def test_train_step_vs_golden(golden):
    """One training step: loss items, loss, gradient norms (median / max of the relative error, tests/test_gpu_carafe.py's formula),
    the first layer's gradient, the gradients of the GSConv rows' four convolution weights element by element and, after one clipped
    SGD-nesterov step, the norms of every tensor's change, at 4 x the tolerances the generator measured for them (tol/<model>/...).
    The ``res`` tensors: masked, a zero gradient slice, unchanged."""
    from ultralytics.hip.train import StepPlan
    G = golden("slimneck")
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
    assert ops.count("dy_gs_shuffle_forward") == N_SHUFFLES and ops.count("dy_gs_shuffle_backward") == N_SHUFFLES
    rt = plan.rt
    unused = [str(k) for k in G[f"{U.MODEL}/unused"]]
    assert rt.unused_parameter_names() == sorted(unused, key=rt.param_off.get) and set(unused) == set(rt.unused_parameter_names())
    params = dict(m.named_parameters())
    mask = torch.zeros_like(rt.frozen)
    for k in unused:
        o, n = rt.param_off[k], params[k].numel()
        assert params[k].requires_grad and bool(rt.frozen[o:o + n].all()) and float(rt.flat_g[o:o + n].abs().max()) == 0.0, k
        mask[o:o + n] = 1
    live = [k for k in params if k not in unused and ".dfl" not in k]
    assert not any(bool(rt.frozen[rt.param_off[k]:rt.param_off[k] + params[k].numel()].any()) for k in live)  # exactly the res tensors
    s = plan.crit.scalars.cpu()
    ref_items = G.t(f"{U.MODEL}/items")
    per_item = float(((s[5:8] - ref_items).abs() / ref_items.abs()).max())
    eloss = abs(float(s[8]) - float(G[f"{U.MODEL}/loss"])) / float(G[f"{U.MODEL}/loss"])
    names = [str(k) for k in G[f"{U.MODEL}/grad_names"]]
    assert not set(names) & set(unused)
    scale = float(plan.state[0])
    l2 = torch.stack([params[k].grad.float().norm() / scale for k in names]).cpu()
    ref = G.t(f"{U.MODEL}/grad_l2")
    rel = ((l2 - ref).abs() / (ref.abs() + 1e-3 * ref.abs().max())).numpy()
    ef = l2err(params[names[0]].grad.float().cpu() / scale, G.t(f"{U.MODEL}/grad_first"))
    got = dict(items=per_item, loss=eloss, grad_l2_median=float(np.median(rel)), grad_l2_max=float(rel.max()), grad_first=ef)
    sd = m.state_dict()
    rm = [str(k) for k in G[f"{U.MODEL}/run_mean_names"]]
    got.update(run_mean_sum=relerr(torch.stack([sd[k].sum() for k in rm]).cpu(), G.t(f"{U.MODEL}/run_mean_sum")),
               run_var_sum=relerr(torch.stack([sd[k.replace("mean", "var")].sum() for k in rm]).cpu(), G.t(f"{U.MODEL}/run_var_sum")))
    tol.update({k: float(G[f"tol/{U.MODEL}/{k}"]) for k in ("run_mean_sum", "run_var_sum")})
    assert torch.isfinite(rt.flat_g).all() and float(plan.state[2]) == 0.0
    plan.optimizer_step()
    torch.cuda.synchronize()
    after = dict(m.named_parameters())
    for k in unused:
        assert torch.equal(after[k].detach(), start[k]), k
    upd = torch.stack([(after[k].detach() - start[k]).float().norm() for k in names]).cpu()
    ref_u = G.t(f"{U.MODEL}/upd_l2")
    relu = ((upd - ref_u).abs() / (ref_u.abs() + 1e-3 * ref_u.abs().max())).numpy()
    got.update(upd_l2_median=float(np.median(relu)), upd_l2_max=float(relu.max()))
    print("items", s[5:8].tolist(), ref_items.tolist())
    print({k: f"{got[k]:.2e} (4 x {tol[k]:.2e})" for k in got}, "worst gradient norm:", names[int(rel.argmax())])
    for i in U.GS_LAYERS:
        for cv in ("cv1", "cv2"):
            j = names.index(f"model.{i}.{cv}.conv.weight")
            e, t = l2err(params[names[j]].grad.float().cpu() / scale, G.t(f"{U.MODEL}/grad/{names[j]}")), float(G[f"tol/{U.MODEL}/grad/{names[j]}"])
            got[f"grad/{names[j]}"], tol[f"grad/{names[j]}"] = e, t
            print(names[j], f"l2 {float(l2[j]):.4e} reference {float(ref[j]):.4e} rel {float(rel[j]):.2e}; l2err {e:.2e} (4 x {t:.2e})")
    for k in got:
        assert got[k] < 4 * tol[k], k


def test_captured_step_equals_the_eager_step(golden):
    """One StepPlan step replayed as a hipGraph against the eager tape step of another plan on the same state and batch: the same
    launches, no atomics in the shuffle kernels, so loss items and ALL gradients are EQUAL."""
    from ultralytics.hip.train import StepPlan
    G = golden("slimneck")
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
        assert ops.count("dy_gs_shuffle_forward") == N_SHUFFLES and ops.count("dy_gs_shuffle_backward") == N_SHUFFLES
        outs.append((plan.rt.flat_g.clone(), plan.crit.scalars.clone()))
    assert torch.isfinite(outs[0][0]).all() and float(outs[0][0].abs().max()) > 0
    assert torch.equal(outs[0][1][5:9], outs[1][1][5:9]) and torch.equal(outs[0][0], outs[1][0])


def test_concatenations_as_one_buffer(golden, monkeypatch):
    """DY_PLANAR=0: Concats are buffers their producers write into -- row 18's shuffle stores into its slice of Concat 19's buffer,
    rows 12 and 20 write theirs, and inside every VoVGSCSP ``cv2`` and the bottleneck's sum write the two halves of the buffer ``cv3``
    reads.  The same step at the same tolerances (4 x the generator's): loss items, gradient-norm median, the eval forward."""
    from ultralytics.hip import engine as E
    from ultralytics.hip.train import StepPlan
    monkeypatch.setattr(E, "PLANAR", False)
    G = golden("slimneck")
    m = _model(G).train()
    for k, v in m.named_parameters():
        v.requires_grad = ".dfl" not in k
    plan = StepPlan(m, 2, 64, nmax=8, optimizer="SGD", init_scale=1024.0, dynamic_scale=False)
    plan.forward_backward(U.batch(G))
    torch.cuda.synchronize()
    ops = _names(plan.rec_fb.ops)
    assert ops.count("dy_gs_shuffle_forward") == N_SHUFFLES and ops.count("dy_gs_shuffle_backward") == N_SHUFFLES
    s = plan.crit.scalars.cpu()
    ref_items = G.t(f"{U.MODEL}/items")
    per_item = float(((s[5:8] - ref_items).abs() / ref_items.abs()).max())
    names = [str(k) for k in G[f"{U.MODEL}/grad_names"]]
    params, scale = dict(m.named_parameters()), float(plan.state[0])
    l2 = torch.stack([params[k].grad.float().norm() / scale for k in names]).cpu()
    ref = G.t(f"{U.MODEL}/grad_l2")
    rel = ((l2 - ref).abs() / (ref.abs() + 1e-3 * ref.abs().max())).numpy()
    print(f"items {per_item:.2e}, gradient norms median {float(np.median(rel)):.2e} max {float(rel.max()):.2e}")
    assert per_item < 4 * float(G[f"tol/{U.MODEL}/items"])
    assert float(np.median(rel)) < 4 * float(G[f"tol/{U.MODEL}/grad_l2_median"]) and float(rel.max()) < 4 * float(G[f"tol/{U.MODEL}/grad_l2_max"])
    m2 = _model(G).eval()
    with torch.no_grad():
        y, _ = m2(G.t("batch/img").cuda())
    ref = G.t(f"{U.MODEL}/y_eval")
    eb, ec = relerr(y[:, :4].cpu(), ref[:, :4]), relerr(y[:, 4:].cpu(), ref[:, 4:])
    print(f"eval: box relerr {eb:.2e} cls relerr {ec:.2e}")
    assert eb < 4 * float(G[f"tol/{U.MODEL}/y_eval_box"]) and ec < 4 * float(G[f"tol/{U.MODEL}/y_eval_cls"])


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


def _specs_of(plan, mod):
    from ultralytics.nn.modules import Conv
    return [plan.rt.specs[id(c)] for c in mod.modules() if isinstance(c, Conv) and id(c) in plan.rt.specs]


def test_freeze_18_keeps_the_row_and_its_input_gradient(golden):
    """freeze=[18], everything upstream trainable: row 18's two weight-gradient launches are pruned, its parameters keep their bits,
    its shuffle backward and both input gradients run, and the gradient everything upstream receives EQUALS the unfrozen step's."""
    from ultralytics.engine.trainer import frozen_parameter_names
    G = golden("slimneck")
    names = [k for k, _ in _model(G).named_parameters()]
    frozen = set(frozen_parameter_names(names, [18]))
    assert frozen and all(k.startswith("model.18.") for k in frozen if ".dfl" not in k)
    m, plan, start = _frozen_step(G, frozen)
    sp18 = _specs_of(plan, m.model[18])
    assert len(sp18) == 2 and not any(sp.trainable for sp in sp18)
    ops = [o for o in plan.rec_fb.ops if o[0] is not None]
    assert _names(ops).count("dy_gs_shuffle_forward") == N_SHUFFLES and _names(ops).count("dy_gs_shuffle_backward") == N_SHUFFLES
    ws = {id(s) for s in plan.wgrad_specs}
    assert not any(id(sp) in ws for sp in sp18)
    gptrs = {sp.gweight.data_ptr() for sp in sp18}
    for fn, args, name, _sid in ops:
        assert not [a for a in args if isinstance(a, int) and a in gptrs], f"{name} writes a frozen weight's gradient"
    sd = m.state_dict()
    for k in frozen:
        assert torch.equal(sd[k], start[k]), k
    m2, plan2, _ = _frozen_step(G, {k for k in frozen if ".dfl" in k})
    for k0 in ("model.17.cv3.conv.weight", "model.17.gsb.0.conv_lighting.1.cv2.conv.weight", "model.17.gsb.0.shortcut.bn.weight", "model.12.cv1.conv.weight",
               "model.0.conv.weight"):
        g1, g2 = dict(m.named_parameters())[k0].grad, dict(m2.named_parameters())[k0].grad
        assert torch.equal(g1, g2) and float(g2.abs().max()) > 0, k0


def test_freeze_13_leaves_no_backward_launch_for_row_12(golden):
    """freeze=13 (layers 0-12): nothing trainable lies upstream of row 12 and the row is frozen, so it leaves nothing on the tape: its
    two shuffles have no backward, none of its Convs a weight gradient, and no launch names one of its gradient views."""
    from ultralytics.engine.trainer import frozen_parameter_names
    G = golden("slimneck")
    names = [k for k, _ in _model(G).named_parameters()]
    frozen = set(frozen_parameter_names(names, 13))
    assert "model.12.cv3.conv.weight" in frozen and "model.13.conv.weight" not in frozen
    m, plan, start = _frozen_step(G, frozen)
    sp12 = _specs_of(plan, m.model[12])
    assert len(sp12) == 8 and not any(sp.trainable for sp in sp12)  # (res has no spec)
    ops = [o for o in plan.rec_fb.ops if o[0] is not None]
    assert _names(ops).count("dy_gs_shuffle_forward") == N_SHUFFLES and _names(ops).count("dy_gs_shuffle_backward") == N_SHUFFLES - 2
    ws = {id(s) for s in plan.wgrad_specs}
    assert not any(id(sp) in ws for sp in sp12) and all(id(sp) in ws for sp in _specs_of(plan, m.model[17]))
    gptrs = {t.data_ptr() for sp in sp12 for t in (sp.gweight, sp.gbn_w, sp.gbn_b)} | {sp.acc_b.data_ptr() for sp in sp12 if sp.acc_b is not None}
    for fn, args, name, _sid in ops:
        assert not [a for a in args if isinstance(a, int) and a in gptrs], f"{name} belongs to the backward of row 12"
    sd = m.state_dict()
    for k in frozen:
        assert torch.equal(sd[k], start[k]), k
    assert not torch.equal(sd["model.17.gsb.0.conv_lighting.0.cv2.conv.weight"], start["model.17.gsb.0.conv_lighting.0.cv2.conv.weight"])
    rt = plan.rt
    assert float(rt.flat_g[rt.frozen.bool()].abs().max()) == 0.0 and torch.isfinite(rt.flat_g).all()


def test_reference_written_checkpoint_runs(golden):
    """attempt_load_weights of tests/golden/ref_ckpt_slimneck.pt: the eval forward is the reference's (4 x tol/ckpt/y_eval_*) and
    EQUALS that of a natively built model with the same fp16-rounded state."""
    from ultralytics.nn.tasks import DetectionModel, attempt_load_weights, torch_safe_load
    G = golden("slimneck")
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
    G = golden("slimneck")
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


def test_two_epochs_through_the_public_trainer(tmp_path):
    """Two epochs with weight decay: the loss falls, every GSConv weight moved, and every ``res.*`` parameter and buffer keeps its bits
    with a zero slice of the flat gradient (no decay, no momentum: the reference's optimizers skip a parameter without a gradient);
    last.pt reloads."""
    from ultralytics import YOLO
    from ultralytics.data import SyntheticDetection
    from ultralytics.nn.extra_modules.block import GSConv
    from ultralytics.nn.tasks import attempt_load_weights
    torch.manual_seed(0)
    y = YOLO(U.MODEL + ".yaml")
    w0 = {k: v.detach().clone() for k, v in y.model.state_dict().items()}
    src = SyntheticDetection(n_batches=4, batch=4, imgsz=64, boxes_per_image=3, wh=(0.1, 0.4), seed=3)
    hist = y.train(data=src, batch=4, imgsz=64, epochs=2, optimizer="SGD", warmup_epochs=0.0, lr0=0.01, nbs=4, hipgraph=True, amp=False,
                   weight_decay=5e-4, project=str(tmp_path), name="slim")
    hist = np.asarray([[float(v) for v in h] for h in hist], dtype=np.float64)
    print("loss items per epoch", hist.tolist())
    assert hist.shape == (2, 3) and np.isfinite(hist).all()
    assert hist[-1].sum() < hist[0].sum()
    plan = y.trainer.plan
    st = plan.state.cpu().numpy()
    assert st[5] == 8 and st[6] == 0 and st[5] == plan.opt_calls, st.tolist()
    model = y.trainer.model
    w1 = model.state_dict()
    keys = [f"{n}.{cv}.conv.weight" for n, mod in model.named_modules() if isinstance(mod, GSConv) for cv in ("cv1", "cv2")]
    assert len(keys) == 2 * N_SHUFFLES
    still = [k for k in keys if torch.equal(w1[k].cpu(), w0[k].cpu())]
    assert not still, f"GSConv weights that never moved: {still}"
    res = _res_names(model)
    assert len(res) == 6 * len(U.VOV_LAYERS)
    for k in res:
        assert torch.equal(w1[k].cpu(), w0[k].cpu()), f"{k} changed"
    rt = plan.rt
    params = dict(model.named_parameters())
    for k in rt.unused_parameter_names():
        o, n = rt.param_off[k], params[k].numel()
        assert ".res." in k and float(rt.flat_g[o:o + n].abs().max()) == 0.0 and params[k].requires_grad, k
    assert len(rt.unused_parameter_names()) == 3 * len(U.VOV_LAYERS)
    assert torch.isfinite(rt.flat_g).all()
    last = tmp_path / "slim" / "weights" / "last.pt"
    assert last.exists()
    back = attempt_load_weights(str(last))  # (the EMA copy, fp16)
    assert list(back.state_dict()) == list(w1) and all(torch.isfinite(v.float()).all() for v in back.state_dict().values())


@pytest.mark.parametrize("optimizer", ["SGD", "Adam", "AdamW", "RMSProp"])
def test_flat_optimizers_leave_res_alone(golden, optimizer):
    """One step of the flat optimizer kernel with weight decay on the decayed group after a real forward + backward: every ``res.*``
    slice of the flat parameter buffer keeps its bits (no decay either: AdamW's is decoupled from the gradient), the used Convs of
    the same block move."""
    from ultralytics.hip.train import StepPlan
    G = golden("slimneck")
    m = _model(G).train()
    plan = StepPlan(m, 2, 64, nmax=8, optimizer=optimizer, init_scale=1024.0, dynamic_scale=False)
    rt = plan.rt
    p0 = rt.flat_p.clone()
    plan.set_hyper([0.001] * 3, 0.9, [0.0, 5e-2, 0.0])
    plan.forward_backward(U.batch(G))
    plan.optimizer_step()
    torch.cuda.synchronize()
    assert float(plan.state[5]) == 1 and float(plan.state[6]) == 0  # the step was taken, not skipped
    params = dict(m.named_parameters())
    names = rt.unused_parameter_names()
    assert len(names) == 3 * len(U.VOV_LAYERS)
    for k in names:
        o, n = rt.param_off[k], params[k].numel()
        assert torch.equal(rt.flat_p[o:o + n], p0[o:o + n]) and float(rt.flat_g[o:o + n].abs().max()) == 0.0, k
    for i in U.VOV_LAYERS:
        k = f"model.{i}.cv3.conv.weight"
        o, n = rt.param_off[k], params[k].numel()
        assert not torch.equal(rt.flat_p[o:o + n], p0[o:o + n]), k


def test_soap_names_a_gsconv_depthwise_weight_and_raises(golden):
    """optimizer='SOAP' on this graph: the grouped HIP step refuses the (C, 1, 5, 5) tensors by name."""
    from ultralytics.hip.train import StepPlan
    G = golden("slimneck")
    m = _model(G).train()
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.set_hyper([0.01] * 3, 0.9, [0.0, 5e-4, 0.0])
    with pytest.raises(NotImplementedError, match=r"cv2\.conv\.weight.*\(C, 1, k, k\)"):
        plan._soap_make()


def test_multi_scale_over_one_arena():
    """multi_scale=True: one recorded launch list per drawn size, all over one arena: every optimizer step takes effect, and the run
    equals, bit for bit, one whose size plans keep separate buffers."""
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
def test_default_graph_launches_no_shuffle_kernel(golden):
    from ultralytics.hip.train import StepPlan
    G = golden("slimneck")
    m = _model(G, "yolov8n-ASF-P2P2").train()
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.forward_backward(U.batch(G))
    torch.cuda.synchronize()
    ops = _names(plan.rec_fb.ops)
    assert ops and not [n for n in ops if n.startswith("dy_gs_")]
    assert plan.rt.unused_parameter_names() == []
