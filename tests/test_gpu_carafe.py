"""-m gpu: CARAFE (content-aware up-sampling, reference nn/extra_modules/block.py:3898-3936, k_up 5, scale 2) on the HIP path.

1. the reassembly kernels (csrc/carafe.hip) per element against the reference's float64 values (tests/golden/carafe_kernel.npz,
   carafe_big_*.npz), dense and on channel slices, under the rule of tests/tensor_ops_ref.py

       |got - ref| <= k16 * 2^-11 * |ref| + k32 * 2^-23 * mag + 2^-24

   mag from tests/carafe_ref.py (which tests/test_host_carafe.py holds to the same float64 values): forward sum_k p_k |x_k|;
   dlogits p_k (G_k + sum_m p_m G_m), G_k = sum_c |dy_c x_{k,c}|; dx sum p |dy|, plus |old| when accumulating.  No element is left
   out.  CARAFE has no floor and no clamp on a coordinate: there is no kink term.  k16 = 1 is the fp16 store.  k32 counts half an
   ulp (0.5) per fp32 rounding on the element's longest path, relative to a quantity that mag bounds:

     a softmax weight p_k (cf_softmax)                                                                       16
        L_k - max as an exact two-term sum hi + lo (0); expf(hi), documented at 1 ulp (1); e = fma(e, lo, e) (0.5; the dropped
        lo^2 / 2 of e^lo is below 2^-36); S = the sum of 25 such e, each 1.5 off, by 24 additions (12): 13.5; 1 / S correctly
        rounded (0.5); e * (1 / S) (0.5)
     forward   k32 = 29: p_k (16) + 25 fused multiply-adds, each rounding a partial sum that mag bounds (12.5) = 28.5
     dlogits   k32 = 46 + C / 2: g_k by C fused multiply-adds of exact fp16 x fp16 products (0.5 C, on G_k); t = sum_m p_m g_m:
               its terms (16 + 0.5 C) and 25 fused multiply-adds (12.5), on T = sum_m p_m G_m; g_k - t (0.5, on G_k + T); the
               product with p_k (16 + 0.5): <= mag (28.5 + 0.5 C + 0.5 + 16.5) = mag (45.5 + 0.5 C)
     dx        k32 = 67: p (16) + at most 100 fused multiply-adds (50) = 66, + 0.5 for the addition of the old value when
               accumulating (mag then includes |old|)

   Values of expf below the normal range (hi < -87) are off by less than 2^-126 in absolute terms: under the 2^-24 floor for any fp16 x.
2. dlogits lanes 100..103 zero, accumulate 0 / 1, dx == NULL, two backward calls bit for bit; 3. refusals; 4. the module against the
reference at 4 x the generator's measured tolerances; 5. the graph: eval / fused eval / InferPlan, one training step, captured =
eager, freeze=, a reference-written checkpoint, augment=True, the public trainer -- at the bounds tests/test_gpu_spd.py applies to
its ASF graph (those of tests/test_gpu_model.py's N graph)."""
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

import carafe_ref as R
from carafe_util import CARAFE_LAYERS, CKPT, KERNEL_CASES, MODEL, MODULE_CASES, SLICE, batch, fetch, kernel_inputs, state
from conftest import CFG_DIR
from golden.cases import rnd
from gpu_util import l2err, relerr, run_fwd_bwd

pytestmark = pytest.mark.gpu
DY_ERR_ARG, DY_ERR_ALIGN = -1, -3  # include/dealyolo_hip.h
POISON = -1234.0  # exactly representable in fp16
_REF = {}


def k_bound(what, C):
    """(k16, k32), counted in the docstring above."""
    return {"y": (1, 29), "dlogits": (1, 46 + C / 2), "dx": (1, 67)}[what]


# ----------------------------------------------------------------------------- helpers
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _store(t, extra=0, c0=0):
    """fp16 device storage (..., C + extra), POISON outside channels [c0, c0 + C), holding ``t`` inside."""
    C = t.shape[-1]
    s = torch.full((*t.shape[:-1], C + extra), POISON, dtype=torch.float16)
    s[..., c0:c0 + C] = t.half()
    return s.cuda()


def _logits(lg, extra):
    """The encoder's output as the engine stores it: 100 channels in a pitch of 104 + extra.  Lanes 100..103 hold zeros there; the
    kernels must not read them, so the sliced variant poisons them too."""
    s = torch.full((*lg.shape[:-1], 104 + extra), POISON if extra else 0.0, dtype=torch.float16)
    s[..., :100] = lg
    return s.cuda()


def _outside_untouched(s, c0, C):
    return bool((s[..., :c0] == POISON).all()) and bool((s[..., c0 + C:] == POISON).all())


def _fwd(x, cx, lg, y, cy, C):
    from ultralytics.hip import lib
    N, H, W = lg.shape[:3]
    return lib().dy_carafe(x.data_ptr() + 2 * cx, x.shape[-1], lg.data_ptr(), lg.shape[-1], y.data_ptr() + 2 * cy, y.shape[-1], N, H, W, C,
                           _stream())


def _bwd(x, cx, lg, dy, cy, dx, cdx, dl, C, accumulate=0):
    from ultralytics.hip import lib
    N, H, W = lg.shape[:3]
    rc = lib().dy_carafe_backward(x.data_ptr() + 2 * cx, x.shape[-1], lg.data_ptr(), lg.shape[-1], dy.data_ptr() + 2 * cy, dy.shape[-1],
                                  0 if dx is None else dx.data_ptr() + 2 * cdx, 0 if dx is None else dx.shape[-1], accumulate,
                                  dl.data_ptr(), dl.shape[-1], N, H, W, C, _stream())
    torch.cuda.synchronize()
    return rc


def _case(golden, name):
    """Inputs, the reference's float64 values and the bound magnitudes of a kernel case, computed once and shared."""
    if name not in _REF:
        G = golden("carafe_kernel")
        C, H, W, gain = KERNEL_CASES[name]
        x, lg, dy = kernel_inputs(C, H, W, int(G[f"ker/{name}/seed"]), gain)
        fw, bw = R.forward(x, lg), R.backward(x, lg, dy)
        ref = {k: fetch(G, f"ker/{name}/{k}").double() for k in ("y", "dx", "dlogits")}
        mag = dict(y=fw["mag"], dx=bw["dx_mag"], dlogits=bw["dlogits_mag"])
        _REF[name] = (x, lg, dy, C, H, W, ref, mag)
    return _REF[name]


def _check(what, got, ref, mag, C, extra=None):
    """The per-element bound of the module docstring; NO element is left out."""
    k16, k32 = k_bound(what, C)
    got, ref = got.double().cpu(), ref.double()
    if extra is not None:  # accumulate: the old value is one more term
        ref, mag = ref + extra.double(), mag + extra.double().abs()
    bound = k16 * 2.0 ** -11 * ref.abs() + k32 * 2.0 ** -23 * mag + 2.0 ** -24
    err = (got - ref).abs()
    worst = float((err / bound).max())
    print(f"{what}: max err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, f"{what}: {int((err > bound).sum())} of {err.numel()} elements beyond the bound"


VARIANTS = {"dense": (0, 0, 0, 0, 0), "sliced": (SLICE["x_off"], SLICE["x_extra"], SLICE["y_off"], SLICE["y_extra"], SLICE["l_extra"])}


# ----------------------------------------------------------------------------- 1. the kernels, per element
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_forward_per_element(golden, name, variant):
    x, lg, dy, C, H, W, ref, mag = _case(golden, name)
    cx, ex, cy, ey, el = VARIANTS[variant]
    xs, ls, ys = _store(x, ex, cx), _logits(lg, el), _store(torch.zeros(x.shape[0], 2 * H, 2 * W, C) + POISON, ey, cy)
    x0, l0 = xs.clone(), ls.clone()
    assert _fwd(xs, cx, ls, ys, cy, C) == 0
    torch.cuda.synchronize()
    _check("y", ys[..., cy:cy + C], ref["y"], mag["y"], C)
    assert _outside_untouched(ys, cy, C) and torch.equal(xs, x0) and torch.equal(ls, l0)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_backward_per_element(golden, name, variant):
    """dlogits and dx; lanes 100..103 of dlogits are zeros and the lanes behind them survive; accumulate = 1 adds; dx == NULL leaves
    the dx buffer alone and gives the same dlogits; a second call gives the same bits."""
    x, lg, dy, C, H, W, ref, mag = _case(golden, name)
    cx, ex, cy, ey, el = VARIANTS[variant]
    xs, ls, dys = _store(x, ex, cx), _logits(lg, el), _store(dy, ey, cy)

    def outputs():
        return (_store(torch.zeros_like(x.float()) + POISON, ex, cx),
                torch.full((*lg.shape[:3], 104 + el), POISON, dtype=torch.float16, device="cuda"))

    dxs, dl = outputs()
    assert _bwd(xs, cx, ls, dys, cy, dxs, cx, dl, C) == 0
    _check("dx", dxs[..., cx:cx + C], ref["dx"], mag["dx"], C)
    _check("dlogits", dl[..., :100], ref["dlogits"], mag["dlogits"], C)
    assert bool((dl[..., 100:104] == 0).all()) and bool((dl[..., 104:] == POISON).all()) and _outside_untouched(dxs, cx, C)
    # the same call again: the same bits
    dx2, dl2 = outputs()
    assert _bwd(xs, cx, ls, dys, cy, dx2, cx, dl2, C) == 0
    assert torch.equal(dx2, dxs) and torch.equal(dl2, dl)
    # accumulate = 1: one fp16 rounding of (old value + gradient); dlogits is written, not accumulated
    dxa, dla = outputs()
    prev = torch.from_numpy(np.random.default_rng(7).standard_normal(tuple(x.shape)).astype(np.float16))
    dxa[..., cx:cx + C] = prev.cuda()
    assert _bwd(xs, cx, ls, dys, cy, dxa, cx, dla, C, accumulate=1) == 0
    _check("dx", dxa[..., cx:cx + C], ref["dx"], mag["dx"], C, extra=prev)
    assert torch.equal(dla, dl) and _outside_untouched(dxa, cx, C)
    # dx == NULL: the logit gradient alone, the same bits
    dxn, dln = outputs()
    assert _bwd(xs, cx, ls, dys, cy, None, 0, dln, C) == 0
    assert torch.equal(dln, dl) and bool((dxn == POISON).all())


# ----------------------------------------------------------------------------- 3. refusals
def test_refusals_launch_nothing():
    from ultralytics.hip import lib
    L = lib()
    N, H, W, C = 1, 4, 4, 32
    x = torch.full((N, H, W, C), POISON, dtype=torch.float16, device="cuda")
    lg = torch.zeros(N, H, W, 112, dtype=torch.float16, device="cuda")
    y = torch.full((N, 2 * H, 2 * W, C), POISON, dtype=torch.float16, device="cuda")
    dl = torch.full((N, H, W, 112), POISON, dtype=torch.float16, device="cuda")
    st = _stream()

    def fwd(xp=None, ldx=C, yp=None, ldy=C, C_=C, ldl=104, lp=None):
        return L.dy_carafe(x.data_ptr() if xp is None else xp, ldx, lg.data_ptr() if lp is None else lp, ldl, y.data_ptr() if yp is None else yp,
                           ldy, N, H, W, C_, st)

    def bwd(xp=None, ldx=C, dxp=None, lddx=C, dlp=None, lddl=104, C_=C, ldl=104):
        return L.dy_carafe_backward(x.data_ptr() if xp is None else xp, ldx, lg.data_ptr(), ldl, y.data_ptr(), C,
                                    x.data_ptr() if dxp is None else dxp, lddx, 0, dl.data_ptr() if dlp is None else dlp, lddl, N, H, W, C_, st)

    assert fwd(C_=12, ldx=16, ldy=16) == DY_ERR_ARG and bwd(C_=12, ldx=16, lddx=16) == DY_ERR_ARG  # 12 channels
    assert fwd(ldl=100) == DY_ERR_ALIGN and bwd(ldl=100) == DY_ERR_ALIGN and bwd(lddl=100) == DY_ERR_ALIGN  # pitch 100 for the logits
    assert fwd(ldl=96) == DY_ERR_ARG and bwd(lddl=96) == DY_ERR_ARG                                # ... and a granule pitch below 104
    assert fwd(xp=x.data_ptr() + 8) == DY_ERR_ALIGN and fwd(yp=y.data_ptr() + 8) == DY_ERR_ALIGN   # a pointer 8 bytes off
    assert fwd(lp=lg.data_ptr() + 8) == DY_ERR_ALIGN and bwd(dxp=x.data_ptr() + 8) == DY_ERR_ALIGN and bwd(dlp=dl.data_ptr() + 8) == DY_ERR_ALIGN
    assert bwd(dlp=0) == DY_ERR_ARG and fwd(xp=0) == DY_ERR_ARG and fwd(yp=0) == DY_ERR_ARG and fwd(lp=0) == DY_ERR_ARG  # null pointers
    assert fwd(ldx=C + 4) == DY_ERR_ALIGN and bwd(lddx=C + 4) == DY_ERR_ALIGN and fwd(ldx=C - 8) == DY_ERR_ARG
    torch.cuda.synchronize()
    assert bool((x == POISON).all()) and bool((y == POISON).all()) and bool((dl == POISON).all())


def test_engine_op_rejects_an_unsupported_geometry():
    from ultralytics.hip.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        eng.carafe(None, None, eng.wrap_act(torch.zeros(1, 4, 4, 24, dtype=torch.float16, device="cuda")).sub(0, 12))


# ----------------------------------------------------------------------------- 4. the module against the reference
@pytest.mark.parametrize("case", list(MODULE_CASES))
def test_module_vs_golden(golden, case):
    """l2err of y, gx and every parameter gradient below 4 x the tolerance the generator measured for the case (tol/<case>/...: the
    error of a float64 emulation of this path's fp16 storage against the same fp32 values).  The factor pays for another fp32
    summation order, not for another algorithm.  Running statistics after the one forward: 2e-3, as tests/test_gpu_spd.py."""
    from ultralytics.nn.extra_modules import CARAFE
    G = golden("carafe")
    C, c_mid, k_enc, H, W = MODULE_CASES[case]
    p = f"mod/{case}"
    seed = int(G[f"{p}/seed"])
    x, gy = rnd(10 * seed, 2, C, H, W), rnd(10 * seed + 1, 2, C, 2 * H, 2 * W)
    m = CARAFE(C, k_enc, 5, c_mid, 2)
    m.load_state_dict(state(G, p), strict=True)
    y, gxs, rt = run_fwd_bwd(m, [x], gy)
    got, want = dict(y=y, gx=gxs[0]), dict(y=fetch(G, f"{p}/y"), gx=fetch(G, f"{p}/gx"))
    for k, q in m.named_parameters():
        got[f"gp/{k}"], want[f"gp/{k}"] = q.grad.float().cpu(), G.t(f"{p}/gp/{k}")
    errs = {k: l2err(got[k].reshape(want[k].shape), want[k]) for k in got}
    tols = {k: float(G[f"tol/{case}/{k}"]) for k in got}
    print(case, {k: f"{errs[k]:.2e} (4 x {tols[k]:.2e})" for k in errs})
    for k in errs:
        assert errs[k] < 4 * tols[k], k
    bufs = dict(m.named_buffers())
    for k in G.keys(f"{p}/buf/"):
        assert relerr(bufs[k.split("/buf/")[1]], G.t(k)) < 2e-3, k


# ----------------------------------------------------------------------------- 5. the graph against the reference
def _model(G):
    from ultralytics.nn.tasks import DetectionModel
    m = DetectionModel(os.path.join(CFG_DIR, MODEL + ".yaml"), ch=3, verbose=False)
    m.load_state_dict(state(G, MODEL), strict=True)
    return m.cuda()


def test_eval_and_fused_eval_vs_golden(golden):
    """2e-2 on boxes and on class scores (the eval bound of tests/test_gpu_spd.py); the second call of a geometry is traced into an
    InferPlan, the third replays it: all three bit for bit, two dy_carafe launches in the list."""
    G = golden("carafe")
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
        assert sum(1 for o in plan.rec.ops if o[2] == "dy_carafe") == 2
        assert not any(o[2] == "dy_upsample2x" for o in plan.rec.ops)
        assert torch.equal(y1, y2) and torch.equal(y1, y3)
        assert y1.shape == ref.shape
        eb, ec = relerr(y1[:, :4].cpu(), ref[:, :4]), relerr(y1[:, 4:].cpu(), ref[:, 4:])
        print(f"{key}: box relerr {eb:.2e} cls relerr {ec:.2e}")
        assert eb < 2e-2 and ec < 2e-2


def test_train_step_vs_golden(golden):
    """One training step: the comparisons of tests/test_gpu_spd.py::test_train_step_vs_golden at its bounds for the ASF graph."""
    from ultralytics.hip.train import StepPlan
    G = golden("carafe")
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
    mine = [f"model.{i}.{c}.{k}" for i in CARAFE_LAYERS for c in ("comp", "enc") for k in ("conv.weight", "bn.weight", "bn.bias")]
    assert all(k in names for k in mine)
    scale = float(plan.state[0])
    l2 = torch.stack([params[k].grad.float().norm() / scale for k in names]).cpu()
    ref = G.t(f"{MODEL}/grad_l2")
    rel = ((l2 - ref).abs() / (ref.abs() + 1e-3 * ref.abs().max())).numpy()
    print("grad-l2 rel err: median %.2e max %.2e (%s)" % (np.median(rel), rel.max(), names[int(rel.argmax())]))
    for k in mine:
        print(k, f"l2 {float(l2[names.index(k)]):.4e} reference {float(ref[names.index(k)]):.4e} rel {float(rel[names.index(k)]):.2e}")
    assert np.median(rel) < 4e-3 and rel.max() < 4e-2
    first = params[names[0]].grad.float().cpu() / scale
    ef = l2err(first, G.t(f"{MODEL}/grad_first"))
    print(f"grad_first err {ef:.3e}")
    assert ef < 5e-2
    sd = m.state_dict()
    rm = [str(k) for k in G[f"{MODEL}/run_mean_names"]]
    assert relerr(torch.stack([sd[k].sum() for k in rm]).cpu(), G.t(f"{MODEL}/run_mean_sum")) < 5e-3
    assert relerr(torch.stack([sd[k.replace("mean", "var")].sum() for k in rm]).cpu(), G.t(f"{MODEL}/run_var_sum")) < 5e-3
    assert torch.isfinite(plan.rt.flat_g).all() and float(plan.state[2]) == 0.0


def test_captured_step_equals_the_eager_step(golden):
    """One StepPlan step replayed as a hipGraph against the eager tape step of another plan on the same state and batch: the same
    launches, no atomics anywhere in CARAFE's backward, so loss items and ALL gradients are EQUAL."""
    from ultralytics.hip.train import StepPlan
    G = golden("carafe")
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
        assert ops.count("dy_carafe") == 2 and ops.count("dy_carafe_backward") == 2 and "dy_upsample2x" not in ops
        outs.append((plan.rt.flat_g.clone(), plan.crit.scalars.clone()))
    assert torch.isfinite(outs[0][0]).all() and float(outs[0][0].abs().max()) > 0
    assert torch.equal(outs[0][1][5:9], outs[1][1][5:9]) and torch.equal(outs[0][0], outs[1][0])


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


# argument positions of dy_carafe_backward (include/dealyolo_hip.h)
A_DX, A_DL, A_C = 6, 9, 14


def test_freeze_10_prunes_layer_9_and_keeps_layer_14(golden):
    """freeze=10 (layers 0-9): nothing trainable lies upstream of layer 9 and its two Convs are frozen, so it leaves nothing on the
    tape -- no CARAFE backward, no weight gradient, nothing of its Convs named after the loss; layer 14 keeps both halves."""
    from ultralytics.engine.trainer import frozen_parameter_names
    G = golden("carafe")
    names = [k for k, _ in _model(G).named_parameters()]
    frozen = set(frozen_parameter_names(names, 10))
    assert {"model.9.comp.conv.weight", "model.9.enc.bn.bias"} <= frozen and "model.14.comp.conv.weight" not in frozen
    m, plan, start = _frozen_step(G, frozen)
    rt = plan.rt
    sp9 = [rt.spec(m.model[9].comp), rt.spec(m.model[9].enc)]
    sp14 = [rt.spec(m.model[14].comp), rt.spec(m.model[14].enc)]
    assert not any(sp.trainable for sp in sp9) and all(sp.trainable for sp in sp14)
    fwd, back = _backward_ops(plan)
    assert [o[2] for o in fwd].count("dy_carafe") == 2  # the forward keeps both
    cf_back = [o for o in back if o[2] == "dy_carafe_backward"]
    assert len(cf_back) == 1 and cf_back[0][1][A_C] == 32 and cf_back[0][1][A_DX] and cf_back[0][1][A_DL]
    ptrs = {t.data_ptr() for sp in sp9 for t in (sp.weight, sp.wpack, sp.wpack_t, sp.gweight) if t is not None}
    for fn, args, name, _sid in back:
        assert not [a for a in args if isinstance(a, int) and a in ptrs], f"{name} after the loss touches layer 9's convolutions"
    ws = {id(sp) for sp in plan.wgrad_specs}
    assert not any(id(sp) in ws for sp in sp9) and all(id(sp) in ws for sp in sp14)
    sd = m.state_dict()
    for k in frozen:
        assert torch.equal(sd[k], start[k]), f"frozen parameter {k} moved"
    for k in ("model.14.comp.conv.weight", "model.14.enc.conv.weight", "model.14.enc.bn.weight"):
        assert not torch.equal(sd[k], start[k]), k
    assert float(rt.flat_g[rt.frozen.bool()].abs().max()) == 0.0 and torch.isfinite(rt.flat_g).all()


def test_frozen_layer_with_a_trainable_prefix_keeps_its_input_gradient(golden):
    """freeze=[9], layer 8 trainable: layer 9's weight-gradient launches are pruned, its input gradient is kept whole -- the
    reassembly's dx AND what comp / enc pass down from dlogits (W^T dL is part of dX whatever the flags say)."""
    from ultralytics.engine.trainer import frozen_parameter_names
    G = golden("carafe")
    names = [k for k, _ in _model(G).named_parameters()]
    frozen = set(frozen_parameter_names(names, [9]))
    assert frozen and all(k.startswith("model.9.") for k in frozen if ".dfl" not in k)
    m, plan, start = _frozen_step(G, frozen)
    rt = plan.rt
    sp9 = [rt.spec(m.model[9].comp), rt.spec(m.model[9].enc)]
    assert not any(sp.trainable for sp in sp9)
    fwd, back = _backward_ops(plan)
    cf_back = [o for o in back if o[2] == "dy_carafe_backward"]
    assert sorted(o[1][A_C] for o in cf_back) == [32, 64] and all(o[1][A_DX] and o[1][A_DL] for o in cf_back)
    assert not any(id(sp) in {id(s) for s in plan.wgrad_specs} for sp in sp9)
    gptrs = {sp.gweight.data_ptr() for sp in sp9}
    for fn, args, name, _sid in back:
        assert not [a for a in args if isinstance(a, int) and a in gptrs], f"{name} writes a frozen weight's gradient"
    # both frozen Convs still pass their input gradient down: their transposed packs are read after the loss
    for sp in sp9:
        assert any(sp.wpack_t.data_ptr() in [a for a in o[1] if isinstance(a, int)] for o in back), f"{sp.name}: W^T dL is missing"
    sd = m.state_dict()
    for k in frozen:
        assert torch.equal(sd[k], start[k])
    # the gradient everything upstream receives equals the unfrozen step's: freezing the layer changes no dX
    m2, plan2, _ = _frozen_step(G, {k for k in frozen if ".dfl" in k})
    k0 = "model.8.conv.weight"
    g1, g2 = dict(m.named_parameters())[k0].grad.float(), dict(m2.named_parameters())[k0].grad.float()
    assert relerr(g1, g2) < 1e-3 and float(g2.abs().max()) > 0


def test_reference_written_checkpoint_runs(golden):
    """attempt_load_weights of tests/golden/ref_ckpt_carafe.pt (module path ultralytics.nn.extra_modules.block.CARAFE): the eval
    forward is the reference's (2e-2) and EQUALS that of a natively built model with the same fp16-rounded state."""
    from ultralytics.nn.tasks import DetectionModel, attempt_load_weights, torch_safe_load
    G = golden("carafe")
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
    G = golden("carafe")
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


def test_three_epochs_through_the_public_trainer():
    from ultralytics import YOLO
    from ultralytics.data import SyntheticDetection
    torch.manual_seed(0)
    y = YOLO("yolov8n-ASF-P2P2-CARAFE.yaml")
    w0 = {k: v.detach().clone() for k, v in y.model.state_dict().items()}
    src = SyntheticDetection(n_batches=4, batch=4, imgsz=64, boxes_per_image=3, wh=(0.1, 0.4), seed=3)
    hist = y.train(data=src, batch=4, imgsz=64, epochs=3, optimizer="SGD", warmup_epochs=0.0, lr0=0.01, nbs=4, hipgraph=True, amp=False)
    hist = np.asarray([[float(v) for v in h] for h in hist], dtype=np.float64)
    print("loss items per epoch", hist.tolist())
    assert hist.shape == (3, 3) and np.isfinite(hist).all()
    assert hist[-1].sum() < hist[0].sum()
    plan = y.trainer.plan
    st = plan.state.cpu().numpy()
    # every optimizer_step() the trainer issued took effect: none skipped at amp=False, the device counter advanced with the host's
    assert st[5] == 12 and st[6] == 0 and st[5] == plan.opt_calls and st[0] == 1.0, st.tolist()
    w1 = y.trainer.model.state_dict()
    mine = [k for k, _ in y.trainer.model.named_parameters() if any(k.startswith(f"model.{i}.") for i in CARAFE_LAYERS)]
    assert mine == [f"model.{i}.{c}.{k}" for i in CARAFE_LAYERS for c in ("comp", "enc") for k in ("conv.weight", "bn.weight", "bn.bias")]
    still = [k for k in mine if torch.equal(w1[k].cpu(), w0[k].cpu())]
    assert not still, f"CARAFE parameters that never moved: {still}"
    assert torch.isfinite(plan.rt.flat_g).all()


def test_multi_scale_over_one_arena():
    """multi_scale=True: one recorded launch list per drawn size, all over one arena: every optimizer step takes effect, and the run
    equals, bit for bit, one whose size plans keep separate buffers -- the logits and their gradient are step-local."""
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
