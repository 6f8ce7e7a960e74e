"""-m gpu: SimAM (reference nn/extra_modules/attention.py:53-77) on the HIP path.

1. the kernels (csrc/simam.hip) through their C entry points, per element against the float64 restatement tests/simam_ref.py
   (tests/test_host_simam.py ties it to the reference's stored values and to autograd), at the shapes of
   tests/simam_util.py::KERNEL_CASES: (2, 5, 7, 8) odd sizes and two images (statistics taken across the batch would show), (2, 5, 7, 24)
   at channel offset 8 of pitch 40, (1, 1, 2, 8) the smallest defined plane, (3, 40, 40, 16), and the shapes that leave the one-run path
   of the design: "runs" (2, 70, 75, 8) -- 5,250 pixels against the 4,096 one run of a one-granule map holds: 2 runs per image --,
   "capped" (1, 91, 91, 256) -- 8,281 pixels against 64 runs of 128: the run count is capped and the runs grow --, "wide"
   (1, 3, 5, 2056) -- 257 granules against the 256 one workgroup covers: two granule blocks.  (1, 1, 1, 8): all NaN, nothing else written.
   y, dx (stored and accumulated) and the statistics within the bounds tests/simam_ref.py counts from the kernel file's stated
   arithmetic BEFORE the first GPU run; constant planes: exact bits; planes of 30 +- 0.01 and of +-60000 within the same bounds; two
   runs: the same bytes; canaries around every buffer.
2. the module against the reference's fp32 values at 4 x the tolerance the generator measured (tol/<case>/...); the engine's refusals.
3. the graph yolov8n-ASF-P2P2-SimAM at 64x64, batch 2, at 4 x the generator's measured tolerances: eval / fused eval / augmented eval /
   the checkpoint's eval; one training step (loss items, every gradient's norm, the first gradient in full, the updated weights, SGD);
   the replayed and the captured step equal the traced one; freeze; multi_scale; the default graph launches no dy_simam_* kernel."""
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

import simam_ref as R
import simam_util as U
from conftest import CFG_DIR
from golden.cases import rnd
from gpu_util import l2err, relerr, run_fwd_bwd

pytestmark = pytest.mark.gpu
POISON = -1234.0  # exactly representable in fp16
GUARD = 3         # canary pixels behind every written tensor
WS_POISON = -4321.0
U32 = 2.0 ** -24


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


def _run(geom, x, g, old=None, lam=U.LAM):
    """Forward and backward of one case through the C entries -> dict(y, dx, mu, inv, raw)."""
    from ultralytics.hip import lib
    L = lib()
    N, H, W, C, c0, ld = geom
    xb, gb = Buf(x, c0, ld), Buf(g, c0, ld)
    x0, g0 = xb.s.clone(), gb.s.clone()
    yb = Buf(np.zeros((N, H, W, C)), c0, ld, fill=POISON)
    dxb = Buf(old, c0, ld) if old is not None else Buf(np.zeros((N, H, W, C)), c0, ld, fill=POISON)
    parts = L.dy_simam_num_partials(H * W, C)
    assert parts == U.num_partials(H * W, C)
    nws = N * parts * 2 * C
    ws = torch.full((nws + 16,), WS_POISON, dtype=torch.float64, device="cuda")
    st = torch.full((N * 2 * C + 16,), WS_POISON, dtype=torch.float32, device="cuda")
    assert L.dy_simam_forward(xb.ptr, ld, yb.ptr, ld, st.data_ptr(), ws.data_ptr(), lam, N, H, W, C, _stream()) == 0
    torch.cuda.synchronize()
    st0 = st.clone()
    assert L.dy_simam_backward(gb.ptr, ld, xb.ptr, ld, st.data_ptr(), dxb.ptr, ld, int(old is not None), ws.data_ptr(), N, H, W, C, _stream()) == 0
    torch.cuda.synchronize()
    assert yb.clean() and dxb.clean() and torch.equal(xb.s, x0) and torch.equal(gb.s, g0)
    assert bool((ws[nws:] == WS_POISON).all()) and bool((st[N * 2 * C:] == WS_POISON).all())
    assert torch.equal(st.view(torch.int32), st0.view(torch.int32))  # the backward only reads the statistics
    s = st[:N * 2 * C].view(N, 2, C).cpu().double().numpy()
    return dict(y=yb.get(), dx=dxb.get(), mu=s[:, 0], inv=s[:, 1], raw=(yb.s.clone(), dxb.s.clone(), st.clone()))


def _check(geom, x, g, old, tag):
    """y, dx (stored, and accumulated into ``old``) and the statistics of one case against the restatement, within the counted bounds."""
    b = R.backward(x, g, U.LAM)
    mu, inv = R.stats(x, U.LAM)
    for o in (None, old):
        got = _run(geom, x, g, o)
        bd = R.bounds(x, g, U.LAM, old=o)
        want = b["dx"] if o is None else b["dx"] + o
        ey, ed = np.abs(got["y"] - b["y"]), np.abs(got["dx"] - want)
        print(tag, "accumulate" if o is not None else "store", f"y: worst err / bound {float((ey / bd['y']).max()):.3f}",
              f"dx: worst err / bound {float((ed / bd['dx']).max()):.3f}  (largest |y| {np.abs(b['y']).max():.3g}, |dx| {np.abs(want).max():.3g})")
        assert np.all(ey <= bd["y"]), tag
        assert np.all(ed <= bd["dx"]), tag
        # mu: one rounding of the fp64 mean; 1 / D: one rounding, and the fp64 sums' own error (S = sum x^2 - (sum x)^2 / M cancels
        # log2(sum x^2 / S) bits of 2^-53 M)
        assert np.all(np.abs(got["mu"] - mu) <= 2 * U32 * np.abs(mu) + 1e-300)
        S_rel = 2.0 ** -50 * x.shape[1] * x.shape[2] * (x * x).sum(axis=(1, 2)) * inv * 4 / max(x.shape[1] * x.shape[2] - 1, 1)
        assert np.all(np.abs(got["inv"] - inv) <= (2 * U32 + S_rel) * np.abs(inv))
    return got


# ----------------------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("name", list(U.KERNEL_CASES))
def test_normal_inputs_within_the_counted_bounds(name):
    geom = U.KERNEL_CASES[name]
    x, g, old = U.normal_inputs(geom[:4])
    _check(geom, x, g, old, name)


def test_statistics_are_per_image():
    """Two images whose planes differ by a factor: each image's (mu, 1 / D) is its own."""
    geom = U.KERNEL_CASES["odd"]
    x, g, _ = U.normal_inputs(geom[:4])
    x[1] = np.asarray(3.0 * x[1] + 2.0).astype(np.float16).astype(np.float64)
    got = _check(geom, x, g, None, "per-image")
    mu, inv = R.stats(x, U.LAM)
    assert np.all(np.abs(mu[0] - mu[1]) > 1.0) and np.all(np.abs(got["mu"][0] - got["mu"][1]) > 1.0) and np.all(got["inv"][0] > 4 * got["inv"][1])


def test_one_pixel_plane_is_nan_and_nothing_else_is_written():
    x = np.arange(1.0, 9.0).reshape(1, 1, 1, 8)
    got = _run(U.ONE_PX, x, x)  # (the canaries are checked inside)
    assert np.isnan(got["y"]).all() and np.isnan(got["dx"]).all() and np.isnan(got["inv"]).all() and np.array_equal(got["mu"], x[:, 0, 0])


@pytest.mark.parametrize("name", ["odd", "map40", "runs"])
def test_constant_planes_give_exact_bits(name):
    """d = 0: e = 0.5 exactly, y = fp16(x a) and dx = fp16(g a) with a = sigmoid(0.5) to a few fp32 ulps; x sigmoid(0.5) and
    g sigmoid(0.5) lie at least 32 fp32 round-offs from every fp16 rounding boundary (asserted in tests/test_host_simam.py), so the
    stored bits are those of the float64 values rounded to fp16.  mu is the plane's value exactly."""
    geom = U.KERNEL_CASES[name]
    x, g = U.const_inputs(geom[:4])
    b = R.backward(x, g, U.LAM)
    got = _run(geom, x, g)
    f16 = lambda a: a.astype(np.float16).astype(np.float64)  # noqa: E731
    assert np.array_equal(got["y"], f16(b["y"])) and np.array_equal(got["dx"], f16(b["dx"]))
    assert np.array_equal(got["mu"], x[:, 0, 0, :])


@pytest.mark.parametrize("name", ["odd", "map40", "runs"])
def test_offset_planes_the_cancellation_case(name):
    """Planes of 30 +- 0.01: sum x^2 - (sum x)^2 / M loses 7 decimal digits; fp64 accumulators keep 9 more."""
    geom = U.KERNEL_CASES[name]
    x, g, old = U.offset_inputs(geom[:4])
    assert 1e-3 < np.std(x) < 0.05 and abs(np.mean(x) - 30) < 0.1
    _check(geom, x, g, old, name + "-offset")


@pytest.mark.parametrize("name", ["odd", "map40"])
def test_large_planes(name):
    geom = U.KERNEL_CASES[name]
    x, g, old = U.large_inputs(geom[:4])
    assert np.all(np.abs(x) == 60000.0)
    got = _check(geom, x, g, old, name + "-large")
    assert np.isfinite(got["y"]).all() and np.isfinite(got["dx"]).all()


@pytest.mark.parametrize("name", ["slice", "runs", "capped"])
def test_two_runs_give_the_same_bytes(name):
    geom = U.KERNEL_CASES[name]
    x, g, old = U.normal_inputs(geom[:4])
    for o in (None, old):
        a, b = _run(geom, x, g, o), _run(geom, x, g, o)
        for p, q in zip(a["raw"], b["raw"]):
            assert torch.equal(p.view(torch.int16) if p.dtype == torch.float16 else p.view(torch.int32),
                               q.view(torch.int16) if q.dtype == torch.float16 else q.view(torch.int32))


# ----------------------------------------------------------------------------- 2. the module against the reference
@pytest.mark.parametrize("case", list(U.MODULE_CASES))
def test_module_vs_golden(golden, case):
    """l2err of y and gx below 4 x the tolerance the generator measured for the case (the error of a float64 emulation of this path's
    fp16 storage against the reference's fp32 values)."""
    from ultralytics.nn.extra_modules.attention import SimAM
    G = golden("simam")
    C, H, W, lam, off, spread = U.MODULE_CASES[case]
    seed = U.MODULE_SEEDS[case]
    m = SimAM(lam)
    x = off + spread * rnd(10 * seed, U.BATCH, C, H, W)
    gy = rnd(10 * seed + 9, U.BATCH, C, H, W)
    y, gxs, rt = run_fwd_bwd(m, [x], gy)
    got, want = dict(y=y, gx=gxs[0]), dict(y=G.t(f"mod/{case}/y"), gx=G.t(f"mod/{case}/gx"))
    tols = {k: float(G[f"tol/{case}/{k}"]) for k in got}
    errs = {k: l2err(got[k].reshape(want[k].shape), want[k]) for k in got}
    print(case, {k: f"{errs[k]:.2e} (4 x {tols[k]:.2e})" for k in errs})
    for k in got:
        assert errs[k] < 4 * tols[k], k


def test_engine_refuses_by_name_and_prunes_without_a_gradient():
    from ultralytics.nn.extra_modules.attention import SimAM
    m = SimAM().cuda()
    rt = m._runtime(torch.device("cuda", 0))
    eng = rt.eng
    act = lambda c, h=4: eng.wrap_act(torch.zeros(1, h, 4, c, dtype=torch.float16, device="cuda"))  # noqa: E731
    with pytest.raises(NotImplementedError, match=r"SimAM.*an input of width 12"):
        eng.simam(act(16).sub(0, 12))
    eng.tape = []
    y = eng.simam(act(16))  # an input that needs no gradient: nothing on the tape, the output marked
    torch.cuda.synchronize()
    assert (y.N, y.H, y.W, y.C) == (1, 4, 4, 16) and len(eng.tape) == 0 and y.needs_grad is False
    eng.tape = None


# ----------------------------------------------------------------------------- 3. the graph against the reference
def _model(G, name=U.MODEL):
    from ultralytics.nn.tasks import DetectionModel
    m = DetectionModel(os.path.join(CFG_DIR, name + ".yaml"), ch=3, verbose=False)
    if name == U.MODEL:
        m.load_state_dict(U.state(G, U.MODEL), strict=True)
    return m.cuda()


def _names(ops):
    return [o[2] for o in ops if o[0] is not None]


def _simam_maps(ops, name="dy_simam_forward"):
    """(H, W, C) of the launches of one entry, in list order (argument positions: include/dealyolo_hip.h)."""
    k = 8 if name == "dy_simam_forward" else 10
    return [tuple(o[1][k:k + 3]) for o in ops if o[0] is not None and o[2] == name]


def test_eval_and_fused_eval_vs_golden(golden):
    """Box rows and class scores at 4 x the generator's measured tolerances; the second call of a geometry is traced into an
    InferPlan, the third replays it: all three bit for bit; three dy_simam_forward launches in the list, one per detection level."""
    G = golden("simam")
    m = _model(G).eval()
    x = G.t("batch/img").cuda()
    for key in ("y_eval", "y_eval_fused"):
        if key == "y_eval_fused":
            m.fuse()
            assert not hasattr(m.model[1], "bn")
        ref = G.t(f"{U.MODEL}/{key}")
        with torch.no_grad():
            y1, _ = m(x)   # walked
            assert not m._infer_plans["plans"]
            y2, _ = m(x)   # traced into a plan
            plan = m._infer_plans["plans"][(2, 3, 64, 64)]
            y3, _ = m(x)   # replayed
        torch.cuda.synchronize()
        assert _simam_maps(plan.rec.ops) == [(16, 16, 32), (8, 8, 64), (4, 4, 128)]
        assert torch.equal(y1, y2) and torch.equal(y1, y3)
        assert y1.shape == ref.shape
        eb, ec = relerr(y1[:, :4].cpu(), ref[:, :4]), relerr(y1[:, 4:].cpu(), ref[:, 4:])
        tb, tc = float(G[f"tol/{U.MODEL}/{key}_box"]), float(G[f"tol/{U.MODEL}/{key}_cls"])
        print(f"{key}: box relerr {eb:.2e} (4 x {tb:.2e}) cls relerr {ec:.2e} (4 x {tc:.2e})")
        assert eb < 4 * tb and ec < 4 * tc


def test_augmented_forward_vs_golden(golden):
    G = golden("simam")
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
    """One training step: loss items, loss, every gradient's norm (median / max of the relative error), the first layer's gradient in
    full and, after one clipped SGD-nesterov step, the norms of every tensor's change, at 4 x the tolerances the generator measured
    for them (tol/<model>/...).  The traced list holds three forward and three backward launches; the backward of row 27 ADDS to
    the gradient of row 20, which the Conv of row 21 wrote first or writes after it (one accumulate flag set among rows 26-28 at least
    when the other writer came first)."""
    from ultralytics.hip.train import StepPlan
    G = golden("simam")
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
    assert _simam_maps(plan.rec_fb.ops) == [(16, 16, 32), (8, 8, 64), (4, 4, 128)]
    assert sorted(_simam_maps(plan.rec_fb.ops, "dy_simam_backward")) == sorted([(16, 16, 32), (8, 8, 64), (4, 4, 128)])
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
    for k in got:
        assert got[k] < 4 * tol[k], k


def test_replayed_and_captured_steps_equal_the_traced_step(golden):
    """The traced step, its replay (twice) and a hipGraph of the same list on the same state and batch: no atomics in the SimAM
    kernels, so loss items and ALL gradients are EQUAL."""
    from ultralytics.hip.train import StepPlan
    G = golden("simam")
    outs = []
    for graph in (False, True):
        m = _model(G).train()
        plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0, use_graph=graph)
        sd0 = {k: v.clone() for k, v in m.state_dict().items()}
        for rep in range(3):  # traced, then replayed twice (captured: the graph's replays)
            m.load_state_dict(sd0)
            plan.forward_backward(U.batch(G))
            torch.cuda.synchronize()
            outs.append((plan.rt.flat_g.clone(), plan.crit.scalars.clone()))
        if graph:
            assert plan.graph_fb is not None
        assert _names(plan.rec_fb.ops).count("dy_simam_backward") == 3
    assert torch.isfinite(outs[0][0]).all() and float(outs[0][0].abs().max()) > 0
    for g, s in outs[1:]:
        assert torch.equal(outs[0][1][5:9], s[5:9]) and torch.equal(outs[0][0], g)


def _frozen_step(G, freeze):
    from ultralytics.engine.trainer import frozen_parameter_names
    from ultralytics.hip.train import StepPlan
    m = _model(G).train()
    frozen = set(frozen_parameter_names([k for k, _ in m.named_parameters()], freeze))
    for k, v in m.named_parameters():
        v.requires_grad = k not in frozen
    start = {k: v.detach().clone() for k, v in m.state_dict().items()}
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.set_hyper([0.01] * 3, 0.9, [0.0, 5e-4, 0.0])
    plan.forward_backward(U.batch(G))
    plan.optimizer_step()
    torch.cuda.synchronize()
    return m, plan, start, frozen


def test_freeze_8_keeps_the_backward_and_a_frozen_upstream_drops_it(golden):
    """freeze=8 (the backbone): every SimAM input still needs a gradient, three backward launches.  freeze=26 (everything upstream of
    the three blocks): no input needs one, no backward launch, three forward launches; only Detect moves.  freeze=[26] names a layer
    without parameters: the list equals the unfrozen one's."""
    G = golden("simam")
    m, plan, start, frozen = _frozen_step(G, 8)
    ops = _names(plan.rec_fb.ops)
    assert [ops.count(k) for k in ("dy_simam_forward", "dy_simam_backward")] == [3, 3]
    sd = m.state_dict()
    assert all(torch.equal(sd[k], start[k]) for k in frozen) and not torch.equal(sd["model.20.cv2.conv.weight"], start["model.20.cv2.conv.weight"])
    m, plan, start, frozen = _frozen_step(G, 26)
    ops = _names(plan.rec_fb.ops)
    assert [ops.count(k) for k in ("dy_simam_forward", "dy_simam_backward")] == [3, 0]
    sd = m.state_dict()
    moved = [k for k in start if start[k].is_floating_point() and "running" not in k and not torch.equal(sd[k], start[k])]
    assert moved and all(k.startswith("model.29.") for k in moved)
    _, plan_a, _, fa = _frozen_step(G, [26])
    _, plan_b, _, fb = _frozen_step(G, None)
    assert fa == fb and _names(plan_a.rec_fb.ops) == _names(plan_b.rec_fb.ops)
    assert torch.equal(plan_a.rt.flat_g, plan_b.rt.flat_g)


def test_reference_written_checkpoint_runs(golden):
    """attempt_load_weights of tests/golden/ref_ckpt_simam.pt (module path ultralytics.nn.extra_modules.attention.SimAM): the eval
    forward is the reference's (4 x tol/ckpt/y_eval_*) and EQUALS that of a natively built model with the same fp16-rounded state."""
    from ultralytics.nn.tasks import DetectionModel, attempt_load_weights, torch_safe_load
    G = golden("simam")
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


def test_multi_scale_over_one_arena():
    """multi_scale=True: one recorded launch list per drawn size, all over one arena; in every list the three planes follow the size
    (H = size / 4, / 8, / 16, so n = H W - 1 does too); every optimizer step takes effect."""
    from ultralytics import YOLO
    from ultralytics.data import SyntheticDetection
    torch.manual_seed(0)
    y = YOLO(os.path.join(CFG_DIR, U.MODEL + ".yaml"))
    src = SyntheticDetection(n_batches=8, batch=4, imgsz=64, boxes_per_image=3, wh=(0.1, 0.4), seed=3)
    hist = y.train(data=src, batch=4, imgsz=64, epochs=1, optimizer="SGD", warmup_epochs=0.0, lr0=0.01, nbs=4, hipgraph=True,
                   multi_scale=True, amp=False)
    tr = y.trainer
    plans = {k[1]: p for k, p in tr.plans.items() if isinstance(k, tuple)}
    assert len(plans) >= 2 and all(torch.isfinite(torch.as_tensor(h)).all() for h in hist), sorted(plans)
    for size, p in plans.items():
        sz = size if isinstance(size, int) else size[0]
        assert _simam_maps(p.rec_fb.ops) == [(sz // 4, sz // 4, 32), (sz // 8, sz // 8, 64), (sz // 16, sz // 16, 128)], size
        assert len(_simam_maps(p.rec_fb.ops, "dy_simam_backward")) == 3
    assert float(tr.plan.state[5]) == 8 and float(tr.plan.state[6]) == 0
    assert tr.arena is not None and 0 < tr.arena.peak <= tr.arena.cap


def test_tiled_prediction_runs_the_blocks(golden):
    """Sliced inference over a 100 x 150 frame in 64 x 64 tiles: the tiles' eval plan holds the three forward launches at the tile's
    planes, the merged boxes are finite, and a second call gives the same rows."""
    from ultralytics.utils.tiled import tiled_predict
    G = golden("simam")
    m = _model(G).eval()
    frame = np.random.default_rng(1).integers(0, 255, (100, 150, 3), dtype=np.uint8)
    a = tiled_predict([frame], m, tile=64, conf=0.001)[0]
    b = tiled_predict([frame], m, tile=64, conf=0.001)[0]
    assert a.shape[-1] == 6 and torch.isfinite(a).all() and torch.equal(a, b)
    plans = [p for p in m._infer_plans["plans"].values()]
    assert plans and all(_simam_maps(p.rec.ops) == [(16, 16, 32), (8, 8, 64), (4, 4, 128)] for p in plans)


def test_default_graph_launches_no_simam_kernel(golden):
    from ultralytics.hip.train import StepPlan
    G = golden("simam")
    m = _model(G, U.BASE).train()
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.forward_backward(U.batch(G))
    torch.cuda.synchronize()
    ops = _names(plan.rec_fb.ops)
    assert ops and not [n for n in ops if n.startswith("dy_simam")]
