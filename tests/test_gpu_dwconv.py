"""-m gpu: depthwise convolution (DWConv, reference nn/modules/conv.py:106-111; DSConv, :113-122) on the HIP path.

1. the kernels (csrc/dwconv.hip) per element against the float64 values of tests/dwconv_ref.py (F.conv2d(groups=c1) and
   torch.nn.grad in float64 on the fp16 activations and fp32 weights the kernels see; tests/test_host_dwconv.py ties them to
   autograd at 1e-11), dense and on channel slices, under the rule of tests/tensor_ops_ref.py

       |got - ref| <= k16 * 2^-11 * |ref| + k32 * 2^-23 * mag + 2^-24

   mag = the sum of the absolute values of the element's terms.  No element is left out.  k16 = 1 is an fp16 store, 0 for the fp32
   outputs.  k32 counts half an ulp (0.5) per fp32 rounding on the element's longest path, each relative to a partial sum that mag
   bounds; a product of an fp16 value and an fp16 / fp32 value enters through a fused multiply-add, so it adds no rounding of its
   own.  Counted from the orders the kernel file documents, before the first GPU run (tests/dwconv_util.py::k_bound holds the
   numbers, tests/test_host_dwconv.py runs an fp32 emulation of the orders against them):

     forward      k32 = k k / 2: one fused multiply-add per tap (4.5 for k 3, 12.5 for k 5)
     input grad   k32 = m k k / 2: at most k k taps reach a pixel (fewer at stride 2), m output channels per tap; + 0.5 for the
                  addition of the old value when accumulating (mag then includes |old|)
     weight grad  k32 = (T + S + ceil(P / 8) + 8) / 2: T = ceil(npix / (P S)) fused multiply-adds of one thread over its pixels,
                  S pixel slots added in order, the slabs of one of 8 runs, the 8 runs (P slabs, S = 256 / granules of the chunk;
                  the chunk that makes T + S largest); + 0.5 when accumulating
     statistics   k32 = (T + S) / 2 per partial row, for the sum (mag = sum |v|) and for the sum of squares (mag = sum v^2: v v
                  is exact in fp32); the rows are added in float64 here

2. each entry twice: the same bits; the statistics epilogue against float64 sums of the raw output the kernel wrote; the
   bias + SiLU epilogue against SiLU(raw + bias) of that raw output within one fp16 ulp; canaries around everything written.
3. the modules against the reference's fp32 values at 4 x the tolerance the generator measured (tol/<case>/...: the error of a
   float64 emulation of this path's storage against the same values); 4. the graph yolov8n-ASF-P2P2-DW: eval / fused eval
   (2e-2, the eval bound of tests/test_gpu_spd.py), one training step at 4 x the generator's measured tolerances, captured =
   eager, freeze, a reference-written checkpoint, augment=True, the public trainer, SOAP's refusal; 5. the default graph
   launches no dy_dwconv_* kernel."""
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

import dwconv_ref as R
import dwconv_util as U
from conftest import CFG_DIR
from golden.cases import rnd
from gpu_util import l2err, relerr, run_fwd_bwd

pytestmark = pytest.mark.gpu
POISON = -1234.0  # exactly representable in fp16
GUARD = 3         # canary pixels behind every written tensor
SEED = 900
EPI_STATS, EPI_BIAS, EPI_SILU = 1, 2, 4
_REF = {}
VARIANTS = [(n, "dense") for n in U.KERNEL_CASES] + [(U.SLICED, "sliced")]
IDS = [f"{n}-{v}" for n, v in VARIANTS]


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
        return self.s[:self.npix, self.c0:self.c0 + self.C].reshape(self.shape).cpu()

    def clean(self):
        """Nothing outside the slice was written."""
        return bool((self.s[self.npix:] == POISON).all()) and bool((self.s[:, :self.c0] == POISON).all()) and \
            bool((self.s[:, self.c0 + self.C:] == POISON).all())


def _f32(n, fill=POISON):
    return torch.full((n + 8,), fill, dtype=torch.float32, device="cuda")


def _case(name):
    """Operands, float64 references and magnitudes of a kernel case, computed once and shared."""
    if name not in _REF:
        geom = U.KERNEL_CASES[name]
        N, H, W, C1, m, k, s = geom
        x, w, dy, bias = R.inputs(*geom, SEED)
        _REF[name] = dict(geom=geom, x=x, w=w, dy=dy, bias=bias, fw=R.forward(x, w, s), ig=R.input_grad(dy, w, s, H, W, m),
                          wg=R.weight_grad(x, dy, k, s))
    return _REF[name]


def _dev_w(c):
    if "wd" not in c:
        c["wd"] = c["w"].cuda()
    return c["wd"]


def _forward(c, xb, yb, epi=0, part=None, bias=None):
    from ultralytics.hip import lib
    rc = lib().dy_dwconv_forward(xb.ptr, xb.ld, _dev_w(c).data_ptr(), 0 if bias is None else bias.data_ptr(),
                                 yb.ptr, yb.ld, 0 if part is None else part.data_ptr(), *c["geom"], epi, _stream())
    torch.cuda.synchronize()
    return rc


# ----------------------------------------------------------------------------- 1. / 2. the kernels, per element
@pytest.mark.parametrize("name,variant", VARIANTS, ids=IDS)
def test_forward_per_element_and_epilogues(name, variant):
    from ultralytics.hip import lib
    c = _case(name)
    N, H, W, C1, m, k, s = c["geom"]
    sl = variant == "sliced"
    _dev_w(c)
    xb = Buf(c["x"], sl)
    x0 = xb.s.clone()
    y0 = c["fw"]["y"]

    def out():
        return Buf(y0, sl, fill=POISON)

    # raw epilogue
    yb = out()
    assert _forward(c, xb, yb) == 0
    raw = yb.get()
    U.check("y", raw, y0, c["fw"]["mag"], U.k_bound("y", *c["geom"]))
    assert yb.clean() and torch.equal(xb.s, x0)
    y2 = out()
    assert _forward(c, xb, y2) == 0 and torch.equal(y2.s, yb.s)  # the same call again: the same bits
    # statistics epilogue: the same raw output, partial rows whose float64 sums are the sums of what was written
    P = lib().dy_dwconv_num_partials(*c["geom"])
    C2 = C1 * m
    part = _f32(P * 2 * C2)
    ys = out()
    assert _forward(c, xb, ys, EPI_STATS, part) == 0
    assert torch.equal(ys.s, yb.s) and bool((part[P * 2 * C2:] == POISON).all())
    rows = part[:P * 2 * C2].view(P, 2, C2).double().cpu()
    v = raw.double().reshape(-1, C2)
    kb = U.k_bound("stats", *c["geom"])
    U.check("sum", rows[:, 0].sum(0), v.sum(0), v.abs().sum(0), kb)
    U.check("sum of squares", rows[:, 1].sum(0), (v * v).sum(0), (v * v).sum(0), kb)
    part2 = _f32(P * 2 * C2)
    assert _forward(c, xb, out(), EPI_STATS, part2) == 0 and torch.equal(part2, part)
    # bias (+ SiLU) epilogue from the value the raw epilogue stores
    bias = c["bias"].cuda()
    yl = out()
    assert _forward(c, xb, yl, EPI_BIAS, None, bias) == 0 and yl.clean()
    z = raw.float() + c["bias"]  # fp32, as the kernel adds
    assert torch.equal(yl.get(), z.half())
    ya = out()
    assert _forward(c, xb, ya, EPI_BIAS | EPI_SILU, None, bias) == 0 and ya.clean()
    want = (z.double() * torch.sigmoid(z.double())).half().double()
    err = (ya.get().double() - want).abs()
    ulp = 2.0 ** -10 * want.abs() + 2.0 ** -24  # one fp16 ulp is at most 2^-10 of the value (2^-24 among the subnormals)
    print(f"bias + SiLU: worst err / ulp {float((err / ulp).max()):.3f}")
    assert bool((err <= ulp).all())
    ya2 = out()
    assert _forward(c, xb, ya2, EPI_BIAS | EPI_SILU, None, bias) == 0 and torch.equal(ya2.s, ya.s)


@pytest.mark.parametrize("name,variant", VARIANTS, ids=IDS)
def test_input_grad_per_element(name, variant):
    """The store flag, the add flag (one more rounding over |old|), a null destination, twice the same bits."""
    from ultralytics.hip import lib
    c = _case(name)
    N, H, W, C1, m, k, s = c["geom"]
    sl = variant == "sliced"
    w = _dev_w(c)
    db = Buf(c["dy"], sl)
    d0 = db.s.clone()

    def run(dxb, acc):
        rc = lib().dy_dwconv_input_grad(db.ptr, db.ld, w.data_ptr(), 0 if dxb is None else dxb.ptr, 0 if dxb is None else dxb.ld, acc, *c["geom"],
                                        _stream())
        torch.cuda.synchronize()
        return rc

    ref, mag = c["ig"]["dx"], c["ig"]["mag"]
    dxb = Buf(ref, sl, fill=POISON)
    assert run(dxb, 0) == 0
    U.check("dx", dxb.get(), ref, mag, U.k_bound("dx", *c["geom"]))
    assert dxb.clean() and torch.equal(db.s, d0)
    dx2 = Buf(ref, sl, fill=POISON)
    assert run(dx2, 0) == 0 and torch.equal(dx2.s, dxb.s)
    prev = torch.from_numpy(np.random.default_rng(7).standard_normal(tuple(ref.shape)).astype(np.float16))
    dxa = Buf(prev, sl)
    assert run(dxa, 1) == 0
    U.check("dx (add)", dxa.get(), ref + prev.double(), mag + prev.double().abs(), U.k_bound("dx", *c["geom"], accumulate=True))
    assert dxa.clean()
    assert run(None, 0) == 0  # a null destination: no launch


@pytest.mark.parametrize("name,variant", VARIANTS, ids=IDS)
def test_weight_grad_per_element(name, variant):
    from ultralytics.hip import lib
    c = _case(name)
    N, H, W, C1, m, k, s = c["geom"]
    sl = variant == "sliced"
    xb, db = Buf(c["x"], sl), Buf(c["dy"], sl)
    E = C1 * m * k * k
    ns = lib().dy_dwconv_wgrad_slabs(*c["geom"])

    def run(dw, acc):
        slabs = _f32(ns * E)
        rc = lib().dy_dwconv_wgrad(xb.ptr, xb.ld, db.ptr, db.ld, slabs.data_ptr(), dw.data_ptr(), acc, *c["geom"], _stream())
        torch.cuda.synchronize()
        assert bool((slabs[ns * E:] == POISON).all()) and bool(torch.isfinite(slabs[:ns * E]).all()) and not bool((slabs[:ns * E] == POISON).any())
        return rc

    ref, mag = c["wg"]["dw"], c["wg"]["mag"]
    k16, k32 = U.k_bound("dw", *c["geom"])
    dw = _f32(E)
    assert run(dw, 0) == 0
    U.check("dw", dw[:E].view(ref.shape), ref, mag, (k16, k32))
    assert bool((dw[E:] == POISON).all())
    dw2 = _f32(E)
    assert run(dw2, 0) == 0 and torch.equal(dw2, dw)
    prev = torch.from_numpy(np.random.default_rng(11).standard_normal(tuple(ref.shape)).astype(np.float32))
    dwa = _f32(E)
    dwa[:E] = prev.reshape(-1).cuda()
    assert run(dwa, 1) == 0
    U.check("dw (add)", dwa[:E].view(ref.shape), ref + prev.double(), mag + prev.double().abs(), (k16, k32 + 0.5))


# ----------------------------------------------------------------------------- engine-level refusals
def _engine_spec(c1=16, c2=16, k=3, s=1):
    from ultralytics.nn.modules import DWConv
    m = DWConv(c1, c2, k, s).cuda()
    rt = m._runtime(torch.device("cuda", 0))
    return m, rt, rt.spec(m)


def test_engine_refuses_a_12_channel_input_and_a_residual():
    m, rt, spec = _engine_spec()
    eng = rt.eng
    assert spec.dw and (spec.cin, spec.cout, spec.mult) == (16, 16, 1) and spec.wpack is None and spec.acc_f is None
    x = eng.wrap_act(torch.zeros(1, 4, 4, 16, dtype=torch.float16, device="cuda"))
    with pytest.raises(NotImplementedError, match="Conv.*12 channels.*supported: c1 % 8 == 0"):
        eng.conv_bn_act(spec, x.sub(0, 12))
    with pytest.raises(NotImplementedError, match="Conv.*residual operand"):
        eng.conv_bn_act(spec, x, res=x)
    with pytest.raises(NotImplementedError, match="Conv.*residual operand"):
        eng.conv_fused(spec, x, res=x)
    from ultralytics.hip.engine import SegAct
    planes = SegAct(list(eng.new_planes(1, 4, 4, 8)))
    with pytest.raises(NotImplementedError, match="Conv.*two-plane output"):
        eng.conv_bn_act(spec, x, out=planes)
    with pytest.raises(NotImplementedError, match="Conv.*two-plane output"):
        eng.conv_fused(spec, x, out=planes)
    y = eng.conv_bn_act(spec, x)  # ... and the supported call runs
    torch.cuda.synchronize()
    assert (y.N, y.H, y.W, y.C) == (1, 4, 4, 16)


# ----------------------------------------------------------------------------- 3. the modules against the reference
@pytest.mark.parametrize("case", list(U.MODULE_CASES))
def test_module_vs_golden(golden, case):
    """l2err of y, gx and every parameter gradient below 4 x the tolerance the generator measured for the case.  The factor pays for
    another fp32 summation order and another position of the fp16 roundings, not for another algorithm.  Running statistics after
    the one forward: 2e-3, as tests/test_gpu_spd.py."""
    from ultralytics.nn.modules import DSConv, DWConv
    G = golden("dwconv")
    kind, c1, c2, k, s, act, H, W = U.MODULE_CASES[case]
    p = f"mod/{case}"
    seed = int(G[f"{p}/seed"])
    m = DWConv(c1, c2, k, s, act=act) if kind == "DWConv" else DSConv(c1, c2)
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


def _fuse(m):
    """BaseModel.fuse() over a module on its own (is_fused counts norm layers; a single layer has too few to be asked)."""
    from ultralytics.nn.tasks import BaseModel
    h = BaseModel()
    h.m, h.is_fused = m, lambda thresh=10: False
    h.fuse()
    return m


@pytest.mark.parametrize("kind,c1,c2,tol", [("DWConv", 96, 96, 2e-3), ("DWConv", 48, 96, 2e-3), ("DSConv", 96, 64, 4e-3), ("DWConv", 160, 160, 2e-3)])
def test_fused_eval_equals_unfused_eval_at_the_split_widths(kind, c1, c2, tol):
    """k 3, s 1 and 64 m + 16 / 32 outputs are the widths at which a fused DENSE conv runs as two launches (Conv._build_specs); a fused
    depthwise layer must not.  Fused against un-fused eval of the same module with non-trivial BatchNorm state.  Both paths round
    the pre-activation and the output to fp16 once each (2^-11 relative, 3e-4 in the norm), in another order: 2e-3; DSConv's folded
    1x1 weights are rounded to fp16 a second time: 4e-3.  A layer run as a dense convolution is off by its whole norm."""
    from ultralytics.nn.modules import DSConv, DWConv
    from ultralytics.nn.tasks import initialize_weights
    torch.manual_seed(5)
    m = DWConv(c1, c2, 3, 1) if kind == "DWConv" else DSConv(c1, c2)
    initialize_weights(m)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5); mod.bias.data.normal_(0, 0.3); mod.running_mean.normal_(0, 0.3); mod.running_var.uniform_(0.5, 1.5)
    x = rnd(4321, 2, c1, 9, 7).cuda()
    m.cuda().eval()
    with torch.no_grad():
        y0 = m(x).float().cpu()
        _fuse(m)
        convs = [m] if kind == "DWConv" else [m.dwconv, m.pwconv]
        assert all(not hasattr(c, "bn") for c in convs) and tuple(convs[0].conv.weight.shape) == (c2 if kind == "DWConv" else c1, 1, 3, 3)
        y1 = m(x).float().cpu()
    assert all(c.__dict__.get("_split") is None for c in convs[:1])
    e = l2err(y1, y0)
    print(f"{kind}({c1}, {c2}) fused against un-fused eval: l2err {e:.2e} ({tol:.0e})")
    assert e < tol


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
    """2e-2 on boxes and on class scores; the second call of a geometry is traced into an InferPlan, the third replays it: all three
    bit for bit, five dy_dwconv_forward launches in the list."""
    G = golden("dwconv")
    m = _model(G).eval()
    x = G.t("batch/img").cuda()
    for key in ("y_eval", "y_eval_fused"):
        if key == "y_eval_fused":
            m.fuse()
            assert tuple(m.model[1].conv.weight.shape) == (32, 1, 3, 3)
        ref = G.t(f"{U.MODEL}/{key}")
        with torch.no_grad():
            y1, _ = m(x)   # walked
            assert not m._infer_plans["plans"]
            y2, _ = m(x)   # traced into a plan
            plan = m._infer_plans["plans"][(2, 3, 64, 64)]
            y3, _ = m(x)   # replayed
        torch.cuda.synchronize()
        assert _names(plan.rec.ops).count("dy_dwconv_forward") == 5
        assert torch.equal(y1, y2) and torch.equal(y1, y3)
        assert y1.shape == ref.shape
        eb, ec = relerr(y1[:, :4].cpu(), ref[:, :4]), relerr(y1[:, 4:].cpu(), ref[:, 4:])
        print(f"{key}: box relerr {eb:.2e} cls relerr {ec:.2e}")
        assert eb < 2e-2 and ec < 2e-2


def test_train_step_vs_golden(golden):
    """One training step: loss items, loss, gradient norms (median / max of the relative error, tests/test_gpu_carafe.py's formula)
    and the first layer's gradient at 4 x the tolerances the generator measured for them (tol/<model>/...)."""
    from ultralytics.hip.train import StepPlan
    G = golden("dwconv")
    tol = {k: float(G[f"tol/{U.MODEL}/{k}"]) for k in ("items", "loss", "grad_l2_median", "grad_l2_max", "grad_first")}
    m = _model(G).train()
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.forward_backward(U.batch(G))
    torch.cuda.synchronize()
    ops = _names(plan.rec_fb.ops)
    assert ops.count("dy_dwconv_forward") == 5 and ops.count("dy_dwconv_wgrad") == 5 and ops.count("dy_dwconv_input_grad") == 5
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
    print("items", s[5:8].tolist(), ref_items.tolist())
    print({k: f"{got[k]:.2e} (4 x {tol[k]:.2e})" for k in got}, "worst gradient norm:", names[int(rel.argmax())])
    for i in U.DW_LAYERS:
        j = names.index(f"model.{i}.conv.weight")
        print(names[j], f"l2 {float(l2[j]):.4e} reference {float(ref[j]):.4e} rel {float(rel[j]):.2e}")
    for k in got:
        assert got[k] < 4 * tol[k], k
    sd = m.state_dict()
    rm = [str(k) for k in G[f"{U.MODEL}/run_mean_names"]]
    assert relerr(torch.stack([sd[k].sum() for k in rm]).cpu(), G.t(f"{U.MODEL}/run_mean_sum")) < 5e-3
    assert relerr(torch.stack([sd[k.replace("mean", "var")].sum() for k in rm]).cpu(), G.t(f"{U.MODEL}/run_var_sum")) < 5e-3
    assert torch.isfinite(plan.rt.flat_g).all() and float(plan.state[2]) == 0.0


def test_captured_step_equals_the_eager_step(golden):
    """One StepPlan step replayed as a hipGraph against the eager tape step of another plan on the same state and batch: the same
    launches, no atomics in the depthwise kernels, so loss items and ALL gradients are EQUAL."""
    from ultralytics.hip.train import StepPlan
    G = golden("dwconv")
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
        assert ops.count("dy_dwconv_forward") == 5 and ops.count("dy_dwconv_wgrad") == 5
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


A_WG_DW, A_DG_W = 5, 2  # argument positions (include/dealyolo_hip.h): dw of dy_dwconv_wgrad, w of dy_dwconv_input_grad


def test_freeze_4_prunes_rows_1_and_3(golden):
    """freeze=4 (layers 0-3): rows 1 and 3 are frozen and nothing trainable lies upstream of them, so they leave nothing on the tape:
    no weight-gradient launch, no input-gradient launch, their parameters do not move; rows 5, 18, 21 keep both."""
    from ultralytics.engine.trainer import frozen_parameter_names
    G = golden("dwconv")
    names = [k for k, _ in _model(G).named_parameters()]
    frozen = set(frozen_parameter_names(names, 4))
    assert {"model.1.conv.weight", "model.3.bn.bias"} <= frozen and "model.5.conv.weight" not in frozen
    m, plan, start = _frozen_step(G, frozen)
    rt = plan.rt
    sp = {i: rt.spec(m.model[i]) for i in U.DW_LAYERS}
    assert not sp[1].trainable and not sp[3].trainable and all(sp[i].trainable for i in (5, 18, 21))
    ops = [o for o in plan.rec_fb.ops if o[0] is not None]
    assert _names(ops).count("dy_dwconv_forward") == 5
    wg = [o[1][A_WG_DW] for o in ops if o[2] == "dy_dwconv_wgrad"]
    assert sorted(wg) == sorted(sp[i].gweight.data_ptr() for i in (5, 18, 21))
    dg = [o[1][A_DG_W] for o in ops if o[2] == "dy_dwconv_input_grad"]
    assert sorted(dg) == sorted(sp[i].weight.data_ptr() for i in (5, 18, 21))
    ws = {id(s) for s in plan.wgrad_specs}
    assert not (id(sp[1]) in ws or id(sp[3]) in ws) and all(id(sp[i]) in ws for i in (5, 18, 21))
    sd = m.state_dict()
    for k in frozen:
        assert torch.equal(sd[k], start[k]), f"frozen parameter {k} moved"
    for i in (5, 18, 21):
        assert not torch.equal(sd[f"model.{i}.conv.weight"], start[f"model.{i}.conv.weight"]), i
    assert float(rt.flat_g[rt.frozen.bool()].abs().max()) == 0.0 and torch.isfinite(rt.flat_g).all()


def test_frozen_row_with_a_trainable_prefix_keeps_its_input_gradient(golden):
    """freeze=[3], layer 2 trainable: row 3's weight-gradient launch is pruned, its input gradient runs alone, and the gradient
    everything upstream receives equals the unfrozen step's."""
    from ultralytics.engine.trainer import frozen_parameter_names
    G = golden("dwconv")
    names = [k for k, _ in _model(G).named_parameters()]
    frozen = set(frozen_parameter_names(names, [3]))
    assert frozen and all(k.startswith("model.3.") for k in frozen if ".dfl" not in k)
    m, plan, start = _frozen_step(G, frozen)
    sp3 = plan.rt.spec(m.model[3])
    assert not sp3.trainable
    ops = [o for o in plan.rec_fb.ops if o[0] is not None]
    assert _names(ops).count("dy_dwconv_wgrad") == 4 and _names(ops).count("dy_dwconv_input_grad") == 5
    assert sp3.weight.data_ptr() in [o[1][A_DG_W] for o in ops if o[2] == "dy_dwconv_input_grad"]
    assert id(sp3) not in {id(s) for s in plan.wgrad_specs}
    gptr = sp3.gweight.data_ptr()
    for fn, args, name, _sid in ops:
        assert not [a for a in args if isinstance(a, int) and a == gptr], f"{name} writes a frozen weight's gradient"
    sd = m.state_dict()
    for k in frozen:
        assert torch.equal(sd[k], start[k])
    m2, plan2, _ = _frozen_step(G, {k for k in frozen if ".dfl" in k})
    # the frozen row runs the same reduce, apply and input-gradient launches on the same d(raw), all of them deterministic: EQUAL
    for k0 in ("model.2.cv1.conv.weight", "model.2.m.0.cv2.bn.weight", "model.1.conv.weight", "model.1.bn.bias", "model.0.conv.weight"):
        g1, g2 = dict(m.named_parameters())[k0].grad, dict(m2.named_parameters())[k0].grad
        assert torch.equal(g1, g2) and float(g2.abs().max()) > 0, k0


def test_reference_written_checkpoint_runs(golden):
    """attempt_load_weights of tests/golden/ref_ckpt_dw.pt (module path ultralytics.nn.modules.conv.DWConv): the eval forward is the
    reference's (2e-2) and EQUALS that of a natively built model with the same fp16-rounded state."""
    from ultralytics.nn.tasks import DetectionModel, attempt_load_weights, torch_safe_load
    G = golden("dwconv")
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
    print(f"checkpoint eval: box relerr {eb:.2e} cls relerr {ec:.2e}")
    assert eb < 2e-2 and ec < 2e-2


def test_augmented_forward_runs(golden):
    """model(x, augment=True): walked, recorded, replayed give the same bits; against the reference's augmented forward at the
    eval bound (2e-2: the three scales each carry the eval forward's fp16 error)."""
    G = golden("dwconv")
    m = _model(G).eval()
    x = G.t("batch/img").cuda()
    want = G.t(f"{U.MODEL}/y_aug")
    ys = []
    for _ in range(3):
        y, second = m(x, augment=True)
        assert second is None and tuple(y.shape) == tuple(want.shape)
        ys.append(y.clone())
    eb, ec = relerr(ys[0][:, :4], want[:, :4]), relerr(ys[0][:, 4:], want[:, 4:])
    print(f"augment: box relerr {eb:.2e}, class relerr {ec:.2e}")
    assert eb < 2e-2 and ec < 2e-2
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


def test_two_epochs_through_the_public_trainer():
    from ultralytics import YOLO
    from ultralytics.data import SyntheticDetection
    torch.manual_seed(0)
    y = YOLO("yolov8n-ASF-P2P2-DW.yaml")
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
    still = [f"model.{i}.conv.weight" for i in U.DW_LAYERS if torch.equal(w1[f"model.{i}.conv.weight"].cpu(), w0[f"model.{i}.conv.weight"].cpu())]
    assert not still, f"depthwise weights that never moved: {still}"
    assert torch.isfinite(plan.rt.flat_g).all()


def test_soap_names_the_depthwise_weight_and_raises(golden):
    """optimizer='SOAP' on this graph: the grouped HIP step refuses the (C, 1, k, k) tensors by name instead of mis-shaping them."""
    from ultralytics.hip.train import StepPlan
    G = golden("dwconv")
    m = _model(G).train()
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.set_hyper([0.01] * 3, 0.9, [0.0, 5e-4, 0.0])
    with pytest.raises(NotImplementedError, match=r"conv\.weight.*\(C, 1, k, k\)"):
        plan._soap_make()


# ----------------------------------------------------------------------------- 5. the default graph
def test_default_graph_launches_no_depthwise_kernel(golden):
    from ultralytics.hip.train import StepPlan
    G = golden("dwconv")
    m = _model(G, "yolov8n-ASF-P2P2").train()
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.forward_backward(U.batch(G))
    torch.cuda.synchronize()
    ops = _names(plan.rec_fb.ops)
    assert ops and not [n for n in ops if n.startswith("dy_dwconv")]
    assert not any(sp.dw for sp in plan.rt.specs.values())
