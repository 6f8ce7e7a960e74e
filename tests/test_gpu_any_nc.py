"""-m gpu: Conv + BatchNorm of ANY width on the HIP path -- what Detect's class branch needs for any class count (reference
nn/modules/head.py:36: c3 = max(ch[0], min(nc, 100)), so 33 <= nc <= 100 gives a c3 = nc wide Conv chain and nc > 100 a 100-wide one).

Reference everywhere: the CPU oracle (oracle/nn.py, oracle/loss.py) evaluated in float64 on the inputs the engine sees (the image /
input map rounded to fp16, the fp32 master parameters).  Tolerances are the ones the suite already holds the same quantities to for
32- and 64-wide Convs, each named where it is used; none is new.

Before this change every test of this file stopped at ``Storage.__init__`` ("channel count 37 must be a multiple of 8") and the
Conv(24, 40, 1) training case at the three-launch form's "BN channel counts must be multiples of 16"."""
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import CFG_DIR
from gpu_util import act_grad_tensor, l2err, relerr
from oracle import graph as og

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------- module
# (cin, cout, k, nc of the nn.Conv2d behind it): Detect.cv3's shapes for nc = 37 / nc = 120, and a make_divisible(.., 8) width
CONVS = {"32-37k3": (32, 37, 3, 37), "37-37k3": (37, 37, 3, 37), "37-100k3": (37, 100, 3, 120), "24-40k1": (24, 40, 1, 40),
         "32-40k3": (32, 40, 3, 40), "40-40k3": (40, 40, 3, 40)}  # ... and Detect.cv3 at nc = 40: multiples of 8 that are none of 16
MAPS = {"2x8x12": (2, 8, 12), "1x5x7": (1, 5, 7)}
# tests/test_gpu_modules.py:38, TOL["Conv"] = (forward 3e-3, input gradient 6e-3, parameter gradients 4e-3): the Conv's own output;
# :68 running statistics 2e-3; :89 / :98 / :102 (Detect: Conv chain -> nn.Conv2d) logits 8e-3, input and parameter gradients 2e-2 --
# every gradient here has passed through the nn.Conv2d behind the Conv, as Detect's have.
TOL_Y, TOL_BUF, TOL_LOGIT, TOL_GRAD = 3e-3, 2e-3, 8e-3, 2e-2


def _tail_module(cin, cout, k, nc):
    from ultralytics.hip import DY_ACT_NONE
    from ultralytics.hip.runtime import HipModule
    from ultralytics.nn.modules import Conv

    class Tail(HipModule):
        """Conv -> nn.Conv2d(1x1, bias): the last two layers of a Detect branch."""

        def __init__(self):
            super().__init__()
            self.cv = Conv(cin, cout, k)
            self.head = nn.Conv2d(cout, nc, 1)

        def _build_specs(self, rt):
            rt.make_spec((id(self), "head"), self.head, None, DY_ACT_NONE, 1, 1, name="Tail.head")

        def forward_act(self, x):
            eng, ncp = self.rt.eng, (nc + 7) // 8 * 8
            c = self.cv.forward_act(x)
            out = torch.zeros((x.N, c.H, c.W, ncp), dtype=torch.float32, device=eng.device)
            dout = torch.zeros((x.N, c.H, c.W, ncp), dtype=torch.float16, device=eng.device)
            eng.conv_bias(self.rt.specs[(id(self), "head")], c, out.data_ptr(), ncp, True, lambda: (dout.data_ptr(), ncp))
            return c, out, dout
    return Tail()


def _state(cin, cout, k, nc, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {"cv.conv.weight": r(cout, cin, k, k) / (cin * k * k) ** 0.5, "cv.bn.weight": torch.rand(cout, generator=g) + 0.5,
            "cv.bn.bias": r(cout) * 0.2, "cv.bn.running_mean": r(cout) * 0.3, "cv.bn.running_var": torch.rand(cout, generator=g) + 0.5,
            "cv.bn.num_batches_tracked": torch.tensor(3), "head.weight": r(nc, cout, 1, 1) / cout ** 0.5, "head.bias": r(nc) * 0.1}


def _oracle(sd, x, k, training, gy=None):
    """float64: (Conv output, logits, {gradients}, state after the forward)."""
    import oracle.nn as onn
    sd = {n: (v.double().clone().requires_grad_(v.dim() > 0 and "running" not in n) if v.is_floating_point() else v.clone()) for n, v in sd.items()}
    x = x.double().clone().requires_grad_(True)
    c = onn.conv_bn_silu(sd, "cv", x, k, 1, training)
    out = F.conv2d(c, sd["head.weight"], sd["head.bias"])
    grads = {}
    if gy is not None:
        (out * gy.double()).sum().backward()
        grads = {n: v.grad for n, v in sd.items() if v.is_floating_point() and v.requires_grad}
        grads["x"] = x.grad
    return c.detach(), out.detach(), grads, {n: v.detach() for n, v in sd.items()}


def _run(m, x, training, gy=None):
    from ultralytics.nn.tasks import initialize_weights
    initialize_weights(m)
    m.cuda().train(training)
    rt = m._runtime(torch.device("cuda", 0))
    eng = rt.eng
    eng.training, eng.tape = training, ([] if gy is not None else None)
    rt.pack_all(True)
    # the input as a producer of that width would leave it: logical width cin in a round8(cin) storage, zero pad lanes, wanting a gradient
    # (Runtime.to_act pads a width that is not a multiple of 8 like the image: no gradient)
    from ultralytics.hip.runtime import Storage
    N, cin, H, W = x.shape
    st = Storage(eng, N, H, W, (cin + 7) // 8 * 8)
    st.buf.zero_()
    st.buf[..., :cin].copy_(x.cuda().permute(0, 2, 3, 1))
    xa = st.act(0, cin)
    c, out, dout = m.forward_act(xa)
    if gy is not None:
        dout[..., :gy.shape[1]].copy_(gy.cuda().permute(0, 2, 3, 1))
        for f in reversed(eng.tape):
            f()
    eng.tape = None
    torch.cuda.synchronize()
    return rt, xa, c, out


def _check_pads(a, what):
    """The lanes behind the logical width of an activation (and of its gradient twin, where one exists) are +0.0."""
    if a.Cp != a.C:
        assert not bool((a.st.buf[..., a.c0 + a.C:a.c0 + a.Cp].contiguous().view(torch.int16) != 0).any()), f"pad lanes of {what}"


@pytest.mark.parametrize("mp", list(MAPS))
@pytest.mark.parametrize("case", list(CONVS))
def test_conv_training_forward_backward(case, mp):
    cin, cout, k, nc = CONVS[case]
    N, H, W = MAPS[mp]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, cin, H, W, generator=g).half().float()
    gy = torch.randn(N, nc, H, W, generator=g).half().float()
    sd = _state(cin, cout, k, nc, 5)
    m = _tail_module(cin, cout, k, nc)
    m.load_state_dict(sd, strict=True)
    rt, xa, c, out = _run(m, x, True, gy)
    rc, rout, rg, rsd = _oracle(sd, x, k, True, gy)
    assert (c.C, c.ld) == (cout, (cout + 7) // 8 * 8)
    _check_pads(c, "the Conv's output")
    y = rt.to_tensor(c).float().cpu()
    e = {"y": relerr(y, rc), "logits": relerr(out[..., :nc].permute(0, 3, 1, 2).cpu(), rout)}
    assert torch.isfinite(out).all() and not bool((out[..., nc:] != 0).any())
    e["gx"] = relerr(act_grad_tensor(xa).cpu(), rg["x"])
    if xa.Cp != xa.C:  # the input gradient's pad lanes are written too, as zeros
        assert not bool((xa.st.gbuf[..., xa.C:].contiguous().view(torch.int16) != 0).any()), "pad lanes of the input gradient"
    params = dict(m.named_parameters())
    for n in ("cv.conv.weight", "cv.bn.weight", "cv.bn.bias", "head.weight", "head.bias"):
        e[n] = relerr(params[n].grad.cpu(), rg[n])
    bufs = dict(m.named_buffers())
    e["running_mean"] = relerr(bufs["cv.bn.running_mean"].cpu(), rsd["cv.bn.running_mean"])
    e["running_var"] = relerr(bufs["cv.bn.running_var"].cpu(), rsd["cv.bn.running_var"])
    print(case, mp, {n: f"{v:.2e}" for n, v in e.items()})
    assert e["y"] < TOL_Y and e["logits"] < TOL_LOGIT
    assert all(e[n] < TOL_GRAD for n in ("gx", "cv.conv.weight", "cv.bn.weight", "cv.bn.bias", "head.weight", "head.bias")), e
    assert e["running_mean"] < TOL_BUF and e["running_var"] < TOL_BUF
    assert int(bufs["cv.bn.num_batches_tracked"]) == int(rsd["cv.bn.num_batches_tracked"]) == 4


@pytest.mark.parametrize("fused", [False, True], ids=["eval", "fused"])
@pytest.mark.parametrize("mp", list(MAPS))
@pytest.mark.parametrize("case", list(CONVS))
def test_conv_eval_and_fused(case, mp, fused):
    import oracle.nn as onn
    cin, cout, k, nc = CONVS[case]
    N, H, W = MAPS[mp]
    x = torch.randn(N, cin, H, W, generator=torch.Generator().manual_seed(12)).half().float()
    sd = _state(cin, cout, k, nc, 6)
    m = _tail_module(cin, cout, k, nc)
    m.load_state_dict(sd, strict=True)
    if fused:  # BaseModel.fuse's fold (nn/tasks.py), on this two-layer module
        fc = nn.Conv2d(cin, cout, k, 1, k // 2, bias=True).requires_grad_(False)
        fs = onn.fuse_state(None, {"cv.conv.weight": sd["cv.conv.weight"], **{f"cv.bn.{s}": sd[f"cv.bn.{s}"] for s in
                                   ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}})
        fc.weight.copy_(fs["cv.conv.weight"])
        fc.bias.copy_(fs["cv.conv.bias"])
        m.cv.conv = fc
        delattr(m.cv, "bn")
    rt, xa, c, out = _run(m, x, False)
    rc, rout, _, rsd = _oracle(sd, x, k, False)
    _check_pads(c, "the Conv's output")
    e = relerr(rt.to_tensor(c).float().cpu(), rc), relerr(out[..., :nc].permute(0, 3, 1, 2).cpu(), rout)
    print(case, mp, "fused" if fused else "eval", f"y {e[0]:.2e} logits {e[1]:.2e}")
    assert e[0] < TOL_Y and e[1] < TOL_LOGIT
    assert torch.equal(dict(m.named_buffers()).get("cv.bn.running_mean", sd["cv.bn.running_mean"].cuda()).cpu(), sd["cv.bn.running_mean"])


def test_poisoned_arena_leaves_no_trace(monkeypatch):
    """Every buffer the engine hands out filled with 0xFF (NaN as fp16): the pad lanes of the raw conv output are never written, so
    a reader that let one through would turn the logits or a gradient into NaN."""
    from ultralytics.hip import engine as E
    monkeypatch.setattr(E, "POISON", True)
    cin, cout, k, nc = CONVS["37-37k3"]
    g = torch.Generator().manual_seed(13)
    x, gy = torch.randn(2, cin, 8, 12, generator=g), torch.randn(2, nc, 8, 12, generator=g)
    m = _tail_module(cin, cout, k, nc)
    m.load_state_dict(_state(cin, cout, k, nc, 7), strict=True)
    rt, xa, c, out = _run(m, x, True, gy)
    assert torch.isfinite(out).all() and torch.isfinite(xa.st.gbuf).all()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    _check_pads(c, "the Conv's output")


@pytest.mark.parametrize("mode", ["train", "eval", "fused"])
def test_ragged_conv_behind_a_concat_with_a_poisoned_arena(mode, monkeypatch):
    """Concat -> Conv(32, 37, 1) -> Conv(37, 16, 3): a 1x1 Conv normally reads a concatenation through a segment table, and that launch
    takes no output width of its own.  A ragged output must still get its pad lanes written (eval: by the apply; fused: by the conv's
    epilogue), so the engine copies the members together and takes the plain launch.  Every buffer handed out is filled with 0xFF."""
    import oracle.nn as onn
    from ultralytics.hip import engine as E
    from ultralytics.hip.runtime import HipModule, Storage
    from ultralytics.nn.modules import Conv
    from ultralytics.nn.tasks import initialize_weights
    monkeypatch.setattr(E, "POISON", True)

    class CatTail(HipModule):
        def __init__(self):
            super().__init__()
            self.a, self.b = Conv(32, 37, 1), Conv(37, 16, 3)

        def forward_act(self, xs):
            mid = self.a.forward_act(self.rt.eng.concat(xs))
            return mid, self.b.forward_act(mid)
    g = torch.Generator().manual_seed(21)
    r = lambda *sh: torch.randn(*sh, generator=g)  # noqa: E731
    sd = {}
    for p, (ci, co, k) in (("a", (32, 37, 1)), ("b", (37, 16, 3))):
        sd.update({f"{p}.conv.weight": r(co, ci, k, k) / (ci * k * k) ** 0.5, f"{p}.bn.weight": torch.rand(co, generator=g) + 0.5,
                   f"{p}.bn.bias": r(co) * 0.2, f"{p}.bn.running_mean": r(co) * 0.3, f"{p}.bn.running_var": torch.rand(co, generator=g) + 0.5,
                   f"{p}.bn.num_batches_tracked": torch.tensor(0)})
    xs = [r(2, 16, 6, 9).half().float() for _ in range(2)]
    m = CatTail()
    m.load_state_dict(sd, strict=True)
    ref_sd = {n: (v.double().clone() if v.is_floating_point() else v.clone()) for n, v in sd.items()}
    with torch.no_grad():
        rmid = onn.conv_bn_silu(ref_sd, "a", torch.cat(xs, 1).double(), 1, 1, mode == "train")
        rout = onn.conv_bn_silu(ref_sd, "b", rmid, 3, 1, mode == "train")
    if mode == "fused":
        for p, (ci, co, k) in (("a", (32, 37, 1)), ("b", (37, 16, 3))):
            fs = onn.fuse_state(None, {f"{p}.conv.weight": sd[f"{p}.conv.weight"], **{f"{p}.bn.{q}": sd[f"{p}.bn.{q}"] for q in
                                       ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}})
            cv = getattr(m, p)
            fc = nn.Conv2d(ci, co, k, 1, k // 2, bias=True).requires_grad_(False)
            fc.weight.copy_(fs[f"{p}.conv.weight"])
            fc.bias.copy_(fs[f"{p}.conv.bias"])
            cv.conv = fc
            delattr(cv, "bn")
    initialize_weights(m)
    m.cuda().train(mode == "train")
    rt = m._runtime(torch.device("cuda", 0))
    eng = rt.eng
    eng.training, eng.tape = mode == "train", None
    rt.pack_all(True)
    acts = []
    for x in xs:  # two tensors of their own: the concatenation is a segment table (engine.SegAct), not a view
        st = Storage(eng, 2, 6, 9, 16)
        st.buf.copy_(x.cuda().permute(0, 2, 3, 1))
        acts.append(st.act())
    assert isinstance(eng.concat(acts), E.SegAct)
    mid, out = m.forward_act(acts)
    torch.cuda.synchronize()
    assert (mid.C, mid.ld) == (37, 40)
    _check_pads(mid, "the ragged Conv's output")
    y = rt.to_tensor(out).float().cpu()
    assert torch.isfinite(y).all() and torch.isfinite(mid.st.buf).all()
    e = relerr(rt.to_tensor(mid).float().cpu(), rmid), relerr(y, rout)
    print(mode, f"ragged Conv {e[0]:.2e}, Conv behind it {e[1]:.2e}")
    assert e[0] < TOL_Y and e[1] < 2 * TOL_Y  # (tests/test_gpu_modules.py:38 per Conv; two stacked Convs)


def test_other_consumers_refuse_a_ragged_width():
    """Only Conv / nn.Conv2d read a width that is not a multiple of 8: the other ops say so instead of asserting or mis-indexing."""
    from ultralytics.hip.engine import Engine
    eng = Engine("cuda:0")
    a, b = eng.new_act(1, 4, 4, 37), eng.new_act(1, 4, 4, 37)
    for name, f in (("Concat", lambda: eng.concat([a, b])), ("Add", lambda: eng.add([a, b])), ("Upsample", lambda: eng.upsample2x(a)),
                    ("SPDConv", lambda: eng.space_to_depth(a))):
        with pytest.raises(NotImplementedError, match=rf"{name}.*37"):
            f()


# ----------------------------------------------------------------------------------------------------------------------- graph
GRAPHS = [("yolov8n-ASF-P2P2", 37), ("yolov8n-ASF-P2P2", 120), ("yolov8n-LD-P2", 40), ("yolov8n-ASF-P2P2", 40)]
GIDS = [f"{n}-nc{c}" for n, c in GRAPHS]


def _build(name, nc, seed=None):
    # the filled state: seed 31; LD takes the seed tests/test_gpu_model.py fills that graph with (7 + 1)
    seed = seed if seed is not None else (8 if "LD" in name else 31)
    from ultralytics.nn.tasks import DetectionModel
    p = os.path.join(CFG_DIR, name + ".yaml")
    m = DetectionModel(p, ch=3, nc=nc, verbose=False)
    g = og.build_graph(og.load_yaml(p), nc=nc)
    sd = og.fill_state(og.state_layout(g), seed)
    m.load_state_dict(sd, strict=True)
    return m, g, sd


def _dbl(sd):
    return {k: (v.double().clone() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


@pytest.fixture(scope="module")
def oracle_eval():
    """{(name, nc)}: (image, float64 eval y of the un-fused model) -- computed once, shared."""
    import oracle.nn as onn
    out = {}
    for name, nc in GRAPHS:
        _, g, sd = _build(name, nc)
        img = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(nc)).half().float()
        with torch.no_grad():
            y, _ = onn.forward(g, _dbl(sd), img.double(), training=False)
        out[(name, nc)] = (img, y)
    return out


@pytest.mark.parametrize("fused", [False, True], ids=["eval", "fused"])
@pytest.mark.parametrize("name,nc", GRAPHS, ids=GIDS)
def test_graph_eval_vs_oracle(oracle_eval, name, nc, fused, monkeypatch):
    """Eval and fused-eval y (B, 4 + nc, A).  tests/test_gpu_model.py:43 holds the head outputs of the nc = 6 models to 3e-2 of the
    largest reference value (LD: 5e-2 in L2, an fp16 rounding can move an LDConv sample to the next pixel); the same here."""
    m, g, sd = _build(name, nc)
    if fused:
        m.fuse()
    m.cuda().eval()
    img, ref = oracle_eval[(name, nc)]
    # the inference plan asks Detect for its fused tail (dy_head_infer_levels, issued outside any recorded list): for these class
    # branches the answer must be "no" -- the generic final convs and the decode launch run instead
    from ultralytics.nn.modules import Detect
    asked, tail = [], Detect._infer_tail
    monkeypatch.setattr(Detect, "_infer_tail", lambda self, xs: asked.append(tail(self, xs)) or asked[-1])
    with torch.no_grad():
        y, feats = m(img.cuda())
    det = m.model[-1]
    c3 = det.cv3[0][0].conv.out_channels
    assert asked and all(a is None for a in asked), "Detect took the fused inference tail"
    assert m.rt.eng.L.dy_head_infer_supported(det.cv2[0][2].in_channels, det.cv2[0][2].out_channels, c3, nc) == 0
    assert y.shape == ref.shape == (2, 4 + nc, ref.shape[2])
    e, e2 = relerr(y.float().cpu(), ref), l2err(y.float().cpu(), ref)
    ec = relerr(y[:, 4:].float().cpu(), ref[:, 4:])
    print(f"{name} nc={nc} {'fused' if fused else 'eval'}: y relerr {e:.2e} l2err {e2:.2e}; class scores alone relerr {ec:.2e}")
    assert torch.isfinite(y).all()
    assert (e2 < 5e-2) if "LD" in name else (e < 3e-2 and ec < 3e-2)
    assert m.state_dict()["model.%d.cv3.0.0.conv.weight" % (len(m.model) - 1)].shape[0] == max(m.model[-1].cv3[0][0].conv.in_channels, min(nc, 100))


@pytest.mark.parametrize("name,nc", GRAPHS, ids=GIDS)
def test_graph_training_step_vs_oracle_and_graph_replay(golden, name, nc):
    """Loss items of one training step against the float64 oracle at tests/test_gpu_model.py:50 (1.2e-2 per item) and :51 (5e-3 on
    the loss); then one step captured into hipGraphs equals the eager (launch-list) step bit for bit and changes the weights; and the
    head's fall-back is the one recorded: no dy_cls_head_* launch (test_graph_eval_vs_oracle shows the inference tail's)."""
    import oracle.loss as ol
    import oracle.nn as onn
    from golden.cases import synth_batch
    from ultralytics.hip.train import StepPlan
    batch = synth_batch(50 + nc, 2, 4, nc)
    if "LD" in name:
        # LD: the state seed and the batch tests/test_gpu_model.py steps this graph on (class ids 0..5)
        G = golden("models")
        batch = {k: G.t(f"{name}/{k}") for k in ("img", "batch_idx", "cls", "bboxes")}
    else:
        batch["img"] = batch["img"].half().float()
    res = []
    for use_graph in (False, True):
        m, g, sd = _build(name, nc)
        m.cuda().train()
        # (LD: a static loss scale of 1.  The class loss grows with nc -- 3.8e3 here against 9.4e2 at nc = 6 -- and at a scale of 1024
        # the fp16 gradients reaching the first LDConv's offset conv overflow; the dynamic scale of a real run backs off the same way.)
        plan = StepPlan(m, 2, 64, nmax=8, init_scale=1.0 if "LD" in name else 1024.0, use_graph=use_graph)
        plan.set_hyper([0.01] * 3, 0.9, [0.0, 5e-4, 0.0])
        w0 = plan.rt.flat_p.clone()
        plan.forward_backward(batch)   # traced
        plan.forward_backward(batch)   # replayed (use_graph: from the captured graphs)
        plan.optimizer_step()
        torch.cuda.synchronize()
        names = [o[2] for o in plan.rec_fb.ops if o[0] is not None]
        assert not any(n.startswith("dy_cls_head") for n in names), "the stand-alone class-conv kernels ran"
        c3 = m.model[-1].cv3[0][0].conv.out_channels  # max(ch[0], min(nc, 100)): 37, 100, 40
        assert any(n == "dy_bn_act_apply_c" for n in names) == (c3 % 8 != 0), c3
        assert "dy_bn_finalize_ld" in names
        assert torch.isfinite(plan.rt.flat_g).all() and float(plan.state[2]) == 0.0
        assert not torch.equal(plan.rt.flat_p, w0), "the step did not move the weights"
        res.append((plan.crit.scalars[5:9].clone(), plan.rt.flat_g.clone(), plan.rt.flat_p.clone()))
    if "LD" in name:  # LDConv's far-sample scatter adds with fp32 atomics (tests/test_gpu_model.py:162): not bit-stable run to run
        assert relerr(res[0][0], res[1][0]) < 1e-6 and relerr(res[0][1], res[1][1]) < 1e-4
    else:
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    with torch.no_grad():
        _, g, sd = _build(name, nc)
        # (LD keeps the fixture's fp32 image: LDConv floors its sampling coordinates, and rounding the image to fp16 beforehand moves the
        # ORACLE's class item by 1.5 % at nc = 6 already -- 513.75 against the 521.41 of tests/golden/models.npz -- while the engine stays
        # at 521.20; tests/test_gpu_model.py feeds this graph the same way)
        feats = onn.forward(g, _dbl(sd), batch["img"].double(), training=True)
        ref_loss, ref_items = ol.detection_loss([f.float() for f in feats], batch, g.strides, g.nc)
    items = res[0][0][:3].cpu()
    per_item = float(((items - ref_items).abs() / ref_items.abs()).max())
    print(f"{name} nc={nc}: items {items.tolist()} oracle {ref_items.tolist()} worst {per_item:.2e}")
    assert per_item < 1.2e-2
    assert abs(float(res[0][0][3]) - float(ref_loss)) < 5e-3 * float(ref_loss)


@pytest.mark.parametrize("name,nc", GRAPHS[:3], ids=GIDS[:3])
def test_freeze_prunes_as_at_nc6(name, nc):
    """freeze=10: the frozen prefix leaves nothing on the tape -- freezing layers 0..9 takes exactly as many launches off the recorded
    step at this class count as it takes off the nc = 6 step of the same graph (those layers do not depend on nc), and the frozen
    parameters' gradients are exactly zero.  (A static loss scale of 1: the class loss grows with the class count, and what a scale of
    1024 overflows in fp16 -- LD's first offset conv at nc = 40, this batch at nc = 120 -- is the dynamic scale's business, not this test's.)"""
    from golden.cases import synth_batch
    from ultralytics.hip.train import StepPlan
    counts = {}
    for c in (6, nc):
        for freeze in (0, 10):
            m, g, _ = _build(name, c)
            for k, v in m.named_parameters():
                v.requires_grad = not (any(k.startswith(f"model.{i}.") for i in range(freeze)) or ".dfl" in k)
            m.cuda().train()
            plan = StepPlan(m, 2, 64, nmax=8, init_scale=1.0)
            plan.forward_backward(synth_batch(3, 2, 4, c))
            torch.cuda.synchronize()
            frozen = torch.cat([p.grad.flatten() for k, p in m.named_parameters() if not p.requires_grad])
            assert float(frozen.abs().max()) == 0.0 and torch.isfinite(plan.rt.flat_g).all()
            trainable = torch.cat([p.grad.flatten() for k, p in m.named_parameters() if p.requires_grad])
            assert float(trainable.abs().max()) > 0.0
            counts[(c, freeze)] = len([o for o in plan.rec_fb.ops if o[0] is not None])
    print(name, counts)
    assert counts[(nc, 0)] - counts[(nc, 10)] == counts[(6, 0)] - counts[(6, 10)] > 0


@pytest.mark.parametrize("name,nc", GRAPHS[:3], ids=GIDS[:3])
def test_augment_and_tiled_predict_run(name, nc):
    from ultralytics.utils.ops import non_max_suppression
    m, g, sd = _build(name, nc)
    m.cuda().eval()
    x = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(2)).cuda()
    with torch.no_grad():
        y, _ = m(x, augment=True)
    assert y.shape[1] == 4 + nc and torch.isfinite(y).all()
    dets = non_max_suppression(y, 0.001, 0.7, nc=nc)[0]
    assert dets.shape[1] == 6 and (dets.numel() == 0 or int(dets[:, 5].max()) < nc)
    import numpy as np
    from ultralytics.utils.tiled import tiled_predict
    frame = np.random.default_rng(1).integers(0, 255, (100, 150, 3), dtype=np.uint8)
    boxes = tiled_predict([frame], m, tile=64, conf=0.001)[0]
    assert boxes.shape[-1] == 6 and torch.isfinite(boxes).all() and (boxes.numel() == 0 or int(boxes[:, 5].max()) < nc)


# ------------------------------------------------------------------------------------------------------------------ public API
def test_train_val_predict_with_37_classes(tmp_path):
    """YOLO(...).train on a synthetic 37-class dataset end to end: results.csv and last.pt are written; last.pt reloads, predicts and
    validates with a 37 x 37 (+ background) confusion matrix."""
    import numpy as np
    from PIL import Image
    from ultralytics import YOLO
    rng = np.random.default_rng(0)
    for split, n in (("train", 8), ("val", 4)):
        (tmp_path / "images" / split).mkdir(parents=True)
        (tmp_path / "labels" / split).mkdir(parents=True)
        for i in range(n):
            Image.fromarray(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8)).save(tmp_path / "images" / split / f"{i}.jpg")
            rows = [f"{(7 * i + 5 * j) % 37} {rng.uniform(0.3, 0.7):.4f} {rng.uniform(0.3, 0.7):.4f} {rng.uniform(0.1, 0.4):.4f} {rng.uniform(0.1, 0.4):.4f}"
                    for j in range(3)]
            (tmp_path / "labels" / split / f"{i}.txt").write_text("\n".join(rows) + "\n")
    data = tmp_path / "data37.yaml"
    data.write_text(f"path: {tmp_path}\ntrain: images/train\nval: images/val\nnc: 37\nnames:\n" + "".join(f"  {i}: c{i}\n" for i in range(37)))
    model = YOLO("yolov8n-ASF-P2P2.yaml")
    model.train(data=str(data), epochs=2, imgsz=64, batch=4, val_period=1, project=str(tmp_path / "runs"), name="t", workers=0, amp=False)
    run = tmp_path / "runs" / "t"
    assert (run / "results.csv").is_file() and (run / "weights" / "last.pt").is_file()
    again = YOLO(str(run / "weights" / "last.pt"))
    sd = again.model.state_dict()
    last = len(again.model.model) - 1
    assert tuple(sd[f"model.{last}.cv3.0.0.conv.weight"].shape) == (37, 32, 3, 3) and tuple(sd[f"model.{last}.cv3.0.2.weight"].shape) == (37, 37, 1, 1)
    res = again.predict(str(tmp_path / "images" / "val" / "0.jpg"), imgsz=64, conf=0.001)
    assert len(res) == 1 and (len(res[0].boxes) == 0 or int(res[0].boxes.cls.max()) < 37)
    frame = rng.integers(0, 255, (100, 150, 3), dtype=np.uint8)
    res = again.predict([frame], tile=64, conf=0.001)
    assert len(res) == 1 and (len(res[0].boxes) == 0 or int(res[0].boxes.cls.max()) < 37)
    metrics = again.val(data=str(data), imgsz=64, batch=4)
    assert "metrics/mAP50(B)" in metrics
    assert tuple(np.asarray(again.validator.confusion_matrix.matrix).shape) == (38, 38)


# ----------------------------------------------------------------------------------------------------------------- interchange
def test_reference_written_nc37_checkpoint_runs(golden):
    """attempt_load_weights of tests/golden/ref_ckpt_nc37.pt (written by the reference's classes, nc = 37: a 37-wide class branch on
    every level; tests/golden/make_any_nc_golden.py says why it is not scale n): the eval forward is the reference's at the bound
    tests/test_gpu_spd.py::test_reference_spd_checkpoint_runs holds ref_ckpt_spd.pt to (2e-2 on boxes and on class scores) and EQUALS
    that of a natively built model with the same fp16-rounded state, as tests/test_gpu_model.py:277 holds ref_ckpt.pt to."""
    from copy import deepcopy
    from conftest import ROOT
    from ultralytics.nn.tasks import DetectionModel, attempt_load_weights, torch_safe_load
    G = golden("any_nc")
    path = os.path.join(ROOT, "tests", "golden", "ref_ckpt_nc37.pt")
    a = attempt_load_weights(path, device="cuda:0")
    cfg = deepcopy(torch_safe_load(path)[0]["model"].yaml)
    assert cfg["nc"] == 37 and a.model[-1].cv3[0][0].conv.out_channels == 37
    b = DetectionModel(cfg, ch=3, verbose=False)
    g = og.build_graph(deepcopy(cfg))
    sd = og.fill_state(og.state_layout(g), int(G["ckpt/seed"]))
    b.load_state_dict({k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
    b.cuda().eval()
    x = G.t("ckpt/img").cuda()
    with torch.no_grad():
        ya, _ = a(x)
        yb, _ = b(x)
    assert torch.equal(ya, yb)
    ref = G.t("ckpt/y_eval")
    eb, ec = relerr(ya[:, :4].cpu(), ref[:, :4]), relerr(ya[:, 4:].cpu(), ref[:, 4:])
    print(f"nc = 37 checkpoint eval: box relerr {eb:.2e} cls relerr {ec:.2e}")
    assert eb < 2e-2 and ec < 2e-2
