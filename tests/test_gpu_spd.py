"""-m gpu: SPDConv (space-to-depth convolution, reference nn/extra_modules/block.py:2497-2507) on the HIP path.

The permutation kernel (csrc/spd.hip) bit for bit against torch indexing, channel slices and refusals included; the five SPD
convolution shapes through the existing convolution kernels; the module and the two SPD graphs against the reference
(tests/golden/spd.npz, tests/golden/make_spd_golden.py) at the bounds their non-SPD twins are held to; the recorded plans (InferPlan,
StepPlan + hipGraph) against the walked launches; freeze=4; a reference-written SPD checkpoint; test-time augmentation; and two epochs
through the public trainer."""
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

from conftest import CFG_DIR
from gpu_util import l2err, relerr, run_fwd_bwd
from spd_util import CKPT, MODELS, MODULE_CASES, SPD_LAYERS, batch, layout, module_grad, state

pytestmark = pytest.mark.gpu
ASF, LD = MODELS
DY_ERR_ARG, DY_ERR_ALIGN = -1, -3  # include/dealyolo_hip.h
POISON = -1234.0  # exactly representable in fp16


# ----------------------------------------------------------------------------- 1. the kernel
def _s2d(t):
    """(N, H, W, C) -> (N, H/2, W/2, 4C) in the reference's order: cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2],
    x[..., 1::2, 1::2]], 1) written for NHWC."""
    return torch.cat([t[:, ::2, ::2], t[:, 1::2, ::2], t[:, ::2, 1::2], t[:, 1::2, 1::2]], -1)


def _d2s(t, C):
    """The inverse: (N, H/2, W/2, 4C) -> (N, H, W, C)."""
    N, h, w, _ = t.shape
    out = torch.empty(N, 2 * h, 2 * w, C, dtype=t.dtype, device=t.device)
    out[:, ::2, ::2], out[:, 1::2, ::2], out[:, ::2, 1::2], out[:, 1::2, 1::2] = t.split(C, -1)
    return out


def _launch(x, cx, y, cy, N, H, W, C, backward=0, accumulate=0):
    from ultralytics.hip import lib
    return lib().dy_space_to_depth(x.data_ptr() + 2 * cx, x.shape[-1], y.data_ptr() + 2 * cy, y.shape[-1], N, H, W, C, backward, accumulate,
                                   torch.cuda.current_stream().cuda_stream)


# (N, H, W, C, channels of x's storage, first channel in it, channels of y's storage, first channel in it)
KERNEL_CASES = [(1, 2, 2, 8, 8, 0, 32, 0), (2, 6, 10, 16, 16, 0, 64, 0), (3, 4, 4, 24, 24, 0, 96, 0), (1, 34, 66, 64, 64, 0, 256, 0),
                (2, 10, 6, 40, 64, 16, 4 * 40 + 16, 8)]


@pytest.mark.parametrize("N,H,W,C,ldx,cx,ldy,cy", KERNEL_CASES)
def test_permutation_kernel_bit_for_bit(N, H, W, C, ldx, cx, ldy, cy):
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + C)

    def storage(h, w, ld, c0, c):
        t = torch.full((N, h, w, ld), POISON, dtype=torch.float16)
        t[..., c0:c0 + c] = torch.randn(N, h, w, c, generator=g).half()
        return t.cuda()

    def outside_untouched(t, c0, c):
        return bool((t[..., :c0] == POISON).all()) and bool((t[..., c0 + c:] == POISON).all())

    # forward
    x, y = storage(H, W, ldx, cx, C), storage(H // 2, W // 2, ldy, cy, 4 * C)
    x0 = x.clone()
    assert _launch(x, cx, y, cy, N, H, W, C) == 0
    torch.cuda.synchronize()
    assert torch.equal(y[..., cy:cy + 4 * C], _s2d(x0[..., cx:cx + C])) and outside_untouched(y, cy, 4 * C) and torch.equal(x, x0)
    # backward, store: dX <- permuted dY
    dy, dx = storage(H // 2, W // 2, ldy, cy, 4 * C), storage(H, W, ldx, cx, C)
    dy0 = dy.clone()
    assert _launch(dx, cx, dy, cy, N, H, W, C, 1, 0) == 0
    torch.cuda.synchronize()
    perm = _d2s(dy0[..., cy:cy + 4 * C], C)
    assert torch.equal(dx[..., cx:cx + C], perm) and outside_untouched(dx, cx, C) and torch.equal(dy, dy0)
    # backward, accumulate onto a non-zero gradient: one fp16 addition per element
    dx = storage(H, W, ldx, cx, C)
    prev = dx[..., cx:cx + C].clone()
    assert _launch(dx, cx, dy, cy, N, H, W, C, 1, 1) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx[..., cx:cx + C], (prev.float() + perm.float()).half()) and outside_untouched(dx, cx, C) and torch.equal(dy, dy0)
    # the permutation and its backward are inverses
    assert torch.equal(_d2s(_s2d(x0[..., cx:cx + C]), C), x0[..., cx:cx + C])


def test_refusals_launch_nothing():
    x = torch.full((1, 8, 8, 16), POISON, dtype=torch.float16, device="cuda")
    y = torch.full((1, 4, 4, 64), POISON, dtype=torch.float16, device="cuda")
    for backward in (0, 1):
        assert _launch(x, 0, y, 0, 1, 7, 8, 16, backward) == DY_ERR_ARG      # odd H
        assert _launch(x, 0, y, 0, 1, 8, 5, 16, backward) == DY_ERR_ARG      # odd W
        assert _launch(x, 0, y, 0, 1, 1, 8, 16, backward) == DY_ERR_ARG      # below 2
        assert _launch(x, 0, y, 0, 1, 8, 8, 12, backward) == DY_ERR_ALIGN    # C = 12
        assert _launch(x, 4, y, 0, 1, 8, 8, 8, backward) == DY_ERR_ALIGN     # pointer 8 bytes off a 16-byte boundary
    from ultralytics.hip import lib
    s = torch.cuda.current_stream().cuda_stream
    assert lib().dy_space_to_depth(0, 16, y.data_ptr(), 64, 1, 8, 8, 16, 0, 0, s) == DY_ERR_ARG
    assert lib().dy_space_to_depth(x.data_ptr(), 12, y.data_ptr(), 64, 1, 8, 8, 8, 0, 0, s) == DY_ERR_ALIGN
    assert lib().dy_space_to_depth(x.data_ptr(), 16, y.data_ptr(), 60, 1, 8, 8, 8, 0, 0, s) == DY_ERR_ALIGN
    torch.cuda.synchronize()
    assert bool((x == POISON).all()) and bool((y == POISON).all())


def test_engine_op_rejects_an_odd_map():
    from ultralytics.hip.engine import Engine
    eng = Engine(torch.device("cuda", 0))
    with pytest.raises(ValueError, match="7x8"):
        eng.space_to_depth(eng.wrap_act(torch.zeros(1, 7, 8, 16, dtype=torch.float16, device="cuda")))


# ----------------------------------------------------------------------------- 2. the five SPD convolutions on the existing kernels
@pytest.mark.parametrize("cin,cout", [(64, 32), (128, 64), (256, 128), (128, 32), (256, 64)])
def test_spd_convolution_shapes_on_the_existing_conv_path(cin, cout):
    """Forward (fp32 + bias, fp16 + BatchNorm partial sums), input gradient and weight gradient of the 3x3 stride-1 convolution behind
    the permutation, 2 x 6 x 10 maps, against fp32 F.conv2d: the body and the bounds of tests/test_gpu_kernels.py."""
    import test_gpu_kernels as K
    K.test_conv_forward_dgrad_wgrad(cin, cout, 3, 1, 6, 10)


# ----------------------------------------------------------------------------- 3. the module against the reference
TOL_CONV = (3e-3, 6e-3, 4e-3)  # forward, input gradient, parameter gradients: TOL["Conv"] of tests/test_gpu_modules.py


@pytest.mark.parametrize("case", list(MODULE_CASES))
def test_module_vs_golden(golden, case):
    from ultralytics.nn.extra_modules import SPDConv
    G = golden("spd")
    p = f"mod/{case}"
    m = SPDConv(*MODULE_CASES[case])
    m.load_state_dict(state(G, p), strict=True)
    y, gxs, rt = run_fwd_bwd(m, [G.t(f"{p}/x")], G.t(f"{p}/gy"))
    ty, tx, tp = TOL_CONV
    ey, ex = relerr(y, G.t(f"{p}/y")), relerr(gxs[0], G.t(f"{p}/gx"))
    print(f"{case}: forward {ey:.2e} (bound {ty}), input gradient {ex:.2e} (bound {tx})")
    assert ey < ty, "forward"
    assert ex < tx, "grad input"
    for k, q in m.named_parameters():
        ref = module_grad(G, case, k)
        e = relerr(q.grad.reshape(ref.shape), ref)
        print(f"{case}: grad {k} {e:.2e} (bound {tp})")
        assert e < tp, f"grad {k}"
    bufs = dict(m.named_buffers())
    for k in G.keys(f"{p}/buf/"):
        assert relerr(bufs[k.split("/buf/")[1]], G.t(k)) < 2e-3, k


# ----------------------------------------------------------------------------- 4. the two graphs against the reference
def _model(G, name):
    from ultralytics.nn.tasks import DetectionModel
    m = DetectionModel(os.path.join(CFG_DIR, name + ".yaml"), ch=3, verbose=False)
    m.load_state_dict(state(G, name), strict=True)
    return m.cuda()


@pytest.mark.parametrize("name", MODELS)
def test_eval_and_fused_eval_vs_golden(golden, name):
    """Bounds of tests/test_gpu_nms.py / test_gpu_configs.py for the non-SPD graphs (2e-2 on boxes and on class scores); the second
    call of a geometry is the recorded InferPlan and repeats the walked forward bit for bit."""
    G = golden("spd")
    m = _model(G, name).eval()
    x = G.t("batch/img").cuda()
    for key in ("y_eval", "y_eval_fused"):
        if key == "y_eval_fused":
            m.fuse()
        ref = G.t(f"{name}/{key}")
        with torch.no_grad():
            y1, _ = m(x)   # walked
            assert not m._infer_plans["plans"]
            y2, _ = m(x)   # traced into a plan
            plan = m._infer_plans["plans"][(2, 3, 64, 64)]
            y3, _ = m(x)   # replayed
        torch.cuda.synchronize()
        assert sum(1 for o in plan.rec.ops if o[2] == "dy_space_to_depth") == 5
        assert torch.equal(y1, y2) and torch.equal(y1, y3)
        assert y1.shape == ref.shape
        eb, ec = relerr(y1[:, :4].cpu(), ref[:, :4]), relerr(y1[:, 4:].cpu(), ref[:, 4:])
        print(f"{name} {key}: box relerr {eb:.2e} cls relerr {ec:.2e}")
        assert eb < 2e-2 and ec < 2e-2


@pytest.mark.parametrize("name", MODELS)
def test_train_step_vs_golden(golden, name):
    """Loss items, per-parameter gradient norms, the first layer's gradient and the BatchNorm running statistics of one training
    step: the comparisons and bounds of tests/test_gpu_model.py::test_model_step_vs_golden."""
    from ultralytics.hip.train import StepPlan
    G = golden("spd")
    m = _model(G, name).train()
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.forward_backward(batch(G))
    torch.cuda.synchronize()
    ld = "LD" in name
    s = plan.crit.scalars.cpu()
    ref_items = G.t(f"{name}/items")
    per_item = float(((s[5:8] - ref_items).abs() / ref_items.abs()).max())
    print("items", s[5:8].tolist(), ref_items.tolist(), f"worst per-item relative error {per_item:.2e}")
    assert per_item < 1.2e-2
    assert abs(float(s[8]) - float(G[f"{name}/loss"])) < 5e-3 * float(G[f"{name}/loss"])
    names = [str(k) for k in G[f"{name}/grad_names"]]
    params = dict(m.named_parameters())
    assert all(f"model.{i}.conv.conv.weight" in names for i in SPD_LAYERS)
    scale = float(plan.state[0])
    l2 = torch.stack([params[k].grad.float().norm() / scale for k in names]).cpu()
    ref = G.t(f"{name}/grad_l2")
    rel = ((l2 - ref).abs() / (ref.abs() + 1e-3 * ref.abs().max())).numpy()
    print("grad-l2 rel err: median %.2e max %.2e (%s)" % (np.median(rel), rel.max(), names[int(rel.argmax())]))
    assert np.median(rel) < (1e-2 if ld else 4e-3) and rel.max() < (0.2 if ld else 4e-2)
    first = params[names[0]].grad.float().cpu() / scale
    ef = (l2err if ld else relerr)(first, G.t(f"{name}/grad_first"))
    print(f"grad_first err {ef:.3e}")
    assert ef < (0.15 if ld else 5e-2)
    sd = m.state_dict()
    rm = [str(k) for k in G[f"{name}/run_mean_names"]]
    assert relerr(torch.stack([sd[k].sum() for k in rm]).cpu(), G.t(f"{name}/run_mean_sum")) < 5e-3
    assert relerr(torch.stack([sd[k.replace("mean", "var")].sum() for k in rm]).cpu(), G.t(f"{name}/run_var_sum")) < 5e-3
    assert torch.isfinite(plan.rt.flat_g).all() and float(plan.state[2]) == 0.0


@pytest.mark.parametrize("name", MODELS)
def test_captured_step_equals_the_eager_step(golden, name):
    """One StepPlan step replayed as a hipGraph against the eager tape step of another plan on the same state and batch: the same
    launches, so loss items and ALL gradients are EQUAL (LD: LDConv's far-sample scatter adds with fp32 atomics, to their order)."""
    from ultralytics.hip.train import StepPlan
    G = golden("spd")
    outs = []
    for graph in (False, True):
        m = _model(G, name).train()
        plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0, use_graph=graph)
        sd0 = {k: v.clone() for k, v in m.state_dict().items()}
        plan.forward_backward(batch(G))
        if graph:
            assert plan.graph_fb is not None
            m.load_state_dict(sd0)
            plan.forward_backward(batch(G))  # the captured graph's replay
        torch.cuda.synchronize()
        ops = [o for o in plan.rec_fb.ops if o[0] is not None and o[2] == "dy_space_to_depth"]
        assert len(ops) == 10 and sum(1 for o in ops if o[1][8] == 1) == 5  # five layers, forward + backward
        outs.append((plan.rt.flat_g.clone(), plan.crit.scalars.clone()))
    assert torch.isfinite(outs[0][0]).all() and float(outs[0][0].abs().max()) > 0
    if "LD" in name:
        assert relerr(outs[0][1][5:9], outs[1][1][5:9]) < 1e-6 and relerr(outs[0][0], outs[1][0]) < 1e-4
        return
    assert torch.equal(outs[0][1][5:9], outs[1][1][5:9])
    assert torch.equal(outs[0][0], outs[1][0]), f"max diff {float((outs[0][0] - outs[1][0]).abs().max()):.3e}"


# ----------------------------------------------------------------------------- 5. freeze=4
def _spec_ptrs(sp):
    ts = [sp.weight, sp.wpack, sp.wpack_t, sp.coef, sp.acc_b, sp.acc_f, sp.gweight, sp.gbn_w, sp.gbn_b]
    return {t.data_ptr() for t in ts if t is not None}


def test_freeze_4_prunes_the_frozen_spd_layers(golden):
    """Layers 0-3 frozen (two of them SPDConv): their parameters keep their bits through an optimizer step, the recorded backward names
    no buffer of a layer-0..3 convolution -- no weight-gradient launch, no reduction -- and holds the permutation backward of layers
    5, 18 and 21 only: layer 3's input (and layer 1's) needs no gradient, so those two leave nothing on the tape."""
    from ultralytics.engine.trainer import frozen_parameter_names
    from ultralytics.hip.train import StepPlan
    G = golden("spd")
    m = _model(G, ASF).train()
    frozen = set(frozen_parameter_names([k for k, _ in m.named_parameters()], 4))
    assert {f"model.{i}.conv.conv.weight" for i in (1, 3)} <= frozen and "model.5.conv.conv.weight" not in frozen
    for k, v in m.named_parameters():
        v.requires_grad = k not in frozen
    start = {k: v.detach().clone() for k, v in m.state_dict().items()}
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.set_hyper([0.01] * 3, 0.9, [0.0, 5e-4, 0.0])
    plan.forward_backward(batch(G))
    plan.optimizer_step()
    torch.cuda.synchronize()
    rt = plan.rt
    prefix = [rt.specs[id(mod)] for i in range(4) for mod in m.model[i].modules() if id(mod) in rt.specs]
    assert len(prefix) >= 5 and not any(sp.trainable for sp in prefix)
    ptrs = set().union(*[_spec_ptrs(sp) for sp in prefix])
    fwd, back = plan.rec_fb.ops[:plan.fb_split], plan.rec_fb.ops[plan.fb_split:]
    assert [o[1][8] for o in fwd if o[2] == "dy_space_to_depth"] == [0] * 5  # the forward keeps all five permutations
    for fn, args, name, _sid in back:
        hit = [a for a in args if isinstance(a, int) and a in ptrs]
        assert not hit, f"{name} after the loss touches a frozen layer's buffer"
    assert not ({id(sp) for sp in plan.wgrad_specs} & {id(sp) for sp in prefix})
    perm_back = [o for o in back if o[2] == "dy_space_to_depth"]
    assert len(perm_back) == 3 and all(o[1][8] == 1 for o in perm_back), [o[1][4:9] for o in perm_back]
    assert sorted(o[1][7] for o in perm_back) == [32, 64, 64]  # C of the inputs of layers 18, 5 / 21
    sd = m.state_dict()
    for k in frozen:
        assert torch.equal(sd[k], start[k]), f"frozen parameter {k} moved"
    for i in (5, 18, 21):
        assert not torch.equal(sd[f"model.{i}.conv.conv.weight"], start[f"model.{i}.conv.conv.weight"]), i
    assert float(rt.flat_g[rt.frozen.bool()].abs().max()) == 0.0 and torch.isfinite(rt.flat_g).all()
    assert not torch.equal(sd["model.1.conv.bn.running_mean"], start["model.1.conv.bn.running_mean"])  # training-mode statistics


# ----------------------------------------------------------------------------- 6. a reference-written SPD checkpoint
def test_reference_spd_checkpoint_runs(golden):
    """attempt_load_weights of tests/golden/ref_ckpt_spd.pt: the eval forward is the reference's (2e-2, the eval bound above) and
    EQUALS that of a natively built model with the same fp16-rounded state, as tests/test_gpu_model.py holds ref_ckpt.pt to."""
    from ultralytics.nn.tasks import DetectionModel, attempt_load_weights, torch_safe_load
    G = golden("spd")
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


# ----------------------------------------------------------------------------- 7. test-time augmentation
def test_augmented_forward_vs_golden(golden):
    """model(x, augment=True): walked, recorded, replayed; the bound of tests/test_gpu_tta.py (1e-3 on boxes and on class scores)."""
    G = golden("spd")
    m = _model(G, ASF).eval()
    x = G.t("batch/img").cuda()
    want = G.t(f"{ASF}/y_aug")
    ys = []
    for _ in range(3):
        y, second = m(x, augment=True)
        assert second is None and tuple(y.shape) == tuple(want.shape)
        eb, ec = relerr(y[:, :4], want[:, :4]), relerr(y[:, 4:], want[:, 4:])
        print(f"augment: box relerr {eb:.2e}, class relerr {ec:.2e}")
        assert eb <= 1e-3 and ec <= 1e-3
        ys.append(y.clone())
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


# ----------------------------------------------------------------------------- 8. the public trainer
def test_two_epochs_through_the_public_trainer():
    from ultralytics import YOLO
    from ultralytics.data import SyntheticDetection
    torch.manual_seed(0)
    y = YOLO("yolov8n-ASF-P2P2-SPD.yaml")
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
    spd = [k for k, _ in y.trainer.model.named_parameters() if any(k.startswith(f"model.{i}.") for i in SPD_LAYERS)]
    assert len(spd) == 15
    still = [k for k in spd if torch.equal(w1[k].cpu(), w0[k].cpu())]
    assert not still, f"SPDConv parameters that never moved: {still}"
    assert torch.isfinite(plan.rt.flat_g).all()
