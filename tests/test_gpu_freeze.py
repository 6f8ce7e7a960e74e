"""Training with ``freeze=...`` on the HIP path: the trainer applies the reference's rule (engine/trainer.py:662-682), the step plan
traces under the flags it finds and leaves the frozen layers' backward work out, frozen parameters neither move nor enter the clip
norm.  DEAL-YOLO-N at 64x64, batch 2, against tests/golden/freeze.npz (tests/golden/make_freeze_golden.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import CFG_DIR, ROOT
from gpu_util import relerr
from oracle import graph as og

pytestmark = pytest.mark.gpu

NAME = "yolov8n-ASF-P2P2"
CASES = {"8": 8, "5": 5, "l2": [2], "l12_20": [12, 20], "l26": [26]}
TENSORS = ("model.0.conv.weight", "model.12.cv1.conv.weight", "model.26.cv3.0.2.bias")


def _model(freeze="default"):
    """The filled model on the GPU; ``freeze`` other than "default": the trainer's rule applied to its flags."""
    from ultralytics.engine.trainer import frozen_parameter_names
    from ultralytics.nn.tasks import DetectionModel
    m = DetectionModel(os.path.join(CFG_DIR, NAME + ".yaml"), ch=3, verbose=False)
    g = og.build_graph(og.load_yaml(os.path.join(CFG_DIR, NAME + ".yaml")))
    m.load_state_dict(og.fill_state(og.state_layout(g), 11), strict=True)
    if freeze != "default":
        frozen = set(frozen_parameter_names([k for k, _ in m.named_parameters()], freeze))
        for k, v in m.named_parameters():
            v.requires_grad = k not in frozen
    return m.cuda().train(), g


def _batch(g, ni=0):
    from golden.cases import synth_batch
    return synth_batch(900 + ni, 2, 4, g.nc)


def _slices(rt, m, trainable):
    return [(n, rt.param_off[n], p.numel()) for n, p in m.named_parameters() if p.requires_grad == trainable]


@pytest.fixture(scope="module")
def unfrozen():
    """The flat gradient and the recorded call names of one step with nothing frozen but the DFL (computed once, never changed)."""
    from ultralytics.hip.train import StepPlan
    m, g = _model(None)
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.forward_backward(_batch(g))
    torch.cuda.synchronize()
    return dict(g=plan.rt.flat_g.clone(), off=dict(plan.rt.param_off), names=[op[2] for op in plan.rec_fb.ops], split=plan.fb_split,
                reductions=len({id(sp) for sp in plan.wgrad_specs}))


@pytest.mark.parametrize("tag", list(CASES))
def test_trainer_trace_vs_golden(golden, tag):
    """Three iterations of DetectionTrainer(overrides=dict(freeze=...)) against the reference's trace, at the bounds of
    tests/test_gpu_model.py::test_optimizer_trace_vs_golden: loss 1e-2, gradient norm 5e-2, abs-sum of the state 2e-4, final
    tensors 2e-2.  Frozen parameters keep their bits, a frozen layer's BatchNorm running mean moves (training-mode statistics).
    Before the trainer read ``freeze`` the 8-layer case failed here: gradient norm 2512 against 1251, model.0.conv.weight moving."""
    from ultralytics.engine.trainer import DetectionTrainer
    G = golden("freeze")
    m, g = _model()
    start = {k: v.detach().clone() for k, v in m.state_dict().items()}
    tr = DetectionTrainer(m, overrides=dict(freeze=CASES[tag], optimizer="SGD", hipgraph=False, loss_scale=1024.0, nmax=8))
    tr.setup(8, 2, 64)
    frozen = [str(n) for n in G[f"{tag}/frozen_names"]]
    assert [k for k, p in m.named_parameters() if not p.requires_grad] == frozen
    ref = G[f"{tag}/trace"]
    plan = tr.plan
    for ni in range(3):
        row = ref[ni]
        tr.train_step(_batch(g, ni), ni, 0)
        loss, _ = plan.loss_items()
        print(tag, ni, loss, row[0], float(plan.state[3]), row[4], row[5])
        assert abs(loss - row[0]) < 1e-2 * row[0]
        assert (tr.last_opt_step == ni) == bool(row[5])
        if row[5]:
            assert abs(float(plan.state[3]) - row[4]) < 5e-2 * row[4], "grad norm"
        fl = torch.cat([plan.rt.flat_p, plan.rt.flat_b]).double().abs().sum()
        assert abs(float(fl) - row[10]) < 2e-4 * row[10], "abs-sum of the state after the step"
    sd = m.state_dict()
    for t in TENSORS:
        assert relerr(sd[t], G.t(f"{tag}/final/{t}")) < 2e-2, t
    for k in frozen:
        assert torch.equal(sd[k], start[k]), f"frozen parameter {k} moved"
    pnames = {k for k, _ in m.named_parameters()}
    moved = [k for k in sd if k in pnames and k not in frozen and not torch.equal(sd[k], start[k])]
    assert len(moved) > 100
    bn = next(k[:-len(".weight")] for k in frozen if k.endswith(".bn.weight"))  # a frozen layer's BatchNorm keeps training-mode statistics
    assert not torch.equal(sd[bn + ".running_mean"], start[bn + ".running_mean"]), bn
    fr = plan.rt.frozen.bool()
    assert float(plan.rt.flat_g[fr].abs().max()) == 0.0


@pytest.mark.parametrize("tag", ["8", "l12_20", "5"])
def test_frozen_plan_gives_the_unfrozen_plans_gradients(unfrozen, tag):
    """The flat gradient slices of the trainable parameters from a frozen plan EQUAL those of the unfrozen plan on the same batch (the
    frozen layers' forward is unchanged and their input gradients have the bits of the trainable launches); the frozen slices are
    exactly zero.  A replay repeats the trace bit for bit -- for freeze=5 that is the concatenation / ScalSeq with members that need
    no gradient beside members that do."""
    from ultralytics.hip.train import StepPlan
    m, g = _model(CASES[tag])
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    batch = _batch(g)
    plan.forward_backward(batch)
    torch.cuda.synchronize()
    got, rt = plan.rt.flat_g.clone(), plan.rt
    assert rt.param_off == unfrozen["off"]
    assert torch.isfinite(got).all()
    diff = [(n, relerr(got[o:o + k], unfrozen["g"][o:o + k])) for n, o, k in _slices(rt, m, True) if not torch.equal(got[o:o + k], unfrozen["g"][o:o + k])]
    bad, worst = [n for n, _ in diff], max([e for _, e in diff], default=0.0)
    print(tag, "trainable slices that differ:", len(bad), bad[:6], f"worst {worst:.3e}")
    assert not bad, (bad[:6], worst)
    for n, o, k in _slices(rt, m, False):
        assert float(got[o:o + k].abs().max()) == 0.0, n
    assert sum(float(got[o:o + k].abs().max()) > 0 for n, o, k in _slices(rt, m, True)) > 100
    plan.forward_backward(batch)  # replay
    torch.cuda.synchronize()
    assert torch.equal(plan.rt.flat_g, got), f"replay differs from the trace by {float((plan.rt.flat_g - got).abs().max()):.3e}"


def _spec_ptrs(sp):
    ts = [sp.weight, sp.wpack, sp.wpack_t, sp.coef, sp.acc_b, sp.acc_f, sp.gweight, sp.gbn_w, sp.gbn_b]
    return {t.data_ptr() for t in ts if t is not None}


def test_frozen_prefix_leaves_no_backward_launch(unfrozen):
    """freeze=8: behind the loss no recorded launch names a buffer of a layer-0..7 convolution, and the weight-gradient reductions
    (reduce descriptors + launches that reduce at once) are those of the trainable convolutions, one set each.  With nothing frozen
    the trainer's plan records the same call names in the same order as a plan built without the argument."""
    from ultralytics.engine.trainer import DetectionTrainer
    from ultralytics.hip.train import StepPlan
    m, g = _model(8)
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    plan.forward_backward(_batch(g))
    rt = plan.rt
    prefix = [rt.specs[id(mod)] for i in range(8) for mod in m.model[i].modules() if id(mod) in rt.specs]
    assert len(prefix) >= 10 and not any(sp.trainable for sp in prefix)
    ptrs = set().union(*[_spec_ptrs(sp) for sp in prefix])
    back = plan.rec_fb.ops[plan.fb_split:]
    assert len(back) > 50
    for fn, args, name, _sid in back:
        hit = [a for a in args if isinstance(a, int) and a in ptrs]
        assert not hit, f"{name} after the loss touches a frozen layer's buffer"
    assert plan.fb_split == unfrozen["split"] and [op[2] for op in plan.rec_fb.ops[:plan.fb_split]] == unfrozen["names"][:plan.fb_split]  # the forward did not change
    assert len(back) <= len(unfrozen["names"]) - plan.fb_split - 2 * len(prefix)  # (the unfrozen list holds >= 2 backward launches per such layer)
    trainable = {id(sp) for sp in rt.specs.values() if sp.trainable}
    logged = {id(sp) for sp in plan.wgrad_specs}
    print(len(prefix), "frozen prefix convs;", len(trainable), "trainable convs;", len(logged), "weight-gradient reductions;", unfrozen["reductions"], "unfrozen")
    assert logged <= trainable and len(logged) > 30  # no frozen layer has a weight-gradient launch or a reduce descriptor ...
    assert len(logged) == unfrozen["reductions"] - len(prefix)  # ... and every trainable one kept its own
    # nothing frozen: the trainer's rule leaves the plan as it was
    m2, g2 = _model()
    tr = DetectionTrainer(m2, overrides=dict(optimizer="SGD", hipgraph=False, loss_scale=1024.0, nmax=8))
    tr.setup(8, 2, 64)
    tr.train_step(_batch(g2), 0, 0)
    assert [op[2] for op in tr.plan.rec_fb.ops] == unfrozen["names"]


def test_one_captured_replay_of_a_frozen_step():
    """hipGraph: the freeze=8 step is captured, passes the capture check without a retry and replays."""
    from ultralytics.hip.train import StepPlan
    m, g = _model(8)
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0, use_graph=True)
    batch = _batch(g)
    plan.forward_backward(batch)
    assert plan.graph_fb is not None and plan.capture_retries == 0
    torch.cuda.synchronize()
    want = plan.rt.flat_g.clone()
    plan.forward_backward(batch)
    torch.cuda.synchronize()
    assert torch.equal(plan.rt.flat_g, want) and plan.capture_retries == 0
    fr = plan.rt.frozen.bool()
    assert float(plan.rt.flat_g[fr].abs().max()) == 0.0 and float(plan.rt.flat_g.abs().max()) > 0


def test_flags_changed_after_the_trace_raise():
    """A launch list traced under one set of requires_grad flags refuses to run under another, naming the first parameter that
    differs (a host-side comparison); a new plan traces under the new flags."""
    from ultralytics.hip.train import StepPlan
    m, g = _model(8)
    plan = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0)
    batch = _batch(g)
    plan.forward_backward(batch)
    p = dict(m.named_parameters())
    p["model.3.conv.weight"].requires_grad = True
    p["model.5.conv.weight"].requires_grad = True
    with pytest.raises(RuntimeError, match=r"requires_grad of 'model\.3\.conv\.weight' is True now but was False"):
        plan.forward_backward(batch)
    with pytest.raises(RuntimeError, match="model.3.conv.weight"):
        plan.forward_only(batch)
    plan2 = StepPlan(m, 2, 64, nmax=8, init_scale=1024.0, share=plan)
    plan2.forward_backward(batch)
    torch.cuda.synchronize()
    rt = plan2.rt
    o, k = rt.param_off["model.3.conv.weight"], p["model.3.conv.weight"].numel()
    assert float(rt.flat_g[o:o + k].abs().max()) > 0
    o, k = rt.param_off["model.3.bn.weight"], p["model.3.bn.weight"].numel()
    assert float(rt.flat_g[o:o + k].abs().max()) == 0.0


@pytest.mark.parametrize("n_frozen", [8, 6])
def test_frozen_backbone_with_two_gradient_buckets(tmp_path, n_frozen):
    """A one-rank RCCL group told world_size = 2 (tests/test_gpu_dp.py::test_rccl_runs_the_collective_path_on_the_gpu): with
    DY_DP_BUCKETS=2 the step equals the one-bucket step bit for bit.  freeze=8 is this model's whole backbone -- the second bucket has
    no backward launch, the plan falls back to one exchange -- freeze=6 leaves the second half two layers (the worker asserts which)."""
    port = 29500 + (os.getpid() + 13 + 5 * n_frozen) % 2000
    res = {}
    for buckets in (1, 2):
        out = tmp_path / str(buckets)
        out.mkdir()
        env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port + buckets),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", DY_DP_BUCKETS=str(buckets), DY_TEST_FREEZE=str(n_frozen))
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "freeze_dp_worker.py"), str(out)], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=240)
        assert p.returncode == 0, p.stdout[-3000:]
        res[buckets] = torch.load(os.path.join(out, "rank0.pt"))
    for k in ("p", "b", "ema"):
        assert torch.equal(res[1][k], res[2][k]), k
