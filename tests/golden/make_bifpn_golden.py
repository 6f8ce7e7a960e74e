"""Generate tests/golden/bifpn.npz and tests/golden/ref_ckpt_bifpn.pt from the REFERENCE implementation: Fusion in 'bifpn' mode
(reference nn/extra_modules/block.py:453-490, built by nn/tasks.py:922-925) on its own and inside this package's
yolov8-ASF-P2P2-BiFPN graph.

Run in the build container only (needs the reference tree, which ``_refimport`` locates):

    python tests/golden/make_bifpn_golden.py

State: ``tests/bifpn_util.py::fill_state`` (``oracle.graph.fill_state`` over the layout read off the reference module's own
``state_dict()``, every ``fusion_weight`` then positive and unequal); the tests call the same function over the stored ``keys`` /
``shapes`` / ``seed``, so no weights are stored.  The kernels' own cases are seeds only: tests/bifpn_ref.py computes their float64
values where the tests run.

bifpn.npz
  ``mod/<case>/``: the reference module in train mode, fp32, N = 2, ``fusion_weight`` as tests/bifpn_util.py::MODULE_CASES names it:
  ``y``, ``gx<i>``, ``gp`` for ``x<i> = rnd(10 seed + i)`` and ``gy = rnd(10 seed + 9)`` (tests/golden/cases.py).
  ``tol/<case>/<tensor>``: measured here, not derived: the relative Frobenius error, against those fp32 values, of a float64
  emulation of the HIP path's storage -- every x, gy, y and every gx rounded to fp16, the parameter and its gradient left alone.
  ``batch/``, ``<model>/``, ``ckpt/``: as tests/golden/make_adown_golden.py stores them (``y_aug``, ``upd_l2`` included);
  ``<model>/grad/<name>``: the gradients of the three ``fusion_weight`` vectors in full; ``tol/<model>/grad/<name>``: their measured
  l2err; ``<model>/upd/<name>``: the three vectors after the one clipped SGD-nesterov step, ``tol/<model>/upd/<name>`` the measured
  l2err of their CHANGE.
  ``<model>/n_params``, ``<model>/decayed``: the parameter count and the names ending in ``fusion_weight`` in the group that the
  reference's own ``BaseTrainer.build_optimizer`` (engine/trainer.py), called here, gives the weight decay to.
  ``tol/<model>/{y_eval,y_aug,y_eval_fused}_{box,cls}``, ``tol/ckpt/y_eval_{box,cls}``,
  ``tol/<model>/{items,loss,grad_l2_median,grad_l2_max,grad_first,upd_l2_median,upd_l2_max}``: the same measurement over the whole graph:
  the reference's model in float64 with the image, every convolution output, every SiLU / LeakyReLU output and every sum
  (Bottleneck's shortcut, ScalSeq's tail, Fusion) and the gradients that flow back through them rounded to fp16, the convolution
  weights rounded to fp16, Detect's final convolutions' logits left in fp32 with an fp16 gradient at the loss scale, against the fp32
  values: the figures the tests compare, taken by the tests' formulas.
ref_ckpt_bifpn.pt: the reference's on-disk layout (engine/trainer.py:898-923) of the graph at scale ``t = [0.17, 0.25, 128]`` written
  by the reference's classes.  The file is data: tensors, class paths and the YAML dict.
"""
import os
import sys
import warnings

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

os.environ["MKL_CBWR"] = "COMPATIBLE"  # as tests/conftest.py pins it

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

import _refimport  # noqa: E402

_refimport.install()

from ultralytics.cfg import get_cfg  # noqa: E402
from ultralytics.nn.extra_modules.block import Fusion  # noqa: E402
from ultralytics.nn.tasks import DetectionModel  # noqa: E402
from ultralytics.utils import DEFAULT_CFG  # noqa: E402

from cases import rnd, synth_batch  # noqa: E402
import bifpn_util as U  # noqa: E402

assert Fusion.__module__ == "ultralytics.nn.extra_modules.block" and sys.modules[Fusion.__module__].__file__.startswith(_refimport.REF)
OUR_CFG = os.path.join(ROOT, "experiment-yolo_amd", "ultralytics", "cfg", "models")
YAML = "yolov8-ASF-P2P2-BiFPN.yaml"
torch.set_num_threads(8)

MODEL_SEED, BATCH_SEED, CKPT_SEED, CKPT_SCALE = 84, 60, 85, ("t", [0.17, 0.25, 128])
LOSS_SCALE = 1024.0  # the tests' StepPlan(init_scale=...)
STEP_LR, STEP_MOM = U.STEP_LR, U.STEP_MOM


def l2err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-12))


def layout_of(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def put_layout(arrs, prefix, layout, seed):
    arrs[f"{prefix}/keys"] = np.array(list(layout))
    arrs[f"{prefix}/shapes"] = np.array([str(s) for s in layout.values()])
    arrs[f"{prefix}/seed"] = np.int32(seed)


class Round16(torch.autograd.Function):
    """fp16 storage of a float64 value and of the gradient that flows back through it."""

    @staticmethod
    def forward(ctx, t):
        return t.half().double()

    @staticmethod
    def backward(ctx, g):
        return g.half().double()


r16 = Round16.apply


class GradRound16(torch.autograd.Function):
    """An fp32 value whose GRADIENT is stored in fp16 at the step's loss scale (Detect's logits: hip/train.py, init_scale)."""

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return (g * LOSS_SCALE).half().double() / LOSS_SCALE


def gen_modules(arrs):
    for name, (C, H, W, p) in U.MODULE_CASES.items():
        seed, n = U.MODULE_SEEDS[name], len(p)
        m = Fusion([C] * n, "bifpn")
        assert list(layout_of(m)) == ["fusion_weight"] and m.fusion_weight.dtype == torch.float32 and bool((m.fusion_weight == 1).all())
        with torch.no_grad():
            m.fusion_weight.copy_(torch.tensor(p))
        m.train()
        xs = [rnd(10 * seed + i, U.BATCH, C, H, W).requires_grad_(True) for i in range(n)]
        y = m(list(xs))
        gy = rnd(10 * seed + 9, *y.shape)
        y.backward(gy)
        q = f"mod/{name}"
        arrs[f"{q}/y"], arrs[f"{q}/gp"] = y.detach(), m.fusion_weight.grad.clone()
        for i, x in enumerate(xs):
            arrs[f"{q}/gx{i}"] = x.grad
        # the HIP path's storage in float64 arithmetic
        e = Fusion([C] * n, "bifpn").double()
        with torch.no_grad():
            e.fusion_weight.copy_(torch.tensor(p, dtype=torch.float32).double())
        xe = [x.detach().half().double().requires_grad_(True) for x in xs]
        ye = r16(e([r16(t) for t in xe]))
        ye.backward(gy.half().double())
        tol = dict(y=l2err(ye.detach(), y.detach()), gp=l2err(e.fusion_weight.grad, m.fusion_weight.grad))
        for i, x in enumerate(xs):
            tol[f"gx{i}"] = l2err(xe[i].grad, x.grad)
        for k, v in tol.items():
            arrs[f"tol/{name}/{k}"] = np.float64(v)
        print(name, tuple(y.shape), "gp", m.fusion_weight.grad.tolist(), "tol", {k: f"{v:.2e}" for k, v in tol.items()})


def attach_storage(e, fused=False):
    """The HIP path's fp16 storage points as hooks on ``e``, a float64 copy of the reference's model: every convolution's raw output
    (``fused``: a folded Conv stores its activation only), every SiLU / LeakyReLU output, every sum (Bottleneck's shortcut, ScalSeq's
    tail, Fusion), the image as the stem stages it (the scaled images of augment=True too); the weights of the convolutions rounded to
    fp16 (their MFMA packs); Detect's final convolutions' logits left in fp32 with an fp16 gradient at the loss scale."""
    import torch.nn as nn
    det = e.model[-1]
    keep32 = {id(seq[-1]) for seq in list(det.cv2) + list(det.cv3)} | {id(det.dfl.conv)}
    hook = lambda mod, inp, out: r16(out)  # noqa: E731
    sums = ("Bottleneck", "Add", "ScalSeq", "Fusion")  # modules whose output is a sum (or a tail) the HIP path stores in fp16
    for mod in e.modules():
        if isinstance(mod, (nn.SiLU, nn.LeakyReLU)):
            mod.inplace = False
            mod.register_forward_hook(hook)
        elif isinstance(mod, (nn.Conv2d, nn.Conv3d)):
            if mod.groups == 1 and id(mod) != id(det.dfl.conv):
                mod.weight.data = mod.weight.data.half().double()
            if id(mod) not in keep32:
                if not fused or isinstance(mod, nn.Conv3d):  # (a folded Conv adds its bias and applies SiLU in the convolution's launch)
                    mod.register_forward_hook(hook)
            elif id(mod) != id(det.dfl.conv):
                mod.register_forward_hook(lambda mod, inp, out: GradRound16.apply(out))  # fp32 logits, fp16 gradient
        elif type(mod).__name__ in sums:
            mod.register_forward_hook(hook)
    e.model[0].register_forward_pre_hook(lambda mod, inp: (r16(inp[0]),))
    return e


def emulate_graph(m, sd0, batch):
    """One training step of a float64 copy of ``m`` with the HIP path's fp16 storage points -> (loss, items, {name: gradient})."""
    from copy import deepcopy
    e = deepcopy(m)
    e.load_state_dict(sd0)
    attach_storage(e.double().train())
    b64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
    b64["img"] = batch["img"].half().double()  # the stem stages the image as fp16
    loss, items = e(b64)
    loss.backward()
    return loss.detach(), items.detach(), {k: q.grad for k, q in e.named_parameters() if q.grad is not None}


def emulate_eval(m, img, fused=False, augment=False):
    """The eval forward of a float64 copy of ``m`` (its state as it stands; ``fused``: BatchNorm folded in fp32 first, as fuse() folds
    it, then the folded weights rounded to fp16) with the HIP path's fp16 storage points."""
    from copy import deepcopy
    e = deepcopy(m).eval()
    if fused:
        e.fuse(verbose=False)
    attach_storage(e.double(), fused)
    with torch.no_grad():
        return e(img.double(), augment=True)[0] if augment else e(img.double())[0]


def relerr(a, b):
    """tests/gpu_util.py::relerr: the largest error over the largest reference value."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def put_eval_tol(arrs, prefix, got, ref):
    """``tol/<prefix>_box`` / ``_cls``: the relerr of the emulated output's box rows and class rows, as the tests split them."""
    arrs[f"tol/{prefix}_box"], arrs[f"tol/{prefix}_cls"] = np.float64(relerr(got[:, :4], ref[:, :4])), np.float64(relerr(got[:, 4:], ref[:, 4:]))
    print(f"tol/{prefix} box {float(arrs[f'tol/{prefix}_box']):.2e} cls {float(arrs[f'tol/{prefix}_cls']):.2e}")


def decayed_fusion_names(m):
    """The parameters named ``fusion_weight`` that the reference's OWN ``BaseTrainer.build_optimizer`` (engine/trainer.py) puts in
    the group it gives the weight decay to: the optimizer is built on a bare trainer object, as tests/golden/make_golden.py builds
    it, and membership is read off ``optimizer.param_groups`` by tensor identity."""
    from types import SimpleNamespace
    from ultralytics.engine.trainer import BaseTrainer
    decay = 5e-4
    fake = SimpleNamespace(args=m.args, model=m)
    opt = BaseTrainer.build_optimizer(fake, model=m, name="SGD", lr=0.01, momentum=0.9, decay=decay)
    decayed = [pg for pg in opt.param_groups if pg["weight_decay"] == decay]
    others = [pg for pg in opt.param_groups if pg["weight_decay"] != decay]
    assert len(decayed) == 1 and len(others) == 2 and all(pg["weight_decay"] == 0 for pg in others)
    ids = {id(q) for q in decayed[0]["params"]}
    fus = [k for k, q in m.named_parameters() if k.endswith("fusion_weight")]
    assert fus and all(sum(id(dict(m.named_parameters())[k]) == id(q) for pg in opt.param_groups for q in pg["params"]) == 1 for k in fus)
    return [k for k, q in m.named_parameters() if k.endswith("fusion_weight") and id(q) in ids]


def gen_model(arrs):
    batch = synth_batch(BATCH_SEED, 2, 4, 6)
    for k in ("img", "batch_idx", "cls", "bboxes"):
        arrs[f"batch/{k}"] = batch[k]
    name = U.MODEL
    torch.manual_seed(0)
    m = DetectionModel(os.path.join(OUR_CFG, name + ".yaml"), ch=3, verbose=False)
    m.args = get_cfg(DEFAULT_CFG)
    layout = layout_of(m)
    assert m.yaml["nc"] == 6 and m.yaml["fusion_mode"] == "bifpn"
    assert [type(m.model[i]) for i in U.FUSION_LAYERS] == [Fusion] * 3
    assert all(bool((m.model[i].fusion_weight == 1).all()) and tuple(m.model[i].fusion_weight.shape) == (2,) for i in U.FUSION_LAYERS)
    put_layout(arrs, name, layout, MODEL_SEED)
    arrs[f"{name}/n_params"] = np.int64(sum(q.numel() for q in m.parameters()))
    arrs[f"{name}/stride"] = m.stride
    arrs[f"{name}/decayed"] = np.array(decayed_fusion_names(m))
    m.load_state_dict(U.fill_state(layout, MODEL_SEED), strict=True)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()
    loss, items = m(batch)
    loss.backward()
    arrs[f"{name}/loss"], arrs[f"{name}/items"] = loss.detach(), items
    gn = {k: q.grad for k, q in m.named_parameters() if q.grad is not None}
    arrs[f"{name}/grad_names"] = np.array(list(gn))
    arrs[f"{name}/grad_l2"] = torch.stack([v.norm() for v in gn.values()])
    arrs[f"{name}/grad_sum"] = torch.stack([v.sum() for v in gn.values()])
    arrs[f"{name}/grad_first"] = gn[next(iter(gn))].clone()  # (the clip below scales the gradients in place)
    eloss, eitems, eg = emulate_graph(m, sd0, batch)
    for k in U.FUSION_KEYS:  # the three vectors' gradients in full: a norm does not see a wrong direction
        arrs[f"{name}/grad/{k}"] = gn[k].clone()
        arrs[f"tol/{name}/grad/{k}"] = np.float64(l2err(eg[k], gn[k]))
        print(k, "p", sd0[k].tolist(), "grad", gn[k].tolist(), "emulated", eg[k].tolist(), f"tol {float(arrs[f'tol/{name}/grad/{k}']):.2e}")
    ref_l2 = arrs[f"{name}/grad_l2"].double()
    rel = ((torch.stack([eg[k].norm() for k in gn]) - ref_l2).abs() / (ref_l2.abs() + 1e-3 * ref_l2.abs().max())).numpy()
    tol = dict(items=float(((eitems - items.double()).abs() / items.double().abs()).max()), loss=float((eloss - loss.detach().double()).abs() / loss.detach().double().abs()),
               grad_l2_median=float(np.median(rel)), grad_l2_max=float(rel.max()), grad_first=l2err(eg[next(iter(gn))], arrs[f"{name}/grad_first"]))
    for k, v in tol.items():
        arrs[f"tol/{name}/{k}"] = np.float64(v)
    print(name, "tol", {k: f"{v:.2e}" for k, v in tol.items()})
    sdm = m.state_dict()
    rm = [k for k in sdm if k.endswith("running_mean")]
    arrs[f"{name}/run_mean_names"] = np.array(rm)
    arrs[f"{name}/run_mean_sum"] = torch.stack([sdm[k].sum() for k in rm])
    arrs[f"{name}/run_var_sum"] = torch.stack([sdm[k.replace("mean", "var")].sum() for k in rm])
    # the updated parameters: the trainer's clip at 10 (engine/trainer.py:952) and one step of the optimizer build_optimizer makes for
    # 'SGD' (nesterov; no weight decay here), as the L2 norm of every tensor's change; the emulated step's by the same arithmetic
    params = dict(m.named_parameters())
    torch.nn.utils.clip_grad_norm_([params[k] for k in gn], max_norm=10.0)
    torch.optim.SGD([params[k] for k in gn], lr=STEP_LR, momentum=STEP_MOM, nesterov=True).step()
    arrs[f"{name}/upd_l2"] = torch.stack([(params[k].detach() - sd0[k]).norm() for k in gn])
    coef = min(1.0, 10.0 / (float(torch.stack([eg[k].norm() for k in gn]).norm()) + 1e-6))
    ref_u = arrs[f"{name}/upd_l2"].double()
    relu = ((torch.stack([STEP_LR * (1 + STEP_MOM) * coef * eg[k].norm() for k in gn]) - ref_u).abs() / (ref_u.abs() + 1e-3 * ref_u.abs().max())).numpy()
    arrs[f"tol/{name}/upd_l2_median"], arrs[f"tol/{name}/upd_l2_max"] = np.float64(np.median(relu)), np.float64(relu.max())
    print(name, "tol upd_l2 median / max", f"{np.median(relu):.2e} {relu.max():.2e}")
    for k in U.FUSION_KEYS:  # the three vectors after the step, and the measured error of their change
        arrs[f"{name}/upd/{k}"] = params[k].detach().clone()
        arrs[f"tol/{name}/upd/{k}"] = np.float64(l2err(-STEP_LR * (1 + STEP_MOM) * coef * eg[k], params[k].detach().double() - sd0[k].double()))
    m.load_state_dict(sd0)
    m.eval()
    put = lambda key, fused=False, augment=False: put_eval_tol(arrs, f"{name}/{key}", emulate_eval(m, batch["img"], fused, augment), arrs[f"{name}/{key}"])  # noqa: E731
    with torch.no_grad():
        arrs[f"{name}/y_eval"] = m(batch["img"])[0]
        put("y_eval")
        y, second = m(batch["img"], augment=True)
        assert second is None
        arrs[f"{name}/y_aug"] = y
        put("y_aug", augment=True)
        e_fused = emulate_eval(m, batch["img"], fused=True)  # (folds its own copy)
        m.fuse(verbose=False)
        assert m.model[1].conv.bias is not None and not hasattr(m.model[1], "bn") and m.model[11].fusion_weight.dtype == torch.float32
        arrs[f"{name}/y_eval_fused"] = m(batch["img"])[0]
        put_eval_tol(arrs, f"{name}/y_eval_fused", e_fused, arrs[f"{name}/y_eval_fused"])
    print(name, int(arrs[f"{name}/n_params"]), m.stride.tolist(), "loss", float(loss), "items", items.tolist(), "decayed", arrs[f"{name}/decayed"].tolist())


def gen_ckpt(arrs):
    from copy import deepcopy
    d = yaml.safe_load(open(os.path.join(OUR_CFG, YAML)))
    d["scales"][CKPT_SCALE[0]] = CKPT_SCALE[1]
    d["scale"] = CKPT_SCALE[0]
    torch.manual_seed(0)
    m = DetectionModel(d, ch=3, verbose=False)
    layout = layout_of(m)
    m.load_state_dict(U.fill_state(layout, CKPT_SEED), strict=True)
    m.args = dict(get_cfg(DEFAULT_CFG).__dict__)
    ckpt = {"epoch": 3, "best_fitness": 0.25, "model": deepcopy(m).half(), "ema": None, "updates": 57, "optimizer": None,
            "train_args": {"imgsz": 640, "batch": 64, "model": YAML}, "date": "2026-01-01T00:00:00", "version": "8.1.9"}
    path = os.path.join(HERE, "ref_ckpt_bifpn.pt")
    torch.save(ckpt, path)
    assert os.path.getsize(path) < 1 << 20
    # what the checkpoint's (fp16-rounded) state computes in fp32, as a loader of either side runs it
    m.load_state_dict({k: (v.half().float() if v.is_floating_point() else v) for k, v in m.state_dict().items()})
    m.eval()
    img = synth_batch(BATCH_SEED, 2, 4, 6)["img"]
    put_layout(arrs, "ckpt", layout, CKPT_SEED)
    arrs["ckpt/state_keys"] = np.array(list(m.state_dict()))
    arrs["ckpt/fusion_channels"] = np.array([m.model[i - 1].conv.out_channels if i != 25 else m.model[17].cv2.conv.out_channels for i in U.FUSION_LAYERS])
    with torch.no_grad():
        arrs["ckpt/y_eval"] = m(img)[0]
    put_eval_tol(arrs, "ckpt/y_eval", emulate_eval(m, img), arrs["ckpt/y_eval"])
    print(f"ref_ckpt_bifpn.pt  {os.path.getsize(path) / 1024:.1f} KiB, {sum(q.numel() for q in m.parameters())} parameters")


def main():
    arrs = {}
    gen_modules(arrs)
    gen_model(arrs)
    gen_ckpt(arrs)
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(HERE, "bifpn.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, os.path.getsize(path)
    print(f"bifpn.npz  {os.path.getsize(path) / 1024:.1f} KiB  ({len(out)} arrays)")


if __name__ == "__main__":
    main()
