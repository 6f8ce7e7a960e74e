"""Generate tests/golden/slimneck.npz and tests/golden/ref_ckpt_slimneck.pt from the REFERENCE implementation: GSConv, GSBottleneck
and VoVGSCSP (reference nn/extra_modules/block.py:886-967) on their own and inside this package's yolov8-ASF-P2P2-SlimNeck graph.

Run in the build container only (needs the reference tree, which ``_refimport`` locates):

    python tests/golden/make_slimneck_golden.py

State: ``oracle.graph.fill_state`` over the layout read off the reference module's own ``state_dict()`` (the oracle does not know
the modules and is not extended); the tests call the same function over the stored ``keys`` / ``shapes`` / ``seed``, so no weights
are stored.  The shuffle kernels need no fixture: tests/slimneck_ref.py restates them where the tests run.

slimneck.npz
  ``mod/<case>/``: the reference module in train mode, fp32, N = 2: ``y``, ``gx``, ``gp/<name>`` (parameter gradients; a parameter
  whose ``.grad`` stayed None -- VoVGSCSP's ``res`` -- is listed in ``mod/<case>/nograd`` instead), ``buf/<name>`` (running statistics
  after the one forward) for ``x = rnd(10 seed)`` and ``gy = rnd(10 seed + 1)`` (tests/golden/cases.py), and the state's ``keys`` /
  ``shapes`` / ``seed``.
  ``tol/<case>/<tensor>``: measured here, not derived: the relative Frobenius error, against those fp32 values, of a float64 copy of
  the reference module with the HIP path's storage points: x, gy, gx, every convolution's raw output and its gradient, every SiLU
  output, the output of every Conv without activation and GSBottleneck's sum rounded to fp16, the dense convolutions' weights rounded
  to fp16 (their MFMA packs; the depthwise kernels read the fp32 masters).  The shuffle is a permutation and stores nothing new.
  ``tol/<case>/buf/<name>``: the same copy's running statistics after the one forward against the reference's, by the tests' relerr.
  ``tol/<case>/abs/gp/<name>``: for a gradient that is zero in exact arithmetic (ZERO_GRADS), the emulation's largest absolute value;
  ``mod/<case>/ref_abs/gp/<name>``: the reference's.  ``tol/<model>/run_{mean,var}_sum``: the per-layer sums of the running statistics
  after the training step, the emulated graph's against the reference's, by relerr.
  ``<model>/fresh_*``: the buffers of a freshly built reference model (names, minimum and maximum of each BatchNorm2d buffer), the
  ``res`` ones among them; ``<model>/n_params``, ``keys`` / ``shapes``: the parameter count and state-dict layout the reference builds
  from this package's YAML; ``<model>/unused``: the parameters whose ``.grad`` is None after the backward pass.
  ``batch/``, ``<model>/``, ``ckpt/``, ``tol/<model>/...``, ``tol/ckpt/...``: as tests/golden/make_adown_golden.py stores them (eval,
  fused eval, augmented eval, one training step, the change of every tensor over one clipped SGD-nesterov step), measured with the
  same storage points over the whole graph.  ``<model>/grad/<name>``: the gradients of the GSConv rows' four convolution weights in
  full; ``tol/<model>/grad/<name>``: their measured l2err.
  Asserted here of the reference: over one SGD step with weight decay every ``res.*`` parameter has ``.grad`` None and keeps its bits.
ref_ckpt_slimneck.pt: the reference's on-disk layout (engine/trainer.py:898-923) of the graph at scale ``t = [0.17, 0.25, 128]`` written
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
import torch.nn as nn  # noqa: E402
import yaml  # noqa: E402

import _refimport  # noqa: E402

_refimport.install()

from ultralytics.cfg import get_cfg  # noqa: E402
from ultralytics.nn.extra_modules import block as RB  # noqa: E402
from ultralytics.nn.tasks import DetectionModel  # noqa: E402
from ultralytics.utils import DEFAULT_CFG  # noqa: E402
from ultralytics.utils.torch_utils import initialize_weights  # noqa: E402

from cases import rnd, synth_batch  # noqa: E402
import slimneck_ref as R  # noqa: E402
import slimneck_util as U  # noqa: E402

GSConv, VoVGSCSP = RB.GSConv, RB.VoVGSCSP
assert GSConv.__module__ == "ultralytics.nn.extra_modules.block" and sys.modules[GSConv.__module__].__file__.startswith(_refimport.REF)
OUR_CFG = os.path.join(ROOT, "experiment-yolo_amd", "ultralytics", "cfg", "models")
YAML = "yolov8-ASF-P2P2-SlimNeck.yaml"
torch.set_num_threads(8)

MODULE_SEEDS = {"gs_16_32_k3s2": 820, "gs_32_16_k1": 821, "vov_32_32": 822}
MODEL_SEED, BATCH_SEED, CKPT_SEED, CKPT_SCALE = 76, 60, 77, ("t", [0.17, 0.25, 128])
# gradients that are exactly zero in exact arithmetic (a per-channel constant in front of a 1x1 Conv + training-mode BatchNorm): the
# reference's fp32 value is rounding noise, so a RELATIVE tolerance says nothing; the emulation's largest |value| is stored instead
ZERO_GRADS = {"vov_32_32": ("gsb.0.shortcut.bn.bias",)}
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


def check_shuffle():
    """The restatement the tests use IS the reference's reshape / permute form (n = 16 and n = 48)."""
    for n in (16, 48):
        x2 = torch.arange(2 * n * 3 * 5, dtype=torch.float64).reshape(2, n, 3, 5)
        want = R.reference_form(x2)
        got = R.forward(x2[:, :n // 2].permute(0, 2, 3, 1), x2[:, n // 2:].permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
        assert torch.equal(got, want) and torch.equal(want, torch.cat((x2[:, 0::2], x2[:, 1::2]), 1))


def attach_storage(e, fused=False):
    """The HIP path's fp16 storage points as hooks on ``e``, a float64 copy of a reference module or model: every convolution's raw
    output (``fused``: a folded Conv stores its activation only), every SiLU / LeakyReLU output, the output of a Conv without
    activation, every sum (Bottleneck's shortcut, GSBottleneck's, Add, ScalSeq's tail), the image as the stem stages it; the weights of
    the dense convolutions rounded to fp16 (their MFMA packs; depthwise kernels read the fp32 masters); Detect's final convolutions'
    logits left in fp32 with an fp16 gradient at the loss scale.  GSConv's shuffle and VoVGSCSP's concatenation move stored values."""
    det = e.model[-1] if hasattr(e, "model") and type(e.model[-1]).__name__ == "Detect" else None
    keep32, dfl = set(), None
    if det is not None:
        keep32 = {id(seq[-1]) for seq in list(det.cv2) + list(det.cv3)} | {id(det.dfl.conv)}
        dfl = id(det.dfl.conv)
    hook = lambda mod, inp, out: r16(out)  # noqa: E731
    sums = ("Bottleneck", "GSBottleneck", "Add", "ScalSeq")
    for mod in e.modules():
        if isinstance(mod, (nn.SiLU, nn.LeakyReLU)):
            mod.inplace = False
            mod.register_forward_hook(hook)
        elif isinstance(mod, (nn.Conv2d, nn.Conv3d)):
            if mod.groups == 1 and id(mod) != dfl:
                mod.weight.data = mod.weight.data.half().double()
            if id(mod) not in keep32:
                if not fused or isinstance(mod, nn.Conv3d):  # (a folded Conv adds its bias and applies SiLU in the convolution's launch)
                    mod.register_forward_hook(hook)
            elif id(mod) != dfl:
                mod.register_forward_hook(lambda mod, inp, out: GradRound16.apply(out))  # fp32 logits, fp16 gradient
        elif type(mod).__name__ in sums:
            mod.register_forward_hook(hook)
        elif type(mod).__name__ == "Conv" and isinstance(getattr(mod, "act", None), nn.Identity):
            mod.register_forward_hook(hook)  # BatchNorm's (or the folded bias's) output is what is stored
    if det is not None:
        e.model[0].register_forward_pre_hook(lambda mod, inp: (r16(inp[0]),))
    return e


def build_module(name):
    cls, args, H, W = U.MODULE_CASES[name]
    torch.manual_seed(0)
    m = getattr(RB, cls)(*args)
    initialize_weights(m)  # BN eps / momentum as DetectionModel.__init__ sets them
    return m, args[0], H, W


def gen_modules(arrs):
    from copy import deepcopy
    for name in U.MODULE_CASES:
        seed = MODULE_SEEDS[name]
        m, c1, H, W = build_module(name)
        layout = layout_of(m)
        sd = U.fill_state(layout, seed)
        m.load_state_dict(sd, strict=True)
        e = attach_storage(deepcopy(m).double().train())
        m.train()
        x = rnd(10 * seed, U.BATCH, c1, H, W).requires_grad_(True)
        y = m(x)
        gy = rnd(10 * seed + 1, *y.shape)
        y.backward(gy)
        p = f"mod/{name}"
        put_layout(arrs, p, layout, seed)
        arrs[f"{p}/y"], arrs[f"{p}/gx"] = y.detach(), x.grad
        nograd = [n for n, q in m.named_parameters() if q.grad is None]
        assert all(".res." in "." + n or n.startswith("res.") for n in nograd) and (bool(nograd) == (U.MODULE_CASES[name][0] == "VoVGSCSP"))
        arrs[f"{p}/nograd"] = np.array(nograd if nograd else [""])
        for n, q in m.named_parameters():
            if q.grad is not None:
                arrs[f"{p}/gp/{n}"] = q.grad
        for n, b in m.named_buffers():
            if "running" in n:
                arrs[f"{p}/buf/{n}"] = b.clone()
        xe = x.detach().half().double().requires_grad_(True)
        ye = e(xe)
        ye.backward(gy.half().double())
        eg = {n: q.grad for n, q in e.named_parameters()}
        tol = dict(y=l2err(ye.detach(), y.detach()), gx=l2err(xe.grad.half().double(), x.grad))
        for n, q in m.named_parameters():
            if q.grad is not None:
                tol[f"gp/{n}"] = l2err(eg[n], q.grad)
        ebuf = dict(e.named_buffers())
        for n, b in m.named_buffers():  # the running statistics after the one forward, by the tests' relerr
            if "running" in n:
                tol[f"buf/{n}"] = relerr(ebuf[n], b)
        for n in ZERO_GRADS.get(name, ()):  # a gradient that is zero in exact arithmetic: the size of the emulation's rounding noise
            arrs[f"tol/{name}/abs/gp/{n}"] = np.float64(eg[n].abs().max())
            arrs[f"mod/{name}/ref_abs/gp/{n}"] = np.float64(dict(m.named_parameters())[n].grad.abs().max())
        for n, v in tol.items():
            arrs[f"tol/{name}/{n}"] = np.float64(v)
        print(name, tuple(y.shape), "tol", {n: f"{v:.2e}" for n, v in tol.items()})


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
    return loss.detach(), items.detach(), {k: q.grad for k, q in e.named_parameters() if q.grad is not None}, e.state_dict()


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


def assert_res_is_dead(m, batch):
    """The reference over one optimizer step with weight decay and momentum: every ``res.*`` parameter has ``.grad`` None and keeps
    its bits; every ``res.*`` buffer too."""
    from copy import deepcopy
    e = deepcopy(m).train()
    before = {k: v.clone() for k, v in e.state_dict().items()}
    opt = torch.optim.SGD(e.parameters(), lr=0.01, momentum=0.9, nesterov=True, weight_decay=5e-4)
    loss, _ = e(batch)
    loss.backward()
    opt.step()
    after = e.state_dict()
    res = [k for k in before if ".res." in k]
    assert len(res) == 6 * len(U.VOV_LAYERS), res
    for k in res:
        assert torch.equal(before[k], after[k]), k
    assert all((q.grad is None) == (".res." in n) for n, q in e.named_parameters() if ".dfl" not in n)
    moved = [k for k in before if ".res." not in k and before[k].is_floating_point() and not torch.equal(before[k], after[k])]
    assert len(moved) > 100


def gen_model(arrs):
    batch = synth_batch(BATCH_SEED, 2, 4, 6)
    for k in ("img", "batch_idx", "cls", "bboxes"):
        arrs[f"batch/{k}"] = batch[k]
    name = U.MODEL
    torch.manual_seed(0)
    m = DetectionModel(os.path.join(OUR_CFG, name + ".yaml"), ch=3, verbose=False)
    m.args = get_cfg(DEFAULT_CFG)
    layout = layout_of(m)
    assert m.yaml["nc"] == 6
    assert [type(m.model[i]) for i in U.VOV_LAYERS] == [VoVGSCSP] * 4 and [type(m.model[i]) for i in U.GS_LAYERS] == [GSConv] * 2
    assert [(m.model[i].cv1.conv.in_channels, m.model[i].cv3.conv.out_channels) for i in U.VOV_LAYERS] == list(U.VOV_WIDTHS.values())
    assert [(m.model[i].cv1.conv.in_channels, 2 * m.model[i].cv1.conv.out_channels) for i in U.GS_LAYERS] == list(U.GS_WIDTHS.values())
    assert all(len(m.model[i].gsb) == 1 for i in U.VOV_LAYERS)
    put_layout(arrs, name, layout, MODEL_SEED)
    arrs[f"{name}/n_params"] = np.int64(sum(q.numel() for q in m.parameters()))
    arrs[f"{name}/stride"] = m.stride
    # the buffers of the freshly built model (the stride probe ran every BatchNorm that a forward reaches, once)
    fresh = [(k, v) for k, v in m.state_dict().items() if ("running_" in k or "num_batches" in k) and not k.startswith("model.24.bn.")]
    arrs[f"{name}/fresh_names"] = np.array([k for k, _ in fresh])
    arrs[f"{name}/fresh_min"] = np.array([float(v.min()) for _, v in fresh])
    arrs[f"{name}/fresh_max"] = np.array([float(v.max()) for _, v in fresh])
    sdf = m.state_dict()
    for i in U.VOV_LAYERS:
        assert float(sdf[f"model.{i}.res.bn.running_var"].min()) == 1.0 and float(sdf[f"model.{i}.res.bn.running_mean"].abs().max()) == 0.0
        assert int(sdf[f"model.{i}.res.bn.num_batches_tracked"]) == 0 and int(sdf[f"model.{i}.cv1.bn.num_batches_tracked"]) == 1
    m.load_state_dict(U.fill_state(layout, MODEL_SEED), strict=True)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    assert_res_is_dead(m, batch)
    m.train()
    loss, items = m(batch)
    loss.backward()
    arrs[f"{name}/loss"], arrs[f"{name}/items"] = loss.detach(), items
    gn = {k: q.grad for k, q in m.named_parameters() if q.grad is not None}
    unused = [k for k, q in m.named_parameters() if q.grad is None and ".dfl" not in k]
    assert unused == [f"model.{i}.res.{s}" for i in U.VOV_LAYERS for s in ("conv.weight", "bn.weight", "bn.bias")], unused
    arrs[f"{name}/unused"] = np.array(unused)
    arrs[f"{name}/grad_names"] = np.array(list(gn))
    arrs[f"{name}/grad_l2"] = torch.stack([v.norm() for v in gn.values()])
    arrs[f"{name}/grad_sum"] = torch.stack([v.sum() for v in gn.values()])
    arrs[f"{name}/grad_first"] = gn[next(iter(gn))].clone()  # (the clip below scales the gradients in place)
    eloss, eitems, eg, esd = emulate_graph(m, sd0, batch)
    for i in U.GS_LAYERS:  # the gradients of the GSConv rows' convolution weights in full: a norm does not see a wrong direction
        for cv in ("cv1", "cv2"):
            k = f"model.{i}.{cv}.conv.weight"
            arrs[f"{name}/grad/{k}"] = gn[k].clone()
            arrs[f"tol/{name}/grad/{k}"] = np.float64(l2err(eg[k], gn[k]))
    print(name, "tol grad/", {k.split("tol/" + name + "/grad/")[1]: f"{float(v):.2e}" for k, v in arrs.items() if k.startswith(f"tol/{name}/grad/")})
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
    arrs[f"tol/{name}/run_mean_sum"] = np.float64(relerr(torch.stack([esd[k].sum() for k in rm]), arrs[f"{name}/run_mean_sum"]))
    arrs[f"tol/{name}/run_var_sum"] = np.float64(relerr(torch.stack([esd[k.replace("mean", "var")].sum() for k in rm]), arrs[f"{name}/run_var_sum"]))
    print(name, "tol run_mean_sum / run_var_sum", f"{float(arrs[f'tol/{name}/run_mean_sum']):.2e} {float(arrs[f'tol/{name}/run_var_sum']):.2e}")
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
        assert all(m.model[i].res.conv.bias is not None and not hasattr(m.model[i].res, "bn") for i in U.VOV_LAYERS)  # fuse() folds res too
        assert m.model[18].cv2.conv.bias is not None and not hasattr(m.model[18].cv2, "bn")
        arrs[f"{name}/y_eval_fused"] = m(batch["img"])[0]
        put_eval_tol(arrs, f"{name}/y_eval_fused", e_fused, arrs[f"{name}/y_eval_fused"])
    print(name, int(arrs[f"{name}/n_params"]), m.stride.tolist(), "loss", float(loss), "items", items.tolist())


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
    path = os.path.join(HERE, "ref_ckpt_slimneck.pt")
    torch.save(ckpt, path)
    assert os.path.getsize(path) < 1 << 20
    # what the checkpoint's (fp16-rounded) state computes in fp32, as a loader of either side runs it
    m.load_state_dict({k: (v.half().float() if v.is_floating_point() else v) for k, v in m.state_dict().items()})
    m.eval()
    img = synth_batch(BATCH_SEED, 2, 4, 6)["img"]
    put_layout(arrs, "ckpt", layout, CKPT_SEED)
    arrs["ckpt/vov_channels"] = np.array([m.model[i].cv3.conv.out_channels for i in U.VOV_LAYERS])
    arrs["ckpt/n_params"] = np.int64(sum(q.numel() for q in m.parameters()))
    with torch.no_grad():
        arrs["ckpt/y_eval"] = m(img)[0]
    put_eval_tol(arrs, "ckpt/y_eval", emulate_eval(m, img), arrs["ckpt/y_eval"])
    print(f"ref_ckpt_slimneck.pt  {os.path.getsize(path) / 1024:.1f} KiB, {sum(q.numel() for q in m.parameters())} parameters, VoVGSCSP widths {arrs['ckpt/vov_channels'].tolist()}")


def main():
    arrs = {}
    check_shuffle()
    gen_modules(arrs)
    gen_model(arrs)
    gen_ckpt(arrs)
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(HERE, "slimneck.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, os.path.getsize(path)
    print(f"slimneck.npz  {os.path.getsize(path) / 1024:.1f} KiB  ({len(out)} arrays)")


if __name__ == "__main__":
    main()
