"""Generate tests/golden/simam.npz and tests/golden/ref_ckpt_simam.pt from the REFERENCE implementation: SimAM (reference
nn/extra_modules/attention.py:53-77, built by nn/tasks.py:969-970) on its own and inside this package's yolov8-ASF-P2P2-SimAM graph.

Run in the build container only (needs the reference tree, which ``_refimport`` locates):

    python tests/golden/make_simam_golden.py

State: ``tests/simam_util.py::fill_state`` (``oracle.graph.fill_state`` over the layout read off the reference module's own
``state_dict()``); the tests call the same function over the stored ``keys`` / ``shapes`` / ``seed``, so no weights are stored.  The
kernels' own cases are seeds only: tests/simam_ref.py computes their float64 values where the tests run.

simam.npz
  ``mod/<case>/``: the reference module, fp32, N = 2, ``e_lambda`` and the input distribution as tests/simam_util.py::MODULE_CASES
  names them: ``y``, ``gx`` for ``x = offset + spread * rnd(10 seed)`` and ``gy = rnd(10 seed + 9)`` (tests/golden/cases.py).
  ``tol/<case>/<tensor>``: measured here, not derived: the relative Frobenius error, against those fp32 values, of a float64
  emulation of the HIP path's storage (tests/simam_util.py::emulate_module: x, gy, y and gx rounded to fp16).
  ``batch/``, ``<model>/``, ``ckpt/``: as tests/golden/make_bifpn_golden.py stores them (``y_eval``, ``y_aug``, ``y_eval_fused``, ``loss``,
  ``items``, ``grad_names``, ``grad_l2``, ``grad_sum``, ``grad_first``, ``run_mean_*``, ``upd_l2``; ``n_params``, ``stride``, ``state_keys``).
  ``<model>/base_keys_equal``: 1 when the state_dict keys of the reference's base graph (yolov8-ASF-P2P2) with Detect renumbered
  26 -> 29 are this graph's keys.
  ``tol/<model>/{y_eval,y_aug,y_eval_fused}_{box,cls}``, ``tol/ckpt/y_eval_{box,cls}``,
  ``tol/<model>/{items,loss,grad_l2_median,grad_l2_max,grad_first,upd_l2_median,upd_l2_max}``: the same measurement over the whole graph
  (tests/simam_util.py::attach_storage lists the storage points), the figures the tests compare, taken by the tests' formulas.
ref_ckpt_simam.pt: the reference's on-disk layout (engine/trainer.py:898-923) of the graph at scale ``t = [0.17, 0.25, 128]`` written
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
from ultralytics.nn.extra_modules.attention import SimAM  # noqa: E402
from ultralytics.nn.tasks import DetectionModel  # noqa: E402
from ultralytics.utils import DEFAULT_CFG  # noqa: E402

from cases import rnd, synth_batch  # noqa: E402
import simam_util as U  # noqa: E402

assert SimAM.__module__ == "ultralytics.nn.extra_modules.attention" and sys.modules[SimAM.__module__].__file__.startswith(_refimport.REF)
OUR_CFG = os.path.join(ROOT, "experiment-yolo_amd", "ultralytics", "cfg", "models")
YAML = "yolov8-ASF-P2P2-SimAM.yaml"
torch.set_num_threads(8)

MODEL_SEED, BATCH_SEED, CKPT_SEED, CKPT_SCALE = 94, 60, 95, ("t", [0.17, 0.25, 128])
STEP_LR, STEP_MOM = U.STEP_LR, U.STEP_MOM


def l2err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-12))


def relerr(a, b):
    """tests/gpu_util.py::relerr: the largest error over the largest reference value."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def layout_of(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def put_layout(arrs, prefix, layout, seed):
    arrs[f"{prefix}/keys"] = np.array(list(layout))
    arrs[f"{prefix}/shapes"] = np.array([str(s) for s in layout.values()])
    arrs[f"{prefix}/seed"] = np.int32(seed)


def gen_modules(arrs):
    for name, (C, H, W, lam, off, spread) in U.MODULE_CASES.items():
        seed = U.MODULE_SEEDS[name]
        m = SimAM(lam)
        assert not layout_of(m) and not list(m.parameters()) and not list(m.buffers())
        m.train()
        x = (off + spread * rnd(10 * seed, U.BATCH, C, H, W)).requires_grad_(True)
        y = m(x)
        gy = rnd(10 * seed + 9, *y.shape)
        y.backward(gy)
        q = f"mod/{name}"
        arrs[f"{q}/y"], arrs[f"{q}/gx"] = y.detach(), x.grad
        ye, gxe = U.emulate_module(SimAM(lam), x, gy)
        tol = dict(y=l2err(ye, y.detach()), gx=l2err(gxe, x.grad))
        for k, v in tol.items():
            arrs[f"tol/{name}/{k}"] = np.float64(v)
        print(name, tuple(y.shape), repr(m), "tol", {k: f"{v:.2e}" for k, v in tol.items()})


def put_eval_tol(arrs, prefix, got, ref):
    """``tol/<prefix>_box`` / ``_cls``: the relerr of the emulated output's box rows and class rows, as the tests split them."""
    arrs[f"tol/{prefix}_box"], arrs[f"tol/{prefix}_cls"] = np.float64(relerr(got[:, :4], ref[:, :4])), np.float64(relerr(got[:, 4:], ref[:, 4:]))
    print(f"tol/{prefix} box {float(arrs[f'tol/{prefix}_box']):.2e} cls {float(arrs[f'tol/{prefix}_cls']):.2e}")


def gen_model(arrs):
    batch = synth_batch(BATCH_SEED, 2, 4, 6)
    for k in ("img", "batch_idx", "cls", "bboxes"):
        arrs[f"batch/{k}"] = batch[k]
    name = U.MODEL
    torch.manual_seed(0)
    m = DetectionModel(os.path.join(OUR_CFG, name + ".yaml"), ch=3, verbose=False)
    m.args = get_cfg(DEFAULT_CFG)
    layout = layout_of(m)
    assert m.yaml["nc"] == 6 and [type(m.model[i]) for i in U.SIMAM_LAYERS] == [SimAM] * 3
    assert [float(m.model[i].e_lambda) for i in U.SIMAM_LAYERS] == [1e-4] * 3
    base = DetectionModel(os.path.join(OUR_CFG, U.BASE + ".yaml"), ch=3, verbose=False)
    arrs[f"{name}/base_keys_equal"] = np.int32([k.replace("model.26.", "model.29.") for k in base.state_dict()] == list(layout))
    put_layout(arrs, name, layout, MODEL_SEED)
    arrs[f"{name}/n_params"] = np.int64(sum(q.numel() for q in m.parameters()))
    assert int(arrs[f"{name}/n_params"]) == U.N_PARAMS == sum(q.numel() for q in base.parameters())
    arrs[f"{name}/stride"] = m.stride
    arrs[f"{name}/repr"] = np.array([repr(m.model[i]) for i in U.SIMAM_LAYERS])
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
    eloss, eitems, eg = U.emulate_graph(m, sd0, batch)
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
    m.load_state_dict(sd0)
    m.eval()
    put = lambda key, fused=False, augment=False: put_eval_tol(arrs, f"{name}/{key}", U.emulate_eval(m, batch["img"], fused, augment), arrs[f"{name}/{key}"])  # noqa: E731
    with torch.no_grad():
        arrs[f"{name}/y_eval"] = m(batch["img"])[0]
        put("y_eval")
        y, second = m(batch["img"], augment=True)
        assert second is None
        arrs[f"{name}/y_aug"] = y
        put("y_aug", augment=True)
        e_fused = U.emulate_eval(m, batch["img"], fused=True)  # (folds its own copy)
        m.fuse(verbose=False)
        assert m.model[1].conv.bias is not None and not hasattr(m.model[1], "bn") and type(m.model[26]) is SimAM
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
    path = os.path.join(HERE, "ref_ckpt_simam.pt")
    torch.save(ckpt, path)
    assert os.path.getsize(path) < 1 << 20
    # what the checkpoint's (fp16-rounded) state computes in fp32, as a loader of either side runs it
    m.load_state_dict({k: (v.half().float() if v.is_floating_point() else v) for k, v in m.state_dict().items()})
    m.eval()
    img = synth_batch(BATCH_SEED, 2, 4, 6)["img"]
    put_layout(arrs, "ckpt", layout, CKPT_SEED)
    arrs["ckpt/state_keys"] = np.array(list(m.state_dict()))
    arrs["ckpt/n_params"] = np.int64(sum(q.numel() for q in m.parameters()))
    with torch.no_grad():
        arrs["ckpt/y_eval"] = m(img)[0]
    put_eval_tol(arrs, "ckpt/y_eval", U.emulate_eval(m, img), arrs["ckpt/y_eval"])
    print(f"ref_ckpt_simam.pt  {os.path.getsize(path) / 1024:.1f} KiB, {sum(q.numel() for q in m.parameters())} parameters")


def main():
    arrs = {}
    gen_modules(arrs)
    gen_model(arrs)
    gen_ckpt(arrs)
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(HERE, "simam.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, os.path.getsize(path)
    print(f"simam.npz  {os.path.getsize(path) / 1024:.1f} KiB  ({len(out)} arrays)")


if __name__ == "__main__":
    main()
