"""Generate tests/golden/carafe.npz, tests/golden/carafe_kernel.npz, tests/golden/carafe_big_*.npz and tests/golden/ref_ckpt_carafe.pt
from the REFERENCE implementation: CARAFE (content-aware up-sampling, reference nn/extra_modules/block.py:3898-3936) on its own and
inside this package's yolov8-ASF-P2P2-CARAFE graph.

Run in the build container only (needs the reference tree, which ``_refimport`` locates):

    python tests/golden/make_carafe_golden.py

State: ``oracle.graph.fill_state`` over the layout read off the reference module's own ``state_dict()`` (the oracle does not know
CARAFE and is not extended); the tests call the same function over the stored ``keys`` / ``shapes`` / ``seed``, so no weights are stored.

carafe_kernel.npz (float64)
  ``ker/<case>/``: the reassembly alone through the reference's own lines -- ``pix_shf``, ``torch.softmax``, ``upsmp``, ``unfold``,
  the ``einsum`` -- and autograd, on ``carafe_util.kernel_inputs(C, H, W, seed, gain)`` (only ``seed`` is stored): ``y``, ``dx``,
  ``dlogits``, NHWC.  The magnitudes of the per-element bounds are not stored: tests/carafe_ref.py returns them beside the values
  that tests/test_host_carafe.py ties to these at 1e-11.
carafe.npz
  ``mod/<case>/``: the reference CARAFE(C, k_enc, 5, c_mid, 2) in train mode, fp32, N = 2: ``y``, ``gx``, ``gp/<name>`` (parameter
  gradients), ``buf/<name>`` (running statistics after the one forward) for ``x = rnd(10 seed)`` and ``gy = rnd(10 seed + 1)``
  (tests/golden/cases.py), and the state's ``keys`` / ``shapes`` / ``seed``.
  ``tol/<case>/<tensor>``: measured here, not derived: the relative Frobenius error, against those fp32 values, of a float64
  emulation of the HIP path's storage -- x, the convolution weights, gy, comp's output, the logits, y, dlogits and both writes of gx
  rounded to fp16 (tests/carafe_ref.py does the reassembly arithmetic).
  ``batch/``, ``<model>/``, ``ckpt/``: as tests/golden/make_spd_golden.py stores them (``y_aug`` included).
carafe_big_*.npz: the arrays of the 24 x 20 cases in pieces (``key@lo:hi`` of the flattened array, ``key@shape``), so that no fixture
  file exceeds 1 MiB.
ref_ckpt_carafe.pt: the reference's on-disk layout (engine/trainer.py:898-923) of the graph at scale ``t = [0.17, 0.125, 256]``
  written by the reference's classes, as ref_ckpt_spd.pt was; its two layers see 32 and 16 channels there.  The file is data:
  tensors, class paths and the YAML dict.
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
import torch.nn.functional as F  # noqa: E402
import yaml  # noqa: E402

import _refimport  # noqa: E402

_refimport.install()

from ultralytics.cfg import get_cfg  # noqa: E402
from ultralytics.nn.extra_modules.block import CARAFE  # noqa: E402
from ultralytics.nn.tasks import DetectionModel  # noqa: E402
from ultralytics.utils import DEFAULT_CFG  # noqa: E402
from ultralytics.utils.torch_utils import initialize_weights  # noqa: E402

from cases import rnd, synth_batch  # noqa: E402
import carafe_ref as R  # noqa: E402
import carafe_util as U  # noqa: E402

assert CARAFE.__module__ == "ultralytics.nn.extra_modules.block" and sys.modules[CARAFE.__module__].__file__.startswith(_refimport.REF)
OUR_CFG = os.path.join(ROOT, "experiment-yolo_amd", "ultralytics", "cfg", "models")
torch.set_num_threads(8)

MODULE_SEEDS = {"cf_32_64_k3": 600, "cf_64_16_k3": 601, "cf_32_16_k1_big": 602}
KERNEL_SEEDS = {"k_8": 700, "k_32": 701, "k_64": 702, "k_64_big": 703, "k_32_hot": 704, "k_8_wide": 705, "k_72": 706}
MODEL_SEED, BATCH_SEED, CKPT_SEED, CKPT_SCALE = 51, 60, 53, ("t", [0.17, 0.125, 256])
PIECE = 100000  # elements of a float64 piece of a big array (0.8 MB)
BN_EPS = 1e-3   # initialize_weights


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
    """fp16 storage of a float64 value; ``both``: the gradient that flows back through it is stored in fp16 too."""

    @staticmethod
    def forward(ctx, t, both):
        ctx.both = both
        return t.half().double()

    @staticmethod
    def backward(ctx, g):
        return (g.half().double() if ctx.both else g), None


def r16(t, both=False):
    return Round16.apply(t, both)


def emulate(x, gy, sd, k_enc):
    """The HIP path's storage in float64 arithmetic -> y, gx (NCHW) and the parameter gradients by state_dict name."""
    P = {k: v.double().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}
    xa = x.half().double().requires_grad_(True)  # the reassembly's reading of x
    xb = x.half().double().requires_grad_(True)  # comp's

    def conv_bn(t, name, k, act):
        z = F.conv2d(t, r16(P[f"{name}.conv.weight"]), None, 1, k // 2)
        z = F.batch_norm(z, None, None, P[f"{name}.bn.weight"], P[f"{name}.bn.bias"], True, 0.0, BN_EPS)
        return F.silu(z) if act else z

    c = r16(conv_bn(xb, "comp", 1, True))
    lg = r16(conv_bn(c, "enc", k_enc, False), both=True)
    y = r16(R.forward(R.nhwc(xa), R.nhwc(lg))["y"])
    y.backward(R.nhwc(gy.half().double()))
    gx = ((xa.grad.half().double() + xb.grad).half().double())
    return R.nchw(y.detach()), gx, {k: v.grad for k, v in P.items()}


def gen_modules(arrs, big):
    for name, (C, c_mid, k_enc, H, W) in U.MODULE_CASES.items():
        seed = MODULE_SEEDS[name]
        dst = big if name.endswith(U.BIG) else arrs
        torch.manual_seed(0)
        m = CARAFE(C, k_enc, 5, c_mid, 2)
        initialize_weights(m)  # BN eps / momentum as DetectionModel.__init__ sets them
        layout = layout_of(m)
        assert [k for k in layout if "num_batches" not in k] == [f"{c}.{k}" for c in ("comp", "enc") for k in
                                                                 ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")], list(layout)
        sd = U.carafe_state(layout, seed)
        m.load_state_dict(sd, strict=True)
        m.train()
        x = rnd(10 * seed, U.BATCH, C, H, W).requires_grad_(True)
        y = m(x)
        gy = rnd(10 * seed + 1, *y.shape)
        y.backward(gy)
        p = f"mod/{name}"
        put_layout(arrs, p, layout, seed)
        dst[f"{p}/y"], dst[f"{p}/gx"] = y.detach(), x.grad
        for k, q in m.named_parameters():
            arrs[f"{p}/gp/{k}"] = q.grad
        for k, b in m.named_buffers():
            if "running" in k:
                arrs[f"{p}/buf/{k}"] = b.clone()
        ey, ex, eg = emulate(x.detach(), gy, sd, k_enc)
        tol = dict(y=l2err(ey, y.detach()), gx=l2err(ex, x.grad))
        for k, q in m.named_parameters():
            tol[f"gp/{k}"] = l2err(eg[k], q.grad)
        for k, v in tol.items():
            arrs[f"tol/{name}/{k}"] = np.float64(v)
        print(name, tuple(y.shape), "tol", {k: f"{v:.2e}" for k, v in tol.items()})


def gen_kernels(arrs, big):
    m = CARAFE(8).double()  # pix_shf, upsmp and unfold carry no state and do not depend on c
    for name, (C, H, W, gain) in U.KERNEL_CASES.items():
        seed = KERNEL_SEEDS[name]
        p = f"ker/{name}"
        arrs[f"{p}/seed"] = np.int32(seed)
        x, lg, dy = U.kernel_inputs(C, H, W, seed, gain)
        dst = big if name.endswith(U.BIG) else arrs
        xd = R.nchw(x.double()).requires_grad_(True)
        ld = R.nchw(lg.double()).requires_grad_(True)
        b, c, h, w = xd.shape
        Wt = torch.softmax(m.pix_shf(ld), dim=1)              # reference :3928-3929
        X = m.unfold(m.upsmp(xd)).view(b, c, -1, 2 * h, 2 * w)  # :3931-3933
        y = torch.einsum("bkhw,bckhw->bchw", [Wt, X])         # :3935
        y.backward(R.nchw(dy.double()))
        dst[f"{p}/y"], dst[f"{p}/dx"], dst[f"{p}/dlogits"] = R.nhwc(y.detach()), R.nhwc(xd.grad), R.nhwc(ld.grad)
        fw, bw = R.forward(x, lg), R.backward(x, lg, dy)
        errs = [float((fw["y"] - dst[f"{p}/y"]).abs().max()), float((bw["dx"] - dst[f"{p}/dx"]).abs().max()),
                float((bw["dlogits"] - dst[f"{p}/dlogits"]).abs().max())]
        print(name, f"max |logit| {float(lg.abs().max()):.1f} largest weight {float(R.weights(lg).max()):.6f} restatement max abs err", errs)


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
    put_layout(arrs, name, layout, MODEL_SEED)
    arrs[f"{name}/n_params"] = np.int64(sum(q.numel() for q in m.parameters()))
    arrs[f"{name}/stride"] = m.stride
    m.load_state_dict(U.carafe_state(layout, MODEL_SEED), strict=True)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()
    loss, items = m(batch)
    loss.backward()
    arrs[f"{name}/loss"], arrs[f"{name}/items"] = loss.detach(), items
    gn = {k: q.grad for k, q in m.named_parameters() if q.grad is not None}
    arrs[f"{name}/grad_names"] = np.array(list(gn))
    arrs[f"{name}/grad_l2"] = torch.stack([v.norm() for v in gn.values()])
    arrs[f"{name}/grad_sum"] = torch.stack([v.sum() for v in gn.values()])
    arrs[f"{name}/grad_first"] = gn[next(iter(gn))]
    sdm = m.state_dict()
    rm = [k for k in sdm if k.endswith("running_mean")]
    arrs[f"{name}/run_mean_names"] = np.array(rm)
    arrs[f"{name}/run_mean_sum"] = torch.stack([sdm[k].sum() for k in rm])
    arrs[f"{name}/run_var_sum"] = torch.stack([sdm[k.replace("mean", "var")].sum() for k in rm])
    m.load_state_dict(sd0)
    m.eval()
    with torch.no_grad():
        arrs[f"{name}/y_eval"] = m(batch["img"])[0]
        y, second = m(batch["img"], augment=True)
        assert second is None
        arrs[f"{name}/y_aug"] = y
        m.fuse(verbose=False)
        arrs[f"{name}/y_eval_fused"] = m(batch["img"])[0]
    print(name, int(arrs[f"{name}/n_params"]), m.stride.tolist(), "loss", float(loss), "items", items.tolist())
    # the parameter count of the module's defaults (CARAFE []: c_mid 64) on the same graph, for the record
    d = yaml.safe_load(open(os.path.join(OUR_CFG, "yolov8-ASF-P2P2-CARAFE.yaml")))
    d["scale"] = "n"
    for row in d["head"]:
        if row[2] == "CARAFE":
            row[3] = []
    arrs[f"{name}/n_params_default_args"] = np.int64(sum(q.numel() for q in DetectionModel(d, ch=3, verbose=False).parameters()))
    print("CARAFE []:", int(arrs[f"{name}/n_params_default_args"]), "parameters")


def gen_ckpt(arrs):
    from copy import deepcopy
    d = yaml.safe_load(open(os.path.join(OUR_CFG, "yolov8-ASF-P2P2-CARAFE.yaml")))
    d["scales"][CKPT_SCALE[0]] = CKPT_SCALE[1]
    d["scale"] = CKPT_SCALE[0]
    torch.manual_seed(0)
    m = DetectionModel(d, ch=3, verbose=False)
    layout = layout_of(m)
    m.load_state_dict(U.carafe_state(layout, CKPT_SEED), strict=True)
    m.args = dict(get_cfg(DEFAULT_CFG).__dict__)
    ckpt = {"epoch": 3, "best_fitness": 0.25, "model": deepcopy(m).half(), "ema": None, "updates": 57, "optimizer": None,
            "train_args": {"imgsz": 640, "batch": 64, "model": "yolov8-ASF-P2P2-CARAFE.yaml"}, "date": "2026-01-01T00:00:00",
            "version": "8.1.9"}
    path = os.path.join(HERE, "ref_ckpt_carafe.pt")
    torch.save(ckpt, path)
    assert os.path.getsize(path) < 1 << 20
    # what the checkpoint's (fp16-rounded) state computes in fp32, as a loader of either side runs it
    m.load_state_dict({k: (v.half().float() if v.is_floating_point() else v) for k, v in m.state_dict().items()})
    m.eval()
    img = synth_batch(BATCH_SEED, 2, 4, 6)["img"]
    put_layout(arrs, "ckpt", layout, CKPT_SEED)
    arrs["ckpt/carafe_channels"] = np.array([m.model[i].comp.conv.in_channels for i in U.CARAFE_LAYERS])
    with torch.no_grad():
        arrs["ckpt/y_eval"] = m(img)[0]
    print(f"ref_ckpt_carafe.pt  {os.path.getsize(path) / 1024:.1f} KiB, {sum(q.numel() for q in m.parameters())} parameters")


def to_np(arrs):
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()}


def main():
    import glob
    arrs, big = {}, {}
    gen_modules(arrs, big)
    gen_kernels(arrs, big)
    gen_model(arrs)
    gen_ckpt(arrs)
    out = to_np(arrs)
    files = {"carafe": {k: v for k, v in out.items() if not k.startswith("ker/")},
             "carafe_kernel": {k: v for k, v in out.items() if k.startswith("ker/")}}
    # the big cases in pieces, packed greedily into files below 1 MiB
    for f in glob.glob(os.path.join(HERE, "carafe_big_*.npz")):
        os.remove(f)
    pieces = []
    for key, a in to_np(big).items():
        flat = a.reshape(-1)
        step = PIECE * 8 // a.itemsize
        pieces.append((f"{key}@shape", np.array(a.shape, dtype=np.int64)))
        pieces += [(f"{key}@{lo}:{min(lo + step, flat.size)}", flat[lo:lo + step]) for lo in range(0, flat.size, step)]
    cur, size, n = {}, 0, 0
    for k, a in pieces:
        if cur and size + a.nbytes > 900000:
            files[f"carafe_big_{n}"] = cur
            cur, size, n = {}, 0, n + 1
        cur[k] = a
        size += a.nbytes
    if cur:
        files[f"carafe_big_{n}"] = cur
    for fname, arrays in files.items():
        path = os.path.join(HERE, fname + ".npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < 1 << 20, (fname, os.path.getsize(path))
        print(f"{fname}.npz  {os.path.getsize(path) / 1024:.1f} KiB  ({len(arrays)} arrays)")


if __name__ == "__main__":
    main()
