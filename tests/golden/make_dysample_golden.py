"""Generate tests/golden/dysample.npz, tests/golden/dysample_kernel.npz, tests/golden/dysample_big_*.npz and tests/golden/ref_ckpt_dysample.pt from the REFERENCE
implementation: DySample (learned dynamic up-sampling, reference nn/extra_modules/block.py:3819-3892, style 'lp') on its own and
inside this package's yolov8-ASF-P2P2-DySample graph.

Run in the build container only (needs the reference tree, which ``_refimport`` locates):

    python tests/golden/make_dysample_golden.py

State: ``tests/dysample_util.dysample_state(layout, seed, gain)`` -- ``oracle.graph.fill_state`` over the layout read off the
reference module's own ``state_dict()``, every ``init_pos`` set to the closed form, every ``offset.weight`` / ``offset.bias``
multiplied by ``gain``.  The tests call the same function, so no weights are stored; ``keys`` / ``shapes`` / ``seed`` / ``gain`` are.

dysample.npz
  ``mod/<case>/``: the reference DySample(C, s, 'lp', 4) in train mode, fp32, N = 2: ``y``, ``gx``, ``gp/offset.weight``,
  ``gp/offset.bias`` for ``x = rnd(10 seed)`` and ``gy = rnd(10 seed + 1)`` (tests/golden/cases.py; both stored for the small cases),
  ``init_pos`` (the reference's buffer), and the state's ``keys`` / ``shapes`` / ``seed`` / ``gain``.  ``gain`` puts std(0.25 o) at
  0.68 px: the smallest round figure at which 1 % of the samples are displaced by more than 2 px (asserted, with >= 5 % clamped at a
  border); ``mod/ds_32_s2_zero`` has gain 0 (asserted: all offsets zero), the pure init_pos up-sampling.
  ``tol/<case>/{y,gx,gw,gb}``: measured here, not derived: the relative Frobenius error against those fp32 values of a float64
  emulation of the HIP path's storage -- x, the weights and gy rounded to fp16, the offsets the fp32 result of those, y, d(o) and both
  writes of gx rounded to fp16 (tests/dysample_ref.py does the arithmetic).
dysample_kernel.npz (the float64 values)
  ``mod64/<case>/``: ``y``, ``gx``, ``gw``, ``gb`` of the same module, state, x and gy in float64 (the big case: no ``y``; the kernel
  case of that shape covers it).
  ``ker/<case>/``: the sampler alone in float64 through the reference's ``sample`` and autograd: inputs from
  ``dysample_util.kernel_inputs(C, s, H, W, seed)`` (``x``, ``off``, ``dy`` stored for the small cases, ``seed`` for all), ``y``,
  ``dx``, ``doff`` (w.r.t. the RAW offsets), NHWC.  The magnitudes of the per-element bounds (sum of |terms|, |d value / d
  coordinate|) are not stored (they would double the files): tests/dysample_ref.py returns them as ``mag`` / ``dcoord``, ``dx_mag`` /
  ``dx_dcoord``, ``doff_mag`` / ``doff_dcoord`` beside the values that tests/test_host_dysample.py ties to these to 1e-11;
  ``dx_terms_max`` is the largest number of terms in one dx element.
  ``ker/b_s2``, ``ker/b_s4``: ``seed`` only (|0.25 o| <= 0.9: the bit-repeatability cases).
dysample.npz, continued
  ``batch/``, ``<model>/``, ``ckpt/``: as tests/golden/make_spd_golden.py stores them, plus ``gain`` (std(0.25 o) of the two layers
  about 0.5 px on that batch, asserted within [0.35, 0.65]).
dysample_big_*.npz: the arrays of the 64-channel 24 x 20 cases in pieces (``key@lo:hi`` of the flattened array, ``key@shape``), so that
  no fixture file exceeds 1 MiB.
ref_ckpt_dysample.pt: the reference's on-disk layout (engine/trainer.py:898-923) of the graph at scale ``t = [0.17, 0.125, 256]``
  written by the reference's classes, as ref_ckpt_spd.pt was; its two layers see 32 and 16 channels there, so its pickled YAML
  says ``DySample [2, 'lp', 2]`` (two groups; ``ckpt/groups``).  The file is data: tensors, class paths and the YAML dict.
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
from ultralytics.nn.extra_modules.block import DySample  # noqa: E402
from ultralytics.nn.tasks import DetectionModel  # noqa: E402
from ultralytics.utils import DEFAULT_CFG  # noqa: E402

from cases import rnd, synth_batch  # noqa: E402
import dysample_ref as R  # noqa: E402
import dysample_util as U  # noqa: E402

assert DySample.__module__ == "ultralytics.nn.extra_modules.block" and sys.modules[DySample.__module__].__file__.startswith(_refimport.REF)
OUR_CFG = os.path.join(ROOT, "experiment-yolo_amd", "ultralytics", "cfg", "models")
torch.set_num_threads(8)

MODULE_SEEDS = {"ds_32_s2": 400, "ds_64_s2": 401, "ds_32_s4": 402, "ds_64_s2_big": 403, U.ZERO_CASE: 404}
KERNEL_SEEDS = {"k_32_s2": 500, "k_64_s2": 501, "k_32_s4": 502, "k_64_s2_big": 503, "b_s2": 510, "b_s4": 511}
TARGET_STD, MODEL_STD = 0.68, 0.5
MODEL_SEED, BATCH_SEED, CKPT_SEED, CKPT_SCALE = 41, 60, 43, ("t", [0.17, 0.125, 256])
PIECE = 100000  # elements of a float64 piece of a big array (0.8 MB)


def l2err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-12))


def layout_of(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def put_layout(arrs, prefix, layout, seed, gain):
    arrs[f"{prefix}/keys"] = np.array(list(layout))
    arrs[f"{prefix}/shapes"] = np.array([str(s) for s in layout.values()])
    arrs[f"{prefix}/seed"] = np.int32(seed)
    arrs[f"{prefix}/gain"] = np.float64(gain)


def h16(t):
    return t.half().double()


def emulate(x, gy, sd, s, G):
    """The HIP path's storage in float64 arithmetic -> y, gx, gw, gb (NCHW / parameter shapes)."""
    w, b = h16(sd["offset.weight"]), sd["offset.bias"].double()
    xh, gh = R.nhwc(h16(x)), R.nhwc(h16(gy))
    off = R.offset_conv(xh, w, b).float()  # the convolution's fp32 output
    y = h16(R.forward(xh, off, s, G)["y"])
    bw = R.backward(xh, off, gh, s, G)
    doff = h16(bw["doff"])
    w2 = w.reshape(w.shape[0], -1)
    gx = h16(h16(bw["dx"]) + doff @ w2)
    gw = (doff.reshape(-1, doff.shape[-1]).t() @ xh.reshape(-1, xh.shape[-1])).reshape(sd["offset.weight"].shape)
    gb = doff.reshape(-1, doff.shape[-1]).sum(0)
    return R.nchw(y), R.nchw(gx), gw, gb


def gen_modules(arrs, big):
    cases = dict(U.MODULE_CASES)
    cases[U.ZERO_CASE] = U.MODULE_CASES["ds_32_s2"]
    for name, (C, s, H, W) in cases.items():
        seed = MODULE_SEEDS[name]
        dst = big if name.endswith(U.BIG) else arrs
        torch.manual_seed(0)
        m = DySample(C, s, "lp", U.GROUPS)
        layout = layout_of(m)
        assert list(layout) == ["init_pos", "offset.weight", "offset.bias"], list(layout)
        ref_init = m.init_pos.clone()
        x = rnd(10 * seed, U.BATCH, C, H, W)
        gain = 0.0
        if name != U.ZERO_CASE:
            m.load_state_dict(U.dysample_state(layout, seed, 1.0), strict=True)
            with torch.no_grad():
                gain = round(TARGET_STD / float((0.25 * m.offset(x)).std()), 3)
        sd = U.dysample_state(layout, seed, gain)
        assert torch.equal(sd["init_pos"], ref_init), "init_pos formula differs from the reference's buffer"
        m.load_state_dict(sd, strict=True)
        m.train()
        x.requires_grad_(True)
        y = m(x)
        gy = rnd(10 * seed + 1, *y.shape)
        y.backward(gy)
        with torch.no_grad():
            o = m.offset(x)
            ux, uy = R.positions(R.nhwc(o), s, U.GROUPS)
            clamped = ((ux < 0) | (ux > W - 1) | (uy < 0) | (uy > H - 1)).double().mean()
            o2 = (0.25 * R.nhwc(o).double()).view(U.BATCH, H, W, 2, -1)
            far = (o2.pow(2).sum(3).sqrt() > 2.0).double().mean()
        if name == U.ZERO_CASE:
            assert float(o.abs().max()) == 0.0
        else:
            assert float(clamped) >= 0.05 and float(far) >= 0.01, (name, float(clamped), float(far))
        p = f"mod/{name}"
        put_layout(arrs, p, layout, seed, gain)
        arrs[f"{p}/init_pos"] = ref_init
        if dst is arrs:
            arrs[f"{p}/x"], arrs[f"{p}/gy"] = x.detach(), gy
        dst[f"{p}/y"], dst[f"{p}/gx"] = y.detach(), x.grad
        for k, q in m.named_parameters():
            arrs[f"{p}/gp/{k}"] = q.grad
        # the same module, state and tensors in float64: what tests/dysample_ref.py is held to (1e-11), the fp32 run's rounding apart
        m64 = DySample(C, s, "lp", U.GROUPS).double()
        m64.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        m64.train()
        x64 = x.detach().double().requires_grad_(True)
        y64 = m64(x64)
        y64.backward(gy.double())
        q = f"mod64/{name}"
        if dst is arrs:
            arrs[f"{q}/y"] = y64.detach()
        dst[f"{q}/gx"] = x64.grad
        arrs[f"{q}/gw"], arrs[f"{q}/gb"] = m64.offset.weight.grad, m64.offset.bias.grad
        ey, ex, ew, eb = emulate(x.detach(), gy, sd, s, U.GROUPS)
        tol = dict(y=l2err(ey, y.detach()), gx=l2err(ex, x.grad), gw=l2err(ew, m.offset.weight.grad), gb=l2err(eb, m.offset.bias.grad))
        for k, v in tol.items():
            arrs[f"tol/{name}/{k}"] = np.float64(v)
        print(name, tuple(y.shape), f"gain {gain} clamped {float(clamped):.3f} beyond 2 px {float(far):.3f} tol", {k: f"{v:.2e}" for k, v in tol.items()})


def gen_kernels(arrs, big):
    cases = {**{k: (v, False) for k, v in U.KERNEL_CASES.items()}, **{k: (v, True) for k, v in U.BOUNDED_CASES.items()}}
    for name, ((C, s, H, W), bounded) in cases.items():
        seed = KERNEL_SEEDS[name]
        p = f"ker/{name}"
        arrs[f"{p}/seed"] = np.int32(seed)
        x, off, dy = U.kernel_inputs(C, s, H, W, seed, bounded)
        if bounded:
            assert float((0.25 * off).abs().max()) <= 0.9
            continue
        dst = big if name.endswith(U.BIG) else arrs
        m = DySample(C, s, "lp", U.GROUPS).double()
        xd = R.nchw(x.double()).requires_grad_(True)
        od = R.nchw(off.double()).requires_grad_(True)
        y = m.sample(xd, od * 0.25 + m.init_pos)
        y.backward(R.nchw(dy.double()))
        fw, bw = R.forward(x, off, s, U.GROUPS), R.backward(x, off, dy, s, U.GROUPS)
        if dst is arrs:
            arrs[f"{p}/x"], arrs[f"{p}/off"], arrs[f"{p}/dy"] = x, off, dy
        dst[f"{p}/y"], dst[f"{p}/dx"], dst[f"{p}/doff"] = R.nhwc(y.detach()), R.nhwc(xd.grad), R.nhwc(od.grad)
        arrs[f"{p}/dx_terms_max"] = np.int32(int(bw["dx_terms"].max()))
        assert int(bw["dx_terms"].max()) <= 120  # what k32 of the dx bound in tests/test_gpu_dysample.py is counted for
        ux, uy = R.positions(off, s, U.GROUPS)
        clamped = float(((ux < 0) | (ux > W - 1) | (uy < 0) | (uy > H - 1)).double().mean())
        far = float(((0.25 * off).abs() > 1.0).view(U.BATCH, H, W, 2, -1).any(3).double().mean())
        assert clamped >= 0.05 and far >= 0.01
        errs = [float((fw["y"] - dst[f"{p}/y"]).abs().max()), float((bw["dx"] - dst[f"{p}/dx"]).abs().max()),
                float((bw["doff"] - dst[f"{p}/doff"]).abs().max())]
        print(name, f"clamped {clamped:.3f} |0.25 o| > 1 {far:.3f} terms/dx <= {int(bw['dx_terms'].max())} restatement max abs err", errs)


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

    def offset_std(gain):
        m.load_state_dict(U.dysample_state(layout, MODEL_SEED, gain), strict=True)
        seen = []
        hooks = [m.model[i].offset.register_forward_hook(lambda mod, a, out: seen.append(float((0.25 * out).std()))) for i in U.DYSAMPLE_LAYERS]
        m.train()
        with torch.no_grad():
            m(batch["img"])
        for h in hooks:
            h.remove()
        return seen

    s1 = offset_std(1.0)
    gain = round(MODEL_STD / (sum(s1) / len(s1)), 2)
    sg = offset_std(gain)
    assert all(0.35 <= v <= 0.65 for v in sg), sg
    put_layout(arrs, name, layout, MODEL_SEED, gain)
    arrs[f"{name}/n_params"] = np.int64(sum(q.numel() for q in m.parameters()))
    arrs[f"{name}/stride"] = m.stride
    arrs[f"{name}/offset_std"] = np.array(sg)
    m.load_state_dict(U.dysample_state(layout, MODEL_SEED, gain), strict=True)
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
    print(name, int(arrs[f"{name}/n_params"]), m.stride.tolist(), "gain", gain, "std(0.25 o)", sg, "loss", float(loss), "items", items.tolist())
    return gain


def gen_ckpt(arrs, gain):
    from copy import deepcopy
    d = yaml.safe_load(open(os.path.join(OUR_CFG, "yolov8-ASF-P2P2-DySample.yaml")))
    d["scales"][CKPT_SCALE[0]] = CKPT_SCALE[1]
    d["scale"] = CKPT_SCALE[0]
    for row in d["head"]:  # 32 and 16 channels at this scale: two groups keep every group a whole number of 16-byte granules
        if row[2] == "DySample":
            row[3] = [2, "lp", U.CKPT_GROUPS]
    torch.manual_seed(0)
    m = DetectionModel(d, ch=3, verbose=False)
    layout = layout_of(m)
    m.load_state_dict(U.dysample_state(layout, CKPT_SEED, gain, U.CKPT_GROUPS), strict=True)
    m.args = dict(get_cfg(DEFAULT_CFG).__dict__)
    ckpt = {"epoch": 3, "best_fitness": 0.25, "model": deepcopy(m).half(), "ema": None, "updates": 57, "optimizer": None,
            "train_args": {"imgsz": 640, "batch": 64, "model": "yolov8-ASF-P2P2-DySample.yaml"}, "date": "2026-01-01T00:00:00",
            "version": "8.1.9"}
    path = os.path.join(HERE, "ref_ckpt_dysample.pt")
    torch.save(ckpt, path)
    assert os.path.getsize(path) < 1 << 20
    # what the checkpoint's (fp16-rounded) state computes in fp32, as a loader of either side runs it
    m.load_state_dict({k: (v.half().float() if v.is_floating_point() else v) for k, v in m.state_dict().items()})
    m.eval()
    img = synth_batch(BATCH_SEED, 2, 4, 6)["img"]
    put_layout(arrs, "ckpt", layout, CKPT_SEED, gain)
    arrs["ckpt/groups"] = np.int32(U.CKPT_GROUPS)
    with torch.no_grad():
        arrs["ckpt/y_eval"] = m(img)[0]
    print(f"ref_ckpt_dysample.pt  {os.path.getsize(path) / 1024:.1f} KiB, {sum(q.numel() for q in m.parameters())} parameters")


def to_np(arrs):
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()}


def main():
    import glob
    arrs, big = {}, {}
    gen_modules(arrs, big)
    gen_kernels(arrs, big)
    gain = gen_model(arrs)
    gen_ckpt(arrs, gain)
    out = to_np(arrs)  # one fixture file would exceed 1 MiB: the kernel cases go to a file of their own
    f64 = ("ker/", "mod64/")
    files = {"dysample": {k: v for k, v in out.items() if not k.startswith(f64)},
             "dysample_kernel": {k: v for k, v in out.items() if k.startswith(f64)}}
    # the big cases in pieces, packed greedily into files below 1 MiB
    for f in glob.glob(os.path.join(HERE, "dysample_big_*.npz")):
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
            files[f"dysample_big_{n}"] = cur
            cur, size, n = {}, 0, n + 1
        cur[k] = a
        size += a.nbytes
    if cur:
        files[f"dysample_big_{n}"] = cur
    for fname, arrays in files.items():
        path = os.path.join(HERE, fname + ".npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < 1 << 20, (fname, os.path.getsize(path))
        print(f"{fname}.npz  {os.path.getsize(path) / 1024:.1f} KiB  ({len(arrays)} arrays)")


if __name__ == "__main__":
    main()
