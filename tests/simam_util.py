"""Helpers of the SimAM tests: the case lists, the seeded inputs of the kernel cases, the deterministic state the fixtures were taken
with (the generator tests/golden/make_simam_golden.py and the tests call the same functions, so no weights are stored), the run
geometry of csrc/simam.hip as the header states it, and the fp16-storage emulation the generator measures its tolerances with.  The
oracle does not know SimAM, so state layouts come from the name / shape lists the generator stored."""
import os

import numpy as np
import torch

from carafe_util import batch, layout  # noqa: F401  (the same fixture conventions)
from oracle import graph as og

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CKPT = os.path.join(GOLDEN, "ref_ckpt_simam.pt")
MODEL = "yolov8n-ASF-P2P2-SimAM"
BASE = "yolov8n-ASF-P2P2"
SIMAM_LAYERS = (26, 27, 28)
SIMAM_INPUTS = {26: 25, 27: 20, 28: 23}
SIMAM_WIDTHS = {26: 32, 27: 64, 28: 128}  # scale n
N_PARAMS = 997202
BATCH = 2
STEP_LR, STEP_MOM = 0.01, 0.9  # the optimizer step of the graph fixture (tests/golden/make_simam_golden.py)
LOSS_SCALE = 1024.0            # the tests' StepPlan(init_scale=...)
LAM = float(np.float32(1e-4))  # e_lambda as the C entry receives it

# ---- kernel cases: name -> (N, H, W, C, c0, ld): the operand's width C at channel offset c0 of pitch ld ---------------------------
# odd sizes and two images; a slice of wider storage with a granule count that is no power of two (3 granules: 85 pixel rows per
# sweep, one lane idle); the smallest defined plane (n = 1); the undefined one (n = 0: NaN); the issue's 40 x 40 map (ONE run per
# image: 1,600 pixels < the 2,048 of a run at 2 granules); "runs": 5,250 pixels of one granule, more than the 4,096 a run holds ->
# 2 runs per image, the second ragged; "capped": 8,281 pixels of 32 granules, more than SIMAM_MAX_PARTS = 64 runs of 128 -> the runs
# grow to 130 pixels and the last one is ragged; "wide": 257 granules, more than the 256 a workgroup covers -> two granule blocks,
# the second of ONE granule (256 pixel rows per sweep over a 15-pixel plane)
KERNEL_CASES = {"odd": (2, 5, 7, 8, 0, 8), "slice": (2, 5, 7, 24, 8, 40), "two_px": (1, 1, 2, 8, 0, 8), "map40": (3, 40, 40, 16, 0, 16),
                "runs": (2, 70, 75, 8, 0, 8), "capped": (1, 91, 91, 256, 0, 256), "wide": (1, 3, 5, 2056, 0, 2056)}
ONE_PX = (1, 1, 1, 8, 0, 8)
SWEEPS, MAX_PARTS, GBLOCK = 16, 64, 256  # csrc/simam.hip: SIMAM_SWEEPS, SIMAM_MAX_PARTS, SIMAM_GBLOCK
EXPECT_PARTS = {"odd": 1, "slice": 1, "two_px": 1, "map40": 1, "runs": 2, "capped": 64, "wide": 1}

# ---- module cases: name -> (C, H, W, e_lambda, offset, spread): x = offset + spread * rnd -------------------------------------------
MODULE_CASES = {"sa_8": (8, 5, 7, 1e-4, 0.0, 1.0), "sa_24": (24, 6, 10, 1e-4, 0.0, 1.0), "sa_32_lam": (32, 8, 8, 1e-2, 0.0, 1.0),
                "sa_16_offset": (16, 12, 20, 1e-4, 3.0, 0.1)}
MODULE_SEEDS = {name: 950 + i for i, name in enumerate(MODULE_CASES)}


def num_partials(M, C):
    """dy_simam_num_partials as the kernel file states it: runs of (256 / G) * SIMAM_SWEEPS pixels, G = min(C / 8, 256) granules per
    pixel row; more than SIMAM_MAX_PARTS of them: runs of ceil(M / SIMAM_MAX_PARTS) pixels instead."""
    G = min(C // 8, GBLOCK)
    ppc = (256 // G) * SWEEPS
    parts = -(-M // ppc)
    if parts > MAX_PARTS:
        ppc = -(-M // MAX_PARTS)
        parts = -(-M // ppc)
    return parts


def _f16(a):
    return np.asarray(a).astype(np.float16).astype(np.float64)


def normal_inputs(shape, seed=2):
    """x, dy and a stored gradient: standard normal values rounded to fp16 (held in float64), NHWC."""
    rng = np.random.default_rng(seed)
    return tuple(_f16(rng.standard_normal(shape)) for _ in range(3))


def offset_inputs(shape, seed=3):
    """The cancellation case: planes of 30 +- 0.01 (mean >> spread)."""
    rng = np.random.default_rng(seed)
    x = _f16(30.0 + 0.01 * rng.standard_normal(shape))
    return x, _f16(rng.standard_normal(shape)), _f16(rng.standard_normal(shape))


def large_inputs(shape, seed=4):
    """Planes of +-60000: the squares need fp32's range, the sums fp64's."""
    rng = np.random.default_rng(seed)
    x = _f16(60000.0 * np.where(rng.random(shape) < 0.5, -1.0, 1.0))
    return x, _f16(rng.standard_normal(shape)), _f16(rng.standard_normal(shape))


# values whose product with sigmoid(0.5) lies far from every fp16 rounding boundary (asserted where they are used), one per channel
CONST_VALUES = (1.0, 2.0, -3.0, 0.5, 7.0, -0.25, 10.0, 0.0)


def const_inputs(shape):
    """Every plane constant (channel c holds CONST_VALUES[c % 8] * (1 + image index)), dy constant per plane too."""
    N, H, W, C = shape
    v = np.array([CONST_VALUES[c % 8] for c in range(C)], dtype=np.float64)
    x = np.broadcast_to(v[None, None, None, :] * (1.0 + np.arange(N))[:, None, None, None], shape).copy()
    g = np.broadcast_to(v[::-1][None, None, None, :] + 0.0 * x, shape).copy()
    return _f16(x), _f16(g)


# ---- state ------------------------------------------------------------------------------------------------------------------------
def fill_state(layout_, seed):
    """``oracle.graph.fill_state`` over ``layout_`` (name -> shape): SimAM adds no entry."""
    return og.fill_state(dict(layout_), int(seed))


def state(G, prefix):
    return fill_state(layout(G, prefix), int(G[f"{prefix}/seed"]))


# ---- the HIP path's fp16 storage, emulated in float64 (what the generator measures the tolerances with) --------------------------
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


def attach_storage(e, fused=False):
    """The HIP path's fp16 storage points as hooks on ``e``, a float64 copy of a model: every convolution's raw output (``fused``: a
    folded Conv stores its activation only), every SiLU / LeakyReLU output, every sum or product a block stores (Bottleneck's
    shortcut, ScalSeq's tail, Add, SimAM's attended map), the image as the stem stages it; the weights of the convolutions rounded to
    fp16 (their MFMA packs); Detect's final convolutions' logits left in fp32 with an fp16 gradient at the loss scale."""
    import torch.nn as nn
    det = e.model[-1]
    keep32 = {id(seq[-1]) for seq in list(det.cv2) + list(det.cv3)} | {id(det.dfl.conv)}
    hook = lambda mod, inp, out: r16(out)  # noqa: E731
    stored = ("Bottleneck", "Add", "ScalSeq", "SimAM")
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
        elif type(mod).__name__ in stored:
            mod.register_forward_hook(hook)
    e.model[0].register_forward_pre_hook(lambda mod, inp: (r16(inp[0]),))
    return e


def emulate_graph(m, sd0, batch_):
    """One training step of a float64 copy of ``m`` with the HIP path's fp16 storage points -> (loss, items, {name: gradient})."""
    from copy import deepcopy
    e = deepcopy(m)
    e.load_state_dict(sd0)
    attach_storage(e.double().train())
    b64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch_.items()}
    b64["img"] = batch_["img"].half().double()  # the stem stages the image as fp16
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


def emulate_module(mod, x, gy):
    """Forward and backward of a float64 copy of a SimAM-like module with x, y, gy and gx stored in fp16 -> (y, gx)."""
    from copy import deepcopy
    e = deepcopy(mod).double()
    xe = x.detach().half().double().requires_grad_(True)
    ye = r16(e(r16(xe)))
    ye.backward(gy.half().double())
    return ye.detach(), xe.grad
