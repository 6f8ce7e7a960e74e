"""Helpers of the depthwise-convolution tests: the case lists, the deterministic state the fixtures were taken with (the generator
tests/golden/make_dwconv_golden.py and the tests call the same functions, so no weights are stored) and an fp32 emulation of the
summation orders csrc/dwconv.hip documents.  The oracle does not know DWConv / DSConv, so state layouts come from the name / shape
lists the generator stored."""
import os

import numpy as np
import torch

from carafe_util import batch, carafe_state as fill_state, layout, state  # noqa: F401  (the same fixture conventions)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CKPT = os.path.join(GOLDEN, "ref_ckpt_dw.pt")
MODEL = "yolov8n-ASF-P2P2-DW"
DW_LAYERS = (1, 3, 5, 18, 21)
DW_WIDTHS = {1: (16, 32), 3: (32, 64), 5: (64, 128), 18: (32, 32), 21: (64, 64)}  # scale n: (c1, c2)
BATCH = 2
# name -> (N, H, W, C1, m, k, s): the smallest shapes at which each kernel can still go wrong.  An odd map and two images (nothing
# bleeds across images); a kernel larger than the map (taps entirely in the padding); three granules at multiplier 2; k 5 with stride 2
# and multiplier 2; a map of more pixels than one workgroup walks at once.  The last is this project's own: more than 256 output
# channels, so a second channel chunk (blockIdx.y) and its weights' offset are exercised.
KERNEL_CASES = {"k3s2_odd": (2, 7, 9, 8, 1, 3, 2), "k5s1_tiny": (1, 3, 4, 8, 1, 5, 1), "k3s2_m2": (2, 8, 8, 24, 2, 3, 2),
                "k5s2_m2": (1, 10, 6, 16, 2, 5, 2), "k3s1": (2, 12, 20, 32, 1, 3, 1), "k3s2_m2_wide": (1, 5, 4, 136, 2, 3, 2)}
SLICED = "k3s2_m2"  # the case that also runs with ld = C + 8 and channel offset 8 on x, y and the gradients
# name -> (kind, c1, c2, k, s, act, H, W)
MODULE_CASES = {"dw_16_32_k3s2": ("DWConv", 16, 32, 3, 2, True, 9, 7), "dw_24_24_k5s1": ("DWConv", 24, 24, 5, 1, True, 6, 5),
                "dw_32_32_k3s1_id": ("DWConv", 32, 32, 3, 1, False, 5, 8), "ds_16_32": ("DSConv", 16, 32, 1, 1, True, 8, 8)}
CH, FWD_MAXB, WG_MAXB = 256, 1024, 512  # csrc/dwconv.hip: DW_CH, DW_FWD_MAXB, DW_WG_MAXB


def slots(C2):
    """Pixel slots of a workgroup (csrc/dwconv.hip, dw_slots)."""
    return 256 // (min(C2, CH) // 8)


def blocks(npix, C2, cap):
    return max(1, min(cap, (npix + slots(C2) - 1) // slots(C2)))


def chunks(C2):
    """(first channel, width) of every chunk of output channels a workgroup column (blockIdx.y) owns."""
    return [(c0, min(CH, C2 - c0)) for c0 in range(0, C2, CH)]


def chain(npix, C2, cap, runs=False):
    """Additions on the longest path of a sum over ``npix`` pixels as the kernels order it: a thread's pixels, the pixel slots (of the
    chunk where the two together are most: a narrow last chunk has more slots), and (``runs``: the weight gradient's reduction) the
    slabs of a run and the 8 runs."""
    nb = blocks(npix, C2, cap)
    n = max(-(-npix // (nb * slots(cn))) + slots(cn) for _, cn in chunks(C2))
    return n + (-(-nb // 8) + 8 if runs else 0)


def k_bound(what, N, H, W, C1, m, k, s, accumulate=False):
    """(k16, k32) of the per-element bound, as counted in the docstring of tests/test_gpu_dwconv.py."""
    p = k // 2
    npix = N * ((H + 2 * p - k) // s + 1) * ((W + 2 * p - k) // s + 1)
    if what == "y":
        return 1, k * k / 2
    if what == "dx":
        return 1, m * k * k / 2 + (0.5 if accumulate else 0)
    if what == "dw":
        return 0, chain(npix, C1 * m, WG_MAXB, runs=True) / 2
    if what == "stats":
        return 0, chain(npix, C1 * m, FWD_MAXB) / 2
    raise KeyError(what)


def check(what, got, ref, mag, kb):
    """|got - ref| <= k16 2^-11 |ref| + k32 2^-23 mag + 2^-24 on EVERY element; prints the worst ratio."""
    k16, k32 = kb
    got, ref, mag = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double(), torch.as_tensor(mag).double()
    assert got.shape == ref.shape == mag.shape, (what, got.shape, ref.shape, mag.shape)
    bound = k16 * 2.0 ** -11 * ref.abs() + k32 * 2.0 ** -23 * mag + 2.0 ** -24
    err = (got - ref).abs()
    worst = float((err / bound).max())
    print(f"{what}: k16 {k16} k32 {k32}: max err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, f"{what}: {int((err > bound).sum())} of {err.numel()} elements beyond the bound"


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def seq_sum(terms, axis=0):
    """fp32 sum of float64 ``terms`` along ``axis`` in index order, one rounding per addition (the terms are exact products of an fp16
    and an fp16 / fp32 value: each step is a fused multiply-add)."""
    t = np.moveaxis(np.asarray(terms, dtype=np.float64), axis, 0)
    acc = np.zeros(t.shape[1:], dtype=np.float64)
    for i in range(t.shape[0]):
        acc = f32(acc + t[i])
    return acc


def emulate_forward(x, w, s):
    """fp32 accumulation over the taps (ky, kx) ascending, then the fp16 store -> (N,Ho,Wo,C2) float64 holding fp16 values."""
    N, H, W, C1 = x.shape
    C2, k = w.shape[0], w.shape[-1]
    m, p = C2 // C1, w.shape[-1] // 2
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = np.zeros((N, H + 2 * p, W + 2 * p, C2))
    xp[:, p:p + H, p:p + W] = np.repeat(x.double().numpy(), m, axis=-1)
    wd = w.double().numpy()
    terms = [xp[:, ky:ky + s * Ho:s, kx:kx + s * Wo:s] * wd[:, 0, ky, kx] for ky in range(k) for kx in range(k)]
    return torch.from_numpy(seq_sum(np.stack(terms))).half().double()


def emulate_input_grad(dy, w, s, H, W, m):
    """Per input pixel the taps (ky, kx) ascending, per tap the m output channels of the group ascending; then the fp16 store."""
    N, Ho, Wo, C2 = dy.shape
    k, p, C1 = w.shape[-1], w.shape[-1] // 2, C2 // m
    g, wd = dy.double().numpy(), w.double().numpy()
    terms = []
    for ky in range(k):
        for kx in range(k):
            for j in range(m):
                t = np.zeros((N, H + 2 * p + s, W + 2 * p + s, C1))
                # output pixel (oy, ox) reaches input pixel (oy s + ky - p, ox s + kx - p): index + p in the padded frame
                t[:, ky:ky + s * Ho:s, kx:kx + s * Wo:s] = g[..., j::m] * wd[j::m, 0, ky, kx]
                terms.append(t[:, p:p + H, p:p + W])
    return torch.from_numpy(seq_sum(np.stack(terms))).half().double()


def emulate_weight_grad(x, dy, k, s):
    """A thread's pixels ascending, the pixel slots, the 8 interleaved runs of slabs, the runs -> (C2,1,k,k) float64 holding fp32 values."""
    N, H, W, C1 = x.shape
    _, Ho, Wo, C2 = dy.shape
    m, p = C2 // C1, k // 2
    npix = N * Ho * Wo
    nb = blocks(npix, C2, WG_MAXB)
    xp = np.zeros((N, H + 2 * p, W + 2 * p, C2))
    xp[:, p:p + H, p:p + W] = np.repeat(x.double().numpy(), m, axis=-1)
    g = dy.double().numpy()
    out = np.zeros((C2, 1, k, k))
    for ky in range(k):
        for kx in range(k):
            full = (g * xp[:, ky:ky + s * Ho:s, kx:kx + s * Wo:s]).reshape(npix, C2)
            for c0, cn in chunks(C2):
                ps = slots(cn)
                it = -(-npix // (nb * ps))
                t = np.concatenate([full[:, c0:c0 + cn], np.zeros((it * nb * ps - npix, cn))]).reshape(it, nb, ps, cn)  # pixel = (i nb + block) ps + slot
                slab = seq_sum(seq_sum(t, 0), 1)                                              # (nb, cn)
                runs = np.stack([seq_sum(slab[q::8], 0) if q < nb else np.zeros(cn) for q in range(8)])
                out[c0:c0 + cn, 0, ky, kx] = seq_sum(runs, 0)
    return torch.from_numpy(out)
