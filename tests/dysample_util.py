"""Helpers of the DySample tests: the deterministic state the fixtures of tests/golden/make_dysample_golden.py were taken with (the
generator and the tests both call ``dysample_state``, so no weights are stored) and the case lists.  The oracle does not know
DySample, so state layouts come from the name / shape lists the generator stored, not from oracle.graph.state_layout."""
import ast
import os

import torch

from oracle import graph as og

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")  # (not from conftest: the generator imports this file too)

CKPT = os.path.join(GOLDEN, "ref_ckpt_dysample.pt")
MODEL = "yolov8n-ASF-P2P2-DySample"
DYSAMPLE_LAYERS = (9, 14)
CKPT_GROUPS = 2  # the checkpoint's narrower graph (32 and 16 channels in front of the two layers) runs DySample [2, 'lp', 2]
# name -> (C, scale, H, W); groups = 4, N = 2
MODULE_CASES = {"ds_32_s2": (32, 2, 5, 7), "ds_64_s2": (64, 2, 6, 4), "ds_32_s4": (32, 4, 3, 5), "ds_64_s2_big": (64, 2, 24, 20)}
ZERO_CASE = "ds_32_s2_zero"  # gain = 0: the pure init_pos up-sampling
KERNEL_CASES = {"k_32_s2": (32, 2, 5, 7), "k_64_s2": (64, 2, 6, 4), "k_32_s4": (32, 4, 3, 5), "k_64_s2_big": (64, 2, 24, 20)}
BOUNDED_CASES = {"b_s2": (64, 2, 6, 4), "b_s4": (32, 4, 3, 5)}  # |0.25 o| <= 0.9: the bit-repeatability cases
GROUPS, BATCH = 4, 2
SLICE = dict(x_off=16, x_extra=24, y_off=8, y_extra=8)  # sliced variant: x at channel 16 of pitch C + 24, y at channel 8 of pitch C + 8
KINK = 2.0 ** -10  # no unclamped sampling position of a kernel case lies this close to an integer (0, W-1 and H-1 are integers)
BIG = "64_s2_big"  # the arrays of the cases whose name ends so are too large for one fixture file: tests/golden/dysample_big_*.npz


def kernel_inputs(C, s, H, W, seed, bounded=False):
    """The inputs of a kernel case, as the generator drew them: x fp16 (N, H, W, C), raw offsets fp32 (N, H, W, 2 G s^2) and dy fp16
    (N, sH, sW, C).  Offsets: normal with std(0.25 o) = 0.68 px -- clamped and far samples included -- or, ``bounded``, uniform with
    |0.25 o| <= 0.9.  An offset whose unclamped position lies within KINK of an integer is drawn again until none does: the kernel's
    fp32 position (off by < 2^-18 on these maps) then falls on the float64 reference's side of every kink."""
    import numpy as np
    import dysample_ref as R
    rng = np.random.default_rng(seed)
    N, G = BATCH, GROUPS
    x = torch.from_numpy(rng.standard_normal((N, H, W, C)).astype(np.float16))
    dy = torch.from_numpy(rng.standard_normal((N, s * H, s * W, C)).astype(np.float16))

    def draw(n):
        v = rng.uniform(-3.6, 3.6, n) if bounded else rng.standard_normal(n) * (4 * 0.68)
        return torch.from_numpy(v.astype(np.float32))

    off = draw(N * H * W * 2 * G * s * s).reshape(N, H, W, -1)
    while True:
        ux, uy = R.positions(off, s, G)
        u = torch.stack([ux, uy], 3).reshape(off.shape)
        bad = (u - u.round()).abs() < KINK
        if not bool(bad.any()):
            return x, off, dy
        off[bad] = draw(int(bad.sum()))


def load_big(key):
    """An array of the big cases, put together from the pieces tests/golden/dysample_big_*.npz hold (``key@lo:hi`` = those elements of
    the flattened array, ``key@shape`` its shape)."""
    import glob
    import numpy as np
    parts, shape = {}, None
    for f in sorted(glob.glob(os.path.join(GOLDEN, "dysample_big_*.npz"))):
        z = np.load(f, allow_pickle=False)
        for k in z.files:
            base, _, rng_ = k.partition("@")
            if base != key:
                continue
            if rng_ == "shape":
                shape = tuple(int(v) for v in z[k])
            else:
                parts[int(rng_.split(":")[0])] = z[k]
    assert parts and shape is not None, key
    return torch.from_numpy(np.concatenate([parts[k] for k in sorted(parts)]).reshape(shape))


def fetch(G, key):
    """A fixture array by key: from dysample.npz, or from the side files when the case is a big one."""
    return G.t(key) if key in G else load_big(key)


def init_pos(scale, groups):
    """(1, 2 G s^2, 1, 1) fp32: channel d G s^2 + g s^2 + i s + j holds t[j] (d = 0) or t[i] (d = 1), t[k] = (k - (s-1)/2) / s."""
    s = scale
    t = (torch.arange(s, dtype=torch.float32) - (s - 1) / 2) / s
    tx, ty = t.view(1, s).expand(s, s), t.view(s, 1).expand(s, s)
    return torch.stack([tx, ty]).reshape(2, 1, s * s).repeat(1, groups, 1).reshape(1, -1, 1, 1).contiguous()


def dysample_state(layout, seed, gain, groups=GROUPS):
    """``oracle.graph.fill_state`` over ``layout`` (name -> shape), then every ``init_pos`` set to the formula (scale from the offset
    convolution's width: 2 G s^2 channels, G = ``groups``) and every ``offset.weight`` / ``offset.bias`` multiplied by ``gain``."""
    sd = og.fill_state(dict(layout), int(seed))
    for k in list(sd):
        if k.endswith("init_pos"):
            nch = int(layout[k][1])
            s = {2 * groups * 4: 2, 2 * groups * 16: 4}[nch]
            sd[k] = init_pos(s, groups)
        elif k.endswith("offset.weight") or k.endswith("offset.bias"):
            sd[k] = sd[k] * float(gain)
    return sd


def layout(G, prefix):
    """name -> shape as the reference's state_dict() listed them (in order)."""
    return {str(k): tuple(ast.literal_eval(str(s))) for k, s in zip(G[f"{prefix}/keys"], G[f"{prefix}/shapes"])}


def state(G, prefix):
    groups = int(G[f"{prefix}/groups"]) if f"{prefix}/groups" in G else GROUPS
    return dysample_state(layout(G, prefix), int(G[f"{prefix}/seed"]), float(G[f"{prefix}/gain"]), groups)


def batch(G):
    return {k: G.t(f"batch/{k}") for k in ("img", "batch_idx", "cls", "bboxes")}
