"""Helpers of the CARAFE tests: the case lists, the seeded inputs of the kernel cases (the generator
tests/golden/make_carafe_golden.py and the tests both call ``kernel_inputs``, so only seeds are stored) and the deterministic state
the fixtures were taken with.  The oracle does not know CARAFE, so state layouts come from the name / shape lists the generator
stored, not from oracle.graph.state_layout."""
import ast
import os

import torch

from oracle import graph as og

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")  # (not from conftest: the generator imports this file too)

CKPT = os.path.join(GOLDEN, "ref_ckpt_carafe.pt")
MODEL = "yolov8n-ASF-P2P2-CARAFE"
CARAFE_LAYERS = (9, 14)
BATCH = 2
# name -> (C, H, W, logit gain).  The last two are this project's own: a row wider than one workgroup's run of base pixels (column
# seams and halos) and more channels than one LDS chunk holds.
KERNEL_CASES = {"k_8": (8, 3, 4, 1.0), "k_32": (32, 5, 7, 1.0), "k_64": (64, 6, 4, 1.0), "k_64_big": (64, 24, 20, 1.0),
                "k_32_hot": (32, 5, 7, 64.0), "k_8_wide": (8, 3, 37, 1.0), "k_72": (72, 3, 4, 1.0)}
# name -> (C, c_mid, k_enc, H, W)
MODULE_CASES = {"cf_32_64_k3": (32, 64, 3, 5, 7), "cf_64_16_k3": (64, 16, 3, 6, 4), "cf_32_16_k1_big": (32, 16, 1, 24, 20)}
SLICE = dict(x_off=16, x_extra=24, y_off=8, y_extra=8, l_extra=8)  # sliced variant: x at channel 16 of pitch C + 24, y at 8 of C + 8, logits in pitch 112
BIG = "_big"  # the arrays of the cases whose name ends so are too large for one fixture file: tests/golden/carafe_big_*.npz


def kernel_inputs(C, H, W, seed, gain=1.0):
    """x fp16 (N, H, W, C), logits fp16 (N, H, W, 100) = normal * gain, dy fp16 (N, 2H, 2W, C), as the generator drew them."""
    import numpy as np
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((BATCH, H, W, C)).astype(np.float16))
    lg = torch.from_numpy((rng.standard_normal((BATCH, H, W, 100)) * gain).astype(np.float16))
    dy = torch.from_numpy(rng.standard_normal((BATCH, 2 * H, 2 * W, C)).astype(np.float16))
    return x, lg, dy


def load_big(key):
    """An array of the big cases, put together from the pieces tests/golden/carafe_big_*.npz hold (``key@lo:hi`` = those elements of
    the flattened array, ``key@shape`` its shape)."""
    import glob
    import numpy as np
    parts, shape = {}, None
    for f in sorted(glob.glob(os.path.join(GOLDEN, "carafe_big_*.npz"))):
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
    """A fixture array by key: from the named file, or from the side files when the case is a big one."""
    return G.t(key) if key in G else load_big(key)


def carafe_state(layout, seed):
    """``oracle.graph.fill_state`` over ``layout`` (name -> shape)."""
    return og.fill_state(dict(layout), int(seed))


def layout(G, prefix):
    """name -> shape as the reference's state_dict() listed them (in order)."""
    return {str(k): tuple(ast.literal_eval(str(s))) for k, s in zip(G[f"{prefix}/keys"], G[f"{prefix}/shapes"])}


def state(G, prefix):
    return carafe_state(layout(G, prefix), int(G[f"{prefix}/seed"]))


def batch(G):
    return {k: G.t(f"batch/{k}") for k in ("img", "batch_idx", "cls", "bboxes")}
