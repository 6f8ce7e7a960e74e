"""Helpers of the SPDConv tests: the fixtures of tests/golden/make_spd_golden.py (spd.npz and the two weight-gradient side files)
and the deterministic state they were taken with.  The oracle does not know SPDConv, so the state layout comes from the name / shape
list the generator stored, not from oracle.graph.state_layout."""
import ast
import os

import numpy as np
import torch

from conftest import GOLDEN
from oracle import graph as og

CKPT = os.path.join(GOLDEN, "ref_ckpt_spd.pt")
MODELS = ["yolov8n-ASF-P2P2-SPD", "yolov8n-LD-P2-SPD"]
N_PARAMS = {"yolov8n-ASF-P2P2-SPD": 1425746, "yolov8n-LD-P2-SPD": 1430818}
SPD_LAYERS = (1, 3, 5, 18, 21)
MODULE_CASES = {"spd_16_32": (16, 32), "spd_32_64": (32, 64), "spd_64_128": (64, 128)}


def layout(G, prefix):
    """name -> shape as the reference's state_dict() listed them (in order)."""
    return {str(k): tuple(ast.literal_eval(str(s))) for k, s in zip(G[f"{prefix}/keys"], G[f"{prefix}/shapes"])}


def state(G, prefix):
    return og.fill_state(layout(G, prefix), int(G[f"{prefix}/seed"]))


def batch(G):
    return {k: G.t(f"batch/{k}") for k in ("img", "batch_idx", "cls", "bboxes")}


def module_grad(G, case, name):
    """A parameter gradient of a module case: from spd.npz, or put together from the side files that hold the larger ones."""
    key = f"mod/{case}/gp/{name}"
    if key in G:
        return G.t(key)
    parts = {}
    for f in ("spd_wgrad_a", "spd_wgrad_b"):
        z = np.load(os.path.join(GOLDEN, f + ".npz"), allow_pickle=False)
        for k in z.files:
            base, _, rows = k.partition("@")
            if base == key:
                parts[int(rows.split(":")[0]) if rows else 0] = torch.from_numpy(z[k])
    assert parts, key
    return torch.cat([parts[k] for k in sorted(parts)], 0)
