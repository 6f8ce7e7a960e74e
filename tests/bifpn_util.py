"""Helpers of the Fusion ('bifpn') tests: the case lists, the seeded inputs of the kernel cases, the deterministic state the fixtures
were taken with (the generator tests/golden/make_bifpn_golden.py and the tests call the same functions, so no weights are stored)
and the error bounds of csrc/fusion.hip, counted from the orders the kernel file documents.  The oracle does not know Fusion, so
state layouts come from the name / shape lists the generator stored."""
import os

import numpy as np
import torch

from carafe_util import batch, layout  # noqa: F401  (the same fixture conventions)
from oracle import graph as og

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CKPT = os.path.join(GOLDEN, "ref_ckpt_bifpn.pt")
MODEL = "yolov8n-ASF-P2P2-BiFPN"
FUSION_LAYERS = (11, 16, 25)
FUSION_KEYS = tuple(f"model.{i}.fusion_weight" for i in FUSION_LAYERS)
FUSION_WIDTHS = {11: 64, 16: 32, 25: 32}  # scale n
BATCH = 2
STEP_LR, STEP_MOM = 0.01, 0.9  # the optimizer step of the graph fixture (tests/golden/make_bifpn_golden.py)

# ---- kernel cases: name -> (N, H, W, C, c0, ld): the operands' width C at channel offset c0 of pitch ld ---------------------------
# one granule (half-resolution operand 3 x 5); an odd granule count; an odd map (no half-resolution operand can exist on it); a slice
# of wider storage; more than one stage-one partial per dot product (2 * 40 * 40 * 2 granules over 1,024 per workgroup: 7)
KERNEL_CASES = {"one_granule": (2, 6, 10, 8, 0, 8), "odd_granules": (2, 6, 10, 24, 0, 24), "odd_map": (2, 7, 9, 24, 0, 24),
                "slice": (2, 6, 10, 32, 8, 48), "partials": (2, 40, 40, 16, 0, 16)}
EXACT_P = {2: [(1.0, 1.0), (1.0, 3.0)], 3: [(1.0, 1.0, 2.0)]}  # every f a dyadic fraction
NORMAL_P = {2: (0.7, 1.9), 3: (1.3, 0.4, 2.1)}
CUT_P = (-0.5, 1.2)
ITEMS, MAX_PARTS = 4, 1024  # csrc/fusion.hip: FUSION_ITEMS, FUSION_MAX_PARTS

# ---- module cases: name -> (C, H, W, p): equal, unequal and one non-positive weight, 2 and 3 operands ------------------------------
MODULE_CASES = {"bf_2_equal": (16, 6, 10, (1.0, 1.0)), "bf_2_unequal": (24, 7, 9, (0.7, 1.9)), "bf_2_cut": (8, 5, 5, (-0.5, 1.2)),
                "bf_3_equal": (8, 6, 10, (1.0, 1.0, 1.0)), "bf_3_unequal": (32, 8, 8, (1.3, 0.4, 2.1)), "bf_3_cut": (16, 6, 10, (0.9, -0.3, 1.6))}
MODULE_SEEDS = {name: 900 + i for i, name in enumerate(MODULE_CASES)}


def variants(name):
    """(number of operands, index of the half-resolution operand or None) of a kernel case: 2 and 3 operands, the up-sampled operand
    first and last (and none at all); an odd map has no half-resolution operand."""
    H, W = KERNEL_CASES[name][1:3]
    ups = [None] if (H | W) & 1 else [None, "first", "last"]
    return [(n, None if u is None else (0 if u == "first" else n - 1)) for n in (2, 3) for u in ups]


def num_partials(npix, C):
    """dy_fusion_num_partials as the header states it."""
    return max(1, min(MAX_PARTS, -(-(npix * (C // 8)) // (256 * ITEMS))))


def exact_inputs(name, n, up, seed=1):
    """Operands and dy as small integers (|v| <= 3), float64 NHWC; operand ``up`` at half resolution.  -> (xs, dy, old): ``old`` the
    stored gradients of the accumulate mode, one per operand at full resolution."""
    N, H, W, C = KERNEL_CASES[name][:4]
    rng = np.random.default_rng(seed)
    draw = lambda *s: rng.integers(-3, 4, size=s).astype(np.float64)  # noqa: E731
    xs = [draw(N, H // 2, W // 2, C) if i == up else draw(N, H, W, C) for i in range(n)]
    return xs, draw(N, H, W, C), [draw(N, H, W, C) for _ in range(n)]


def normal_inputs(name, n, up, seed=2):
    """The same shapes with standard normal values rounded to fp16 (held in float64)."""
    N, H, W, C = KERNEL_CASES[name][:4]
    rng = np.random.default_rng(seed)
    draw = lambda *s: rng.standard_normal(s).astype(np.float16).astype(np.float64)  # noqa: E731
    xs = [draw(N, H // 2, W // 2, C) if i == up else draw(N, H, W, C) for i in range(n)]
    return xs, draw(N, H, W, C), [draw(N, H, W, C) for _ in range(n)]


# ---- bounds, counted from the orders csrc/fusion.hip documents ---------------------------------------------------------------------
U16, U32 = 2.0 ** -11, 2.0 ** -24  # unit round-offs (half an ulp, relative) of fp16 and fp32


def k_weight(n):
    """fp32 roundings behind one f[i]: the n - 1 additions of s, the division (relu and the conversion of p are exact)."""
    return n


def bound_y(ref, mag, n):
    """y: one fp16 rounding of the fp32 result (half an fp16 ulp: U16 |ref|, or half the subnormal spacing 2^-25) + the fp32 terms over
    mag = sum |f[i] x[i]|: each term carries f's k_weight(n) roundings and its product's one, and passes through at most n - 1
    additions (a fused multiply-add only removes roundings); + 1 for the second-order terms and for the fp16 rounding acting on the
    fp32 error."""
    return U16 * np.abs(ref) + 2.0 ** -25 + (k_weight(n) + 1 + (n - 1) + 1) * U32 * mag


def bound_dx(ref, n, old=None):
    """dx = fp16(f dy) (+ old): one fp16 rounding; fp32: f's roundings, the product, the addition of the stored value, + 1."""
    mag = np.abs(ref) if old is None else np.abs(ref - old) + np.abs(old)
    return U16 * np.abs(ref) + 2.0 ** -25 + (k_weight(n) + 1 + (0 if old is None else 1) + 1) * U32 * mag


def k_dot(npix, C):
    """Chain length plus tree depth of one stage-one partial: a work item visits ceil(granules / (256 parts)) granules and adds 8
    products per granule to a running sum (one rounding per product, one per addition: 2 per element without a fused
    multiply-add), then 6 xor-shuffle levels and 3 additions over the four waves."""
    per_item = -(-(npix * (C // 8)) // (256 * num_partials(npix, C)))
    return 2 * 8 * per_item + 6 + 3


def bound_g(gmag, npix, C):
    """g[i]: k_dot roundings over sum |dy x| inside a partial; the fp64 sum of the partials (<= 1,024 additions at 2^-53 each) and its one
    rounding to fp32 are the + 1."""
    return (k_dot(npix, C) + 1) * U32 * gmag


def bound_dp(p, g, gmag, npix, C):
    """dL/dp[j] = (g[j] - t) / s with t = sum_i f[i] g[i], the Jacobian in fp32 on top of the error of the g: every g[i] enters with
    |f[i]| <= 1 and g[j] with 1, then per term f's roundings, the product, n - 1 additions, the subtraction and the division."""
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    w = np.maximum(p, 0.0)
    s, f = w.sum(), w / w.sum()
    eg = bound_g(gmag, npix, C)
    t_mag = float((f * np.abs(g)).sum())
    out = np.zeros(n)
    for j in range(n):
        prop = eg[j] + float((f * eg).sum())
        arith = (k_weight(n) + 1 + (n - 1) + 2 + 1) * U32 * (abs(g[j]) + t_mag)
        out[j] = (prop + arith) / s * (1 + 4 * U32) if p[j] > 0 else 0.0
    return out


# ---- state ------------------------------------------------------------------------------------------------------------------------
def fill_state(layout_, seed):
    """``oracle.graph.fill_state`` over ``layout_`` (name -> shape); every ``fusion_weight`` then takes values of its own in
    [0.5, 2): positive (a layer whose weights are all <= 0 computes NaN, by the reference's formula) and unequal."""
    sd = og.fill_state(dict(layout_), int(seed))
    rng = np.random.default_rng(int(seed) + 7919)
    for k in sd:
        if k.endswith("fusion_weight"):
            sd[k] = torch.from_numpy((0.5 + 1.5 * rng.random(tuple(sd[k].shape))).astype(np.float32))
    return sd


def state(G, prefix):
    return fill_state(layout(G, prefix), int(G[f"{prefix}/seed"]))
