"""Helpers of the slim-neck tests (GSConv, GSBottleneck, VoVGSCSP): the case lists, the seeded inputs of the kernel cases and the
deterministic state the fixtures were taken with (the generator tests/golden/make_slimneck_golden.py and the tests call the same
functions, so no weights are stored).  The oracle does not know the blocks, so state layouts come from the name / shape lists the
generator stored."""
import os

import numpy as np
import torch

from carafe_util import batch, carafe_state as fill_state, layout, state  # noqa: F401  (the same fixture conventions)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CKPT = os.path.join(GOLDEN, "ref_ckpt_slimneck.pt")
MODEL = "yolov8n-ASF-P2P2-SlimNeck"
VOV_LAYERS = (12, 17, 20, 23)
GS_LAYERS = (18, 21)
VOV_WIDTHS = {12: (128, 64), 17: (64, 32), 20: (96, 64), 23: (128, 128)}  # scale n: (c1, c2)
GS_WIDTHS = {18: (32, 32), 21: (64, 64)}
BATCH = 2
STEP_LR, STEP_MOM = 0.01, 0.9  # the optimizer step of the graph fixture (tests/golden/make_slimneck_golden.py)
GRID_CAP = 4096 * 256  # work items of one pass of csrc/gsconv.hip's capped grid (GS_MAX_BLOCKS workgroups of 256)
# (N, H, W, c_): one group, which straddles both sources; the straddling group in the middle; whole groups only; two whole groups per
# source; the last one is beyond the grid cap: N H W c_ / 8 > GRID_CAP, so a work item's grid-stride loop runs a second time.
KERNEL_CASES = [(2, 3, 5, 8), (1, 2, 3, 24), (2, 4, 4, 16), (1, 5, 7, 32), (1, 257, 512, 64)]
SLICED = (2, 3, 5, 24)    # run with every operand at pitch C + 8, channel offset 8
BIG = KERNEL_CASES[-1]
assert BIG[0] * BIG[1] * BIG[2] * (BIG[3] // 8) > GRID_CAP
# name -> (class, constructor arguments, H, W) at batch 2: a stride-2 3x3 GSConv on an odd map (8-channel halves: one straddling
# group), a 1x1 GSConv whose halves are one granule, the VoVGSCSP of the graph's row 17 width
MODULE_CASES = {"gs_16_32_k3s2": ("GSConv", (16, 32, 3, 2), 15, 17), "gs_32_16_k1": ("GSConv", (32, 16, 1, 1), 16, 16),
                "vov_32_32": ("VoVGSCSP", (32, 32), 12, 10)}


def case_id(g):
    return "x".join(str(v) for v in g)


def exact_inputs(geom, seed):
    """x1, d, dy and the two stored gradients old1, oldd: multiples of 2^-6 with |v| < 4 -- every sum of two is an fp16 number."""
    N, H, W, c = geom
    rng = np.random.default_rng(seed)
    draw = lambda ch: torch.from_numpy(rng.integers(-255, 256, size=(N, H, W, ch)).astype(np.float32) / 64.0).half()  # noqa: E731
    return dict(x1=draw(c), d=draw(c), dy=draw(2 * c), old1=draw(c), oldd=draw(c))


def normal_inputs(geom, seed):
    """The same operands as standard normal values rounded to fp16."""
    N, H, W, c = geom
    rng = np.random.default_rng(seed)
    draw = lambda ch: torch.from_numpy(rng.standard_normal((N, H, W, ch), dtype=np.float32)).half()  # noqa: E731
    return dict(x1=draw(c), d=draw(c), dy=draw(2 * c), old1=draw(c), oldd=draw(c))
