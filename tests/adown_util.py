"""Helpers of the ADown tests: the case lists, the seeded inputs of the kernel cases, the deterministic state the fixtures were
taken with (the generator tests/golden/make_adown_golden.py and the tests call the same functions, so no weights are stored) and an
fp32 emulation of the summation orders csrc/adown.hip documents.  The oracle does not know ADown, so state layouts come from the
name / shape lists the generator stored."""
import os

import numpy as np
import torch

from carafe_util import batch, carafe_state as fill_state, layout, state  # noqa: F401  (the same fixture conventions)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CKPT = os.path.join(GOLDEN, "ref_ckpt_adown.pt")
MODEL = "yolov8n-ASF-P2P2-ADown"
ADOWN_LAYERS = (1, 3, 5, 18, 21)
ADOWN_WIDTHS = {1: (16, 32), 3: (32, 64), 5: (64, 128), 18: (32, 32), 21: (64, 64)}  # scale n: (c1, c2)
BATCH = 2
STEP_LR, STEP_MOM = 0.01, 0.9  # the optimizer step of the graph fixture (tests/golden/make_adown_golden.py)
# (N, H, W, C): one average and one window; a two-pixel column; odd both ways (no zero border); even both ways (a zero border row
# and column); three granules per half; several workgroups (the grid-stride loop starts beyond 2^21 work items: the GPU test repeats
# this case along N to get there).
KERNEL_CASES = [(1, 2, 2, 16), (1, 3, 2, 16), (2, 7, 9, 16), (2, 8, 8, 32), (1, 10, 6, 48), (2, 18, 66, 64)]
SLICED = (2, 8, 8, 32)    # also run with every operand at pitch C + 8, channel offset 8
TIE_CASES = [(2, 7, 9, 16), (2, 8, 8, 32), (1, 10, 6, 48)]
# name -> (c1, c2, H, W): an odd map at the narrowest width (8-channel halves, the scale-n row 1), an even map that narrows, a map
# with one even and one odd side at the widest row of the graph
MODULE_CASES = {"ad_16_32_odd": (16, 32, 9, 7), "ad_32_16_even": (32, 16, 8, 8), "ad_64_128_mixed": (64, 128, 6, 5)}
K32_FIRST, K32_SECOND = 2, 2  # half the additions on the longest path of the two backward gathers: 4 each (tests/test_gpu_adown.py)


def case_id(g):
    return "x".join(str(v) for v in g)


def exact_inputs(geom, seed):
    """x, da, dp: multiples of 2^-6 with |v| < 4.  Every average is then an fp16 number and every gradient sum is exact in fp32."""
    N, H, W, C = geom
    rng = np.random.default_rng(seed)
    draw = lambda *s: torch.from_numpy(rng.integers(-255, 256, size=s).astype(np.float64) / 64.0)  # noqa: E731
    return draw(N, H, W, C), draw(N, 2 * (H // 2), 2 * (W // 2), C // 2), draw(N, H // 2, W // 2, C // 2)


def tie_inputs(geom, seed=0):
    """x: multiples of 1/2 in [-2, 2]: fp16 averages tie often; gradients as ``exact_inputs``."""
    N, H, W, C = geom
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.integers(-4, 5, size=(N, H, W, C)).astype(np.float64) / 2.0)
    _, da, dp = exact_inputs(geom, seed + 1)
    return x, da, dp


def normal_inputs(geom, seed):
    """x, da, dp: standard normal values rounded to fp16 (held in float64)."""
    N, H, W, C = geom
    rng = np.random.default_rng(seed)
    draw = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float16).astype(np.float64))  # noqa: E731
    return draw(N, H, W, C), draw(N, 2 * (H // 2), 2 * (W // 2), C // 2), draw(N, H // 2, W // 2, C // 2)


def check(what, got, ref, mag, k32):
    """|got - ref| <= 2^-11 |ref| + k32 2^-23 mag + 2^-24 on EVERY element; prints the worst ratio."""
    got, ref, mag = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double(), torch.as_tensor(mag).double()
    assert got.shape == ref.shape == mag.shape, (what, got.shape, ref.shape, mag.shape)
    bound = 2.0 ** -11 * ref.abs() + k32 * 2.0 ** -23 * mag + 2.0 ** -24
    err = (got - ref).abs()
    worst = float((err / bound).max())
    print(f"{what}: k32 {k32}: max err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, f"{what}: {int((err > bound).sum())} of {err.numel()} elements beyond the bound"


def backward_k32(C):
    """(C,) the k32 of every channel of dx: the first half, then the second."""
    return torch.cat([torch.full((C // 2,), float(K32_FIRST)), torch.full((C // 2,), float(K32_SECOND))]).double()


# ---- fp32 emulation of the kernel's orders (numpy float32: one rounding per operation) ------------------------------------------
def _f32(t):
    return np.asarray(t, dtype=np.float64).astype(np.float32)


def emulate_forward(x):
    """``a`` and ``p`` as adown_pool_kernel forms them: ((x00 + x01) + x10) + x11 in fp32, times 0.25, one fp16 rounding; the max
    compares those fp16 values -> (a, p) float64 holding fp16 values."""
    x = _f32(x)
    N, H, W, C = x.shape
    Ho, Wo, c = H // 2, W // 2, C // 2
    s = ((x[:, :-1, :-1] + x[:, :-1, 1:]) + x[:, 1:, :-1]) + x[:, 1:, 1:]
    av = (s * np.float32(0.25)).astype(np.float16).astype(np.float64)
    a = np.zeros((N, 2 * Ho, 2 * Wo, c))
    a[:, :H - 1, :W - 1] = av[..., :c]
    pad = np.full((N, 2 * Ho + 2, 2 * Wo + 2, c), -np.inf)
    pad[:, 1:H, 1:W] = av[..., c:]
    p = np.max(np.stack([pad[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] for ky in range(3) for kx in range(3)]), 0)
    return torch.from_numpy(a), torch.from_numpy(p)


def emulate_backward(da, dp, arg, H, W, old=None):
    """dx as adown_pool_bwd_kernel forms it: first half: per pixel the da of the averages (y-1, x-1), (y-1, x), (y, x-1), (y, x) in
    that order; second half: the dp of the windows (oy-, ox-), (oy-, ox+), (oy+, ox-), (oy+, ox+) in that order, each where its
    recorded tap names one of those averages; one running fp32 sum, times 0.25, the stored value added in fp32 when accumulating, one
    fp16 rounding."""
    da, dp, arg = _f32(da), _f32(dp), np.asarray(arg)
    N, Ho, Wo, c = dp.shape
    out = np.zeros((N, H, W, 2 * c), dtype=np.float64)
    for y in range(H):
        for x in range(W):
            s1, s2 = np.zeros((N, c), dtype=np.float32), np.zeros((N, c), dtype=np.float32)
            wyh, wxh = (y + 1) >> 1, (x + 1) >> 1
            mine = [(y - 1 + (k >> 1), x - 1 + (k & 1)) for k in range(4)]
            mine = [(ay, ax) for ay, ax in mine if 0 <= ay < H - 1 and 0 <= ax < W - 1]
            for ay, ax in mine:
                s1 = s1 + da[:, ay, ax]
            for w in range(4):
                wy, wx = wyh - 1 + (w >> 1), wxh - 1 + (w & 1)
                if not (0 <= wy < Ho and 0 <= wx < Wo):
                    continue
                codes = [3 * (ay + 1 - 2 * wy) + (ax + 1 - 2 * wx) for ay, ax in mine if 0 <= ay + 1 - 2 * wy < 3 and 0 <= ax + 1 - 2 * wx < 3]
                if codes:
                    s2 = s2 + np.where(np.isin(arg[:, wy, wx], codes), dp[:, wy, wx], np.float32(0))
            r = np.concatenate([s1, s2], -1) * np.float32(0.25)
            if old is not None:
                r = _f32(old[:, y, x]) + r
            out[:, y, x] = r.astype(np.float16).astype(np.float64)
    return torch.from_numpy(out)
