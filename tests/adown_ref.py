"""float64 restatement of the two entries of csrc/adown.hip on the operands the kernels see (NHWC; fp16 values held in float64).

forward:  average of every complete 2x2 window -> ONE fp16 rounding -> the first half into a zero-bordered (2Ho, 2Wo) map; the second
          half through a 3x3 s2 p1 max over those fp16 values, out-of-range taps skipped, the FIRST maximum in row-major (ky, kx) order
          winning (a tap replaces the running maximum only when it is greater), its code 3 ky + kx recorded.
backward: the two gathers: 0.25 x the sum of the <= 4 entries of da whose average read the pixel; 0.25 x the sum over those averages
          of the dp of the windows whose recorded tap names them.  ``mag`` is the sum of the absolute values of the same terms.
tests/test_host_adown.py ties both to torch (avg_pool2d / max_pool2d and autograd), tie cases included."""
import numpy as np
import torch


def out_hw(H, W):
    return H // 2, W // 2


def averages(x, round16=True):
    """(N, H, W, C) -> (N, H-1, W-1, C): the float64 sum of the four values (exact for fp16 inputs) times 0.25, rounded once to fp16
    (``round16=False``: left in float64 -- what a value stored with one fp16 rounding is compared with)."""
    x = torch.as_tensor(x).double()
    s = (((x[:, :-1, :-1] + x[:, :-1, 1:]) + x[:, 1:, :-1]) + x[:, 1:, 1:]) * 0.25
    return s.half().double() if round16 else s


def forward(x, round16=True):
    """-> dict(a (N, 2Ho, 2Wo, c) with its zero border, p (N, Ho, Wo, c), arg (N, Ho, Wo, c) uint8, ties: the fraction of windows
    whose maximum is reached by more than one in-range tap).  ``round16=False``: a and p without the fp16 rounding (rounding is
    monotonic: the maximum of the rounded averages is the rounded maximum)."""
    x = torch.as_tensor(x).double()
    N, H, W, C = x.shape
    Ho, Wo = out_hw(H, W)
    c = C // 2
    av = averages(x, round16)
    a = torch.zeros(N, 2 * Ho, 2 * Wo, c, dtype=torch.float64)
    a[:, :H - 1, :W - 1] = av[..., :c]  # (H - 1 <= 2 Ho: an even side leaves one zero row / column, an odd side none)
    pad = torch.full((N, 2 * Ho + 2, 2 * Wo + 2, c), -np.inf, dtype=torch.float64)  # index = average index + 1
    pad[:, 1:H, 1:W] = av[..., c:]
    best = torch.full((N, Ho, Wo, c), -np.inf, dtype=torch.float64)
    arg = torch.zeros(N, Ho, Wo, c, dtype=torch.uint8)
    arg[:, 0, :] += 3  # the first in-range tap of a window on the top / left edge: what a window that nothing wins records
    arg[:, :, 0] += 1
    hits = torch.zeros(N, Ho, Wo, c, dtype=torch.int64)
    taps = [(ky, kx, pad[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]) for ky in range(3) for kx in range(3)]
    for ky, kx, t in taps:
        win = t > best
        best = torch.where(win, t, best)
        arg = torch.where(win, torch.tensor(3 * ky + kx, dtype=torch.uint8), arg)
    for _, _, t in taps:
        hits += (t == best)
    return dict(a=a, p=best, arg=arg, ties=float((hits > 1).double().mean()))


def _spread(g, H, W):
    """dx[y, x] = 0.25 * sum of g[ay, ax] over the averages (ay, ax) in {y-1, y} x {x-1, x} of the (H-1) x (W-1) map -> (dx, mag)."""
    N, c = g.shape[0], g.shape[-1]
    dx = torch.zeros(N, H, W, c, dtype=torch.float64)
    mag = torch.zeros_like(dx)
    for sy in (slice(1, H), slice(0, H - 1)):      # (y-1, .) first: the kernel's order (it does not matter in float64)
        for sx in (slice(1, W), slice(0, W - 1)):
            dx[:, sy, sx] += g
            mag[:, sy, sx] += g.abs()
    return 0.25 * dx, 0.25 * mag


def backward(da, dp, arg, H, W):
    """da (N, 2Ho, 2Wo, c), dp (N, Ho, Wo, c), arg as ``forward`` (or the kernel) recorded it -> dict(dx (N, H, W, 2c), mag)."""
    da, dp = torch.as_tensor(da).double(), torch.as_tensor(dp).double()
    N, Ho, Wo, c = dp.shape
    d1, m1 = _spread(da[:, :H - 1, :W - 1], H, W)
    pad = torch.zeros(N, 2 * Ho + 2, 2 * Wo + 2, c, dtype=torch.float64)  # gradient of the averaged map, index + 1
    pmag = torch.zeros_like(pad)
    for ky in range(3):
        for kx in range(3):
            sel = torch.where(torch.as_tensor(arg) == 3 * ky + kx, dp, torch.zeros_like(dp))
            pad[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] += sel
            pmag[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] += sel.abs()
    d2, _ = _spread(pad[:, 1:H, 1:W], H, W)
    m2, _ = _spread(pmag[:, 1:H, 1:W], H, W)
    return dict(dx=torch.cat([d1, d2], -1), mag=torch.cat([m1, m2], -1))
