"""Float64 numpy restatement of Fusion in 'bifpn' mode (BiFPN's fast normalised fusion), written from the formulas alone:

    w = relu(p);  s = sum(w);  f = w / s                 (no epsilon; all weights <= 0: 0 / 0 = NaN)
    y = sum_i f[i] x[i]                                   (operands in list order, all of one shape)
    g[i] = <dy, x[i]>  over every element
    dx[i] = f[i] dy
    dL/dw[j] = (g[j] - sum_i f[i] g[i]) / s
    dL/dp[j] = dL/dw[j] where p[j] > 0, else 0

Layout-free: the operands are arrays of one shape, whatever it is.  ``up2`` restates nn.Upsample(None, 2, 'nearest') for the
operand the kernels read at half resolution (NHWC), ``fold2`` its backward (the 2x2 sums)."""
import numpy as np


def weights(p):
    """-> (f, s, mask): the normalised weights, their sum and where p > 0."""
    p = np.asarray(p, dtype=np.float64)
    w = np.maximum(p, 0.0)
    s = w.sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        f = w / s
    return f, s, p > 0


def forward(xs, p):
    """y in float64 -> dict(y=, mag=): mag = sum_i |f[i] x[i]|, what the rounding bounds scale with."""
    f, _, _ = weights(p)
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    assert len(xs) == len(f) and all(x.shape == xs[0].shape for x in xs)
    y, mag = np.zeros_like(xs[0]), np.zeros_like(xs[0])
    for fi, x in zip(f, xs):
        y = y + fi * x
        mag = mag + np.abs(fi * x)
    return dict(y=y, mag=mag)


def backward(xs, p, dy):
    """-> dict(dx=[...], g=(n,), gmag=(n,), dw=(n,), dp=(n,)): gmag[i] = sum |dy x[i]|."""
    f, s, mask = weights(p)
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    dy = np.asarray(dy, dtype=np.float64)
    g = np.array([float((dy * x).sum()) for x in xs])
    gmag = np.array([float(np.abs(dy * x).sum()) for x in xs])
    with np.errstate(invalid="ignore", divide="ignore"):
        dw = (g - float((f * g).sum())) / s
    return dict(dx=[fi * dy for fi in f], g=g, gmag=gmag, dw=dw, dp=np.where(mask, dw, 0.0))


def up2(x):
    """(N, h, w, C) -> (N, 2h, 2w, C), nearest."""
    return np.repeat(np.repeat(np.asarray(x), 2, axis=1), 2, axis=2)


def fold2(g):
    """The backward of ``up2``: (N, 2h, 2w, C) -> (N, h, w, C), the 2x2 sums."""
    g = np.asarray(g, dtype=np.float64)
    N, H, W, C = g.shape
    return g.reshape(N, H // 2, 2, W // 2, 2, C).sum(axis=(2, 4))
