"""Float64 numpy restatement of SimAM (reference nn/extra_modules/attention.py:69-77) and of its backward, written from the formulas,
layout-free: the plane axes are named by the caller (``axes``; (1, 2) for an (N, H, W, C) array, (2, 3) for (N, C, H, W)).

Per image and channel over the M values of the plane, n = M - 1, lam = e_lambda:

    mu = mean(x)    d = x - mu    S = sum(d^2)    D = 4 (S / n + lam)    e = d^2 / D + 0.5    a = sigmoid(e)    y = x a

and with g = dy:

    q = g x a (1 - a)    T = sum(q d^2)    U = sum(q d)    dx = g a + (2 d / D) (q - 4 T / (n D)) - 2 U / (M D)

Derivation of the backward.  y = x a(e), e = d^2 / D + 1/2, and with a' = a (1 - a), q = g x a' is dL/de.  e depends on x_k through
d_j = x_j - mu (dd_j/dx_k = delta_jk - 1/M) and through D = 4 (sum_j d_j^2 / n + lam) (dD/dx_k = 8 d_k / n, because sum_j d_j = 0):
de_j/dx_k = (2 d_j / D)(delta_jk - 1/M) - (d_j^2 / D^2)(8 d_k / n).  Summing q_j de_j/dx_k over j gives
(2 d_k / D) q_k - 2 U / (M D) - (8 d_k / (n D^2)) T, i.e. the formula above; tests/test_host_simam.py checks it against autograd.
A plane of ONE pixel has n = 0 and S = 0: S / n is 0 / 0, so y and dx are NaN, as the reference computes them.

The bounds of the GPU tests are counted here, from the arithmetic csrc/simam.hip states, BEFORE any GPU run; nothing is taken from
the kernel's output.  u = 2^-24 is the unit round-off of fp32 (half an ulp, relative), U16 = 2^-11 that of fp16.
The kernel: sums of x and x^2 in fp64 (every term exact, the sums to ~M 2^-53 relative: neglected against u), mu and invD = 1 / D each
ONE rounding of the fp64 value to fp32; then per element in fp32
    d = x - mu                      |err d|  <= u (|mu| + |d|)                     =: ed     (mu's rounding + the subtraction's)
    e = fma(d * d, invD, 0.5)       |err e|  <= (2 |d| ed + 3 u d^2) / D + u e     =: ee     (d's error twice, the square's, invD's and
                                                                                              the fma's roundings)
    a = 1 / (1 + exp(-e))           |err a|  <= a (1 - a) (ee + 8 u) + 2 u a       =: ea     (the fast exponential to 4 ulp = 8 u, the
                                                                                              addition and the division one rounding each)
    y = fp16(x * a)                 |err y|  <= U16 |y| + 2^-25 + |x| ea + u |y|              (the product's rounding, then the one
                                                                                              fp16 rounding; 2^-25: half the subnormal spacing)
    p = a - a * a                   |err p|  <= ea + 2 u a (1 - a) + u a^2         =: ep     (|1 - 2a| <= 1)
    q = (g * x) * p                 |err q|  <= |g x| ep + 2 u |q|                 =: eq
    T += fp64(q * d * d), U += fp64(q * d): per term  eq d^2 + |q| (2 |d| ed + 2 u d^2)  and  eq |d| + |q| ed + u |q d|, summed: eT, eU
    k1 = fp32(4 T invD / n)         |err k1| <= 4 eT / (n D) + 2 u |k1|            =: ek1    (invD's rounding and k1's own)
    k2 = fp32(2 U invD / M)         |err k2| <= 2 eU / (M D) + 2 u |k2|            =: ek2
    dx = fp16(fma(g, a, fma((2 d) * invD, q - k1, -k2)))
         with w = 2 d / D:  |err w| <= 2 ed / D + 2 u |w|,  |err (q - k1)| <= eq + ek1 + u |q - k1|
         |err dx| <= U16 |dx| + 2^-25 + |g| ea + |err w| (|q| + |k1|) + |w| (eq + ek1 + u (|q| + |k1|)) + ek2
                     + 2 u (|g a| + |w| (|q| + |k1|) + |k2|)                                  (the two fma roundings over the magnitudes)
    accumulate: fp16(old + dx): the bound with U16 |old + dx| and + u (|old| + |dx|) for the fp32 addition.
``bounds`` returns these per element, times SLACK = 2 for the second-order terms dropped above."""
import numpy as np

U16, U32 = 2.0 ** -11, 2.0 ** -24
SLACK = 2.0


def _sig(e):
    return 1.0 / (1.0 + np.exp(-e))


def forward(x, lam=1e-4, axes=(1, 2)):
    """-> dict(y, a, d, mu, D): float64; mu and D keep the reduced axes (size 1)."""
    x = np.asarray(x, dtype=np.float64)
    M = int(np.prod([x.shape[a] for a in axes]))
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = x.mean(axis=axes, keepdims=True)
        d = x - mu
        S = (d * d).sum(axis=axes, keepdims=True)
        D = 4.0 * (S / np.float64(M - 1) + lam)
        e = d * d / D + 0.5
        a = _sig(e)
    return dict(y=x * a, a=a, d=d, e=e, mu=mu, D=D, M=M)


def backward(x, g, lam=1e-4, axes=(1, 2)):
    """-> dict(dx, q, T, U, k1, k2) on top of forward()'s entries."""
    f = forward(x, lam, axes)
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    a, d, D, M = f["a"], f["d"], f["D"], f["M"]
    with np.errstate(invalid="ignore", divide="ignore"):
        q = g * x * a * (1.0 - a)
        T = (q * d * d).sum(axis=axes, keepdims=True)
        U = (q * d).sum(axis=axes, keepdims=True)
        k1 = 4.0 * T / (np.float64(M - 1) * D)
        k2 = 2.0 * U / (M * D)
        dx = g * a + (2.0 * d / D) * (q - k1) - k2
    return dict(f, dx=dx, q=q, T=T, U=U, k1=k1, k2=k2)


def stats(x, lam=1e-4, axes=(1, 2)):
    """(mu, 1 / D) per (image, channel) as the kernel leaves them, rounded to fp32 (held in float64), reduced axes dropped."""
    f = forward(x, lam, axes)
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = 1.0 / f["D"]
    r32 = lambda t: np.squeeze(t, axis=axes).astype(np.float32).astype(np.float64)  # noqa: E731
    return r32(f["mu"]), r32(inv)


def bounds(x, g=None, lam=1e-4, axes=(1, 2), old=None):
    """Per-element bounds (docstring) -> dict(y[, dx]) plus the magnitudes they scale with (``mag_y`` = |x|, ``mag_dx`` = the sum of
    the absolute values of dx's three terms)."""
    x = np.asarray(x, dtype=np.float64)
    b = backward(x, np.zeros_like(x) if g is None else g, lam, axes)
    a, d, D, M, mu, e = b["a"], b["d"], b["D"], b["M"], b["mu"], b["e"]
    u = U32
    ed = u * (np.abs(mu) + np.abs(d))
    ee = (2 * np.abs(d) * ed + 3 * u * d * d) / D + u * e
    ea = a * (1 - a) * (ee + 8 * u) + 2 * u * a
    out = dict(y=SLACK * (U16 * np.abs(b["y"]) + 2.0 ** -25 + np.abs(x) * ea + u * np.abs(b["y"])), mag_y=np.abs(x))
    if g is None:
        return out
    g = np.asarray(g, dtype=np.float64)
    q, k1, k2 = b["q"], b["k1"], b["k2"]
    ep = ea + 2 * u * a * (1 - a) + u * a * a
    eq = np.abs(g * x) * ep + 2 * u * np.abs(q)
    eT = (eq * d * d + np.abs(q) * (2 * np.abs(d) * ed + 2 * u * d * d)).sum(axis=axes, keepdims=True)
    eU = (eq * np.abs(d) + np.abs(q) * ed + u * np.abs(q * d)).sum(axis=axes, keepdims=True)
    n = np.float64(M - 1)
    ek1 = 4 * eT / (n * D) + 2 * u * np.abs(k1)
    ek2 = 2 * eU / (M * D) + 2 * u * np.abs(k2)
    w = 2 * d / D
    ew = 2 * ed / D + 2 * u * np.abs(w)
    mag = np.abs(g * a) + np.abs(w) * (np.abs(q) + np.abs(k1)) + np.abs(k2)
    err32 = np.abs(g) * ea + ew * (np.abs(q) + np.abs(k1)) + np.abs(w) * (eq + ek1 + u * (np.abs(q) + np.abs(k1))) + ek2 + 2 * u * mag
    res = b["dx"]
    if old is not None:
        old = np.asarray(old, dtype=np.float64)
        err32 = err32 + u * (np.abs(old) + np.abs(res))
        res = res + old
    out.update(dx=SLACK * (U16 * np.abs(res) + 2.0 ** -25 + err32), mag_dx=mag)
    return out
