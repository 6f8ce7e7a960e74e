"""Float64 NHWC restatement of CARAFE's reassembly stage (reference nn/extra_modules/block.py:3926-3935, k_up = 5, scale = 2) and
its two gradients, with the magnitudes the per-element bounds of tests/test_gpu_carafe.py are stated in.

    p[(h,w),(i,j),k]  = softmax over k = 0..24 of L[4k + 2i + j, h, w]
    Y[c, 2h+i, 2w+j]  = sum_{a,b} p[.., 5a+b] X[c, h+a-2, w+b-2]                          (X = 0 outside the map)
    g[(h,w),(i,j),k]  = sum_c dY[c, 2h+i, 2w+j] X[c, h+a-2, w+b-2]
    dL[4k+2i+j, h, w] = p_k (g_k - sum_m p_m g_m)
    dX[c, h', w']     = sum over base pixels within 2 of (h', w') and (i, j) of p[(h,w),(i,j), 5(h'-h+2)+(w'-w+2)] dY[c, 2h+i, 2w+j]

tests/test_host_carafe.py holds these to the reference's own float64 values (tests/golden/carafe_kernel.npz) at 1e-11."""
import torch
import torch.nn.functional as F

K_UP, SCALE, NLOGIT = 5, 2, 100


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def weights(logits):
    """(N, H, W, >= 100) -> p (N, H, W, 4, 25): [..., 2i + j, k] = softmax_k logits[..., 4k + 2i + j]."""
    N, H, W = logits.shape[:3]
    L = logits[..., :NLOGIT].double().reshape(N, H, W, 25, 4).transpose(-1, -2)
    return torch.softmax(L, -1)


def taps(x):
    """(N, H, W, C) -> (N, H, W, 25, C): [..., 5a + b, :] = x[h + a - 2, w + b - 2] or 0 outside the map."""
    N, H, W, C = x.shape
    xp = F.pad(x.double(), (0, 0, 2, 2, 2, 2))
    return torch.stack([xp[:, a:a + H, b:b + W] for a in range(5) for b in range(5)], 3)


def _to_sub(t):
    """(N, 2H, 2W, C) -> (N, H, W, 4, C) with sub-pixel 2i + j."""
    N, H2, W2, C = t.shape
    return t.reshape(N, H2 // 2, 2, W2 // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H2 // 2, W2 // 2, 4, C)


def _from_sub(t):
    N, H, W, _, C = t.shape
    return t.reshape(N, H, W, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, C)


def _gather_back(dT):
    """Adjoint of ``taps``: (N, H, W, 25, C) -> (N, H, W, C)."""
    N, H, W, _, C = dT.shape
    out = torch.zeros(N, H + 4, W + 4, C, dtype=torch.float64)
    for a in range(5):
        for b in range(5):
            out[:, a:a + H, b:b + W] += dT[:, :, :, 5 * a + b]
    return out[:, 2:-2, 2:-2].contiguous()


def forward(x, logits):
    """-> dict(y, mag): y (N, 2H, 2W, C) float64; mag = sum_k p_k |x_k| per element."""
    p, T = weights(logits), taps(x)
    return dict(y=_from_sub(torch.einsum("nhwqk,nhwkc->nhwqc", p, T)), mag=_from_sub(torch.einsum("nhwqk,nhwkc->nhwqc", p, T.abs())))


def backward(x, logits, dy):
    """-> dict(dlogits (N, H, W, 100), dlogits_mag = p_k (G_k + sum_m p_m G_m) with G_k = sum_c |dy_c x_{k,c}|, dx, dx_mag = sum p |dy|)."""
    N, H, W = logits.shape[:3]
    p, T, d4 = weights(logits), taps(x), _to_sub(dy.double())
    g = torch.einsum("nhwqc,nhwkc->nhwqk", d4, T)
    Gm = torch.einsum("nhwqc,nhwkc->nhwqk", d4.abs(), T.abs())
    dl = p * (g - (p * g).sum(-1, keepdim=True))
    dlm = p * (Gm + (p * Gm).sum(-1, keepdim=True))
    flat = lambda t: t.transpose(-1, -2).reshape(N, H, W, NLOGIT)  # noqa: E731  channel 4k + 2i + j
    dx = _gather_back(torch.einsum("nhwqk,nhwqc->nhwkc", p, d4))
    dxm = _gather_back(torch.einsum("nhwqk,nhwqc->nhwkc", p, d4.abs()))
    return dict(dlogits=flat(dl), dlogits_mag=flat(dlm), dx=dx, dx_mag=dxm)
