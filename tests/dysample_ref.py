"""Float64 CPU restatement of DySample's sampling stage (style 'lp', no dyscope), written from the layer's description, with the
magnitudes the per-element bounds of tests/test_gpu_dysample.py need.  No GPU, no reference code.

Layout (the kernels' own): ``x`` (N, H, W, C); ``off`` the RAW output of the 1x1 offset convolution, (N, H, W, 2 G s^2), channel
d G s^2 + g s^2 + i s + j = coordinate d (0 = x, 1 = y) of group g at sub-position (row i, column j); ``y`` / ``dy`` (N, sH, sW, C).
Output pixel (s h + i, s w + j) of group g reads x at px = clamp(w + 0.25 o_x + t[j], 0, W-1), py = clamp(h + 0.25 o_y + t[i], 0, H-1),
t[k] = (k - (s-1)/2) / s, bilinearly; a neighbour index beyond the last row / column carries weight 0.  The coordinate gradient is 0
where the unclamped position is at or beyond 0 / size-1 (grid_sample's border rule)."""
import torch

F64 = torch.float64


def init_pos(s, G):
    """(2 G s^2,) float64: t[j] for d = 0, t[i] for d = 1."""
    t = (torch.arange(s, dtype=F64) - (s - 1) / 2) / s
    tx, ty = t.view(1, s).expand(s, s), t.view(s, 1).expand(s, s)
    return torch.stack([tx, ty]).reshape(2, 1, s * s).repeat(1, G, 1).reshape(-1)


def positions(off, s, G):
    """Unclamped sampling positions (ux, uy), each (N, H, W, G, s, s) float64, from the raw offsets."""
    N, H, W, _ = off.shape
    o = off.to(F64) * 0.25 + init_pos(s, G)
    o = o.view(N, H, W, 2, G, s, s)
    ux = o[:, :, :, 0] + torch.arange(W, dtype=F64).view(1, 1, W, 1, 1, 1)
    uy = o[:, :, :, 1] + torch.arange(H, dtype=F64).view(1, H, 1, 1, 1, 1)
    return ux, uy


def _geometry(off, s, G):
    N, H, W, _ = off.shape
    ux, uy = positions(off, s, G)
    px, py = ux.clamp(0, W - 1), uy.clamp(0, H - 1)
    x0, y0 = px.floor(), py.floor()
    fx, fy = px - x0, py - y0
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)  # held inside the map: its weight is 0 whenever it had to be
    in_x, in_y = ((ux > 0) & (ux < W - 1)).to(F64), ((uy > 0) & (uy < H - 1)).to(F64)
    return (x0, x1, y0, y1), (fx, fy), (in_x, in_y)


def _corners(x, idx, G):
    """x (N, H, W, C) -> the four corner values, each (N, H, W, G, s, s, C/G)."""
    N, H, W, C = x.shape
    x0, x1, y0, y1 = idx
    xg = x.to(F64).reshape(N, H * W, G, C // G)
    n = torch.arange(N).view(N, 1, 1, 1, 1, 1)
    g = torch.arange(G).view(1, 1, 1, G, 1, 1)
    return [xg[n, yy * W + xx, g] for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))]


def _to_out(v, s):
    """(N, H, W, G, s, s, cpg) -> (N, sH, sW, C)"""
    N, H, W, G, _, _, cpg = v.shape
    return v.permute(0, 1, 4, 2, 5, 3, 6).reshape(N, s * H, s * W, G * cpg)


def _from_out(t, s, G):
    """(N, sH, sW, C) -> (N, H, W, G, s, s, cpg)"""
    N, sH, sW, C = t.shape
    return t.to(F64).reshape(N, sH // s, s, sW // s, s, G, C // G).permute(0, 1, 3, 5, 2, 4, 6)


def forward(x, off, s, G):
    """-> dict: ``y`` (N, sH, sW, C); ``mag`` the sum of |weight * corner| per output; ``dcoord`` |dy/dpx| + |dy/dpy| per output."""
    idx, (fx, fy), _ = _geometry(off, s, G)
    v00, v01, v10, v11 = _corners(x, idx, G)
    fx, fy = fx.unsqueeze(-1), fy.unsqueeze(-1)
    ws = ((1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx)
    y = sum(w * v for w, v in zip(ws, (v00, v01, v10, v11)))
    mag = sum(w * v.abs() for w, v in zip(ws, (v00, v01, v10, v11)))
    dcoord = ((1 - fy) * (v01 - v00) + fy * (v11 - v10)).abs() + ((1 - fx) * (v10 - v00) + fx * (v11 - v01)).abs()
    return dict(y=_to_out(y, s), mag=_to_out(mag, s), dcoord=_to_out(dcoord, s))


def backward(x, off, dy, s, G):
    """-> dict: ``dx`` (N, H, W, C) with ``dx_mag`` (sum of |terms|), ``dx_dcoord`` (sum of |dy| * |d weight / d coordinate|) and
    ``dx_terms`` (number of non-zero terms per element); ``doff`` (N, H, W, 2 G s^2), the gradient w.r.t. the RAW offsets, with
    ``doff_mag`` and ``doff_dcoord``."""
    N, H, W, C = x.shape
    cpg = C // G
    idx, (fx, fy), (in_x, in_y) = _geometry(off, s, G)
    x0, x1, y0, y1 = idx
    v00, v01, v10, v11 = _corners(x, idx, G)
    g = _from_out(dy, s, G)
    fxu, fyu = fx.unsqueeze(-1), fy.unsqueeze(-1)
    # offsets: d value / d px = (1 - fy)(v01 - v00) + fy (v11 - v10), d value / d py likewise; 0.25 from the raw offset's scale
    sx = (g * ((1 - fyu) * (v01 - v00) + fyu * (v11 - v10))).sum(-1)
    sy = (g * ((1 - fxu) * (v10 - v00) + fxu * (v11 - v01))).sum(-1)
    mx = (g.abs() * ((1 - fyu) * (v01.abs() + v00.abs()) + fyu * (v11.abs() + v10.abs()))).sum(-1)
    my = (g.abs() * ((1 - fxu) * (v10.abs() + v00.abs()) + fxu * (v11.abs() + v01.abs()))).sum(-1)
    cross = (g.abs() * (v11 - v10 - v01 + v00).abs()).sum(-1)  # |d/d(other coordinate)| of either sum
    doff = torch.stack([0.25 * in_x * sx, 0.25 * in_y * sy], 3).reshape(N, H, W, -1)
    doff_mag = torch.stack([0.25 * mx, 0.25 * my], 3).reshape(N, H, W, -1)
    doff_dcoord = torch.stack([0.25 * cross, 0.25 * cross], 3).reshape(N, H, W, -1)
    # input: every corner receives weight * dy
    n = torch.arange(N).view(N, 1, 1, 1, 1, 1)
    gi = torch.arange(G).view(1, 1, 1, G, 1, 1)
    dx, dmag, dco, cnt = (torch.zeros(N * H * W * G, cpg, dtype=F64) for _ in range(4))
    for yy, xx, wy, wx in ((y0, x0, 1 - fy, 1 - fx), (y0, x1, 1 - fy, fx), (y1, x0, fy, 1 - fx), (y1, x1, fy, fx)):
        flat = (((n * H + yy) * W + xx) * G + gi).reshape(-1)
        w = (wy * wx).unsqueeze(-1)
        dx.index_add_(0, flat, (w * g).reshape(-1, cpg))
        dmag.index_add_(0, flat, (w * g.abs()).reshape(-1, cpg))
        dco.index_add_(0, flat, ((wy + wx).unsqueeze(-1) * g.abs()).reshape(-1, cpg))
        cnt.index_add_(0, flat, ((w != 0).to(F64) * torch.ones_like(g)).reshape(-1, cpg))
    shape = (N, H, W, C)
    return dict(dx=dx.reshape(shape), dx_mag=dmag.reshape(shape), dx_dcoord=dco.reshape(shape), dx_terms=cnt.reshape(shape),
                doff=doff, doff_mag=doff_mag, doff_dcoord=doff_dcoord)


def offset_conv(x, weight, bias):
    """The 1x1 offset convolution on NHWC: x (N, H, W, C), weight (Co, C[, 1, 1]), bias (Co,) -> (N, H, W, Co)."""
    return x @ weight.reshape(weight.shape[0], -1).t() + bias


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()
