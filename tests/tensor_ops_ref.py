"""Float64 CPU references of the csrc/tensor_ops.hip kernels and the per-element comparison rule of tests/test_gpu_tensor_ops.py.
Everything here runs without a GPU; tests/test_host_tensor_ops_ref.py checks these references against ATen / autograd.

Layout: maps are channels-last (N, H, W, C), as the kernels see them.  Inputs are fp16-rounded values held in float64.

The comparison rule:  |got - ref| <= k16 * 2^-11 * |ref| + k32 * 2^-23 * mag + 2^-24
  k16  fp16 roundings on the kernel's path to that output (2^-11: half an fp16 ulp, relative)
  mag  sum of the absolute values of the fp32 terms that were added to produce it (computed by the reference)
  k32  number of those fp32 operations (2^-23: one fp32 ulp, relative -- twice the rounding error, which pays for a fused or
       re-associated form of the same chain)
  2^-24  half the smallest fp16 subnormal step
Where a rounded intermediate is added to something else (ScalSeq's residual, Zoom_cat's max + mean) the fp16 term is written out per
rounding, each with the magnitude it acts on; ``bound`` then takes it ready-made as ``abs16``."""
import torch
import torch.nn.functional as F

EPS16, EPS32, TINY = 2.0 ** -11, 2.0 ** -23, 2.0 ** -24
GAP = 1e-4  # realistic regime: top-two gap of the reference below which fp32 and fp64 may pick another level (~200 fp32 ulps at |z| <= 5.4)


def bound(ref, k16=0, k32=0, mag=None, abs16=None):
    b = torch.full_like(ref, TINY, dtype=torch.float64)
    if k16:
        b = b + k16 * EPS16 * ref.abs()
    if abs16 is not None:
        b = b + EPS16 * abs16
    if k32:
        b = b + k32 * EPS32 * mag
    return b


def check(got, ref, bnd, what="", mask=None):
    """Assert |got - ref| <= bnd per element (``mask``: True where the comparison applies); prints the worst ratio first."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(ref).all()), what
    ratio = (got - ref).abs() / bnd
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    if mask is not None:
        ratio = torch.where(mask, ratio, torch.zeros_like(ratio))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{what}: worst |got - ref| / bound = {worst:.3f} over {ratio.numel()} elements")
    if worst > 1.0:
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements out of bound; worst at {idx}: got "
                             f"{float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} bound {float(bnd.flatten()[i]):.3e}")


def same_bits(got, ref, what=""):
    """Bit equality of two fp16 / integer tensors (NaNs must sit at the same places; their payload is not compared)."""
    got, ref = torch.as_tensor(got).cpu(), torch.as_tensor(ref).cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if got.is_floating_point():
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{what}: NaNs at other places"
        got, ref = torch.nan_to_num(got, nan=0.0), torch.nan_to_num(ref, nan=0.0)
    bad = got != ref
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"


def h16(t):
    """Round to fp16, keep as float64."""
    return t.half().double()


# ---- element-wise ------------------------------------------------------------------------------------------------------------------
def add_f32_chain(a, b, c=None):
    """dy_add in IEEE arithmetic: ((a + b) in fp32 -> fp16) + c in fp32 -> fp16.  fp16 tensors in, fp16 tensor out."""
    v = (a.float() + b.float()).half()
    if c is not None:
        v = (v.float() + c.float()).half()
    return v


def upsample2x(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def block_sum(x, s):
    """Sum over the s x s blocks of a (N, H, W, C) map."""
    N, H, W, C = x.shape
    return x.reshape(N, H // s, s, W // s, s, C).sum((2, 4))


def upsample2x_backward(dy, old=None):
    """(ref, mag): 2x2 sums of dy (+ the old content when accumulating)."""
    ref, mag = block_sum(dy, 2), block_sum(dy.abs(), 2)
    if old is not None:
        ref, mag = ref + old, mag + old.abs()
    return ref, mag


# ---- 5x5 / stride 1 / pad 2 max-pool ------------------------------------------------------------------------------------------------
def maxpool5(x):
    """(y, code, flat): ATen's CPU max_pool2d on the float64 map; code = dy * 5 + dx of the arg-max inside its window (the kernel's
    uint8 map), flat = ATen's index iy * W + ix.  ATen keeps the first maximum and the last NaN of the row-major window scan."""
    N, H, W, C = x.shape
    y, flat = F.max_pool2d(x.permute(0, 3, 1, 2).contiguous(), 5, 1, 2, return_indices=True)
    iy, ix = flat // W, flat % W
    oy = torch.arange(H).view(1, 1, H, 1)
    ox = torch.arange(W).view(1, 1, 1, W)
    code = (iy - oy + 2) * 5 + (ix - ox + 2)
    assert int(code.min()) >= 0 and int(code.max()) <= 24
    return y.permute(0, 2, 3, 1).contiguous(), code.permute(0, 2, 3, 1).to(torch.uint8).contiguous(), flat.permute(0, 2, 3, 1).contiguous()


def maxpool5_backward(dy, flat, old=None):
    """(ref, mag): dy scattered to the arg-max ``flat`` (N, H, W, C) of its window (+ the old content when accumulating)."""
    N, H, W, C = dy.shape
    idx = flat.reshape(N, H * W, C)
    ref = torch.zeros(N, H * W, C, dtype=torch.float64).scatter_add_(1, idx, dy.reshape(N, H * W, C))
    mag = torch.zeros(N, H * W, C, dtype=torch.float64).scatter_add_(1, idx, dy.abs().reshape(N, H * W, C))
    ref, mag = ref.view(N, H, W, C), mag.view(N, H, W, C)
    if old is not None:
        ref, mag = ref + old, mag + old.abs()
    return ref, mag


def scatter_bound(b, flat):
    """A per-element error bound on dy carried through maxpool5_backward (linear, so the bounds scatter like the values)."""
    N, H, W, C = b.shape
    return torch.zeros(N, H * W, C, dtype=torch.float64).scatter_add_(1, flat.reshape(N, H * W, C), b.reshape(N, H * W, C)).view(N, H, W, C)


# ---- Zoom_cat's fine branch ---------------------------------------------------------------------------------------------------------
def zoom_pool(x):
    """(y, mean): adaptive_max_pool2d + adaptive_avg_pool2d to half size."""
    N, H2, W2, C = x.shape
    xc = x.permute(0, 3, 1, 2)
    mx = F.adaptive_max_pool2d(xc, (H2 // 2, W2 // 2))
    mean = F.adaptive_avg_pool2d(xc, (H2 // 2, W2 // 2))
    return (mx + mean).permute(0, 2, 3, 1).contiguous(), mean.permute(0, 2, 3, 1).contiguous()


def zoom_pool_backward(x, dy, old=None):
    """(ref, mag) by float64 autograd of the same expression (the first arg-max takes a tie)."""
    N, H2, W2, C = x.shape
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.adaptive_max_pool2d(xr, (H2 // 2, W2 // 2)) + F.adaptive_avg_pool2d(xr, (H2 // 2, W2 // 2))
    y.backward(dy.permute(0, 3, 1, 2))
    ref = xr.grad.permute(0, 2, 3, 1).contiguous()
    mag = ref.abs()
    if old is not None:
        ref, mag = ref + old, mag + old.abs()
    return ref, mag


# ---- ScalSeq tail --------------------------------------------------------------------------------------------------------------------
def leaky(z):
    return torch.where(z > 0, z, 0.1 * z)


def scalseq_levels(r, coef):
    """(z, pre, mag): z[l] = leaky_0.1(up(r_l) * coef[0] + coef[1]) at full resolution, pre[l] the value before the LeakyReLU, mag[l] the
    fp32 terms of it."""
    sc, sh = coef[0].double(), coef[1].double()
    z, pre, mag = [], [], []
    for l, rl in enumerate(r):
        up = rl
        for _ in range(l):
            up = upsample2x(up)
        p = up * sc + sh
        pre.append(p)
        z.append(leaky(p))
        mag.append((up * sc).abs() + sh.abs())
    return z, pre, mag


def scalseq_tail(r, coef, res=None):
    """(y, m, mag): m = the max over the three levels taken with F.max_pool3d over a depth-3 stack (as the reference module does),
    y = m + res.  mag: fp32 terms of the winning (largest-magnitude) level's affine form."""
    z, _, mags = scalseq_levels(r, coef)
    vol = torch.stack(z, 1).permute(0, 4, 1, 2, 3).contiguous()  # (N, C, 3, H, W)
    m = F.max_pool3d(vol, (3, 1, 1)).squeeze(2).permute(0, 2, 3, 1).contiguous()
    mag = torch.stack(mags, 0).amax(0)
    return (m if res is None else m + res), m, mag


def scalseq_argmax(z):
    """First maximum over the levels, and the gap between the two largest values."""
    am = torch.zeros(z[0].shape, dtype=torch.long)
    zb = z[0]
    for l in (1, 2):
        am = torch.where(z[l] > zb, torch.full_like(am, l), am)
        zb = torch.maximum(zb, z[l])
    top2 = torch.stack(z, 0).sort(0).values
    return am, zb, top2[2] - top2[1]


def scalseq_backward(r, dy, coef, bwdcoef=None):
    """Closed form of the tail's backward.  Returns a dict:
    S1, S2 (C,): sum_l sum g_l and sum_l sum g_l * xhat_l over the up-sampled volume, with magS1 / magS2 (sums of absolute terms);
    dr[l], magdr[l] when ``bwdcoef`` is given: coef[0] * (sum_block g_l - 4^l bwdcoef[0] - 4^l xhat_l bwdcoef[1]);
    gap: top-two gap per full-resolution position, xhatmax: max |xhat| over the levels."""
    sc, mean, inv = coef[0].double(), coef[2].double(), coef[3].double()
    z, _, _ = scalseq_levels(r, coef)
    am, zb, gap = scalseq_argmax(z)
    gg = dy * torch.where(zb > 0, 1.0, 0.1)
    out = dict(gap=gap, am=am, S1=0.0, S2=0.0, magS1=0.0, magS2=0.0, dr=[], magdr=[], xhatmax=0.0)
    for l in range(3):
        s = 1 << l
        gl = torch.where(am == l, gg, torch.zeros_like(gg))
        G, Ga = block_sum(gl, s), block_sum(gl.abs(), s)
        xhat = (r[l] - mean) * inv
        xmag = (r[l].abs() + mean.abs()) * inv.abs()  # the terms of the subtraction, scaled
        out["xhatmax"] = max(out["xhatmax"], float(xhat.abs().max()))
        out["S1"] = out["S1"] + G.sum((0, 1, 2))
        out["S2"] = out["S2"] + (G * xhat).sum((0, 1, 2))
        out["magS1"] = out["magS1"] + Ga.sum((0, 1, 2))
        out["magS2"] = out["magS2"] + (Ga * xmag).sum((0, 1, 2))
        if bwdcoef is not None:
            b0, b1 = bwdcoef[0].double(), bwdcoef[1].double()
            cnt = float(s * s)
            out["dr"].append(sc * (G - cnt * b0 - cnt * xhat * b1))
            out["magdr"].append(sc.abs() * (Ga + cnt * b0.abs() + cnt * xmag * b1.abs()))
    return out


def scalseq_exempt(gap):
    """Per level: True where a level-l pixel covers a position whose top-two gap is below GAP."""
    ex = gap < GAP
    return [block_sum(ex.double(), 1 << l) > 0 for l in range(3)]


def scalseq_autograd(r, dy, gamma, beta, eps=1e-3):
    """The reference module's tail in float64 autograd: interpolate(nearest) -> stack -> batch_norm(training) -> leaky_relu(0.1) ->
    max_pool3d over the depth.  Returns (r grads, gamma.grad, beta.grad, coef (4, C) from the batch statistics)."""
    rs = [t.clone().permute(0, 3, 1, 2).requires_grad_(True) for t in r]
    g, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    H, W = rs[0].shape[2:]
    vol = torch.stack([rs[0], F.interpolate(rs[1], size=(H, W), mode="nearest"), F.interpolate(rs[2], size=(H, W), mode="nearest")], 2)
    y = F.max_pool3d(F.leaky_relu(F.batch_norm(vol, None, None, g, b, True, 0.0, eps), 0.1), (3, 1, 1)).squeeze(2)
    y.backward(dy.permute(0, 3, 1, 2))
    v = vol.detach()
    mean, var = v.mean((0, 2, 3, 4)), v.var((0, 2, 3, 4), unbiased=False)
    inv = (var + eps).rsqrt()
    coef = torch.stack([gamma * inv, beta - mean * gamma * inv, mean, inv])
    return [t.grad.permute(0, 2, 3, 1).contiguous() for t in rs], g.grad, b.grad, coef


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn16(g, *shape):
    return h16(torch.randn(*shape, generator=g, dtype=torch.float64))


def grid16(g, *shape):
    """Values on the grid k/4 in [-2, 2]: products with the dyadic scales below are exact in fp32, ties are exact."""
    return torch.randint(-8, 9, shape, generator=g).double() / 4


def coarse16(g, *shape):
    """round(2x)/2 of N(0,1): a coarse grid that makes neighbouring pixels tie."""
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * 2).round() / 2 + 0.0


def scalseq_inputs(seed, N, H, W, C, exact):
    """r (3 levels), dy, coef (4, C) fp32.  exact: inputs on the k/4 grid, scale in {0.5, 1, 2, -1}, shift a multiple of 1/4;
    realistic: N(0,1) inputs, |scale| in [0.5, 1.5] with every third channel negative, shift ~ 0.3 N(0,1).  coef[2:4] are random."""
    g = gen(seed)
    if exact:
        r = [grid16(g, N, H >> l, W >> l, C) for l in range(3)]
        sc = torch.tensor([0.5, 1.0, 2.0, -1.0], dtype=torch.float64)[torch.randint(0, 4, (C,), generator=g)]
        sh = torch.randint(-4, 5, (C,), generator=g).double() / 4
    else:
        r = [randn16(g, N, H >> l, W >> l, C) for l in range(3)]
        sc = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
        sc[2::3] *= -1
        sh = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    dy = randn16(g, N, H, W, C)
    mean = 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    inv = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    coef = torch.stack([sc, sh, mean, inv]).float()  # what the kernel reads; the reference takes the same fp32 values
    return r, dy, coef


# ---- the cases of section "ScalSeq" (N, H, W, C) ---------------------------------------------------------------------------------------
SCALSEQ_FWD_SHAPES = [(2, 4, 4, 8), (2, 8, 12, 24), (1, 8, 8, 136)]
SCALSEQ_BWD_SHAPES = [  # shape, the kernel dy_scalseq_tail_backward_all takes for it
    ((2, 8, 64, 8), "cols"),    # cpp = 1: 64 columns per wave
    ((2, 8, 32, 16), "cols"),
    ((2, 8, 16, 32), "cols"),   # cpp = 4: the DPP path
    ((2, 8, 48, 32), "cols"),   # three chunks per row
    ((2, 8, 16, 64), "cols"),
    ((2, 4, 4, 128), "cols"),   # cpp = 16: one quad per wave, 1x1 level-2 map
    ((2, 8, 12, 24), "block"),  # cpp = 3 leaves thread 255 idle
    ((2, 8, 24, 32), "block"),  # W is no multiple of 16
    ((1, 8, 8, 136), "block"),  # cpp = 17
    ((2, 8, 32, 8), "block"),   # cpp = 1 but W is no multiple of 64
]
EXEMPT_CAPS = (0.005, 0.01, 0.03)  # share of level-0 / 1 / 2 pixels the realistic regime may exempt


def scalseq_kernel(W, C):
    """The selection rule of dy_scalseq_tail_backward_all, recomputed: cols when cpp = C / 8 divides 64, cpp <= 16 and W is a multiple of
    64 / cpp columns; the block-per-lane kernel otherwise."""
    cpp = C // 8
    return "cols" if cpp <= 16 and 64 % cpp == 0 and W % (64 // cpp) == 0 else "block"


def seed_of(shape, exact):
    N, H, W, C = shape
    return 1000 * H + 10 * W + C + (7 if exact else 0)
