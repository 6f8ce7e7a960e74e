"""Float64 CPU reference of the tiled convolution kernels of csrc/conv.hip (forward with every epilogue, input gradient, weight
gradient, BatchNorm sums) and the per-element comparison rule of tests/test_gpu_conv_fallback.py.  Everything here runs without a
GPU; tests/test_host_conv_ref.py validates the reference and shows that the bounds have teeth.

Inputs are fp16-exact values held in float64 (weights scaled by (cin ks^2)^-1/2, the bias fp32-exact); tensors are NCHW here and
become channels-last where they meet a kernel's buffer.  The reference is F.conv2d in float64 and its autograd.

The bounds are derived, never measured.  With K accumulated terms and S = the same convolution over absolute values:
  fp32 value   |got - ref| <= K 2^-23 S + 2^-23 |ref| + 2^-24 |bias|
      fp16 x fp16 products are exact in fp32; each of the K accumulation steps is off by at most one fp32 ulp of a partial sum, which
      S bounds, whatever the order or rounding mode of the MFMA (2^-23, not 2^-24); the last fp32 operation (bias or old-value add)
      and the fp32 bias itself take the other two terms
  fp16 store   the fp32 bound of the value before rounding + 2^-11 |ref| (half an fp16 ulp) + 2^-24 (half the subnormal step)
  ACCUM        ref = old + conv with old exact (fp16, or the fp32 content): the same terms.  That is v1 / v3, which add the old value
      to the fp32 accumulator and round once.  The ping-pong and dg2 kernels turn every N-tile through an fp16 LDS scratch before their
      16-byte stores (csrc/conv.hip, ``fast``): their fp16 accumulate is fp16(fp16(conv) + old), the bits of "store, then dy_add", so
      the first rounding adds 2^-11 |conv| + 2^-24 of its own -- which shows where conv and old cancel ("two roundings" below)
  SiLU         + SILU_ULPS 2^-23 |ref| for __expf and the division of common.h's silu_f (tests/tensor_ops_ref.py has no SiLU
      comparison to take a constant from: v_exp_f32 is 1 ulp, the argument scaling by log2(e) costs |z| 2^-24 relative, the division
      and the add one rounding each -- 4 ulps covers |z| <= 12); silu' <= 1.1 on the fp32 bound of z is paid by that bound's factor
      of two over round-to-nearest
  BN sums      v1 / v3 add the fp16 values they stored, in fp32: against the float64 sums of the kernel's OWN stored y and y^2,
      |sum - ref| <= P 2^-23 sum|y| resp. (P + 1) 2^-23 sum y^2 with P = N Ho Wo (y itself is held to the reference by the rules
      above).  The ping-pong kernel's fast epilogue adds its fp32 accumulators instead: its sums are held to the float64 reference
      sums, with the per-element bounds added up on top ("ref" mode).
  dW           K = N Ho Wo, S = sum |x| |dy|; accumulate: ref = old + dW

How to read a failure: ``check`` names the worst element, the bound there and every term of it -- the term that dominates says what
the element was allowed (K 2^-23 S: accumulation; 2^-11 |ref|: the output rounding), and an error many times the whole bound at a
border pixel, one channel group or one image is a wrong tap, mask or index, not rounding."""
import functools
import math
from typing import NamedTuple

import torch
import torch.nn.functional as F

EPS16, EPS32, HALF32, TINY = 2.0 ** -11, 2.0 ** -23, 2.0 ** -24, 2.0 ** -24
SILU_ULPS = 4
CANARY = 777.0
BN_COPIES = 16  # DY_BN_COPIES of include/dealyolo_hip.h (the GPU side asserts that it is)


def round8(c):
    return (c + 7) // 8 * 8


def round16(c):
    return (c + 15) // 16 * 16


class Case(NamedTuple):
    cin: int
    cout: int
    ks: int
    s: int
    kernel: str  # what dy_conv_forward runs for (cin -> cout)
    dgrad: str   # the base family of the input gradient (round8(cout) -> cin, stride 1; dil = s)
    maps: tuple  # (N, H, W) of the input
    pp: str = ""  # FORCED_V1 only: the ping-pong instantiation the shape runs without DY_CONV_V1

    @property
    def id(self):
        return f"{self.cin}>{self.cout}k{self.ks}s{self.s}"


V3, V1, PP = "conv_mfma_wlds_kernel<%s, 8>", "conv_mfma_kernel<%s>", "conv_mfma_pp_kernel<%s, false, 0>"
MAPS_S1 = ((2, 19, 37), (1, 5, 7), (3, 8, 32))   # two tile columns with the second ragged + a height inside a tile; below one tile; exact
MAPS_S2 = ((2, 21, 39), (1, 9, 7))               # odd extents
MAPS_K1 = ((2, 19, 37), (1, 5, 7))               # pixel counts that end inside a wave's 64-pixel strip / below one strip


def _case(cin, cout, ks, s, kernel, dgrad):
    return Case(cin, cout, ks, s, kernel, dgrad, MAPS_K1 if ks == 1 else (MAPS_S1 if s == 1 else MAPS_S2))


# every v3 / v1 instantiation tests/golden/conv_select.json.gz names, at the smallest widths of its sweep that reach it
FALLBACK_CASES = [
    _case(88, 48, 3, 1, V3 % "8, 4, 3, 1, 2", PP % "16, 4, 3, 1, 2"),
    _case(264, 48, 1, 1, V3 % "8, 4, 1, 1, 2", PP % "16, 4, 1, 1, 2"),
    _case(72, 48, 3, 2, V3 % "8, 4, 3, 2, 1", PP % "16, 4, 3, 1, 2"),
    _case(80, 48, 3, 2, V3 % "16, 4, 3, 2, 1", PP % "16, 4, 3, 1, 2"),
    _case(96, 144, 3, 1, V3 % "32, 4, 3, 1, 1", V1 % "16, 4, 3, 1, 2"),
    _case(320, 16, 3, 1, V3 % "64, 1, 3, 1, 1", PP % "16, 4, 3, 1, 2"),
    _case(144, 48, 3, 1, V1 % "16, 4, 3, 1, 2", PP % "16, 4, 3, 1, 2"),
    _case(144, 48, 3, 2, V1 % "16, 4, 3, 2, 1", PP % "16, 4, 3, 1, 2"),
    _case(256, 16, 3, 2, V1 % "32, 1, 3, 2, 1", PP % "16, 4, 3, 1, 2"),
    _case(160, 24, 3, 2, V1 % "32, 2, 3, 2, 1", PP % "8, 4, 3, 1, 2"),
    _case(128, 144, 3, 1, V1 % "32, 4, 3, 1, 2", V1 % "16, 4, 3, 1, 2"),  # cout_p = 192: the last cout group is padding
    _case(96, 144, 3, 2, V1 % "32, 4, 3, 2, 1", V1 % "16, 4, 3, 1, 2"),
    _case(384, 16, 3, 1, V1 % "64, 1, 3, 1, 2", PP % "16, 4, 3, 1, 2"),
    _case(192, 24, 3, 1, V1 % "64, 2, 3, 1, 2", PP % "8, 4, 3, 1, 2"),
    _case(1024, 48, 1, 1, V1 % "64, 4, 1, 1, 2", PP % "16, 4, 1, 1, 2"),
    _case(264, 24, 3, 1, V1 % "8, 2, 3, 1, 2", PP % "8, 4, 3, 1, 2"),
    _case(264, 24, 3, 2, V1 % "8, 2, 3, 2, 1", PP % "8, 4, 3, 1, 2"),
    _case(264, 48, 3, 1, V1 % "8, 4, 3, 1, 2", PP % "16, 4, 3, 1, 2"),
    _case(88, 48, 3, 2, V1 % "8, 4, 3, 2, 1", PP % "16, 4, 3, 1, 2"),
]
# a cout that is no multiple of 8 (scalar tail stores, the co0 + j < cout masks); 88 -> 81 is Detect's class branch at 81 classes
RAGGED_CASES = [
    _case(144, 37, 3, 1, V1 % "16, 4, 3, 1, 2", PP % "8, 4, 3, 1, 2"),
    _case(88, 81, 3, 1, V3 % "8, 4, 3, 1, 2", V3 % "8, 4, 3, 1, 2"),
]
# stride-2 layers whose INPUT GRADIENT is a v3 / v1 launch with dil = 2 (the zero-fill and parity predicates of the halo staging)
DGRAD_CASES = [
    _case(48, 144, 3, 2, PP % "16, 4, 3, 2, 1", V1 % "16, 4, 3, 1, 2"),
    _case(144, 96, 3, 2, V1 % "16, 4, 3, 2, 1", V3 % "32, 4, 3, 1, 1"),   # conv_mfma_dg2_kernel<32, 4> unless DY_CONV_NO_DG2
    _case(144, 128, 3, 2, V1 % "16, 4, 3, 2, 1", V1 % "32, 4, 3, 1, 2"),  # (the dg2 weights do not fit LDS: the base family either way)
    _case(48, 88, 3, 2, PP % "16, 4, 3, 2, 1", V3 % "8, 4, 3, 1, 2"),
]
# the one-row (TR = 1) stride-1 forms of the ping-pong kernel
PP_ONE_ROW_CASES = [
    _case(512, 48, 1, 1, PP % "64, 4, 1, 1, 1", PP % "16, 4, 1, 1, 2"),
    _case(128, 24, 3, 1, PP % "64, 2, 3, 1, 1", PP % "8, 4, 3, 1, 2"),
    _case(192, 16, 3, 1, PP % "64, 1, 3, 1, 1", PP % "16, 4, 3, 1, 2"),
]
CASES = FALLBACK_CASES + RAGGED_CASES + DGRAD_CASES + PP_ONE_ROW_CASES
# ping-pong shapes of tests/test_gpu_kernels.py's CONV_CASES run under DY_CONV_V1=1 (``kernel``: conv_mfma_kernel) and without the switch
# (``pp``): one per (ks, stride) and Cin chunk 8 / 16 / 32 / 64
def _forced(cin, cout, ks, s, nhw, args):
    return Case(cin, cout, ks, s, V1 % args, "", (nhw,), PP % args)


FORCED_V1 = [_forced(3, 16, 3, 2, (2, 32, 48), "8, 1, 3, 2, 1"), _forced(16, 32, 3, 1, (2, 12, 20), "16, 2, 3, 1, 2"),
             _forced(32, 64, 3, 2, (2, 26, 34), "32, 4, 3, 2, 1"), _forced(64, 32, 3, 1, (2, 5, 80), "64, 2, 3, 1, 2"),
             _forced(256, 128, 1, 1, (2, 10, 10), "64, 4, 1, 1, 2"), _forced(96, 64, 1, 1, (2, 13, 5), "32, 4, 1, 1, 2")]
# v3's persistent tile loop only iterates beyond DY_WLDS_MAX_WGS = 512 tiles: 513 tiles of 32 x 16 resp. 32 x 8 output pixels
PERSISTENT = [(FALLBACK_CASES[0], (1, 8208, 32), 16), (FALLBACK_CASES[2], (1, 8193, 39), 8)]  # case, input map, tile height


def is_fallback(name):
    return name.startswith(("conv_mfma_wlds_kernel<", "conv_mfma_kernel<"))


def dg2_takes(case, cc, mt, nch):
    """conv_plan()'s rule for the parity-class kernel, recomputed: the input gradient of a stride-2 3x3 (dil = 2) whose transposed
    geometry (cc, mt, nch from dy_conv_geometry(round8(cout), cin, 3, 1)) stages 32- / 64-channel chunks and fits 156 KiB of LDS."""
    lds = nch * 9 * (cc // 32) * 16 * mt * 64 + 2 * 5 * 17 * (cc * 2 + 32) + 8 * 16 * (32 * mt + 16)
    return case.s == 2 and case.ks == 3 and cc in (32, 64) and case.cin % 8 == 0 and lds <= 156 * 1024


def out_hw(case, H, W):
    p = case.ks // 2
    return (H + 2 * p - case.ks) // case.s + 1, (W + 2 * p - case.ks) // case.s + 1


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def h16(t):
    return t.half().double()


def seed_of(case, nhw):
    N, H, W = nhw
    return (((case.cin * 1031 + case.cout) * 7 + case.ks) * 3 + case.s) * 100003 + N * 10007 + H * 101 + W


def inputs(case, nhw, only=None):
    """x, w (fp16-exact), b, old32 (fp32-exact), dy, old16 (fp16-exact), float64 NCHW, from a generator seeded by the case."""
    N, H, W = nhw
    Ho, Wo = out_hw(case, H, W)
    g = torch.Generator().manual_seed(seed_of(case, nhw))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    d = dict(w=h16(rn(case.cout, case.cin, case.ks, case.ks) / math.sqrt(case.cin * case.ks ** 2)), b=rn(case.cout).float().double())
    d["x"] = h16(rn(N, case.cin, H, W))
    if only == "forward":
        return d
    d.update(dy=h16(rn(N, case.cout, Ho, Wo)), old16=h16(rn(N, case.cout, Ho, Wo)), old32=rn(N, case.cout, Ho, Wo).float().double())
    return d


# ---- reference -------------------------------------------------------------------------------------------------------------------------
def conv_grads(x, w, dy, ks, s):
    """(y, dX, dW) of y = conv2d(x, w, stride s, pad ks // 2) by float64 autograd."""
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, None, s, ks // 2)
    y.backward(dy)
    return y.detach(), xr.grad, wr.grad


def dilate(dy, s):
    """The zero-dilated map the stride-s input gradient reads: dy at the positions that are multiples of s, zeros between."""
    N, C, Ho, Wo = dy.shape
    v = torch.zeros(N, C, (Ho - 1) * s + 1, (Wo - 1) * s + 1, dtype=dy.dtype)
    v[:, :, ::s, ::s] = dy
    return v


def dgrad_direct(v, w, ks, H, W):
    """dX[iy, ix] = sum_k V[iy + pad - ky, ix + pad - kx] w[ky, kx] over the (already dilated) map V: a stride-1 convolution with the
    flipped, transposed kernel -- what the kernels compute over the transposed pack."""
    pad = ks // 2
    top = ks - 1 - pad
    vp = F.pad(v, (top, W - 1 + pad - (v.shape[3] - 1), top, H - 1 + pad - (v.shape[2] - 1)))
    return F.conv2d(vp, w.flip(2, 3).transpose(0, 1).contiguous())


def wgrad_direct(x, dy, ks, s):
    """dW[co, ci, ky, kx] = sum over pixels of dy[n, co, oy, ox] x[n, ci, oy s - pad + ky, ox s - pad + kx]."""
    pad = ks // 2
    N, Co, Ho, Wo = dy.shape
    xp = F.pad(x, (pad, pad, pad, pad))
    dw = torch.zeros(Co, x.shape[1], ks, ks, dtype=torch.float64)
    for ky in range(ks):
        for kx in range(ks):
            dw[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", dy, xp[:, :, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s])
    return dw


@functools.lru_cache(maxsize=4)
def reference(case, nhw):
    """The inputs plus y (no bias), dx, dw and the absolute-value forms S, Sdx, Sdw.  Computed once per (case, map); do not modify."""
    d = inputs(case, nhw)
    d["y"], d["dx"], d["dw"] = conv_grads(d["x"], d["w"], d["dy"], case.ks, case.s)
    d["S"], d["Sdx"], d["Sdw"] = conv_grads(d["x"].abs(), d["w"].abs(), d["dy"].abs(), case.ks, case.s)
    return d


def silu(z):
    return z * torch.sigmoid(z)


# ---- bounds: dicts of named terms, so that a failure can say which one dominated --------------------------------------------------------
def b32(ref, S, K, bias=None):
    t = {"K 2^-23 S": K * EPS32 * S, "2^-23 |ref|": EPS32 * ref.abs()}
    if bias is not None:
        t["2^-24 |bias|"] = (HALF32 * bias.abs()).view(1, -1, 1, 1).expand_as(ref)
    return t


def b16(ref, pre):
    return {**pre, "2^-11 |ref|": EPS16 * ref.abs(), "2^-24": torch.full_like(ref, TINY)}


def accum16(ref, conv, S, K, two):
    """fp16 ACCUM: one rounding of old + conv (v1 / v3), or two -- conv to fp16 first (ping-pong, dg2)."""
    t = b32(ref, S, K)
    if two:
        t["2^-11 |conv| (first rounding)"] = EPS16 * (conv.abs() + total(b32(conv, S, K))) + TINY
    return b16(ref, t)


def total(terms):
    return sum(terms.values())


def fp32_part(terms):
    """The bound of the value before its fp16 rounding."""
    return {k: v for k, v in terms.items() if k not in ("2^-11 |ref|", "2^-24")}


def expected(case, nhw, fwd_pp=False):
    """{output: (ref, terms)} of every forward epilogue, NCHW float64.  fwd_pp: the ping-pong kernel runs the forward."""
    r = reference(case, nhw)
    K = round8(case.cin) * case.ks ** 2
    y, S, b = r["y"], r["S"], r["b"]
    yb = y + b.view(1, -1, 1, 1)
    out = {"y0": (y, b16(y, b32(y, S, K)))}
    out["y_stats"] = out["y_acc_stats"] = out["y0"]
    sl = silu(yb)
    pre = b32(yb, S, K, b)
    pre[f"{SILU_ULPS} 2^-23 |silu|"] = SILU_ULPS * EPS32 * sl.abs()
    out["y_silu"] = (sl, b16(sl, pre))
    out["y32"] = (yb, b32(yb, S, K, b))
    a16, a32 = r["old16"] + y, r["old32"] + y
    out["y16_accum"] = (a16, accum16(a16, y, S, K, fwd_pp))
    out["y32_accum"] = (a32, b32(a32, S, K))
    return out


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def check(got, ref, terms, what, log=None):
    """|got - ref| <= sum(terms) per element; prints the worst ratio, returns it, raises with the terms at the worst element."""
    got = torch.as_tensor(got).double().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(ref).all()), what
    bnd = total(terms)
    ratio = (got - ref).abs() / bnd
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    worst = float(ratio.max())
    print(f"{what}: worst |got - ref| / bound = {worst:.3f} over {ratio.numel()} elements")
    if log is not None:
        log[what] = worst
    if worst > 1.0:
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        parts = ", ".join(f"{k} = {float(torch.as_tensor(v).expand_as(ref).flatten()[i]):.3e}" for k, v in terms.items())
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements out of bound; worst at {idx}: got "
                             f"{float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} bound {float(bnd.flatten()[i]):.3e} ({parts})")
    return worst


def check_canary(buf, real, what):
    """Channels [real, pitch) of a canary-filled buffer are bit-unchanged."""
    tail = torch.as_tensor(buf)[..., real:]
    bad = tail != CANARY
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} canary elements behind channel {real} overwritten, first at {bad.nonzero()[0].tolist()}"


def check_sums(s1, s2, y, what, log=None, elem_bound=None, yref=None):
    """BatchNorm sums (C,) float64 against the float64 sums over the pixels of ``y`` (P, C): the kernel's own stored values ("stored"
    mode), or -- elem_bound (P, C) given -- the reference ``yref`` the kernel's values sit within elem_bound of ("ref" mode)."""
    P = y.shape[0]
    if elem_bound is None:
        r1, r2 = y.sum(0), (y * y).sum(0)
        t1 = {"P 2^-23 sum|y|": P * EPS32 * y.abs().sum(0)}
        t2 = {"(P + 1) 2^-23 sum y^2": (P + 1) * EPS32 * (y * y).sum(0)}
    else:
        r1, r2 = yref.sum(0), (yref * yref).sum(0)
        big = yref.abs() + elem_bound
        t1 = {"P 2^-23 sum|y|": P * EPS32 * big.sum(0), "sum of element bounds": elem_bound.sum(0)}
        t2 = {"(P + 1) 2^-23 sum y^2": (P + 1) * EPS32 * (big * big).sum(0), "sum of element bounds": (elem_bound * (2 * yref.abs() + elem_bound)).sum(0)}
    for t in (t1, t2):
        t["2^-126"] = torch.full_like(r1, 2.0 ** -126)  # a channel whose every value is zero
    return max(check(s1, r1, t1, what + " sum y", log), check(s2, r2, t2, what + " sum y^2", log))


def compare(res, case, nhw, log=None, fwd_pp=False, dgrad_pp=False):
    """Hold everything a run left in ``res`` (tests/conv_fallback_worker.py: whole buffers, canary included) to the reference.
    fwd_pp / dgrad_pp: the forward / the input gradient ran on the ping-pong (or dg2) kernel -- BatchNorm sums in "ref" mode, fp16
    accumulate with two roundings (module docstring).  Returns {what: worst ratio}."""
    log = {} if log is None else log
    N, H, W = nhw
    Ho, Wo = out_hw(case, H, W)
    cout, cin, ctot, P = case.cout, case.cin, round16(case.cout), N * Ho * Wo
    tag = f"{case.id} {N}x{H}x{W}"
    r = reference(case, nhw)
    exp = expected(case, nhw, fwd_pp)
    for k, (ref, terms) in exp.items():
        if k not in res:
            continue
        assert tuple(res[k].shape) == (N, Ho, Wo, round8(cout) + 8), (k, tuple(res[k].shape))
        check(res[k][..., :cout], nhwc(ref), {n: nhwc(v) for n, v in terms.items()}, f"{tag} {k}", log)
        check_canary(res[k], round8(cout), f"{tag} {k}")  # (the pad lanes of a ragged last granule may hold anything: dealyolo_hip.h)
    if "y_stats" in res:
        yref, terms = exp["y0"]
        mode = dict(elem_bound=nhwc(total(terms)).reshape(P, cout), yref=nhwc(yref).reshape(P, cout)) if fwd_pp else {}
        part, nparts = res["part"], res["nparts"]
        assert tuple(part.shape) == (nparts + 2, 2, ctot)
        assert bool((part[nparts:] == CANARY).all()), f"{tag}: partial rows written behind row {nparts}"
        pad = part[:nparts, :, cout:]
        assert bool((pad == 0).all()) and not bool(torch.signbit(pad).any()), f"{tag}: partial sums of channels [{cout}, {ctot}) are not +0.0"
        ps = part[:nparts].double().sum(0)
        check_sums(ps[0, :cout], ps[1, :cout], res["y_stats"][..., :cout].double().reshape(P, cout), f"{tag} partial rows", log, **mode)
        acc = res["acc"]
        assert tuple(acc.shape) == (BN_COPIES, 2, ctot)
        assert bool((acc[:, :, cout:] == 0).all()), f"{tag}: accumulator channels [{cout}, {ctot}) are not zero"
        a = acc.sum(0)
        check_sums(a[0, :cout], a[1, :cout], res["y_acc_stats"][..., :cout].double().reshape(P, cout), f"{tag} fp64 accumulator", log, **mode)
    Kdx = round8(cout) * case.ks ** 2
    if "dx" in res:
        cinp = round8(cin)
        assert tuple(res["dx"].shape) == (N, H, W, cinp + 8)
        dx, Sdx = nhwc(r["dx"]), nhwc(r["Sdx"])
        check(res["dx"][..., :cin], dx, b16(dx, b32(dx, Sdx, Kdx)), f"{tag} dX", log)
        check_canary(res["dx"], cinp, f"{tag} dX")
        if "dx2" in res:
            ref2 = res["dx"][..., :cin].double() + dx
            check(res["dx2"][..., :cin], ref2, accum16(ref2, dx, Sdx, Kdx, dgrad_pp), f"{tag} dX accumulate", log)
            check_canary(res["dx2"], cinp, f"{tag} dX accumulate")
    if "dw" in res:
        check(res["dw"], r["dw"], b32(r["dw"], r["Sdw"], P), f"{tag} dW", log)
        if "dw2" in res:
            ref2 = res["dw"].double() + r["dw"]
            check(res["dw2"], ref2, b32(ref2, r["Sdw"], P), f"{tag} dW accumulate", log)
    return log


# ---- the kernel's arithmetic on the CPU (IEEE fp32): what tests/test_host_conv_ref.py runs through ``compare`` ---------------------------
def conv32_chunked(x, w, ks, s):
    """fp32 convolution accumulated per tap and per 32-channel k-step, in that order (another order than ATen's)."""
    pad = ks // 2
    N, Cin, H, W = x.shape
    Ho, Wo = (H + 2 * pad - ks) // s + 1, (W + 2 * pad - ks) // s + 1
    xp = F.pad(x, (pad, pad, pad, pad))
    acc = torch.zeros(N, w.shape[0], Ho, Wo, dtype=torch.float32)
    for c0 in range(0, Cin, 32):
        for ky in range(ks):
            for kx in range(ks):
                acc = acc + torch.einsum("nchw,oc->nohw", xp[:, c0:c0 + 32, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s], w[:, c0:c0 + 32, ky, kx])
    return acc


def pitched(t, pad=8, dtype=torch.float16):
    """NCHW values -> a channels-last buffer of pitch round8(C) + pad with the canary behind the real channels (pad lanes zero)."""
    t = nhwc(t)
    C = t.shape[-1]
    buf = torch.full((*t.shape[:-1], round8(C) + pad), CANARY, dtype=dtype)
    buf[..., C:round8(C)] = 0
    buf[..., :C] = t.to(dtype)
    return buf


def emulate(case, nhw, chunked=False, pp=False):
    """A ``res`` as the GPU run leaves it, from IEEE fp32 arithmetic on the CPU: the convolution in fp32 (ATen's order, or per tap and
    k-step), every epilogue as the kernels write it, the gradients by fp32 autograd, the sums over the rounded values in fp32.
    pp: as the ping-pong kernel does it -- accumulate after a first rounding to fp16, sums over the fp32 values."""
    r = reference(case, nhw)
    x, w, dy, b = r["x"].float(), r["w"].float(), r["dy"].float(), r["b"].float().view(1, -1, 1, 1)
    y = conv32_chunked(x, w, case.ks, case.s) if chunked else F.conv2d(x, w, None, case.s, case.ks // 2)
    z = y + b
    res = {"y0": pitched(y), "y_stats": pitched(y), "y_acc_stats": pitched(y), "y_silu": pitched(z / (1 + torch.exp(-z))),
           "y32": pitched(z, dtype=torch.float32), "y16_accum": pitched((y.half().float() if pp else y) + r["old16"].float()),
           "y32_accum": pitched(y + r["old32"].float(), dtype=torch.float32)}
    ctot, cout = round16(case.cout), case.cout
    yq = nhwc(y).reshape(-1, cout) if pp else res["y0"][..., :cout].float().reshape(-1, cout)
    part = torch.full((3, 2, ctot), CANARY, dtype=torch.float32)
    part[0] = 0
    part[0, 0, :cout], part[0, 1, :cout] = yq.sum(0), (yq * yq).sum(0)
    acc = torch.zeros(BN_COPIES, 2, ctot, dtype=torch.float64)
    acc[3] = part[0].double()
    res.update(part=part, nparts=1, acc=acc)
    _, dx, dw = conv_grads(x, w, dy, case.ks, case.s)
    res["dx"] = pitched(dx)
    res["dx2"] = pitched((dx.half().float() if pp else dx) + nhwc_inv(res["dx"][..., :case.cin].float()))
    res["dw"] = dw
    res["dw2"] = dw + dw
    # the fp32 values the fp16 outputs were rounded from (``compare`` does not look at them: test_host_conv_ref.py does)
    res["pre"] = {"y0": y, "y_silu": z / (1 + torch.exp(-z)), "y16_accum": y + r["old16"].float(), "dx": dx,
                  "dx2": dx + nhwc_inv(res["dx"][..., :case.cin].float())}
    return res


def nhwc_inv(t):
    return t.permute(0, 3, 1, 2).contiguous()
