"""Attentional scale-sequence fusion blocks: Zoom_cat, ScalSeq, Add (drop-in for reference
nn/extra_modules/block.py:3402-3484), SPDConv, the space-to-depth down-sampling layer (reference :2497-2507), DySample, the
learned dynamic up-sampler (reference :3819-3892), CARAFE, the content-aware up-sampler (reference :3898-3936), ADown, the
YOLOv9 pooled down-sampler (reference :4685-4698), Fusion, BiFPN's weighted feature fusion (reference :453-490), and the slim-neck
blocks GSConv, GSBottleneck and VoVGSCSP (reference :886-967)."""
from __future__ import annotations

import torch
import torch.nn as nn

from ...hip import DY_ACT_LEAKY, DY_ACT_NONE
from ...hip.engine import BN3D_EPS, BN3D_MOM, FusionVec
from ...hip.runtime import HipModule
from ..modules.conv import Conv
from ..rows import conv_row, same_width_row

__all__ = ("Zoom_cat", "ScalSeq", "Add", "SPDConv", "DySample", "CARAFE", "ADown", "adown_check", "Fusion", "fusion_check", "GSConv", "GSBottleneck", "VoVGSCSP",
           "gsconv_check")


class Zoom_cat(HipModule):
    """cat(maxpool+avgpool of the fine map, middle map, nearest-upsampled coarse map) (reference :3402-3412)."""

    @classmethod
    def yaml_row(cls, row):  # reference tasks.py:1001-1002; the output has the middle map's size
        return row.args, sum(row.chs), row.down[1]

    def forward_act(self, xs, out=None):
        return self.rt.eng.zoom_cat(list(xs), out)


class ScalSeq(HipModule):
    """Scale-sequence feature fusion (reference :3414-3443): 1x1 Convs on the two coarser levels, nearest resize to the
    finest, Conv3d(1x1x1)+BatchNorm3d+LeakyReLU(0.1) over the 3-deep stack, max over depth."""
    concat_dst = True

    @classmethod
    def yaml_row(cls, row):  # reference tasks.py:1005-1008: the width is scaled without the max_channels cap
        c2 = row.scaled(row.args[0], capped=False)
        return [row.chs, c2], c2, row.down[0]

    def __init__(self, inc, channel):
        super().__init__()
        if channel != inc[0]:
            self.conv0 = Conv(inc[0], channel, 1)
        self.conv1 = Conv(inc[1], channel, 1)
        self.conv2 = Conv(inc[2], channel, 1)
        self.conv3d = nn.Conv3d(channel, channel, kernel_size=(1, 1, 1))
        self.bn = nn.BatchNorm3d(channel)
        self.act = nn.LeakyReLU(0.1)
        self.pool_3d = nn.MaxPool3d(kernel_size=(3, 1, 1))

    def _build_specs(self, rt):
        sp = rt.make_spec((id(self), "conv3d"), self.conv3d, None, DY_ACT_LEAKY, 1, 1, name="ScalSeq.conv3d")
        sp.bn3d = dict(weight=self.bn.weight.data, bias=self.bn.bias.data, running_mean=self.bn.running_mean,
                       running_var=self.bn.running_var)
        sp.coef3d = rt.eng.f32(4 * sp.cout)
        sp.bwdcoef3d = rt.eng.f32(2 * sp.cout)
        sp.params.update(bn3d_w=self.bn.weight, bn3d_b=self.bn.bias)
        rt._bind_grads(sp)

    def forward_act(self, xs, out=None, res=None):
        p3, p4, p5 = xs
        if hasattr(self, "conv0"):
            p3 = self.conv0.forward_act(p3)
        p4 = self.conv1.forward_act(p4)
        p5 = self.conv2.forward_act(p5)
        sp = self.rt.specs[(id(self), "conv3d")]
        return self.rt.eng.scalseq(sp, sp.bn3d, sp.coef3d, sp.bwdcoef3d, sp.gbn3d, [p3, p4, p5], out, res=res)


class Add(HipModule):
    """Element-wise sum of the inputs (reference :3479-3484)."""
    concat_dst = True

    @classmethod
    def yaml_row(cls, row):  # reference tasks.py:1003-1004
        return row.args, row.chs[-1], row.down[-1]

    def forward_act(self, xs, out=None):
        return self.rt.eng.add(list(xs), out)


class SPDConv(HipModule):
    """Space-to-depth convolution (reference :2497-2507): the four pixels of every 2x2 block become four channel groups
    (``cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)``), then Conv(4 * inc, ouc, k=3) -- a
    down-sampling layer that drops no pixel.  The rearrangement is one permutation launch (csrc/spd.hip); the convolution is the
    ordinary 3x3 path on the 4 * inc-channel tensor, its weights in ``state_dict`` order."""
    concat_dst = True

    @classmethod
    def yaml_row(cls, row):
        return conv_row(cls, row, stride=2)

    def __init__(self, inc, ouc, dimension=1):
        super().__init__()
        self.d = dimension
        self.conv = Conv(inc * 4, ouc, k=3)

    def out_hw(self, h, w):
        return h // 2, w // 2

    def forward_act(self, x, out=None):
        if x.H % 2 or x.W % 2 or x.H < 2 or x.W < 2:
            raise ValueError(f"SPDConv (layer {getattr(self, 'i', '?')}) needs a map with even sides, got {x.H}x{x.W}: "
                             "the reference's torch.cat of the four parity views fails on it too")
        return self.conv.forward_act(self.rt.eng.space_to_depth(x), out)


class DySample(HipModule):
    """Learned dynamic up-sampling (reference :3819-3892), style 'lp' without dyscope: a 1x1 ``offset`` convolution (bias, no
    BatchNorm, no activation) predicts, per channel group and per sub-position of the ``scale`` x ``scale`` output block, where the
    low-resolution map is sampled bilinearly: at the base pixel + 0.25 * offset + ``init_pos``, clamped to the map
    (``F.grid_sample(..., padding_mode='border')`` after the reference's normalisation cancels).  ``state_dict`` keys, shapes and
    initialisation are the reference's; the sampler (csrc/dysample.hip) computes ``init_pos`` in closed form, the buffer is kept for
    the checkpoints."""

    SUPPORTED = "style='lp', dyscope=False, scale 2 or 4 and in_channels a multiple of 8 * groups"
    concat_dst = True

    @classmethod
    def yaml_row(cls, row):  # reference tasks.py:965-967
        return same_width_row(row, [row.chs[0], *row.args], row.args[0] if row.args else 2)

    def __init__(self, in_channels, scale=2, style="lp", groups=4, dyscope=False):
        super().__init__()
        if style != "lp" or dyscope:
            raise NotImplementedError(f"DySample(style={style!r}, dyscope={dyscope}) is outside the HIP path (supported: {self.SUPPORTED})")
        if scale not in (2, 4) or groups < 1 or in_channels < 8 * groups or in_channels % (8 * groups):
            raise NotImplementedError(f"DySample(in_channels={in_channels}, scale={scale}, groups={groups}) is outside the HIP path "
                                      f"(supported: {self.SUPPORTED})")
        self.scale, self.style, self.groups = scale, style, groups
        self.offset = nn.Conv2d(in_channels, 2 * groups * scale ** 2, 1)
        nn.init.normal_(self.offset.weight, 0.0, 0.001)  # reference normal_init(self.offset, std=0.001) :3837, :3844-3848
        nn.init.constant_(self.offset.bias, 0.0)
        self.register_buffer("init_pos", self._init_pos())

    def _init_pos(self):
        """(1, 2 * groups * scale^2, 1, 1): channel d G s^2 + g s^2 + i s + j holds t[j] for d = 0 (x) and t[i] for d = 1 (y),
        t[k] = (k - (s - 1) / 2) / s (reference :3856-3858)."""
        s = self.scale
        t = (torch.arange(s, dtype=torch.float32) - (s - 1) / 2) / s
        tx, ty = t.view(1, s).expand(s, s), t.view(s, 1).expand(s, s)
        return torch.stack([tx, ty]).reshape(2, 1, s * s).repeat(1, self.groups, 1).reshape(1, -1, 1, 1).contiguous()

    def out_hw(self, h, w):
        return self.scale * h, self.scale * w

    def _build_specs(self, rt):
        rt.make_spec((id(self), "offset"), self.offset, None, DY_ACT_NONE, 1, 1, name="DySample.offset")

    def forward_act(self, x, out=None):
        return self.rt.eng.dysample(self.rt.specs[(id(self), "offset")], self.scale, self.groups, x, out)


class CARAFE(HipModule):
    """Content-aware reassembly of features (arXiv 1905.02188; reference :3898-3936): ``comp`` (1x1 Conv to ``c_mid``) and ``enc``
    (``k_enc`` x ``k_enc`` Conv to (scale * k_up)^2 = 100 channels, BatchNorm, no activation) predict, per output pixel, a softmax
    kernel over the 5x5 neighbourhood of its base pixel; the output is that weighted sum (csrc/carafe.hip; the reference's
    pixel_shuffle / Upsample / Unfold / einsum chain :3926-3935 reduces to it).  ``state_dict`` keys, shapes and initialisation are
    the reference's: both Convs are this package's ``Conv``; pixel_shuffle, Upsample and Unfold carry no state."""

    SUPPORTED = "k_up=5, scale=2, c a multiple of 8, k_enc 1 or 3"
    concat_dst = True

    @classmethod
    def yaml_row(cls, row):  # reference tasks.py:965-967 (DySample's branch); scale 2 is the only one the module takes
        return same_width_row(row, [row.chs[0], *row.args], 2)

    def __init__(self, c, k_enc=3, k_up=5, c_mid=64, scale=2):
        super().__init__()
        if k_up != 5 or scale != 2 or c < 8 or c % 8 or k_enc not in (1, 3):
            raise NotImplementedError(f"CARAFE(c={c}, k_enc={k_enc}, k_up={k_up}, scale={scale}) is outside the HIP path "
                                      f"(supported: {self.SUPPORTED})")
        self.scale, self.k_up = scale, k_up
        self.comp = Conv(c, c_mid)
        self.enc = Conv(c_mid, (scale * k_up) ** 2, k=k_enc, act=False)

    def out_hw(self, h, w):
        return self.scale * h, self.scale * w

    def forward_act(self, x, out=None):
        return self.rt.eng.carafe(self.rt.spec(self.comp), self.rt.spec(self.enc), x, out)


ADOWN_SUPPORTED = "supported: c1 % 16 == 0 and c2 % 16 == 0 (both halves whole 8-channel granules), SiLU"


def adown_check(layer, c1, c2):
    """The ADown widths the HIP path takes (csrc/adown.hip moves whole granules of each half).  Anything else raises, naming the
    layer, its arguments and the supported set."""
    if not (isinstance(c1, int) and isinstance(c2, int) and c1 >= 16 and c2 >= 16 and c1 % 16 == 0 and c2 % 16 == 0):
        raise NotImplementedError(f"{layer}(c1={c1}, c2={c2}) is outside the HIP hot path ({ADOWN_SUPPORTED})")


class ADown(HipModule):
    """YOLOv9's pooled down-sampling (reference :4685-4698): a 2x2 stride-1 average, then the first half of the channels through
    ``cv1`` (Conv 3x3 s2) and the second half through a 3x3 s2 max pool and ``cv2`` (Conv 1x1), concatenated.  The average, the
    chunk and the max pool are one launch (csrc/adown.hip); both Convs are this package's ``Conv`` and write the two halves of one
    output buffer.  Attribute names, ``state_dict`` keys and initialisation are the reference's."""
    concat_dst = True

    @classmethod
    def yaml_row(cls, row):  # reference tasks.py:840
        return conv_row(cls, row, stride=2, check=lambda row, c1, c2, a: adown_check(row.layer, c1, c2))

    def __init__(self, c1, c2):
        super().__init__()
        adown_check("ADown", c1, c2)
        self.c = c2 // 2
        self.cv1 = Conv(c1 // 2, self.c, 3, 2, 1)
        self.cv2 = Conv(c1 // 2, self.c, 1, 1, 0)

    def out_hw(self, h, w):
        return h // 2, w // 2

    def forward_act(self, x, out=None):
        return self.rt.eng.adown(self.rt.spec(self.cv1), self.rt.spec(self.cv2), x, out, name=f"ADown (layer {getattr(self, 'i', '?')})")


FUSION_MODES = ("weight", "adaptive", "concat", "bifpn", "SDI")  # the reference's menu (:457)
FUSION_SUPPORTED = "supported: fusion 'bifpn' over 2 or 3 inputs of one width and map size, the width a multiple of 8; fusion 'concat'"


def fusion_check(layer, inc_list, fusion):
    """The Fusion forms the HIP path takes (csrc/fusion.hip for 'bifpn', the engine's Concat for 'concat').  Anything else raises,
    naming the layer, its arguments and the supported set."""
    inc = list(inc_list) if isinstance(inc_list, (list, tuple)) else None
    ok = inc is not None and len(inc) >= 1 and all(isinstance(c, int) and c >= 8 and c % 8 == 0 for c in inc) and fusion in ("bifpn", "concat")
    if ok and fusion == "bifpn":
        ok = 2 <= len(inc) <= 3 and len(set(inc)) == 1
    if not ok:
        raise NotImplementedError(f"{layer}(inc_list={inc_list}, fusion={fusion!r}) is outside the HIP hot path ({FUSION_SUPPORTED})")


class Fusion(HipModule):
    """BiFPN's fast normalised fusion (reference :453-490, mode 'bifpn'): ``y = sum_i f[i] x[i]`` with ``f = relu(fusion_weight) /
    sum(relu(fusion_weight))`` -- no epsilon: the reference sets ``self.epsilon = 1e-4`` and never uses it, so weights that are all
    <= 0 give NaN (0 / 0) here as there.  ``fusion_weight`` is an fp32 vector of one value per input, initialised to ones; its
    gradient is a dot product over whole maps (csrc/fusion.hip).  Mode 'concat' is the engine's Concat and has no parameter.
    Constructor signature, attribute names (``fusion``, ``fusion_weight``, ``relu``, ``epsilon``) and ``state_dict`` keys are the
    reference's, so its pickles rebuild; the other modes ('weight', 'adaptive', 'SDI') raise."""
    # (concat_dst stays False although 'bifpn' takes ``out``: that is how the Concat plan was before the attribute, not a decision)

    @classmethod
    def yaml_row(cls, row):  # reference tasks.py:922-925: the mode is looked up in the YAML dict, so its NAME is a top-level key
        args, d = row.args, row.yaml
        if not (args and isinstance(args[0], str) and args[0] in d):
            raise KeyError(f"{row.layer}: its argument {args[0] if args else None!r} must name a top-level key of the model YAML that "
                           f"holds the fusion mode (e.g. 'fusion_mode: bifpn')")
        mode, c1 = d[args[0]], row.chs
        fusion_check(row.layer, c1, mode)
        if mode == "bifpn" and len(set(row.down)) != 1:
            raise NotImplementedError(f"{row.layer}(inc_list={c1}, fusion={mode!r}) reads maps of different sizes (down-sampling "
                                      f"{row.down}): outside the HIP hot path (supported: fusion 'bifpn' over 2 or 3 inputs of "
                                      f"one width and map size)")
        return [c1, mode], (sum(c1) if mode == "concat" else c1[0]), row.down[0]

    def __init__(self, inc_list, fusion="bifpn"):
        super().__init__()
        if fusion not in FUSION_MODES:
            raise ValueError(f"Fusion: fusion={fusion!r} is none of {FUSION_MODES}")
        fusion_check("Fusion", inc_list, fusion)
        self.fusion = fusion
        if fusion == "bifpn":
            self.fusion_weight = nn.Parameter(torch.ones(len(inc_list), dtype=torch.float32), requires_grad=True)
            self.relu = nn.ReLU()
            self.epsilon = 1e-4

    def forward_act(self, xs, out=None):
        name = f"Fusion (layer {getattr(self, 'i', '?')})"
        if self.fusion == "concat":
            return self.rt.eng.concat(list(xs))
        if self.fusion != "bifpn":  # (an unpickled reference module of another mode)
            raise NotImplementedError(f"{name}: fusion={self.fusion!r} is outside the HIP hot path ({FUSION_SUPPORTED})")
        p = self.fusion_weight
        return self.rt.eng.fusion(list(xs), FusionVec(p.data, self.rt.gviews.get(id(p)), p.requires_grad), out, name=name)


GSCONV_SUPPORTED = ("supported: GSConv with c1 % 8 == 0, c2 % 16 == 0 (both halves whole 8-channel granules), (k, s) in (1, 1) | (3, 1) | (3, 2), "
                    "p=None, g=1, d=1; VoVGSCSP / GSBottleneck with int(c2 * e) % 16 == 0; VoVGSCSP with n >= 1")


def gsconv_check(layer, c1, c2, k=1, s=1, p=None, g=1, d=1, e=None, n=1):
    """The slim-neck shapes the HIP path takes (csrc/gsconv.hip moves whole granules of each half of the shuffle).  ``e`` None: a
    GSConv row; otherwise a VoVGSCSP / GSBottleneck whose hidden width ``int(c2 * e)`` is the ``c2`` of the GSConvs inside it (``n``: a
    VoVGSCSP's bottleneck count -- without one, nothing writes the second half of the buffer ``cv3`` reads).
    Anything else raises, naming the layer, its arguments and the supported set."""
    ints = isinstance(c1, int) and isinstance(c2, int) and c1 >= 8 and c1 % 8 == 0
    if e is not None:
        if not (ints and c2 >= 16 and c2 % 8 == 0 and isinstance(e, (int, float)) and int(c2 * e) >= 16 and int(c2 * e) % 16 == 0):
            raise NotImplementedError(f"{layer}(c1={c1}, c2={c2}, e={e}) is outside the HIP hot path ({GSCONV_SUPPORTED})")
        if not (isinstance(n, int) and n >= 1):
            raise NotImplementedError(f"{layer}(c1={c1}, c2={c2}, n={n}) is outside the HIP hot path ({GSCONV_SUPPORTED})")
    elif not (ints and c2 >= 16 and c2 % 16 == 0 and (k, s) in ((1, 1), (3, 1), (3, 2)) and p is None and g == 1 and d == 1):
        raise NotImplementedError(f"{layer}(c1={c1}, c2={c2}, k={k}, s={s}, p={p}, g={g}, d={d}) is outside the HIP hot path ({GSCONV_SUPPORTED})")


class GSConv(HipModule):
    """GSConv of slim-neck (reference :886-908): ``x1 = cv1(x)`` (Conv c1 -> c2 / 2, k, s), ``x2 = cat(x1, cv2(x1))`` with ``cv2`` a
    depthwise 5x5, then the channel shuffle ``cat(x2[:, 0::2], x2[:, 1::2])`` -- one launch that reads x1 and cv2's output where they
    lie (csrc/gsconv.hip, ``Engine.gsconv``).  ``act`` is accepted and ignored, as in the reference: both Convs always use SiLU.
    Attribute names, ``state_dict`` keys and initialisation are the reference's."""
    concat_dst = True

    @classmethod
    def yaml_row(cls, row):  # reference tasks.py:828
        return conv_row(cls, row, stride_arg=True, check=lambda row, c1, c2, a: gsconv_check(row.layer, *a[:7]))

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, d=1, act=True):
        super().__init__()
        gsconv_check("GSConv", c1, c2, k, s, p, g, d)
        c_ = c2 // 2
        self.cv1 = Conv(c1, c_, k, s, p, g, d, Conv.default_act)
        self.cv2 = Conv(c_, c_, 5, 1, p, c_, d, Conv.default_act)

    def out_hw(self, h, w):
        return self.cv1.out_hw(h, w)

    def forward_act(self, x, out=None):
        return self.rt.eng.gsconv(self.rt.spec(self.cv1), self.rt.spec(self.cv2), x, out, name=f"GSConv (layer {getattr(self, 'i', '?')})")


class GSBottleneck(HipModule):
    """GS bottleneck (reference :923-935): ``conv_lighting(x) + shortcut(x)`` with ``conv_lighting`` two GSConvs (1x1, then 3x3) and
    ``shortcut`` a 1x1 Conv without activation.  ``k`` and ``s`` are accepted and ignored, as in the reference.  The sum is one
    ``Engine.add`` launch, which may write a slice of the caller's buffer."""

    def __init__(self, c1, c2, k=3, s=1, e=0.5):
        super().__init__()
        gsconv_check("GSBottleneck", c1, c2, e=e)
        c_ = int(c2 * e)
        self.conv_lighting = nn.Sequential(GSConv(c1, c_, 1, 1), GSConv(c_, c2, 3, 1, act=False))
        self.shortcut = Conv(c1, c2, 1, 1, act=False)

    def forward_act(self, x, out=None):
        a = self.conv_lighting[1].forward_act(self.conv_lighting[0].forward_act(x))
        return self.rt.eng.add([a, self.shortcut.forward_act(x)], out)


class VoVGSCSP(HipModule):
    """VoV-GSCSP (reference :953-967): ``cv3(cat(cv2(x), gsb(cv1(x))))`` with ``gsb`` a chain of ``n`` GSBottlenecks at e = 1.
    ``shortcut`` and ``g`` are accepted and ignored.  ``res``, a 3x3 Conv, is constructed and NEVER called, exactly as in the
    reference: its parameters and BatchNorm buffers are in ``state_dict()`` and in the parameter count, and nothing ever reads or
    changes them (``unused_modules``: no ConvSpec, no pack, no launch, no gradient, no optimizer update).  ``cv2`` and the last
    bottleneck's sum write the two halves of one buffer that ``cv3`` reads, or stay where they are as the members of a segment table."""
    repeat_is_arg = concat_dst = True

    @classmethod
    def yaml_row(cls, row):  # reference tasks.py:828, :874-875; (a[2], when present, is ``shortcut``: n goes in front of it)
        return conv_row(cls, row, check=lambda row, c1, c2, a: gsconv_check(row.layer, c1, c2, e=a[4] if len(a) > 4 else 0.5))

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        gsconv_check("VoVGSCSP", c1, c2, e=e, n=n)
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.gsb = nn.Sequential(*(GSBottleneck(c_, c_, e=1.0) for _ in range(n)))
        self.res = Conv(c_, c_, 3, 1, act=False)
        self.cv3 = Conv(2 * c_, c2, 1)

    def unused_modules(self):
        return (self.res,)

    def forward_act(self, x, out=None):
        from ...hip.engine import PLANAR, SegAct
        eng, c_, n = self.rt.eng, self.cv1.conv.out_channels, len(self.gsb)
        x1 = self.cv1.forward_act(x)
        if PLANAR:
            y = self.cv2.forward_act(x)
            for b in self.gsb:
                x1 = b.forward_act(x1)
            return self.cv3.forward_act(SegAct([y, x1]), out)
        cat = eng.new_storage(x1.N, x1.H, x1.W, 2 * c_)
        self.cv2.forward_act(x, cat.act(0, c_))
        for j, b in enumerate(self.gsb):
            x1 = b.forward_act(x1, cat.act(c_, c_) if j == n - 1 else None)
        return self.cv3.forward_act(cat.act(), out)
