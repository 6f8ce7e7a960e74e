"""Test-time augmentation of the eval forward: ``model(x, augment=True)`` (reference nn/tasks.py:335-371
DetectionModel._predict_augment / _descale_pred / _clip_augmented, utils/torch_utils.py:355-366 scale_img).

Three passes (scale 1, 0.83 flipped left-right, 0.67).  The pass geometry -- scaled and padded sizes, the columns each pass keeps --
is host arithmetic done here exactly as the reference writes it (``tta_geometry``).  On the device a pass is ``dy_scale_img`` (flip +
bilinear resize + pad in one launch; the unscaled, unflipped pass reads the caller's tensor) followed by the eval forward of that
geometry (``InferPlan``, or the walked launches before a plan exists), and one ``dy_tta_merge`` de-scales, de-flips, clips and
concatenates the three outputs into a fresh tensor the caller owns.  Everything runs in order on the caller's stream.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import check, lib
from . import infer as I

SCALES = (1, 0.83, 0.67)
FLIPS = (None, 3, None)  # 2: up-down, 3: left-right


def scaled_size(H, W, ratio, gs):
    """scale_img's output geometry -> (Ho, Wo, Hp, Wp): the resized extent and the padded one (``same_shape=False``)."""
    if ratio == 1.0:
        return H, W, H, W
    Ho, Wo = int(H * ratio), int(W * ratio)
    return Ho, Wo, math.ceil(H * ratio / gs) * gs, math.ceil(W * ratio / gs) * gs


def kept_columns(As, nl):
    """_clip_augmented on the passes' anchor counts ``As`` -> [(lo, hi)] per pass: the first pass drops its last (A // g) columns, the
    last pass its first (A // g) * 4**(nl-1), g = sum(4**k, k < nl) -- column counts, as the reference slices (``[..., :-0]`` keeps
    nothing)."""
    g = sum(4 ** k for k in range(nl))
    cols = [(0, A) for A in As]
    i = As[0] // g
    cols[0] = (0, As[0] - i if i else 0)
    i = (As[-1] // g) * 4 ** (nl - 1)
    cols[-1] = (min(i, As[-1]), As[-1])
    return cols


def tta_geometry(H, W, gs, nl, As=None):
    """Per pass: dict(scale, flip, Ho, Wo, Hp, Wp) and, given the passes' anchor counts ``As``, the kept column range ``cols``."""
    out = []
    for si, fi in zip(SCALES, FLIPS):
        Ho, Wo, Hp, Wp = scaled_size(H, W, si, gs)
        out.append(dict(scale=si, flip=fi or 0, Ho=Ho, Wo=Wo, Hp=Hp, Wp=Wp))
    if As is not None:
        for p, c in zip(out, kept_columns(list(As), nl)):
            p["cols"] = c
    return out


def _grid(model):
    """(gs, nl): ``int(model.stride.max())`` and Detect's level count, read once per parameter storage (the strides may live on the
    device; reading them there would synchronise every forward)."""
    st = model.__dict__.setdefault("_tta_grid", {})
    dev = next(model.parameters()).device
    if st.get("dev") != dev:
        st["dev"], st["g"] = dev, (int(model.stride.max()), int(model.model[-1].nl))
    return st["g"]


def _is_identity(p):
    return p["Ho"] == p["Hp"] and p["Wo"] == p["Wp"] and p["scale"] == 1 and not p["flip"]


def scale_into(x, p, out):
    """dy_scale_img of one pass: fp32 contiguous ``x`` (B, 3, H, W) -> ``out`` (B, 3, Hp, Wp)."""
    B, _, H, W = x.shape
    check(lib().dy_scale_img(x.data_ptr(), B, H, W, p["flip"], p["Ho"], p["Wo"], p["Hp"], p["Wp"], out.data_ptr(),
                             torch.cuda.current_stream(x.device).cuda_stream), "dy_scale_img")
    return out


def merge(ys, geo, H, W):
    """dy_tta_merge of the passes' outputs ``ys`` (B, no, A_k) into a fresh (B, no, sum of kept columns) tensor."""
    n, (B, no) = len(ys), ys[0].shape[:2]
    out = torch.empty((B, no, sum(hi - lo for lo, hi in (p["cols"] for p in geo))), dtype=torch.float32, device=ys[0].device)
    arr = lambda t, v: (t * n)(*v)  # noqa: E731
    check(lib().dy_tta_merge(n, arr(C.c_void_p, [y.data_ptr() for y in ys]), arr(C.c_int, [y.shape[-1] for y in ys]),
                             arr(C.c_int, [p["cols"][0] for p in geo]), arr(C.c_int, [p["cols"][1] for p in geo]),
                             arr(C.c_float, [p["scale"] for p in geo]), arr(C.c_int, [p["flip"] for p in geo]), B, no, H, W,
                             out.data_ptr(), torch.cuda.current_stream(out.device).cuda_stream), "dy_tta_merge")
    return out


class TtaPlan:
    """The three passes of one input geometry as recorded eval plans: pass 0 replays on the caller's tensor (its stem reads it
    directly), passes 1 and 2 on the static input of their own plan, which ``dy_scale_img`` writes."""

    def __init__(self, model, B, H, W):
        gs, nl = _grid(model)
        self.shape, self.nl = (B, 3, H, W), nl
        self.geo = tta_geometry(H, W, gs, nl)
        self.plans = [I.InferPlan(model, B, p["Hp"], p["Wp"]) for p in self.geo]
        self.last = 0

    def __call__(self, x):
        B, _, H, W = self.shape
        xf = None
        ys = []
        for p, plan in zip(self.geo, self.plans):
            if _is_identity(p):
                ys.append(plan(x))
                continue
            if xf is None:
                xf = x if (x.dtype == torch.float32 and x.is_contiguous()) else x.float().contiguous()
            ys.append(plan(scale_into(xf, p, plan.img)))
        if "cols" not in self.geo[0]:
            self.geo = _with_cols(self.geo, ys, self.nl)
        return merge(ys, self.geo, H, W)


def _with_cols(geo, ys, nl):
    """``geo`` with each pass's kept column range, from the anchor counts of the passes' outputs ``ys``."""
    cols = kept_columns([y.shape[-1] for y in ys], nl)
    return [dict(p, cols=c) for p, c in zip(geo, cols)]


def forward_tta(model, x):
    """``model(x, augment=True)`` in eval mode -> (y (B, 4+nc, sum of kept columns), None), as _predict_augment returns it."""
    H, W = x.shape[-2:]
    plan = tta_plan_for(model, x)
    with torch.no_grad():
        if plan is not None:
            return plan(x), None
        gs, nl = _grid(model)
        geo = tta_geometry(H, W, gs, nl)
        xf = x.float().contiguous()
        ys = []
        for p in geo:
            xi = xf if _is_identity(p) else scale_into(xf, p, torch.empty((x.shape[0], 3, p["Hp"], p["Wp"]), dtype=torch.float32, device=x.device))
            ys.append(I.walk_eval(model, xi)[0])
        return merge(ys, _with_cols(geo, ys, nl), H, W), None


def tta_plan_for(model, x):
    """The recorded TTA plan of ``model`` for input ``x``, or None when this forward should walk: the same policy as
    ``infer.plan_for`` -- recorded on the SECOND forward of a geometry, at most ``MAX_PLANS`` kept, least recently used first out --
    in a registry of its own, so that single-scale and augmented forwards of one geometry never evict or re-record each other."""
    if not I.wants_plan(model, x):
        return None
    st = model.__dict__.setdefault("_tta_plans", {"rt": None, "plans": {}, "seen": {}})
    rt = model._runtime(x.device)
    if st["rt"] is not rt:  # parameters were re-created (.to / .half / fuse): every recorded pointer is stale
        st["rt"], st["plans"], st["seen"] = rt, {}, {}
    key = tuple(x.shape)
    plan = st["plans"].get(key)
    if plan is None:
        st["seen"][key] = st["seen"].get(key, 0) + 1
        if st["seen"][key] < 2:
            return None
        if len(st["plans"]) >= I.MAX_PLANS:
            old = min(st["plans"], key=lambda k: st["plans"][k].last)
            del st["plans"][old]
        plan = st["plans"][key] = TtaPlan(model, key[0], key[2], key[3])
    st["tick"] = plan.last = st.get("tick", 0) + 1
    return plan


def wants_tta(model, x):
    """An eval forward of a detection model on a (B, 3, H, W) device tensor (plans on or off)."""
    from ..nn.modules import Detect
    return (torch.is_tensor(x) and x.dim() == 4 and x.shape[1] == 3 and x.is_cuda and x.is_floating_point()
            and isinstance(model.model[-1], Detect))
