"""CPU: depthwise convolution (DWConv, reference nn/modules/conv.py:106-111; DSConv, :113-122) without a GPU -- the float64
restatement of tests/dwconv_ref.py against autograd through F.conv2d (1e-11), an fp32 emulation of the summation orders
csrc/dwconv.hip documents against the per-element bounds tests/test_gpu_dwconv.py applies to the kernels (so the counted k32 are
checked without a GPU), the new graph's layout and parameter count against the reference's DetectionModel on this package's YAML, the
modules' keys and class paths, the refusals of what the HIP path does not take, the flat layout, fuse(), the new fact of
``conv_bwd_form``, the bound entry points and a reference-written checkpoint."""
import itertools
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import dwconv_ref as R
import dwconv_util as U
from conftest import CFG_DIR, ROOT

SEED = 900


def _maxerr(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max())


# ----------------------------------------------------------------------------- the restatement and the bounds
@pytest.mark.parametrize("name", list(U.KERNEL_CASES))
def test_restatement_vs_autograd(name):
    N, H, W, C1, m, k, s = U.KERNEL_CASES[name]
    x, w, dy, _ = R.inputs(N, H, W, C1, m, k, s, SEED)
    xd, wd = R.nchw(x.double()).requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv2d(xd, wd, None, s, k // 2, 1, C1)
    y.backward(R.nchw(dy.double()))
    fw, ig, wg = R.forward(x, w, s), R.input_grad(dy, w, s, H, W, m), R.weight_grad(x, dy, k, s)
    errs = dict(y=_maxerr(fw["y"], R.nhwc(y.detach())), dx=_maxerr(ig["dx"], R.nhwc(xd.grad)), dw=_maxerr(wg["dw"], wd.grad))
    print(name, errs)
    assert max(errs.values()) < 1e-11
    assert tuple(fw["y"].shape) == (N, *R.out_hw(H, W, k, s), C1 * m)
    for val, mag in ((fw["y"], fw["mag"]), (ig["dx"], ig["mag"]), (wg["dw"], wg["mag"])):
        assert bool((mag >= val.abs() - 1e-12).all())  # the magnitudes bound the values they belong to


@pytest.mark.parametrize("name", list(U.KERNEL_CASES))
def test_fp32_emulation_of_the_documented_orders_meets_the_bounds(name):
    geom = U.KERNEL_CASES[name]
    N, H, W, C1, m, k, s = geom
    x, w, dy, _ = R.inputs(*geom, SEED)
    fw, ig, wg = R.forward(x, w, s), R.input_grad(dy, w, s, H, W, m), R.weight_grad(x, dy, k, s)
    U.check("y", U.emulate_forward(x, w, s), fw["y"], fw["mag"], U.k_bound("y", *geom))
    U.check("dx", U.emulate_input_grad(dy, w, s, H, W, m), ig["dx"], ig["mag"], U.k_bound("dx", *geom))
    U.check("dw", U.emulate_weight_grad(x, dy, k, s), wg["dw"], wg["mag"], U.k_bound("dw", *geom))


def test_the_cases_reach_what_they_are_there_for():
    from ultralytics.hip import lib
    L = lib()
    for name, (N, H, W, C1, m, k, s) in U.KERNEL_CASES.items():
        Ho, Wo = R.out_hw(H, W, k, s)
        assert L.dy_dwconv_supported(C1, m, k, s) == 1
        assert L.dy_dwconv_wgrad_slabs(N, H, W, C1, m, k, s) == U.blocks(N * Ho * Wo, C1 * m, U.WG_MAXB)
        assert L.dy_dwconv_num_partials(N, H, W, C1, m, k, s) == U.blocks(N * Ho * Wo, C1 * m, U.FWD_MAXB)
    assert U.KERNEL_CASES["k5s1_tiny"][1] < 5                                       # a kernel larger than the map
    assert U.blocks(2 * 12 * 20, 32, U.WG_MAXB) > 1                                 # more than one workgroup
    assert len(U.chunks(2 * U.KERNEL_CASES["k3s2_m2_wide"][3])) == 2                # two channel chunks


# ----------------------------------------------------------------------------- modules, parser, graph
def _model(name=U.MODEL):
    from ultralytics.nn.tasks import DetectionModel
    return DetectionModel(os.path.join(CFG_DIR, name + ".yaml"), ch=3, verbose=False)


def test_module_keys_class_paths_and_defaults():
    import ultralytics.nn.modules as M
    import ultralytics.nn.modules.conv as Cv
    assert {"DWConv", "DSConv"} <= set(M.__all__) and {"DWConv", "DSConv"} <= set(Cv.__all__) and M.DWConv is Cv.DWConv and M.DSConv is Cv.DSConv
    assert Cv.DWConv.__module__ == Cv.DSConv.__module__ == "ultralytics.nn.modules.conv" and issubclass(Cv.DWConv, Cv.Conv)
    bn = ["bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"]
    m = Cv.DWConv(16, 32, 3, 2)
    assert list(m.state_dict()) == ["conv.weight"] + bn and tuple(m.conv.weight.shape) == (32, 1, 3, 3)
    assert m.conv.groups == 16 and m.conv.bias is None and m.conv.padding == (1, 1) and isinstance(m.act, torch.nn.SiLU)
    assert isinstance(Cv.DWConv(8, 8, 5, 1, act=False).act, torch.nn.Identity) and Cv.DWConv(8, 8, 5).conv.padding == (2, 2)
    d = Cv.DSConv(16, 40, 7, 2, 3, False)  # k, s, d, act are ignored, exactly as the reference does
    assert list(d.state_dict()) == [f"{c}.{k}" for c in ("dwconv", "pwconv") for k in ["conv.weight"] + bn]
    assert tuple(d.dwconv.conv.weight.shape) == (16, 1, 3, 3) and d.dwconv.conv.stride == (1, 1) and tuple(d.pwconv.conv.weight.shape) == (40, 16, 1, 1)
    assert isinstance(d.dwconv.act, torch.nn.SiLU) and isinstance(d.pwconv.act, torch.nn.SiLU)
    # default initialisation: nn.Conv2d's own (kaiming_uniform with a = sqrt 5 over a fan-in of k k): |w| <= 1 / sqrt(fan_in)
    torch.manual_seed(0)
    w = Cv.DWConv(64, 64, 3).conv.weight.detach()
    assert float(w.abs().max()) <= 1 / 3 and float(w.abs().max()) > 0.3
    # a plain Conv with g = c1 and a supported geometry is the same layer
    c = Cv.Conv(16, 16, 3, 1, g=16)
    assert tuple(c.conv.weight.shape) == (16, 1, 3, 3)


def test_graph_builds_like_the_reference(golden):
    """Before this feature: "module 'DWConv' is outside the DEAL-YOLO hot path"."""
    G = golden("dwconv")
    m = _model()
    from ultralytics.nn.modules import DWConv
    want = U.layout(G, U.MODEL)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want) and got == want
    assert sum(p.numel() for p in m.parameters()) == int(G[f"{U.MODEL}/n_params"]) == 857234
    assert m.stride.tolist() == [4.0, 8.0, 16.0] == G[f"{U.MODEL}/stride"].tolist()
    assert [i for i, mod in enumerate(m.model) if isinstance(mod, DWConv)] == list(U.DW_LAYERS)
    assert [(m.model[i].conv.in_channels, m.model[i].conv.out_channels) for i in U.DW_LAYERS] == list(U.DW_WIDTHS.values())
    assert all(m.model[i].conv.groups == m.model[i].conv.in_channels and m.model[i].conv.stride == (2, 2) for i in U.DW_LAYERS)
    assert all(m.model[i].type == "ultralytics.nn.modules.conv.DWConv" for i in U.DW_LAYERS)
    assert [m._cout[i] for i in U.DW_LAYERS] == [b for _, b in U.DW_WIDTHS.values()]
    m.load_state_dict(U.state(G, U.MODEL), strict=True)


def _custom():
    """A small graph with a DSConv row and a DWConv [c, 5, 1] row."""
    return dict(nc=3, scale="n", scales=dict(n=[0.33, 0.25, 1024]),
                backbone=[[-1, 1, "Conv", [64, 3, 2]], [-1, 1, "DSConv", [128]], [-1, 1, "DWConv", [128, 5, 1]], [-1, 1, "Conv", [128, 3, 2]],
                          [-1, 1, "DWConv", [256, 3, 2]], [-1, 1, "C2f", [256, True]]],
                head=[[[2, 3, 5], 1, "Detect", ["nc"]]])


def test_custom_yaml_with_dsconv_and_k5_builds():
    """Before this feature: "Conv(k=3, s=2, g=16, d=1) is outside the HIP hot path" / "module 'DSConv' is outside ..."."""
    from ultralytics.nn.modules import DSConv, DWConv
    from ultralytics.nn.tasks import DetectionModel
    m = DetectionModel(_custom(), ch=3, verbose=False)
    assert isinstance(m.model[1], DSConv) and isinstance(m.model[2], DWConv)
    assert tuple(m.model[1].dwconv.conv.weight.shape) == (16, 1, 3, 3) and tuple(m.model[1].pwconv.conv.weight.shape) == (32, 16, 1, 1)
    assert tuple(m.model[2].conv.weight.shape) == (32, 1, 5, 5) and m.model[2].conv.padding == (2, 2)
    assert tuple(m.model[4].conv.weight.shape) == (64, 1, 3, 3)
    assert m._cout[:5] == [16, 32, 32, 32, 64] and m.stride.tolist() == [2.0, 4.0, 8.0]  # DSConv's factor is 1, DWConv's is args[3]
    assert m.model[1].type == "ultralytics.nn.modules.conv.DSConv"


REFUSED = [(dict(c1=16, c2=24), "c2=24"),        # gcd(c1, c2) = 8 != c1
           (dict(c1=16, c2=48), "c2=48"),        # multiplier 3
           (dict(c1=16, c2=16, k=1), "k=1"), (dict(c1=16, c2=16, k=7), "k=7"),
           (dict(c1=16, c2=16, k=3, d=2), "d=2"),  # dilation
           (dict(c1=12, c2=12, k=3), "c1=12"),   # a ragged width
           (dict(c1=16, c2=16, k=3, s=3), "s=3")]


@pytest.mark.parametrize("kw,what", REFUSED)
def test_unsupported_arguments_raise(kw, what):
    from ultralytics.nn.modules import DWConv
    with pytest.raises(NotImplementedError, match=r"supported: depthwise g == c1, c1 % 8 == 0, c2 / c1 in 1\|2, k in 3\|5, s in 1\|2, d=1") as e:
        DWConv(**kw)
    assert what in str(e.value) and str(e.value).startswith("DWConv(")


def test_other_groupings_of_a_plain_conv_raise():
    from ultralytics.nn.modules import Conv, DSConv
    for g in (2, 4, 8):
        with pytest.raises(NotImplementedError, match="supported: depthwise g == c1") as e:
            Conv(16, 16, 3, 1, g=g)
        assert f"g={g}" in str(e.value) and str(e.value).startswith("Conv(")
    with pytest.raises(NotImplementedError, match="c1=12"):
        DSConv(12, 16)
    with pytest.raises(NotImplementedError, match=r"k in 1\|3, s in 1\|2, g=d=1"):  # the dense refusals are what they were
        Conv(16, 16, 5, 1)


def test_unsupported_rows_raise_in_the_parser():
    from ultralytics.nn.tasks import DetectionModel
    for row, what in (([-1, 1, "DWConv", [128, 7, 1]], "k=7"), ([-1, 1, "DWConv", [192, 3, 1]], "c2=48"), ([-1, 1, "DWConv", [128, 3, 1, 2]], "d=2")):
        d = _custom()
        d["backbone"][2] = row
        with pytest.raises(NotImplementedError, match="supported: depthwise") as e:
            DetectionModel(d, ch=3, verbose=False)
        assert what in str(e.value) and "layer 2 (DWConv)" in str(e.value)
    d = _custom()
    d["backbone"][1] = [-1, 1, "GhostConv", [128]]
    with pytest.raises(NotImplementedError, match="outside the DEAL-YOLO hot path"):
        DetectionModel(d, ch=3, verbose=False)


def test_flat_layout_puts_the_depthwise_weights_in_the_decayed_segment():
    from ultralytics.hip.runtime import Runtime
    m = _model()
    rt = object.__new__(Runtime)
    rt.root, rt.eng = m, SimpleNamespace(device=torch.device("cpu"))
    rt._flatten()
    nb = len(m.yaml["backbone"])
    for i in U.DW_LAYERS:
        w, g, b = (f"model.{i}.{k}" for k in ("conv.weight", "bn.weight", "bn.bias"))
        assert (rt.param_group[w], rt.param_group[g], rt.param_group[b]) == (1, 2, 0)
        seg = sum(rt.param_off[w] >= e for e in rt.seg_bounds)
        assert seg == (1 if i >= nb else 4), (w, seg)  # [neck + head: bias | decayed | norm][backbone: bias | decayed | norm]
        assert rt.param_off[w] % 8 == 0 and m.model[i].conv.weight.data.data_ptr() == rt.flat_p[rt.param_off[w]:].data_ptr()


def test_fuse_keeps_the_grouped_weight(golden):
    G = golden("dwconv")
    m = _model()
    m.load_state_dict(U.state(G, U.MODEL), strict=True)
    conv, bn = m.model[1].conv, m.model[1].bn
    scale = bn.weight.detach() / torch.sqrt(bn.eps + bn.running_var)
    want_w, want_b = conv.weight.detach() * scale.view(-1, 1, 1, 1), bn.bias.detach() - bn.running_mean * scale
    m.fuse()
    for i in U.DW_LAYERS:
        c1, c2 = U.DW_WIDTHS[i]
        f = m.model[i].conv
        assert tuple(f.weight.shape) == (c2, 1, 3, 3) and f.groups == c1 and f.bias is not None and not hasattr(m.model[i], "bn")
    assert torch.allclose(m.model[1].conv.weight, want_w) and torch.allclose(m.model[1].conv.bias, want_b)
    d = __import__("ultralytics.nn.tasks", fromlist=["DetectionModel"]).DetectionModel(_custom(), ch=3, verbose=False).fuse()
    assert tuple(d.model[1].dwconv.conv.weight.shape) == (16, 1, 3, 3) and tuple(d.model[2].conv.weight.shape) == (32, 1, 5, 5)


# ----------------------------------------------------------------------------- the backward form
def test_depthwise_is_a_fact_of_conv_bwd_form(monkeypatch):
    """Whatever the other facts and switches say, a depthwise layer's form materialises d(raw): the apply launch, then weight
    gradient + input gradient (input gradient alone when frozen, nothing when frozen and the input needs no gradient); its reduce and
    its shortcut are those of the same facts without it.  The field is the last one and defaults to False, so every tuple
    tests/test_host_conv_bwd_form.py builds is a non-depthwise one: that file, unchanged, is what pins the other answers."""
    from ultralytics.hip import DY_ACT_NONE, DY_ACT_SILU
    from ultralytics.hip import engine as E
    Fc = E.ConvBwdFacts
    assert Fc._fields[-1] == "depthwise" and Fc._field_defaults["depthwise"] is False
    bools = [f for f in Fc._fields if f not in ("act", "x_kind", "depthwise")]
    static, flow = bools[:bools.index("reduced")], bools[bools.index("reduced"):]
    # the product of the layer's facts with the dataflow facts at their defaults, and the product of the dataflow facts over a plain
    # layer (they bear on the reduce and the shortcut only): the enumeration of tests/test_host_conv_bwd_form.py
    combos = [dict(zip(static, v)) for v in itertools.product((False, True), repeat=len(static))]
    combos += [dict(dict.fromkeys(static, False), trainable=t, acc=a, **dict(zip(flow, v))) for t in (False, True) for a in (False, True)
               for v in itertools.product((False, True), repeat=len(flow))]
    for acc_on, wg, fused, frozen_dg in ((False,) * 4, (True, True, True, True)):
        for n, v in zip(("BN_ACC", "BN_WGRAD", "WGRAD_DGRAD", "FROZEN_DGRAD"), (acc_on, wg, fused, frozen_dg)):
            monkeypatch.setattr(E, n, v)
        for kw in combos:
            for act, kind in ((DY_ACT_SILU, "plain"), (DY_ACT_NONE, "seg")):
                f = Fc(**{**dict.fromkeys(flow, False), **kw}, act=act, x_kind=kind)
                form = E.conv_bwd_form(f._replace(depthwise=True))
                if not f.trainable and not f.planes and not f.x_grad:
                    assert form.launch == E.BWD_NONE and form.draw == E.DRAW_NONE and not form.wgrad, (f, form)
                else:
                    assert form.launch == E.BWD_APPLY and form.draw in (E.DRAW_SHARED, E.DRAW_OWN) and form.wgrad == f.trainable, (f, form)
                plain = E.conv_bwd_form(f)
                assert (form.reduce, form.shortcut) == (plain.reduce, plain.shortcut), (f, form, plain)
    # the engine gives a depthwise spec no accumulators: its reduce is the three-launch one
    f = Fc(trainable=True, acc=False, act=DY_ACT_SILU, k1s1=False, ld=False, whole_in=True, whole_out=True, raw_dense=True, x_kind="plain",
           x_grad=True, planes=False, branch=False, side_wgrad=False, deferred=True, fused_ok=False, dgrad_ok=False, depthwise=True)
    assert E.conv_bwd_form(f) == E.ConvBwdForm(E.RED_3L, E.RES_NONE, E.BWD_APPLY, E.DRAW_SHARED, True)
    assert E.conv_bwd_form(f._replace(trainable=False)) == E.ConvBwdForm(E.RED_3L, E.RES_NONE, E.BWD_APPLY, E.DRAW_SHARED, False)
    assert E.conv_bwd_form(f._replace(trainable=False, x_grad=False)).launch == E.BWD_NONE


def test_conv_spec_knows_the_geometry():
    from ultralytics.hip.engine import ConvSpec
    w = torch.zeros(32, 1, 3, 3)
    sp = ConvSpec("dw", w, None, None, 3, 2, 1, groups=16)
    assert (sp.cin, sp.cout, sp.groups, sp.mult, sp.dw) == (16, 32, 16, 2, True)
    sp = ConvSpec("dense", torch.zeros(32, 16, 3, 3), None, None, 3, 2, 1)
    assert (sp.cin, sp.cout, sp.groups, sp.mult, sp.dw) == (16, 32, 1, 1, False)


def test_soap_refuses_a_depthwise_weight_by_name():
    """optimizer='SOAP' on a graph with depthwise weights: the grouped HIP step names the (C, 1, k, k) tensor and raises; it does not
    silently mis-shape.  The refusal keys on the layer being grouped (``grouped``: the names StepPlan hands over), not on the shape: a
    dense convolution over one input channel has the same shape and is not refused.  (A host test: the refusal comes before anything
    touches the device.)"""
    from ultralytics.hip.soap import SoapHip, SoapTable
    views = [("model.0.conv.weight", 0, 16 * 3 * 9, (16, 3, 3, 3), 1), ("model.1.conv.weight", 432, 32 * 9, (32, 1, 3, 3), 1)]
    z = torch.zeros(1024)
    with pytest.raises(NotImplementedError, match=r"model\.1\.conv\.weight.*\(32, 1, 3, 3\).*\(C, 1, k, k\)"):
        SoapHip(views, z, z, z, z, grouped={"model.1.conv.weight"})
    so = SoapHip(views, z, z, z, z)  # the same shapes, nothing grouped: built as before
    assert len(so.table.entries) == 2 and len(SoapTable(views).entries) == 2


def test_a_fused_depthwise_layer_never_takes_the_cout_split():
    """Conv._build_specs splits a fused DENSE 3x3 conv of 64 m + 16 / 32 outputs into two launches; a depthwise layer of such a width
    (96: DWConv(96, 96, 3, 1), DSConv(96, .).dwconv) keeps its one spec -- the parts would be read as dense (c2, 1, 3, 3) weights."""
    from ultralytics.nn.modules import Conv, DSConv, DWConv
    from ultralytics.nn.tasks import BaseModel

    def fused(m):
        h = BaseModel()
        h.m, h.is_fused = m, lambda thresh=10: False
        h.fuse()
        return m

    def specs_of(conv):
        calls = []
        conv._build_specs(SimpleNamespace(make_spec=lambda key, *a, **k: calls.append(key)))
        return calls, conv.__dict__["_split"]

    for conv in (fused(DWConv(96, 96, 3, 1)), fused(DSConv(96, 64)).dwconv, fused(DWConv(48, 96, 3, 1)), fused(DWConv(160, 160, 3, 1))):
        assert conv.conv.groups == conv.conv.in_channels and conv.conv.bias is not None and not hasattr(conv, "bn")
        calls, split = specs_of(conv)
        assert split is None and calls == [id(conv)]
    calls, split = specs_of(fused(Conv(32, 96, 3, 1)))  # the dense layer of that width still splits
    assert split is not None and split[0] == 64 and len(calls) == 3


def test_bottleneck_refuses_a_grouped_second_convolution_at_build():
    """A Bottleneck's cv2 adds the shortcut in its epilogue and C2f.cv1 writes two planes; the depthwise kernels take neither.  C2f.cv1 is
    1x1 (never depthwise); Bottleneck(g != 1) is refused where it is built, as before this feature, now by name."""
    from ultralytics.nn.modules import C2f
    from ultralytics.nn.modules.block import Bottleneck
    for build in (lambda: Bottleneck(16, 16, True, g=16), lambda: Bottleneck(16, 16, False, g=2), lambda: C2f(32, 32, 1, True, g=16)):
        with pytest.raises(NotImplementedError, match=r"Bottleneck\(c1=16, c2=16, g=\d+\) is outside the HIP hot path"):
            build()


# ----------------------------------------------------------------------------- header and binding
def test_header_declares_and_the_library_binds_the_entry_points():
    import ctypes as C
    from ultralytics.hip import SIGNATURES, lib
    txt = open(os.path.join(ROOT, "include", "dealyolo_hip.h")).read()
    for name, nargs in (("dy_dwconv_supported", 4), ("dy_dwconv_num_partials", 7), ("dy_dwconv_wgrad_slabs", 7), ("dy_dwconv_forward", 16),
                        ("dy_dwconv_input_grad", 14), ("dy_dwconv_wgrad", 15)):
        assert f"int {name}(" in txt
        res, args = SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
        assert getattr(lib(), name).argtypes == list(args)
    assert "conv.py:106-111" in txt and ":113-122" in txt  # the reference lines the entries replace
    L = lib()
    ok = [(8, 1, 3, 1), (8, 2, 5, 2), (24, 2, 3, 2), (64, 1, 5, 1), (512, 2, 3, 2)]
    bad = [(12, 1, 3, 1), (0, 1, 3, 1), (4, 1, 3, 1), (16, 3, 3, 1), (16, 0, 3, 1), (16, 1, 1, 1), (16, 1, 7, 1), (16, 1, 3, 3), (16, 1, 3, 0), (-8, 1, 3, 1)]
    assert all(L.dy_dwconv_supported(*a) == 1 for a in ok) and all(L.dy_dwconv_supported(*a) == 0 for a in bad)
    assert L.dy_dwconv_num_partials(1, 4, 4, 12, 1, 3, 1) == -1 and L.dy_dwconv_wgrad_slabs(0, 4, 4, 16, 1, 3, 1) == -1
    # dy_conv_geometry keeps refusing k = 5: the depthwise entries are separate
    g = [C.c_int() for _ in range(8)]
    assert L.dy_conv_geometry(16, 16, 5, 1, *[C.byref(v) for v in g]) != 0
    # refusals need no device: nothing is launched (host numbers stand in for pointers)
    ARG, ALIGN = -1, -3
    base = dict(x=4096, ldx=16, w=8192, bias=0, y=16384, ldy=32, part=0, n=1, H=4, W=4, C1=16, m=2, k=3, s=2, epi=0)

    def fwd(**kw):
        a = dict(base, **kw)
        return L.dy_dwconv_forward(a["x"], a["ldx"], a["w"], a["bias"], a["y"], a["ldy"], a["part"], a["n"], a["H"], a["W"], a["C1"], a["m"],
                                   a["k"], a["s"], a["epi"], None)

    def dgrad(draw=4096, lddy=32, w=8192, dx=16384, lddx=16, **kw):
        a = dict(base, **kw)
        return L.dy_dwconv_input_grad(draw, lddy, w, dx, lddx, 0, a["n"], a["H"], a["W"], a["C1"], a["m"], a["k"], a["s"], None)

    def wgrad(x=4096, ldx=16, draw=8192, lddy=32, slabs=16384, dw=32768, **kw):
        a = dict(base, **kw)
        return L.dy_dwconv_wgrad(x, ldx, draw, lddy, slabs, dw, 0, a["n"], a["H"], a["W"], a["C1"], a["m"], a["k"], a["s"], None)

    assert fwd(x=0) == ARG and fwd(w=0) == ARG and fwd(y=0) == ARG and fwd(n=0) == ARG and fwd(H=0) == ARG and fwd(W=0) == ARG
    assert fwd(C1=12, ldx=16) == ARG and fwd(m=3, ldy=48) == ARG and fwd(k=7) == ARG and fwd(s=3) == ARG
    assert fwd(epi=1) == ARG and fwd(epi=2) == ARG and fwd(epi=4, bias=64) == ARG and fwd(epi=3, bias=64, part=64) == ARG and fwd(epi=8) == ARG
    assert fwd(ldx=8) == ARG and fwd(ldy=24) == ARG                                                  # pitches below the width
    assert fwd(ldx=20) == ALIGN and fwd(ldy=36) == ALIGN                                             # pitches off the granule
    assert fwd(x=4104) == ALIGN and fwd(y=16392) == ALIGN and fwd(w=8196) == ALIGN and fwd(epi=2, bias=72) == ALIGN and fwd(epi=1, part=72) == ALIGN
    assert dgrad(draw=0) == ARG and dgrad(w=0) == ARG and dgrad(C1=12) == ARG and dgrad(k=1) == ARG and dgrad(lddy=24) == ARG and dgrad(lddx=8) == ARG
    assert dgrad(draw=4104) == ALIGN and dgrad(dx=16392) == ALIGN and dgrad(lddy=36) == ALIGN and dgrad(lddx=20) == ALIGN and dgrad(w=8200) == ALIGN
    assert dgrad(dx=0) == 0                                                                          # a null destination: no launch, no error
    assert wgrad(x=0) == ARG and wgrad(draw=0) == ARG and wgrad(slabs=0) == ARG and wgrad(dw=0) == ARG and wgrad(m=4) == ARG and wgrad(ldx=8) == ARG
    assert wgrad(x=4104) == ALIGN and wgrad(draw=8200) == ALIGN and wgrad(slabs=16392) == ALIGN and wgrad(dw=32776) == ALIGN and wgrad(ldx=20) == ALIGN


# ----------------------------------------------------------------------------- checkpoints
def test_reference_written_checkpoint_rebuilds(golden):
    """tests/golden/ref_ckpt_dw.pt: a whole-module fp16 pickle written by the REFERENCE's classes; its module path
    ultralytics.nn.modules.conv.DWConv resolves to this package's class."""
    from ultralytics.nn.modules import DWConv
    from ultralytics.nn.tasks import DetectionModel, _rebuild, attempt_load_weights, torch_safe_load
    G = golden("dwconv")
    ckpt, _ = torch_safe_load(U.CKPT)
    obj = ckpt["model"]
    assert [type(obj.model[i]) for i in U.DW_LAYERS] == [DWConv] * 5
    assert sum(1 for row in obj.yaml["backbone"] + obj.yaml["head"] if row[2] == "DWConv") == 5
    m = _rebuild(obj, ckpt)
    assert isinstance(m, DetectionModel)
    assert [m.model[i].conv.in_channels for i in U.DW_LAYERS] == G["ckpt/dw_channels"].tolist() == [8, 16, 32, 16, 32]
    want = U.state(G, "ckpt")
    got = m.state_dict()
    assert list(want) == list(got)
    for k, v in want.items():
        assert torch.equal(got[k].float(), (v.half().float() if v.is_floating_point() else v.float())), k
    assert not attempt_load_weights(U.CKPT).training


def test_checkpoint_roundtrip_in_the_reference_format(tmp_path):
    from ultralytics.nn.modules import DWConv
    from ultralytics.nn.tasks import attempt_load_weights, save_reference_format, torch_safe_load
    m = _model()
    path = save_reference_format(str(tmp_path / "last.pt"), m, updates=4, epoch=1, train_args={"imgsz": 64})
    obj = torch_safe_load(path)[0]["model"]
    assert next(obj.parameters()).dtype == torch.float16 and all("rt" not in mod.__dict__ for mod in obj.modules())
    assert [type(obj.model[i]) for i in U.DW_LAYERS] == [DWConv] * 5
    back = attempt_load_weights(path)
    for (k, a), (_, b) in zip(m.state_dict().items(), back.state_dict().items()):
        assert torch.equal(a.half().float() if a.is_floating_point() else a, b.float() if a.is_floating_point() else b), k
