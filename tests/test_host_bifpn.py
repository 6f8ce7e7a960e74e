"""CPU: Fusion in 'bifpn' mode (reference nn/extra_modules/block.py:453-490) -- the float64 restatement tests/bifpn_ref.py against
the reference's stored fp32 values and against torch's autograd; the bounds of tests/bifpn_util.py against an fp32 evaluation; the
module, the parser, the YAML, the flat parameter layout, the header and the checkpoints."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

import bifpn_ref as R
import bifpn_util as U
from conftest import CFG_DIR, ROOT
from golden.cases import rnd

U32 = 2.0 ** -24


def _nhwc(t):
    return t.permute(0, 2, 3, 1).double().numpy()


def _model(name=U.MODEL):
    from ultralytics.nn.tasks import DetectionModel
    return DetectionModel(os.path.join(CFG_DIR, name + ".yaml"), ch=3, verbose=False)


# ----------------------------------------------------------------------------- the restatement against the reference's values
@pytest.mark.parametrize("case", list(U.MODULE_CASES))
def test_restatement_reproduces_the_reference(golden, case):
    """y, every gx and g(fusion_weight) of the reference module (fp32, stored) against the float64 restatement on the same inputs, to
    the round-off of the fp32 reference: per element (n + 3) 2^-24 of the terms' absolute sum for y and gx (f: n roundings, a product,
    n - 1 additions, + 1), and for the parameter gradient a float32 sum of E elements in torch's pairwise order: (log2 E + 8) 2^-24 of
    sum |dy x| per dot product, carried through the Jacobian."""
    G = golden("bifpn")
    C, H, W, p = U.MODULE_CASES[case]
    seed, n = U.MODULE_SEEDS[case], len(p)
    xs = [_nhwc(rnd(10 * seed + i, U.BATCH, C, H, W)) for i in range(n)]
    gy = _nhwc(rnd(10 * seed + 9, U.BATCH, C, H, W))
    p32 = np.asarray(p, dtype=np.float32).astype(np.float64)
    f = R.forward(xs, p32)
    b = R.backward(xs, p32, gy)
    k = (n + 3) * U32
    y = _nhwc(G.t(f"mod/{case}/y"))
    assert np.all(np.abs(y - f["y"]) <= k * f["mag"] + 1e-30)
    for i in range(n):
        gx = _nhwc(G.t(f"mod/{case}/gx{i}"))
        assert np.all(np.abs(gx - b["dx"][i]) <= k * np.abs(b["dx"][i]) + 1e-30), i
        if p[i] <= 0:
            assert not gx.any()
    gp = G.t(f"mod/{case}/gp").double().numpy()
    fw, s, mask = R.weights(p32)
    eg = (np.log2(gy.size) + 8) * U32 * b["gmag"]
    bound = (eg + float((fw * eg).sum()) + (n + 4) * U32 * (np.abs(b["g"]) + float((fw * np.abs(b["g"])).sum()))) / s
    print(case, "gp", gp.tolist(), "restatement", b["dp"].tolist(), "bound", bound.tolist())
    assert np.all(np.abs(gp - b["dp"]) <= np.where(mask, bound, 0.0))
    assert abs(float((np.maximum(p32, 0) * b["dp"]).sum())) <= 1e-12 * float(np.abs(b["g"]).sum())  # sum_j relu(p_j) dL/dp_j = 0


@pytest.mark.parametrize("p", [(1.0, 1.0), (0.7, 1.9), (-0.5, 1.2), (1.3, 0.4, 2.1), (0.9, -0.3, 1.6), (0.0, 2.0, 1.0)])
def test_restatement_equals_autograd_in_float64(p):
    n = len(p)
    rng = np.random.default_rng(5)
    xs = [rng.standard_normal((2, 5, 7, 8)) for _ in range(n)]
    dy = rng.standard_normal((2, 5, 7, 8))
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    xt = [torch.from_numpy(x).requires_grad_(True) for x in xs]
    w = torch.relu(pt)  # the formulas as the module docstring states them: w = relu(p), f = w / s, y = sum_i f[i] x[i]
    f_ = w / w.sum()
    y = sum(f_[i] * xt[i] for i in range(n))
    y.backward(torch.from_numpy(dy))
    f, b = R.forward(xs, p), R.backward(xs, p, dy)
    assert np.abs(y.detach().numpy() - f["y"]).max() < 1e-14
    for i in range(n):
        assert np.abs(xt[i].grad.numpy() - b["dx"][i]).max() < 1e-14
    assert np.abs(pt.grad.numpy() - b["dp"]).max() < 1e-12 * max(1.0, float(np.abs(b["g"]).max()))
    assert all(b["dp"][j] == 0 and not b["dx"][j].any() for j in range(n) if p[j] <= 0)


def test_all_weights_nonpositive_give_nan():
    """0 / 0: the reference returns NaN, the restatement too, and nothing guards it."""
    x = np.ones((1, 2, 2, 8))
    assert np.isnan(R.forward([x, x], (-1.0, 0.0))["y"]).all()
    pt = torch.tensor([-1.0, 0.0])
    w = torch.relu(pt)
    assert torch.isnan(w / w.sum()).all()


def test_up2_and_fold2_are_adjoint():
    rng = np.random.default_rng(0)
    x, g = rng.standard_normal((2, 3, 5, 8)), rng.standard_normal((2, 6, 10, 8))
    assert R.up2(x).shape == g.shape and bool((R.up2(x)[:, 3, 5] == x[:, 1, 2]).all())
    assert abs(float((R.up2(x) * g).sum() - (x * R.fold2(g)).sum())) < 1e-10


# ----------------------------------------------------------------------------- the counted bounds against an fp32 evaluation
@pytest.mark.parametrize("name", list(U.KERNEL_CASES))
def test_fp32_evaluation_meets_the_counted_bounds(name):
    """What tests/test_gpu_bifpn.py asserts of the kernels, asserted here of a float32 numpy evaluation in the documented order
    (sequential per-item chains are replaced by numpy's pairwise sums, which round less): equality on the exact inputs, the counted
    bounds on the normal ones."""
    N, H, W, C = U.KERNEL_CASES[name][:4]
    for n, up in U.variants(name):
        full = lambda xs: [R.up2(x) if i == up else x for i, x in enumerate(xs)]  # noqa: E731
        for p in U.EXACT_P[n]:
            xs, dy, old = U.exact_inputs(name, n, up)
            xs = full(xs)
            f, b = R.forward(xs, p), R.backward(xs, p, dy)
            assert float(b["gmag"].max()) < 2 ** 22  # every sum an integer below 2^24, every f g exact in fp32
            assert np.array_equal(f["y"].astype(np.float16).astype(np.float64), f["y"])
            assert all(np.array_equal(d.astype(np.float16).astype(np.float64), d) for d in b["dx"])
            assert np.array_equal(b["g"].astype(np.float32).astype(np.float64), b["g"])
            assert np.array_equal(b["dp"].astype(np.float32).astype(np.float64), b["dp"])
        p = np.asarray(U.NORMAL_P[n], dtype=np.float32)
        xs, dy, old = U.normal_inputs(name, n, up)
        xs = full(xs)
        p64 = p.astype(np.float64)
        f, b = R.forward(xs, p64), R.backward(xs, p64, dy)
        w = np.maximum(p, np.float32(0))
        s = (w[0] + w[1]) + (w[2] if n > 2 else np.float32(0))
        f32 = w / s
        acc = f32[0] * xs[0].astype(np.float32) + f32[1] * xs[1].astype(np.float32)
        if n > 2:
            acc = acc + f32[2] * xs[2].astype(np.float32)
        y16 = acc.astype(np.float16).astype(np.float64)
        assert np.all(np.abs(y16 - f["y"]) <= U.bound_y(f["y"], f["mag"], n))
        g32 = np.array([float((dy.astype(np.float32) * x.astype(np.float32)).sum(dtype=np.float32)) for x in xs])
        assert np.all(np.abs(g32 - b["g"]) <= U.bound_g(b["gmag"], N * H * W, C))
        bd = U.bound_dp(p64, b["g"], b["gmag"], N * H * W, C)
        assert np.all(bd > 0) and np.all(bd < 1e-2 * np.abs(b["gmag"]).max())  # a bound that says something


def test_num_partials_formula():
    assert U.num_partials(2 * 6 * 10, 8) == 1 and U.num_partials(2 * 40 * 40, 16) == 7 and U.num_partials(64 * 160 * 160, 32) == 1024
    assert U.k_dot(2 * 40 * 40, 16) == 2 * 8 * 4 + 9


# ----------------------------------------------------------------------------- module, parser, YAML
def test_module_keys_class_path_and_attributes():
    from ultralytics.nn.extra_modules import Fusion as exported
    from ultralytics.nn.extra_modules.block import Fusion
    assert exported is Fusion and Fusion.__module__ == "ultralytics.nn.extra_modules.block"
    for n in (2, 3):
        m = Fusion([16] * n, "bifpn")
        assert list(m.state_dict()) == ["fusion_weight"]
        p = m.fusion_weight
        assert isinstance(p, torch.nn.Parameter) and p.dtype == torch.float32 and tuple(p.shape) == (n,) and bool((p == 1).all()) and p.requires_grad
        own = {k for k in list(m.__dict__) + list(m._parameters) + list(m._modules) if not k.startswith("_") and k not in ("training", "rt")}
        assert own == {"fusion", "fusion_weight", "relu", "epsilon"}
        assert m.fusion == "bifpn" and isinstance(m.relu, torch.nn.ReLU) and m.epsilon == 1e-4
    assert Fusion([16, 16]).fusion == "bifpn"  # the reference's default


def test_concat_mode_has_no_parameters_and_the_concat_widths():
    from ultralytics.nn.extra_modules.block import Fusion
    from ultralytics.nn.tasks import DetectionModel
    m = Fusion([16, 32, 8], "concat")
    assert not list(m.parameters()) and m.fusion == "concat"
    rows = [[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "Conv", [32, 3, 1]], [[-1, 0], 1, "Fusion", ["mode"]]]
    d = {"nc": 6, "mode": "concat", "scales": {"n": [1.0, 1.0, 1024]}, "scale": "n", "backbone": rows, "head": [[[-1], 1, "Detect", ["nc"]]]}
    dm = DetectionModel(d, verbose=False)
    assert dm._cout[:3] == [16, 32, 48] and dm.model[2].fusion == "concat" and dm.model[3].cv2[0][0].conv.in_channels == 48
    d["mode"] = "bifpn"
    d["backbone"][1][3] = [16, 3, 1]
    dm = DetectionModel(d, verbose=False)
    assert dm._cout[:3] == [16, 16, 16] and tuple(dm.model[2].fusion_weight.shape) == (2,)


@pytest.mark.parametrize("mode", ["weight", "adaptive", "SDI"])
def test_other_modes_raise_by_name(mode):
    from ultralytics.nn.extra_modules.block import Fusion
    with pytest.raises(NotImplementedError, match=rf"Fusion\(inc_list=\[16, 16\], fusion='{mode}'\) is outside the HIP hot path \(supported: fusion 'bifpn'"):
        Fusion([16, 16], mode)
    with pytest.raises(ValueError, match="is none of"):
        Fusion([16, 16], "mean")


@pytest.mark.parametrize("inc", [[16, 32], [12, 12], [16, 16, 16, 16], [16]])
def test_constructor_refuses_by_name(inc):
    from ultralytics.nn.extra_modules.block import Fusion
    with pytest.raises(NotImplementedError, match=r"Fusion\(inc_list=.*fusion='bifpn'\) is outside the HIP hot path \(supported: fusion 'bifpn' over 2 or 3"):
        Fusion(inc, "bifpn")


def _custom(rows, mode="bifpn", nc=6):
    return {"nc": nc, "fusion_mode": mode, "scales": {"n": [1.0, 1.0, 1024]}, "scale": "n", "backbone": rows, "head": [[[-1], 1, "Detect", ["nc"]]]}


def test_parser_refuses_by_layer():
    from ultralytics.nn.tasks import DetectionModel
    fus = lambda f: [f, 1, "Fusion", ["fusion_mode"]]  # noqa: E731
    with pytest.raises(NotImplementedError, match=r"layer 2 \(Fusion\)\(inc_list=\[32, 16\], fusion='bifpn'\) is outside the HIP hot path"):
        DetectionModel(_custom([[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "Conv", [32, 3, 1]], fus([-1, 0])]), verbose=False)
    with pytest.raises(NotImplementedError, match=r"layer 2 \(Fusion\).*reads maps of different sizes"):
        DetectionModel(_custom([[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "Conv", [16, 3, 2]], fus([-1, 0])]), verbose=False)
    with pytest.raises(NotImplementedError, match=r"layer 2 \(Fusion\) reads layer 1, which is 12 channels wide"):
        DetectionModel(_custom([[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "Conv", ["nc", 3, 1]], fus([-1, 0])], nc=12), verbose=False)
    four = [[-1, 1, "Conv", [16, 3, 2]]] + [[-1, 1, "Conv", [16, 3, 1]]] * 3 + [fus([0, 1, 2, 3])]
    with pytest.raises(NotImplementedError, match=r"layer 4 \(Fusion\)\(inc_list=\[16, 16, 16, 16\], fusion='bifpn'\)"):
        DetectionModel(_custom(four), verbose=False)
    for mode in ("weight", "adaptive", "SDI"):
        with pytest.raises(NotImplementedError, match=rf"layer 2 \(Fusion\)\(inc_list=\[16, 16\], fusion='{mode}'\)"):
            DetectionModel(_custom([[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "Conv", [16, 3, 1]], fus([-1, 0])], mode=mode), verbose=False)
    with pytest.raises(KeyError, match=r"layer 2 \(Fusion\).*top-level key"):  # a literal mode: the reference's d[args[0]] fails on it too
        DetectionModel(_custom([[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "Conv", [16, 3, 1]], [[-1, 0], 1, "Fusion", ["bifpn"]]]), verbose=False)
    three = [[-1, 1, "Conv", [16, 3, 2]]] + [[-1, 1, "Conv", [16, 3, 1]]] * 2 + [fus([0, 1, 2])]
    m = DetectionModel(_custom(three), verbose=False)  # ... and a supported row builds
    assert m._cout[:4] == [16, 16, 16, 16] and tuple(m.model[3].fusion_weight.shape) == (3,) and m.stride.tolist() == [2.0]


def test_graph_builds_like_the_reference(golden):
    from ultralytics.nn.extra_modules.block import Fusion
    G = golden("bifpn")
    m = _model()
    assert [type(m.model[i]) for i in U.FUSION_LAYERS] == [Fusion] * 3
    assert sum(q.numel() for q in m.parameters()) == int(G[f"{U.MODEL}/n_params"]) == 992088
    assert m.stride.tolist() == G[f"{U.MODEL}/stride"].tolist() == [4.0, 8.0, 16.0]
    want = U.layout(G, U.MODEL)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want) and got == want
    sd = m.state_dict()
    for k in U.FUSION_KEYS:
        assert tuple(sd[k].shape) == (2,) and sd[k].dtype == torch.float32 and bool((sd[k] == 1).all())
    assert [k for k in sd if "fusion" in k] == list(U.FUSION_KEYS)
    assert [m._cout[i] for i in U.FUSION_LAYERS] == list(U.FUSION_WIDTHS.values())
    assert all(m.model[i].type == "ultralytics.nn.extra_modules.block.Fusion" for i in U.FUSION_LAYERS)
    # the same rows as the default graph, the three fused rows and the mode key apart
    a = yaml.safe_load(open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2-BiFPN.yaml")))
    d = yaml.safe_load(open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2.yaml")))
    assert a["fusion_mode"] == "bifpn" and "fusion_mode" not in d
    for i, (ra, rd) in enumerate(zip(a["backbone"] + a["head"], d["backbone"] + d["head"])):
        if i in U.FUSION_LAYERS:
            assert ra == [rd[0], 1, "Fusion", ["fusion_mode"]] and rd[2] in ("Concat", "Add"), i
        else:
            assert ra == rd, i
    assert (a["head"][19 - 8][2], a["head"][22 - 8][2]) == ("Concat", "Concat")
    m.load_state_dict(U.state(G, U.MODEL), strict=True)
    assert all(bool((m.state_dict()[k] >= 0.5).all()) for k in U.FUSION_KEYS)


def test_decayed_group_in_the_neck_and_head_segment(golden):
    """The reference's build_optimizer puts the three vectors in its decayed group (stored by the generator); hip/runtime.py sorts by
    the same rule, and they lie in the neck + head half of the flat layout: segment 1 of [bias | decayed | norm] x 2."""
    from ultralytics.hip.runtime import Runtime
    G = golden("bifpn")
    assert [str(k) for k in G[f"{U.MODEL}/decayed"]] == list(U.FUSION_KEYS)
    m = _model()
    rt = object.__new__(Runtime)
    rt.root, rt.eng = m, SimpleNamespace(device=torch.device("cpu"))
    rt._flatten()
    params = dict(m.named_parameters())
    for k in U.FUSION_KEYS:
        o = rt.param_off[k]
        assert rt.param_group[k] == 1 and rt.seg_bounds[0] <= o < rt.seg_bounds[1] <= rt.bucket_split, k
        assert o % 8 == 0 and params[k].data.data_ptr() == rt.flat_p[o:].data_ptr() and params[k].grad.data_ptr() == rt.flat_g[o:].data_ptr()
        assert bool((rt.flat_p[o:o + 2] == 1).all()) and rt.frozen[o:o + 8].tolist() == [0, 0, 1, 1, 1, 1, 1, 1]  # (the padding never moves)


def test_fuse_leaves_the_layer_alone():
    m = _model().eval()
    before = {k: m.state_dict()[k].clone() for k in U.FUSION_KEYS}
    m.fuse()
    assert not hasattr(m.model[10], "bn")
    for i, k in zip(U.FUSION_LAYERS, U.FUSION_KEYS):
        assert isinstance(m.model[i].fusion_weight, torch.nn.Parameter) and torch.equal(m.state_dict()[k], before[k])


def test_other_shipped_yamls_hold_no_fusion_row():
    files = sorted(glob.glob(os.path.join(CFG_DIR, "*.yaml")))
    assert len(files) > 5
    with_rows = [os.path.basename(f) for f in files
                 if any(row[2] == "Fusion" for row in (lambda d: d["backbone"] + d["head"])(yaml.safe_load(open(f))))]
    assert with_rows == ["yolov8-ASF-P2P2-BiFPN.yaml"]


def test_freeze_names_cover_the_vector():
    from ultralytics.engine.trainer import frozen_parameter_names
    names = [k for k, _ in _model().named_parameters()]
    assert "model.11.fusion_weight" in set(frozen_parameter_names(names, [11]))
    assert "model.16.fusion_weight" not in set(frozen_parameter_names(names, [11]))


def test_launch_list_tool_lists_the_graph():
    txt = open(os.path.join(ROOT, "tools", "launch_list.py")).read()
    assert '"yolov8n-ASF-P2P2-BiFPN"' in txt


# ----------------------------------------------------------------------------- header and binding
def test_header_declares_and_the_library_binds_the_entry_points():
    import ctypes as C
    from ultralytics.hip import SIGNATURES, lib
    txt = open(os.path.join(ROOT, "include", "dealyolo_hip.h")).read()
    for name, nargs in (("dy_fusion_forward", 18), ("dy_fusion_backward", 28), ("dy_fusion_wgrad_finish", 7), ("dy_fusion_num_partials", 2)):
        assert f"int {name}(" in txt
        res, args = SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
        assert getattr(lib(), name).argtypes == list(args)
    assert "block.py:453-490" in txt and "tasks.py:922-925" in txt  # the reference lines the entries replace
    assert "dy_fusion_forward" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = lib()
    for (N, H, W, C_, _, _) in U.KERNEL_CASES.values():
        assert L.dy_fusion_num_partials(N * H * W, C_) == U.num_partials(N * H * W, C_)
    assert L.dy_fusion_num_partials(64 * 160 * 160, 32) == 1024 and L.dy_fusion_num_partials(0, 8) < 0 and L.dy_fusion_num_partials(8, 12) < 0
    # refusals need no device: nothing is launched (host numbers stand in for pointers)
    ARG, ALIGN = -1, -3
    base = dict(x0=4096, ld0=16, h0=0, x1=8192, ld1=16, h1=0, x2=0, ld2=0, h2=0, p=256, y=16384, ldy=16, nops=2, n=1, H=4, W=4, C=16)

    def fwd(**kw):
        v = dict(base, **kw)
        return L.dy_fusion_forward(v["x0"], v["ld0"], v["h0"], v["x1"], v["ld1"], v["h1"], v["x2"], v["ld2"], v["h2"], v["p"], v["y"], v["ldy"],
                                   v["nops"], v["n"], v["H"], v["W"], v["C"], None)

    def bwd(ws=512, **kw):
        v = dict(base, **kw)  # (y stands for dy; the dx are the operands' own addresses)
        return L.dy_fusion_backward(v["y"], v["ldy"], v["x0"], v["ld0"], v["h0"], v["x0"], v["ld0"], 0, v["x1"], v["ld1"], v["h1"], v["x1"], v["ld1"], 0,
                                    v["x2"], v["ld2"], v["h2"], v["x2"], v["ld2"], 0, v["p"], ws, v["nops"], v["n"], v["H"], v["W"], v["C"], None)

    for f in (fwd, bwd):
        assert f(x0=0) == ARG and f(x1=0) == ARG and f(p=0) == ARG and f(y=0) == ARG and f(n=0) == ARG and f(H=0) == ARG and f(W=0) == ARG
        assert f(nops=1) == ARG and f(nops=4) == ARG and f(nops=3) == ARG  # (three operands, the third null)
        assert f(ld0=8) == ARG and f(ldy=8) == ARG and f(h1=1, H=5) == ARG and f(h0=1, W=3) == ARG
        assert f(C=12) == ALIGN and f(ld1=20) == ALIGN and f(ldy=20) == ALIGN and f(x0=4104) == ALIGN and f(y=16392) == ALIGN and f(p=258) == ALIGN
    assert bwd(ws=514) == ALIGN
    fin = lambda ws=512, parts=1, p=256, gw=1024, nops=2: L.dy_fusion_wgrad_finish(ws, parts, p, gw, nops, 0, None)  # noqa: E731
    assert fin(ws=0) == ARG and fin(p=0) == ARG and fin(gw=0) == ARG and fin(parts=0) == ARG and fin(nops=1) == ARG and fin(nops=4) == ARG
    assert fin(ws=514) == ALIGN and fin(gw=1026) == ALIGN


# ----------------------------------------------------------------------------- checkpoints
def test_reference_written_checkpoint_rebuilds(golden):
    """tests/golden/ref_ckpt_bifpn.pt: a whole-module fp16 pickle written by the REFERENCE's classes; its module path
    ultralytics.nn.extra_modules.block.Fusion resolves to this package's class, and the state_dict keys equal the stored list."""
    from ultralytics.nn.extra_modules.block import Fusion
    from ultralytics.nn.tasks import DetectionModel, _rebuild, attempt_load_weights, torch_safe_load
    G = golden("bifpn")
    ckpt, _ = torch_safe_load(U.CKPT)
    obj = ckpt["model"]
    assert [type(obj.model[i]) for i in U.FUSION_LAYERS] == [Fusion] * 3 and obj.yaml["fusion_mode"] == "bifpn"
    assert sum(1 for row in obj.yaml["backbone"] + obj.yaml["head"] if row[2] == "Fusion") == 3
    m = _rebuild(obj, ckpt)
    assert isinstance(m, DetectionModel)
    assert [m._cout[i] for i in U.FUSION_LAYERS] == G["ckpt/fusion_channels"].tolist()
    want = U.state(G, "ckpt")
    got = m.state_dict()
    assert list(got) == [str(k) for k in G["ckpt/state_keys"]] == list(want)
    for k, v in want.items():
        assert torch.equal(got[k].float(), (v.half().float() if v.is_floating_point() else v.float())), k
    loaded = attempt_load_weights(U.CKPT)
    assert not loaded.training
    for k in U.FUSION_KEYS:
        assert loaded.state_dict()[k].dtype == torch.float32 and tuple(loaded.state_dict()[k].shape) == (2,)


def test_checkpoint_roundtrip_in_the_reference_format(tmp_path):
    from ultralytics.nn.extra_modules.block import Fusion
    from ultralytics.nn.tasks import attempt_load_weights, save_reference_format, torch_safe_load
    m = _model()
    with torch.no_grad():
        m.model[11].fusion_weight.copy_(torch.tensor([0.75, 1.5]))
    path = save_reference_format(str(tmp_path / "last.pt"), m, updates=4, epoch=1, train_args={"imgsz": 64})
    obj = torch_safe_load(path)[0]["model"]
    assert next(obj.parameters()).dtype == torch.float16 and all("rt" not in mod.__dict__ for mod in obj.modules())
    assert [type(obj.model[i]) for i in U.FUSION_LAYERS] == [Fusion] * 3
    back = attempt_load_weights(path)
    assert back.state_dict()["model.11.fusion_weight"].tolist() == [0.75, 1.5]
    for (k, a), (_, b) in zip(m.state_dict().items(), back.state_dict().items()):
        assert torch.equal(a.half().float() if a.is_floating_point() else a, b.float() if a.is_floating_point() else b), k
