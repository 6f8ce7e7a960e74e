"""CPU: SimAM (reference nn/extra_modules/attention.py:53-77) -- the float64 restatement tests/simam_ref.py against the reference's
stored fp32 values, against torch's autograd and against the closed forms; its counted bounds against an fp32 evaluation; the module,
the parser, the YAML, the header and the checkpoints."""
import glob
import os

import numpy as np
import pytest
import torch
import yaml

import simam_ref as R
import simam_util as U
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
    """y and gx of the reference module (fp32, stored) against the float64 restatement on the same inputs, to the round-off of an fp32
    evaluation: tests/simam_ref.py's per-element fp32 terms (its bound without the fp16 rounding is not separable, so the whole bound
    is used: it is the fp32 error plus half an fp16 ulp, and the reference's own fp32 sums over a plane of M values add
    (log2 M + 2) 2^-24 of the same magnitudes) -- asserted as the relative Frobenius error staying below 1e-4 for the plain cases and
    1e-3 for the offset case, where fp32 loses log2(offset / spread) bits of d."""
    G = golden("simam")
    C, H, W, lam, off, spread = U.MODULE_CASES[case]
    seed = U.MODULE_SEEDS[case]
    x = _nhwc(off + spread * rnd(10 * seed, U.BATCH, C, H, W))
    gy = _nhwc(rnd(10 * seed + 9, U.BATCH, C, H, W))
    b = R.backward(x, gy, lam)
    y, gx = _nhwc(G.t(f"mod/{case}/y")), _nhwc(G.t(f"mod/{case}/gx"))
    ey = np.linalg.norm(y - b["y"]) / np.linalg.norm(b["y"])
    eg = np.linalg.norm(gx - b["dx"]) / np.linalg.norm(b["dx"])
    print(case, f"y {ey:.2e} gx {eg:.2e}")
    lim = 1e-3 if off else 1e-4
    assert ey < lim and eg < lim


@pytest.mark.parametrize("shape,off,spread", [((2, 5, 7, 8), 0.0, 1.0), ((2, 5, 7, 8), 30.0, 0.01), ((1, 40, 40, 16), 0.0, 1.0)])
def test_restatement_equals_autograd_in_float64(shape, off, spread):
    """The reference's own lines (:72-77) in float64 under autograd against the restatement's closed-form backward."""
    rng = np.random.default_rng(5)
    x = off + spread * rng.standard_normal(shape)
    g = rng.standard_normal(shape)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).clone().requires_grad_(True)
    n = shape[1] * shape[2] - 1
    d2 = (xt - xt.mean(dim=[2, 3], keepdim=True)).pow(2)
    y = xt * torch.sigmoid(d2 / (4 * (d2.sum(dim=[2, 3], keepdim=True) / n + 1e-4)) + 0.5)
    y.backward(torch.from_numpy(g).permute(0, 3, 1, 2))
    b = R.backward(x, g, 1e-4)
    ey = np.abs(_nhwc(y.detach()) - b["y"]).max()
    ed = np.abs(_nhwc(xt.grad) - b["dx"]).max() / np.abs(b["dx"]).max()
    print(shape, off, f"y {ey:.1e} dx {ed:.1e}")
    assert ey < 1e-13 * max(1.0, abs(off)) and ed < (1e-10 if off else 1e-14)


def test_layout_free():
    rng = np.random.default_rng(1)
    x, g = rng.standard_normal((2, 5, 7, 8)), rng.standard_normal((2, 5, 7, 8))
    a = R.backward(x, g)
    b = R.backward(x.transpose(0, 3, 1, 2), g.transpose(0, 3, 1, 2), axes=(2, 3))
    assert np.array_equal(a["y"], b["y"].transpose(0, 2, 3, 1)) and np.allclose(a["dx"], b["dx"].transpose(0, 2, 3, 1), rtol=1e-13, atol=0)


def test_constant_plane_gives_sigmoid_of_one_half():
    """d = 0 everywhere: e = 0.5 whatever D is, a = sigmoid(0.5), y = x sigmoid(0.5), and dx = g sigmoid(0.5) (T = U = 0)."""
    x, g = U.const_inputs((2, 5, 7, 8))
    b = R.backward(x, g)
    s = 1.0 / (1.0 + np.exp(-0.5))
    assert np.all(b["a"] == s) and np.array_equal(b["y"], x * s) and np.array_equal(b["dx"], g * s)
    mu, inv = R.stats(x)
    assert np.array_equal(mu, x[:, 0, 0, :]) and np.allclose(inv, 1.0 / 4e-4, rtol=1e-6)
    # the property the GPU test's bit-equality rests on: x s and g s lie far from every fp16 rounding boundary (16 fp32 ulps at least)
    for v in (b["y"], b["dx"]):
        v = np.abs(v[v != 0])
        lo = v.astype(np.float16).astype(np.float64)
        ulp = np.spacing(lo.astype(np.float16)).astype(np.float64)
        frac = np.abs(v - lo) / ulp  # distance to the rounded value in fp16 ulps; 0.5 = a tie
        assert np.all(np.abs(frac - 0.5) * ulp > 32 * U32 * v)


def test_one_pixel_plane_gives_nan():
    """n = 0: 0 / 0, as the reference; nothing guards it."""
    x = np.ones((1, 1, 1, 8))
    b = R.backward(x, x)
    assert np.isnan(b["y"]).all() and np.isnan(b["dx"]).all()
    xt = torch.ones(1, 8, 1, 1)
    d2 = (xt - xt.mean(dim=[2, 3], keepdim=True)).pow(2)
    assert torch.isnan(xt * torch.sigmoid(d2 / (4 * (d2.sum(dim=[2, 3], keepdim=True) / 0 + 1e-4)) + 0.5)).all()
    two = R.forward(np.array([1.0, 3.0]).reshape(1, 1, 2, 1))  # the smallest defined plane: n = 1, S = 2, D = 4 (2 + 1e-4)
    assert np.allclose(two["y"].ravel(), np.array([1.0, 3.0]) / (1 + np.exp(-(1 / (4 * 2.0001) + 0.5))), rtol=1e-15)


# ----------------------------------------------------------------------------- the counted bounds against an fp32 evaluation
def _fp32_eval(x, g, lam, old=None):
    """The arithmetic csrc/simam.hip states, in numpy float32 (sums in float64, numpy's exp instead of the fast one)."""
    f = np.float32
    x32, g32 = x.astype(f), g.astype(f)
    M = x.shape[1] * x.shape[2]
    s, sq = x.sum(axis=(1, 2), keepdims=True), (x * x).sum(axis=(1, 2), keepdims=True)
    mu64 = s / M
    S = np.maximum(sq - s * mu64, 0.0)
    mu, inv = mu64.astype(f), (1.0 / (4.0 * (S / (M - 1) + np.float64(f(lam))))).astype(f)
    d = x32 - mu
    e = (d * d) * inv + f(0.5)
    a = f(1) / (f(1) + np.exp(-e))
    y = (x32 * a).astype(np.float16).astype(np.float64)
    q = (g32 * x32) * (a - a * a)
    qd = q * d
    T, Uu = (qd * d).astype(np.float64).sum(axis=(1, 2), keepdims=True), qd.astype(np.float64).sum(axis=(1, 2), keepdims=True)
    k1 = (4.0 * T * inv.astype(np.float64) / (M - 1)).astype(f)
    k2 = (2.0 * Uu * inv.astype(np.float64) / M).astype(f)
    r = g32 * a + ((f(2) * d) * inv * (q - k1) - k2)
    if old is not None:
        r = old.astype(f) + r
    return y, r.astype(np.float16).astype(np.float64)


@pytest.mark.parametrize("kind", ["normal", "offset", "large"])
@pytest.mark.parametrize("name", ["odd", "slice", "two_px", "map40"])
def test_fp32_evaluation_meets_the_counted_bounds(name, kind):
    """What tests/test_gpu_simam.py asserts of the kernels, asserted here of a float32 numpy evaluation of the documented arithmetic;
    and the bounds say something: below 1 % of the largest value for y, and for dx on the normal inputs."""
    shape = U.KERNEL_CASES[name][:4]
    x, g, old = dict(normal=U.normal_inputs, offset=U.offset_inputs, large=U.large_inputs)[kind](shape)
    for o in (None, old):
        b = R.backward(x, g, U.LAM)
        bd = R.bounds(x, g, U.LAM, old=o)
        y, dx = _fp32_eval(x, g, U.LAM, o)
        want = b["dx"] if o is None else b["dx"] + o
        assert np.all(np.abs(y - b["y"]) <= bd["y"]) and np.all(np.abs(dx - want) <= bd["dx"]), (name, kind)
        assert bd["y"].max() < 1e-2 * np.abs(b["y"]).max()
        if kind == "normal" and name != "two_px":
            assert np.median(bd["dx"]) < 1e-2 * np.abs(want).max()


def test_num_partials_formula():
    for name, (N, H, W, C, _, _) in U.KERNEL_CASES.items():
        assert U.num_partials(H * W, C) == U.EXPECT_PARTS[name], name
    assert [U.num_partials(m * m, c) for m, c in ((160, 32), (80, 64), (40, 128))] == [25, 13, 7]


# ----------------------------------------------------------------------------- module, parser, YAML
def test_module_keys_class_path_and_attributes():
    from ultralytics.nn.extra_modules import SimAM as exported
    from ultralytics.nn.extra_modules.attention import SimAM
    assert exported is SimAM and SimAM.__module__ == "ultralytics.nn.extra_modules.attention"
    m = SimAM()
    assert not m.state_dict() and not list(m.parameters()) and not list(m.buffers())
    own = {k for k in list(m.__dict__) + list(m._modules) if not k.startswith("_") and k not in ("training", "rt")}
    assert own == {"activaton", "e_lambda"} and isinstance(m.activaton, torch.nn.Sigmoid) and m.e_lambda == 1e-4
    assert repr(m) == "SimAM(lambda=0.000100)" and repr(SimAM(1e-2)) == "SimAM(lambda=0.010000)" and SimAM.get_module_name() == "simam"
    with pytest.raises(RuntimeError, match="GPU only"):
        m(torch.zeros(1, 8, 4, 4))


def _custom(rows, nc=6):
    return {"nc": nc, "scales": {"n": [1.0, 1.0, 1024]}, "scale": "n", "backbone": rows, "head": [[[-1], 1, "Detect", ["nc"]]]}


def test_parser_builds_and_refuses_by_layer():
    from ultralytics.nn.extra_modules.attention import SimAM
    from ultralytics.nn.tasks import DetectionModel
    m = DetectionModel(_custom([[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "SimAM", []], [0, 1, "SimAM", ["1e-2"]], [1, 1, "SimAM", [0.5]]]), verbose=False)
    assert m._cout[:4] == [16, 16, 16, 16] and [type(m.model[i]) for i in (1, 2, 3)] == [SimAM] * 3 and m.stride.tolist() == [2.0]
    assert [m.model[i].e_lambda for i in (1, 2, 3)] == [1e-4, 1e-2, 0.5] and m.model[4].cv2[0][0].conv.in_channels == 16
    with pytest.raises(NotImplementedError, match=r"layer 1 \(SimAM\) reads layer 0, which is 12 channels wide"):
        DetectionModel(_custom([[-1, 1, "Conv", ["nc", 3, 2]], [-1, 1, "SimAM", []]], nc=12), verbose=False)
    with pytest.raises(NotImplementedError, match=r"module 'SpatialGroupEnhance' is outside the DEAL-YOLO hot path"):
        DetectionModel(_custom([[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "SpatialGroupEnhance", []]]), verbose=False)


def test_graph_builds_like_the_reference(golden):
    from ultralytics.nn.extra_modules.attention import SimAM
    G = golden("simam")
    m = _model()
    assert [type(m.model[i]) for i in U.SIMAM_LAYERS] == [SimAM] * 3
    assert sum(q.numel() for q in m.parameters()) == int(G[f"{U.MODEL}/n_params"]) == U.N_PARAMS == 997202
    assert sum(q.numel() for q in _model(U.BASE).parameters()) == U.N_PARAMS
    assert m.stride.tolist() == G[f"{U.MODEL}/stride"].tolist() == [4.0, 8.0, 16.0]
    want = U.layout(G, U.MODEL)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want) and got == want
    # no new state_dict keys: the base graph's, Detect renumbered 26 -> 29 (the reference agrees: stored by the generator)
    assert int(G[f"{U.MODEL}/base_keys_equal"]) == 1
    assert [k.replace("model.26.", "model.29.") for k in _model(U.BASE).state_dict()] == list(got)
    assert not [k for k in got if any(f"model.{i}." in k for i in U.SIMAM_LAYERS)]
    assert [m._cout[i] for i in U.SIMAM_LAYERS] == list(U.SIMAM_WIDTHS.values())
    assert all(m.model[i].type == "ultralytics.nn.extra_modules.attention.SimAM" and m.model[i].np == 0 for i in U.SIMAM_LAYERS)
    assert [m.model[i].f for i in U.SIMAM_LAYERS] == list(U.SIMAM_INPUTS.values()) and [m.model[i].e_lambda for i in U.SIMAM_LAYERS] == [1e-4] * 3
    assert [repr(m.model[i]) for i in U.SIMAM_LAYERS] == [str(s) for s in G[f"{U.MODEL}/repr"]]
    # the default graph unchanged through row 25, then the three blocks and Detect on them
    a = yaml.safe_load(open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2-SimAM.yaml")))
    d = yaml.safe_load(open(os.path.join(CFG_DIR, "yolov8-ASF-P2P2.yaml")))
    ra, rd = a["backbone"] + a["head"], d["backbone"] + d["head"]
    assert ra[:26] == rd[:26] and len(ra) == 30 and len(rd) == 27
    assert ra[26:] == [[25, 1, "SimAM", []], [20, 1, "SimAM", ["1e-4"]], [23, 1, "SimAM", []], [[26, 27, 28], 1, "Detect", ["nc"]]]
    m.load_state_dict(U.state(G, U.MODEL), strict=True)


def test_fuse_and_freeze_leave_the_layer_alone():
    from ultralytics.engine.trainer import frozen_parameter_names
    from ultralytics.nn.extra_modules.attention import SimAM
    m = _model().eval()
    keys = list(m.state_dict())
    m.fuse()
    assert not hasattr(m.model[10], "bn") and [type(m.model[i]) for i in U.SIMAM_LAYERS] == [SimAM] * 3
    assert all(not list(m.model[i].parameters()) and m.model[i].e_lambda == 1e-4 for i in U.SIMAM_LAYERS)
    assert not [k for k in keys if "model.26." in k]
    names = [k for k, _ in _model().named_parameters()]
    assert frozen_parameter_names(names, [26]) == frozen_parameter_names(names, None) == [k for k in names if ".dfl" in k]


def test_other_shipped_yamls_hold_no_simam_row():
    files = sorted(glob.glob(os.path.join(CFG_DIR, "*.yaml")))
    assert len(files) > 5
    with_rows = [os.path.basename(f) for f in files
                 if any(row[2] == "SimAM" for row in (lambda d: d["backbone"] + d["head"])(yaml.safe_load(open(f))))]
    assert with_rows == ["yolov8-ASF-P2P2-SimAM.yaml"]


def test_launch_list_tool_lists_the_graph():
    txt = open(os.path.join(ROOT, "tools", "launch_list.py")).read()
    assert '"yolov8n-ASF-P2P2-SimAM"' in txt


# ----------------------------------------------------------------------------- header and binding
def test_header_declares_and_the_library_binds_the_entry_points():
    import ctypes as C
    from ultralytics.hip import SIGNATURES, lib
    txt = open(os.path.join(ROOT, "include", "dealyolo_hip.h")).read()
    for name, nargs, res_t in (("dy_simam_forward", 12, C.c_int), ("dy_simam_backward", 14, C.c_int), ("dy_simam_num_partials", 2, C.c_int)):
        assert f"int {name}(" in txt
        res, args = SIGNATURES[name]
        assert res is res_t and len(args) == nargs
        assert getattr(lib(), name).argtypes == list(args)
    assert "attention.py:53-77" in txt and "tasks.py:969-970" in txt  # the reference lines the entries replace
    assert "dy_simam_forward" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = lib()
    for (N, H, W, C_, _, _) in U.KERNEL_CASES.values():
        assert L.dy_simam_num_partials(H * W, C_) == U.num_partials(H * W, C_)
    assert L.dy_simam_num_partials(160 * 160, 32) == 25 and L.dy_simam_num_partials(0, 8) < 0 and L.dy_simam_num_partials(8, 12) < 0
    # refusals need no device: nothing is launched (host numbers stand in for pointers)
    ARG, ALIGN = -1, -3
    base = dict(x=4096, ldx=16, y=8192, ldy=16, stats=256, ws=512, n=1, H=4, W=4, C=16)

    def fwd(**kw):
        v = dict(base, **kw)
        return L.dy_simam_forward(v["x"], v["ldx"], v["y"], v["ldy"], v["stats"], v["ws"], 1e-4, v["n"], v["H"], v["W"], v["C"], None)

    def bwd(**kw):
        v = dict(base, **kw)  # (y stands for dy; dx is x's own address)
        return L.dy_simam_backward(v["y"], v["ldy"], v["x"], v["ldx"], v["stats"], v["x"], v["ldx"], 0, v["ws"], v["n"], v["H"], v["W"], v["C"], None)

    for f in (fwd, bwd):
        assert f(x=0) == ARG and f(y=0) == ARG and f(stats=0) == ARG and f(ws=0) == ARG and f(n=0) == ARG and f(H=0) == ARG and f(W=0) == ARG
        assert f(C=12) == ARG and f(C=0) == ARG and f(ldx=8) == ARG and f(ldy=8) == ARG
        assert f(ldx=20) == ALIGN and f(ldy=20) == ALIGN and f(x=4104) == ALIGN and f(y=8200) == ALIGN and f(stats=260) == ALIGN and f(ws=516) == ALIGN


# ----------------------------------------------------------------------------- checkpoints
def test_reference_written_checkpoint_rebuilds(golden):
    """tests/golden/ref_ckpt_simam.pt: a whole-module fp16 pickle written by the REFERENCE's classes; its module path
    ultralytics.nn.extra_modules.attention.SimAM resolves to this package's class, and the state_dict keys equal the stored list."""
    from ultralytics.nn.extra_modules.attention import SimAM
    from ultralytics.nn.tasks import DetectionModel, _rebuild, attempt_load_weights, torch_safe_load
    G = golden("simam")
    ckpt, _ = torch_safe_load(U.CKPT)
    obj = ckpt["model"]
    assert [type(obj.model[i]) for i in U.SIMAM_LAYERS] == [SimAM] * 3 and [obj.model[i].e_lambda for i in U.SIMAM_LAYERS] == [1e-4] * 3
    assert sum(1 for row in obj.yaml["backbone"] + obj.yaml["head"] if row[2] == "SimAM") == 3
    m = _rebuild(obj, ckpt)
    assert isinstance(m, DetectionModel) and sum(q.numel() for q in m.parameters()) == int(G["ckpt/n_params"])
    want = U.state(G, "ckpt")
    got = m.state_dict()
    assert list(got) == [str(k) for k in G["ckpt/state_keys"]] == list(want)
    for k, v in want.items():
        assert torch.equal(got[k].float(), (v.half().float() if v.is_floating_point() else v.float())), k
    loaded = attempt_load_weights(U.CKPT)
    assert not loaded.training and [type(loaded.model[i]) for i in U.SIMAM_LAYERS] == [SimAM] * 3


def test_checkpoint_roundtrip_in_the_reference_format(tmp_path):
    from ultralytics.nn.extra_modules.attention import SimAM
    from ultralytics.nn.tasks import attempt_load_weights, save_reference_format, torch_safe_load
    m = _model()
    path = save_reference_format(str(tmp_path / "last.pt"), m, updates=4, epoch=1, train_args={"imgsz": 64})
    obj = torch_safe_load(path)[0]["model"]
    assert next(obj.parameters()).dtype == torch.float16 and all("rt" not in mod.__dict__ for mod in obj.modules())
    assert [type(obj.model[i]) for i in U.SIMAM_LAYERS] == [SimAM] * 3
    back = attempt_load_weights(path)
    for (k, a), (_, b) in zip(m.state_dict().items(), back.state_dict().items()):
        assert torch.equal(a.half().float() if a.is_floating_point() else a, b.float() if a.is_floating_point() else b), k
