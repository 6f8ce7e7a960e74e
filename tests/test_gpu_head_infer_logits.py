"""-m gpu: Detect's fused inference tail that also hands out its logits (csrc/head_infer.hip dy_head_infer_levels_logits).

A validation inside training needs the loss of the same forward; the plain tail keeps the head logits in registers and writes only
y, so the loss had to re-run the two final convs per level (``HeadOut.materialize``).  What is pinned here: the logits the fused
launch writes are the BITS of those eager convs (dy_conv_forward, fp32 out + bias) on the same activations, y is the BITS of the
plain launch, padding channels [nc, ncp) are exact zeros, nothing outside the outputs' rows is written, and shapes the plain entry
refuses are refused with the same code."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD, FILL = 7, 12345.0  # rows of a fill pattern in front of and behind every logits output


def _setup(cin_cls, nc, hw, B=3):
    from ultralytics.hip import DY_EPI_BIAS, DY_EPI_F32OUT
    from ultralytics.hip.engine import ConvSpec, Engine
    eng = Engine("cuda:0")
    gen = torch.Generator().manual_seed(cin_cls * 100 + nc)
    ncp = (nc + 7) // 8 * 8
    xs, specs, box, cls = [], [], [], []
    for h, w in hw:
        xb = (torch.randn(B, h, w, 64 + 16, generator=gen) * 1.5).half().cuda()  # leading dimensions larger than the channel counts
        xc = (torch.randn(B, h, w, cin_cls + 8, generator=gen) * 1.5).half().cuda()
        wb, bb = (torch.randn(64, 64, 1, 1, generator=gen) * 0.2).cuda(), torch.randn(64, generator=gen).cuda()
        wc, bc = (torch.randn(nc, cin_cls, 1, 1, generator=gen) * 0.2).cuda(), torch.randn(nc, generator=gen).cuda()
        sb, sc = ConvSpec("b", wb, bb, None, 1, 1, 0), ConvSpec("c", wc, bc, None, 1, 1, 0)
        for sp in (sb, sc):
            eng.prepare_conv(sp)
            eng.pack(sp, transposed=False)
        ab, ac = eng.wrap_act(xb).sub(8, 64), eng.wrap_act(xc).sub(0, cin_cls)
        fb = torch.empty(B, h, w, 64, dtype=torch.float32, device="cuda")  # what materialize() writes: the eager final convs
        fc = torch.zeros(B, h, w, ncp, dtype=torch.float32, device="cuda")
        eng._conv_raw(sb, ab, fb.data_ptr(), 64, DY_EPI_BIAS | DY_EPI_F32OUT, 0, bb)
        eng._conv_raw(sc, ac, fc.data_ptr(), ncp, DY_EPI_BIAS | DY_EPI_F32OUT, 0, bc)
        xs.append((ab, ac, xb, xc)); specs.append((sb, sc)); box.append(fb); cls.append(fc)
    return eng, xs, specs, box, cls, ncp


def _args(xs, specs, hw, strides, B, cin_cls, nc):
    P, I, F = C.c_void_p, C.c_int, C.c_float
    arr = lambda t, v: (t * len(v))(*v)  # noqa: E731
    return (len(hw), arr(P, [x[0].ptr for x in xs]), arr(I, [x[0].ld for x in xs]), arr(P, [sb.weight.data_ptr() for sb, _ in specs]),
            arr(P, [sb.bias.data_ptr() for sb, _ in specs]), arr(P, [x[1].ptr for x in xs]), arr(I, [x[1].ld for x in xs]),
            arr(P, [sc.weight.data_ptr() for _, sc in specs]), arr(P, [sc.bias.data_ptr() for _, sc in specs]),
            arr(I, [h for h, _ in hw]), arr(I, [w for _, w in hw]), arr(F, strides), B, cin_cls, nc)


@pytest.mark.parametrize("cin_cls,nc", [(32, 6), (48, 20), (64, 80)])
def test_fused_logits_are_the_eager_convs_bit_for_bit(cin_cls, nc):
    """B = 3, levels 12x12 / 6x6 / 3x3 (432, 108, 27 pixels: every level ends inside a wave's 64 pixels, waves straddle images);
    32-channel and 16-channel k-steps, a partly filled 16-row tile, ncp > nc (6 -> 8, 20 -> 24) and ncp == nc (80)."""
    from ultralytics.hip import check, lib
    L = lib()
    B, hw, strides = 3, [(12, 12), (6, 6), (3, 3)], [8.0, 16.0, 32.0]
    assert L.dy_head_infer_supported(64, 64, cin_cls, nc) == 1
    eng, xs, specs, box, cls, ncp = _setup(cin_cls, nc, hw, B)
    A = sum(h * w for h, w in hw)
    s = torch.cuda.current_stream().cuda_stream
    args = _args(xs, specs, hw, strides, B, cin_cls, nc)
    plain = torch.full((B, 4 + nc, A), float("nan"), dtype=torch.float32, device="cuda")
    check(L.dy_head_infer_levels(*args, plain.data_ptr(), s), "dy_head_infer_levels")
    got = torch.full((B, 4 + nc, A), float("nan"), dtype=torch.float32, device="cuda")
    gb = [torch.full((B * h * w + 2 * GUARD, 64), FILL, dtype=torch.float32, device="cuda") for h, w in hw]
    gc = [torch.full((B * h * w + 2 * GUARD, ncp), FILL, dtype=torch.float32, device="cuda") for h, w in hw]
    P = C.c_void_p
    ob = (P * len(hw))(*[t[GUARD:].data_ptr() for t in gb])
    oc = (P * len(hw))(*[t[GUARD:].data_ptr() for t in gc])
    check(L.dy_head_infer_levels_logits(*args, got.data_ptr(), ob, oc, s), "dy_head_infer_levels_logits")
    torch.cuda.synchronize()
    assert torch.isfinite(plain).all() and torch.equal(got, plain), "y of the logits launch differs from the plain launch's"
    for l, (h, w) in enumerate(hw):
        n = B * h * w
        assert torch.equal(gb[l][GUARD:GUARD + n], box[l].view(n, 64)), f"level {l}: box logits differ from the eager conv's"
        assert torch.equal(gc[l][GUARD:GUARD + n], cls[l].view(n, ncp)), f"level {l}: class logits differ from the eager conv's"
        assert bool((gc[l][GUARD:GUARD + n, nc:] == 0).all()), f"level {l}: padding channels [nc, ncp) must be exact zeros"
        for t in (gb[l], gc[l]):
            assert bool((t[:GUARD] == FILL).all()) and bool((t[GUARD + n:] == FILL).all()), f"level {l}: rows outside the output were written"
    # the inputs' padding channels were only read
    for (_, _, xb, xc) in xs:
        assert torch.isfinite(xb).all() and torch.isfinite(xc).all()


def test_unsupported_shapes_get_the_plain_entrys_error_codes():
    from ultralytics.hip import lib
    L = lib()
    B, hw, strides = 1, [(3, 3)], [8.0]
    eng, xs, specs, box, cls, ncp = _setup(32, 6, hw, B)
    s = torch.cuda.current_stream().cuda_stream
    y = torch.zeros((B, 4 + 6, 9), dtype=torch.float32, device="cuda")
    P = C.c_void_p
    ob, oc = (P * 1)(box[0].data_ptr()), (P * 1)(cls[0].data_ptr())
    for cin_cls, nc, nl in ((24, 6, 1), (32, 81, 1), (32, 0, 1), (256, 6, 1), (32, 6, 5), (32, 6, 0)):
        a = list(_args(xs, specs, hw, strides, B, cin_cls, nc))
        a[0] = nl
        want = L.dy_head_infer_levels(*a, y.data_ptr(), s)
        assert want != 0 and L.dy_head_infer_levels_logits(*a, y.data_ptr(), ob, oc, s) == want, (cin_cls, nc, nl)
    # a misaligned activation pointer: the same alignment error
    a = list(_args(xs, specs, hw, strides, B, 32, 6))
    a[1] = (P * 1)(xs[0][0].ptr + 2)
    want = L.dy_head_infer_levels(*a, y.data_ptr(), s)
    assert want != 0 and L.dy_head_infer_levels_logits(*a, y.data_ptr(), ob, oc, s) == want
    # missing / misaligned logits outputs are refused before anything is launched
    a = _args(xs, specs, hw, strides, B, 32, 6)
    assert L.dy_head_infer_levels_logits(*a, y.data_ptr(), None, oc, s) != 0
    assert L.dy_head_infer_levels_logits(*a, y.data_ptr(), (P * 1)(box[0].data_ptr() + 4), oc, s) != 0
    torch.cuda.synchronize()


def test_detect_hands_out_the_logits_it_was_asked_for():
    """Through the eval forward: ``model(x, logits=True)`` leaves box / cls filled (``materialize()`` launches nothing) with the bits
    of ``model(x)`` + ``materialize()``; y is the plain forward's; a later plain forward marks the logits stale again."""
    import os
    from conftest import CFG_DIR
    from oracle import graph as og
    from ultralytics.nn.tasks import DetectionModel
    p = os.path.join(CFG_DIR, "yolov8n-ASF-P2P2.yaml")
    m = DetectionModel(p, ch=3, verbose=False)
    m.load_state_dict(og.fill_state(og.state_layout(og.build_graph(og.load_yaml(p))), 11), strict=True)
    m = m.cuda().eval()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        for rnd in range(3):  # walked, traced, replayed
            y0, f0 = m(x)
            ho = f0._ho
            assert ho.infer is not None and not ho.logits_current
            ho.materialize()
            want = [t.clone() for t in ho.box], [t.clone() for t in ho.cls]
            for t in ho.box + ho.cls:
                t.fill_(FILL)
            y1, f1 = m(x, logits=True)
            ho = f1._ho
            assert ho.logits_current and torch.equal(y1, y0)
            launches = []
            conv_raw, ho_eng = None, m.rt.eng
            conv_raw, ho_eng._conv_raw = ho_eng._conv_raw, lambda *a, **k: launches.append(a)
            try:
                ho.materialize()
            finally:
                ho_eng._conv_raw = conv_raw
            assert not launches, "materialize() launched convs although the forward wrote the logits"
            for l in range(len(ho.box)):
                assert torch.equal(ho.box[l], want[0][l]) and torch.equal(ho.cls[l], want[1][l]), (rnd, l)
    torch.cuda.synchronize()
