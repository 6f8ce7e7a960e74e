"""CPU: models of any class count are built with the reference's parameter names and shapes -- nothing is padded in the state_dict or
in the flat parameter buffer -- and a width that is not a multiple of 8 reaching anything but a Conv / Detect is refused when the
model is built.  Fixture: tests/golden/any_nc_layout.json.gz (tests/golden/make_any_nc_golden.py: the reference's own
DetectionModel(yaml, nc=nc).state_dict() keys and shapes)."""
import gzip
import json
import os
from copy import deepcopy
from types import SimpleNamespace

import pytest
import torch
import yaml

from conftest import CFG_DIR, GOLDEN

MODELS = ["yolov8n-ASF-P2P2", "yolov8n-LD-P2", "yolov8n-p2"]
NCS = [1, 6, 33, 37, 40, 100, 120]


@pytest.fixture(scope="module")
def layouts():
    with gzip.open(os.path.join(GOLDEN, "any_nc_layout.json.gz")) as f:
        return json.loads(f.read().decode())


def _model(name, nc):
    from ultralytics.nn.tasks import DetectionModel
    return DetectionModel(os.path.join(CFG_DIR, name + ".yaml"), ch=3, nc=nc, verbose=False)


@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("name", MODELS)
def test_state_dict_is_the_references(layouts, name, nc):
    m = _model(name, nc)
    det = m.model[-1]
    ch0 = det.cv3[0][0].conv.in_channels
    c3 = max(ch0, min(nc, 100))  # reference nn/modules/head.py:36
    assert ch0 == 32 and (c3 == nc if 33 <= nc <= 100 else c3 == (100 if nc > 100 else 32))
    for seq in det.cv3:
        assert (seq[0].conv.out_channels, seq[1].conv.in_channels, seq[1].conv.out_channels) == (c3, c3, c3)
        assert (seq[2].in_channels, seq[2].out_channels) == (c3, nc)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert got == layouts[f"{name}/{nc}"]
    last = len(m.model) - 1
    assert tuple(m.state_dict()[f"model.{last}.cv3.0.0.conv.weight"].shape) == (c3, 32, 3, 3)


@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("name", MODELS)
def test_flat_layout_holds_the_logical_parameters(name, nc):
    """The six-segment flat buffer (hip/runtime.py: [neck + head | backbone] x [bias | decayed | norm]) places every parameter with its
    own numel, at a multiple of 8 floats: a 37-wide Conv contributes 37 * cin * 9 weights, 37 gammas and 37 betas, nothing more."""
    from ultralytics.hip.runtime import PAD, Runtime
    m = _model(name, nc)
    want = {k: p.numel() for k, p in m.named_parameters()}
    rt = object.__new__(Runtime)
    rt.root, rt.eng = m, SimpleNamespace(device=torch.device("cpu"))
    rt._flatten()
    names, total, _, _ = rt.layout()
    assert sorted(n for n, _ in names) == sorted(want)
    offs = dict(names)
    order = [n for n, _ in names]
    for a, b in zip(order, order[1:] + [None]):
        end = offs[b] if b is not None else total
        assert offs[a] % PAD == 0 and end - offs[a] == (want[a] + PAD - 1) // PAD * PAD, a
    params = dict(m.named_parameters())
    for n in order:
        assert params[n].data.data_ptr() == rt.flat_p[offs[n]:].data_ptr() and params[n].numel() == want[n]
    assert len(rt.seg_bounds) == 5 and rt.bucket_split == rt.seg_bounds[2]
    nb = len(m.yaml["backbone"])
    late = [n for n in order if int(n.split(".")[1]) >= nb]
    assert order[:len(late)] == late, "neck + head parameters come first"


def test_ragged_width_into_a_concat_is_refused_at_build():
    """A ``Conv [nc, ...]`` layer is the one width make_divisible leaves alone.  Routed into a Concat at nc = 37 the model is refused
    when it is built, naming the layer and the width; routed into a Conv or Detect it builds."""
    from ultralytics.nn.tasks import DetectionModel
    base = dict(nc=37, scales=dict(n=[0.33, 0.25, 1024]), scale="n",
                backbone=[[-1, 1, "Conv", [64, 3, 2]], [-1, 1, "Conv", [128, 3, 2]], [-1, 1, "Conv", ["nc", 3, 1]], [1, 1, "Conv", [128, 3, 1]]])
    bad = dict(deepcopy(base), head=[[[2, 3], 1, "Concat", [1]], [-1, 1, "Conv", [64, 1, 1]], [[5], 1, "Detect", ["nc"]]])
    with pytest.raises(NotImplementedError, match=r"layer 4 \(Concat\).*layer 2.*37"):
        DetectionModel(bad, ch=3, verbose=False)
    for mod in ("Add", "nn.Upsample", "SPPF", "C2f"):
        args = {"Add": [], "nn.Upsample": [None, 2, "nearest"], "SPPF": [64, 5], "C2f": [64]}[mod]
        f = [2, 2] if mod == "Add" else 2
        with pytest.raises(NotImplementedError, match=r"layer 4 .*37"):
            DetectionModel(dict(deepcopy(base), head=[[f, 1, mod, args], [[4], 1, "Detect", ["nc"]]]), ch=3, verbose=False)
    # a hidden width that is no multiple of 8 -- C2f's chunk of a 24- or 40-wide output (what make_divisible(.., 8) can produce), SPPF's
    # halved input -- is refused with the layer named, not by an assertion inside the engine at the first forward
    for args, pat in (([96], r"layer 4 \(C2f\).*hidden width of 12"), ([160], r"layer 4 \(C2f\).*hidden width of 20")):
        with pytest.raises(NotImplementedError, match=pat):
            DetectionModel(dict(deepcopy(base), head=[[1, 1, "C2f", args], [[4], 1, "Detect", ["nc"]]]), ch=3, verbose=False)
    with pytest.raises(NotImplementedError, match=r"layer 5 \(SPPF\).*hidden width of 12"):  # behind a 24-wide Conv
        DetectionModel(dict(deepcopy(base), head=[[1, 1, "Conv", [96, 1, 1]], [-1, 1, "SPPF", [64, 5]], [[5], 1, "Detect", ["nc"]]]), ch=3, verbose=False)
    from ultralytics.nn.modules import C2f, SPPF
    for make in (lambda: C2f(32, 24, 1), lambda: C2f(32, 40, 2, True), lambda: SPPF(24, 32)):
        with pytest.raises(NotImplementedError, match="hidden width"):
            make()
    ok = dict(deepcopy(base), head=[[2, 1, "Conv", [64, 3, 1]], [[2, 4], 1, "Detect", ["nc"]]])
    m = DetectionModel(ok, ch=3, verbose=False)
    assert m.model[2].conv.out_channels == 37 and m.model[4].conv.in_channels == 37 and m.model[-1].cv2[0][0].conv.in_channels == 37
    assert yaml.safe_dump(ok)  # (plain data: what a user writes as a model YAML)
