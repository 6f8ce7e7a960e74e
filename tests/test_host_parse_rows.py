"""CPU: every model-YAML row means what it meant before the rows moved from ``parse_model``'s class chains to the module classes'
``yaml_row`` hooks.  tests/golden/parse_rows.json was recorded at the commit before the move (tests/golden/make_parse_rows_golden.py):
what every YAML builds at scales n, s and m with the default class count and with 3 classes, and every refusal with its full text."""
import hashlib
import inspect
import json
import os
import re
from copy import deepcopy

import pytest

from conftest import GOLDEN

with open(os.path.join(GOLDEN, "parse_rows.json")) as _f:
    G = json.load(_f)


def _state_digest(sd):  # as tests/golden/make_parse_rows_golden.py::state_digest
    lines = "".join(f"{k} {','.join(map(str, v.shape))}\n" for k, v in sd.items())
    return [len(sd), hashlib.sha256(lines.encode()).hexdigest()]


@pytest.mark.parametrize("case", sorted(G["build"]))
def test_build_is_what_the_class_chains_built(case, monkeypatch):
    from ultralytics.nn import tasks
    stem, sc, nc = case.split("|")
    want, graph = G["build"][case], G["graph"][stem]
    parsed, parse = [], tasks.parse_model  # (the per-layer down-sampling is parse_model's fourth result and is kept nowhere else)
    monkeypatch.setattr(tasks, "parse_model", lambda *a, **k: parsed.append(parse(*a, **k)) or parsed[-1])
    m = tasks.DetectionModel(str(tasks.CFG_MODELS / (stem.replace("yolov8", "yolov8" + sc, 1) + ".yaml")), nc=None if nc == "None" else int(nc),
                             verbose=False)
    (_, _, chs, down), = parsed
    assert chs == m._cout
    assert [l.type for l in m.model] == graph["type"]
    assert [l.f for l in m.model] == graph["f"]
    assert down == graph["down"]
    assert m.save == graph["save"]
    assert m.stride.tolist() == graph["stride"]
    assert [l.np for l in m.model] == want["np"]
    assert m._cout == want["width"]
    assert _state_digest(m.state_dict()) == want["state"]  # the ordered keys and shapes


@pytest.mark.parametrize("name", sorted(G["refuse"]))
def test_refusal_is_the_same_error_with_the_same_text(name):
    from ultralytics.nn.tasks import DetectionModel
    want = G["refuse"][name]
    with pytest.raises(Exception) as e:  # noqa: B017,PT011  (type and text are compared below, verbatim)
        DetectionModel(deepcopy(want["yaml"]), verbose=False)
    assert type(e.value).__name__ == want["type"]
    assert str(e.value) == want["message"]


def test_a_new_module_needs_only_its_modules_entry(monkeypatch):
    """The contract: a class that brings its row hook and ``out_hw`` joins the graph through its ``_MODULES`` entry alone."""
    from ultralytics.hip.runtime import HipModule
    from ultralytics.nn import tasks
    from ultralytics.nn.rows import same_width_row

    class HalfMap(HipModule):
        """A same-width module that halves the map."""
        built = []

        @classmethod
        def yaml_row(cls, row):
            return same_width_row(row, [row.chs[0], *row.args], 0.5)

        def __init__(self, c, tag):
            super().__init__()
            self.built.append((c, tag))

        def out_hw(self, h, w):
            return h // 2, w // 2

    monkeypatch.setitem(tasks._MODULES, "HalfMap", HalfMap)
    d = dict(nc=5, backbone=[[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "HalfMap", ["toy"]]], head=[[[1], 1, "Detect", ["nc"]]])
    m = tasks.DetectionModel(d, verbose=False)
    assert m._cout == [16, 16, 5 + 64]
    assert m.stride.tolist() == [4.0]
    assert HalfMap.built == [(16, "toy")]
    assert isinstance(m.model[1], HalfMap) and m.model[1].type.endswith("HalfMap") and m.model[1].out_hw(8, 6) == (4, 3)


def test_tasks_keeps_no_list_of_module_classes():
    from ultralytics.nn import tasks
    names = {c.__name__ for c in tasks._MODULES.values()}
    for fn in (tasks.parse_model, tasks.BaseModel._concat_plan, tasks.BaseModel.forward_act):
        for inner in re.findall(r"\(([^()]*)\)", inspect.getsource(fn)):
            items = [t.strip() for t in inner.split(",") if t.strip()]
            assert not (len(items) > 1 and all(t in names for t in items)), (fn.__name__, inner)
    assert not hasattr(tasks.DetectionModel, "_layer_channels")
