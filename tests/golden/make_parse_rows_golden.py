"""Generate tests/golden/parse_rows.json: what ``DetectionModel`` builds from every model YAML, and what ``parse_model`` refuses.

Recorded at the commit BEFORE the YAML rows moved from ``parse_model``'s class chains to the module classes' row hooks; the file
pins that behaviour and is not regenerated from the code under test (tests/test_host_parse_rows.py compares against it).

    python tests/golden/make_parse_rows_golden.py

``graph``: per YAML under cfg/models what neither the scale nor the class count changes (the generator asserts that): per layer
  ``type``, ``f`` and ``down`` -- ``parse_model``'s own ``down`` list, read from its frame when it returns (it was a local there) --,
  and ``save``, ``stride``.
``build``: one entry per (YAML, scale n | s | m, nc default | 3), key ``<yaml>|<scale>|<nc>``: per layer ``np`` and ``width``
  (``model._cout``); ``state``: the number of ``state_dict`` tensors and a sha256 over their ordered keys and shapes
  (``state_digest``; the lists themselves would make a file of 600 kB).
``refuse``: named YAML dicts that ``DetectionModel`` must refuse, each with the exception type and its full message: one per
  ``raise`` reachable from ``parse_model`` (SITES below; the generator asserts that each produced a row), and rows that break two
  rules at once, to pin which rule wins.
"""
import hashlib
import json
import os
import sys
from copy import deepcopy

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]

from ultralytics.nn import tasks  # noqa: E402

SCALES, NCS = ("n", "s", "m"), (None, 3)


def built(cfg, nc):
    """(model, parse_model's ``chs`` and ``down`` lists as they stood when it returned)."""
    seen = {}

    def prof(frame, event, arg):
        if event == "return" and frame.f_code is tasks.parse_model.__code__:
            seen.update(chs=list(frame.f_locals["chs"]), down=list(frame.f_locals["down"]))
    sys.setprofile(prof)
    try:
        m = tasks.DetectionModel(cfg, nc=nc, verbose=False)
    finally:
        sys.setprofile(None)
    return m, seen["chs"], seen["down"]


def state_digest(sd):
    """[number of tensors, sha256 over one ``key d0,d1,...`` line per tensor, in ``state_dict`` order]."""
    lines = "".join(f"{k} {','.join(map(str, v.shape))}\n" for k, v in sd.items())
    return [len(sd), hashlib.sha256(lines.encode()).hexdigest()]


def build_cases():
    out, graphs = {}, {}
    for y in sorted(os.listdir(tasks.CFG_MODELS)):
        stem = y[:-len(".yaml")]
        for sc in SCALES:
            for nc in NCS:
                name = stem.replace("yolov8", "yolov8" + sc, 1) + ".yaml"
                m, chs, down = built(str(tasks.CFG_MODELS / name), nc)
                assert chs == m._cout, (name, nc)
                assert not any(isinstance(l, tasks.nn.Sequential) for l in m.model), (name, nc)
                graph = dict(type=[l.type for l in m.model], f=[l.f for l in m.model], down=down, save=m.save, stride=m.stride.tolist())
                assert graphs.setdefault(stem, graph) == graph, (name, nc)
                out[f"{stem}|{sc}|{nc}"] = dict(np=[l.np for l in m.model], width=m._cout, state=state_digest(m.state_dict()))
    return out, graphs


def ydict(rows, nc=80, **top):
    """A minimal model YAML dict: width and depth 1, every row in the backbone."""
    return dict(nc=nc, backbone=[list(r) for r in rows], head=[], **top)


C16, C24 = [-1, 1, "Conv", [16, 3, 2]], [-1, 1, "Conv", [24, 3, 2]]
NC3 = [-1, 1, "Conv", ["nc", 1, 1]]  # 3 channels wide under nc=3: the one width that is no multiple of 8
# name -> (site it pins, YAML dict)
REFUSE = {
    "unknown": ("unknown", ydict([[-1, 1, "GhostConv", [64, 3, 2]]])),
    "ragged_read": ("ragged", ydict([C16, NC3, [-1, 1, "nn.Upsample", ["None", 2, "nearest"]]], nc=3)),
    "ragged_read_absolute_from": ("ragged", ydict([C16, NC3, C16, [[2, 1], 1, "Concat", [1]]], nc=3)),
    "nc_wide": ("nc_wide", ydict([C16, [-1, 1, "LDConv", ["nc", 5, 1]]], nc=3)),
    "c2f_hidden": ("c2f_hidden", ydict([C16, [-1, 1, "C2f", [24, True]]])),
    "sppf_hidden": ("sppf_hidden", ydict([C24, [-1, 1, "SPPF", [64, 5]]])),
    "dwconv_check": ("depthwise_dwconv", ydict([C16, [-1, 1, "DWConv", [24, 3, 1]]])),
    "dsconv_check": ("depthwise_dsconv", ydict([[-1, 1, "DSConv", [16]]])),
    "adown_check": ("adown", ydict([C24, [-1, 1, "ADown", [32]]])),
    "gsconv_check": ("gsconv", ydict([C16, [-1, 1, "GSConv", [24, 1, 1]]])),
    "vovgscsp_e": ("vovgscsp_e", ydict([C16, [-1, 1, "VoVGSCSP", [24]]])),
    "vovgscsp_n": ("vovgscsp_n", ydict([C16, [-1, 0, "VoVGSCSP", [32]]])),
    "fusion_key": ("fusion_key", ydict([C16, C16, [[0, 1], 1, "Fusion", ["fusion_mode"]]])),
    "fusion_no_args": ("fusion_key", ydict([C16, C16, [[0, 1], 1, "Fusion", []]], fusion_mode="bifpn")),
    "fusion_sizes": ("fusion_sizes", ydict([C16, C16, [[0, 1], 1, "Fusion", ["fusion_mode"]]], fusion_mode="bifpn")),
    "fusion_check": ("fusion_check", ydict([C16, [-1, 1, "Conv", [24, 3, 1]], [[0, 1], 1, "Fusion", ["fusion_mode"]]], fusion_mode="bifpn")),
    "constructor": ("constructor", ydict([[-1, 1, "Conv", [16, 5, 1]]])),
    # two rules at once
    "unknown_over_ragged": ("precedence", ydict([C16, NC3, [-1, 1, "GhostConv", [64]]], nc=3)),
    "ragged_over_nc_wide": ("precedence", ydict([C16, NC3, [-1, 1, "C2f", ["nc"]]], nc=3)),
    "ragged_over_fusion_key": ("precedence", ydict([C16, NC3, [[0, 1], 1, "Fusion", ["fusion_mode"]]], nc=3)),
    "nc_wide_over_hidden": ("precedence", ydict([C16, [-1, 1, "C2f", ["nc"]]], nc=3)),
    "nc_wide_over_check": ("precedence", ydict([C16, [-1, 1, "ADown", ["nc"]]], nc=3)),
    "hidden_over_constructor": ("precedence", ydict([C24, [-1, 1, "SPPF", [64, 3]]])),
    "check_over_constructor": ("precedence", ydict([C16, [-1, 1, "DWConv", [16, 7, 1]]])),
    "fusion_key_over_check": ("precedence", ydict([C16, [-1, 1, "Conv", [24, 3, 1]], [[0, 1], 1, "Fusion", ["fusion_mode"]]])),
    "fusion_check_over_sizes": ("precedence", ydict([C16, C24, [[0, 1], 1, "Fusion", ["fusion_mode"]]], fusion_mode="bifpn")),
}
SITES = {"unknown": "outside the DEAL-YOLO hot path", "ragged": "can only feed a Conv or Detect", "nc_wide": "only a Conv can produce a width",
         "c2f_hidden": "(C2f) has a hidden width", "sppf_hidden": "(SPPF) has a hidden width", "depthwise_dwconv": "(DWConv)(c1=",
         "depthwise_dsconv": "(DSConv.dwconv)(c1=", "adown": "(ADown)(c1=", "gsconv": "(GSConv)(c1=", "vovgscsp_e": "(VoVGSCSP)(c1=16, c2=24, e=",
         "vovgscsp_n": "VoVGSCSP(c1=16, c2=32, n=0)", "fusion_key": "must name a top-level key", "fusion_sizes": "reads maps of different sizes",
         "fusion_check": "(Fusion)(inc_list=[16, 24], fusion='bifpn') is outside", "constructor": "Conv(k=5, s=1, g=1, d=1) is outside"}


def refusals():
    out, hit = {}, set()
    for name, (site, d) in REFUSE.items():
        try:
            tasks.DetectionModel(deepcopy(d), verbose=False)
        except Exception as e:  # noqa: BLE001  (the type is what is recorded)
            out[name] = dict(yaml=d, type=type(e).__name__, message=str(e))
            if site in SITES:
                assert SITES[site] in str(e), (name, site, str(e))
                hit.add(site)
        else:
            raise AssertionError(f"{name}: the model was built")
    assert hit == set(SITES), sorted(set(SITES) - hit)
    return out


if __name__ == "__main__":
    build, graphs = build_cases()
    doc = dict(graph=graphs, build=build, refuse=refusals())
    path = os.path.join(HERE, "parse_rows.json")
    with open(path, "w") as f:  # one entry per line
        f.write("{\n" + ",\n".join(json.dumps(sec) + ": {\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in body.items()) + "\n}"
                                   for sec, body in doc.items()) + "\n}\n")
    print(f"{path}: {len(build)} builds, {len(doc['refuse'])} refusals, {os.path.getsize(path)} bytes")
