"""CPU: the descriptor table of the grouped SOAP step (ultralytics.hip.soap.SoapTable -> DySoapDesc, csrc/soap.hip): mode geometry,
pools grouped by matrix size, offsets, workgroup columns -- and that the library declares, exports and binds the new entry points."""
import ctypes as C
import os
import re

import pytest

from conftest import CFG_DIR, ROOT

SHAPES = [(16, 8, 3, 3), (16, 3, 3, 3), (8, 16, 1, 1), (24, 6), (8, 8, 1, 1, 1), (16,)]
ENTRIES = ["dy_soap_desc_bytes", "dy_grad_norm", "dy_soap_rotate", "dy_soap_gram", "dy_soap_adam", "dy_soap_apply", "dy_soap_permute_v"]


def _views(shapes, start=24):
    """(name, offset, numel, shape, group) with offsets padded to 8 floats as the runtime pads them (and not starting at 0)."""
    out, off = [], start
    for i, sh in enumerate(shapes):
        k = 1
        for s in sh:
            k *= s
        out.append((f"p{i}", off, k, sh, i % 3))
        off += -(-k // 8) * 8
    return out, off


def test_mode_geometry_per_dimension():
    from ultralytics.hip.soap import SoapTable
    views, _ = _views(SHAPES)
    tb = SoapTable(views)
    want = {(16, 8, 3, 3): [(1, 16, 72), (16, 8, 9), (128, 3, 3), (384, 3, 1)],
            (16, 3, 3, 3): [(1, 16, 27), (16, 3, 9), (48, 3, 3), (144, 3, 1)],
            (8, 16, 1, 1): [(1, 8, 16), (8, 16, 1), (128, 1, 1), (128, 1, 1)],
            (24, 6): [(1, 24, 6), (24, 6, 1)],
            (8, 8, 1, 1, 1): [(1, 8, 8), (8, 8, 1), (64, 1, 1), (64, 1, 1), (64, 1, 1)],
            (16,): [(1, 16, 1)]}
    for e, (name, off, numel, sh, grp) in zip(tb.entries, views):
        assert e["geom"] == want[sh], sh
        assert all(a * n * b == numel for a, n, b in e["geom"])
        assert (e["off"], e["numel"], e["group"], e["ndim"], e["shape"]) == (off, numel, grp, len(sh), sh)  # offsets follow param_off
        assert e["has_q"] == ([0] if len(sh) == 1 else [1] * len(sh))  # 1-D tensors run plain Adam
    assert tb.passes == 5
    with pytest.raises(ValueError, match="dimensions"):
        SoapTable([("w", 0, 64, (2, 2, 2, 2, 2, 2), 1)])
    with pytest.raises(ValueError, match="does not hold"):
        SoapTable([("w", 0, 65, (8, 8), 1)])


@pytest.mark.parametrize("max_dim", [10000, 12])
def test_pools_are_grouped_by_size_without_overlap(max_dim):
    from ultralytics.hip.soap import SoapTable
    views, _ = _views(SHAPES + [(136, 72, 3, 3)])
    tb = SoapTable(views, max_precond_dim=max_dim)
    mats = []  # (n, pool offset, order offset)
    for e in tb.entries:
        for d, n in enumerate(e["shape"]):
            assert e["has_q"][d] == int(e["ndim"] > 1 and n <= max_dim)
            if e["has_q"][d]:
                mats.append((n, e["pool_off"][d], e["ord_off"][d]))
    assert len(mats) == tb.n_gram == sum(c for _, _, c, _ in tb.sizes)
    assert [n for n, *_ in tb.sizes] == sorted({n for n, _, _ in mats})
    # every size is one contiguous (count_n, n, n) block, the blocks tile the pool exactly
    end, oend = 0, 0
    for n, start, count, ostart in tb.sizes:
        assert (start, ostart) == (end, oend)
        assert sorted(p for m, p, _ in mats if m == n) == [start + i * n * n for i in range(count)]
        assert sorted(o for m, _, o in mats if m == n) == [ostart + i * n for i in range(count)]
        end, oend = start + count * n * n, ostart + count * n
    assert (end, oend) == (tb.gram_floats, tb.order_ints)
    if max_dim == 12:
        assert max(n for n, *_ in tb.sizes) == 8 and tb.entries[0]["has_q"] == [0, 1, 1, 1]


def test_workgroup_columns_partition_every_launch():
    """rot_blk / gram_blk / ew_blk are running sums of the tile counts the kernels assume (32 x 32 tiles, 1024-element slices)."""
    from ultralytics.hip.soap import SoapTable
    views, _ = _views(SHAPES + [(136, 72, 3, 3)])
    tb = SoapTable(views, max_precond_dim=100)
    cd = lambda a, b: -(-a // b)  # noqa: E731
    rot, gram, ew = [0] * 5, 0, 0
    for e in tb.entries:
        assert e["rot_blk"] == rot and e["ew_blk"] == ew
        for d in range(5):
            assert e["gram_blk"][d] == gram
            if d < e["ndim"] and e["has_q"][d]:
                n = e["shape"][d]
                rot[d] += cd(n, 32) * cd(e["numel"] // n, 32)
                gram += 1 if n <= 8 else cd(n, 32) ** 2
            else:
                rot[d] += cd(e["numel"], 1024)
        ew += cd(e["numel"], 1024)
    assert (tb.rot_blocks, tb.gram_blocks, tb.ew_blocks) == (rot, gram, ew)
    assert tb.entries[-1]["has_q"] == [0, 1, 1, 1]  # 136 > 100: that dimension passes through


def test_descriptors_match_the_library_layout():
    from ultralytics.hip import DySoapDesc, lib
    from ultralytics.hip.soap import SoapTable
    assert lib().dy_soap_desc_bytes() == C.sizeof(DySoapDesc)
    views, _ = _views(SHAPES)
    tb = SoapTable(views)
    arr = tb.descriptors()
    assert len(arr) == len(SHAPES) and C.sizeof(arr) == len(SHAPES) * C.sizeof(DySoapDesc)
    for t, e in zip(arr, tb.entries):
        nd = e["ndim"]
        assert (t.off, t.numel, t.group, t.ndim, t.ew_blk) == (e["off"], e["numel"], e["group"], nd, e["ew_blk"])
        assert list(t.shape) == list(e["shape"]) + [1] * (5 - nd) and list(t.has_q) == e["has_q"] + [0] * (5 - nd)
        assert list(t.pool_off)[:nd] == e["pool_off"] and list(t.ord_off)[:nd] == e["ord_off"]
        assert list(t.rot_blk) == e["rot_blk"] and list(t.gram_blk) == e["gram_blk"]


def test_flagship_model_table():
    """yolov8n-ASF-P2P2 at nc = 6: 190 trainable tensors (the DFL conv is frozen), 261 Gram matrices in 11 sizes, 688,952 floats."""
    from ultralytics.hip.soap import SoapTable
    from ultralytics.nn.tasks import DetectionModel
    m = DetectionModel(os.path.join(CFG_DIR, "yolov8n-ASF-P2P2.yaml"), nc=6, verbose=False)
    views, off = [], 0
    for n, p in m.named_parameters():
        if p.requires_grad:
            views.append((n, off, p.numel(), tuple(p.shape), 1))
            off += -(-p.numel() // 8) * 8
    tb = SoapTable(views)
    assert len(tb.entries) == 190 and sum(e["ndim"] == 1 for e in tb.entries) == 125
    assert (tb.n_gram, tb.gram_floats) == (261, 688952)
    assert [n for n, *_ in tb.sizes] == [1, 3, 6, 16, 32, 48, 64, 96, 128, 192, 256]
    assert tb.passes == 5 and sum(e["ndim"] == 5 for e in tb.entries) == 1


def test_entry_points_are_declared_exported_and_bound():
    from ultralytics.hip import SIGNATURES, lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dealyolo_hip.h")).read(), flags=re.S)
    L = lib()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", txt), f"{name} is not declared in dealyolo_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in SIGNATURES and getattr(L, name).argtypes == SIGNATURES[name][1]
    assert "DySoapDesc" in txt and "soap.hip" in open(os.path.join(ROOT, "experiment-yolo_amd", "csrc", "Makefile")).read()
    # argument checks run on the host, before anything is launched
    assert L.dy_soap_rotate(None, None, None, 0, 0, None, 0, 0, 0, None, None) == -1
    assert L.dy_grad_norm(None, 0, None, None, None, None) == -1
