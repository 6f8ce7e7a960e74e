"""-m gpu: sliced inference -- dy_tile_gather_f32 against the crop kernel whose pixels it converts, dy_tile_merge against its numpy
statement (tests/tiled_util.py) bit for bit, tiled_predict against a per-tile loop with a stand-in detector and with the real model,
and the public interface (YOLO.predict(tile=...))."""
import os

import numpy as np
import pytest
import torch

from tiled_util import merge_reference, planted_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD_SCORE = 0.987654  # the stand-in's detection on a pad canvas: must never reach a result
FLOW_SIZES = [(70, 100), (64, 64), (40, 150)]


def _images(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _convert(u8_nhwc):
    """What the forward has been fed so far: permute + ``.float() / 255`` on the device."""
    return u8_nhwc.permute(0, 3, 1, 2).float() / 255


# ---- 1. gather ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [32, 36, 30])
def test_gather_equals_the_crop_kernel_converted(S):
    from ultralytics.utils.double_inference import crop_letterbox_multi, image_pool
    from ultralytics.utils.tiled import full_pass_record, tile_gather, tile_grid
    sizes = [(37, 53), (64, 64), (90, 41), (20, 24)]  # 37 * 53 * 3 and 64 * 64 * 3 + that: the later images start at odd addresses
    images = _images(sizes, 3)
    pool, off, hw = image_pool(images, torch.device(DEV))
    assert off[1] % 4 and off[2] % 4
    tile_img, rects, geom = [], [], []
    for b in (0, 1, 2):  # native S x S tiles, the shifted-back edge tiles among them
        for x1, y1, x2, y2 in tile_grid(*sizes[b], S, 0.25):
            tile_img.append(b), rects.append((x1, y1, x2, y2)), geom.append((x2 - x1, y2 - y1, 0, 0))
    n_native = len(tile_img)
    # the tile of an image narrower / lower than the canvas: placed top-left, the rest 114
    tile_img.append(3), rects.append((0, 0, 24, 20)), geom.append((24, 20, 0, 0))
    tile_img.append(0), rects.append((30, 20, 53, 37)), geom.append((23, 17, 0, 0))  # a padded corner piece of the 37 x 53 image
    for b in (2, 3):  # whole-image passes: 90 x 41 scales down, 20 x 24 scales up
        rc, g, _ = full_pass_record(*sizes[b], S)
        tile_img.append(b), rects.append(rc), geom.append(g)
        assert (g[0] < sizes[b][1]) == (b == 2)
    K = len(tile_img)
    order = [K, *range(n_native), K + 1, *range(n_native, K)]  # two pad canvases: the first record and one in the middle
    t_img = np.array([-1 if k >= K else tile_img[k] for k in order], np.int32)
    t_rc = np.array([(7, 7, 7, 7) if k >= K else rects[k] for k in order], np.int32)  # a pad canvas's tables are not read
    t_g = np.array([(-5, 0, 99, 99) if k >= K else geom[k] for k in order], np.int32)
    out = torch.full((K + 3, 3, S, S), -1.0, device=DEV)
    tile_gather(pool, off, hw, t_img, t_rc, t_g, out, S)
    assert (out[K + 2] == -1).all(), "wrote past the last record"
    real = [j for j, k in enumerate(order) if k < K]
    crops = torch.zeros((K, S, S, 3), dtype=torch.uint8, device=DEV)
    crop_letterbox_multi(pool, off, hw, t_img[real], t_rc[real], t_g[real], crops, size=S)
    assert torch.equal(out[real], _convert(crops))
    pad = (torch.full((1,), 114, dtype=torch.uint8, device=DEV).float() / 255).item()
    for j, k in enumerate(order):
        if k >= K:
            assert (out[j] == pad).all()
    # native interior tiles against the image itself -- not through the crop kernel
    checked = 0
    for j, k in enumerate(order):
        if k < n_native and geom[k][:2] == (S, S):
            x1, y1, x2, y2 = rects[k]
            want = _convert(torch.from_numpy(images[tile_img[k]][y1:y2, x1:x2].copy()).to(DEV)[None])[0]
            assert torch.equal(out[j], want), (S, k)
            checked += 1
    assert checked >= 6
    with pytest.raises(ValueError):  # the wrapper refuses a rectangle that leaves its image: the kernel never sees it
        tile_gather(pool, off, hw, [0], [(30, 20, 54, 37)], [(24, 17, 0, 0)], out, S)


# ---- 2. merge ----------------------------------------------------------------------------------------------------------------------
def _run_merge(cases, thr, ios, agnostic):
    """cases: [(rows, row_tile, maps, (H, W))] -> per image (mapped rows, kept indices relative to the image) from ONE call."""
    from ultralytics.utils.tiled import tile_merge
    row_off = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).astype(np.int32)
    map_off = np.concatenate([[0], np.cumsum([len(c[2]) for c in cases])])
    rows = np.concatenate([c[0].reshape(-1, 6) for c in cases], 0).astype(np.float32)
    row_tile = np.concatenate([np.asarray(c[1], np.int32).reshape(-1) + map_off[i] for i, c in enumerate(cases)]).astype(np.int32)
    maps = np.concatenate([np.asarray(c[2], np.float32).reshape(-1, 6) for c in cases], 0)
    mapped, order, nkeep = tile_merge(torch.from_numpy(rows).to(DEV), row_off, row_tile, maps, [c[3] for c in cases], thr,
                                      "ios" if ios else "iou", agnostic)
    mapped, order = mapped.cpu().numpy(), order.cpu().numpy()
    return [(mapped[row_off[i]:row_off[i + 1]], (order[row_off[i]:row_off[i] + nkeep[i]] - row_off[i]).tolist()) for i in range(len(cases))]


def _assert_equal(got, case, thr, ios, agnostic, tag):
    rows, row_tile, maps, (H, W) = case
    want_rows, want_keep, _ = merge_reference(rows, row_tile, maps, H, W, thr, ios=ios, agnostic=agnostic)
    assert got[0].shape == want_rows.shape and np.array_equal(got[0].view(np.int32), want_rows.view(np.int32)), tag
    assert got[1] == want_keep, tag


@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("ios", [False, True])
def test_merge_equals_the_numpy_reference(ios, agnostic):
    cases = [planted_case(seed) for seed in range(6)]
    for seed, (rows, row_tile, maps, (H, W)) in enumerate(cases):  # the inputs do what they are for
        _, keep, n = merge_reference(rows, row_tile, maps, H, W, 0.5, ios=ios, agnostic=agnostic)
        tied = sum((rows[:, 4] == s).sum() > 1 for s in rows[:, 4])
        print(f"seed {seed}: {len(rows)} rows, {n - len(keep)} suppressed, {tied} tied")
        assert n - len(keep) >= 0.25 * len(rows) and tied >= 5, seed
    for seed, case in enumerate(cases):  # six one-image calls
        _assert_equal(_run_merge([case], 0.5, ios, agnostic)[0], case, 0.5, ios, agnostic, ("alone", seed))
    empty = (np.zeros((0, 6), np.float32), np.zeros(0, np.int32), cases[0][2], (100, 150))
    packed = cases[:3] + [empty] + cases[3:]  # ONE call of 7 images, one of them without rows
    got = _run_merge(packed, 0.5, ios, agnostic)
    assert len(got) == 7 and got[3][1] == [] and got[3][0].shape == (0, 6)
    for i, case in enumerate(packed):
        _assert_equal(got[i], case, 0.5, ios, agnostic, ("packed", i))


def test_merge_drops_rows_that_clip_to_nothing():
    rows, row_tile, maps, (H, W) = planted_case(1)
    full = len(maps) - 1
    extra = np.array([[-9, 5, -2, 20, 1.0, 0],      # left of tile 0: clips to x 0..0
                      [10, 2, 40, 8, 1.0, 1],       # inside the whole-image pass's upper pad band (pad_y = 10): clips to y 0..0
                      [70, 10, 80, 30, 1.0, 2],     # right of the frame from the shifted-back tile: clips to x 150..150
                      [5, 60, 30, 64, 1.0, 0]],     # the lower pad band of the whole-image pass: clips to y 100..100
                     np.float32)
    etile = np.array([0, full, 2, full], np.int32)
    case = (np.concatenate([extra[:2], rows, extra[2:]], 0), np.concatenate([etile[:2], row_tile, etile[2:]]), maps, (H, W))
    want_rows, want_keep, n = merge_reference(*case[:3], H, W, 0.5)
    assert n == merge_reference(rows, row_tile, maps, H, W, 0.5)[2] and not set(want_keep) & {0, 1, len(rows) + 2, len(rows) + 3}  # all four dropped although they lead the scores
    for ios in (False, True):
        _assert_equal(_run_merge([case], 0.5, ios, False)[0], case, 0.5, ios, False, ios)


def test_merge_capacity():
    from ultralytics.utils.tiled import MERGE_MAX_ROWS, tile_merge
    assert MERGE_MAX_ROWS == 8192
    rng = np.random.default_rng(0)
    n = MERGE_MAX_ROWS + 1
    cell = np.arange(n)
    xy = np.stack([(cell % 128) * 4, (cell // 128) * 4], 1).astype(np.float32)  # disjoint 3 x 3 boxes on a 4 px lattice
    rows = np.concatenate([xy, xy + 3, rng.integers(1, 4097, (n, 1)) / 4096, rng.integers(0, 3, (n, 1))], 1).astype(np.float32)
    maps, size = np.array([[0, 0, 0, 0, 1, 1]], np.float32), [(300, 512)]
    with pytest.raises(RuntimeError, match="dy_tile_merge capacity"):
        tile_merge(torch.from_numpy(rows).to(DEV), [0, n], np.zeros(n, np.int32), maps, size, 0.5)
    n = MERGE_MAX_ROWS
    mapped, order, nkeep = tile_merge(torch.from_numpy(rows[:n]).to(DEV), [0, n], np.zeros(n, np.int32), maps, size, 0.5, "ios", True)
    assert nkeep.tolist() == [n] and np.array_equal(mapped.cpu().numpy(), rows[:n])
    want = sorted(range(n), key=lambda i: (-rows[i, 4], i))
    assert len(set(rows[:n, 4].tolist())) < n, "no tied scores"
    assert order.cpu().numpy().tolist() == want


# ---- 4. flow against a per-tile loop ---------------------------------------------------------------------------------------------------
def _stand_in_rows(byte_sum, S):
    """Detections that depend on a canvas's pixels alone."""
    if byte_sum == 114 * S * S * 3:
        return np.array([[10.0, 10.0, 50.0, 50.0, PAD_SCORE, 0.0]], np.float32)
    g = np.random.default_rng(byte_sum)
    m = int(g.integers(0, 9))
    cxy, half = g.uniform(0.2 * S, 0.8 * S, (m, 2)), g.uniform(0.08 * S, 0.4 * S, (m, 2))
    b = np.concatenate([cxy - half, cxy + half], 1).clip(0, S)
    return np.concatenate([b, g.integers(4, 17, (m, 1)) / 16, g.integers(0, 3, (m, 1))], 1).astype(np.float32).reshape(-1, 6)


def _stand_in(seen):
    def fake(model_, x, conf, iou, classes=None, agnostic=False, max_det=300, augment=False):
        seen.append(tuple(x.shape))
        sums = (x * 255).round().to(torch.int64).reshape(x.shape[0], -1).sum(1).tolist()
        return [torch.from_numpy(_stand_in_rows(s, x.shape[-1])).to(x.device) for s in sums]
    return fake


def _own_canvases(images, S, overlap):
    """Every record of every image cut by the test: native tiles are numpy slices padded with 114, the whole-image pass comes through
    crop_letterbox_multi.  -> per image [(S, S, 3) uint8], and the plan."""
    from ultralytics.utils.double_inference import crop_letterbox_multi, image_pool
    from ultralytics.utils.tiled import plan_tiles
    plan = plan_tiles([im.shape[:2] for im in images], S, overlap)
    pool, off, hw = image_pool(images, torch.device(DEV))
    per_image = []
    for i, im in enumerate(images):
        canv = []
        for k in range(plan["rec_off"][i], plan["rec_off"][i + 1]):
            x1, y1, x2, y2 = plan["rects"][k].tolist()
            if plan["maps"][k, 4] == 1:
                c = np.full((S, S, 3), 114, np.uint8)
                c[:y2 - y1, :x2 - x1] = im[y1:y2, x1:x2]
            else:
                out = torch.zeros((1, S, S, 3), dtype=torch.uint8, device=DEV)
                crop_letterbox_multi(pool, off, hw, [i], [plan["rects"][k]], [plan["geom"][k]], out, size=S)
                c = out[0].cpu().numpy()
            canv.append(c)
        per_image.append(canv)
    return per_image, plan


def test_flow_equals_a_per_tile_loop(monkeypatch):
    from ultralytics.utils import tiled
    images = _images(FLOW_SIZES, 11)
    seen = []
    monkeypatch.setattr(tiled, "_detect_tiles", _stand_in(seen))
    net = torch.nn.Linear(1, 1).to(DEV)  # the stand-in never calls it
    got = tiled.tiled_predict(images, net, tile=64, overlap=0.25, batch=8, merge_iou=0.5, metric="ios")
    assert seen == [(8, 3, 64, 64)] * 2  # 5 + 1 + 4 records: two forwards, six pad canvases
    canvases, plan = _own_canvases(images, 64, 0.25)
    assert [len(c) for c in canvases] == [5, 1, 4]
    suppressed = 0
    for i, (H, W) in enumerate(FLOW_SIZES):
        rows = [_stand_in_rows(int(c.astype(np.int64).sum()), 64) for c in canvases[i]]
        row_tile = np.repeat(np.arange(len(rows)), [len(r) for r in rows]) + plan["rec_off"][i]
        want_rows, keep, n = merge_reference(np.concatenate(rows, 0), row_tile, plan["maps"], H, W, 0.5, ios=True)
        suppressed += n - len(keep)
        g = got[i].cpu().numpy()
        assert g.shape == (len(keep), 6) and np.array_equal(g.view(np.int32), want_rows[keep].view(np.int32)), i
        assert not np.isclose(g[:, 4], PAD_SCORE).any()
        assert (np.diff(g[:, 4]) <= 0).all()
    assert suppressed > 0 and sum(len(g) for g in got) > 10


# ---- 5. real model, same chunking --------------------------------------------------------------------------------------------------------
def _model():
    from ultralytics.nn.tasks import DetectionModel
    torch.manual_seed(0)
    m = DetectionModel("yolov8n-ASF-P2P2.yaml", verbose=False)
    for seq in m.model[-1].cv3:  # class scores near 0.5: candidates exist at conf 0.25
        torch.nn.init.zeros_(seq[-1].bias)
    return m.to(DEV).eval()


def test_real_model_same_chunking():
    from ultralytics.utils import ops, tiled
    from ultralytics.utils.double_inference import image_pool
    model = _model()
    images = _images(FLOW_SIZES, 12)
    shapes = []
    hook = model.register_forward_pre_hook(lambda m, args: shapes.append(tuple(args[0].shape)))
    got = tiled.tiled_predict(images, model, tile=64, overlap=0.25, batch=8, conf=0.25)
    hook.remove()
    assert shapes == [(8, 3, 64, 64)] * 2
    # expected: the same records in the same chunks, the pad canvases in the same slots
    plan = tiled.plan_tiles(FLOW_SIZES, 64, 0.25)
    K = len(plan["tile_img"])
    assert K == 10
    pool, off, hw = image_pool(images, torch.device(DEV))
    x = torch.empty((16, 3, 64, 64), device=DEV)
    pad = lambda a, v: np.concatenate([a, np.full((16 - K,) + a.shape[1:], v, a.dtype)])  # noqa: E731
    tiled.tile_gather(pool, off, hw, pad(plan["tile_img"], -1), pad(plan["rects"], 0), pad(plan["geom"], 0), x, 64)
    dets = []
    with torch.no_grad():
        for f in range(2):
            dets += ops.non_max_suppression(model(x[f * 8:(f + 1) * 8]), 0.25, 0.7, max_det=300)
    dets = [d.cpu().numpy() for d in dets[:K]]
    suppressed = 0
    for i, (H, W) in enumerate(FLOW_SIZES):
        lo, hi = plan["rec_off"][i], plan["rec_off"][i + 1]
        rows = np.concatenate(dets[lo:hi], 0)
        row_tile = np.repeat(np.arange(lo, hi), [len(d) for d in dets[lo:hi]])
        want_rows, keep, n = merge_reference(rows, row_tile, plan["maps"], H, W, 0.5, ios=True)
        suppressed += n - len(keep)
        g = got[i].cpu().numpy()
        print(f"image {i}: {len(rows)} rows, {n} swept, {len(keep)} kept")
        assert g.shape == (len(keep), 6) and np.array_equal(g.view(np.int32), want_rows[keep].view(np.int32)), i
    assert suppressed > 0, "the merge suppressed nothing: no image ends with a box whose duplicate another tile reported"


# ---- 6. public interface -----------------------------------------------------------------------------------------------------------------
def test_public_interface():
    from ultralytics import YOLO
    from ultralytics.utils.tiled import tiled_predict
    torch.manual_seed(0)
    yolo = YOLO("yolov8n-ASF-P2P2.yaml")
    for seq in yolo.model.model[-1].cv3:
        torch.nn.init.zeros_(seq[-1].bias)
    bgr = _images([(70, 100), (40, 150)], 13)
    plain = yolo.predict(bgr, batch=8)
    res = yolo.predict(bgr, tile=64, tile_overlap=0.25, batch=8)
    assert len(res) == 2
    want = tiled_predict([np.ascontiguousarray(im[..., ::-1]) for im in bgr], yolo.model, tile=64, overlap=0.25, batch=8)
    for r, w, (H, W) in zip(res, want, [(70, 100), (40, 150)]):
        assert r.orig_shape == (H, W)
        xyxy = r.boxes.xyxy
        assert len(xyxy) and (xyxy >= 0).all() and (xyxy[:, [0, 2]] <= W).all() and (xyxy[:, [1, 3]] <= H).all()
        assert torch.equal(r.boxes.data, w)
    again = yolo.predict(bgr, batch=8)  # without tile: the letterboxed single pass, as before
    assert len(again) == len(plain) == 2
    for a, b in zip(again, plain):
        assert torch.equal(a.boxes.data, b.boxes.data)
    assert not all(torch.equal(a.boxes.data, r.boxes.data) for a, r in zip(again, res))
    with pytest.raises(ValueError, match="tile"):
        yolo.predict(torch.rand(1, 3, 64, 64), tile=64)
    with pytest.raises(ValueError, match="multiple of the stride"):
        yolo.predict(bgr, tile=48)


def test_sliced_inference_script(tmp_path):
    """sliced_inference.py over a directory of three small frames with labels: both passes counted and scored, the JSON written."""
    import json
    from PIL import Image
    import sliced_inference
    from ultralytics import YOLO
    img_dir, lab_dir = tmp_path / "images", tmp_path / "labels"
    img_dir.mkdir(), lab_dir.mkdir()
    for i, im in enumerate(_images([(70, 100), (70, 100), (40, 150)], 14)):
        Image.fromarray(im).save(img_dir / f"f{i}.png")
        (lab_dir / f"f{i}.txt").write_text("0 0.5 0.5 0.2 0.3\n1 0.2 0.25 0.1 0.2\n" if i else "")
    torch.manual_seed(0)
    yolo = YOLO("yolov8n-ASF-P2P2.yaml")
    for seq in yolo.model.model[-1].cv3:
        torch.nn.init.zeros_(seq[-1].bias)
    lines = []
    out = sliced_inference.run(yolo, str(img_dir), str(lab_dir), tile=64, overlap=0.25, batch=8, json_path=str(tmp_path / "p.json"), log=lines.append)
    assert out["images"] == 3 and len(lines) == 5 and lines[0].startswith("f0.png: single ") and lines[4].startswith("[sliced] detections: ")
    for s in ("single", "sliced"):
        m = out[s]
        assert m["detections"] > 0 and m["tp"] + m["fn"] == 4 and m["tp"] + m["fp"] == m["detections"] and 0 <= m["map_50"] <= 1
    recs = json.load(open(tmp_path / "p.json"))
    assert len(recs) == out["sliced"]["detections"] and {r["image_id"] for r in recs} <= {"f0", "f1", "f2"}
    bare = sliced_inference.run(yolo, str(img_dir), tile=64, overlap=0.25, batch=8, log=lines.append)
    assert bare["sliced"] == {"detections": out["sliced"]["detections"]}
