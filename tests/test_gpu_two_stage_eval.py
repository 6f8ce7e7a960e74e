"""-m gpu: the batched, dataset-level two-stage path -- dy_crop_letterbox_u8_multi / dy_refine_select_multi against the one-image
kernels they must reproduce bit for bit, dy_two_stage_merge against the restatement pinned by tests/test_host_two_stage_eval.py and the
reference-generated counts of tests/golden/two_stage_eval.npz, double_inference_batch against double_inference per image, and
evaluate_two_stage end to end."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_host_two_stage_eval import G as GE, greedy_case, merge_reference

pytestmark = pytest.mark.gpu
G2 = np.load(os.path.join(os.path.dirname(__file__), "golden", "two_stage.npz"))
PAD_CANVAS_SUM = 114 * 640 * 640 * 3
PAD_SCORE = 0.987654  # the stand-in's detection on a pad canvas: must never reach a result


def test_multi_image_crops_equal_the_one_image_kernel_bit_for_bit():
    from ultralytics.utils.double_inference import crop_geometry, crop_letterbox_multi, image_pool, prepare_cropped_images
    rng = np.random.default_rng(1)
    hw = [(37, 53), (64, 48), (120, 90)]  # 37 * 53 * 3 = 5,883 bytes: the second image starts at an odd address
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in hw]
    pool, off, sizes = image_pool(images, torch.device("cuda:0"))
    assert off.tolist() == [0, 5883, 5883 + 64 * 48 * 3] and sizes == hw and pool.numel() == sum(h * w * 3 for h, w in hw)
    crops = [(0, [43, 29, 53, 37]),   # the last row and column of every image: out of bounds if an offset or stride is wrong
             (1, [38, 56, 48, 64]),
             (2, [80, 112, 90, 120]),
             (1, [5, 3, 6, 40]),      # one pixel wide
             (0, [0, 0, 53, 37]),     # a whole image
             (2, [10, 20, 70, 100]),
             (0, [1, 1, 9, 36]),      # the same image again, not adjacent in crop order
             (1, [20, 5, 48, 60]),
             (2, [0, 0, 90, 120])]
    for S, sel in ((64, range(9)), (30, (1, 4))):  # 30: not a multiple of 4, the one-pixel-per-thread kernel
        cimg = [crops[k][0] for k in sel]
        rects = [crops[k][1] for k in sel]
        infos = [dict(x1=r[0], y1=r[1], x2=r[2], y2=r[3]) for r in rects]
        geom = [[*g["new_size"], g["pad_x"], g["pad_y"]] for g in (crop_geometry(c, S) for c in infos)]
        out = torch.zeros((len(rects), S, S, 3), dtype=torch.uint8, device="cuda")
        crop_letterbox_multi(pool, off, sizes, cimg, rects, geom, out, size=S)
        got = out.cpu().numpy()
        for b in range(3):
            mine = [j for j, c in enumerate(cimg) if c == b]
            if mine:
                ref, _ = prepare_cropped_images(torch.from_numpy(images[b]).cuda(), [infos[j] for j in mine], size=S)
                assert np.array_equal(got[mine], ref.cpu().numpy()), (S, b)
        assert (got != 114).any(axis=(1, 2, 3)).all()
    with pytest.raises(ValueError):  # the launcher refuses a rectangle that leaves its image: the kernel never sees it
        crop_letterbox_multi(pool, off, sizes, [0], [[0, 0, 54, 37]], [[64, 44, 0, 10]], torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device="cuda"), size=64)


def test_refine_select_multi_takes_each_crops_own_image_bounds():
    from ultralytics.hip import check, lib
    K = int(G2["ref/n"])
    hw = np.array([[600, 900], [300, 450]], np.int32)  # even cases keep the fixture's 900x600 image, odd ones get 450x300
    per = [np.concatenate([G2[f"ref/{k}/cand"].reshape(-1, 4), G2[f"ref/{k}/confs"].reshape(-1, 1),
                           G2[f"ref/{k}/labels"].reshape(-1, 1).astype(np.float32)], 1).astype(np.float32) for k in range(K)]
    orig = np.stack([G2[f"ref/{k}/orig"] for k in range(K)]).astype(np.float32)
    rects = np.stack([G2[f"ref/{k}/rect"] for k in range(K)]).astype(np.int32)
    scale = np.stack([G2[f"ref/{k}/geom"] for k in range(K)]).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    def run(ks, fn, tail):
        off = np.concatenate([[0], np.cumsum([len(per[k]) for k in ks])]).astype(np.int32)
        dets = np.concatenate([per[k] for k in ks], 0) if off[-1] else np.zeros((0, 6), np.float32)
        d = [t(dets), t(off), t(orig[ks]), t(rects[ks]), t(scale[ks])]
        out = torch.zeros((len(ks), 6), device="cuda")
        found = torch.zeros(len(ks), dtype=torch.int32, device="cuda")
        check(fn(*[x.data_ptr() for x in d], *tail(ks), out.data_ptr(), found.data_ptr(), None), "refine")
        torch.cuda.synchronize()
        return out.cpu().numpy(), found.cpu().numpy()

    ks = list(range(K))
    cimg, hwd = t((np.arange(K) % 2).astype(np.int32)), t(hw)
    out, found = run(ks, lib().dy_refine_select_multi, lambda ks: (cimg.data_ptr(), hwd.data_ptr(), len(ks)))
    single = {}
    for b in (0, 1):
        single[b] = run(ks, lib().dy_refine_select, lambda ks, b=b: (len(ks), float(hw[b, 1]), float(hw[b, 0])))
        grp = ks[b::2]
        ref_out, ref_found = run(grp, lib().dy_refine_select, lambda ks, b=b: (len(ks), float(hw[b, 1]), float(hw[b, 0])))
        assert np.array_equal(found[grp], ref_found)
        assert np.array_equal(out[grp][ref_found == 1], ref_out[ref_found == 1])
    assert found[0::2].sum() >= 3
    assert (single[0][1] != single[1][1]).any(), "no case depends on the image size: the per-image bounds are not exercised"
    assert (found[1::2] != single[0][1][1::2]).any(), "no odd case changed outcome with its own, smaller image"


def _merge_inputs(seed):
    """The six fixture cases as six images of one chunk, with crops for two rows in three and seeded refinements: a jittered label box
    (or the row's own box) at a higher score, found for about 60 % of them."""
    rng = np.random.default_rng(seed)
    rows, labels, slots, refined, found = [], [], [], [], []
    for k in range(int(GE["greedy/n"])):
        r, lab = greedy_case(k)
        s = [i for i in range(len(r)) if i % 3 != 1]
        ref = np.zeros((len(s), 6), np.float32)
        for j, i in enumerate(s):
            box = lab[rng.integers(len(lab)), 1:] if len(lab) and rng.random() < 0.7 else r[i, :4]
            ref[j] = [*(box + rng.normal(0, 3, 4)), min(1.0, r[i, 4] + rng.uniform(0.01, 0.3)), r[i, 5] if rng.random() < 0.8 else (r[i, 5] + 1) % 3]
        rows.append(r), labels.append(lab), slots.append(s), refined.append(ref), found.append((rng.random(len(s)) < 0.6).astype(np.int32))
    return rows, labels, slots, refined, found


def _run_merge(rows, labels, slots, refined, found, aligned, nms_iou):
    from ultralytics.utils.double_inference import two_stage_merge
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)  # noqa: E731
    row_off = off(rows)
    crop_row = np.concatenate([np.asarray(s, np.int32) + row_off[b] for b, s in enumerate(slots)]).astype(np.int32)
    K = len(crop_row)
    ref_d = torch.from_numpy(np.concatenate(refined, 0)).cuda() if K else None
    found_d = torch.from_numpy(np.concatenate(found)).cuda() if K else None
    out = two_stage_merge(np.concatenate(rows, 0), row_off, ref_d, found_d, crop_row, off(slots), np.concatenate(labels, 0), off(labels), aligned,
                          nms_iou, 0.5, torch.device("cuda:0"))
    return out, row_off


def test_merge_kernel_applies_suppresses_and_counts_exactly():
    rows, labels, slots, refined, found = _merge_inputs(4)
    assert [len(r) for r in rows] == [0, 4, 1, 7, 40, 300] and len(labels[1]) == 0  # 300 rows > 256 threads; an image without labels
    n_img = len(rows)
    # nothing found: the fixture's own numbers -- reference counts on all rows (no NMS) and on the rows the 0.45 NMS keeps
    nothing = [np.zeros_like(f) for f in found]
    (r_out, keep, cnt), row_off = _run_merge(rows, labels, slots, refined, nothing, True, -1.0)
    assert np.array_equal(r_out, np.concatenate(rows, 0)) and keep.all()
    assert cnt.tolist() == [GE[f"greedy/{k}/counts"].tolist() for k in range(n_img)]
    (r_out, keep, cnt), _ = _run_merge(rows, labels, slots, refined, nothing, True, 0.45)
    for k in range(n_img):
        assert np.array_equal(np.where(keep[row_off[k]:row_off[k + 1]])[0], GE[f"greedy/{k}/keep"]), k
    assert cnt.tolist() == [GE[f"greedy/{k}/counts_kept"].tolist() for k in range(n_img)]
    # with refinements, both ways of applying them: the rows bit for bit, the mask and the counts against the restatement
    differs = 0
    for aligned in (1, 0):
        (r_out, keep, cnt), _ = _run_merge(rows, labels, slots, refined, found, aligned, 0.45)
        for k in range(n_img):
            want_rows, want_keep, want_cnt = merge_reference(rows[k], refined[k], found[k], slots[k], aligned, 0.45, labels[k], 0.5)
            lo, hi = row_off[k], row_off[k + 1]
            assert np.array_equal(r_out[lo:hi], want_rows), (aligned, k)
            assert np.array_equal(keep[lo:hi], want_keep), (aligned, k)
            assert tuple(cnt[k]) == want_cnt, (aligned, k, cnt[k], want_cnt)
            differs += not np.array_equal(want_rows, rows[k])
        if aligned:
            rows_aligned = r_out
    assert differs >= 6 and not np.array_equal(rows_aligned, r_out), "the refinements (or the zip quirk) changed nothing"


def test_merge_capacity_raises():
    from ultralytics.utils.double_inference import two_stage_merge
    rng = np.random.default_rng(0)
    n = 2049
    xy = rng.uniform(0, 500, (n, 2))
    rows = np.concatenate([xy, xy + 20, rng.uniform(0.3, 1, (n, 1)), np.zeros((n, 1))], 1).astype(np.float32)
    none, z2 = np.zeros(0, np.int32), np.zeros(2, np.int32)
    with pytest.raises(RuntimeError, match="dy_two_stage_merge capacity"):
        two_stage_merge(rows, [0, n], None, None, none, z2, np.zeros((0, 5), np.float32), z2, True, 0.45, 0.5, torch.device("cuda:0"))
    out = two_stage_merge(rows[:2048], [0, 2048], None, None, none, z2, np.zeros((0, 5), np.float32), z2, True, -1.0, 0.5, torch.device("cuda:0"))
    assert out[1].all() and out[2].tolist() == [[0, 2048, 0]]


def _content_stand_in(seen):
    """A second stage that depends on the crop's pixels alone, so that a crop gets the same rows whether it arrives with its own image's
    crops (double_inference) or with a whole chunk's (double_inference_batch); a pad canvas gets a detection of its own."""
    def fake(model_, crops, conf, iou, bs, augment=False):
        seen.setdefault("shapes", []).append(tuple(crops.shape))
        out = []
        for s in crops.reshape(crops.shape[0], -1).sum(1, dtype=torch.int64).tolist():
            if s == PAD_CANVAS_SUM:
                out.append(torch.tensor([[100.0, 100.0, 500.0, 500.0, PAD_SCORE, 0.0]], device=crops.device))
                continue
            g = np.random.default_rng(s)
            m = int(g.integers(0, 9))
            cxy, half = g.uniform(280, 360, (m, 2)), g.uniform(150, 260, (m, 2))
            b = np.concatenate([cxy - half, cxy + half], 1).clip(0, 640)
            out.append(torch.tensor(np.concatenate([b, g.uniform(0.25, 1, (m, 1)), g.integers(0, 3, (m, 1))], 1), dtype=torch.float32).reshape(-1, 6).to(crops.device))
        return out
    return fake


def test_batched_flow_equals_the_one_image_flow(monkeypatch):
    from ultralytics.nn.tasks import DetectionModel
    from ultralytics.utils import double_inference as di
    torch.manual_seed(0)
    model = DetectionModel("yolov8n-ASF-P2P2.yaml", verbose=False).cuda().eval()
    rng = np.random.default_rng(7)
    images, preds, labels = [], [], []
    for (H, W), n in (((200, 320), 0), ((300, 260), 5), ((480, 640), 16)):
        images.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        c = np.stack([rng.uniform(30, W - 30, n), rng.uniform(30, H - 30, n)], 1)
        wh = rng.uniform(8, 100, (n, 2))
        boxes = np.concatenate([c - wh / 2, c + wh / 2], 1)
        preds.append({"boxes": boxes.tolist(), "scores": rng.uniform(0.1, 0.6, n).tolist(), "labels": rng.integers(0, 3, n).tolist()})
        lab = np.concatenate([np.asarray(preds[-1]["labels"], np.float32).reshape(-1, 1), boxes + rng.normal(0, 2, boxes.shape)], 1).astype(np.float32)
        labels.append(np.concatenate([lab, [[1, 5, 5, 25, 25]]], 0).astype(np.float32))  # one label nothing finds
    # the real second pass, once, for its contract: forwards of exactly (64, 3, 640, 640), one (k, 6) result per canvas
    shapes = []
    hook = model.register_forward_pre_hook(lambda m, args: shapes.append(tuple(args[0].shape)))
    out, counts, _ = di.double_inference_batch(images, model, preds, labels)
    hook.remove()
    n_crops = sum(s >= 0.25 for p in preds for s in p["scores"])
    assert 0 < n_crops <= 64 and shapes and set(shapes) == {(64, 3, 640, 640)}
    assert len(out) == 3 and out[0] == {"boxes": [], "scores": [], "labels": []} and counts.shape == (3, 3)
    seen = {}
    monkeypatch.setattr(di, "_second_stage", _content_stand_in(seen))
    replaced = 0
    for aligned in (True, False):
        seen.clear()
        out, counts, _ = di.double_inference_batch(images, model, preds, labels, aligned=aligned)
        assert seen["shapes"] == [(64, 640, 640, 3)]  # all crops of the chunk in one padded block
        for b in range(3):
            want, _ = di.double_inference(torch.from_numpy(images[b]), model, preds[b], aligned=aligned)
            assert len(out[b]["boxes"]) == len(want["boxes"])
            np.testing.assert_allclose(np.array(out[b]["boxes"]).reshape(-1, 4), np.array(want["boxes"]).reshape(-1, 4), rtol=0, atol=1e-3)
            np.testing.assert_allclose(np.array(out[b]["scores"]), np.array(want["scores"]), rtol=0, atol=1e-6)
            assert out[b]["labels"] == want["labels"]
            assert PAD_SCORE not in [round(s, 6) for s in out[b]["scores"]]
            rows = np.concatenate([np.array(want["boxes"], np.float32).reshape(-1, 4), np.array(want["scores"], np.float32).reshape(-1, 1),
                                   np.array(want["labels"], np.float32).reshape(-1, 1)], 1)
            assert tuple(counts[b]) == merge_reference(rows, np.zeros((0, 6)), [], [], True, -1.0, labels[b], 0.5)[2]
            first = {tuple(np.float32(v) for v in bx) for bx in preds[b]["boxes"]}
            replaced += sum(tuple(np.float32(v) for v in bx) not in first for bx in out[b]["boxes"])
        assert counts[0].tolist() == [0, 0, 1] and counts[:, 0].sum() > 0
    assert replaced >= 2, "no refinement happened: the stand-in second pass does not exercise the replacement branch"


def _write_split(tmp_path):
    """4 small PNGs of two sizes with 3 labels each; first-stage detections = the label boxes moved by multiples of half a pixel, with
    scores that 5 decimals hold exactly, so that the predictions JSON carries them unchanged."""
    from PIL import Image
    rng = np.random.default_rng(2)
    img_dir, lab_dir = tmp_path / "images", tmp_path / "labels"
    img_dir.mkdir(), lab_dir.mkdir()
    first = {}
    for i, (H, W) in enumerate(((96, 128), (96, 128), (80, 100), (80, 100))):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(img_dir / f"im{i}.png")
        lines, dets = [], []
        for j in range(3):
            w, h = rng.integers(20, 30, 2)
            x1, y1 = 4 + j * (W // 3 - 2), rng.integers(6, H - h - 6)
            cls = int(rng.integers(0, 3))
            lines.append(f"{cls} {(x1 + w / 2) / W:.6f} {(y1 + h / 2) / H:.6f} {w / W:.6f} {h / H:.6f}")
            jit = rng.integers(-3, 4, 4) * 0.5
            dets.append([x1 + jit[0], y1 + jit[1], x1 + w + jit[2], y1 + h + jit[3], 0.5 + 0.125 * j, cls])
        (lab_dir / f"im{i}.txt").write_text("\n".join(lines) + "\n")
        first[f"im{i}"] = np.asarray(dets, np.float32)
    return str(img_dir), str(lab_dir), first


def test_evaluate_two_stage(tmp_path, monkeypatch):
    from ultralytics.models.yolo.detect.val import DetectionValidator
    from ultralytics.utils import double_inference as di
    img_dir, lab_dir, first = _write_split(tmp_path)
    stems = sorted(first)
    sizes = {s: ((96, 128) if s in ("im0", "im1") else (80, 100)) for s in stems}
    net = torch.nn.Linear(1, 1).cuda()
    net.nc = 3

    class StandIn:  # a YOLO as far as evaluate_two_stage looks at it
        model, names = net, {0: "a", 1: "b", 2: "c"}

        def predict(self, source, conf, batch, verbose):
            return [SimpleNamespace(boxes=SimpleNamespace(data=torch.from_numpy(first[os.path.splitext(os.path.basename(p))[0]]).cuda()),
                                    orig_shape=sizes[os.path.splitext(os.path.basename(p))[0]]) for p in source]

    # the second stage returns, for every crop, the label box its detection was made from, mapped into the crop canvas, at 0.9375
    gt = {s: di.ground_truth_rows(os.path.join(lab_dir, s + ".txt"), sizes[s][1], sizes[s][0]) for s in stems}
    dicts = [{"boxes": first[s][:, :4].tolist(), "scores": first[s][:, 4].tolist(), "labels": first[s][:, 5].astype(int).tolist()} for s in stems]
    plan = di.plan_two_stage_chunk(dicts, [sizes[s] for s in stems], 0.25)
    assert len(plan["crop_img"]) == 12
    canvas = []
    for k in range(12):
        b, i = plan["crop_img"][k], plan["crop_row"][k] - plan["row_off"][plan["crop_img"][k]]
        ratio, px, py = plan["scale"][k]
        x1, y1 = plan["rects"][k][:2]
        box = (gt[stems[b]][i, 1:] - [x1, y1, x1, y1]) * ratio + [px, py, px, py]
        canvas.append(torch.tensor([[*box, 0.9375, gt[stems[b]][i, 0]]], dtype=torch.float32).cuda())
    calls = []

    def fake(model_, crops, conf, iou, bs, augment=False):
        calls.append((tuple(crops.shape), augment))
        return canvas + [torch.zeros((0, 6), device=crops.device)] * (crops.shape[0] - 12)

    monkeypatch.setattr(di, "_second_stage", fake)
    res = di.evaluate_two_stage(StandIn(), img_dir, lab_dir)
    assert calls == [((64, 640, 640, 3), True)]  # the script's main runs the second pass with augment on
    assert res["images"] == 4 and res["extra_seconds"] > 0
    r = res["refined"]
    assert (r["tp"], r["fp"], r["fn"]) == (12, 0, 0) and r["precision"] == 1.0 and r["recall"] == 1.0 and r["scored_images"] == 4
    s = res["single"]
    assert s["tp"] + s["fp"] == 12 and s["tp"] + s["fn"] == 12 and s["scored_images"] == 4
    assert s["precision"] == s["tp"] / 12 and list(s["predictions"]) == stems
    for st in stems:  # the refined boxes are the label boxes (up to the fp32 round trip through the canvas)
        np.testing.assert_allclose(np.array(r["predictions"][st]["boxes"]), gt[st][:, 1:], rtol=0, atol=1e-3)
        assert r["predictions"][st]["scores"] == [0.9375] * 3
    # map_50: what DetectionValidator gives for the same rows, one update per image size
    v = DetectionValidator()
    v.device, v.nc, v.names, v.plots_gate = torch.device("cuda:0"), 3, StandIn.names, False
    v.metrics.names = StandIn.names
    for grp in (stems[:2], stems[2:]):
        H, W = sizes[grp[0]]
        preds = [torch.tensor(np.concatenate([np.array(r["predictions"][st]["boxes"], np.float32), np.full((3, 1), 0.9375, np.float32),
                                              np.array(r["predictions"][st]["labels"], np.float32).reshape(-1, 1)], 1)).cuda() for st in grp]
        raw = np.concatenate([di.read_label_rows(os.path.join(lab_dir, st + ".txt")) for st in grp], 0).astype(np.float32)
        v.update_metrics(preds, {"img": torch.empty((0, 3, H, W)), "cls": torch.from_numpy(raw[:, 0].copy()).cuda(),
                                 "bboxes": torch.from_numpy(raw[:, 1:].copy()).cuda(), "ori_shape": [(H, W)] * 2,
                                 "batch_idx": torch.tensor([0.0] * 3 + [1.0] * 3).cuda()})
    v.get_stats()
    assert r["map_50"] == float(v.metrics.box.map50) and r["map_50"] > 0.99
    assert set(r["per_class_ap"]) == {int(c) for c in v.metrics.box.ap_class_index}
    # the same first stage through the JSON the reference's scripts read
    path = str(tmp_path / "predictions.json")
    di.predictions_to_json(StandIn().predict([os.path.join(img_dir, st + ".png") for st in stems], 0.25, 4, False), stems, path)
    again = di.evaluate_two_stage(StandIn(), img_dir, lab_dir, predictions=path)
    for stage in ("single", "refined"):
        for key in ("tp", "fp", "fn", "map_50", "precision", "recall", "per_class_ap", "scored_images", "predictions"):
            assert again[stage][key] == res[stage][key], (stage, key)
