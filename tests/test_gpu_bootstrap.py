"""-m gpu: the device-side bootstrap of the validation statistics (csrc/bootstrap.hip: dy_bootstrap_ap, behind
ultralytics/utils/bootstrap.py) against the reference fixture tests/golden/bootstrap.npz and the CPU oracle on replicated lists,
against the existing validator on the metric cases, and end to end through ``paired_bootstrap_test``.

Tolerance: 1e-9 absolute, the bound tests/test_gpu_metrics.py uses for mAP (counts are exact integers, the quotients and the
integral are fp64 on both sides)."""
import csv
import os

import numpy as np
import pytest
import torch

from golden.cases import metric_cases, metric_geometry, synth_detections, write_dataset
from oracle import metrics as om

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _pack(tp, conf, pred_cls, det_img, lab_cls, lab_img, n_img, nc):
    from ultralytics.utils.bootstrap import pack_stats
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    return pack_stats(t(tp, torch.bool), t(conf, torch.float64), t(pred_cls, torch.int64), t(det_img, torch.int64), t(lab_cls, torch.int64),
                      t(lab_img, torch.int64), n_img, nc)


def _oracle(tp, conf, pred_cls, det_img, lab_cls, lab_img, mult, nc):
    """oracle.metrics.ap_per_class on the replicated list of every resample -> (ap (S, nc, 10), nl (S, nc), map50, map50-95)."""
    S = mult.shape[0]
    ap, nl, m50, m = np.zeros((S, nc, 10)), np.zeros((S, nc), np.int64), np.zeros(S), np.zeros(S)
    for s in range(S):
        rd, rl = mult[s][det_img], mult[s][lab_img]
        res = om.ap_per_class(np.repeat(tp, rd, 0), np.repeat(conf, rd), np.repeat(pred_cls, rd).astype(np.float64),
                              np.repeat(lab_cls, rl).astype(np.float64))
        ap[s, res["classes"]] = res["ap"]
        nl[s] = np.bincount(np.repeat(lab_cls, rl).astype(int), minlength=nc)
        _, _, m50[s], m[s] = om.mean_results(res)
    return ap, nl, m50, m


@pytest.mark.parametrize("case", ["big", "exact"])
def test_kernel_vs_reference_fixture_and_oracle(golden, case):
    """7 images, 3 classes, 6 resamples, multiplicities 0..4 (the situations each case covers: tests/golden/make_bootstrap_golden.py)."""
    from ultralytics.utils.bootstrap import bootstrap_map
    G = golden("bootstrap")
    a = {k: G[f"{case}/{k}"] for k in ("tp", "conf", "pred_cls", "det_img", "lab_cls", "lab_img", "mult", "ap", "nl")}
    stats = _pack(a["tp"], a["conf"], a["pred_cls"], a["det_img"], a["lab_cls"], a["lab_img"], 7, 3)
    assert stats["cls_off"].tolist() == [0, *np.cumsum(np.bincount(a["pred_cls"], minlength=3)).tolist()]
    assert (stats["lab_cnt"].sum(0).cpu().numpy() == np.bincount(a["lab_cls"], minlength=3)).all()
    map50, map5095, ap = bootstrap_map(stats, a["mult"])
    o_ap, o_nl, o50, o5095 = _oracle(a["tp"], a["conf"], a["pred_cls"], a["det_img"], a["lab_cls"], a["lab_img"], a["mult"], 3)
    print(case, "max |ap - fixture|", np.abs(ap - a["ap"]).max(), "max |ap - oracle|", np.abs(ap - o_ap).max(),
          "max |mAP50 - oracle|", np.abs(map50 - o50).max(), "max |mAP50-95 - oracle|", np.abs(map5095 - o5095).max())
    assert ap.shape == (6, 3, 10) and (o_nl == a["nl"]).all()
    assert np.abs(ap - a["ap"]).max() < TOL and np.abs(ap - o_ap).max() < TOL
    # Metric.map50 / Metric.map: the mean over the classes that have a label in the resample (a class without detections counts as 0)
    assert np.abs(map50 - o50).max() < TOL and np.abs(map5095 - o5095).max() < TOL
    has = a["nl"] > 0
    assert np.abs(map50 - np.array([a["ap"][s, has[s], 0].mean() for s in range(6)])).max() < TOL


def test_kernel_many_images_and_large_multiplicities():
    """More images than the kernel stages in LDS (8,192: the multiplicity row is gathered from global memory instead), multiplicities
    up to 300, two classes whose lists cross several 256-detection chunks; against the oracle on the replicated lists."""
    from ultralytics.utils.bootstrap import bootstrap_map
    rng = np.random.default_rng(31)
    n_img, nc, S, busy = 8200, 2, 3, 40
    imgs = np.sort(rng.choice(n_img, busy, replace=False))
    tp, conf, cls, dimg, lcls, limg = [], [], [], [], [], []
    for c, per in ((0, 20), (1, 9)):
        for i in imgs:
            n_lab = int(rng.integers(1, 6))
            depth = np.where(rng.random(per) < 0.5, rng.integers(1, 11, per), 0)
            t = depth[:, None] > np.arange(10)[None, :]
            for j in range(10):  # no more true positives than labels per (image, class, threshold)
                hits = np.flatnonzero(t[:, j])
                t[hits[n_lab:], j:] = False
            tp.append(t); cls += [c] * per; dimg += [i] * per; lcls += [c] * n_lab; limg += [i] * n_lab
        n = per * busy
        conf.append((rng.permutation(n) + 1) / (n + 1))
    tp, conf, cls, dimg, lcls, limg = np.concatenate(tp), np.concatenate(conf), np.array(cls), np.array(dimg), np.array(lcls), np.array(limg)
    mult = np.zeros((S, n_img), np.int64)
    mult[0] = 1
    mult[1, imgs] = rng.integers(0, 4, busy)
    mult[2, imgs[:5]] = [300, 1, 0, 257, 64]
    mult[:, n_img - 1] += 2  # an image without detections or labels
    map50, map5095, ap = bootstrap_map(_pack(tp, conf, cls, dimg, lcls, limg, n_img, nc), mult)
    o_ap, _, o50, o5095 = _oracle(tp, conf, cls, dimg, lcls, limg, mult, nc)
    print("max |ap - oracle|", np.abs(ap - o_ap).max())
    assert np.abs(ap - o_ap).max() < TOL and np.abs(map50 - o50).max() < TOL and np.abs(map5095 - o5095).max() < TOL
    assert o_ap[:, :, 0].min() > 0


@pytest.mark.parametrize("case", metric_cases(), ids=lambda c: c[0])
def test_every_image_once_equals_the_validator(golden, case):
    """S = 1, all multiplicities 1: the bootstrap path gives the validator's own mAP50 / mAP50-95 (and with it metrics.npz)."""
    from ultralytics.utils.bootstrap import BootstrapValidator, bootstrap_map
    name, seed, n_images, nc, ml, md, jit = case
    batch, preds = synth_detections(seed, n_images, nc, ml, md, jit)
    geo = metric_geometry(name, n_images)
    tb = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    tb["img"] = torch.zeros(n_images, 3, 640, 640, device="cuda")
    tb["ori_shape"], tb["ratio_pad"] = [g[0] for g in geo], [g[1] for g in geo]
    v = BootstrapValidator(args=None)
    v.device = torch.device("cuda:0")
    v.nc, v.names = nc, {i: str(i) for i in range(nc)}
    v.metrics.names = v.names
    v.update_metrics([torch.from_numpy(p).cuda() for p in preds], tb)
    res = v.get_stats()
    stats = v.image_stats()
    assert stats["n_img"] == n_images and len(stats["im_files"]) == n_images
    assert stats["det_per_img"].tolist() == [len(p) for p in preds]
    map50, map5095, ap = bootstrap_map(stats, np.ones((1, n_images), np.int64))
    print(name, "mAP50", map50[0], res["metrics/mAP50(B)"], "mAP50-95", map5095[0], res["metrics/mAP50-95(B)"])
    assert abs(map50[0] - res["metrics/mAP50(B)"]) < TOL and abs(map5095[0] - res["metrics/mAP50-95(B)"]) < TOL
    mp, mr, m50, m = golden("metrics")[f"{name}/mean_results"]
    assert abs(map50[0] - m50) < TOL and abs(map5095[0] - m) < TOL
    # every image twice is the same curve
    twice = bootstrap_map(stats, np.full((1, n_images), 2))
    assert abs(twice[0][0] - map50[0]) < TOL and abs(twice[1][0] - map5095[0]) < TOL


def test_paired_bootstrap_test_end_to_end(tmp_path):
    """Two randomly initialised yolov8n-ASF-P2P2 models on the fixture dataset (its 9 readable train images as the 'test' split), imgsz 64,
    5 resamples: finite scores that equal this package's host ap_per_class on the replicated statistics of the same pass, a CSV with
    one row per resample, and bit-identical results from a second call.  (Untrained models: this test is about the plumbing -- image
    order, pairing, files, determinism; the numbers are the business of the tests above.)"""
    from ultralytics import YOLO
    from ultralytics.nn.tasks import DetectionModel
    from ultralytics.utils.bootstrap import paired_bootstrap_test
    from ultralytics.utils.metrics import ap_per_class
    root = str(tmp_path / "ds")
    write_dataset(root)
    data = os.path.join(root, "data_test.yaml")
    with open(data, "w") as f:
        f.write("path: .\ntrain: images/train\nval: images/val\ntest: images/train\nnc: 4\nnames: [a, b, c, d]\n")
    models = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        y = YOLO("yolov8n-ASF-P2P2.yaml")
        y.model = DetectionModel("yolov8n-ASF-P2P2.yaml", nc=4, verbose=False)
        models.append(y)
    S = 5
    # conf=1e-6: an untrained head scores below the validation default 0.001 everywhere and would hand over no detection at all
    kw = dict(split="test", num_samples=S, sample_fraction=0.5, seed=42, ci_iters=50, plot=False, imgsz=64, batch=4, conf=1e-6)
    res = paired_bootstrap_test(models[0], models[1], data, save_dir=str(tmp_path / "out1"), **kw)
    n_img = len(res["im_files"])
    assert n_img == 9 and res["im_files"] == sorted(res["im_files"]) and res["mult"].shape == (S, n_img)
    assert (res["mult"].sum(1) == 4).all()
    for key in ("deal_map50", "base_map50", "deal_map", "base_map", "diffs"):
        assert res[key].shape == (S,) and np.isfinite(res[key]).all()
    assert res["histogram"] is None and not os.path.exists(tmp_path / "out1" / "diffs_histogram.png")
    for y, key in zip(models, ("deal_map50", "base_map50")):
        st = y.validator.image_stats()
        assert st["n_img"] == n_img and st["im_files"] == res["im_files"]
        assert st["det_per_img"].sum() == st["tp_bits"].numel() > 0 and int(st["lab_cnt"].sum()) == 15  # the split's 15 labels
        conf = st["conf"].double().cpu().numpy()
        cls, tp = st["pred_cls"].cpu().numpy(), st["tp"].cpu().numpy()
        assert all((np.diff(conf[cls == c]) <= 0).all() for c in range(4))  # sorted by confidence inside every class
        # numpy's argsort is not stable: exact confidence ties are broken in the (stable) order the device path defines; 1e-17 per place
        # (at most 2.7e-14 over 9 x 300 detections) is below the spacing of fp32 confidences above the threshold 1e-6 (1.1e-13)
        assert len(conf) <= 2700 and conf.min() >= 1e-6
        conf = conf - np.arange(len(conf)) * 1e-17
        dimg, tcls, timg = st["det_img"].cpu().numpy(), st["target_cls"].cpu().numpy(), st["target_img"].cpu().numpy()
        for s in range(S):
            rd, rl = res["mult"][s][dimg].astype(int), res["mult"][s][timg].astype(int)
            want = 0.0
            if rl.sum():
                out = ap_per_class(np.repeat(tp, rd, 0), np.repeat(conf, rd), np.repeat(cls, rd), np.repeat(tcls, rl))
                want = out[5][:, 0].mean() if len(out[5]) else 0.0
            print(key, s, res[key][s], want)
            assert abs(res[key][s] - want) < TOL
    rows = list(csv.reader(open(res["csv"])))
    assert rows[0] == ["iter", "deal_map50", "base_map50", "diff"] and len(rows) == 1 + S
    assert [int(r[0]) for r in rows[1:]] == list(range(1, S + 1))
    assert [float(r[1]) for r in rows[1:]] == res["deal_map50"].tolist() and [float(r[3]) for r in rows[1:]] == res["diffs"].tolist()
    again = paired_bootstrap_test(models[0], models[1], data, save_dir=str(tmp_path / "out2"), **kw)
    for key in ("deal_map50", "base_map50", "deal_map", "base_map", "mult"):
        assert np.array_equal(again[key], res[key])
    assert open(again["csv"]).read() == open(res["csv"]).read()


def test_image_order_from_the_loader_to_the_sorted_file_list(tmp_path):
    """``YOLO.val(validator=...)`` on the fixture dataset with a validator that answers the labels with detections (the label's own box
    and a shifted copy; which of them, and in which order of confidence, is a function of the image's FILE), so that scores are
    non-zero without a trained model and differ between resamples.  The loader's rectangular batches are aspect-sorted; the
    multiplicity table is indexed by the SORTED file list.  The host side replicates by file name from the validator's raw,
    loader-ordered statistics."""
    from ultralytics import YOLO
    from ultralytics.utils.bootstrap import BootstrapValidator, bootstrap_map, draw_resamples
    from ultralytics.utils.metrics import ap_per_class

    class LabelEcho(BootstrapValidator):
        def update_metrics(self, preds, batch):
            h, w = batch["img"].shape[2:]
            bi, cls, box = batch["batch_idx"].reshape(-1), batch["cls"].reshape(-1).float(), batch["bboxes"].reshape(-1, 4).float()
            fake = []
            for i, f in enumerate(batch["im_file"]):
                g = int(os.path.basename(f)[1:3])  # t00 .. t12
                sel = bi == i
                b, c = box[sel], cls[sel]
                xyxy = torch.stack([(b[:, 0] - b[:, 2] / 2) * w, (b[:, 1] - b[:, 3] / 2) * h, (b[:, 0] + b[:, 2] / 2) * w, (b[:, 1] + b[:, 3] / 2) * h], 1)
                shifted = xyxy + (b[:, 2:3] * w * 0.7) * torch.tensor([1.0, 0.0, 1.0, 0.0], device=b.device)  # IoU 0.18 with its label
                # what an image adds depends on the image (so a resample's score depends on WHICH images it holds): in even files the
                # label's own box outranks the shifted copy, in odd ones the copy comes first; every third file has no copies; files
                # 1, 5, 9 miss their first label
                n = len(b)
                k = torch.arange(n, device=b.device)
                base = 1 + ((g * 7) % 13) * 8  # confidences distinct over the dataset, not monotone in the file order
                own = torch.cat([xyxy, ((base + k + (n if g % 2 == 0 else 0)).float() / 200)[:, None], c[:, None]], 1)[(1 if g % 4 == 1 else 0):]
                copy = torch.cat([shifted, ((base + k + (0 if g % 2 == 0 else n)).float() / 200)[:, None], c[:, None]], 1)[:(0 if g % 3 == 0 else n)]
                det = torch.cat([own, copy], 0)
                fake.append(det[torch.argsort(det[:, 4], descending=True)])
            return super().update_metrics(fake, batch)

    root = str(tmp_path / "ds")
    write_dataset(root)
    data = os.path.join(root, "data_test.yaml")
    with open(data, "w") as f:
        f.write("path: .\ntrain: images/train\nval: images/val\ntest: images/train\nnc: 4\nnames: [a, b, c, d]\n")
    y = YOLO("yolov8n-ASF-P2P2.yaml")
    y.val(validator=LabelEcho, data=data, split="test", imgsz=64, batch=4)
    v = y.validator
    files = sorted(v.im_files)
    assert len(files) == 9 and v.im_files != files  # the loader did reorder
    st = v.image_stats()
    assert st["im_files"] == files
    mult = draw_resamples(9, 5, 0.5, 42)
    map50, map5095, ap = bootstrap_map(st, mult)
    tp, conf, cls = (torch.cat(v.stats[k], 0).cpu().numpy() for k in ("tp", "conf", "pred_cls"))
    assert len(np.unique(conf)) == len(conf)
    where = np.array([files.index(f) for f in v.im_files])  # loader position -> place in the sorted list
    dimg, timg = where[torch.cat(v._det_img, 0).cpu().numpy()], where[torch.cat(v._lab_img, 0).cpu().numpy()]
    tcls = torch.cat(v.stats["target_cls"], 0).cpu().numpy()
    for s in range(5):
        rd, rl = mult[s][dimg].astype(int), mult[s][timg].astype(int)
        out = ap_per_class(np.repeat(tp, rd, 0), np.repeat(conf, rd).astype(np.float64), np.repeat(cls, rd), np.repeat(tcls, rl))[5]
        want50, want = (out[:, 0].mean(), out.mean()) if len(out) else (0.0, 0.0)
        print(s, map50[s], want50, map5095[s], want)
        assert abs(map50[s] - want50) < TOL and abs(map5095[s] - want) < TOL
    assert map50.max() > 0.1 and len(np.unique(np.round(map50, 12))) > 1  # real scores that differ between resamples
