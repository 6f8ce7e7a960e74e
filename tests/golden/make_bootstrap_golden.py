"""Generate tests/golden/bootstrap.npz from the REFERENCE implementation: ``ap_per_class`` (reference ultralytics/utils/metrics.py
:1142-1230) on REPLICATED validation statistics -- every detection and label of image i repeated ``mult[s, i]`` times -- which is
what the reference's bootstrap script (testandcox.py:150-227) scores per resample, and what ``dy_bootstrap_ap`` must reproduce from
the multiplicity table alone.

Run in the build container only (needs the reference tree, which ``_refimport`` locates):

    python tests/golden/make_bootstrap_golden.py

Every case has 7 images, 3 classes, 6 resamples with multiplicities 0..4.  Per case ``<case>/``: the un-replicated statistics ``tp``
(D, 10) bool, ``conf`` (D) float64, ``pred_cls`` (D), ``det_img`` (D), ``lab_cls`` (L), ``lab_img`` (L); ``mult`` (6, 7); and the
reference's answer ``ap`` (6, 3, 10) float64 (rows of classes without labels in the resample stay zero) with ``nl`` (6, 3).

Conditions the generator keeps (the reference is undefined otherwise): confidences are distinct within a class (a permutation); for
every (image, class, threshold) the true positives do not exceed that image's labels of the class (recall <= 1); every resample holds at
least one label.

  big     class 0: 701 detections over all images (chunk and wave boundaries, not a multiple of 64); class 1: labels in images 2, 4, 6,
          detections in images 0, 1, 2, 4 -- a resample with labels but no detections (counts as 0), one with detections but no labels
          (left out), n_l = 1 and n_l = 3 in two single-image resamples; class 2 absent altogether.
  exact   class 0: 50 labels, every one found at IoU 0.5 behind three leading false positives (recall reaches exactly 1; recalls land
          on grid points; n_l = 100 when every image counts twice); class 1: labels but only false positives; class 2: three labels in
          one image, list FP FP TP FP TP TP.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N_IMG, NC, NT = 7, 3, 10


def _tp_rows(rng, n, budget, p0):
    """n detections of one (image, class): nested true-positive flags (a hit at threshold j + 1 is a hit at j), at most ``budget`` hits
    per threshold."""
    depth = np.where(rng.random(n) < p0, rng.integers(1, NT + 1, n), 0)  # number of thresholds the detection passes
    tp = depth[:, None] > np.arange(NT)[None, :]
    for j in range(NT):
        hits = np.flatnonzero(tp[:, j])
        if len(hits) > budget:
            tp[rng.permutation(hits)[budget:], j:] = False
    return tp


def case_big():
    rng = np.random.default_rng(2024)
    labels = {0: [20, 15, 30, 10, 25, 0, 12], 1: [0, 0, 1, 0, 3, 0, 2], 2: [0] * 7}
    dets = {0: [100, 101, 100, 100, 100, 100, 100], 1: [9, 7, 3, 0, 5, 0, 0], 2: [0] * 7}
    mult = np.array([[1, 1, 1, 1, 1, 1, 1], [0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0], [4, 0, 3, 2, 0, 1, 2], [2, 3, 0, 0, 0, 4, 0],
                     [0, 0, 0, 3, 0, 2, 4]])
    return _assemble(rng, labels, dets, mult, p0=0.6)


def case_exact():
    rng = np.random.default_rng(2025)
    lab0 = [10, 5, 8, 7, 6, 4, 10]
    labels = {0: lab0, 1: [0, 3, 0, 0, 0, 0, 0], 2: [0, 0, 0, 3, 0, 0, 0]}
    mult = np.array([[1, 1, 1, 1, 1, 1, 1], [2, 2, 2, 2, 2, 2, 2], [4, 0, 1, 2, 3, 0, 1], [0, 0, 0, 1, 0, 0, 0], [1, 2, 3, 4, 0, 1, 2],
                     [3, 3, 0, 0, 1, 1, 4]])
    tp, cls, img = [], [], []
    # class 0: three false positives first (images 0, 2, 5), then every label as a hit at IoU 0.5 interleaved with false positives
    rows = [(0, np.zeros(NT, bool)), (2, np.zeros(NT, bool)), (5, np.zeros(NT, bool))]
    body = []
    for i, n in enumerate(lab0):
        depth = rng.integers(1, NT + 1, n)
        body += [(i, d > np.arange(NT)) for d in depth]
        body += [(i, np.zeros(NT, bool)) for _ in range(int(rng.integers(0, 4)))]
    rows += [body[k] for k in rng.permutation(len(body))]
    conf0 = 1.0 - (np.arange(len(rows)) + 1) / (len(rows) + 1)  # list order = confidence order
    for i, t in rows:
        tp.append(t); cls.append(0); img.append(i)
    conf = list(conf0)
    for i in (0, 1, 1, 4, 6):  # class 1: false positives only
        tp.append(np.zeros(NT, bool)); cls.append(1); img.append(i)
    conf += [0.9, 0.8, 0.55, 0.3, 0.1]
    seq = [0, 0, 10, 0, 4, 1]  # class 2, image 3: FP FP TP FP TP TP (depths)
    for d in seq:
        tp.append(d > np.arange(NT)); cls.append(2); img.append(3)
    conf += [0.95, 0.85, 0.75, 0.65, 0.45, 0.35]
    lab_cls = np.concatenate([np.full(sum(v), c) for c, v in labels.items()])
    lab_img = np.concatenate([np.repeat(np.arange(N_IMG), v) for v in labels.values()])
    shuffle = rng.permutation(len(tp))  # the stored order is not the sorted one
    return dict(tp=np.array(tp)[shuffle], conf=np.array(conf, np.float64)[shuffle], pred_cls=np.array(cls)[shuffle],
                det_img=np.array(img)[shuffle], lab_cls=lab_cls, lab_img=lab_img, mult=mult)


def _assemble(rng, labels, dets, mult, p0):
    tp, cls, img, conf = [], [], [], []
    for c in range(NC):
        n_c = sum(dets[c])
        conf_c = (rng.permutation(n_c) + 1) / (n_c + 1)
        k = 0
        for i in range(N_IMG):
            n = dets[c][i]
            tp.append(_tp_rows(rng, n, labels[c][i], p0)); cls.append(np.full(n, c)); img.append(np.full(n, i))
            conf.append(conf_c[k:k + n])
            k += n
    lab_cls = np.concatenate([np.full(sum(v), c) for c, v in labels.items()])
    lab_img = np.concatenate([np.repeat(np.arange(N_IMG), v) for v in labels.values()])
    return dict(tp=np.concatenate(tp), conf=np.concatenate(conf).astype(np.float64), pred_cls=np.concatenate(cls),
                det_img=np.concatenate(img), lab_cls=lab_cls.astype(np.int64), lab_img=lab_img, mult=mult)


CASES = {"big": case_big, "exact": case_exact}


def check_conditions(c):
    for k in range(NC):
        sel = c["pred_cls"] == k
        assert len(np.unique(c["conf"][sel])) == sel.sum(), "confidences must be distinct within a class"
        for i in range(N_IMG):
            n_lab = int(((c["lab_cls"] == k) & (c["lab_img"] == i)).sum())
            assert (c["tp"][sel & (c["det_img"] == i)].sum(0) <= n_lab).all(), "more true positives than labels"
    assert c["mult"].shape == (6, N_IMG) and c["mult"].min() >= 0 and c["mult"].max() <= 4
    for m in c["mult"]:
        assert m[c["lab_img"]].sum() > 0, "a resample without labels"


def replicate(c, m):
    """Statistics of the resample in which image i occurs m[i] times."""
    rd, rl = m[c["det_img"]], m[c["lab_img"]]
    return (np.repeat(c["tp"], rd, 0), np.repeat(c["conf"], rd), np.repeat(c["pred_cls"], rd).astype(np.float64),
            np.repeat(c["lab_cls"], rl).astype(np.float64))


def main():
    import _refimport
    _refimport.install()
    from ultralytics.utils import metrics as ref_metrics
    assert ref_metrics.__file__.startswith(_refimport.REF)
    arrs = {}
    for name, make in CASES.items():
        c = make()
        check_conditions(c)
        S = c["mult"].shape[0]
        ap, nl = np.zeros((S, NC, NT)), np.zeros((S, NC), np.int32)
        for s in range(S):
            tp, conf, pcls, tcls = replicate(c, c["mult"][s])
            res = ref_metrics.ap_per_class(tp, conf, pcls, tcls, plot=False, names={i: str(i) for i in range(NC)})
            ap[s, res[6]] = res[5]
            nl[s] = np.bincount(tcls.astype(int), minlength=NC)
        for k, v in c.items():
            arrs[f"{name}/{k}"] = v
        arrs[f"{name}/ap"], arrs[f"{name}/nl"] = ap, nl
        print(name, "detections", len(c["conf"]), "per class", np.bincount(c["pred_cls"], minlength=NC).tolist(), "nl", nl.tolist())
        print("  mAP50 per resample", [round(float(ap[s, nl[s] > 0, 0].mean()), 6) for s in range(S)])
    path = os.path.join(HERE, "bootstrap.npz")
    np.savez_compressed(path, **arrs)
    assert os.path.getsize(path) < 1 << 20
    print(f"bootstrap.npz  {os.path.getsize(path) / 1024:.1f} KiB  ({len(arrs)} arrays)")


if __name__ == "__main__":
    main()
