"""Paired bootstrap significance test of two detectors' mAP (drop-in for the numeric part of reference testandcox.py:150-307).

The reference draws 30 resamples of the test split with replacement (half the split each), writes a temporary dataset file per
resample and runs a full ``model.val`` for both models -- 60 validation passes -- then runs Shapiro-Wilk, a paired t-test, Wilcoxon,
a t-interval, a bootstrap confidence interval and Cohen's d on the 30 mAP50 pairs.  Here every model runs over the split ONCE
(``BootstrapValidator`` through the existing hook ``YOLO.val(validator=...)``), the per-detection statistics stay on the device, and
``dy_bootstrap_ap`` computes the AP of every (resample, class, IoU threshold) in one launch from a table of image multiplicities:
no resampled list and no (resamples x detections) array is ever built, so thousands of resamples cost what thirty did.

One divergence from the reference, on purpose: it re-runs inference per resample, so its rectangular validation batches -- and with
them the letterbox padding of every image -- depend on the resample.  Here every image is inferred once, in the batches of the full
split, and only the metric is resampled.
"""
from __future__ import annotations

import csv
import os

import numpy as np
import torch

from ..hip import check, lib
from ..hip.engine import dev_empty
from ..models.yolo.detect import DetectionValidator

NUM_SAMPLES = 30           # testandcox.py:21
SAMPLE_FRACTION = 0.5      # :22
RNG_SEED = 42              # :23
BOOTSTRAP_CI_ITERS = 2000  # :24
MAX_MULT = 65535           # multiplicities travel as uint16


class BootstrapValidator(DetectionValidator):
    """DetectionValidator that also remembers which image every detection and label came from (global index = images seen before
    the batch + position in the batch) and every image's file name.  ``image_stats()`` turns that into the device tensors
    ``bootstrap_map`` reads."""

    def init_metrics(self, model):
        super().init_metrics(model)
        self._det_img, self._lab_img, self.im_files = [], [], []

    def update_metrics(self, preds, batch):
        if not hasattr(self, "_det_img"):
            self._det_img, self._lab_img, self.im_files = [], [], []
        base = self.seen
        tp = super().update_metrics(preds, batch)
        dev = tp.device
        B = len(preds)
        counts = torch.tensor([int(p.shape[0]) for p in preds], dtype=torch.int64, device=dev)
        self._det_img.append(base + torch.repeat_interleave(torch.arange(B, device=dev), counts))
        self._lab_img.append(base + batch["batch_idx"].reshape(-1).to(dev).long())
        files = batch.get("im_file")
        self.im_files += [str(f) for f in files] if files is not None else [f"{base + i:08d}" for i in range(B)]
        return tp

    def image_stats(self):
        """-> dict of device tensors, prepared once per model outside the resample loop: ``tp_bits`` int16 (D) (bit j = true positive
        at IoU threshold j; the bits of an unsigned 16-bit word), ``det_img`` int32 (D), ``cls_off`` int32 (nc + 1), ``lab_cnt``
        int32 (n_img, nc) -- detections sorted by (class, confidence descending), stably -- plus ``conf`` / ``pred_cls`` / ``tp`` in
        that order, ``target_cls`` / ``target_img``, the host array ``det_per_img`` and ``im_files`` / ``n_img`` / ``nc``.
        Image index = position in the SORTED file list (the reference's ``get_image_list``), not the loader's aspect-sorted order."""
        if not self.stats["tp"]:
            raise RuntimeError("image_stats(): no batch has been validated")
        n_img, nc = self.seen, self.nc
        if len(set(self.im_files)) != n_img:
            raise RuntimeError("image_stats(): image file names must be unique")
        dev = self.stats["tp"][0].device
        rank_h = np.empty(n_img, np.int64)
        rank_h[sorted(range(n_img), key=self.im_files.__getitem__)] = np.arange(n_img)
        rank = torch.from_numpy(rank_h).to(dev)
        tp, conf, cls = (torch.cat(self.stats[k], 0) for k in ("tp", "conf", "pred_cls"))
        out = pack_stats(tp, conf, cls, rank[torch.cat(self._det_img, 0)], torch.cat(self.stats["target_cls"], 0),
                         rank[torch.cat(self._lab_img, 0)], n_img, nc)
        out["im_files"] = sorted(self.im_files)
        return out


def pack_stats(tp, conf, pred_cls, det_img, target_cls, target_img, n_img, nc):
    """Concatenated validation statistics (device tensors: tp bool (D, 10), conf (D), pred_cls (D), det_img (D), target_cls (L),
    target_img (L)) -> the dict ``BootstrapValidator.image_stats`` documents.  One stable sort by confidence and one by class: equal
    confidences keep their detection order."""
    dev = tp.device
    cls, det_img = pred_cls.long(), det_img.long()
    tcls, timg = target_cls.long(), target_img.long()
    order = torch.sort(conf, descending=True, stable=True)[1]
    order = order[torch.sort(cls[order], stable=True)[1]]
    tp, conf, cls, det_img = tp[order].bool(), conf[order], cls[order], det_img[order]
    shifts = torch.arange(tp.shape[1], device=dev, dtype=torch.int32)
    tp_bits = (tp.to(torch.int32) << shifts).sum(1).to(torch.int16).contiguous()
    cls_off = torch.zeros(nc + 1, dtype=torch.int32, device=dev)
    cls_off[1:] = torch.bincount(cls, minlength=nc)[:nc].cumsum(0)
    lab_cnt = torch.bincount(timg * nc + tcls, minlength=n_img * nc).to(torch.int32).reshape(n_img, nc).contiguous()
    det_per_img = torch.bincount(det_img, minlength=n_img).cpu().numpy()
    return dict(tp_bits=tp_bits, det_img=det_img.to(torch.int32).contiguous(), cls_off=cls_off, lab_cnt=lab_cnt, conf=conf,
                pred_cls=cls, tp=tp, target_cls=tcls, target_img=timg, det_per_img=det_per_img, n_img=n_img, nc=nc)


def check_mult(mult, n_images=None):
    """(S, n_images) multiplicities as the uint16 table the kernel reads; raises when a count does not fit."""
    mult = np.asarray(mult)
    if mult.ndim != 2 or (n_images is not None and mult.shape[1] != n_images) or mult.shape[0] < 1:
        raise ValueError(f"mult must be (resamples, {n_images if n_images is not None else 'images'}), got {mult.shape}")
    if not np.issubdtype(mult.dtype, np.integer) or mult.min() < 0:
        raise ValueError("mult must hold non-negative integers")
    if mult.max() > MAX_MULT:
        raise ValueError(f"an image occurs {int(mult.max())} times in one resample: more than the {MAX_MULT} a uint16 table holds")
    return np.ascontiguousarray(mult.astype(np.uint16))


def draw_resamples(n_images, num_samples=NUM_SAMPLES, sample_fraction=SAMPLE_FRACTION, seed=RNG_SEED):
    """-> mult uint16 (num_samples, n_images): how often image i (position in the sorted file list) occurs in resample s.
    Consumes the legacy generator exactly as the reference's ``np.random.seed(seed)`` followed by one
    ``np.random.choice(all_test_images, size=n_size, replace=True)`` per iteration does (testandcox.py:153, 162, 176)."""
    if n_images < 1:
        raise ValueError("no images to resample")
    n_size = max(1, int(n_images * sample_fraction))
    rs = np.random.RandomState(seed)
    mult = np.stack([np.bincount(rs.choice(n_images, size=n_size, replace=True), minlength=n_images) for _ in range(num_samples)])
    return check_mult(mult, n_images)


def bootstrap_map(stats, mult):
    """AP of every resample from one validation pass.  stats: ``BootstrapValidator.image_stats()``; mult: (S, n_img) multiplicities.
    -> (map50 (S), map50_95 (S), ap (S, nc, 10)) float64 numpy: the means of ``Metric.map50`` / ``Metric.map`` -- over the classes
    that have a label in the resample; a class with labels and no detection counts as 0."""
    n_img, nc = stats["n_img"], stats["nc"]
    mult = check_mult(mult, n_img)
    S = mult.shape[0]
    if int((mult.astype(np.int64) @ stats["det_per_img"].astype(np.int64)).max(initial=0)) >= 2 ** 31:
        raise ValueError("a resample holds 2^31 detections or more")
    dev = stats["tp_bits"].device
    if dev.type != "cuda":
        raise RuntimeError("bootstrap_map: HIP path only (no CPU fallback)")
    m = torch.from_numpy(mult.view(np.int16)).to(dev)
    ap = dev_empty((S, nc, 10), torch.float64, dev)
    nl = dev_empty((S, nc), torch.int32, dev)
    D = int(stats["tp_bits"].numel())
    check(lib().dy_bootstrap_ap(stats["tp_bits"].data_ptr(), stats["det_img"].data_ptr(), stats["cls_off"].data_ptr(),
                                stats["lab_cnt"].data_ptr(), m.data_ptr(), D, n_img, nc, S, ap.data_ptr(), nl.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream), "dy_bootstrap_ap")
    ap_h, has = ap.cpu().numpy(), nl.cpu().numpy() > 0
    n_cls = np.maximum(has.sum(1), 1)
    map50 = (ap_h[:, :, 0] * has).sum(1) / n_cls
    map5095 = (ap_h * has[:, :, None]).sum((1, 2)) / (n_cls * ap_h.shape[2])
    return map50, map5095, ap_h


def paired_statistics(deal_scores, base_scores, seed=RNG_SEED, ci_iters=BOOTSTRAP_CI_ITERS, alpha=0.05):
    """The statistics of testandcox.py:233-296 on paired scores, as a dict: means, Shapiro-Wilk on the differences, paired t-test,
    Wilcoxon signed-rank (``zero_method='wilcox'``), the 95 % t-interval and bootstrap interval of the mean difference, Cohen's d and
    the verdict at ``alpha`` (Wilcoxon first, then the t-test).  A test that cannot run on the data gives nan, as in the reference."""
    from scipy import stats
    a, b = np.asarray(deal_scores, np.float64), np.asarray(base_scores, np.float64)
    diffs = a - b
    n = len(diffs)
    try:
        p_norm = float(stats.shapiro(diffs)[1])
    except Exception:
        p_norm = float("nan")
    t_stat, p_t = (float(v) for v in stats.ttest_rel(a, b))
    try:
        w_stat, p_w = (float(v) for v in stats.wilcoxon(a, b, zero_method="wilcox", alternative="two-sided"))
    except Exception:
        w_stat, p_w = float("nan"), float("nan")
    mean_diff, sd = float(diffs.mean()), float(diffs.std(ddof=1))
    stderr = sd / np.sqrt(n)
    t_crit = float(stats.t.ppf(1 - 0.025, df=n - 1))
    rng = np.random.RandomState(seed)
    bs_means = np.array([rng.choice(diffs, size=n, replace=True).mean() for _ in range(ci_iters)])
    bs_ci = np.percentile(bs_means, [2.5, 97.5])
    if not np.isnan(p_w) and p_w < alpha:
        significant, verdict = True, f"Significant difference (Wilcoxon p = {p_w:.4e})"
    elif p_t < alpha:
        significant, verdict = True, f"Significant difference (paired t-test p = {p_t:.4e})"
    else:
        significant, verdict = False, "No significant difference detected by either test."
    return dict(n=n, deal_mean=float(a.mean()), base_mean=float(b.mean()), mean_diff=mean_diff, std_diff=sd, shapiro_p=p_norm,
                t_stat=t_stat, t_p=p_t, wilcoxon_w=w_stat, wilcoxon_p=p_w,
                ci_t=(mean_diff - t_crit * stderr, mean_diff + t_crit * stderr), ci_bootstrap=(float(bs_ci[0]), float(bs_ci[1])),
                cohens_d=float("nan") if sd == 0 else mean_diff / sd, alpha=alpha, significant=significant, verdict=verdict)


def summary_lines(res):
    """The lines the reference script prints (testandcox.py:236-296)."""
    mark = "✅ " if res["significant"] else "❌ "
    return ["", "Summary statistics:", f"Deal-YOLO mean mAP@0.5: {res['deal_mean']:.6f}", f"Baseline mean mAP@0.5:   {res['base_mean']:.6f}",
            f"Mean difference (deal - base): {res['mean_diff']:.6f}", f"Std of differences: {res['std_diff']:.6f}",
            f"Shapiro-Wilk p-value for differences: {res['shapiro_p']:.4f}", "",
            f"Paired t-test: t={res['t_stat']:.4f}, p={res['t_p']:.4e}", "",
            f"Wilcoxon signed-rank: W={res['wilcoxon_w']}, p={res['wilcoxon_p']:.4e}", "",
            f"95% CI (t-interval) for mean difference: [{res['ci_t'][0]:.6f}, {res['ci_t'][1]:.6f}]",
            f"95% Bootstrap CI for mean difference: [{res['ci_bootstrap'][0]:.6f}, {res['ci_bootstrap'][1]:.6f}]", "",
            f"Cohen's d (paired): {res['cohens_d']:.4f}", "", f"Final decision (alpha = {res['alpha']}):", mark + res["verdict"]]


def _plot_histogram(diffs, path):
    """testandcox.py:299-306; control plane: skipped when matplotlib is not installed."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return None
    plt.figure(figsize=(6, 4))
    plt.hist(diffs, bins=min(15, len(diffs)), edgecolor="k")
    plt.axvline(diffs.mean(), linestyle="--", label=f"mean diff = {diffs.mean():.4f}")
    plt.title("Distribution of per-iteration mAP@0.5 differences (deal - baseline)")
    plt.xlabel("mAP@0.5 difference")
    plt.legend()
    plt.tight_layout()
    plt.savefig(path)
    plt.close()
    return path


def paired_bootstrap_test(model_a, model_b, data, split="test", num_samples=NUM_SAMPLES, sample_fraction=SAMPLE_FRACTION, seed=RNG_SEED,
                          ci_iters=BOOTSTRAP_CI_ITERS, save_dir=".", plot=True, **val_kwargs):
    """``model_a`` ("deal") against ``model_b`` ("base"): ``YOLO`` objects or weight / YAML paths; ``data``: the dataset YAML.
    One validation pass per model over ``split``, the SAME resamples for both (paired), then ``paired_statistics``.  Returns its
    dict plus ``deal_map50`` / ``base_map50`` / ``diffs`` (num_samples each), ``deal_map`` / ``base_map`` (mAP50-95), ``mult``,
    ``im_files`` and ``csv``; writes ``<save_dir>/bootstrap_map50_results.csv`` (iter, deal_map50, base_map50, diff) and, with
    ``plot`` and matplotlib, ``diffs_histogram.png``.  Inference runs once per image, in the batches of the full split -- the
    reference's per-resample batch shapes are not reproduced (module docstring)."""
    from ..engine.model import YOLO
    stats = []
    for m in (model_a, model_b):
        m = m if isinstance(m, YOLO) else YOLO(m)
        m.val(validator=BootstrapValidator, data=data, split=split, **val_kwargs)
        stats.append(m.validator.image_stats())
    if stats[0]["im_files"] != stats[1]["im_files"]:
        raise RuntimeError("the two models validated different image lists")
    mult = draw_resamples(stats[0]["n_img"], num_samples, sample_fraction, seed)
    (a50, a95, _), (b50, b95, _) = (bootstrap_map(s, mult) for s in stats)
    res = paired_statistics(a50, b50, seed, ci_iters)
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, "bootstrap_map50_results.csv")
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["iter", "deal_map50", "base_map50", "diff"])
        for i, (x, y) in enumerate(zip(a50, b50)):
            w.writerow([i + 1, repr(float(x)), repr(float(y)), repr(float(x) - float(y))])
    res.update(deal_map50=a50, base_map50=b50, diffs=a50 - b50, deal_map=a95, base_map=b95, mult=mult, im_files=stats[0]["im_files"],
               csv=path, histogram=_plot_histogram(a50 - b50, os.path.join(save_dir, "diffs_histogram.png")) if plot else None)
    return res
