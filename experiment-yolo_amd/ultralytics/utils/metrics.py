"""Detection metrics with the reference's names and return conventions (reference ultralytics/utils/metrics.py).

``box_iou`` runs on the GPU (libdealyolo_hip: dy_box_iou); the per-batch matching lives in
``ultralytics.models.yolo.detect.DetectionValidator`` (dy_match_predictions).  ``ap_per_class`` / ``compute_ap`` / ``smooth``
and the ``Metric`` / ``DetMetrics`` containers are host arithmetic in the reference as well (numpy on the concatenated
statistics, utils/metrics.py:1051-1480) and stay host arithmetic here.  ``ConfusionMatrix`` counts on the device (dy_confusion_matrix:
one launch per batch from the validator, one per ``process_batch`` call) and is read back when ``.matrix`` is asked for; plotting is
control plane.
"""
import ctypes as C

import numpy as np
import torch

from ..hip import check, lib
from ..hip.engine import dev_empty


def box_iou(box1, box2, eps=1e-7):
    """(N,4) x (M,4) xyxy -> (N,M) IoU (reference utils/metrics.py:53-73); CUDA tensors only."""
    if box1.device.type != "cuda" or box2.device.type != "cuda":
        raise RuntimeError("box_iou: HIP path only (no CPU fallback)")
    if eps != 1e-7:
        raise NotImplementedError("box_iou: eps is fixed at the reference default 1e-7")
    a, b = box1.float().contiguous(), box2.float().contiguous()
    out = dev_empty((a.shape[0], b.shape[0]), torch.float32, a.device)
    check(lib().dy_box_iou(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], out.data_ptr(),
                           torch.cuda.current_stream(a.device).cuda_stream), "dy_box_iou")
    return out


def smooth(y, f=0.05):
    """Box filter of fraction f (reference :1051-1056)."""
    nf = round(len(y) * f * 2) // 2 + 1  # odd number of taps
    edge = np.ones(nf // 2)
    padded = np.concatenate((edge * y[0], y, edge * y[-1]), 0)
    return np.convolve(padded, np.ones(nf) / nf, mode="valid")


def compute_ap(recall, precision):
    """AP by 101-point interpolation of the precision envelope (reference :1109-1139).  Returns (ap, mpre, mrec)."""
    mrec = np.r_[0.0, recall, 1.0]
    envelope = np.maximum.accumulate(np.r_[1.0, precision, 0.0][::-1])[::-1]  # right-to-left running maximum
    grid = np.linspace(0, 1, 101)
    integrate = getattr(np, "trapezoid", None) or np.trapz
    return integrate(np.interp(grid, mrec, envelope), grid), envelope, mrec


def ap_per_class(tp, conf, pred_cls, target_cls, plot=False, on_plot=None, save_dir=None, names=(), eps=1e-16, prefix=""):
    """Per-class AP and the max-F1 operating point (reference :1142-1230); same 12-tuple, plotting not available."""
    if plot:
        raise NotImplementedError("PR-curve plotting is control plane (SURVEY.md section 8: out of scope)")
    order = np.argsort(-conf)
    tp, conf, pred_cls = tp[order], conf[order], pred_cls[order]
    classes, n_labels = np.unique(target_cls, return_counts=True)
    n_cls, n_thr, n_grid = classes.shape[0], tp.shape[1], 1000
    x = np.linspace(0, 1, n_grid)
    ap = np.zeros((n_cls, n_thr))
    p_curve, r_curve = np.zeros((n_cls, n_grid)), np.zeros((n_cls, n_grid))
    for ci, (c, n_l) in enumerate(zip(classes, n_labels)):
        sel = pred_cls == c
        if not sel.any() or n_l == 0:
            continue
        hits = tp[sel].cumsum(0)
        misses = (1 - tp[sel]).cumsum(0)
        recall, precision = hits / (n_l + eps), hits / (hits + misses)
        r_curve[ci] = np.interp(-x, -conf[sel], recall[:, 0], left=0)  # negated: xp must increase
        p_curve[ci] = np.interp(-x, -conf[sel], precision[:, 0], left=1)
        ap[ci] = [compute_ap(recall[:, j], precision[:, j])[0] for j in range(n_thr)]
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    k = smooth(f1_curve.mean(0), 0.1).argmax()
    p, r, f1 = p_curve[:, k], r_curve[:, k], f1_curve[:, k]
    tpn = (r * n_labels).round()
    fpn = (tpn / (p + eps) - tpn).round()
    return tpn, fpn, p, r, f1, ap, classes.astype(int), p_curve, r_curve, f1_curve, x, np.array([])


class ConfusionMatrix:
    """Detection confusion matrix (reference :903-997) counted on the device.  ``matrix[predicted, true]`` with index ``nc`` =
    background, an (nc+1, nc+1) float64 array read back from the int32 device counter on access.  ``process_batch`` takes one image
    (reference :935-986); ``DetectionValidator.update_metrics`` adds a whole batch to the same counter in one launch.  The matching
    rule, its tie order and the reference's ``if n:`` quirk: csrc/confusion.hip, DESIGN.md."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45, task="detect"):
        if task != "detect":
            raise NotImplementedError("ConfusionMatrix: only task='detect' (classification is out of scope, SURVEY.md section 8)")
        self.task, self.nc = task, int(nc)
        self.conf = 0.25 if conf in (None, 0.001) else conf  # the default validation confidence means 0.25 (reference :920)
        self.iou_thres = iou_thres
        self._buf = None  # (nc+1)^2 counters + one status word, int32, on the device that first uses it

    def counter(self, device):
        """The device counter (created and zeroed on first use); ``[-1]`` is the kernel's status word."""
        device = torch.device(device)
        if self._buf is None:
            self._buf = torch.zeros((self.nc + 1) ** 2 + 1, dtype=torch.int32, device=device)
        elif self._buf.device != device:
            raise RuntimeError(f"ConfusionMatrix counts on {self._buf.device}, got tensors on {device}")
        return self._buf

    def zero_(self, device=None):
        if self._buf is not None:
            self._buf.zero_()
        elif device is not None:
            self.counter(device)
        return self

    def launch(self, predn, pred_off, n_preds, t_bidx, t_cls, t_boxes, n_targets, geom, B, imgsz, skip_unlabelled, device):
        """One dy_confusion_matrix launch on the current stream; pointers as ints (0 = NULL).  No synchronisation."""
        buf = self.counter(device)
        check(lib().dy_confusion_matrix(predn, pred_off, n_preds, t_bidx, t_cls, t_boxes, n_targets, geom, B, imgsz[0], imgsz[1], self.nc,
                                        self.conf, self.iou_thres, int(skip_unlabelled), buf.data_ptr(), buf.data_ptr() + 4 * (buf.numel() - 1),
                                        torch.cuda.current_stream(buf.device).cuda_stream), "dy_confusion_matrix")

    def status(self):
        """The kernel's status word (synchronises): bit 0 = an image had more than 1024 labels, bit 1 = a class outside [0, nc)."""
        return 0 if self._buf is None else int(self._buf[-1].item())

    def process_batch(self, detections, gt_bboxes, gt_cls):
        """One image: detections (N,6) x1 y1 x2 y2 conf cls or None, gt_bboxes (M,4) native xyxy, gt_cls (M); CUDA tensors only."""
        if gt_cls.device.type != "cuda" or (detections is not None and detections.device.type != "cuda"):
            raise RuntimeError("ConfusionMatrix.process_batch: HIP path only (no CPU fallback)")
        det = detections.reshape(-1, 6).float().contiguous() if detections is not None else None
        box, cls = gt_bboxes.reshape(-1, 4).float().contiguous(), gt_cls.reshape(-1).float().contiguous()
        nd, nl = (det.shape[0] if det is not None else 0), cls.shape[0]
        self.launch(det.data_ptr() if nd else 0, 0, nd, 0, cls.data_ptr() if nl else 0, box.data_ptr() if nl else 0, nl, 0, 1, (0, 0), False,
                    gt_cls.device)

    @property
    def matrix(self):
        n = self.nc + 1
        if self._buf is None:
            return np.zeros((n, n))
        host = self._buf.cpu().numpy()
        if host[-1] & 1:
            raise RuntimeError("an image carried more than 1024 labels (dy_confusion_matrix capacity)")
        if host[-1] & 2:
            raise RuntimeError(f"a detection or label class lies outside [0, {self.nc}) (dy_confusion_matrix)")
        return host[:-1].reshape(n, n).astype(np.float64)

    def tp_fp(self):
        """True and false positives per class, background dropped (reference :992-997)."""
        m = self.matrix
        tp = m.diagonal()
        return tp[:-1], (m.sum(1) - tp)[:-1]

    def print(self):
        m = self.matrix
        for i in range(self.nc + 1):
            print(" ".join(map(str, m[i])))

    def process_cls_preds(self, preds, targets):
        raise NotImplementedError("ConfusionMatrix: classification is out of scope (SURVEY.md section 8)")

    def plot(self, *args, **kwargs):
        raise NotImplementedError("confusion-matrix plotting is control plane (SURVEY.md section 8: out of scope)")


def _avg(a, empty=0.0):
    return a.mean() if len(a) else empty


class Metric:
    """Per-class results container with the reference's attribute names (reference :1233-1402): ``p, r, f1, all_ap
    (classes x 10 IoU thresholds), ap_class_index, nc`` and the derived ``ap50, ap, mp, mr, map50, map75, map, maps``."""

    def __init__(self):
        self.p, self.r, self.f1, self.all_ap, self.ap_class_index, self.nc = [], [], [], [], [], 0

    def update(self, results):
        self.p, self.r, self.f1, self.all_ap, self.ap_class_index = results[:5]

    def _ap_at(self, col):
        return self.all_ap[:, col] if len(self.all_ap) else []

    ap50 = property(lambda self: self._ap_at(0))
    ap = property(lambda self: self.all_ap.mean(1) if len(self.all_ap) else [])
    mp = property(lambda self: _avg(self.p))
    mr = property(lambda self: _avg(self.r))
    map50 = property(lambda self: _avg(self._ap_at(0)))
    map75 = property(lambda self: _avg(self._ap_at(5)))
    map = property(lambda self: _avg(self.all_ap) if len(self.all_ap) else 0.0)

    @property
    def maps(self):
        out = np.full(self.nc, self.map, dtype=np.float64)
        out[np.asarray(self.ap_class_index, dtype=int)] = self.ap
        return out

    def mean_results(self):
        return [self.mp, self.mr, self.map50, self.map]

    def class_result(self, i):
        return self.p[i], self.r[i], self.ap50[i], self.ap[i]

    def fitness(self):
        mp, mr, m50, m = self.mean_results()
        return 0.1 * m50 + 0.9 * m  # weights [0, 0, 0.1, 0.9] over (P, R, mAP50, mAP50-95)


class DetMetrics:
    """Reference :1405-1480: ``process`` the concatenated statistics, then read ``results_dict`` / ``mean_results``."""
    keys = ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)"]
    task = "detect"

    def __init__(self, save_dir=None, plot=False, on_plot=None, names=()):
        self.save_dir, self.plot, self.on_plot, self.names = save_dir, plot, on_plot, names
        self.box = Metric()
        self.confusion_matrix = None  # the validator's ConfusionMatrix after get_stats (reference val.py:166)
        self.speed = dict.fromkeys(("preprocess", "inference", "loss", "postprocess"), 0.0)

    def process(self, tp, conf, pred_cls, target_cls):
        self.box.nc = len(self.names)
        self.box.update(ap_per_class(tp, conf, pred_cls, target_cls, plot=False, names=self.names)[2:])

    def __getattr__(self, name):  # mean_results / class_result / maps / ap_class_index are the box metric's
        if name in ("mean_results", "class_result", "maps", "ap_class_index"):
            return getattr(self.box, name)
        raise AttributeError(name)

    @property
    def fitness(self):
        return self.box.fitness()

    @property
    def results_dict(self):
        return dict(zip(self.keys + ["fitness"], [*self.box.mean_results(), self.fitness]))


class WiseIouLoss:
    """Configuration of the Wise-IoU box loss (reference utils/metrics.py:567-741): ``ltype``, ``monotonous`` (None = v1, True =
    v2, False = v3), ``inner_iou``, ``focaler_iou`` and the running mean ``iou_mean`` (starts at 1).  Assign it to
    ``criterion.bbox_loss.wiou_loss`` with ``bbox_loss.use_wiseiou = True``; the loss itself runs in the criterion's HIP kernels
    (``dy_detection_loss``), so the object is not called on tensors."""
    momentum = 1e-2
    alpha = 1.7
    delta = 2.7
    LTYPES = ("IoU", "WIoU", "EIoU", "GIoU", "DIoU", "CIoU", "SIoU", "ShapeIoU", "PIoU", "PIoU2", "MPDIoU")

    def __init__(self, ltype="WIoU", monotonous=False, inner_iou=False, focaler_iou=False):
        assert ltype in self.LTYPES, f"The loss function {ltype} does not exist"
        self.ltype = ltype
        self.monotonous = monotonous
        self.inner_iou = inner_iou
        self.focaler_iou = focaler_iou
        self._s = None  # the criterion's scalar block once assigned to bbox_loss.wiou_loss (utils/loss.py BboxLoss)
        self._mean = torch.tensor(1.0)
        self.training = True

    @property
    def iou_mean(self):
        """The running mean of the IoU term: the criterion's device scalar once assigned, else this object's own value."""
        return self._s[4] if self._s is not None else self._mean

    @iou_mean.setter
    def iou_mean(self, v):
        if self._s is not None:
            self._s[4] = float(v)
        else:
            self._mean = torch.tensor(float(v))

    def __call__(self, *args, **kwargs):
        raise NotImplementedError("WiseIouLoss runs inside the detection criterion's HIP kernels: assign it to "
                                  "v8DetectionLoss.bbox_loss.wiou_loss and call the criterion")

    forward = __call__

    def __repr__(self):
        return f"{self.ltype}(iou_mean={float(self.iou_mean):.3f})"

    __name__ = property(lambda self: self.ltype)
