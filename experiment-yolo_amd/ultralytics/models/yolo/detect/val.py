"""DetectionValidator with the reference's method names (reference models/yolo/detect/val.py, engine/validator.py).

``update_metrics`` handles a whole batch with ONE launch of dy_match_predictions (label/prediction rescaling, IoU, greedy
matching at the ten IoU thresholds); the statistics stay on the device until ``get_stats``.  With ``args.plots`` (the reference's
gate, val.py:136) one launch of dy_confusion_matrix per batch adds the batch to ``confusion_matrix`` from the same native-space
predictions.  Dataset construction, JSON / txt dumps and plots are control plane or data pipeline."""
import ctypes as C

import numpy as np
import torch

from ....hip import check, lib
from ....utils import LOGGER, ops
from ....utils.metrics import ConfusionMatrix, DetMetrics
from ....hip.engine import dev_empty


class DetectionValidator:
    def __init__(self, dataloader=None, save_dir=None, pbar=None, args=None, _callbacks=None):
        from ....cfg import get_cfg
        self.args = get_cfg(overrides=args if isinstance(args, dict) else None) if not hasattr(args, "conf") else args
        self.dataloader = dataloader
        self.device = None
        self.nc, self.names, self.seen = 0, {}, 0
        self.iouv = torch.linspace(0.5, 0.95, 10)  # mAP@0.5:0.95 thresholds (reference val.py:37)
        self.niou = self.iouv.numel()
        self.metrics = DetMetrics()
        self.confusion_matrix = None
        self.stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[])
        self.training = False
        self.loss = None        # training mode: sum of the per-batch loss items (box, cls, dfl)
        self.plots_gate = None  # training mode: the reference's ``args.plots &= possible_stop or final epoch`` (validator.py:118), args untouched

    # ---- reference validator hooks -------------------------------------------------------------------------------
    def init_metrics(self, model):
        names = getattr(model, "names", None) or {i: str(i) for i in range(model.model[-1].nc)}
        self.names = dict(enumerate(names)) if isinstance(names, (list, tuple)) else names
        self.nc = len(self.names)
        self.metrics.names = self.names
        self.seen = 0
        self.stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[])
        self.confusion_matrix = ConfusionMatrix(nc=self.nc, conf=self.args.conf).zero_(self.device)  # reference val.py:75

    def preprocess(self, batch):
        dev = self.device
        img = batch["img"].to(dev, non_blocking=True)
        if img.dtype == torch.uint8 and img.shape[-1] == 3 and img.shape[1] != 3:  # the loader's NHWC layout
            img = img.permute(0, 3, 1, 2)
        batch["img"] = img.float() / 255 if img.dtype == torch.uint8 else img.float()
        for k in ("batch_idx", "cls", "bboxes"):
            batch[k] = batch[k].to(dev)
        return batch

    def postprocess(self, preds):
        a = self.args
        conf = 0.001 if a.conf is None else a.conf  # reference engine/validator.py: default validation confidence
        return ops.non_max_suppression(preds, conf, a.iou, multi_label=True, agnostic=bool(a.single_cls), max_det=a.max_det)

    @staticmethod
    def _geometry(batch, B, imgsz):
        """(B,5) gain, padw, padh, ori_h, ori_w: what scale_boxes derives from ori_shape / ratio_pad (utils/ops.py)."""
        g = np.zeros((B, 5), np.float32)
        oris, rps = batch.get("ori_shape"), batch.get("ratio_pad")
        for i in range(B):
            oh, ow = (oris[i] if oris is not None else imgsz)
            rp = rps[i] if rps is not None else None
            if rp is None:
                gain = min(imgsz[0] / oh, imgsz[1] / ow)
                pad = (round((imgsz[1] - ow * gain) / 2 - 0.1), round((imgsz[0] - oh * gain) / 2 - 0.1))
            else:
                gain, pad = rp[0][0], rp[1]
            g[i] = (gain, pad[0], pad[1], oh, ow)
        return g

    def update_metrics(self, preds, batch):
        """preds: the NMS output list; batch: img / batch_idx / cls / bboxes (+ ori_shape, ratio_pad when letterboxed)."""
        dev = preds[0].device if len(preds) else batch["cls"].device
        B = len(preds)
        imgsz = tuple(batch["img"].shape[2:])
        counts = [int(p.shape[0]) for p in preds]
        off = np.zeros(B + 1, np.int32)
        off[1:] = np.cumsum(counts)
        ntot = int(off[-1])
        packed = torch.cat([p.reshape(-1, 6).float() for p in preds], 0).contiguous() if ntot else torch.zeros((0, 6), device=dev)
        tcls = batch["cls"].reshape(-1).float().contiguous()
        tidx = batch["batch_idx"].reshape(-1).float().contiguous()
        tbox = batch["bboxes"].reshape(-1, 4).float().contiguous()
        tp = torch.zeros((ntot, self.niou), dtype=torch.uint8, device=dev)
        predn = dev_empty((ntot, 6), torch.float32, dev)
        ntgt = tcls.numel()
        plots = self.args.plots if self.plots_gate is None else self.plots_gate
        confusion = bool(plots and self.nc >= 1 and (ntot or ntgt))  # reference val.py:136; nothing to count in an empty batch
        if ntot or confusion:
            geom = torch.from_numpy(self._geometry(batch, B, imgsz)).to(dev)
            offd = torch.from_numpy(off).to(dev)
        if ntot:
            if getattr(self, "_status", None) is None or self._status.device != dev:
                self._status = torch.zeros(1, dtype=torch.int32, device=dev)  # ONE word for the whole run: every batch ORs into it
            status = self._status
            iouv = self.iouv.to(dev)
            check(lib().dy_match_predictions(packed.data_ptr(), offd.data_ptr(), tidx.data_ptr(), tcls.data_ptr(), tbox.data_ptr(),
                                             tcls.numel(), geom.data_ptr(), iouv.data_ptr(), self.niou, B, imgsz[0], imgsz[1],
                                             tp.data_ptr(), predn.data_ptr(), status.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream), "dy_match_predictions")
        if confusion:  # labelled images only (val.py:131-152 never hands an unlabelled one over); no synchronisation
            if self.confusion_matrix is None or self.confusion_matrix.nc != self.nc:
                self.confusion_matrix = ConfusionMatrix(nc=self.nc, conf=self.args.conf)
            self.confusion_matrix.launch(predn.data_ptr() if ntot else 0, offd.data_ptr(), ntot, tidx.data_ptr() if ntgt else 0,
                                         tcls.data_ptr() if ntgt else 0, tbox.data_ptr() if ntgt else 0, ntgt, geom.data_ptr(), B, imgsz, True, dev)
        self.seen += B
        # images with neither predictions nor labels contribute nothing; label-only images contribute their target classes
        self.stats["tp"].append(tp.bool())
        self.stats["conf"].append(predn[:, 4])
        self.stats["pred_cls"].append(predn[:, 5])
        self.stats["target_cls"].append(tcls)
        self.last_predn = predn
        return tp

    def get_stats(self):
        if getattr(self, "_status", None) is not None and int(self._status.item()) & 1:
            self._status.zero_()
            raise RuntimeError("an image carried more than 1024 labels (dy_match_predictions capacity)")
        if self.confusion_matrix is not None and self.confusion_matrix.status() & 1:
            raise RuntimeError("an image carried more than 1024 labels (dy_confusion_matrix capacity)")
        stats = {k: torch.cat(v, 0).cpu().numpy() for k, v in self.stats.items() if len(v)}
        if len(stats) and stats["tp"].any():
            self.metrics.process(**stats)
        self.nt_per_class = np.bincount(stats["target_cls"].astype(int), minlength=self.nc) if len(stats) else np.zeros(self.nc, int)
        self.metrics.confusion_matrix = self.confusion_matrix  # reference val.py:166
        return self.metrics.results_dict

    def print_results(self):
        mp, mr, m50, m = self.metrics.mean_results()
        LOGGER.info(("%22s" + "%11i" * 2 + "%11.3g" * 4) % ("all", self.seen, int(self.nt_per_class.sum()), mp, mr, m50, m))

    # ---- driver (reference engine/validator.py:104-216, inference part) -------------------------------------------
    @torch.no_grad()
    def __call__(self, trainer=None, model=None):
        """``validator(model=m)`` / ``validator(trainer=t, model=m)``: one validation of ``m`` (never TTA with a trainer).
        ``validator(trainer=t)``: the reference's training mode (engine/validator.py:108-118, 180-181, 199-201) -- the trainer's
        persistent EMA evaluation model, the validation loss summed per batch from the forward's own logits, the confusion matrix only on
        the final epoch or when early stopping may strike; returns metrics + ``val/*_loss`` rounded to 5 decimals."""
        from ....utils.torch_utils import select_device
        self.training = trainer is not None and model is None
        if self.training:
            model = trainer.ema.eval_model()
            self.device = trainer.device
            self.loss = torch.zeros(3, dtype=torch.float32, device=self.device)
            self.plots_gate = bool(self.args.plots) and bool(trainer.stopper.possible_stop or trainer.epoch == trainer.args.epochs - 1)
            model.eval()
        else:
            self.plots_gate = None
            self.device = next(model.parameters()).device if next(model.parameters()).is_cuda else select_device("0")
            if next(model.parameters()).device != self.device:  # (.to() on a model already there would only drop its runtime and plans)
                model.to(self.device)
            model.eval()
        self.init_metrics(model)
        augment = bool(self.args.augment) and trainer is None  # engine/validator.py:109: never while training
        for batch in self.dataloader:
            batch = self.preprocess(batch)
            if self.training:
                preds = model(batch["img"], logits=True)  # the Detect tail writes its fp32 logits beside y: model.loss has nothing to launch for them
                self.loss += model.loss(batch, preds)[1]
            else:
                preds = model(batch["img"], augment=augment)
            self.update_metrics(self.postprocess(preds), batch)
        stats = self.get_stats()
        self.print_results()
        if self.training:
            results = {**stats, **trainer.label_loss_items(self.loss.cpu() / len(self.dataloader), prefix="val")}
            return {k: round(float(v), 5) for k, v in results.items()}
        return stats
