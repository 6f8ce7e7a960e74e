"""Device / seeding / EMA helpers (drop-in for the pieces of reference utils/torch_utils.py used by the entry scripts)."""
from __future__ import annotations

import math
import os
import random
from copy import deepcopy

import numpy as np
import torch


def select_device(device="", batch=0, newline=False, verbose=True):
    """'0' / 'cuda:0' / 0 -> torch.device; CPU requests raise because the hot path is GPU-only."""
    if isinstance(device, torch.device):
        return device
    d = "" if device is None else str(device).lower().replace("cuda:", "").strip()
    if d in ("cpu", "mps"):
        raise ValueError("the MI355X DEAL-YOLO path runs on GPUs only (device='cpu' is served by the reference implementation)")
    ids = [int(x) for x in d.split(",") if x != ""] or [0]
    if len(ids) > 1 and "LOCAL_RANK" not in os.environ:
        raise ValueError(f"device='{device}' lists {len(ids)} GPUs but this process is not a rank of a distributed launch: "
                         "YOLO.train(device='0,1,...') re-launches itself under torch.distributed.run; other entry points take one GPU")
    if not torch.cuda.is_available():
        raise ValueError(f"Invalid device '{device}' requested: no GPU visible")
    if "LOCAL_RANK" in os.environ:  # one rank per GPU under torch.distributed.run: the launcher narrowed the visible devices
        return torch.device("cuda", 0 if os.environ.get("DY_REHEARSE_ON_ONE_GPU") == "1" else int(os.environ["LOCAL_RANK"]))
    return torch.device("cuda", ids[0])


def init_seeds(seed=0, deterministic=False):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def de_parallel(model):
    return model.module if hasattr(model, "module") else model


class ModelEMA:
    """Exponential moving average of parameters and float buffers (reference utils/torch_utils.py:431-464).  The averages
    live in the StepPlan's flat device buffers and are updated inside the optimizer kernel; ``.ema`` materialises a model
    carrying them (for validation / checkpoints)."""

    def __init__(self, plan, decay=0.9999, tau=2000, updates=0):
        self.plan, self.decay0, self.tau = plan, decay, tau
        self.enabled = True
        self._eval = None  # eval_model(): built once per run

    @property
    def updates(self):
        return self.plan.ema_updates

    def decay(self, x):
        return self.decay0 * (1 - math.exp(-x / self.tau))

    def state_dict(self):
        """EMA values under the model's state_dict keys (parameters and float buffers; integer buffers are copied)."""
        plan, rt = self.plan, self.plan.rt
        out = {}
        params = dict(plan.model.named_parameters())
        fb_off, o = {}, 0
        for mname, mod in plan.model.named_modules():
            for bname, b in mod.named_buffers(recurse=False):
                if b is not None and b.dtype.is_floating_point:
                    fb_off[f"{mname}.{bname}" if mname else bname] = (o, b.numel())
                    o += (b.numel() + 7) // 8 * 8
        for k, v in plan.model.state_dict().items():
            if k in params:
                off = rt.param_off[k]
                out[k] = plan.ema[off:off + v.numel()].view(v.shape).clone()
            elif k in fb_off:
                off, n = fb_off[k]
                out[k] = plan.ema_b[off:off + n].view(v.shape).clone()
            else:
                out[k] = v.clone()
        return out

    @property
    def ema(self):
        """A fresh eval-mode model carrying the averaged weights."""
        from ..nn.tasks import DetectionModel
        m = DetectionModel(deepcopy(self.plan.model.yaml), verbose=False)
        m.load_state_dict({k: v.cpu() for k, v in self.state_dict().items()}, strict=True)
        return m.eval()

    def eval_model(self):
        """The run's ONE evaluation model, refreshed from the flat EMA buffers on the device (per-epoch validation,
        reference engine/trainer.py:844-859 validates ``ema.ema``).  A model built from the same YAML flattens its parameters and
        float buffers in the same order as the trained one (``Runtime._flatten``), so a refresh is two device copies and
        ``mark_dirty()``: no host round trip, no ``load_state_dict``.  Its Runtime, packed-weight storage and recorded InferPlans
        survive from epoch to epoch; only the packing pass reruns.  Carries ``names`` / ``nc`` / ``args`` / ``stride`` (reference
        ``ema.update_attr``) and a criterion of its own (own result scalars and running WIoU mean; the box-loss modes are the
        training criterion's), so a validation never touches the training criterion's state."""
        plan, rt = self.plan, self.plan.rt
        src = plan.model
        m = self._eval
        if m is None:
            from ..nn.tasks import DetectionModel
            dev = rt.eng.device
            with torch.random.fork_rng(devices=[dev]):  # the constructor draws initial weights: the training run's RNG streams stay where they were
                m = DetectionModel(deepcopy(src.yaml), verbose=False)
            m.to(dev).eval()
            ert = m._runtime(dev)
            if ert.layout() != rt.layout():
                raise RuntimeError("ModelEMA.eval_model: a model built from the plan's YAML does not lay its parameters and buffers out like "
                                   "the trained one (was the trained model modified after construction?)")
            if ert.flat_p.numel() != plan.ema.numel() or ert.flat_b.numel() != plan.ema_b.numel():
                raise RuntimeError("ModelEMA.eval_model: flat buffer sizes differ from the EMA buffers'")
            self._eval = m
        ert = m._runtime(rt.eng.device)
        ert.flat_p.copy_(plan.ema)
        ert.flat_b.copy_(plan.ema_b)
        for (_, b), (_, e) in zip(src.named_buffers(), m.named_buffers()):  # integer buffers (num_batches_tracked, ...) are copied
            if not b.dtype.is_floating_point:
                e.copy_(b)
        ert.mark_dirty()
        for k in ("names", "args"):
            if hasattr(src, k):
                setattr(m, k, getattr(src, k))
        m.nc = getattr(src, "nc", src.model[-1].nc)
        if "criterion" not in m.__dict__:
            crit, bl = m.init_criterion(), plan.crit.bbox_loss
            eb = crit.bbox_loss
            eb.use_wiseiou, eb.nwd_loss, eb.iou_ratio = bl.use_wiseiou, bl.nwd_loss, bl.iou_ratio
            eb.configure_from_cfg(getattr(src, "args", None))
            for k in ("iou_type", "iou_variant", "inner_ratio", "focaler_d", "focaler_u", "shape_scale", "piou_lambda"):
                setattr(eb, k, getattr(bl, k))
            m.criterion = crit
        return m.eval()


class EarlyStopping:
    """Stops a run when the fitness has not improved for ``patience`` epochs (semantics of reference utils/torch_utils.py:568-610):
    an equal fitness counts as an improvement (``>=``: the early zero-fitness epochs move ``best_epoch`` along), ``possible_stop``
    announces that the next epoch may stop, ``patience=0`` never stops, ``fitness=None`` (an epoch without a validation yet) changes
    nothing."""

    def __init__(self, patience=50):
        self.best_fitness, self.best_epoch = 0.0, 0
        self.patience = patience or float("inf")
        self.possible_stop = False

    def __call__(self, epoch, fitness):
        if fitness is None:
            return False
        if fitness >= self.best_fitness:
            self.best_epoch, self.best_fitness = epoch, fitness
        since = epoch - self.best_epoch
        self.possible_stop = since >= self.patience - 1
        if since >= self.patience:
            from . import LOGGER
            LOGGER.info(f"Stopping training early: no improvement in the last {self.patience} epochs; best results at epoch "
                        f"{self.best_epoch}, saved as best.pt (patience=0 disables early stopping)")
            return True
        return False
