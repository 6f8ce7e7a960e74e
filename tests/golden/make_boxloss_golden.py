"""Generate tests/golden/boxloss_{0,1,2}.npz: the REFERENCE's box-loss menu (utils/loss.py:199-217, utils/metrics.py:75-741) on the loss
fixtures' inputs, and three of its modes through a whole DEAL-YOLO-N training step.

Run in the build container only (needs the reference tree, which ``_refimport`` locates):

    python tests/golden/make_boxloss_golden.py

Criterion part -- make_golden.py::gen_loss's recipe: ``_FakeModel(6, [4, 8, 16])``, the targets of ``cases.loss_cases()``, feature
seeds ``400 + 10 * case_index + level``.  A mode (``boxloss_modes.py``) is selected as a user of the reference does: ``BboxLoss.forward``
is replaced by ``_forward`` below, which is the reference's own body (utils/loss.py:202-233) with the call of the chosen line --
``self.wiou_loss(..., **kwargs)`` (a reference ``WiseIouLoss`` assigned to ``bbox_loss.wiou_loss``, kwargs as at :208-209) or the
reference's ``bbox_iou`` / ``bbox_inner_iou`` / ``bbox_focaler_iou`` / ``bbox_*mpdiou`` with the chosen flag.
Per ``<case>/<mode>[/call<k>]``: ``loss``, ``items``, ``iou_mean`` (Wise modes); per ``<case>/<mode>`` for the LAST call: ``gbox``, the
box-logit gradient rows (nfg, 64) at the foreground anchors (loss.npz's ``fg_mask``, level-major, row-major), float32.

StepPlan part: the reference DEAL-YOLO-N (yolov8n-ASF-P2P2) with ``oracle.graph.fill_state(layout, 7)``, train mode, models.npz's
batch of that model; per ``step/<mode>``: ``loss``, ``items``, ``grad_names``, ``grad_l2``.

The arrays of mode i of ``modes`` (``boxloss_modes.boxloss_modes()`` order) are in shard i % 3; ``modes`` and ``step/`` in shard 0.
"""
import os
import sys
import types
import warnings

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

os.environ["MKL_CBWR"] = "COMPATIBLE"  # as tests/conftest.py pins it

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _refimport  # noqa: E402

_refimport.install()

from ultralytics.cfg import get_cfg  # noqa: E402
from ultralytics.nn.tasks import DetectionModel  # noqa: E402
from ultralytics.utils import DEFAULT_CFG  # noqa: E402
from ultralytics.utils import metrics as rm  # noqa: E402
from ultralytics.utils.loss import v8DetectionLoss  # noqa: E402
from ultralytics.utils.tal import bbox2dist  # noqa: E402

from boxloss_modes import STEP_MODES, boxloss_modes, cases_of, n_calls, step_spec  # noqa: E402
from cases import loss_cases, rnd  # noqa: E402
from make_golden import _FakeModel  # noqa: E402
from oracle import graph as og  # noqa: E402

CFG_DIR = os.path.join(_refimport.REF, "ultralytics/cfg/models")
torch.set_num_threads(8)
NSHARD = 3
FLAG = {"GIoU": "GIoU", "DIoU": "DIoU", "CIoU": "CIoU", "EIoU": "EIoU", "SIoU": "SIoU", "ShapeIoU": "ShapeIoU", "PIoU": "PIoU", "PIoU2": "PIoU2"}


def _forward(spec):
    """BboxLoss.forward (reference utils/loss.py:202-233) with the box-loss line of ``spec``."""
    ratio, d, u, scale = 0.7, spec.get("d", 0.0), spec.get("u", 0.95), spec.get("scale", 0.0)

    def forward(self, pred_dist, pred_bboxes, anchor_points, target_bboxes, target_scores, target_scores_sum, fg_mask, mpdiou_hw=None):
        weight = target_scores.sum(-1)[fg_mask].unsqueeze(-1)
        p, t = pred_bboxes[fg_mask], target_bboxes[fg_mask]
        if spec["wise"]:
            kw = {"scale": scale} if spec["ltype"] == "ShapeIoU" else ({"mpdiou_hw": mpdiou_hw[fg_mask]} if spec["ltype"] == "MPDIoU" else {})
            wiou = self.wiou_loss(p, t, ret_iou=False, ratio=ratio, d=d, u=u, **kw).unsqueeze(-1)
            loss_iou = (wiou * weight).sum() / target_scores_sum
        else:
            v, lt = spec["variant"], spec["ltype"]
            if lt == "MPDIoU":
                hw = mpdiou_hw[fg_mask]
                iou = (rm.bbox_mpdiou(p, t, xywh=False, mpdiou_hw=hw) if v is None else
                       rm.bbox_inner_mpdiou(p, t, xywh=False, mpdiou_hw=hw, ratio=ratio) if v == "inner" else
                       rm.bbox_focaler_mpdiou(p, t, xywh=False, mpdiou_hw=hw, d=d, u=u))
            else:
                flags = {FLAG[lt]: True} if lt in FLAG else {}
                if lt == "ShapeIoU":
                    flags["scale"] = scale
                iou = (rm.bbox_iou(p, t, xywh=False, **flags) if v is None else
                       rm.bbox_inner_iou(p, t, xywh=False, ratio=ratio, **flags) if v == "inner" else
                       rm.bbox_focaler_iou(p, t, xywh=False, d=d, u=u, **flags))
            loss_iou = ((1.0 - iou) * weight).sum() / target_scores_sum
        if self.nwd_loss:
            nwd = rm.wasserstein_loss(p, t)
            nwd_loss = ((1.0 - nwd) * weight).sum() / target_scores_sum
            loss_iou = self.iou_ratio * loss_iou + (1 - self.iou_ratio) * nwd_loss
        target_ltrb = bbox2dist(anchor_points, target_bboxes, self.reg_max)
        loss_dfl = self._df_loss(pred_dist[fg_mask].view(-1, self.reg_max + 1), target_ltrb[fg_mask]) * weight
        loss_dfl = loss_dfl.sum() / target_scores_sum
        return loss_iou, loss_dfl

    return forward


def select(crit, spec):
    bl = crit.bbox_loss
    bl.use_wiseiou, bl.nwd_loss = spec["wise"], spec["nwd"]
    if spec["wise"]:
        bl.wiou_loss = rm.WiseIouLoss(ltype=spec["ltype"], monotonous=spec["mono"], inner_iou=spec["variant"] == "inner",
                                      focaler_iou=spec["variant"] == "focaler")
    bl.forward = types.MethodType(_forward(spec), bl)


def gen_criterion(arrs):
    shapes = [(16, 16), (8, 8), (4, 4)]
    L = np.load(os.path.join(HERE, "loss.npz"))
    modes = boxloss_modes()
    for ci, (case, tg) in enumerate(loss_cases().items()):
        fg = torch.from_numpy(L[f"{case}/fg_mask"]).bool()
        for mode, spec in modes.items():
            if case not in cases_of(mode):
                continue
            crit = v8DetectionLoss(_FakeModel(6, [4.0, 8.0, 16.0]))
            select(crit, spec)
            feats = [rnd(400 + 10 * ci + l, 2, 70, *s, scale=1.5).requires_grad_(True) for l, s in enumerate(shapes)]
            for call in range(n_calls(spec, case)):
                for f in feats:
                    f.grad = None
                loss, items = crit([f for f in feats], dict(tg))
                loss.backward()
                tag = f"{case}/{mode}" + (f"/call{call}" if n_calls(spec, case) > 1 else "")
                arrs[f"{tag}/loss"], arrs[f"{tag}/items"] = loss.detach().numpy(), items.numpy()
                if spec["wise"]:
                    arrs[f"{tag}/iou_mean"] = crit.bbox_loss.wiou_loss.iou_mean.clone().numpy()
            g = torch.cat([(f.grad if f.grad is not None else torch.zeros_like(f))[:, :64].flatten(2).transpose(1, 2) for f in feats], 1)
            arrs[f"{case}/{mode}/gbox"] = g[fg].numpy().astype(np.float32)
            assert all(np.isfinite(v).all() for k, v in arrs.items() if k.startswith(f"{case}/{mode}")), (case, mode)
        print(case, "done")
    arrs["modes"] = np.array(list(modes))


def gen_step(arrs):
    name = "yolov8n-ASF-P2P2"
    M = np.load(os.path.join(HERE, "models.npz"))
    batch = {k: torch.from_numpy(M[f"{name}/{k}"]) for k in ("img", "batch_idx", "cls", "bboxes")}
    cfg = os.path.join(CFG_DIR, name + ".yaml")
    torch.manual_seed(0)
    m = DetectionModel(cfg, ch=3, verbose=False)
    m.args = get_cfg(DEFAULT_CFG)
    g = og.build_graph(og.load_yaml(cfg))
    sd = og.fill_state(og.state_layout(g), 7)
    for mode in STEP_MODES:
        m.load_state_dict(sd, strict=True)
        m.train()
        m.zero_grad()
        if hasattr(m, "criterion"):
            del m.criterion
        m.criterion = m.init_criterion()
        select(m.criterion, step_spec(mode))
        loss, items = m(batch)
        loss.backward()
        gn = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
        arrs[f"step/{mode}/loss"] = loss.detach().numpy()
        arrs[f"step/{mode}/items"] = items.numpy()
        arrs[f"step/{mode}/grad_names"] = np.array(list(gn))
        arrs[f"step/{mode}/grad_l2"] = torch.stack([v.norm() for v in gn.values()]).numpy()
        print("step", mode, float(loss), items.tolist())


def main():
    arrs = {}
    gen_criterion(arrs)
    gen_step(arrs)
    # three shards (a committed file stays under 1 MiB): mode i lives in boxloss_<i % 3>.npz; 'modes' and 'step/' in shard 0
    modes = list(arrs["modes"])
    shards = [{} for _ in range(NSHARD)]
    for k, v in arrs.items():
        parts = k.split("/")
        shards[modes.index(parts[1]) % NSHARD if len(parts) > 2 and parts[0] != "step" else 0][k] = v
    for i, sh in enumerate(shards):
        path = os.path.join(HERE, f"boxloss_{i}.npz")
        np.savez_compressed(path, **sh)
        print(f"boxloss_{i}.npz  {os.path.getsize(path) / 1024:.1f} KiB  ({len(sh)} arrays)")


if __name__ == "__main__":
    main()
