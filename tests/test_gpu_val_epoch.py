"""-m gpu: validating every epoch (cfg ``val_period >= 1``; reference engine/trainer.py:844-923, 963-973, 1038-1048).

What is pinned: the persistent evaluation model ``ModelEMA.eval_model()`` carries exactly the EMA state, is the same object with the
same recorded InferPlans from refresh to refresh and computes what a fresh ``ema.ema`` computes; the validator's training-mode loss
is, bit for bit, the mean of ``model.loss(batch, model(img))[1]`` with the logits materialised the old way, and leaves the training
criterion's scalars alone; the loop writes results.csv / last.pt / best.pt / epoch{N}.pt by the reference's rules, stops on
``patience``, resumes, and does not disturb the training it runs beside."""
import os

import numpy as np
import pytest
import torch

from conftest import CFG_DIR
from golden.cases import write_dataset

pytestmark = pytest.mark.gpu

ZERO = dict(mosaic=0.0, mixup=0.0, copy_paste=0.0, hsv_h=0.0, hsv_s=0.0, hsv_v=0.0, degrees=0.0, translate=0.0, scale=0.0, shear=0.0,
            perspective=0.0, flipud=0.0, fliplr=0.0)
KW = dict(batch=4, imgsz=64, optimizer="SGD", workers=2, amp=False, seed=0, deterministic=True, close_mosaic=0, **ZERO)
COLS = ["epoch", "train/box_loss", "train/cls_loss", "train/dfl_loss", "metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)",
        "metrics/mAP50-95(B)", "val/box_loss", "val/cls_loss", "val/dfl_loss", "lr/pg0", "lr/pg1", "lr/pg2"]
MODEL = os.path.join(CFG_DIR, "yolov8n-ASF-P2P2.yaml")


@pytest.fixture(scope="module")
def data_yaml(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("val_epoch") / "ds")
    write_dataset(root)
    return os.path.join(root, "data.yaml")


@pytest.fixture(scope="module")
def trained(data_yaml):
    """One epoch (three optimizer steps at nbs=4) of the tiny model, no validation: the state the model / loss tests look at."""
    from ultralytics import YOLO
    torch.manual_seed(0)
    y = YOLO(MODEL)
    y.train(data=data_yaml, epochs=1, val=False, nbs=4, **KW)
    return y.trainer


def _read_csv(path):
    lines = open(path).read().splitlines()
    return [c.strip() for c in lines[0].split(",")], np.loadtxt(path, delimiter=",", skiprows=1, ndmin=2)


def test_eval_model_is_persistent_and_carries_the_ema(trained):
    tr, ema = trained, trained.ema
    assert tr.plan.ema_updates >= 3
    m = ema.eval_model()
    want, got = ema.state_dict(), m.state_dict()
    assert list(want) == list(got)
    assert all(torch.equal(want[k], got[k]) and want[k].dtype == got[k].dtype for k in want), "eval_model() != ModelEMA.state_dict()"
    assert not m.training and m.names == tr.model.names and m.args is tr.model.args and m.nc == tr.model.model[-1].nc == 4
    assert torch.equal(m.stride.cpu(), tr.model.stride.cpu())
    assert m.criterion is not tr.plan.crit and m.criterion.scalars.data_ptr() != tr.plan.crit.scalars.data_ptr()
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(1)).cuda()
    fresh = ema.ema.cuda().eval()
    with torch.no_grad():
        y_fresh = fresh(x)[0]
        y1 = m(x)[0]
        y2 = m(x)[0]  # second sight of the geometry: recorded
    assert torch.equal(y1, y_fresh) and torch.equal(y2, y_fresh)
    rt, plans = m.rt, dict(m._infer_plans["plans"])
    assert plans
    # a refresh without a change: same object, same runtime, same plans, same output
    m2 = ema.eval_model()
    assert m2 is m and m2.rt is rt and m2._infer_plans["plans"] == plans and all(m2._infer_plans["plans"][k] is plans[k] for k in plans)
    with torch.no_grad():
        assert torch.equal(m2(x)[0], y1)
    # the EMA moves (more optimizer steps): the next refresh carries it, through the same plans
    before = tr.plan.ema.clone()
    for i, batch in enumerate(tr.train_loader):
        tr.train_step(batch, tr.nb + i, 0)
    torch.cuda.synchronize()
    assert not torch.equal(tr.plan.ema, before)
    with torch.no_grad():
        assert torch.equal(m(x)[0], y1)  # not refreshed yet: still the old weights
        m3 = ema.eval_model()
        y3 = m3(x)[0]
    assert m3 is m and m3.rt is rt and all(m3._infer_plans["plans"][k] is plans[k] for k in plans)
    assert not torch.equal(y3, y1)
    with torch.no_grad():
        assert torch.equal(y3, ema.ema.cuda().eval()(x)[0])
    got, want = m3.state_dict(), ema.state_dict()
    assert all(torch.equal(want[k], got[k]) for k in want)


def test_validation_loss_is_the_materialised_loss_bit_for_bit(trained, monkeypatch):
    from ultralytics.models.yolo.detect import DetectionValidator
    from ultralytics.nn.modules import head
    tr = trained
    tr.args.epochs = 1  # (the plots gate reads epoch / epochs)
    tr._begin_val_loop()
    vloader = tr.get_dataloader(tr.data["val"], 4, 0, "val", tr.data)
    v = DetectionValidator(dataloader=vloader, args=tr.args)
    scal = tr.plan.crit.scalars.clone()
    assert head.HEAD_INFER_LOGITS
    res = v(trainer=tr)
    fused = v.loss.clone()
    torch.cuda.synchronize()
    assert torch.equal(tr.plan.crit.scalars, scal), "a validation pass touched the training criterion's scalars"
    assert set(res) == {"metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)", "fitness", "val/box_loss",
                        "val/cls_loss", "val/dfl_loss"}
    # the old way: the plain fused tail, then materialize() (two eager conv launches per level) inside model.loss
    monkeypatch.setattr(head, "HEAD_INFER_LOGITS", False)
    m = tr.ema.eval_model()
    total, n = torch.zeros(3, device="cuda"), 0
    with torch.no_grad():
        for batch in vloader:
            batch = v.preprocess(batch)
            preds = m(batch["img"])
            assert not preds[1]._ho.logits_current
            total += m.loss(batch, preds)[1]
            n += 1
    assert n == len(vloader) and n >= 2
    print("validation loss sums, fused logits / materialised:", fused.tolist(), total.tolist())
    assert torch.equal(fused, total)
    mean = total.cpu() / n
    assert [res[k] for k in ("val/box_loss", "val/cls_loss", "val/dfl_loss")] == [round(float(x), 5) for x in mean]
    assert all(np.isfinite(list(res.values()))) and res["val/box_loss"] > 0
    # and the switch itself: the validator with DY_HEAD_INFER_LOGITS=0 in effect gives the same numbers through materialize()
    res0 = v(trainer=tr)
    assert torch.equal(v.loss, fused) and res0 == res


def _trainer_class(stub=None):
    from ultralytics.engine.trainer import DetectionTrainer

    class Recording(DetectionTrainer):
        """Keeps every validation's fitness and the best_fitness the loop started from; ``stub``: a scripted fitness list replaces the
        validator's (the validation itself still runs)."""
        fits, started_with = None, None

        def _begin_val_loop(self):
            super()._begin_val_loop()
            type(self).started_with, type(self).fits = self.best_fitness, []

        def validate(self):
            if stub is not None:
                real = self.validator

                def scripted(trainer=None, model=None):
                    return dict(real(trainer=trainer, model=model), fitness=stub[trainer.epoch])
                self.validator = scripted
                try:
                    out = super().validate()
                finally:
                    self.validator = real
            else:
                out = super().validate()
            self.fits.append(out[1])
            return out
    return Recording


def _best_epoch(fits):
    best, at = None, None
    for e, f in enumerate(fits):
        if not best or best < f:  # the reference's rule (engine/trainer.py:971): equal fitness does not replace the best
            best, at = f, e
    return best, at


def test_loop_writes_results_checkpoints_and_resumes(data_yaml, tmp_path):
    from ultralytics import YOLO
    T = _trainer_class()
    kw = dict(KW, project=str(tmp_path), name="run", val_period=1, save_period=1, patience=0)
    torch.manual_seed(0)
    y = YOLO(MODEL)
    hist = y.train(trainer=T, data=data_yaml, epochs=3, **kw)
    tr, run = y.trainer, tmp_path / "run"
    assert len(hist) == 3 and len(T.fits) == 3 and T.started_with is None
    head, rows = _read_csv(run / "results.csv")
    assert head == COLS and rows.shape == (3, 14) and rows[:, 0].tolist() == [1, 2, 3] and np.isfinite(rows).all()
    assert [list(r) for r in tr.results] == [COLS] * 3
    assert np.all(rows[:, 8:11] > 0) and np.all(rows[:, 11:] > 0)
    np.testing.assert_allclose(rows[:, 1:4], np.asarray(hist, dtype=np.float64), rtol=1e-4)  # the training columns are the returned history
    names = sorted(p.name for p in (run / "weights").iterdir())
    assert names == ["best.pt", "epoch1.pt", "epoch2.pt", "last.pt"], names  # save_period=1: the 0-based epochs 1 and 2, never 0
    last, best = (torch.load(run / "weights" / n, weights_only=False) for n in ("last.pt", "best.pt"))
    want_best, want_at = _best_epoch(T.fits)
    print("fitness per epoch", T.fits, "-> best.pt of epoch", want_at)
    assert last["epoch"] == 2 and best["epoch"] == want_at and best["best_fitness"] == best["fitness"] == want_best
    assert last["best_fitness"] == want_best and last["fitness"] == T.fits[-1] and set(last["train_metrics"]) >= {"fitness", "val/box_loss"}
    assert torch.load(run / "weights" / "epoch1.pt", weights_only=False)["epoch"] == 1
    # final_eval: trainer.metrics is the validation of best.pt's EMA weights (no fitness key, as in the reference)
    assert set(tr.metrics) == set(COLS[4:8]) and tr.validator.seen == 7 and tr.validator.training is False
    # resume from last.pt: the csv goes on, the best fitness is carried over, last.pt stayed resumable
    y2 = YOLO(str(run / "weights" / "last.pt"))
    hist2 = y2.train(trainer=T, data=data_yaml, resume=True, epochs=5, **kw)
    assert y2.trainer.start_epoch == 3 and len(hist2) == 2 and T.started_with == want_best
    head, rows2 = _read_csv(run / "results.csv")
    assert head == COLS and rows2[:, 0].tolist() == [1, 2, 3, 4, 5]
    np.testing.assert_array_equal(rows2[:3], rows)
    assert y2.trainer.best_fitness == max(want_best, _best_epoch([want_best] + T.fits)[0])
    assert torch.load(run / "weights" / "last.pt", weights_only=False)["epoch"] == 4


def test_patience_ends_the_run(data_yaml, tmp_path):
    """patience=1 and a fitness that falls after the first epoch: the run ends after epoch 2 of 6.  (A CONSTANT fitness never runs
    out of patience: EarlyStopping's ``>=`` moves its best epoch along, as in the reference -- tests/test_host_val_epoch.py.)"""
    from ultralytics import YOLO
    T = _trainer_class(stub=[0.5, 0.4, 0.3, 0.2, 0.1, 0.05])
    torch.manual_seed(0)
    y = YOLO(MODEL)
    hist = y.train(trainer=T, data=data_yaml, epochs=6, project=str(tmp_path), name="stop", val_period=1, patience=1, **KW)
    tr = y.trainer
    assert len(hist) == 2 and tr.stop and tr.epoch == 1 and T.fits == [0.5, 0.4]
    head, rows = _read_csv(tmp_path / "stop" / "results.csv")
    assert rows[:, 0].tolist() == [1, 2]
    assert torch.load(tmp_path / "stop" / "weights" / "best.pt", weights_only=False)["epoch"] == 0
    assert torch.load(tmp_path / "stop" / "weights" / "last.pt", weights_only=False)["epoch"] == 1


def test_validating_every_epoch_leaves_the_training_undisturbed(data_yaml):
    """val_period=0 twice: are parameters and history bit-equal run to run under deterministic=True?  If so the same is required of
    val_period=0 against val_period=1; if not, the difference must stay within the run-to-run spread."""
    from ultralytics import YOLO

    def run(period):
        torch.manual_seed(0)
        y = YOLO(MODEL)
        hist = y.train(data=data_yaml, epochs=3, val=False, val_period=period, **KW)
        tr = y.trainer
        return np.asarray(hist, dtype=np.float64), tr.plan.rt.flat_p.clone(), tr.plan.ema.clone(), tr.plan.rt.flat_b.clone()

    a, b, c = run(0), run(0), run(1)
    same = all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])) and np.array_equal(a[0], b[0])
    spread = max(float((x - y).abs().max()) for x, y in zip(a[1:], b[1:]))
    diff = max(float((x - y).abs().max()) for x, y in zip(a[1:], c[1:]))
    print(f"val_period=0 run to run: bit-equal {same} (max abs parameter difference {spread:.3e}); val_period=0 vs 1: {diff:.3e}")
    if same:
        assert np.array_equal(a[0], c[0]) and all(torch.equal(x, y) for x, y in zip(a[1:], c[1:]))
    else:
        assert diff <= 2 * spread and np.abs(a[0] - c[0]).max() <= 2 * np.abs(a[0] - b[0]).max()
