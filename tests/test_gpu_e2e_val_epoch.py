"""-m gpu: the end-to-end protocol of tests/test_gpu_e2e_trainer.py (same dataset, models and overrides) with ``val_period=1``: the
results.csv this package writes against the reference trainer's own results.csv (tests/golden/e2e_trainer*.npz) -- the learning-rate
columns, the per-epoch validation losses of the EMA model and the last epoch's mAP50.  One 40-epoch run per model, shared by the
tests of that model."""
import os

import numpy as np
import pytest
import torch

from golden.cases import E2E, write_e2e_dataset

pytestmark = pytest.mark.gpu

MODELS = [("yolov8n-ASF-P2P2.yaml", "e2e_trainer.npz"), ("yolov8n-LD-P2.yaml", "e2e_trainer_ld.npz")]
# epochs 1 and 2 of val/*_loss: twice the measured worst relative deviation over the three losses (measured N 1.5e-4 / 4e-5, LD 9e-5 /
# 1.9e-4; one unit of the csv's fifth digit is 2.4e-5 of these values), never looser than what tests/test_gpu_e2e_trainer.py puts on
# the same epochs' training losses (1e-2; 2e-2, LD 3e-2)
EARLY = {"yolov8n-ASF-P2P2.yaml": (min(2 * 1.5e-4, 1e-2), min(2 * 4e-5, 2e-2)), "yolov8n-LD-P2.yaml": (min(2 * 9e-5, 1e-2), min(2 * 1.9e-4, 3e-2))}
VAL = ("val/box_loss", "val/cls_loss", "val/dfl_loss")


@pytest.fixture(scope="module", params=MODELS, ids=["DEAL-YOLO-N", "LD"])
def run(request, tmp_path_factory):
    from ultralytics import YOLO
    model, fixture = request.param
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", fixture))
    head = [str(h) for h in G["header"]]
    ref = {h: G["results"][:, j] for j, h in enumerate(head)}
    tmp = tmp_path_factory.mktemp("e2e_val")
    root = str(tmp / "e2e")
    write_e2e_dataset(root)
    zero = dict(mosaic=0.0, mixup=0.0, copy_paste=0.0, hsv_h=0.0, hsv_s=0.0, hsv_v=0.0, degrees=0.0, translate=0.0, scale=0.0, shear=0.0,
                perspective=0.0, flipud=0.0, fliplr=0.0)
    torch.manual_seed(0)
    y = YOLO(model)
    y.train(data=os.path.join(root, "data.yaml"), epochs=E2E["epochs"], batch=E2E["batch"], imgsz=E2E["imgsz"], workers=2, optimizer="SGD",
            amp=False, val=True, close_mosaic=0, seed=0, deterministic=True, log_every=1, val_period=1, patience=0, project=str(tmp), name="run",
            **zero)
    lines = open(tmp / "run" / "results.csv").read().splitlines()
    names = [c.strip() for c in lines[0].split(",")]
    rows = np.loadtxt(tmp / "run" / "results.csv", delimiter=",", skiprows=1)
    assert names == head and rows.shape == (E2E["epochs"], 14)
    return model, {h: rows[:, j] for j, h in enumerate(names)}, ref, y.trainer


def test_learning_rate_columns_follow_the_reference_schedule(run):
    """lr/pg0..2 of all 40 epochs to the fixture's printed precision: the warm-up's interpolation towards ``lr0 * lf(epoch)`` through
    epoch 13 (ni <= 100), and past it the reference's one-epoch lag -- its LambdaLR is stepped at the END of an epoch after
    ``last_epoch`` was set to start_epoch - 1 (engine/trainer.py:737, :873), so epoch e trains with ``lr0 * lf(e - 1)``.  (Before
    ``train_step`` followed the lag this failed on epochs 14-40: 3.5 % at epoch 14, 41.6 % at epoch 40.)"""
    model, ours, ref, tr = run
    keys = ("lr/pg0", "lr/pg1", "lr/pg2")
    dev = np.array([[abs(ours[k][e] - ref[k][e]) / ref[k][e] for k in keys] for e in range(E2E["epochs"])])
    print("relative deviation of lr/pg0..2 from the reference's results.csv, per epoch:\n", np.round(dev, 5))
    bad = [e + 1 for e in range(E2E["epochs"]) if dev[e].max() >= 1e-4]
    assert not bad, f"epochs whose lr differs from the reference's by more than 1e-4 relative: {bad} (worst {dev.max():.4f})"


def test_validation_losses_follow_the_reference_curve(run):
    """val/{box,cls,dfl}_loss: epochs 1 and 2 number for number (early in training the EMA follows the weights almost exactly, decay
    ~ updates / 2000, so the validation loss is a function of the same state as the training loss) at twice the measured deviation
    (EARLY); the last epoch within the existing test's last-epoch margin.  Measured, relative, (box, cls, dfl): DEAL-YOLO-N epoch 1
    (5e-5, 1.5e-4, 2e-5), epoch 2 (2e-5, 4e-5, 2e-5), epochs 3-5 up to 1.4e-3, last epoch (0.018, 0.044, 0.085); LD epoch 1 (2e-5, 9e-5,
    2e-5), epoch 2 (1.9e-4, 0, 7e-5), epochs 3-5 up to 1.3e-3, last epoch (0.010, 0.044, 0.022)."""
    model, ours, ref, tr = run
    dev = np.array([[abs(ours[k][e] - ref[k][e]) / ref[k][e] for k in VAL] for e in range(E2E["epochs"])])
    print("relative deviation of val/{box,cls,dfl}_loss from the reference's results.csv, epochs 1-5:\n", np.round(dev[:5], 5))
    print("last epoch:", np.round(dev[-1], 4), " ours", [ours[k][-1] for k in VAL], " reference", [ref[k][-1] for k in VAL])
    assert all(np.isfinite(ours[k]).all() for k in VAL)
    assert dev[0].max() <= EARLY[model][0] and dev[1].max() <= EARLY[model][1], "epochs 1 and 2: same initial weights, same batches"
    assert dev[-1].max() < 0.25, "last-epoch validation losses"


def test_last_epoch_map_is_within_reach_of_the_reference(run):
    """The csv's last row -- the EMA model's validation after epoch 40, as in the reference's results.csv -- not ``trainer.metrics``
    (final_eval's validation of best.pt, printed only)."""
    model, ours, ref, tr = run
    m = tr.metrics
    print(f"last row: ours P {ours['metrics/precision(B)'][-1]:.3f} R {ours['metrics/recall(B)'][-1]:.3f} mAP50 {ours['metrics/mAP50(B)'][-1]:.3f} "
          f"mAP50-95 {ours['metrics/mAP50-95(B)'][-1]:.3f}   reference mAP50 {ref['metrics/mAP50(B)'][-1]:.3f} mAP50-95 "
          f"{ref['metrics/mAP50-95(B)'][-1]:.3f}   best.pt (final_eval): mAP50 {m['metrics/mAP50(B)']:.3f} mAP50-95 {m['metrics/mAP50-95(B)']:.3f}")
    assert abs(ours["metrics/mAP50(B)"][-1] - ref["metrics/mAP50(B)"][-1]) < 0.2
