"""CPU: the host side of the per-epoch validation loop (cfg ``val_period >= 1``; reference engine/trainer.py:844-923, 963-973,
1021-1027 and utils/torch_utils.py:568-610): EarlyStopping, the results.csv writer against the rows of the reference's own
results.csv (tests/golden/e2e_trainer.npz), the best_fitness / best.pt rule through the trainer's own methods with the validator
stubbed, the cfg key, and the stop-flag broadcast between two gloo ranks."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN, PKG, ROOT


def test_early_stopping_follows_the_reference_semantics():
    from ultralytics.utils.torch_utils import EarlyStopping
    fit = [0, 0, .1, .3, .2, .2, .3, .1, .1, .1]
    es = EarlyStopping(3)
    best, possible, stops = [], [], []
    for e, f in enumerate(fit, 1):
        stops.append(es(e, f))
        best.append(es.best_epoch)
        possible.append(es.possible_stop)
    assert best == [1, 2, 3, 4, 4, 4, 7, 7, 7, 7]  # >=: an equal fitness moves best_epoch along
    assert [e for e, p in enumerate(possible, 1) if p] == [6, 9, 10]
    assert stops == [False] * 9 + [True]
    never = EarlyStopping(0)
    assert not any(never(e, 0.0 if e > 1 else 1.0) for e in range(1, 500)) and never.best_epoch == 1
    es = EarlyStopping(3)
    es(1, 0.5)
    before = (es.best_epoch, es.best_fitness, es.possible_stop)
    assert es(7, None) is False and (es.best_epoch, es.best_fitness, es.possible_stop) == before


def _bare_trainer(tmp_path, **overrides):
    """A DetectionTrainer without a device: the loop's host methods only (the constructor selects a GPU)."""
    from ultralytics.cfg import get_cfg
    from ultralytics.engine.trainer import DetectionTrainer
    tr = object.__new__(DetectionTrainer)
    tr.args = get_cfg(overrides=dict(val_period=1, **overrides))
    tr.rank, tr.world_size, tr.validator = 0, 1, None
    tr.save_dir = tmp_path
    if tmp_path is not None:
        (tmp_path / "weights").mkdir(parents=True, exist_ok=True)
    tr._begin_val_loop()
    return tr


def test_save_metrics_reproduces_the_reference_results_csv(tmp_path):
    G = np.load(os.path.join(GOLDEN, "e2e_trainer.npz"))
    head, rows = [str(h) for h in G["header"]], G["results"]
    tr = _bare_trainer(tmp_path)
    for r in rows[:5]:
        tr.epoch = int(r[0]) - 1
        tr.save_metrics(dict(zip(head[1:], r[1:])))
    text = (tmp_path / "results.csv").read_text().splitlines()
    assert len(text) == 6 and [c.strip() for c in text[0].split(",")] == head and len(head) == 14
    assert all(len(c) == 23 for line in text for c in line.split(","))  # the reference's fixed-width columns
    back = np.loadtxt(tmp_path / "results.csv", delimiter=",", skiprows=1)
    want = np.array([[float("%.5g" % v) for v in r] for r in rows[:5]])
    np.testing.assert_array_equal(back, want)
    tr.epoch = 5
    tr.save_metrics(dict(zip(head[1:], rows[5][1:])))  # a later call appends one row, no second header
    text = (tmp_path / "results.csv").read_text().splitlines()
    assert len(text) == 7 and sum("epoch" in line for line in text) == 1
    assert [r["epoch"] for r in tr.results] == [1, 2, 3, 4, 5, 6] and list(tr.results[0]) == head
    # a run without a save directory keeps the rows and writes nothing
    tr2 = _bare_trainer(None)
    tr2.epoch = 0
    tr2.save_metrics(dict(zip(head[1:], rows[0][1:])))
    assert tr2.csv is None and len(tr2.results) == 1


def test_best_fitness_and_best_pt_follow_the_reference_rule(tmp_path):
    """``not best_fitness or best_fitness < fitness`` replaces the best (reference engine/trainer.py:971): a zero best is always
    replaced, an equal non-zero fitness is not, and best.pt is the checkpoint of the epoch that set the best."""
    fit = [0.0, 0.0, 0.2, 0.2, 0.5, 0.3, 0.5, 0.1]
    tr = _bare_trainer(tmp_path, epochs=len(fit), patience=0, save_period=3)

    class Stub:
        calls = 0

        def __call__(self, trainer=None, model=None):
            self.calls += 1
            return {**dict.fromkeys(trainer.metric_keys, 0.25), "fitness": fit[trainer.epoch],
                    **trainer.label_loss_items([1.0, 2.0, 3.0], prefix="val")}

    tr.validator = Stub()
    tr._checkpoint = lambda: {"epoch": tr.epoch, "best_fitness": tr.best_fitness, "fitness": tr.fitness}
    best_epoch, want_best, want_epoch = [], None, None
    for e, f in enumerate(fit):
        tr.epoch, tr.lr = e, {"lr/pg0": 0.1, "lr/pg1": 0.01, "lr/pg2": 0.01}
        tr._end_of_epoch([3.0, 2.0, 1.0], 1)
        if not want_best or want_best < f:
            want_best, want_epoch = f, e
        assert tr.best_fitness == want_best and tr.fitness == f
        last, best = (torch.load(tmp_path / "weights" / n, weights_only=False) for n in ("last.pt", "best.pt"))
        assert last["epoch"] == e and best["epoch"] == want_epoch and best["fitness"] == best["best_fitness"] == want_best
        best_epoch.append(best["epoch"])
    assert best_epoch == [0, 1, 2, 2, 4, 4, 4, 4]  # the ties at 0.2 and 0.5 leave best.pt alone
    assert tr.validator.calls == len(fit) and not tr.stop
    assert sorted(p.name for p in (tmp_path / "weights").iterdir()) == ["best.pt", "epoch3.pt", "epoch6.pt", "last.pt"]  # save_period=3, never epoch 0
    row = tr.results[-1]
    assert list(row) == ["epoch", "train/box_loss", "train/cls_loss", "train/dfl_loss", *tr.metric_keys, "val/box_loss", "val/cls_loss",
                         "val/dfl_loss", "lr/pg0", "lr/pg1", "lr/pg2"]
    assert (row["epoch"], row["train/box_loss"], row["val/dfl_loss"], row["lr/pg0"]) == (len(fit), 3.0, 3.0, 0.1)


def test_epochs_between_validations_keep_stale_metrics_and_fitness(tmp_path):
    tr = _bare_trainer(tmp_path, epochs=5, patience=0)
    seen = []

    def stub(trainer=None, model=None):
        seen.append(trainer.epoch)
        return {**dict.fromkeys(trainer.metric_keys, 0.1 * (trainer.epoch + 1)), "fitness": 0.1 * (trainer.epoch + 1),
                **trainer.label_loss_items([1.0, 1.0, 1.0], prefix="val")}

    tr.validator = stub
    tr._checkpoint = lambda: {"epoch": tr.epoch}
    for e in range(5):
        tr.epoch, tr.lr = e, {"lr/pg0": 0.1, "lr/pg1": 0.01, "lr/pg2": 0.01}
        tr._end_of_epoch([1.0, 1.0, 1.0], 2)
    assert seen == [1, 3, 4]  # every second epoch, and the final one
    m = [r["metrics/mAP50(B)"] for r in tr.results]
    assert m[0] == 0 and m[1] == m[2] == pytest.approx(0.2) and m[3] == pytest.approx(0.4) and m[4] == pytest.approx(0.5)
    assert torch.load(tmp_path / "weights" / "best.pt", weights_only=False)["epoch"] == 4


def test_patience_stops_the_loop_on_constant_fitness(tmp_path):
    tr = _bare_trainer(tmp_path, epochs=10, patience=1)
    tr.validator = lambda trainer=None, model=None: {**dict.fromkeys(trainer.metric_keys, 0.0), "fitness": 0.3,
                                                     **trainer.label_loss_items([1.0, 1.0, 1.0], prefix="val")}
    tr._checkpoint = lambda: {"epoch": tr.epoch}
    stops = []
    for e in range(3):
        tr.epoch, tr.lr = e, {"lr/pg0": 0.1, "lr/pg1": 0.01, "lr/pg2": 0.01}
        tr._end_of_epoch([1.0, 1.0, 1.0], 1)
        stops.append(tr.stop)
    # EarlyStopping's >= moves its best epoch along on a constant fitness: patience never runs out, as in the reference
    assert stops == [False, False, False] and tr.stopper.best_epoch == 3


def test_val_period_is_a_typed_cfg_key():
    from ultralytics.cfg import DEFAULT_CFG_DICT, get_cfg
    assert DEFAULT_CFG_DICT["val_period"] == 0 and get_cfg().val_period == 0
    assert get_cfg(overrides={"val_period": 1}).val_period == 1
    with pytest.raises(TypeError):
        get_cfg(overrides={"val_period": "x"})


def _flag_worker(rank, world, port, q):
    sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ultralytics.hip.dist import broadcast_flag
    got = [broadcast_flag(rank == 0, 0), broadcast_flag(rank != 0, 0)]  # rank 0 says stop, then go on; rank 1 says the opposite
    q.put((rank, got))
    dist.barrier()
    dist.destroy_process_group()


def test_stop_flag_is_broadcast_from_rank_zero():
    from ultralytics.hip.dist import broadcast_flag
    assert broadcast_flag(True) is True and broadcast_flag(False) is False  # single process: the flag itself
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_flag_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    assert got[0] == [True, False] and got[1] == [True, False]  # rank 1 receives rank 0's flag, whatever its own was
