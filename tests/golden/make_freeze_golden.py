"""Generate tests/golden/freeze.npz from the REFERENCE implementation: training with ``freeze=...``.

Run in the build container only (needs the reference tree, see _refimport):

    python tests/golden/make_freeze_golden.py

DEAL-YOLO-N (yolov8n-ASF-P2P2) at 64x64, batch 2, the shared deterministic state ``fill_state(seed=11)`` and the batches
``synth_batch(900 + ni, 2, 4, nc)`` -- the protocol of ``gen_trainer`` in make_golden.py -- once per freeze case.  Each case records
the names the reference's rule freezes, the names that hold a gradient after a backward pass, a 3-iteration SGD trace with
``gen_trainer``'s columns and three tensors after the trace.  The fixture holds names, scalars and those tensors only.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference import harness and pins the numeric environment)
from make_golden import BaseTrainer, DetectionModel, ModelEMA, SimpleNamespace, get_cfg, np, og, synth_batch, torch  # noqa: E402
from make_golden import DEFAULT_CFG  # noqa: E402

CASES = {"8": 8, "5": 5, "l2": [2], "l12_20": [12, 20], "l26": [26]}
TENSORS = ("model.0.conv.weight", "model.12.cv1.conv.weight", "model.26.cv3.0.2.bias")  # stem, one neck, one head tensor


def freeze_rule(names, freeze):
    """The three lines of reference engine/trainer.py:663-671 + :674: ``freeze`` int -> range(n), list -> itself, else nothing;
    a parameter is frozen when 'model.{i}.' of a listed layer or '.dfl' is a substring of its name."""
    layers = freeze if isinstance(freeze, list) else range(freeze) if isinstance(freeze, int) else []
    keys = [f"model.{x}." for x in layers] + [".dfl"]
    return [k for k in names if any(x in k for x in keys)]


def gen_freeze():
    arrs = {}
    name = "yolov8n-ASF-P2P2"
    yaml_path = os.path.join(mg.CFG_DIR, name + ".yaml")
    for tag, freeze in CASES.items():
        torch.manual_seed(0)
        m = DetectionModel(yaml_path, ch=3, verbose=False)
        args = get_cfg(DEFAULT_CFG)
        m.args = args
        g = og.build_graph(og.load_yaml(yaml_path))
        m.load_state_dict(og.fill_state(og.state_layout(g), seed=11), strict=True)
        frozen = freeze_rule([k for k, _ in m.named_parameters()], freeze)
        for k, v in m.named_parameters():  # reference engine/trainer.py:672-682
            v.requires_grad = k not in frozen
        bs, nb, epochs = 2, 8, 100
        fake = SimpleNamespace(args=args, model=m)
        accumulate = max(round(args.nbs / bs), 1)
        wd = args.weight_decay * bs * accumulate / args.nbs
        fake.optimizer = BaseTrainer.build_optimizer(fake, model=m, name="SGD", lr=args.lr0, momentum=args.momentum, decay=wd)
        fake.scaler = torch.cuda.amp.GradScaler(enabled=False)
        fake.ema = ModelEMA(m)
        lf = lambda x: max(1 - x / epochs, 0) * (1.0 - args.lrf) + args.lrf  # noqa: E731
        for pg in fake.optimizer.param_groups:
            pg["initial_lr"] = pg["lr"]
        nw = max(round(args.warmup_epochs * nb), 100)
        last_opt_step = -1
        m.train()  # frozen layers keep BatchNorm in training mode, as the reference's trainer leaves them
        trace, with_grad = [], None
        for ni in range(3):
            xi = [0, nw]
            accumulate = max(1, int(np.interp(ni, xi, [1, args.nbs / bs]).round()))
            for j, x in enumerate(fake.optimizer.param_groups):
                x["lr"] = np.interp(ni, xi, [args.warmup_bias_lr if j == 0 else 0.0, x["initial_lr"] * lf(0)])
                if "momentum" in x:
                    x["momentum"] = np.interp(ni, xi, [args.warmup_momentum, args.momentum])
            batch = synth_batch(900 + ni, bs, 4, g.nc)
            loss, items = m(batch)
            loss.backward()
            if with_grad is None:
                with_grad = [k for k, p in m.named_parameters() if p.grad is not None]
            gnorm = torch.sqrt(sum((p.grad.float() ** 2).sum() for p in m.parameters() if p.grad is not None))
            stepped = 0
            if ni - last_opt_step >= accumulate:
                BaseTrainer.optimizer_step(fake)
                last_opt_step = ni
                stepped = 1
            sd = m.state_dict()
            esd = fake.ema.ema.state_dict()
            trace.append([float(loss), *[float(v) for v in items], float(gnorm), stepped,
                          *[float(pg["lr"]) for pg in fake.optimizer.param_groups],
                          float(sum(v.double().sum() for k, v in sd.items() if v.dtype.is_floating_point)),
                          float(sum(v.double().abs().sum() for k, v in sd.items() if v.dtype.is_floating_point)),
                          float(sum(v.double().abs().sum() for k, v in esd.items() if v.dtype.is_floating_point))])
        arrs[f"{tag}/freeze"] = np.array(freeze if isinstance(freeze, list) else [freeze])
        arrs[f"{tag}/freeze_is_list"] = np.array(isinstance(freeze, list))
        arrs[f"{tag}/frozen_names"] = np.array(frozen)
        arrs[f"{tag}/grad_names"] = np.array(with_grad)
        arrs[f"{tag}/trace"] = np.array(trace, dtype=np.float64)
        for t in TENSORS:
            arrs[f"{tag}/final/{t}"] = m.state_dict()[t]
        print(tag, len(frozen), "frozen,", len(with_grad), "with a gradient; grad norms", [round(r[4], 1) for r in trace])
    arrs["param_names"] = np.array([k for k, _ in m.named_parameters()])
    arrs["trace_columns"] = np.array(["loss", "box", "cls", "dfl", "grad_norm", "stepped", "lr_bias", "lr_w", "lr_bn",
                                      "sum_state", "abs_state", "abs_ema"])
    mg.npz("freeze", **arrs)


if __name__ == "__main__":
    gen_freeze()
