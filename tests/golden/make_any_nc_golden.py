"""Generate tests/golden/any_nc_layout.json.gz, tests/golden/any_nc.npz and tests/golden/ref_ckpt_nc37.pt from the REFERENCE
implementation (generation-time only: needs the reference tree, see _refimport.py; run on the CPU).

    python tests/golden/make_any_nc_golden.py

any_nc_layout.json.gz: {"<yaml>/<nc>": [[state_dict key, shape], ...]} in the reference's registration order, for
  yolov8n-ASF-P2P2 / yolov8n-LD-P2 / yolov8n-p2 built by the reference's DetectionModel(yaml, nc=nc) at nc in {1, 6, 33, 37, 40, 100,
  120} -- what tests/test_host_any_nc.py holds this package's models to.  Names and shapes only.

ref_ckpt_nc37.pt: the reference's on-disk layout (engine/trainer.py:898-923: whole-module pickle, fp16) of yolov8-ASF-P2P2 with
  nc = 37, written by the reference's classes.  At scale n the fp16 state alone is 2.1 MiB, over the size limit for a committed
  file, so the graph is built at scale ``t = [0.33, 0.125, 1024]`` (half of n's width): Detect's ch[0] is 16 there and its class
  branch max(16, min(37, 100)) = 37 wide on every level -- the same Conv(x, 37, 3) -> Conv(37, 37, 3) -> Conv2d(37, 37, 1) chains.
  The file is data: tensors, class paths and the YAML dict.

any_nc.npz: ckpt/img (the batch), ckpt/y_eval (what the checkpoint's fp16-rounded state computes in the reference's eval forward,
  fp32 arithmetic), ckpt/seed."""
import gzip
import json
import os
import sys
import warnings
from copy import deepcopy

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

os.environ["MKL_CBWR"] = "COMPATIBLE"  # as tests/conftest.py pins it

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

import _refimport  # noqa: E402

_refimport.install()

from ultralytics.cfg import get_cfg  # noqa: E402
from ultralytics.nn.tasks import DetectionModel  # noqa: E402
from ultralytics.utils import DEFAULT_CFG  # noqa: E402

from cases import synth_batch  # noqa: E402
from oracle import graph as og  # noqa: E402

assert sys.modules[DetectionModel.__module__].__file__.startswith(_refimport.REF)
OUR_CFG = os.path.join(ROOT, "experiment-yolo_amd", "ultralytics", "cfg", "models")
torch.set_num_threads(8)

MODELS = ["yolov8n-ASF-P2P2", "yolov8n-LD-P2", "yolov8n-p2"]
NCS = [1, 6, 33, 37, 40, 100, 120]
CKPT_SEED, CKPT_SCALE, CKPT_NC = 37, ("t", [0.33, 0.125, 1024]), 37


def gen_layouts():
    out = {}
    for name in MODELS:
        for nc in NCS:
            m = DetectionModel(os.path.join(OUR_CFG, name + ".yaml"), ch=3, nc=nc, verbose=False)
            out[f"{name}/{nc}"] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    path = os.path.join(HERE, "any_nc_layout.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print(f"any_nc_layout.json.gz  {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} models")


def ckpt_yaml():
    d = yaml.safe_load(open(os.path.join(OUR_CFG, "yolov8-ASF-P2P2.yaml")))
    d["scales"][CKPT_SCALE[0]] = CKPT_SCALE[1]
    d["scale"] = CKPT_SCALE[0]
    d["nc"] = CKPT_NC
    return d


def gen_ckpt():
    d = ckpt_yaml()
    m = DetectionModel(deepcopy(d), ch=3, verbose=False)
    g = og.build_graph(deepcopy(d))
    m.load_state_dict(og.fill_state(og.state_layout(g), CKPT_SEED), strict=True)
    m.args = dict(get_cfg(DEFAULT_CFG).__dict__)
    ckpt = {"epoch": 3, "best_fitness": 0.25, "model": deepcopy(m).half(), "ema": None, "updates": 57, "optimizer": None,
            "train_args": {"imgsz": 640, "batch": 64, "model": "yolov8-ASF-P2P2.yaml"}, "date": "2026-01-01T00:00:00", "version": "8.1.9"}
    path = os.path.join(HERE, "ref_ckpt_nc37.pt")
    torch.save(ckpt, path)
    assert os.path.getsize(path) < 1 << 20, os.path.getsize(path)
    m.load_state_dict({k: (v.half().float() if v.is_floating_point() else v) for k, v in m.state_dict().items()})
    m.eval()
    img = synth_batch(370, 2, 4, CKPT_NC)["img"]
    with torch.no_grad():
        y = m(img)[0]
    assert tuple(m.state_dict()[f"model.{len(m.model) - 1}.cv3.0.0.conv.weight"].shape) == (37, 16, 3, 3)
    np.savez_compressed(os.path.join(HERE, "any_nc.npz"), **{"ckpt/img": img.numpy(), "ckpt/y_eval": y.numpy(), "ckpt/seed": np.int32(CKPT_SEED)})
    print(f"ref_ckpt_nc37.pt  {os.path.getsize(path) / 1024:.1f} KiB, {sum(q.numel() for q in m.parameters())} parameters; y_eval {tuple(y.shape)}")


if __name__ == "__main__":
    gen_layouts()
    gen_ckpt()
