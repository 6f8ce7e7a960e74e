#!/usr/bin/env python3
"""The recorded launch list of one traced step (or one inference plan), argument for argument, as JSON: the check that an engine
refactor left the launches as they were.  Two checkouts are compared by running this same file in each and diffing the directories.

One configuration = one model YAML (scale n), a set of DY_* switches, a ``freeze`` and a class count.  The switches are read when the
engine is imported, so the driver runs every configuration in a fresh child process, one after the other, each under its own time
limit, and stops at the first that fails.  The child builds the model under torch.manual_seed(11) (its own initialisation: a tool may
not import the oracle that fills tests/test_gpu_freeze.py's model, and no recorded argument depends on a weight's value), applies
``freeze`` by the trainer's rule, makes StepPlan(m, 2, 64, nmax=8, init_scale=1024.0) without a graph, runs one forward_backward on
synth_batch(900, 2, 4, nc) and writes ``plan.rec_fb.ops`` with ``fb_split`` / ``fb_cut`` (inference: InferPlan at 64x64, ``plan.rec.ops``),
one entry per op: name, stream id (fork / join markers keep their stream argument) and the normalised arguments --
  float -> repr, small integer -> itself, device / host address -> [buffer, byte offset] with ``buffer`` the allocation that holds it
  (the engine's kept-alive buffers, the arena, the runtime's flat buffers; an address in none of them is an allocation of its own),
  numbered by first appearance in the list; ctypes structures and arrays field by field; a byref out-parameter by value.

usage: launch_list.py --out DIR [--only REGEX] [--limit SECONDS] [--imgsz 64]   every configuration (whose tag matches) into DIR/<tag>.json
       launch_list.py --compare DIR_A DIR_B                                     table of op counts and verdicts (exit 1 on a difference)"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "experiment-yolo_amd", "ultralytics", "cfg", "models")
MAIN = "yolov8n-ASF-P2P2"
MODELS = ["yolov8n-p2", "yolov8n-ASF", "yolov8n-ASF-P2", MAIN, "yolov8n-ASF-P2P2-SPD", "yolov8n-ASF-P2P2-DySample",
          "yolov8n-ASF-P2P2-CARAFE", "yolov8n-ASF-P2P2-DW", "yolov8n-ASF-P2P2-ADown", "yolov8n-ASF-P2P2-BiFPN",
          "yolov8n-ASF-P2P2-SlimNeck", "yolov8n-ASF-P2P2-SimAM", "yolov8n-LD-P2", "yolov8n-LD-P2-SPD"]
SWITCHES = ["DY_BN_ACC=0", "DY_BN_WGRAD=0", "DY_BN_RES=0", "DY_BIAS_WGRAD=0", "DY_BN_GROUP=0", "DY_HEAD_ROWS=0",
            "DY_HEAD_CLS=0 DY_HEAD_APPLY=0", "DY_WGRAD_DGRAD=0", "DY_PLANAR=0", "DY_PLANAR_CV1=0", "DY_PLANAR_CV1=0 DY_SIDE_WGRAD=1",
            "DY_SIDE_WGRAD=1", "DY_HEAD_STREAMS=1", "DY_UPSEG_TRAIN=0", "DY_STEM_DIRECT=0", "DY_BN_DGRED=1 DY_BN_DGRED_MAXC=32"]
FREEZE = {"8": 8, "5": 5, "l2": [2], "l12_20": [12, 20], "l26": [26]}  # tests/test_gpu_freeze.py::CASES
ADDRESS = 1 << 40  # integers from here on are addresses (no count, size or stride of a 64x64 step comes near)


def matrix():
    """[(tag, dict(model, env, freeze, nc, infer))]: the configurations, in the order they run."""
    cfgs = [(m, dict(model=m)) for m in MODELS]
    for m in (MAIN, "yolov8n-LD-P2"):
        for sw in SWITCHES:
            cfgs.append((m + "+" + sw.replace(" ", "+"), dict(model=m, env=dict(kv.split("=") for kv in sw.split()))))
    for tag, fr in FREEZE.items():
        cfgs.append((f"{MAIN}+freeze={tag}", dict(model=MAIN, freeze=fr)))
    cfgs.append((f"{MAIN}+freeze=8+DY_FROZEN_DGRAD=0", dict(model=MAIN, freeze=8, env={"DY_FROZEN_DGRAD": "0"})))
    cfgs.append((f"{MAIN}+nc=3", dict(model=MAIN, nc=3)))
    cfgs.append((f"{MAIN}+infer", dict(model=MAIN, infer="unfused")))
    cfgs.append((f"{MAIN}+infer+fused", dict(model=MAIN, infer="fused")))
    return cfgs


class Normaliser:
    def __init__(self, tensors):
        spans = {}
        for t in tensors:
            if t is not None and t.is_cuda:
                s = t.untyped_storage()
                spans[s.data_ptr()] = max(spans.get(s.data_ptr(), 0), s.nbytes())
        self.spans = sorted(spans.items())
        self.ids = {}

    def address(self, a):
        base = a
        for b, n in self.spans:
            if b <= a < b + max(n, 1):
                base = b
                break
        return [self.ids.setdefault(base, len(self.ids)), a - base]

    def __call__(self, v):
        if type(v).__name__ == "CArgObject":  # byref(x): by value
            return self(v._obj)
        if isinstance(v, C.Structure):
            return {name: self(getattr(v, name)) for name, *_ in v._fields_}
        if isinstance(v, C.Array):
            return [self(x) for x in v]
        if isinstance(v, C._SimpleCData):
            return self(v.value)
        if isinstance(v, bool) or v is None:
            return v
        if isinstance(v, float):
            return repr(v)
        if isinstance(v, int):
            return self.address(v) if v >= ADDRESS else v
        if isinstance(v, bytes):
            return v.hex()
        raise TypeError(f"launch argument of type {type(v).__name__}")


def synth_batch(torch, np, seed, B, n_per, nc, hw):
    """tests/golden/cases.py::synth_batch (that module imports the oracle, which a tool may not)."""
    rng = np.random.default_rng(seed)
    img = torch.from_numpy(rng.random((B, 3, *hw), dtype=np.float32))
    cls = torch.from_numpy(rng.integers(0, nc, (B * n_per, 1)).astype(np.float32))
    wh = torch.from_numpy((rng.random((B * n_per, 2)) * 0.3 + 0.05).astype(np.float32))
    xy = torch.from_numpy((rng.random((B * n_per, 2)) * 0.7 + 0.15).astype(np.float32))
    return dict(img=img, batch_idx=torch.arange(B).repeat_interleave(n_per).float(), cls=cls, bboxes=torch.cat([xy, wh], 1))


def child(cfg, out, S=64):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
    import numpy as np
    import torch
    from ultralytics.engine.trainer import frozen_parameter_names
    from ultralytics.nn.tasks import DetectionModel
    torch.manual_seed(11)
    m = DetectionModel(os.path.join(CFG_DIR, cfg["model"] + ".yaml"), ch=3, nc=cfg.get("nc"), verbose=False)
    nc = m.yaml["nc"]
    if "freeze" in cfg:
        frozen = set(frozen_parameter_names([k for k, _ in m.named_parameters()], cfg["freeze"]))
        for k, v in m.named_parameters():
            v.requires_grad = k not in frozen
    extra = {}
    if cfg.get("infer"):
        from ultralytics.hip.infer import InferPlan
        m = m.cuda().eval()
        if cfg["infer"] == "fused":
            m = m.fuse()
        plan = InferPlan(m, 2, S, S, use_graph=False)
        with torch.no_grad():
            plan(synth_batch(torch, np, 900, 2, 4, nc, (S, S))["img"].cuda())
        rec, kept = plan.rec, list(plan.keep)
        extra["head"] = plan.head
    else:
        from ultralytics.hip.train import StepPlan
        plan = StepPlan(m.cuda().train(), 2, S, nmax=8, init_scale=1024.0)
        plan.forward_backward(synth_batch(torch, np, 900, 2, 4, nc, (S, S)))
        rec, kept = plan.rec_fb, []
        extra.update(fb_split=plan.fb_split, fb_cut=plan.fb_cut)
    torch.cuda.synchronize()
    eng, rt = plan.eng, plan.rt
    arena = getattr(plan, "arena", None)
    flats = [getattr(rt, n, None) for n in ("flat_p", "flat_gb", "flat_g", "flat_b", "flat_sink")]
    norm = Normaliser(list(eng.keep) + kept + [getattr(arena, "buf", None)] + flats)
    ops = [dict(name=name, sid=sid, args=[norm(a) for a in args]) for _fn, args, name, sid in rec.ops]
    with open(out, "w") as f:
        json.dump(dict(config=cfg, **extra, n_ops=len(ops), ops=ops), f, indent=0)
    print(f"{os.path.basename(out)}: {len(ops)} ops, {len(norm.ids)} buffers")


def drive(a):
    os.makedirs(a.out, exist_ok=True)
    for tag, cfg in matrix():
        if a.only and not re.search(a.only, tag):
            continue
        env = dict(os.environ, **cfg.get("env", {}))
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", json.dumps(cfg),
               "--out", os.path.join(a.out, tag + ".json"), "--imgsz", str(a.imgsz)]
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            print(f"{tag}: exit status {rc}; stopping")
            return rc
    return 0


def compare(da, db):
    bad = 0
    print("| configuration | ops | verdict |\n|---|---|---|")
    for tag, _ in matrix():
        fa, fb = (os.path.join(d, tag + ".json") for d in (da, db))
        if not (os.path.exists(fa) or os.path.exists(fb)):
            continue  # (a run restricted with --only)
        if not (os.path.exists(fa) and os.path.exists(fb)):
            print(f"| `{tag}` | - | MISSING |")
            bad += 1
            continue
        ja, jb = (json.load(open(f)) for f in (fa, fb))
        if ja == jb:
            print(f"| `{tag}` | {ja['n_ops']} | identical |")
            continue
        bad += 1
        first = next((i for i, (x, y) in enumerate(zip(ja["ops"], jb["ops"])) if x != y), min(ja["n_ops"], jb["n_ops"]))
        print(f"| `{tag}` | {ja['n_ops']} / {jb['n_ops']} | DIFFERS from op {first} |")
        for j in (ja, jb):
            if first < j["n_ops"]:
                print("    ", json.dumps(j["ops"][first])[:600], file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--only", default="")
    ap.add_argument("--limit", type=int, default=150, help="seconds one configuration may take")
    ap.add_argument("--imgsz", type=int, default=64, help="input size (64: the suite's; larger maps reach the one-launch 1x1 backward forms)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--compare", nargs=2, metavar="DIR")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if a.child:
        child(json.loads(a.child), a.out, a.imgsz)
    else:
        sys.exit(drive(a))
