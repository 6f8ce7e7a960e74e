#!/usr/bin/env python3
"""The on-device confusion matrix and false-positive count (csrc/confusion.hip) timed at the shape tests/val_bench.py uses: batch 64,
300 detections and 40 labels per image, 6 classes.

  update_metrics, plots off   DetectionValidator.update_metrics as before: one dy_match_predictions launch per batch
  update_metrics, plots on    the same plus one dy_confusion_matrix launch
  dy_confusion_matrix alone   device events around the launch, on the native-space predictions update_metrics left
  dy_count_fp alone           device events around the launch, the same detections against fp64 label rows
  host loop                   the per-image numpy restatement of both rules (tests/test_host_confusion.py) on the same data, the
                              predictions copied to the host first, as the reference's per-image loop does

The update_metrics legs alternate (off, on, off, on, ...) in one process after a warm-up and are timed with a host clock around
``reps`` calls that end in a device synchronise; the kernel legs with device events around ``reps`` launches.  Device and host counts
must be identical.

usage: confusion_bench.py [--out profiles/r11_confusion.md] [--rounds 5] [--reps 20] [--batch 64] [--dets 300] [--labels 40]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "experiment-yolo_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

NC = 6


def synth(B, ND, NL, seed=0):
    """The data of tests/val_bench.py: labels anywhere, detections jittered off random labels of their image (sigma 6 px)."""
    rng = np.random.default_rng(seed)
    lab = np.concatenate([rng.random((B * NL, 2)) * 0.8 + 0.1, rng.random((B * NL, 2)) * 0.15 + 0.02], 1).astype(np.float32)
    bidx = np.repeat(np.arange(B), NL).astype(np.float32)
    cls = rng.integers(0, NC, (B * NL, 1)).astype(np.float32)
    preds = []
    for i in range(B):
        src = rng.integers(0, NL, ND)
        l = lab[i * NL + src] * 640
        bx = np.stack([l[:, 0] - l[:, 2] / 2, l[:, 1] - l[:, 3] / 2, l[:, 0] + l[:, 2] / 2, l[:, 1] + l[:, 3] / 2], 1) + rng.normal(0, 6, (ND, 4)).astype(np.float32)
        conf = np.sort(rng.random((ND, 1)).astype(np.float32), 0)[::-1]
        preds.append(np.concatenate([bx, conf, cls[i * NL + src]], 1).astype(np.float32))
    return dict(batch_idx=bidx, cls=cls, bboxes=lab), preds


def validator(plots):
    from ultralytics.models.yolo.detect import DetectionValidator
    v = DetectionValidator(args=dict(plots=plots))
    v.device = torch.device("cuda:0")
    v.init_metrics(type("M", (), {"names": {i: str(i) for i in range(NC)}})())
    return v


def timed_calls(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def timed_launches(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_confusion.md"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--labels", type=int, default=40)
    o = ap.parse_args()
    from test_host_confusion import confusion_rule, count_fp_rule
    from ultralytics.hip import check, lib
    assert torch.cuda.is_available(), "confusion_bench.py measures on the GPU"
    B, ND, NL = o.batch, o.dets, o.labels
    batch, preds = synth(B, ND, NL)
    tb = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    tb["img"] = torch.zeros(B, 3, 640, 640, device="cuda")
    plist = [torch.from_numpy(p).cuda() for p in preds]
    v_off, v_on = validator(False), validator(True)
    for v in (v_off, v_on):
        for _ in range(3):
            v.update_metrics(plist, tb)
            v.stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[])
    t_off, t_on = [], []
    for _ in range(o.rounds):
        for v, acc in ((v_off, t_off), (v_on, t_on)):
            acc.append(timed_calls(lambda: v.update_metrics(plist, tb), o.reps))
            v.stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[])
    # ---- the kernels alone, on what update_metrics left on the device
    stream = torch.cuda.current_stream().cuda_stream
    predn = v_on.last_predn
    off = torch.from_numpy(np.arange(B + 1, dtype=np.int32) * ND).cuda()
    geom = torch.tensor([[1, 0, 0, 640, 640]] * B, dtype=torch.float32, device="cuda")
    tcls, tidx, tbox = tb["cls"].reshape(-1).contiguous(), tb["batch_idx"].contiguous(), tb["bboxes"].contiguous()
    cm = torch.zeros((NC + 1) ** 2 + 1, dtype=torch.int32, device="cuda")

    def launch_cm():
        check(lib().dy_confusion_matrix(predn.data_ptr(), off.data_ptr(), B * ND, tidx.data_ptr(), tcls.data_ptr(), tbox.data_ptr(), B * NL,
                                        geom.data_ptr(), B, 640, 640, NC, 0.25, 0.45, 1, cm.data_ptr(), cm.data_ptr() + 4 * (NC + 1) ** 2, stream),
              "dy_confusion_matrix")

    rows = np.concatenate([batch["cls"].astype(np.float64), batch["bboxes"].astype(np.float64)], 1)  # cls xc yc w h
    lab64 = torch.from_numpy(rows).cuda()
    loff = torch.from_numpy(np.arange(B + 1, dtype=np.int32) * NL).cuda()
    wh = torch.full((B, 2), 640, dtype=torch.int32, device="cuda")
    fp, st = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")

    def launch_fp():
        check(lib().dy_count_fp(predn.data_ptr(), off.data_ptr(), lab64.data_ptr(), loff.data_ptr(), wh.data_ptr(), B, 0.25, 0.5, fp.data_ptr(),
                                st.data_ptr(), stream), "dy_count_fp")

    launch_cm(), launch_fp()
    k_cm = [timed_launches(launch_cm, o.reps) for _ in range(o.rounds)]
    k_fp = [timed_launches(launch_fp, o.reps) for _ in range(o.rounds)]
    cm.zero_()
    launch_cm()
    dev_cm, dev_fp = cm.cpu().numpy()[:-1].reshape(NC + 1, NC + 1), fp.cpu().numpy()
    # ---- the host loop on the same data
    lab, s = batch["bboxes"], np.float32(640)  # the kernel's fp32 formulas at gain 1, padding 0
    dw, dh = lab[:, 2] / np.float32(2), lab[:, 3] / np.float32(2)
    nat = np.clip(np.stack([(lab[:, 0] - dw) * s, (lab[:, 1] - dh) * s, (lab[:, 0] + dw) * s, (lab[:, 1] + dh) * s], 1), np.float32(0), s)
    t0 = time.perf_counter()
    pn = predn.cpu().numpy()
    host_cm = sum(confusion_rule(pn[i * ND:(i + 1) * ND], nat[i * NL:(i + 1) * NL], batch["cls"][i * NL:(i + 1) * NL, 0], NC, skip_unlabelled=True)
                  for i in range(B))
    h_cm = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    pn = predn.cpu().numpy()
    host_fp = [count_fp_rule(pn[i * ND:(i + 1) * ND], rows[i * NL:(i + 1) * NL], 640, 640) for i in range(B)]
    h_fp = (time.perf_counter() - t0) * 1e3
    same_cm, same_fp = bool((host_cm == dev_cm).all()), host_fp == dev_fp.tolist()
    med = lambda a: float(np.median(a))
    spread = lambda a: f"{min(a):.3f} .. {max(a):.3f}"
    lines = [
        f"shape: batch {B} x {ND} detections x {NL} labels, {NC} classes; {o.rounds} rounds of {o.reps} calls, legs alternating",
        "",
        "| leg | median ms per batch | range over rounds |",
        "|---|---|---|",
        f"| update_metrics, plots off (host clock, incl. host packing) | {med(t_off):.3f} | {spread(t_off)} |",
        f"| update_metrics, plots on (host clock, incl. host packing) | {med(t_on):.3f} | {spread(t_on)} |",
        f"| dy_confusion_matrix alone (device events) | {med(k_cm):.4f} | {spread(k_cm)} |",
        f"| dy_count_fp alone (device events) | {med(k_fp):.4f} | {spread(k_fp)} |",
        f"| host loop, confusion matrix (numpy per image, one run) | {h_cm:.1f} | |",
        f"| host loop, false positives (numpy per image, one run) | {h_fp:.1f} | |",
        "",
        f"device counts equal the host loop's: confusion matrix {same_cm} ({int(dev_cm.sum())} counts, {int(dev_cm[:NC, :NC].sum())} matched), "
        f"false positives {same_fp} ({int(dev_fp.sum())} of {int((pn[:, 4] >= 0.25).sum())} kept detections)",
    ]
    print("\n".join(lines))
    if o.out:
        with open(o.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert same_cm and same_fp, "device and host counts differ"


if __name__ == "__main__":
    main()
