#!/usr/bin/env python3
"""The device-side bootstrap of the validation statistics (csrc/bootstrap.hip behind ultralytics.utils.bootstrap.bootstrap_map) timed
against the host loop a user would write without it: this package's ``ap_per_class`` on the replicated statistics, once per resample.

Synthetic statistics of a realistic size: 1,500 images, 6 classes, about 150 detections per image (what validation at conf 0.001
keeps), resamples of half the split.  S = 30, 1,000 and 10,000 resamples on the device; the host loop runs at S = 30 only and is
extrapolated linearly (every resample costs it the same).  The two legs alternate in one process after a warm-up; the device leg is
timed with device events around the launch, and once more with a host clock around bootstrap_map (upload of the table, launch,
download, the means); the host leg with a host clock.  The two must agree to 1e-9 on mAP50 and mAP50-95 of all 30 resamples.

usage: bootstrap_bench.py [--out profiles/r10_bootstrap.md] [--rounds 3] [--images 1500] [--dets 150] [--host-samples 30]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "experiment-yolo_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

NC = 6
SIZES = (30, 1000, 10000)


def synth_stats(n_img, per_img, seed=0):
    """Validation statistics like a trained detector's at conf 0.001: ~8 labels per image, most of them found by a confident detection,
    the long tail of low-confidence detections false.  -> numpy tp (D, 10), conf, cls, det_img, lab_cls, lab_img."""
    rng = np.random.default_rng(seed)
    n_lab = rng.integers(2, 15, n_img)
    lab_img = np.repeat(np.arange(n_img), n_lab)
    lab_cls = rng.integers(0, NC, len(lab_img))
    # one candidate detection per label (found with probability 0.85, at a random depth of IoU thresholds) ...
    found = rng.random(len(lab_img)) < 0.85
    depth = np.where(found, rng.integers(1, 11, len(lab_img)), 0)
    tp_a = depth[:, None] > np.arange(10)[None, :]
    conf_a = np.clip(rng.beta(5, 2, len(lab_img)) * np.where(found, 1.0, 0.4), 0.001, 0.999)
    # ... and the false-positive tail
    n_fp = np.maximum(per_img - n_lab, 0)
    img_b = np.repeat(np.arange(n_img), n_fp)
    tp_b = np.zeros((len(img_b), 10), bool)
    conf_b = np.clip(rng.beta(1, 12, len(img_b)), 0.001, 0.999)
    cls_b = rng.integers(0, NC, len(img_b))
    tp, conf = np.concatenate([tp_a, tp_b]), np.concatenate([conf_a, conf_b]).astype(np.float32)
    conf = (np.argsort(np.argsort(conf, kind="stable"), kind="stable") + 1) / (len(conf) + 1)  # distinct: a permutation
    return tp, conf.astype(np.float64), np.concatenate([lab_cls, cls_b]), np.concatenate([lab_img, img_b]), lab_cls, lab_img


def host_loop(a, mult):
    """What a user of the parent commit writes: per resample, replicate the statistics and call ap_per_class."""
    from ultralytics.utils.metrics import ap_per_class
    tp, conf, cls, dimg, lcls, limg = a
    m50, m = np.zeros(len(mult)), np.zeros(len(mult))
    for s, row in enumerate(mult):
        rd, rl = row[dimg].astype(np.int64), row[limg].astype(np.int64)
        ap = ap_per_class(np.repeat(tp, rd, 0), np.repeat(conf, rd), np.repeat(cls, rd), np.repeat(lcls, rl))[5]
        m50[s], m[s] = ap[:, 0].mean(), ap.mean()
    return m50, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_bootstrap.md"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--images", type=int, default=1500)
    ap.add_argument("--dets", type=int, default=150)
    ap.add_argument("--host-samples", type=int, default=30)
    o = ap.parse_args()
    from ultralytics.hip import check, lib
    from ultralytics.utils.bootstrap import bootstrap_map, draw_resamples, pack_stats
    if not torch.cuda.is_available():
        raise SystemExit("bootstrap_bench.py measures on the GPU: no device found")
    a = synth_stats(o.images, o.dets)
    tp, conf, cls, dimg, lcls, limg = a
    D, L = len(conf), len(lcls)
    t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).cuda()  # noqa: E731
    stats = pack_stats(t(tp, torch.bool), t(conf, torch.float64), t(cls, torch.int64), t(dimg, torch.int64), t(lcls, torch.int64),
                       t(limg, torch.int64), o.images, NC)
    mults = {S: draw_resamples(o.images, S, 0.5, 42) for S in SIZES}
    n_size = int(mults[SIZES[0]][0].sum())
    # bytes the kernel moves per resample, from the shapes: each class's workgroup reads its segment of tp_bits (2 B) + det_img (4 B)
    # twice (totals, then the scan), the resample's multiplicity row (2 B per image) and its column of lab_cnt (4 B per image) once,
    # and writes 10 fp64 + 1 int32
    bytes_per_resample = 2 * 6 * D + NC * o.images * (2 + 4) + NC * (10 * 8 + 4)
    L_ = lib()
    stream = torch.cuda.current_stream().cuda_stream

    def kernel_ms(S, reps):
        m = torch.from_numpy(mults[S].view(np.int16)).cuda()
        out, nl = torch.empty((S, NC, 10), dtype=torch.float64, device="cuda"), torch.empty((S, NC), dtype=torch.int32, device="cuda")
        call = lambda: check(L_.dy_bootstrap_ap(stats["tp_bits"].data_ptr(), stats["det_img"].data_ptr(), stats["cls_off"].data_ptr(),  # noqa: E731
                                                stats["lab_cnt"].data_ptr(), m.data_ptr(), D, o.images, NC, S, out.data_ptr(), nl.data_ptr(),
                                                stream), "dy_bootstrap_ap")
        call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def call_ms(S):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = bootstrap_map(stats, mults[S])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    for S in SIZES:  # warm-up: code object, allocator, every shape
        call_ms(S)
    host_loop(a, mults[SIZES[0]][:2])
    rows = {S: dict(kernel=[], call=[]) for S in SIZES}
    host_ms, dev30, host30 = [], None, None
    for r in range(o.rounds):  # the legs alternate
        for S in SIZES:
            rows[S]["kernel"].append(kernel_ms(S, 20 if S <= 1000 else 5))
            ms, res = call_ms(S)
            rows[S]["call"].append(ms)
            if S == SIZES[0]:
                dev30 = res
        t0 = time.perf_counter()
        host30 = host_loop(a, mults[SIZES[0]][:o.host_samples])
        host_ms.append((time.perf_counter() - t0) * 1e3)
    err50 = float(np.abs(dev30[0][:o.host_samples] - host30[0]).max())
    err95 = float(np.abs(dev30[1][:o.host_samples] - host30[1]).max())
    assert err50 < 1e-9 and err95 < 1e-9, (err50, err95)
    host_per = float(np.median(host_ms)) / o.host_samples
    lines = ["# Bootstrap of the validation statistics: device kernel against the host loop, one MI355X", "",
             f"`python tools/bootstrap_bench.py`: {o.images} images, {NC} classes, {D} detections ({D / o.images:.0f} per image), {L} labels; "
             f"resamples of {n_size} images (half the split); {o.rounds} rounds, the two legs alternating in one process after a warm-up; "
             "medians (min .. max).", "",
             "Device kernel: device events around `dy_bootstrap_ap`, mean of 20 launches (5 at S = 10,000) per round.  Device call: host "
             "clock around `bootstrap_map` (upload of the multiplicity table, launch, download of `ap` / `nl`, the means), ending in a "
             f"synchronise.  Host loop: host clock around `ap_per_class` on the replicated statistics of {o.host_samples} resamples "
             "(`np.repeat`, one call per resample: what a user of the parent commit writes); larger S are that time per resample times S "
             "(extrapolated, not run).", "",
             f"Bytes the kernel moves per resample, from the shapes: 2 x 6 B x {D} detections + {NC} x {o.images} images x 6 B + "
             f"{NC} x 84 B out = {bytes_per_resample / 1e6:.2f} MB (the statistics are read once per resample and class segment, twice "
             "over; they stay in the last-level cache between workgroups).", "",
             "| S | device kernel ms | GB/s (bytes above) | device call ms | host loop ms | host / device call |", "|---|---|---|---|---|---|"]
    for S in SIZES:
        k, c = np.array(rows[S]["kernel"]), np.array(rows[S]["call"])
        host = host_per * S
        tag = "" if S == o.host_samples else " (extrapolated)"
        lines.append(f"| {S} | {np.median(k):.3f} ({k.min():.3f} .. {k.max():.3f}) | {bytes_per_resample * S / np.median(k) / 1e6:.0f} | "
                     f"{np.median(c):.2f} ({c.min():.2f} .. {c.max():.2f}) | {host:.0f}{tag} | {host / np.median(c):.0f}x |")
    h = np.array(host_ms)
    lines += ["", f"Host loop at S = {o.host_samples}: {np.median(h):.0f} ms ({h.min():.0f} .. {h.max():.0f}), {host_per:.1f} ms per resample.",
              f"Agreement of the two legs on the {o.host_samples} resamples: max |mAP50 difference| = {err50:.2e}, max |mAP50-95 difference| = "
              f"{err95:.2e} (asserted below 1e-9).", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
