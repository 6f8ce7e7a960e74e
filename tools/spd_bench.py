#!/usr/bin/env python3
"""SPDConv's space-to-depth permutation (csrc/spd.hip) measured: (a) stand-alone, each way, at the DEAL-YOLO-N 640x640 batch-64
shapes, beside the other byte movers of the library at the same element count in the same run; (b) its share of a training step of
yolov8n-ASF-P2P2-SPD (event-timed replay of the recorded launch list, as tools/op_profile.py times it).

usage: spd_bench.py [--kernel] [--step] [--batch 64] [--model yolov8n-ASF-P2P2-SPD]     (both parts when neither is named)

Every timed loop walks a ring of buffer sets larger than the 256 MB last-level cache, so a kernel never finds its operands resident
from its previous repetition; TB/s are algorithmic bytes (each operand read or written once) over the mean time per launch."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "experiment-yolo_amd")]
import torch  # noqa: E402

SHAPES = [(64, 320, 320, 16), (64, 160, 160, 32), (64, 80, 80, 64)]  # inputs of SPDConv layers 1, 3 / 18, 5 / 21 of scale n
RING_BYTES = 1 << 30


def timeit(fns, reps=40):
    """Mean ms per call of the callables in ``fns`` taken in turn (one per ring slot)."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_part():
    from ultralytics.hip import check, lib
    L = lib()
    s = torch.cuda.current_stream().cuda_stream

    def call(name, *a):
        check(getattr(L, name)(*a, s), name)

    print("(a) stand-alone, fp16 NHWC; us per launch and TB/s of algorithmic bytes")
    for N, H, W, C in SHAPES:
        e = N * H * W * C
        ring = max(2, -(-RING_BYTES // (4 * e)))
        xs = [torch.randn(N, H, W, C, device="cuda").half() for _ in range(ring)]
        ys = [torch.empty(N, H // 2, W // 2, 4 * C, dtype=torch.float16, device="cuda") for _ in range(ring)]
        lo = [torch.randn(N, H // 2, W // 2, C, device="cuda").half() for _ in range(ring)]  # nn.Upsample's input for an output like x
        coef = torch.rand(4 * C, device="cuda") + 0.5
        rows = []

        def row(label, nbytes, fns):
            t = timeit(fns)
            rows.append(f"  {label:34s} {t * 1e3:8.1f} us  {nbytes / t / 1e9:5.2f} TB/s")

        p = lambda t: t.data_ptr()  # noqa: E731
        row("space_to_depth forward", 4 * e, [lambda x=x, y=y: call("dy_space_to_depth", p(x), C, p(y), 4 * C, N, H, W, C, 0, 0) for x, y in zip(xs, ys)])
        row("space_to_depth backward, store", 4 * e, [lambda x=x, y=y: call("dy_space_to_depth", p(x), C, p(y), 4 * C, N, H, W, C, 1, 0) for x, y in zip(xs, ys)])
        row("space_to_depth backward, accumulate", 6 * e, [lambda x=x, y=y: call("dy_space_to_depth", p(x), C, p(y), 4 * C, N, H, W, C, 1, 1) for x, y in zip(xs, ys)])
        row("upsample2x forward (same output)", 2 * e + e // 2, [lambda a=a, x=x: call("dy_upsample2x", p(a), C, p(x), C, N, H // 2, W // 2, C, 0, 0) for a, x in zip(lo, xs)])
        row("upsample2x backward (same input)", 2 * e + e // 2, [lambda a=a, x=x: call("dy_upsample2x", p(x), C, p(a), C, N, H // 2, W // 2, C, 1, 0) for a, x in zip(lo, xs)])
        row("add of two tensors", 6 * e, [lambda x=x, y=y: call("dy_add", p(x), C, p(y), C, 0, 0, p(y), C, N * H * W, C) for x, y in zip(xs, ys)])
        row("bn_act_apply (SiLU)", 4 * e, [lambda x=x, y=y: call("dy_bn_act_apply", p(x), C, 0, 0, p(y), C, p(coef), N * H * W, C, 1) for x, y in zip(xs, ys)])
        row("torch copy_", 4 * e, [lambda x=x, y=y: y.view(-1).copy_(x.view(-1)) for x, y in zip(xs, ys)])
        print(f"x = ({N}, {H}, {W}, {C}): {2 * e / 1e6:.0f} MB per tensor, ring of {ring}")
        print("\n".join(rows))
        del xs, ys, lo
        torch.cuda.empty_cache()


def step_part(model_name, B):
    from bench import CFG, synth_batch
    from ultralytics.hip.train import StepPlan
    from ultralytics.nn.tasks import DetectionModel
    torch.manual_seed(0)
    model = DetectionModel(os.path.join(os.path.dirname(CFG), model_name + ".yaml"), verbose=False).cuda().train()
    plan = StepPlan(model, B, 640, nmax=8)
    batch = {k: v.cuda() for k, v in synth_batch(1, B, 640, 6).items()}
    plan.set_hyper([0.01] * 3, 0.937, [0, 5e-4, 0])
    for _ in range(3):
        plan.forward_backward(batch)
        plan.optimizer_step()
    prof = plan.profile_ops(5)
    total = sum(ms for _, _, ms in prof)
    perm = [(a, ms) for name, a, ms in prof if name == "dy_space_to_depth"]
    print(f"(b) {model_name}, batch {B}, 640x640: {len(prof)} launches in forward + backward, {total:.3f} ms of device time")
    for a, ms in perm:
        n, h, w, c, back, acc = a[4], a[5], a[6], a[7], a[8], a[9]
        by = n * h * w * c * 2 * (3 if acc else 2)
        print(f"  space_to_depth {'backward' if back else 'forward '} ({n}, {h}, {w}, {c}){' +=' if acc else '   '} {ms * 1e3:8.1f} us  {by / ms / 1e9:5.2f} TB/s")
    psum = sum(ms for _, ms in perm)
    print(f"  {len(perm)} permutation launches: {psum:.3f} ms = {100 * psum / total:.2f} % of the step's device time")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--model", default="yolov8n-ASF-P2P2-SPD")
    a = ap.parse_args()
    if a.kernel or not a.step:
        kernel_part()
    if a.step or not a.kernel:
        step_part(a.model, a.batch)
