"""Rank process of tests/test_gpu_freeze.py: a one-rank RCCL group whose StepPlan is told world_size = 2 (the pattern of
tests/dp_worker.py), training with layers 0..DY_TEST_FREEZE-1 frozen.  8 is the whole backbone of this model: with DY_DP_BUCKETS=2 the second gradient bucket
(the backbone's) has no backward launch at all and the plan exchanges one bucket at the optimizer step; 6 leaves it two layers.  Writes the final weights / buffers / EMA for the parent to compare across bucket counts."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "experiment-yolo_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
import torch.distributed as dist

from dp_common import build_model, global_batch, hyper


def main(out_dir):
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    from ultralytics.engine.trainer import frozen_parameter_names
    from ultralytics.hip.train import StepPlan
    n_frozen = int(os.environ.get("DY_TEST_FREEZE", "8"))
    m = build_model()
    frozen = set(frozen_parameter_names([k for k, _ in m.named_parameters()], n_frozen))
    for k, v in m.named_parameters():
        v.requires_grad = k not in frozen
    m.cuda().train()
    plan = StepPlan(m, 2, 64, nmax=8, optimizer="SGD", world_size=2, use_graph=True, init_scale=1.0, dynamic_scale=False)
    for it in range(2):
        plan.set_hyper(*hyper(it))
        plan.forward_backward(global_batch(it, 0, 2), exchange=True)
        plan.all_reduce()
        plan.optimizer_step()
    torch.cuda.synchronize()
    if os.environ.get("DY_DP_BUCKETS") == "2":
        assert plan.buckets == 2
        if n_frozen >= len(m.yaml["backbone"]):  # an empty second half: no cut, no second graph, nothing started on the side stream
            assert plan.fb_cut is None and plan.graph_fb2 is None and not plan._bucket_pending
        else:
            assert plan.fb_cut is not None and plan.graph_fb2 is not None, "the bucketed path was asked for and not taken"
    taken, skipped, _ = plan.check_progress()
    assert (taken, skipped) == (2, 0)
    rt = plan.rt
    fr = rt.frozen.bool()
    assert int(fr.sum()) > 0 and float(rt.flat_g[fr].abs().max()) == 0.0, "a frozen parameter's flat gradient is not zero"
    torch.save({"p": rt.flat_p.cpu(), "b": rt.flat_b.cpu(), "ema": plan.ema.cpu(), "retries": plan.capture_retries}, os.path.join(out_dir, "rank0.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
