#!/usr/bin/env python3
"""Entry script with the reference's shape (reference testandcox.py without its Kaggle paths): paired bootstrap test of the mAP@0.5
of two models on the test split of a dataset.  Each model validates the split once; the resamples are evaluated on the GPU from the
kept statistics (ultralytics/utils/bootstrap.py).

    python testandcox.py <deal weights.pt | model.yaml> <baseline weights.pt | model.yaml> <data.yaml> [split=test] [num_samples=30]
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "experiment-yolo_amd"))
from ultralytics.utils.bootstrap import (BOOTSTRAP_CI_ITERS, NUM_SAMPLES, RNG_SEED, SAMPLE_FRACTION, paired_bootstrap_test,  # noqa: E402
                                         summary_lines)

if __name__ == "__main__":
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    deal_weights, baseline_weights, data_yaml = sys.argv[1:4]
    split = sys.argv[4] if len(sys.argv) > 4 else "test"
    num_samples = int(sys.argv[5]) if len(sys.argv) > 5 else NUM_SAMPLES
    res = paired_bootstrap_test(deal_weights, baseline_weights, data_yaml, split=split, num_samples=num_samples,
                                sample_fraction=SAMPLE_FRACTION, seed=RNG_SEED, ci_iters=BOOTSTRAP_CI_ITERS)
    n_size = int(res["mult"][0].sum())
    print(f"Found {len(res['im_files'])} test images. Each sample uses {n_size} images. Ran {num_samples} iterations.")
    print("\n".join(summary_lines(res)))
    print(f"\nSaved: {res['csv']}" + (f" and {res['histogram']}" if res["histogram"] else ""))
