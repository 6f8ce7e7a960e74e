"""Generate tests/golden/tta.npz: test-time augmentation (``model(x, augment=True)``) of the REFERENCE implementation.

Run in the build container only (needs the reference tree, which ``_refimport`` locates):

    python tests/golden/make_tta_golden.py

Weights come from ``oracle.graph.fill_state(layout, 7)``, inputs are uint8 images (used as u8 / 255) from a numpy PCG64 stream.
``img/<tag>``: the uint8 images; per case ``<case>/``: ``img`` (the tag of its images), ``y`` (the reference's augmented output),
per pass ``hw`` (Hp, Wp of the scaled image), ``A`` (anchor count of the pass's output) and ``cols`` (the kept column range [lo, hi)
after _clip_augmented), and ``gs`` / ``nl``.
The 96x128 case also holds ``scaled2``, the reference's scale_img output of the third pass (ratio 0.67).
"""
import os
import sys
import warnings

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

os.environ["MKL_CBWR"] = "COMPATIBLE"  # as tests/conftest.py pins it

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _refimport  # noqa: E402

_refimport.install()

import ultralytics.nn.tasks as ref_tasks  # noqa: E402
from ultralytics.nn.tasks import DetectionModel  # noqa: E402

from oracle import graph as og  # noqa: E402

CFG_DIR = os.path.join(_refimport.REF, "ultralytics/cfg/models")
torch.set_num_threads(8)

# (case, model, fused, batch, H, W, image tag): the fused case reads the same images as its unfused twin
CASES = [
    ("asf_p2p2_64", "yolov8n-ASF-P2P2", False, 2, 64, 64, "asf_p2p2_64"),
    ("asf_p2p2_96x128", "yolov8n-ASF-P2P2", False, 2, 96, 128, "asf_p2p2_96x128"),
    ("asf_p2p2_160", "yolov8n-ASF-P2P2", False, 2, 160, 160, "asf_p2p2_160"),
    ("asf_p2p2_96x128_fused", "yolov8n-ASF-P2P2", True, 2, 96, 128, "asf_p2p2_96x128"),
    ("p2_64", "yolov8n-p2", False, 1, 64, 64, "p2_64"),
]


def model(name, fused):
    cfg = os.path.join(CFG_DIR, name + ".yaml")
    torch.manual_seed(0)
    m = DetectionModel(cfg, ch=3, verbose=False)
    g = og.build_graph(og.load_yaml(cfg))
    m.load_state_dict(og.fill_state(og.state_layout(g), 7), strict=True)
    m.eval()
    if fused:
        m.fuse(verbose=False)
    return m


def main():
    arrs, imgs = {}, {}
    rng = np.random.default_rng(20261016)
    for case, name, fused, B, H, W, tag in CASES:
        if tag not in imgs:
            imgs[tag] = rng.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
        u8 = imgs[tag]
        m = model(name, fused)
        scaled, counts = [], {}
        real_scale = ref_tasks.scale_img

        def spy_scale(img, ratio=1.0, same_shape=False, gs=32):
            out = real_scale(img, ratio, same_shape, gs)
            scaled.append(out.detach().clone())
            counts["gs"] = gs
            return out

        real_clip = m._clip_augmented

        def spy_clip(y):
            counts["A"] = [int(t.shape[-1]) for t in y]
            out = real_clip(y)
            counts["kept"] = [int(t.shape[-1]) for t in out]
            return out

        ref_tasks.scale_img, m._clip_augmented = spy_scale, spy_clip
        try:
            with torch.no_grad():
                y, train_out = m(torch.from_numpy(u8).float() / 255, augment=True)
        finally:
            ref_tasks.scale_img = real_scale
        assert train_out is None and len(scaled) == 3
        A, kept = counts["A"], counts["kept"]
        cols = [(0, kept[0])] + [(0, a) for a in A[1:-1]] + [(A[-1] - kept[-1], A[-1])]
        arrs[f"img/{tag}"] = u8
        arrs[f"{case}/img"] = np.array(tag)
        arrs[f"{case}/y"] = y.numpy()
        arrs[f"{case}/hw"] = np.array([t.shape[-2:] for t in scaled], dtype=np.int32)
        arrs[f"{case}/A"] = np.array(A, dtype=np.int32)
        arrs[f"{case}/cols"] = np.array(cols, dtype=np.int32)
        arrs[f"{case}/gs"] = np.int32(counts["gs"])
        arrs[f"{case}/nl"] = np.int32(m.model[-1].nl)
        if case == "asf_p2p2_96x128":
            arrs[f"{case}/scaled2"] = scaled[2].numpy()
        print(case, tuple(y.shape), "hw", arrs[f"{case}/hw"].tolist(), "A", A, "cols", cols, "gs", counts["gs"])
    path = os.path.join(HERE, "tta.npz")
    np.savez_compressed(path, **arrs)
    print(f"tta.npz  {os.path.getsize(path) / 1024:.1f} KiB  ({len(arrs)} arrays)")


if __name__ == "__main__":
    main()
