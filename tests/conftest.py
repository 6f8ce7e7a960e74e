import os
import sys

# MKL's code path depends on the host CPU (vendor, vector width), and with it the last bits of exp, matmul and eigh: the
# fixtures that pin the oracle bit for bit (soft-NMS scores, the trainer traces, SOAP's eigenbases) hold on every x86 host
# only on MKL's processor-independent branch.  tests/golden/make_golden.py generates them on the same branch.  Set before
# torch loads MKL.
os.environ["MKL_CBWR"] = "COMPATIBLE"

import numpy as np  # noqa: E402
import pytest  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "experiment-yolo_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import ultralytics.hip  # noqa: E402,F401  (sets DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 before any test initialises HIP)

GOLDEN = os.path.join(ROOT, "tests", "golden")
CFG_DIR = os.path.join(PKG, "ultralytics", "cfg", "models")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


class Golden:
    """Lazy view of one tests/golden/*.npz fixture with '/'-separated keys."""

    def __init__(self, name):
        self.z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)

    def __getitem__(self, k):
        return self.z[k]

    def t(self, k):
        import torch

        a = self.z[k]
        return torch.from_numpy(a.astype(np.float32) if a.dtype == np.float16 else a)

    def keys(self, prefix=""):
        return [k for k in self.z.files if k.startswith(prefix)]

    def __contains__(self, k):
        return k in self.z.files


@pytest.fixture(scope="session")
def golden():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Golden(name)
        return cache[name]

    return get
