"""Host side of the streaming 1x1 convolution (csrc/conv.hip conv_plan, dy_conv1x1_kernel_name_live): which kernel a 1x1
launch runs under DY_CONV1X1_STREAM = 0 / force / unset.  No GPU: the helpers only do arithmetic on the geometry."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
import ctypes as C, json, sys
sys.path[:0] = [%r, %r]
from ultralytics.hip import DY_EPI_ACCUM, DY_EPI_BIAS, DY_EPI_F32OUT, DY_EPI_SILU, DY_EPI_STATS, DY_EPI_STATS_ACC, DySegs, lib
L, buf, out = lib(), C.create_string_buffer(128), {}
def live(key, cin, cout, n, h, w, epi, xs=None, ys=None):
    rc = L.dy_conv1x1_kernel_name_live(cin, cout, n, h, w, epi, xs, ys, buf, 128)
    out[key] = buf.value.decode() if rc == 0 else rc
for tag, (n, h, w) in (("big", (64, 160, 160)), ("small", (1, 40, 40))):
    live(tag + "/plain", 64, 64, n, h, w, 0)
    live(tag + "/accum", 64, 64, n, h, w, DY_EPI_ACCUM)
    live(tag + "/stats_acc", 64, 64, n, h, w, DY_EPI_STATS | DY_EPI_STATS_ACC)
    live(tag + "/stats_rows", 64, 64, n, h, w, DY_EPI_STATS)
    live(tag + "/f32", 64, 64, n, h, w, DY_EPI_F32OUT | DY_EPI_BIAS)
    live(tag + "/bias_silu", 64, 64, n, h, w, DY_EPI_BIAS | DY_EPI_SILU)
    live(tag + "/wide", 256, 64, n, h, w, 0)
    live(tag + "/cin16", 16, 32, n, h, w, 0)
    live(tag + "/cin8", 8, 32, n, h, w, 0)
    live(tag + "/cout48", 64, 48, n, h, w, 0)
t = DySegs()
t.nseg = 4
for i in range(4):
    t.c_end[i], t.ld[i], t.ptr[i] = 32 * (i + 1), 32, 4096
live("segx", 128, 64, 64, 80, 80, DY_EPI_STATS | DY_EPI_STATS_ACC, C.byref(t), None)
live("segy", 64, 128, 64, 80, 80, 0, None, C.byref(t))
t.acc[1] = 2
live("segx_up", 128, 64, 64, 80, 80, 0, C.byref(t), None)
t.acc[1] = 0
def name(fn, *a):
    return buf.value.decode() if fn(*a, buf, 128) == 0 else None
out["pinned"] = [name(L.dy_conv_kernel_name, 64, 64, 1, 1), name(L.dy_conv_kernel_name, 128, 64, 1, 1),
                 name(L.dy_conv_kernel_name_at, 64, 64, 1, 1, 160, 1, 0), name(L.dy_conv1x1_segs_kernel_name, 128, 64, C.byref(t))]
t.nseg = 3
for i in range(3):
    t.c_end[i], t.ld[i] = 16 * (i + 1), 16
out["pinned"].append(name(L.dy_conv1x1_segs_kernel_name, 48, 32, C.byref(t)))
print(json.dumps(out))
""" % (ROOT, os.path.join(ROOT, "experiment-yolo_amd"))

PINNED = ["conv_mfma_pp_kernel<64, 4, 1, 1, 2, false, 0>", "conv_mfma_pp_kernel<64, 4, 1, 1, 2, false, 0>",
          "conv_mfma_pp_kernel<64, 4, 1, 1, 2, false, 0>", "conv_mfma_pp_kernel<32, 4, 1, 1, 2, false, 0>",
          "conv_mfma_pp_kernel<16, 2, 1, 1, 2, false, 0>"]  # what tests/test_abi.py pins


def probe(mode):
    env = {k: v for k, v in os.environ.items() if k != "DY_CONV1X1_STREAM"}
    if mode is not None:
        env["DY_CONV1X1_STREAM"] = mode
    r = subprocess.run([sys.executable, "-c", PROBE], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


FALLBACK = ("stats_rows", "f32", "bias_silu", "wide", "cin8")


def test_force_takes_every_supported_launch_and_nothing_else():
    o = probe("force")
    for tag in ("big", "small"):
        assert o[tag + "/plain"] == o[tag + "/accum"] == "conv1x1_stream_kernel<2, 4, false>", o
        assert o[tag + "/stats_acc"] == "conv1x1_stream_kernel<2, 4, true>", o  # with sums: the instantiation on the ping-pong pixel map
        assert o[tag + "/cin16"] == "conv1x1_stream_kernel<1, 2, false>" and o[tag + "/cout48"] == "conv1x1_stream_kernel<2, 4, false>", o
        for k in FALLBACK:  # partial-row statistics, fp32 output, the fused inference epilogue, Cin > 128, 8-channel chunks
            assert o[f"{tag}/{k}"].startswith(("conv_mfma_pp_kernel<", "conv_mfma_wlds_kernel<", "conv_mfma_kernel<")), (k, o[f"{tag}/{k}"])
        assert o[tag + "/stats_rows"] == "conv_mfma_pp_kernel<64, 4, 1, 1, 2, false, 0>"
    assert o["segx"] == "conv1x1_stream_kernel<4, 4, true>" and o["segx_up"] == "conv1x1_stream_kernel<4, 4, false>", o
    assert o["segy"] == "conv1x1_stream_kernel<2, 4, false>", o
    assert o["pinned"] == PINNED


def test_zero_never_takes_it():
    o = probe("0")
    for k, v in o.items():
        if k != "pinned":
            assert isinstance(v, str) and not v.startswith("conv1x1_stream_kernel"), (k, v)
    assert o["segx"] == "conv_mfma_pp_kernel<32, 4, 1, 1, 2, false, 0>" and o["segy"] == "conv_mfma_pp_kernel<64, 4, 1, 1, 2, false, 0>"
    assert o["pinned"] == PINNED


def test_unset_applies_the_rule_and_keeps_the_pinned_names():
    o, f = probe(None), probe("force")
    for k, v in o.items():
        if k == "pinned":
            continue
        assert isinstance(v, str), (k, v)
        if v.startswith("conv1x1_stream_kernel"):  # the rule only ever picks among the launches the kernel supports
            assert v == f[k], (k, v, f[k])
    for tag in ("big", "small"):
        for k in FALLBACK:
            assert not o[f"{tag}/{k}"].startswith("conv1x1_stream_kernel"), (k, o[f"{tag}/{k}"])
    # the rule itself: launches of at least 8192 pixels (DY_STREAM_MIN_PIX) take the stream kernel, smaller ones keep the ping-pong kernel
    for k in ("big/plain", "big/accum", "big/stats_acc", "big/cin16", "big/cout48", "segx", "segx_up", "segy"):
        assert o[k] == f[k] and o[k].startswith("conv1x1_stream_kernel<"), (k, o[k])
    for k in ("small/plain", "small/accum", "small/stats_acc"):  # 1600 pixels
        assert o[k] == "conv_mfma_pp_kernel<64, 4, 1, 1, 2, false, 0>", (k, o[k])
    assert o["pinned"] == PINNED
