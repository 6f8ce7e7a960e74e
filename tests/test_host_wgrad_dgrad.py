"""Host side of the fused 1x1 backward (csrc/conv_wgrad.hip, dy_conv1x1_wgrad_dgrad_supported / dy_wgrad_dgrad_kernel_name): which
1x1 Conv + BatchNorm layers of the training models take weight gradient and input gradient in ONE launch at the benchmark's size
(batch 64, 640 x 640).  No GPU: the helpers only do arithmetic on the geometry."""
import ctypes as C
import os

from conftest import ROOT
from oracle import graph as og


def layers_1x1(stem, imgsz=640):
    """(name, cin, cout, map side) of every 1x1 Conv + BatchNorm of a model YAML, from the layer graph: plain Convs with k = 1, the
    cv1 / cv2 of C2f and SPPF, ScalSeq's channel-matching convs (each on its own pyramid level).  LDConv's column conv is not one."""
    g = og.build_graph(og.load_yaml(os.path.join(ROOT, "experiment-yolo_amd", "ultralytics", "cfg", "models", stem + ".yaml")))
    down, out = [], []
    for l in g.layers:
        fl = [l.f] if isinstance(l.f, int) else list(l.f)
        d = [(down[x] if x >= 0 else down[l.i + x]) if l.i else 1 for x in fl]
        if l.kind in ("Conv", "LDConv"):
            ds = d[0] * l.args["s"]
        elif l.kind == "nn.Upsample":
            ds = d[0] / l.args["scale"]
        elif l.kind == "Zoom_cat":
            ds = d[1]
        elif l.kind == "Add":
            ds = d[-1]
        else:
            ds = d[0]
        down.append(ds)
        p = f"model.{l.i}"
        if l.kind == "Conv" and l.args["k"] == 1:
            out.append((p, l.cin, l.cout, int(imgsz / ds)))
        elif l.kind == "C2f":
            c = int(l.cout * 0.5)
            out += [(p + ".cv1", l.cin, 2 * c, int(imgsz / ds)), (p + ".cv2", (2 + l.args["n"]) * c, l.cout, int(imgsz / ds))]
        elif l.kind == "SPPF":
            out += [(p + ".cv1", l.cin, l.cin // 2, int(imgsz / ds)), (p + ".cv2", l.cin // 2 * 4, l.cout, int(imgsz / ds))]
        elif l.kind == "ScalSeq":
            for j, nm in enumerate(("conv0", "conv1", "conv2")):
                if j or l.cout != l.cin[0]:
                    out.append((f"{p}.{nm}", l.cin[j], l.cout, int(imgsz / d[j])))
    return out


# the flagship model at batch 64, 640 x 640: (layer, cin, cout, map side) of the layers whose backward is one launch
FUSED_ASF = [("model.2.cv1", 32, 32, 160), ("model.2.cv2", 48, 32, 160), ("model.4.cv1", 64, 64, 80), ("model.4.cv2", 128, 64, 80),
             ("model.7.cv1", 128, 64, 40), ("model.8", 128, 64, 40), ("model.10", 64, 64, 80), ("model.12.cv1", 128, 64, 80),
             ("model.12.cv2", 96, 64, 80), ("model.13", 64, 32, 80), ("model.15", 32, 32, 160), ("model.17.cv1", 64, 32, 160),
             ("model.17.cv2", 48, 32, 160), ("model.20.cv1", 96, 64, 80), ("model.20.cv2", 96, 64, 80), ("model.24.conv1", 64, 32, 80),
             ("model.24.conv2", 128, 32, 40)]
TWO_LAUNCH_ASF = [("model.6.cv1", 128, 128, 40), ("model.6.cv2", 256, 128, 40), ("model.7.cv2", 256, 128, 40), ("model.23.cv1", 128, 128, 40),
                  ("model.23.cv2", 192, 128, 40)]


def test_which_layers_of_the_flagship_model_fuse():
    from ultralytics.hip import lib
    L = lib()
    ls = layers_1x1("yolov8n-ASF-P2P2")
    assert len(ls) == 22
    fused = [x for x in ls if L.dy_conv1x1_wgrad_dgrad_supported(64, x[3], x[3], x[1], x[2]) == 1]
    assert fused == FUSED_ASF, fused
    assert [x for x in ls if x not in fused] == TWO_LAUNCH_ASF
    # the rule behind the two lists: every 1x1 Conv + BatchNorm with (padded) Cout <= 64 fuses, nothing wider does
    for _, cin, cout, side in ls:
        assert L.dy_conv1x1_wgrad_dgrad_supported(64, side, side, cin, cout) == int((cout + 15) // 16 * 16 <= 64)
    # the LD model's 1x1 Convs follow the same rule; its LDConv column convs (9 x 16 ... gathered channels -> cout through
    # dy_conv_wgrad_ld_bn) have no fused entry point at all
    for _, cin, cout, side in layers_1x1("yolov8n-LD-P2"):
        assert L.dy_conv1x1_wgrad_dgrad_supported(64, side, side, cin, cout) == int(cout <= 64)
    from ultralytics.hip import SIGNATURES
    assert not any("wgrad_dgrad" in k and "ld" in k.split("_") for k in SIGNATURES)


def test_kernel_names_of_the_fused_launch():
    from ultralytics.hip import lib
    L, buf = lib(), C.create_string_buffer(128)

    def name(*a):
        return buf.value.decode() if L.dy_wgrad_dgrad_kernel_name(*a, buf, 128) == 0 else None
    # the instantiation is the weight-gradient kernel's for that map, with BNF 5 (one input tensor) or 7 (a concatenation)
    assert name(64, 80, 80, 64, 64, 0) == "conv_wgrad_kernel<1, 1, 4, 4, 5>"
    assert name(64, 80, 80, 96, 64, 1) == "conv_wgrad_kernel<1, 1, 3, 4, 7>"
    assert name(64, 160, 160, 48, 32, 1) == "conv_wgrad_kernel<1, 1, 3, 2, 7>"
    assert name(64, 40, 40, 128, 32, 0) == "conv_wgrad_kernel<1, 1, 4, 2, 5>"
    assert L.dy_wgrad_kernel_name_at(64, 80, 80, 64, 64, 1, 1, buf, 128) == 0 and buf.value == b"conv_wgrad_kernel<1, 1, 4, 4, 0>"  # unchanged
    assert name(64, 40, 40, 128, 128, 0) is None
    assert L.dy_wgrad_dgrad_kernel_name(64, 80, 80, 64, 64, 0, None, 128) != 0


def test_refusals():
    from ultralytics.hip import lib
    ok = lib().dy_conv1x1_wgrad_dgrad_supported
    assert ok(64, 80, 80, 64, 64) == 1
    assert ok(64, 80, 80, 64, 128) == 0 and ok(64, 80, 80, 64, 80) == 0      # K would be split over workgroups
    assert ok(64, 80, 80, 64, 24) == 0 and ok(64, 80, 80, 64, 8) == 0        # the BatchNorm forms want whole 16-channel tiles
    assert ok(64, 80, 80, 12, 64) == 0 and ok(64, 80, 80, 3, 16) == 0        # dX leaves in 8-channel pieces
    assert ok(0, 80, 80, 64, 64) == 0 and ok(64, 0, 80, 64, 64) == 0 and ok(64, 80, -1, 64, 64) == 0
    assert ok(64, 80, 80, 0, 64) == 0 and ok(64, 80, 80, 64, 0) == 0
    # a small map: wgrad_geometry gives a workgroup a (32, 32) block of the 64 x 64 weights, so no workgroup sees all of d(raw)'s
    # channels -- two launches (the step never runs this: its smallest 1x1 map has 64 * 40 * 40 pixels)
    assert ok(1, 20, 20, 64, 64) == 0
    assert ok(64, 80, 80, 256, 64) == 1 and ok(64, 160, 160, 16, 16) == 1 and ok(64, 80, 80, 64, 48) == 1
