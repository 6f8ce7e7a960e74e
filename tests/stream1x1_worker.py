"""Runs 1x1 convolutions through every form the training step launches them in and saves the results: tests/test_gpu_conv1x1_stream.py
compares the files of two processes started with DY_CONV1X1_STREAM=0 (the ping-pong kernel's 1x1 branch) and =force (the streaming
kernel, csrc/conv1x1_stream.hip); the switch is read once per process.  The (cin, cout) pairs come from the recorded launch lists of
the two training models, the hand-made cases add segmented inputs / outputs, strides, ragged pixel counts and maps large enough for a wave to walk several tiles.
usage: stream1x1_worker.py <out.pt>"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "experiment-yolo_amd")
sys.path[:0] = [ROOT, PKG, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from ultralytics.hip import DY_BN_COPIES, DY_EPI_ACCUM, DY_EPI_STATS, DY_EPI_STATS_ACC, DySegs  # noqa: E402
from ultralytics.hip.engine import ConvSpec, Engine  # noqa: E402

MODE = os.environ.get("DY_CONV1X1_STREAM")
SIZES = [(2, 7, 9), (3, 40, 40), (1, 33, 31)]  # N, H, W: 126, 4800 and 1023 pixels (none a multiple of a 64-pixel wave tile but 4800)
ORACLE = [(64, 64), (128, 64), (32, 48)]       # pairs whose inputs are saved too: the test compares them with fp32 F.conv2d


def model_pairs():
    """Every (cin, cout) a 1x1 forward or input-gradient launch of the two training models runs with, from StepPlan's launch list."""
    from oracle import graph as og
    from ultralytics.hip.train import StepPlan
    from ultralytics.nn.tasks import DetectionModel
    pairs = set()
    for stem in ("yolov8n-ASF-P2P2", "yolov8n-LD-P2"):
        cfg = os.path.join(PKG, "ultralytics", "cfg", "models", stem + ".yaml")
        g = og.build_graph(og.load_yaml(cfg))
        m = DetectionModel(cfg, verbose=False)
        m.load_state_dict(og.fill_state(og.state_layout(g), 3), strict=True)
        m.cuda().train()
        gen = torch.Generator().manual_seed(0)
        B, nb = 2, 4
        batch = dict(img=torch.rand(B, 3, 64, 64, generator=gen), batch_idx=torch.arange(B).repeat_interleave(nb).float(),
                     cls=torch.randint(0, 6, (B * nb, 1), generator=gen).float(),
                     bboxes=torch.cat([torch.rand(B * nb, 2, generator=gen) * 0.6 + 0.2, torch.rand(B * nb, 2, generator=gen) * 0.3 + 0.05], 1))
        plan = StepPlan(m, B, 64, nmax=8, init_scale=1024.0)
        plan.set_hyper([0.01] * 3, 0.9, [0.0, 5e-4, 0.0])
        plan.forward_backward(batch)
        torch.cuda.synchronize()
        for op in plan.rec_fb.ops:
            if op[0] is None:
                continue
            args, name = op[1], op[2]
            if name == "dy_conv_forward" and args[12] == 1:
                pairs.add((int(args[10]), int(args[11])))
            elif name == "dy_conv1x1_forward_segs":
                pairs.add((int(args[9]), int(args[10])))
            elif name == "dy_conv1x1_input_grad_segs":
                pairs.add((int(args[7]), int(args[8])))
        del plan, m
    return sorted(pairs)


def main(out):
    pairs = model_pairs()
    eng = Engine("cuda:0")
    L = eng.L
    res, live = {}, {}

    def stream_takes(cin, cout):  # the register plan of csrc/conv1x1_stream.hip: at most four k-steps of 16- or 32-channel chunks
        g = [C.c_int() for _ in range(8)]
        assert L.dy_conv_geometry(cin, cout, 1, 1, *[C.byref(x) for x in g]) == 0
        return g[0].value == cin and g[2].value >= 16 and g[3].value * g[6].value <= 4 and cout % 8 == 0

    def name_live(key, cin, cout, N, H, W, epi, xs=None, ys=None, expect=True):
        buf = C.create_string_buffer(128)
        assert L.dy_conv1x1_kernel_name_live(cin, cout, N, H, W, epi, xs, ys, buf, 128) == 0, key
        live[key] = buf.value.decode()
        if MODE == "force" and expect:
            assert live[key].startswith("conv1x1_stream_kernel<"), f"{key}: DY_CONV1X1_STREAM=force runs {live[key]}"
        if MODE == "0":
            assert not live[key].startswith("conv1x1_stream_kernel"), f"{key}: DY_CONV1X1_STREAM=0 runs {live[key]}"

    def spec_of(cin, cout, gen):
        w = (torch.randn(cout, cin, 1, 1, generator=gen) / cin ** 0.5).cuda()
        sp = ConvSpec("c", w, None, None, 1, 1, 0)
        eng.prepare_conv(sp)
        eng.pack(sp)
        return sp, w

    def rnd(gen, *shape):
        return torch.randn(*shape, generator=gen).half().cuda()

    # ---- every (cin, cout) of the models: plain store, accumulate onto old values, statistics; three pixel counts
    for cin, cout in pairs:
        if cin % 8 or cout % 8:
            continue
        ok = stream_takes(cin, cout)
        for N, H, W in SIZES:
            gen = torch.Generator().manual_seed(cin * 131 + cout * 7 + H)
            sp, w = spec_of(cin, cout, gen)
            ldx, ldy = cin + 8, cout + 16  # pixel strides larger than the channel counts
            x = rnd(gen, N, H, W, ldx)
            old = rnd(gen, N, H, W, ldy)
            key = f"{cin}_{cout}_{N}x{H}x{W}"

            def fwd(epi, part=0, y=None):
                y = torch.zeros(N, H, W, ldy, dtype=torch.float16, device="cuda") if y is None else y
                eng.call("dy_conv_forward", x.data_ptr(), ldx, sp.wpack.data_ptr(), 0, y.data_ptr(), ldy, part, N, H, W, cin, cout, 1, 1, 1, 0, 0,
                         epi, None)
                return y[..., :cout].contiguous()
            name_live(key + "/plain", cin, cout, N, H, W, 0, expect=ok)
            res[key + "/plain"] = fwd(0)
            name_live(key + "/accum", cin, cout, N, H, W, DY_EPI_ACCUM, expect=ok)
            res[key + "/accum"] = fwd(DY_EPI_ACCUM, 0, old.clone())
            if cout % 16 == 0:
                acc = torch.zeros(DY_BN_COPIES * 2 * cout, dtype=torch.float64, device="cuda")
                name_live(key + "/stats_y", cin, cout, N, H, W, DY_EPI_STATS | DY_EPI_STATS_ACC, expect=ok)
                res[key + "/stats_y"] = fwd(DY_EPI_STATS | DY_EPI_STATS_ACC, acc.data_ptr())
                live[key + "/stats_acc"] = live[key + "/stats_y"]
                res[key + "/stats_acc"] = acc.view(DY_BN_COPIES, 2, cout).sum(0)
            if (cin, cout) in ORACLE and (N, H, W) == SIZES[1]:
                res[f"oracle/{cin}_{cout}/x"] = x[..., :cin].contiguous()
                res[f"oracle/{cin}_{cout}/w"] = w

    # ---- segmented inputs: two and three members of 16 / 32 / 64 channels, one of them up-sampled, strides larger than the members
    keep = []

    def segs(parts, N, H, W, gen, up=None, acc=None, fill=True):
        t, end, tens = DySegs(), 0, []
        t.nseg = len(parts)
        for i, c in enumerate(parts):
            end += c
            ld = c + 8 * (i % 2)
            h, w_ = (H // 2, W // 2) if up == i else (H, W)
            buf = rnd(gen, N, h, w_, ld) if fill else torch.zeros(N, h, w_, ld, dtype=torch.float16, device="cuda")
            tens.append(buf)
            t.c_end[i], t.ld[i], t.ptr[i] = end, ld, buf.data_ptr()
            t.acc[i] = (2 if up == i else 0) if acc is None else acc[i]
        keep.append(tens)
        return t, tens

    for parts, cout, up in [((32, 32), 64, None), ((32, 32, 32), 64, None), ((16, 16, 16), 32, None), ((64, 32, 32), 64, 0), ((64, 64), 64, 1),
                            ((32, 64), 32, None), ((16, 16, 16), 48, 2), ((64, 64), 128, None)]:
        cin = sum(parts)
        for N, H, W in [(2, 6, 10), (3, 40, 40)]:
            gen = torch.Generator().manual_seed(cin + cout + H + len(parts))
            sp, _ = spec_of(cin, cout, gen)
            t, _tens = segs(parts, N, H, W, gen, up=up)
            if not L.dy_conv1x1_segs_supported(cin, cout, C.byref(t)):
                continue
            key = f"segx_{'+'.join(map(str, parts))}_{cout}_up{up}_{N}x{H}x{W}"
            for tag, epi in (("plain", 0), ("stats_y", DY_EPI_STATS | DY_EPI_STATS_ACC)):
                if epi and cout % 16:
                    continue
                acc = torch.zeros(DY_BN_COPIES * 2 * cout, dtype=torch.float64, device="cuda")
                y = torch.zeros(N, H, W, cout, dtype=torch.float16, device="cuda")
                name_live(f"{key}/{tag}", cin, cout, N, H, W, epi, xs=C.byref(t), expect=stream_takes(cin, cout))
                eng.call("dy_conv1x1_forward_segs", C.byref(t), sp.wpack.data_ptr(), 0, y.data_ptr(), cout, acc.data_ptr() if epi else 0, N, H, W,
                         cin, cout, epi)
                res[f"{key}/{tag}"] = y
                if epi:
                    live[f"{key}/stats_acc"] = live[f"{key}/{tag}"]
                    res[f"{key}/stats_acc"] = acc.view(DY_BN_COPIES, 2, cout).sum(0)

    # ---- segmented outputs (the input gradient of a 1x1 Conv over a concatenation): members stored and accumulated side by side
    for cdy, parts, accs in [(64, (32, 32), (0, 1)), (64, (32, 32, 32), (1, 0, 1)), (32, (16, 16, 16), (0, 0, 1)), (64, (64, 64), (0, 0)),
                             (48, (32, 64), (1, 1)), (128, (64, 32, 32), (1, 0, 0))]:
        ctot = sum(parts)
        for N, H, W in [(2, 7, 9), (3, 40, 40)]:
            gen = torch.Generator().manual_seed(cdy + ctot + H + len(parts))
            sp, _ = spec_of(ctot, cdy, gen)  # the layer: ctot -> cdy; its input gradient multiplies dy (cdy channels) by W^T
            dy = rnd(gen, N, H, W, cdy)
            t, tens = segs(parts, N, H, W, gen, acc=accs)
            key = f"segy_{cdy}_{'+'.join(map(str, parts))}_acc{''.join(map(str, accs))}_{N}x{H}x{W}"
            name_live(key, sp.cout_phys, ctot, N, H, W, 0, ys=C.byref(t), expect=stream_takes(sp.cout_phys, ctot))
            eng.call("dy_conv1x1_input_grad_segs", dy.data_ptr(), cdy, sp.wpack_t.data_ptr(), C.byref(t), N, H, W, sp.cout_phys, ctot)
            for i, c in enumerate(parts):
                live[f"{key}/m{i}"] = live[key]
                res[f"{key}/m{i}"] = tens[i][..., :c].contiguous()
            del live[key]

    # ---- the steady state: more wave tiles than resident waves (2048 with one cout group, 1024 per group with two), so that a wave walks 3-5
    # tiles, an odd count among them, through both register buffers, the refill two tiles ahead and the old values one tile ahead; ragged tail.
    # The tensors are too large to keep: 64 position-weighted integer sums of the fp16 bit patterns stand for each of them.
    def prints(y):
        v = y.contiguous().view(torch.int16).to(torch.int64).reshape(-1)
        idx = torch.arange(v.numel(), device=v.device)
        pad = (-v.numel()) % 64
        a = torch.nn.functional.pad(v * (idx % 65521 + 1), (0, pad)).view(64, -1).sum(1)
        b = torch.nn.functional.pad(v * (idx % 8191 + 3), (0, pad)).view(64, -1).sum(1)
        assert bool(torch.isfinite(y.float()).all()) and float(y.float().abs().max()) > 0
        return torch.cat([a, b])

    N, H, W = 11, 160, 157  # 276320 pixels: 4318 wave tiles of 64, 8636 of 32
    for cin, cout in [(64, 64), (128, 64), (64, 128), (32, 32)]:
        gen = torch.Generator().manual_seed(cin * 5 + cout)
        sp, _ = spec_of(cin, cout, gen)
        x = rnd(gen, N, H, W, cin)
        old = rnd(gen, N, H, W, cout)
        key = f"big_{cin}_{cout}_{N}x{H}x{W}"

        def fwd(epi, part=0, y=None):
            y = torch.zeros(N, H, W, cout, dtype=torch.float16, device="cuda") if y is None else y
            eng.call("dy_conv_forward", x.data_ptr(), cin, sp.wpack.data_ptr(), 0, y.data_ptr(), cout, part, N, H, W, cin, cout, 1, 1, 1, 0, 0, epi,
                     None)
            return prints(y)
        name_live(key + "/plain", cin, cout, N, H, W, 0)
        res[key + "/plain"] = fwd(0)
        name_live(key + "/accum", cin, cout, N, H, W, DY_EPI_ACCUM)
        res[key + "/accum"] = fwd(DY_EPI_ACCUM, 0, old.clone())
        acc = torch.zeros(DY_BN_COPIES * 2 * cout, dtype=torch.float64, device="cuda")
        name_live(key + "/stats_y", cin, cout, N, H, W, DY_EPI_STATS | DY_EPI_STATS_ACC)
        res[key + "/stats_y"] = fwd(DY_EPI_STATS | DY_EPI_STATS_ACC, acc.data_ptr())
        live[key + "/stats_acc"] = live[key + "/stats_y"]
        res[key + "/stats_acc"] = acc.view(DY_BN_COPIES, 2, cout).sum(0)
    for cdy, parts, accs in [(64, (32, 32, 32), (1, 0, 1)), (64, (64, 64), (0, 1))]:
        ctot = sum(parts)
        gen = torch.Generator().manual_seed(cdy + ctot + 11)
        sp, _ = spec_of(ctot, cdy, gen)
        dy = rnd(gen, N, H, W, cdy)
        t, tens = segs(parts, N, H, W, gen, acc=accs)
        key = f"big_segy_{cdy}_{'+'.join(map(str, parts))}_acc{''.join(map(str, accs))}_{N}x{H}x{W}"
        name_live(key, sp.cout_phys, ctot, N, H, W, 0, ys=C.byref(t))
        eng.call("dy_conv1x1_input_grad_segs", dy.data_ptr(), cdy, sp.wpack_t.data_ptr(), C.byref(t), N, H, W, sp.cout_phys, ctot)
        for i, c in enumerate(parts):
            live[f"{key}/m{i}"] = live[key]
            res[f"{key}/m{i}"] = prints(tens[i][..., :c])
        del live[key]
    torch.cuda.synchronize()
    torch.save({"res": {k: v.cpu() for k, v in res.items()}, "live": live, "pairs": pairs}, out)


if __name__ == "__main__":
    main(sys.argv[1])
