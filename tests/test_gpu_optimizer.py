"""-m gpu: the flat optimizer step (csrc/optim.hip) as the trainer calls it -- dy_optimizer_step_seg over the six-segment layout with
the frozen mask, the EMA of parameters and buffers and the GradScaler bookkeeping -- against torch.optim on the CPU in float64.

Inputs are drawn in float32, so both sides see identical values.  The tolerance is not fixed in advance: the same torch.optim run in
float32 on the CPU gives e32, its worst ``relerr`` against the float64 run over parameters and EMA; the kernel's error against
float64 must stay below FACTOR * max(e32, ULP).  FACTOR = 8 allows the GPU's powf / sqrtf / division to differ from the host's by a
few ulp per step; ULP = 1.2e-7 is one fp32 ulp, the floor of the measure."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from conftest import CFG_DIR
from gpu_util import relerr
from oracle import graph as og

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ["SGD", "Adam", "AdamW", "RMSProp", "RAdam", "Adamax", "NAdam"]
MOM, BETA2, EPS, MAX_NORM = 0.9, 0.999, 1e-8, 10.0
ULP, FACTOR = 1.2e-7, 8.0
DY_ERR_ARG = -1


def _f32(x):
    return float(np.float32(x))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    torch.cuda.synchronize()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _make_opt(name, groups):
    """Built like the reference's build_optimizer (engine/trainer.py:1146-1180): betas = (momentum, 0.999); lr and weight decay
    come from the parameter groups."""
    lr = groups[0]["lr"]
    return {"SGD": lambda: torch.optim.SGD(groups, lr=lr, momentum=MOM, nesterov=True),
            "Adam": lambda: torch.optim.Adam(groups, lr=lr, betas=(MOM, BETA2)),
            "AdamW": lambda: torch.optim.AdamW(groups, lr=lr, betas=(MOM, BETA2)),
            "RMSProp": lambda: torch.optim.RMSprop(groups, lr=lr, momentum=MOM),
            "RAdam": lambda: torch.optim.RAdam(groups, lr=lr, betas=(MOM, BETA2)),
            "Adamax": lambda: torch.optim.Adamax(groups, lr=lr, betas=(MOM, BETA2)),
            "NAdam": lambda: torch.optim.NAdam(groups, lr=lr, betas=(MOM, BETA2))}[name]()


def _chunks(n, ends, frozen):
    """Maximal runs of trainable elements inside one segment, as (start, end, optimizer group): segment k holds group k % 3."""
    seg = np.searchsorted(np.asarray(ends), np.arange(n), side="right")
    key = seg * 2 + frozen
    cuts = [0] + (np.flatnonzero(np.diff(key)) + 1).tolist() + [n]
    return [(s, e, int(seg[s]) % 3) for s, e in zip(cuts[:-1], cuts[1:]) if not frozen[s]]


class _Ref:
    """torch.optim on the CPU in ``dtype``: one leaf tensor per trainable chunk, each in the parameter group of its segment, plus the
    EMA of ALL elements (frozen ones included) and of the buffers."""

    def __init__(self, name, p0, chunks, lrs, wds, dtype, ema_b0=None):
        self.dtype, self.chunks = dtype, chunks
        self.full = p0.detach().cpu().to(dtype).clone()
        self.leaves = [self.full[s:e].clone().requires_grad_(True) for s, e, _ in chunks]
        groups = [dict(params=[q for q, c in zip(self.leaves, chunks) if c[2] == k], lr=lrs[k], weight_decay=wds[k]) for k in range(3)]
        self.opt = _make_opt(name, groups)
        self.ema = self.full.clone()
        self.ema_b = None if ema_b0 is None else ema_b0.detach().cpu().to(dtype).clone()

    def step(self, grad, d, buf=None):
        """``grad``: the unscaled fp32 gradient, or None for a non-finite step (GradScaler.step does not call optimizer.step then).
        Returns (total norm, clip coefficient) of a clean step."""
        norm = coef = None
        if grad is not None:
            for q, (s, e, _) in zip(self.leaves, self.chunks):
                q.grad = grad[s:e].to(self.dtype, copy=True)  # (clip_grad_norm_ scales it in place)
            norm = float(torch.nn.utils.clip_grad_norm_(self.leaves, MAX_NORM))
            coef = min(1.0, MAX_NORM / (norm + 1e-6))
            self.opt.step()
            with torch.no_grad():
                for q, (s, e, _) in zip(self.leaves, self.chunks):
                    self.full[s:e] = q
        self.ema = d * self.ema + (1 - d) * self.full  # ModelEMA.update runs whether or not the step was skipped
        if buf is not None:
            self.ema_b = d * self.ema_b + (1 - d) * buf.to(self.dtype)
        return norm, coef

    def mu_product(self):
        # (torch.optim.NAdam keeps this scalar in the DEFAULT dtype, float32, whatever the parameters' dtype: as a reference for
        # state[7] it is good to about 1e-7 per step taken, which the 1e-6 of the comparison allows for and a tighter one would not)
        return float(self.opt.state[self.leaves[0]]["mu_product"])


def _references(name, p0, chunks, lrs, wds, grads, decays, bufs, ema_b0):
    """The float64 run (per step: parameters, EMA, buffer EMA, norm, clip coefficient, NAdam mu product) and e32, the worst
    ``relerr`` of the same run in float32 against it over parameters and EMA."""
    runs = {}
    for dtype in (torch.float64, torch.float32):
        ref, out = _Ref(name, p0, chunks, lrs, wds, dtype, ema_b0), []
        for g, d, b in zip(grads, decays, bufs):
            norm, coef = ref.step(g if g is not None and bool(torch.isfinite(g).all()) else None, d, b)
            out.append(dict(p=ref.full.clone(), ema=ref.ema.clone(), ema_b=None if ref.ema_b is None else ref.ema_b.clone(), norm=norm,
                            coef=coef, mu=ref.mu_product() if name == "NAdam" and ref.opt.state else None))
        runs[dtype] = out
    e32 = max(max(relerr(b["p"], a["p"]), relerr(b["ema"], a["ema"])) for a, b in zip(runs[torch.float64], runs[torch.float32]))
    return runs[torch.float64], e32


class _Scaler:
    """torch.amp.GradScaler's policy in plain Python (growth 2, backoff 0.5, interval 2000) plus the counters the kernel keeps beside it.
    ``dynamic`` False (amp=False): the scale is a constant; a non-finite step is still skipped and counted."""

    def __init__(self, scale, tracker=0, dynamic=True):
        self.scale, self.tracker, self.dynamic, self.taken, self.skipped = float(scale), int(tracker), dynamic, 0, 0

    def update(self, found_inf):
        if found_inf:
            self.skipped += 1
            self.tracker = 0
            if self.dynamic:
                self.scale *= 0.5
        else:
            self.taken += 1
            self.tracker += 1
            if self.dynamic and self.tracker == 2000:
                self.scale *= 2.0
                self.tracker = 0

    def state(self):
        return [self.scale, float(self.tracker), float(self.taken), float(self.skipped)]


class _Flat:
    """The device side of a step as StepPlan keeps it: flat parameters, moments, EMA, frozen mask, hyper[], state[], partials."""

    def __init__(self, name, p0, ends, frozen, scale, n_buf=0, seed=0):
        from ultralytics.hip import lib
        self.L, self.mode, self.n = lib(), MODES.index(name), p0.numel()
        g = torch.Generator().manual_seed(1000 + seed)
        self.p = p0.clone().to(DEV)
        self.ema = p0.clone().to(DEV)
        # NOT zeros: the kernels promise that the first step taken does not read the moments (the ``first`` guards)
        self.m = torch.randn(self.n, generator=g).to(DEV)
        self.v = (torch.rand(self.n, generator=g) + 0.5).to(DEV)
        self.frozen = None if frozen is None else torch.from_numpy(frozen.astype(np.uint8)).to(DEV)
        self.ends = (C.c_long * 5)(*ends)
        self.hyper = torch.zeros(16, device=DEV)
        self.state = torch.zeros(8, device=DEV)
        self.state[0] = scale
        self.partials = torch.zeros(4096, device=DEV)
        self.n_buf = n_buf
        self.buf = torch.zeros(max(n_buf, 8), device=DEV)
        self.ema_b = torch.zeros(max(n_buf, 8), device=DEV)
        self.host = (C.c_float * 16)()

    def set_hyper(self, lrs, wds, d, dynamic=1.0):
        from ultralytics.hip import check
        for i, v in enumerate([*lrs, MOM, *wds, d, MAX_NORM, BETA2, EPS, dynamic]):
            self.host[i] = v
        check(self.L.dy_set_hyper(self.hyper.data_ptr(), self.host, _stream()), "dy_set_hyper")

    def call(self, grad, n=None, ends=None, mode=None, v="own"):
        v = (self.v.data_ptr() if self.mode else None) if v == "own" else v
        return self.L.dy_optimizer_step_seg(self.p.data_ptr(), grad.data_ptr(), self.m.data_ptr(), v, self.ema.data_ptr(),
                                            self.n if n is None else n, self.ends if ends is None else ends,
                                            None if self.frozen is None else self.frozen.data_ptr(), self.buf.data_ptr(), self.ema_b.data_ptr(),
                                            self.n_buf, self.hyper.data_ptr(), self.state.data_ptr(), self.partials.data_ptr(),
                                            self.mode if mode is None else mode, _stream())

    def step(self, grad):
        from ultralytics.hip import check
        gd = grad.to(DEV)
        check(self.call(gd), "dy_optimizer_step_seg")
        _sync()
        return self.state.cpu().tolist()


def _run_schedule(name, n, ends, frozen_ranges, amps, bad, n_buf, seed):
    """``len(amps)`` steps of mode ``name`` over the layout (n, ends, frozen_ranges): Gaussian gradients of standard deviation amps[k],
    zero under the mask, with one non-finite value at a trainable index in the steps of ``bad``.  Every assertion of the module
    docstring's bound after every step; returns (e32, worst kernel error)."""
    gen = torch.Generator().manual_seed(seed)
    frozen = np.zeros(n, dtype=np.int64)
    for s, e in frozen_ranges:
        frozen[s:e] = 1
    fr = torch.from_numpy(frozen.astype(bool))
    chunks = _chunks(n, ends, frozen)
    assert {c[2] for c in chunks} == {0, 1, 2} and sum(e - s for s, e, _ in chunks) == n - int(frozen.sum())
    lrs, wds, d, scale0 = [_f32(0.02), _f32(0.01), _f32(0.005)], [0.0, _f32(0.05), _f32(0.01)], _f32(0.37), 8.0
    p0 = torch.randn(n, generator=gen)
    grads, bufs = [], []
    buf0 = torch.randn(n_buf, generator=gen)
    for k, amp in enumerate(amps):
        g = torch.randn(n, generator=gen) * amp
        g[fr] = 0.0  # the runtime keeps the flat gradient exactly zero under the mask (tests/test_gpu_freeze.py)
        if k in bad:
            idx, val = bad[k]
            assert not frozen[idx]
            g[idx] = val
        grads.append(g)
        bufs.append(buf0 + 0.1 * (k + 1) * torch.randn(n_buf, generator=gen))  # running statistics move every step
    ref, e32 = _references(name, p0, chunks, lrs, wds, grads, [d] * len(amps), bufs, buf0)
    # measured on the MI355X, kernel error (e32) -- n = 4001, ten steps: SGD 1.75e-7 (1.75e-7), Adam 1.23e-7 (1.22e-7), AdamW 3.00e-7
    # (3.00e-7), RMSProp 1.62e-7 (1.80e-7), RAdam 2.21e-7 (1.34e-7), Adamax 1.75e-7 (1.75e-7), NAdam 2.03e-7 (1.90e-7);
    # n = 525065, three steps: SGD 1.48e-7 (1.48e-7), AdamW 2.03e-7 (2.03e-7)
    bound = FACTOR * max(e32, ULP)

    dev = _Flat(name, p0, ends, frozen, scale0, n_buf, seed)
    dev.ema_b.copy_(buf0)
    m0, v0 = dev.m.cpu().clone(), dev.v.cpu().clone()
    dev.set_hyper(lrs, wds, d)
    sc, worst, clipped = _Scaler(scale0), 0.0, []
    for k, (g, r) in enumerate(zip(grads, ref)):
        dev.buf.copy_(bufs[k])
        st = dev.step(g * sc.scale)  # a power of two: the kernel's unscale gives back g's bits
        is_bad = k in bad
        sc.update(is_bad)
        p, ema = dev.p.cpu(), dev.ema.cpu()
        err = max(relerr(p, r["p"]), relerr(ema, r["ema"]), relerr(dev.ema_b.cpu(), r["ema_b"]))
        worst = max(worst, err)
        assert err < bound, (name, k, err, e32)
        assert _same_bits(p[fr], p0[fr]) and _same_bits(dev.m.cpu()[fr], m0[fr]) and _same_bits(dev.v.cpu()[fr], v0[fr]), (name, k)
        # a frozen element's EMA started equal to the parameter, which never moves: fl(fl(d e) + fl((1 - d) p)) keeps it within
        # 1.5 ulp / (1 - d) = 2.4 ulp of the parameter however many steps run
        assert bool(((ema[fr] - p0[fr]).abs() <= 4 * ULP * p0[fr].abs()).all()), (name, k)
        assert st[2] == (1.0 if is_bad else 0.0), (name, k, st)
        if not is_bad:
            assert abs(st[3] - r["norm"]) < 1e-6 * r["norm"], (name, k, st[3], r["norm"])
            assert abs(st[4] - r["coef"]) < 1e-6 * r["coef"] and (st[4] == 1.0) == (r["coef"] == 1.0), (name, k, st[4], r["coef"])
        if st[4] < 1.0:
            clipped.append(k)
        assert [st[0], st[1], st[5], st[6]] == sc.state(), (name, k, st)
        if name == "NAdam" and r["mu"] is not None:
            assert abs(st[7] - r["mu"]) < 1e-6 * r["mu"], (k, st[7], r["mu"])
    print(f"{name}: n {n}  e32 {e32:.3e}  kernel {worst:.3e}  bound {bound:.3e}")
    return e32, worst, clipped, st


@pytest.mark.parametrize("name", MODES)
def test_seg_step_all_modes_vs_torch_optim(name):
    """Ten steps of every mode in the production shape of the call: six segments (one empty, no boundary a multiple of 8), three
    learning rates and weight decays, a frozen range and frozen padding, EMA of parameters and of 70001 buffer floats (above one pass
    of ema_buffers_kernel), the clip engaging at step 2, an inf at step 0 and a nan at step 4 (both skipped: Adam's clock stops, the
    EMA moves, the scale halves)."""
    n, ends = 4001, (300, 1500, 1500, 1723, 3601)
    assert all(e % 8 for e in ends)
    amps = [0.1] * 10
    amps[2] = 0.6
    e32, worst, clipped, st = _run_schedule(name, n, ends, [(296, 300), (1723, 2500)], amps, {0: (777, float("inf")), 4: (3001, float("nan"))},
                                            70001, MODES.index(name))
    assert clipped == [2]
    assert st[5] == 8.0 and st[6] == 2.0 and st[0] == 8.0 * 0.5 * 0.5


@pytest.mark.parametrize("name", ["SGD", "AdamW"])
def test_seg_step_beyond_the_block_cap(name):
    """n = 2 * 262144 + 777: the launch is capped at 1024 blocks of 256 threads, so every thread strides (three times for the first
    777); two segment boundaries and a frozen range lie beyond the first pass.  ``partials`` holds 4096 floats as in StepPlan: the
    capped grid writes 2048 of them."""
    n, ends = 2 * 262144 + 777, (1003, 150001, 250005, 300007, 412345)
    assert all(e % 8 for e in ends) and sum(e > 262144 for e in ends) == 2
    e32, worst, clipped, st = _run_schedule(name, n, ends, [(262000, 262300), (412341, 412345)], [0.01, 0.03, 0.01], {}, 1001, 20 + MODES.index(name))
    assert clipped == [1]
    assert st[5] == 3.0 and st[6] == 0.0 and st[0] == 8.0


@pytest.mark.parametrize("name", ["SGD", "AdamW"])
def test_loss_scale_policy_is_gradscalers(name):
    """state[0], [1], [5], [6] EQUAL a plain-Python GradScaler (growth 2, backoff 0.5, interval 2000) step by step; a skipped step
    leaves the bits of p, m and v alone and still moves the EMA; hyper[11] = 0 (amp=False) holds the scale, up and down."""
    n, ends = 1003, (101, 333, 333, 500, 901)
    gen = torch.Generator().manual_seed(77)
    p0 = torch.randn(n, generator=gen)
    lrs, wds, d = [0.02, 0.01, 0.005], [0.0, 0.05, 0.01], _f32(0.37)
    dev = _Flat(name, p0, ends, None, 8.0)
    dev.ema.add_(1.0)  # away from the parameters, so that a moving EMA shows
    dev.state[1] = 1998.0
    sc = _Scaler(8.0, 1998)
    clean = lambda: torch.randn(n, generator=gen) * 0.1  # noqa: E731

    def bad(val):
        g = clean()
        g[517] = val
        return g

    def step(g, found, dynamic):
        dev.set_hyper(lrs, wds, d, 1.0 if dynamic else 0.0)
        sc.dynamic = dynamic
        before = [t.cpu().clone() for t in (dev.p, dev.m, dev.v, dev.ema)]
        st = dev.step(g * sc.scale)
        sc.update(found)
        assert st[2] == float(found)
        assert [st[0], st[1], st[5], st[6]] == sc.state(), (st, sc.state())
        p, m, v, ema = [t.cpu() for t in (dev.p, dev.m, dev.v, dev.ema)]
        if found:
            assert _same_bits(p, before[0]) and _same_bits(m, before[1]) and _same_bits(v, before[2])
        else:
            assert not _same_bits(p, before[0])
        # (1 - d, the two products and the sum each round once, by half an ulp of a value no larger than the largest: 2 ulp)
        want = d * before[3].double() + (1 - d) * p.double()
        assert relerr(ema, want) < 2 * ULP and not _same_bits(ema, before[3])
        return st

    assert step(clean(), False, True)[0:2] == [8.0, 1999.0]
    assert step(clean(), False, True)[0:2] == [16.0, 0.0]  # 2000 clean steps in a row: the scale doubles, the tracker restarts
    assert step(clean(), False, True)[0:2] == [16.0, 1.0]
    assert step(bad(float("inf")), True, True)[0:2] == [8.0, 0.0]
    assert step(bad(float("nan")), True, False)[0:2] == [8.0, 0.0]  # amp=False: skipped and counted, the scale stays
    dev.state[1] = 1999.0
    sc.tracker = 1999
    st = step(clean(), False, False)  # ... and never grows
    assert st[0] == 8.0 and [st[5], st[6]] == [4.0, 2.0]


def test_seg_step_argument_checks_write_nothing():
    """Every DY_ERR_ARG of dy_optimizer_step_seg returns before a launch: parameters, moments, EMA and state keep their bits."""
    n, ends = 1003, (101, 333, 333, 500, 901)
    gen = torch.Generator().manual_seed(78)
    p0 = torch.randn(n, generator=gen)
    dev = _Flat("AdamW", p0, ends, None, 8.0)
    dev.set_hyper([0.02, 0.01, 0.005], [0.0, 0.05, 0.01], 0.37)
    g = (torch.randn(n, generator=gen) * 0.8).to(DEV)
    L5 = C.c_long * 5
    _sync()
    keep = [t.cpu().clone() for t in (dev.p, dev.m, dev.v, dev.ema, dev.state, dev.ema_b)]
    cases = dict(null_ends=dict(ends=C.cast(None, C.POINTER(C.c_long))), decreasing=dict(ends=L5(101, 333, 332, 500, 901)),
                 first_negative=dict(ends=L5(-1, 333, 333, 500, 901)), above_n=dict(ends=L5(101, 333, 333, 500, n + 1)),
                 n_zero=dict(n=0, ends=L5(0, 0, 0, 0, 0)), mode_7=dict(mode=7), mode_negative=dict(mode=-1), null_v=dict(mode=1, v=None),
                 null_v_nadam=dict(mode=6, v=None))
    for tag, kw in cases.items():
        assert dev.call(g, **kw) == DY_ERR_ARG, tag
        _sync()
        for a, b in zip((dev.p, dev.m, dev.v, dev.ema, dev.state, dev.ema_b), keep):
            assert _same_bits(a, b), tag
    assert dev.call(g, ends=L5(101, 333, 333, 500, n)) == 0  # an end AT n is a legal (empty last segment) layout
    _sync()
    assert not _same_bits(dev.p, keep[0]) and float(dev.state[5]) == 1.0


def test_set_hyper_delivers_the_values_of_its_own_call():
    """dy_set_hyper copies the 16 floats at enqueue time: two calls queued behind other work from ONE host array that is overwritten
    in between (and after) deliver each call's own values bit for bit.  An event recorded behind each call shows that its kernel had
    NOT run yet when the host array was overwritten (the queue of work in front is lengthened until that holds), so a copy read from
    the host array when the kernel runs would deliver the later values."""
    from ultralytics.hip import lib
    L = lib()
    gen = torch.Generator().manual_seed(79)
    a, b = torch.randn(16, generator=gen), torch.randn(16, generator=gen)
    a[5], b[2] = 1e-38 * 0.01, -0.0  # a denormal and a negative zero travel too
    assert len(set(_bits(a).tolist())) == 16
    host = (C.c_float * 16)()
    va, vb, nan = a.tolist(), b.tolist(), [float("nan")] * 16
    busy = torch.randn(2048, 2048, device=DEV)
    pending = False
    for rounds in (8, 64, 512):
        da, db = torch.zeros(16, device=DEV), torch.zeros(16, device=DEV)
        ev_a, ev_b = torch.cuda.Event(), torch.cuda.Event()
        _sync()
        for _ in range(rounds):
            busy = torch.tanh(busy @ busy)  # keeps the stream occupied while the host runs ahead
        host[:] = va
        assert L.dy_set_hyper(da.data_ptr(), host, _stream()) == 0
        ev_a.record()
        host[:] = vb
        pending = not ev_a.query()
        assert L.dy_set_hyper(db.data_ptr(), host, _stream()) == 0
        ev_b.record()
        host[:] = nan
        pending = pending and not ev_b.query()
        _sync()
        assert _same_bits(da, a) and _same_bits(db, b), rounds
        if pending:
            break
    assert pending, "the stream drained before the host array was overwritten: the test did not see a queued call"
    assert L.dy_set_hyper(None, host, _stream()) == DY_ERR_ARG and L.dy_set_hyper(da.data_ptr(), None, _stream()) == DY_ERR_ARG
    _sync()
    assert _same_bits(da, a)


def test_axpy_beyond_the_block_cap():
    """dy_axpy_f32 at n = 262144 + 5 (the capped grid strides): the bits of y + 0.5 x in fp32 on the host (0.5 x is exact, so a
    fused multiply-add rounds as the two operations do); the element behind n is not touched."""
    from ultralytics.hip import lib
    n = 262144 + 5
    gen = torch.Generator().manual_seed(80)
    x, y = torch.randn(n + 1, generator=gen), torch.randn(n + 1, generator=gen)
    want = y.clone()
    want[:n] = y[:n] + 0.5 * x[:n]
    xd, yd = x.to(DEV), y.to(DEV)
    assert lib().dy_axpy_f32(yd.data_ptr(), xd.data_ptr(), 0.5, n, _stream()) == 0
    _sync()
    assert _same_bits(yd, want)


# ---- the six non-SGD optimizers through StepPlan.optimizer_step ------------------------------------------------------------

NAME = "yolov8n-ASF-P2P2"


def _model():
    """The filled model on the GPU with the '.dfl' parameters frozen, as the trainer does (engine/trainer.py: frozen_parameter_names)."""
    from ultralytics.engine.trainer import frozen_parameter_names
    from ultralytics.nn.tasks import DetectionModel
    cfg = os.path.join(CFG_DIR, NAME + ".yaml")
    m = DetectionModel(cfg, ch=3, verbose=False)
    m.load_state_dict(og.fill_state(og.state_layout(og.build_graph(og.load_yaml(cfg))), 11), strict=True)
    frozen = set(frozen_parameter_names([k for k, _ in m.named_parameters()], None))
    assert frozen
    for k, v in m.named_parameters():
        v.requires_grad = k not in frozen
    return m.cuda().train()


PLAN_STEPS, PLAN_SCALE = 3, 4.0
PLAN_LRS, PLAN_WDS = [_f32(0.02), _f32(0.01), _f32(0.005)], [0.0, _f32(0.05), 0.0]
PLAN_AMPS = [0.005, 0.02, 0.005]  # about 1e6 trainable elements: norms of about 5, 20, 5 -- the clip engages in the middle step


def _plan_inputs(n, n_buf):
    gen = torch.Generator().manual_seed(81)
    return [torch.randn(n, generator=gen) * a for a in PLAN_AMPS], [1.0 + 0.05 * torch.rand(n_buf, generator=gen) for _ in PLAN_AMPS]


def _run_plan(name, use_graph):
    """Three optimizer_step() calls on gradients written into rt.flat_g (no forward pass).  Returns the plan and what the reference
    needs: start values, per-step gradients (unscaled, zero under rt.frozen) and buffers."""
    from ultralytics.hip.train import StepPlan
    m = _model()
    plan = StepPlan(m, 2, 64, nmax=8, optimizer=name, init_scale=PLAN_SCALE, use_graph=use_graph)
    rt = plan.rt
    fr = rt.frozen.bool().cpu()
    p0, b0 = rt.flat_p.cpu().clone(), rt.flat_b.cpu().clone()
    grads, bmul = _plan_inputs(rt.n_params_flat, rt.n_buffers_flat)
    bufs = []
    for g, bm in zip(grads, bmul):
        g[fr] = 0.0
        rt.flat_g.copy_(g * PLAN_SCALE)
        rt.flat_b.mul_(bm.to(rt.flat_b.device))  # the running statistics move between steps, as a forward pass would move them
        bufs.append(rt.flat_b.cpu().clone())
        plan.set_hyper(PLAN_LRS, MOM, PLAN_WDS)
        plan.optimizer_step()
    _sync()
    return m, plan, p0, b0, grads, bufs


@pytest.mark.parametrize("name", MODES[1:])
def test_step_plan_optimizers_vs_torch_optim(name):
    """StepPlan.optimizer_step (eager) for Adam ... NAdam over the model's own flat layout, frozen mask and EMA ramp against torch.optim
    over the model's named trainable parameters, grouped by rt.param_group; bound as above."""
    m, plan, p0, b0, grads, bufs = _run_plan(name, False)
    rt = plan.rt
    chunks = [(rt.param_off[n], rt.param_off[n] + p.numel(), rt.param_group[n]) for n, p in m.named_parameters() if p.requires_grad]
    chunks.sort()
    fr = rt.frozen.bool().cpu()
    assert int(fr.sum()) + sum(e - s for s, e, _ in chunks) == rt.n_params_flat and not any(bool(fr[s:e].any()) for s, e, _ in chunks)
    decays = [0.9999 * (1 - math.exp(-k / 2000)) for k in range(1, PLAN_STEPS + 1)]
    ref, e32 = _references(name, p0, chunks, PLAN_LRS, PLAN_WDS, grads, decays, bufs, b0)
    # measured on the MI355X, worst of flat_p / ema / ema_b (e32): Adam, AdamW, RAdam, Adamax, NAdam 8.4e-8 (6.4e-8) -- the buffer EMA;
    # their parameters 1.1e-8 ... 1.7e-8 -- RMSProp 2.1e-7 (1.9e-7)
    bound = FACTOR * max(e32, ULP)
    r = ref[-1]
    errs = [relerr(rt.flat_p, r["p"]), relerr(plan.ema, r["ema"]), relerr(plan.ema_b, r["ema_b"])]
    print(f"{name}: StepPlan n {rt.n_params_flat}  e32 {e32:.3e}  kernel p {errs[0]:.3e} ema {errs[1]:.3e} ema_b {errs[2]:.3e}  bound {bound:.3e}")
    assert [q["coef"] < 1.0 for q in ref] == [False, True, False]
    assert max(errs) < bound, (name, errs, e32)
    assert _same_bits(rt.flat_p.cpu()[fr], p0[fr])
    assert plan.check_progress() == (3, 0, 4.0)
    # the model's parameters are views of the flat buffer: what the optimizer wrote is what the model holds
    n0, q0 = next((n, p) for n, p in m.named_parameters() if p.requires_grad)
    assert _same_bits(q0.detach().flatten(), rt.flat_p[rt.param_off[n0]:rt.param_off[n0] + q0.numel()])


def test_step_plan_captured_optimizer_step_equals_eager():
    """use_graph=True: the optimizer step is traced once, captured and replayed; parameters, moments, EMA and state equal the eager
    run's bit for bit."""
    _, eager, *_ = _run_plan("AdamW", False)
    want = [t.cpu().clone() for t in (eager.rt.flat_p, eager.mom, eager.adam_v, eager.ema, eager.ema_b, eager.state)]
    del eager
    _, plan, *_ = _run_plan("AdamW", True)
    assert len(plan.graph_opt) == 1
    for tag, a, b in zip(("p", "m", "v", "ema", "ema_b", "state"), (plan.rt.flat_p, plan.mom, plan.adam_v, plan.ema, plan.ema_b, plan.state), want):
        assert _same_bits(a, b), tag
    assert plan.check_progress() == (3, 0, 4.0)
