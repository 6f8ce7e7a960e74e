"""-m gpu: the BatchNorm + activation kernels for ANY channel count (csrc/bn_act.hip: dy_bn_finalize_ld, dy_bn_act_apply_c,
dy_bn_act_bwd_reduce_c, dy_bn_bwd_finalize_ld, dy_bn_act_bwd_apply_c) through their C entry points.

One tensor set per C in {1, 5, 12, 37, 40, 100}, on 2x3x5 pixels (one workgroup, a ragged last block) and 2x24x20 pixels (several
partial rows).  The tensors are round8(C) wide; the pad lanes of the last 8-channel granule of every tensor a kernel READS (the raw
conv output, the output gradient, the residual operand) hold NaN, and every buffer a kernel writes is pre-filled with NaN.

Reference = the entry points that existed before (dy_bn_act_apply, dy_bn_act_bwd_reduce, dy_bn_bwd_finalize, dy_bn_act_bwd_apply,
dy_bn_finalize) run at width round8(C) on a copy of the same data whose pad channels are zero and whose per-channel vectors are
padded with gamma 1 / beta 0 / mean 0 / var 1.  Every per-channel result is a function of that channel's column alone, and which
pixels a lane visits, in which order, is a function of the physical width only -- the same for both -- so the comparison is BIT
EQUALITY on every element of every real channel; no comparison here needs the float64 fall-back bound.  (The old kernels themselves
are held to float64 references by tests/test_gpu_kernels.py.)  The old dy_bn_finalize takes any C with rows C floats wide, so its
reference is the partial table compacted to [P][2][C].

Besides: pad lanes of every written tensor (y, d(raw)) are +0.0 bit patterns, nothing written holds a NaN, the partial columns and
per-channel vectors behind C are untouched (canaries), two runs give the same bits, and C = 48 / 64 through the new entry points give
the bits of the old ones."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = [1, 5, 12, 37, 40, 100]
MAPS = {"2x3x5": 2 * 3 * 5, "2x24x20": 2 * 24 * 20}
ACTS = {"silu": 1, "none": 0, "leaky": 2}
EPS, MOM = 1e-3, 0.03
CANARY = -777.0


@pytest.fixture(scope="module")
def L():
    from ultralytics.hip import DY_ACT_LEAKY, DY_ACT_NONE, DY_ACT_SILU
    from ultralytics.hip.engine import Engine
    ACTS["silu"], ACTS["none"], ACTS["leaky"] = DY_ACT_SILU, DY_ACT_NONE, DY_ACT_LEAKY
    return Engine("cuda:0").L


def _s():
    return torch.cuda.current_stream().cuda_stream


def r8(c):
    return (c + 7) // 8 * 8


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.fixture(scope="module")
def sets():
    """{(C, npix)}: the shared inputs, made once and never written.  *_p: pad lanes NaN (what the new entry points read);
    *_z: pad lanes zero (the reference's copy)."""
    out = {}
    for Cc in WIDTHS + [48, 64]:
        for npix in MAPS.values():
            g = torch.Generator().manual_seed(1000 * Cc + npix)
            Cp = r8(Cc)
            d = {}
            for k, scale in (("x", 2.0), ("dy", 0.5), ("res", 1.0)):
                v = (torch.randn(npix, Cc, generator=g) * scale).half()
                z = torch.zeros(npix, Cp, dtype=torch.float16)
                z[:, :Cc] = v
                p = z.clone()
                p[:, Cc:] = float("nan")
                d[k + "_z"], d[k + "_p"] = z.cuda(), p.cuda()
            vec = dict(gamma=torch.rand(Cc, generator=g) + 0.5, beta=torch.randn(Cc, generator=g) * 0.3,
                       mean=torch.randn(Cc, generator=g) * 0.5, var=torch.rand(Cc, generator=g) * 3 + 0.2)
            fill = dict(gamma=1.0, beta=0.0, mean=0.0, var=1.0)
            for k, v in vec.items():
                d[k] = v.float().cuda()
                pz = torch.full((Cp,), fill[k])
                pz[:Cc] = v
                d[k + "_z"] = pz.float().cuda()
            out[(Cc, npix)] = d
    return out


def _coef(L, d, Cc, padded):
    """[4][C] coefficient table from (gamma, beta, mean, var) by dy_bn_eval_coef: stride C, or stride round8(C) from the padded vectors."""
    n = r8(Cc) if padded else Cc
    sfx = "_z" if padded else ""
    coef = torch.full((4 * n + 8,), CANARY, dtype=torch.float32, device="cuda")
    assert L.dy_bn_eval_coef(d["gamma" + sfx].data_ptr(), d["beta" + sfx].data_ptr(), d["mean" + sfx].data_ptr(), d["var" + sfx].data_ptr(),
                             coef.data_ptr(), n, EPS, _s()) == 0
    return coef


def _nan16(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float16, device="cuda")


def _apply_new(L, d, Cc, npix, act, res):
    Cp = r8(Cc)
    y = _nan16(npix, Cp)
    coef = _coef(L, d, Cc, False)
    assert L.dy_bn_act_apply_c(d["x_p"].data_ptr(), Cp, d["res_p"].data_ptr() if res else 0, Cp if res else 0, y.data_ptr(), Cp,
                               coef.data_ptr(), npix, Cc, act, _s()) == 0
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("mp", list(MAPS))
@pytest.mark.parametrize("Cc", WIDTHS)
def test_apply(L, sets, Cc, mp, act, res):
    npix, Cp, a = MAPS[mp], r8(Cc), ACTS[act]
    d = sets[(Cc, npix)]
    y = _apply_new(L, d, Cc, npix, a, res)
    ref = _nan16(npix, Cp)
    coef = _coef(L, d, Cc, True)
    assert L.dy_bn_act_apply(d["x_z"].data_ptr(), Cp, d["res_z"].data_ptr() if res else 0, Cp if res else 0, ref.data_ptr(), Cp,
                             coef.data_ptr(), npix, Cp, a, _s()) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(y).any(), "a NaN reached the output"
    assert torch.equal(bits(y[:, :Cc]), bits(ref[:, :Cc])), "real channels differ from the old entry point's bits"
    assert not bool((bits(y[:, Cc:]) != 0).any()), "pad lanes of y are not +0.0"
    assert torch.equal(bits(y), bits(_apply_new(L, d, Cc, npix, a, res))), "two runs differ"


def _bwd_sums_new(L, d, Cc, npix, act):
    Cp = r8(Cc)
    coef = _coef(L, d, Cc, False)
    part = torch.full((2048 * 2 * Cp,), float("nan"), dtype=torch.float32, device="cuda")
    n = C.c_int(0)
    assert L.dy_bn_act_bwd_reduce_c(d["dy_p"].data_ptr(), Cp, d["x_p"].data_ptr(), Cp, coef.data_ptr(), part.data_ptr(), 2048, npix, Cc, act,
                                    C.byref(n), _s()) == 0
    dg = torch.full((Cc + 8,), CANARY, dtype=torch.float32, device="cuda")
    db, bw = dg.clone(), torch.full((2 * Cc + 8,), CANARY, dtype=torch.float32, device="cuda")
    assert L.dy_bn_bwd_finalize_ld(part.data_ptr(), n.value, Cp, dg.data_ptr(), db.data_ptr(), bw.data_ptr(), Cc, float(npix), 0, _s()) == 0
    torch.cuda.synchronize()
    return part[:n.value * 2 * Cp].view(n.value, 2, Cp), dg, db, bw, coef, n.value


def _bwd_sums_ref(L, d, Cc, npix, act):
    Cp = r8(Cc)
    coef = _coef(L, d, Cc, True)
    part = torch.full((2048 * 2 * Cp,), float("nan"), dtype=torch.float32, device="cuda")
    n = C.c_int(0)
    assert L.dy_bn_act_bwd_reduce(d["dy_z"].data_ptr(), Cp, d["x_z"].data_ptr(), Cp, coef.data_ptr(), part.data_ptr(), 2048, npix, Cp, act,
                                  C.byref(n), _s()) == 0
    dg = torch.zeros(Cp, dtype=torch.float32, device="cuda")
    db, bw = dg.clone(), torch.zeros(2 * Cp, dtype=torch.float32, device="cuda")
    assert L.dy_bn_bwd_finalize(part.data_ptr(), n.value, dg.data_ptr(), db.data_ptr(), bw.data_ptr(), Cp, float(npix), 0, _s()) == 0
    torch.cuda.synchronize()
    return part[:n.value * 2 * Cp].view(n.value, 2, Cp), dg, db, bw, coef, n.value


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("mp", list(MAPS))
@pytest.mark.parametrize("Cc", WIDTHS)
def test_backward_reduce_finalize(L, sets, Cc, mp, act):
    npix, Cp, a = MAPS[mp], r8(Cc), ACTS[act]
    d = sets[(Cc, npix)]
    part, dg, db, bw, _, n = _bwd_sums_new(L, d, Cc, npix, a)
    rpart, rdg, rdb, rbw, _, rn = _bwd_sums_ref(L, d, Cc, npix, a)
    assert n == rn and (n == 1 if mp == "2x3x5" else (n > 1 or Cc < 37)), n  # (narrow tensors: 256 / cpp pixels per trip, one block)
    assert not torch.isnan(part[:, :, :Cc]).any() and not torch.isnan(torch.cat([dg[:Cc], db[:Cc], bw[:2 * Cc]])).any()
    assert torch.equal(bits(part[:, :, :Cc]), bits(rpart[:, :, :Cc])), "partial sums"
    assert torch.isnan(part[:, :, Cc:]).all(), "a partial column behind C was written"
    assert torch.equal(bits(dg[:Cc]), bits(rdg[:Cc])) and torch.equal(bits(db[:Cc]), bits(rdb[:Cc])), "dgamma / dbeta"
    assert torch.equal(bits(bw[:Cc]), bits(rbw[:Cc])) and torch.equal(bits(bw[Cc:2 * Cc]), bits(rbw[Cp:Cp + Cc])), "mean(g), mean(g xhat)"
    assert bool((dg[Cc:] == CANARY).all() and (db[Cc:] == CANARY).all() and (bw[2 * Cc:] == CANARY).all()), "a vector was written behind C"
    part2, dg2, db2, bw2, _, _ = _bwd_sums_new(L, d, Cc, npix, a)
    assert torch.equal(bits(part2[:, :, :Cc]), bits(part[:, :, :Cc])) and torch.equal(bits(dg2), bits(dg)) and torch.equal(bits(bw2), bits(bw))


def _bwd_apply_new(L, d, Cc, npix, act, coef, bw, frozen=0):
    Cp = r8(Cc)
    dx = _nan16(npix, Cp)
    assert L.dy_bn_act_bwd_apply_c(d["dy_p"].data_ptr(), Cp, d["x_p"].data_ptr(), Cp, dx.data_ptr(), Cp, coef.data_ptr(), bw.data_ptr(), npix, Cc,
                                   act, frozen, _s()) == 0
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("mp", list(MAPS))
@pytest.mark.parametrize("Cc", WIDTHS)
def test_backward_apply(L, sets, Cc, mp, act):
    npix, Cp, a = MAPS[mp], r8(Cc), ACTS[act]
    d = sets[(Cc, npix)]
    _, _, _, bw, coef, _ = _bwd_sums_new(L, d, Cc, npix, a)
    _, _, _, rbw, rcoef, _ = _bwd_sums_ref(L, d, Cc, npix, a)
    for frozen in (0, 1):
        dx = _bwd_apply_new(L, d, Cc, npix, a, coef, bw, frozen)
        ref = _nan16(npix, Cp)
        assert L.dy_bn_act_bwd_apply(d["dy_z"].data_ptr(), Cp, d["x_z"].data_ptr(), Cp, ref.data_ptr(), Cp, rcoef.data_ptr(), rbw.data_ptr(), npix,
                                     Cp, a, frozen, _s()) == 0
        torch.cuda.synchronize()
        assert not torch.isnan(dx).any(), "a NaN reached d(raw)"
        assert torch.equal(bits(dx[:, :Cc]), bits(ref[:, :Cc])), "real channels differ from the old entry point's bits"
        assert not bool((bits(dx[:, Cc:]) != 0).any()), "pad lanes of d(raw) are not +0.0"
        assert torch.equal(bits(dx), bits(_bwd_apply_new(L, d, Cc, npix, a, coef, bw, frozen))), "two runs differ"


@pytest.mark.parametrize("P", [1, 3, 300])
@pytest.mark.parametrize("Cc", WIDTHS)
def test_finalize_partial_stride(L, sets, Cc, P):
    """Partial rows as the convolution's DY_EPI_STATS epilogue lays them out, [P][2][round16(C)], columns behind C poisoned."""
    d = sets[(Cc, MAPS["2x3x5"])]
    ldp, count = (Cc + 15) // 16 * 16, 977.0
    g = torch.Generator().manual_seed(7 * Cc + P)
    s1 = torch.randn(P, Cc, generator=g)
    s2 = s1.abs() * 1.5 + torch.rand(P, Cc, generator=g) * 40
    tab = torch.full((P, 2, ldp), float("nan"))
    tab[:, 0, :Cc], tab[:, 1, :Cc] = s1, s2
    compact = torch.stack([s1, s2], 1).contiguous().cuda()
    tab = tab.cuda()

    def run(new):
        rm, rv = d["mean"].clone(), d["var"].clone()
        rm = torch.cat([rm, torch.full((8,), CANARY, device="cuda")])
        rv = torch.cat([rv, torch.full((8,), CANARY, device="cuda")])
        coef = torch.full((4 * Cc + 8,), CANARY, dtype=torch.float32, device="cuda")
        nbt = torch.tensor([5, 9], dtype=torch.int64, device="cuda")
        if new:
            rc = L.dy_bn_finalize_ld(tab.data_ptr(), P, ldp, d["gamma"].data_ptr(), d["beta"].data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                     coef.data_ptr(), Cc, count, EPS, MOM, 1, nbt.data_ptr(), _s())
        else:
            rc = L.dy_bn_finalize(compact.data_ptr(), P, 1.0, 0, 0, 0.0, 0, 0, 0.0, d["gamma"].data_ptr(), d["beta"].data_ptr(), rm.data_ptr(),
                                  rv.data_ptr(), coef.data_ptr(), Cc, count, EPS, MOM, 1, _s())
        assert rc == 0
        torch.cuda.synchronize()
        assert nbt.tolist() == [6 if new else 5, 9]  # the new entry counts the launch (once, whatever C), the old one has no counter
        return rm, rv, coef
    got, ref, again = run(True), run(False), run(True)
    for a, b, c in zip(got, ref, again):
        assert not torch.isnan(a).any()
        assert torch.equal(bits(a), bits(b)), "differs from dy_bn_finalize over the compacted table"
        assert torch.equal(bits(a), bits(c)), "two runs differ"
    assert bool((got[0][Cc:] == CANARY).all() and (got[1][Cc:] == CANARY).all() and (got[2][4 * Cc:] == CANARY).all())
    assert not torch.equal(got[0][:Cc], d["mean"]), "the running mean did not move"


@pytest.mark.parametrize("Cc", [48, 64])
def test_whole_granule_widths_keep_their_bits(L, sets, Cc):
    """C % 8 == 0 through the new entry points: every bit of the old ones (same tensors, no pad lane exists)."""
    npix, a = MAPS["2x24x20"], ACTS["silu"]
    d = sets[(Cc, npix)]
    y = _apply_new(L, d, Cc, npix, a, True)
    ref = _nan16(npix, Cc)
    coef = _coef(L, d, Cc, True)
    assert L.dy_bn_act_apply(d["x_z"].data_ptr(), Cc, d["res_z"].data_ptr(), Cc, ref.data_ptr(), Cc, coef.data_ptr(), npix, Cc, a, _s()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(y), bits(ref))
    part, dg, db, bw, coef, n = _bwd_sums_new(L, d, Cc, npix, a)
    rpart, rdg, rdb, rbw, rcoef, rn = _bwd_sums_ref(L, d, Cc, npix, a)
    assert n == rn and torch.equal(bits(part), bits(rpart)) and torch.equal(bits(dg[:Cc]), bits(rdg)) and torch.equal(bits(db[:Cc]), bits(rdb))
    assert torch.equal(bits(bw[:2 * Cc]), bits(rbw))
    dx = _bwd_apply_new(L, d, Cc, npix, a, coef, bw)
    ref = _nan16(npix, Cc)
    assert L.dy_bn_act_bwd_apply(d["dy_z"].data_ptr(), Cc, d["x_z"].data_ptr(), Cc, ref.data_ptr(), Cc, rcoef.data_ptr(), rbw.data_ptr(), npix, Cc,
                                 a, 0, _s()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(dx), bits(ref))


@pytest.mark.parametrize("Cc", [5, 37])
def test_backward_finalize_accumulates(L, sets, Cc):
    """accumulate = 1 (the bias gradient of a conv whose weights are shared by several calls): dgamma / dbeta are ADDED to, for the C
    real channels only, with the bits of the old entry point's sums."""
    npix, Cp, a = MAPS["2x24x20"], r8(Cc), ACTS["none"]
    d = sets[(Cc, npix)]
    part, dg, db, bw, _, n = _bwd_sums_new(L, d, Cc, npix, a)
    dg2 = torch.cat([torch.arange(Cc, dtype=torch.float32, device="cuda") * 0.25, torch.full((8,), CANARY, device="cuda")])
    db2, bw2 = dg2.clone() + 1.0, torch.full((2 * Cc + 8,), CANARY, dtype=torch.float32, device="cuda")
    db2[Cc:] = CANARY
    start_g, start_b = dg2.clone(), db2.clone()
    assert L.dy_bn_bwd_finalize_ld(part.data_ptr(), n, Cp, dg2.data_ptr(), db2.data_ptr(), bw2.data_ptr(), Cc, float(npix), 1, _s()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(dg2[:Cc]), bits(start_g[:Cc] + dg[:Cc])) and torch.equal(bits(db2[:Cc]), bits(start_b[:Cc] + db[:Cc]))
    assert torch.equal(bits(bw2), bits(bw)) and bool((dg2[Cc:] == CANARY).all() and (db2[Cc:] == CANARY).all())


def test_refusals(L):
    """Bad arguments are refused before anything is launched."""
    DY_ERR_ARG, DY_ERR_ALIGN = -1, -3
    t = torch.zeros(64, dtype=torch.float16, device="cuda")
    f = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = t.data_ptr()
    assert L.dy_bn_act_apply_c(p, 8, 0, 0, p, 8, f.data_ptr(), 1, 0, 1, _s()) == DY_ERR_ALIGN        # C < 1
    assert L.dy_bn_act_apply_c(p, 8, 0, 0, p, 8, f.data_ptr(), 1, 12, 1, _s()) == DY_ERR_ALIGN       # pitch below round8(C)
    assert L.dy_bn_act_apply_c(p, 12, 0, 0, p, 16, f.data_ptr(), 1, 12, 1, _s()) == DY_ERR_ALIGN     # pitch not a multiple of 8
    assert L.dy_bn_act_bwd_apply_c(p, 8, p, 8, p, 8, f.data_ptr(), 0, 1, 5, 1, 0, _s()) == DY_ERR_ARG  # live statistics need bwdcoef
    assert L.dy_bn_finalize_ld(f.data_ptr(), 1, 4, f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), 5, 1.0, EPS, MOM, 1,
                               0, _s()) == DY_ERR_ARG                                                   # rows narrower than C
    assert L.dy_bn_bwd_finalize_ld(f.data_ptr(), 1, 4, 0, 0, f.data_ptr(), 5, 1.0, 0, _s()) == DY_ERR_ARG
