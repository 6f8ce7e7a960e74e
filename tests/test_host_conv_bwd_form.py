"""``engine.conv_bwd_form``: the one place that decides which launches make up the backward of a Conv + BatchNorm + activation.  Pure
host logic (no library, no GPU): the product of its facts under the settings of BN_ACC, BN_WGRAD, WGRAD_DGRAD and FROZEN_DGRAD that
the module can derive from the environment, against the properties the launches it selects rely on."""
import itertools

import pytest

from ultralytics.hip import DY_ACT_LEAKY, DY_ACT_SILU
from ultralytics.hip import engine as E

F = E.ConvBwdFacts
BOOLS = [f for f in F._fields if f not in ("act", "x_kind")]
DATAFLOW = BOOLS[BOOLS.index("reduced"):]        # what the backward pass found out about dY and the shortcut
STATIC = BOOLS[:BOOLS.index("reduced")]          # the facts of the layer, its input and the trace
BASE = dict(act=DY_ACT_SILU, x_kind="plain", **{k: False for k in BOOLS})
# the full product of the layer's facts (the dataflow facts at their defaults: they bear on the reduce and the shortcut only, below); the
# two kernels' answers exist where they are asked (Engine._bwd_facts: 1x1 stride 1, no LDConv, a tensor or a concatenation), else False
FACTS = [f for f in (F(*vals[:2], act, *vals[2:7], kind, *vals[7:]) for vals in itertools.product((False, True), repeat=len(STATIC))
                     for act in (DY_ACT_SILU, DY_ACT_LEAKY) for kind in ("plain", "seg", "other"))
         if (f.k1s1 and not f.ld and f.x_kind != "other") or not (f.fused_ok or f.dgrad_ok)]
# BN_ACC, BN_WGRAD, WGRAD_DGRAD, FROZEN_DGRAD on and off, as the module can derive them: BN_WGRAD needs BN_ACC, both fusions need BN_WGRAD
SWITCHES = ("BN_ACC", "BN_WGRAD", "WGRAD_DGRAD", "FROZEN_DGRAD")
SETTINGS = [(False,) * 4, (True, False, False, False)] + [(True, True, a, b) for a in (False, True) for b in (False, True)]
NO_DRAW = (E.BWD_NONE, E.BWD_DGRAD_ONLY, E.BWD_FUSED)
IN_WGRAD = (E.BWD_FUSED, E.BWD_WGRAD_BN)


@pytest.fixture(params=SETTINGS, ids=lambda p: "".join("01"[v] for v in p))
def switches(request, monkeypatch):
    for name, v in zip(SWITCHES, request.param):
        monkeypatch.setattr(E, name, v)
    return dict(zip(SWITCHES, request.param))


def test_form_of_every_combination_of_facts(switches):
    assert F._fields[2] == "act" and F._fields[8] == "x_kind" and len(FACTS) == 6 * 2 ** len(STATIC) * 3 // 8
    bn_wgrad, fused_on, dgrad_on = switches["BN_ACC"] and switches["BN_WGRAD"], switches["WGRAD_DGRAD"], switches["FROZEN_DGRAD"]
    for f in FACTS:
        form = E.conv_bwd_form(f)
        launch, draw = form.launch, form.draw
        # 1. the fused and dgrad-only forms stage no d(raw); the other launching forms do
        assert (draw == E.DRAW_NONE) == (launch in NO_DRAW), (f, form)
        # 2. off the main stream -- and with weight gradients on the side stream that a deferred reduction finishes -- never the shared scratch
        if f.branch or (f.side_wgrad and f.deferred):
            assert draw != E.DRAW_SHARED, (f, form)
        # 3. the fused form stays on the main stream
        if launch == E.BWD_FUSED:
            assert not f.branch and not f.side_wgrad and f.fused_ok and fused_on and f.x_grad and f.x_kind != "other", (f, form)
        elif launch == E.BWD_DGRAD_ONLY:  # (a frozen layer's one launch: its kernel's word, its switch, an input that takes a gradient)
            assert f.dgrad_ok and dgrad_on and f.x_grad and f.x_kind != "other" and not f.trainable, (f, form)
        # 4. a frozen layer (output not in two planes): no weight-gradient launch; an input that needs no gradient: no launch at all
        if not f.trainable and not f.planes:
            assert not form.wgrad and launch not in IN_WGRAD and (launch == E.BWD_NONE) == (not f.x_grad), (f, form)
        # 5. where the forward predicates let a layer read a concatenation or write two planes, a trainable layer's form takes them:
        #    the weight-gradient kernels with the BatchNorm backward inside (the condition those predicates once spelled out by hand)
        by_hand = bool(bn_wgrad and f.acc and f.act == DY_ACT_SILU and not f.side_wgrad and f.raw_dense)
        if f.trainable:
            assert (launch in IN_WGRAD) == by_hand and form.wgrad, (f, form)
        elif by_hand != E.conv_bwd_reads_parts(f):
            raise AssertionError((f, form))


def test_forward_predicate_is_the_trainable_layers_form(switches):
    for f in FACTS[::7]:
        assert E.conv_bwd_reads_parts(f) == (E.conv_bwd_form(f._replace(trainable=True)).launch in IN_WGRAD), f


def test_reduce_and_shortcut_of_every_combination_of_dataflow_facts(switches, monkeypatch):
    for bn_res, acc_b, whole_out, vals in itertools.product(*[(False, True)] * 3, itertools.product((False, True), repeat=len(DATAFLOW))):
        monkeypatch.setattr(E, "BN_RES", bn_res)
        f = F(**dict(BASE, trainable=True, acc=acc_b, whole_out=whole_out, **dict(zip(DATAFLOW, vals))))
        form = E.conv_bwd_form(f)
        acc = switches["BN_ACC"] and acc_b
        assert (form.shortcut == E.RES_NONE) == (not f.res_grad), (f, form)
        # a shortcut's gradient rides only on a reduce launch that runs, and then that launch is the dense accumulator one
        if form.shortcut == E.RES_RIDE:
            assert form.reduce == E.RED_ACC and bn_res and f.res_same, (f, form)
        elif f.res_grad:
            assert (form.shortcut == E.RES_ADD) == f.res_acc, (f, form)
        if not acc:
            assert form.reduce == (E.RED_3L if whole_out else E.RED_3L_ANY), (f, form)
        else:
            assert (form.reduce == E.RED_DONE) == f.reduced and form.reduce not in (E.RED_3L, E.RED_3L_ANY), (f, form)
            if form.reduce == E.RED_ROWS:
                assert f.rows and form.shortcut != E.RES_RIDE, (f, form)
