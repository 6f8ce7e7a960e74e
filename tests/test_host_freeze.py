"""CPU: the trainer's freeze rule (engine/trainer.py, frozen_parameter_names) against the names the reference froze
(tests/golden/freeze.npz, written by tests/golden/make_freeze_golden.py), and ``freeze`` through get_cfg."""
import pytest

from ultralytics.cfg import get_cfg
from ultralytics.engine.trainer import frozen_parameter_names

CASES = ("8", "5", "l2", "l12_20", "l26")


def _freeze_arg(G, tag):
    v = [int(x) for x in G[f"{tag}/freeze"]]
    return v if bool(G[f"{tag}/freeze_is_list"]) else v[0]


@pytest.mark.parametrize("tag", CASES)
def test_name_rule_matches_the_reference(golden, tag):
    G = golden("freeze")
    names = [str(n) for n in G["param_names"]]
    frozen = frozen_parameter_names(names, _freeze_arg(G, tag))
    assert frozen == [str(n) for n in G[f"{tag}/frozen_names"]]
    # every other parameter held a gradient after the reference's backward pass, no frozen one did
    assert [n for n in names if n not in set(frozen)] == [str(n) for n in G[f"{tag}/grad_names"]]


def test_a_layer_index_is_not_a_prefix_of_another(golden):
    """'model.2.' must not catch model.12., model.20. or model.22. (the rule matches the dotted key, not the digits)."""
    names = [str(n) for n in golden("freeze")["param_names"]]
    names += ["model.22.cv1.conv.weight", "model.22.cv1.bn.bias"]  # (layer 22 of this model owns no parameter: a Concat)
    frozen = frozen_parameter_names(names, [2])
    assert any(n.startswith("model.2.") for n in frozen)
    for other in ("model.12.", "model.20.", "model.22."):
        assert any(n.startswith(other) for n in names), other
        assert not any(n.startswith(other) for n in frozen), other
    assert all(n.startswith("model.2.") or ".dfl" in n for n in frozen)


def test_none_freezes_the_dfl_alone_and_int_means_a_range(golden):
    names = [str(n) for n in golden("freeze")["param_names"]]
    assert frozen_parameter_names(names, None) == [n for n in names if ".dfl" in n] != []
    assert frozen_parameter_names(names, 3) == frozen_parameter_names(names, [0, 1, 2])
    assert frozen_parameter_names(names, 0) == frozen_parameter_names(names, None)


def test_get_cfg_passes_freeze_through_unchanged():
    assert get_cfg(overrides=dict(freeze=8)).freeze == 8 and isinstance(get_cfg(overrides=dict(freeze=8)).freeze, int)
    assert get_cfg(overrides=dict(freeze=[12, 20])).freeze == [12, 20]
    assert get_cfg().freeze is None
