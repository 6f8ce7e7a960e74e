"""The selection of csrc/conv.hip -- which kernel family, with which template arguments and how many partial rows, a convolution
launch runs -- pinned against tests/golden/conv_select.json.gz, the answers of the library before conv_plan() took the decision over
(tests/golden/make_conv_select_golden.py: the sweep, the fixture's layout and how it was taken).  No GPU: the helpers only do
arithmetic on the geometry."""
import re

import pytest
from golden.make_conv_select_golden import RUNS, labels_sha, load, sweep

GOLD, META, SHAS = load()


@pytest.mark.parametrize("tag", [t for t, _, _ in RUNS])
def test_selection_matches_the_fixture(tag):
    pairs = sweep(tag)
    assert labels_sha(pairs) == SHAS[tag] and len(pairs) == len(GOLD[tag]), "the sweep is not the one the fixture was taken with"
    diff = [(k, v, g) for (k, v), g in zip(pairs, GOLD[tag]) if v != g]
    if diff:
        k, v, g = diff[0]
        print(f"{len(diff)} of {len(pairs)} answers differ; first: {k}: library {v!r}, fixture {g!r}")
    assert not diff, diff[:5]


def test_fixture_covers_every_family_and_every_refusal():
    """The fixture cannot pass by covering nothing: every family the helpers can spell is in it, in every form."""
    assert re.fullmatch(r"[0-9a-f]{40}", META["commit"])
    names = {t: [v for v in vals if isinstance(v, str)] for t, vals in GOLD.items()}
    every = [v for vals in names.values() for v in vals]

    def some(pattern, where=every):
        return any(re.fullmatch(pattern, v) for v in where)

    assert some(r"conv_mfma_pp_kernel<.*, false, 0>") and some(r"conv_mfma_pp_kernel<.*, false, 40>")
    assert some(r"conv_mfma_pp_kernel<.*, false, 80>", names["fw80"]) and not some(r"conv_mfma_pp_kernel<.*, false, 80>", names["unset"])
    assert not some(r"conv_mfma_pp_kernel<.*, false, (40|80)>", names["fw0"])
    assert some(r"conv_mfma_wlds_kernel<.*, 2, 8>") and some(r"conv_mfma_wlds_kernel<.*, 1, 8>") and some(r"conv_mfma_kernel<.*>")
    assert some(r"conv1x1_stream_kernel<.*, true>") and some(r"conv1x1_stream_kernel<.*, false>")
    assert not some(r"conv1x1_stream_kernel<.*>", names["stream0"])
    assert not some(r"conv_mfma_wlds_kernel<.*, 2, 4>")  # the 4-wave form was opt-in only and is gone
    # refusals: the unsupported kernel size (DY_ERR_ARG = -1 from every naming helper) and segment tables no chunk fits
    pairs = dict(zip((k for k, _ in sweep("unset")), GOLD["unset"]))  # the fixture's values under the sweep's labels
    assert pairs["geom/64>64/k5s1/rc"] == -1 and pairs["name/64>64/k5s1"] == -1 and pairs["at/64>64/k5s1/64x40x40/e0/d1"] == -1
    assert pairs["red/64>64/k5s1"] == 0 and pairs["res/64>64/k5s1"] == 0
    assert pairs["segs/8+56>64/supported"] == 0 and pairs["segs/8+56>64/name"] == -1 and pairs["segs/null_ptr/supported"] == 0
    assert pairs["segs/32+32>64/supported"] == 1
    # the shapes that reach the 2-row v3 form, and the full-width 80 tiles where they fit
    assert pairs["name/88>64/k3s1"] == "conv_mfma_wlds_kernel<8, 4, 3, 1, 2, 8>" and pairs["name/264>64/k1s1"] == "conv_mfma_wlds_kernel<8, 4, 1, 1, 2, 8>"
    fw80 = dict(zip((k for k, _ in sweep("fw80")), GOLD["fw80"]))
    assert fw80["at/32>32/k3s1/64x80x80/e0/d1"] == "conv_mfma_pp_kernel<32, 2, 3, 1, 1, false, 80>"
    assert fw80["at/64>64/k3s1/64x80x80/e0/d1"] == "conv_mfma_pp_kernel<32, 4, 3, 1, 2, false, 0>"
