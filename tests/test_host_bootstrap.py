"""CPU: the host half of the paired bootstrap test (ultralytics/utils/bootstrap.py) -- the resample draw against the reference
script's ``np.random.seed`` / ``np.random.choice`` sequence, the statistics step against direct scipy calls -- and the fixture
tests/golden/bootstrap.npz (the REFERENCE's ap_per_class on replicated statistics) against the CPU oracle."""
import numpy as np
import pytest

from oracle import metrics as om


def replicate(G, case, s):
    """The statistics of resample s of a fixture case: every detection / label of image i repeated mult[s, i] times."""
    m = G[f"{case}/mult"][s]
    rd, rl = m[G[f"{case}/det_img"]], m[G[f"{case}/lab_img"]]
    return (np.repeat(G[f"{case}/tp"], rd, 0), np.repeat(G[f"{case}/conf"], rd), np.repeat(G[f"{case}/pred_cls"], rd).astype(np.float64),
            np.repeat(G[f"{case}/lab_cls"], rl).astype(np.float64))


def oracle_ap(G, case, nc=3):
    S = G[f"{case}/mult"].shape[0]
    ap = np.zeros((S, nc, 10))
    for s in range(S):
        res = om.ap_per_class(*replicate(G, case, s))
        ap[s, res["classes"]] = res["ap"]
    return ap


@pytest.mark.parametrize("case", ["big", "exact"])
def test_oracle_on_replicated_lists_reproduces_the_fixture(golden, case):
    G = golden("bootstrap")
    ap = oracle_ap(G, case)
    assert ap.shape == G[f"{case}/ap"].shape == (6, 3, 10)
    assert np.abs(ap - G[f"{case}/ap"]).max() < 1e-12
    nl = G[f"{case}/nl"]
    assert (ap[nl == 0] == 0).all()
    # the situations the cases were arranged for are there
    if case == "big":
        assert np.bincount(G["big/pred_cls"], minlength=3).tolist() == [701, 24, 0] and (nl[:, 2] == 0).all()
        assert nl[1, 1] == 1 and nl[2, 1] == 3 and nl[4, 1] == 0 and nl[5, 1] > 0 and (ap[5, 1] == 0).all()
        assert (G["big/mult"][1:3].sum(1) == 1).all()  # single-image resamples
    else:
        assert nl[0, 0] == 50 and nl[1, 0] == 100 and (ap[:, 1] == 0).all() and nl[3].tolist() == [7, 0, 3]


def test_draw_resamples_consumes_the_reference_stream():
    from ultralytics.utils.bootstrap import draw_resamples
    paths = sorted(f"/data/test/images/im_{i * 7919 % 1000:04d}.jpg" for i in range(37))
    np.random.seed(42)  # testandcox.py:153, :162, :176
    n_size = max(1, int(len(paths) * 0.5))
    assert n_size == 18
    subsets = [list(np.random.choice(paths, size=n_size, replace=True)) for _ in range(3)]
    mult = draw_resamples(37, num_samples=3, sample_fraction=0.5, seed=42)
    assert mult.shape == (3, 37) and mult.dtype == np.uint16
    for s, subset in enumerate(subsets):
        want = np.array([subset.count(p) for p in paths])
        assert (mult[s] == want).all()
    assert (mult.sum(1) == n_size).all()
    assert (draw_resamples(3, 4, 0.1, 0).sum(1) == 1).all()  # n_size = max(1, int(0.3))
    assert (draw_resamples(37, 3, 0.5, 42) == mult).all() and (draw_resamples(37, 3, 0.5, 43) != mult).any()


def test_multiplicity_above_uint16_raises():
    from ultralytics.utils.bootstrap import check_mult, draw_resamples
    with pytest.raises(ValueError, match="65535"):
        draw_resamples(1, num_samples=2, sample_fraction=70000.0, seed=0)  # one image drawn 70,000 times
    with pytest.raises(ValueError, match="65535"):
        check_mult(np.array([[1, 65536, 0]]), 3)
    assert check_mult(np.array([[1, 65535, 0]]), 3).tolist() == [[1, 65535, 0]]
    with pytest.raises(ValueError):
        check_mult(np.array([[1, -1, 0]]), 3)
    with pytest.raises(ValueError):
        check_mult(np.array([[1, 2]]), 3)


def test_statistics_step_equals_scipy_and_the_formulae():
    from scipy import stats
    from ultralytics.utils.bootstrap import paired_statistics, summary_lines
    rng = np.random.default_rng(7)
    base = 0.55 + 0.03 * rng.standard_normal(30)
    deal = base + 0.01 + 0.008 * rng.standard_normal(30)
    res = paired_statistics(deal, base, seed=42, ci_iters=2000)
    d = deal - base
    n = 30
    assert res["n"] == n and res["deal_mean"] == deal.mean() and res["base_mean"] == base.mean()
    assert res["mean_diff"] == d.mean() and res["std_diff"] == d.std(ddof=1)
    assert res["shapiro_p"] == stats.shapiro(d)[1]
    t, p = stats.ttest_rel(deal, base)
    assert (res["t_stat"], res["t_p"]) == (t, p)
    w, pw = stats.wilcoxon(deal, base, zero_method="wilcox", alternative="two-sided")
    assert (res["wilcoxon_w"], res["wilcoxon_p"]) == (w, pw)
    half = stats.t.ppf(1 - 0.025, df=n - 1) * (d.std(ddof=1) / np.sqrt(n))  # testandcox.py:269-271
    assert res["ci_t"] == (d.mean() - half, d.mean() + half)
    gen = np.random.RandomState(42)
    means = np.array([gen.choice(d, size=n, replace=True).mean() for _ in range(2000)])
    assert res["ci_bootstrap"] == tuple(np.percentile(means, [2.5, 97.5]))
    assert res["cohens_d"] == d.mean() / d.std(ddof=1)
    assert res["significant"] == (pw < 0.05 or p < 0.05) and res["significant"]  # a 0.01 shift against 0.008 noise
    assert "Wilcoxon" in res["verdict"]
    lines = summary_lines(res)
    assert f"Mean difference (deal - base): {d.mean():.6f}" in lines and any(l.startswith("Paired t-test: t=") for l in lines)
    # identical scores: Wilcoxon cannot run (nan, as in the reference), nothing is significant, Cohen's d is undefined
    same = paired_statistics(base, base, ci_iters=10)
    assert np.isnan(same["wilcoxon_p"]) and np.isnan(same["cohens_d"]) and not same["significant"]


def test_entry_point_rejects_bad_arguments_without_a_launch():
    from ultralytics.hip import lib
    L = lib()
    assert L.dy_bootstrap_ap(8, 8, 8, 8, 8, 4, 7, 3, 0, 8, 8, None) == -1   # no resample
    assert L.dy_bootstrap_ap(8, 8, 8, 8, 8, 4, 0, 3, 1, 8, 8, None) == -1   # no image
    assert L.dy_bootstrap_ap(None, None, 8, 8, 8, 4, 7, 3, 1, 8, 8, None) == -1  # detections without their arrays
    assert L.dy_bootstrap_ap(8, 8, 8, 8, 8, 4, 7, 3, 1, None, 8, None) == -1  # no output
    assert L.dy_bootstrap_ap(8, 8, 8, 8, 8, 4, 7, 1 << 16, 1 << 16, 8, 8, None) == -1  # more workgroups than a grid holds
