"""tests/_navact_ref64.py (the float64 reference of magic_nav_act) against independent statements of the same rules, and the checks of
tests/_navact_cases.py against planted defects.  No GPU."""
import numpy as np
import pytest
import torch

from tests import _navact_cases as C
from tests import _navact_ref64 as R
from tests._loss_ref64 import f32


def _rows(B=6, K=37, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = (4.0 * torch.randn(B, K, generator=g)).float()
    x[torch.rand(B, K, generator=g) < 0.3] = R.NEG
    x[:, 5] = 1.0                                        # (no row fully masked here)
    x[0] = R.NEG
    x[0, K - 1] = 2.0                                    # one-hot row: p = 1, the clamp's top end
    x[1, :] = torch.linspace(-40.0, 40.0, K)             # probabilities far below 2^-23: the clamp's bottom end
    return x


def test_entropy_is_categorical_entropy_on_fp32_probabilities():
    x = _rows()
    ref = R.navact_ref(x)
    p32 = torch.softmax(x, 1)
    want = torch.distributions.Categorical(probs=p32).entropy().double()
    assert torch.isfinite(want).all()
    # fp32 rounding of K products of size <= p |log p| around an fp32 softmax: 1e-5 of the envelope, as every fp32 kernel is held to
    assert ((ref["entropy"] - want).abs() <= R.bound(ref["entropy"], ref["entropy_env"])).all()
    assert abs(float(ref["entropy"][0]) - (-np.log(1 - R.EPS))) < 1e-15 and float(want[0]) > 1e-7          # the clamp is what torch does too
    nc = R.navact_ref(x, no_clamp=True)["entropy"]
    assert not ((nc - want).abs() <= R.bound(ref["entropy"], ref["entropy_env"])).all()


def test_stop_probability_and_masked_rows():
    x = _rows()
    x[2] = R.NEG
    ref = R.navact_ref(x)
    assert torch.allclose(ref["stop_prob"][3:], torch.softmax(x.double(), 1)[3:, 0], rtol=1e-12, atol=0)
    assert not bool(ref["live"][2]) and float(ref["stop_prob"][2]) == 0.0 and float(ref["entropy"][2]) == 0.0 and int(ref["argmax"][2]) == 0
    assert all(torch.isfinite(ref[k]).all() for k in ("p", "cdf", "stop_prob", "entropy", "entropy_env"))
    modes = np.array([0, 1, 2, 3, 0, 2], np.uint8)
    a = R.actions(ref, np.ones(x.shape, bool), modes, np.full((6, 3), 0.5), f32(0.6))
    assert a[0] == -1 and a[4] == -1 and a[2] == 0                    # mode 0: -1; a dead row under any other mode: 0


def test_sampling_rule_is_the_cdf_count_outside_the_margin():
    """`(cdf < u cdf[-1]).sum()` -- what host/nav_rollout.py computes with torch -- on every draw outside the margin (inside it the fp32 cdf of
    that expression and the fp64 one here may differ by a class)"""
    x = _rows()
    ref = R.navact_ref(x)
    K = x.shape[1]
    cdf32 = torch.softmax(x, 1).double().cumsum(1).numpy()
    u = np.random.default_rng(11).random(4000)
    used = 0
    for r in range(x.shape[0]):
        mine = R.sample_actions(ref, r, u)
        ok = np.array([R.decided(ref, r, float(v)) for v in u])
        theirs = (cdf32[r][None, :] < (u * cdf32[r, -1])[:, None]).sum(1)
        assert (mine[ok] == theirs[ok]).all()
        assert (ref["p"][r].numpy()[mine] > 0).all() and mine.max() < K          # never a masked column
        used += int(ok.sum())
    assert used > 0.99 * u.size * x.shape[0]                          # the margin is ~4e-5 per boundary: it sets hardly anything aside
    assert 1e-5 < R.delta(1) < R.delta(1100) < 1e-4


def test_exploration_rule_is_an_index_into_the_candidate_list():
    g = np.random.default_rng(5)
    K = 23
    for trial in range(200):
        cand = g.random(K) < 0.4
        ue, uc, ratio = g.random(), g.random(), f32(g.choice([0.0, 0.6, 1.0]))
        a, go = R.explore_action(7, cand, ue, uc, ratio)
        if ue > ratio and cand.any():
            assert go and a == np.arange(K)[cand][int(uc * cand.sum())]          # agent.py:1050 picks from the candidate indices
        else:
            assert not go and a == 7
    assert R.explore_action(7, np.zeros(K, bool), 0.9, 0.5, 0.0) == (7, False)
    assert R.explore_action(7, None, 0.9, 0.5, 0.0) == (7, False)
    cand = np.zeros(K, bool)
    cand[[2, 9, 22]] = True
    assert R.explore_action(7, cand, 0.9, 1.0 - 2.0 ** -53, 0.0) == (22, True)


def test_exploration_picks_are_uniform():
    cand = np.zeros(31, bool)
    cand[[1, 4, 9, 20, 30]] = True
    g = np.random.default_rng(2024)
    n = 20000
    a, go = R.explore_actions(0, cand, np.ones(n) * 0.9, g.random(n), f32(0.6))
    assert go.all() and set(a.tolist()) == {1, 4, 9, 20, 30}
    counts = np.array([(a == c).sum() for c in (1, 4, 9, 20, 30)])
    sigma = np.sqrt(n * 0.2 * 0.8)
    assert (np.abs(counts - n / 5) < 4 * sigma).all(), counts
    _, go = R.explore_actions(0, cand, g.random(n), g.random(n), f32(0.6))          # P(explore) = 1 - ratio
    assert abs(go.sum() - 0.4 * n) < 4 * np.sqrt(n * 0.4 * 0.6)


@pytest.mark.parametrize("B, K", [(1, 1), (5, 2), (5, 7), (5, 65), (7, 130)])
def test_reference_passes_its_own_cases(B, K):
    C.verify(C.reference_impl(), B, K)


@pytest.mark.parametrize("defect", ["count_off_by_one", "reverse_prefix", "no_clamp", "last_max", "flip_test"])
def test_planted_defect_is_rejected_by_the_gpu_tests_checks(defect):
    with pytest.raises(AssertionError):
        C.verify(C.reference_impl(**{defect: True}), 5, 65)
