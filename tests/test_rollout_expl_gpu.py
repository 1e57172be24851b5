"""The navigator rollout's fourth feedback mode and its policy entropy (-m gpu): 'expl_sample' (agent.py:1041-1051) and `entropy=True`
(agent.py:1037-1039) through the one-launch action selection (magic_nav_act), on the models and synthetic episodes of tests/test_rollout_gpu.py
(fp32 compute, H = 128, SynthNavEnv(B=5), max_action_len=7)."""
import numpy as np
import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host.config import make_config
from magic_amd.host.nav_rollout import FEEDBACKS, NavRollout
from tests import _navact_ref64 as R
from tests.test_rollout_gpu import DEV, KW, _env, _pair, close

pytestmark = pytest.mark.gpu
B, T = 5, 7
SEED = 9                     # episodes and draws of the 'sample' rollouts below: default_rng(9) leaves no draw inside the margin of its row
_CACHE = {}


def _model():
    if "m" not in _CACHE:
        _CACHE["m"] = _pair(make_config(128, role="student", **KW), "student", 1)[1]
    return _CACHE["m"]


def _run(feedback, seed=SEED, ratio=0.6, **kw):
    env = _env(seed, B=B)
    ro = NavRollout(_model(), torch.from_numpy(env.feature_table).to(DEV), max_action_len=T, expl_max_ratio=ratio)
    kw.setdefault("grad", False)
    return ro.run(env, env.reset(features=False), feedback=feedback, train_ml=1.0, record=True, **kw)


def _plain(feedback):
    """the rollouts on today's path (no kernel), once"""
    if feedback not in _CACHE:
        _CACHE[feedback] = _run(feedback, sample_draws=_draws())
    return _CACHE[feedback]


def _draws():
    return np.random.default_rng(SEED).uniform(size=(T, B))


def _same_rollout(a, b, bitwise=True):
    assert len(a["steps"]) == len(b["steps"]) and a["n_steps"] == b["n_steps"]
    for t, (x, y) in enumerate(zip(a["steps"], b["steps"])):
        if bitwise:
            assert torch.equal(x["logits"], y["logits"]), t
        assert x["actions"] == y["actions"] and x["vpids"] == y["vpids"] and torch.equal(x["targets"], y["targets"]), t
    assert [p["path"] for p in a["traj"]] == [p["path"] for p in b["traj"]]
    if bitwise:
        assert float(a["loss"]) == float(b["loss"])


def test_expl_sample_that_never_explores_is_the_argmax_rollout():
    ed = np.random.default_rng(3).uniform(size=(T, B, 2))
    got, want = _run("expl_sample", ratio=1.0, explore_draws=ed), _plain("argmax")
    _same_rollout(got, want)
    assert got["explored"] == 0 and "explored" not in want and "entropy_steps" not in want
    assert got["entropy_steps"] == [0.0] * got["n_steps"]            # no 'sample' row


def test_expl_sample_that_always_explores_takes_the_drawn_candidate():
    """ratio 0 and positive draws: every live decision is the reference's pick (agent.py:1050-1051) from the step's own recorded logits --
    the candidates are the finite columns -- and index 0 ends the episode.  (The parent commit ran the argmax rollout here.)"""
    ed = np.maximum(np.random.default_rng(4).uniform(size=(T, B, 2)), 1e-9)
    got = _run("expl_sample", ratio=0.0, explore_draws=ed)
    ended, n_live, off_argmax = np.zeros(B, bool), 0, 0
    for t, st in enumerate(got["steps"]):
        live = (st["targets"] != -100).numpy()
        assert (live == ~ended).all(), t
        for i in np.flatnonzero(live):
            lg = st["logits"][i]
            cand = torch.isfinite(lg).numpy()
            pick, went = R.explore_action(int(lg.argmax()), cand, ed[t, i, 0], ed[t, i, 1], 0.0)
            assert went and pick == np.arange(len(cand))[cand][min(int(ed[t, i, 1] * cand.sum()), cand.sum() - 1)]
            n_live += 1
            off_argmax += pick != int(lg.argmax())
            if pick == 0 or t == T - 1:
                assert st["actions"][i] is None, (t, i)
                ended[i] = True
            else:
                assert st["actions"][i] == st["vpids"][i][pick], (t, i)
    assert got["explored"] == got["decisions"] == n_live and off_argmax > 0


@pytest.mark.parametrize("graphs", [False, True])
def test_teacher_and_expl_sample_as_one_batch_equal_the_two_rollouts(graphs):
    g = _model()
    env = _env(23, B=B)
    batch = [env._draw_episode() for _ in range(B)]
    ed = np.random.default_rng(6).uniform(size=(T, B, 2))
    table = torch.from_numpy(env.feature_table).to(DEV)
    ro = NavRollout(g, table, max_action_len=T, expl_max_ratio=0.5)
    g.train()                                                         # (dropout 0; captured step instances serve training steps)
    try:
        r1 = ro.run(env, env.reset(batch=batch, features=False), feedback="teacher", train_ml=0.2, record=True, grad=False)
        r2 = ro.run(env, env.reset(batch=batch, features=False), feedback="expl_sample", train_ml=1.0, explore_draws=ed, record=True, grad=False)
        assert 0 < r2["explored"] < r2["decisions"]
        env2 = _env(23, B=2 * B)
        ed2 = np.concatenate([np.zeros((T, B, 2)), ed], 1)
        rc_ro = NavRollout(g, table, max_action_len=T, expl_max_ratio=0.5, graphs=True, Lcap=16) if graphs else ro
        for it in range(3 if graphs else 1):                          # (graphs: first sight runs eagerly, then the instances are captured, then replayed)
            g.store.zero_grad()
            rc = rc_ro.run(env2, env2.reset(batch=batch + batch, features=False), feedback=["teacher"] * B + ["expl_sample"] * B,
                           train_ml=[0.2] * B + [1.0] * B, explore_draws=ed2, record=True, text_copies=2, grad=graphs)
            if graphs:
                rc["loss"].backward()
                torch.cuda.synchronize()
        if graphs:
            assert rc_ro.graph_report()["student"]["instances"] > 0
    finally:
        g.eval()
    close(rc["loss"], float(r1["loss"]) + float(r2["loss"]), "combined loss", 2e-5, 1e-6)
    assert rc["decisions"] == r1["decisions"] + r2["decisions"] and rc["explored"] == r2["explored"]
    for t, st in enumerate(rc["steps"]):
        for half, rr in ((0, r1), (1, r2)):
            if t < len(rr["steps"]):
                a, b = st["logits"][half * B:(half + 1) * B], rr["steps"][t]["logits"]
                K = min(a.shape[1], b.shape[1])
                live = rr["steps"][t]["targets"] != -100
                close(torch.nan_to_num(a[live][:, :K], neginf=0), torch.nan_to_num(b[live][:, :K], neginf=0), f"step {t} half {half}", 1e-5, 1e-5)
                assert st["actions"][half * B:(half + 1) * B] == rr["steps"][t]["actions"]
    assert [x["path"] for x in rc["traj"]] == [x["path"] for x in r1["traj"]] + [x["path"] for x in r2["traj"]]


def test_entropy_of_a_sample_rollout():
    draws = _draws()
    got, want = _run("sample", sample_draws=draws, entropy=True), _plain("sample")
    _same_rollout(got, want)
    assert "entropy_steps" not in want and len(got["entropy_steps"]) == got["n_steps"] and got["explored"] == 0
    for t, st in enumerate(got["steps"]):
        ref = R.navact_ref(st["logits"])
        for i in np.flatnonzero((st["targets"] != -100).numpy()):
            assert R.decided(ref, i, float(draws[t, i])), f"seed {SEED}: the draw of step {t} row {i} lies inside the margin: pick another seed"
        bnd = R.bound(ref["entropy"], ref["entropy_env"]).sum().item()
        err = abs(got["entropy_steps"][t] - ref["entropy"].sum().item())
        print(f"entropy step {t}: {got['entropy_steps'][t]:.7f} ref {ref['entropy'].sum().item():.7f} err/bound {err / bnd:.3g}")
        assert err <= bnd, t


def test_feedback_strings_are_checked_before_anything_is_planned():
    env = _env(SEED, B=B)
    ro = NavRollout(_model(), torch.from_numpy(env.feature_table).to(DEV), max_action_len=T)
    obs = env.reset(features=False)
    before = [dict(s) for s in env.state]
    for fb in ("argmx", ["teacher"] * (B - 1) + ["explore"]):
        with pytest.raises(ValueError, match="expl_sample") as e:
            ro.run(env, obs, feedback=fb)
        assert all(f in str(e.value) for f in FEEDBACKS)
    with pytest.raises(ValueError, match="explore_draws"):
        ro.run(env, obs, feedback="expl_sample")
    with pytest.raises(ValueError, match="explore_draws"):
        ro.run(env, obs, feedback=["teacher"] * (B - 1) + ["expl_sample"], sample_draws=_draws())
    assert [dict(s) for s in env.state] == before                      # nothing was planned: the environment was not touched


def test_existing_modes_through_the_kernel_give_the_same_rollouts(monkeypatch):
    monkeypatch.setenv("MAGIC_NAV_ACT", "1")
    for fb in ("argmax", "sample"):
        got = _run(fb, sample_draws=_draws())
        assert "entropy_steps" in got                                   # the kernel path ran
        monkeypatch.delenv("MAGIC_NAV_ACT")
        want = _plain(fb)
        monkeypatch.setenv("MAGIC_NAV_ACT", "1")
        _same_rollout(got, want)
    monkeypatch.delenv("MAGIC_NAV_ACT")
    assert "entropy_steps" not in _run("teacher")
