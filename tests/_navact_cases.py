"""The cases and checks of magic_nav_act, shared by tests/test_navact_gpu.py (the kernel) and tests/test_navact_ref64_cpu.py (the reference
with a planted defect must FAIL these same checks).

An implementation under test is a callable
    impl(logits_full [B, K + 3] fp32, cand_full [B, K + 5] bool or None, K, modes [n, B] uint8, draws [n, B, 3] float64, ratio)
        -> (actions [n, B] integers, stop_prob [B], entropy [B])          (one launch per leading index of modes / draws; numpy or torch)
`verify(impl, B, K)` builds the rows, constructs every draw, and asserts.  No draw is filtered: the builder asserts that the reference decides
each one it constructs (a class that is swept holds more than 4 delta, so its midpoint and the points 2 delta inside its ends are all further than
delta from both ends)."""
import numpy as np
import torch

from tests import _navact_ref64 as R
from tests._loss_ref64 import f32

NEG = float("-inf")
RATIOS = (0.0, 0.6, 1.0)
U_TOP = 1.0 - 2.0 ** -53


def make_rows(B, K, seed=0):
    """logits [B, K + 3] fp32 with NaN in the padding, cand [B, K + 5] bool with set bytes in the padding.  Row kinds (r % 5; one row: the +-80 span):
    0 random masks, 1 all masked, 2 one finite logit at the last column, 3 the maximum at two columns, 4 logits spanning +-80 (a few heavy
    classes near +80, the first and the last unmasked column among them, the rest anywhere down to -80: some exponentials underflow in fp32)"""
    g = np.random.default_rng(1000 * K + 10 * B + seed)
    x = np.full((B, K + 3), np.nan, np.float32)
    cand = np.ones((B, K + 5), bool)
    kinds = [4] if B == 1 else [r % 5 for r in range(B)]
    for r, kind in enumerate(kinds):
        row = g.uniform(-0.5, 0.5, K).astype(np.float32)
        keep = g.random(K) > 0.3
        keep[g.integers(K)] = True
        if kind == 1:
            keep[:] = False
        elif kind == 2:
            keep[:] = False
            keep[K - 1] = True
        elif kind == 3:
            keep[:] = True
            c = g.choice(K, size=min(2, K), replace=False)
            row[c] = np.float32(0.75)
        elif kind == 4:
            row = g.uniform(-80.0, 40.0, K).astype(np.float32)
            un = np.flatnonzero(keep)
            heavy = np.unique(np.concatenate([un[[0, -1]], g.choice(un, size=min(4, len(un)), replace=False)]))
            row[heavy] = (80.0 - g.uniform(0.0, 2.0, len(heavy))).astype(np.float32)
            light = np.setdiff1d(un, heavy)
            if len(light):
                row[light[len(light) // 2]] = np.float32(-80.0)
        x[r, :K] = np.where(keep, row, np.float32(NEG))
        cand[r, :K] = keep & (g.random(K) > 0.25)                 # the candidate set: a subset of the unmasked columns (may be empty)
        if kind == 3:
            cand[r, :K] = g.random(K) > 0.5
    return x, cand


def _ue_sides(ratio32):
    """u_explore values that keep the argmax / that explore, hugging the ratio from both sides (u in [0, 1))"""
    keep = [0.0, ratio32] if ratio32 < 1.0 else [0.0, U_TOP]
    if ratio32 > 0.0:
        keep.append(min(float(np.nextafter(ratio32, -1.0)), U_TOP))
    go = []
    if ratio32 < 1.0:
        go = [float(np.nextafter(ratio32, 2.0)), min(ratio32 + 0.25, U_TOP), U_TOP]
    return keep, go


def build(x_full, cand_full, K):
    """-> ref, groups: each group dict(name, ratio, cand (bool: the launch gets the candidate bytes), modes [n, B], draws [n, B, 3], expect [n, B])"""
    B = x_full.shape[0]
    x, cand = torch.from_numpy(x_full[:, :K]), cand_full[:, :K]
    ref = R.navact_ref(x)
    dl = R.delta(K)
    groups = []
    # ---- sample: per row every swept class's midpoint and the two points 2 delta inside its ends, u = 0 and u = 1 - 2^-53
    per_row, per_exp = [], []
    for r in range(B):
        us, want = [0.0, U_TOP], []
        iv = R.intervals(ref, r)
        if iv:
            assert iv[0][2] - iv[0][1] > 4 * dl and iv[-1][2] - iv[-1][1] > 4 * dl, "inputs: the first and the last unmasked class must be heavy"
            want = [iv[0][0], iv[-1][0]]
        else:
            want = [0, 0]
        for c, lo, hi, _, _ in iv:
            if hi - lo > dl:
                assert hi - lo > 4 * dl, f"inputs: row {r} class {c} holds {hi - lo:.3g}, between delta and 4 delta: its draws would sit inside the margin"
                us += [0.5 * (lo + hi), lo + 2 * dl, hi - 2 * dl]
                want += [c, c, c]
        us = np.array(us)
        exp = R.sample_actions(ref, r, us)
        assert (exp == np.array(want)).all(), f"row {r}: the reference does not decide its own draws"
        assert all(R.decided(ref, r, float(u)) for u in us[:50]), f"row {r}: a constructed draw lies inside the margin"
        per_row.append(us)
        per_exp.append(exp)
    n = max(len(u) for u in per_row)
    draws = np.zeros((n, B, 3))
    expect = np.zeros((n, B), np.int64)
    for r in range(B):
        idx = np.arange(n) % len(per_row[r])
        draws[:, r, 0], expect[:, r] = per_row[r][idx], per_exp[r][idx]
    draws[:, :, 1:] = 0.999                                        # (a sample row reads neither)
    groups.append(dict(name="sample", ratio=0.6, cand=True, modes=np.full((n, B), 2, np.uint8), draws=draws, expect=expect))
    # ---- expl_sample: u_explore on both sides of every ratio, u_choice at j / n and (j + 0.5) / n for every j
    am = ref["argmax"].numpy()
    for ratio in RATIOS:
        r32 = f32(ratio)
        keep, go = _ue_sides(r32)
        rows_d, rows_e = [], []
        for r in range(B):
            nc = int(cand[r].sum())
            uc = np.array([(j + h) / nc for j in range(nc) for h in (0.0, 0.5)] + [0.0, U_TOP])
            ue = np.array(keep + [g_ for g_ in go for _ in uc])
            ucc = np.array([0.5] * len(keep) + list(uc) * len(go))
            e, _ = R.explore_actions(am[r], cand[r], ue, ucc, r32)
            if not bool(ref["live"][r]):
                e[:] = 0
            rows_d.append(np.stack([np.full(len(ue), 0.5), ue, ucc], 1))
            rows_e.append(e)
        n = max(len(d) for d in rows_d)
        draws, expect = np.zeros((n, B, 3)), np.zeros((n, B), np.int64)
        for r in range(B):
            idx = np.arange(n) % len(rows_d[r])
            draws[:, r], expect[:, r] = rows_d[r][idx], rows_e[r][idx]
        groups.append(dict(name=f"expl_sample ratio {ratio}", ratio=ratio, cand=True, modes=np.full((n, B), 3, np.uint8), draws=draws, expect=expect))
    # ---- argmax everywhere; the four modes mixed (mode 0 rows return -1); expl_sample without candidate bytes keeps the argmax
    d1 = np.tile(np.array([0.5, 0.9, 0.5]), (1, B, 1))
    live = ref["live"].numpy()
    groups.append(dict(name="argmax", ratio=0.6, cand=True, modes=np.full((1, B), 1, np.uint8), draws=d1, expect=am[None].copy()))
    modes = np.stack([(np.arange(B) + s) % 4 for s in range(4)]).astype(np.uint8)
    dm = np.tile(d1, (4, 1, 1))
    exp = np.stack([R.actions(ref, cand, modes[s], dm[s], f32(0.6)) for s in range(4)])
    groups.append(dict(name="mixed modes", ratio=0.6, cand=True, modes=modes, draws=dm, expect=exp))
    groups.append(dict(name="expl_sample, no candidate bytes", ratio=0.0, cand=False, modes=np.full((1, B), 3, np.uint8), draws=d1,
                       expect=np.where(live, am, 0)[None]))
    return ref, groups


def verify(impl, B, K, seed=0):
    x_full, cand_full = make_rows(B, K, seed)
    ref, groups = build(x_full, cand_full, K)
    stop = ent = None
    for gp in groups:
        act, stop, ent = impl(x_full, cand_full if gp["cand"] else None, K, gp["modes"], gp["draws"], gp["ratio"])
        act = np.asarray(act.cpu() if torch.is_tensor(act) else act).astype(np.int64)
        bad = np.argwhere(act != gp["expect"])
        assert len(bad) == 0, (f"B={B} K={K} {gp['name']}: {len(bad)} actions differ, first at launch {bad[0][0]} row {bad[0][1]}: got {act[tuple(bad[0])]}, "
                               f"reference {gp['expect'][tuple(bad[0])]}, draws {gp['draws'][tuple(bad[0])]}")
        assert act.min() >= -1 and act.max() < K
        stop_t, ent_t = (torch.as_tensor(np.asarray(t.cpu() if torch.is_tensor(t) else t)) for t in (stop, ent))
        R.check("nav_act", f"stop_prob B={B} K={K} {gp['name']}", stop_t, ref["stop_prob"], ref["stop_env"])
        R.check("nav_act", f"entropy   B={B} K={K} {gp['name']}", ent_t, ref["entropy"], ref["entropy_env"])
    return ref


def reference_impl(**defects):
    """the float64 reference as an implementation under test (tests/test_navact_ref64_cpu.py), with planted defects"""
    rd = {k: v for k, v in defects.items() if k in ("reverse_prefix", "no_clamp", "last_max")}
    ad = {k: v for k, v in defects.items() if k in ("count_off_by_one", "flip_test")}

    def impl(x_full, cand_full, K, modes, draws, ratio):
        ref = R.navact_ref(torch.from_numpy(x_full[:, :K]), **rd)
        cand = None if cand_full is None else cand_full[:, :K]
        act = np.stack([R.actions(ref, cand, modes[j], draws[j], f32(ratio), **ad) for j in range(modes.shape[0])])
        return act, ref["stop_prob"], ref["entropy"]
    return impl
