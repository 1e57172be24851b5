"""Float64 reference of magic_nav_act (csrc/loss.hip nav_act_kernel): the action selection of a navigation step (agent.py:1028-1051).

Like tests/_kdcols_ref64.py: nothing here launches a kernel or rounds "the way the kernel would".  The logits are taken as stored (fp32) and
everything from there is float64:

    x = logits[r, :K], -inf = masked;  e = exp(x - max x),  cdf_c = e_0 + ... + e_c (column order),  Z = cdf_{K-1},  p = e / Z
    stop_prob = p_0
    entropy   = -sum_c p_c log(clamp(p_c, EPS, 1 - EPS)),  EPS = 2^-23      (torch.distributions.Categorical(probs=p).entropy() on fp32 p)
    argmax    = the lowest index among the maxima
    sample    = the smallest c with p_c > 0 and cdf_c >= u_sample Z; none: the last c with p_c > 0
    explore   = argmax, replaced when u_explore > ratio by the min(floor(u_choice n), n - 1)-th set byte of cand[r, :K] (n of them; n == 0 keeps it)
    a row with no finite logit: action 0, stop_prob 0, entropy 0;  mode 0: action -1

Envelopes (for _loss_ref64.bound: |got - ref| <= 1e-5 envelope).  A probability's is p (1 + |log p|), as _loss_ref64._lse has it.  The entropy
term p L(p), L = log clamp(p), moves by (L + [p not clamped]) dp + p dL: the envelope is sum_c penv_c (|L_c| + inside_c) + p_c |L_c|, with inside_c = 0
only where the class stays clamped at the top whatever fp32 does to it (p_c >= 1 - EPS / 2: the other classes hold <= EPS / 2 together, so the fp32
probability is 1 or 1 - 2^-24, both above 1 - EPS).  A one-hot row's entropy is therefore pinned to ~1e-12 around -log(1 - EPS) = 1.19e-7: the
clamp is visible.

The margin delta(K).  The contract's arithmetic is fp32 exponentials and ONE fp64 ordered sum, so a kernel's normalised cdf F_c = cdf_c / Z differs
from the one here only through the relative error eps_c of each e_c:  |dF_c| = |sum_{j<=c} e_j eps_j / Z - F_c sum_j e_j eps_j / Z| <= 2 max_c eps_c.
`__expf(d)` is exp2(d log2(e)) on the hardware's exp2: the fp32 difference d = x - max carries |d| 2^-24, the product with log2(e) another
|d| 2^-24 (relative error of e = absolute error of the exponent), the exp2 itself 1 ulp = 2^-23; doubled for slack: eps(d) = 2^-21 + |d| 2^-22.
A class with d < -88.8 has e < 2^-127 and may be flushed to zero: it holds < 2^-127 of the mass, K of them K 2^-127; the fp64 sum adds K 2^-53.
So eps_max = 2^-21 + 88.8 2^-22 and
    delta(K) = 2 eps_max + K (2^-127 + 2^-53)          (~4.3e-5; K hardly matters)
A draw u decides class c when F_{c-1} + delta < u < F_c - delta.  An edge that is exact in ANY arithmetic needs no margin: the lower edge when
every column before c is masked (F = 0 exactly, and u >= 0), the upper edge when every column behind c is masked (no earlier class can reach
u Z, and c is also what the "rounding leaves none" rule returns).  Inside the margin the outcome is not determined by the contract."""
import numpy as np
import torch

from tests._loss_ref64 import REL, bound, check  # noqa: F401  (re-exported: the GPU tests take the bound from here)

NEG = float("-inf")
EPS = 2.0 ** -23


def delta(K):
    eps_max = 2.0 ** -21 + 88.8 * 2.0 ** -22
    return 2.0 * eps_max + K * (2.0 ** -127 + 2.0 ** -53)


def navact_ref(logits, reverse_prefix=False, no_clamp=False, last_max=False):
    """logits [B, K] as stored (columns beyond K already cut away).  dict of float64 tensors: p, cdf [B, K] (unnormalised, column order), Z [B],
    stop_prob, stop_env, entropy, entropy_env [B]; argmax [B] int64; live [B] bool (the row has a finite logit).
    The flags PLANT a defect (tests only): the prefix accumulated from the last column down, the entropy without its clamp, the argmax as the
    LAST maximum."""
    x = logits.double()
    B, K = x.shape
    finite = torch.isfinite(x)
    live = finite.any(1)
    xs = torch.where(finite, x, torch.full_like(x, NEG))
    mx = torch.where(live, xs.max(1).values, torch.zeros(B, dtype=torch.float64))
    d = xs - mx[:, None]
    e = torch.where(finite, d.exp(), torch.zeros_like(x))
    cdf = e.flip(1).cumsum(1).flip(1) if reverse_prefix else e.cumsum(1)
    Z = e.sum(1) if reverse_prefix else cdf[:, -1]
    Zs = torch.where(live, Z, torch.ones_like(Z))
    p = e / Zs[:, None]
    z = torch.where(p > 0, p.clamp_min(1e-300).log(), torch.zeros_like(p))          # log p where it exists
    penv = p * (1 + z.abs())
    Lc = (p if no_clamp else p.clamp(EPS, 1 - EPS)).clamp_min(1e-300).log()
    ent = -(p * Lc).sum(1)
    inside = (p < 1 - EPS / 2).double()
    ent_env = (penv * (Lc.abs() + inside) + p * Lc.abs()).sum(1)
    top = xs == xs.max(1, keepdim=True).values
    idx = torch.arange(K)[None].expand(B, K)
    am = torch.where(top, idx, torch.full_like(idx, -1)).max(1).values if last_max else torch.where(top, idx, torch.full_like(idx, K)).min(1).values
    am = torch.where(live, am, torch.zeros_like(am))
    return dict(p=p, cdf=cdf, Z=Z, stop_prob=p[:, 0], stop_env=penv[:, 0], entropy=ent, entropy_env=ent_env, argmax=am, live=live)


def sample_actions(ref, r, u, count_off_by_one=False):
    """the sampling rule on row r for an array of draws u -> int64 array.  count_off_by_one PLANTS a defect (tests only): the class AFTER the
    one the rule names"""
    u = np.atleast_1d(np.asarray(u, np.float64))
    if not bool(ref["live"][r]):
        return np.zeros(len(u), np.int64)
    p, cdf, Z = ref["p"][r].numpy(), ref["cdf"][r].numpy(), float(ref["Z"][r])
    pos = np.flatnonzero(p > 0)
    cp = cdf[pos]
    thr = u * Z
    if np.all(np.diff(cp) >= 0):                         # a forward fp64 sum of non-negatives: the first cdf_c >= thr by bisection
        k = np.searchsorted(cp, thr, side="left")
    else:                                                # (a planted reverse prefix is not monotone: the rule as written)
        k = np.array([(np.flatnonzero(cp >= t)[:1].tolist() or [len(pos)])[0] for t in thr], np.int64)
    k = np.minimum(k, len(pos) - 1)                      # none: the last positive class
    if count_off_by_one:
        k = np.minimum(k + 1, len(pos) - 1)
    return pos[k].astype(np.int64)


def sample_action(ref, r, u, **kw):
    return int(sample_actions(ref, r, [u], **kw)[0])


def explore_actions(argmax, cand_row, u_explore, u_choice, ratio, flip_test=False):
    """the exploration rule for arrays of draws -> (actions, replaced).  ratio is the fp32 the C ABI carries, widened.  flip_test PLANTS `<` for
    `>` (tests only)"""
    ue, uc = np.atleast_1d(np.asarray(u_explore, np.float64)), np.atleast_1d(np.asarray(u_choice, np.float64))
    out = np.full(len(ue), int(argmax), np.int64)
    where = np.flatnonzero(np.asarray(cand_row)) if cand_row is not None else np.zeros(0, np.int64)
    n = len(where)
    go = ((ue < ratio) if flip_test else (ue > ratio)) & (n > 0)
    if n:
        j = np.minimum(np.floor(uc * n).astype(np.int64), n - 1)
        out[go] = where[j[go]]
    return out, go


def explore_action(argmax, cand_row, u_explore, u_choice, ratio, **kw):
    a, go = explore_actions(argmax, cand_row, [u_explore], [u_choice], ratio, **kw)
    return int(a[0]), bool(go[0])


def actions(ref, cand, mode, draws, ratio, **defects):
    """reference action per row: mode [B] (0..3), draws [B, 3] float64 or None, cand [B, K] bool or None, ratio as given (pass f32(ratio))"""
    B = ref["p"].shape[0]
    out = np.zeros(B, np.int64)
    sd = {k: v for k, v in defects.items() if k == "count_off_by_one"}
    ed = {k: v for k, v in defects.items() if k == "flip_test"}
    for r in range(B):
        m = int(mode[r])
        if m == 0:
            out[r] = -1
        elif not bool(ref["live"][r]):
            out[r] = 0
        elif m == 2:
            out[r] = sample_action(ref, r, float(draws[r, 0]), **sd)
        elif m == 3:
            out[r] = explore_action(int(ref["argmax"][r]), None if cand is None else cand[r], float(draws[r, 1]), float(draws[r, 2]), ratio, **ed)[0]
        else:
            out[r] = int(ref["argmax"][r])
    return out


def intervals(ref, r):
    """row r: the classes with p > 0 as (c, F_lo, F_hi, lo_exact, hi_exact) -- the normalised cdf interval of each and whether its edges are
    exact in any arithmetic (nothing unmasked before / behind it)"""
    p, cdf, Z = ref["p"][r].numpy(), ref["cdf"][r].numpy(), float(ref["Z"][r])
    pos = np.flatnonzero(p > 0)
    out = []
    for i, c in enumerate(pos):
        lo = 0.0 if i == 0 else cdf[pos[i - 1]] / Z
        out.append((int(c), lo, cdf[c] / Z, i == 0, i == len(pos) - 1))
    return out


def decided(ref, r, u, K=None):
    """is the sample draw u on row r outside the margin of every cdf boundary it could be confused across?  (a dead row decides everything: 0)"""
    if not bool(ref["live"][r]):
        return True
    dl = delta(ref["p"].shape[1] if K is None else K)
    c = sample_action(ref, r, u)
    for cc, lo, hi, lo_exact, hi_exact in intervals(ref, r):
        if cc == c:
            return (lo_exact or lo + dl < u) and (hi_exact or u < hi - dl)
    return False
