"""The float64 references of tests/_loss_ref64.py against plain float64 autograd, and the probe layouts against their 100-times-bound condition
(no GPU): GPU tests of the loss and optimizer-tail kernels (csrc/loss.hip, csrc/optim.hip) compare against references shown right here first."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import optim_ref as OR
from tests import _loss_ref64 as R

TOL = 1e-12


def close(a, b, name):
    a, b = a.double(), b.double()
    err = (a - b).abs().max().item()
    assert err <= TOL * max(1.0, b.abs().max().item()), (name, err)


def rn(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("N", [1, 7, 257])
def test_ce_closed_form_is_the_autograd_gradient(N):
    r = rn(N)
    M = 6
    x = (2 * r(M, N)).requires_grad_(True)
    if N > 4:
        x.data[0, 3] = float("-inf")
        x.data[2, 0] = float("-inf")
    labels = torch.tensor([0, N - 1, N // 2, -100, N - 1, N + 3][:M], dtype=torch.int32)       # N + 3: out of range counts as ignored
    row_w = r(M).abs() + 0.1
    ok = (labels >= 0) & (labels < N)
    per = torch.zeros(M, dtype=torch.float64)
    per[ok] = F.cross_entropy(x[ok], labels[ok].long(), reduction="none")
    (0.37 * (per * row_w).sum()).backward()
    ref = R.ce_ref(x.detach(), labels, 0.37, row_w, w_rate=0.7)
    close(ref["loss"], per.detach(), "ce loss")
    close(ref["w"], torch.exp(-0.7 * per.detach()), "ce w")
    close(ref["grad"], torch.nan_to_num(x.grad, nan=0.0), "ce grad")
    assert (ref["grad_env"] >= ref["grad"].abs() - 1e-15).all() and torch.isfinite(ref["grad_env"]).all() and torch.isfinite(ref["loss_env"]).all()


@pytest.mark.parametrize("N", [1, 9, 300])
def test_softkl_closed_form_is_the_autograd_gradient(N):
    r = rn(N + 1)
    M = 4
    x = (2 * r(M, N)).requires_grad_(True)
    t = torch.softmax(r(M, N), 1)
    t[1] = 0.0                                   # a target row of zeros
    t[2] *= 0.5                                  # a row that sums to 0.5
    row_w = r(M).abs() + 0.1
    per = F.kl_div(torch.log_softmax(x, 1), t, reduction="none").sum(1)
    (0.25 * (per * row_w).sum()).backward()
    ref = R.softkl_ref(x.detach(), t, 0.25, row_w)
    close(ref["loss"], per.detach(), "softkl loss")
    close(ref["grad"], x.grad, "softkl grad")
    close(ref["grad"], (0.25 * row_w)[:, None] * (t.sum(1)[:, None] * torch.softmax(x.detach(), 1) - t), "coef (sum_t p - t)")


@pytest.mark.parametrize("N", [1, 13, 130])
def test_kd_rows_reference_is_the_oracle_loss_and_the_closed_form_gradient(N):
    from oracle import makd_ref as MK
    r = rn(N + 2)
    M, T = 5, 2.0
    s, t = 2 * r(M, N), 2 * r(M, N)
    if N > 2:
        s[:, N - 2] = float("-inf")
        t[:, N - 2] = float("-inf")
    w = r(M).abs()
    rows, renv, grad, genv = R.kd_ref(s, t, T, w, norm=0.5, coef=0.6)
    close(rows.sum(), 0.5 * MK.kd_loss(s, t, T, w, "sum"), "kd loss")
    sc = torch.where(s == float("-inf"), torch.full_like(s, -1e6), s) / T
    tc = torch.where(t == float("-inf"), torch.full_like(t, -1e6), t) / T
    want = 0.6 * 0.5 * T * w[:, None] * (torch.softmax(sc, 1) - torch.softmax(tc, 1))
    close(grad, torch.where(s == float("-inf"), torch.zeros_like(s), want), "kd grad")
    assert torch.isfinite(renv).all() and torch.isfinite(genv).all() and (genv >= grad.abs() - 1e-15).all()


@pytest.mark.parametrize("B,H", [(1, 8), (5, 16), (17, 24)])
def test_cfp_closed_form_is_the_autograd_gradient(B, H):
    r = rn(B * H)
    a = [(0.5 * r(B, H)).requires_grad_(True) for _ in range(3)]
    txt = (0.5 * r(B, H)).requires_grad_(True)
    temp, coef = 0.7, 0.37 / B
    ar, tot, want = torch.arange(B), 0.0, []
    for x in a:
        sim = x @ txt.t() / temp
        l1, l2 = F.cross_entropy(sim, ar, reduction="none"), F.cross_entropy(sim.t(), ar, reduction="none")
        want += [l1, l2]
        tot = tot + coef * (l1.sum() + l2.sum())
    tot.backward()
    rows, renv, d_a, d_a_env, d_t, d_t_env = R.cfp_ref([x.detach() for x in a], txt.detach(), temp, coef)
    close(rows, torch.stack(want).detach(), "cfp rows")
    for i in range(3):
        close(d_a[i], a[i].grad, f"cfp d_a{i}")
        assert (d_a_env[i] >= d_a[i].abs() - 1e-15).all()
    close(d_t, txt.grad, "cfp d_txt")


def test_mse_closed_form_with_strides_weights_and_valid_extents():
    r = rn(5)
    outer, inner, ss, ts = 6, 24, 40, 56
    S, Tt = r(outer, ss).requires_grad_(True), r(outer, ts)
    w = r(2).abs()
    vo, vi, vm = 5, 5, 8
    o, c = torch.arange(outer)[:, None], torch.arange(inner)[None, :]
    mask = ((o < vo) & (c % vm < vi)).double()
    loss = 0.25 * (w[torch.arange(outer) // 3][:, None] * mask * (S[:, :inner] - Tt[:, :inner]) ** 2).sum()
    (0.8 * loss).backward()
    terms, grad = R.mse_ref(S.detach()[:, :inner], Tt[:, :inner], w, 3, norm=0.25, coef=0.8, valid=(vo, vi), valid_mod=vm)
    close(terms.sum(), loss.detach(), "mse loss")
    close(grad, S.grad[:, :inner], "mse grad")
    assert (S.grad[:, inner:] == 0).all()
    terms, grad = R.mse_ref(S.detach()[:, :inner], Tt[:, :inner], None, 1, norm=1.0, coef=1.0)
    close(terms.sum(), ((S.detach()[:, :inner] - Tt[:, :inner]) ** 2).sum(), "mse plain")


@pytest.mark.parametrize("decay_first", [False, True])
def test_adamw_restatement_against_torch_and_the_oracle(decay_first):
    """both sides get the SAME fp32-rounded eps and step size (the kernel's arguments), so they agree to 1e-12: torch.optim.AdamW takes them through
    its per-step lr / eps / weight_decay (host/trainer.py's identity: eps sqrt(bc2), lr sqrt(bc2) / bc1), the oracle through correct_bias=False"""
    r = rn(9)
    n, lr, b1, b2, eps, wd = 50, 1e-2, 0.9, 0.98, 1e-6, 0.1
    b1f, b2f, lw = R.f32(b1), R.f32(b2), R.f32(lr) * R.f32(wd)
    p0, gs = r(n), [r(n) for _ in range(3)]
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    if decay_first:
        tp = p0.clone().requires_grad_(True)
        opt = torch.optim.AdamW([tp], lr=lr, betas=(b1f, b2f), eps=eps, weight_decay=wd)
    else:
        op, st = [p0.clone()], OR.adamw_init([p0])
    for t, g in enumerate(gs, 1):
        bc1, bc2 = 1 - b1f ** t, 1 - b2f ** t
        eps_k, ss = R.f32(eps * math.sqrt(bc2)), R.f32(lr * math.sqrt(bc2) / bc1)              # what the kernel is handed
        p, m, v, *_ = R.adamw_ref(p, g, m, v, lr=lr, b1=b1, b2=b2, eps=eps_k, wd=wd, step_size=ss, decay_first=decay_first)
        if decay_first:
            grp = opt.param_groups[0]
            grp["lr"] = ss * bc1 / math.sqrt(bc2)
            grp["eps"] = eps_k / math.sqrt(bc2)
            grp["weight_decay"] = lw / grp["lr"]
            tp.grad = g.clone()
            opt.step()
            close(p, tp.detach(), f"p against torch.optim.AdamW, step {t}")
        else:
            OR.adamw_step(op, [g], st, ss, betas=(b1f, b2f), eps=eps_k, weight_decay=lw / ss, correct_bias=False)
            close(p, op[0], f"p against the oracle, step {t}")
            close(m, st["m"][0], "m")
            close(v, st["v"][0], "v")


def test_adamw_restatement_decays_only_below_n_decay():
    r = rn(3)
    n = 10
    p, g = r(n), r(n)
    z = torch.zeros(n, dtype=torch.float64)
    kw = dict(lr=1e-2, b1=0.9, b2=0.98, eps=1e-6, wd=0.1, step_size=1e-2)
    full, *_ = R.adamw_ref(p, g, z, z, n_decay=-1, **kw)
    none, *_ = R.adamw_ref(p, g, z, z, n_decay=0, **kw)
    half, *_ = R.adamw_ref(p, g, z, z, n_decay=5, **kw)
    assert torch.equal(half[:5], full[:5]) and torch.equal(half[5:], none[5:]) and not torch.equal(full[5:], none[5:])


def test_assemble_and_dact_references():
    r = rn(4)
    rows, row_w, kd, slots, rw = r(40), r(40).abs(), r(7), r(10), r(5).abs()
    out, env, s9, terms = R.assemble_ref(rows, row_w, 0.5, kd, slots, rw, 0.25, True)
    sup = 0.5 * (rows * row_w).sum()
    sl = slots.clone()
    sl[9] = kd.sum()
    t = sl * rw[torch.tensor([0, 0, 1, 1, 1, 2, 2, 3, 3, 4])]
    close(out, torch.cat([sup[None], t, t.sum()[None], (0.25 * t.sum() + 0.75 * sup)[None]]), "assemble")
    close(terms.sum(), sup, "assemble terms")
    out, env, _, _ = R.assemble_ref(rows, None, 0.5, None, slots, None, 0.25, False)
    close(out, torch.cat([0.5 * rows.sum()[None], torch.zeros(11, dtype=torch.float64), 0.5 * rows.sum()[None]]), "assemble no kd")
    z = r(64).requires_grad_(True)
    dy = r(64)
    (F.gelu(z) * dy).sum().backward()
    close(R.dact_ref(dy, z.detach(), 1)[0], z.grad, "dgelu")
    close(R.dact_ref(dy, z.detach(), 2)[0], dy * (z.detach() > 0), "drelu")


SUMSQ_N = [1, 2, 3, 5, 4095, 4097, 2 ** 20 + 3, 4 * 256 * 1024 * 4 + 7]


@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq_probe_layout_meets_the_100_bound_condition(n):
    pos = R.sumsq_seams(n)
    assert pos[0] == 0 and pos[-1] == n - 1 and len(pos) <= 64
    if n > 4 * 256 * 1024 * 4:                 # the second trip of the four-in-flight loop, and its scalar tail
        assert 4 * 256 * 1024 * 4 in pos and n - (n & 3) in pos
    x = R.probe_data(n, pos, 1e-3, 8.0, n)
    assert R.probes_ok(x * x, pos)


def test_mse_and_assemble_probe_layouts_meet_the_100_bound_condition():
    for outer, inner, block, grid in ((7, 15001, 256, 384), (9, 8 * 29131, 8 * 1024, 256)):
        pos = R.mse_seams(outer, inner, block, grid)
        d = R.probe_data(outer * inner, pos, 1e-2, 4.0, inner)
        assert len(pos) <= 80 and R.probes_ok(0.5 * d * d, pos), (outer, inner)
    for n in (1, 255, 257, 1000):
        pos = R.seams(n, (64, 256))
        assert R.probes_ok(R.probe_data(n, pos, 1e-3, 8.0, n), pos), n


# ------------------------------------------------------------------------------------------ the comparison machinery itself
def _fp32_ce(x, labels, coef, row_w, rate, dtype):
    """what a correct kernel returns: the same mathematics in fp32 from the stored logits, the gradient rounded to the storage type"""
    x32 = x.float()
    lse = torch.logsumexp(x32, 1)
    ok = labels >= 0
    lab = labels.clamp_min(0).long()
    loss = torch.where(ok, lse - x32.gather(1, lab[:, None])[:, 0], torch.zeros_like(lse))
    hot = torch.zeros_like(x32)
    hot[torch.arange(x.shape[0])[ok], lab[ok]] = 1.0
    cf = torch.where(ok, coef * row_w.float(), torch.zeros_like(lse))
    return loss, torch.exp(-rate * loss), (cf[:, None] * (torch.exp(x32 - lse[:, None]) - hot)).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_check_passes_fp32_arithmetic_and_fails_a_reference_without_the_last_column(dtype):
    r = rn(21)
    M, N = 6, 300
    x = (2 * r(M, N)).to(dtype)
    x[:, N - 1] = 4.0
    x[0, 3] = float("-inf")
    labels = torch.tensor([0, N - 1, 296, -100, 150, 7], dtype=torch.int32)
    row_w = (r(M).abs() + 0.25).float()
    fam = f"self {dtype}"
    loss, w, grad = _fp32_ce(x, labels, 0.37, row_w, 0.7, dtype)
    ref = R.ce_ref(x, labels, 0.37, row_w, w_rate=0.7)
    c = R.ce_ref(x[:, :N - 1], labels, 0.37, row_w, w_rate=0.7)
    R.check(fam, "loss", loss, ref["loss"], ref["loss_env"], ctrl=c["loss"])
    R.check(fam, "w", w, ref["w"], ref["w_env"], ctrl=c["w"])
    assert R.check(fam, "grad", grad, ref["grad"], ref["grad_env"], dtype, ctrl=R.pad_cols(c["grad"], N)) <= 1.0
    assert 0 < R.WORST[fam] <= 1.0
    # a gradient without its last column, or off by 2.5 bounds in one element, is refused
    bad = grad.clone()
    bad[:, N - 1] = 0
    with pytest.raises(AssertionError, match="max err/bound"):
        R.check("self bad", "grad", bad, ref["grad"], ref["grad_env"], dtype)
    bad = grad.double().clone()
    bad[1, 5] += 2.5 * R.bound(ref["grad"], ref["grad_env"], dtype)[1, 5]
    with pytest.raises(AssertionError, match="max err/bound"):
        R.check("self bad", "grad", bad, ref["grad"], ref["grad_env"], dtype)
    # a control that lacks nothing is reported as a bound that cannot see
    with pytest.raises(AssertionError, match="cannot see"):
        R.check("self", "grad", grad, ref["grad"], ref["grad_env"], dtype, ctrl=ref["grad"])
    nan = grad.clone()
    nan[0, 0] = float("nan")
    assert R.ratio(nan, ref["grad"], R.bound(ref["grad"], ref["grad_env"], dtype)) == float("inf")


def test_bound_is_rel_of_the_envelope_plus_one_unit_in_the_last_place():
    ref, env = torch.tensor([2.0, 0.0], dtype=torch.float64), torch.tensor([3.0, 0.0], dtype=torch.float64)
    assert torch.allclose(R.bound(ref, env), torch.tensor([3e-5, 1e-30], dtype=torch.float64), rtol=1e-12, atol=0)
    assert torch.allclose(R.bound(ref, env, torch.bfloat16), torch.tensor([2.0 ** -6 + 3e-5, 1e-30], dtype=torch.float64), rtol=1e-12, atol=0)
    assert torch.allclose(R.bound(ref, env, torch.float16), torch.tensor([2.0 ** -9 + 3e-5 + 6e-8, 6e-8], dtype=torch.float64), rtol=1e-12, atol=0)
    assert torch.allclose(R.bound(ref, env, factor=4.0), torch.tensor([12e-5, 1e-30], dtype=torch.float64), rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", ["softkl", "kd", "cfp"])
def test_envelopes_admit_fp32_arithmetic_and_refuse_a_missing_column(name):
    """each envelope is wide enough for the same mathematics in fp32 and tight enough that a reference without the last column / sample fails"""
    r = rn(33)
    if name == "softkl":
        M, N = 3, 257
        x, t = (2 * r(M, N)).float(), torch.softmax(r(M, N), 1).float()
        t[1] = 0
        t[2] *= 0.5
        lp = torch.log_softmax(x, 1)
        loss = F.kl_div(lp, t, reduction="none").sum(1)
        grad = 0.37 * (t.sum(1)[:, None] * lp.exp() - t)
        ref, c = R.softkl_ref(x, t, 0.37), R.softkl_ref(x[:, :N - 1], t[:, :N - 1], 0.37)
        R.check("self", "softkl loss", loss, ref["loss"], ref["loss_env"], ctrl=c["loss"])
        R.check("self", "softkl grad", grad, ref["grad"], ref["grad_env"], ctrl=R.pad_cols(c["grad"], N))
    elif name == "kd":
        M, N, T = 5, 129, 2.0
        s, t = (2 * r(M, N)).float(), (2 * r(M, N)).float()
        s[:, 7] = t[:, 7] = float("-inf")
        sc, tc = torch.where(s == float("-inf"), torch.full_like(s, -1e6), s) / T, torch.where(t == float("-inf"), torch.full_like(t, -1e6), t) / T
        ls, lt = torch.log_softmax(sc, 1), torch.log_softmax(tc, 1)
        rows = (torch.where(lt.exp() > 0, lt.exp() * (lt - ls), torch.zeros_like(ls))).sum(1) * T * T
        grad = 0.6 * T * (ls.exp() - lt.exp())
        rr, renv, g, genv = R.kd_ref(s, t, T, coef=0.6)
        cr, _, cg, _ = R.kd_ref(s[:, :N - 1], t[:, :N - 1], T, coef=0.6)
        R.check("self", "kd loss", rows, rr, renv, ctrl=cr)
        R.check("self", "kd grad", grad, g, genv, ctrl=R.pad_cols(cg, N))
    else:
        B, H, temp, coef = 17, 72, 0.7, 0.37 / 17
        a = [(0.5 * r(B, H)).float().requires_grad_(True) for _ in range(3)]
        txt = (0.5 * r(B, H)).float().requires_grad_(True)
        ar, tot, want = torch.arange(B), 0.0, []
        for x in a:
            sim = x @ txt.t() / temp
            l1, l2 = F.cross_entropy(sim, ar, reduction="none"), F.cross_entropy(sim.t(), ar, reduction="none")
            want += [l1, l2]
            tot = tot + coef * (l1.sum() + l2.sum())
        tot.backward()
        det = [x.detach() for x in a]
        rows, renv, d_a, d_a_env, d_t, d_t_env = R.cfp_ref(det, txt.detach(), temp, coef)
        cr, _, ca, _, ct, _ = R.cfp_ref([x[:B - 1] for x in det], txt.detach()[:B - 1], temp, coef)
        pad = lambda m: torch.cat([m, m.new_zeros((1,) + m.shape[1:])], 0)
        R.check("self", "cfp rows", torch.stack(want).detach(), rows, renv, ctrl=R.pad_cols(cr, B))
        R.check("self", "cfp d_a", a[0].grad, d_a[0], d_a_env[0], ctrl=pad(ca[0]))
        R.check("self", "cfp d_txt", txt.grad, d_t, d_t_env, ctrl=pad(ct))


def test_check_probes_sees_every_probe_and_nothing_else():
    n = 4097
    pos = R.sumsq_seams(n)
    g = R.probe_data(n, pos, 1e-3, 8.0, n).float()
    terms = g.double() ** 2
    got = (g * g).sum() + 2.0                                   # an fp32 sum on top of what the word held
    assert R.check_probes("self", "sumsq", got, 2.0, terms, pos) <= 1.0
    for p in (pos[0], pos[len(pos) // 2], pos[-1]):              # a sum that lacks one probe element is refused
        with pytest.raises(AssertionError, match="err/bound"):
            R.check_probes("self", "sumsq", got - terms[p].float(), 2.0, terms, pos)
    with pytest.raises(AssertionError, match="below 100 bounds"):   # an element of the noise is no probe
        R.check_probes("self", "sumsq", got, 2.0, terms, pos + [10])
    with pytest.raises(AssertionError, match="err/bound"):
        R.check_probes("self", "sumsq", torch.tensor(float("nan")), 2.0, terms, pos)


def test_clip_and_schedule_references_are_the_formulas_of_the_optimizer_kernels():
    """csrc/optim.hip adamw_kernel: clip = gscale min(1, max_norm / (sqrt(sumsq) gscale + 1e-6)), plain gscale without a norm word or with
    max_norm <= 0; sched_advance: lr = lr0 warmup_linear(global step), <= 0 -> 1e-8; step size = lr sqrt(1 - b2^t) / (1 - b1^t)"""
    f = torch.float32
    for sumsq, max_norm, gscale in ((400.0, 5.0, 0.125), (400.0, 1.0, 0.125), (1e-4, 5.0, 1.0), (7.0, 0.3, 0.5)):
        nrm = torch.sqrt(torch.tensor(sumsq, dtype=f)) * torch.tensor(gscale, dtype=f)
        want = torch.tensor(gscale, dtype=f) * torch.minimum(torch.tensor(1.0, dtype=f), torch.tensor(max_norm, dtype=f) / (nrm + torch.tensor(1e-6, dtype=f)))
        got = R.clip_ref(sumsq, max_norm, gscale)
        assert abs(got - want.item()) <= 4 * 2.0 ** -24 * got, (sumsq, max_norm, gscale)
        assert (got < R.f32(gscale)) == (math.sqrt(sumsq) * gscale > max_norm)
    assert R.clip_ref(None, 5.0, 0.125) == 0.125 and R.clip_ref(400.0, 0.0, 0.125) == 0.125
    for gs, t in ((0, 1), (3, 4), (10, 11), (50, 41), (1000, 7), (2000, 7)):
        lr, ss = R.sched_ref(gs, t, 1e-3, 10, 1000, 0.9, 0.98)
        want_lr = OR.get_lr_sched(gs, R.f32(1e-3), 10, 1000)
        assert abs(lr - want_lr) <= 1e-15 * want_lr, gs
        want_ss = want_lr * math.sqrt(1 - R.f32(0.98) ** t) / (1 - R.f32(0.9) ** t)
        assert abs(ss - want_ss) <= 1e-15 * want_ss, (gs, t)
    assert R.sched_ref(0, 1, 1e-3, 10, 1000, 0.9, 0.98)[0] == 1e-8 and R.sched_ref(2000, 7, 1e-3, 10, 1000, 0.9, 0.98)[0] == 1e-8
