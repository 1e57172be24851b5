"""Float64 references, bounds and probe layouts of the loss and optimizer-tail kernels (csrc/loss.hip, csrc/optim.hip).

For the GPU tests of those kernels (device-agnostic: the same code runs on the device there) and for tests/test_loss_ref64_cpu.py, which checks
every closed form here against plain float64 autograd, and every probe layout against its 100-times-bound condition.  Nothing here launches a kernel or rounds
anything "the way the kernel would": a reference takes the operands the kernel reads (16-bit logits as stored, fp32 targets / weights / moments as
passed, scalars rounded to the fp32 the C ABI carries) and works in float64 from there.

Bound of every comparison: REL times the envelope (the sum of the absolute values of the terms that form the output), plus one unit in the last
place of the storage type where the output is 16-bit -- the figures of check_dx in tests/test_partial_rows_gpu.py."""
import math

import torch

REL = 1e-5
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
WORST = {}                                                # family -> largest err / bound seen in this process


def f32(x):
    """a Python scalar as the fp32 the C ABI passes"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def bound(ref, env, dtype=torch.float32, factor=1.0):
    floor = 6e-8 if dtype == torch.float16 else 1e-30
    return ULP.get(dtype, 0.0) * ref.abs() + REL * factor * env + floor


def ratio(got, ref, bnd):
    """max err / bound (inf where got is not finite)"""
    got = got.double()
    if not torch.isfinite(got).all():
        return float("inf")
    if got.numel() == 0:
        return 0.0
    return ((got - ref).abs() / bnd).max().item()


def check(family, name, got, ref, env, dtype=torch.float32, ctrl=None, factor=1.0):
    """got within bound(ref, env); and, for every reference in ctrl (each lacks one unit of work), the SAME comparison fails"""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bnd = bound(ref, env, dtype, factor)
    r = ratio(got, ref, bnd)
    WORST[family] = max(WORST.get(family, 0.0), r)
    print(f"FP64 {family:14s} {r:9.3g}  {name}")
    assert r <= 1.0, f"{name}: max err/bound {r:.3g}"
    for i, c in enumerate(ctrl if isinstance(ctrl, (list, tuple)) else ([] if ctrl is None else [ctrl])):
        assert ratio(got, c, bnd) > 1.0, f"{name}: the bound cannot see missing unit {i}"
    return r


def check_probes(family, name, got, init, terms, probes, factor=1.0):
    """got (one fp32 word) = init + sum(terms); every probe position alone must break the comparison and be worth 100 bounds"""
    terms = terms.reshape(-1)
    ref = init + terms.sum()
    bnd = REL * factor * (abs(init) + terms.abs().sum()) + 1e-30
    r = (abs(float(got) - ref) / bnd).item() if math.isfinite(float(got)) else float("inf")
    WORST[family] = max(WORST.get(family, 0.0), r)
    print(f"FP64 {family:14s} {r:9.3g}  {name} ({len(probes)} probes)")
    assert r <= 1.0, f"{name}: err/bound {r:.3g}"
    pv = terms[torch.as_tensor(probes, device=terms.device)]
    assert (pv.abs() > 100 * bnd).all(), f"{name}: a probe is below 100 bounds"
    miss = (float(got) - (ref - pv)).abs() > bnd                  # the same comparison against a reference without that one element
    assert miss.all(), f"{name}: the bound cannot see element(s) {[probes[i] for i in (~miss).nonzero().flatten().tolist()]}"
    return r


def probes_ok(terms, probes, init=0.0, factor=1.0):
    terms = terms.reshape(-1)
    bnd = REL * factor * (abs(init) + terms.abs().sum())
    return bool((terms[torch.as_tensor(probes)].abs() > 100 * bnd).all())


# ------------------------------------------------------------------------------------------ probe layouts
def _uniq(pos, n):
    return sorted({int(p) for p in pos if 0 <= p < n})


def seams(n, units):
    """first, last, and each side of every multiple of every unit (capped at 6 multiples per unit, plus the last one)"""
    pos = [0, n - 1]
    for u in units:
        ks = list(range(1, 7)) + [(n - 1) // u]
        for k in ks:
            pos += [k * u - 1, k * u]
    return _uniq(pos, n)


def sumsq_seams(n):
    """magic_sumsq: float4 loads, 1024-thread blocks, at most 256 of them (one per 4096 elements), four strides in flight, scalar tail n & 3"""
    grid = min(256, max(1, (n + 4095) // 4096))
    stride = grid * 1024 * 4
    return _uniq(seams(n, (4, 4096, stride, 4 * stride)) + list(range(n - (n & 3) - 1, n)), n)


def mse_seams(outer, inner, block, grid):
    return seams(outer * inner, (8, inner, block, block * grid, 2 * block * grid))


def probe_data(n, probes, noise, big, seed, dtype=torch.float64):
    """small noise everywhere, +-big at the probe positions"""
    g = torch.Generator().manual_seed(seed)
    x = noise * torch.randn(n, generator=g, dtype=torch.float64)
    idx = torch.as_tensor(probes)
    x[idx] = big * (1.0 - 2.0 * (torch.arange(len(probes)) % 2).double())
    return x.to(dtype)


# ------------------------------------------------------------------------------------------ softmax pieces
def _lse(x):
    """x float64 [M, N] (may hold -inf, never a whole row): lse, its envelope |max| + |log s|, p and p's envelope p (1 + |x - lse|)"""
    mx = x.max(1).values
    lse = torch.logsumexp(x, 1)
    z = x - lse[:, None]
    p = z.exp()
    penv = torch.where(p > 0, p * (1 + z.abs()), torch.zeros_like(p))
    return lse, mx.abs() + (lse - mx).abs(), p, penv


def ce_ref(x, labels, coef, row_w=None, ignore_index=-100, w_rate=0.0):
    """cross-entropy rows of x[M, N] (as stored): dict of loss, w_out = exp(-rate loss), grad = coef row_w (p - onehot), and their envelopes"""
    x = x.double()
    M, N = x.shape
    lab = labels.long()
    ign = (lab == ignore_index) | (lab < 0) | (lab >= N)
    safe = torch.where(ign, torch.zeros_like(lab), lab)
    lse, lenv, p, penv = _lse(x)
    xl = x.gather(1, safe[:, None])[:, 0]
    zero = torch.zeros_like(lse)
    loss = torch.where(ign, zero, lse - xl)
    loss_env = torch.where(ign, zero, lenv + xl.abs())
    w = (-w_rate * loss).exp()
    w_env = w * (1 + abs(w_rate) * (loss.abs() + loss_env))
    cf = torch.full_like(lse, float(coef)) * (row_w.double() if row_w is not None else 1.0)
    cf = torch.where(ign, zero, cf)
    hot = torch.zeros_like(x)
    hot[torch.arange(M, device=x.device)[~ign], safe[~ign]] = 1.0
    return dict(loss=loss, loss_env=loss_env, w=w, w_env=w_env, grad=cf[:, None] * (p - hot), grad_env=cf.abs()[:, None] * (penv + hot))


def pad_cols(t, n):
    return torch.cat([t, t.new_zeros(t.shape[0], n - t.shape[1])], 1) if t.shape[1] < n else t


def softkl_ref(x, t, coef, row_w=None):
    """loss = sum_j t (log t - log p) over t > 0 ; grad = coef row_w ((sum_j t) p - t)"""
    x, t = x.double(), t.double()
    lse, lenv, p, penv = _lse(x)
    pos = t > 0
    lt = torch.where(pos, t.clamp_min(1e-300).log(), torch.zeros_like(t))
    loss = torch.where(pos, t * (lt - x + lse[:, None]), torch.zeros_like(t)).sum(1)
    st = t.sum(1)
    loss_env = torch.where(pos, t * (lt.abs() + x.abs()), torch.zeros_like(t)).sum(1) + t.abs().sum(1) * (lse.abs() + lenv)
    cf = torch.full_like(lse, float(coef)) * (row_w.double() if row_w is not None else 1.0)
    return dict(loss=loss, loss_env=loss_env, grad=cf[:, None] * (st[:, None] * p - t),
                grad_env=cf.abs()[:, None] * (t.abs().sum(1)[:, None] * penv + t.abs()))


def kd_ref(s, t, T, w=None, norm=1.0, coef=0.0):
    """temperature KL rows through oracle.makd_ref.kd_loss in float64, row by row, and the autograd gradient of sum_r coef w_r norm kd_loss(row r).
    Returns loss rows, their envelope, the gradient (0 where the student logit is -inf) and its envelope"""
    from oracle import makd_ref as MK
    s64 = s.double().clone().requires_grad_(True)
    t64 = t.double()
    M = s64.shape[0]
    wr = w.double() if w is not None else torch.ones(M, dtype=torch.float64, device=s.device)
    rows = torch.stack([MK.kd_loss(s64[r:r + 1], t64[r:r + 1], T) for r in range(M)]) * wr * norm
    (coef * rows.sum()).backward()
    grad = torch.nan_to_num(s64.grad, nan=0.0)
    neg = float("-inf")
    sc = torch.where(s64.detach() == neg, torch.full_like(t64, -1e6), s64.detach()) / T
    tc = torch.where(t64 == neg, torch.full_like(t64, -1e6), t64) / T
    ls, lsenv, ps, psenv = _lse(sc)
    lt, ltenv, pt, ptenv = _lse(tc)
    kenv = (pt * ((tc - lt[:, None]).abs() + (sc - ls[:, None]).abs())).sum(1) + lsenv + ltenv
    return rows.detach(), wr.abs() * abs(norm) * T * T * kenv, grad, abs(coef * norm * T) * wr.abs()[:, None] * (psenv + ptenv)


def mse_ref(s, t, w=None, rows_per_w=1, norm=1.0, coef=0.0, valid=None, valid_mod=0):
    """s, t [outer, inner] (the strided views the kernel walks).  Returns the loss terms norm w d^2 (their sum is the loss word) and the gradient
    2 coef norm w d; valid = (rows, columns): only o < rows and (r mod valid_mod) < columns count"""
    s, t = s.double(), t.double()
    outer, inner = s.shape
    d = s - t
    if valid is not None:
        o = torch.arange(outer, device=s.device)[:, None]
        r = torch.arange(inner, device=s.device)[None, :]
        d = torch.where((o < valid[0]) & ((r % valid_mod if valid_mod > 0 else r) < valid[1]), d, torch.zeros_like(d))
    wv = w.double()[torch.arange(outer, device=s.device) // rows_per_w][:, None] if w is not None else 1.0
    return norm * wv * d * d, 2.0 * coef * norm * wv * d


def cfp_ref(a, txt, temp, coef):
    """the three contrastive terms in closed form: rows [6, B], gradients of coef sum(rows) wrt each a_i and txt, and envelopes"""
    t = txt.double()
    B = t.shape[0]
    eye = torch.eye(B, dtype=torch.float64, device=t.device)
    rows, rows_env, d_a, d_a_env = [], [], [], []
    d_t, d_t_env = torch.zeros_like(t), torch.zeros_like(t)
    for x in a:
        x = x.double()
        sim = x @ t.t() / temp
        senv = (x.abs() @ t.abs().t()) / temp                       # the dot product's own envelope
        for mat, e in ((sim, senv), (sim.t(), senv.t())):
            lse, lenv, _, _ = _lse(mat)
            rows.append(lse - mat.diagonal())
            rows_env.append(lenv + mat.diagonal().abs() + e.max(1).values + e.diagonal())
        _, _, pr, prenv = _lse(sim)
        _, _, pc, pcenv = _lse(sim.t())
        G = coef * ((pr - eye) + (pc.t() - eye))
        # a similarity off by d moves its probabilities by p (d - sum_k p_k d_k): the entry's own dot-product envelope and its row's / column's mean
        Genv = abs(coef) * (prenv + pcenv.t() + 2 * eye + (pr + pc.t()) * senv + pr * (pr * senv).sum(1, keepdim=True) + pc.t() * (pc.t() * senv).sum(0, keepdim=True))
        d_a.append(G @ t / temp)
        d_a_env.append((Genv @ t.abs()) / temp)
        d_t += G.t() @ x / temp
        d_t_env += (Genv.t() @ x.abs()) / temp
    return torch.stack(rows), torch.stack(rows_env), d_a, d_a_env, d_t, d_t_env


def assemble_ref(rows, row_w, row_scale, kd_rows, slots, rw, alpha, has_kd):
    """loss_assemble: out[13] and its envelope, plus the two row sums' terms (for the probes)"""
    r = rows.double() * (row_w.double() if row_w is not None else 1.0)
    row_scale, alpha = f32(row_scale), f32(alpha)
    sup, sup_env = r.sum() * row_scale, r.abs().sum() * abs(row_scale)
    slots = slots.double().clone()
    senv = slots.abs()
    if kd_rows is not None:
        slots[9], senv[9] = kd_rows.double().sum(), kd_rows.double().abs().sum()
    ab = torch.tensor([0, 0, 1, 1, 1, 2, 2, 3, 3, 4], device=rows.device)
    wgt = rw.double()[ab] if rw is not None else torch.ones(10, dtype=torch.float64, device=rows.device)
    terms = slots * wgt if has_kd else torch.zeros_like(slots)
    tenv = senv * wgt.abs() if has_kd else torch.zeros_like(slots)
    kdl, kenv = terms.sum(), tenv.sum()
    loss = alpha * kdl + (1 - alpha) * sup if has_kd else sup
    lenv = abs(alpha) * kenv + abs(1 - alpha) * sup_env if has_kd else sup_env
    out = torch.cat([sup[None], terms, kdl[None], loss[None]])
    env = torch.cat([sup_env[None], tenv, kenv[None], lenv[None]])
    return out, env, slots[9], r * row_scale


def adamw_ref(p, g, m, v, *, lr, b1, b2, eps, wd, step_size, clip=1.0, n_decay=-1, decay_first=False):
    """the kernel's documented formula (csrc/optim.hip adamw_kernel) in float64; scalars as the fp32 the ABI carries.  Returns p, m, v and the
    per-element bound envelopes of each"""
    lr, b1, b2, eps, wd, step_size = (f32(x) for x in (lr, b1, b2, eps, wd, step_size))
    p, g, m, v = p.double(), g.double() * clip, m.double(), v.double()
    n = p.numel()
    nd = n if n_decay < 0 else n_decay
    dec = (torch.arange(n, device=p.device) < nd) & (wd > 0)
    mi = b1 * m + (1 - b1) * g
    vi = b2 * v + (1 - b2) * g * g
    pi = p.clone()
    if decay_first:
        pi = torch.where(dec, pi - lr * wd * pi, pi)
    upd = step_size * mi / (vi.sqrt() + eps)
    pi = pi - upd
    if not decay_first:
        pi = torch.where(dec, pi - lr * wd * pi, pi)
    penv = p.abs() + (lr * wd * p).abs() + upd.abs()
    return pi, mi, vi, penv, (b1 * m).abs() + ((1 - b1) * g).abs(), (b2 * v).abs() + (1 - b2) * g * g


def clip_ref(sumsq, max_norm, gscale):
    """the factor the kernel multiplies every gradient element by"""
    gscale, max_norm = f32(gscale), f32(max_norm)
    if sumsq is None or max_norm <= 0:
        return gscale
    nrm = math.sqrt(float(sumsq)) * gscale
    return gscale * min(1.0, max_norm / (nrm + f32(1e-6)))


def dact_ref(dy, z, kind):
    dy, z = dy.double(), z.double()
    if kind == 2:
        d = (z > 0).double()
        return dy * d, dy.abs() * d
    cdf_e = 0.5 * torch.erf(z / math.sqrt(2.0))
    zpdf = z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return dy * (0.5 + cdf_e + zpdf), dy.abs() * (0.5 + cdf_e.abs() + zpdf.abs())


def sched_ref(gs, t, lr0, warmup, total, b1, b2):
    """lr and the bias-corrected step size of global step gs, optimizer state step t (after the advance)"""
    lr0, b1, b2 = f32(lr0), f32(b1), f32(b2)
    f = gs / warmup if gs < warmup else max(0.0, (total - gs) / (total - warmup))
    lr = lr0 * f
    if lr <= 0:
        lr = 1e-8
    return lr, lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
