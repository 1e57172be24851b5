"""Partial-row parameter gradients against float64 references, in the form a backward pass uses (-m gpu).

Inside a backward pass (the weight-gradient queue active) the row kernels store every workgroup's parameter-gradient sums in its own row of a
scratch buffer and the flush adds the rows up in block order.  The host sizes those buffers from its own row count while the launch sizes its grid:
the seam in host/ops.py (`PART_POISON`) allocates every buffer with as many guard rows again behind it, all NaN, so a row the host counted but no
workgroup wrote shows up as a non-finite gradient and a row written past the count as a guard row that is no longer NaN.  The count also travels to the
launch as an argument, and every entry point refuses one that is not its grid before it launches anything (the `refuses` cases).

Every reference is built in float64 from the operands the kernel reads (the stored 16-bit y, fp32 rstd / gamma / beta, dy as passed), and every fp32
parameter-gradient sum is held to 1e-5 of the sum of its rows' absolute contributions.  Each partial-row case also shows that the same check FAILS
against a reference without the last workgroup's rows: the tolerance is tighter than one workgroup at that shape."""
import ctypes as C

import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from magic_amd.host import ops as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
REL = 1e-5
LNB_R = {128: 64, 256: 32, 384: 8, 768: 8}          # rows per workgroup and grid-stride turn of magic_ln_bwd (H = 768: lean 8 x 1, or 4 x 2 with tables)
LNB_CAP = 512                                       # its grid cap with gamma / beta gradients


@pytest.fixture
def poison(monkeypatch):
    """partial rows on at every width, every partial-row buffer NaN-filled with guard rows; yields the list of [buffer, rows used]"""
    guards = []
    monkeypatch.setattr(O, "PART_PG", True)
    monkeypatch.setattr(O, "PART_MIN_H", 128)
    monkeypatch.setattr(O, "PART_POISON", True)
    monkeypatch.setattr(O, "PART_GUARDS", guards)
    return guards


def check_guards(guards):
    """every counted row written (finite), every guard row untouched (NaN); returns how many buffers were checked"""
    torch.cuda.synchronize()
    for i, (full, n) in enumerate(guards):
        assert full.dim() == 3 and full.shape[1] >= 2 * n
        assert torch.isfinite(full[:, :n]).all(), f"partial buffer {i} {tuple(full.shape)}: a counted row was left unwritten (rows used {n})"
        assert torch.isnan(full[:, n:]).all(), f"partial buffer {i} {tuple(full.shape)}: a row past the host's count {n} was written"
    n = len(guards)
    guards.clear()
    return n


def run(partial, launch):
    """launch() outside a backward pass (the atomic form) or inside one (partial rows + the flush)"""
    if partial:
        O.defer_dw(True)
        try:
            launch()
            O.flush_dw()
        finally:
            O.defer_dw(False)
    else:
        launch()
    torch.cuda.synchronize()


def gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)


def within(got, ref, bound):
    return ((got.double() - ref).abs() <= bound).all().item()


def check_sum(got, init, terms, env, name, block=None, nblk=None):
    """got (fp32) = init + sum over rows (dim 0) of terms; |err| <= 1e-5 (|init| + sum of the rows' envelopes env >= |terms|).  block: the workgroup of
    every row -- the same check against a reference without the last workgroup's rows must fail"""
    got = got.double()
    bound = REL * (init.double().abs() + env.sum(0)) + 1e-30
    ref = init.double() + terms.sum(0)
    err = (got - ref).abs()
    assert torch.isfinite(got).all(), f"{name}: not finite"
    assert (err <= bound).all(), f"{name}: max err/bound {(err / bound).max().item():.3g}"
    if block is not None:
        keep = block != nblk - 1
        ref_d = init.double() + terms[keep].sum(0)
        assert not within(got, ref_d, bound), f"{name}: the tolerance cannot see the last workgroup's rows ({int((~keep).sum())} of {len(keep)})"


def check_dx(got, ref, env, name, dtype):
    """16-bit: one unit in the last place + the fp32 arithmetic (1e-5 of the terms' envelope env); fp32: 1e-5 relative to the terms"""
    ulp = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}.get(dtype, 0.0)
    bound = ulp * ref.abs() + REL * (ref.abs() + env) + (6e-8 if dtype == torch.float16 else 1e-30)
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all(), f"{name}: not finite"
    assert (err <= bound).all(), f"{name}: max err/bound {(err / bound).max().item():.3g}"


def ln_bwd64(dy, y, gamma, beta, rstd):
    """LayerNorm backward in float64 from what the kernel reads: x-hat rebuilt from the stored y.  Returns dx, the envelope of dx's terms, x-hat"""
    dy, y, g, b, r = dy.double(), y.double(), gamma.double(), beta.double(), rstd.double()[:, None]
    xh = (y - b) / g
    gg = dy * g
    m1, m2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    dx = r * (gg - m1 - xh * m2)
    env = r * (gg.abs() + gg.abs().mean(1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(1, keepdim=True))
    return dx, env, xh


def scatter(rows_to, vals, n):
    out = torch.zeros(n, vals.shape[1], dtype=torch.float64, device=vals.device)
    return out.index_add_(0, rows_to, vals)


# ------------------------------------------------------------------------------------------ LayerNorm backward
def _ln_shapes():
    out = []
    for H, R in LNB_R.items():
        for M in (1, R - 1, R + 1, 608):
            out += [(H, M, dt) for dt in DTYPES]
        out.append((H, LNB_CAP * R + 1, torch.bfloat16))
    return out


def _ln_block(M, R, nblk, pm_mod):
    """workgroup of every PHYSICAL row: logical row i -> block (i // R) % nblk (grid stride), physical row (i % Bs) mod + i / Bs when a position
    table makes the kernel walk position-major"""
    i = torch.arange(M, device=DEV)
    blk = (i // R) % nblk
    if pm_mod and M % pm_mod == 0:
        Bs = M // pm_mod
        phys = (i % Bs) * pm_mod + i // Bs
        out = torch.empty_like(blk)
        out[phys] = blk
        return out
    return blk


@pytest.mark.parametrize("H,M,dtype", _ln_shapes())
def test_ln_bwd_partial_and_atomic_forms_match_float64(H, M, dtype, poison):
    rn = gen(H * 7 + M)
    R, L_, V = LNB_R[H], 19, 50
    y, dy = rn(M, H).to(dtype), rn(M, H).to(dtype)
    gamma, beta, rstd = (1 + 0.2 * rn(H)).float().to(DEV), (0.2 * rn(H)).float().to(DEV), (rn(M).abs() + 0.5).float().to(DEV)
    y, dy = y.to(DEV), dy.to(DEV)
    ids = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(M)).to(DEV, torch.int32)
    ids[::3] = 0                                                         # a hot padding row (hot0 = 0)
    navi = torch.randint(0, 3, (M,), generator=torch.Generator().manual_seed(M + 1)).to(DEV, torch.int32)
    dx64, env, xh = ln_bwd64(dy, y, gamma, beta, rstd)
    i = torch.arange(M, device=DEV)
    for case in ("plain", "text", "image", "sum"):
        do_ln = case != "sum"
        if case == "text":
            tabs = [(ids, 0, 0, (V, H), 0), (None, L_, 2, (L_ + 2, H), 0), (None, 0, 0, (1, H), 0)]
            rows = [ids.long(), i % L_ + 2, torch.zeros_like(i)]
        elif case == "image":
            tabs = [(navi, 0, 0, (3, H), 1), (None, 0, 1, (2, H), 0), None]
            rows = [navi.long(), torch.ones_like(i)]
        elif case == "sum":
            tabs = [(ids, 0, 0, (V, H), 0), None, None]
            rows = [ids.long()]
        else:
            tabs, rows = [None, None, None], []
        hot0 = 0 if case in ("text", "sum") else -1
        pm_mod = L_ if case == "text" else 0
        gin = dx64 if do_ln else dy.double()
        genv = env if do_ln else dy.double().abs()

        def once(partial):
            dx = torch.empty(M, H, dtype=dtype, device=DEV)
            dg, db = torch.full((H,), 0.25, device=DEV), torch.full((H,), -0.5, device=DEV)
            dts = [None if t is None else torch.zeros(t[3], device=DEV) for t in tabs]
            dtabs = tuple(None if t is None else (t[0], t[1], t[2], d, t[4]) for t, d in zip(tabs, dts))
            run(partial, lambda: O.ln_bwd(M, H, dy, y=y, gamma=gamma, beta=beta, rstd=rstd, dx=dx, dgamma=dg if do_ln else None,
                                          dbeta=db if do_ln else None, dtabs=dtabs, do_ln=do_ln, hot0=hot0))
            return dx, dg, db, [d for d in dts if d is not None]
        forms = {}
        for partial in (False, True):
            forms[partial] = once(partial)
            n_guard = check_guards(poison)
            assert n_guard == (1 if (partial and do_ln) else 0), case
            dx, dg, db, dts = forms[partial]
            tag = f"{case} {'partial' if partial else 'atomic'} H={H} M={M} {dtype}"
            check_dx(dx, gin, genv, f"dx[{tag}]", dtype)
            blk = nblk = None
            if partial and do_ln:
                nblk = O._ln_blocks(M, H, any(t is not None for t in tabs))
                assert nblk == min((M + R - 1) // R, LNB_CAP), (nblk, R)
                blk = _ln_block(M, R, nblk, pm_mod)
            if do_ln:
                check_sum(dg, torch.full((H,), 0.25, device=DEV), dy.double() * xh, dy.double().abs() * xh.abs(), f"dgamma[{tag}]", blk, nblk)
                check_sum(db, torch.full((H,), -0.5, device=DEV), dy.double(), dy.double().abs(), f"dbeta[{tag}]", blk, nblk)
            for d, t, r in zip(dts, [t for t in tabs if t is not None], rows):
                n = t[3][0]
                check_sum(d, torch.zeros(n, H, device=DEV), scatter(r, gin, n)[None], scatter(r, genv, n)[None], f"dtable[{tag}]")
        if do_ln:                                          # the partial form twice: bitwise the same dx and gamma / beta gradients
            again = once(True)
            check_guards(poison)
            for a, b in zip(forms[True][:3], again[:3]):
                assert torch.equal(a, b), case


def _paired_ln_bwd(H, MA, MB, dtype, poison):
    R = LNB_R[H]
    probs = []
    for M in (MA, MB):
        rn = gen(H + 3 * M)
        probs.append(dict(M=M, y=rn(M, H).to(dtype).to(DEV), dy=rn(M, H).to(dtype).to(DEV), rstd=(rn(M).abs() + 0.5).float().to(DEV)))
    rn = gen(H)
    gamma, beta = (1 + 0.2 * rn(H)).float().to(DEV), (0.2 * rn(H)).float().to(DEV)

    def once(partial):
        outs = [(torch.empty(q["M"], H, dtype=dtype, device=DEV), torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)) for q in probs]

        def launch():
            with L.group():
                for q, (dx, dg, db) in zip(probs, outs):
                    O.ln_bwd(q["M"], H, q["dy"], y=q["y"], gamma=gamma, beta=beta, rstd=q["rstd"], dx=dx, dgamma=dg, dbeta=db)
        run(partial, launch)
        return outs
    a = once(True)
    assert check_guards(poison) == 2
    b = once(True)
    check_guards(poison)
    c = once(False)
    for q, (dx, dg, db), (dx2, dg2, db2), (dx3, dg3, db3) in zip(probs, a, b, c):
        M = q["M"]
        dx64, env, xh = ln_bwd64(q["dy"], q["y"], gamma, beta, q["rstd"])
        nblk = O._ln_blocks(M, H, False)
        blk = _ln_block(M, R, nblk, 0)
        z = torch.zeros(H, device=DEV)
        for got, tag in ((dx, "partial"), (dx3, "atomic")):
            check_dx(got, dx64, env, f"pair dx {tag} M={M}", dtype)
        check_sum(dg, z, q["dy"].double() * xh, q["dy"].double().abs() * xh.abs(), f"pair dgamma M={M}", blk, nblk)
        check_sum(db, z, q["dy"].double(), q["dy"].double().abs(), f"pair dbeta M={M}", blk, nblk)
        check_sum(dg3, z, q["dy"].double() * xh, q["dy"].double().abs() * xh.abs(), f"pair dgamma atomic M={M}")
        assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)


@pytest.mark.parametrize("H,MA,MB", [(128, 600, 97), (128, 1, 4097), (768, 608, 9), (768, 1, 4097)])
def test_paired_ln_bwd_under_a_group_sizes_both_problems_partial_rows(H, MA, MB, poison):
    """two LayerNorm backwards of one width recorded under L.group() go out as ONE paired launch: each problem's partial rows are sized by the
    single-launch count (magic_ln_bwd_blocks) and must be exactly what the pair writes"""
    _paired_ln_bwd(H, MA, MB, torch.bfloat16, poison)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("H", [128, 768])
def test_paired_ln_bwd_in_the_other_storage_types(H, dtype, poison):
    """the paired launch's fp16 and fp32 instantiations (H = 768: the lean pair), one row short of a workgroup's rows beside one row past them"""
    _paired_ln_bwd(H, LNB_R[H] - 1, LNB_R[H] + 1, dtype, poison)


# ------------------------------------------------------------------------------------------ the MLM transform's LayerNorm backward
@pytest.mark.parametrize("H", [128, 256, 384, 768])
@pytest.mark.parametrize("M,nslab,dtype", [(1, 1, torch.float32), (257, 1, torch.bfloat16), (257, 3, torch.float16), (257, 2, torch.float32), (None, 2, torch.bfloat16)])
def test_ln_bwd_tail_partial_and_atomic_forms_match_float64(H, M, nslab, dtype, poison):
    R = {128: 64, 256: 32, 384: 8, 768: 8}[H]
    M = M if M is not None else LNB_CAP * R + 1
    rn = gen(H + M + nslab)
    slabs = rn(nslab, M, H).float().to(DEV).contiguous()
    y, pre = rn(M, H).to(dtype).to(DEV), rn(M, H).to(dtype).to(DEV)
    gamma, beta, rstd = (1 + 0.2 * rn(H)).float().to(DEV), (0.2 * rn(H)).float().to(DEV), (rn(M).abs() + 0.5).float().to(DEV)
    dy64 = slabs.double().sum(0)
    dyenv = slabs.double().abs().sum(0)
    dx64, _, xh = ln_bwd64(dy64, y, gamma, beta, rstd)
    _, envd, _ = ln_bwd64(dyenv, y, gamma, beta, rstd)          # (the slabs are added in fp32: the envelope takes their magnitudes)
    z = pre.double()
    for act in (1, 2):
        dact = (0.5 * (1 + torch.erf(z / 2 ** 0.5)) + z * torch.exp(-0.5 * z * z) / (2 * torch.pi) ** 0.5) if act == 1 else (z > 0).double()
        part_expected = H <= 384                          # (H = 768 keeps the atomic form: its lean block count differs)
        res = {}
        for partial in (False, True):
            def once():
                dx = torch.empty(M, H, dtype=dtype, device=DEV)
                dg, db = torch.full((H,), 0.5, device=DEV), torch.zeros(H, device=DEV)
                run(partial, lambda: O.ln_bwd_tail(M, H, slabs, y, gamma, beta, rstd, pre, act, dx, dg, db, nslab=nslab))
                return dx, dg, db
            dx, dg, db = res[partial] = once()
            assert check_guards(poison) == (1 if partial and part_expected else 0)
            tag = f"tail act={act} {'partial' if partial else 'atomic'} H={H} M={M} S={nslab}"
            check_dx(dx, dx64 * dact, envd * (dact.abs() + 0.1), f"dx[{tag}]", dtype)
            blk = nblk = None
            if partial and part_expected:
                nblk = O._ln_blocks(M, H, False)
                assert nblk == min((M + R - 1) // R, LNB_CAP)
                blk = _ln_block(M, R, nblk, 0)
            check_sum(dg, torch.full((H,), 0.5, device=DEV), dy64 * xh, dyenv * xh.abs(), f"dgamma[{tag}]", blk, nblk)
            check_sum(db, torch.zeros(H, device=DEV), dy64, dyenv, f"dbeta[{tag}]", blk, nblk)
            if partial and part_expected:                 # (the atomic form: fp32 atomics in any order)
                again = once()
                check_guards(poison)
                assert all(torch.equal(a, b) for a, b in zip(res[True], again))


# ------------------------------------------------------------------------------------------ position-embedding backward (Kin -> H linear + LayerNorm)
def _skb_rows(H, Mmax):
    return 64 if (H == 128 and Mmax >= 4096) else 8 if (H >= 384 and Mmax <= 4096) else 32


def _skb_refs(q, gamma, beta):
    dz, env, xh = ln_bwd64(q["dy"], q["y"], gamma, beta, q["rstd"])
    x = q["x"].double()
    dyd = q["dy"].double()
    return dict(dW=((dz[:, :, None] * x[:, None, :]).reshape(q["M"], -1), (env[:, :, None] * x.abs()[:, None, :]).reshape(q["M"], -1)),
                db=(dz, env), dgamma=(dyd * xh, dyd.abs() * xh.abs()), dbeta=(dyd, dyd.abs()))


def _skb_problem(M, H, Kin, dtype, seed):
    rn = gen(seed)
    return dict(M=M, Kin=Kin, x=rn(M, Kin).float().to(DEV).contiguous(), dy=rn(M, H).to(dtype).to(DEV), y=rn(M, H).to(dtype).to(DEV),
                rstd=(rn(M).abs() + 0.5).float().to(DEV))


@pytest.mark.parametrize("H,M,Kin,dtype", [(128, 100, 7, torch.float32), (128, 100, 1, torch.float16), (128, 5000, 16, torch.bfloat16),
                                           (256, 33, 7, torch.bfloat16), (256, 5000, 7, torch.bfloat16), (384, 9, 16, torch.float16),
                                           (384, 5000, 7, torch.bfloat16), (768, 1, 7, torch.float32), (768, 600, 1, torch.bfloat16),
                                           (768, 5000, 16, torch.bfloat16)])
def test_smallk_ln_bwd_partial_and_atomic_forms_match_float64(H, M, Kin, dtype, poison):
    q = _skb_problem(M, H, Kin, dtype, H + M + Kin)
    rn = gen(H)
    gamma, beta = (1 + 0.2 * rn(H)).float().to(DEV), (0.2 * rn(H)).float().to(DEV)
    refs = _skb_refs(q, gamma, beta)
    R = _skb_rows(H, M)
    nblk = (M + R - 1) // R
    res = {}
    for partial in (False, True, True):
        outs = dict(dW=torch.full((H, Kin), 0.125, device=DEV), db=torch.zeros(H, device=DEV), dgamma=torch.zeros(H, device=DEV), dbeta=torch.zeros(H, device=DEV))
        run(partial, lambda: O.smallk_ln_bwd(M, H, Kin, q["x"], q["dy"], q["y"], gamma, beta, q["rstd"], outs["dW"], outs["db"], outs["dgamma"], outs["dbeta"]))
        assert check_guards(poison) == (1 if partial else 0)
        if partial and partial in res:
            assert all(torch.equal(outs[k], res[True][k]) for k in outs)
            continue
        res[partial] = outs
        if partial:
            assert int(L.load().magic_smallk_ln_bwd_blocks(M, H, M)) == nblk
        blk = (torch.arange(M, device=DEV) // R) if partial else None
        for k, (terms, env) in refs.items():
            init = outs[k].new_full(outs[k].shape, 0.125 if k == "dW" else 0.0).reshape(-1)
            check_sum(outs[k].reshape(-1), init, terms, env, f"smallk {k} {'partial' if partial else 'atomic'}", blk, nblk if partial else None)


@pytest.mark.parametrize("H,MA,MB,Kin", [(768, 5000, 600, 7), (128, 4096, 100, 16), (384, 3000, 1, 1)])
def test_smallk_ln_bwd_pair_takes_the_larger_problems_tile_shape(H, MA, MB, Kin, poison):
    """the pair launch picks ONE tile shape from its larger problem: the smaller one's partial rows follow that shape, not its own"""
    dtype = torch.bfloat16
    qs = [_skb_problem(M, H, Kin, dtype, H + M) for M in (MA, MB)]
    rn = gen(H + 1)
    gamma, beta = (1 + 0.2 * rn(H)).float().to(DEV), (0.2 * rn(H)).float().to(DEV)
    R = _skb_rows(H, max(MA, MB))
    res = []
    for partial in (True, True, False):
        outs = [dict(dW=torch.zeros(H, Kin, device=DEV), db=torch.zeros(H, device=DEV), dgamma=torch.zeros(H, device=DEV), dbeta=torch.zeros(H, device=DEV)) for _ in qs]
        probs = [dict(q, gamma=gamma, beta=beta, **o) for q, o in zip(qs, outs)]
        run(partial, lambda: O.smallk_ln_bwd_pair(H, probs))
        assert check_guards(poison) == (2 if partial else 0)
        res.append(outs)
    for j, q in enumerate(qs):
        M = q["M"]
        nblk = (M + R - 1) // R
        assert int(L.load().magic_smallk_ln_bwd_blocks(M, H, max(MA, MB))) == nblk
        blk = torch.arange(M, device=DEV) // R
        for k, (terms, env) in _skb_refs(q, gamma, beta).items():
            z = torch.zeros(terms.shape[1], device=DEV)
            check_sum(res[0][j][k].reshape(-1), z, terms, env, f"pair smallk {k} M={M}", blk, nblk)
            check_sum(res[2][j][k].reshape(-1), z, terms, env, f"pair smallk {k} M={M} atomic")
            assert torch.equal(res[0][j][k], res[1][j][k])


# ------------------------------------------------------------------------------------------ SAP head: LayerNorm + dot
@pytest.mark.parametrize("H", [128, 256, 384, 768])
@pytest.mark.parametrize("M,dtype", [(1, torch.float32), (15, torch.bfloat16), (17, torch.float16), (1000, torch.bfloat16), (1000, torch.float32)])
def test_lndot_bwd_partial_and_atomic_forms_match_float64(H, M, dtype, poison):
    rn = gen(H + M)
    Y = torch.relu(rn(M, H) + 0.3).to(dtype).to(DEV)
    gamma, beta, w2 = (1 + 0.2 * rn(H)).float().to(DEV), (0.2 * rn(H)).float().to(DEV), (0.3 * rn(H)).float().to(DEV)
    dl = rn(M).float().to(DEV)
    eps = 1e-12
    x = Y.double()
    mean = x.mean(1, keepdim=True)
    r = 1 / ((x - mean).pow(2).mean(1, keepdim=True) + eps).sqrt()
    xh = (x - mean) * r
    xenv = xh.abs() + (x.abs() + mean.abs()) * r                    # (x - mean is formed in fp32)
    d = dl.double()[:, None]
    g64, w64, b64 = gamma.double(), w2.double(), beta.double()
    gg = d * w64 * g64
    m1, m2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    dZ64 = torch.where(x > 0, r * (gg - m1 - xh * m2), torch.zeros_like(x))
    dZenv = r * (gg.abs() + gg.abs().mean(1, keepdim=True) + xenv * (gg.abs() * xenv).mean(1, keepdim=True))
    refs = dict(dgamma=(d * w64 * xh, (d * w64).abs() * xenv), dbeta=(d * w64, (d * w64).abs()),
                dw2=(d * (xh * g64 + b64), d.abs() * (xenv * g64.abs() + b64.abs())), db2=(d, d.abs()))
    nblk = (M + 15) // 16
    res = {}
    for partial in (False, True, True):
        outs = dict(dgamma=torch.zeros(H, device=DEV), dbeta=torch.zeros(H, device=DEV), dw2=torch.full((H,), 0.5, device=DEV), db2=torch.zeros(1, device=DEV))
        dZ = torch.empty(M, H, dtype=dtype, device=DEV)
        run(partial, lambda: O.lndot_bwd(Y, M, H, gamma, beta, eps, w2, dl, dZ, outs["dgamma"], outs["dbeta"], outs["dw2"], outs["db2"]))
        assert check_guards(poison) == (1 if partial else 0)
        if partial and partial in res:
            assert torch.equal(dZ, res[True][1]) and all(torch.equal(outs[k], res[True][0][k]) for k in outs)
            continue
        res[partial] = (outs, dZ)
        if partial:
            assert int(L.load().magic_lndot_bwd_blocks(M)) == nblk
        check_dx(dZ, dZ64, dZenv * (x > 0), f"lndot dZ M={M} H={H}", dtype)
        blk = torch.arange(M, device=DEV) // 16 if partial else None
        for k, (terms, env) in refs.items():
            init = torch.full_like(outs[k], 0.5 if k == "dw2" else 0.0)
            check_sum(outs[k], init, terms, env, f"lndot {k} {'partial' if partial else 'atomic'} M={M} H={H}", blk, nblk if partial else None)


# ------------------------------------------------------------------------------------------ panorama fusion
@pytest.mark.parametrize("H", [128, 384, 768])
@pytest.mark.parametrize("N,V,dtype", [(1, 36, torch.float32), (7, 64, torch.bfloat16), (7, 37, torch.float16), (2000, 36, torch.bfloat16)])
def test_pano_fuse_bwd_partial_and_atomic_forms_match_float64(H, N, V, dtype, poison):
    rn = gen(H + N + V)
    x = rn(N, V, H).to(dtype).to(DEV)
    lens = torch.randint(1, V + 1, (N,), generator=torch.Generator().manual_seed(N)).to(DEV, torch.int32)
    lens[0] = V
    mask = torch.arange(V, device=DEV)[None] < lens[:, None]
    probs = torch.softmax(rn(N, V).to(DEV).masked_fill(~mask, float("-inf")), -1).float().contiguous()
    wf, df = (0.2 * rn(H)).float().to(DEV), rn(N, H).to(dtype).to(DEV)
    p, xd, dfd = probs.double(), x.double(), df.double()
    dp = (xd * dfd[:, None]).sum(-1)
    dpenv = (xd * dfd[:, None]).abs().sum(-1)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    dsenv = p * (dpenv + (p * dpenv).sum(-1, keepdim=True))
    dx64 = p[..., None] * dfd[:, None] + ds[..., None] * wf.double()
    dxenv = p[..., None] * dfd.abs()[:, None] + dsenv[..., None] * wf.double().abs()
    terms_w = (ds[..., None] * xd).sum(1)
    env_w = (dsenv[..., None] * xd.abs()).sum(1)
    nblk = (N + 1) // 2
    res = {}
    for partial in (False, True, True):
        dx = torch.zeros(N, V, H, dtype=dtype, device=DEV)
        dwf, dbf = torch.full((H,), 0.25, device=DEV), torch.zeros(1, device=DEV)
        run(partial, lambda: O.pano_fuse_bwd(x, probs, wf, df, dx, dwf, dbf, N, V, H))
        assert check_guards(poison) == (1 if partial else 0)
        if partial and partial in res:
            assert torch.equal(dx, res[True][0]) and torch.equal(dwf, res[True][1]) and torch.equal(dbf, res[True][2])
            continue
        res[partial] = (dx, dwf, dbf)
        if partial:
            assert int(L.load().magic_pano_fuse_bwd_blocks(N)) == nblk
        check_dx(dx, dx64, dxenv, f"pano dx N={N} H={H}", dtype)
        blk = torch.arange(N, device=DEV) // 2 if partial else None
        check_sum(dwf, torch.full((H,), 0.25, device=DEV), terms_w, env_w, f"pano dwf {partial}", blk, nblk if partial else None)
        check_sum(dbf, torch.zeros(1, device=DEV), ds.sum(1, keepdim=True), dsenv.sum(1, keepdim=True), f"pano dbf {partial}")   # (sum of a softmax gradient: zero up to rounding)


# ------------------------------------------------------------------------------------------ row dot / row gate (atomic only)
@pytest.mark.parametrize("H", [128, 512, 768, 1024])
@pytest.mark.parametrize("M,dtype", [(1, torch.float32), (4, torch.bfloat16), (17, torch.float16), (17, torch.float32), (5000, torch.bfloat16)])
def test_rowgate_fwd_bwd_match_float64(H, M, dtype):
    rn = gen(H + M)
    x, e = rn(M, H).to(dtype).to(DEV), rn(M, H).to(dtype).to(DEV)
    wx, we = (rn(H) / H ** 0.5).float().to(DEV), (rn(H) / H ** 0.5).float().to(DEV)
    b0, b1 = torch.tensor([0.3], device=DEV), torch.tensor([-0.1], device=DEV)
    xd, ed, wxd, wed = x.double(), e.double(), wx.double(), we.double()
    # mode 0: the critic's value dot
    s = (xd * wxd).sum(1) + 0.3
    senv = (xd * wxd).abs().sum(1) + 0.3
    out_s = torch.empty(M, device=DEV)
    O.rowgate_fwd(0, x, M, H, wx, b0=b0, out_s=out_s)
    torch.cuda.synchronize()
    assert ((out_s.double() - s).abs() <= REL * senv).all()
    dy = rn(M).float().to(DEV)
    dx = torch.empty(M, H, dtype=dtype, device=DEV)
    dwx, db0 = torch.full((H,), 0.5, device=DEV), torch.zeros(1, device=DEV)
    O.rowgate_bwd(0, x, M, H, wx, dy=dy, dx=dx, dwx=dwx, db0=db0)
    torch.cuda.synchronize()
    dyd = dy.double()[:, None]
    check_dx(dx, dyd * wxd, (dyd * wxd).abs(), f"rowgate dx mode 0 M={M}", dtype)
    check_sum(dwx, torch.full((H,), 0.5, device=DEV), dyd * xd, (dyd * xd).abs(), "rowgate dwx mode 0")
    check_sum(db0, torch.zeros(1, device=DEV), dyd, dyd.abs(), "rowgate db0 mode 0")
    # mode 1: the causal door gate
    s = (xd * wxd).sum(1) + (ed * wed).sum(1) + 0.2
    senv = (xd * wxd).abs().sum(1) + (ed * wed).abs().sum(1) + 0.4
    out, gsave = torch.empty(M, H, dtype=dtype, device=DEV), torch.empty(M, device=DEV)
    O.rowgate_fwd(1, x, M, H, wx, e=e, we=we, b0=b0, b1=b1, out=out, gsave=gsave)
    torch.cuda.synchronize()
    g64 = torch.sigmoid(s)
    assert ((gsave.double() - g64).abs() <= g64 * (1 - g64) * REL * senv + 1e-7).all()
    check_dx(out, ed * g64[:, None], ed.abs() * (g64 * (1 - g64) * REL * senv + 1e-7)[:, None] / REL, f"rowgate out M={M}", dtype)
    dout = rn(M, H).to(dtype).to(DEV)
    dx, de = torch.empty(M, H, dtype=dtype, device=DEV), torch.empty(M, H, dtype=dtype, device=DEV)
    dwx, dwe, db0, db1 = torch.zeros(H, device=DEV), torch.full((H,), -0.25, device=DEV), torch.zeros(1, device=DEV), torch.full((1,), 1.0, device=DEV)
    O.rowgate_bwd(1, x, M, H, wx, e=e, we=we, gsave=gsave, dout=dout, dx=dx, de=de, dwx=dwx, dwe=dwe, db0=db0, db1=db1)
    torch.cuda.synchronize()
    gs = gsave.double()[:, None]
    dod = dout.double()
    ds = (dod * ed).sum(1, keepdim=True) * gs * (1 - gs)
    dsenv = (dod * ed).abs().sum(1, keepdim=True) * gs * (1 - gs)
    check_dx(dx, ds * wxd, dsenv * wxd.abs(), f"rowgate dx mode 1 M={M}", dtype)
    check_dx(de, dod * gs + ds * wed, (dod * gs).abs() + dsenv * wed.abs(), f"rowgate de mode 1 M={M}", dtype)
    check_sum(dwx, torch.zeros(H, device=DEV), ds * xd, dsenv * xd.abs(), "rowgate dwx mode 1")
    check_sum(dwe, torch.full((H,), -0.25, device=DEV), ds * ed, dsenv * ed.abs(), "rowgate dwe mode 1")
    check_sum(db0, torch.zeros(1, device=DEV), ds, dsenv, "rowgate db0 mode 1")
    check_sum(db1, torch.ones(1, device=DEV), ds, dsenv, "rowgate db1 mode 1")


# ------------------------------------------------------------------------------------------ the finishers
def test_colsum_finishers_add_every_queued_job_in_queue_order():
    """magic_colsum_add_v (flush_part_jobs) and magic_colsum_add (flush_rbw_parts) against float64 column sums: more than 96 jobs in one flush, the same
    destination queued several times (the chunking must keep every contribution), lengths that are not multiples of 64, strides past the length, 1 to
    4096 rows -- and bitwise the same from the same starting buffers.  Queue order: one destination per finisher takes three single-row jobs whose
    fp32 sum, 1 + 2^24 - 2^24 + 3, is 3 only when they are added in the order they were queued (any other order gives 4)"""
    rn = gen(11)
    dsts0 = [rn(n).float().to(DEV) for n in (128, 200, 1, 768, 65, 3000)]
    jobs = []                                # (dst index, nblk, len, stride)
    for j in range(130):
        d = j % len(dsts0)
        n = dsts0[d].numel()
        nblk = (1, 3, 7, 64)[j % 4] if j % 13 else 4096
        stride = n + (j % 3) * 5
        jobs.append((d, nblk, n, stride, rn(nblk, stride).float().to(DEV)))
    H = 128                                  # (magic_colsum_add: the row-block launches' width, a divisor of 1024)
    rbw = [(j % 4, (1, 3, 300)[j % 3], rn((1, 3, 300)[j % 3], H).float().to(DEV)) for j in range(110)]
    rdst0 = [rn(H).float().to(DEV) for _ in range(4)]
    ordered = (2.0 ** 24, -2.0 ** 24, 3.0)
    dsts0.append(torch.ones(70, device=DEV))
    rdst0.append(torch.ones(H, device=DEV))
    for pos, v in zip((5, 50, 100), ordered):
        jobs.insert(pos, (len(dsts0) - 1, 1, 70, 70, torch.full((1, 70), v, device=DEV)))
        rbw.insert(pos, (len(rdst0) - 1, 1, torch.full((1, H), v, device=DEV)))

    def once():
        dsts = [d.clone() for d in dsts0]
        rdst = [d.clone() for d in rdst0]
        for d, nblk, n, stride, pt in jobs:
            O.PART_JOBS.append((pt.view(-1), dsts[d], nblk, n, stride))
        for d, nblk, pt in rbw:
            O.RBW_JOBS.append((pt.view(-1), rdst[d], nblk))
        O.flush_rbw_parts()
        torch.cuda.synchronize()
        assert not O.PART_JOBS and not O.RBW_JOBS
        return dsts, rdst
    a, b = once(), once()
    for u, v in zip(a[0] + a[1], b[0] + b[1]):
        assert torch.equal(u, v)
    assert (a[0][-1] == 3.0).all() and (a[1][-1] == 3.0).all(), (a[0][-1][:4], a[1][-1][:4])
    for d, d0 in enumerate(dsts0):
        mine = [(pt[:, :n].double()) for dd, nblk, n, stride, pt in jobs if dd == d]
        terms = torch.cat(mine, 0)
        check_sum(a[0][d], d0, terms, terms.abs(), f"colsum_add_v destination {d}")
    for d, d0 in enumerate(rdst0):
        terms = torch.cat([pt.double() for dd, nblk, pt in rbw if dd == d], 0)
        check_sum(a[1][d], d0, terms, terms.abs(), f"colsum_add destination {d}")


# ------------------------------------------------------------------------------------------ embedding stage: argument check
def _pano_desc(H, M, Kin, dt, nblk):
    """a magic_pano_in_bwd descriptor over zero-filled operands with a zero-filled partial buffer of nblk + 2 rows (pad0_, the row count, is left to the
    caller); returns (descriptor, partial buffer, the tensors it points at)"""
    big = lambda dtype=torch.float32: torch.zeros(M * H * (Kin + 3), dtype=dtype, device=DEV)
    keep = []
    a = L.PanoInBwd()
    a.M, a.Kin = M, Kin
    for k in ("dy", "X0", "A1", "A2", "dP0"):
        keep.append(big(dt)); setattr(a, k, L.P(keep[-1]))
    for k in ("rstd3", "g3", "b3", "dg3", "db3", "d_nav", "d_tok", "rstd1", "g1", "b1", "dg1", "db1", "rstd2", "g2", "b2", "dg2", "db2", "loc", "dW", "dbl"):
        keep.append(big()); setattr(a, k, L.P(keep[-1]))
    keep.append(torch.zeros(M, dtype=torch.int32, device=DEV)); a.nav_idx = L.P(keep[-1])
    stride = (11 + Kin) * H
    part = torch.zeros(nblk + 2, stride, device=DEV)
    a.part, a.pad1_ = L.P(part), stride
    return a, part, keep


def test_embed_in_bwd_refuses_a_partial_buffer_of_the_wrong_row_count():
    """magic_embed_in_bwd takes a partial buffer of EXACTLY the launch's row count: one row more would be summed unwritten by the flush (refused before
    anything is launched)"""
    H, M, Kin, dt = 128, 40, 7, torch.bfloat16
    nblk = int(L.load().magic_embed_in_bwd_blocks(M, H, 0, 1))
    assert nblk > 0
    a, part, keep = _pano_desc(H, M, Kin, dt, nblk)
    z = (C.c_void_p * 1)(), (C.c_void_p * 1)(), (C.c_int * 1)()
    for rows in (nblk + 1, nblk - 1):
        a.pad0_ = rows
        with pytest.raises(L.MagicHipError, match="MAGIC_ERR_ARG"):
            L.call("magic_embed_in_bwd", L.dt(dt), H, C.addressof(a), None, 0, C.addressof(z[0]), C.addressof(z[1]), C.addressof(z[2]), L.stream())
    torch.cuda.synchronize()
    assert (part == 0).all()


def test_embed_in_bwd_text_half_row_count_follows_its_gamma_gradient():
    """the text half's grid cap depends on whether it has gamma / beta gradients (512 with, 4096 without): the host takes that count from the launch's rule"""
    lib = L.load()
    for H in (128, 256):
        R = LNB_R[H]
        M = 600 * R
        assert lib.magic_embed_in_bwd_text_blocks(M, H, 1, 1) == LNB_CAP == lib.magic_ln_bwd_blocks(M, H, 1)
        assert lib.magic_embed_in_bwd_text_blocks(M, H, 1, 0) == 600
        assert lib.magic_embed_in_bwd_text_blocks(97, H, 0, 1) == lib.magic_ln_bwd_blocks(97, H, 0) == (97 + R - 1) // R


# ------------------------------------------------------------------------------------------ every partial-row launch: the row count is an argument
# Each entry point below takes the row count its caller sized the partial buffers with and returns MAGIC_ERR_ARG, before anything is launched, unless
# that is its own grid (the library's *_blocks query).  Shapes: at least two workgroups (one less is not the atomic form's 0), the last one ragged.
BF = torch.bfloat16


def _z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def refuses(name, args, good, parts, outs):
    """args(*rows) -> the arguments of L.call(name, ...) with one row count per partial-row problem of the launch; good: the counts of the queries;
    parts[i]: the zero-filled partial buffers ([good[i] + 2, stride] each) of problem i; outs: every other zero-filled tensor the launch writes.
    One count too many or too few, on any one problem alone: MAGIC_ERR_ARG and nothing written.  The exact counts: the launch runs and writes
    exactly those rows (the buffers are NaN-filled for it)."""
    good = tuple(int(g) for g in good)
    for i, g in enumerate(good):
        assert g >= 2, (name, good)
        for wrong in (g + 1, g - 1):
            with pytest.raises(L.MagicHipError, match="MAGIC_ERR_ARG"):
                L.call(name, *args(*good[:i], wrong, *good[i + 1:]))
    torch.cuda.synchronize()
    flat = [p for ps in parts for p in ps]
    assert all((t == 0).all() for t in flat + list(outs)), f"{name}: a refused call wrote something"
    for p in flat:
        p.fill_(float("nan"))
    L.call(name, *args(*good))
    torch.cuda.synchronize()
    for g, ps in zip(good, parts):
        for p in ps:
            assert p.shape[0] == g + 2 and torch.isfinite(p[:g]).all() and torch.isnan(p[g:]).all(), f"{name}: the exact count {g} did not write exactly its rows"


def _ln_args(H, M, table):
    """magic_ln_bwd over benign operands (gamma = rstd = 1); returns (args(rows), query count, partial planes, outputs)"""
    dy, y, dx = torch.ones(M, H, dtype=BF, device=DEV), _z(M, H, dtype=BF), _z(M, H, dtype=BF)
    gamma, beta, rstd = torch.ones(H, device=DEV), _z(H), torch.ones(M, device=DEV)
    d0 = _z(1, H) if table else None
    n = int(L.load().magic_ln_bwd_blocks(M, H, 1 if table else 0))
    pg, pb = _z(n + 2, H), _z(n + 2, H)
    args = lambda rows: (L.dt(BF), M, H, L.P(dy), L.P(y), L.P(gamma), L.P(beta), L.P(rstd), L.P(dx), L.P(pg), L.P(pb),      # noqa: E731
                         None, 0, 0, L.P(d0), 0, None, 0, 0, None, 0, None, 0, 0, None, 0, 1, None, 0.0, 0, 0, None, -1, rows, L.stream())
    return args, n, [pg, pb], [dx] + ([d0] if table else [])


@pytest.mark.parametrize("H,M,table", [(128, 65, False), (768, 9, False), (768, 9, True)])
def test_ln_bwd_refuses_any_row_count_but_its_grid(H, M, table):
    """H = 768 on 9 rows: the lean shape (8 waves x 1 row) without a table gradient, the 4 x 2 shape with one -- two workgroups either way"""
    args, n, planes, outs = _ln_args(H, M, table)
    assert n == (M + LNB_R[H] - 1) // LNB_R[H] == 2
    refuses("magic_ln_bwd", args, [n], [planes], outs)


def test_ln_bwd_with_a_wrong_row_count_raises_while_a_group_records_and_the_group_ends_clean():
    (a, n, pa, oa), (b, _, pb, ob) = _ln_args(128, 65, False), _ln_args(128, 65, False)
    with pytest.raises(L.MagicHipError, match="MAGIC_ERR_ARG"):
        with L.group():
            L.call("magic_ln_bwd", *a(n + 1))
    torch.cuda.synchronize()
    assert all((t == 0).all() for t in pa + oa)
    for p in pa + pb:
        p.fill_(float("nan"))
    with L.group():                                  # (nothing of the refused call is left in the group: this pair is one launch of two problems)
        L.call("magic_ln_bwd", *a(n))
        L.call("magic_ln_bwd", *b(n))
    torch.cuda.synchronize()
    for p in pa + pb:
        assert torch.isfinite(p[:n]).all() and torch.isnan(p[n:]).all()
        assert (p[:n].sum(0) == (0 if p is pa[0] or p is pb[0] else 65)).all()      # (y = beta: x-hat = 0, so dgamma = 0; dy = 1: dbeta = the row count)


def test_ln_bwd_tail_refuses_any_row_count_but_its_grid_and_the_retired_flag_bit():
    H, M = 128, 65
    dy32, y, pre, dx = torch.ones(M, H, device=DEV), _z(M, H, dtype=BF), _z(M, H, dtype=BF), _z(M, H, dtype=BF)
    gamma, beta, rstd = torch.ones(H, device=DEV), _z(H), torch.ones(M, device=DEV)
    n = int(L.load().magic_ln_bwd_blocks(M, H, 0))
    pg, pb = _z(n + 2, H), _z(n + 2, H)
    args = lambda rows, act=1: (L.dt(BF), M, H, L.P(dy32), L.P(y), L.P(gamma), L.P(beta), L.P(rstd), L.P(pre), act, L.P(dx), L.P(pg), L.P(pb), rows, L.stream())      # noqa: E731
    for rows in (n, 0):                              # bit 6 of `act` used to say "partial": refused with and without a count
        with pytest.raises(L.MagicHipError, match="MAGIC_ERR_ARG"):
            L.call("magic_ln_bwd_tail", *args(rows, act=1 | 0x40))
    refuses("magic_ln_bwd_tail", args, [n], [[pg, pb]], [dx])


def _skb_prob(d, M, H, Kin, n):
    """fills the magic_skb_prob d (part_rows left to the caller); returns (partial buffer of n + 2 rows, the gradient vectors, everything to keep alive)"""
    t = dict(x=_z(M, Kin), dy=torch.ones(M, H, dtype=BF, device=DEV), y=_z(M, H, dtype=BF), gamma=torch.ones(H, device=DEV), beta=_z(H),
             rstd=torch.ones(M, device=DEV), dW=_z(H, Kin), db=_z(H), dgamma=_z(H), dbeta=_z(H), part=_z(n + 2, H * (Kin + 3)))
    d.M, d.Kin = M, Kin
    for k, v in t.items():
        setattr(d, k, L.P(v))
    return t["part"], [t[k] for k in ("dW", "db", "dgamma", "dbeta")], t


def test_smallk_ln_bwd_refuses_any_row_count_but_its_grid():
    H, M, Kin = 128, 33, 7
    n = int(L.load().magic_smallk_ln_bwd_blocks(M, H, M))
    d = (L.SkbProb * 1)()
    part, outs, t = _skb_prob(d[0], M, H, Kin, n)
    args = lambda rows: (L.dt(BF), M, H, Kin, *[L.P(t[k]) for k in ("x", "dy", "y", "gamma", "beta", "rstd", "dW", "db", "dgamma", "dbeta", "part")], rows, L.stream())      # noqa: E731
    refuses("magic_smallk_ln_bwd", args, [n], [[part]], outs)


def test_smallk_ln_bwd_pair_refuses_a_wrong_row_count_on_either_problem():
    H, Ms, Kin = 128, (33, 70), 7
    ns = [int(L.load().magic_smallk_ln_bwd_blocks(m, H, max(Ms))) for m in Ms]
    d = (L.SkbProb * 2)()
    probs = [_skb_prob(d[i], m, H, Kin, n) for i, (m, n) in enumerate(zip(Ms, ns))]

    def args(ra, rb):
        d[0].part_rows, d[1].part_rows = ra, rb
        return (L.dt(BF), H, C.addressof(d), L.stream())
    refuses("magic_smallk_ln_bwd_pair", args, ns, [[p[0]] for p in probs], probs[0][1] + probs[1][1])


def test_lndot_bwd_refuses_any_row_count_but_its_grid():
    H, M = 128, 17
    n = int(L.load().magic_lndot_bwd_blocks(M))
    Y, dZ = _z(M, H, dtype=BF), _z(M, H, dtype=BF)
    gamma, beta, w2, dlogit = torch.ones(H, device=DEV), _z(H), torch.ones(H, device=DEV), torch.ones(M, device=DEV)
    vecs = [_z(H), _z(H), _z(H), _z(1)]
    part = _z(n + 2, 3 * H + 1)
    args = lambda rows: (L.dt(BF), M, H, L.P(Y), L.P(gamma), L.P(beta), 1e-12, L.P(w2), L.P(dlogit), L.P(dZ), *[L.P(v) for v in vecs], L.P(part), rows, L.stream())      # noqa: E731
    refuses("magic_lndot_bwd", args, [n], [[part]], vecs + [dZ])


def _fuse_ops(N, V, H):
    """operands of the panorama-fusion backward with dwf a partial buffer; (pointer arguments x .. dbf, query count, partial buffer, outputs)"""
    n = int(L.load().magic_pano_fuse_bwd_blocks(N))
    t = [torch.ones(N * V, H, dtype=BF, device=DEV), _z(N, V), _z(H), _z(N, H, dtype=BF), _z(N * V, H, dtype=BF), _z(n + 2, H + 1)]
    return t, n, t[5], [t[3], t[4]]


def test_pano_fuse_bwd_refuses_any_row_count_but_its_grid():
    H, N, V = 128, 3, 36
    t, n, part, outs = _fuse_ops(N, V, H)
    args = lambda rows: (L.dt(BF), N, V, H, *[L.P(v) for v in t], None, rows, L.stream())      # noqa: E731
    refuses("magic_pano_fuse_bwd", args, [n], [[part]], outs[1:])


def test_node_in_bwd_refuses_a_wrong_row_count_of_its_fusion_job_and_of_a_position_embedding_job():
    H, N, V, M, Kin = 128, 3, 36, 33, 7
    notab, noadd = (0, None, None, None), (0, 0, None, None)
    t, n, part, outs = _fuse_ops(N, V, H)
    fuse = lambda rows: (L.dt(BF), H, N, V, *[L.P(v) for v in t], None, rows, None, 0, None, *notab, *noadd, L.stream())      # noqa: E731
    refuses("magic_node_in_bwd", fuse, [n], [[part]], outs)
    nk = int(L.load().magic_smallk_ln_bwd_blocks(M, H, M))
    d = (L.SkbProb * 1)()
    kpart, kouts, keep = _skb_prob(d[0], M, H, Kin, nk)

    def skb(rows):
        d[0].part_rows = rows
        return (L.dt(BF), H, 0, 0, None, None, None, None, None, None, None, 0, None, 1, C.addressof(d), *notab, *noadd, L.stream())
    refuses("magic_node_in_bwd", skb, [nk], [[kpart]], kouts)


def test_embed_in_bwd_refuses_a_wrong_row_count_of_its_text_half():
    H, M, Kin, MT = 128, 40, 7, 65
    lib = L.load()
    nbt = int(lib.magic_embed_in_bwd_text_blocks(MT, H, 0, 1))
    nblk = int(lib.magic_embed_in_bwd_blocks(M, H, nbt, 1))
    a, part, keep = _pano_desc(H, M, Kin, BF, nblk)
    a.pad0_ = nblk                                   # the panorama half exact
    dy, y, dx = torch.ones(MT, H, dtype=BF, device=DEV), _z(MT, H, dtype=BF), _z(MT, H, dtype=BF)
    gamma, beta, rstd = torch.ones(H, device=DEV), _z(H), torch.ones(MT, device=DEV)
    pg, pb = _z(nbt + 2, H), _z(nbt + 2, H)
    t = L.LnBwdIn()
    t.M, t.do_ln, t.hot0 = MT, 1, -1
    t.dy, t.y, t.gamma, t.beta, t.rstd, t.dx, t.dgamma, t.dbeta = (L.P(v) for v in (dy, y, gamma, beta, rstd, dx, pg, pb))
    z = (C.c_void_p * 1)(), (C.c_void_p * 1)(), (C.c_int * 1)()

    def args(rows):
        t.partial = rows
        return (L.dt(BF), H, C.addressof(a), C.addressof(t), 0, C.addressof(z[0]), C.addressof(z[1]), C.addressof(z[2]), L.stream())
    refuses("magic_embed_in_bwd", args, [nbt], [[pg, pb]], [dx, part] + keep)
    assert (part[nblk:] == 0).all()                  # (the exact call left the rows past the panorama half's count alone)


RBW_H, RBW_I = 128, 512


def _rbw_seg(S, M, n, mode=0, N=0):
    """fills magic_rowbwd_seg S with a full chain over zero-filled operands -- the given-(d_fo, d_fod) form, or behind the attention stage (mode 1, samples
    of N rows) -- whose LayerNorm gradients point at partial buffers of n + 2 rows; returns (partial buffers, outputs, everything to keep alive)"""
    H, I = RBW_H, RBW_I
    h = lambda *s: _z(*s, dtype=BF)                  # noqa: E731
    t = dict(y2=h(M, H), rstd2=_z(M), g2=_z(H), b2=_z(H), z=h(M, I), W2T=h(H * I), W1T=h(H * I), y1=h(M, H), rstd1=_z(M), g1=_z(H), b1=_z(H), WoT=h(H * H),
             dz=h(M, I), daod=h(M, H), dao=h(M, H), dctx=h(M, H))
    # (the given form starts behind the output LayerNorm: it has the attention-output norm's two gradients only)
    parts = {k: _z(n + 2, H) for k in (("dg2", "db2") if mode else ()) + ("dg1", "db1")}
    outs = ["dz", "daod", "dao", "dctx"]
    S.M, S.kt, S.mode = M, 12, mode
    if mode:
        ldp = (N + 7) // 8 * 8
        S.N, S.ntile, S.ldp = N, (N + 15) // 16, ldp
        t.update(qkv_a=h(M, 3 * H), P_a=h(M // N, 2, N, ldp), o_a=h(M, H), dctx_a=h(M, H), dqkv_out=h(M, 3 * H), WqkvT_n=h(3 * H * H), dao_n=h(M, H), dfo=h(M, H), dfod=h(M, H))
        outs += ["dqkv_out", "dfo", "dfod"]
    else:
        t.update(dfo_in=h(M, H), dfod_in=h(M, H))
    for k, v in {**t, **parts}.items():
        setattr(S, k, L.P(v))
    return list(parts.values()), [t[k] for k in outs], t


def test_rowbwd_refuses_any_row_count_but_each_segments_grid():
    lib = L.load()
    assert O.rowbwd_ok(BF, RBW_H, RBW_I)

    def launch(shapes):
        """shapes: (M, mode, N) per segment; the refusals and the exact call of one launch over them"""
        total, att = sum(s[0] for s in shapes), int(any(s[1] for s in shapes))
        good = [int(lib.magic_rowbwd_seg_blocks(total, att, M, N, mode)) for M, mode, N in shapes]
        P = L.RbwParams()
        P.nseg, P.pad1, P.scale = len(shapes), 1, 0.125
        segs = [_rbw_seg(P.seg[i], M, good[i], mode, N) for i, (M, mode, N) in enumerate(shapes)]

        def args(*rows):
            pr = (C.c_int * len(rows))(*rows)
            args.keep = pr
            return (L.dt(BF), C.addressof(P), C.sizeof(P), C.addressof(pr), L.stream())
        with pytest.raises(L.MagicHipError, match="MAGIC_ERR_ARG"):      # partial buffers (pad1) without their row counts
            L.call("magic_rowbwd", L.dt(BF), C.addressof(P), C.sizeof(P), None, L.stream())
        refuses("magic_rowbwd", args, good, [s[0] for s in segs], [o for s in segs for o in s[1]])
        return good, P, args
    good, P, args = launch([(33, 0, 0)])
    assert good == [3]
    P.pad1 = 0                                       # ... and row counts without partial buffers
    with pytest.raises(L.MagicHipError, match="MAGIC_ERR_ARG"):
        L.call("magic_rowbwd", *args(*good))
    launch([(33, 0, 0), (50, 0, 0)])
    # samples of 20 rows are tiled one by one: 2 samples x 2 tiles, where the flat rule over 40 rows gives 3 -- which `refuses` tries as one too few
    good, _, _ = launch([(40, 1, 20)])
    assert good == [4] and (40 + 15) // 16 == 3


def test_rowbwd_seg_blocks_is_the_rule_the_host_used_to_spell_out():
    """flat: ceil(M / rows), rows = 16 up to 16 rows per CU over the whole launch, else 32 (MAGIC_RBW_ROWS unset); a segment with the attention stage:
    samples x 16-row tiles per sample, whether or not it has LayerNorm gradients (mode 2 has none: its launch takes 0 partial rows)"""
    lib = L.load()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    rows_of = lambda total: 16 if total <= 16 * ncu else 32      # noqa: E731
    assert lib.magic_rowbwd_seg_blocks(33, 0, 33, 0, 0) == (33 + 15) // 16 == 3
    M = 16 * ncu + 1                                 # (4097 on a 256-CU card: the launch flips to 32-row tiles)
    assert lib.magic_rowbwd_rows(M) == rows_of(M) == 32 and lib.magic_rowbwd_rows(M - 1) == 16
    assert lib.magic_rowbwd_seg_blocks(M, 0, M, 0, 0) == (M + 31) // 32
    assert lib.magic_rowbwd_seg_blocks(M + 33, 0, 33, 0, 0) == 2          # a small segment beside a large one shares its 32-row tiles
    assert lib.magic_rowbwd_seg_blocks(40, 1, 40, 20, 1) == (40 // 20) * ((20 + 15) // 16) == 4
    assert lib.magic_rowbwd_seg_blocks(96, 1, 96, 96, 2) == (96 // 96) * ((96 + 15) // 16) == 6
    assert lib.magic_rowbwd_seg_blocks(40 + 33, 1, 33, 0, 0) == 3         # a flat segment beside an attention-stage one: 16-row tiles
    for bad in ((33, 0, 0, 0, 0), (40, 0, 40, 20, 1), (40, 1, 40, 0, 1), (40, 1, 40, 16, 1), (40, 1, 40, 20, 3), (20, 0, 33, 0, 0)):
        assert lib.magic_rowbwd_seg_blocks(*bad) == -1, bad


# ------------------------------------------------------------------------------------------ embedding stage, both halves
def _eib_case(H, M, Kin, text, MT, dtype, seed):
    """operands of magic_embed_in_bwd: the panorama half (sum / image / location LayerNorm backwards, nav-type / token-type rows, the location
    Linear) and optionally the text half (LayerNorm backward + word / position / token-type scatters); text: None | "dgamma" | "no_dgamma" """
    rn = gen(seed)
    t = lambda *s: rn(*s).to(dtype).to(DEV)
    f = lambda v: v.float().to(DEV)
    pano = dict(M=M, Kin=Kin, dy=t(M, H), X0=t(M, H), A1=t(M, H), A2=t(M, H), rstd3=f(rn(M).abs() + 0.5), rstd1=f(rn(M).abs() + 0.5),
                rstd2=f(rn(M).abs() + 0.5), loc=f(rn(M, Kin)).contiguous(),
                nav_idx=torch.randint(0, 3, (M,), generator=torch.Generator().manual_seed(seed)).to(DEV, torch.int32))
    for k in ("3", "1", "2"):
        pano["g" + k], pano["b" + k] = f(1 + 0.2 * rn(H)), f(0.2 * rn(H))
    tx = None
    if text is not None:
        V, L_ = 50, 19
        ids = torch.randint(0, V, (MT,), generator=torch.Generator().manual_seed(seed + 1)).to(DEV, torch.int32)
        ids[::4] = 0
        tx = dict(M=MT, dy=t(MT, H), y=t(MT, H), gamma=f(1 + 0.2 * rn(H)), beta=f(0.2 * rn(H)), rstd=f(rn(MT).abs() + 0.5), ids=ids, V=V, L=L_,
                  pgrad=text == "dgamma")
    return pano, tx


def _eib_launch(H, pano, tx, init):
    """one magic_embed_in_bwd launch into fresh destinations (parameter gradients start at `init`); returns them"""
    M, Kin = pano["M"], pano["Kin"]
    out = {k: torch.full((H,), init, device=DEV) for k in ("dg3", "db3", "d_tok", "dg1", "db1", "dg2", "db2", "dbl")}
    out["d_nav"] = torch.full((3, H), init, device=DEV)
    out["dW"] = torch.full((H, Kin), init, device=DEV)
    out["dP0"] = torch.empty(M, H, dtype=pano["dy"].dtype, device=DEV)
    text = None
    if tx is not None:
        MT = tx["M"]
        out["t_word"], out["t_pos"], out["t_typ"] = torch.zeros(tx["V"], H, device=DEV), torch.zeros(tx["L"] + 2, H, device=DEV), torch.zeros(1, H, device=DEV)
        if tx["pgrad"]:
            out["t_dg"], out["t_db"] = torch.full((H,), init, device=DEV), torch.full((H,), init, device=DEV)
        text = dict(M=MT, dy=tx["dy"], y=tx["y"], gamma=tx["gamma"], beta=tx["beta"], rstd=tx["rstd"], hot0=0,
                    dgamma=out.get("t_dg"), dbeta=out.get("t_db"),
                    dtabs=((tx["ids"], 0, 0, out["t_word"], 0), (None, tx["L"], 2, out["t_pos"], 0), (None, 0, 0, out["t_typ"], 0)))
    O.embed_in_bwd(H, dict(pano, **{k: out[k] for k in ("dg3", "db3", "d_nav", "d_tok", "dg1", "db1", "dP0", "dg2", "db2", "dW", "dbl")}), text)
    return out


def _eib_refs(H, pano, tx, dtype):
    """float64 references: (terms [rows, n], envelopes) per parameter gradient, dP0 and its envelope.  The kernel rounds the sum LayerNorm's input
    gradient to the storage type before the image / location LayerNorm backwards (as the per-op path hands it on): `exact` = False when that rounding
    is not the identity -- the gradients downstream of it are then compared with the atomic form instead"""
    M, Kin = pano["M"], pano["Kin"]
    v, env3, xh3 = ln_bwd64(pano["dy"], pano["X0"], pano["g3"], pano["b3"], pano["rstd3"])
    d = pano["dy"].double()
    sid = pano["nav_idx"].long()
    nav = torch.zeros(M, 3, H, dtype=torch.float64, device=DEV)
    nav[torch.arange(M, device=DEV), sid] = v
    navenv = torch.zeros_like(nav)
    navenv[torch.arange(M, device=DEV), sid] = env3
    r = dict(dg3=(d * xh3, d.abs() * xh3.abs()), db3=(d, d.abs()), d_nav=(nav.reshape(M, -1), navenv.reshape(M, -1)), d_tok=(v, env3))
    ds = v.to(dtype).double()
    dP0, env1, xh1 = ln_bwd64(ds, pano["A1"], pano["g1"], pano["b1"], pano["rstd1"])
    _, envp, _ = ln_bwd64(env3, pano["A1"], pano["g1"], pano["b1"], pano["rstd1"])
    dz, _, xh2 = ln_bwd64(ds, pano["A2"], pano["g2"], pano["b2"], pano["rstd2"])
    _, envz, _ = ln_bwd64(env3, pano["A2"], pano["g2"], pano["b2"], pano["rstd2"])
    loc = pano["loc"].double()
    r.update(dg1=(ds * xh1, env3 * xh1.abs()), db1=(ds, env3), dg2=(ds * xh2, env3 * xh2.abs()), db2=(ds, env3), dbl=(dz, envz),
             dW=((dz[:, :, None] * loc[:, None, :]).reshape(M, -1), (envz[:, :, None] * loc.abs()[:, None, :]).reshape(M, -1)))
    tr = None
    if tx is not None:
        dxt, envt, xht = ln_bwd64(tx["dy"], tx["y"], tx["gamma"], tx["beta"], tx["rstd"])
        i = torch.arange(tx["M"], device=DEV)
        tr = dict(t_word=(tx["ids"].long(), tx["V"]), t_pos=(i % tx["L"] + 2, tx["L"] + 2), t_typ=(torch.zeros_like(i), 1), dx=dxt, env=envt,
                  t_dg=(tx["dy"].double() * xht, tx["dy"].double().abs() * xht.abs()), t_db=(tx["dy"].double(), tx["dy"].double().abs()))
    return r, (dP0, envp), tr


PIB_NW = {128: 16, 256: 8}
PIB_CAP = 128


def _eib_cases():
    out = []
    for H, nw in PIB_NW.items():
        R = 2 * nw
        for j, (M, Kin, text, MT) in enumerate([(1, 1, None, 0), (R - 1, 7, "dgamma", 97), (R + 1, 8, "no_dgamma", 608), (1000, 7, "dgamma", 608),
                                                (1000, 1, "no_dgamma", 600 * LNB_R[H]), (PIB_CAP * R + 1, 8, None, 0), (PIB_CAP * R + 1, 7, "dgamma", 4097)]):
            out.append((H, M, Kin, text, MT, torch.float32))
        out += [(H, 1000, 7, "dgamma", 608, torch.bfloat16), (H, PIB_CAP * R + 1, 8, "no_dgamma", 97, torch.float16)]
    return out


@pytest.mark.parametrize("H,M,Kin,text,MT,dtype", _eib_cases())
def test_embed_in_bwd_partial_and_atomic_forms_match_float64(H, M, Kin, text, MT, dtype, poison):
    """magic_embed_in_bwd, both halves, in both forms against float64: pano M = 1, 2 nw -+ 1, 1000 and past the 128-workgroup partial cap; Kin 1, 7
    and PIB_KMAX; without a text half, with one that has gamma / beta gradients (partial rows of its own) and with one that has none -- whose grid
    cap differs (4096 workgroups, not 512), and the panorama half's row count with it.  Partial-row jobs of the row-block launches ride along in the
    same launch and must equal what the standalone finisher gives."""
    pano, tx = _eib_case(H, M, Kin, text, MT, dtype, H + M + Kin + MT)
    refs, (dP0_64, envp), tr = _eib_refs(H, pano, tx, dtype)
    exact = dtype == torch.float32
    R = 2 * PIB_NW[H]
    rn = gen(M + 5)
    rbw = [(rn(nb * H).float().to(DEV), rn(H).float().to(DEV), nb) for nb in (1, 3, 70)]
    res = {}
    for form in ("atomic", "partial", "partial2"):
        partial = form != "atomic"
        rd = [d.clone() for _, d, _ in rbw]

        def launch():
            if partial:
                for (pt, _, nb), dd in zip(rbw, rd):
                    O.RBW_JOBS.append((pt, dd, nb))
            return _eib_launch(H, pano, tx, 0.25)
        box = {}
        run(partial, lambda: box.update(out=launch()))
        out = box["out"]
        if partial:
            assert not O.RBW_JOBS                          # (taken by the launch)
        n_guard = check_guards(poison)
        assert n_guard == (0 if not partial else 1 + (1 if (tx is not None and tx["pgrad"]) else 0)), n_guard
        if form == "partial2":
            assert all(torch.equal(out[k], res["partial"][0][k]) for k in out if not k.startswith("t_") or k in ("t_dg", "t_db")), "partial form not reproducible"
            assert all(torch.equal(a, b) for a, b in zip(rd, res["partial"][1]))
            continue
        res[form] = (out, rd)
        nbt = int(L.load().magic_embed_in_bwd_text_blocks(MT, H, 1, 1 if tx["pgrad"] else 0)) if tx is not None else 0
        na = int(L.load().magic_embed_in_bwd_blocks(M, H, nbt, 1))
        assert na == min((M + R - 1) // R, PIB_CAP, max(256 - nbt, 64)), (na, nbt)
        blk = ((torch.arange(M, device=DEV) // R) % na) if partial else None
        init = lambda t: torch.full_like(t, 0.25).reshape(-1)
        for k, (terms, env) in refs.items():
            if exact or k in ("dg3", "db3", "d_nav", "d_tok"):
                check_sum(out[k].reshape(-1), init(out[k]), terms, env, f"embed {k} {form}", blk, na if partial else None)
        if exact:
            check_dx(out["dP0"], dP0_64, envp, f"embed dP0 {form}", dtype)
        if tx is not None:
            MT_ = tx["M"]
            RT = LNB_R[H]
            i = torch.arange(MT_, device=DEV)
            Bs = MT_ // tx["L"] if MT_ % tx["L"] == 0 else 0
            for k in ("t_word", "t_pos", "t_typ"):
                rows, n = tr[k]
                check_sum(out[k], torch.zeros(n, H, device=DEV), scatter(rows, tr["dx"], n)[None], scatter(rows, tr["env"], n)[None], f"embed text {k} {form}")
            if tx["pgrad"]:
                tblk = _ln_block(MT_, RT, nbt, tx["L"]) if partial else None
                assert nbt == min((MT_ + RT - 1) // RT, LNB_CAP)
                for k in ("t_dg", "t_db"):
                    check_sum(out[k], torch.full((H,), 0.25, device=DEV), tr[k][0], tr[k][1], f"embed text {k} {form}", tblk, nbt if partial else None)
            else:
                assert nbt == min((MT_ + RT - 1) // RT, 4096)
        if partial:
            for (pt, d0, nb), got in zip(rbw, rd):
                terms = pt.view(nb, H).double()
                check_sum(got, d0, terms, terms.abs(), f"riding column sum nblk={nb}")
            # the same jobs through the standalone finisher (magic_colsum_add): the same sums (bitwise where its workgroup has the same shape)
            alone = [d.clone() for _, d, _ in rbw]
            for (pt, _, nb), dd in zip(rbw, alone):
                O.RBW_JOBS.append((pt, dd, nb))
            O.flush_rbw_parts()
            torch.cuda.synchronize()
            for a, b in zip(alone, rd):
                assert torch.equal(a, b) if PIB_NW[H] * 64 == 1024 else within(a, b.double(), 1e-5 * b.double().abs().max())
    if not exact:                                          # downstream of the storage-type rounding: the partial form against the atomic form
        a, p = res["atomic"][0], res["partial"][0]
        for k in ("dg1", "db1", "dg2", "db2", "dbl", "dW"):
            terms, env = refs[k]
            bound = REL * (0.25 + env.sum(0)) * 2
            assert ((a[k].reshape(-1).double() - p[k].reshape(-1).double()).abs() <= bound).all(), k
        assert torch.equal(a["dP0"], p["dP0"])


# ------------------------------------------------------------------------------------------ graph-distance attention bias
def _attn_case(B, nh, N, dtype, seed):
    H = nh * 64
    rn = gen(seed)
    qkv = rn(B * N, 3 * H).to(dtype).to(DEV)
    dist = (rn(B, N, N).abs() * 3).float().to(DEV).contiguous()
    kmask = torch.ones(B, N, dtype=torch.uint8, device=DEV)
    kmask[0, N - 2:] = 0
    sw, sb = torch.tensor([0.2], device=DEV), torch.tensor([-0.1], device=DEV)
    ldp = (N + 7) // 8 * 8
    Pm = torch.zeros(B, nh, N, ldp, dtype=dtype, device=DEV)
    ctx = torch.empty(B * N, H, dtype=dtype, device=DEV)
    O.attn_fwd(qkv, 3 * H, qkv[:, H:], qkv[:, 2 * H:], 3 * H, Pm, ldp, ctx, B, nh, N, N, H, 0.125, kmask=kmask, dist=dist, sprel_w=sw, sprel_b=sb)
    dctx = rn(B * N, H).to(dtype).to(DEV)
    # float64 dS of the logits from what the backward reads (the stored P, V, dO): dS = P (dP - rowsum(P dP)), dP = dO V^T
    P = Pm[..., :N].double()
    v = qkv[:, 2 * H:].double().reshape(B, N, nh, 64).transpose(1, 2)
    do = dctx.double().reshape(B, N, nh, 64).transpose(1, 2)
    dP = do @ v.transpose(-1, -2)
    dPe = do.abs() @ v.abs().transpose(-1, -2)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    dSe = P * (dPe + (P * dPe).sum(-1, keepdim=True))
    dd = dist.double()[:, None]
    per_wg_w, per_wg_we = (dS * dd).sum((-1, -2)).reshape(-1), (dSe * dd).sum((-1, -2)).reshape(-1)      # one (sample, head) workgroup each
    per_wg_b, per_wg_be = dS.sum((-1, -2)).reshape(-1), dSe.sum((-1, -2)).reshape(-1)
    return dict(B=B, nh=nh, N=N, H=H, qkv=qkv, Pm=Pm, ldp=ldp, dctx=dctx, dist=dist, w=(per_wg_w, per_wg_we), b=(per_wg_b, per_wg_be))


def _attn_bwd(c, dsw, dsb):
    B, nh, N, H = c["B"], c["nh"], c["N"], c["H"]
    qkv = c["qkv"]
    dqkv = torch.zeros_like(qkv)
    dP0 = torch.zeros(B, nh, N, c["ldp"], device=DEV)
    O.attn_bwd(qkv, 3 * H, qkv[:, H:], qkv[:, 2 * H:], 3 * H, c["Pm"], c["ldp"], c["dctx"], B, nh, N, N, H, 0.125, dP0, dqkv, 3 * H, dqkv[:, H:],
               dqkv[:, 2 * H:], 3 * H, dist=c["dist"], dsprel_w=dsw, dsprel_b=dsb)


@pytest.mark.parametrize("dtype", DTYPES)
def test_attn_bwd_distance_bias_gradients_match_float64_in_both_forms(dtype, poison):
    """one (sample, head) workgroup per partial pair: the two bias-gradient scalars against float64, and the tolerance can see one workgroup"""
    if not O.attn_supported(dtype, 18, 18, True):
        pytest.skip("no fused backward at this shape")
    c = _attn_case(3, 2, 18, dtype, 5)
    res = {}
    for form in ("atomic", "partial", "partial2"):
        dsw, dsb = torch.full((1,), 0.5, device=DEV), torch.zeros(1, device=DEV)
        run(form != "atomic", lambda: _attn_bwd(c, dsw, dsb))
        assert check_guards(poison) == (0 if form == "atomic" else 1)
        if form == "partial2":
            assert torch.equal(dsw, res["partial"][0]) and torch.equal(dsb, res["partial"][1])
            continue
        res[form] = (dsw, dsb)
        nwg = c["B"] * c["nh"]
        blk = torch.arange(nwg, device=DEV) if form == "partial" else None
        check_sum(dsw, torch.full((1,), 0.5, device=DEV), c["w"][0][:, None], c["w"][1][:, None], f"dsprel_w {form}", blk, nwg if blk is not None else None)
        check_sum(dsb, torch.zeros(1, device=DEV), c["b"][0][:, None], c["b"][1][:, None], f"dsprel_b {form}")     # (a softmax gradient's sum: zero up to rounding)


@pytest.mark.parametrize("grouped", [False, True])
def test_attn_bwd_distance_bias_partial_pairs_across_calls_and_reallocation(grouped, poison):
    """several attention backwards into the same bias-gradient pair in one flush window share ONE partial buffer of max(16 rows, 1024) pairs; a call
    past its capacity takes a new buffer (and two more column-sum jobs).  Every call's pairs land in rows of their own, the rows after the last used
    one stay untouched, and the two scalars equal float64 sums over every call -- eagerly and with pairs of calls recorded under L.group()"""
    dtype = torch.bfloat16
    cases = [_attn_case(B, 2, 18, dtype, 10 + j) for j, B in enumerate((2, 3, 600, 2, 5, 1))]     # 4 + 6 rows, then 1200 > 1024: a new buffer
    res = []
    for rep in range(2):
        dsw, dsb = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)

        def launch():
            if grouped:
                for a in range(0, len(cases), 2):
                    with L.group():
                        _attn_bwd(cases[a], dsw, dsb)
                        _attn_bwd(cases[a + 1], dsw, dsb)
            else:
                for cc in cases:
                    _attn_bwd(cc, dsw, dsb)
            assert len(O.PART_JOBS) == 4                  # two buffers, a pair of jobs each
            assert [g[1] for g in poison] == [4 + 6, 1200 + 4 + 10 + 2]
        run(True, launch)
        assert check_guards(poison) == 2
        res.append((dsw, dsb))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    z = torch.zeros(1, device=DEV)
    check_sum(res[0][0], z, torch.cat([cc["w"][0] for cc in cases])[:, None], torch.cat([cc["w"][1] for cc in cases])[:, None], "dsprel_w over calls")
    check_sum(res[0][1], z, torch.cat([cc["b"][0] for cc in cases])[:, None], torch.cat([cc["b"][1] for cc in cases])[:, None], "dsprel_b over calls")


# ------------------------------------------------------------------------------------------ one whole training step under poison
EXEMPT = ("bert.embeddings.word_embeddings.weight", "bert.embeddings.position_embeddings.weight", "bert.embeddings.token_type_embeddings.weight",
          "bert.global_encoder.gmap_step_embeddings.weight")


@pytest.mark.parametrize("task", ["sap", "mlm", "cfp"])
def test_a_student_step_with_poisoned_partial_rows_gives_the_same_gradients(task, monkeypatch):
    """every partial-row buffer of one default training step (LayerNorms, embedding stage, position embeddings, SAP head, panorama fusion, graph-distance
    bias, row-block launches) NaN-filled with guard rows: all gradients finite, every guard row intact, and the gradients equal the same step without
    poison -- bitwise, except the four embedding-table scatters whose fp32 atomics make them differ run to run"""
    from magic_amd.host import synth
    from tests.test_model_gpu import RW, build
    _, _, g_t, g_s = build(torch.bfloat16)
    batch = synth.make_batch(task, batch_size=7, seed=5, vocab=600, min_len=8, max_len=19, min_steps=2, max_steps=4)
    with torch.no_grad():
        gt = g_t(batch, task, compute_loss=False, return_outputs=True)

    def step():
        g_s.store.zero_grad()
        out = g_s(batch, task, compute_loss=True, teacher_outputs=gt, rw=RW, plan=gt["plan"])
        g_s.backward()
        torch.cuda.synchronize()
        return float(out["loss"]), g_s.store.grad.clone()
    l0, g0 = step()
    guards = []
    monkeypatch.setattr(O, "PART_POISON", True)
    monkeypatch.setattr(O, "PART_GUARDS", guards)
    l1, g1 = step()
    assert len(guards) >= 8, len(guards)
    check_guards(guards)
    assert abs(l1 - l0) <= 1e-6 * abs(l0)            # (the forward is the same; the loss kernels' own reductions may land in another order)
    assert torch.isfinite(g1).all()
    differ = []
    for name, (off, n, shape) in g_s.store.offsets.items():
        a, b = g0[off:off + n], g1[off:off + n]
        if name in EXEMPT:
            assert ((a - b).abs() <= 1e-5 * a.abs().max().clamp_min(1e-30)).all(), name
        elif not torch.equal(a, b):
            differ.append(name)
    assert not differ, differ
