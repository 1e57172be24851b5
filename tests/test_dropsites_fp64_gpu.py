"""The counter-based dropout sites of the row and GEMM kernels against float64 per element (-m gpu): the `drop` site of magic_linear_ln (single
and pair launch), site_in0 / site_out of magic_ln_fwd (with and without tables, pair launch), site_dy / site_dx of magic_ln_bwd (plain, text,
image and sum table forms, atomic and partial-row form, the position-major walk live and not), dout / X0d and the text half's sites of
magic_embed_in_fwd, ddy and the text half's sites of magic_embed_in_bwd.  bf16, fp16 and fp32; p in {0.1, 0.5}.

The mask is tests/_drop_ref64.mask64, asserted bit-identical to magic_dropout's export in every case; references, bounds and planted defects
are that module's (tests/test_drop_ref64_cpu.py proves that each defect bites).  In every case: dropped positions of a dropped output are
exactly zero, fp32 / p = 0.5 dropped copies are the clean copy times the keep factor bit for bit (one ulp apart only at a rounding boundary),
clean outputs do not depend on the presence of a site, NaN guard rows survive.

Measured on an MI355X (test_zz_report prints these with -s), and the three temporary kernel breaks: MEASURED below the imports.
Branches that could not be entered: none.
Kernel change this module brought: magic_ln_bwd (and the text half of magic_embed_in_bwd) dropped a supplied dxm whenever site_dx did not
drop, leaving the caller's buffer unwritten; they now store a bit-identical copy of dx there (csrc/rowops.hip).  First case it turns green:
test_ln_bwd_dxm_without_dropout_is_a_copy_of_dx[bf16-128].
"""
import os
import re

import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from tests import _drop_ref64 as D
from tests import _gemm_ref64 as G
from tests import _rowfwd_ref64 as RF
from tests.test_partial_rows_gpu import LNB_R, _eib_case, _eib_refs, _ln_block, check_guards, poison, run, scatter  # noqa: F401 (poison: a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
F32 = torch.float32
STATS = {}
_HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "magic_hip.h")).read()
BIT = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define MAGIC_GEMM_(FORM_\w+) (0x[0-9a-fA-F]+)", _HDR)}
MEASURED = """worst |err| / bound           bf16     fp16     fp32
  linear_ln drop out          0.4994   0.4994   0.0352
  linear_ln drop rstd         0.0316   0.0348   0.0473
  ln_fwd drop out             0.4994   0.4994   0.0428
  ln_fwd drop out_drop        0.4994   0.4994   0.0415
  ln_fwd drop rstd            0.3239   0.2996   0.2903
  ln_bwd drop dx              0.4961   0.4858   0.0088
  ln_bwd drop dxm             0.4961   0.4854   0.0104
  ln_bwd drop dgamma          0.0159   0.0157   0.0164
  ln_bwd drop dbeta           0.0107   0.0106   0.0119
  embed_in_fwd drop X0d       0.4988   0.4992   0.0348
  embed_in_fwd drop tout_drop 0.4985   0.4985   0.0383
  embed_in_bwd drop dg3       0.0172   0.0182   0.0156
  embed_in_bwd drop text dxm  0.4952   0.4822   0.0087
(16-bit outputs: the storage rounding, half of the ulp allowed; ln_bwd / embed_in_bwd rows are ratios to check_dx's / check_sum's bounds.)
Temporary kernel breaks, each in a library built aside and run against these modules on an MI355X, then discarded:
  row * H + col + 1 in linear_lnb_body's dxm index: tests/test_lnbwd_fp64_gpu.py fails at its first case (bf16 H 128 M 1 K 8, dxm at 1.7e40 bounds:
    a kept value where the reference has an exact zero);
  ln_bwd's mask indexed by the walk's logical row instead of phys(): test_ln_bwd_sites passes at M = 1, 5, 33, 257 (no position-major walk) and
    fails at M = 38 (text form, atomic, site_dy: dx at 1.4e5 bounds);
  linear_ln's mask in front of the bias: test_linear_ln_drop_site fails at its first case (bf16 H 128 M 1 K 8 p 0.1: 1970 bounds).
"""


def same(a, b):
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def nan_out(rows, cols, dtype):
    """[rows + 2, cols], NaN: rows past `rows` are guard rows"""
    return torch.full((rows + 2, cols), NAN, dtype=dtype, device=DEV)


def guard_ok(t, rows):
    return bool(torch.isnan(t[rows:].float()).all())


def masks(p, sites, M, H):
    """(seed tensor, seed words, [float64 mask per site]) -- each asserted equal to what magic_dropout exports"""
    seed = D.pick_seed(p, sites, M, H)
    seed_t = D.seed_tensor(seed, DEV)
    out = []
    for s in sites:
        m = D.mask64(seed_t, p, s, M, H)
        assert not D.mask_faults(m, p)
        ones, got = torch.ones(M * H, device=DEV), torch.empty(M * H, device=DEV)
        O.dropout(ones, got, 1, M * H, M * H, (seed_t, p, s))
        assert torch.equal(got.view(M, H).double(), m), f"mask64 differs from magic_dropout (p {p} site {s:#x} [{M}, {H}])"
        out.append(m)
    return seed_t, seed, out


def note(key, r):
    STATS[key] = max(STATS.get(key, 0.0), r)


def held(got, ref, store, key, tag):
    r = G.ratio(got, ref, store)
    STATS[key] = max(STATS.get(key, 0.0), r)
    assert r <= 1.0, f"{tag}: worst |err| / bound = {r:.3f}"


# ---- magic_linear_ln ------------------------------------------------------------------------------------------------------------------------------
def lln_call(dtype, M, H, K, ops, with_res, drop):
    x, W, bias, gamma, beta, res = ops
    out, rstd = nan_out(M, H, dtype), torch.full((M + 2,), NAN, device=DEV)
    L.call("magic_linear_ln", L.dt(dtype), M, H, K, L.P(x), x.stride(0), L.P(W), W.stride(0), L.P(bias), L.P(res) if with_res else None,
           H if with_res else 0, L.P(gamma), L.P(beta), G.LLN_EPS, L.P(out), L.P(rstd), *O._dr(drop), L.stream())
    return out, rstd


def lln_verify(dt, M, K, ops, out, rstd, with_res, seed, p, site, tag):
    dtype = D.DTYPES[dt]
    mask, (r_out, r_rstd), bad = D.lln_drop_refs(dtype, K, ops, with_res, seed, p, site)
    held(out[:M], r_out, dtype, ("linear_ln drop out", dt), tag)
    held(rstd[:M], r_rstd, F32, ("linear_ln drop rstd", dt), tag + " rstd")
    assert guard_ok(out, M) and torch.isnan(rstd[M:]).all(), f"{tag}: guard rows written"
    for name, ref in bad.items():
        assert not G.passes(out[:M], ref, dtype), f"{tag}: the check does not notice {name}"


@pytest.mark.parametrize("H", G.LLN_H)
@pytest.mark.parametrize("dt", D.DTYPES)
def test_linear_ln_drop_site(dt, H):
    dtype = D.DTYPES[dt]
    for K in G.LLN_K[G.bits(dtype)][:2]:
        for M in D.LLN_DROP_M:
            ops = G.lln_operands(dtype, M, H, K, 90, DEV)
            for p, site, with_res in ((0.1, 21, True), (0.5, D.LNB_BIG_SITE, False)):
                seed_t, seed, _ = masks(p, (site,), M, H)
                out, rstd = lln_call(dtype, M, H, K, ops, with_res, (seed_t, p, site))
                assert int(L.load().magic_gemm_last_form()) == BIT["FORM_LLN"]
                lln_verify(dt, M, K, ops, out, rstd, with_res, seed, p, site, f"{dt} linear_ln drop H {H} M {M} K {K} p {p}")


@pytest.mark.parametrize("H", G.LLN_H)
@pytest.mark.parametrize("dt", D.DTYPES)
def test_linear_ln_pair_with_one_dropping_side(dt, H):
    dtype = D.DTYPES[dt]
    K = G.LLN_K[G.bits(dtype)][1]
    p, site = 0.1, 21
    (Ma, sa, _), (Mb, sb, _) = G.LLN_PAIR
    seed_t, seed, _ = masks(p, (site,), Ma, H)
    oa, ob = G.lln_operands(dtype, Ma, H, K, sa, DEV), G.lln_operands(dtype, Mb, H, K, sb, DEV)
    single_a, single_b = lln_call(dtype, Ma, H, K, oa, True, (seed_t, p, site)), lln_call(dtype, Mb, H, K, ob, False, None)
    with L.group():
        pa, pb = lln_call(dtype, Ma, H, K, oa, True, (seed_t, p, site)), lln_call(dtype, Mb, H, K, ob, False, None)
    assert int(L.load().magic_gemm_last_form()) == BIT["FORM_LLN_PAIR"]
    lln_verify(dt, Ma, K, oa, *pa, True, seed, p, site, f"{dt} linear_ln pair H {H} dropping side")
    (r_out, r_rstd, _), bad = G.lln_refs(dtype, K, ob, 0, False, 0.0)
    held(pb[0][:Mb], r_out, dtype, ("linear_ln drop out", dt), f"{dt} linear_ln pair H {H} clean side")
    for name, ref in bad.items():
        assert not G.passes(pb[0][:Mb], ref, dtype), name
    for a, b in ((pa, single_a), (pb, single_b)):
        assert same(a[0], b[0]) and same(a[1], b[1]), f"{dt} H {H}: the pair launch differs from the single launches"


# ---- magic_ln_fwd ---------------------------------------------------------------------------------------------------------------------------------
def lnf_call(o, dtype, seed_t=None, p=0.0, s_in=0, s_out=0, want_drop=False):
    M, H = o.M, o.H
    out, rstd = nan_out(M, H, dtype), torch.full((M + 2,), NAN, device=DEV)
    od = nan_out(M, H, dtype) if want_drop else None
    tabs = []
    for t in o.tabs:
        tabs += list(O._tab(t))
    L.call("magic_ln_fwd", L.dt(dtype), M, H, L.P(o.in0), L.P(o.in1), *tabs, L.P(o.gamma), L.P(o.beta), RF.EPS, L.P(out), L.P(rstd), 1,
           L.P(seed_t), float(p), int(s_in), int(s_out), L.P(od), L.stream())
    return dict(out=out, rstd=rstd, out_drop=od)


def lnf_verify(o, dt, outs, mi, mo, seed, p, tag):
    dtype, M = D.DTYPES[dt], o.M
    ref = D.ln_fwd_drop_ref(o, dtype, mi, mo)
    who = ("ln_fwd drop", dt)
    RF.check(who, "out", outs["out"][:M], *ref["out"], tag, STATS)
    RF.check(who, "rstd", outs["rstd"][:M], *ref["rstd"], tag, STATS)
    assert guard_ok(outs["out"], M) and torch.isnan(outs["rstd"][M:]).all(), f"{tag}: guard rows written"
    if mo is not None:
        RF.check(who, "out_drop", outs["out_drop"][:M], *ref["out_drop"], tag, STATS)
        assert guard_ok(outs["out_drop"], M), f"{tag}: guard rows of out_drop written"
        assert not D.dropped_exact(outs["out"][:M], outs["out_drop"][:M], mo, p, dtype, *ref["out_drop"]), tag
    elif outs["out_drop"] is not None:
        assert torch.isnan(outs["out_drop"].float()).all(), f"{tag}: out_drop written without site_out"
    for name, bad in D.ln_fwd_drop_defects(o, dtype, mi, mo, seed, p, D.S_IN0, D.S_OUT).items():
        which = name.split(":")[0]
        got = outs[which][:M]
        assert D.fails(lambda: RF.check(("x", dt), which, got, *bad, tag)), f"{tag}: {name} not noticed"


LNF_CASES = D.ln_fwd_drop_cases()


@pytest.mark.parametrize("c", LNF_CASES, ids=[c.id for c in LNF_CASES])
def test_ln_fwd_sites(c):
    for dt, dtype in D.DTYPES.items():
        o = D.ln_operands_on(c, dtype, DEV)
        clean = lnf_call(o, dtype)
        for p in D.DROP_P:
            seed_t, seed, (m_in, m_out) = masks(p, (D.S_IN0, D.S_OUT), c.M, c.H)
            for mi, mo in D.site_combos(m_in, m_out):
                tag = f"{dt} {c.id} p {p} in0 {mi is not None} out {mo is not None}"
                outs = lnf_call(o, dtype, seed_t, p, D.S_IN0 if mi is not None else 0, D.S_OUT if mo is not None else 0, want_drop=True)
                lnf_verify(o, dt, outs, mi, mo, seed, p, tag)
                if mi is None:
                    assert same(outs["out"], clean["out"]) and same(outs["rstd"], clean["rstd"]), f"{tag}: the clean output depends on site_out"


@pytest.mark.parametrize("H", (128, 256, 768))
@pytest.mark.parametrize("dt", D.DTYPES)
def test_ln_fwd_pair_with_sites(dt, H):
    dtype, p = D.DTYPES[dt], 0.1
    ca, cb = RF.C("ln", f"H{H}-M33-image", [], H=H, M=33, form="image"), RF.C("ln", f"H{H}-M5-in0+in1", [], H=H, M=5, form="in0+in1")
    oa, ob = D.ln_operands_on(ca, dtype, DEV), D.ln_operands_on(cb, dtype, DEV)
    sa_t, sa, (ma_in, _) = masks(p, (D.S_IN0, D.S_OUT), 33, H)
    sb_t, sb, (mb_in, mb_out) = masks(p, (D.S_IN0, D.S_OUT), 5, H)
    single = [lnf_call(oa, dtype, sa_t, p, D.S_IN0, 0, True), lnf_call(ob, dtype, sb_t, p, D.S_IN0, D.S_OUT, True)]
    with L.group():
        pair = [lnf_call(oa, dtype, sa_t, p, D.S_IN0, 0, True), lnf_call(ob, dtype, sb_t, p, D.S_IN0, D.S_OUT, True)]
    lnf_verify(oa, dt, pair[0], ma_in, None, sa, p, f"{dt} ln_fwd pair H {H} side a")
    lnf_verify(ob, dt, pair[1], mb_in, mb_out, sb, p, f"{dt} ln_fwd pair H {H} side b")
    for a, b in zip(pair, single):
        assert all(same(a[k], b[k]) for k in a if a[k] is not None), f"{dt} H {H}: the pair launch differs from the single launches"


# ---- magic_ln_bwd ---------------------------------------------------------------------------------------------------------------------------------
L_, V = 19, 50
LNB_M = D.DROP_M + (2 * L_,)                      # 38 rows: the text form's position-major walk is live (M % 19 == 0); at the others it is not
LNB_COMBOS = (("dy", 0.1), ("dx", 0.5), ("both", 0.1), ("both", 0.5))


def lnb_tables(case, M, H):
    ids = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(M)).to(DEV, torch.int32)
    ids[::3] = 0
    navi = torch.randint(0, 3, (M,), generator=torch.Generator().manual_seed(M + 1)).to(DEV, torch.int32)
    i = torch.arange(M, device=DEV)
    if case == "text":
        return [(ids, 0, 0, (V, H), 0), (None, L_, 2, (L_ + 2, H), 0), (None, 0, 0, (1, H), 0)], [ids.long(), i % L_ + 2, torch.zeros_like(i)]
    if case == "image":
        return [(navi, 0, 0, (3, H), 1), (None, 0, 1, (2, H), 0), None], [navi.long(), torch.ones_like(i)]
    if case == "sum":
        return [(ids, 0, 0, (V, H), 0), None, None], [ids.long()]
    return [None, None, None], []


def lnb_shapes():
    out = [(H, M) for H in (128, 256) for M in LNB_M]
    return out + [(384, 5), (768, 33)]


@pytest.mark.parametrize("H,M", lnb_shapes())
@pytest.mark.parametrize("dt", D.DTYPES)
def test_ln_bwd_sites(dt, H, M, poison):  # noqa: F811
    dtype = D.DTYPES[dt]
    rn = torch.Generator().manual_seed(H * 7 + M)
    r = lambda *s: torch.randn(*s, generator=rn, dtype=torch.float64)       # noqa: E731
    y, dy = r(M, H).to(dtype).to(DEV), r(M, H).to(dtype).to(DEV)
    gamma, beta, rstd = (1 + 0.2 * r(H)).float().to(DEV), (0.2 * r(H)).float().to(DEV), (r(M).abs() + 0.5).float().to(DEV)
    R = LNB_R[H]
    ig, ib = torch.full((H,), 0.25, device=DEV), torch.full((H,), -0.5, device=DEV)
    for which, p in LNB_COMBOS:
        seed_t, seed, (m_dy, m_dx) = masks(p, (D.S_DY, D.S_DX), M, H)
        a, b = (m_dy if which != "dx" else None), (m_dx if which != "dy" else None)
        for case in ("plain", "text", "image", "sum"):
            do_ln = case != "sum"
            tabs, rows = lnb_tables(case, M, H)
            ref = D.ln_bwd_drop_ref(dy, y, gamma, beta, rstd, a, b, do_ln)
            walk = case == "text" and M % L_ == 0
            for partial in (False, True):
                tag = f"{dt} H {H} M {M} {case} {'partial' if partial else 'atomic'} {which} p {p}"
                dx, dxm = nan_out(M, H, dtype), nan_out(M, H, dtype)
                dg, db = ig.clone(), ib.clone()
                dts = [None if t is None else torch.zeros(t[3], device=DEV) for t in tabs]
                dtabs = tuple(None if t is None else (t[0], t[1], t[2], d, t[4]) for t, d in zip(tabs, dts))
                run(partial, lambda: O.ln_bwd(M, H, dy, y=y, gamma=gamma, beta=beta, rstd=rstd, dx=dx, dgamma=dg if do_ln else None,
                                              dbeta=db if do_ln else None, dtabs=dtabs, do_ln=do_ln, hot0=0 if case in ("text", "sum") else -1,
                                              drop_dy=(seed_t, p, D.S_DY) if a is not None else None,
                                              drop_dx=(seed_t, p, D.S_DX) if b is not None else None, dxm=dxm if b is not None else None))
                assert check_guards(poison) == (1 if (partial and do_ln) else 0), tag
                assert guard_ok(dx, M) and guard_ok(dxm, M), f"{tag}: guard rows written"
                D.check_dx(dx[:M], ref["dx"], ref["env"], f"dx[{tag}]", dtype)
                note(("ln_bwd drop", "dx", dt), D.dx_ratio(dx[:M], ref["dx"], ref["env"], dtype))
                if b is not None:
                    D.check_dx(dxm[:M], ref["dxm"], ref["dxm_env"], f"dxm[{tag}]", dtype)
                    note(("ln_bwd drop", "dxm", dt), D.dx_ratio(dxm[:M], ref["dxm"], ref["dxm_env"], dtype))
                    assert not D.dropped_exact(dx[:M], dxm[:M], b, p, dtype, ref["dxm"], D.REL * (ref["dxm"].abs() + ref["dxm_env"])), tag
                else:
                    assert torch.isnan(dxm.float()).all()
                if a is not None:
                    assert bool((dx[:M].float()[a == 0] == 0).all()) or do_ln, f"{tag}: a dropped dy element came through the plain sum"
                # controls: the mask of the next site, H + 1 columns, the logical row on the position-major walk
                bads = {}
                for k, (mk, site) in (("dy", (a, D.S_DY)), ("dx", (b, D.S_DX))):
                    if mk is None:
                        continue
                    bads[k + ":next site"] = D.mask64(seed_t, p, (site + 1) & D.M32, M, H)
                    if M > 1:
                        bads[k + ":columns off by one"] = D.mask64(seed_t, p, site, M, H + 1)[:, :H]
                    if walk:
                        bads[k + ":logical row on the position-major walk"] = D.permuted_rows_mask(mk, L_)
                for name, bm in bads.items():
                    o2 = D.ln_bwd_drop_ref(dy, y, gamma, beta, rstd, bm if name.startswith("dy") else a, bm if name.startswith("dx") else b, do_ln)
                    if name.startswith("dx"):
                        assert D.dx_ratio(dxm[:M], o2["dxm"], o2["dxm_env"], dtype) > 1.0, f"{tag}: {name} not noticed in dxm"
                    else:
                        assert D.dx_ratio(dx[:M], o2["dx"], o2["env"], dtype) > 1.0, f"{tag}: {name} not noticed in dx"
                blk = nblk = None
                if partial and do_ln:
                    nblk = O._ln_blocks(M, H, any(t is not None for t in tabs))
                    blk = _ln_block(M, R, nblk, L_ if case == "text" else 0)
                if do_ln:
                    D.check_sum(dg, ig, ref["dg_terms"], ref["dg_env"], f"dgamma[{tag}]", blk, nblk)
                    D.check_sum(db, ib, ref["db_terms"], ref["db_env"], f"dbeta[{tag}]", blk, nblk)
                    note(("ln_bwd drop", "dgamma", dt), D.sum_ratio(dg, ig, ref["dg_terms"], ref["dg_env"]))
                    note(("ln_bwd drop", "dbeta", dt), D.sum_ratio(db, ib, ref["db_terms"], ref["db_env"]))
                    if a is not None:                      # site_dy applied after the gamma / beta sums
                        late = D.ln_bwd_drop_ref(dy, y, gamma, beta, rstd, None, b)
                        assert D.sum_ratio(dg, ig, late["dg_terms"], late["dg_env"]) > 1.0, f"{tag}: dgamma summed before site_dy not noticed"
                        assert D.sum_ratio(db, ib, late["db_terms"], late["db_env"]) > 1.0, f"{tag}: dbeta summed before site_dy not noticed"
                for d, t, rr in zip([d for d in dts if d is not None], [t for t in tabs if t is not None], rows):
                    n = t[3][0]
                    D.check_sum(d, torch.zeros(n, H, device=DEV), scatter(rr, ref["dx"], n)[None], scatter(rr, ref["env"], n)[None], f"dtable[{tag}]")


@pytest.mark.parametrize("H", (128, 256, 384, 768))
@pytest.mark.parametrize("dt", D.DTYPES)
def test_ln_bwd_dxm_without_dropout_is_a_copy_of_dx(dt, H):
    dtype, M = D.DTYPES[dt], 33
    rn = torch.Generator().manual_seed(H)
    r = lambda *s: torch.randn(*s, generator=rn, dtype=torch.float64)       # noqa: E731
    y, dy = r(M, H).to(dtype).to(DEV), r(M, H).to(dtype).to(DEV)
    gamma, beta, rstd = (1 + 0.2 * r(H)).float().to(DEV), (0.2 * r(H)).float().to(DEV), (r(M).abs() + 0.5).float().to(DEV)
    seed_t, seed, (m_dy,) = masks(0.1, (D.S_DY,), M, H)
    for drop_dy in (None, (seed_t, 0.1, D.S_DY)):
        dx, dxm = nan_out(M, H, dtype), nan_out(M, H, dtype)
        O.ln_bwd(M, H, dy, y=y, gamma=gamma, beta=beta, rstd=rstd, dx=dx, drop_dy=drop_dy, dxm=dxm)
        ref = D.ln_bwd_drop_ref(dy, y, gamma, beta, rstd, m_dy if drop_dy else None, None)
        D.check_dx(dx[:M], ref["dx"], ref["env"], f"{dt} H {H} dx", dtype)
        assert same(dx, dxm), f"{dt} H {H}: dxm given without site_dx is not a copy of dx (site_dy {'on' if drop_dy else 'off'})"


# ---- magic_embed_in_fwd ---------------------------------------------------------------------------------------------------------------------------
EIF_CASES, S_X0D, S_TOUT = D.EIF_CASES, D.S_X0D, D.S_TOUT


def eif_call(c, dtype, o, keep, pano_drop=None, text_drop=None):
    dv = lambda t: None if t is None else t.to(DEV).contiguous()            # noqa: E731
    M, H = c.M, c.H
    outs = {n: nan_out(M, H, dtype) for n in ("A1", "A2", "X0", "X0d")}
    outs.update({n: torch.full((M + 2,), NAN, device=DEV) for n in ("rstd1", "rstd2", "rstd3")})
    pano = dict(M=M, Kin=c.Kin, eps=RF.EPS, P0=dv(o.P0), g1=dv(o.g1), b1=dv(o.b1), loc=dv(o.x), W=dv(o.W), b=dv(o.b), g2=dv(o.gamma), b2=dv(o.beta),
                nav_tab=dv(o.nav_tab), nav_idx=dv(o.nav_idx), tok_tab=dv(o.tok_tab), g3=dv(o.g3), b3=dv(o.b3), **outs)
    if pano_drop is not None:
        pano["drop"] = pano_drop
    text = None
    if o.text is not None:
        t = o.text
        outs.update(tout=nan_out(t.M, H, dtype), trstd=torch.full((t.M + 2,), NAN, device=DEV), tout_drop=nan_out(t.M, H, dtype))
        text = dict(M=t.M, out=outs["tout"], rstd=outs["trstd"], in0=None, in1=None, tabs=[(dv(x[0]), dv(x[1]), x[2], x[3]) for x in t.tabs],
                    gamma=dv(t.gamma), beta=dv(t.beta), eps=RF.EPS)
        if text_drop is not None:
            text.update(drop_out=text_drop, out_drop=outs["tout_drop"])
    keep.append((pano, text))
    O.embed_in_fwd(H, pano, text)
    return outs


@pytest.mark.parametrize("c", EIF_CASES, ids=[c.id for c in EIF_CASES])
def test_embed_in_fwd_dout_and_text_site(c):
    for dt, dtype in D.DTYPES.items():
        o = RF.operands(c, dt)
        keep = []
        clean = eif_call(c, dtype, o, keep)
        Mt = o.text.M if o.text is not None else 0
        for p in D.DROP_P:
            tag = f"{dt} {c.id} p {p}"
            seed_t, seed, (m_x,) = masks(p, (S_X0D,), c.M, c.H)
            m_t = None
            if Mt:
                seed = D.pick_seed(p, ((S_X0D, c.M), (S_TOUT, Mt)), c.M, c.H)            # one seed for both halves, as a training step has
                seed_t = D.seed_tensor(seed, DEV)
                m_x, m_t = D.mask64(seed_t, p, S_X0D, c.M, c.H), D.mask64(seed_t, p, S_TOUT, Mt, c.H)
                assert not D.mask_faults(m_x, p) and not D.mask_faults(m_t, p), tag
                for m, site in ((m_x, S_X0D), (m_t, S_TOUT)):
                    ones, got = torch.ones(m.numel(), device=DEV), torch.empty(m.numel(), device=DEV)
                    O.dropout(ones, got, 1, m.numel(), m.numel(), (seed_t, p, site))
                    assert torch.equal(got.view_as(m).double(), m), tag
            outs = eif_call(c, dtype, o, keep, (seed_t, p, S_X0D), (seed_t, p, S_TOUT) if Mt else None)
            torch.cuda.synchronize()
            for k in clean:                                     # the saved tensors: bit for bit the run without dropout, guard rows included
                if k not in ("X0d", "tout_drop"):
                    assert same(outs[k], clean[k]), f"{tag}: {k} depends on the dropout sites"
            assert torch.isnan(clean["X0d"].float()).all(), f"{tag}: X0d written without dropout"
            rows = {k: (Mt if k.startswith("t") else c.M) for k in outs}
            RF.verify(c, dt, o, {k: v[:rows[k]].cpu() for k, v in outs.items()}, tag, STATS)
            o3 = RF.SimpleNamespace(M=c.M, H=c.H, in0=outs["A1"][:c.M], in1=outs["A2"][:c.M], do_ln=True,
                                    tabs=[(o.nav_tab.to(DEV), o.nav_idx.to(DEV), 0, 0), (o.tok_tab.to(DEV), None, 0, 0), None], gamma=o.g3.to(DEV), beta=o.b3.to(DEV))
            checks = [("X0", "X0d", o3, m_x, S_X0D, c.M)]
            if Mt:
                ot = D.ln_operands_on(RF.C("ln", c.tag + "-text", [], H=c.H, M=Mt, form="text"), dtype, DEV)
                checks.append(("tout", "tout_drop", ot, m_t, S_TOUT, Mt))
            for cn, dn, oo, m, site, rws in checks:
                ref = D.ln_fwd_drop_ref(oo, dtype, None, m)["out_drop"]
                RF.check(("embed_in_fwd drop", dt), dn, outs[dn][:rws], *ref, tag, STATS)
                assert guard_ok(outs[dn], rws), f"{tag}: guard rows of {dn} written"
                assert not D.dropped_exact(outs[cn][:rws], outs[dn][:rws], m, p, dtype, *ref), f"{tag} {dn}"
                bad = D.ln_fwd_drop_ref(oo, dtype, None, D.mask64(seed_t, p, (site + 1) & D.M32, rws, c.H))["out_drop"]
                assert D.fails(lambda: RF.check(("x", dt), dn, outs[dn][:rws], *bad, tag)), f"{tag}: {dn} with the mask of the next site not noticed"
                if rws > 1:
                    bad = D.ln_fwd_drop_ref(oo, dtype, None, D.mask64(seed_t, p, site, rws, c.H + 1)[:, :c.H])["out_drop"]
                    assert D.fails(lambda: RF.check(("x", dt), dn, outs[dn][:rws], *bad, tag)), f"{tag}: {dn} with H + 1 mask columns not noticed"


# ---- magic_embed_in_bwd ---------------------------------------------------------------------------------------------------------------------------
S_DDY = D.S_DDY


def eib_launch(H, pano, tx, init, seed_t, p):
    """tests/test_partial_rows_gpu._eib_launch with the output-dropout site of the panorama half and both sites of the text half"""
    M, Kin = pano["M"], pano["Kin"]
    dt_ = pano["dy"].dtype
    out = {k: torch.full((H,), init, device=DEV) for k in ("dg3", "db3", "d_tok", "dg1", "db1", "dg2", "db2", "dbl")}
    out["d_nav"], out["dW"], out["dP0"] = torch.full((3, H), init, device=DEV), torch.full((H, Kin), init, device=DEV), nan_out(M, H, dt_)
    text = None
    if tx is not None:
        MT = tx["M"]
        out["t_word"], out["t_pos"], out["t_typ"] = torch.zeros(tx["V"], H, device=DEV), torch.zeros(tx["L"] + 2, H, device=DEV), torch.zeros(1, H, device=DEV)
        out["t_dg"], out["t_db"] = torch.full((H,), init, device=DEV), torch.full((H,), init, device=DEV)
        out["t_dx"], out["t_dxm"] = nan_out(MT, H, dt_), nan_out(MT, H, dt_)
        text = dict(M=MT, dy=tx["dy"], y=tx["y"], gamma=tx["gamma"], beta=tx["beta"], rstd=tx["rstd"], hot0=0, dgamma=out["t_dg"], dbeta=out["t_db"],
                    dx=out["t_dx"], dxm=out["t_dxm"], drop_dy=(seed_t, p, D.S_DY), drop_dx=(seed_t, p, D.S_DX),
                    dtabs=((tx["ids"], 0, 0, out["t_word"], 0), (None, tx["L"], 2, out["t_pos"], 0), (None, 0, 0, out["t_typ"], 0)))
    O.embed_in_bwd(H, dict(pano, drop_dy=(seed_t, p, S_DDY), **{k: out[k] for k in ("dg3", "db3", "d_nav", "d_tok", "dg1", "db1", "dP0", "dg2", "db2", "dW", "dbl")}), text)
    return out


@pytest.mark.parametrize("H,M,MT", D.EIB_SHAPES)
@pytest.mark.parametrize("dt", D.DTYPES)
def test_embed_in_bwd_ddy_and_text_sites(dt, H, M, MT, poison):  # noqa: F811
    dtype, Kin = D.DTYPES[dt], 7
    pano, tx = _eib_case(H, M, Kin, "dgamma", MT, dtype, H + M + MT)
    for p in D.DROP_P:
        seed = D.pick_seed(p, ((S_DDY, M), (D.S_DY, MT), (D.S_DX, MT)), M, H)
        seed_t = D.seed_tensor(seed, DEV)
        m_p, m_dy, m_dx = D.mask64(seed_t, p, S_DDY, M, H), D.mask64(seed_t, p, D.S_DY, MT, H), D.mask64(seed_t, p, D.S_DX, MT, H)
        for m, site in ((m_p, S_DDY), (m_dy, D.S_DY), (m_dx, D.S_DX)):
            assert not D.mask_faults(m, p)
            ones, got = torch.ones(m.numel(), device=DEV), torch.empty(m.numel(), device=DEV)
            O.dropout(ones, got, 1, m.numel(), m.numel(), (seed_t, p, site))
            assert torch.equal(got.view_as(m).double(), m)
        masked = dict(pano, dy=pano["dy"].double() * m_p)                     # the references take dy in float64: the product is exact there
        refs, (dP0_64, envp), _ = _eib_refs(H, masked, None, dtype)
        other = _eib_refs(H, dict(pano, dy=pano["dy"].double() * D.mask64(seed_t, p, S_DDY + 1, M, H)), None, dtype)[0]
        tref = D.ln_bwd_drop_ref(tx["dy"], tx["y"], tx["gamma"], tx["beta"], tx["rstd"], m_dy, m_dx)
        for partial in (False, True):
            tag = f"{dt} embed_in_bwd H {H} M {M} MT {MT} p {p} {'partial' if partial else 'atomic'}"
            box = {}
            run(partial, lambda: box.update(out=eib_launch(H, pano, tx, 0.25, seed_t, p)))
            out = box["out"]
            assert check_guards(poison) == (2 if partial else 0), tag
            init = lambda t: torch.full_like(t, 0.25).reshape(-1)              # noqa: E731
            first = ("dg3", "db3", "d_nav", "d_tok")                           # upstream of the storage-type rounding of the sum LayerNorm's input gradient
            for k, (terms, env) in refs.items():
                if dtype == torch.float32 or k in first:
                    D.check_sum(out[k].reshape(-1), init(out[k]), terms, env, f"{k} [{tag}]")
            for k in first:                                                    # control: the mask of the next site
                assert D.sum_ratio(out[k].reshape(-1), init(out[k]), *other[k]) > 1.0, f"{tag}: {k} with the mask of the next site not noticed"
            if dtype == torch.float32:
                D.check_dx(out["dP0"][:M], dP0_64, envp, f"dP0 [{tag}]", dtype)
            assert guard_ok(out["dP0"], M) and guard_ok(out["t_dx"], MT) and guard_ok(out["t_dxm"], MT), f"{tag}: guard rows written"
            D.check_dx(out["t_dx"][:MT], tref["dx"], tref["env"], f"text dx [{tag}]", dtype)
            D.check_dx(out["t_dxm"][:MT], tref["dxm"], tref["dxm_env"], f"text dxm [{tag}]", dtype)
            note(("embed_in_bwd drop", "text dxm", dt), D.dx_ratio(out["t_dxm"][:MT], tref["dxm"], tref["dxm_env"], dtype))
            note(("embed_in_bwd drop", "dg3", dt), D.sum_ratio(out["dg3"], torch.full((H,), 0.25, device=DEV), *refs["dg3"]))
            assert not D.dropped_exact(out["t_dx"][:MT], out["t_dxm"][:MT], m_dx, p, dtype, tref["dxm"], D.REL * (tref["dxm"].abs() + tref["dxm_env"])), tag
            D.check_sum(out["t_dg"], torch.full((H,), 0.25, device=DEV), tref["dg_terms"], tref["dg_env"], f"text dgamma [{tag}]")
            D.check_sum(out["t_db"], torch.full((H,), 0.25, device=DEV), tref["db_terms"], tref["db_env"], f"text dbeta [{tag}]")
            i = torch.arange(MT, device=DEV)
            for k, rows, n in (("t_word", tx["ids"].long(), tx["V"]), ("t_pos", i % tx["L"] + 2, tx["L"] + 2), ("t_typ", torch.zeros_like(i), 1)):
                D.check_sum(out[k], torch.zeros(n, H, device=DEV), scatter(rows, tref["dx"], n)[None], scatter(rows, tref["env"], n)[None], f"text {k} [{tag}]")
            if MT % tx["L"] == 0:                                             # the position-major walk is live: the mask follows the physical row
                for mk, name in ((m_dy, "dy"), (m_dx, "dx")):
                    bm = D.permuted_rows_mask(mk, tx["L"])
                    o2 = D.ln_bwd_drop_ref(tx["dy"], tx["y"], tx["gamma"], tx["beta"], tx["rstd"], bm if name == "dy" else m_dy, bm if name == "dx" else m_dx)
                    got, key = (out["t_dx"], "dx") if name == "dy" else (out["t_dxm"], "dxm")
                    assert D.dx_ratio(got[:MT], o2[key], o2["env"] if key == "dx" else o2["dxm_env"], dtype) > 1.0, f"{tag}: logical-row {name} mask not noticed"


# ---- report ---------------------------------------------------------------------------------------------------------------------------------------
def test_zz_report():
    assert STATS, "nothing recorded: run the whole module in one process"
    names = sorted({k[:2] if len(k) == 3 else k[:1] for k in STATS}, key=str)
    for n in names:
        vals = [STATS.get(n + (dt,), float("nan")) for dt in D.DTYPES]
        print("  worst err / bound  " + f"{' '.join(n):28s}" + "  ".join(f"{v:.4f}" for v in vals))
