"""No GPU: the mask restatement and the dropout-site references of tests/_drop_ref64.py on the builders the GPU files use.  An fp32 emulation of
every kernel (ascending sums, the kernel's rounding points) passes each check -- its worst error-to-bound ratio is printed with -s -- and every
planted defect fails on every case it is attached to.  Every case's mask has both values in its last row and last 16-column block and a keep count
within 4 sigma."""
import pytest
import torch

from tests import _drop_ref64 as D
from tests import _gemm_ref64 as G
from tests import _rowfwd_ref64 as RF

WORST = {}


def stat(k, r):
    WORST[k] = max(WORST.get(k, 0.0), r)


# ---- the mask ---------------------------------------------------------------------------------------------------------------------------------
def test_fmix32_published_vectors():
    """murmur3's fmix32 (with ka = kb = 0 the word drop_mul compares is fmix32(idx))"""
    want = {0: 0, 1: 0x514E28B7, 2: 0x30F4C306, 0xFFFFFFFF: 0x81F16F39}
    got = D.fmix32(torch.tensor(list(want), dtype=torch.int64))
    assert [int(v) for v in got] == list(want.values())
    assert [int(v) for v in D.hash_words(0, 0, 3)] == [0, 0x514E28B7, 0x30F4C306]


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate_and_values(p):
    m = D.mask64((11, 12), p, 5, 1 << 10, 1 << 10)
    thr, scale = D.keep_scale(p)
    assert set(m.unique().tolist()) == {0.0, scale}
    assert not D.mask_faults(m, p)
    assert scale == (2.0 if p == 0.5 else float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(0.1))))
    assert thr == (1 << 31 if p == 0.5 else int(float(torch.tensor(0.1, dtype=torch.float32)) * 4294967296.0))


def test_mask_is_flat_index_and_takes_any_site_and_seed_form():
    for site in (1, 777, 0xABCDEF01, 0xFFFFFFFF):
        a = D.mask64((3, 4), 0.1, site, 33, 128)
        assert torch.equal(a.view(-1), D.mask64((3, 4), 0.1, site, 1, 33 * 128).view(-1))
        assert torch.equal(a, D.mask64(torch.tensor([3, 4], dtype=torch.int32), 0.1, site, 33, 128))
        assert not torch.equal(a, D.mask64((3, 4), 0.1, (site + 1) & D.M32, 33, 128))
    hi = torch.tensor([0xFFFFFFF0, 0x80000001], dtype=torch.int64).to(torch.int32)          # seed words with the top bit set
    assert torch.equal(D.mask64(hi, 0.5, 9, 4, 128), D.mask64((0xFFFFFFF0, 0x80000001), 0.5, 9, 4, 128))
    # restated once more with Python integers
    ka, kb = 3 ^ (777 * 0x9E3779B1 & D.M32), (4 + 777 * 0x85EBCA77) & D.M32
    thr, scale = D.keep_scale(0.1)
    for idx in (0, 1, 127, 128, 4223):
        x = ((idx ^ ka) + kb) & D.M32
        x ^= x >> 16; x = x * 0x85EBCA6B & D.M32; x ^= x >> 13; x = x * 0xC2B2AE35 & D.M32; x ^= x >> 16      # noqa: E702
        assert D.mask64((3, 4), 0.1, 777, 33, 128).view(-1)[idx].item() == (scale if x >= thr else 0.0)


# ---- magic_linear_lnbwd -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", D.LNB_H)
@pytest.mark.parametrize("mode", D.LNB_MODES)
def test_linear_lnbwd_reference_accepts_the_emulation_and_rejects_every_defect(mode, H):
    dtype, x3 = D.DTYPES[mode[:4]], mode.endswith("x3")
    for K in D.LNB_K[G.bits(dtype)]:
        for M in D.LNB_M:
            o = D.lnb_operands(dtype, M, H, K, 90)
            for p, site, with_res in ((D.LNB_P, D.LNB_SITE, True), (0.5, D.LNB_BIG_SITE, False), (0.0, 0, True)):
                tag = f"{mode} H {H} M {M} K {K} p {p} site {site:#x}"
                mask = seed = None
                if p > 0:
                    seed = D.pick_seed(p, site, M, H)
                    mask = D.mask64(seed, p, site, M, H)
                    assert not D.mask_faults(mask, p), tag
                good, bad = D.lnb_refs(o, mask, with_res, x3, site, seed, p)
                got = dict(zip(("dx", "dxm", "dgamma", "dbeta"), D.emulate_linear_lnbwd(o, mask, with_res, x3)))
                refs = dict(zip(("dx", "dxm", "dgamma", "dbeta"), good))
                for name, ref in refs.items():
                    if ref is None:
                        continue
                    store = dtype if name in ("dx", "dxm") else torch.float32
                    r = G.ratio(got[name], ref, store)
                    stat(f"linear_lnbwd {name} {mode}", r)
                    assert r <= 1.0, f"{tag} {name}: {r:.3f}"
                for name, ref in bad.items():
                    out = name.split(":")[0]
                    store = dtype if out in ("dx", "dxm") else torch.float32
                    assert not G.passes(got[out], ref, store), f"{tag}: the check does not notice {name}"
                if mask is not None:
                    assert not D.dropped_exact(got["dx"], got["dxm"], mask, p, dtype, refs["dxm"].val, refs["dxm"].extra), tag
                    # why "dxm from the rounded dx" is no control: it stays inside the bound of the true reference
                    twice = (got["dx"].double() * mask)
                    if dtype != torch.float32 and p != 0.5:
                        assert ((twice - refs["dxm"].val).abs() <= G.bound(refs["dxm"], dtype) + G.ulp(refs["dx"].val, dtype) * mask).all()


# ---- magic_linear_ln ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", (128, 256, 384))
@pytest.mark.parametrize("dt", D.DTYPES)
def test_linear_ln_drop_reference(dt, H):
    dtype = D.DTYPES[dt]
    for K in G.LLN_K[G.bits(dtype)][:2]:
        for M in D.LLN_DROP_M:
            for p, site, with_res in ((0.1, 21, True), (0.5, D.LNB_BIG_SITE, False)):
                tag = f"{dt} H {H} M {M} K {K} p {p}"
                ops = G.lln_operands(dtype, M, H, K, 90)
                seed = D.pick_seed(p, site, M, H)
                mask, (r_out, r_rstd), bad = D.lln_drop_refs(dtype, K, ops, with_res, seed, p, site)
                assert not D.mask_faults(mask, p), tag
                x, W, bias, gamma, beta, res = ops
                out, rstd = D.emulate_linear_ln_drop(x[:, :K], W[:, :K], bias, gamma, beta, G.LLN_EPS, dtype, mask, res if with_res else None)
                for name, got, ref, store in (("out", out, r_out, dtype), ("rstd", rstd, r_rstd, torch.float32)):
                    r = G.ratio(got, ref, store)
                    stat(f"linear_ln drop {name} {dt}", r)
                    assert r <= 1.0, f"{tag} {name}: {r:.3f}"
                for name, ref in bad.items():
                    assert not G.passes(out, ref, dtype), f"{tag}: the check does not notice {name}"


# ---- magic_ln_fwd ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", D.DTYPES)
def test_ln_fwd_drop_reference(dt):
    dtype = D.DTYPES[dt]
    for c in D.ln_fwd_drop_cases():
        o = RF.ln_operands(c, dtype)
        for p in D.DROP_P:
            s_in, s_out = D.S_IN0, D.S_OUT
            seed = D.pick_seed(p, (s_in, s_out), c.M, c.H)
            m_in, m_out = D.mask64(seed, p, s_in, c.M, c.H), D.mask64(seed, p, s_out, c.M, c.H)
            assert not D.mask_faults(m_in, p) and not D.mask_faults(m_out, p), c.id
            for mi, mo in D.site_combos(m_in, m_out):
                tag = f"{dt} {c.id} p {p} in0 {mi is not None} out {mo is not None}"
                ref = D.ln_fwd_drop_ref(o, dtype, mi, mo)
                out, rstd, od = D.emulate_ln_fwd_drop(o, dtype, mi, mo)
                RF.check(("ln_fwd drop", dt), "out", out, *ref["out"], tag, WORST)
                RF.check(("ln_fwd drop", dt), "rstd", rstd, *ref["rstd"], tag, WORST)
                if mo is not None:
                    RF.check(("ln_fwd drop", dt), "out_drop", od, *ref["out_drop"], tag, WORST)
                    assert not D.dropped_exact(out, od, mo, p, dtype, *ref["out_drop"]), tag
                for name, bad in D.ln_fwd_drop_defects(o, dtype, mi, mo, seed, p, s_in, s_out).items():
                    which = name.split(":")[0]
                    got = od if which == "out_drop" else out
                    assert D.fails(lambda: RF.check(("x", dt), which, got, *bad, tag)), f"{tag}: {name} not noticed"


def rejected_dx(got, ref, env, dtype):
    """check_dx rejects -- and the ratio form the GPU file's controls use (no assertion message to build per control) says the same"""
    out = D.fails(lambda: D.check_dx(got, ref, env, "x", dtype))
    assert out == (D.dx_ratio(got, ref, env, dtype) > 1.0)
    return out


def rejected_sum(got, init, terms, env):
    out = D.fails(lambda: D.check_sum(got, init, terms, env, "x"))
    assert out == (D.sum_ratio(got, init, terms, env) > 1.0)
    return out


# ---- magic_ln_bwd ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", (128, 256))
@pytest.mark.parametrize("dt", D.DTYPES)
def test_ln_bwd_drop_reference(dt, H):
    dtype = D.DTYPES[dt]
    L_ = 19
    for M in (1, 5, 33, 2 * L_):
        rn = torch.Generator().manual_seed(H + M)
        r = lambda *s: torch.randn(*s, generator=rn, dtype=torch.float64)       # noqa: E731
        y, dy = r(M, H).to(dtype), r(M, H).to(dtype)
        gamma, beta, rstd = (1 + 0.2 * r(H)).float(), (0.2 * r(H)).float(), (r(M).abs() + 0.5).float()
        for p in (0.1, 0.5):
            s_dy, s_dx = D.S_DY, D.S_DX
            seed = D.pick_seed(p, (s_dy, s_dx), M, H)
            m_dy, m_dx = D.mask64(seed, p, s_dy, M, H), D.mask64(seed, p, s_dx, M, H)
            assert not D.mask_faults(m_dy, p) and not D.mask_faults(m_dx, p)
            for a, b in D.site_combos(m_dy, m_dx):
                tag = f"{dt} H {H} M {M} p {p} dy {a is not None} dx {b is not None}"
                ref = D.ln_bwd_drop_ref(dy, y, gamma, beta, rstd, a, b)
                dx, dxm, dg, db = D.emulate_ln_bwd_drop(dy, y, gamma, beta, rstd, dtype, a, b)
                i_g, i_b = torch.full((H,), 0.25), torch.full((H,), -0.5)
                D.check_dx(dx, ref["dx"], ref["env"], f"dx {tag}", dtype)
                assert not rejected_dx(dx, ref["dx"], ref["env"], dtype) and not rejected_sum(dg, i_g, ref["dg_terms"], ref["dg_env"])
                D.check_sum(dg, i_g, ref["dg_terms"], ref["dg_env"], f"dgamma {tag}")
                D.check_sum(db, i_b, ref["db_terms"], ref["db_env"], f"dbeta {tag}")
                if b is not None:
                    D.check_dx(dxm, ref["dxm"], ref["dxm_env"], f"dxm {tag}", dtype)
                    assert not D.dropped_exact(dx, dxm, b, p, dtype), tag
                    bads = {"next site": D.mask64(seed, p, (s_dx + 1) & D.M32, M, H), "columns off by one": D.mask64(seed, p, s_dx, M, H + 1)[:, :H]}
                    if M % L_ == 0:
                        bads["logical-row mask on the position-major walk"] = D.permuted_rows_mask(b, L_)
                    for name, bm in bads.items():
                        o2 = D.ln_bwd_drop_ref(dy, y, gamma, beta, rstd, a, bm)
                        assert (M == 1 and name == "columns off by one") or rejected_dx(dxm, o2["dxm"], o2["dxm_env"], dtype), f"{tag}: dxm defect '{name}' not noticed"
                if a is not None:
                    bads = {"next site": D.mask64(seed, p, s_dy + 1, M, H), "columns off by one": D.mask64(seed, p, s_dy, M, H + 1)[:, :H]}
                    if M % L_ == 0:
                        bads["logical-row mask on the position-major walk"] = D.permuted_rows_mask(a, L_)
                    for name, bm in bads.items():
                        o2 = D.ln_bwd_drop_ref(dy, y, gamma, beta, rstd, bm, b)
                        assert (M == 1 and name == "columns off by one") or rejected_dx(dx, o2["dx"], o2["env"], dtype), f"{tag}: dy defect '{name}' not noticed"
                    late = D.ln_bwd_drop_ref(dy, y, gamma, beta, rstd, None, b)          # site_dy applied after the gamma and beta sums
                    assert rejected_sum(dg, i_g, late["dg_terms"], late["dg_env"]), f"{tag}: dgamma summed before site_dy not noticed"
                    assert rejected_sum(db, i_b, late["db_terms"], late["db_env"]), f"{tag}: dbeta summed before site_dy not noticed"


def test_embedding_stage_masks_have_both_values_at_the_edges():
    """the seeds tests/test_dropsites_fp64_gpu.py picks for magic_embed_in_fwd / _bwd: one seed per launch, every site's mask within the rule"""
    assert {c.H for c in D.EIF_CASES} == set(RF.WIDTHS) and any(c.text for c in D.EIF_CASES) and not all(c.text for c in D.EIF_CASES)
    for p, sites, H in D.embed_mask_shapes():
        seed = D.pick_seed(p, sites, sites[0][1], H)
        for site, rows in sites:
            assert not D.mask_faults(D.mask64(seed, p, site, rows, H), p), (p, site, rows, H)


def test_zz_report():
    for k in sorted(WORST, key=str):
        print(f"  emulation worst err / bound  {str(k):48s} {WORST[k]:.4f}")
