"""The float64 references, bounds and case table of tests/_chain_ref64.py (the teacher's row chain, csrc/chain.hip), checked without a GPU on the
very operands tests/test_chain_fp64_gpu.py launches:
  1. each reference is plain float64 torch, and the derived y2 bound really bounds a LayerNorm whose input moves by up to D_t;
  2. the honest fp32 emulation (the kernel's rounding points, one summation order per tile form) passes every bound at every case of the
     table in both types -- the worst err / bound per output and type is printed (-s) and stays below 1;
  3. every planted defect FAILS the bound of the output it corrupts, at every M of the table it applies to, in both orders and types
     (swaps need M >= 2, proj_off needs Np >= 512); gelu_trunc cannot be caught by a worst-case bound (see _chain_ref64's docstring): its
     figure is printed and it stays listed;
  4. the fragment-order mirror equals the formula of include/magic_hip.h, the launch-rule mirror the rule of launch_chain at the boundary
     tile counts."""
import pytest
import torch
import torch.nn.functional as F

from tests import _chain_ref64 as C

DT = list(C.DTYPES.items())
_HON = {}


def honest(dt, M, order):
    """the honest emulation of both variants at (type, M, order) and the references built from ITS stored stage inputs"""
    key = (dt, M, order)
    if key not in _HON:
        o = C.operands(dt, M)
        e = C.emulate(o, order)
        n = C.emulate(o, order, ffn=False)
        refs = C.stage_refs(o, True, 768, e["y1"], e["y2"])
        refs["proj_noffn"] = C.proj_ref(o, n["y1"], 768)
        assert torch.equal(e["y1"].view(torch.int16), n["y1"].view(torch.int16))
        _HON[key] = (o, e, n, refs)
    return _HON[key]


def cut(ref, Np):
    """a projection reference restricted to the first Np columns (columns are independent)"""
    return C.R.Ref(ref.val[:, :Np], ref.env[:, :Np], ref.n)


# ---- 1. the references --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt", DT)
def test_references_are_plain_float64_torch(name, dt):
    o, e, _, refs = honest(dt, 33, 32)
    d = lambda k: getattr(o, k).double()                                                  # noqa: E731
    y1 = F.layer_norm(d("x") @ d("Wa").t() + d("ba") + d("res"), (C.H,), d("g1"), d("b1"), C.EPS)
    assert (refs["y1"].val - y1).abs().max().item() <= 1e-11
    s1 = e["y1"].double()
    y2 = F.layer_norm(F.gelu(s1 @ d("W1").t() + d("bi")) @ d("W2").t() + d("bo2") + s1, (C.H,), d("g2"), d("b2"), C.EPS)
    assert (refs["y2"].val - y2).abs().max().item() <= 1e-11
    assert (refs["proj"].val - (e["y2"].double() @ d("Wp").t() + d("bp"))).abs().max().item() <= 1e-11


@pytest.mark.parametrize("name,dt", DT)
def test_the_derived_y2_bound_holds_for_any_input_error_within_D(name, dt):
    """t moved by +-D_t with the signs that move the mean, the variance, both, and random ones: the float64 LayerNorm of the moved t stays
    within first order + remainder of the reference"""
    o, e, _, refs = honest(dt, 65, 32)
    r = refs["y2"]
    g2, b2 = o.g2.double(), o.b2.double()
    xhat = (r.val - b2) / g2
    gen = torch.Generator().manual_seed(3)
    signs = [torch.ones_like(xhat), -torch.ones_like(xhat), xhat.sign(), -xhat.sign(), (g2 * xhat).sign(),
             torch.where(torch.rand(xhat.shape, generator=gen) < 0.5, -1.0, 1.0).double()]
    worst = 0.0
    for s in signs:
        for scale in (1.0, 0.5):
            moved = F.layer_norm(r.t + scale * s * r.Dt, (C.H,), g2, b2, C.EPS)
            worst = max(worst, ((moved - r.val).abs() / r.carry).max().item())
    print(f"{name}: worst |LN(t + d) - LN(t)| / (first order + remainder) = {worst:.4f}; carried bound up to {r.carried:.4f} sigma")
    assert worst <= 1.0


# ---- 2. the honest emulation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [32, 16])
@pytest.mark.parametrize("name,dt", DT)
def test_honest_emulation_passes_every_bound_at_every_case(name, dt, order):
    worst = {"y1": 0.0, "y2": 0.0, "proj": 0.0}
    for ffn, Np, store_y1, M, _ in C.CASES:
        o, e, n, refs = honest(dt, M, order)
        got = e if ffn else n
        rs = {"y1": refs["y1"]}
        if ffn:
            rs["y2"] = refs["y2"]
        if Np:
            rs["proj"] = cut(refs["proj" if ffn else "proj_noffn"], Np)
        for k, ref in rs.items():
            val = got[k][:, :Np] if k == "proj" else got[k]
            x = C.ratio(val, ref, dt)
            worst[k] = max(worst[k], x)
            assert x <= 1.0, (C.case_id((ffn, Np, store_y1, M, False)), k, x)
    print(f"honest emulation, order {order}, {name}: worst err / bound " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(0.0 < v < 1.0 for v in worst.values())


# ---- 3. planted defects ---------------------------------------------------------------------------------------------------------------------------
def defect_ratios(dt, d, outk):
    """[(M, order, variant, err / bound of the corrupted output)] over every M the defect applies to"""
    out = []
    for M in C.ROWS:
        if d.startswith("swap") and M < 2:
            continue
        for order in (32, 16):
            o, e, n, refs = honest(dt, M, order)
            for Np in ((768, 512) if d == "proj_off" else (768,)):
                bad = C.emulate(o, order, True, Np, d)
                ref = cut(refs["proj"], Np) if outk == "proj" else refs[outk]
                out.append((M, order, f"ffn np{Np}", C.ratio(bad[outk], ref, dt)))
                if outk == "proj":                                  # the projection reads y1 in the variant without FFN
                    bad = C.emulate(o, order, False, Np, d)
                    out.append((M, order, f"noffn np{Np}", C.ratio(bad["proj"], cut(refs["proj_noffn"], Np), dt)))
    return out


@pytest.mark.parametrize("d", list(C.DEFECTS))
@pytest.mark.parametrize("name,dt", DT)
def test_planted_defect_fails_the_bound_of_the_output_it_corrupts(name, dt, d):
    rs = defect_ratios(dt, d, C.DEFECTS[d])
    assert {r[0] for r in rs} == {M for M in C.ROWS if M >= 2 or not d.startswith("swap")}
    low = min(rs, key=lambda r: r[3])
    print(f"defect {d} ({name}) -> {C.DEFECTS[d]}: caught at every M, least err / bound {low[3]:.2f} (M = {low[0]}, order {low[1]}, {low[2]})")
    assert low[3] > 1.0, low


@pytest.mark.parametrize("name,dt", DT)
def test_truncated_gelu_is_planted_but_stays_inside_the_worst_case_bound(name, dt):
    assert "gelu_trunc" in C.UNCATCHABLE and "gelu_trunc" in C.__doc__
    rs = defect_ratios(dt, "gelu_trunc", "y2")
    o, e, _, _ = honest(dt, 33, 32)
    assert not torch.equal(C.emulate(o, 32, defect="gelu_trunc")["y2"].view(torch.int16), e["y2"].view(torch.int16))
    print(f"defect gelu_trunc ({name}) -> y2: NOT caught, err / bound {min(r[3] for r in rs):.3f} .. {max(r[3] for r in rs):.3f}")


# ---- 4. the table and the mirrors -------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_form_and_row_edge():
    assert len(C.FORMS) == 15 and len(set(C.FORMS)) == 15 and (False, 0, False) not in C.FORMS
    assert len(C.CASES) == len(set(C.CASES)) == 15 * 2 + 4 * 6
    for form in C.FORMS:
        assert {c[3] for c in C.CASES if c[:3] == form} >= {33, 65}
    for form in C.EDGE_FORMS:
        assert {c[3] for c in C.CASES if c[:3] == form} == {1, 31, 32, 33, 63, 64, 65, 97}
    for c in C.CASES:
        assert c[4] == (c[:3] in C.PRODUCTION)
    # row scales over 2^-6 .. 2^3, row 0 at 1 | 1; every row distinct; NaN around the slice
    o = C.operands(torch.bfloat16, 97)
    assert torch.isnan(o.x_full[:, :C.H].float()).all() and torch.isnan(o.x_full[:, 2 * C.H:].float()).all() and torch.isfinite(o.x.float()).all()
    rms = o.x.double().pow(2).mean(-1).sqrt()
    assert rms.max() / rms.min() > 2.0 ** 7 and len({tuple(r.tolist()) for r in o.x.float()}) == 97
    for k in ("g1", "g2"):
        g = getattr(o, k)
        assert (g > 0).any() and (g < 0).any() and g.unique().numel() == C.H
    for k in ("ba", "bi", "bo2", "bp", "b1", "b2"):
        assert getattr(o, k).unique().numel() == getattr(o, k).numel()


def test_fragment_order_mirror_is_the_formula_of_the_header():
    """chunk ((nt K / 32 + ks) 64 + l) of 8 elements = W[16 nt + (l & 15), 32 ks + 8 (l >> 4) .. + 7]"""
    N, K = 48, 96
    W = torch.arange(N * K, dtype=torch.float32).view(N, K)
    f = C.frag_order(W).view(-1, 8)
    for nt in range(N // 16):
        for ks in range(K // 32):
            for l in range(64):
                row, col = 16 * nt + (l & 15), 32 * ks + 8 * (l >> 4)
                assert torch.equal(f[(nt * (K // 32) + ks) * 64 + l], W[row, col:col + 8])


def test_launch_rule_mirror_at_the_boundary_tile_counts():
    cus = 256
    assert C.launch_rule(1, 32 * cus, None, cus) == (32, cus, 0, cus)                    # exactly one round of 32-row tiles
    assert C.launch_rule(1, 32 * cus + 1, None, cus) == (64, cus // 2 + 1, 0, cus // 2 + 1)
    assert C.launch_rule(1, 32 * 200, 32 * 56, cus) == (32, 200, 56, 200)                # a pair counts both problems' tiles
    assert C.launch_rule(1, 32 * 200, 32 * 56 + 1, cus) == (64, 100, 29, 100)
    assert C.launch_rule(1, 1, 1, 1)[0] == 64 and C.launch_rule(1, 1, None, 1)[0] == 32
    for M, t32, t64 in ((1, 1, 1), (32, 1, 1), (33, 2, 1), (64, 2, 1), (65, 3, 2), (97, 4, 2)):
        assert C.launch_rule(32, M, None, cus) == (32, t32, 0, t32) and C.launch_rule(64, M, None, cus) == (64, t64, 0, t64)
    assert C.launch_rule(64, 1, 65, cus) == (64, 1, 2, 1) and C.launch_rule(32, 64, 1, cus) == (32, 2, 1, 2)
