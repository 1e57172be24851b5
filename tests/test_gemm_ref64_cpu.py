"""The float64 GEMM references of tests/_gemm_ref64.py, checked without a GPU:
  1. they equal torch.matmul / float64 autograd to 1e-12;
  2. fp32-arithmetic emulations of an honest kernel (k after k; four interleaved partial sums; the result rounded to 16-bit storage) pass `check`;
  3. every planted defect test_gemm_fp64_gpu.py uses fails it, on the same seeded inputs at every shape that file runs -- so the controls bite.
Both files take their problems from the builders of tests/_gemm_ref64.py (magic_gemm cases, slabs, magic_gemm_dw_grouped / magic_gemm_dw_cat
problems, Linear + LayerNorm operands), so shapes and seeds cannot drift apart."""
import pytest
import torch
import torch.nn.functional as F

from tests import _gemm_ref64 as R

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
ACT_A = 2.0 ** -20          # the CPU emulation's erf is torch's fp32 erf, a few units of fp32 from the fp64 one


def close(a, b):
    return (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item())


# ---- 1. the reference itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_product_and_epilogues_equal_matmul_and_autograd(layout):
    g = torch.Generator().manual_seed(layout)
    nb, nh, M, N, K = 2, 3, 5, 7, 11
    A = torch.randn(*((nb, nh, M, K) if layout != 2 else (nb, nh, K, M)), generator=g, dtype=R.F64)
    B = torch.randn(*((nb, nh, N, K) if layout == 0 else (nb, nh, K, N)), generator=g, dtype=R.F64)
    a = A if layout != 2 else A.transpose(-1, -2)
    b = B.transpose(-1, -2) if layout == 0 else B
    bias, res, cin, aux = (torch.randn(*s, generator=g, dtype=R.F64) for s in ((N,), (nb, nh, M, N), (nb, nh, M, N), (nb, nh, M, N)))
    want = torch.matmul(a, b)
    r = R.gemm_ref(layout, A, B)
    assert close(r.val, want) and close(r.env, torch.matmul(a.abs(), b.abs())) and r.n == K
    v = -0.75 * want + bias
    r = R.gemm_ref(layout, A, B, alpha=-0.75, bias=bias, epilogue=1, residual=res, c_in=cin)
    assert close(r.val, F.gelu(v) + res + cin) and close(r.c2.val, v) and close(r.pre, v.abs())
    assert close(r.env, 0.75 * torch.matmul(a.abs(), b.abs()) + bias.abs() + res.abs() + cin.abs())
    assert close(R.gemm_ref(layout, A, B, bias=bias, epilogue=2).val, F.relu(want + bias))
    z = aux.clone().requires_grad_(True)
    F.gelu(z).backward(torch.ones_like(z))
    assert close(R.gemm_ref(layout, A, B, alpha=-0.75, bias=bias, epilogue=3, aux=aux).val, v * z.grad)
    assert close(R.gemm_ref(layout, A, B, epilogue=4, aux=aux).val, want * (aux > 0))
    # the slabs of a split-K add up to the product; an empty split is zeros
    s = R.slab_ref(layout, A, B, 4, 4, alpha=0.5, bias=bias)          # 3 tiles of 4 over 4 splits
    assert s.val.shape[0] == 4 and close(s.val.sum(0), 0.5 * want + bias) and (s.val[3] == 0).all() and (s.env[3] == 0).all()
    assert R.split_ranges(320, 64, 4) == [(0, 128), (128, 256), (256, 320), (320, 320)]


def test_weight_gradient_and_linear_ln_equal_autograd():
    g = torch.Generator().manual_seed(5)
    N, K = 6, 9
    parts = [(torch.randn(m, N, generator=g, dtype=R.F64), torch.randn(m, K, generator=g, dtype=R.F64)) for m in (4, 0, 1, 7)]
    W = torch.randn(N, K, generator=g, dtype=R.F64, requires_grad=True)
    bvec = torch.randn(N, generator=g, dtype=R.F64, requires_grad=True)
    sum((F.linear(x, W, bvec) * dy).sum() for dy, x in parts).backward()
    w0, b0 = torch.randn(N, K, generator=g, dtype=R.F64), torch.randn(N, generator=g, dtype=R.F64)
    rw, rb = R.dw_ref(parts, w0, b0)
    assert close(rw.val, W.grad + w0) and close(rb.val, bvec.grad + b0) and rw.n == rb.n == 12
    H, M = 128, 5
    x, Wl = torch.randn(M, K, generator=g, dtype=R.F64), torch.randn(H, K, generator=g, dtype=R.F64)
    bias, gam, bet, res = (torch.randn(*s, generator=g, dtype=R.F64) for s in ((H,), (H,), (H,), (M, H)))
    for act, fn in ((0, lambda t: t), (1, F.gelu), (2, F.relu)):
        for rr in (None, res):
            v = fn(F.linear(x, Wl, bias)) + (0 if rr is None else rr)
            out, rstd, pre = R.linear_ln_ref(x, Wl, bias, gam, bet, 1e-12, torch.float32, residual=rr, act=act)
            assert close(out.val, F.layer_norm(v, (H,), gam, bet, 1e-12)) and close(pre.val, F.linear(x, Wl, bias))
            assert close(rstd.val, 1.0 / torch.sqrt(v.var(-1, unbiased=False) + 1e-12))


# ---- 2. + 3. honest fp32 arithmetic passes, every planted defect fails, on the GPU file's inputs ------------------------------------------------
def honest_and_defects(c, tag):
    kw = {k: (v.view() if isinstance(v, R.Buf) else v) for k, v in c["kw"].items()}
    A, B = c["A"].view(), c["B"].view()
    for ways in (1, 4):
        out, pre = R.emulate_gemm(c["layout"], A, B, ways, store=c["store"], **kw)
        r = R.ratio(out, c["ref"], c["store"], ACT_A)
        assert r <= 1.0, f"{tag}: fp32 emulation ({ways} partial sums) at {r:.3f} of the bound"
        assert R.passes(pre.to(c["dtype"]), c["ref"].c2, c["dtype"])
    out, _ = R.emulate_gemm(c["layout"], A, B, 1, store=c["store"], **kw)
    defects = R.gemm_defects(c)
    assert {"last_row_missing", "last_col_missing"} <= set(defects)
    for name, d in defects.items():
        assert not R.passes(out, d, c["store"], ACT_A), f"{tag}: the check does not notice {name}"
    return set(defects)


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("dt", DTYPES)
def test_tile_edge_sweep_inputs(dt, layout):
    dtype = DTYPES[dt]
    for K in R.SWEEP_K[R.bits(dtype)]:
        for M in R.SWEEP_MN:
            for N in R.SWEEP_MN:
                seen = honest_and_defects(R.gemm_case(dtype, layout, M, N, K, bias=True, seed=1), f"{dt} layout {layout} {M}x{N}x{K}")
                assert {"last_k_missing", "bias_missing", "bias_doubled"} <= seen


@pytest.mark.parametrize("dt", DTYPES)
def test_operand_branch_inputs(dt):
    seen = set()
    for tag, kw in R.branch_cases(DTYPES[dt]):
        seen |= honest_and_defects(R.gemm_case(DTYPES[dt], seed=2, **kw), f"{dt} {tag}")
    assert seen == {"last_k_missing", "last_row_missing", "last_col_missing", "bias_missing", "bias_doubled", "alpha_one", "residual_missing",
                    "split_missing", "neighbour_aux"}


@pytest.mark.parametrize("dt", DTYPES)
def test_launch_form_inputs(dt):
    dtype = DTYPES[dt]
    for tag, _, kw in R.form_cases(dtype):
        honest_and_defects(R.gemm_case(dtype, seed=3, **kw), f"{dt} {tag}")
    c, rb, bad = R.bias_grad_case(dtype)
    honest_and_defects(c, f"{dt} xcd tn")
    A = c["A"].view()[0, 0]
    for ways in (1, 4):
        db = R.emulate_dw([(A, A[:, :1])], ways=ways)[1]
        assert R.passes(db, rb, torch.float32) and not R.passes(db, bad["last_k_missing"], torch.float32)
    if dtype != torch.float32:
        for M, N, K, _ in R.WIDE_SHAPES:
            for layout in (0, 1, 2):
                honest_and_defects(R.gemm_case(dtype, layout, M, N, K, bias=True, seed=4), f"{dt} wide {layout} {M}x{N}x{K}")


@pytest.mark.parametrize("dt", DTYPES)
def test_grouped_launch_inputs(dt):
    for family, _, _, kws in R.grouped_cases(DTYPES[dt]):
        for i, kw in enumerate(kws):
            honest_and_defects(R.gemm_case(DTYPES[dt], **kw), f"{dt} {family} problem {i} of {len(kws)}")


@pytest.mark.parametrize("dt", DTYPES)
def test_slab_mode_inputs(dt):
    for layout, K in R.slab_cases(DTYPES[dt]):
        c = R.slab_case(DTYPES[dt], layout, K)
        A, B = c["A"].view()[0, 0], c["B"].view()[0, 0]
        assert [hi - lo for lo, hi in c["slab_ranges"]] == c["slab_ref"].n.flatten().tolist() and c["slab_ranges"][2][0] == c["slab_ranges"][2][1] == K
        for ways in (1, 4):
            got = torch.stack([R.emulate_gemm(layout, A, B, ways, alpha=R.SLAB_ALPHA, bias=c["bias"] if s == 0 else None, lo=lo, hi=hi)[0]
                               for s, (lo, hi) in enumerate(c["slab_ranges"])])
            assert R.passes(got, c["slab_ref"], torch.float32) and (got[2] == 0).all(), (dt, layout, K, ways)
        for name, d in c["slab_defects"].items():
            assert not R.passes(got, d, torch.float32), f"{dt} slab layout {layout} K {K}: the check does not notice {name}"


def dw_honest_and_defects(parts, w0, b0, refs, defects, tag):
    rw, rb = refs
    for ways in (1, 4):
        w, b = R.emulate_dw(parts, w0, b0, ways)
        assert R.passes(w, rw, torch.float32), f"{tag}: fp32 emulation ({ways} partial sums) of dW"
        assert b0 is None or R.passes(b, rb, torch.float32), f"{tag}: fp32 emulation ({ways} partial sums) of db"
    for name, (dw_, db_) in defects.items():
        assert not R.passes(w, dw_, torch.float32), f"{tag}: the check does not notice {name} in dW"
        assert b0 is None or not R.passes(b, db_, torch.float32), f"{tag}: the check does not notice {name} in db"


@pytest.mark.parametrize("dt", DTYPES)
def test_dw_grouped_inputs(dt):
    """every problem of the GPU file's placement launch and its shared-dW launches, same seeds: honest fp32 sums pass; the last row missing and
    (shared dW) a problem missing fail, in dW and in db"""
    dtype = DTYPES[dt]
    groups = [p for p, _ in R.dw_placement_problems(dtype)] + R.dw_shared_problems(dtype, True) + R.dw_shared_problems(dtype, False)
    seen = set()
    for p in groups:
        if p.leader is p:
            bad = p.defects()
            seen |= set(bad)
            dw_honest_and_defects(p.parts(), p.w0, p.b0, p.refs(), bad, f"{dt} dW {p.N}x{p.K} over {[m.M for m in p.members]} rows")
    assert seen == {"last_row_missing", "problem_missing"}


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("dt", DTYPES)
def test_dw_cat_inputs(dt, wide):
    """every (N, K) of the GPU file's concatenated launch, same seeds: a segment, the first segment, the last row and dW_in / db_in missing fail"""
    probs = R.dw_cat_problems(DTYPES[dt], wide)
    assert len(probs) == 10 and not any(probs[-1].rows)
    for p in probs[:-1]:
        bad = p.defects()
        assert set(bad) == {"segment_missing", "first_segment_missing", "last_row_missing", "dW_in_missing"}
        dw_honest_and_defects(p.parts, p.w0, p.b0, p.refs(), bad, f"{dt} dw_cat {p.N}x{p.K}")


def lln_honest_and_defects(dtype, M, H, K, seed, variants, tag):
    ops = R.lln_operands(dtype, M, H, K, seed)
    x, W, bias, gamma, beta, res = ops
    for act, with_res in variants:
        (r_out, r_rstd, r_pre), bad = R.lln_refs(dtype, K, ops, act, with_res, ACT_A)
        out, rstd, pre = R.emulate_linear_ln(x[:, :K], W[:, :K], bias, gamma, beta, R.LLN_EPS, dtype, residual=res if with_res else None, act=act)
        t = f"{tag} act {act} res {with_res}"
        assert R.passes(out, r_out, dtype, ACT_A), f"{t}: fp32 emulation at {R.ratio(out, r_out, dtype, ACT_A):.3f} of the bound"
        assert R.passes(rstd, r_rstd, torch.float32) and R.passes(pre, r_pre, dtype), t
        assert {"last_k_missing", "bias_missing", "bias_doubled"} <= set(bad) and ("residual_missing" in bad) == with_res
        for name, d in bad.items():
            assert not R.passes(out, d, dtype, ACT_A), f"{t}: the check does not notice {name}"


@pytest.mark.parametrize("H", R.LLN_H)
@pytest.mark.parametrize("dt", DTYPES)
def test_linear_ln_inputs(dt, H):
    """the GPU file's magic_linear_ln / magic_linear_act_ln problems, same seeds: an fp32 Linear + LayerNorm passes, each control fails"""
    dtype = DTYPES[dt]
    for K in R.LLN_K[R.bits(dtype)]:
        for M in R.LLN_M:
            lln_honest_and_defects(dtype, M, H, K, 90, ((0, True), (0, False), (1, False), (2, False)), f"{dt} linear_ln H {H} M {M} K {K}")
    for M, seed, with_res in R.LLN_PAIR:
        lln_honest_and_defects(dtype, M, H, R.LLN_K[R.bits(dtype)][1], seed, ((0, with_res),), f"{dt} linear_ln pair H {H} M {M}")
