"""The float64 attention reference and the bounds of tests/_attn_ref64.py, checked without a GPU:
  1. the reference's backward equals float64 autograd of its own forward to 1e-12, with and without mask, dist, dropout mask and dP_init;
  2. an fp32 / 16-bit emulation of the kernels' documented dataflow passes every check on every case's inputs that
     tests/test_attn_fp64_gpu.py launches (same builders, same seeds), in bf16, fp16 and fp32;
  3. every planted defect, applied to the emulated result for those inputs, fails at least one check in each storage type;
  4. the case table claims every branch of the kernels it is meant to reach (by the mirrored C rules).
The dropout masks here are drawn by torch (tests/_attn_ref64.synthetic_keep); the GPU file exports the kernels' own."""
import pytest
import torch

from tests import _attn_ref64 as R

ALL = R.FWD_CASES + R.BWD_CASES + [c for _, a, b in R.PAIRS for c in (a, b)] + R.LDP_CASES
IDS = lambda cs: [c.id for c in cs]
_CACHE = {}
_REFS = {}


def emulated(c, dt):
    """operands, mask, and the honest emulation of forward (and backward) for a case, computed once"""
    key = (c.id, dt)
    if key not in _CACHE:
        dtype = R.DTYPES[dt]
        o, keep = R.operands(c, dtype), R.synthetic_keep(c)
        P, Pd, ctx = R.emulate_fwd(c, dtype, o, keep)
        _CACHE[key] = (dtype, o, keep, P, Pd, ctx)
    return _CACHE[key]


def refs(c, dt):
    """the parts of the float64 reference that depend on the case's operands (and its honest P / ctx) only, computed once"""
    return _REFS.setdefault((c.id, dt), {})


def is_bwd(c):
    return c.kernel.startswith("bwd")


# ---- 1. the reference itself ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask,dist,drop,init", [(False, False, False, False), (True, False, False, False), (True, True, False, True),
                                                 (False, True, True, False), (True, False, True, True), (True, True, True, True)])
def test_reference_backward_equals_autograd_of_its_forward(mask, dist, drop, init):
    c = R.C("bwd8", 21, 37, ["self-check"], B=2, nh=3, mask=mask, dist=dist, p=0.1 if drop else 0.0, init=init, tag="autograd")
    o = R.operands(c, torch.float32)
    for n in ("q", "k", "v", "dO"):
        setattr(o, n, getattr(o, n).to(R.F64))
    keep = R.synthetic_keep(c)
    q, k, v = (t.clone().requires_grad_(True) for t in (o.q, o.k, o.v))
    oo = R.SimpleNamespace(**{**o.__dict__, "q": q, "k": k, "v": v})
    P, Pd, ctx = R.ref_forward(c, oo, keep)
    loss = (ctx * o.dO).sum()
    if init:
        loss = loss + (Pd * o.dP_init[..., :c.Nk].to(R.F64)).sum()
    gq, gk, gv = torch.autograd.grad(loss, (q, k, v))
    r = R.ref_backward(c, o, P.detach(), keep)
    for name, a, b in (("dQ", r.dQ, gq), ("dK", r.dK, gk), ("dV", r.dV, gv)):
        assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item()), name
    if mask:
        assert (P[0, :, :, c.Nk - 3:] == 0).all() and (P[1, :, :, 1] == 0).all()      # exp(-10000 - max) is 0 in fp64 as in fp32


def test_rule_mirrors_and_branch_coverage():
    """every branch named in the GPU file's table, and every pair form, is claimed by a case whose shape takes it by the mirrored rules"""
    claimed = {k: set() for k in R.BRANCHES}
    for c in R.FWD_CASES + R.BWD_CASES:
        assert c.dtypes(), c.id
        for dt in c.dtypes():
            R.check_case_rules(c, R.DTYPES[dt])
            claimed[c.kernel] |= set(c.branch) & R.inferred_branches(c, R.DTYPES[dt])
    for k, need in R.BRANCHES.items():
        assert need <= claimed[k], f"{k}: branches without a case: {sorted(need - claimed[k])}"
    # the table's alias column holds in all three storage types
    for c in R.BWD_CASES:
        if c.kernel != "bwd_ks":
            assert {R.bwd_alias(R.DTYPES[dt], c.Nq, c.Nk) for dt in c.dtypes()} == {c.branch[0] == "alias"}, c.id
    assert not R.attn_supported(torch.float32, 80, 80, 1) and not R.attn_supported(torch.float32, 128, 128, 1) and R.attn_supported(torch.bfloat16, 128, 128, 1)
    (_, fa, fb), (_, la, lb), (_, ba, bb), (_, b4a, b4b) = R.PAIRS
    assert R.fwd_lds(torch.bfloat16, fb.Nk) > R.fwd_lds(torch.bfloat16, fa.Nk) and fb.Nq > 64 and (fa.B, fa.nh) != (fb.B, fb.nh)
    assert la.Nk <= 128 < lb.Nk
    assert not R.bwd_waves8(ba.Nq, ba.Nk) and R.bwd_alias(torch.bfloat16, ba.Nq, ba.Nk) and R.bwd_waves8(bb.Nq, bb.Nk) and not R.bwd_alias(torch.bfloat16, bb.Nq, bb.Nk)
    assert not R.bwd_waves8(b4a.Nq, b4a.Nk) and not R.bwd_waves8(b4b.Nq, b4b.Nk) and R.bwd_lds(torch.bfloat16, b4a.Nq, b4a.Nk) > R.bwd_lds(torch.bfloat16, b4b.Nq, b4b.Nk)
    for c in R.LDP_CASES:
        assert c.ldp == R.rup(c.Nk, 32) > R.rup(c.Nk, 8)


# ---- 2. an honest emulation passes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL, ids=IDS(ALL))
def test_emulated_dataflow_passes_every_check(c):
    for dt in c.dtypes():
        dtype, o, keep, P, Pd, ctx = emulated(c, dt)
        tag = f"{dt} {c.id}"
        R.verify_fwd(c, dtype, o, keep, P, Pd, ctx, tag, cache=refs(c, dt))
        if is_bwd(c):
            dq, dk, dv = R.emulate_bwd(c, dtype, o, keep, P, ctx)
            R.verify_bwd(c, dtype, o, keep, P, ctx, dq, dk, dv, tag, cache=refs(c, dt))


# ---- 3. planted defects fail --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", R.FWD_DEFECTS)
def test_forward_defects_are_caught(defect):
    hit = {dt: 0 for dt in R.DTYPES}
    for c in ALL:
        for dt in c.dtypes():
            dtype, o, keep, _, _, _ = emulated(c, dt)
            if not R.defect_applies(c, dtype, defect):
                continue
            P, Pd, ctx = R.emulate_fwd(c, dtype, o, keep, defect)
            with pytest.raises(AssertionError):
                R.verify_fwd(c, dtype, o, keep, P, Pd, ctx, f"{dt} {c.id} [{defect}]", cache=refs(c, dt))
            hit[dt] += 1
    assert all(hit.values()), hit


@pytest.mark.parametrize("defect", R.BWD_DEFECTS)
def test_backward_defects_are_caught(defect):
    hit = {dt: 0 for dt in R.DTYPES}
    for c in ALL:
        if not is_bwd(c):
            continue
        for dt in c.dtypes():
            dtype, o, keep, P, _, ctx = emulated(c, dt)
            if not R.defect_applies(c, dtype, defect):
                continue
            dq, dk, dv = R.emulate_bwd(c, dtype, o, keep, P, ctx, defect)
            with pytest.raises(AssertionError):
                R.verify_bwd(c, dtype, o, keep, P, ctx, dq, dk, dv, f"{dt} {c.id} [{defect}]", cache=refs(c, dt))
            hit[dt] += 1
    need = ("bf16", "fp16") if defect == "accumulate overwrites" else tuple(R.DTYPES)         # accumulate_kv exists in 16-bit storage only
    assert all(hit[dt] for dt in need), hit


@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_pair_indexed_with_the_first_problems_head_count_is_caught(dt):
    """problem B of each pair with its (sample, head) taken from problem A's nh: the slots no block reaches keep the NaN fill"""
    for _, a, b in R.PAIRS:
        if a.nh == b.nh or dt not in b.dtypes():
            continue
        dtype, o, keep, P, Pd, ctx = emulated(b, dt)
        if is_bwd(b):
            dq, dk, dv = R.emulate_bwd(b, dtype, o, keep, P, ctx)
            R.verify_bwd(b, dtype, o, keep, P, ctx, dq, dk, dv, "clean")
            bad = [R.pair_with_first_problems_heads(t.float(), b, a.nh).to(dtype) for t in (dq, dk, dv)]
            with pytest.raises(AssertionError):
                R.verify_bwd(b, dtype, o, keep, P, ctx, *bad, "B with A's nh")
        else:
            bad = R.pair_with_first_problems_heads(ctx.float(), b, a.nh).to(dtype)
            with pytest.raises(AssertionError):
                R.verify_fwd(b, dtype, o, keep, P, Pd, bad, "B with A's nh")
