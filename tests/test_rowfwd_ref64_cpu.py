"""The float64 references and bounds of tests/_rowfwd_ref64.py, checked without a GPU:
  1. each reference agrees with plain float64 torch (layer_norm, softmax and its autograd, a dense matrix for the CSR gather);
  2. an fp32 / 16-bit emulation of each kernel's documented dataflow passes every check on every case's inputs that
     tests/test_rowfwd_fp64_gpu.py launches (same builders, same seeds), in bf16, fp16 and fp32;
  3. every planted defect, applied to the emulated result for those inputs, fails the same check in every storage type it applies to;
  4. the case table claims every branch it is meant to reach (by the mirrored launch rules)."""
import pytest
import torch
import torch.nn.functional as F

from tests import _rowfwd_ref64 as R

IDS = lambda cs: [c.id for c in cs]
_OPS = {}


def ops(c, dt):
    key = (c.id, dt)
    if key not in _OPS:
        _OPS[key] = R.operands(c, dt)
    return _OPS[key]


# ---- 1. the references themselves ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CASES["ln"][:6] + R.CASES["embed_in"][:2], ids=IDS(R.CASES["ln"][:6] + R.CASES["embed_in"][:2]))
def test_layernorm_reference_is_torch_layer_norm(c):
    o = ops(c, "fp32") if c.kind == "ln" else ops(c, "fp32").text
    if o is None or not o.do_ln:
        return
    x = sum(R.ln_terms(o, R.F64))
    y, gx, rstd = R.ln64(x, o.gamma, o.beta)
    want = F.layer_norm(x, (o.H,), o.gamma.double(), o.beta.double(), R.EPS)
    assert (y - want).abs().max().item() <= 1e-12
    assert (rstd - 1 / (x.var(-1, unbiased=False) + R.EPS).sqrt()).abs().max().item() <= 1e-12


def test_table_row_rule():
    idx = torch.tensor([4, 0, 2], dtype=torch.int32)
    assert R.tab_rows((None, idx, 5, 9), 3).tolist() == [4, 0, 2]
    assert R.tab_rows((None, None, 3, 2), 5).tolist() == [2, 3, 4, 2, 3]
    assert R.tab_rows((None, None, 0, 1), 3).tolist() == [1, 1, 1]


@pytest.mark.parametrize("c", R.CASES["csr"][:8] + R.CASES["csrm"][:2], ids=IDS(R.CASES["csr"][:8] + R.CASES["csrm"][:2]))
def test_gather_reference_is_a_dense_product(c):
    o = ops(c, "fp32")
    for p in (o.probs if c.kind == "csrm" else [o]):
        ptr, idx, w = p.csr
        A = torch.zeros(p.M, p.src.shape[0], dtype=R.F64)
        for r in range(p.M):
            for e in range(int(ptr[r]), int(ptr[r + 1])):
                A[r, int(idx[e])] += 1.0 if w is None else float(w[e])
        got, env, deg = R.gather64(p.src, p.csr)
        assert (got - A @ p.src.double()).abs().max().item() <= 1e-12
        assert deg.tolist() == (ptr[1:] - ptr[:-1]).tolist() and (env >= got.abs() - 1e-12).all()


@pytest.mark.parametrize("c", R.CASES["softmax"][4:12], ids=IDS(R.CASES["softmax"][4:12]))
def test_softmax_reference_and_its_backward_equal_autograd(c):
    o = ops(c, "fp32")
    S = o.S[..., :c.Nk].double().requires_grad_(True)
    x = S * R.SCALE
    if o.kmask is not None:
        x = x + ((o.kmask == 0).double() * R.NEG)[:, None, None, :]
    sw = sb = None
    if o.dist is not None:
        sw, sb = o.sw.double().requires_grad_(True), o.sb.double().requires_grad_(True)
        x = x + (sw * o.dist.double() + sb)[:, None]
    P = torch.softmax(x, -1)
    Pr, _, _ = R.softmax_ref(c, o)
    assert (Pr - P).abs().max().item() <= 1e-12
    g = o.dP[..., :c.Nk].double()
    grads = torch.autograd.grad((P * g).sum(), [S] + ([sw, sb] if sw is not None else []))
    r = R.softmax_bwd_ref(c, o, P.detach())
    assert (r[0] - grads[0]).abs().max().item() <= 1e-12
    if sw is not None:
        assert abs(r[2].item() - grads[1].item()) <= 1e-10 and abs(r[4].item() - grads[2].item()) <= 1e-10


def test_smallk_lndot_headmean_and_pano_references_are_plain_torch():
    c = R.CASES["smallk"][7]
    o = ops(c, "fp32")
    z, _ = R.smallk_pre64(o)
    assert (z - F.linear(o.x.double(), o.W.double(), o.b.double())).abs().max().item() <= 1e-12
    c = R.CASES["lndot"][6]
    o = ops(c, "fp32")
    want = F.layer_norm(o.Y.double(), (c.H,), o.gamma.double(), o.beta.double(), R.EPS) @ o.w2.double() + o.b2.double()
    assert (R.lndot64(o)[0] - want).abs().max().item() <= 1e-12
    for c in R.CASES["headmean"]:
        o = ops(c, "fp32")
        P = o.P.double().requires_grad_(True)
        mean, _, dP, _ = R.headmean64(o.P, o.g, o.base)
        assert (mean - P.mean(1)).abs().max().item() <= 1e-15
        grad, = torch.autograd.grad((P.mean(1) * o.g.double()).sum(), P)
        assert (dP - (grad + (o.base.double() if o.base is not None else 0))).abs().max().item() <= 1e-15
    c = R.CASES["pano"][9]
    o = ops(c, "fp32")
    r = R.pano_ref(o.x, o.lens, o.wf, o.bf, torch.float32, o.P)
    valid = torch.arange(c.V)[None] < o.lens[:, None]
    p = torch.softmax((o.x.double() @ o.wf.double() + o.bf.double()).masked_fill(~valid, float("-inf")), -1)
    assert (r.p - p).abs().max().item() <= 1e-15 and (r.fused - torch.einsum("nv,nvh->nh", p, o.x.double())).abs().max().item() <= 1e-12


# ---- 4. rules and coverage -----------------------------------------------------------------------------------------------------------------------
def test_rule_mirrors_and_branch_coverage():
    """every named branch is claimed by a case whose shape and operands take it by the mirrored rules, in every storage type (a case's shape and
    integer operands are the same in all three, which is asserted)"""
    assert [R.ROWS_PER_WG[k] for k in ("ln", "lndot", "softmax", "csr", "smallk", "node_in", "embed_in")] == [4, 4, 4, 4, 16, 16, 16]
    assert [R.smallk_body(H) for H in R.WIDTHS] == ["W in registers", "W in registers", "W re-read", "W re-read"]
    assert R.pano_register_form(40, 768) and not R.pano_register_form(41, 128) and not R.pano_register_form(5, 192)
    assert not any(R.h_ok(H) for H in (64, 512, 896))
    for kind, cases in R.CASES.items():
        claimed = {dt: set() for dt in R.DTYPES}
        assert len({c.id for c in cases}) == len(cases)
        for c in cases:
            for dt in R.DTYPES:
                inf = R.inferred_branches(c, ops(c, dt))
                missing = set(c.branch) - inf
                assert not missing, f"{c.id} {dt}: declares {sorted(missing)}, the rules give {sorted(inf)}"
                claimed[dt] |= set(c.branch)
        for dt in R.DTYPES:
            assert R.BRANCHES[kind] <= claimed[dt], f"{kind} {dt}: branches without a case: {sorted(R.BRANCHES[kind] - claimed[dt])}"
    claimed = set()
    for a, b in R.PAIRS:
        for c in (a, b):
            assert set(c.branch) <= R.inferred_branches(c) | {f"split {R.pair_split(a.M)}"}, c.id      # B's workgroups start where A's end
            claimed |= set(c.branch)
        assert a.H == b.H and R.pair_split(a.M) == -(-a.M // 4)
    assert R.BRANCHES["pair"] <= claimed
    assert {(a.M, b.M) for a, b in R.PAIRS} == {(5, 1), (1, 9), (4, 4)} and {a.H for a, _ in R.PAIRS} == set(R.WIDTHS)


# ---- 2. an honest emulation passes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.ALL, ids=IDS(R.ALL))
def test_emulated_dataflow_passes_every_check(c):
    for dt in R.DTYPES:
        o = ops(c, dt)
        R.verify(c, dt, o, R.emulate(c, dt, o), f"{dt} {c.id}")


def test_emulated_pair_launch_passes_every_check():
    for a, b in R.PAIRS:
        for dt in R.DTYPES:
            for c, (o, outs) in zip((a, b), R.emulate_pair(a, b, dt)):
                R.verify(c, dt, o, outs, f"{dt} {c.id}")


# ---- 3. planted defects fail ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", [d for d in R.DEFECTS if d != "pair gamma"])
def test_defects_are_caught(defect):
    hit = {dt: 0 for dt in R.DTYPES}
    for c in R.ALL:
        for dt in R.DTYPES:
            if not R.defect_applies(c, dt, defect):
                continue
            o = ops(c, dt)
            with pytest.raises(AssertionError):
                R.verify(c, dt, o, R.emulate(c, dt, o, defect), f"{dt} {c.id} [{defect}]")
            hit[dt] += 1
    need = ("bf16", "fp16") if defect == "unrounded A" else tuple(R.DTYPES)         # the rounding it skips is the identity in fp32 storage
    assert all(hit[dt] for dt in need), hit


def test_pair_launch_with_the_first_problems_gamma_is_caught():
    for a, b in R.PAIRS:
        for dt in R.DTYPES:
            _, (o, outs) = R.emulate_pair(a, b, dt, "pair gamma")
            with pytest.raises(AssertionError):
                R.verify(b, dt, o, outs, f"{dt} {b.id} [pair gamma]")
