"""The float64 reference of magic_kd_cols (tests/_kdcols_ref64.py) shown right without a GPU: it reproduces what the reference's own kd_loss
returned on 2-D, 3-D and 4-D input (tests/golden/makd_kl.pt, minted by tests/golden/mint_makd_kl.py), equals oracle.makd_ref.kd_loss where that is
defined, its closed-form gradient equals autograd, its step aggregation reproduces GMapNavAgent.compute_kd_losses with 'kl' terms -- and three planted
defects (softmax over the last axis, T handed to the global / local terms, the weighted mean divided by numel) are caught by the same comparisons.
Plus the C ABI side that needs no device: magic_kd_cols is declared, exported, fastcall-bound, and its partial count is a pure host function."""
import os

import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from oracle import makd_ref as MK
from tests import _kdcols_ref64 as KR

RTOL = 1e-12                     # float64 against float64 of the same formula in another order


@pytest.fixture(scope="module")
def fx(golden_dir):
    return torch.load(os.path.join(golden_dir, "makd_kl.pt"), weights_only=False)


def _case(name):
    parts = name.split("_")
    return parts[0], float(parts[1][1:]), parts[2], len(parts) > 3


def test_reference_reproduces_every_primitive_value_of_the_fixture(fx):
    p = fx["prim"]
    assert len(p["cases"]) == 24
    for name, want in p["cases"].items():
        key, T, lt, weighted = _case(name)
        s, t = p["inputs"][key]
        assert s.dtype == torch.float32 and torch.isinf(s).any() | torch.isinf(t).any()
        got = KR.kd_loss_ref(s, t, T, p["w"] if weighted else None, lt)
        assert abs(float(got) - want) <= RTOL * abs(want) + 1e-15, (name, float(got), want)
        expr = KR.kd_expr(s.double(), t.double(), T, p["w"].double() if weighted else None, lt)
        assert abs(float(expr) - want) <= RTOL * abs(want) + 1e-15, (name, float(expr), want)


def test_planted_defects_are_caught_on_the_fixture(fx):
    """the softmax over the last axis instead of dim 1 (3-D and 4-D input), and the weighted mean divided by numel instead of numel / C"""
    p = fx["prim"]
    for name, want in p["cases"].items():
        key, T, lt, weighted = _case(name)
        s, t = p["inputs"][key]
        w = p["w"] if weighted else None
        if key != "d2":
            bad = float(KR.kd_loss_ref(s, t, T, w, lt, softmax_last=True))
            assert abs(bad - want) > 1e-3 * abs(want), name
        if weighted and lt == "mean":
            bad = float(KR.kd_loss_ref(s, t, T, w, lt, mean_by_numel=True))
            assert abs(bad * s.shape[1] - want) <= 1e-9 * abs(want) and abs(bad - want) > 0.5 * abs(want), name


def test_reference_equals_the_oracle_on_2d_unweighted_input():
    g = torch.Generator().manual_seed(3)
    s, t = 2 * torch.randn(5, 37, generator=g, dtype=torch.float64), 2 * torch.randn(5, 37, generator=g, dtype=torch.float64)
    s[1, 4] = t[1, 4] = float("-inf")
    w = torch.rand(5, generator=g, dtype=torch.float64)
    for T in (1.0, 2.0):
        for lt in ("sum", "mean"):
            assert abs(float(KR.kd_loss_ref(s, t, T, None, lt)) - float(MK.kd_loss(s, t, T, None, lt))) < 1e-12
            assert abs(float(KR.kd_loss_ref(s, t, T, w, lt)) - float(MK.kd_loss(s, t, T, w, lt))) < 1e-12


@pytest.mark.parametrize("shape", [(3, 5, 1), (2, 9, 3), (2, 7, 65)])
def test_closed_form_gradient_equals_autograd_through_the_reference_expression(shape):
    g = torch.Generator().manual_seed(sum(shape))
    s = (2 * torch.randn(*shape, generator=g)).double()
    t = (2 * torch.randn(*shape, generator=g)).double()
    t[0, 1, 0] = float("-inf")
    s[1, 2, 0] = t[1, 2, 0] = float("-inf")
    w = torch.rand(shape[0], generator=g, dtype=torch.float64) + 0.25
    for T, ww, norm, coef in ((1.0, None, 1.0, 1.0), (2.0, w, 0.37, 0.6)):
        ref = KR.kdcols_ref(s, t, T, ww, norm, coef)
        x = s.clone().requires_grad_(True)
        loss = KR.kd_expr(x, t, T, ww, "sum") * norm
        assert abs(float(ref["terms"].sum()) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
        (coef * loss).backward()
        auto = torch.nan_to_num(x.grad, nan=0.0)            # (autograd through where(-inf) leaves 0 there, as the closed form does: p_s = p_t = 0)
        assert (ref["grad"] - auto).abs().max().item() <= 1e-12 * max(1.0, auto.abs().max().item())
        assert (ref["grad_env"] >= ref["grad"].abs() - 1e-15).all() and (ref["terms_env"] >= ref["terms"].abs() - 1e-15).all()


def _agent(golden_dir):
    a = torch.load(os.path.join(golden_dir, "makd_agent.pt"), weights_only=False)
    heads = {n: (lambda x, w=w.double(), b=b.double(): torch.nn.functional.linear(x, w, b)) for n, (w, b) in a["heads"].items()}
    return a, heads


def _agent_case(name):
    kinds, role, lt, t, mode = name.split("_")
    feat, attn = kinds.split("-")
    return feat, attn, role, lt, int(t[1:]), mode == "RW"


def test_step_aggregation_reproduces_the_reference_method_with_kl_terms(fx, golden_dir):
    a, heads = _agent(golden_dir)
    assert fx["agent"]["inputs"] == "makd_agent.pt" and len(fx["agent"]["cases"]) == 36
    for name, want in fx["agent"]["cases"].items():
        feat, attn, role, lt, t, rw = _agent_case(name)
        so, to = (a["s_out"], a["t_out"]) if role == "t2s" else (a["t_out"], a["s_out"])
        got = KR.makd_kl_ref(t, so, to, heads, role=role, loss_type=lt, temperature=fx["agent"]["temperature"], weights=a["rw"].double() if rw else None,
                             feat_loss=feat, attn_loss=attn)
        assert set(want) <= set(got) and (t == 0 or "txt_emb_loss" not in want), name
        for k, v in want.items():
            assert abs(float(got[k]) - v) <= 1e-10 * abs(v) + 1e-14, (name, k, float(got[k]), v)


def test_temperature_on_the_global_and_local_terms_is_caught(fx, golden_dir):
    """the reference calls the global / local terms without a temperature (agent.py:651-673): handing them kdl_temperature = 2 moves every 'kl' term of the two
    abilities away from the fixture, and none of the others"""
    a, heads = _agent(golden_dir)
    name = "kl-kl_t2s_sum_t0_RW"
    want = fx["agent"]["cases"][name]
    bad = KR.makd_kl_ref(0, a["s_out"], a["t_out"], heads, role="t2s", loss_type="sum", temperature=2.0, weights=a["rw"].double(),
                         feat_loss="kl", attn_loss="kl", global_local_T=2.0)
    for k, v in want.items():
        off = abs(float(bad[k]) - v) > 1e-3 * abs(v)
        assert off == k.startswith(("global", "local")), (k, float(bad[k]), v)


def test_kd_cols_is_declared_exported_and_fastcall_bound():
    assert "magic_kd_cols" in L.SIGNATURES and "magic_kd_cols_parts" in L.SIGNATURES
    assert L.SIGNATURES["magic_kd_cols_parts"] == [L.i64, L.i32, L.i64]
    L.load()
    for n in ("magic_kd_cols", "magic_kd_cols_parts"):
        assert type(L._FN[n]).__name__ == "builtin_function_or_method", n
    parts = L._FN["magic_kd_cols_parts"]
    assert parts(3, 5, 1) == 1 and parts(4, 768, 1) == 1 and parts(2, 9, 3) == 2           # row form: four (o, i) rows per workgroup
    assert parts(2, 7, 64) == 1 and parts(2, 7, 65) == 1 and parts(1, 12, 257) == 2          # column form, C < 16: four 64-lane groups per workgroup
    assert parts(2, 300, 128) == 4                                                         # C >= 16: one group per workgroup
    assert parts(1 << 20, 2, 4096) == 1024                                                 # capped: the launch grid-strides
    assert parts(0, 5, 1) == parts(3, 0, 1) == parts(3, 5, 0) == -1
    assert parts(3, 5, 1) == L.load().magic_kd_cols_parts(3, 5, 1)                           # both bindings, one host function
