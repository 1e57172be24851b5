"""The fp64 harness of tests/test_navmodes_fp64_gpu.py, checked without a GPU at H = 128 with 2 / 2 / 1 layers:

  * without rounding, tests/_navmodes_ref64.Ref64 (its functional restatement, the K/V cache included) gives what oracle.nav_ref.RefVLNBert gives
    under tests/test_nav_gpu.one_step / tests/test_causal_gpu.step -- every output and every gradient to 1e-12: the harness is the oracle the fp32
    tests use, not a second opinion;
  * every planted defect moves at least one compared quantity beyond the fp16 bound of its class (H = 128 bounds of the GPU file) and beyond
    10 x 2^-11, the floor this test held before the bounds were measured; CAUGHT_BY says which quantity catches which defect;
  * the action-argmax precondition of the GPU file holds on the seeds it uses: every row's top-2 gap of the oracle's logits exceeds twice the fp16
    logit bound, at least 3 of 4 rows twice the bf16 bound."""
import pytest
import torch

from tests import _navmodes_ref64 as NR
from tests import test_navmodes_fp64_gpu as G

FLOOR = 10 * 2.0 ** -11
# defect -> the compared quantity that moves most in units of its fp16 bound (asserted below: it is one of DEFECTS[n]'s candidates)
CAUGHT_BY = {1: "fwd gmap_embeds", 2: "grad sprel", 3: "fwd cls_embeds", 4: "din vp_img", 5: "grad w", 6: "dkv", 7: "dkv", 8: "logit",
             9: "grad gate", 10: "fwd pano_embeds", 11: "value"}
_REFS = {}


def clean(kind, causal=None):
    """the clean reference of one case kind at H = 128 (kept for the file)"""
    key = (kind, causal)
    if key not in _REFS:
        case = G.case_of(kind, 128, causal=causal)
        o = NR.oracle(G.config(case), seed=case["seed"])
        _REFS[key] = (case, o, G.reference_of(case, o, None))
    return _REFS[key]


def _close(a, b, name):
    if a is None or b is None:
        assert a is None and b is None, name
        return
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin), name
    d = torch.where(fin, a - b, torch.zeros_like(b)).abs().max().item()
    assert d <= 1e-12 * max(1.0, b[fin].abs().max().item()), f"{name}: {d:.3e}"


@pytest.mark.parametrize("kind,causal", [("step", None), ("step-nogate", None), ("cached", None)] + [("causal", c) for c in G.CAUSAL_COMBOS])
def test_unrounded_harness_equals_the_oracle_under_the_fp32_tests_drivers(kind, causal):
    case, o, want = clean(kind, causal)
    for p in o.parameters():
        p.grad = None
    # the oracle itself under the same driver and loss; it has no K/V cache: the cached case must agree with the plain one
    r = NR.run(o, G.inputs_of(case), G.driver_of(case), dz=G.dicts_of(case), device="cpu", f64=True)
    for a, b in zip(want.outs, r.outs):
        for k in b:
            _close(a[k], b[k].detach(), k)
    _close(want.loss, r.loss, "loss")
    n = 0
    for name, p in o.named_parameters():
        _close(want.grads[name], None if p.grad is None else p.grad, "grad " + name)
        n += p.grad is not None
    assert n > 60
    for key, taps in (("gmap_img", r.tap.gimg), ("vp_img", r.tap.vimg)):
        for a, t in zip(want.din[key], taps):
            _close(a, t.grad, "d " + key)
    _close(want.din["txt"], r.tap.txt.grad, "d txt_embeds")
    if case["use_kv"]:
        assert want.dkv is not None and want.dkv.abs().max() > 0


def _moved(n):
    what, cands, kind = NR.DEFECTS[n]
    if kind == "critic":
        sd, x = G.critic_inputs()
        v, dx, gr = NR.critic_reference(sd, x, None)
        vb, _, _ = NR.critic_reference(sd, x, None, defect=11)
        return {"value": (vb - v).abs().max().item()}
    causal = {9: G.CAUSAL_COMBOS[1], 10: G.CAUSAL_COMBOS[2]}.get(n)
    case, o, want = clean(kind, causal)
    bad = G.reference_of(case, o, None, defect=n)
    return {q: v for q, v in NR.compare(bad, want).items() if isinstance(v, float)}


@pytest.mark.parametrize("n", sorted(NR.DEFECTS))
def test_every_planted_defect_moves_a_compared_quantity_beyond_its_fp16_bound(n):
    moved = _moved(n)
    bound = G.BOUNDS["fp16"][128]
    ratio = {q: v / bound[NR.qclass(q)] for q, v in moved.items() if not q.startswith("cos ") and NR.qclass(q) in bound}
    best = max(ratio, key=ratio.get)
    print(f"defect {n} ({NR.DEFECTS[n][0]}): " + ", ".join(f"{q} {moved[q]:.3g} ({ratio[q]:.3g}x)" for q in sorted(ratio, key=ratio.get)[::-1][:4]))
    q = CAUGHT_BY[n]
    assert q in NR.DEFECTS[n][1]
    assert moved[q] > bound[NR.qclass(q)] and moved[q] > (FLOOR if q != "value" else bound["value"]), (n, q, moved[q])
    assert ratio[best] > 1.0


def test_argmax_precondition_holds_on_the_chosen_seeds():
    """(H = 128, unrounded weights; the GPU file asserts the same on the reference of every case, width and type before it compares an argmax)"""
    for kind, causal in [("step", None), ("step-nogate", None), ("cached", None)] + [("causal", c) for c in G.CAUSAL_COMBOS]:
        case, o, want = clean(kind, causal)
        lens = G.inputs_of(case)[0]["txt_masks"].sum(1).tolist()
        assert 6 in lens and case["L"] in lens, lens
        for out in want.outs:
            gap = NR.top2_gap(out["fused_logits"])
            assert (gap > 2 * G.BOUNDS["fp16"][128]["logit"]).all(), (kind, causal, gap)
            assert int((gap > 2 * G.BOUNDS["bf16"][128]["logit"]).sum()) >= len(gap) - 1, (kind, causal, gap)
