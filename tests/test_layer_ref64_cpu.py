"""tests/_layer_ref64.py checked on the CPU: the cross-stack fp64 reference that tests/test_layer_fp64_gpu.py holds the per-op layer path
to is oracle.model_ref.RefCrossLayer's autograd (two chained layers, replayed dropout masks, graph-distance bias, a seed on the top block's
dropped cross map); its kv-given form is consistent with the form that projects K/V inside; chained accumulating calls add up; and the
backward checks reject planted defects applied to fp64 results rounded ONCE to the storage type (the least noise a correct kernel can have),
at the H = 128 bounds BWD_BOUNDS -- the tightest the GPU file uses for the parameter and stack-input classes."""
import pytest
import torch

import oracle.layer_ref as LR
import oracle.model_ref as R
from magic_amd.host.config import make_config
from tests import _layer_ref64 as LH
from types import SimpleNamespace

H, NH, B, NQ, NK, NL, P = 128, 2, 4, 20, 40, 2, 0.1
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
FMT = "enc.{}."
SUFFIX = {"attention.self.dropout": "attn", "attention.output.dropout": "ao", "output.dropout": "out",
          "crossattention.self.dropout": "cattn", "crossattention.output.dropout": "co"}


def _close(a, b, what, tol=1e-10):
    err = ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
    assert err < tol, (what, err)


def _layers(seed):
    torch.manual_seed(seed)
    cfg = make_config(H, role="student")
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(NL):
        lyr = R.RefCrossLayer(cfg).double()
        with torch.no_grad():
            for n, p in lyr.named_parameters():
                if n.endswith("bias"):
                    p.copy_(torch.randn(p.shape, generator=g, dtype=p.dtype) * 0.05)
                if "LayerNorm.weight" in n:
                    p.add_(torch.randn(p.shape, generator=g, dtype=p.dtype) * 0.1)
        R.name_modules(lyr)
        out.append(lyr)
    return cfg, out


def _problem(seed=0, p=P, with_dist=True, with_dP=True):
    """operands of one backward through NL chained cross layers (ragged queries and keys, one 1-key sample)"""
    cfg, layers = _layers(seed + 1)
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)          # noqa: E731
    qlens, klens = torch.tensor([1, NQ - 1, NQ, 16]), torch.tensor([32, NK, NK - 1, 1])
    pr = SimpleNamespace(cfg=cfg, layers=layers, x=rnd(B, NQ, H), cx=rnd(B, NK, H), qmask=R.seq_mask(qlens, NQ), cmask=R.seq_mask(klens, NK),
                         d_top=rnd(B, NQ, H) * 0.1, dist=torch.rand(B, NQ, NQ, generator=g, dtype=torch.float64) * 6 if with_dist else None,
                         sprel=(-0.6, 0.25), dP=rnd(B, NH, NQ, NK) * 0.1 if with_dP else None, masks=None,
                         ws=[LR.self_weights(lyr) for lyr in layers])
    if p > 0:
        keep = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) >= p).double() / (1.0 - p)       # noqa: E731
        pr.masks = [{"attn": keep(B, NH, NQ, NQ), "ao": keep(B, NQ, H), "out": keep(B, NQ, H), "cattn": keep(B, NH, NQ, NK), "co": keep(B, NQ, H)}
                    for _ in range(NL)]
    return pr


def _reference(pr, **kw):
    args = dict(masks=pr.masks, dist=pr.dist, sprel=pr.sprel, dP=pr.dP)
    args.update(kw)
    x = args.pop("x", pr.x)
    return LH.cross_stack_reference(x, pr.cx, pr.ws, pr.qmask, pr.cmask, NH, args.pop("d_top", pr.d_top), **args)


def _oracle_autograd(pr):
    """the same backward through oracle.model_ref's layers: (dx, dctx, (d sprel w, d sprel b), per layer {layer_ref name: gradient})"""
    x, cx = pr.x.clone().requires_grad_(True), pr.cx.clone().requires_grad_(True)
    sp = torch.nn.Linear(1, 1).double()
    with torch.no_grad():
        sp.weight.fill_(pr.sprel[0])
        sp.bias.fill_(pr.sprel[1])
    cur = [0]

    def hook(name, t):
        m = pr.masks[cur[0]][SUFFIX[name.lstrip(".")]]
        assert m.shape == t.shape, (name, tuple(t.shape))
        return t * m
    sbias = R.key_bias(pr.qmask).double()
    if pr.dist is not None:
        sbias = sbias + sp(pr.dist.unsqueeze(3)).squeeze(3).unsqueeze(1)             # oracle.model_ref global_encode's form
    R.DROPOUT = hook if pr.masks else None
    try:
        h = x
        for j, lyr in enumerate(pr.layers):
            cur[0] = j
            h, pc = lyr(h, sbias, cx, R.key_bias(pr.cmask).double())
    finally:
        R.DROPOUT = None
    loss = (h * pr.d_top).sum() + ((pc * pr.dP).sum() if pr.dP is not None else 0.0)
    loss.backward()
    grads = []
    for lyr in pr.layers:
        at, ca = lyr.attention, lyr.crossattention
        g = lambda m: (m.weight.grad, m.bias.grad)                # noqa: E731
        d = {"Wqkv": torch.cat([at.self.query.weight.grad, at.self.key.weight.grad, at.self.value.weight.grad]),
             "bqkv": torch.cat([at.self.query.bias.grad, at.self.key.bias.grad, at.self.value.bias.grad]),
             "Wkv": torch.cat([ca.self.key.weight.grad, ca.self.value.weight.grad]), "bkv": torch.cat([ca.self.key.bias.grad, ca.self.value.bias.grad])}
        for (wn, bn), m in ((("Wo", "bo"), at.output.dense), (("g1", "be1"), at.output.LayerNorm), (("Wq", "bq"), ca.self.query),
                            (("Woc", "boc"), ca.output.dense), (("gc", "bec"), ca.output.LayerNorm), (("W1", "bi"), lyr.intermediate.dense),
                            (("W2", "bo2"), lyr.output.dense), (("g2", "be2"), lyr.output.LayerNorm)):
            d[wn], d[bn] = g(m)
        grads.append(d)
    dsp = (sp.weight.grad.reshape(()), sp.bias.grad.reshape(())) if pr.dist is not None else None
    return x.grad, cx.grad, dsp, grads


@pytest.mark.parametrize("p,with_dist,with_dP", [(0.0, False, False), (0.1, True, True), (0.1, False, True), (0.0, True, False)])
def test_cross_stack_reference_is_the_oracle_layers_autograd(p, with_dist, with_dP):
    pr = _problem(3, p, with_dist, with_dP)
    r = _reference(pr)
    dx, dctx, dsp, grads = _oracle_autograd(pr)
    _close(r.dx, dx, "d x")
    _close(r.dctx, dctx, "d context")
    assert set(r.grads[0]) == set(grads[0]) == set(LR.SELF_KEYS + LR.CROSS_KEYS + LR.FFN_KEYS)
    top = max(v.abs().max().item() for d in grads for v in d.values())
    for j in range(NL):
        for k, v in grads[j].items():
            assert ((r.grads[j][k] - v).abs().max() / top).item() < 1e-10, (j, k)
    if with_dist:
        _close(r.dsprel[0], dsp[0], "d sprel weight")
        # (the bias shifts every logit of a row alike: its gradient is analytically zero, noise on both sides)
        assert abs(r.dsprel[1].item()) < 1e-12 * abs(dsp[0].item()) and abs(dsp[1].item()) < 1e-12 * abs(dsp[0].item())
    else:
        assert r.dsprel is None
    # the context accumulator's earlier content is kept
    acc0 = torch.randn(B, NK, H, dtype=torch.float64)
    _close(_reference(pr, d_ctx0=acc0).dctx, acc0 + dctx, "d context on a pre-filled accumulator")


def test_kv_given_form_is_the_inside_form_split_at_the_projection():
    pr = _problem(5)
    inside = _reference(pr)
    kv = [LR.linear(pr.cx, w["Wkv"], w["bkv"]) for w in pr.ws]
    given = _reference(pr, kv=kv)
    assert given.dctx is None and all("Wkv" not in d and "bkv" not in d for d in given.grads)
    _close(given.dx, inside.dx, "d x")
    _close(sum(d @ w["Wkv"] for d, w in zip(given.dkv, pr.ws)), inside.dctx, "d kv through Wkv = d context")
    for j in range(NL):
        _close(torch.einsum("bnk,bnh->kh", given.dkv[j], pr.cx), inside.grads[j]["Wkv"], f"layer {j} d Wkv")
        _close(given.dkv[j].sum((0, 1)), inside.grads[j]["bkv"], f"layer {j} d bkv")
        for k, v in given.grads[j].items():
            _close(v, inside.grads[j][k], f"layer {j} {k}")
    # keys beyond a sample's length receive exactly nothing
    for j in range(NL):
        assert (given.dkv[j][~pr.cmask] == 0).all()


def test_two_chained_accumulating_calls_equal_the_sum():
    pr = _problem(7)
    kv = [LR.linear(pr.cx, w["Wkv"], w["bkv"]) for w in pr.ws]
    x2, top2 = torch.randn(B, NQ, H, dtype=torch.float64), torch.randn(B, NQ, H, dtype=torch.float64) * 0.1
    a, b = _reference(pr, kv=kv), _reference(pr, kv=kv, x=x2, d_top=top2)
    chained = _reference(pr, kv=kv, x=x2, d_top=top2, dkv0=a.dkv)
    for j in range(NL):
        _close(chained.dkv[j], a.dkv[j] + b.dkv[j], f"layer {j} accumulated d kv")
        assert (b.dkv[j] - a.dkv[j]).abs().max() > 1e-3 * a.dkv[j].abs().max()            # (the second call is another problem)
    c1 = _reference(pr)
    c2 = _reference(pr, x=x2, d_top=top2, d_ctx0=c1.dctx)
    _close(c2.dctx, c1.dctx + _reference(pr, x=x2, d_top=top2).dctx, "accumulated d context")


def _store_of(grads, dtype):
    """a stand-in for the engine's ParamStore holding `grads` (per layer, layer_ref names) rounded once to dtype under the store's names"""
    offsets, flat, off = {}, [], 0
    for j, d in enumerate(grads):
        for pn, rn, part in LH.CROSS_PNAMES:
            if rn not in d:
                continue
            r = d[rn]
            if part is not None:
                r = r.view(r.shape[0] // H, H, -1)[part] if r.dim() == 2 else r.view(-1, H)[part]
            r = r.reshape(-1).to(dtype).double()
            offsets[FMT.format(j) + pn] = (off, r.numel(), None)
            flat.append(r)
            off += r.numel()
    return SimpleNamespace(store=SimpleNamespace(offsets=offsets, grad=torch.cat(flat)))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_checks_reject_planted_defects(dtype):
    dt = DTYPES[dtype]
    kept = dict(LH.STATS)
    pr = _problem(9)
    sg = SimpleNamespace(ns=B, N=NQ)
    good = _reference(pr)
    m = _store_of(good.grads, dt)
    rounded = lambda t: t.to(dt).double()             # noqa: E731
    LH.check_param_grads(m, FMT, sg, good.grads, dtype, "clean", H, names=LH.CROSS_PNAMES)
    LH.check_dx_tiles(rounded(good.dx), good.dx, sg, dtype, "clean", H)
    LH.check_dx_tiles(rounded(good.dctx), good.dctx, sg, dtype, "clean", H, rows=NK, what="d context")
    # one 16-row tile of dx taken from the neighbouring sample
    t = rounded(good.dx)
    t[1, :16] = t[2, :16]
    with pytest.raises(AssertionError):
        LH.check_dx_tiles(t, good.dx, sg, dtype, "tile from the neighbouring sample", H)
    # d kv of the first of two accumulated calls missing
    kv = [LR.linear(pr.cx, w["Wkv"], w["bkv"]) for w in pr.ws]
    x2, top2 = torch.randn(B, NQ, H, dtype=torch.float64), torch.randn(B, NQ, H, dtype=torch.float64) * 0.1
    a = _reference(pr, kv=kv)
    both = _reference(pr, kv=kv, x=x2, d_top=top2, dkv0=a.dkv)
    for j in range(NL):
        LH.check_dx_tiles(rounded(both.dkv[j]), both.dkv[j], sg, dtype, "clean", H, rows=NK, what="d kv")
        with pytest.raises(AssertionError):
            LH.check_dx_tiles(rounded(both.dkv[j] - a.dkv[j]), both.dkv[j], sg, dtype, "first call's d kv missing", H, rows=NK, what="d kv")
    # the 'co' mask left out of the reference: every gradient class moves
    bad = _reference(pr, masks=[{k: v for k, v in mk.items() if k != "co"} for mk in pr.masks])
    with pytest.raises(AssertionError):
        LH.check_param_grads(m, FMT, sg, bad.grads, dtype, "reference without the 'co' mask", H, names=LH.CROSS_PNAMES)
    with pytest.raises(AssertionError):
        LH.check_dx_tiles(rounded(good.dx), bad.dx, sg, dtype, "reference without the 'co' mask", H)
    with pytest.raises(AssertionError):
        LH.check_dx_tiles(rounded(good.dctx), bad.dctx, sg, dtype, "reference without the 'co' mask", H, rows=NK, what="d context")
    # dP_init left out of the reference: the seed sits on the top block's cross map, so the top block's query projection carries most of it
    # (rel-L2 0.3 on its weight at this seed scale, 0.02 - 0.1 on the context rows' tiles, under 1e-2 on everything below the top block)
    bad = _reference(pr, dP=None)
    with pytest.raises(AssertionError):
        LH.check_param_grads(m, FMT, sg, bad.grads, dtype, "reference without dP_init", H, names=LH.CROSS_PNAMES)
    with pytest.raises(AssertionError):
        LH.check_dx_tiles(rounded(good.dctx), bad.dctx, sg, dtype, "reference without dP_init", H, rows=NK, what="d context")
    LH.STATS.clear()
    LH.STATS.update(kept)
