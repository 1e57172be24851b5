"""oracle/layer_ref.py (the per-stage fp64 restatement the encoder kernels are checked against) chained through whole layers reproduces
oracle.model_ref's RefSelfLayer / RefCrossLayer in fp64: same dropout masks (replayed through the R.DROPOUT hook), distance bias, ragged key
masks -- so the stage-by-stage GPU checks and the full-size oracle tests hold the kernels to the same arithmetic."""
import torch

import oracle.layer_ref as LR
import oracle.model_ref as R
from magic_amd.host.config import make_config

NH = 2


def _cfg():
    return make_config(128, role="student")


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g, dtype=p.dtype) * 0.05)
            if "LayerNorm.weight" in n:
                p.add_(torch.randn(p.shape, generator=g, dtype=p.dtype) * 0.1)
    return m


def _masks(B, Nq, Nk, H, p, seed, cross):
    """keep masks (scaled by 1/(1-p)) per dropout site, keyed by the site suffix the oracle's hook sees and by layer_ref's name"""
    g = torch.Generator().manual_seed(seed)

    def keep(*shape):
        return (torch.rand(*shape, generator=g, dtype=torch.float64) >= p).double() / (1.0 - p)
    m = {"attn": keep(B, NH, Nq, Nq), "ao": keep(B, Nq, H), "out": keep(B, Nq, H)}
    if cross:
        m["cattn"], m["co"] = keep(B, NH, Nq, Nk), keep(B, Nq, H)
    return m


def _hook(masks, cross):
    site = {"attention.self.dropout": "attn", "attention.output.dropout": "ao", "output.dropout": "out"}
    if cross:
        site.update({"crossattention.self.dropout": "cattn", "crossattention.output.dropout": "co"})
    used = []

    def hook(name, x):
        key = site[name.lstrip(".")]
        used.append(key)
        assert masks[key].shape == x.shape, (name, tuple(x.shape))
        return x * masks[key]
    return hook, used


def _close(a, b, what):
    err = ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
    assert err < 1e-12, (what, err)


def _ragged(B, N):
    lens = torch.tensor([1, N - 1, N, 16 if N > 16 else N][:B] + [N] * max(0, B - 4))
    return R.seq_mask(lens.clamp(1, N), N)


def test_self_layer_stages_chain_to_the_oracle_layer():
    torch.manual_seed(0)
    cfg = _cfg()
    lyr = _perturb(R.RefSelfLayer(cfg).double(), 1)
    R.name_modules(lyr)
    B, N, H = 4, 23, cfg.hidden_size
    x = torch.randn(B, N, H, dtype=torch.float64)
    kmask = _ragged(B, N)
    w = LR.self_weights(lyr)
    for p in (0.0, 0.1):
        masks = _masks(B, N, N, H, p, 7, False) if p else None
        hook, used = _hook(masks or {}, False)
        R.DROPOUT = hook if p else None
        try:
            with torch.no_grad():
                want, want_p = lyr(x, R.key_bias(kmask).double())
        finally:
            R.DROPOUT = None
        st = LR.self_layer(x, w, kmask, NH, cfg.layer_norm_eps, masks)
        if p:
            assert sorted(used) == ["ao", "attn", "out"]
            assert not torch.equal(st["Pd"], st["P"])
        _close(st["out"], want, f"p={p} out")
        _close(st["Pd"], want_p, f"p={p} probabilities after dropout")
        # rstd is the LayerNorm's own: the output is (v - mean) * rstd * gamma + beta
        v = x + (LR.linear(st["ctx"], w["Wo"], w["bo"]) * (masks["ao"] if p else 1.0))
        _close(st["rstd_a"], 1.0 / torch.sqrt(v.var(-1, unbiased=False) + cfg.layer_norm_eps), "rstd_a")
        # a masked key gets no probability, a one-key sample attends to its first key only
        assert (st["P"][1, :, :, N - 1] < 1e-300).all() and torch.allclose(st["P"][0, :, :, 0], torch.ones(NH, N, dtype=torch.float64))


def test_cross_layer_stages_with_distance_bias_chain_to_the_oracle_layer():
    torch.manual_seed(0)
    cfg = _cfg()
    lyr = _perturb(R.RefCrossLayer(cfg).double(), 2)
    R.name_modules(lyr)
    B, Nq, Nk, H = 4, 17, 49, cfg.hidden_size
    x, cx = torch.randn(B, Nq, H, dtype=torch.float64), torch.randn(B, Nk, H, dtype=torch.float64)
    qmask, cmask = _ragged(B, Nq), _ragged(B, Nk)
    dist = torch.rand(B, Nq, Nq, dtype=torch.float64) * 8
    sw, sb = torch.tensor(-0.7, dtype=torch.float64), torch.tensor(0.3, dtype=torch.float64)
    w = LR.self_weights(lyr)
    sp = torch.nn.Linear(1, 1).double()
    with torch.no_grad():
        sp.weight.fill_(sw.item())
        sp.bias.fill_(sb.item())
    for p, with_dist in ((0.0, False), (0.1, False), (0.1, True)):
        masks = _masks(B, Nq, Nk, H, p, 11, True) if p else None
        hook, used = _hook(masks or {}, True)
        sbias = R.key_bias(qmask).double()
        if with_dist:
            with torch.no_grad():
                sbias = sbias + sp(dist.unsqueeze(3)).squeeze(3).unsqueeze(1)          # oracle.model_ref global_encode's form
        R.DROPOUT = hook if p else None
        try:
            with torch.no_grad():
                want, want_p = lyr(x, sbias, cx, R.key_bias(cmask).double())
        finally:
            R.DROPOUT = None
        st = LR.cross_layer(x, cx, w, qmask, cmask, NH, cfg.layer_norm_eps, masks, dist=dist if with_dist else None, sprel=(sw, sb))
        if p:
            assert sorted(used) == ["ao", "attn", "cattn", "co", "out"]
        _close(st["out"], want, f"p={p} dist={with_dist} out")
        _close(st["Pdc"], want_p, f"p={p} dist={with_dist} cross probabilities")


def test_stages_are_differentiable_and_match_the_oracle_gradient():
    """the GPU backward tests take fp64 autograd of chained stages as their reference: its gradients must be the oracle layer's"""
    torch.manual_seed(0)
    cfg = _cfg()
    lyr = _perturb(R.RefSelfLayer(cfg).double(), 3)
    R.name_modules(lyr)
    B, N, H = 3, 20, cfg.hidden_size
    x = torch.randn(B, N, H, dtype=torch.float64, requires_grad=True)
    kmask = _ragged(B, N)
    dy = torch.randn(B, N, H, dtype=torch.float64)
    want, _ = lyr(x, R.key_bias(kmask).double())
    gx_want, gw_want = torch.autograd.grad(want, (x, lyr.intermediate.dense.weight), dy)
    w = {k: v.clone().requires_grad_(True) for k, v in LR.self_weights(lyr).items()}
    st = LR.self_layer(x, w, kmask, NH, cfg.layer_norm_eps)
    gx, gw = torch.autograd.grad(st["out"], (x, w["W1"]), dy)
    _close(gx, gx_want, "d x")
    _close(gw, gw_want, "d W1")


def test_gelu_derivative():
    z = torch.linspace(-6, 6, 97, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(LR.gelu_erf(z).sum(), z)
    _close(LR.dgelu_erf(z.detach()), g, "gelu'")
    _close(LR.gelu_erf(z.detach()), torch.nn.functional.gelu(z.detach()), "gelu")
