"""Float64 reference of magic_kd_cols (csrc/loss.hip kd_cols_kernel / kd_cols_row_kernel) and of the N-d kd_loss above it.

Like tests/_loss_ref64.py: nothing here launches a kernel or rounds "the way the kernel would".  A reference takes the operands as stored (16-bit
inputs as they are, scalars as the fp32 the C ABI carries) and works in float64 from there; tests/test_kdcols_ref64_cpu.py shows it equal to the
reference's own kd_loss (tests/golden/makd_kl.pt), to oracle.makd_ref.kd_loss on 2-D input and to float64 autograd.

    x = (v == -inf ? -1e6 : v) / T,  p_t = softmax_c(x_t),  log p_s = log_softmax_c(x_s)            c = the MIDDLE axis of [outer, C, inner]
    loss = norm T^2 sum_o w[o] sum_{c,i} p_t (log p_t - log p_s)          (p_t == 0 adds 0)
    ds   = coef norm w[o] T (p_s - p_t)

Envelopes as _loss_ref64.kd_ref builds them: a KL column's is sum_c p_t (|log p_t| + |log p_s|) plus both log-sum-exps' own (|max| + |lse - max|);
a probability's is p (1 + |log p|)."""
import torch

from tests._loss_ref64 import REL, ULP, bound, check, f32  # noqa: F401  (re-exported: the GPU tests take the bound from here)

NEG = float("-inf")


def _clean(v, T):
    v = v.double()
    return torch.where(v == NEG, torch.full_like(v, -1e6), v) / T


def _lse1(x):
    """x float64 [outer, C, inner]: log-softmax over C, its lse envelope [outer, inner], p and p's envelope"""
    mx = x.max(1).values
    lse = torch.logsumexp(x, 1)
    z = x - lse[:, None]
    p = z.exp()
    return z, mx.abs() + (lse - mx).abs(), p, torch.where(p > 0, p * (1 + z.abs()), torch.zeros_like(p))


def kdcols_ref(s, t, T, w=None, norm=1.0, coef=0.0):
    """s, t [outer, C, inner] (the strided views the kernel walks).  dict: terms [outer, inner] (their sum is the loss; the kernel's partials
    add up to it), terms_env, grad [outer, C, inner] = coef norm w T (p_s - p_t), grad_env.  Scalars are used as given: a kernel test passes
    them through f32() first"""
    xs, xt = _clean(s, T), _clean(t, T)
    zs, senv, ps, psenv = _lse1(xs)
    zt, tenv, pt, ptenv = _lse1(xt)
    wo = (w.double() if w is not None else torch.ones(s.shape[0], dtype=torch.float64, device=s.device))[:, None]
    live = pt > 0
    kl = torch.where(live, pt * (zt - zs), torch.zeros_like(pt)).sum(1)
    kenv = torch.where(live, pt * (zt.abs() + zs.abs()), torch.zeros_like(pt)).sum(1) + senv + tenv
    k = norm * T * T
    g = coef * norm * T
    return dict(terms=k * wo * kl, terms_env=abs(k) * wo.abs() * kenv,
                grad=g * wo[:, :, None] * (ps - pt), grad_env=abs(g) * wo.abs()[:, :, None] * (psenv + ptenv))


def as3(x):
    """an N-d input of kd_loss (N >= 2) as [outer, C, inner]: dim 0, dim 1, everything behind"""
    return x.reshape(x.shape[0], x.shape[1], -1)


def kd_norm(shape, weighted, loss_type):
    """the reference's reduction as one factor: 'sum' -> 1; 'mean' -> 1 / numel without weights (KLDivLoss 'mean'), 1 / (numel / C) with them
    (the weighted branch sums over dim 1 first, then takes the mean over what remains)"""
    numel = 1
    for d in shape:
        numel *= d
    if loss_type == "sum":
        return 1.0
    return shape[1] / numel if weighted else 1.0 / numel


def kd_loss_ref(s, t, T=1.0, w=None, loss_type="sum", softmax_last=False, mean_by_numel=False):
    """map_nav_src/utils/kd_loss.py kd_loss on N-d input in float64, through kdcols_ref.  The two flags PLANT a defect (tests only): the softmax
    over the last axis instead of dim 1; the weighted mean divided by numel"""
    s3, t3 = as3(s), as3(t)
    if softmax_last:
        s3, t3 = (x.reshape(x.shape[0], -1, x.shape[-1]).transpose(1, 2) for x in (s, t))
    norm = kd_norm(tuple(s.shape), w is not None and not mean_by_numel, loss_type)
    return kdcols_ref(s3, t3, T, w, norm)["terms"].sum()


def kd_expr(s, t, T=1.0, w=None, loss_type="sum"):
    """the reference's expression, line by line, in whatever dtype it is given (autograd-able): the independent restatement kdcols_ref is held to"""
    s = torch.where(s == NEG, torch.full_like(s, -1e6), s)
    t = torch.where(t == NEG, torch.full_like(t, -1e6), t)
    pt = torch.softmax(t / T, dim=1)
    ls = torch.log_softmax(s / T, dim=1)
    kl = torch.where(pt > 0, pt * (pt.clamp_min(1e-300).log() - ls), torch.zeros_like(pt))
    if w is None:
        r = kl.sum() if loss_type == "sum" else kl.mean()
    else:
        row = kl.sum(1) * w.view(-1, *([1] * (kl.dim() - 2)))
        r = row.sum() if loss_type == "sum" else row.mean()
    return r * T ** 2


LOSS_KEYS = ("txt_emb_loss", "txt_attn_loss", "img_emb_loss", "avg_img_emb_loss", "img_attn_loss",
             "global_emb_loss", "global_attn_loss", "local_emb_loss", "local_attn_loss", "predict_loss")


def makd_kl_ref(t_step, s_out, t_out, heads, *, role="t2s", loss_type="sum", temperature=2.0, weights=None, feat_loss="mse", attn_loss="mse",
                global_local_T=1.0):
    """GMapNavAgent.compute_kd_losses (agent.py:546-719) of ONE step in float64 with the feature / attention terms 'mse' or 'kl'.  Temperature
    per term as the reference passes it: txt and img terms get `temperature` (:574-582, :610-631), global and local terms none, i.e. 1
    (:651-673); `global_local_T` = 2 PLANTS the defect of handing it to them too (tests only).  heads: name -> callable on float64"""
    loss_type = loss_type if role == "t2s" else "mean"
    w = t_out["sample_weights"].double()
    d = lambda x: x.double()
    hmin = min(s_out["txt_attns"].shape[1], t_out["txt_attns"].shape[1])
    k = (lambda i: float(weights[i])) if weights is not None else (lambda i: 1.0)
    half = 1.0 if weights is not None else 0.5

    def term(kind, a, b, T):
        if kind == "kl":
            return kd_loss_ref(a, b, T, w, loss_type)
        e = (a - b) ** 2 * w.view(-1, *([1] * (a.dim() - 1)))
        return e.sum() if loss_type == "sum" else e.mean()

    def feat(name, a, b, T):
        a, b = (heads[name](d(a)), d(b)) if role == "t2s" else (d(a), heads[name](d(b)))
        return term(feat_loss, a, b, T)

    def attn(a, b, T):
        return term(attn_loss, d(a), d(b), T)

    out = {}
    sn, tn = s_out["nav_outs"], t_out["nav_outs"]
    if t_step == 0:
        out["txt_emb_loss"] = feat("txt_emb_w", s_out["txt_embeds"], t_out["txt_embeds"], temperature) * k(0)
        out["txt_attn_loss"] = attn(s_out["txt_attns"][:, :hmin], t_out["txt_attns"][:, :hmin], temperature) * k(0)
    out["img_emb_loss"] = feat("kdl_img_w", s_out["pano_embeds"], t_out["pano_embeds"], temperature) * k(1) * half
    out["avg_img_emb_loss"] = feat("kdl_avg_img_w", s_out["pano_fused_embeds"], t_out["pano_fused_embeds"], temperature) * k(1) * half
    out["img_attn_loss"] = attn(s_out["img_attns"], t_out["img_attns"], temperature) * k(1)
    out["global_emb_loss"] = feat("global_cross_w", sn["gmap_embeds"], tn["gmap_embeds"], global_local_T) * k(2)
    out["global_attn_loss"] = attn(sn["gmap_attns"][:, :hmin], tn["gmap_attns"][:, :hmin], global_local_T) * k(2)
    out["local_emb_loss"] = feat("local_cross_w", sn["vp_embeds"], tn["vp_embeds"], global_local_T) * k(3)
    out["local_attn_loss"] = attn(sn["vp_attns"][:, :hmin], tn["vp_attns"][:, :hmin], global_local_T) * k(3)
    out["predict_loss"] = kd_loss_ref(d(s_out["nav_logits"]), d(t_out["nav_logits"]), temperature, w, loss_type) * k(4)
    return out
