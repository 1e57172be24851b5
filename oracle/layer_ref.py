"""ORACLE (test infrastructure, never shipped): one encoder layer restated stage by stage in fp64.

Each function takes explicit operands and computes ONE stage, in the order the whole-encoder kernels save them
(`magic_enc_layer` / `magic_xenc_layer`, csrc/encoder.hip):

  self block   qkv = x Wqkv^T + bqkv ; P = softmax(scale S + key bias [+ sprel_w dist + sprel_b]) ; Pd = P keep ; ctx = Pd V ;
               a = LN(x + drop(ctx Wo^T + bo)), rstd_a
  cross block  q = s Wq^T + bq ; kv = cx Wkv^T + bkv ; Pc ; Pdc ; cctx ; c = LN(s + drop(cctx Woc^T + boc)), rstd_c
  FFN          z = a W1^T + bi ; g = gelu_erf(z) ; out = LN(a + drop(g W2^T + bo2)), rstd_o

A test can feed every stage the kernel's own saved 16-bit inputs (so each compared tensor carries one rounding), or chain the
stages (`self_layer` / `cross_layer`), which tests/test_layer_ref_cpu.py ties to oracle.model_ref's RefSelfLayer / RefCrossLayer.
Dropout masks are arguments (already scaled by 1/(1-p), as tests.test_dropout_gpu.export_mask returns them); nothing is drawn here.
Shapes: activations [B, N, H], probabilities [B, heads, Nq, Nk], key masks [B, Nk] bool (True = valid), dist [B, Nq, Nk].
Every function is differentiable (fp64 autograd gives the reference backward).
"""
import math

import torch

NEG = -10000.0          # the additive key bias of a masked key (oracle.model_ref.NEG, the kernels' -10000.0f)
HEAD_DIM = 64

SELF_KEYS = ("Wqkv", "bqkv", "Wo", "bo", "g1", "be1")
CROSS_KEYS = ("Wq", "bq", "Wkv", "bkv", "Woc", "boc", "gc", "bec")
FFN_KEYS = ("W1", "bi", "W2", "bo2", "g2", "be2")


def linear(x, W, b):
    return x @ W.transpose(0, 1) + b


def gelu_erf(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def dgelu_erf(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _heads(t, nh):
    B, N, H = t.shape
    return t.reshape(B, N, nh, H // nh).transpose(1, 2)


def probs(q, k, kmask, nh, scale=None, dist=None, sprel=None):
    """P = softmax(scale q k^T + key bias [+ sprel_w dist + sprel_b]) per head; q [B, Nq, H], k [B, Nk, H]"""
    scale = 1.0 / math.sqrt(q.shape[-1] // nh) if scale is None else scale
    s = _heads(q, nh) @ _heads(k, nh).transpose(-1, -2) * scale
    s = s + ((~kmask.bool()).to(s.dtype) * NEG)[:, None, None, :]
    if dist is not None:
        s = s + (sprel[0] * dist + sprel[1])[:, None]
    return torch.softmax(s, dim=-1)


def dropped(P, keep=None):
    """Pd = P keep (keep = mask / (1 - p)); the identity without a mask"""
    return P if keep is None else P * keep


def context(Pd, v, nh):
    """ctx = Pd V, heads concatenated: [B, Nq, H]"""
    B, _, Nq, _ = Pd.shape
    return (Pd @ _heads(v, nh)).transpose(1, 2).reshape(B, Nq, v.shape[-1])


def layer_norm(v, gamma, beta, eps):
    """(LN(v), rstd) over the last dimension; rstd = 1 / sqrt(biased variance + eps)"""
    mu = v.mean(-1, keepdim=True)
    d = v - mu
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    return d * rstd * gamma + beta, rstd.squeeze(-1)


def dense_add_ln(res, h, W, b, gamma, beta, eps, keep=None):
    """LN(res + drop(h W^T + b)) and its rstd: the attention-output, cross-output and FFN-output stages"""
    y = linear(h, W, b)
    if keep is not None:
        y = y * keep
    return layer_norm(res + y, gamma, beta, eps)


def self_block(x, w, kmask, nh, eps, masks=None, dist=None, sprel=None, prefix=""):
    """the self-attention block's stages; w: Wqkv, bqkv, Wo, bo, g1, be1 (prefix + key); masks: dict with 'attn' [B, nh, N, N] and 'ao'
    [B, N, H] (either may be missing)"""
    masks = masks or {}
    H = x.shape[-1]
    st = {"qkv": linear(x, w[prefix + "Wqkv"], w[prefix + "bqkv"])}
    q, k, v = st["qkv"][..., :H], st["qkv"][..., H:2 * H], st["qkv"][..., 2 * H:]
    st["P"] = probs(q, k, kmask, nh, dist=dist, sprel=sprel)
    st["Pd"] = dropped(st["P"], masks.get("attn"))
    st["ctx"] = context(st["Pd"], v, nh)
    st["a"], st["rstd_a"] = dense_add_ln(x, st["ctx"], w[prefix + "Wo"], w[prefix + "bo"], w[prefix + "g1"], w[prefix + "be1"], eps, masks.get("ao"))
    return st


def cross_block(s, cx, w, cmask, nh, eps, masks=None, kv=None):
    """the cross-attention block's stages: queries from s, keys / values from the context cx; masks: 'cattn', 'co'; kv: the key | value
    projection of the context [B, Nk, 2H] when the caller computed it (the navigator's per-episode cache): cx, Wkv and bkv are then unused"""
    masks = masks or {}
    H = s.shape[-1]
    st = {"q": linear(s, w["Wq"], w["bq"]), "kv": linear(cx, w["Wkv"], w["bkv"]) if kv is None else kv}
    st["Pc"] = probs(st["q"], st["kv"][..., :H], cmask, nh)
    st["Pdc"] = dropped(st["Pc"], masks.get("cattn"))
    st["cctx"] = context(st["Pdc"], st["kv"][..., H:], nh)
    st["c"], st["rstd_c"] = dense_add_ln(s, st["cctx"], w["Woc"], w["boc"], w["gc"], w["bec"], eps, masks.get("co"))
    return st


def ffn_block(a, w, eps, masks=None):
    """z, g, out, rstd_o; masks: 'out'"""
    masks = masks or {}
    st = {"z": linear(a, w["W1"], w["bi"])}
    st["g"] = gelu_erf(st["z"])
    st["out"], st["rstd_o"] = dense_add_ln(a, st["g"], w["W2"], w["bo2"], w["g2"], w["be2"], eps, masks.get("out"))
    return st


def self_layer(x, w, kmask, nh, eps, masks=None, dist=None, sprel=None):
    """one post-LN self-attention layer (oracle.model_ref.RefSelfLayer): every stage, chained"""
    st = self_block(x, w, kmask, nh, eps, masks, dist, sprel)
    st.update(ffn_block(st["a"], w, eps, masks))
    return st


def cross_layer(x, cx, w, qmask, cmask, nh, eps, masks=None, dist=None, sprel=None, kv=None):
    """one METER cross layer (oracle.model_ref.RefCrossLayer): self-attention [+ distance bias] -> cross-attention -> FFN"""
    st = self_block(x, w, qmask, nh, eps, masks, dist, sprel)
    st.update(cross_block(st["a"], cx, w, cmask, nh, eps, masks, kv))
    st.update(ffn_block(st["c"], w, eps, masks))
    return st


def _lin(m):
    return m.weight.detach(), m.bias.detach()


def self_weights(layer):
    """RefSelfLayer / RefCrossLayer parameters under this file's names (Wqkv = query | key | value rows, as the engine packs them)"""
    at = layer.attention
    w = {"Wqkv": torch.cat([at.self.query.weight, at.self.key.weight, at.self.value.weight]).detach(),
         "bqkv": torch.cat([at.self.query.bias, at.self.key.bias, at.self.value.bias]).detach()}
    w["Wo"], w["bo"] = _lin(at.output.dense)
    w["g1"], w["be1"] = _lin(at.output.LayerNorm)
    w["W1"], w["bi"] = _lin(layer.intermediate.dense)
    w["W2"], w["bo2"] = _lin(layer.output.dense)
    w["g2"], w["be2"] = _lin(layer.output.LayerNorm)
    if hasattr(layer, "crossattention"):
        ca = layer.crossattention
        w["Wq"], w["bq"] = _lin(ca.self.query)
        w["Wkv"] = torch.cat([ca.self.key.weight, ca.self.value.weight]).detach()
        w["bkv"] = torch.cat([ca.self.key.bias, ca.self.value.bias]).detach()
        w["Woc"], w["boc"] = _lin(ca.output.dense)
        w["gc"], w["bec"] = _lin(ca.output.LayerNorm)
    return w
