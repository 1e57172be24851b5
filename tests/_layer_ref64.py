"""fp64 layer harness shared by tests/test_encoder_fp64_gpu.py (the fused H = 128 forms) and tests/test_layer_fp64_gpu.py (the per-op layer
path of host/engine.py at every width): storage ulps, the per-element stage check, the engine's saved tensors and weights in the shape the
checks read, and fp64 autograd over chained oracle/layer_ref.py stages as the backward reference.  Nothing here is tied to a width: H, NH and
I are arguments.  Importing this module needs no GPU; only the functions that replay the engine's own dropout masks (`_masks`) launch a kernel.

Forward bound, per element, of a tensor that carries ONE rounding from its fp32 result (each stage is recomputed from the kernel's own saved
16-bit inputs):

    |k - ref| <= c * ulp(|ref|) + extra + floor * ulp(rms of the ref's row)

ulp = the storage type's unit in the last place.  `extra` is the part the kernel does not round from the saved input: g = gelu(z) is taken
from the fp32 z, not from the saved 16-bit z (|gelu'(z)| * ulp(z) / 2), and gelu_fast replaces erf by Abramowitz & Stegun 7.1.26 (its
error, evaluated here in fp64, plus fp32 slack).  The floor covers fp32 accumulation and LayerNorm cancellation.

Backward reference (`stack_reference`, `cross_stack_reference`): the stages chained in fp64 from the stack's saved input, with the 16-bit
shadow weights upcast, the fp32 biases / LayerNorm parameters, the engine's own dropout masks, the same d_top and the same dP_init on the top
block's exposed (dropped) attention map.  Parameter gradients are compared by rel-L2 and cosine per tensor, gradients wrt rows (stack input,
context rows, K/V rows) per (sample, 16-row tile): one wrong tile cannot hide in a batch norm."""
import math
from types import SimpleNamespace

import torch

import oracle.layer_ref as LR

EPS, SCALE = 1e-12, 0.125
MEASURE = False                 # True: record and print the worst error of every stage, assert nothing (how the bounds were set)

# (c ulps of |ref|, floor in ulps of the row's rms) per stage.  Measured on MI355X over every case of test_encoder_fp64_gpu.py (H = 128;
# test_zz_report, -s), bf16 / fp16: worst |k - ref| / ulp(|ref|) where |ref| >= the row's rms, and the floor an element needed beyond c ulps:
#   qkv 0.5000 / 0.5005, floor 0 / 0          q 0.5000 / 0.5003, floor 0 / 0.0001      kv 0.5000 / 0.5003, floor 0 / 0.0002
#   z   0.5001 / 0.5006, floor 0 / 0.0003     P, Pc, Pd, Pdc <= 0.5000 / 0.5004, floor 0 / 0
#   ctx, cctx 0.5000 / 0.5003, floor 0 / 0    a, c 0.5000 / 0.5003, floor 0 / 0.0001   out 0.5001 / 0.5005, floor 0.0001 / 0.0009
#   g (with the gelu input term and gelu_fast's own error in `extra`) 1.57 / 1.59 ulp, floor 0 / 0
# Every stage is correctly rounded from its fp32 result: c = 1 ulp is 2x the worst, the floor 0.003 row-rms ulp ~3x the worst fp16 floor.
# gelu_fast alone against erf, in ulps of g: up to 0.96 (fp16) on the negative tail z < -3, where |g| < 4e-3; bf16's 1.9 sits at
# |g| < 1e-6, where bf16 keeps normal numbers.  In absolute terms it is <= 2.2e-7, under 1e-3 of an fp16 ulp of a row's rms.
BOUNDS = {k: (1.0, 0.003) for k in ("qkv", "q", "kv", "z", "P", "Pc", "Pd", "Pdc", "ctx", "cctx", "a", "c", "out", "g")}
RSTD_REL = 4e-7                 # measured worst 1.55e-7 (rstd_a), 1.42e-7 (rstd_c), 1.54e-7 (rstd_o)
STATS = {}
STAT_PREFIX = [""]              # put in front of every STATS name (tests/test_layer_fp64_gpu.py records per width)

# Row-block backward at H = 128, measured worst on MI355X over test_encoder_fp64_gpu.BWD_CASES at p 0 and 0.1 (bf16 / fp16), bound ~2.5x:
#   weights / gammas rel-L2 1.08e-2 / 1.27e-3     biases / betas (cancellation class) 1.32e-2 / 1.48e-3     input gradient per tile 4.7e-3 / 5.8e-4
BWD_BOUNDS = {"bf16": {"w": 2.7e-2, "b": 3.3e-2, "dx": 1.2e-2}, "fp16": {"w": 3.2e-3, "b": 3.7e-3, "dx": 1.5e-3}}
BWD_COS = 0.999


# ---- storage ulps ------------------------------------------------------------------------------------------------------------------
def ulp(x, dtype):
    """unit in the last place of |x| in the storage type (subnormals: the smallest normal's)"""
    mant, emin = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}[dtype]
    _, e = torch.frexp(x.abs().clamp_min(1e-300))
    return torch.ldexp(torch.ones_like(x), (e - 1).clamp_min(emin) - mant)


def gelu_as(z):
    """gelu_fast (csrc/enc_common.hpp) evaluated in fp64: erf from Abramowitz & Stegun 7.1.26"""
    ax = z.abs() / math.sqrt(2.0)
    t = 1.0 / (1.0 + 0.3275911 * ax)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    e = 1.0 - poly * torch.exp(-ax * ax)
    return 0.5 * z * (1.0 + torch.where(z < 0, -e, e))


def check(name, k, ref, dtype, tag, extra=None, bounds=None):
    """per-element bound of the module docstring over the last dimension's rows; records the measured worst into STATS"""
    c, floor = (bounds or BOUNDS)[name]
    k = k.double()
    assert torch.isfinite(k).all(), f"{tag} {name}: non-finite elements where the kernel writes"
    d = (k - ref).abs()
    rms = ref.pow(2).mean(-1, keepdim=True).sqrt()
    ue, ur = ulp(ref, dtype), ulp(rms, dtype).expand_as(ref)
    allow = c * ue + (0.0 if extra is None else extra)
    need = ((d - allow).clamp_min(0) / ur).max().item()
    big = ref.abs() >= rms
    ulps = (d / ue)[big].max().item() if big.any() else 0.0
    key = (str(dtype).replace("torch.", ""), STAT_PREFIX[0] + name)
    old = STATS.get(key, (0.0, 0.0))
    STATS[key] = (max(old[0], ulps), max(old[1], need))
    if MEASURE:
        return
    bad = d > allow + floor * ur
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{tag} {name}: {int(bad.sum())} of {bad.numel()} elements beyond {c} ulp + {floor} row-rms ulp; first at {i}: "
                             f"kernel {k[tuple(i)].item():.6g} ref {ref[tuple(i)].item():.6g} (floor needed {need:.3f}, worst {ulps:.2f} ulp)")


def check_rstd(name, k, ref, tag, rel_bound=None, extra=None, store=None):
    """relative error of the fp32 statistics; extra: per-row relative allowance (ln_input_rounding); store: the storage type's name, kept apart in
    STATS when the allowance depends on it"""
    k = k.double()
    assert torch.isfinite(k).all(), f"{tag} {name}: non-finite"
    rel = (k - ref).abs() / ref
    need = (rel - (0.0 if extra is None else extra)).max().item()
    key = ("fp32", STAT_PREFIX[0] + name + (f" ({store})" if store else ""))
    old = STATS.get(key, (0.0, 0.0))
    STATS[key] = (max(old[0], rel.max().item()), max(old[1], need / RSTD_REL))
    if not MEASURE:
        assert need < (rel_bound or RSTD_REL), f"{tag} {name}: relative error {rel.max().item():.3e} ({need:.3e} beyond the input rounding's share)"


def ln_input_rounding(res, h, W, b, gamma, eps, keep, dtype):
    """What a dense + add + LayerNorm stage may differ by when the dense output is STORED in `dtype` before the LayerNorm reads it (the
    unfused forms of MagicNet._dense_add_ln: linear_fwd + ln_fwd) -- a second rounding, in front of the LayerNorm, that the one-rounding bound
    of `check` does not cover.  v = res + keep (h W^T + b); the stored tensor is the dense output (dropout form) or the sum v (residual form,
    keep None), each within D = half a storage ulp of its fp64 value.  To first order, with xhat = (v - mean) rstd:
        |d out_i| <= |gamma_i| rstd (D_i + mean D + |xhat_i| mean(|xhat| D))          |d rstd| / rstd <= rstd mean(|xhat| D)
    Returns (allowance on the output [.., H], relative allowance on rstd [..])."""
    dense = LR.linear(h, W, b)
    v = res + (dense if keep is None else dense * keep)
    D = 0.5 * ulp(v, dtype) if keep is None else 0.5 * ulp(dense, dtype) * keep
    mu = v.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mu) ** 2).mean(-1, keepdim=True) + eps)
    xhat = ((v - mu) * rstd).abs()
    cross = (xhat * D).mean(-1, keepdim=True)
    return gamma.abs() * rstd * (D + D.mean(-1, keepdim=True) + xhat * cross), (rstd * cross).squeeze(-1)


def check_gelu(k, z, dtype, tag, bounds=None):
    """g = gelu_fast(z32) rounded: against gelu_erf(z16) with the input term |gelu'| ulp(z) / 2 and gelu_fast's own error (fp64 A&S + fp32 slack)"""
    ref = LR.gelu_erf(z)
    extra = LR.dgelu_erf(z).abs() * ulp(z, dtype) / 2 + (gelu_as(z) - ref).abs() + z.abs() * 2.0 ** -21
    check("g", k, ref, dtype, tag, extra=extra, bounds=bounds)
    # how far gelu_fast alone is from erf, in storage ulps of g (the fp16 question of the erf shortcut)
    r = ((gelu_as(z) - ref).abs() / ulp(ref, dtype)).max().item()
    key = (str(dtype).replace("torch.", ""), STAT_PREFIX[0] + "gelu_fast_vs_erf_ulps")
    STATS[key] = (max(STATS.get(key, (0.0, 0.0))[0], r), 0.0)


# ---- per-stage references ------------------------------------------------------------------------------------------------------------
def _masks(sg, sites, p, seed, cross, H, NH):
    """the engine's own dropout masks (scaled by 1 / (1 - p)) of one layer, under layer_ref's names"""
    if p == 0:
        return {}
    from tests.test_dropout_gpu import export_mask
    ns, N = sg.ns, sg.N

    def m(s, shape):
        return export_mask(seed, p, s, shape).double().cpu()
    r = {"attn": m(sites["site_attn"], (ns, NH, N, N)), "ao": m(sites["site_ao"], (sg.M, H)).view(ns, N, H),
         "out": m(sites["site_out"], (sg.M, H)).view(ns, N, H)}
    if cross:
        r["cattn"] = m(sites["site_cattn"], (ns, NH, N, sg.Nk))
        r["co"] = m(sites["site_co"], (sg.M, H)).view(ns, N, H)
    return r


def _probs_check(name, Pk, ref, n, dtype, tag, bounds=None):
    """pad columns exactly 0, the logical block against ref"""
    assert torch.isfinite(Pk).all(), f"{tag} {name}: non-finite (incl. pad columns)"
    assert (Pk[..., n:] == 0).all(), f"{tag} {name}: pad columns not zero"
    check(name, Pk[..., :n], ref, dtype, tag, bounds=bounds)


def check_segment(sg, p, seed, tag, H, NH, I, bounds=None, rstd_rel=None, stored_dense=None):
    """every saved tensor of every layer of one segment against its fp64 stage, from the kernel's own saved inputs.  stored_dense(K): True
    where the dense (K inputs) in front of a LayerNorm stores its output before the LayerNorm reads it (ln_input_rounding); None: nowhere"""
    dt, ns, N = sg.dtype, sg.ns, sg.N
    sname = str(dt).replace("torch.", "")

    def ln_extra(res, h, W, b, gamma, keep):
        if stored_dense is None or not stored_dense(W.shape[1]):
            return None, None
        return ln_input_rounding(res, h, W, b, gamma, EPS, keep, dt)
    x = sg.x.double().cpu().view(ns, N, H)
    if sg.cross:
        cx = sg.cx.double().cpu().view(ns, sg.Nk, H)
        dist = sg.dist.double().cpu() if sg.dist is not None else None
        sprel = (float(sg.sprel[0]), float(sg.sprel[1])) if sg.sprel else None
    for li, (w, _, o, sites) in enumerate(sg.layers):
        t = f"{tag} layer {li}"
        k = {n: v.double().cpu() for n, v in o.items() if v is not None}
        mk = _masks(sg, sites, p, seed, sg.cross, H, NH)
        qkv = k["qkv"].view(ns, N, 3 * H)
        check("qkv", qkv, LR.linear(x, w["Wqkv"], w["bqkv"]), dt, t, bounds=bounds)
        Pref = LR.probs(qkv[..., :H], qkv[..., H:2 * H], sg.kmask, NH, SCALE, dist=dist if sg.cross else None, sprel=sprel if sg.cross else None)
        Pk = k["P"].view(ns, NH, N, sg.ldp)
        _probs_check("P", Pk, Pref, N, dt, t, bounds)
        if p > 0:
            Pdk = k["Pd"].view(ns, NH, N, sg.ldp)
            _probs_check("Pd", Pdk, LR.dropped(Pref, mk["attn"]), N, dt, t, bounds)
        else:
            Pdk = Pk
        ctx = k["ctx"].view(ns, N, H)
        check("ctx", ctx, LR.context(Pdk[..., :N], qkv[..., 2 * H:], NH), dt, t, bounds=bounds)
        a = k["a"].view(ns, N, H)
        aref, ra = LR.dense_add_ln(x, ctx, w["Wo"], w["bo"], w["g1"], w["be1"], EPS, mk.get("ao"))
        ex, exr = ln_extra(x, ctx, w["Wo"], w["bo"], w["g1"], mk.get("ao"))
        check("a", a, aref, dt, t, extra=ex, bounds=bounds)
        check_rstd("rstd_a", k["rstd_a"].view(ns, N), ra, t, rstd_rel, exr, sname if stored_dense else None)
        f_in = a
        if sg.cross:
            q, kv = k["q"].view(ns, N, H), k["kv"].view(ns, sg.Nk, 2 * H)
            check("q", q, LR.linear(a, w["Wq"], w["bq"]), dt, t, bounds=bounds)
            check("kv", kv, LR.linear(cx, w["Wkv"], w["bkv"]), dt, t, bounds=bounds)
            Pcref = LR.probs(q, kv[..., :H], sg.cmask, NH, SCALE)
            Pck = k["Pc"].view(ns, NH, N, sg.ldpc)
            _probs_check("Pc", Pck, Pcref, sg.Nk, dt, t, bounds)
            if p > 0:
                Pdck = k["Pdc"].view(ns, NH, N, sg.ldpc)
                _probs_check("Pdc", Pdck, LR.dropped(Pcref, mk["cattn"]), sg.Nk, dt, t, bounds)
            else:
                Pdck = Pck
            cctx = k["cctx"].view(ns, N, H)
            check("cctx", cctx, LR.context(Pdck[..., :sg.Nk], kv[..., H:], NH), dt, t, bounds=bounds)
            c = k["c"].view(ns, N, H)
            cref, rc = LR.dense_add_ln(a, cctx, w["Woc"], w["boc"], w["gc"], w["bec"], EPS, mk.get("co"))
            ex, exr = ln_extra(a, cctx, w["Woc"], w["boc"], w["gc"], mk.get("co"))
            check("c", c, cref, dt, t, extra=ex, bounds=bounds)
            check_rstd("rstd_c", k["rstd_c"].view(ns, N), rc, t, rstd_rel, exr, sname if stored_dense else None)
            f_in = c
        z = k["z"].view(ns, N, I)
        check("z", z, LR.linear(f_in, w["W1"], w["bi"]), dt, t, bounds=bounds)
        g = k["g"].view(ns, N, I)
        check_gelu(g, z, dt, t, bounds)
        out = k["out"].view(ns, N, H)
        oref, ro = LR.dense_add_ln(f_in, g, w["W2"], w["bo2"], w["g2"], w["be2"], EPS, mk.get("out"))
        ex, exr = ln_extra(f_in, g, w["W2"], w["bo2"], w["g2"], mk.get("out"))
        check("out", out, oref, dt, t, extra=ex, bounds=bounds)
        check_rstd("rstd_o", k["rstd_o"].view(ns, N), ro, t, rstd_rel, exr, sname if stored_dense else None)
        x = out


# ---- the engine's weights and saved activations ----------------------------------------------------------------------------------------
def engine_layer(n, lp, H):
    """fp64 weights under layer_ref's names of one self-attention layer as the kernels read them (16-bit shadow matrices upcast, fp32 vectors)"""
    ql = n.lin(lp + "attention.self.query.weight", rows=3 * H, cols=H)
    o, f1, f2 = n.lin(lp + "attention.output.dense.weight"), n.lin(lp + "intermediate.dense.weight"), n.lin(lp + "output.dense.weight")
    n1, n2 = n.ln(lp + "attention.output.LayerNorm"), n.ln(lp + "output.LayerNorm")
    d = lambda t: t.detach().double().cpu().clone()        # noqa: E731
    w = {"Wqkv": d(ql.W), "bqkv": d(ql.b), "Wo": d(o.W), "bo": d(o.b), "g1": d(n1.g), "be1": d(n1.b),
         "W1": d(f1.W), "bi": d(f1.b), "W2": d(f2.W), "bo2": d(f2.b), "g2": d(n2.g), "be2": d(n2.b)}
    return w


def engine_cross_layer(n, lp, H):
    """engine_layer plus the cross-attention block of one co-attention layer: Wq, Wkv (key | value rows), Woc, gc, bec and their biases"""
    w = engine_layer(n, lp, H)
    q = n.lin(lp + "crossattention.self.query.weight")
    kv = n.lin(lp + "crossattention.self.key.weight", lp + "crossattention.self.key.bias", rows=2 * H, cols=H)
    o, nc = n.lin(lp + "crossattention.output.dense.weight"), n.ln(lp + "crossattention.output.LayerNorm")
    d = lambda t: t.detach().double().cpu().clone()        # noqa: E731
    w.update({"Wq": d(q.W), "bq": d(q.b), "Wkv": d(kv.W), "bkv": d(kv.b), "Woc": d(o.W), "boc": d(o.b), "gc": d(nc.g), "bec": d(nc.b)})
    return w


def engine_sites(n, lp, cross=False):
    from magic_amd.host.engine import MagicNet
    s = {"site_attn": MagicNet.site_id(lp + "attention.self.dropout"), "site_ao": MagicNet.site_id(lp + "attention.output.dropout"),
         "site_out": MagicNet.site_id(lp + "output.dropout")}
    if cross:
        s.update({"site_cattn": MagicNet.site_id(lp + "crossattention.self.dropout"),
                  "site_co": MagicNet.site_id(lp + "crossattention.output.dropout")})
    return s


def engine_segment(n, c, fmt, kmask, dtype, p, H):
    """the engine's saved forward of one self-attention stack in the shape check_segment reads"""
    l0 = c.layers[0].sa
    layers = []
    for j, lc in enumerate(c.layers):
        sa, ffn = lc.sa, lc.ffn
        o = dict(qkv=sa.qkv, P=sa.Ppre, Pd=sa.P if sa.adrop else None, ctx=sa.ctx, a=sa.a, rstd_a=sa.rstd_a, z=ffn.z, g=ffn.g, out=ffn.out,
                 rstd_o=ffn.rstd)
        layers.append((engine_layer(n, fmt.format(j), H), None, o, engine_sites(n, fmt.format(j))))
    return SimpleNamespace(dtype=dtype, ns=l0.Bn, N=l0.N, M=l0.Bn * l0.N, ldp=l0.ldp, x=l0.x, kmask=kmask.bool().cpu().view(l0.Bn, l0.N),
                           cross=False, layers=layers, nl=len(layers), p=p)


def engine_cross_segment(n, c, fmt, qmask, cmask, dtype, p, H, sprel=None):
    """the engine's saved forward of one co-attention encoder (MagicNet.cross_fwd's context) in the shape check_segment reads; sprel: the
    (weight, bias) scalars of the graph-distance bias when the context was built with `dist`"""
    l0 = c.layers[0]
    sa0 = l0.sa
    layers = []
    for j, lc in enumerate(c.layers):
        sa, ffn = lc.sa, lc.ffn
        o = dict(qkv=sa.qkv, P=sa.Ppre, Pd=sa.P if sa.adrop else None, ctx=sa.ctx, a=sa.a, rstd_a=sa.rstd_a,
                 q=lc.q, kv=lc.kv, Pc=lc.Ppre, Pdc=lc.P if lc.adrop else None, cctx=lc.cctx, c=lc.c, rstd_c=lc.rstd_c,
                 z=ffn.z, g=ffn.g, out=ffn.out, rstd_o=ffn.rstd)
        layers.append((engine_cross_layer(n, fmt.format(j), H), None, o, engine_sites(n, fmt.format(j), cross=True)))
    return SimpleNamespace(dtype=dtype, ns=sa0.Bn, N=sa0.N, M=sa0.Bn * sa0.N, ldp=sa0.ldp, x=sa0.x, kmask=qmask.bool().cpu().view(sa0.Bn, sa0.N),
                           cross=True, Nk=l0.Nk, ldpc=l0.ldp, cx=l0.ctx, cmask=cmask.bool().cpu().view(sa0.Bn, l0.Nk),
                           dist=c.dist, sprel=sprel if c.dist is not None else None, layers=layers, nl=len(layers), p=p)


# (store name suffix, layer_ref name, part of a fused span or None)
PNAMES = (("attention.self.query.weight", "Wqkv", 0), ("attention.self.key.weight", "Wqkv", 1), ("attention.self.value.weight", "Wqkv", 2),
          ("attention.self.query.bias", "bqkv", 0), ("attention.self.key.bias", "bqkv", 1), ("attention.self.value.bias", "bqkv", 2),
          ("attention.output.dense.weight", "Wo", None), ("attention.output.dense.bias", "bo", None),
          ("attention.output.LayerNorm.weight", "g1", None), ("attention.output.LayerNorm.bias", "be1", None),
          ("intermediate.dense.weight", "W1", None), ("intermediate.dense.bias", "bi", None),
          ("output.dense.weight", "W2", None), ("output.dense.bias", "bo2", None),
          ("output.LayerNorm.weight", "g2", None), ("output.LayerNorm.bias", "be2", None))
KV_PNAMES = (("crossattention.self.key.weight", "Wkv", 0), ("crossattention.self.value.weight", "Wkv", 1),
             ("crossattention.self.key.bias", "bkv", 0), ("crossattention.self.value.bias", "bkv", 1))
CROSS_PNAMES = PNAMES + (("crossattention.self.query.weight", "Wq", None), ("crossattention.self.query.bias", "bq", None)) + KV_PNAMES + \
    (("crossattention.output.dense.weight", "Woc", None), ("crossattention.output.dense.bias", "boc", None),
     ("crossattention.output.LayerNorm.weight", "gc", None), ("crossattention.output.LayerNorm.bias", "bec", None))


def stack_reference(sg, p, seed, d_top, dP, H, NH):
    """fp64 autograd of the chained stages: (d stack input [ns, N, H], {layer_ref name per layer: gradient})"""
    x0 = sg.x.double().cpu().view(sg.ns, sg.N, H).requires_grad_(True)
    ws = [{k: v.clone().requires_grad_(True) for k, v in w.items()} for w, _, _, _ in sg.layers]
    x, loss = x0, 0.0
    for (w, _, _, sites), wl in zip(sg.layers, ws):
        st = LR.self_layer(x, wl, sg.kmask, NH, EPS, _masks(sg, sites, p, seed, False, H, NH))
        x = st["out"]
    loss = (x * d_top.double().cpu().view_as(x)).sum()
    if dP is not None:
        loss = loss + (st["Pd"] * dP.double().cpu()[..., :sg.N]).sum()
    flat = [t for wl in ws for t in wl.values()]
    gr = torch.autograd.grad(loss, [x0] + flat)
    out, k = [], 1
    for wl in ws:
        out.append({name: gr[k + i] for i, name in enumerate(wl)})
        k += len(wl)
    return gr[0], out


def cross_stack_reference(x0, cx, ws, qmask, cmask, NH, d_top, masks=None, dist=None, sprel=None, dP=None, kv=None, d_ctx0=None, dkv0=None,
                          eps=EPS):
    """fp64 autograd over chained LR.cross_layer stages.  x0 [B, Nq, H] stack input, cx [B, Nk, H] context rows, ws: per-layer weights under
    layer_ref's names, masks: per-layer dropout masks (dicts, already scaled; None = no dropout), dist [B, Nq, Nq] and sprel = (weight, bias)
    of the graph-distance bias, dP [B, NH, Nq, >= Nk]: the seed on the TOP block's exposed (dropped) cross-attention map, d_top: the gradient
    wrt the stack's output.  kv: per-layer [B, Nk, 2H] key | value rows computed by the caller (the kv-given form: they are leaves here, their
    gradients come back as `dkv` and neither Wkv, bkv nor the context rows receive one); d_ctx0 / dkv0: what the context accumulator / the
    per-layer K/V accumulators held before the call (the results are added to them).
    Returns a namespace: dx, dctx (None in the kv-given form), grads (per layer: {layer_ref name: gradient}), dkv (per layer, or None),
    dsprel ((d weight, d bias), or None), top (the top layer's stages)."""
    d = lambda t: t.detach().double().clone()             # noqa: E731
    x0, cx = d(x0).requires_grad_(True), d(cx).requires_grad_(kv is None)
    ws = [{k: d(v).requires_grad_(True) for k, v in w.items()} for w in ws]
    kvs = [d(t).requires_grad_(True) for t in kv] if kv is not None else None
    sp = tuple(torch.as_tensor(float(s), dtype=torch.float64).requires_grad_(True) for s in sprel) if dist is not None else None
    dist = d(dist) if dist is not None else None
    x = x0
    for j, wl in enumerate(ws):
        st = LR.cross_layer(x, cx, wl, qmask, cmask, NH, eps, masks[j] if masks else None, dist=dist, sprel=sp,
                            kv=kvs[j] if kvs is not None else None)
        x = st["out"]
    loss = (x * d(d_top).view_as(x)).sum()
    if dP is not None:
        loss = loss + (st["Pdc"] * d(dP)[..., :cx.shape[1]]).sum()
    skip = ("Wkv", "bkv") if kvs is not None else ()
    wrt = [x0] + ([cx] if kvs is None else kvs) + (list(sp) if sp else []) + [t for wl in ws for k, t in wl.items() if k not in skip]
    gr = list(torch.autograd.grad(loss, wrt))
    r = SimpleNamespace(dx=gr.pop(0), dctx=None, dkv=None, dsprel=None, grads=[], top={k: v.detach() for k, v in st.items()})
    if kvs is None:
        r.dctx = gr.pop(0) + (0.0 if d_ctx0 is None else d(d_ctx0).view_as(cx))
    else:
        r.dkv = [gr.pop(0) + (0.0 if dkv0 is None else d(dkv0[j]).view_as(kvs[j])) for j in range(len(kvs))]
    if sp:
        r.dsprel = (gr.pop(0), gr.pop(0))
    for wl in ws:
        r.grads.append({k: gr.pop(0) for k in wl if k not in skip})
    assert not gr
    return r


def engine_cross_reference(sg, p, seed, d_top, H, NH, dP=None, kv_given=False, d_ctx0=None, dkv0=None, without=()):
    """cross_stack_reference fed from the engine's own saved forward (engine_cross_segment): its stack input and context rows, its weights,
    its dropout masks; kv_given: K/V are leaves equal to the engine's saved c.kv upcast.  without: mask names ('co', ...) or 'dP' to leave
    out -- the planted-defect tests use it to make a reference that is wrong in one known way."""
    masks = [_masks(sg, sites, p, seed, True, H, NH) for _, _, _, sites in sg.layers] if p > 0 else None
    if masks:
        masks = [{k: v for k, v in m.items() if k not in without} for m in masks]
    x0 = sg.x.double().cpu().view(sg.ns, sg.N, H)
    cx = sg.cx.double().cpu().view(sg.ns, sg.Nk, H)
    kv = [o["kv"].double().cpu().view(sg.ns, sg.Nk, 2 * H) for _, _, o, _ in sg.layers] if kv_given else None
    cpu = lambda t: None if t is None else t.double().cpu()             # noqa: E731
    return cross_stack_reference(x0, cx, [w for w, _, _, _ in sg.layers], sg.kmask, sg.cmask, NH, cpu(d_top), masks=masks,
                                 dist=cpu(sg.dist), sprel=sg.sprel, dP=None if "dP" in without else cpu(dP), kv=kv,
                                 d_ctx0=cpu(d_ctx0), dkv0=None if dkv0 is None else [cpu(t) for t in dkv0])


# ---- backward checks ---------------------------------------------------------------------------------------------------------------------
def rel_cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item(), torch.nn.functional.cosine_similarity(a, b, dim=0).item()


def check_param_grads(m, fmt, sg, ref, dtype, tag, H, grad=None, names=PNAMES, bounds=None, skip=()):
    """every parameter gradient of one stack against fp64 (rel-L2 and cosine; biases and betas are the cancellation class).  m: anything with
    a `.store` (offsets, flat gradient buffer); ref: per layer {layer_ref name: gradient}; skip: store-name suffixes the engine does not
    produce in this form (the K/V projection when its result is given)"""
    grad = m.store.grad if grad is None else grad
    b = (bounds or BWD_BOUNDS)[dtype]
    top = max(r.norm().item() for lr in ref for r in lr.values())
    for j, lr in enumerate(ref):
        for pn, rn, part in names:
            if pn in skip:
                continue
            nm = fmt.format(j) + pn
            off, cnt, _ = m.store.offsets[nm]
            k = grad[off:off + cnt].double().cpu()
            r = lr[rn]
            if part is not None:
                r = r.view(r.shape[0] // H, H, -1)[part].reshape(-1) if r.dim() == 2 else r.view(-1, H)[part]
            r = r.reshape(-1)
            cls = "b" if (pn.endswith("bias")) else "w"
            if pn.endswith("attention.self.key.bias"):   # analytically zero (a softmax is shift invariant): noise on both sides
                assert k.norm().item() < 1e-3 * top and r.norm().item() < 1e-6 * top, (tag, nm)
                continue
            rel, cos = rel_cos(k, r)
            key = (dtype, STAT_PREFIX[0] + "grad " + ("bias/beta" if cls == "b" else "weight/gamma"))
            STATS[key] = (max(STATS.get(key, (0.0, 0.0))[0], rel), 0.0)
            if not MEASURE:
                assert rel < b[cls] and cos > BWD_COS, f"{tag} {nm}: rel-L2 {rel:.3e} (bound {b[cls]}), cosine {cos:.6f}"


def check_dx_tiles(dx, ref, sg, dtype, tag, H, bounds=None, cls="dx", rows=None, what="d input"):
    """a gradient wrt rows per (sample, 16-row tile): one wrong tile cannot hide in the batch norm.  The stack input by default; rows / cls /
    what: the same check over `rows` rows per sample of another tensor (the context rows, a layer's K/V rows: ref's own width)"""
    N = sg.N if rows is None else rows
    k = dx.double().cpu().view(sg.ns, N, ref.shape[-1])
    ref = ref.view(sg.ns, N, -1)
    assert torch.isfinite(k).all(), f"{tag} {what}: non-finite"
    worst = 0.0
    for s in range(sg.ns):
        for t0 in range(0, N, 16):
            r = ref[s, t0:t0 + 16]
            if r.norm() == 0:
                continue
            rel = ((k[s, t0:t0 + 16] - r).norm() / r.norm()).item()
            worst = max(worst, rel)
            if not MEASURE:
                assert rel < (bounds or BWD_BOUNDS)[dtype][cls], f"{tag} {what} sample {s} rows {t0}..: rel-L2 {rel:.3e}"
    key = (dtype, STAT_PREFIX[0] + ("grad input per tile" if cls == "dx" else f"grad {what} per tile"))
    STATS[key] = (max(STATS.get(key, (0.0, 0.0))[0], worst), 0.0)
