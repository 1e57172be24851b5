"""The kernels whose prologue requests its global operands ahead of the first wait -- the row images staged in two phases (csrc/common.hpp stage_issue /
stage_store: 4-wave attention backward, row-block backward), the attention forward's key-mask bytes and sprel words -- and their 8-wave twins, against
float64, at every row count where the staging takes another path (-m gpu):

  attention forward / backward (csrc/attention.hip attn_fwd_body, attn_bwd_body), B = 2 with 2 heads, Nq x Nk in SHAPES, each plain and with the key
      mask, dist + sprel, dropout, the seeded dP_init (backward), and all of them; fp16 and -- at 33 x 33 and 64 x 64 -- fp32 plain and with all;
      the pair forms with two problems of different padded size.  References and bounds: tests/_attn_ref64.py, through the helpers of
      tests/test_attn_fp64_gpu.py.
  row-block backward (csrc/encbwd.hip rowbwd_body), M in ROWS on 16-row and on 32-row tiles: the tail with kt 0 / 4 / 12, the short chain, given
      d_fo / d_fod; modes 1 and 2 (attention stage in front, lean and with a seeded dP_init) on samples of exactly 17, 36 and 80 rows -- all launched
      directly.  Reference: fp64 autograd over oracle/layer_ref.py's stages; bounds BWD_BOUNDS / BWD_COS of tests/test_encoder_fp64_gpu.py
      (per 16-row tile for row outputs, rel-L2 + cosine for the LayerNorm gradients).

Guard rows: in every case each row operand (q, k, v, dO, dP_init; dQKV, d_ao, y1, y2, z, d_fo, d_fod, rstd; qkv, P, O, d_ctx of the attention stage) is a view into a larger
buffer whose other rows hold NaN, and every output sits between NaN guard rows: a read outside the valid rows, or a pad row that was not zeroed,
shows up as NaN or as a miss of the fp64 bound; a write outside shows up in the guards.  (The stand-alone attention backward reads P from the forward's
output buffer, which sits between sentinel rows.)

32-row tiles are what magic_rowbwd takes when a launch has more rows than 16 x CUs: the small problem is then the SECOND segment of a launch
whose first segment is a filler of 16 x CUs + 1 rows (zeros; not checked)."""
from types import SimpleNamespace

import pytest
import torch

import magic_amd  # noqa: F401
import oracle.layer_ref as LR
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from tests import _attn_ref64 as R
from tests import test_attn_fp64_gpu as A
from tests import test_encoder_fp64_gpu as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
G = 3                       # NaN guard rows on either side of every row operand


@pytest.fixture(autouse=True)
def exact_f32():
    prev = L.set_f32_mfma("exact")
    yield
    L.set_f32_mfma(prev)


def nan_rows(t):
    """the [rows, cols] tensor as a view into a device buffer with G rows of NaN before and after it"""
    buf = torch.full((t.shape[0] + 2 * G, t.shape[1]), NAN, dtype=t.dtype, device=DEV)
    buf[G:-G] = t.to(DEV)
    return buf[G:-G]


# ---- attention ------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (16, 17), (33, 33), (36, 38), (64, 64), (65, 80), (80, 80), (96, 97), (128, 128)]
OPTS = {"plain": {}, "mask": dict(mask=True), "dist": dict(dist=True), "drop": dict(p=0.1), "init": dict(init=True),
        "all": dict(mask=True, dist=True, p=0.1, init=True)}


def attn_case(Nq, Nk, opt, cross):
    kern = "bwd8" if R.bwd_waves8(Nq, Nk) else "bwd4"
    return R.C(kern, Nq, Nk, [], B=2, nh=2, cross=cross, **{"mask": False, **OPTS[opt]}, tag=opt)


def attn_params():
    out = []
    for i, (Nq, Nk) in enumerate(SHAPES):
        for opt in OPTS:
            out.append((attn_case(Nq, Nk, opt, cross=bool(i & 1)), "bf16"))
        for opt in ("plain", "all"):
            out.append((attn_case(Nq, Nk, opt, cross=not (i & 1)), "fp16"))
    for Nq, Nk in ((33, 33), (64, 64)):
        for opt in ("plain", "all"):
            out.append((attn_case(Nq, Nk, opt, cross=Nq == 64), "fp32"))
    return out


ATTN = attn_params()


def guarded_inputs(c, dtype, o):
    """A.inputs with NaN guard rows around every buffer"""
    B, Nq, Nk, H = c.B, c.Nq, c.Nk, c.H
    if c.cross:
        q = nan_rows(o.q.reshape(B * Nq, H))
        kv = nan_rows(torch.cat([o.k.reshape(B * Nk, H), o.v.reshape(B * Nk, H)], 1))
        return SimpleNamespace(q=q, k=kv, v=kv[:, H:], ldq=H, ldkv=2 * H)
    qkv = torch.full((B * max(Nq, Nk), 3 * H), NAN, dtype=dtype)
    qkv[:B * Nq, :H] = o.q.reshape(B * Nq, H)
    qkv[:B * Nk, H:2 * H] = o.k.reshape(B * Nk, H)
    qkv[:B * Nk, 2 * H:] = o.v.reshape(B * Nk, H)
    qkv = nan_rows(qkv)
    return SimpleNamespace(q=qkv, k=qkv[:, H:], v=qkv[:, 2 * H:], ldq=3 * H, ldkv=3 * H)


def fwd_state(c, dt):
    f = A.prepare_fwd(c, dt)
    f.x = guarded_inputs(c, f.dtype, f.o)
    return f


def bwd_state(c, dt, f):
    s = A.prepare_bwd(c, dt, f)
    s.dO = nan_rows(f.o.dO.reshape(c.B * c.Nq, c.H))
    if f.o.dP_init is not None:
        s.dP_init = nan_rows(f.o.dP_init.reshape(-1, c.ldp))
    return s


@pytest.mark.parametrize("c,dt", ATTN, ids=[f"{dt}-{c.Nq}x{c.Nk}-{c.tag}" for c, dt in ATTN])
def test_attention_forward_and_backward(c, dt):
    assert dt in c.dtypes(), "the case table holds supported problems only"
    tag = f"{dt} {c.Nq}x{c.Nk} {c.tag}"
    f = fwd_state(c, dt)
    A.launch_fwd(f)
    A.verify_fwd(A.collect_fwd(f, tag), tag)
    s = bwd_state(c, dt, f)
    A.launch_bwd(s)
    A.verify_bwd(A.collect_bwd(s, tag), tag)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_attention_pair_forms(dt):
    """a panorama problem (pads to 64 x 64, 4 waves alone) and a text problem (96 x 96, 8 waves) in ONE forward and ONE backward launch"""
    cases = [attn_case(36, 38, "all", cross=True), attn_case(80, 80, "all", cross=False)]
    fs = [fwd_state(c, dt) for c in cases]
    with L.group():
        for f in fs:
            A.launch_fwd(f)
    for f in fs:
        tag = f"{dt} pair forward {f.c.Nq}x{f.c.Nk}"
        A.verify_fwd(A.collect_fwd(f, tag), tag)
    ss = [bwd_state(c, dt, f) for c, f in zip(cases, fs)]
    with L.group():
        for s in ss:
            A.launch_bwd(s)
    for s in ss:
        tag = f"{dt} pair backward {s.c.Nq}x{s.c.Nk}"
        A.verify_bwd(A.collect_bwd(s, tag), tag)


# ---- row-block backward, launched directly ----------------------------------------------------------------------------------------------------
H, I, EPS = E.H, E.I, E.EPS
ROWS = [1, 15, 16, 17, 31, 32, 33, 47]
FORMS = ["tail0", "tail4", "tail12", "short", "given"]
_W = {}
_FILLER = {}


def weights(dt):
    """one set of block weights per storage type: fp64 values of the stored 16-bit matrices, their transposes in fragment order, fp32 vectors"""
    if dt in _W:
        return _W[dt]
    dtype = E.DTYPES[dt]
    g = torch.Generator().manual_seed(11)
    w = SimpleNamespace()
    for name, shape in (("Wqkv", (3 * H, H)), ("Wq", (H, H)), ("Wo", (H, H)), ("W1", (I, H)), ("W2", (H, I))):
        m = (torch.randn(*shape, generator=g) * shape[1] ** -0.5).to(dtype)
        setattr(w, name, m.double())
        setattr(w, name + "T", O.pack_frag(m.t().contiguous().to(DEV)))
    for name, n, base in (("bo", H, 0.0), ("bi", I, 0.0), ("bo2", H, 0.0), ("g1", H, 1.0), ("be1", H, 0.0), ("g2", H, 1.0), ("be2", H, 0.0)):
        v = base + torch.randn(n, generator=g) * 0.1
        setattr(w, name, v.double())
        setattr(w, name + "_d", v.float().to(DEV))
    _W[dt] = w
    return w


def filler(dt):
    """a first segment of 16 x CUs + 1 rows of zeros in the given-d_fo form: it makes magic_rowbwd take 32-row tiles for the whole launch"""
    if dt not in _FILLER:
        dtype, w = E.DTYPES[dt], weights(dt)
        M = 16 * E.ncu() + 1
        z = lambda c, t=dtype: torch.zeros(M, c, dtype=t, device=DEV)      # noqa: E731
        rs = torch.zeros(M, device=DEV)
        _FILLER[dt] = dict(M=M, dfo_in=z(H), dfod_in=z(H), y2=z(H), rstd2=rs, g2=w.g2_d, b2=w.be2_d, z=z(I), W2T=w.W2T, W1T=w.W1T, y1=z(H), rstd1=rs,
                           g1=w.g1_d, b1=w.be1_d, WoT=w.WoT, dz=z(I), daod=z(H), dao=z(H), dctx=z(H), flops=0.0)
    return _FILLER[dt]


def rowblock_problem(M, form, dt, att=None):
    """(segment for O.rowbwd, {name: (kernel output [M, cols], fp64 reference)}, {name: (fp32 gradient vector, reference, bound class)}); form
    "mode1": the full chain behind the attention stage `att` (attention_stage), whose dQKV rows take the place of the tail's dQKV operand"""
    dtype, w = E.DTYPES[dt], weights(dt)
    g = torch.Generator().manual_seed(1000 * M + (FORMS + ["mode1"]).index(form))
    rnd = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(dtype)      # noqa: E731
    leaf = lambda t: t.double().requires_grad_(True)                           # noqa: E731
    x, ctx = rnd(M, H).double(), leaf(rnd(M, H))
    g1, be1, g2, be2 = leaf(w.g1), leaf(w.be1), leaf(w.g2), leaf(w.be2)
    a_pre = x + LR.linear(ctx, w.Wo, w.bo)
    a, rstd1 = LR.layer_norm(a_pre, g1, be1, EPS)
    z = LR.linear(a, w.W1, w.bi)
    gl = LR.gelu_erf(z)
    out_pre = a + LR.linear(gl, w.W2, w.bo2)
    out, rstd2 = LR.layer_norm(out_pre, g2, be2, EPS)
    new = lambda c: nan_rows(torch.full((M, c), NAN, dtype=dtype))             # noqa: E731
    vec = lambda: torch.zeros(H, device=DEV)                                   # noqa: E731
    rows32 = lambda t: nan_rows(t.detach().float().view(M, 1))[:, 0]          # noqa: E731
    seg = dict(M=M, WoT=w.WoT, flops=0.0)
    outs, vecs = {}, {}
    if form == "mode1":
        dx = att.dqkv @ w.Wqkv + att.dao.double()
        seg.update(mode=1, **att.fields, dfo=new(H), dfod=new(H), dctx=new(H), dg2=vec(), db2=vec())
        outs["dqkv_out"] = (att.fields["dqkv_out"], att.dqkv)
    elif form.startswith("tail") or form == "short":
        kt = 4 if form == "short" else int(form[4:])
        dao = rnd(M, H, k=0.1)
        if kt == 0:          # the top of a stack: dx is the plain gradient, passed as both operands (the engine does the same)
            dx = dao.double()
            top = nan_rows(dao)
            seg.update(kt=0, dqkv_n=top, dao_n=top, WqkvT_n=w.WoT)
        else:
            Wt, WtT = (w.Wq, w.WqT) if kt == 4 else (w.Wqkv, w.WqkvT)
            dq = rnd(M, 32 * kt, k=0.1)
            dx = dq.double() @ Wt + dao.double()
            seg.update(kt=kt, dqkv_n=nan_rows(dq), dao_n=nan_rows(dao), WqkvT_n=WtT)
        seg.update(dfo=new(H), dfod=new(H), dctx=new(H), dg2=vec(), db2=vec())
    if form == "short":      # tail -> LayerNorm backward (the attention-output norm in the role of the output norm) -> output projection
        gr = torch.autograd.grad((a * dx).sum(), [a_pre, ctx, g1, be1])
        seg.update(y2=nan_rows(a.detach().to(dtype)), rstd2=rows32(rstd1), g2=w.g1_d, b2=w.be1_d)
        outs = {"dfo": (seg["dfo"], gr[0]), "dfod": (seg["dfod"], gr[0]), "dctx": (seg["dctx"], gr[1])}
        vecs = {"dg2": (seg["dg2"], gr[2], "w"), "db2": (seg["db2"], gr[3], "b")}
        return seg, outs, vecs
    seg.update(y2=nan_rows(out.detach().to(dtype)), rstd2=rows32(rstd2), g2=w.g2_d, b2=w.be2_d, z=nan_rows(z.detach().to(dtype)), W2T=w.W2T, W1T=w.W1T,
               y1=nan_rows(a.detach().to(dtype)), rstd1=rows32(rstd1), g1=w.g1_d, b1=w.be1_d, dg1=vec(), db1=vec(),
               dz=new(I), daod=new(H), dao=new(H), dctx=seg["dctx"] if "dctx" in seg else new(H))
    if form == "given":
        dfo, dfod = rnd(M, H, k=0.1), rnd(M, H, k=0.1)
        seg.update(dfo_in=nan_rows(dfo), dfod_in=nan_rows(dfod))
        loss = ((gl @ w.W2.t()) * dfod.double()).sum() + (a * dfo.double()).sum()
        gr = torch.autograd.grad(loss, [z, a_pre, ctx, g1, be1])
        gz, gap, gctx, gg1, gb1 = gr
    else:
        gr = torch.autograd.grad((out * dx).sum(), [out_pre, z, a_pre, ctx, g1, be1, g2, be2])
        gop, gz, gap, gctx, gg1, gb1, gg2, gb2 = gr
        outs.update(dfo=(seg["dfo"], gop), dfod=(seg["dfod"], gop))
        vecs.update(dg2=(seg["dg2"], gg2, "w"), db2=(seg["db2"], gb2, "b"))
    outs.update(dz=(seg["dz"], gz), daod=(seg["daod"], gap), dao=(seg["dao"], gap), dctx=(seg["dctx"], gctx))
    vecs.update(dg1=(seg["dg1"], gg1, "w"), db1=(seg["db1"], gb1, "b"))
    return seg, outs, vecs


def guards_of(body):
    """the G NaN rows before and the G after a nan_rows view"""
    base = body._base
    return torch.cat([base[:G], base[-G:]])


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("rows", [16, 32])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M", ROWS)
def test_rowblock_backward_direct(M, form, rows, dt):
    seg, outs, vecs = rowblock_problem(M, form, dt)
    segs = [seg] if rows == 16 else [filler(dt), seg]
    assert int(L.load().magic_rowbwd_rows(sum(s["M"] for s in segs))) == rows
    O.rowbwd(segs, None, 0.0)
    O.flush_rbw_parts()
    torch.cuda.synchronize()
    check_rows(outs, vecs, M, dt, f"{dt} {form} M={M} on {rows}-row tiles")


# ---- row-block backward behind the attention stage (modes 1 and 2), launched directly ---------------------------------------------------------
NSAMP = 2


def attention_stage(N, with_dP, dt):
    """the attention backward of the block above for NSAMP samples of exactly N rows: the segment fields of modes 1 / 2 (every row operand between
    NaN guard rows), the fp64 dQKV [M, 3H] of tests/_attn_ref64.ref_backward on the stored P, and the residual d_ao of the tail"""
    dtype, w = E.DTYPES[dt], weights(dt)
    c = R.C("bwd8" if R.bwd_waves8(N, N) else "bwd4", N, N, [], B=NSAMP, nh=E.NH, cross=False, mask=False, init=with_dP, tag=f"stage{int(with_dP)}")
    o = R.operands(c, dtype)
    M, ldp = NSAMP * N, c.ldp
    P = torch.zeros(NSAMP, E.NH, N, ldp, dtype=dtype)
    P[..., :N] = R.ref_probs(c, o).to(dtype)
    ctx = LR.context(P[..., :N].double(), o.v.double(), E.NH).to(dtype)          # the stored forward output: the stage takes rowsum(P dP) = dO . O
    r = R.ref_backward(c, o, P[..., :N], None)
    g = torch.Generator().manual_seed(c.seed ^ 0xA0)
    dao = (torch.randn(M, H, generator=g) * 0.1).to(dtype)
    fields = dict(N=N, ldp=ldp, qkv_a=nan_rows(torch.cat([o.q, o.k, o.v], -1).reshape(M, 3 * H)), P_a=nan_rows(P.reshape(-1, ldp)),
                  o_a=nan_rows(ctx.reshape(M, H)), dctx_a=nan_rows(o.dO.reshape(M, H)),
                  dP_init=nan_rows(o.dP_init.reshape(-1, ldp)) if with_dP else None,
                  dqkv_out=nan_rows(torch.full((M, 3 * H), NAN, dtype=dtype)), site_attn=0, WqkvT_n=w.WqkvT, dao_n=nan_rows(dao))
    return SimpleNamespace(fields=fields, dqkv=torch.cat([r.dQ, r.dK, r.dV], -1).reshape(M, 3 * H), dao=dao, M=M)


def check_rows(outs, vecs, M, dt, tag):
    bound = E.BWD_BOUNDS[dt]
    for name, (k, ref) in outs.items():
        assert torch.isnan(guards_of(k)).all(), f"{tag} {name}: the kernel wrote outside its rows"
        kd = k.double().cpu()
        assert torch.isfinite(kd).all(), f"{tag} {name}: non-finite elements"
        for t0 in range(0, M, 16):
            r = ref[t0:t0 + 16]
            rel = ((kd[t0:t0 + 16] - r).norm() / r.norm()).item()
            assert rel < bound["dx"], f"{tag} {name} rows {t0}..: rel-L2 {rel:.3e} (bound {bound['dx']})"
    for name, (k, ref, cls) in vecs.items():
        rel, cos = E.rel_cos(k.cpu(), ref)
        assert rel < bound[cls] and cos > E.BWD_COS, f"{tag} {name}: rel-L2 {rel:.3e} (bound {bound[cls]}), cosine {cos:.6f}"


def attention_stage_problem(N, mode, with_dP, dt):
    att = attention_stage(N, with_dP, dt)
    if mode == 1:
        return rowblock_problem(att.M, "mode1", dt, att)
    w = weights(dt)
    dx0 = nan_rows(torch.full((att.M, H), NAN, dtype=E.DTYPES[dt]))
    seg = dict(M=att.M, mode=2, dfo=dx0, flops=0.0, **att.fields)
    return seg, {"dqkv_out": (att.fields["dqkv_out"], att.dqkv), "dx0": (dx0, att.dqkv @ w.Wqkv + att.dao.double())}, {}


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("with_dP", [False, True], ids=["lean", "dP_init"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("N", [17, 36, 80])
def test_rowblock_backward_behind_the_attention_stage(N, mode, with_dP, dt):
    """modes 1 (attention backward of the block above + the full chain) and 2 (+ dx0 = dQKV Wqkv + d_ao only) on samples of exactly 17, 36 and 80 rows
    (2, 3 and 5 tiles, the last with 1, 4 and 16 valid rows), in the lean kernel and in the full one (a gradient seeded into the attention map)"""
    seg, outs, vecs = attention_stage_problem(N, mode, with_dP, dt)
    assert seg["N"] == N and seg["M"] == NSAMP * N and seg["mode"] == mode
    O.rowbwd([seg], None, 0.0)
    O.flush_rbw_parts()
    torch.cuda.synchronize()
    check_rows(outs, vecs, seg["M"], dt, f"{dt} mode {mode} N={N} dP_init={with_dP}")
