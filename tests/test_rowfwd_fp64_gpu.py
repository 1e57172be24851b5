"""The row-wise forward kernels of csrc/rowops.hip and the gather / fusion glue of csrc/graphops.hip against float64, at every width and row
edge (-m gpu).

References, bounds, rule mirrors, emulation and the case table live in tests/_rowfwd_ref64.py; tests/test_rowfwd_ref64_cpu.py proves on these
very inputs that an honest fp32 / 16-bit emulation passes the bounds and that every planted defect fails them.

Every kernel is called through host/ops.py.  Every output buffer is NaN-filled before the launch (or holds the accumulate base) and sits
between two NaN guard rows that must come back untouched; the pad columns of the softmax inputs hold NaN too, so a kernel that reads past its
problem shows up.  The fused launches (node_in_fwd, embed_in_fwd, csr_gather_multi, the ln_fwd pair under L.group()) are checked against
float64 stage by stage AND bit for bit against the per-op launches they replace.

The kernels leave no trace of which branch ran: the branches a case is there for are inferred from the launch rules mirrored in
tests/_rowfwd_ref64.py (test_rule_mirrors_and_branch_coverage of the CPU file).  test_zz_report prints (with -s) the worst error / bound of
every kernel output and storage type this process measured: the figures in the docstring of tests/_rowfwd_ref64.py."""
import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from tests import _rowfwd_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
STATS = {}
F32 = torch.float32
_GUARDS, _KEEP = [], []
ids = lambda cs: [c.id for c in cs]


@pytest.fixture(autouse=True)
def fresh_buffers():
    _GUARDS.clear()
    _KEEP.clear()
    yield
    _GUARDS.clear()
    _KEEP.clear()


def alloc(shape, dtype, base=None):
    """a NaN-filled output of `shape` (or a copy of `base`) between two NaN guard rows"""
    cols = 1
    for s in shape[1:]:
        cols *= s
    buf = torch.full((shape[0] + 2, cols), NAN, dtype=dtype, device=DEV)
    _GUARDS.append(buf)
    body = buf[1:-1].view(shape)
    if base is not None:
        body.copy_(base.to(DEV))
    return body


def guards_untouched(tag):
    torch.cuda.synchronize()
    for i, buf in enumerate(_GUARDS):
        assert torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all(), f"{tag}: guard rows of output buffer {i} were written"


def dev(t):
    if t is None:
        return None
    t = t.to(DEV).contiguous()
    _KEEP.append(t)
    return t


def dev_csr(csr):
    return None if csr is None else tuple(dev(t) for t in csr)


def dev_tab(t):
    return None if t is None else (dev(t[0]), dev(t[1]), t[2], t[3])


def cpu(outs):
    return {k: v.cpu() for k, v in outs.items()}


def same_outs(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert R.same(a[k], b[k]), f"{tag} {k}: differs from the per-op launches"


# ---- launches ---------------------------------------------------------------------------------------------------------------------------------
def launch_ln(o, dtype, pre=""):
    out = alloc((o.M, o.H), dtype)
    rstd = alloc((o.M,), F32) if (o.do_ln and o.want_rstd) else None
    O.ln_fwd(o.M, o.H, out, in0=dev(o.in0), in1=dev(o.in1), tabs=[dev_tab(t) for t in o.tabs], gamma=dev(o.gamma), beta=dev(o.beta), eps=R.EPS,
             rstd=rstd, do_ln=o.do_ln)
    return {pre + "out": out, **({pre + "rstd": rstd} if rstd is not None else {})}


def launch_smallk(o, dtype, names=("out", "rstd")):
    out, rstd = alloc((o.M, o.H), dtype), alloc((o.M,), F32)
    O.smallk_ln_fwd(o.M, o.H, o.Kin, dev(o.x), dev(o.W), dev(o.b), dev(o.gamma), dev(o.beta), R.EPS, out, rstd)
    return {names[0]: out, names[1]: rstd}


def launch_gather(p, dtype, H):
    out = alloc((p.M, H), dtype, p.base)
    O.csr_gather(dev(p.src), *dev_csr(p.csr), out, p.M, H, accumulate=p.base is not None)
    if getattr(p, "csr2", None) is not None:
        O.csr_gather(dev(p.src2), *dev_csr(p.csr2), out, p.M, H, accumulate=True)
    return out


def node_problem(p, dtype, H):
    q = dict(M=p.M, Kin=p.Kin, x=dev(p.x), W=dev(p.W), b=dev(p.b), gamma=dev(p.gamma), beta=dev(p.beta), eps=R.EPS,
             A=alloc((p.M, H), dtype), rstd=alloc((p.M,), F32), out=alloc((p.M, H), dtype))
    if p.add0 is not None:
        q["add0"] = dev(p.add0)
    if p.csr1 is not None:
        q["src1"], q["csr1"] = dev(p.src1), dev_csr(p.csr1)
    if p.csr2 is not None:
        q["src2"], q["csr2"] = dev(p.src2), dev_csr(p.csr2)
    if p.tab is not None:
        q["tab"], q["tab_idx"] = dev(p.tab), dev(p.tab_idx)
    return q


def node_per_op(p, dtype, H):
    """csr_gather (+ accumulate) -> smallk_ln_fwd -> ln_fwd(do_ln = 0): the launches node_in_fwd replaces"""
    g = dev(p.add0)
    if p.csr1 is not None:
        g = launch_gather(R.SimpleNamespace(M=p.M, src=p.src1, csr=p.csr1, src2=p.src2, csr2=p.csr2, base=None), dtype, H)
    s = launch_smallk(p, dtype, names=("A", "rstd"))
    out = alloc((p.M, H), dtype)
    O.ln_fwd(p.M, H, out, in0=g, in1=s["A"], tabs=[(dev(p.tab), dev(p.tab_idx), 0, 0) if p.tab is not None else None, None, None], do_ln=False)
    return s["A"], s["rstd"], out


def text_kwargs(t, dtype):
    out, rstd = alloc((t.M, t.H), dtype), alloc((t.M,), F32)
    return dict(M=t.M, out=out, rstd=rstd, in0=dev(t.in0), in1=dev(t.in1), tabs=[dev_tab(x) for x in t.tabs], gamma=dev(t.gamma), beta=dev(t.beta), eps=R.EPS)


def launch(c, dt, o):
    """the case's kernel(s) through host/ops.py -> outputs by the names of R.verify (device tensors); fused launches also return the per-op result"""
    dtype, k = R.DTYPES[dt], c.kind
    per_op = None
    if k == "ln":
        outs = launch_ln(o, dtype)
    elif k == "smallk":
        outs = launch_smallk(o, dtype)
    elif k == "lndot":
        outs = {"logit": alloc((c.M,), F32)}
        O.lndot_fwd(dev(o.Y), c.M, c.H, dev(o.gamma), dev(o.beta), R.EPS, dev(o.w2), dev(o.b2), outs["logit"])
    elif k == "csr":
        outs = {"out": launch_gather(o, dtype, c.H)}
    elif k == "csrm":
        probs = []
        for p in o.probs:
            q = dict(out=alloc((p.M, c.H), dtype, p.base), n_out=p.M, src1=dev(p.src), csr1=dev_csr(p.csr), accumulate=p.base is not None)
            if p.csr2 is not None:
                q["src2"], q["csr2"] = dev(p.src2), dev_csr(p.csr2)
            probs.append(q)
        O.csr_gather_multi(c.H, probs)
        outs = {f"out{i}": q["out"] for i, q in enumerate(probs)}
        per_op = {f"out{i}": launch_gather(p, dtype, c.H) for i, p in enumerate(o.probs)}
    elif k == "softmax":
        B, nh, Nq, Nk, ldp = c.B, c.nh, c.Nq, c.Nk, c.ldp
        P, dS = alloc((B, nh, Nq, ldp), dtype), alloc((B, nh, Nq, ldp), dtype)
        km, dist, sw, sb = dev(o.kmask), dev(o.dist), dev(o.sw), dev(o.sb)
        O.softmax_fwd(dev(o.S), P, B, nh, Nq, Nk, ldp, R.SCALE, kmask=km, dist=dist, sprel_w=sw, sprel_b=sb)
        outs = {"P": P, "dS": dS}
        if dist is not None:
            outs["dsw"], outs["dsb"] = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        O.softmax_bwd(P, dev(o.dP), dS, B, nh, Nq, Nk, ldp, R.SCALE, dist=dist, dsprel_w=outs.get("dsw"), dsprel_b=outs.get("dsb"))
    elif k == "headmean":
        outs = {"out": alloc((c.B, c.inner), F32), "dP": alloc((c.B, c.nh, c.inner), F32, o.base)}
        O.head_mean_fwd(dev(o.P), outs["out"], c.B, c.nh, c.inner)
        O.head_mean_bwd(dev(o.g), outs["dP"], c.B, c.nh, c.inner, accumulate=o.base is not None)
    elif k == "pano":
        outs = {"fused": alloc((c.N, c.H), dtype), "probs": alloc((c.N, c.V), F32)}
        if o.P is not None:
            outs["pmean"] = alloc((c.N, o.inner), F32)
        O.pano_fuse_fwd(dev(o.x), dev(o.lens), dev(o.wf), dev(o.bf), outs["fused"], outs["probs"], c.N, c.V, c.H, P=dev(o.P), nh=o.nh if o.P is not None else 0,
                        inner=o.inner if o.P is not None else 0, pmean=outs.get("pmean"))
    elif k == "node_in":
        probs = [node_problem(p, dtype, c.H) for p in o.probs]
        O.node_in_fwd(c.H, probs)
        outs, per_op = {}, {}
        for i, (p, q) in enumerate(zip(o.probs, probs)):
            outs.update({f"A{i}": q["A"], f"rstd{i}": q["rstd"], f"out{i}": q["out"]})
            per_op[f"A{i}"], per_op[f"rstd{i}"], per_op[f"out{i}"] = node_per_op(p, dtype, c.H)
    elif k == "embed_in":
        M, H = c.M, c.H
        outs = {n: alloc((M, H), dtype) for n in ("A1", "A2", "X0")}
        outs.update({n: alloc((M,), F32) for n in ("rstd1", "rstd2", "rstd3")})
        pano = dict(M=M, Kin=c.Kin, eps=R.EPS, P0=dev(o.P0), g1=dev(o.g1), b1=dev(o.b1), loc=dev(o.x), W=dev(o.W), b=dev(o.b), g2=dev(o.gamma), b2=dev(o.beta),
                    nav_tab=dev(o.nav_tab), nav_idx=dev(o.nav_idx), tok_tab=dev(o.tok_tab), g3=dev(o.g3), b3=dev(o.b3), **outs)
        text = text_kwargs(o.text, dtype) if o.text is not None else None
        O.embed_in_fwd(H, pano, text)
        if text is not None:
            outs.update({"tout": text["out"], "trstd": text["rstd"]})
        # ln_fwd -> smallk_ln_fwd -> ln_fwd (+ the text ln_fwd): the launches embed_in_fwd replaces
        a1 = launch_ln(R.SimpleNamespace(M=M, H=H, in0=o.P0, in1=None, tabs=[None] * 3, gamma=o.g1, beta=o.b1, do_ln=True, want_rstd=True), dtype)
        a2 = launch_smallk(o, dtype)
        x0, r3 = alloc((M, H), dtype), alloc((M,), F32)
        O.ln_fwd(M, H, x0, in0=a1["out"], in1=a2["out"], tabs=[(pano["nav_tab"], pano["nav_idx"], 0, 0), (pano["tok_tab"], None, 0, 0), None],
                 gamma=pano["g3"], beta=pano["b3"], eps=R.EPS, rstd=r3)
        per_op = {"A1": a1["out"], "rstd1": a1["rstd"], "A2": a2["out"], "rstd2": a2["rstd"], "X0": x0, "rstd3": r3}
        if o.text is not None:
            per_op.update(launch_ln(o.text, dtype, pre="t"))
    else:
        raise KeyError(k)
    return outs, per_op


def run(c):
    for dt in R.DTYPES:
        tag = f"{dt} {c.id}"
        o = R.operands(c, dt)
        outs, per_op = launch(c, dt, o)
        guards_untouched(tag)
        outs = cpu(outs)
        R.verify(c, dt, o, outs, tag, STATS)
        if per_op is not None:
            same_outs(outs, cpu(per_op), tag)
        _GUARDS.clear()
        _KEEP.clear()


@pytest.mark.parametrize("c", R.CASES["ln"], ids=ids(R.CASES["ln"]))
def test_ln_fwd_matches_float64(c):
    run(c)


@pytest.mark.parametrize("pair", range(len(R.PAIRS)), ids=[f"{a.id}+{b.id}" for a, b in R.PAIRS])
def test_ln_fwd_pair_launch_matches_float64_and_the_single_launches(pair):
    a, b = R.PAIRS[pair]
    for dt in R.DTYPES:
        dtype = R.DTYPES[dt]
        oa, ob = R.operands(a, dt), R.operands(b, dt)
        single = [cpu(launch_ln(o, dtype)) for o in (oa, ob)]
        with L.group():
            both = [launch_ln(o, dtype) for o in (oa, ob)]
        guards_untouched(f"{dt} {a.id}+{b.id}")
        for c, o, got, one in zip((a, b), (oa, ob), both, single):
            tag = f"{dt} pair {c.id}"
            got = cpu(got)
            R.verify(c, dt, o, got, tag, STATS)
            assert got.keys() == one.keys() and all(R.same(got[k], one[k]) for k in got), f"{tag}: differs from the single launch"
        _GUARDS.clear()
        _KEEP.clear()


@pytest.mark.parametrize("c", R.CASES["smallk"], ids=ids(R.CASES["smallk"]))
def test_smallk_ln_fwd_matches_float64(c):
    run(c)


@pytest.mark.parametrize("c", R.CASES["lndot"], ids=ids(R.CASES["lndot"]))
def test_lndot_fwd_matches_float64(c):
    run(c)


@pytest.mark.parametrize("c", R.CASES["csr"], ids=ids(R.CASES["csr"]))
def test_csr_gather_matches_float64(c):
    run(c)


@pytest.mark.parametrize("c", R.CASES["csrm"], ids=ids(R.CASES["csrm"]))
def test_csr_gather_multi_matches_float64_and_the_sequential_launches(c):
    run(c)


@pytest.mark.parametrize("c", R.CASES["softmax"], ids=ids(R.CASES["softmax"]))
def test_softmax_fwd_bwd_match_float64(c):
    run(c)


@pytest.mark.parametrize("c", R.CASES["headmean"], ids=ids(R.CASES["headmean"]))
def test_head_mean_fwd_bwd_match_float64(c):
    run(c)


@pytest.mark.parametrize("c", R.CASES["pano"], ids=ids(R.CASES["pano"]))
def test_pano_fuse_fwd_register_form_matches_float64(c):
    run(c)


@pytest.mark.parametrize("c", R.CASES["node_in"], ids=ids(R.CASES["node_in"]))
def test_node_in_fwd_matches_float64_and_the_per_op_launches(c):
    run(c)


@pytest.mark.parametrize("c", R.CASES["embed_in"], ids=ids(R.CASES["embed_in"]))
def test_embed_in_fwd_matches_float64_and_the_per_op_launches(c):
    run(c)


def test_row_forward_launches_refuse_what_they_cannot_serve():
    """unsupported widths, Kin, Nk, ldp, V and operand sets raise and write nothing"""
    dtype = torch.bfloat16
    outs = []

    def nan(*shape, dt=dtype):
        outs.append(torch.full(shape, NAN, dtype=dt, device=DEV))
        return outs[-1]

    def refused(fn, *a, **kw):
        with pytest.raises(L.MagicHipError):
            fn(*a, **kw)

    def smallk_args(M, H, Kin):
        kk = max(Kin, 1)
        return dict(x=torch.zeros(M, kk, device=DEV), W=torch.zeros(H, kk, device=DEV), b=torch.zeros(H, device=DEV), gamma=torch.ones(H, device=DEV),
                    beta=torch.zeros(H, device=DEV))

    def node(M, H, Kin, **kw):
        return dict(M=M, Kin=Kin, eps=R.EPS, A=nan(M, H), rstd=nan(M, dt=F32), out=nan(M, H), **smallk_args(M, H, Kin), **kw)

    def pano(M, H, Kin):
        s = smallk_args(M, H, Kin)
        one, zero = torch.ones(H, device=DEV), torch.zeros(H, device=DEV)
        return dict(M=M, Kin=Kin, eps=R.EPS, P0=torch.zeros(M, H, dtype=dtype, device=DEV), g1=one, b1=zero, A1=nan(M, H), rstd1=nan(M, dt=F32), loc=s["x"], W=s["W"],
                    b=s["b"], g2=one, b2=zero, A2=nan(M, H), rstd2=nan(M, dt=F32), nav_tab=torch.zeros(3, H, dtype=dtype, device=DEV),
                    nav_idx=torch.zeros(M, dtype=torch.int32, device=DEV), tok_tab=torch.zeros(2, H, dtype=dtype, device=DEV), g3=one, b3=zero, X0=nan(M, H),
                    rstd3=nan(M, dt=F32))

    M = 5
    for H, Kin in ((64, 7), (512, 7), (896, 7), (128, 0), (128, 17)):
        s = smallk_args(M, H, Kin)
        refused(O.smallk_ln_fwd, M, H, Kin, s["x"], s["W"], s["b"], s["gamma"], s["beta"], R.EPS, nan(M, H), nan(M, dt=F32))
        refused(O.node_in_fwd, H, [node(M, H, Kin)])
        refused(O.embed_in_fwd, H, pano(M, H, Kin))
        if Kin == 7:
            x = torch.zeros(M, H, dtype=dtype, device=DEV)
            refused(O.ln_fwd, M, H, nan(M, H), in0=x, gamma=s["gamma"], beta=s["beta"], rstd=nan(M, dt=F32))
            refused(O.lndot_fwd, x, M, H, s["gamma"], s["beta"], R.EPS, s["b"], torch.zeros(1, device=DEV), nan(M, dt=F32))
    for Nk, ldp in ((513, 520), (20, 16)):
        S = torch.zeros(6, 520, device=DEV)
        refused(O.softmax_fwd, S, nan(6, 520), 1, 2, 3, Nk, ldp, R.SCALE)
        refused(O.softmax_bwd, torch.zeros(6, 520, dtype=dtype, device=DEV), S, nan(6, 520), 1, 2, 3, Nk, ldp, R.SCALE)
    N, V, H = 2, 65, 128
    refused(O.pano_fuse_fwd, torch.zeros(N, V, H, dtype=dtype, device=DEV), torch.ones(N, dtype=torch.int32, device=DEV), torch.zeros(H, device=DEV),
            torch.zeros(1, device=DEV), nan(N, H), nan(N, V, dt=F32), N, V, H)
    ptr, idx = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    src = torch.zeros(2, 128, dtype=dtype, device=DEV)
    refused(O.csr_gather, src, ptr, idx, None, nan(2, 128), 2, 127)
    refused(O.csr_gather_multi, 127, [dict(out=nan(2, 128), n_out=2, src1=src, csr1=(ptr, idx, None))])
    refused(O.node_in_fwd, 128, [node(2, 128, 7, src2=src, csr2=(ptr, idx, None))])
    torch.cuda.synchronize()
    for i, t in enumerate(outs):
        assert torch.isnan(t).all(), f"refused launch wrote output {i}"


def test_zz_report():
    """prints (with -s) the worst error / bound per kernel output and storage type that this process measured"""
    for key in sorted(STATS):
        print(f"fp64 rowfwd {key[0]:9s} {key[1]:9s} {key[2]:5s} worst err / bound {STATS[key]:8.4f}")
    assert all(v <= 1.0 for v in STATS.values())
