"""The SAP action-logit fusion of csrc/graphops.hip -- magic_sap_fuse_fwd, magic_sap_fuse_loss, magic_sap_fuse_bwd -- against float64 at every loop
edge (-m gpu).

References, bounds and the case table: tests/_sapfuse_ref64.py (shown right on the CPU by tests/test_sapfuse_ref64_cpu.py).  Every case runs the three
kernels through host/ops.py: K on each side of the 64-lane wave and up to the 8-slot distillation ring's 512 (513 and 700 for the two kernels without
a K limit), Vp up to the 128-float LDS rows, both gate settings, [mem] or none, every label kind, every option set of the fused loss (gradient
buffers or none, w_out, kd_rows, kd_coef_dev, the dynamic loss scale), every non-empty subset of {dgl, dll, dfl} in the backward, a saturated gate,
and the hand-made rows the planners cannot write.  Every output buffer starts as NaN with a guard row before and behind it; inputs are compared with
their copies afterwards; stage 1 of the fused loss is torch.equal to the forward kernel; the separate launches the fused loss replaces pass the
identical float64 check (the calibration of stage 2) and agree with the fused launch at the tolerances of tests/test_kernels_gpu.py."""
import ctypes as C
import inspect

import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import heads
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from tests import _sapfuse_ref64 as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
INPUTS = ("g_raw", "l_raw", "fuse_raw", "gmask", "lmask", "fsrc", "bw", "glab", "llab", "t_fused")
LOSS_CASES = [c for c in S.CASES if c.loss]


@pytest.fixture(autouse=True)
def _no_seed_scale():
    O.seed_scale(None)
    yield
    O.seed_scale(None)


def dev(P):
    return {k: getattr(P, k).to(DEV).contiguous() for k in INPUTS}


def guarded(rows, *shape):
    """a NaN-filled buffer with one guard row before and one behind the part a kernel is handed"""
    buf = torch.full((rows + 2,) + shape, NAN, device=DEV)
    return buf, buf[1:rows + 1]


def guards_ok(*bufs):
    return all(bool(torch.isnan(b[0]).all() and torch.isnan(b[-1]).all()) for b in bufs)


def unchanged(P, D):
    return all(torch.equal(D[k].cpu(), getattr(P, k)) for k in INPUTS)


def fwd(P, D, gate):
    B, K, Vp = P.B, P.K, P.Vp
    bufs = [guarded(B, K), guarded(B, Vp), guarded(B, K)]
    (_, gl), (_, ll), (_, fl) = bufs
    O.sap_fuse_fwd(B, K, Vp, D["g_raw"], D["l_raw"], D["fuse_raw"], D["gmask"], D["lmask"], D["fsrc"], D["bw"], gate, gl, ll, fl)
    torch.cuda.synchronize()
    assert guards_ok(*(b for b, _ in bufs)), "sap_fuse_fwd wrote outside its rows"
    return gl, ll, fl


@pytest.mark.parametrize("c", S.CASES, ids=[c.name for c in S.CASES])
def test_forward_and_backward_match_float64_at_every_loop_edge(c):
    P = S.get(c)
    D = dev(P)
    B, K, Vp = P.B, P.K, P.Vp
    run = S.Run("sap")
    gl, ll, fl = fwd(P, D, c.gate)
    S.verify_stage1(run, c.name, P, c.gate, gl, ll, fl)
    full = S.upstream(P)
    for sub in S.SUBSETS:
        up = {k: full[k] for k in sub}
        upd = {k: v.to(DEV) for k, v in up.items()}
        bufs = [guarded(B, K), guarded(B, Vp), guarded(B)]
        (_, dg), (_, dl), (_, df) = bufs
        O.sap_fuse_bwd(B, K, Vp, D["g_raw"], D["l_raw"], D["fuse_raw"], D["gmask"], D["lmask"], D["fsrc"], D["bw"], c.gate,
                       upd.get("dgl"), upd.get("dll"), upd.get("dfl"), dg, dl, df)
        torch.cuda.synchronize()
        tag = f"{c.name} {'+'.join(sub)}"
        assert guards_ok(*(b for b, _ in bufs)), f"sap_fuse_bwd wrote outside its rows: {tag}"
        assert all(torch.equal(upd[k].cpu(), up[k]) for k in up), f"upstream gradients modified: {tag}"
        S.verify_bwd(run, tag, P, c.gate, up, dg, dl, df)
    if c.fuse is not None:                                 # the saturated gate: finite wherever the reference is, fw (1 - fw) -> 0 without NaN
        assert (df.cpu()[P.fuse_raw.abs() == 90.0] == 0).all()
    assert unchanged(P, D), "an input was modified"


def separate_launches(P, D, o, k, gl, ll, fl):
    """the launches magic_sap_fuse_loss replaces, from the SAME stored logits: three ce_rows, ce_rows(w_out) on the teacher, kd_rows accumulated into dfl"""
    B, K, Vp = P.B, P.K, P.Vp
    rows = torch.full((3, B), NAN, device=DEV)
    g = {n: torch.full((B, Vp if n == "dll" else K), NAN, device=DEV) if n in o.grads else None for n in ("dgl", "dll", "dfl")}
    O.ce_rows(gl, B, K, K, D["glab"], coef=k.coef, loss_row=rows[0], dlogits=g["dgl"], ldd=K)
    O.ce_rows(ll, B, Vp, Vp, D["llab"], coef=k.coef, loss_row=rows[1], dlogits=g["dll"], ldd=Vp)
    O.ce_rows(fl, B, K, K, D["glab"], coef=k.coef, loss_row=rows[2], dlogits=g["dfl"], ldd=K)
    got = dict(rows=rows, **{n: v for n, v in g.items() if v is not None})
    if o.w:
        got["w"] = torch.full((B,), NAN, device=DEV)
        O.ce_rows(D["t_fused"], B, K, K, D["glab"], w_out=got["w"], w_rate=k.rate)
    if o.kd:
        got["kd"] = torch.full((B,), NAN, device=DEV)
        O.kd_rows(fl, D["t_fused"], B, K, K, k.T, w=got.get("w"), norm=k.norm, coef=k.kd_coef, coef_dev=None if o.dev is None else torch.tensor([o.dev], device=DEV),
                  loss_row=got["kd"], ds=g["dfl"], accumulate=True)
    torch.cuda.synchronize()
    return got


def allclose(a, b, name, rtol, atol):
    a, b = a.float().cpu(), b.float().cpu()
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{name}: max|err|={(a - b).abs().max().item():.3e} (ref max {b.abs().max().item():.3e}) rtol={rtol} atol={atol}"


@pytest.mark.parametrize("c", LOSS_CASES, ids=[c.name for c in LOSS_CASES])
def test_fused_loss_matches_float64_with_every_option_set(c):
    P = S.get(c)
    D = dev(P)
    B, K, Vp = P.B, P.K, P.Vp
    gl0, ll0, fl0 = fwd(P, D, c.gate)
    run, sep = S.Run("sap"), S.Run("sap-separate")
    for od in S.opts_of(c):
        o = S.opt(od)
        k = S.constants(P, o)
        tag = f"{c.name} {o.name}"
        state = torch.tensor([o.scale, 1.0 / o.scale, 0.0, 0.0], device=DEV) if o.scale != 1.0 else None
        bufs = dict(gl=guarded(B, K), ll=guarded(B, Vp), fl=guarded(B, K), rows=guarded(3, B), dgl=guarded(B, K), dll=guarded(B, Vp), dfl=guarded(B, K),
                    w=guarded(B), kd=guarded(B))
        v = {n: view for n, (_, view) in bufs.items()}
        kdev = None if o.dev is None else torch.tensor([o.dev], device=DEV)
        try:
            O.seed_scale(state)
            O.sap_fuse_loss(B, K, Vp, D["g_raw"], D["l_raw"], D["fuse_raw"], D["gmask"], D["lmask"], D["fsrc"], D["bw"], c.gate, v["gl"], v["ll"], v["fl"],
                            D["glab"], D["llab"], k.coef, v["rows"], dgl=v["dgl"] if "dgl" in o.grads else None, dll=v["dll"] if "dll" in o.grads else None,
                            dfl=v["dfl"] if "dfl" in o.grads else None, t_fused=D["t_fused"] if (o.w or o.kd) else None, w_rate=k.rate,
                            w_out=v["w"] if o.w else None, T=k.T, kd_norm=k.norm, kd_coef=k.kd_coef, kd_coef_dev=kdev, kd_rows=v["kd"] if o.kd else None)
            torch.cuda.synchronize()
            ref = separate_launches(P, D, o, k, gl0, ll0, fl0)
        finally:
            O.seed_scale(None)
        assert guards_ok(*(b for b, _ in bufs.values())), f"sap_fuse_loss wrote outside its rows: {tag}"
        asked = set(o.grads) | {"gl", "ll", "fl", "rows"} | ({"w"} if o.w else set()) | ({"kd"} if o.kd else set())
        for n, (buf, _) in bufs.items():
            if n not in asked:
                assert torch.isnan(buf).all(), f"{tag}: {n} was not asked for and was written"
        for a, b, n in ((v["gl"], gl0, "gl"), (v["ll"], ll0, "ll"), (v["fl"], fl0, "fl")):       # stage 1: the forward kernel's arithmetic, element for element
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{tag}: {n} differs from magic_sap_fuse_fwd"
        got = {n: v[n] for n in asked if n not in ("gl", "ll", "fl")}
        S.verify_stage2(run, tag, P, o, v["gl"], v["ll"], v["fl"], got)
        S.verify_stage2(sep, tag, P, o, gl0, ll0, fl0, ref)                      # calibration: the pinned separate launches under the identical check
        allclose(got["rows"], ref["rows"], f"rows {tag}", 2e-6, 1e-7)
        for n in o.grads:                                                        # (the absolute term is in units of the gradient: it carries the loss scale)
            allclose(got[n], ref[n], f"{n} {tag}", 2e-5, 1e-8 * o.scale)
        if o.w:
            allclose(got["w"], ref["w"], f"w_out {tag}", 2e-6, 1e-7)
        if o.kd:
            allclose(got["kd"], ref["kd"], f"kd_rows {tag}", 2e-5, 1e-8)
    assert unchanged(P, D), "an input was modified"


# ------------------------------------------------------------------------------------------ refusals
def _zeros(B, K, Vp):
    """valid operands of any extent (every index 0, [stop] open): a launch that is NOT refused stays in bounds of these"""
    d = dict(g_raw=torch.zeros(B, K), l_raw=torch.zeros(B, Vp), fuse_raw=torch.zeros(B), gmask=torch.ones(B, K, dtype=torch.uint8),
             lmask=torch.ones(B, Vp, dtype=torch.uint8), fsrc=torch.zeros(B, K, dtype=torch.int32), bw=torch.zeros(B, Vp, dtype=torch.uint8),
             glab=torch.zeros(B, dtype=torch.int32), llab=torch.zeros(B, dtype=torch.int32), t_fused=torch.zeros(B, K))
    return {k: v.to(DEV) for k, v in d.items()}


def _outs(B, K, Vp):
    return dict(gl=torch.full((B, K), NAN, device=DEV), ll=torch.full((B, Vp), NAN, device=DEV), fl=torch.full((B, K), NAN, device=DEV),
                rows=torch.full((3, B), NAN, device=DEV), dgl=torch.full((B, K), NAN, device=DEV), dll=torch.full((B, Vp), NAN, device=DEV),
                dfl=torch.full((B, K), NAN, device=DEV), w=torch.full((B,), NAN, device=DEV), kd=torch.full((B,), NAN, device=DEV),
                dg=torch.full((B, K), NAN, device=DEV), dl=torch.full((B, Vp), NAN, device=DEV), df=torch.full((B,), NAN, device=DEV))


def _loss_struct(B, K, Vp, D, X, **over):
    """the parameter block host/ops.py sap_fuse_loss fills, with single fields overridden (None: a null pointer)"""
    p = L.SapLossParams()
    p.B, p.K, p.Vp, p.use_gate = B, K, Vp, 1
    ptr = dict(g_raw=D["g_raw"], l_raw=D["l_raw"], fuse_raw=D["fuse_raw"], gmask=D["gmask"], lmask=D["lmask"], fsrc=D["fsrc"], bwmask=D["bw"], gl=X["gl"], ll=X["ll"],
               fl=X["fl"], glab=D["glab"], llab=D["llab"], rows=X["rows"], dgl=X["dgl"], dll=X["dll"], dfl=X["dfl"], t_fused=D["t_fused"], w_out=X["w"],
               kd_coef_dev=None, kd_rows=X["kd"])
    sc = dict(ignore_index=-100, coef=0.1, w_rate=0.7, T=2.0, kd_norm=0.5, kd_coef=0.2)
    for key, val in over.items():
        (ptr if key in ptr else sc)[key] = val
    for key, t in ptr.items():
        setattr(p, key, L.P(t))
    for key, val in sc.items():
        setattr(p, key, val)
    return p


def _refused(fn):
    with pytest.raises(L.MagicHipError, match="MAGIC_ERR_ARG"):
        fn()


REQUIRED = ("g_raw", "l_raw", "fuse_raw", "gmask", "lmask", "fsrc", "bwmask")


def test_launches_refuse_what_they_cannot_serve_and_write_nothing():
    B, K, Vp = 2, 8, 6
    D, X = _zeros(B, K, Vp), _outs(B, K, Vp)
    st = L.stream()

    def f(B_, K_, Vp_, D_, X_, **null):
        a = dict(g_raw=D_["g_raw"], l_raw=D_["l_raw"], fuse_raw=D_["fuse_raw"], gmask=D_["gmask"], lmask=D_["lmask"], fsrc=D_["fsrc"], bwmask=D_["bw"],
                 gl=X_["gl"], ll=X_["ll"], fl=X_["fl"])
        a.update(null)
        return lambda: O.sap_fuse_fwd(B_, K_, Vp_, a["g_raw"], a["l_raw"], a["fuse_raw"], a["gmask"], a["lmask"], a["fsrc"], a["bwmask"], True, a["gl"], a["ll"], a["fl"])

    def b(B_, K_, Vp_, D_, X_, **null):
        a = dict(g_raw=D_["g_raw"], l_raw=D_["l_raw"], fuse_raw=D_["fuse_raw"], gmask=D_["gmask"], lmask=D_["lmask"], fsrc=D_["fsrc"], bwmask=D_["bw"],
                 dg_raw=X_["dg"], dl_raw=X_["dl"], dfuse_raw=X_["df"])
        a.update(null)
        z = torch.zeros(B_ if B_ > 0 else 1, max(K_, Vp_), device=DEV)
        return lambda: O.sap_fuse_bwd(B_, K_, Vp_, a["g_raw"], a["l_raw"], a["fuse_raw"], a["gmask"], a["lmask"], a["fsrc"], a["bwmask"], True, z, z, z,
                                      a["dg_raw"], a["dl_raw"], a["dfuse_raw"])

    def lo(B_, K_, Vp_, D_, X_, nbytes=None, **over):
        p = _loss_struct(B_, K_, Vp_, D_, X_, **over)
        return lambda: L.call("magic_sap_fuse_loss", C.addressof(p), C.sizeof(p) if nbytes is None else nbytes, st)

    written = []
    # extents: Vp = 129 (all three), K = 513 (the fused loss only), B = 0
    D9, X9 = _zeros(B, K, 129), _outs(B, K, 129)
    for mk in (f, b, lo):
        _refused(mk(B, K, 129, D9, X9))
        _refused(mk(0, K, Vp, D, X))
    D5, X5 = _zeros(B, 513, Vp), _outs(B, 513, Vp)
    _refused(lo(B, 513, Vp, D5, X5))
    written += [X9, X5]
    # the parameter block: its size; options that need the teacher's logits; the temperature
    _refused(lo(B, K, Vp, D, X, nbytes=C.sizeof(L.SapLossParams) - 4))
    _refused(lo(B, K, Vp, D, X, nbytes=C.sizeof(L.SapLossParams) + 8))
    _refused(lo(B, K, Vp, D, X, t_fused=None, kd_rows=None))         # w_out without t_fused
    _refused(lo(B, K, Vp, D, X, t_fused=None, w_out=None))           # kd_rows without t_fused
    _refused(lo(B, K, Vp, D, X, T=0.0))
    _refused(lo(B, K, Vp, D, X, T=-1.0))
    with pytest.raises(L.MagicHipError, match="MAGIC_ERR_ARG"):      # the same through host/ops.py
        O.sap_fuse_loss(B, K, Vp, D["g_raw"], D["l_raw"], D["fuse_raw"], D["gmask"], D["lmask"], D["fsrc"], D["bw"], True, X["gl"], X["ll"], X["fl"], D["glab"], D["llab"],
                        0.1, X["rows"], w_out=X["w"])
    # every required pointer
    for name in REQUIRED + ("gl", "ll", "fl", "glab", "llab", "rows"):
        _refused(lo(B, K, Vp, D, X, **{name: None}))
    for name in REQUIRED + ("gl", "ll", "fl"):
        _refused(f(B, K, Vp, D, X, **{name: None}))
    for name in REQUIRED + ("dg_raw", "dl_raw", "dfuse_raw"):
        _refused(b(B, K, Vp, D, X, **{name: None}))
    torch.cuda.synchronize()
    written.append(X)
    for outs in written:
        for name, t in outs.items():
            assert torch.isnan(t).all(), f"a refused launch wrote {name}"
    # what was refused above is accepted one step inside the limits (the backward also with no upstream gradient at all: dg = dl = dfuse = 0)
    D2, X2 = _zeros(B, 513, 128), _outs(B, 513, 128)
    f(B, 513, 128, D2, X2)()
    O.sap_fuse_bwd(B, 513, 128, D2["g_raw"], D2["l_raw"], D2["fuse_raw"], D2["gmask"], D2["lmask"], D2["fsrc"], D2["bw"], True, None, None, None, X2["dg"], X2["dl"], X2["df"])
    D3, X3 = _zeros(B, 512, 128), _outs(B, 512, 128)
    lo(B, 512, 128, D3, X3)()
    torch.cuda.synchronize()
    assert (X2["dg"] == 0).all() and (X2["dl"] == 0).all() and (X2["df"] == 0).all()
    assert torch.isfinite(X2["fl"]).all() and torch.isfinite(X3["rows"]).all() and torch.isfinite(X3["kd"]).all()


def test_host_rule_for_the_fused_loss_is_the_launch_limit():
    """host/heads.py fuses the logit fusion into the loss launch only for K <= 512 and Vp <= 128 -- exactly what magic_sap_fuse_loss accepts"""
    assert "K <= 512 and Vp <= 128" in inspect.getsource(heads)
    st = L.stream()
    for K, Vp in ((512, 128), (513, 128), (512, 129), (513, 129), (1, 1)):
        D, X = _zeros(1, K, Vp), _outs(1, K, Vp)
        p = _loss_struct(1, K, Vp, D, X)
        call = lambda: L.call("magic_sap_fuse_loss", C.addressof(p), C.sizeof(p), st)
        if S.sap_fused_rule(K, Vp):
            call()
            torch.cuda.synchronize()
            assert torch.isfinite(X["rows"]).all()
        else:
            _refused(call)
            torch.cuda.synchronize()
            assert torch.isnan(X["rows"]).all() and torch.isnan(X["gl"]).all()


def test_zz_report():
    """largest err / bound per output over this file's run (pytest -s): the figures of tests/_sapfuse_ref64.py's docstring"""
    for prefix in ("sap ", "sap-separate "):
        worst = S.report(prefix)
        for key, val in worst.items():
            print(f"WORST {key:24s} {val:.3g}")
        assert all(val <= 1.0 for val in worst.values())
