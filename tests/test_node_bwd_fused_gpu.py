"""magic_node_in_bwd (csrc/rowops.hip node_in_bwd_kernel): the backward of the map / viewpoint input stage, the text-gradient fold and the panorama fusion's
backward as ONE launch, against float64 and against the five-launch sequence it replaces (add_n -> ln_bwd(do_ln=False) -> smallk_ln_bwd_pair ->
csr_gather_multi -> pano_fuse_bwd).

Bounds.  Activation gradients must be torch.equal to the sequence.  Against float64: one unit in the last place of the storage type + 1e-5 of the terms'
envelope (tests/test_partial_rows_gpu.py check_dx); a d_pano row is rounded up to three times (after each gather source, then with the fusion term), so every
EARLIER rounding point adds half a unit in the last place of the intermediate value it rounds (2^-8 / 2^-11 relative for bf16 / fp16; nothing for fp32).
Parameter sums: 1e-5 of the summed envelopes (check_sum), in the atomic and the partial-row form, and the same check against a reference without the last
workgroup's rows must fail."""
import ctypes as C

import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from tests.test_partial_rows_gpu import REL, _skb_problem, _skb_refs, check_dx, check_guards, check_sum, gen, run

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
WIDTHS = [H for H in (128, 256, 384, 768) if O.node_in_bwd_ok(torch.bfloat16, H, 37, 39, (7, 16))]      # H = 128 plus every other width the predicate accepts
NP, V, B, K, VP, KG, KV, NTAB, TXT = 5, 37, 3, 6, 13, 7, 16, 8, 33       # Np odd: a dead half-block; V = 37: not a multiple of the four waves, above 36
MG, MV = B * K, B * VP                                                 # 18: one partly filled 32-row block; 39: two blocks, the second with 7 rows
ALL = ("fuse", "gat", "skb0", "skb1", "table", "add")


@pytest.fixture
def poison(monkeypatch):
    """partial rows on at every width, every partial-row buffer NaN-filled with guard rows; yields the list of [buffer, rows used]"""
    guards = []
    monkeypatch.setattr(O, "PART_PG", True)
    monkeypatch.setattr(O, "PART_MIN_H", 128)
    monkeypatch.setattr(O, "PART_POISON", True)
    monkeypatch.setattr(O, "PART_GUARDS", guards)
    return guards


def _csr(rows, n_out, weighted):
    """rows: {output row: [(source row, weight), ...]} -> (ptr, idx, w | None) on the device"""
    ptr, idx, w = [0], [], []
    for r in range(n_out):
        for i, wt in rows.get(r, ()):
            idx.append(i); w.append(wt)
        ptr.append(len(idx))
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=DEV)
    return t(ptr, torch.int32), t(idx or [0], torch.int32), (t(w or [0.0], torch.float32) if weighted else None)


def _dense(rows, n_out, n_src, weighted):
    m = torch.zeros(n_out, n_src, dtype=torch.float64, device=DEV)
    for r, es in rows.items():
        for i, wt in es:
            m[r, i] += wt if weighted else 1.0
    return m


_CASES = {}


def case(dtype, H):
    """inputs + float64 references, built once per (dtype, H) and never modified"""
    if (dtype, H) in _CASES:
        return _CASES[(dtype, H)]
    rn = gen(H + {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[dtype])
    c = dict(dtype=dtype, H=H)
    c["x"] = rn(NP, V, H).to(dtype).to(DEV)
    lens = torch.tensor([1, V, 20, 5, V], device=DEV)
    mask = torch.arange(V, device=DEV)[None] < lens[:, None]
    c["probs"] = torch.softmax(rn(NP, V).to(DEV).masked_fill(~mask, float("-inf")), -1).float().contiguous()
    c["wf"] = (0.2 * rn(H)).float().to(DEV)
    c["d_gin"], c["d_vin"] = rn(MG, H).to(dtype).to(DEV), rn(MV, H).to(dtype).to(DEV)
    c["pano0"], c["fused0"] = rn(NP * V, H).to(dtype).to(DEV), rn(NP, H).to(dtype).to(DEV)
    c["ids"] = torch.tensor([0, 0, 3, NTAB - 1, 0, 0, 0, 1, 1, 2, 0, NTAB - 1, 5, 0, 0, 0, 0, 4], dtype=torch.int32, device=DEV)      # 0: the hot row; NTAB - 1: the largest id
    # rows of every kind.  source 1 (viewpoint tokens, unweighted) / source 2 (map nodes, weighted) into d_pano; one weighted source into d_fused
    last = NP * V - 1
    s1 = {3: [(0, 1.0)], 10: [(4, 1.0), (38, 1.0)], 36: [(7, 1.0)], 37: [(8, 1.0)], 100: [(20, 1.0)], last: [(12, 1.0)]}
    s2 = {3: [(2, 0.5)], 4: [(5, 0.25)], 36: [(1, 1.0), (17, 0.75), (9, 0.125)], 150: [(3, 2.0)], last: [(17, 0.5), (0, 1.5)]}       # row 5: in neither
    sf = {1: [(4, 0.5), (11, 1.0)], 2: [(6, 0.25)], 4: [(17, 1.0)]}                                              # panorama 0 and 3: referenced by no node
    c["csr1"], c["csr2"], c["csrf"] = _csr(s1, NP * V, False), _csr(s2, NP * V, True), _csr(sf, NP, True)
    c["skb"] = [_skb_problem(MG, H, KG, dtype, H + 11), _skb_problem(MV, H, KV, dtype, H + 12)]
    c["skb"][0]["dy"], c["skb"][1]["dy"] = c["d_gin"], c["d_vin"]
    c["gamma"] = [(1 + 0.2 * rn(H)).float().to(DEV) for _ in range(2)]
    c["beta"] = [(0.2 * rn(H)).float().to(DEV) for _ in range(2)]
    c["txt0"] = rn(TXT, H).to(dtype).to(DEV)
    c["parts"] = [rn(TXT, H).to(dtype).to(DEV) for _ in range(6)]
    # ---- float64
    gd, vd = c["d_gin"].double(), c["d_vin"].double()
    m1, m2, mf = _dense(s1, NP * V, MV, False), _dense(s2, NP * V, MG, True), _dense(sf, NP, MG, True)
    c["f64"] = dict(s1=m1 @ vd, e1=m1.abs() @ vd.abs(), has1=m1.abs().sum(1) > 0, s2=m2 @ gd, e2=m2.abs() @ gd.abs(), has2=m2.abs().sum(1) > 0,
                    sf=mf @ gd, ef=mf.abs() @ gd.abs(), skb=[_skb_refs(q, g, b) for q, g, b in zip(c["skb"], c["gamma"], c["beta"])])
    onehot = torch.nn.functional.one_hot(c["ids"].long(), NTAB).double()
    c["f64"]["tab"] = (onehot[:, :, None] * gd[:, None, :]).reshape(MG, -1)
    _CASES[(dtype, H)] = c
    return c


def outputs(c):
    H = c["H"]
    f = lambda *s, v=0.0: torch.full(s, v, device=DEV)
    return dict(d_pano=c["pano0"].clone(), d_fused=c["fused0"].clone(), d_txt=c["txt0"].clone(), dwf=f(H, v=0.25), dbf=f(1), dtab=f(NTAB, H, v=0.5),
                skb=[dict(dW=f(H, kin, v=0.125), db=f(H), dgamma=f(H), dbeta=f(H)) for kin in (KG, KV)])


def _skb_args(c, o, j):
    q = c["skb"][j]
    return dict(M=q["M"], Kin=q["Kin"], x=q["x"], dy=q["dy"], y=q["y"], gamma=c["gamma"][j], beta=c["beta"][j], rstd=q["rstd"], **o["skb"][j])


def _gathers(c, o):
    return (dict(out=o["d_pano"], n_out=NP * V, accumulate=True, src1=c["d_vin"], csr1=c["csr1"], src2=c["d_gin"], csr2=c["csr2"]),
            dict(out=o["d_fused"], n_out=NP, accumulate=True, src1=c["d_gin"], csr1=c["csrf"]))


def launch_fused(c, o, jobs, nadd):
    H = c["H"]
    O.node_in_bwd(H, fuse=dict(x=c["x"], probs=c["probs"], wf=c["wf"], dfused=o["d_fused"], dx=o["d_pano"], dwf=o["dwf"], dbf=o["dbf"], N=NP, V=V) if "fuse" in jobs else None,
                  gathers=_gathers(c, o) if "gat" in jobs and "fuse" in jobs else None,
                  skb=[_skb_args(c, o, j) for j in (0, 1) if f"skb{j}" in jobs],
                  table=dict(M=MG, dy=c["d_gin"], idx=c["ids"], dtab=o["dtab"]) if "table" in jobs else None,
                  add=(o["d_txt"], c["parts"][:nadd]) if "add" in jobs else None)


def launch_sequence(c, o, jobs, nadd):
    H = c["H"]
    if "add" in jobs:
        O.add_n(o["d_txt"], c["parts"][:nadd])
    if "table" in jobs:
        O.ln_bwd(MG, H, c["d_gin"], dx=None, do_ln=False, dtabs=((c["ids"], 0, 0, o["dtab"], 0), None, None), hot0=0)
    sk = [_skb_args(c, o, j) for j in (0, 1) if f"skb{j}" in jobs]
    if len(sk) == 2:
        O.smallk_ln_bwd_pair(H, sk)
    elif sk:
        q = sk[0]
        O.smallk_ln_bwd(q["M"], H, q["Kin"], q["x"], q["dy"], q["y"], q["gamma"], q["beta"], q["rstd"], q["dW"], q["db"], q["dgamma"], q["dbeta"])
    if "fuse" in jobs:
        if "gat" in jobs:
            O.csr_gather_multi(H, list(_gathers(c, o)))
        O.pano_fuse_bwd(c["x"], c["probs"], c["wf"], o["d_fused"], o["d_pano"], o["dwf"], o["dbf"], NP, V, H)


def check64(c, o, jobs, nadd, partial, tag):
    """every present job's outputs against float64, every absent job's outputs untouched"""
    H, dtype, r = c["H"], c["dtype"], c["f64"]
    hu = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}.get(dtype, 0.0) * 1.01
    fresh = outputs(c)
    if "add" in jobs:
        xs = torch.stack([t.double() for t in c["parts"][:nadd]])
        check_dx(o["d_txt"], c["txt0"].double() + xs.sum(0), c["txt0"].double().abs() + xs.abs().sum(0), f"{tag} d_txt", dtype)
    else:
        assert torch.equal(o["d_txt"], fresh["d_txt"])
    if "table" in jobs:
        check_sum(o["dtab"].reshape(-1), fresh["dtab"].reshape(-1), r["tab"], r["tab"].abs(), f"{tag} step table", torch.zeros(MG, device=DEV), 1)
    else:
        assert torch.equal(o["dtab"], fresh["dtab"])
    for j, (M_, kin) in enumerate(((MG, KG), (MV, KV))):
        if f"skb{j}" in jobs:
            blk, nblk = torch.arange(M_, device=DEV) // 32, (M_ + 31) // 32
            for k, (terms, env) in r["skb"][j].items():
                check_sum(o["skb"][j][k].reshape(-1), fresh["skb"][j][k].reshape(-1), terms, env, f"{tag} skb{j} {k}", blk, nblk)
        else:
            assert all(torch.equal(o["skb"][j][k], fresh["skb"][j][k]) for k in fresh["skb"][j])
    if "fuse" not in jobs:
        assert torch.equal(o["d_pano"], fresh["d_pano"]) and torch.equal(o["d_fused"], fresh["d_fused"]) and torch.equal(o["dwf"], fresh["dwf"])
        return
    f0, p0 = c["fused0"].double(), c["pano0"].double()
    gat = "gat" in jobs
    if gat:
        check_dx(o["d_fused"], f0 + r["sf"], f0.abs() + r["ef"], f"{tag} d_fused", dtype)
        assert torch.equal(o["d_fused"][0], c["fused0"][0]) and torch.equal(o["d_fused"][3], c["fused0"][3])       # no entries: the old row, untouched
    else:
        assert torch.equal(o["d_fused"], c["fused0"])
    # the fusion term is formed from the gathered d_fused row AS STORED (checked above), the fusion Linear's gradients likewise
    p, xd, dfd, wfd = c["probs"].double(), c["x"].double(), o["d_fused"].double(), c["wf"].double()
    dp, dpenv = (xd * dfd[:, None]).sum(-1), (xd * dfd[:, None]).abs().sum(-1)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    dsenv = p * (dpenv + (p * dpenv).sum(-1, keepdim=True))
    fz = (p[..., None] * dfd[:, None] + ds[..., None] * wfd).reshape(NP * V, H)
    fzenv = (p[..., None] * dfd.abs()[:, None] + dsenv[..., None] * wfd.abs()).reshape(NP * V, H)
    i1 = p0 + (r["s1"] if gat else 0.0)
    i2 = i1 + (r["s2"] if gat else 0.0)
    ref, env = i2 + fz, p0.abs() + fzenv + ((r["e1"] + r["e2"]) if gat else 0.0)
    early = (hu * (i1.abs() * r["has1"][:, None] + i2.abs() * r["has2"][:, None])) if gat else 0.0      # the roundings after source 1 / source 2, where they happen
    ulp = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}.get(dtype, 0.0)
    bound = ulp * ref.abs() + REL * (ref.abs() + env) + early + (6e-8 if dtype == torch.float16 else 1e-30)
    err = (o["d_pano"].double() - ref).abs()
    assert torch.isfinite(o["d_pano"]).all() and (err <= bound).all(), f"{tag} d_pano: max err/bound {(err / bound).max().item():.3g}"
    blk, nblk = torch.arange(NP, device=DEV) // 2, (NP + 1) // 2
    check_sum(o["dwf"], fresh["dwf"], (ds[..., None] * xd).sum(1), (dsenv[..., None] * xd.abs()).sum(1), f"{tag} dwf", blk, nblk)
    check_sum(o["dbf"], fresh["dbf"], ds.sum(1, keepdim=True), dsenv.sum(1, keepdim=True), f"{tag} dbf")


VARIANTS = [(ALL, 6), (ALL, 1)] + [(tuple(j for j in ALL if j != drop), 6) for drop in ALL]


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_launch_matches_float64_and_the_five_launch_sequence(dtype, H):
    assert 128 in WIDTHS and O.node_in_bwd_ok(dtype, H, V, MV, (KG, KV))
    c = case(dtype, H)
    for jobs, nadd in VARIANTS:
        for partial in (False, True):
            tag = f"{'+'.join(jobs)} n={nadd} {'partial' if partial else 'atomic'}"
            of, os_ = outputs(c), outputs(c)
            run(partial, lambda: launch_fused(c, of, jobs, nadd))
            run(partial, lambda: launch_sequence(c, os_, jobs, nadd))
            for k in ("d_pano", "d_fused", "d_txt"):
                assert torch.equal(of[k], os_[k]), f"{tag}: {k} differs from the sequence"
            if "fuse" in jobs and "gat" in jobs:
                assert not torch.equal(of["d_fused"], c["fused0"])
            check64(c, of, jobs, nadd, partial, tag)
            if partial:          # virtual blocks preserved: the fusion Linear's and the position embeddings' dW / db sums are the sequence's, bit for bit
                assert torch.equal(of["dwf"], os_["dwf"]) and torch.equal(of["dbf"], os_["dbf"])
                assert all(torch.equal(of["skb"][j][k], os_["skb"][j][k]) for j in (0, 1) for k in ("dW", "db"))
                o2 = outputs(c)
                run(True, lambda: launch_fused(c, o2, jobs, nadd))
                same = lambda a, b: torch.equal(a, b)
                assert all(same(of[k], o2[k]) for k in ("d_pano", "d_fused", "d_txt", "dwf", "dbf")), f"{tag}: two partial-row runs differ"
                assert all(same(of["skb"][j][k], o2["skb"][j][k]) for j in (0, 1) for k in of["skb"][j]), f"{tag}: two partial-row runs differ"


def test_partial_row_buffers_have_the_rows_the_launch_writes(poison):
    c = case(torch.bfloat16, 128)
    o = outputs(c)
    want = O.node_in_bwd_blocks(Np=NP, Ms=(MG, MV), H=128)
    assert want == ((NP + 1) // 2, [(MG + 31) // 32, (MV + 31) // 32])
    run(True, lambda: launch_fused(c, o, ALL, 6))
    assert [n for _, n in poison] == [want[0]] + want[1]          # one buffer per job with parameter sums, sized by the helper
    assert check_guards(poison) == 3                               # every counted row finite, every guard row still NaN
    check64(c, o, ALL, 6, True, "poisoned")


@pytest.mark.parametrize("form", ["sap", "mlm"])
def test_engine_fused_method_matches_the_old_sequence(form):
    """setup of test_node_inputs_backward_in_shared_launches_matches_the_per_op_sequence; sap: both encoders + the six-part fold; mlm: the map
    encoder only with add_(d_txt, d_t2) as the fold.  Old sequence: fold, nodes_in_bwd / gmap_in_bwd, _pano_head_bwd."""
    from magic_amd.host import synth
    from magic_amd.host.plan import build_plan
    from tests.test_encoder_gpu import student
    m = student(0.0)
    batch = synth.make_batch("sap", batch_size=7, seed=5, step=0, dup_view_prob=0.3)
    plan = build_plan(batch, "sap", torch.device(DEV))
    inp = m._inputs(batch, plan)
    m.store.sync_shadow()
    m.store.ensure_grads()
    n = m.net
    n.set_dropout(None, 0.0, 0.0)
    ct = n.text_fwd(plan)
    cp = n.pano_fwd(plan, inp.feats, inp.loc)
    gin, vin = n.nodes_in_fwd(plan, cp, inp.gpos, inp.vpos)
    if form == "mlm":
        vin = None
    assert n.nodes_pano_ok(plan, gin=gin, vin=vin)
    g = torch.Generator().manual_seed(7)
    H, Bb, Kk, Vp, Np, Vv = n.H, plan["B"], plan["K"], plan["Vp"], plan["Np"], plan["V"]
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.1).to(DEV).bfloat16()
    d_gin, d_vin, base_p, base_f = rnd(Bb * Kk, H), rnd(Bb * Vp, H), rnd(Np * Vv, H), rnd(Np, H)
    base_t = rnd(Bb * plan["L"], H)
    parts = [rnd(Bb * plan["L"], H) for _ in range(6 if form == "sap" else 1)]
    off, numel = m.store.offsets[n.p + "global_encoder.gmap_step_embeddings.weight"][:2]      # (its scatter stays fp32 atomics: order-dependent in every form)
    res = []
    for fused in (False, True, True):
        m.store.zero_grad()
        dp, df, dt = base_p.clone(), base_f.clone(), base_t.clone()

        def go():
            if fused:
                n.nodes_pano_bwd(plan, cp, gin, d_gin, vin, d_vin if vin is not None else None, dp, df, add=(dt, parts))
            else:
                if form == "sap":
                    O.add_n(dt, parts)
                    n.nodes_in_bwd(plan, gin, d_gin, vin, d_vin, dp, df)
                else:
                    O.add_(dt, parts[0])
                    n.gmap_in_bwd(gin, plan, d_gin, dp, df)
                n._pano_head_bwd(cp, dp, df)
        run(True, go)
        res.append((dp, df, dt, m.store.grad.clone()))
    old, new, again = res
    for i, k in enumerate(("d_pano", "d_fused", "d_txt")):
        assert torch.equal(new[i], old[i]), k
        assert torch.equal(again[i], new[i]), k
    assert not torch.equal(new[0], base_p) and not torch.equal(new[2], base_t)
    ga, gb = new[3], old[3]
    assert gb.abs().max() > 0 and torch.allclose(ga, gb, rtol=1e-4, atol=1e-5), (ga - gb).abs().max().item()
    keep = torch.ones_like(ga, dtype=torch.bool)
    keep[off:off + numel] = False
    assert torch.equal(again[3][keep], ga[keep]), "two fused runs in the partial-row form differ outside the step table"
    assert torch.allclose(again[3], ga, rtol=1e-4, atol=1e-5)


def test_argument_errors_return_err_arg_and_launch_nothing():
    c = case(torch.bfloat16, 128)
    o = outputs(c)
    fn = L.load().magic_node_in_bwd
    P = L.P
    st = L.stream()
    fuse = [NP, V, P(c["x"]), P(c["probs"]), P(c["wf"]), P(o["d_fused"]), P(o["d_pano"]), P(o["dwf"]), P(o["dbf"]), 0]      # (dbf given: the atomic form, 0 partial rows)
    nofuse = [0, 0, None, None, None, None, None, None, None, 0]
    notab, noadd = [0, None, None, None], [0, 0, None, None]
    tab = [MG, P(c["d_gin"]), P(c["ids"]), P(o["dtab"])]

    def skb(kin=KG, **over):
        a = (L.SkbProb * 1)()
        q = _skb_args(c, o, 0)
        a[0].M, a[0].Kin = q["M"], kin
        for k in ("x", "dy", "y", "gamma", "beta", "rstd", "dW", "db", "dgamma", "dbeta"):
            setattr(a[0], k, P(over.get(k, q[k])) if over.get(k, q[k]) is not None else None)
        return a

    def adds(n):
        return (C.c_void_p * n)(*[c["parts"][i % 6].data_ptr() for i in range(n)])
    ERR = -1
    xs9, xs2, good, bad_k, bad_x = adds(9), adds(2), skb(), skb(kin=17), skb(x=None)
    assert fn(1, 128, *nofuse, None, 0, None, *notab, *noadd, st) == ERR                                               # no job at all
    for i in (3, 4, 5, 6, 7):                                                                                            # a required fusion pointer missing (x NULL = the job is absent)
        assert fn(1, 128, *[None if j == i else v for j, v in enumerate(fuse)], None, 0, None, *notab, *noadd, st) == ERR, i
    assert fn(1, 128, *nofuse, None, 1, C.addressof(bad_x), *notab, *noadd, st) == ERR
    assert fn(1, 128, *nofuse, None, 1, None, *notab, *noadd, st) == ERR
    assert fn(1, 128, *nofuse, None, 1, C.addressof(bad_k), *notab, *noadd, st) == ERR                                 # Kin > 16
    assert fn(1, 128, *nofuse, None, 0, None, MG, P(c["d_gin"]), None, P(o["dtab"]), *noadd, st) == ERR                 # table without ids
    assert fn(1, 128, *nofuse, None, 0, None, *notab, TXT * 128, 9, C.addressof(xs9), P(o["d_txt"]), st) == ERR         # n > 8 addends
    assert fn(1, 128, *nofuse, None, 0, None, *notab, TXT * 128, 2, None, P(o["d_txt"]), st) == ERR
    for H in (384, 768, 64, 200):                                                                                        # unsupported widths
        assert fn(1, H, *fuse, None, 1, C.addressof(good), *tab, TXT * H, 2, C.addressof(xs2), P(o["d_txt"]), st) == ERR, H
    assert fn(1, 128, NP, 41, *fuse[2:], None, 0, None, *notab, *noadd, st) == ERR                                      # more views than a wave's registers hold
    torch.cuda.synchronize()
    fresh = outputs(c)
    assert all(torch.equal(o[k], fresh[k]) for k in ("d_pano", "d_fused", "d_txt", "dwf", "dbf", "dtab"))
    assert all(torch.equal(o["skb"][0][k], fresh["skb"][0][k]) for k in fresh["skb"][0])
    with pytest.raises(L.MagicHipError, match="MAGIC_ERR_ARG"):
        O.node_in_bwd(128, add=(o["d_txt"], [c["parts"][i % 6] for i in range(9)]))
    assert fn(1, 128, *nofuse, None, 0, None, *notab, TXT * 128, 2, C.addressof(xs2), P(o["d_txt"]), st) == 0           # and a well-formed call goes through
    torch.cuda.synchronize()
    assert not torch.equal(o["d_txt"], fresh["d_txt"])
