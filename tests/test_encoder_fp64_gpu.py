"""Whole-encoder forwards (csrc/encoder.hip: magic_encoder_fwd, magic_xencoder_fwd) against fp64, stage by stage (-m gpu).

Every output buffer is NaN-filled before the launch.  After it, every tensor the contract says is written must be finite, the pad columns
N <= c < ldp of P / Pd / Pc / Pdc exactly 0 (attention.hip and encbwd.hip read whole ldp rows), and the give-up word of the sync buffer 0.
Each saved tensor is then recomputed in fp64 (oracle/layer_ref.py) from the kernel's OWN saved 16-bit inputs to that stage -- the layer
input of layer l > 0 is layer l-1's saved `out` -- with the 16-bit weights upcast and the kernel's own dropout masks
(tests.test_dropout_gpu.export_mask).  Each compared tensor then carries one rounding, and the bound is per element:

    |k - ref| <= c * ulp(|ref|) + extra + floor * ulp(rms of the ref's row)

ulp = the storage type's unit in the last place.  `extra` is the part the kernel does not round from the saved input: g = gelu(z) is taken
from the fp32 z, not from the saved 16-bit z (|gelu'(z)| * ulp(z) / 2), and gelu_fast replaces erf by Abramowitz & Stegun 7.1.26 (its
error, evaluated here in fp64, plus fp32 slack).  The floor covers fp32 accumulation and LayerNorm cancellation.  The measured worst of each
stage is printed with -s and the bounds sit at ~2-3x the measured values (BOUNDS, with the width-independent checks, in tests/_layer_ref64.py).

Launch forms: every form of magic_encoder_fwd (row-split, mixed, per-sample full / compact, the per-sample fallback when the tiles do not
fit the chip) and of magic_xencoder_fwd (row-split, per-sample) is reached through shapes; `enc_form` / `xenc_form` mirror the C rules and
each case asserts the form that ran from its sync buffer (pre-filled with a sentinel: the per-sample forms zero only its first 16 bytes,
the row-split forms zero and count all of it).  The buffer cannot tell the two per-sample LDS layouts apart (compact when every sample has
<= 48 rows, full otherwise): which of them ran is inferred from the C rule, not observed; the cases put N on both sides of 48."""
import ctypes as C
import math
import zlib

import pytest
import torch

import magic_amd  # noqa: F401
import oracle.layer_ref as LR
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from tests._layer_ref64 import (BOUNDS, BWD_BOUNDS, BWD_COS, RSTD_REL, STATS, check, check_dx_tiles, check_gelu, check_param_grads,  # noqa: F401
                                check_rstd, check_segment, engine_layer, engine_segment, engine_sites, gelu_as, rel_cos,  # noqa: F401
                                stack_reference, ulp)
from tests.test_dropout_gpu import seed_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, I, NH, EPS, SCALE = 128, 512, 2, 1e-12, 0.125
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
SENT = 0x5A5A5A5A


# ---- synthetic operands --------------------------------------------------------------------------------------------------------------
def rup8(n):
    return (n + 7) // 8 * 8


def ragged(nsamp, N):
    """1, N-1, N and a length that ends a 16-row tile, cycled"""
    base = [1, max(1, N - 1), N, max(1, (N - 1) // 16 * 16) if N > 16 else N]
    return [base[i % 4] for i in range(nsamp)]


def mask_of(lens, N):
    return torch.arange(N)[None, :] < torch.tensor(lens)[:, None]


def weights(dtype, g, cross):
    """16-bit matrices (upcast copy for the reference, fragment-order copy for the kernel) with non-trivial biases and LayerNorm parameters"""
    def W(n, k, s=1.0):
        return (torch.randn(n, k, generator=g) * (s / math.sqrt(k))).to(dtype)

    def vec(n, s=0.1, one=False):
        return (1.0 if one else 0.0) + torch.randn(n, generator=g) * s
    w = {"Wqkv": W(3 * H, H), "bqkv": vec(3 * H), "Wo": W(H, H), "bo": vec(H), "g1": vec(H, 0.2, True), "be1": vec(H),
         "W1": W(I, H, 1.5), "bi": vec(I), "W2": W(H, I), "bo2": vec(H), "g2": vec(H, 0.2, True), "be2": vec(H)}
    if cross:
        w.update({"Wq": W(H, H), "bq": vec(H), "Wkv": W(2 * H, H), "bkv": vec(2 * H), "Woc": W(H, H), "boc": vec(H), "gc": vec(H, 0.2, True),
                  "bec": vec(H)})
    ref = {k: v.double() for k, v in w.items()}
    dev = {k: (O.pack_frag(v.to(DEV).contiguous()) if k.startswith("W") else v.float().to(DEV).contiguous()) for k, v in w.items()}
    return ref, dev


def nan(*shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


SITE = [100]


def site():
    SITE[0] += 7919
    return SITE[0]


class Seg:
    """one encoder segment of a launch: inputs, per-layer weights and NaN-filled outputs"""

    def __init__(self, dtype, nsamp, N, nlayers, p, g, cross=False, Nk=None, with_dist=False):
        self.dtype, self.ns, self.N, self.nl, self.p, self.cross = dtype, nsamp, N, nlayers, p, cross
        self.lens = ragged(nsamp, N)
        self.M, self.ldp = nsamp * N, rup8(N)
        self.x = torch.randn(self.M, H, generator=g).to(dtype).to(DEV)
        self.kmask = mask_of(self.lens, N)
        self.kmask_d = self.kmask.to(torch.uint8).to(DEV).contiguous()
        if cross:
            self.Nk, self.ldpc = Nk, rup8(Nk)
            self.klens = ragged(nsamp, Nk)[::-1]
            self.cmask = mask_of(self.klens, Nk)
            self.cmask_d = self.cmask.to(torch.uint8).to(DEV).contiguous()
            self.cx = torch.randn(nsamp * Nk, H, generator=g).to(dtype).to(DEV)
            self.dist = (torch.rand(nsamp, N, N, generator=g) * 6).to(DEV) if with_dist else None
            self.sprel = (torch.tensor([-0.6], device=DEV), torch.tensor([0.25], device=DEV)) if with_dist else None
        self.layers = []
        for _ in range(nlayers):
            ref, dev = weights(dtype, g, cross)
            M, ns, ldp = self.M, nsamp, self.ldp
            o = dict(qkv=nan(M, 3 * H, dtype=dtype), P=nan(ns, NH, N, ldp, dtype=dtype), Pd=nan(ns, NH, N, ldp, dtype=dtype) if p > 0 else None,
                     ctx=nan(M, H, dtype=dtype), a=nan(M, H, dtype=dtype), rstd_a=nan(M, dtype=torch.float32),
                     z=nan(M, I, dtype=dtype), g=nan(M, I, dtype=dtype), out=nan(M, H, dtype=dtype), rstd_o=nan(M, dtype=torch.float32))
            sites = dict(site_attn=site(), site_ao=site(), site_out=site())
            if cross:
                o.update(q=nan(M, H, dtype=dtype), kv=nan(nsamp * Nk, 2 * H, dtype=dtype), Pc=nan(ns, NH, N, self.ldpc, dtype=dtype),
                         Pdc=nan(ns, NH, N, self.ldpc, dtype=dtype) if p > 0 else None, cctx=nan(M, H, dtype=dtype), c=nan(M, H, dtype=dtype),
                         rstd_c=nan(M, dtype=torch.float32))
                sites.update(site_cattn=site(), site_co=site())
            self.layers.append((ref, dev, o, sites))


def _sync_buffer(segs):
    words = 4 + 6 * sum(s.ns for s in segs)
    return torch.full(((words + 3) // 4 * 4,), SENT, dtype=torch.int32, device=DEV)


def launch_enc(segs, p, seed):
    """magic_encoder_fwd with a sentinel-filled sync buffer of the test's own (host/ops.encoder_fwd allocates it uninitialised)"""
    P = L.EncParams()
    P.nseg, P.p_attn, P.p_hidden, P.eps, P.scale = len(segs), p, p, EPS, SCALE
    P.seed = L.P(seed if p > 0 else None)
    for i, sg in enumerate(segs):
        S = P.seg[i]
        S.x, S.kmask, S.nsamp, S.N, S.ldp, S.nlayers = L.P(sg.x), L.P(sg.kmask_d), sg.ns, sg.N, sg.ldp, sg.nl
        for j, (_, dev, o, sites) in enumerate(sg.layers):
            D = S.L[j]
            for k, v in list(dev.items()) + list(o.items()):
                setattr(D, k, L.P(v))
            for k, v in sites.items():
                setattr(D, k, v)
    sync = _sync_buffer(segs)
    P.sync, P.sync_words = L.P(sync), sync.numel()
    L.call("magic_encoder_fwd", L.dt(segs[0].dtype), C.addressof(P), C.sizeof(P), L.stream())
    torch.cuda.synchronize()
    return sync.cpu()


def launch_xenc(segs, p, seed):
    P = L.XParams()
    P.nseg, P.p_attn, P.p_hidden, P.eps, P.scale = len(segs), p, p, EPS, SCALE
    P.seed = L.P(seed if p > 0 else None)
    for i, sg in enumerate(segs):
        S = P.seg[i]
        S.x, S.cx, S.qmask, S.cmask = L.P(sg.x), L.P(sg.cx), L.P(sg.kmask_d), L.P(sg.cmask_d)
        S.dist = L.P(sg.dist)
        S.sprel_w, S.sprel_b = (L.P(sg.sprel[0]), L.P(sg.sprel[1])) if sg.sprel else (None, None)
        S.nsamp, S.Nq, S.Nk, S.ldps, S.ldpc, S.nlayers = sg.ns, sg.N, sg.Nk, sg.ldp, sg.ldpc, sg.nl
        for j, (_, dev, o, sites) in enumerate(sg.layers):
            D = S.L[j]
            for k, v in list(dev.items()) + list(o.items()):
                setattr(D, k, L.P(v))
            for k, v in sites.items():
                setattr(D, k, v)
    sync = _sync_buffer(segs)
    P.sync, P.sync_words = L.P(sync), sync.numel()
    L.call("magic_xencoder_fwd", L.dt(segs[0].dtype), C.addressof(P), C.sizeof(P), L.stream())
    torch.cuda.synchronize()
    return sync.cpu()


# ---- launch forms --------------------------------------------------------------------------------------------------------------------
def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def enc_form(shapes, cus):
    """magic_encoder_fwd's rule (row-split launch requested): shapes = [(nsamp, N)] per segment"""
    nt = [(n + 15) // 16 for _, n in shapes]
    ns = [s for s, _ in shapes]
    rs0 = nt[0] >= 4 and ns[0] * nt[0] <= cus
    rs1 = len(shapes) > 1 and nt[1] >= 4 and ns[0] * nt[0] + ns[1] * nt[1] <= cus
    if rs0 and (rs1 or len(shapes) == 1):
        return "row_split"
    if rs0 and len(shapes) == 2 and nt[1] <= 3:
        return "mixed"
    return "per_sample_compact" if all(n <= 48 for _, n in shapes) else "per_sample_full"


def xenc_form(shapes, cus):
    """magic_xencoder_fwd's rule: shapes = [(nsamp, Nq)]"""
    grid = sum(s * ((n + 15) // 16) for s, n in shapes)
    return "row_split" if grid <= cus and grid > sum(s for s, _ in shapes) else "per_sample"


def observed_form(sync, segs):
    """what the sync buffer says ran: untouched past word 4 -> a per-sample form.  Otherwise the launch zeroed it, and every row-split tile
    adds 1 to its sample's word l after layer l (l < layers - 1): a row-split segment of >= 2 layers reads ceil(N / 16) there, a segment that
    ran per sample inside the mixed launch reads 0.  A 1-layer segment counts nothing ("?": row-split or mixed)."""
    assert int(sync[0]) == 0, "a bounded hand-off wait gave up"
    w = sync[4:4 + 6 * sum(s.ns for s in segs)]
    if (w == SENT).all():
        return "per_sample"
    assert not (w == SENT).any(), "the sync buffer is partly zeroed"
    kinds, off = [], 0
    for sg in segs:
        c = w[off:off + 6 * sg.ns].view(sg.ns, 6)
        off += 6 * sg.ns
        if sg.nl < 2 or (c == 0).all():
            kinds.append("?" if sg.nl < 2 else "per_sample")
            continue
        want = torch.zeros_like(c)
        want[:, :sg.nl - 1] = (sg.N + 15) // 16
        assert torch.equal(c, want), f"hand-off counters {c.tolist()} != {want.tolist()}"
        kinds.append("tiles")
    return kinds


def form_matches(seen, form, nseg):
    if form.startswith("per_sample"):
        return seen == "per_sample"
    want = ["tiles"] * nseg if form == "row_split" else ["tiles", "per_sample"]
    return seen != "per_sample" and all(a in ("?", b) for a, b in zip(seen, want))


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
# (id, [(nsamp, N)] per segment, layers); nsamp None: one more 80-row sample than the chip holds as 5-tile row-split workgroups
ENC_CASES = [
    ("N1", [(3, 1)], 1), ("N16", [(4, 16)], 2), ("N17", [(4, 17)], 1), ("N48", [(4, 48)], 2),
    ("N49", [(4, 49)], 1), ("N79", [(4, 79)], 2), ("N80x6", [(4, 80)], 6),
    ("text80+pano36", [(6, 80), (6, 36)], 2), ("text80+pano37", [(5, 80), (7, 37)], 1),
    ("text80+seg64", [(3, 80), (3, 64)], 2), ("seg48+seg80", [(3, 48), (3, 80)], 1), ("seg17+seg48", [(4, 17), (3, 48)], 2),
    ("fallback80", [(None, 80)], 1),
]
# (id, [(nsamp, Nq, Nk, dist)] per segment, layers)
XENC_CASES = [
    ("q1k80", [(3, 1, 80, False)], 1), ("q16k17+dist", [(4, 16, 17, True)], 3), ("q17k48+dist", [(4, 17, 48, True)], 1),
    ("q48k1", [(4, 48, 1, False)], 1), ("q49k79", [(3, 49, 79, False)], 3), ("q80k49", [(3, 80, 49, False)], 1),
    ("global37+local20", [(4, 37, 80, True), (4, 20, 80, False)], 3), ("q79k16+q1k80", [(2, 79, 16, True), (3, 1, 80, False)], 1),
    ("fallback80", [(None, 80, 17, True)], 1),
]


def _ns(n, cus):
    return n if n is not None else cus // 5 + 1


def test_every_launch_form_is_reached_by_the_cases():
    """the case lists together reach every form of both entry points on this chip (each case asserts the form that actually ran)"""
    cus = ncu()
    assert {enc_form([(_ns(s, cus), n) for s, n in sh], cus) for _, sh, _ in ENC_CASES} == \
        {"row_split", "mixed", "per_sample_full", "per_sample_compact"}
    assert enc_form([(_ns(None, cus), 80)], cus) == "per_sample_full"          # the fallback: row-split requested, tiles > CUs
    assert {xenc_form([(_ns(s, cus), q) for s, q, _, _ in sh], cus) for _, sh, _ in XENC_CASES} == {"row_split", "per_sample"}
    assert xenc_form([(_ns(None, cus), 80)], cus) == "per_sample"


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", ENC_CASES, ids=[c[0] for c in ENC_CASES])
def test_encoder_forward_stages_vs_fp64(case, dtype, p):
    name, shapes, nl = case
    cus = ncu()
    dt = DTYPES[dtype]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 10007)
    segs = [Seg(dt, _ns(s, cus), n, nl, p, g) for s, n in shapes]
    seed = seed_of(2024, 7)
    sync = launch_enc(segs, p, seed)
    want = enc_form([(s.ns, s.N) for s in segs], cus)
    seen = observed_form(sync, segs)
    assert form_matches(seen, want, len(segs)), (name, want, seen)
    for i, sg in enumerate(segs):
        check_segment(sg, p, seed, f"{name} {dtype} p={p} seg {i} ({want})", H, NH, I)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", XENC_CASES, ids=[c[0] for c in XENC_CASES])
def test_cross_encoder_forward_stages_vs_fp64(case, dtype, p):
    name, shapes, nl = case
    cus = ncu()
    dt = DTYPES[dtype]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 10007 + 1)
    segs = [Seg(dt, _ns(s, cus), q, nl, p, g, cross=True, Nk=k, with_dist=d) for s, q, k, d in shapes]
    seed = seed_of(99, 2025)
    sync = launch_xenc(segs, p, seed)
    want = xenc_form([(s.ns, s.N) for s in segs], cus)
    seen = observed_form(sync, segs)
    assert form_matches(seen, want, len(segs)), (name, want, seen)
    for i, sg in enumerate(segs):
        check_segment(sg, p, seed, f"x{name} {dtype} p={p} seg {i} ({want})", H, NH, I)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_forward_bounds_catch_planted_defects(dtype):
    """one element moved by 4 storage ulps, and one sample's probability row taken from the fp64 variant with its last valid key
    masked, each applied to a copy of the kernel's result, must fail the stage check"""
    dt = DTYPES[dtype]
    g = torch.Generator().manual_seed(5)
    kept = dict(STATS)             # (the defective copies are not measurements)
    sg = Seg(dt, 4, 49, 1, 0.0, g)
    launch_enc([sg], 0.0, None)
    check_segment(sg, 0.0, None, "clean", H, NH, I)
    w, _, o, _ = sg.layers[0]
    ns, N = sg.ns, sg.N
    x = sg.x.double().cpu().view(ns, N, H)
    for stage in ("qkv", "a", "z", "out"):
        k = o[stage].double().cpu()
        r, c = k.shape[0] // 3, 5
        bad = k.clone()
        bad[r, c] += 4 * ulp(bad[r, c], dt)
        bad = bad.to(dt).double()          # (the moved value is a storage value)
        ref = {"qkv": lambda: LR.linear(x, w["Wqkv"], w["bqkv"]).view(-1, 3 * H),
               "a": lambda: LR.dense_add_ln(x, o["ctx"].double().cpu().view(ns, N, H), w["Wo"], w["bo"], w["g1"], w["be1"], EPS)[0].view(-1, H),
               "z": lambda: LR.linear(o["a"].double().cpu(), w["W1"], w["bi"]),
               "out": lambda: LR.dense_add_ln(o["a"].double().cpu(), o["g"].double().cpu(), w["W2"], w["bo2"], w["g2"], w["be2"], EPS)[0]}[stage]()
        check(stage, k, ref, dt, "clean copy")
        with pytest.raises(AssertionError):
            check(stage, bad, ref, dt, f"{stage} moved by 4 ulp")
    # the last valid key of sample 1 (length N-1) dropped from the mask: its rows, rounded to storage, in place of the kernel's
    qkv = o["qkv"].double().cpu().view(ns, N, 3 * H)
    Pk = o["P"].double().cpu().view(ns, NH, N, sg.ldp)[..., :N]
    Pref = LR.probs(qkv[..., :H], qkv[..., H:2 * H], sg.kmask, NH, SCALE)
    km = sg.kmask.clone()
    km[1, sg.lens[1] - 1] = False
    Pvar = LR.probs(qkv[..., :H], qkv[..., H:2 * H], km, NH, SCALE).to(dt).double()
    check("P", Pk, Pref, dt, "clean copy")
    bad = Pk.clone()
    bad[1] = Pvar[1]
    with pytest.raises(AssertionError):
        check("P", bad, Pref, dt, "sample 1 without its last key")
    STATS.clear()
    STATS.update(kept)


# =====================================================================================================================================
# Row-block backward (csrc/encbwd.hip: magic_rowbwd) against fp64 autograd of oracle/layer_ref.py
# =====================================================================================================================================
# Students with 1-3 layers per stack drive MagicNet.self_stacks_bwd (text + panorama stacks together).  The reference chains layer_ref's
# stages in fp64 from the kernel's saved stack input, with the engine's 16-bit shadow weights upcast, the fp32 biases / LayerNorm parameters,
# the engine's own dropout masks, the same d_top and the same dP_init on the top block's exposed (dropped) attention map.  Every parameter
# gradient of both stacks (after flush_dw, which also adds up the row-block partial rows) is compared by rel-L2 and cosine; the gradient wrt
# the stack input per (sample, 16-row tile).  Measured worst on MI355X over BWD_CASES at p 0 and 0.1 (bf16 / fp16), bound ~2.5x:
#   weights / gammas rel-L2 1.08e-2 / 1.27e-3     biases / betas (cancellation class) 1.32e-2 / 1.48e-3     input gradient per tile 4.7e-3 / 5.8e-4
# (BWD_BOUNDS / BWD_COS, with the checks that assert them, in tests/_layer_ref64.py)


def bwd_student(dtype, p, nl, npano):
    from magic_amd.host.config import make_config
    from magic_amd.host.model_pretrain import GlocalTextPathCMTPreTraining
    from tests.test_model_gpu import KDL
    cfg = make_config(128, role="student", teacher_hidden_size=256, kdl=KDL, hidden_dropout_prob=p, attention_probs_dropout_prob=p,
                      num_l_layers=nl, num_pano_layers=npano, num_x_layers=1)
    m = GlocalTextPathCMTPreTraining(cfg, device=DEV, compute_dtype=dtype, seed=3)
    with torch.no_grad():          # non-trivial biases / LayerNorm parameters
        g = torch.Generator().manual_seed(1)
        for nm, q in m.named_parameters():
            if nm.endswith("bias") and q.dim() == 1:
                q.copy_((torch.randn(q.shape, generator=g) * 0.05).to(DEV))
            if "LayerNorm.weight" in nm:
                q.add_((torch.randn(q.shape, generator=g) * 0.1).to(DEV))
    m.store.shadow_clean = False
    return m


def recorder(cover, jobs):
    """wraps O.rowbwd: records (mode, rows, with_dist, kt) of every segment it launches, and the partial-row jobs it queues"""
    inner = O.rowbwd

    def rowbwd(segs, seed, p_hidden, p_attn=0.0, scale=0.125):
        att = any(int(sg.get("mode", 0)) for sg in segs)
        rows = 16 if att else int(L.load().magic_rowbwd_rows(sum(int(sg["M"]) for sg in segs)))
        for sg in segs:
            mode = int(sg.get("mode", 0))
            cover.add((mode, rows, bool(mode and (sg.get("dist") is not None or sg.get("dP_init") is not None)),
                       int(sg.get("kt", 12)) if (not mode and sg.get("dqkv_n") is not None) else None))
        n0 = len(O.RBW_JOBS)
        inner(segs, seed, p_hidden, p_attn=p_attn, scale=scale)
        jobs.extend(O.RBW_JOBS[n0:])
    return rowbwd


def run_self_stacks(dtype, p, nl, npano, B, attn_mode, with_dP, monkeypatch, cover, max_len=80):
    """forward (text + panorama in one whole-encoder launch) and the row-block backward of both stacks; returns what the checks need"""
    from magic_amd.host import synth
    from magic_amd.host.plan import build_plan
    from tests.test_encoder_gpu import _check_partial_rows, _poison_partial_rows
    dt = DTYPES[dtype]
    m = bwd_student(dt, p, nl, npano)
    m.train()
    guards = _poison_partial_rows(monkeypatch)
    jobs = []
    monkeypatch.setattr(O, "RBW_ATTN_MODE", attn_mode)
    monkeypatch.setattr(O, "rowbwd", recorder(cover, jobs))
    batch = synth.make_batch("sap", batch_size=B, seed=5, step=0, dup_view_prob=0.3, max_len=max_len, min_len=min(20, max_len))
    plan = build_plan(batch, "sap", torch.device(DEV))
    inp = m._inputs(batch, plan)
    m.store.sync_shadow()
    n = m.net
    assert n.rbw_ok() and n.enc_ok(plan["L"], nl)
    seed = seed_of(4321, 99)
    n.set_dropout(seed if p > 0 else None, p, p)
    ct = n.text_fwd(plan, defer=True)
    cp = n.pano_fwd(plan, inp.feats, inp.loc, defer=True)
    n.encoders_fwd(ct, cp)                       # one launch for both stacks, as the training step runs them
    sync = O.ENC_SYNC_LAST[0].cpu() if O.ENC_SYNC_LAST[0] is not None else None
    fmts = (n.p + "lang_encoder.layer.{}.", n.p + "img_embeddings.pano_encoder.layer.{}.")
    segs = [engine_segment(n, ct, fmts[0], plan["txt_mask"], dt, p, H), engine_segment(n, cp, fmts[1], plan["pano_mask"], dt, p, H)]
    g = torch.Generator().manual_seed(3)
    tops, dPs = [], []
    for sg in segs:
        tops.append((torch.randn(sg.M, H, generator=g) * 0.1).to(dt).to(DEV))
        if with_dP:
            dP = torch.zeros(sg.ns, NH, sg.N, sg.ldp)
            dP[..., :sg.N] = torch.randn(sg.ns, NH, sg.N, sg.N, generator=g) * 0.02
            dPs.append(dP.to(DEV))
        else:
            dPs.append(None)
    m.store.zero_grad()
    O.defer_dw(True)
    dx = n.self_stacks_bwd([(ct, fmts[0], tops[0].clone(), dPs[0]), (cp, fmts[1], tops[1].clone(), dPs[1])])
    O.flush_dw()
    torch.cuda.synchronize()
    _check_partial_rows(guards, True)
    return m, segs, fmts, tops, dPs, dx, seed, sync, jobs


# (layers text / panorama, samples, RBW_ATTN_MODE, dP_init): together they reach mode 0 at 16 and 32 rows, modes 1 and 2, the rowbwd16ad form
# (dP_init on the top block's attention backward inside the launch) and the tail chain with kt 0 and 12
BWD_CASES = [(2, 1, 6, 0, True), (3, 1, 6, 1, False), (2, 2, 5, 2, True), (2, 2, 48, 0, False)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_rowblock_backward_vs_fp64_autograd(dtype, p, monkeypatch):
    """text + panorama stacks' backward on magic_rowbwd against fp64 autograd, in every (mode, rows, kt) form the engine launches; the
    48-sample case is the benchmark's shape (its forward -- the mixed whole-encoder launch -- is checked stage by stage too)"""
    cover = set()
    for nl, npano, B, attn_mode, with_dP in BWD_CASES:
        tag = f"{dtype} p={p} text {nl} / pano {npano} layers, B={B}, RBW_ATTN_MODE={attn_mode}, dP_init={with_dP}"
        with monkeypatch.context() as mp:
            m, segs, fmts, tops, dPs, dx, seed, sync, _ = run_self_stacks(dtype, p, nl, npano, B, attn_mode, with_dP, mp, cover)
            if B == 48:
                want = enc_form([(s.ns, s.N) for s in segs], ncu())
                assert want == "mixed" and sync is not None and form_matches(observed_form(sync, segs), want, 2), (want, sync[:24].tolist())
                for i, sg in enumerate(segs):
                    check_segment(sg, p, seed, f"engine B=48 seg {i}", H, NH, I)
            for i, sg in enumerate(segs):
                rdx, rw = stack_reference(sg, p, seed, tops[i], dPs[i], H, NH)
                check_param_grads(m, fmts[i], sg, rw, dtype, f"{tag} stack {i}", H)
                check_dx_tiles(dx[i], rdx, sg, dtype, f"{tag} stack {i}", H)
    # (mode, rows, with_dist | dP_init, kt)
    need = {(0, 16, False, 0), (0, 16, False, 12), (0, 32, False, 0), (0, 32, False, 12), (1, 16, False, None), (2, 16, False, None),
            (1, 16, True, None)}
    assert need <= cover, f"rowbwd forms not reached: {sorted(need - cover, key=str)} (reached {sorted(cover, key=str)})"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_backward_bounds_catch_planted_defects(dtype, monkeypatch):
    """applied to copies of the kernel's result, each must fail: the largest workgroup's partial LayerNorm row left out of a dgamma, and
    one 16-row tile of the input gradient taken from the neighbouring sample"""
    kept = dict(STATS)
    cover = set()
    m, segs, fmts, tops, dPs, dx, seed, _, jobs = run_self_stacks(dtype, 0.0, 2, 1, 6, 0, False, monkeypatch, cover)
    sg = segs[0]
    rdx, rw = stack_reference(sg, 0.0, seed, tops[0], None, H, NH)
    check_param_grads(m, fmts[0], sg, rw, dtype, "clean", H)
    check_dx_tiles(dx[0], rdx, sg, dtype, "clean", H)
    # dgamma of the top block's output LayerNorm: its partial rows (one per workgroup) are still in the buffer the flush summed
    dst = m.net.ln(fmts[0].format(1) + "output.LayerNorm").dg
    part, nblk = next((pt, k) for pt, d, k in jobs if d.data_ptr() == dst.data_ptr())
    rows = part.view(nblk, -1).double().cpu()
    bad = m.store.grad.clone()
    off, cnt, _ = m.store.offsets[fmts[0].format(1) + "output.LayerNorm.weight"]
    bad[off:off + cnt] -= rows[rows.norm(dim=1).argmax()].to(bad)
    with pytest.raises(AssertionError):
        check_param_grads(m, fmts[0], sg, rw, dtype, "dgamma without one workgroup", H, grad=bad)
    t = dx[0].clone().view(sg.ns, sg.N, H)
    t[1, :16] = t[2, :16]
    with pytest.raises(AssertionError):
        check_dx_tiles(t, rdx, sg, dtype, "tile from the neighbouring sample", H)
    STATS.clear()
    STATS.update(kept)


def test_zz_report_measured_worst():
    """prints (with -s) the worst error per stage and storage type that this process measured (what BOUNDS / RSTD_REL were set from)"""
    for key in sorted(STATS):
        u, f = STATS[key]
        print(f"fp64 stage check {key[0]:5s} {key[1]:22s} worst {u:10.4g}  floor needed {f:8.4f}")
