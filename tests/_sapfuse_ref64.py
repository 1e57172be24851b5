"""Float64 references, bounds and the case table of the SAP action-logit fusion (csrc/graphops.hip: magic_sap_fuse_fwd, magic_sap_fuse_loss,
magic_sap_fuse_bwd).

For tests/test_sapfuse_fp64_gpu.py (the kernels) and tests/test_sapfuse_ref64_cpu.py (every closed form here against plain float64 autograd of the
oracle composition, the planners' contract, the fp32 emulation, the planted defects).  Nothing here launches a kernel.  REL, bound, check, ratio,
f32, ce_ref, kd_ref and WORST are those of tests/_loss_ref64.py.

Problems are generated from VIEWPOINT LISTS (map tokens [stop] ([mem]) visited.. unvisited.., local tokens [stop] ([mem]) candidates..
non-navigable views..), not from index arrays: the reference fused logits of those samples come from oracle.model_ref.fuse_logits itself, in
float64, and fsrc / the back-track mask come from the planners (host/nav_plan.py fusion_map, host/model_nav.py nav_fusion_plan: equal element for
element).  Rows the planners cannot produce but the kernel contract allows are hand-made (hand_sample) and take the dense form fl = gl + F ll.

Stage by stage (the rule of tests/test_encoder_fp64_gpu.py): stage 1 (gl, ll, fl) from the raw logits as stored; stage 2 (rows, dgl, dll, dfl, w_out,
kd_rows) from the kernel's OWN stored gl / ll / fl (and its own stored w_out inside the distillation rows); the backward from dgl / dll / dfl as
passed.  Bound: REL = 1e-5 of the envelope (sum of the absolute terms), factor 1 everywhere.  One absolute term is added wherever the kernel
multiplies by 1 - fw: it forms 1 - fw from the ROUNDED fp32 fw, so that factor is off by up to half a unit in the last place of 1 (2^-24) whatever
its size -- with fuse_raw = 20 the fp32 gate is exactly 1 and 1 - fw is 0 where the true value is 2e-9.  That is fp32's own limit, derived, not
measured: 2^-23 |l_raw| for ll (and through it fl), 2^-23 sum|terms of d| for dl_raw, 2^-23 sum|terms| for dfuse_raw.  Without it no fp32 kernel
holds the saturated-gate case.

Not covered on purpose: the GRADIENT the distillation part writes at a slot whose student logit is -inf while the teacher's is finite (the kernel
writes -coef w T p_t there, float64 autograd of the oracle gives 0: the -1e6 stand-in is a constant).  The teacher carries the student's masks and
the backward drops masked tokens, so nothing reads that slot; the case that opens the teacher at a masked slot (`t_open`, for the -inf -> -1e6 rule
of the ROWS) runs the option sets without gradient buffers only.

Largest err / bound per output on an MI355X (test_zz_report of tests/test_sapfuse_fp64_gpu.py, one run of that file, factor 1 throughout):
  gl 0.018   ll 0.055   fl 0.031   rows 0.013   dgl 0.019   dll 0.019   dfl 0.018   w_out 0.0053   kd_rows 0.030
  dg_raw 0.019   dl_raw 0.056   dfuse_raw 0.026
  the separate launches the fused loss replaces (ce_rows, kd_rows) under the identical stage-2 check, same inputs:
  rows 0.013   dgl 0.019   dll 0.017   dfl 0.017   w_out 0.0053   kd_rows 0.030
The fp32 emulation below (plain torch fp32 on the CPU) stays under 0.5 on every output (asserted in tests/test_sapfuse_ref64_cpu.py; its own worst
figure is 0.056, on dl_raw)."""
from types import SimpleNamespace

import numpy as np
import torch

from tests._loss_ref64 import REL, WORST, bound, ce_ref, check, f32, kd_ref

NEG = float("-inf")
EPS32 = 2.0 ** -23
BIG = 1e4                                                 # raw logits at masked positions: a leak is worth many bounds
T_KD, W_RATE, KD_COEF, CE_COEF = 2.0, 0.7, 0.23, 0.37     # (CE_COEF is divided by B)
MEM = "[mem]"                                             # the [mem] local token in the oracle's candidate list: a name no map holds


def sap_fused_rule(K, Vp):
    """host/heads.py: the logit fusion rides in the loss launch only for K <= 512 and Vp <= 128"""
    return K <= 512 and Vp <= 128


# ------------------------------------------------------------------------------------------ case table
def case(name, B, K, Vp, mem, gate, hand=2, loss=True, fuse=None, all_local_ignored=False, t_open=False):
    return SimpleNamespace(name=name, B=B, K=K, Vp=Vp, mem=mem, gate=gate, hand=hand if (K >= 4 and Vp >= 5) else 0, loss=loss and sap_fused_rule(K, Vp),
                           fuse=fuse, all_local_ignored=all_local_ignored, t_open=t_open)


# B counts the generated samples; `hand` hand-made samples follow them (B + hand <= 5)
CASES = [
    case("K1-Vp1", 1, 1, 1, False, True),                                  # one token each: every loop runs one lane once, CE rows are 0
    case("K2-Vp2", 3, 2, 2, False, False),                                 # K = 2: the three fsrc kinds over three samples; gate off
    case("K1-Vp37", 2, 1, 37, False, True),                                # K = 1 beside a full local row
    case("K63-Vp37-mem", 3, 63, 37, True, True),                           # one lane short of the wave, [mem] in both rows
    case("K64-Vp64", 3, 64, 64, False, False),                             # exactly one turn of both loops, gate off
    case("K65-Vp37-saturated", 4, 65, 37, True, True, hand=1, fuse=[20.0, -20.0, 90.0, -90.0, 20.0]),   # second turn by one token; fw = 0 / 1
    case("K130-Vp65-mem", 3, 130, 65, True, True),                         # third turn of the K loop, second turn of the Vp loop by one view (j = 64)
    case("K65-Vp128-off", 3, 65, 128, True, False),                        # full LDS row, gate off
    case("K512-Vp128", 2, 512, 128, False, True),                          # all 8 slots of the distillation ring, full LDS rows
    case("K5-Vp6-all-local-ignored", 3, 5, 6, False, True, all_local_ignored=True),
    case("K37-Vp37-teacher-open", 3, 37, 37, True, True, hand=0, t_open=True),     # the -inf -> -1e6 rule of the distillation rows
    case("K513-Vp37", 2, 513, 37, True, True, loss=False),                 # past the fused loss's K limit: forward and backward only
    case("K700-Vp128", 2, 700, 128, False, False, loss=False),             # eleven turns
]

# option sets of the fused loss: which gradient buffers, w_out, kd_rows, kd_coef_dev, the dynamic loss scale
OPTS = [
    dict(name="eval", grads=()),
    dict(name="grads", grads=("dgl", "dll", "dfl")),
    dict(name="grads-scaled", grads=("dgl", "dll", "dfl"), scale=4096.0),
    dict(name="w_out", grads=("dgl", "dll", "dfl"), w=True),
    dict(name="kd_rows", grads=("dgl", "dll", "dfl"), kd=True),
    dict(name="kd_rows-dev", grads=("dgl", "dll", "dfl"), kd=True, dev=1.7),
    dict(name="both", grads=("dgl", "dll", "dfl"), w=True, kd=True, dev=1.7),
    dict(name="both-scaled", grads=("dgl", "dll", "dfl"), w=True, kd=True, dev=1.7, scale=4096.0),
    dict(name="both-dfl-only", grads=("dfl",), w=True, kd=True),
    dict(name="both-eval", grads=(), w=True, kd=True, dev=1.7),
    dict(name="both-eval-scaled", grads=(), w=True, kd=True, scale=4096.0),
]
SUBSETS = [("dgl",), ("dll",), ("dfl",), ("dgl", "dll"), ("dgl", "dfl"), ("dll", "dfl"), ("dgl", "dll", "dfl")]


def opt(o):
    return SimpleNamespace(**dict(dict(grads=(), w=False, kd=False, dev=None, scale=1.0), **o))


def opts_of(c):
    return [o for o in OPTS if not (c.t_open and o["grads"])]


# ------------------------------------------------------------------------------------------ problems
def _gen_sample(rng, b, K, Vp, mem):
    """viewpoint lists of one sample: map tokens, their visited mask, local tokens (viewpoint of each candidate slot, None elsewhere), candidates"""
    base = 2 if mem else 1
    nfree, mfree = K - base, Vp - base
    style = b % 3                                          # 0: full row; 1: shown-heavy; 2: EMPTY back-track set
    n_nodes = nfree if b == 0 else int(rng.integers((nfree + 1) // 2, nfree + 1))
    nv = 0 if n_nodes == 0 else ((1 if style == 0 else 0) if n_nodes == 1 else max(1, n_nodes // 3))
    n_unv = n_nodes - nv
    max_c = mfree if b == 0 else int(rng.integers((mfree + 1) // 2, mfree + 1))
    back_t = 0 if (style == 2 or max_c == 0) else (min(nv, max(1, max_c // 3)) if max_c >= 2 else (1 if style == 0 else 0))
    showable = n_unv - 1 if n_unv > 1 else (n_unv if style != 2 else 0)
    n_shown = max(0, min(showable, max_c - back_t))
    n_back = 0 if style == 2 else min(nv, max_c - n_shown)
    vis = [f"s{b}v{i}" for i in range(nv)]
    unv = [f"s{b}u{i}" for i in range(n_unv)]
    shown_ix = set()
    if n_shown:
        shown_ix.add(n_unv - 1)                            # the LAST unvisited token is shown, the one before it is not: k >= 64 holds both kinds
        pool = [i for i in range(n_unv - 2)] if n_unv >= 2 else []
        extra = rng.permutation(len(pool))[:n_shown - 1].tolist()
        shown_ix.update(pool[i] for i in extra)
    shown = [unv[i] for i in sorted(shown_ix)]
    back = [vis[i] for i in rng.permutation(nv)[:n_back].tolist()]
    shown = [shown[i] for i in rng.permutation(len(shown)).tolist()]
    cands = back + shown                                   # even samples: back-track views first, so the shown ones reach the last local slots
    if b % 2 and len(cands) > 1:
        cands = [cands[i] for i in rng.permutation(len(cands)).tolist()]
    head = [None, None] if mem else [None]
    vpids = head + vis + unv
    visited = ([False, True] if mem else [False]) + [True] * nv + [False] * n_unv          # [mem] counts as visited (host/nav_plan.py)
    local = head + cands + [None] * (Vp - base - len(cands))
    return vpids, visited, local, cands


def hand_sample(K, Vp, variant):
    """rows the planners cannot write but the kernel contract allows.  variant 0: a back-track view with lmask = 0 beside a live one (the masked one
    is skipped); variant 1: fsrc = -2 with NO back-track view (adds 0).  Both: a global token with gmask = 0 whose source is live (k = 1, and
    k = K - 1 where K > 64), a live global token whose local source is masked (fl = -inf)"""
    fsrc = np.full(K, -1, np.int32)
    gmask, lmask, bw = np.zeros(K, np.uint8), np.zeros(Vp, np.uint8), np.zeros(Vp, np.uint8)
    gmask[0] = lmask[0] = 1
    fsrc[0] = 0
    lmask[2] = 1                                           # live local view
    lmask[4] = 1
    if variant == 0:
        bw[1] = 1                                          # back-track view, masked: skipped
        bw[4] = 1                                          # back-track view, live
    fsrc[1], gmask[1] = 2, 0                               # masked global token, live source
    fsrc[2], gmask[2] = -2, 1
    fsrc[3], gmask[3] = 3, 1                               # live global token, masked source: fl = -inf
    for k in range(4, K):
        gmask[k] = k % 2
        fsrc[k] = (-1, -2, 2, 4)[k % 4]
    if K > 64:
        lmask[Vp - 1] = 1
        fsrc[K - 1], gmask[K - 1] = Vp - 1, 0              # masked global token past the first turn, live source (past j = 64 where Vp > 64)
        fsrc[K - 2], gmask[K - 2] = Vp - 1, 1
    return fsrc, gmask, lmask, bw


def planners(P):
    """fsrc / back-track mask of the generated samples from both Python planners (host/nav_plan.py fusion_map, host/model_nav.py nav_fusion_plan)"""
    import magic_amd  # noqa: F401
    from magic_amd.host.model_nav import nav_fusion_plan
    from magic_amd.host.nav_plan import fusion_map
    n, K, Vp = P.n_gen, P.K, P.Vp
    vm = torch.zeros(n, K, dtype=torch.bool)
    for b in range(n):
        vm[b, :len(P.visited[b])] = torch.tensor(P.visited[b])
    return fusion_map(P.vpids, P.visited, P.local, K, Vp), nav_fusion_plan(P.vpids, vm, P.local, K, Vp)


def assert_contract(fsrc, bw, gmask, lmask, cand_slots=None):
    """what the kernels rely on unchecked: fsrc[:, 0] = 0, every entry -2, -1 or in [0, Vp); back-track bits on candidate slots only; [stop] open"""
    fsrc, bw = np.asarray(fsrc), np.asarray(bw)
    Vp = bw.shape[1]
    assert fsrc.dtype == np.int32 and bw.dtype == np.uint8
    assert (fsrc[:, 0] == 0).all(), "fsrc[:, 0] != 0"
    assert ((fsrc >= -2) & (fsrc < Vp)).all(), "fsrc outside {-2, -1} and [0, Vp)"
    assert (np.asarray(gmask)[:, 0] != 0).all() and (np.asarray(lmask)[:, 0] != 0).all(), "[stop] masked: a wholly masked row is outside the kernels' contract"
    if cand_slots is not None:
        assert not (bw.astype(bool) & ~np.asarray(cand_slots, bool)).any(), "back-track bit outside the candidate slots"
        assert not ((fsrc[:, 1:] >= 0) & ~np.take_along_axis(np.asarray(cand_slots, bool), fsrc[:, 1:].clip(min=0), 1)).any(), "fsrc names a slot that is no candidate"


def problem(c):
    """the inputs of one case (CPU tensors in the kernels' types) and the lists they were made from"""
    rng = np.random.default_rng(c.K * 1009 + c.Vp * 31 + c.B)
    g = torch.Generator().manual_seed(c.K * 7919 + c.Vp)
    n, B, K, Vp = c.B, c.B + c.hand, c.K, c.Vp
    P = SimpleNamespace(B=B, K=K, Vp=Vp, n_gen=n, mem=c.mem, vpids=[], visited=[], local=[], cands=[])
    for b in range(n):
        v, m, loc, cd = _gen_sample(rng, b, K, Vp, c.mem)
        P.vpids.append(v); P.visited.append(m); P.local.append(loc); P.cands.append(cd)
    fsrc, bw = np.full((B, K), -1, np.int32), np.zeros((B, Vp), np.uint8)
    gmask, lmask = np.zeros((B, K), np.uint8), np.zeros((B, Vp), np.uint8)
    cand_slots = np.zeros((n, Vp), bool)
    for b in range(n):
        gmask[b, :len(P.vpids[b])] = ~np.array(P.visited[b])
        cand_slots[b] = [x is not None for x in P.local[b]]
        lmask[b] = cand_slots[b]
        lmask[b, 0] = 1
    (f1, b1), (f2, b2) = planners(P)
    assert np.array_equal(f1, f2) and np.array_equal(b1, b2), "fusion_map and nav_fusion_plan disagree"
    assert_contract(f1, b1, gmask[:n], lmask[:n], cand_slots)
    fsrc[:n], bw[:n] = f1, b1
    for h in range(c.hand):
        fsrc[n + h], gmask[n + h], lmask[n + h], bw[n + h] = hand_sample(K, Vp, h)
    assert_contract(fsrc, bw, gmask, lmask)
    P.cand_slots = cand_slots
    P.fsrc, P.bw, P.gmask, P.lmask = torch.from_numpy(fsrc), torch.from_numpy(bw), torch.from_numpy(gmask), torch.from_numpy(lmask)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)

    def raw(mask, N):
        x = 2 * rn(B, N)
        sign = 1.0 - 2.0 * (torch.arange(N) % 2).double()
        x = torch.where(mask.bool(), x, BIG * sign.expand(B, N))
        x[:, N - 1] = torch.where(mask[:, N - 1].bool(), torch.full((B,), 3.0, dtype=torch.float64), x[:, N - 1])     # a live last column carries weight
        return x.float()
    P.g_raw, P.l_raw = raw(P.gmask, K), raw(P.lmask, Vp)
    P.fuse_raw = (1.5 * rn(B) + 0.3).float() if c.fuse is None else torch.tensor(c.fuse[:B], dtype=torch.float32)
    pick = lambda mask, b: int(mask[b].nonzero().flatten()[int(rng.integers(0, int(mask[b].sum())))])
    glab = [K + 3 if b % 4 == 2 else pick(P.gmask, b) for b in range(B)]                 # out of range counts as ignored
    llab = [-100 if b % 3 == 1 else pick(P.lmask, b) for b in range(B)]
    if c.all_local_ignored:
        llab = [(-100, Vp + 2)[b % 2] for b in range(B)]
    if B > 1 and P.gmask[0, K - 1]:
        glab[0] = K - 1                                    # the label on the last column once
    P.glab, P.llab = torch.tensor(glab, dtype=torch.int32), torch.tensor(llab, dtype=torch.int32)
    fl = stage1_ref(P, c.gate)["fl"]
    for b in range(n):                                     # labels stay off -inf logits (a fused logit is -inf only where hand-made)
        assert glab[b] >= K or fl[b, glab[b]] > NEG
    for b in range(n, B):
        if glab[b] < K and fl[b, glab[b]] == NEG:
            P.glab[b] = 0
    t = (2 * rn(B, K)).float()
    t[fl == NEG] = NEG                                     # the teacher carries the student's masks
    if c.t_open:
        for b in range(B):
            k = int((fl[b] == NEG).nonzero().flatten()[0])
            t[b, k] = 1.0                                  # ... except here: the student's -inf meets a finite teacher logit
    P.t_fused = t
    return P


_PROBLEMS = {}


def get(c):
    if c.name not in _PROBLEMS:
        _PROBLEMS[c.name] = problem(c)
    return _PROBLEMS[c.name]


def coverage(c, P):
    """what the case's index arrays hold, and what its K / Vp make possible (so must hold)"""
    n, K, Vp = P.n_gen, P.K, P.Vp
    base = 2 if c.mem else 1
    f, gm, lm, bw = P.fsrc.numpy(), P.gmask.numpy().astype(bool), P.lmask.numpy().astype(bool), P.bw.numpy().astype(bool)
    k = np.arange(K)[None]
    src_live = np.take_along_axis(lm, f.clip(min=0), 1) & (f >= 0)
    have = dict(kind_src=bool((f[:, 1:] >= 0).any()), kind_none=bool((f == -1).any()), kind_back=bool((f == -2).any()),
                k64_src=bool(((f >= 0) & (k >= 64) & gm).any()), k64_back=bool(((f == -2) & (k >= 64) & gm).any()), j64_src=bool(((f >= 64) & gm).any()),
                empty_back=bool((~(bw & lm).any(1)).any()), masked_live=bool((~gm & src_live)[:, 1:].any()), no_masked_row=bool(gm.any(1).all() and lm.any(1).all()),
                last_g=bool(gm[:, K - 1].any()), last_l=bool(lm[:, Vp - 1].any()))
    nfree, mfree = K - base, Vp - base
    need = dict(kind_src=nfree >= 1 and mfree >= 1, kind_none=K >= 2, kind_back=nfree >= 1, k64_src=K >= 65 and mfree >= 1, k64_back=K >= 66,
                j64_src=Vp > 64 and nfree - 1 >= mfree, empty_back=True, masked_live=c.hand > 0, no_masked_row=True, last_g=K >= 2, last_l=False)
    return have, need


# ------------------------------------------------------------------------------------------ stage 1: gl, ll, fl
def dense_add(ll, fsrc, bw, lmask):
    """what fl adds to gl: ll[fsrc] | the back-track views' sum over live views (fsrc = -2) | 0 -- differentiable, -inf where the source is masked"""
    zero = torch.zeros_like(ll[:, :1])
    src = ll.gather(1, fsrc.clamp(min=0).long())
    live = bw.bool() & lmask.bool()
    bsum = torch.where(live, ll, zero.expand_as(ll)).sum(1, keepdim=True)
    return torch.where(fsrc >= 0, src, torch.where(fsrc == -2, bsum.expand_as(src), zero.expand_as(src)))


def oracle_fuse(gl, ll, P):
    """oracle.model_ref.fuse_logits on the generated samples' own lists (never on fsrc)"""
    from oracle import model_ref
    n = P.n_gen
    batch = dict(gmap_visited_masks=P.visited, gmap_vpids=P.vpids, traj_cand_vpids=[[([MEM] if P.mem else []) + P.cands[b]] for b in range(n)])
    return model_ref.fuse_logits(gl[:n], ll[:n], batch)


def gate(P, use_gate):
    """fw and 1 - fw in float64 from the stored fp32 fuse_raw (1 - sigmoid(x) = sigmoid(-x): no cancellation)"""
    x = P.fuse_raw.double()
    if not use_gate:
        return torch.full_like(x, 0.5), torch.full_like(x, 0.5)
    return torch.sigmoid(x), torch.sigmoid(-x)


def stage1_ref(P, use_gate):
    fw, omf = gate(P, use_gate)
    g, l = P.g_raw.double(), P.l_raw.double()
    gm, lm = P.gmask.bool(), P.lmask.bool()
    ninf_g, ninf_l, zg, zl = torch.full_like(g, NEG), torch.full_like(l, NEG), torch.zeros_like(g), torch.zeros_like(l)
    gl = torch.where(gm, g * fw[:, None], ninf_g)
    ll = torch.where(lm, l * omf[:, None], ninf_l)
    gl_env = torch.where(gm, g.abs() * fw[:, None], zg)
    ll_env = torch.where(lm, l.abs() * omf[:, None] + (EPS32 / REL) * l.abs(), zl)            # + 2^-23 |l_raw|: 1 - fw from a rounded fw
    fl = gl + dense_add(ll, P.fsrc, P.bw, P.lmask)
    if P.n_gen:
        fl[:P.n_gen] = oracle_fuse(gl, ll, P)
    fl_env = gl_env + dense_add(ll_env, P.fsrc, P.bw, P.lmask)
    fl_env = torch.where(fl == NEG, zg, fl_env)
    return dict(gl=gl, ll=ll, fl=fl, gl_env=gl_env, ll_env=ll_env, fl_env=fl_env)


# ------------------------------------------------------------------------------------------ stage 2: rows, gradients, w_out, kd_rows
def constants(P, o):
    """the scalars as the fp32 the C ABI carries; norm as host/heads.py sets it"""
    B, K = P.B, P.K
    norm = 1.0 / B if o.w else 1.0 / (B * K)
    return SimpleNamespace(coef=CE_COEF / B, T=T_KD, rate=W_RATE, kd_coef=KD_COEF, norm=norm)


def stage2_ref(P, o, gl, ll, fl, w_stored=None):
    """from the logits as STORED (fp32 tensors): CE rows and gradients through ce_ref, w_out through ce_ref on the teacher's logits, distillation rows
    and the gradient ADDED to dfl through kd_ref (w = the stored w_out where hard mining is on).  The loss scale multiplies gradients only."""
    k = constants(P, o)
    coef = f32(k.coef) * o.scale
    cg, cl, cf = ce_ref(gl, P.glab, coef), ce_ref(ll, P.llab, coef), ce_ref(fl, P.glab, coef)
    out = dict(rows=torch.stack([cg["loss"], cl["loss"], cf["loss"]]), rows_env=torch.stack([cg["loss_env"], cl["loss_env"], cf["loss_env"]]),
               dgl=cg["grad"], dgl_env=cg["grad_env"], dll=cl["grad"], dll_env=cl["grad_env"], dfl=cf["grad"], dfl_env=cf["grad_env"], dfl_ce=cf["grad"])
    if o.w:
        cw = ce_ref(P.t_fused, P.glab, 0.0, w_rate=f32(k.rate))
        out.update(w=cw["w"], w_env=cw["w_env"])
    if o.kd:
        w = None
        if o.w:
            w = out["w"] if w_stored is None else w_stored.double()
        kc = f32(k.kd_coef) * (f32(o.dev) if o.dev is not None else 1.0) * o.scale
        rows, renv, grad, genv = kd_ref(fl, P.t_fused, f32(k.T), w=w, norm=f32(k.norm), coef=kc)
        out.update(kd=rows, kd_env=renv, dfl=out["dfl"] + grad, dfl_env=out["dfl_env"] + genv, kd_grad=grad)
    return out


def ce_last_col_ctrl(x, lab, coef):
    """the CE reference without the row's last column (None where nothing would be left or the last column is -inf everywhere)"""
    N = x.shape[1]
    if N == 1 or not (x[:, N - 1] > NEG).any():
        return None
    c = ce_ref(x[:, :N - 1], lab, coef)
    c["grad"] = torch.cat([c["grad"], torch.zeros_like(c["grad"][:, :1])], 1)
    return c


# ------------------------------------------------------------------------------------------ backward
def bwd_ref(P, use_gate, dgl, dll, dfl, drop=None):
    """dg_raw = gmask (dgl + dfl) fw; dl_raw = lmask (dll + sum_{k live, fsrc[k] = j} dfl[k] + bw[j] sum_{k live, fsrc[k] = -2} dfl[k]) (1 - fw);
    dfuse_raw = fw (1 - fw) (sum dg g_raw - sum d l_raw), exactly 0 without the gate.  drop (a missing unit): 'last' -- the last live global token
    that has a live source, 'back' -- the back-track term, 'local' -- the local half of dfuse_raw"""
    fw, omf = gate(P, use_gate)
    B, K, Vp = P.B, P.K, P.Vp
    g, l = P.g_raw.double(), P.l_raw.double()
    gm, lm, bw = P.gmask.bool(), P.lmask.bool(), P.bw.bool()
    z = lambda t, N: torch.zeros(B, N, dtype=torch.float64) if t is None else t.double()
    a, c_, f = z(dgl, K), z(dll, Vp), z(dfl, K)
    f = torch.where(gm, f, torch.zeros_like(f))
    a = torch.where(gm, a, torch.zeros_like(a))
    dg, dg_abs = a + f, a.abs() + f.abs()
    fs = f.clone()
    if drop == "last":
        hit = False
        for b in range(B):
            src_ok = torch.where(P.fsrc[b] >= 0, lm[b][P.fsrc[b].clamp(min=0).long()], (P.fsrc[b] == -2) & bool((bw[b] & lm[b]).any()))
            ks = (gm[b] & src_ok & (fs[b] != 0)).nonzero().flatten()
            if len(ks):
                fs[b, ks[-1]] = 0.0
                hit = True
        if not hit:
            return None
    idx = P.fsrc.clamp(min=0).long()
    S = torch.zeros(B, Vp, dtype=torch.float64).scatter_add(1, idx, torch.where(P.fsrc >= 0, fs, torch.zeros_like(fs)))
    Sabs = torch.zeros(B, Vp, dtype=torch.float64).scatter_add(1, idx, torch.where(P.fsrc >= 0, fs.abs(), torch.zeros_like(fs)))
    back = torch.where(P.fsrc == -2, fs, torch.zeros_like(fs)).sum(1, keepdim=True)
    back_abs = torch.where(P.fsrc == -2, fs.abs(), torch.zeros_like(fs)).sum(1, keepdim=True)
    if drop == "back":
        if not (bw & lm & (back != 0)).any():
            return None
        back = torch.zeros_like(back)
    d = torch.where(lm, c_ + S + bw * back, torch.zeros_like(c_))
    d_abs = torch.where(lm, c_.abs() + Sabs + bw * back_abs, torch.zeros_like(c_))
    dg_raw, dl_raw = dg * fw[:, None], d * omf[:, None]
    sg, sl_ = (dg * g).sum(1), (d * l).sum(1)
    if drop == "local":
        if not use_gate:
            return None
        sl_ = torch.zeros_like(sl_)
    sabs = (dg_abs * g.abs()).sum(1) + (d_abs * l.abs()).sum(1)
    df = fw * omf * (sg - sl_) if use_gate else torch.zeros(B, dtype=torch.float64)
    df_env = (fw * omf + (EPS32 / REL) * fw) * sabs if use_gate else torch.zeros(B, dtype=torch.float64)       # + 2^-23: 1 - fw from a rounded fw
    return dict(dg=dg_raw, dg_env=dg_abs * fw[:, None], dl=dl_raw, dl_env=d_abs * (omf[:, None] + EPS32 / REL), df=df, df_env=df_env)


def upstream(P, seed=0):
    """dgl, dll, dfl as a caller might pass them: noise, and LARGE values at masked positions (the kernel must drop them)"""
    g = torch.Generator().manual_seed(1000 + seed + P.K)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    dgl, dll, dfl = rn(P.B, P.K), rn(P.B, P.Vp), rn(P.B, P.K)
    dgl[~P.gmask.bool()] = 1e3
    dfl[~P.gmask.bool()] = -1e3
    dll[~P.lmask.bool()] = 1e3
    return dict(dgl=dgl.float(), dll=dll.float(), dfl=dfl.float())


# ------------------------------------------------------------------------------------------ comparisons
class Run:
    """the comparisons of one output set.  strict: assert; else collect the failures (the planted defects).  fam: prefix of the WORST keys"""

    def __init__(self, fam="sap", strict=True):
        self.fam, self.strict, self.fails, self.units = fam, strict, [], {}

    def chk(self, out, name, got, ref, env, ctrl=None):
        """ctrl: {missing unit: the reference without it}.  A control is asserted where the unit is worth more than 4 bounds in the REFERENCES (never
        judged from `got`); self.units counts the assertions per unit, so that a unit no case can see is noticed (tests/test_sapfuse_ref64_cpu.py)"""
        try:
            got = got.detach().cpu()
            assert torch.equal(got == NEG, ref == NEG), f"{name}: -inf positions differ"
            fin = lambda t: torch.where(ref == NEG, torch.zeros_like(t.double()), t.double())
            bnd = bound(fin(ref), env)
            cs = []
            for unit, c in (ctrl or {}).items():
                if c is not None and ((fin(c) - fin(ref)).abs() > 4 * bnd).any():
                    cs.append(fin(c))
                    self.units[unit] = self.units.get(unit, 0) + 1
            check(f"{self.fam} {out}", name, fin(got), fin(ref), env, ctrl=cs or None)
        except AssertionError as e:
            if self.strict:
                raise
            self.fails.append(f"{name}: {e}")

    def exact(self, name, ok):
        if not ok:
            if self.strict:
                raise AssertionError(name)
            self.fails.append(name)


def verify_stage1(run, tag, P, use_gate, gl, ll, fl):
    r = stage1_ref(P, use_gate)
    run.chk("gl", f"gl {tag}", gl, r["gl"], r["gl_env"])
    run.chk("ll", f"ll {tag}", ll, r["ll"], r["ll_env"])
    run.chk("fl", f"fl {tag}", fl, r["fl"], r["fl_env"])


def verify_stage2(run, tag, P, o, gl, ll, fl, got):
    """got: dict of the outputs that the option set asks for (rows, dgl, dll, dfl, w, kd); gl / ll / fl: the logits the rows were computed from"""
    gl, ll, fl = gl.detach().cpu(), ll.detach().cpu(), fl.detach().cpu()
    w_st = got["w"].detach().cpu() if o.w else None
    r = stage2_ref(P, o, gl, ll, fl, w_st)
    k = constants(P, o)
    coef = f32(k.coef) * o.scale
    ctrls = [ce_last_col_ctrl(gl, P.glab, coef), ce_last_col_ctrl(ll, P.llab, coef), ce_last_col_ctrl(fl, P.glab, coef)]
    for i, nm in enumerate(("global", "local", "fused")):
        c = ctrls[i]
        run.chk("rows", f"rows[{nm}] {tag}", got["rows"][i], r["rows"][i], r["rows_env"][i], ctrl={"last CE column": c and c["loss"]})
    for i, nm in enumerate(("dgl", "dll")):
        if nm in o.grads:
            c = ctrls[i]
            run.chk(nm, f"{nm} {tag}", got[nm], r[nm], r[nm + "_env"], ctrl={"last CE column": c and c["grad"]})
    if "dfl" in o.grads:
        cs = {"distillation gradient": r["dfl_ce"]} if o.kd else {"last CE column": ctrls[2] and ctrls[2]["grad"]}
        run.chk("dfl", f"dfl {tag}", got["dfl"], r["dfl"], r["dfl_env"], ctrl=cs)
    if o.w:
        run.chk("w_out", f"w_out {tag}", got["w"], r["w"], r["w_env"])
    if o.kd:
        run.chk("kd_rows", f"kd_rows {tag}", got["kd"], r["kd"], r["kd_env"])


def verify_bwd(run, tag, P, use_gate, up, dg, dl, df):
    r = bwd_ref(P, use_gate, up.get("dgl"), up.get("dll"), up.get("dfl"))
    c = {d: bwd_ref(P, use_gate, up.get("dgl"), up.get("dll"), up.get("dfl"), drop=d) for d in ("last", "back", "local")}
    pick = lambda d, key: c[d] and c[d][key]
    run.chk("dg_raw", f"dg_raw {tag}", dg, r["dg"], r["dg_env"])
    run.chk("dl_raw", f"dl_raw {tag}", dl, r["dl"], r["dl_env"], ctrl={"last global token in dl_raw": pick("last", "dl"), "back-track term": pick("back", "dl")})
    run.chk("dfuse_raw", f"dfuse_raw {tag}", df, r["df"], r["df_env"], ctrl={"local half of dfuse_raw": pick("local", "df")})
    masked_zero = bool((dg.detach().cpu()[~P.gmask.bool()] == 0).all() and (dl.detach().cpu()[~P.lmask.bool()] == 0).all())
    run.exact(f"masked positions exactly zero {tag}", masked_zero)
    if not use_gate:
        run.exact(f"dfuse_raw exactly 0 without the gate {tag}", bool((df.detach().cpu() == 0).all()))


# ------------------------------------------------------------------------------------------ the same mathematics in plain fp32 (CPU) -- with planted defects
F32 = torch.float32


def _gate32(P, use_gate, defect):
    if use_gate or defect == "gate_when_off":
        fw = torch.sigmoid(P.fuse_raw)
    else:
        fw = torch.full_like(P.fuse_raw, 0.5)
    return fw, 1.0 - fw


def emu_stage1(P, use_gate, defect=None):
    fw, omf = _gate32(P, use_gate, defect)
    gm, lm = P.gmask.bool(), P.lmask.bool()
    gl = torch.where(gm, P.g_raw * fw[:, None], torch.full_like(P.g_raw, NEG))
    ll = torch.where(lm, P.l_raw * omf[:, None], torch.full_like(P.l_raw, NEG))
    fsrc = P.fsrc
    if defect == "m2_as_m1":
        fsrc = torch.where(fsrc == -2, torch.full_like(fsrc, -1), fsrc)
    add = dense_add(ll, fsrc, P.bw, torch.ones_like(P.lmask) if defect == "bw_ignores_lmask" else P.lmask)
    fl = gl + add
    if defect == "drop_k64":                               # tokens of the second turn never written (buffers start at zero)
        gl, fl = gl.clone(), fl.clone()
        gl[:, 64:], fl[:, 64:] = 0.0, 0.0
    return gl, ll, fl


def _ce32(x, lab, coef, defect_keep=False):
    N = x.shape[1]
    lab = lab.long()
    ign = (lab == -100) | (lab < 0) | (lab >= N)
    safe = torch.where(ign, torch.zeros_like(lab), lab)
    lse = torch.logsumexp(x, 1)
    loss = torch.where(ign, torch.zeros_like(lse), lse - x.gather(1, safe[:, None])[:, 0])
    hot = torch.zeros_like(x)
    hot[torch.arange(x.shape[0])[~ign], safe[~ign]] = 1.0
    cf = torch.where(ign & (not defect_keep), torch.zeros_like(lse), torch.full_like(lse, coef))
    return loss, cf[:, None] * (torch.exp(x - lse[:, None]) - hot)


def emu_stage2(P, o, gl, ll, fl, defect=None):
    k = constants(P, o)
    sc = torch.tensor(o.scale, dtype=F32)
    coef = float(torch.tensor(k.coef, dtype=F32) * sc)
    l0, dgl = _ce32(gl, P.glab, coef)
    l1, dll = _ce32(ll, P.llab, coef, defect_keep=defect == "ignored_llab_dll")
    l2, dfl = _ce32(fl, P.glab, coef)
    rows = torch.stack([l0, l1, l2])
    if defect == "scale_on_rows":
        rows = rows * sc
    got = dict(rows=rows, dgl=dgl, dll=dll, dfl=dfl)
    wr = torch.ones(P.B, dtype=F32)
    if o.w:
        wr = torch.exp(-torch.tensor(k.rate, dtype=F32) * _ce32(P.t_fused, P.glab, 0.0)[0])
        got["w"] = wr
    if o.kd:
        T = torch.tensor(k.T, dtype=F32)
        kc = torch.tensor(k.kd_coef, dtype=F32) * sc * (torch.tensor(o.dev, dtype=F32) if o.dev is not None else 1.0)
        norm = torch.tensor(k.norm, dtype=F32)
        rep = (lambda x: x) if defect == "kd_keep_inf" else (lambda x: torch.where(x == NEG, torch.full_like(x, -1e6), x))
        ls, lt = torch.log_softmax(rep(fl) / T, 1), torch.log_softmax(rep(P.t_fused) / T, 1)
        pt, ps = lt.exp(), ls.exp()
        kl = torch.where(pt > 0, pt * (lt - ls), torch.zeros_like(pt)).sum(1)
        got["kd"] = wr * kl * T * T * norm
        gw = torch.ones_like(wr) if defect == "kd_no_weight" else wr
        kg = kc * gw[:, None] * T * (ps - pt) * norm
        got["dfl"] = kg if defect == "kd_overwrites" else dfl + kg
    return got


def emu_bwd(P, use_gate, up, defect=None):
    fw, omf = _gate32(P, use_gate, defect)
    B, K, Vp = P.B, P.K, P.Vp
    gm, lm, bw = P.gmask.bool(), P.lmask.bool(), P.bw.bool()
    z = lambda t, N: torch.zeros(B, N, dtype=F32) if t is None else t
    a, c_, f = z(up.get("dgl"), K), z(up.get("dll"), Vp), z(up.get("dfl"), K)
    zero = torch.zeros_like(f)
    dg = torch.where(gm, a + f, zero)
    fs = torch.where(gm, f, zero)
    if defect == "drop_k64":
        fs = fs.clone()
        fs[:, 64:] = 0.0
    S = torch.zeros(B, Vp, dtype=F32).scatter_add(1, P.fsrc.clamp(min=0).long(), torch.where(P.fsrc >= 0, fs, zero))
    back = torch.where(P.fsrc == -2, fs, zero).sum(1, keepdim=True)
    if defect == "m2_as_m1":
        back = torch.zeros_like(back)
    d = torch.where(lm, c_, torch.zeros_like(c_)) + S + bw * back
    if defect != "masked_local_grad":
        d = torch.where(lm, d, torch.zeros_like(d))
    sl_ = (d * P.l_raw).sum(1)
    if defect == "dfuse_no_local":
        sl_ = torch.zeros_like(sl_)
    dfw = (dg * P.g_raw).sum(1) - sl_
    df = dfw * fw * omf if (use_gate or defect == "gate_when_off") else torch.zeros(B, dtype=F32)
    return dg * fw[:, None], d * omf[:, None], df


DEFECTS = {                                                # planted defect -> the stages it touches
    "bw_ignores_lmask": "1",        # the back-track sum ignoring lmask
    "m2_as_m1": "1b",               # fsrc = -2 treated as -1
    "drop_k64": "1b",               # tokens k >= 64 dropped in the forward; their dfl not scattered in the backward
    "gate_when_off": "1b",          # the gate applied although use_gate = 0, and dfuse_raw non-zero there
    "masked_local_grad": "b",       # a masked local entry receiving gradient
    "dfuse_no_local": "b",          # dfuse_raw without the local half
    "kd_no_weight": "2",            # the distillation gradient without the teacher-sample weight
    "kd_keep_inf": "2",             # -inf not replaced by -1e6 in the distillation rows
    "scale_on_rows": "2",           # the loss scale applied to rows
    "ignored_llab_dll": "2",        # an ignored local label still producing dll
    "kd_overwrites": "2",           # the distillation part overwriting dfl instead of adding to it
}


def emulate(run, c, defect=None):
    """every check of one case on the fp32 emulation (with `defect` planted in the stages it names)"""
    P = get(c)
    stages = DEFECTS.get(defect, "")
    d = lambda s: defect if s in stages else None
    gl, ll, fl = emu_stage1(P, c.gate, d("1"))
    verify_stage1(run, c.name, P, c.gate, gl, ll, fl)
    if c.loss:
        gl0, ll0, fl0 = emu_stage1(P, c.gate)              # stage 2 is judged from clean logits: one stage per check
        for od in opts_of(c):
            o = opt(od)
            verify_stage2(run, f"{c.name} {o.name}", P, o, gl0, ll0, fl0, emu_stage2(P, o, gl0, ll0, fl0, d("2")))
    full = upstream(P)
    for sub in SUBSETS:
        up = {k: full[k] for k in sub}
        dg, dl, df = emu_bwd(P, c.gate, up, d("b"))
        verify_bwd(run, f"{c.name} {'+'.join(sub)}", P, c.gate, up, dg, dl, df)


UNITS = ("last global token in dl_raw", "back-track term", "local half of dfuse_raw", "distillation gradient", "last CE column")


def report(prefix="sap "):
    return {k: v for k, v in sorted(WORST.items()) if k.startswith(prefix)}
