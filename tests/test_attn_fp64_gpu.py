"""Fused attention (csrc/attention.hip) against float64: every kernel, both pair forms, every tile edge (-m gpu).

Reference, bounds, rule mirrors and the case table live in tests/_attn_ref64.py; tests/test_attn_ref64_cpu.py proves on these very inputs
that an honest fp32 / 16-bit emulation passes the bounds and that every planted defect fails them.

Every output buffer (P, Pd, ctx, dq, dk, dv) is NaN-filled before the launch and sits between two guard rows holding a sentinel.  dq / dk /
dv are column slabs of wider buffers ([rows, 3H] in the self-attention layout, [rows, 2H] in the cross layout).  After the launch everything
the contract says is written must be finite and everything else -- guard rows, the slabs that are no output, rows past the problem's --
must still hold its fill bit for bit.  The unused rows of the input buffers hold NaN too: a kernel that reads past its problem shows up.

| kernel                | storage              | (Nq, Nk)                                                                         | branches |
| attn_fwd_kernel       | bf16, fp16, fp32     | 1x1 17x15 16x16 33x17 63x31 64x32 65x33 37x64 70x65 128x127 130x128              | NT = NKP / 16 in {2, 4, 6, 8} (NKP is a multiple of 32), partial last query tile, second / third query tile |
| attn_fwd_tiled_kernel | fp32; 16-bit + dist  | 1x129 65x255 64x256 40x257 33x512                                                | one valid key in the last tile, tile - 1, full tiles, tile + 1, late maximum, every key of tile 0 masked, fp32 with dropout |
| attn_fwd_ks_kernel    | bf16, fp16           | 1x129 64x191 65x192 40x193 33x449 70x512                                         | nact 3, 3, 3, 4, 8, 8; a slab with one valid key; every key of slab 1 masked |
| attn_bwd_kernel<4>    | all                  | 36x36 32x17 64x64 (alias); 64x17 33x32 (no alias)                                | |
| attn_bwd_kernel<8>    | all, where supported | 40x128 64x65 (alias); 80x80 65x64 128x128 97x33 (no alias)                       | |
| attn_bwd_ks_kernel    | bf16, fp16           | 1x129 16x192 64x193 65x256 130x512                                               | query-tile loop of 1, 2, 3; accumulate_kv on / off |
plus one fully masked sample per forward kernel, the pair forms (tests/_attn_ref64.PAIRS) and the ldp contract (LDP_CASES).

The kernels leave no trace of which branch ran: kernel and branch of each case are INFERRED from the C rules, mirrored in
tests/_attn_ref64.py (check_case_rules) and asserted here against the library's own magic_attn_supported answers.
MEASURE = True records and prints the worst of every figure and asserts no bound (how EXPF_A, TILE_REL and the measured figures in the
docstring of _attn_ref64.py were set); test_zz_report prints them with -s."""
import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from tests import _attn_ref64 as R
from tests.test_dropout_gpu import export_mask, seed_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEASURE = False
STATS = {}
SENT = -12345.0
NAN = float("nan")

FWD = [(c, dt) for c in R.FWD_CASES for dt in c.dtypes()]
BWD = [(c, dt) for c in R.BWD_CASES for dt in c.dtypes()]
ids = lambda ps: [f"{dt}-{c.id}" for c, dt in ps]


@pytest.fixture(autouse=True)
def exact_f32():
    prev = L.set_f32_mfma("exact")
    yield
    L.set_f32_mfma(prev)


def stats(dt, c):
    return STATS.setdefault((dt, c.kernel), {})


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class Guarded:
    """a NaN-filled [rows, cols] buffer between two sentinel rows; `body` is what the kernel gets"""

    def __init__(self, rows, cols, dtype, fill=NAN):
        self.buf = torch.full((rows + 2, cols), fill, dtype=dtype, device=DEV)
        self.buf[0] = SENT
        self.buf[-1] = SENT
        self.body = self.buf[1:-1]
        self.written = torch.zeros(rows, cols, dtype=torch.bool, device=DEV)

    def snap(self):
        self.before = self.buf.clone()

    def check(self, tag):
        """what the contract says is written is finite; everything else holds its fill bit for bit"""
        assert torch.isfinite(self.body[self.written].float()).all(), f"{tag}: non-finite elements where the kernel writes"
        w = torch.zeros_like(self.buf, dtype=torch.bool)
        w[1:-1] = self.written
        assert torch.equal(bits(self.buf)[~w], bits(self.before)[~w]), f"{tag}: the kernel wrote outside its contract"


class SimpleView(R.SimpleNamespace):
    pass


def inputs(c, dtype, o):
    """q / k / v views and pitches in the case's layout; unused rows of the shared buffer hold NaN"""
    B, Nq, Nk, H = c.B, c.Nq, c.Nk, c.H
    if c.cross:
        qb = o.q.reshape(B * Nq, H).to(DEV)
        kvb = torch.cat([o.k.reshape(B * Nk, H), o.v.reshape(B * Nk, H)], 1).to(DEV)
        return SimpleView(q=qb, k=kvb, v=kvb[:, H:], ldq=H, ldkv=2 * H)
    qkv = torch.full((B * max(Nq, Nk), 3 * H), NAN, dtype=dtype, device=DEV)
    qkv[:B * Nq, :H] = o.q.reshape(B * Nq, H).to(DEV)
    qkv[:B * Nk, H:2 * H] = o.k.reshape(B * Nk, H).to(DEV)
    qkv[:B * Nk, 2 * H:] = o.v.reshape(B * Nk, H).to(DEV)
    return SimpleView(q=qkv, k=qkv[:, H:], v=qkv[:, 2 * H:], ldq=3 * H, ldkv=3 * H)


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def prepare_fwd(c, dt, ldp=None):
    dtype = R.DTYPES[dt]
    o = R.operands(c, dtype)
    s = SimpleView(c=c, dt=dt, dtype=dtype, o=o, x=inputs(c, dtype, o), ldp=ldp or c.ldp)
    rows = c.B * c.nh * c.Nq
    s.P, s.Pd, s.ctx = Guarded(rows, s.ldp, dtype), (Guarded(rows, s.ldp, dtype) if c.p > 0 else None), Guarded(c.B * c.Nq, c.H, dtype)
    s.P.written[:] = True
    s.ctx.written[:] = True
    if s.Pd:
        s.Pd.written[:] = True
    s.kmask, s.dist = dev(o.kmask), dev(o.dist)
    s.sw = torch.tensor([R.SPREL[0]], device=DEV) if c.dist else None
    s.sb = torch.tensor([R.SPREL[1]], device=DEV) if c.dist else None
    s.seed = seed_of(c.seed & 0xFFFF, (c.seed >> 16) & 0x7FFF)
    s.site = 0x1000 + (c.seed & 0xFFF)
    s.drop = (s.seed, c.p, s.site) if c.p > 0 else None
    for g in (s.P, s.Pd, s.ctx):
        if g:
            g.snap()
    return s


def launch_fwd(s):
    c, x = s.c, s.x
    O.attn_fwd(x.q, x.ldq, x.k, x.v, x.ldkv, s.P.body, s.ldp, s.ctx.body, c.B, c.nh, c.Nq, c.Nk, c.H, R.SCALE, kmask=s.kmask, dist=s.dist,
               sprel_w=s.sw, sprel_b=s.sb, drop=s.drop, Pd=s.Pd.body if s.Pd else None)


def collect_fwd(s, tag):
    c = s.c
    torch.cuda.synchronize()
    for name, g in (("P", s.P), ("Pd", s.Pd), ("ctx", s.ctx)):
        if g:
            g.check(f"{tag} {name}")
    s.keep = export_mask(s.seed, c.p, s.site, (c.B, c.nh, c.Nq, c.Nk)).cpu() if c.p > 0 else None
    shape = (c.B, c.nh, c.Nq, s.ldp)
    s.Pc, s.Pdc, s.ctxc = s.P.body.cpu().view(shape), (s.Pd.body.cpu().view(shape) if s.Pd else None), s.ctx.body.cpu().view(c.B, c.Nq, c.H)
    return s


def verify_fwd(s, tag):
    R.verify_fwd(s.c, s.dtype, s.o, s.keep, s.Pc, s.Pdc, s.ctxc, tag, stats(s.dt, s.c), MEASURE)


def prepare_bwd(c, dt, f):
    """outputs of a backward over the forward state f (its stored P, and its ctx for the key-split kernel)"""
    dtype, o = f.dtype, f.o
    B, Nq, Nk, H = c.B, c.Nq, c.Nk, c.H
    s = SimpleView(c=c, dt=dt, dtype=dtype, o=o, f=f)
    s.dO = o.dO.reshape(B * Nq, H).to(DEV)
    s.dP_init = dev(o.dP_init)
    if c.cross:
        # dq is the SECOND slab of a [B Nq, 2H] buffer (the first is no output), dk | dv the two slabs of a [B Nk, 2H] buffer
        gq, gkv = Guarded(B * Nq, 2 * H, dtype), Guarded(B * Nk, 2 * H, dtype)
        s.dq, s.dk, s.dv, s.lddq, s.lddkv = gq.body[:, H:], gkv.body, gkv.body[:, H:], 2 * H, 2 * H
        gq.written[:, H:] = True
        gkv.written[:] = True
        s.guards = (gq, gkv)
        s.views = (gq.body[:, H:], gkv.body[:, :H], gkv.body[:, H:])
    else:
        g = Guarded(B * max(Nq, Nk), 3 * H, dtype)
        s.dq, s.dk, s.dv, s.lddq, s.lddkv = g.body, g.body[:, H:], g.body[:, 2 * H:], 3 * H, 3 * H
        g.written[:B * Nq, :H] = True
        g.written[:B * Nk, H:] = True
        s.guards = (g,)
        s.views = (g.body[:B * Nq, :H], g.body[:B * Nk, H:2 * H], g.body[:B * Nk, 2 * H:])
    if c.acc:
        s.views[1][:] = o.base_k.reshape(B * Nk, H).to(DEV)
        s.views[2][:] = o.base_v.reshape(B * Nk, H).to(DEV)
    s.dsw = torch.zeros(1, device=DEV) if c.dist else None
    s.dsb = torch.zeros(1, device=DEV) if c.dist else None
    for g in s.guards:
        g.snap()
    return s


def launch_bwd(s):
    c, f, x = s.c, s.f, s.f.x
    if c.kernel == "bwd_ks":
        O.attn_bwd_ks(x.q, x.ldq, x.k, x.v, x.ldkv, f.P.body, f.ldp, f.ctx.body, s.dO, c.B, c.nh, c.Nq, c.Nk, c.H, R.SCALE, s.dq, s.lddq, s.dk, s.dv,
                      s.lddkv, accumulate_kv=c.acc, drop=f.drop)
    else:
        O.attn_bwd(x.q, x.ldq, x.k, x.v, x.ldkv, f.P.body, f.ldp, s.dO, c.B, c.nh, c.Nq, c.Nk, c.H, R.SCALE, s.dP_init, s.dq, s.lddq, s.dk, s.dv,
                   s.lddkv, dist=f.dist, dsprel_w=s.dsw, dsprel_b=s.dsb, drop=f.drop)


def collect_bwd(s, tag):
    c = s.c
    O.flush_part_jobs()
    torch.cuda.synchronize()
    for g in s.guards:
        g.check(f"{tag} dq/dk/dv")
    s.out = [v.cpu().reshape(c.B, -1, c.H) for v in s.views]
    if c.dist:
        assert torch.isfinite(s.dsw).all() and torch.isfinite(s.dsb).all(), f"{tag}: distance-bias gradients"
    return s


def verify_bwd(s, tag):
    f = s.f
    R.verify_bwd(s.c, s.dtype, s.o, f.keep, f.Pc, f.ctxc, *s.out, tag, stats(s.dt, s.c), MEASURE)


def forward_of(c, dt, tag):
    f = prepare_fwd(c, dt)
    launch_fwd(f)
    return collect_fwd(f, tag)


# ---- rules ------------------------------------------------------------------------------------------------------------------------------------
def test_rule_mirrors_equal_the_library_and_every_branch_has_a_case():
    every = R.FWD_CASES + R.BWD_CASES + [c for _, a, b in R.PAIRS for c in (a, b)] + R.LDP_CASES
    for c in every:
        for dtype in R.DTYPES.values():
            assert O.attn_supported(dtype, c.Nq, c.Nk, False) == R.attn_supported(dtype, c.Nq, c.Nk, 0), (c.id, dtype)
            assert O.attn_supported(dtype, c.Nq, c.Nk, True) == R.attn_supported(dtype, c.Nq, c.Nk, 1), (c.id, dtype)
            assert O.attn_bwd_ks_ok(dtype, c.Nq, c.Nk) == R.attn_supported(dtype, c.Nq, c.Nk, 2), (c.id, dtype)
        for dt in c.dtypes():
            R.check_case_rules(c, R.DTYPES[dt])
    claimed = {k: set() for k in R.BRANCHES}
    for c, dt in FWD + BWD:
        claimed[c.kernel] |= set(c.branch) & R.inferred_branches(c, R.DTYPES[dt])
    for k, need in R.BRANCHES.items():
        assert need <= claimed[k], f"{k}: branches without a case: {sorted(need - claimed[k])}"
    assert {n for n, _, _ in R.PAIRS} == {"fwd pair", "fwd long-key group", "bwd pair 4 on 8", "bwd pair 4 + 4 large first"}


# ---- single launches ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,dt", FWD, ids=ids(FWD))
def test_forward(c, dt):
    tag = f"{dt} {c.id}"
    verify_fwd(forward_of(c, dt, tag), tag)


@pytest.mark.parametrize("c,dt", BWD, ids=ids(BWD))
def test_backward(c, dt):
    """forward (checked like test_forward's), then the backward over the P -- and, key-split, the ctx -- it stored"""
    tag = f"{dt} {c.id}"
    f = forward_of(c, dt, tag)
    verify_fwd(f, tag)
    s = prepare_bwd(c, dt, f)
    launch_bwd(s)
    verify_bwd(collect_bwd(s, tag), tag)


# ---- pair forms -----------------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def pair_params(which):
    """(pair, storage type) where both problems exist (the fp32 backward of 80 x 80 does not fit LDS: that pair is 16-bit only)"""
    return [(i, dt) for i in which for dt in R.DTYPES if dt in R.PAIRS[i][1].dtypes() and dt in R.PAIRS[i][2].dtypes()]


pair_ids = lambda ps: [f"{dt}-{R.PAIRS[i][0]}" for i, dt in ps]


@pytest.mark.parametrize("pair,dt", pair_params([0, 1]), ids=pair_ids(pair_params([0, 1])))
def test_forward_pair(pair, dt):
    """two forwards recorded under one group: the short pair goes out as ONE attn_fwd_pair_kernel launch (block -> problem map, LDS of the
    larger problem); with a long-key member launch_attn_fwd issues one launch per problem.  Same checks as single launches, and bit-identical
    to them (they share the body)."""
    name, a, b = R.PAIRS[pair]
    single = [forward_of(c, dt, f"{dt} {name} single {c.id}") for c in (a, b)]
    both = [prepare_fwd(c, dt) for c in (a, b)]
    with L.group():
        for s in both:
            launch_fwd(s)
    for s, one in zip(both, single):
        tag = f"{dt} {name} {s.c.id}"
        verify_fwd(collect_fwd(s, tag), tag)
        assert same_bits(s.P.body, one.P.body) and same_bits(s.ctx.body, one.ctx.body), f"{tag}: differs from the single launch"
        if s.Pd:
            assert same_bits(s.Pd.body, one.Pd.body), f"{tag}: Pd differs from the single launch"


@pytest.mark.parametrize("pair,dt", pair_params([2, 3]), ids=pair_ids(pair_params([2, 3])))
def test_backward_pair(pair, dt):
    """two backwards under one group = ONE attn_bwd_pair_kernel launch with max(lds_a, lds_b) and 8 waves if either side wants them: a 4-wave
    aliasing problem then runs on 8 waves.  Same checks as single launches, and bit-identical to them."""
    name, a, b = R.PAIRS[pair]
    cases = [a, b]
    fs = [forward_of(c, dt, f"{dt} {name} forward {c.id}") for c in cases]
    single = []
    for c, f in zip(cases, fs):
        s = prepare_bwd(c, dt, f)
        launch_bwd(s)
        single.append(collect_bwd(s, f"{dt} {name} single {c.id}"))
    both = [prepare_bwd(c, dt, f) for c, f in zip(cases, fs)]
    with L.group():
        for s in both:
            launch_bwd(s)
    for s, one in zip(both, single):
        tag = f"{dt} {name} {s.c.id}"
        verify_bwd(collect_bwd(s, tag), tag)
        for x, y in zip(s.views, one.views):
            assert same_bits(x, y), f"{tag}: differs from the single launch"


# ---- the ldp contract ------------------------------------------------------------------------------------------------------------------------------
LDP = [(c, dt) for c in R.LDP_CASES for dt in c.dtypes()]


@pytest.mark.parametrize("c,dt", LDP, ids=ids(LDP))
def test_row_pitch_up_to_rup32_is_accepted_and_beyond_is_refused(c, dt):
    """ldp = rup(Nk, 32), wider than any caller passes today, is accepted and its pad columns are zero; ldp = rup(Nk, 32) + 8 is refused by the
    forward and both backwards with MAGIC_ERR_ARG and nothing is written"""
    tag = f"{dt} {c.id}"
    f = forward_of(c, dt, tag)
    assert f.ldp == R.rup(c.Nk, 32)
    verify_fwd(f, tag)
    wide = prepare_fwd(c, dt, ldp=c.ldp + 8)
    with pytest.raises(L.MagicHipError):
        launch_fwd(wide)
    torch.cuda.synchronize()
    for g in (wide.P, wide.Pd, wide.ctx):
        assert same_bits(g.buf, g.before), f"{tag}: a refused forward wrote"
    # the backward of the same problem: accepted at rup(Nk, 32), refused one vector further (it reads whole ldp rows of P)
    kern = "bwd_ks" if c.Nk > 128 else "bwd4"
    if kern == "bwd_ks" and (not R.is16(f.dtype) or c.dist):
        return
    cb = R.Case(**{**c.__dict__, "kernel": kern})
    s = prepare_bwd(cb, dt, f)
    launch_bwd(s)
    verify_bwd(collect_bwd(s, tag), tag)
    s = prepare_bwd(cb, dt, f)
    f.ldp += 8
    try:
        with pytest.raises(L.MagicHipError):
            launch_bwd(s)
    finally:
        f.ldp -= 8
    torch.cuda.synchronize()
    for g in s.guards:
        assert same_bits(g.buf, g.before), f"{tag}: a refused backward wrote"


def test_zz_report_measured_worst():
    """prints (with -s) the worst of every figure this process measured, per storage type and kernel (what the constants were set from)"""
    for (dt, kern), d in sorted(STATS.items()):
        print(f"\n{dt:5s} {kern:7s} " + "  ".join(f"{n} {k} {v:.4g}" for (n, k), v in sorted(d.items())))
