"""magic_linear_lnbwd (csrc/gemm.hip: linear_lnb_body, linear_lnb_kernel, linear_lnb_pair_kernel, launch_llb) against float64 per element (-m gpu),
in bf16, fp16, fp32 with the exact MFMA and fp32 with the split-bf16 ("bf16x3") contraction on the natural-orientation weight tile.

References, bounds, operand builders and planted defects are tests/_drop_ref64.py's (its docstring has the derivation);
tests/test_drop_ref64_cpu.py proves on the same operands that every defect bites.  Operands: H in {128, 256}, M in {1, 31, 32, 33, 65}, K = one
k-tile short / exactly one / one and a tail / the second trip of the register prefetch; x, W and R at pitches above their extents with NaN in
every pad column and guard row; NaN-filled dx / dxm with two guard rows; dgamma / dbeta prefilled with 0.25 / -0.5; one gamma element exactly 0.
Every dropping case first asserts that mask64 equals, bit for bit, what magic_dropout exports for fp32 ones.

Forms per operand set: residual + dropout (launched twice: bitwise the same); residual, p > 0 with site 0 and dxm supplied (no dropout: dxm must
stay NaN -- "site 0 / p 0: dxm unused"); no residual with site 0xABCDEF01 at p = 0.5 (dxm == 2 dx bit for bit); dgamma = dbeta = NULL (dx
bitwise the run with them).  The pair launch under L.group() -- sides of different M, K and dropping / not -- against the single launches
(dx, dxm bitwise; dgamma, dbeta within the bound), two recorded calls of different H, and the refusals, each leaving every output byte alone.

The control "dxm from the rounded dx" is left out in every case (tests/_drop_ref64.py says why); dropped_exact checks instead, exactly, that
dropped positions are zero, that fp32 dxm == dx * the float32 keep factor and that p = 0.5 dxm == 2 dx (one ulp apart only at a rounding boundary).

Measured on an MI355X (test_zz_report prints these with -s), worst |err| / bound per output and mode:
                bf16     fp16     fp32     fp32 bf16x3
    dx          0.4973   0.4828   0.0100   0.2753
    dxm         0.4971   0.4803   0.0104   0.2753
    dgamma      0.0081   0.0105   0.0130   0.1912
    dbeta       0.0063   0.0069   0.0099   0.1871
  (16-bit dx / dxm: the storage rounding, half of the one ulp allowed; bf16x3 sits at a quarter of its 2^-16 term.)
  p = 0.5, fp16: two positions of all cases have dxm one ulp from 2 dx, both with the float64 value within 5e-5 ulp of a rounding boundary (the
  compiler rounds the fp32 product rs * t straight to 16 bits for dx, and its fp32 rounding times 2 for dxm); dropped_exact accepts exactly those.
Branches that could not be entered: none of the kernel's.  The launch has no form word (magic_gemm_last_form is not set by launch_llb), so that
the pair kernel ran follows from magic_group_end's rule -- two records of one kind, type and width -- not from an observation; that the bf16x3
branch ran is observed (its dx differs from the exact mode's on the same operands).
Kernel defects found: none.
"""
import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from tests import _drop_ref64 as D
from tests import _gemm_ref64 as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATS = {}
NAMES = ("dx", "dxm", "dgamma", "dbeta")
NAN = float("nan")
SEEN_X3, SEEN_EXACT = [], []          # dx of the dropping form at K >= one k-tile, in the two fp32 contraction modes


def same(a, b):
    """bit for bit, NaN guard rows included"""
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return a.shape == b.shape and torch.equal(a.view(v), b.view(v))


def export_mask(seed_t, p, site, M, H):
    ones, out = torch.ones(M * H, device=DEV), torch.empty(M * H, device=DEV)
    O.dropout(ones, out, 1, M * H, M * H, (seed_t, p, site))
    return out.view(M, H)


def mask_of(p, site, M, H):
    """(seed tensor, seed words, float64 mask on the device), asserted equal to the kernel's own export"""
    seed = D.pick_seed(p, site, M, H)
    seed_t = D.seed_tensor(seed, DEV)
    mask = D.mask64(seed_t, p, site, M, H)
    assert not D.mask_faults(mask, p)
    got = export_mask(seed_t, p, site, M, H)
    assert torch.equal(got, mask.float()) and torch.equal(got.double(), mask), f"mask64 differs from magic_dropout (p {p} site {site:#x} [{M}, {H}])"
    return seed_t, seed, mask


def fresh(o, dxm=True, grads=True):
    M, H, dtype = o["M"], o["H"], o["dtype"]
    return dict(dx=torch.full((M + 2, H), NAN, dtype=dtype, device=DEV), dxm=torch.full((M + 2, H), NAN, dtype=dtype, device=DEV) if dxm else None,
                dgamma=torch.full((H,), 0.25, device=DEV) if grads else None, dbeta=torch.full((H,), -0.5, device=DEV) if grads else None)


def raw_call(o, out, *, with_res=True, seed_t=None, p=0.0, site=0, x=None, lda=None, ldb=None, M=None, H=None):
    x = o["x"].data_ptr() if x is None else x
    L.call("magic_linear_lnbwd", L.dt(o["dtype"]), o["M"] if M is None else M, o["H"] if H is None else H, o["K"], x,
           o["x"].stride(0) if lda is None else lda, L.P(o["W"]), o["W"].stride(0) if ldb is None else ldb, L.P(o["R"]) if with_res else None,
           o["R"].stride(0) if with_res else 0, L.P(o["y"]), L.P(o["gamma"]), L.P(o["beta"]), L.P(o["rstd"]), L.P(out["dx"]), L.P(out["dxm"]),
           L.P(out["dgamma"]), L.P(out["dbeta"]), L.P(seed_t), float(p), int(site), L.stream())
    return out


def held(got, ref, store, key, tag):
    r = G.ratio(got, ref, store)
    STATS[key] = max(STATS.get(key, 0.0), r)
    assert r <= 1.0, f"{tag}: worst |err| / bound = {r:.3f}"


def verify(o, out, mode, tag, *, mask=None, with_res=True, site=None, seed=None, p=None, controls=True):
    M, dtype, x3 = o["M"], o["dtype"], mode.endswith("x3")
    good, bad = D.lnb_refs(o, mask, with_res, x3, site, seed, p)
    for name, ref in zip(NAMES, good):
        got = out[name]
        if got is None or ref is None:
            continue
        rows = got[:M] if name in ("dx", "dxm") else got
        held(rows, ref, dtype if name in ("dx", "dxm") else torch.float32, (name, mode), f"{tag} {name}")
        if name in ("dx", "dxm"):
            assert torch.isnan(got[M:].float()).all(), f"{tag} {name}: guard rows written"
    if mask is None and out["dxm"] is not None:
        assert torch.isnan(out["dxm"].float()).all(), f"{tag}: dxm written although nothing drops"
    if mask is not None:
        assert not D.dropped_exact(out["dx"][:M], out["dxm"][:M], mask, p, dtype, good[1].val, good[1].extra), tag
    if controls:
        for name, ref in bad.items():
            which = name.split(":")[0]
            if out[which] is None:
                continue
            rows = out[which][:M] if which in ("dx", "dxm") else out[which]
            assert not G.passes(rows, ref, dtype if which in ("dx", "dxm") else torch.float32), f"{tag}: the check does not notice {name}"


class f32_mode:
    """the fp32 contraction mode of `mode` for the block, the previous one restored afterwards"""

    def __init__(self, mode):
        self.want = "bf16x3" if mode.endswith("x3") else "exact"

    def __enter__(self):
        self.prev = L.set_f32_mfma(self.want)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        L.set_f32_mfma(self.prev)
        return False


@pytest.mark.parametrize("H", D.LNB_H)
@pytest.mark.parametrize("mode", D.LNB_MODES)
def test_single_launch_forms(mode, H):
    dtype = D.DTYPES[mode[:4]]
    with f32_mode(mode):
        for K in D.LNB_K[G.bits(dtype)]:
            for M in D.LNB_M:
                o = D.lnb_operands(dtype, M, H, K, 90, DEV)
                tag = f"{mode} H {H} M {M} K {K}"
                # residual + dropout, twice
                seed_t, seed, mask = mask_of(D.LNB_P, D.LNB_SITE, M, H)
                a = raw_call(o, fresh(o), seed_t=seed_t, p=D.LNB_P, site=D.LNB_SITE)
                b = raw_call(o, fresh(o), seed_t=seed_t, p=D.LNB_P, site=D.LNB_SITE)
                verify(o, a, mode, tag + " drop", mask=mask, site=D.LNB_SITE, seed=seed, p=D.LNB_P)
                assert same(a["dx"], b["dx"]) and same(a["dxm"], b["dxm"]), f"{tag}: two identical launches differ"
                # residual, p > 0 at site 0 = no dropout; dxm supplied and left alone
                c = raw_call(o, fresh(o), seed_t=seed_t, p=D.LNB_P, site=0)
                verify(o, c, mode, tag + " site 0")
                assert same(c["dx"], a["dx"]), f"{tag}: dx depends on the dropout site"
                # no gamma / beta gradients: the same dx
                d = raw_call(o, fresh(o, dxm=False, grads=False))
                assert same(d["dx"], c["dx"]), f"{tag}: dx differs without dgamma / dbeta"
                # no residual, a site with the top bit set, keep factor 2
                seed_t, seed, mask = mask_of(0.5, D.LNB_BIG_SITE, M, H)
                e = raw_call(o, fresh(o), with_res=False, seed_t=seed_t, p=0.5, site=D.LNB_BIG_SITE)
                verify(o, e, mode, tag + " no residual", mask=mask, with_res=False, site=D.LNB_BIG_SITE, seed=seed, p=0.5)
                if mode == "fp32x3" and K >= 32:
                    SEEN_X3.append(a["dx"][:M].clone())
                if mode == "fp32" and K >= 32:
                    SEEN_EXACT.append(a["dx"][:M].clone())


@pytest.mark.parametrize("H", D.LNB_H)
@pytest.mark.parametrize("mode", D.LNB_MODES)
def test_pair_launch(mode, H):
    dtype = D.DTYPES[mode[:4]]
    with f32_mode(mode):
        sides = []
        for M, ki, drops in D.LNB_PAIR:
            K = D.LNB_K[G.bits(dtype)][ki]
            o = D.lnb_operands(dtype, M, H, K, 91 + ki, DEV)
            kw = dict(with_res=drops)
            vk = dict(with_res=drops)
            if drops:
                seed_t, seed, mask = mask_of(D.LNB_P, D.LNB_SITE, M, H)
                kw.update(seed_t=seed_t, p=D.LNB_P, site=D.LNB_SITE)
                vk.update(mask=mask, site=D.LNB_SITE, seed=seed, p=D.LNB_P)
            sides.append((o, kw, vk, raw_call(o, fresh(o), **kw)))
        with L.group():
            paired = [raw_call(o, fresh(o), **kw) for o, kw, _, _ in sides]
        for (o, kw, vk, single), out in zip(sides, paired):
            tag = f"{mode} pair H {H} M {o['M']} K {o['K']}"
            verify(o, out, mode, tag, **vk)
            assert same(out["dx"], single["dx"]), f"{tag}: dx differs from the single launch"
            assert same(out["dxm"], single["dxm"]), f"{tag}: dxm differs from the single launch"


@pytest.mark.parametrize("mode", D.LNB_MODES)
def test_two_recorded_calls_of_different_width(mode):
    dtype = D.DTYPES[mode[:4]]
    K = D.LNB_K[G.bits(dtype)][2]
    with f32_mode(mode):
        seed_t, seed, mask = mask_of(D.LNB_P, D.LNB_SITE, 33, 128)
        oa, ob = D.lnb_operands(dtype, 33, 128, K, 95, DEV), D.lnb_operands(dtype, 31, 256, K, 96, DEV)
        with L.group():
            a = raw_call(oa, fresh(oa), seed_t=seed_t, p=D.LNB_P, site=D.LNB_SITE)
            b = raw_call(ob, fresh(ob))
        verify(oa, a, mode, f"{mode} recorded H 128", mask=mask, site=D.LNB_SITE, seed=seed, p=D.LNB_P)
        verify(ob, b, mode, f"{mode} recorded H 256")


@pytest.mark.parametrize("dt", D.DTYPES)
def test_refusals_leave_every_output_byte_alone(dt):
    dtype = D.DTYPES[dt]
    ve = G.ve_of(dtype)
    K = D.LNB_K[G.bits(dtype)][2]
    o = D.lnb_operands(dtype, 33, 128, K, 97, DEV)
    seed_t = D.seed_tensor((3, 4), DEV)

    def refused(code, *, dxm=True, grads=True, **kw):
        out = fresh(o, dxm=dxm)
        if grads == "dgamma only":
            out["dbeta"] = None
        with pytest.raises(L.MagicHipError, match=code):
            raw_call(o, out, **kw)
        torch.cuda.synchronize()
        clean = fresh(o, dxm=dxm)
        for k, v in out.items():
            if v is not None:
                assert same(v, clean[k]), f"{dt}: {k} touched by a refused call ({kw})"
    refused("MAGIC_ERR_UNSUPPORTED", H=384, ldb=384 + ve)                       # (refused before anything is read: no operands of that width needed)
    refused("MAGIC_ERR_ARG", lda=o["x"].stride(0) + 1)
    refused("MAGIC_ERR_ARG", ldb=o["H"] - ve)
    refused("MAGIC_ERR_ARG", x=o["x"].data_ptr() + o["x"].element_size())
    refused("MAGIC_ERR_ARG", grads="dgamma only")
    refused("MAGIC_ERR_ARG", dxm=False, seed_t=seed_t, p=0.1, site=5)
    refused("MAGIC_ERR_ARG", seed_t=seed_t, p=1.0, site=5)
    refused("MAGIC_ERR_ARG", M=0)


def test_zy_the_bf16x3_branch_ran():
    """needs the cases above in this process: the split-bf16 contraction gives another dx than the exact MFMA on the same operands"""
    assert SEEN_X3 and len(SEEN_X3) == len(SEEN_EXACT), "run the whole module in one process"
    assert any(not torch.equal(a, b) for a, b in zip(SEEN_X3, SEEN_EXACT))


def test_zz_report():
    assert STATS, "nothing recorded: run the whole module in one process"
    for name in NAMES:
        print("  worst err / bound  " + f"{name:8s}" + "  ".join(f"{m} {STATS.get((name, m), 0.0):.4f}" for m in D.LNB_MODES))
