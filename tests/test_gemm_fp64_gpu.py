"""Every kernel form of csrc/gemm.hip against float64 per element (-m gpu): magic_gemm's single launches (64 x 64, XCD row order, K-groups, the
128 x 128 tile with and without its XCD order), the grouped launches and their placements, split-K with atomics and with slabs,
magic_gemm_dw_grouped (atomic and deterministic, all four placements), magic_gemm_dw_cat (narrow and wide) and magic_linear_ln /
magic_linear_act_ln (single and pair), in bf16, fp16 and fp32 (exact-MFMA mode).

References, envelopes and the check are tests/_gemm_ref64.py's: |got - ref| <= (n + 8) 2^-23 E + one storage ulp (+ A |pre-activation| for the erf
epilogues; LayerNorm outputs: 1 ulp + 0.003 row-rms ulp).  Every output buffer is NaN-filled and everything outside the logical extent (pitch
padding, guard rows, the gaps between batches) must still be NaN afterwards.  Every case asserts magic_gemm_last_form() and then shows that
the same check REJECTS references with one planted defect each (last k / row / column missing, bias missing / doubled, alpha of 1, a split /
problem / segment missing, residual missing, the neighbouring batch's aux); tests/test_gemm_ref64_cpu.py proves on the same inputs that each of
them bites.  Outputs that are identically zero (the empty third slab of the slab-mode cases) have no controls of their own.

The problems come from the builders of tests/_gemm_ref64.py, which test_gemm_ref64_cpu.py runs too.  k-contiguous input operands carry NaN in
every element past K and past the last row (extra pad vector, guard rows, batch gaps), so a read past the extent poisons the result.

Measured on an MI355X (test_zz_report_measured_worst prints these with -s), all three types together:
  worst err / bound per family
    gemm 64x64 0.4998   gemm branches 0.4982   gemm kg 0.4567   gemm xcd 0.4998   gemm wide 0.4998   grouped 0.4998   grouped kg 0.3734
    slab 0.0326   dw_grouped 0.0555   dw_grouped shared 0.0102   dw_cat 0.0077   dw_cat wide 0.0088
    linear_ln 0.4997   linear_ln pre 0.4998   linear_ln rstd 0.0480   erf epilogues with A = 0: 0.4995
    ~0.50 is the 16-bit storage rounding (half of the one ulp the check allows); the fp32-stored families sit at a few % of the worst-case
    sum bound.
  activation allowance: the worst |kernel - float64 erf form of the kernel's own fp32 pre-activation| / |pre-activation| over the fp32 cases with C2
    and no residual is 1.548e-7, well under one fp16 ulp (2^-11), so ACT_A = twice that, rounded up = 3.1e-7.  With A = 0 the bound already holds
    (the last family above): the allowance widens nothing that the sum term does not cover at these K.
  branches that could not be entered: none.  Every launch form, placement and gemm_block operand branch named above is entered, and
    the coverage test sees every form and placement bit (it and the report read what the cases above recorded, so they need the whole
    module run in one process).
"""
import os
import re

import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from tests import _gemm_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
HALF = ("bf16", "fp16")
ACT_A = 3.1e-7            # allowance of the erf epilogues per unit of |pre-activation|: twice the measured worst, see the module docstring

_HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "magic_hip.h")).read()
BIT = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define MAGIC_GEMM_((?:FORM|PLACE)_\w+) (0x[0-9a-fA-F]+)", _HDR)}
SEEN = {}                 # dtype name -> OR of every form word a case observed
STATS = {}                # family -> worst err / bound
ERF = {"worst": 0.0}      # worst |kernel - fp64 erf form of the kernel's own fp32 pre-activation| / |pre-activation| (fp32 cases with C2, no residual)


def last_form(dt, *names):
    got = int(L.load().magic_gemm_last_form())
    want = 0
    for n in names:
        want |= BIT[n]
    assert got == want, f"launch form {got:#x}, expected {'|'.join(names)} = {want:#x}"
    SEEN[dt] = SEEN.get(dt, 0) | got


def stat(family, r):
    STATS[family] = max(STATS.get(family, 0.0), r)


def held(got, ref, store, family, tag):
    r = R.ratio(got, ref, store, ACT_A)
    stat(family, r)
    assert r <= 1.0, f"{tag}: worst |err| / bound = {r:.3f}"
    if ref.pre is not None:
        stat("erf epilogues with A = 0", R.ratio(got, ref, store, 0.0))


def rejected(got, defects, store, tag):
    for name, d in defects.items():
        assert not R.passes(got, d, store, ACT_A), f"{tag}: the check does not notice {name}"


def launch(c, bias_grad=None):
    A, B, Cb = c["A"], c["B"], c["C"]
    aux, res, c2 = c.get("aux"), c.get("residual"), c.get("C2")
    O.gemm(c["layout"], A.flat, B.flat, Cb.flat, c["M"], c["N"], c["K"], A.ld, B.ld, Cb.ld, batch=c["batch"], nh=c["nh"],
           sA=(A.sb, A.sh), sB=(B.sb, B.sh), sC=(Cb.sb, Cb.sh), bias=c.get("bias"), epilogue=c["epilogue"],
           aux=aux.flat if aux else None, ldaux=aux.ld if aux else 0, residual=res.flat if res else None, ldr=res.ld if res else 0,
           C2=c2.flat if c2 else None, ldc2=c2.ld if c2 else 0, alpha=c["alpha"], splitk=c["splitk"], bias_grad=bias_grad,
           accumulate=c["accumulate"])


def verify(c, family, tag):
    got = c["C"].view()
    held(got, c["ref"], c["store"], family, tag)
    assert c["C"].untouched(), f"{tag}: C written outside its logical extent"
    if "C2" in c:
        held(c["C2"].view(), c["ref"].c2, c["dtype"], family, tag + " C2")
        assert c["C2"].untouched(), f"{tag}: C2 written outside its logical extent"
    rejected(got, R.gemm_defects(c), c["store"], tag)
    if c["dtype"] == torch.float32 and "C2" in c and c["epilogue"] in (1, 3) and "residual" not in c:
        # the erf forms alone: fp32 C2 is the kernel's own pre-activation v, exactly; C against the float64 activation of that v
        v = c["C2"].view().double()
        want = R.gelu(v) if c["epilogue"] == 1 else v * R.dgelu(c["aux"].view().double())
        ERF["worst"] = max(ERF["worst"], ((got.double() - want).abs() / v.abs().clamp_min(1e-30)).max().item())
        ERF["cases"] = ERF.get("cases", 0) + 1


# ---- single launches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("dt", DTYPES)
def test_tile_edges_64(dt, layout):
    dtype = DTYPES[dt]
    for K in R.SWEEP_K[R.bits(dtype)]:
        for M in R.SWEEP_MN:
            for N in R.SWEEP_MN:
                c = R.gemm_case(dtype, layout, M, N, K, device=DEV, bias=True, seed=1)
                launch(c)
                last_form(dt, "FORM_PLAIN")
                verify(c, "gemm 64x64", f"{dt} layout {layout} {M}x{N}x{K}")


@pytest.mark.parametrize("dt", DTYPES)
def test_operand_branches(dt):
    for tag, kw in R.branch_cases(DTYPES[dt]):
        c = R.gemm_case(DTYPES[dt], device=DEV, seed=2, **kw)
        launch(c)
        last_form(dt, "FORM_PLAIN")
        verify(c, "gemm branches", f"{dt} {tag}")


@pytest.mark.parametrize("dt", DTYPES)
def test_kgroup_and_xcd_forms(dt):
    dtype = DTYPES[dt]
    for tag, form, kw in R.form_cases(dtype):
        c = R.gemm_case(dtype, device=DEV, seed=3, **kw)
        launch(c)
        last_form(dt, "FORM_" + form)
        verify(c, "gemm " + form.lower(), f"{dt} {tag}")
    # TN on the XCD order with the fused bias gradient (17 row tiles)
    c, rb, bad = R.bias_grad_case(dtype, DEV)
    db = torch.zeros(1025 + 8, device=DEV)
    db[1025:] = float("nan")
    launch(c, bias_grad=db)
    last_form(dt, "FORM_XCD")
    verify(c, "gemm xcd", f"{dt} xcd tn")
    held(db[:1025], rb, torch.float32, "gemm xcd", f"{dt} xcd tn bias_grad")
    assert torch.isnan(db[1025:]).all()
    rejected(db[:1025], bad, torch.float32, f"{dt} xcd tn bias_grad")


@pytest.fixture
def big_tiles():
    L.call("magic_gemm_set_big", 2)
    yield
    L.call("magic_gemm_set_big", 1)


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("dt", HALF)
def test_wide_tile(dt, layout, big_tiles):
    for M, N, K, form in R.WIDE_SHAPES:
        c = R.gemm_case(DTYPES[dt], layout, M, N, K, device=DEV, bias=True, seed=4)
        launch(c)
        last_form(dt, "FORM_" + form)
        verify(c, "gemm wide", f"{dt} wide layout {layout} {M}x{N}x{K}")


# ---- grouped launches -------------------------------------------------------------------------------------------------------------------
def grouped(dt, cases, form, places, family):
    with L.group():
        for c in cases:
            launch(c)
    last_form(dt, form, *places)
    for i, c in enumerate(cases):
        verify(c, family, f"{dt} {family} problem {i} of {len(cases)}")


@pytest.mark.parametrize("dt", DTYPES)
def test_grouped_launches(dt):
    for family, form, places, kws in R.grouped_cases(DTYPES[dt]):
        grouped(dt, [R.gemm_case(DTYPES[dt], device=DEV, **kw) for kw in kws], form, places, family)


# ---- split-K with slabs, and the refusals that guard the split modes -----------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_slab_mode(dt):
    for layout, K in R.slab_cases(DTYPES[dt]):
        c = R.slab_case(DTYPES[dt], layout, K, DEV)
        M, N, ldc, n = c["M"], c["N"], c["C"].ld, R.SLAB_SPLITS
        slabs = torch.full((n * M * ldc + 64,), float("nan"), device=DEV)
        A, B = c["A"], c["B"]
        O.gemm(layout, A.flat, B.flat, slabs, M, N, K, A.ld, B.ld, ldc, bias=c["bias"], alpha=R.SLAB_ALPHA, splitk=-n)
        last_form(dt, "FORM_PLAIN")
        got = slabs[:n * M * ldc].view(n, M, ldc)
        held(got[:, :, :N], c["slab_ref"], torch.float32, "slab", f"{dt} slab layout {layout} K {K}")
        assert torch.isnan(got[:, :, N:]).all() and torch.isnan(slabs[n * M * ldc:]).all()
        assert (got[2, :, :N] == 0).all(), "the empty third slab must be zeros"
        rejected(got[:, :, :N], c["slab_defects"], torch.float32, f"{dt} slab layout {layout} K {K}")


def test_split_mode_refusals():
    x = torch.zeros(64, 64, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(3 * 64 * 64, device=DEV)

    def refused(C_, **kw):
        with pytest.raises(L.MagicHipError):
            O.gemm(kw.pop("layout", 0), x, x, C_, 64, 64, 64, 64, 64, 64, **kw)
    refused(x, splitk=-2)                                   # slabs are fp32
    refused(f, splitk=-2, epilogue=1)
    refused(f, splitk=-2, residual=f, ldr=64)
    refused(f, splitk=-2, C2=x, ldc2=64)
    refused(f, splitk=-2, layout=2, bias_grad=f)
    refused(f, splitk=-2, batch=2, sA=(0, 0))
    refused(f, splitk=2)                                    # atomics need accumulate
    refused(x, splitk=2, accumulate=True)                   # ... and an fp32 C
    refused(x, accumulate=True)
    refused(f, splitk=2, accumulate=True, epilogue=2)
    refused(f, splitk=2, accumulate=True, residual=f, ldr=64)
    refused(f, splitk=2, accumulate=True, C2=x, ldc2=64)
    refused(f, bias_grad=f)                                 # the bias gradient is TN's
    refused(f, splitk=0)
    assert (f == 0).all()


# ---- magic_gemm_dw_grouped ------------------------------------------------------------------------------------------------------------------
def run_dw(dt, probs, det, places, family):
    dtype = DTYPES[dt]
    leaders = [p for p in probs if p.leader is p]
    for p in leaders:
        p.reset()
    arr = (L.DwDesc * len(probs))()
    for j, p in enumerate(probs):
        q = p.leader
        arr[j] = L.DwDesc(L.P(p.dy), L.P(p.x), L.P(q.dW), L.P(q.db), p.M, p.N, p.K, p.lda, p.ldb, q.ldc, p.splitk)
    assert O.dw_grouped(dtype, arr, len(probs), torch.device(DEV, torch.cuda.current_device()), deterministic=det) == det
    last_form(dt, "FORM_DW_DET" if det else "FORM_DW_ATOMIC", *places)
    for i, p in enumerate(leaders):
        tag = f"{dt} {family} {'det' if det else 'atomic'} dW {i} ({p.N}x{p.K})"
        rw, rb = p.refs()
        held(p.dW[:p.N, :p.K], rw, torch.float32, family, tag)
        assert torch.isnan(p.dW[p.N:]).all() and torch.isnan(p.dW[:, p.K:]).all(), f"{tag}: dW written outside its extent"
        bad = p.defects()
        rejected(p.dW[:p.N, :p.K], {k: v[0] for k, v in bad.items()}, torch.float32, tag)
        if p.db is not None:
            held(p.db[:p.N], rb, torch.float32, family, tag + " db")
            assert torch.isnan(p.db[p.N:]).all()
            rejected(p.db[:p.N], {k: v[1] for k, v in bad.items()}, torch.float32, tag + " db")
    if det:
        assert int(O.dw_counters(DEV).abs().sum().item()) == 0, "arrival counters not back at zero"
    return [p.dW.clone() for p in leaders] + [p.db.clone() for p in leaders if p.db is not None]


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("dt", DTYPES)
def test_dw_grouped_placements(dt, det):
    """all four placements in one launch of nine problems (R.dw_placement_problems: 8 splits; 1 / 2 / 4 splits over 3 and 5 tiles, wide and
    tall; 3 splits over 17 row tiles, seven surplus; single tiles), then every problem in a launch of its own, where the form word shows the
    one placement it took"""
    listed = R.dw_placement_problems(DTYPES[dt], DEV)
    probs = [p for p, _ in listed]
    places = sorted({place for _, place in listed})
    assert len(places) == 4
    first = run_dw(dt, probs, det, places, "dw_grouped")
    if det:
        again = run_dw(dt, probs, det, places, "dw_grouped")
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again)), "deterministic form differs between two runs"
    for p, place in listed:
        run_dw(dt, [p], det, [place], "dw_grouped")


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("dt", DTYPES)
def test_dw_grouped_shared_dw(dt, det):
    """one dW shared by three problems with different row counts and split counts (320 rows over 4 splits leave an empty trailing split
    in the 16-bit types), ldc = K + 8, with and without db"""
    for with_db in (True, False):
        probs = R.dw_shared_problems(DTYPES[dt], with_db, DEV)
        first = run_dw(dt, probs, det, ["PLACE_XCD_GROUPS", "PLACE_PLAIN"], "dw_grouped shared")
        if det:
            again = run_dw(dt, probs, det, ["PLACE_XCD_GROUPS", "PLACE_PLAIN"], "dw_grouped shared")
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(first, again))


# ---- magic_gemm_dw_cat --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("dt", DTYPES)
def test_dw_cat(dt, wide):
    dtype = DTYPES[dt]
    probs = R.dw_cat_problems(dtype, wide, DEV)
    descs, dyp, xp, mt, outs = [], [], [], [], []
    for p in probs:
        N, K, segs, w0, b0 = p.N, p.K, p.segs, p.w0, p.b0
        dW = torch.full((N + 2, K + 8), float("nan"), device=DEV)
        dW[:N, :K] = w0
        db = torch.full((N + 2,), float("nan"), device=DEV)
        db[:N] = b0
        outs.append((dW, db))
        descs.append((dW.data_ptr(), db.data_ptr(), N, K, segs[0][2], segs[0][3], K + 8))
        dyp.append([s[0].data_ptr() for s in segs])
        xp.append([s[1].data_ptr() for s in segs])
        mt.append(list(p.rows))
    dy_tab, x_tab = torch.tensor(dyp, dtype=torch.int64, device=DEV), torch.tensor(xp, dtype=torch.int64, device=DEV)
    m_tab = torch.tensor(mt, dtype=torch.int32, device=DEV)
    O.dw_cat(dtype, descs, 4, dy_tab.data_ptr(), x_tab.data_ptr(), m_tab.data_ptr())
    last_form(dt, "FORM_DW_CAT_WIDE" if wide and dtype != torch.float32 else "FORM_DW_CAT")
    fam = "dw_cat wide" if wide else "dw_cat"
    for p, (dW, db) in zip(probs, outs):
        N, K = p.N, p.K
        tag = f"{dt} {fam} {N}x{K} rows {p.rows}"
        assert torch.isnan(dW[N:]).all() and torch.isnan(dW[:, K:]).all() and torch.isnan(db[N:]).all(), f"{tag}: written outside the extent"
        if not any(p.rows):
            assert torch.equal(dW[:N, :K].view(torch.int32), p.w0.view(torch.int32)) and torch.equal(db[:N].view(torch.int32), p.b0.view(torch.int32)), tag
            continue
        rw, rb = p.refs()
        held(dW[:N, :K], rw, torch.float32, fam, tag)
        held(db[:N], rb, torch.float32, fam, tag + " db")
        bad = p.defects()
        rejected(dW[:N, :K], {k: v[0] for k, v in bad.items()}, torch.float32, tag)
        rejected(db[:N], {k: v[1] for k, v in bad.items()}, torch.float32, tag + " db")


# ---- magic_linear_ln / magic_linear_act_ln ----------------------------------------------------------------------------------------------------
def lln_outputs(dtype, M, H):
    return torch.full((M + 2, H), float("nan"), dtype=dtype, device=DEV), torch.full((M + 2,), float("nan"), device=DEV)


def lln_verify(dtype, M, K, ops, out, rstd, pre_out, act, with_res, tag):
    (r_out, r_rstd, r_pre), bad = R.lln_refs(dtype, K, ops, act, with_res, ACT_A)
    held(out[:M], r_out, dtype, "linear_ln", tag)
    assert torch.isnan(out[M:].float()).all(), f"{tag}: guard rows written"
    if rstd is not None:
        held(rstd[:M], r_rstd, torch.float32, "linear_ln rstd", tag + " rstd")
        assert torch.isnan(rstd[M:]).all()
    if pre_out is not None:
        held(pre_out[:M], r_pre, dtype, "linear_ln pre", tag + " pre")
        assert torch.isnan(pre_out[M:].float()).all()
    rejected(out[:M], bad, dtype, tag)


@pytest.mark.parametrize("H", R.LLN_H)
@pytest.mark.parametrize("dt", DTYPES)
def test_linear_ln_and_act_ln(dt, H):
    dtype = DTYPES[dt]
    for K in R.LLN_K[R.bits(dtype)]:
        for M in R.LLN_M:
            ops = R.lln_operands(dtype, M, H, K, 90, DEV)
            x, W, bias, gamma, beta, res = ops
            for with_res, with_rstd in ((True, True), (False, False)):
                out, rstd = lln_outputs(dtype, M, H)
                L.call("magic_linear_ln", L.dt(dtype), M, H, K, L.P(x), x.stride(0), L.P(W), W.stride(0), L.P(bias), L.P(res) if with_res else None,
                       H if with_res else 0, L.P(gamma), L.P(beta), R.LLN_EPS, L.P(out), L.P(rstd) if with_rstd else None, None, 0.0, 0, L.stream())
                last_form(dt, "FORM_LLN")
                lln_verify(dtype, M, K, ops, out, rstd if with_rstd else None, None, 0, with_res, f"{dt} linear_ln H {H} M {M} K {K} res {with_res}")
            for act in (1, 2):
                out, rstd = lln_outputs(dtype, M, H)
                pre = torch.full((M + 2, H), float("nan"), dtype=dtype, device=DEV)
                L.call("magic_linear_act_ln", L.dt(dtype), M, H, K, L.P(x), x.stride(0), L.P(W), W.stride(0), L.P(bias), act, L.P(pre),
                       L.P(gamma), L.P(beta), R.LLN_EPS, L.P(out), L.P(rstd) if act == 1 else None, L.stream())
                last_form(dt, "FORM_LLN")
                lln_verify(dtype, M, K, ops, out, rstd if act == 1 else None, pre, act, False, f"{dt} linear_act_ln H {H} M {M} K {K} act {act}")


@pytest.mark.parametrize("H", R.LLN_H)
@pytest.mark.parametrize("dt", DTYPES)
def test_linear_ln_pair(dt, H):
    dtype = DTYPES[dt]
    K = R.LLN_K[R.bits(dtype)][1]
    sides = []
    with L.group():
        for M, seed, with_res in R.LLN_PAIR:
            ops = R.lln_operands(dtype, M, H, K, seed, DEV)
            out, rstd = lln_outputs(dtype, M, H)
            O.linear_ln(ops[0], ops[1][:, :K], ops[2], M, ops[5] if with_res else None, ops[3], ops[4], R.LLN_EPS, out, rstd)
            sides.append((M, ops, out, rstd, with_res))
    last_form(dt, "FORM_LLN_PAIR")
    for M, ops, out, rstd, with_res in sides:
        lln_verify(dtype, M, K, ops, out, rstd, None, 0, with_res, f"{dt} linear_ln pair H {H} M {M}")


# ---- coverage and report ------------------------------------------------------------------------------------------------------------------
def test_zy_every_form_and_placement_was_seen():
    """runs after the cases above (file order): every form and placement bit for each 16-bit type; fp32 has no 128 x 128 kernels"""
    assert SEEN, "nothing recorded: this test reads what the cases above observed, so run the whole module in one process (no -k, no xdist split)"
    every = 0
    for v in BIT.values():
        every |= v
    for dt in HALF:
        missing = [n for n, v in BIT.items() if not SEEN.get(dt, 0) & v]
        assert not missing, f"{dt}: never launched {missing} (by the cases of this module that ran in this process)"
    wide = BIT["FORM_WIDE"] | BIT["FORM_WIDE_XCD"] | BIT["FORM_DW_CAT_WIDE"]
    assert SEEN.get("fp32", 0) == every & ~wide, f"fp32 saw {SEEN.get('fp32', 0):#x} of {every & ~wide:#x}"


def test_zz_report_measured_worst():
    """prints (-s) the figures the module docstring records; needs the cases above to have run in this process"""
    assert ERF.get("cases", 0) >= 2, "no erf case was measured: run the whole module in one process (no -k, no xdist split)"
    for k in sorted(STATS):
        print(f"  worst err / bound  {k:24s} {STATS[k]:.4f}")
    print(f"  erf epilogues on fp32 outputs: worst |kernel - fp64| / |pre-activation| = {ERF['worst']:.3e} (ACT_A = {ACT_A:.3e})")
    assert ERF["worst"] < 2.0 ** -11, "the erf epilogues are off by more than one fp16 ulp of the pre-activation"
    assert 2.0 * ERF["worst"] <= ACT_A, "ACT_A is below twice the measured worst: measure again"
