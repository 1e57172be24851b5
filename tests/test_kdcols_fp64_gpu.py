"""magic_kd_cols (csrc/loss.hip kd_cols_kernel / kd_cols_row_kernel) against the float64 reference at every launch branch (-m gpu).

The reference (tests/_kdcols_ref64.py, shown right on the CPU by tests/test_kdcols_ref64_cpu.py) is float64 arithmetic on the operands as stored.
Every comparison is held to the project's bound -- REL = 1e-5 of the envelope of the output's terms, plus one unit in the last place of a 16-bit
gradient -- and every assertable case shows the SAME comparison failing against a reference that lacks the last class, the last inner column or the
last sample.  ds and the partials are pre-filled with a sentinel: nothing before or past their extents is written.

Launch branches entered here (dispatch of magic_kd_cols; `parts` = magic_kd_cols_parts):
  row form     inner < 64: one lane pass (C = 5, 9), nine and twelve strided passes (C = 513, 768), inner = 3 and 63, a second grid-stride trip
               (4200 rows over the 1024-workgroup cap)
  column form  inner = 64 / 65 / 257 (wave seam, lanes past the last column, a second workgroup), C < 16 (four column groups per workgroup) and
               C >= 16 (the four waves share the walk over C: 300 classes, and 16 with a second grid-stride trip), the 16-byte vector body
               (aligned base, inner and strides multiples of 8 / 4) and the scalar body (odd inner, a base sliced by one element), the head slice
               [:, :hmin] through s_stride = 2 C inner, a second grid-stride trip of the scalar body (inner = 262209) and of the vector body
  both         -inf in s only / t only / both, T in {1, 2}, w given / NULL, norm and coef != 1, fp32 / bf16 / fp16, ds NULL, the registered seed
               scale, two identical calls bitwise equal, every MAGIC_ERR_ARG refusal
Not assertable: with C = 1 loss and gradient are identically zero, so no reference can lack anything -- that case checks the values and the
untouched memory only.

Largest err / bound per family on an MI355X (every call of R.check prints its figure, `pytest -s`); REL = 1e-5 holds for both, factor 1:
  kdc_row   fp32 0.031   bf16 0.495   fp16 0.495
  kdc_col   fp32 0.058   bf16 0.497   fp16 0.497          (16-bit: the gradient's own rounding, half a unit in the last place of the bound's one)
Loss words, any dtype: at most 0.042 of their bound (the 513-class fp16 row, T = 2, weighted)."""
import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from tests import _kdcols_ref64 as KR
from tests import _loss_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
F32 = torch.float32
SENT = 7.0
NEG = float("-inf")

# (outer, C, inner, s_stride / (C inner), base offset in elements)
ROW_SHAPES = [(3, 5, 1, 1, 0), (2, 513, 1, 1, 0), (4, 768, 1, 1, 0), (2, 9, 3, 1, 0), (2, 7, 63, 1, 0), (4200, 2, 1, 1, 0)]
COL_SHAPES = [(2, 7, 64, 1, 0), (2, 7, 64, 1, 1), (2, 7, 65, 1, 0), (1, 12, 257, 1, 0), (2, 300, 128, 1, 0), (2, 300, 128, 1, 1),
              (3, 2, 81, 2, 0), (3, 2, 128, 2, 0), (1, 2, 262209, 1, 0), (1, 16, 524352, 1, 0)]
# T, weighted, norm, coef, -inf in s alone at the very last element
CONFIGS = [(1.0, False, 1.0, 1.0, False), (2.0, True, 0.37, 0.6, True)]


@pytest.fixture(autouse=True)
def _no_seed_scale():
    O.seed_scale(None)
    yield
    O.seed_scale(None)


def family(inner):
    return "kdc_row" if inner < 64 else "kdc_col"


def strided(flat, off, outer, C, inner, stride):
    return torch.as_strided(flat, (outer, C, inner), (stride, inner, 1), storage_offset=off)


def inputs(outer, C, inner, mult, off, dtype, s_only):
    """s with outer stride mult * C * inner (the head slice of a wider map), t dense; sentinel in the gaps; both on the device in `dtype`"""
    g = torch.Generator().manual_seed(outer * 1000003 + C * 1009 + inner)
    s_stride, t_stride = mult * C * inner, C * inner
    sv = 2 * torch.randn(outer, C, inner, generator=g, dtype=torch.float64)
    tv = 2 * torch.randn(outer, C, inner, generator=g, dtype=torch.float64)
    tv[:, C - 1] += 2.0                                     # the last class carries weight in every column
    if C > 2:
        sv[0, 1, 0] = tv[0, 1, 0] = NEG                     # both sides (a masked logit)
        tv[outer - 1, 0, inner // 2] = NEG                  # teacher alone: p_t = 0, the term adds nothing, the gradient is p_s
    if s_only and C > 1:
        sv[outer - 1, C - 1, inner - 1] = NEG               # student alone: log p_s ~ -1e6 / T under a live p_t -- every control below loses this element
    s_flat = torch.full((outer * s_stride + off + 8,), SENT, dtype=dtype, device=DEV)
    t_flat = torch.full((outer * t_stride + off + 8,), SENT, dtype=dtype, device=DEV)
    s, t = strided(s_flat, off, outer, C, inner, s_stride), strided(t_flat, off, outer, C, inner, t_stride)
    s.copy_(sv.to(dtype))
    t.copy_(tv.to(dtype))
    w = (torch.rand(outer, generator=g) + 0.25).float().to(DEV)
    return s, t, s_stride, t_stride, w


def launch(s, t, outer, C, inner, s_stride, t_stride, T, w, norm, coef, off, want_ds=True):
    n = O.kd_cols_parts(outer, C, inner)
    parts = torch.full((n + 3,), SENT, dtype=F32, device=DEV)
    dflat = torch.full((outer * C * inner + off + 16,), SENT, dtype=s.dtype, device=DEV)
    ds = dflat[off:off + outer * C * inner]
    O.kd_cols(s, t, outer, C, inner, s_stride, t_stride, T, w=w, norm=norm, coef=coef, loss_part=parts[:n], ds=ds if want_ds else None)
    torch.cuda.synchronize()
    assert bool((parts[n:] == SENT).all()), "a partial past the count was written"
    assert bool((dflat[:off] == SENT).all()) and bool((dflat[off + outer * C * inner:] == SENT).all()), "memory around ds was written"
    if not want_ds:
        assert bool((dflat == SENT).all()), "ds = NULL, yet ds memory was written"
    return parts[:n], ds.view(outer, C, inner), dflat


def controls(s, t, T, w, norm, coef):
    """references that lack the last class / the last inner column / the last sample: (loss, gradient padded with zeros) each"""
    outer, C, inner = s.shape
    out = []
    cuts = []
    if C > 1:
        cuts.append((slice(None), slice(0, C - 1), slice(None)))
    if inner > 1:
        cuts.append((slice(None), slice(None), slice(0, inner - 1)))
    if outer > 1:
        cuts.append((slice(0, outer - 1), slice(None), slice(None)))
    for cut in cuts:
        r = KR.kdcols_ref(s[cut], t[cut], T, None if w is None else w[cut[0]], norm, coef)
        g = torch.zeros(outer, C, inner, dtype=torch.float64, device=s.device)
        g[cut] = r["grad"]
        out.append((r["terms"].sum().reshape(1), g))
    return out


def check_case(tag, dtype, s, t, T, w, norm, coef, parts, ds):
    outer, C, inner = s.shape
    fam = family(inner)
    Tr, nr, cr = R.f32(T), R.f32(norm), R.f32(coef)
    ref = KR.kdcols_ref(s, t, Tr, w, nr, cr)
    ctrl = controls(s, t, Tr, w, nr, cr)
    assert ctrl, tag
    R.check(fam, f"loss {tag}", parts.double().sum().reshape(1), ref["terms"].sum().reshape(1), ref["terms_env"].sum().reshape(1),
            ctrl=[c[0] for c in ctrl])
    if ds is not None:
        R.check(fam, f"grad {tag}", ds, ref["grad"], ref["grad_env"], dtype, ctrl=[c[1] for c in ctrl])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("outer,C,inner,mult,off", ROW_SHAPES + COL_SHAPES)
def test_kd_cols_every_launch_form_matches_float64(outer, C, inner, mult, off, dtype):
    for T, weighted, norm, coef, s_only in CONFIGS:
        # past ~1000 columns one ordinary column's share of the loss word (1 / columns of an envelope of ~10 per column) sinks under REL = 1e-5 of it:
        # there the last element is the student-alone -inf in both configurations, so that each control still lacks something the bound can see
        s_only = s_only or outer * inner > 1024
        s, t, s_stride, t_stride, w = inputs(outer, C, inner, mult, off, dtype, s_only)
        w = w if weighted else None
        parts, ds, _ = launch(s, t, outer, C, inner, s_stride, t_stride, T, w, norm, coef, off)
        tag = f"({outer},{C},{inner}) x{mult} +{off} T={T} w={weighted} {dtype}"
        check_case(tag, dtype, s, t, T, w, norm, coef, parts, ds)
        # the same call again: bitwise the same partials and gradient; and with ds = NULL the same partials, nothing else written
        parts2, ds2, _ = launch(s, t, outer, C, inner, s_stride, t_stride, T, w, norm, coef, off)
        assert torch.equal(parts.view(torch.int32), parts2.view(torch.int32)) and torch.equal(ds.contiguous().view(torch.uint8), ds2.contiguous().view(torch.uint8)), tag
        parts3, _, _ = launch(s, t, outer, C, inner, s_stride, t_stride, T, w, norm, coef, off, want_ds=False)
        assert torch.equal(parts.view(torch.int32), parts3.view(torch.int32)), tag


@pytest.mark.parametrize("dtype", DTYPES)
def test_kd_cols_single_class_is_identically_zero(dtype):
    outer, C, inner = 1, 1, 70
    s, t, ss, ts, w = inputs(outer, C, inner, 1, 0, dtype, False)
    parts, ds, _ = launch(s, t, outer, C, inner, ss, ts, 2.0, w, 0.37, 0.6, 0)
    assert bool((parts == 0).all()) and bool((ds == 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("outer,C,inner", [(2, 9, 3), (2, 7, 65), (2, 300, 128)])
def test_kd_cols_seed_scale_scales_the_gradient_and_not_the_loss(outer, C, inner, dtype):
    s, t, ss, ts, w = inputs(outer, C, inner, 1, 0, dtype, False)
    parts0, _, _ = launch(s, t, outer, C, inner, ss, ts, 2.0, w, 0.37, 0.6, 0)
    scale = torch.tensor([8.0, 0.125, 0.0, 0.0], device=DEV)
    O.seed_scale(scale)
    parts, ds, _ = launch(s, t, outer, C, inner, ss, ts, 2.0, w, 0.37, 0.6, 0)
    O.seed_scale(None)
    assert torch.equal(parts.view(torch.int32), parts0.view(torch.int32))
    ref = KR.kdcols_ref(s, t, 2.0, w, R.f32(0.37), R.f32(0.6) * 8.0)
    unscaled = KR.kdcols_ref(s, t, 2.0, w, R.f32(0.37), R.f32(0.6))
    R.check(family(inner), f"seed-scaled grad ({outer},{C},{inner}) {dtype}", ds, ref["grad"], ref["grad_env"], dtype, ctrl=unscaled["grad"])


def test_kd_cols_refuses_bad_arguments():
    outer, C, inner = 2, 7, 64
    s, t, ss, ts, w = inputs(outer, C, inner, 1, 0, F32, False)
    n = O.kd_cols_parts(outer, C, inner)
    parts = torch.full((n + 3,), SENT, dtype=F32, device=DEV)
    ds = torch.full((outer * C * inner,), SENT, dtype=F32, device=DEV)
    ok = dict(dtype=0, outer=outer, C=C, inner=inner, s=s.data_ptr(), ss=ss, t=t.data_ptr(), ts=ts, T=1.0, w=None, norm=1.0, coef=1.0,
              part=parts.data_ptr(), n=n, ds=ds.data_ptr(), st=L.stream())
    f = L._fn("magic_kd_cols")
    for k, v in (("outer", 0), ("outer", -1), ("C", 0), ("inner", 0), ("ss", C * inner - 1), ("ts", C * inner - 1), ("T", 0.0), ("T", -1.0),
                 ("s", None), ("t", None), ("part", None), ("n", n + 1), ("n", 0), ("dtype", 3)):
        assert f(*dict(ok, **{k: v}).values()) == -1, (k, v)
    torch.cuda.synchronize()
    assert bool((parts == SENT).all()) and bool((ds == SENT).all()), "a refused call wrote memory"
    assert f(*ok.values()) == 0
    torch.cuda.synchronize()
    assert bool((parts[:n] != SENT).all()) and bool((parts[n:] == SENT).all())
    with pytest.raises(L.MagicHipError):
        O.kd_cols(s, t, outer, C, inner, ss, ts, 1.0, loss_part=parts[:n + 1])
