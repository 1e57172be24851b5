"""magic_chain_fwd (csrc/chain.hip) against float64, stage by stage, at every tile form, launch form and row edge (-m gpu).

References, bounds, inputs and the case table are tests/_chain_ref64.py's (shown right on the CPU by tests/test_chain_ref64_cpu.py, which also
shows every planted defect failing these very checks).  Every case is one launch of at most 4 workgroups at H = 256, I = 1024:
  forms      FFN on / off x Np in {0, 256, 512, 768} x y1 stored / NULL (15), each at M = 33 and 65; the three production forms of host/engine.py
             and (FFN, 768, y1 stored) also at M = 1, 31, 32, 63, 64, 97; every case on the 32-row and on the 64-row kernel, forced, bf16 / fp16
  memory     every output is NaN-filled between NaN guard rows (one in front, 128 behind): what the contract writes is finite, every guard is
             still NaN; the production forms read x as the column slice of an [M, 3H] buffer whose other columns are NaN
  stages     y1, y2, proj against the float64 reference of their own stored input; a y1 = NULL launch must equal, bit for bit, the same launch
             with y1 stored, whose y1 then feeds the references
  controls   the same check FAILS against a reference that lacks the last k-step of the stage's product (y2: of either product)
  twice      the same launch again is bit-identical
  pairs      two problems in one launch (L.group): (Ma, Mb) on both sides of a `split` edge, FFN / no FFN in both orders, different Np, one
             strided input -- every output bit-identical to the two single launches, guards untouched
test_zz_report prints (-s) the worst err / bound and ulps per output, type and tile form; the figures are kept in _chain_ref64's docstring."""
import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from tests import _chain_ref64 as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
BEHIND = 128
DT = list(C.DTYPES.items())
STATS, _PK = {}, {}


@pytest.fixture(params=C.TILE_ROWS, ids=["rows32", "rows64"])
def tile_rows(request):
    before = O.chain_tile_rows()
    assert O.chain_tile_rows(request.param) == request.param
    yield request.param
    O.chain_tile_rows(before)


def packed(o):
    """the weights in fragment order, packed once per type (the kernel's packing equals the mirror)"""
    if o.dtype not in _PK:
        pk = {k: O.pack_frag(getattr(o, k)) for k in ("Wa", "W1", "W2")}
        for Np in (256, 512, 768):
            pk[Np] = O.pack_frag(o.Wp[:Np])
        assert torch.equal(pk["W1"], C.frag_order(o.W1)) and torch.equal(pk[512], C.frag_order(o.Wp[:512]))
        _PK[o.dtype] = pk
    return _PK[o.dtype]


class Out:
    """M rows of an output inside NaN guard rows"""

    def __init__(self, M, cols, dtype):
        self.buf = torch.full((1 + M + BEHIND, cols), NAN, dtype=dtype, device=DEV)
        self.M, self.v = M, self.buf[1:1 + M]

    def check(self, tag):
        assert bool(torch.isfinite(self.v.float()).all()), f"{tag}: elements the contract writes are missing or not finite (NaN input columns?)"
        assert bool(torch.isnan(self.buf[0].float()).all()) and bool(torch.isnan(self.buf[1 + self.M:].float()).all()), f"{tag}: a guard row was written"


def launch(o, ffn, Np, store_y1, strided):
    """one magic_chain_fwd call (queued when inside L.group()) -> {output: Out}"""
    pk = packed(o)
    out = {}
    if store_y1:
        out["y1"] = Out(o.M, C.H, o.dtype)
    if ffn:
        out["y2"] = Out(o.M, C.H, o.dtype)
    if Np:
        out["proj"] = Out(o.M, Np, o.dtype)
    v = lambda k: out[k].v if k in out else None                                        # noqa: E731
    O.chain_fwd(o.x if strided else o.x_flat, o.res, o.M, pk["Wa"], o.ba, o.g1, o.b1, C.EPS, y1=v("y1"),
                ffn=(pk["W1"], o.bi, pk["W2"], o.bo2, o.g2, o.b2, C.I) if ffn else None, y2=v("y2"),
                proj=(pk[Np], o.bp[:Np], Np) if Np else None, proj_out=v("proj"))
    return out


def same_bits(a, b):
    return torch.equal(a.buf.view(torch.int16), b.buf.view(torch.int16))


def checked(out, tag):
    torch.cuda.synchronize()
    for k, b in out.items():
        b.check(f"{tag} {k}")
    return out


@pytest.mark.parametrize("case", C.CASES, ids=[C.case_id(c) for c in C.CASES])
@pytest.mark.parametrize("name,dt", DT)
def test_chain_matches_float64_stage_by_stage(name, dt, case, tile_rows):
    ffn, Np, store_y1, M, strided = case
    assert O.chain_ok(dt, C.H, C.I)
    o = C.operands(dt, M, DEV)
    tag = f"{C.case_id(case)} {name} rows{tile_rows}"
    got = checked(launch(o, ffn, Np, store_y1, strided), tag)
    again = checked(launch(o, ffn, Np, store_y1, strided), tag + " again")
    for k in got:
        assert same_bits(got[k], again[k]), f"{tag} {k}: the same launch twice differs"
    y1 = got.get("y1")
    if not store_y1:                                  # the unsaved stage: pinned through the same launch with y1 stored
        full = checked(launch(o, ffn, Np, True, strided), tag + " with y1")
        for k in got:
            assert same_bits(got[k], full[k]), f"{tag} {k}: differs from the launch that stores y1"
        y1 = full["y1"]
    y2 = got["y2"].v if ffn else None
    refs = C.stage_refs(o, ffn, Np, y1.v, y2)
    ctrl = C.control_refs(o, ffn, Np, y1.v, y2)
    vals = dict({k: b.v for k, b in got.items()}, y1=y1.v)
    for k, ref in refs.items():
        x, u = C.ratio(vals[k], ref, dt), C.ulps(vals[k], ref, dt)
        key = (k, name, tile_rows)
        STATS[key] = tuple(max(a, b) for a, b in zip(STATS.get(key, (0.0, 0.0)), (x, u)))
        print(f"{tag} {k}: err / bound {x:.3f}, {u:.2f} ulp")
        assert x <= 1.0, f"{tag} {k}: err / bound {x:.3f} ({u:.2f} ulp)"
        for i, c in enumerate(ctrl[k]):
            assert C.ratio(vals[k], c, dt) > 1.0, f"{tag} {k}: control {i} (a reference without the last k-step) passes the check"


@pytest.mark.parametrize("order", [0, 1], ids=["ffn_first", "noffn_first"])
@pytest.mark.parametrize("Ma,Mb", C.PAIR_ROWS)
@pytest.mark.parametrize("name,dt", DT)
def test_paired_launch_equals_the_two_single_launches(name, dt, Ma, Mb, order, tile_rows):
    fa, fb = C.PAIR_FORMS[order]
    oa, ob = C.operands(dt, Ma, DEV), C.operands(dt, Mb, DEV)
    tag = f"pair ({Ma}, {Mb}) {fa} | {fb} {name} rows{tile_rows}"
    sa, sb = checked(launch(oa, *fa), tag + " single a"), checked(launch(ob, *fb), tag + " single b")
    with L.group():
        pa, pb = launch(oa, *fa), launch(ob, *fb)
    checked(pa, tag + " a")
    checked(pb, tag + " b")
    for single, pair, side in ((sa, pa, "a"), (sb, pb, "b")):
        assert single.keys() == pair.keys()
        for k in single:
            assert same_bits(single[k], pair[k]), f"{tag}: {side} {k} differs from its single launch"


def test_zz_report():
    """worst err / bound and |err| in ulps of |ref| per output, type and tile form over every case above (run the whole file with -s)"""
    for (k, name, rows), (x, u) in sorted(STATS.items()):
        print(f"chain {k:4s} {name} rows{rows}: worst err / bound {x:.3f}, {u:.2f} ulp")
    if STATS:
        assert {k[0] for k in STATS} <= {"y1", "y2", "proj"} and all(x <= 1.0 for x, _ in STATS.values())
