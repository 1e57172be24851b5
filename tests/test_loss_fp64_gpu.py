"""The loss kernels of csrc/loss.hip against float64 references at every launch branch (-m gpu).

Every reference (tests/_loss_ref64.py, shown right on the CPU by tests/test_loss_ref64_cpu.py) is float64 arithmetic on the operands the kernel reads.
Every comparison is held to REL = 1e-5 of the envelope of the output's terms (+ one unit in the last place of a 16-bit output), and every case shows
that the same comparison FAILS against a reference that lacks one unit of work of the path under test (the last column, vector, row, grid-stride
trip or problem; for the large loss words: each probe element alone).  Outputs are pre-filled with a sentinel: promised padding is zero, everything
else past a row's extent and past the last row is untouched.

Launch branches entered here (dispatch conditions of magic_ce_rows, magic_kd_rows, magic_mse, magic_mse_multi):
  ce_rows     wide <*, 256> (M = 513) with two vectors per thread; wide <*, 1024> with a second trip (N = 8200); both sides of N = 2048; the narrow
              kernel through ld/ldd = N, a misaligned base, accumulate (a 16-bit row of 2051 columns included); ldd > ld; every row ignored
  kd_rows     register passes 1 .. 8 (N = 1 .. 512), ld > N, partial last workgroup (M = 1, 5), coef_dev, accumulate, norm
  softkl_rows three dtypes, N on each side of the 256-thread block, distinct ld / ldt / ldd, row weights, zero and half-mass target rows
  mse         second grid-stride trip under the 384-block cap, rows_per_w > 1, accumulate, coef_dev, both gradient types
  mse_multi   minimum-one-block share, second unrolled load live for a few lanes, second loop trip, scalar 16-bit body (inner % 8, sliced base),
              fp32 inputs in a 16-bit launch, accumulate x gradient type, device-side extents on the vector body, fp16, the fp32 launch
  cfp_loss    fp16; B = 1 .. 64, H = 8 .. 256
  loss_assemble  more than one pass of the 256-thread block

Largest err / bound per family on an MI355X: NOT MEASURED YET -- these tests were written without a GPU run; every call of R.check prints its
figure (`pytest -s`), and the first run fills this in.  REL = 1e-5 is kept for every family until a measurement says otherwise.
Not assertable: with N = 1 (ce, kd) and B = 1 (cfp) the outputs are identically zero, so no reference can lack anything -- those cases check the
values and the untouched memory only."""
import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from tests import _loss_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
HALF = [torch.bfloat16, torch.float16]
F32 = torch.float32
SENT = 7.0


@pytest.fixture(autouse=True)
def _no_seed_scale():
    O.seed_scale(None)
    yield
    O.seed_scale(None)


def gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)


def sent(*shape, dtype=F32):
    return torch.full(shape, SENT, dtype=dtype, device=DEV)


def untouched(t):
    return bool((t == SENT).all())


def ceil8(n):
    return (n + 7) // 8 * 8


# ------------------------------------------------------------------------------------------ ce_rows
CE_SHAPES = [(513, 2051), (3, 8200), (3, 2048), (3, 2047), (5, 255), (5, 256), (5, 257), (5, 1)]


def ce_inputs(M, N, dtype):
    rn = gen(M * 100003 + N)
    ld = ceil8(N)
    x = torch.zeros(M, ld, dtype=torch.float64)
    x[:, :N] = 2 * rn(M, N)
    pv = (N - 1) // 8 * 8                                   # first column of the last (partial) vector
    pat = [0, N - 1, pv, -100, N // 2]
    labels = torch.tensor([pat[r % 5] for r in range(M)], dtype=torch.int32)
    if N > 1:
        x[:, N - 1] = 4.0                                   # the last column carries weight in every row
    if N > 8:
        x[0, 3] = float("-inf")
        x[2, 0] = float("-inf")
    return x.to(dtype).to(DEV), labels.to(DEV), (rn(M).abs() + 0.25).float().to(DEV), ld


def ce_ctrl(x, labels, N, roww, coef, rate):
    """the reference without the last column (None when N = 1: nothing is left)"""
    if N == 1:
        return None
    c = R.ce_ref(x[:, :N - 1], labels, coef, roww, w_rate=rate)
    c["grad"] = R.pad_cols(c["grad"], N)
    return c


def ce_check(tag, dtype, ref, ctrl, N, loss_row, w_out, d, M, ldd):
    k = (lambda key: None if ctrl is None else ctrl[key])
    R.check("ce", f"loss {tag}", loss_row[:M], ref["loss"], ref["loss_env"], ctrl=k("loss"))
    R.check("ce", f"w_out {tag}", w_out[:M], ref["w"], ref["w_env"], ctrl=k("w"))
    R.check("ce", f"grad {tag}", d[:M, :N], ref["grad"], ref["grad_env"], dtype, ctrl=k("grad"))
    assert (d[:M, N:ldd] == 0).all(), f"{tag}: padding columns [N, ldd) not zero"
    assert untouched(d[M:]) and untouched(loss_row[M:]) and untouched(w_out[M:]), f"{tag}: memory past the last row written"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N", CE_SHAPES)
def test_ce_rows_every_launch_form_matches_float64(M, N, dtype):
    x, labels, roww, ld = ce_inputs(M, N, dtype)
    coef, rate = 0.37, 0.7
    ref = R.ce_ref(x[:, :N], labels, coef, roww, w_rate=rate)
    ctrl = ce_ctrl(x, labels, N, roww, coef, rate)
    flat = torch.zeros(M * ld + 8, dtype=dtype, device=DEV)
    x_off = flat[1:1 + M * ld].view(M, ld)                  # base off by one element: never the vector kernel
    x_off.copy_(x)
    for tag, xin, ldd in (("aligned", x, ld), ("ldd=ld+8", x, ld + 8), ("base+1", x_off, ld)):
        loss_row, w_out = sent(M + 3), sent(M + 3)
        dflat = sent((M + 1) * ldd + 8, dtype=dtype)
        d = (dflat[1:1 + (M + 1) * ldd] if tag == "base+1" else dflat[:(M + 1) * ldd]).view(M + 1, ldd)
        O.ce_rows(xin, M, N, ld, labels, coef=coef, row_w=roww, loss_row=loss_row, dlogits=d, ldd=ldd, w_out=w_out, w_rate=rate)
        torch.cuda.synchronize()
        ce_check(f"{tag} M={M} N={N} {dtype}", dtype, ref, ctrl, N, loss_row, w_out, d, M, ldd)
        assert untouched(dflat[(M + 1) * ldd + 1:]) and (tag != "base+1" or untouched(dflat[:1]))
    # every row ignored: zero loss, unit weight, zero gradient -- exactly
    ign = torch.full((M,), -100, dtype=torch.int32, device=DEV)
    loss_row, w_out, d = sent(M + 3), sent(M + 3), sent(M + 1, ld, dtype=dtype)
    O.ce_rows(x, M, N, ld, ign, coef=coef, row_w=roww, loss_row=loss_row, dlogits=d, ldd=ld, w_out=w_out, w_rate=rate)
    torch.cuda.synchronize()
    assert (loss_row[:M] == 0).all() and (w_out[:M] == 1).all() and (d[:M] == 0).all() and untouched(d[M:]) and untouched(loss_row[M:])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N", [(5, 257), (3, 2051)])
def test_ce_rows_accumulates_into_a_prefilled_gradient(M, N, dtype):
    """accumulate = 1 is the narrow kernel at every width: a 16-bit row of 2051 columns reaches it no other way"""
    x, labels, roww, ld = ce_inputs(M, N, dtype)
    init = gen(N)(M, ld).to(dtype).to(DEV)
    ref = R.ce_ref(x[:, :N], labels, 0.37, roww)
    ctrl = ce_ctrl(x, labels, N, roww, 0.37, 0.0)
    i64 = init[:, :N].double()
    d = sent(M + 1, ld, dtype=dtype)
    d[:M] = init
    O.ce_rows(x, M, N, ld, labels, coef=0.37, row_w=roww, dlogits=d, ldd=ld, accumulate=True)
    torch.cuda.synchronize()
    R.check("ce", f"accumulate M={M} N={N} {dtype}", d[:M, :N], i64 + ref["grad"], i64.abs() + ref["grad_env"], dtype,
            ctrl=[i64 + ctrl["grad"], i64 + ref["grad"] * (torch.arange(M, device=DEV) < M - 1)[:, None]])        # last column; last row
    assert (d[:M, N:] == 0).all() and untouched(d[M:])


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("M,N", [(513, 2051), (3, 8200)])
def test_ce_rows_wide_forms_in_place_equal_out_of_place_bitwise(M, N, dtype):
    x, labels, roww, ld = ce_inputs(M, N, dtype)
    d = sent(M, ld, dtype=dtype)
    O.ce_rows(x, M, N, ld, labels, coef=0.37, row_w=roww, dlogits=d, ldd=ld)
    x2 = x.clone()
    O.ce_rows(x2, M, N, ld, labels, coef=0.37, row_w=roww, dlogits=x2, ldd=ld)
    torch.cuda.synchronize()
    assert torch.equal(d.view(torch.int16), x2.view(torch.int16))
    ref = R.ce_ref(x[:, :N], labels, 0.37, roww)
    R.check("ce", f"in-place M={M} N={N} {dtype}", x2[:, :N], ref["grad"], ref["grad_env"], dtype, ctrl=ce_ctrl(x, labels, N, roww, 0.37, 0.0)["grad"])


# ------------------------------------------------------------------------------------------ kd_rows
@pytest.mark.parametrize("M", [1, 5, 8])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 128, 129, 449, 511, 512])
def test_kd_rows_every_register_pass_matches_the_oracle_in_float64(N, M):
    rn = gen(N * 17 + M)
    ld, T = N + 3, 2.0
    s, t = sent(M + 1, ld), sent(M + 1, ld)
    s[:M, :N], t[:M, :N] = (2 * rn(M, N)).float().to(DEV), (2 * rn(M, N)).float().to(DEV)
    if N > 3:
        for r in range(M):                                  # -inf at the same place in student and teacher; row 0 keeps a live last column
            s[r, N - 1 - ((r + 1) % 3)] = float("-inf")
            t[r, N - 1 - ((r + 1) % 3)] = float("-inf")
    w = (rn(M).abs() + 0.25).float().to(DEV)
    cdev = torch.tensor([0.5], device=DEV)
    init = rn(M, N).float().to(DEV)
    for tag, kw, rkw, acc in (("plain", dict(coef=0.6), dict(coef=0.6), False),
                              ("w+coef_dev+accumulate+norm", dict(w=w, norm=1.0 / M, coef=0.6, coef_dev=cdev), dict(w=w, norm=R.f32(1.0 / M), coef=R.f32(0.6) * 0.5), True)):
        rows, renv, grad, genv = R.kd_ref(s[:M, :N], t[:M, :N], T, **rkw)
        base = init.double() if acc else torch.zeros_like(grad)
        c_rows = c_grad = None
        if N > 1:
            c_rows, _, cg, _ = R.kd_ref(s[:M, :N - 1], t[:M, :N - 1], T, **rkw)
            c_grad = base + R.pad_cols(cg, N)
        loss_row, ds = sent(M + 3), sent(M + 1, ld)
        if acc:
            ds[:M, :N] = init
        O.kd_rows(s, t, M, N, ld, T, loss_row=loss_row, ds=ds, accumulate=acc, **kw)
        torch.cuda.synchronize()
        name = f"{tag} M={M} N={N}"
        R.check("kd", f"loss {name}", loss_row[:M], rows, renv, ctrl=c_rows)
        R.check("kd", f"grad {name}", ds[:M, :N], base + grad, base.abs() + genv, ctrl=c_grad)
        assert untouched(ds[:M, N:]) and untouched(ds[M:]) and untouched(loss_row[M:]), name


# ------------------------------------------------------------------------------------------ softkl_rows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 255, 257, 1000])
def test_softkl_rows_matches_float64(N, dtype):
    rn = gen(N)
    M, ld, ldt, ldd = 3, N + 5, N + 2, N + 9
    x = sent(M + 1, ld, dtype=dtype)
    x[:M, :N] = (2 * rn(M, N)).to(dtype).to(DEV)
    t = sent(M + 1, ldt)
    tt = torch.softmax(rn(M, N), 1)
    tt[1] = 0.0                                             # a target row of zeros
    tt[2] *= 0.5                                            # a row whose mass is 0.5
    t[:M, :N] = tt.float().to(DEV)
    roww = (rn(M).abs() + 0.25).float().to(DEV)
    for rw in (None, roww):
        ref = R.softkl_ref(x[:M, :N], t[:M, :N], 0.37, rw)
        if N > 1:
            c = R.softkl_ref(x[:M, :N - 1], t[:M, :N - 1], 0.37, rw)
            c_loss, c_grad = c["loss"], R.pad_cols(c["grad"], N)
        else:                                               # one column: the gradient is identically zero, the loss t log t is not
            c_loss, c_grad = torch.zeros_like(ref["loss"]), None
        rows, d = sent(M + 3), sent(M + 1, ldd, dtype=dtype)
        O.softkl_rows(x, M, N, ld, t, coef=0.37, row_w=rw, loss_row=rows, dlogits=d, ldd=ldd)
        torch.cuda.synchronize()
        name = f"N={N} {dtype} row_w={rw is not None}"
        R.check("softkl", f"loss {name}", rows[:M], ref["loss"], ref["loss_env"], ctrl=c_loss)
        R.check("softkl", f"grad {name}", d[:M, :N], ref["grad"], ref["grad_env"], dtype, ctrl=c_grad)
        assert (d[:M, N:] == 0).all() and untouched(d[M:]) and untouched(rows[M:]), name


# ------------------------------------------------------------------------------------------ mse / mse_multi
def mse_problem(seed, dtype, outer, inner, *, gdtype=None, pads=(8, 16, 24), off=0, units=(), w=None, rows_per_w=1, accumulate=False, valid=None, valid_mod=0,
                norm=0.5, coef=0.8, coef_dev=None, norm_dev=None, loss_init=0.0, ctrl_from=None):
    """one MSE problem: operands with distinct row pitches (inner + pads), small noise with large differences at the seams, a sentinel-filled
    gradient (or a pre-filled one to accumulate into), the float64 terms / gradient and the launch keywords.  off: slice every base by `off` elements"""
    gdtype = gdtype or dtype
    n = outer * inner
    pos = R.seams(n, (8, inner) + tuple(units))
    dd = R.probe_data(n, pos, 1e-2, 4.0, seed).view(outer, inner)
    rn = gen(seed + 1)
    ss, ts, gs = (inner + p for p in pads)

    def buf(rows, pitch, dt, fill):
        flat = torch.full((rows * pitch + 8,), fill, dtype=dt, device=DEV)
        return flat, flat[off:off + rows * pitch].view(rows, pitch)
    _, t = buf(outer, ts, dtype, 0.0)
    _, s = buf(outer, ss, dtype, 0.0)
    t64 = (0.5 * rn(outer, inner)).to(dtype)
    t[:, :inner] = t64.to(DEV)
    s[:, :inner] = (t64.double() + dd).to(dtype).to(DEV)
    gflat, g = buf(outer + 1, gs, gdtype, SENT)
    init = None
    if accumulate:
        init = rn(outer, inner).to(gdtype).to(DEV)
        g[:outer, :inner] = init
    loss = torch.full((2,), SENT, device=DEV)
    loss[0] = loss_init
    vt = None if valid is None else torch.tensor(valid, dtype=torch.int32, device=DEV)
    nd = None if norm_dev is None else torch.tensor([norm_dev], device=DEV)
    cd = None if coef_dev is None else torch.tensor([coef_dev], device=DEV)
    nrm = R.f32(norm) * (R.f32(norm_dev) if norm_dev is not None else 1.0)
    cf = R.f32(coef) * (R.f32(coef_dev) if coef_dev is not None else 1.0)
    terms, grad = R.mse_ref(s[:, :inner], t[:, :inner], w, rows_per_w, nrm, cf, valid, valid_mod)
    kw = dict(s=s, t=t, outer=outer, inner=inner, s_stride=ss, t_stride=ts, w=w, rows_per_w=rows_per_w, norm=norm, coef=coef, coef_dev=cd, loss=loss[0:1],
              ds=g, g_stride=gs, accumulate=accumulate)
    return dict(kw=kw, multi=dict(kw, valid_dev=vt, norm_dev=nd, valid_mod=valid_mod), terms=terms, grad=grad, init=init, g=g, gflat=gflat, loss=loss,
                loss_init=loss_init, pos=pos, gdtype=gdtype, outer=outer, inner=inner, off=off, ctrl_from=n - 1 if ctrl_from is None else ctrl_from)


def mse_check(fam, name, q, dropped=False):
    """loss word by probes (every seam element alone breaks it), gradient against float64 with the control `everything from ctrl_from on is missing`;
    dropped: the whole problem is the missing unit (the word and the gradient as they were before the launch must fail)"""
    outer, inner = q["outer"], q["inner"]
    terms = q["terms"].reshape(-1)
    pos = [p for p in q["pos"] if terms[p] != 0]
    assert pos, name
    R.check_probes(fam, f"loss {name}", q["loss"][0], q["loss_init"], terms, pos)
    base = q["init"].double() if q["init"] is not None else torch.zeros_like(q["grad"])
    ref, env = base + q["grad"], base.abs() + q["grad"].abs()
    keep = (torch.arange(outer * inner, device=DEV) < q["ctrl_from"]).view(outer, inner)
    ctrl = [base + q["grad"] * keep]
    if dropped:
        ctrl.append(base if q["init"] is not None else torch.full_like(ref, SENT))
        assert abs(q["loss_init"] - float(q["loss"][0])) > R.REL * terms.abs().sum().item(), name
    R.check(fam, f"grad {name}", q["g"][:outer, :inner], ref, env, q["gdtype"], ctrl=ctrl)
    gf, off, n = q["gflat"], q["off"], (outer + 1) * q["g"].shape[1]
    assert untouched(q["g"][:outer, inner:]) and untouched(q["g"][outer:]) and untouched(gf[:off]) and untouched(gf[off + n:]) and untouched(q["loss"][1:]), \
        f"{name}: memory outside the gradient's extent written"


@pytest.mark.parametrize("dtype,gdtype", [(F32, F32), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, F32), (torch.float16, torch.float16), (torch.float16, F32)])
def test_mse_second_grid_stride_trip_matches_float64(dtype, gdtype):
    """7 x 15001 = 105 007 elements over the 384-block cap (98 304 per trip): the loop body runs a second trip"""
    w = torch.tensor([0.5, 1.5, 0.75], device=DEV)
    trip = 384 * 256
    for tag, extra in (("fresh", dict(coef_dev=0.5)), ("accumulate", dict(accumulate=True, loss_init=3.0))):
        q = mse_problem(3, dtype, 7, 15001, gdtype=gdtype, units=(256, trip), w=w, rows_per_w=3, ctrl_from=trip, **extra)
        assert trip in q["pos"] and trip - 1 in q["pos"]
        O.mse(**q["kw"])
        torch.cuda.synchronize()
        mse_check("mse", f"{tag} {dtype}->{gdtype}", q)


def multi_run(fam, name, probs, dropped_last=False):
    O.mse_multi([q["multi"] for q in probs])
    torch.cuda.synchronize()
    for i, q in enumerate(probs):
        mse_check(fam, f"{name} problem {i}", q, dropped=dropped_last and i == len(probs) - 1)


@pytest.mark.parametrize("dtype", HALF)
def test_mse_multi_small_problems_each_get_their_one_block(dtype):
    """(a) one problem of 2.1M elements and nine of 8 .. 64: by size the small ones would get no block at all"""
    big = mse_problem(1, dtype, 8, 262152, units=(8 * 1024, 8 * 1024 * 256), ctrl_from=8 * 1024 * 256)
    small = [mse_problem(10 + i, dtype, 1, n) for i, n in enumerate((8, 16, 24, 32, 40, 48, 56, 64, 64))]
    multi_run("mse_multi", f"(a) {dtype}", [big] + small, dropped_last=True)


@pytest.mark.parametrize("dtype,gdtype", [(torch.bfloat16, torch.bfloat16), (torch.float16, F32)])
def test_mse_multi_second_unrolled_load_live_for_a_few_lanes(dtype, gdtype):
    """(b) 9 x (8 x 29 131): 262 179 vectors for 256 x 1024 lanes -- the second load of the 2-way unrolled loop serves 35 vectors"""
    first = 8 * 1024 * 256
    q = mse_problem(2, dtype, 9, 8 * 29131, gdtype=gdtype, units=(8 * 1024, first), ctrl_from=first)
    assert first in q["pos"] and q["outer"] * q["inner"] - first == 8 * 35
    multi_run("mse_multi", f"(b) {dtype}->{gdtype}", [q])
    q2 = mse_problem(2, dtype, 9, 8 * 29131, gdtype=gdtype, units=(8 * 1024, first), ctrl_from=9 * 8 * 29131 - 8)        # the last 8-element vector
    multi_run("mse_multi", f"(b') {dtype}->{gdtype}", [q2])


@pytest.mark.parametrize("dtype", HALF)
def test_mse_multi_two_equal_problems_take_a_second_loop_trip(dtype):
    """(c) 128 blocks each: one trip of the unrolled loop covers 2 x 128 x 1024 vectors, the problems have 262 400"""
    trip = 8 * 2 * 128 * 1024
    probs = [mse_problem(20 + i, dtype, 4, 8 * 65600, units=(8 * 128 * 1024, trip), ctrl_from=trip) for i in range(2)]
    assert all(trip in q["pos"] for q in probs)
    multi_run("mse_multi", f"(c) {dtype}", probs, dropped_last=True)


@pytest.mark.parametrize("dtype", HALF)
def test_mse_multi_scalar_body_in_a_16_bit_launch(dtype):
    """(d) inner % 8 != 0, and a base sliced by one element; (f) accumulate with both gradient types, scalar and vector body"""
    w = torch.tensor([0.5, 1.5], device=DEV)
    probs = [mse_problem(30, dtype, 5, 1003, pads=(5, 13, 21), units=(1024,), w=w, rows_per_w=3),
             mse_problem(31, dtype, 5, 1000, off=1, units=(1024,)),
             mse_problem(32, dtype, 5, 1003, gdtype=F32, accumulate=True, units=(1024,)),
             mse_problem(33, dtype, 5, 1000, off=1, accumulate=True, loss_init=2.0, units=(1024,)),
             mse_problem(34, dtype, 5, 1024, accumulate=True, units=(1024,)),
             mse_problem(35, dtype, 5, 1024, gdtype=F32, accumulate=True, units=(1024,), coef_dev=0.5)]
    multi_run("mse_multi", f"(d,f) {dtype}", probs, dropped_last=True)


@pytest.mark.parametrize("dtype", HALF)
def test_mse_multi_fp32_inputs_ride_in_a_16_bit_launch(dtype):
    """(e) descriptor flag bit 1"""
    probs = [mse_problem(40, dtype, 3, 64), mse_problem(41, F32, 6, 1003, units=(1024,)), mse_problem(42, F32, 4, 2048, units=(1024,), accumulate=True)]
    multi_run("mse_multi", f"(e) {dtype}", probs, dropped_last=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mse_multi_device_side_extents(dtype):
    """(g) valid_dev / valid_mod / norm_dev with a valid width that is no multiple of 8 (vector body in 16-bit, scalar body in fp32 and with inner % 8)"""
    probs = [mse_problem(50, dtype, 6, 2 * 96, valid=(5, 77), valid_mod=96, norm_dev=0.25, ctrl_from=4 * 192 + 96),
             mse_problem(51, dtype, 6, 200, gdtype=F32, valid=(4, 133), norm_dev=0.5, ctrl_from=3 * 200),
             mse_problem(52, dtype, 3, 2 * 1003, pads=(5, 13, 21), valid=(3, 77), valid_mod=1003, ctrl_from=2 * 2006)]
    O.mse_multi([q["multi"] for q in probs])
    torch.cuda.synchronize()
    for i, q in enumerate(probs):
        mse_check("mse_multi", f"(g) {dtype} problem {i}", q)
        assert (q["grad"] == 0).any() and (q["g"][:q["outer"], :q["inner"]][q["grad"] == 0] == 0).all()         # outside the valid extent: exactly zero


# ------------------------------------------------------------------------------------------ cfp_loss
CFP_SHAPES = [(1, 8), (1, 256), (64, 8), (64, 256), (2, 72), (17, 248), (63, 72), (17, 8), (63, 256)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H", CFP_SHAPES)
def test_cfp_loss_matches_float64(B, H, dtype):
    rn = gen(B * 1000 + H)
    a = [(0.5 * rn(B, H)).to(dtype).to(DEV) for _ in range(3)]
    txt = (0.5 * rn(B, H)).to(dtype).to(DEV)
    temp, coef = 0.7, 0.37 / B
    assert O.cfp_loss_ok(B, H)

    def launch(grads):
        rows = sent(6 * B + 4)
        d_a = [sent(B + 1, H, dtype=dtype) for _ in range(3)] if grads else None
        d_t = sent(B + 1, H, dtype=dtype) if grads else None
        O.cfp_loss(B, H, a, txt, temp, coef, rows, d_a=d_a, d_txt=d_t)
        return rows, d_a, d_t
    rows, d_a, d_t = launch(True)
    rows2, d_a2, d_t2 = launch(True)                       # the last-block counter resets itself
    rows_f, _, _ = launch(False)
    torch.cuda.synchronize()
    assert torch.equal(rows, rows_f) and torch.equal(rows, rows2) and torch.equal(d_t, d_t2) and all(torch.equal(x, y) for x, y in zip(d_a, d_a2))
    r64, renv, g_a, g_a_env, g_t, g_t_env = R.cfp_ref(a, txt, R.f32(temp), R.f32(coef))
    c = None
    if B > 1:                                               # the reference without sample B - 1
        pad = lambda m: torch.cat([m, m.new_zeros((1,) + m.shape[1:])], 0)
        cr, _, ca, _, ct, _ = R.cfp_ref([x[:B - 1] for x in a], txt[:B - 1], R.f32(temp), R.f32(coef))
        c = dict(rows=R.pad_cols(cr, B), d_a=[pad(x) for x in ca], d_t=pad(ct))
    name = f"B={B} H={H} {dtype}"
    R.check("cfp", f"rows {name}", rows[:6 * B].view(6, B), r64, renv, ctrl=c and c["rows"])
    for i in range(3):
        R.check("cfp", f"d_a{i} {name}", d_a[i][:B], g_a[i], g_a_env[i], dtype, ctrl=c and c["d_a"][i])
        assert untouched(d_a[i][B:])
    R.check("cfp", f"d_txt {name}", d_t[:B], g_t, g_t_env, dtype, ctrl=c and c["d_t"])
    assert untouched(d_t[B:]) and untouched(rows[6 * B:]) and untouched(rows_f[6 * B:])


# ------------------------------------------------------------------------------------------ loss_assemble
@pytest.mark.parametrize("n_rows", [1, 255, 257, 1000])
def test_loss_assemble_all_outputs_match_float64(n_rows):
    rn = gen(n_rows)
    pos = R.seams(n_rows, (64, 256))
    rows = R.probe_data(n_rows, pos, 1e-3, 8.0, n_rows).float().to(DEV)
    roww = (rn(n_rows).abs() + 0.5).float().to(DEV)
    rw = (rn(5).abs() + 0.2).float().to(DEV)
    for n_kd in (1, 300):
        kpos = R.seams(n_kd, (64, 256))
        kd = R.probe_data(n_kd, kpos, 1e-3, 8.0, n_kd + 1).float().to(DEV)
        for weighted in (False, True):
            for has_kd in (False, True):
                slots = torch.cat([rn(10), torch.full((1,), SENT, dtype=torch.float64)]).float().to(DEV)
                s0 = slots[:10].clone()
                out = sent(16)
                O.loss_assemble(rows, roww if weighted else None, 0.37, kd, slots[:10], rw if weighted else None, 0.3, has_kd, out[:13])
                torch.cuda.synchronize()
                ref, env, s9, terms = R.assemble_ref(rows, roww if weighted else None, 0.37, kd, s0, rw if weighted else None, 0.3, has_kd)
                name = f"n_rows={n_rows} n_kd={n_kd} weighted={weighted} has_kd={has_kd}"
                c_rows, _, _, _ = R.assemble_ref(rows[:-1], roww[:-1] if weighted else None, 0.37, kd, s0, rw if weighted else None, 0.3, has_kd)      # the last row
                R.check("assemble", name, out[:13], ref, env, ctrl=c_rows)
                R.check_probes("assemble", f"sup {name}", out[0], 0.0, terms, pos)
                R.check_probes("assemble", f"slots[9] {name}", slots[9], 0.0, kd.double(), kpos)
                assert torch.equal(slots[:9], s0[:9]) and untouched(slots[10:]) and untouched(out[13:]), name


# ------------------------------------------------------------------------------------------ error returns
def test_loss_launches_refuse_what_they_cannot_serve():
    z = torch.zeros(70, 520, device=DEV)
    with pytest.raises(L.MagicHipError):
        O.kd_rows(z, z, 2, 513, 520, 2.0, loss_row=torch.zeros(2, device=DEV))
    a = [torch.zeros(65, 16, device=DEV) for _ in range(3)]
    with pytest.raises(L.MagicHipError):
        O.cfp_loss(65, 16, a, a[0], 0.7, 1.0, torch.zeros(6 * 65, device=DEV))
    b = [torch.zeros(4, 12, device=DEV) for _ in range(3)]
    with pytest.raises(L.MagicHipError):
        O.cfp_loss(4, 12, b, b[0], 0.7, 1.0, torch.zeros(24, device=DEV))
    x = torch.zeros(3, 16, device=DEV)
    with pytest.raises(L.MagicHipError):
        O.softkl_rows(x, 3, 16, 16, torch.zeros(3, 16, device=DEV), coef=1.0, dlogits=x, ldd=16)
    torch.cuda.synchronize()
    assert (x == 0).all()
