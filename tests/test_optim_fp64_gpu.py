"""The optimizer-tail kernels of csrc/optim.hip against float64 references at every launch branch (-m gpu).

Same rules as tests/test_loss_fp64_gpu.py: float64 references from the operands the kernels read (tests/_loss_ref64.py), REL = 1e-5 of the terms'
envelope (+ one unit in the last place of a 16-bit output), a reference lacking one unit of work must fail the same comparison, sentinels past every
buffer's extent.

Launch branches entered here (nblocks and the grid caps of magic_sumsq, magic_adamw, magic_add_n, magic_cast, magic_add, magic_dact):
  sumsq / sumsq_sched   1 block .. the 256-block cap (first binding at n = 2^20 + 3), the second trip of the four-in-flight loop with its scalar tail
                        (n = 4 x 256 x 1024 x 4 + 7), n & 3 = 1, 2, 3 alone and behind vectors; probes on each side of every vector, block and stride seam
  adamw                 decay_first both ways, n_decay inside the range, gscale != 1, clip active and inactive, lr / step size from device memory,
                        fp16 and bf16 shadows, past the 2048-block cap (n = 2048 x 256 + 5)
  add_n                 (no test before) 1, 3, 8 addends, vector body only, tail only, both, past the 2048-block cap
  cast / add / dact     n & 3 tails and the grid-stride loop past the 2048-block cap, both 16-bit types

Largest err / bound per family on an MI355X: NOT MEASURED YET -- these tests were written without a GPU run; every call of R.check prints its
figure (`pytest -s`), and the first run fills this in.  REL = 1e-5 is kept for every family until a measurement says otherwise.
"""
import math

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
CAP = 2048 * 256                                           # elements of one grid-stride trip of the 256-thread kernels


@pytest.fixture(autouse=True)
def _no_seed_scale():
    O.seed_scale(None)
    yield
    O.seed_scale(None)


def gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)


def guarded(x, dtype=None):
    """x in a buffer with 8 sentinel elements behind it: (view of the first n, the guard)"""
    x = x.to(dtype or x.dtype)
    buf = torch.full((x.numel() + 8,), SENT, dtype=x.dtype, device=DEV)
    buf[:x.numel()] = x.to(DEV)
    return buf[:x.numel()], buf[x.numel():]


def untouched(t):
    return bool((t == SENT).all())


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


# ------------------------------------------------------------------------------------------ sumsq
SUMSQ_N = [1, 2, 3, 5, 4095, 4097, 2 ** 20 + 3, 4 * 256 * 1024 * 4 + 7]


@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq_and_sumsq_sched_match_a_float64_sum_at_every_seam(n):
    pos = R.sumsq_seams(n)
    g, guard = guarded(R.probe_data(n, pos, 1e-3, 8.0, n), F32)
    terms = g.double() ** 2
    out = torch.tensor([2.0, SENT], device=DEV)
    O.sumsq(g, out[0:1])
    torch.cuda.synchronize()
    R.check_probes("sumsq", f"sumsq n={n}", out[0], 2.0, terms, pos)
    for gs, t in ((3, 3), (50, 41)):                        # inside the warm-up, and on the decay
        out = torch.tensor([0.5, SENT], device=DEV)
        step = torch.tensor([gs, t, 77], dtype=torch.int32, device=DEV)
        lr_ss = torch.full((3,), SENT, device=DEV)
        O.sumsq_sched(g, out[0:1], step, 1e-3, 10, 1000, 0.9, 0.98, lr_ss)
        torch.cuda.synchronize()
        R.check_probes("sumsq", f"sumsq_sched n={n} gs={gs}", out[0], 0.5, terms, pos)
        assert step.tolist() == [gs + 1, t + 1, 77]
        lr, ss = R.sched_ref(gs, t + 1, 1e-3, 10, 1000, 0.9, 0.98)
        assert abs(lr_ss[0].item() - lr) <= 2.0 ** -23 * lr and abs(lr_ss[1].item() - ss) <= 2.0 ** -23 * ss and untouched(lr_ss[2:])
    assert untouched(guard) and untouched(out[1:])


# ------------------------------------------------------------------------------------------ adamw
HYP = dict(lr=1e-2, b1=0.9, b2=0.98, eps=1e-6, wd=0.1)


@pytest.mark.parametrize("shadow_dt", [None] + HALF)
@pytest.mark.parametrize("decay_first", [False, True])
@pytest.mark.parametrize("n", [1, 255, 257, CAP + 5])
def test_adamw_three_steps_match_the_float64_restatement(n, decay_first, shadow_dt):
    rn = gen(n)
    # weights and second moments bounded away from zero, as a trained model's are: the per-element bound REL (|p| + |lr wd p| + |update|) is relative to
    # p, and next to a weight of 1e-5 the fp32 rounding of m alone (6e-8 of |b1 m| + |(1 - b1) g|) would be a visible share of it
    z = rn(n)
    p0, m0, v0 = (torch.sign(z) * (0.5 + z.abs())).float(), (0.1 * rn(n)).float(), (0.01 * (0.25 + rn(n) ** 2)).float()
    grads = [rn(n).float() for _ in range(3)]
    # (n_decay, clipping: the norm is over / under max_norm / no norm word passed, lr and step size from device memory)
    for nd, clipping, dev_lr in ((-1, "active", True), (0, "inactive", False), (n // 2, "active", False), (n, "none", True)):
        (p, pg), (m, mg), (v, vg) = guarded(p0), guarded(m0), guarded(v0)
        shadow, sg = guarded(torch.zeros(n), shadow_dt) if shadow_dt else (None, None)
        p64, m64, v64 = p.double(), m.double(), v.double()
        for t, g_cpu in enumerate(grads, 1):
            g, gg = guarded(g_cpu)
            g_before = g.clone()
            ss = (g.double() ** 2).sum().float().reshape(1) if clipping != "none" else None
            max_norm = {"active": 0.5 * math.sqrt(ss.item()) * 0.125, "inactive": 1e9}[clipping] if ss is not None else 0.0
            step_size = HYP["lr"] * math.sqrt(1 - HYP["b2"] ** t) / (1 - HYP["b1"] ** t)
            lr_ss = torch.tensor([HYP["lr"], step_size], device=DEV) if dev_lr else None
            zero = t == 3
            O.adamw(n, p, g, m, v, shadow, 0.0 if dev_lr else HYP["lr"], HYP["b1"], HYP["b2"], HYP["eps"], HYP["wd"], 0.0 if dev_lr else step_size,
                    ss, max_norm, 0.125, lr_ss=lr_ss, n_decay=nd, zero_grad=zero, decay_first=decay_first)
            torch.cuda.synchronize()
            clip = R.clip_ref(None if ss is None else ss.item(), max_norm, 0.125)
            assert (clip < 0.1) == (clipping == "active"), "the clip is active exactly where the case means it to be"
            kw = dict(HYP, step_size=step_size, clip=clip, decay_first=decay_first)
            prev = p64
            p64, m64, v64, penv, menv, venv = R.adamw_ref(p64, g_before, m64, v64, n_decay=nd, **kw)       # from the state this launch was handed
            ctrl = [torch.cat([p64[:-1], prev[-1:]])]                                              # the last element never updated
            if n > CAP:
                ctrl.append(torch.cat([p64[:CAP], prev[CAP:]]))                                  # the second grid-stride trip
            nd_eff = n if nd < 0 else nd
            if nd_eff > 0:                                                                       # the last decayed element without its decay
                ctrl.append(torch.where(torch.arange(n, device=DEV) == nd_eff - 1, _no_decay(prev, p64, kw), p64))
            name = f"n={n} decay_first={decay_first} n_decay={nd} clip {clipping} step {t}"
            R.check("adamw", f"p {name}", p, p64, penv, ctrl=ctrl)
            R.check("adamw", f"m {name}", m, m64, menv)
            R.check("adamw", f"v {name}", v, v64, venv)
            if shadow is not None:
                assert torch.equal(bits(shadow), bits(p.to(shadow_dt))), f"shadow {name}"
                assert untouched(sg)
            assert (g == 0).all() if zero else torch.equal(g, g_before), f"zero_grad {name}"
            assert untouched(pg) and untouched(mg) and untouched(vg) and untouched(gg), name
            # the next step's reference starts from what the next launch reads (p, m, v as passed): a moment that came out of a cancellation carries
            # the fp32 rounding of its terms, which no later step's envelope knows about
            p64, m64, v64 = p.double(), m.double(), v.double()


def _no_decay(prev, p64, kw):
    """p64 with every element's weight decay taken out again (both orders of the decay)"""
    lr, wd = R.f32(kw["lr"]), R.f32(kw["wd"])
    if kw["decay_first"]:
        return p64 + lr * wd * prev                       # p (1 - lr wd) - u  ->  p - u
    return p64 / (1 - lr * wd)                            # (p - u) (1 - lr wd)  ->  p - u


def test_adamw_decay_first_is_torch_adamw_in_float64():
    """the navigator's call (host/trainer.py): eps sqrt(bc2) and lr sqrt(bc2) / bc1 turn the kernel's form into torch.optim.AdamW's"""
    n = 257
    rn = gen(5)
    z = rn(n)
    (p, _), (m, _), (v, _) = guarded((torch.sign(z) * (0.5 + z.abs())).float()), guarded(torch.zeros(n)), guarded(torch.zeros(n))      # (weights away from zero, as above)
    tp = p.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([tp], lr=R.f32(HYP["lr"]), betas=(R.f32(HYP["b1"]), R.f32(HYP["b2"])), eps=HYP["eps"], weight_decay=R.f32(HYP["wd"]))
    p64, m64, v64 = p.double(), m.double(), v.double()
    for t in range(1, 4):
        g, _ = guarded(rn(n).float())
        bc1, bc2 = 1 - HYP["b1"] ** t, 1 - HYP["b2"] ** t
        eps_k, step_size = HYP["eps"] * math.sqrt(bc2), HYP["lr"] * math.sqrt(bc2) / bc1
        prev = tp.detach().clone()
        tp.grad = g.double()
        opt.step()
        p64, m64, v64, penv, _, _ = R.adamw_ref(p64, g, m64, v64, lr=HYP["lr"], b1=HYP["b1"], b2=HYP["b2"], eps=eps_k, wd=HYP["wd"], step_size=step_size, decay_first=True)
        O.adamw(n, p, g, m, v, None, HYP["lr"], HYP["b1"], HYP["b2"], eps_k, HYP["wd"], step_size, None, 0.0, 1.0, n_decay=-1, decay_first=True)
        torch.cuda.synchronize()
        ref = tp.detach()
        R.check("adamw", f"torch.optim.AdamW step {t}", p, ref, penv, ctrl=[torch.cat([ref[:-1], prev[-1:]]), ref + R.f32(HYP["lr"]) * R.f32(HYP["wd"]) * prev])


# ------------------------------------------------------------------------------------------ add_n
def add_n_case(n, count, dtype):
    rn = gen(n + count)
    y, guard = guarded(rn(n), dtype)
    xs = [rn(n).to(dtype).to(DEV) for _ in range(count)]
    y0 = y.double()
    terms = [x.double() for x in xs]
    ref, env = y0 + sum(terms), y0.abs() + sum(t.abs() for t in terms)
    O.add_n(y, xs)
    torch.cuda.synchronize()
    ve = 4 if dtype == F32 else 8
    body = n // ve * ve
    ctrl = [ref - terms[-1]]                                                                     # the last addend
    if body < n:
        ctrl.append(torch.cat([ref[:body], y0[body:]]))                                          # the scalar tail
    if body > 0:
        ctrl.append(torch.cat([ref[:body - ve], y0[body - ve:body], ref[body:]]))                # the last vector
    if body > CAP * ve:
        ctrl.append(torch.cat([ref[:CAP * ve], y0[CAP * ve:body], ref[body:]]))                  # the second grid-stride trip
    R.check("add_n", f"n={n} count={count} {dtype}", y, ref, env, dtype, ctrl=ctrl)
    assert untouched(guard)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("count", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 1003, CAP * 8 + 5])
def test_add_n_is_a_float64_sum_rounded_once(n, count, dtype):
    """fp32 storage is held to REL of the addends' envelope: a 9-term fp32 sum is not within one fp32 unit in the last place of the exact sum.
    CAP * 8 + 5 is past the 2048-block cap for fp32 (4 elements per lane) and exactly at it for 16-bit: the test below takes those past it"""
    add_n_case(n, count, dtype)


@pytest.mark.parametrize("dtype", HALF)
def test_add_n_16_bit_second_grid_stride_trip(dtype):
    add_n_case(CAP * 8 + 8 * 300 + 5, 3, dtype)


def test_add_n_refuses_what_it_cannot_serve():
    y = torch.zeros(64, device=DEV)
    x = torch.ones(64, device=DEV)
    with pytest.raises(L.MagicHipError):
        O.add_n(y, [])
    with pytest.raises(L.MagicHipError):
        O.add_n(y, [x] * 9)
    buf = torch.zeros(72, device=DEV)
    with pytest.raises(L.MagicHipError):
        O.add_n(buf[1:65], [x])                           # the sum's base off by one element
    with pytest.raises(L.MagicHipError):
        O.add_n(y, [torch.ones(72, device=DEV)[1:65]])    # an addend's
    torch.cuda.synchronize()
    assert (y == 0).all() and (buf == 0).all()


# ------------------------------------------------------------------------------------------ cast / add / dact
TAIL_N = [1, 3, 4, 5, 2048 * 1024 + 3]


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("n", TAIL_N)
def test_casts_are_torch_bit_for_bit(n, dtype):
    x = gen(n)(n) * 10.0 ** torch.randint(-4, 4, (n,), generator=torch.Generator().manual_seed(n)).double()
    special = torch.tensor([float("inf"), 70000.0, -1e-6, 0.0, -float("inf")], dtype=torch.float64)
    k = min(n, 5)
    x[n - k:] = special[:k]                                 # the specials sit in the scalar tail and the last vector
    x = x.float().to(DEV)
    y, guard = guarded(torch.zeros(n), dtype)
    O.cast_to(x, dtype, out=y)
    z, zguard = guarded(torch.zeros(n), F32)
    O.cast_to(y, F32, out=z)
    torch.cuda.synchronize()
    assert torch.equal(bits(y), bits(x.to(dtype))) and torch.equal(bits(z), bits(x.to(dtype).float()))
    assert untouched(guard) and untouched(zguard)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", TAIL_N)
def test_add_and_dact_match_float64(n, dtype):
    rn = gen(n + 1)
    y, guard = guarded(rn(n), dtype)
    x = rn(n).to(dtype).to(DEV)
    y0 = y.double()
    O.add_(y, x)
    torch.cuda.synchronize()
    ref = y0 + x.double()
    R.check("add", f"add n={n} {dtype}", y, ref, y0.abs() + x.double().abs(), dtype, ctrl=torch.cat([ref[:-1], y0[-1:]]))
    assert untouched(guard)
    z = rn(n)
    dy = rn(n)
    z[-1], dy[-1] = 1.0, 1.0                                # the last element is live under both activations
    z, dy = z.to(dtype).to(DEV), dy.to(dtype).to(DEV)
    for kind in (1, 2):
        out, oguard = guarded(torch.zeros(n), dtype)
        O.dact(dy, z, kind, out=out)
        torch.cuda.synchronize()
        ref, env = R.dact_ref(dy, z, kind)
        R.check("dact", f"dact kind={kind} n={n} {dtype}", out, ref, env, dtype, ctrl=torch.cat([ref[:-1], torch.zeros_like(ref[-1:])]))
        assert untouched(oguard)
