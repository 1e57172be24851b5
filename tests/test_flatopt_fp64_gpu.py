"""The flat optimizers of csrc/flatopt.hip (SGD, RMSprop, Adam, AdamW; clip, skip, schedule on the device) against the float64 restatements of
tests/_flatopt_ref64.py, at every launch branch (-m gpu).

Same rules as tests/test_optim_fp64_gpu.py: references in float64 from the operands the kernel reads, REL = 1e-5 of the terms' envelope (+ one unit in the
last place of a 16-bit shadow), a reference lacking one unit of work must fail the same comparison, sentinels past every buffer's extent.

Launch branches entered here:
  update        n = 1, 3 (scalar loop only), 255 / 257 (both sides of a block of the scalar loop), 1027 (vectors + an n & 3 tail), 2048 x 256 x 4 + 7 (the
                second trip of the grid-stride loop of the 16-byte path), a base 4 bytes off a 16-byte boundary (the scalar path) at n = 257; shadow none /
                bf16 / fp16; n_decay -1, 0, inside a vector, n; clip active / inactive / no norm word; gscale 0.125; zero_grad on the last step
  norm launch   with and without a norm word, both norm words in turn, constant and cosine schedules

Largest err / bound per rule on an MI355X (`pytest -s` prints every figure), over the first runs of this file, nothing tightened or loosened before or
after them: sgd 0.0318, rms 0.0296, adam 0.0918, adamW 0.0910, the norm launch 0.0201 (its atomics arrive in another order every run).
REL = 1e-5 stays: it is the rule of tests/test_optim_fp64_gpu.py, and every planted defect of tests/test_flatopt_ref64_cpu.py is more than one bound away under it.
"""
import math
from types import SimpleNamespace

import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from magic_amd.host import trainer as T
from magic_amd.host.params import ParamStore
from tests import _flatopt_ref64 as F
from tests import _loss_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
HALF = [torch.bfloat16, torch.float16]
SENT = 7.0
CAP4 = 2048 * 256 * 4                                      # elements of one grid-stride trip of the 16-byte path
RULE_MU = [("sgd", 0.0), ("sgd", 0.9), ("rms", 0.0), ("rms", 0.9), ("adam", 0.0), ("adamW", 0.0)]
TORCH = {"sgd": torch.optim.SGD, "rms": torch.optim.RMSprop, "adam": torch.optim.Adam, "adamW": torch.optim.AdamW}


def guarded(x, dtype=None, lead=0):
    """x in a buffer with 8 sentinel elements behind it (and `lead` in front: a base off the 16-byte boundary): (view of the n, the guards)"""
    x = x.to(dtype or x.dtype)
    n = x.numel()
    buf = torch.full((lead + n + 8,), SENT, dtype=x.dtype, device=DEV)
    buf[lead:lead + n] = x.to(DEV)
    return buf[lead:lead + n], torch.cat([buf[:lead], buf[lead + n:]])


def untouched(t):
    return bool((t == SENT).all())


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def ulp32(x):
    """one unit in the last place of the fp32 nearest x"""
    return math.ldexp(1.0, math.frexp(x)[1] - 24)


def words_for(rule, lr, t, slot, hyp):
    """the float block the norm launch leaves for state step t (host values, as fp32), a sentinel behind it"""
    _, lr_bc1, sq_bc2 = F.words_ref(0, t, rule, lr, hyp["a1"], hyp["b2"])
    return torch.tensor([lr, lr_bc1 or SENT, sq_bc2 or SENT, float(slot), SENT], dtype=F32, device=DEV)


def launch_update(rule, n, p, g, m, v, shadow, hyp, ss2, max_norm, gscale, words, nd, zero, overflow=None, step3=None):
    O.flat_update(O.FLAT_RULES[rule], n, p, g, m, v, shadow, hyp["a1"], hyp["b2"], hyp["eps"], hyp["wd"], hyp["mu"], ss2, max_norm, gscale, words,
                  n_decay=nd, zero_grad=zero, overflow=overflow, step3=step3)


# ------------------------------------------------------------------------------------------ three steps per rule
@pytest.mark.parametrize("shadow_dt", [None] + HALF)
@pytest.mark.parametrize("n,lead", [(1, 0), (3, 0), (255, 0), (257, 0), (1027, 0), (CAP4 + 7, 0), (257, 1)])
@pytest.mark.parametrize("rule,mu", RULE_MU)
def test_three_steps_match_the_float64_restatement(rule, mu, n, lead, shadow_dt):
    p0, m0, v0, grads = F.case_data(n, n)
    hyp = F.rule_hyp(rule, mu)
    keeps_m, keeps_v = rule in ("adam", "adamW") or mu > 0, rule != "sgd"
    for nd, clipping in ((-1, "active"), (0, "inactive"), (min(n, n // 2 | 1), "active"), (n, "none")):
        (p, pg), (m, mg), (v, vg) = guarded(p0, lead=lead), guarded(m0, lead=lead), guarded(v0, lead=lead)
        shadow, sg = guarded(torch.zeros(n), shadow_dt, lead=lead) if shadow_dt else (None, None)
        for t, g_cpu in enumerate(grads, 1):
            g, gg = guarded(g_cpu, lead=lead)
            # the reference starts from what this launch reads (tests/test_optim_fp64_gpu.py gives the reason)
            p_in, g_in, m_in, v_in = p.double(), g.clone(), m.double(), v.double()
            slot = t & 1
            ssv = float((g.double() ** 2).sum().float()) if clipping != "none" else None
            max_norm = {"active": 0.5 * math.sqrt(ssv) * 0.125, "inactive": 1e9}[clipping] if ssv is not None else 0.0
            ss2 = torch.full((3,), SENT, device=DEV)
            if ssv is not None:
                ss2[slot] = ssv
            step3 = torch.tensor([t, t, slot, 77], dtype=torch.int32, device=DEV)
            words = words_for(rule, hyp["lr"], t, slot, hyp)
            zero = t == 3
            launch_update(rule, n, p, g, m, v, shadow, hyp, ss2 if ssv is not None else None, max_norm, 0.125, words, nd, zero, step3=step3)
            torch.cuda.synchronize()
            clip = R.clip_ref(ssv, max_norm, 0.125)
            assert (clip < 0.1) == (clipping == "active"), "the clip is active exactly where the case means it to be"
            kw = dict(hyp, t=t, clip=clip)
            p64, m64, v64, penv, menv, venv = F.update_ref(rule, p_in, g_in, m_in, v_in, n_decay=nd, **kw)
            ctrl = [torch.cat([p64[:-1], p_in[-1:]])]                                              # the last element never updated
            if n > CAP4:
                ctrl.append(torch.cat([p64[:CAP4], p_in[CAP4:]]))                                  # the second grid-stride trip
            nd_eff = n if nd < 0 else nd
            if nd_eff > 0:                                                                         # the last decayed element without its decay
                ctrl.append(F.update_ref(rule, p_in, g_in, m_in, v_in, n_decay=nd_eff - 1, **kw)[0])
            name = f"{rule} mu={mu} n={n}+{lead} n_decay={nd} clip {clipping} step {t}"
            R.check(rule, f"p {name}", p, p64, penv, ctrl=ctrl)
            if keeps_m:
                R.check(rule, f"m {name}", m, m64, menv)
            else:
                assert torch.equal(m.double(), m_in), f"m is not this rule's to write: {name}"
            if keeps_v:
                R.check(rule, f"v {name}", v, v64, venv)
            else:
                assert torch.equal(v.double(), v_in), f"v is not this rule's to write: {name}"
            if shadow is not None:
                assert torch.equal(bits(shadow), bits(p.to(shadow_dt))), f"shadow {name}"
                assert untouched(sg)
            assert (g == 0).all() if zero else torch.equal(g, g_in), f"zero_grad {name}"
            assert untouched(pg) and untouched(mg) and untouched(vg) and untouched(gg), name
            if ssv is not None:                            # the other norm word zeroed for the next step, the switch thrown, the word in use left alone
                assert ss2.tolist() == [R.f32(ssv) if i == slot else 0.0 if i == 1 - slot else SENT for i in range(3)], name
                assert step3.tolist() == [t, t, 1 - slot, 77], name
            else:
                assert step3.tolist() == [t, t, slot, 77], name
            assert words[4].item() == SENT


@pytest.mark.parametrize("n,lead", [(1, 0), (257, 1), (1027, 0), (CAP4 + 7, 0)])
def test_norm_launch_adds_a_float64_sum_to_the_word_in_use(n, lead):
    """both norm words in turn; a base off the 16-byte boundary takes the scalar loop; CAP4 + 7 is past the 256-block cap and the four-in-flight loop's first trip"""
    g, guard = guarded(F.case_data(n, n + 1)[3][0], lead=lead)
    terms = g.double() ** 2
    for slot in (0, 1):
        ss2 = torch.tensor([SENT, SENT, SENT], device=DEV)
        ss2[slot] = 0.5
        step3 = torch.tensor([6, 4, slot, 77], dtype=torch.int32, device=DEV)
        words = torch.full((5,), SENT, device=DEV)
        O.flat_sumsq_sched(n, g, ss2, step3, words, O.FLAT_RULES["adam"], 1e-3, b1=0.9, b2=0.98)
        torch.cuda.synchronize()
        ref, env = 0.5 + terms.sum(), 0.5 + terms.sum()
        r = R.check("norm", f"n={n}+{lead} word {slot}", ss2[slot], ref, env, ctrl=[ref - terms[-1]] if n < 10 ** 4 else None)
        assert r <= 1.0 and ss2[1 - slot].item() == SENT and ss2[2].item() == SENT
        assert step3.tolist() == [7, 5, slot, 77], "the norm launch advances both counts and leaves the switch to the update launch"
        lr, lr_bc1, sq_bc2 = F.words_ref(6, 5, "adam", 1e-3, 0.9, 0.98)
        assert abs(words[0].item() - lr) <= ulp32(lr) and abs(words[1].item() - lr_bc1) <= ulp32(lr_bc1) and abs(words[2].item() - sq_bc2) <= ulp32(sq_bc2)
        assert words[3].item() == slot and words[4].item() == SENT
    assert untouched(guard)


def test_update_refuses_what_it_cannot_serve():
    n = 8
    p, g, m, v = (torch.ones(n + 1, device=DEV) for _ in range(4))
    words = torch.tensor([1e-2, 1e-2, 1.0, 0.0], device=DEV)
    ss2 = torch.zeros(2, device=DEV)
    step3 = torch.zeros(3, dtype=torch.int32, device=DEV)
    hyp = F.rule_hyp("adam")
    ok = dict(rule="adam", n=n, p=p, g=g, m=m, v=v, shadow=None, hyp=hyp, ss2=ss2, max_norm=1.0, gscale=1.0, words=words, nd=-1, zero=False, step3=step3)
    i16 = torch.zeros(n, dtype=torch.int16, device=DEV)
    bad = [dict(n=0), dict(m=None), dict(v=None), dict(ss2=None), dict(step3=None), dict(hyp=dict(hyp, mu=0.9)), dict(rule="rms", v=None),
           dict(rule="sgd", hyp=dict(hyp, mu=0.9), m=None)]
    for change in bad:
        with pytest.raises(L.MagicHipError):
            launch_update(**dict(ok, **change))
    with pytest.raises(L.MagicHipError):                   # a base that is not 4-byte aligned
        L.call("magic_flat_update", 2, n, p.data_ptr() + 2, L.P(g), L.P(m), L.P(v), None, 1, 0.9, 0.98, 1e-3, 0.0, 0.0, None, 0.0, 1.0, L.P(words), -1, 0,
               None, None, L.stream())
    with pytest.raises(L.MagicHipError):                   # a shadow that is not 16-bit
        L.call("magic_flat_update", 2, n, L.P(p), L.P(g), L.P(m), L.P(v), L.P(i16), 0, 0.9, 0.98, 1e-3, 0.0, 0.0, None, 0.0, 1.0, L.P(words), -1, 0,
               None, None, L.stream())
    with pytest.raises(L.MagicHipError):                   # an unknown rule
        L.call("magic_flat_update", 4, n, L.P(p), L.P(g), L.P(m), L.P(v), None, 1, 0.9, 0.98, 1e-3, 0.0, 0.0, None, 0.0, 1.0, L.P(words), -1, 0,
               None, None, L.stream())
    for kind, t_max, warmup in ((2, 4, 0), (1, 0, 0), (1, 4, -1)):      # an unknown schedule, a cosine of no length, a negative warm-up
        with pytest.raises(L.MagicHipError):
            O.flat_sumsq_sched(n, g, ss2, step3, words, 2, 1e-2, kind=kind, t_max=t_max, warmup=warmup)
    torch.cuda.synchronize()
    assert all((x == 1).all() for x in (p, g, m, v)) and (ss2 == 0).all() and (step3 == 0).all()
    assert [L._fn("magic_flat_rule_supported")(*a) for a in ((0, 1, 0, 0, 0), (1, 1, 0, 0, 0), (2, 0, 0, 0, 0), (3, 0, 0, 0, 0), (2, 1, 0, 0, 0),
                                                             (1, 0, 1, 0, 0), (0, 1, 0, 1, 0), (3, 0, 0, 0, 1), (4, 0, 0, 0, 0))] == [1, 1, 1, 1, 0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------ a store-like pair of flat buffers
def flat_store(n, seed, dtype=F32):
    """what trainer.FlatOptimizer reads of a ParamStore, over guarded buffers of n elements"""
    p0, _, _, _ = F.case_data(n, seed)
    s = SimpleNamespace(total=n, device=torch.device(DEV), compute_dtype=dtype, half=dtype in HALF, n_decay=n // 2, t_spans={}, f_spans={}, shadow_clean=False)
    (s.flat, pg), (s.grad, gg), (s.m, mg), (s.v, vg) = (guarded(x) for x in (p0, torch.zeros(n), torch.zeros(n), torch.zeros(n)))
    s.shadow, sg = guarded(p0, dtype) if s.half else (s.flat, pg)
    s.guards = (pg, gg, mg, vg, sg)
    s.zero_grad = s.grad.zero_
    return s


def make_opt(rule, mu, store, lr=5e-2, **kw):
    hyp = F.rule_hyp(rule, mu)
    args = dict(eps=hyp["eps"], weight_decay=hyp["wd"])
    if rule in ("sgd", "rms"):
        args["momentum"] = mu
    if rule == "sgd":
        del args["eps"]
        return T.FlatOptimizer(store, rule, lr, weight_decay=hyp["wd"], momentum=mu, **kw), hyp
    if rule == "rms":
        args["alpha"] = hyp["a1"]
    else:
        args["betas"] = (hyp["a1"], hyp["b2"])
    return T.FlatOptimizer(store, rule, lr, **args, **kw), hyp


# ------------------------------------------------------------------------------------------ a non-finite norm
@pytest.mark.parametrize("shadow_dt", [F32] + HALF)
@pytest.mark.parametrize("rule,mu", RULE_MU)
def test_a_non_finite_norm_skips_the_step_and_the_next_one_counts_it_the_same_way(rule, mu, shadow_dt):
    n, lr0, sched = 1027, 5e-2, (4, 5e-3, 1)
    s = flat_store(n, 11, shadow_dt)
    opt, hyp = make_opt(rule, mu, s, lr=lr0, schedule=("cosine",) + sched, decay_all=False)
    _, _, _, grads = F.case_data(n, 12)
    p64, m64, v64 = s.flat.double(), s.m.double(), s.v.double()
    k = t = 0
    for i, g_cpu in enumerate([grads[0], grads[1], grads[2]]):
        g = g_cpu.to(DEV)
        if i == 1:
            g[n // 3] = float("inf")
        s.grad.copy_(g)
        before = [bits(x).clone() for x in (s.flat, s.m, s.v, s.shadow)]
        opt.step(max_norm=40.0)
        torch.cuda.synchronize()
        k += 1
        assert (s.grad == 0).all(), "the gradient is consumed, skipped or not"
        if i == 1:
            assert all(torch.equal(bits(x), b) for x, b in zip((s.flat, s.m, s.v, s.shadow), before)), "a skipped step touches nothing"
            assert opt.skipped_steps() == 1 and opt.step_dev[:2].tolist() == [k, t]
            continue
        t += 1
        assert opt.step_dev[:2].tolist() == [k, t] and opt.skipped_steps() == (1 if i == 2 else 0)
        ssv = float((g.double() ** 2).sum())
        lr = F.lr_ref(k - 1, lr0, sched)
        assert abs(opt.param_groups[0]["lr"] - lr) <= ulp32(lr)
        p64, m64, v64, penv, menv, venv = F.update_ref(rule, p64, g, m64, v64, n_decay=s.n_decay, **dict(hyp, lr=lr, t=t, clip=R.clip_ref(ssv, 40.0, 1.0)))
        R.check(rule, f"p skip {rule} mu={mu} step {i}", s.flat, p64, penv)
        if rule != "sgd":
            R.check(rule, f"v skip {rule} mu={mu} step {i}", s.v, v64, venv)
        if s.half:
            assert torch.equal(bits(s.shadow), bits(s.flat.to(shadow_dt)))
        p64, m64, v64 = s.flat.double(), s.m.double(), s.v.double()
    assert all(untouched(x) for x in s.guards)


# ------------------------------------------------------------------------------------------ the schedule words
@pytest.mark.parametrize("rule", ["rms", "adam"])
def test_schedule_words_over_eight_launches(rule):
    """W = 3, T = 4, eta_min = 0.1 lr0: lr within one fp32 unit of the float64 value at every k (k = W - 1, W, W + T among them); lr / bc1 and sqrt(bc2) follow
    the state step across a skipped step; set_lr_step takes effect on the next launch"""
    lr0, w, t_max = 1e-3, 3, 4
    sched = (t_max, 0.1 * lr0, w)
    s = flat_store(5, 3)
    opt, hyp = make_opt(rule, 0.0, s, lr=lr0, schedule={"t_max": t_max, "eta_min": 0.1 * lr0, "warmup": w})
    assert abs(opt.param_groups[0]["lr"] - F.lr_ref(0, lr0, sched)) <= ulp32(lr0)
    t = 0
    seq = list(range(8)) + [1, 2]                          # ... then the host sets the lr step back to 1
    for i, k in enumerate(seq):
        if i == 8:
            opt.set_lr_step(1)
        s.grad.fill_(0.25)
        opt.step(max_norm=40.0 if i % 2 else None)         # with and without a norm word: the one-block launch advances the schedule alike
        torch.cuda.synchronize()
        t += 1
        lr, lr_bc1, sq_bc2 = F.words_ref(k, t, rule, lr0, hyp["a1"], hyp["b2"], sched)
        got = opt.words.tolist()
        assert abs(got[0] - lr) <= ulp32(lr), (k, got[0], lr)
        assert opt.param_groups[0]["lr"] == got[0]
        if rule == "adam":
            assert abs(got[1] - lr_bc1) <= ulp32(lr_bc1) and abs(got[2] - sq_bc2) <= ulp32(sq_bc2), (k, t, got)
        else:
            assert got[1:3] == [0.0, 0.0], "not this rule's words"
        assert opt.step_dev[:2].tolist() == [k + 1, t]
    # a skipped step: the lr step advances, the state step and with it the bias-correction words of the NEXT step do not
    s.grad.fill_(float("nan"))
    opt.step(max_norm=40.0)
    s.grad.fill_(0.25)
    opt.step(max_norm=40.0)
    torch.cuda.synchronize()
    assert opt.step_dev[:2].tolist() == [5, t + 1] and opt.skipped_steps() == 1
    lr, lr_bc1, sq_bc2 = F.words_ref(4, t + 1, rule, lr0, hyp["a1"], hyp["b2"], sched)
    got = opt.words.tolist()
    assert abs(got[0] - lr) <= ulp32(lr)
    if rule == "adam":
        assert abs(got[1] - lr_bc1) <= ulp32(lr_bc1) and abs(got[2] - sq_bc2) <= ulp32(sq_bc2)
    assert all(untouched(x) for x in s.guards)


# ------------------------------------------------------------------------------------------ capture
@pytest.mark.parametrize("rule,mu", RULE_MU)
def test_a_captured_step_replays_as_three_eager_steps_bitwise(rule, mu):
    n, lr0, sched = 1027, 5e-2, (3, 5e-3, 1)
    eager, graphed = flat_store(n, 21, torch.bfloat16), flat_store(n, 21, torch.bfloat16)
    oe, _ = make_opt(rule, mu, eager, lr=lr0, schedule=("cosine",) + sched)
    og, _ = make_opt(rule, mu, graphed, lr=lr0, schedule=("cosine",) + sched)
    _, _, _, grads = F.case_data(n, 22)
    grads = [g.to(DEV) * (40.0 if i == 1 else 1.0) for i, g in enumerate(grads)]          # the second step is clipped
    for g in grads:
        eager.grad.copy_(g)
        oe.step(max_norm=40.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with L.capture(graph):
        og.step(max_norm=40.0)
    assert og.step_dev.tolist() == [0, 0, 0], "a capture launches nothing"
    for i, g in enumerate(grads):
        graphed.grad.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        lr = F.lr_ref(i, lr0, sched)
        assert abs(og.param_groups[0]["lr"] - lr) <= ulp32(lr), "the device lr follows the cosine across the replays"
    for name in ("flat", "m", "v", "shadow", "grad"):
        assert torch.equal(bits(getattr(graphed, name)), bits(getattr(eager, name))), name
    assert torch.equal(og.step_dev, oe.step_dev) and torch.equal(og.words, oe.words) and og.step_dev[:2].tolist() == [3, 3]
    assert all(untouched(x) for x in eager.guards + graphed.guards)


# ------------------------------------------------------------------------------------------ state_dict, both ways
SPECS = [("a.weight", (64, 64), "normal"), ("a.bias", (37,), "zeros"), ("n.LayerNorm.weight", (64,), "ones"), ("b.weight", (5, 3), "normal")]


def small_target(kind, seed):
    """(what the optimizer is given, its store, the parameter names in the order torch numbers them): the smallest navigator model the GPU tests build
    (H = 128, fp32; numbered in model.parameters() order, which is not the store's) or a four-tensor ParamStore"""
    if kind == "model":
        from magic_amd.host.config import make_config
        from magic_amd.host.model_nav import VLNBert
        cfg = make_config(128, role="teacher", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
        model = VLNBert(None, role="student", config=cfg, device=torch.device(DEV), compute_dtype=F32, seed=seed)
        model.store.checkpoint_like_(4)
        by_id = {id(p): n for n, p in model.store._params}
        return model, model.store, [by_id[id(p)] for p in model.parameters()]
    st = ParamStore(SPECS, DEV, F32, seed=seed).checkpoint_like_(4)
    return st, st, [n for n, _, _ in SPECS]


def set_grads(st, names, params, seed):
    gen = torch.Generator(DEV).manual_seed(seed)
    st.grad.zero_()
    for n, p in zip(names, params):
        g = torch.randn(st.offsets[n][2], device=DEV, generator=gen)
        st.g(n).copy_(g)
        if p is not None:
            p.grad = g.clone()
    return st.grad.clone()


def check_params(rule, what, st, names, params, p64, penv):
    for n, p in zip(names, params):
        off, cnt, shape = st.offsets[n]
        R.check(rule, f"{what} {n}", p.detach(), p64[off:off + cnt].view(shape), penv[off:off + cnt].view(shape))


@pytest.mark.parametrize("kind", ["store", "model"])
@pytest.mark.parametrize("rule,mu", RULE_MU)
def test_state_dict_round_trip_with_torch_optim_both_ways(rule, mu, kind):
    hyp = F.rule_hyp(rule, mu)
    target, st, names = small_target(kind, 3)
    fopt, _ = make_opt(rule, mu, target, lr=1e-2)
    # flat -> torch: two flat steps, export, the third step in both
    for i in range(2):
        set_grads(st, names, [None] * len(names), i)
        fopt.step(max_norm=40.0)
    params = [torch.nn.Parameter(st.master(n).clone()) for n in names]
    topt = TORCH[rule](params, **fopt._hyper())
    topt.load_state_dict(fopt.state_dict())
    p_in, m_in, v_in = st.flat.double(), st.m.double(), st.v.double()
    g_in = set_grads(st, names, params, 2)
    torch.nn.utils.clip_grad_norm_(params, 40.0)
    topt.step()
    fopt.step(max_norm=40.0)
    torch.cuda.synchronize()
    kw = dict(hyp, lr=1e-2, t=3, clip=R.clip_ref(float((g_in.double() ** 2).sum()), 40.0, 1.0))
    p64, _, _, penv, _, _ = F.update_ref(rule, p_in, g_in, m_in, v_in, **kw)
    R.check(rule, f"flat step 3 {rule} mu={mu} {kind}", st.flat, p64, penv)
    check_params(rule, f"torch after the flat state, {rule} mu={mu}", st, names, params, p64, penv)
    # torch -> flat: torch's state after its third step into a fresh flat optimizer over torch's weights, the fourth step in both
    target2, st2, names2 = small_target(kind, 9)
    assert names2 == names
    for n, p in zip(names, params):
        st2.master(n).copy_(p.detach())
    fopt2, _ = make_opt(rule, mu, target2, lr=1.0)
    fopt2.load_state_dict(topt.state_dict())
    assert fopt2.lr == 1e-2
    p_in, m_in, v_in = st2.flat.double(), st2.m.double(), st2.v.double()
    g_in = set_grads(st2, names, params, 3)
    torch.nn.utils.clip_grad_norm_(params, 40.0)
    topt.step()
    fopt2.step(max_norm=40.0)
    torch.cuda.synchronize()
    kw = dict(hyp, lr=1e-2, t=4, clip=R.clip_ref(float((g_in.double() ** 2).sum()), 40.0, 1.0))
    p64, _, _, penv, _, _ = F.update_ref(rule, p_in, g_in, m_in, v_in, **kw)
    R.check(rule, f"flat step 4 after torch's state, {rule} mu={mu} {kind}", st2.flat, p64, penv)
    check_params(rule, f"torch step 4 {rule} mu={mu}", st2, names, params, p64, penv)
    # another rule's state, another shape
    other = "adam" if rule != "adam" else "rms"
    with pytest.raises(ValueError):
        T.flat_optimizer(other, target2, 1e-2).load_state_dict(fopt2.state_dict())
    if rule != "sgd" or mu:
        sd = topt.state_dict()
        key = next(iter(sd["state"][0].keys() - {"step"}))
        sd["state"][0] = dict(sd["state"][0], **{key: torch.zeros(3, 3, device=DEV)})
        with pytest.raises(ValueError):
            fopt2.load_state_dict(sd)


# ------------------------------------------------------------------------------------------ isolation
@pytest.mark.parametrize("dtype", HALF)
def test_the_shadows_after_a_step_are_a_fresh_sync_of_the_master_weights(dtype):
    st = ParamStore(SPECS, DEV, dtype, seed=3).checkpoint_like_(4)
    st.sync_shadow(force=True)
    wt, wf, wtf = st.t_span("a.weight", 64, 64), st.f_span("a.weight", 64, 64), st.tf_span("a.weight", 64, 64)
    opt = T.flat_optimizer("rms", st, 1e-2, momentum=0.9)
    set_grads(st, [n for n, _, _ in SPECS], [None] * 4, 0)
    opt.step(max_norm=40.0)
    torch.cuda.synchronize()
    assert st.shadow_clean
    got = [bits(x).clone() for x in (st.shadow, wt, wf, wtf)]
    assert not torch.equal(st.w("a.weight").float(), torch.zeros(64, 64, device=DEV))
    st.shadow.zero_(), st.shadow_t.zero_(), st.shadow_f.zero_(), st.shadow_tf.zero_()
    st.sync_shadow(force=True)
    torch.cuda.synchronize()
    for name, a, b in zip(("shadow", "transposed", "fragment order", "transposed fragment order"), got, (st.shadow, wt, wf, wtf)):
        assert torch.equal(a, bits(b)), name
    assert torch.equal(wt.float(), st.w("a.weight").float().t())


def test_magic_adamw_is_bitwise_what_it_was_around_the_new_launches():
    n = 1027
    p0, m0, v0, grads = F.case_data(n, 31)

    def adamw():
        p, g, m, v = (x.clone().to(DEV) for x in (p0, grads[0], m0, v0))
        sh = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
        ss = (g.double() ** 2).sum().float().reshape(1)
        O.adamw(n, p, g, m, v, sh, 1e-2, 0.9, 0.98, 1e-6, 0.1, 2e-2, ss, 1.0, 0.125, n_decay=n // 2, zero_grad=True, decay_first=True)
        torch.cuda.synchronize()
        return [bits(x).clone() for x in (p, g, m, v, sh)]
    before = adamw()
    s = flat_store(n, 32, torch.bfloat16)
    opt, _ = make_opt("adamW", 0.0, s)
    s.grad.copy_(grads[1])
    opt.step(max_norm=40.0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, adamw()))
