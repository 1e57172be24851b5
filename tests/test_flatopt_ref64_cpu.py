"""The float64 restatements of tests/_flatopt_ref64.py against torch.optim on float64 CPU tensors, the planted defects against the bound the GPU test
uses, and what trainer.FlatOptimizer does without a device: names, defaults, refusals, torch's state_dict layout.  No GPU."""
import math

import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import trainer as T
from magic_amd.host.params import ParamStore
from tests import _flatopt_ref64 as F
from tests import _loss_ref64 as R

TORCH = {"sgd": torch.optim.SGD, "rms": torch.optim.RMSprop, "adam": torch.optim.Adam, "adamW": torch.optim.AdamW}
RULE_MU = [("sgd", 0.0), ("sgd", 0.9), ("rms", 0.0), ("rms", 0.9), ("adam", 0.0), ("adamW", 0.0)]


def torch_kwargs(rule, lr, a1, b2, eps, wd, mu):
    lr, a1, b2, eps, wd, mu = (R.f32(x) for x in (lr, a1, b2, eps, wd, mu))         # the values the restatement works with
    if rule == "sgd":
        return dict(lr=lr, momentum=mu, weight_decay=wd)
    if rule == "rms":
        return dict(lr=lr, alpha=a1, eps=eps, weight_decay=wd, momentum=mu)
    return dict(lr=lr, betas=(a1, b2), eps=eps, weight_decay=wd)


@pytest.mark.parametrize("clip_on", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("rule,mu", RULE_MU)
def test_restatements_are_torch_optim_in_float64(rule, mu, wd, clip_on):
    n = 33
    gen = torch.Generator().manual_seed(7)
    rn = lambda: torch.randn(n, generator=gen, dtype=torch.float64)       # noqa: E731
    hyp = dict(lr=1e-2, a1=0.95 if rule == "rms" else 0.9, b2=0.98, eps=1e-8, wd=wd, mu=mu)
    tp = torch.nn.Parameter(rn())
    opt = TORCH[rule]([tp], **torch_kwargs(rule, **hyp))
    p, m, v = tp.detach().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, 6):
        g = rn() * (30.0 if clip_on else 0.5)
        tp.grad = g.clone()
        norm = torch.nn.utils.clip_grad_norm_([tp], 40.0)
        assert (float(norm) > 40.0) == clip_on
        opt.step()
        clip = R.clip_ref(float((g * g).sum()), 40.0, 1.0)
        assert (clip < 1.0) == clip_on
        p, m, v, penv, menv, venv = F.update_ref(rule, p, g, m, v, t=t, clip=clip, **hyp)
        st = opt.state[tp]
        assert ((p - tp.detach()).abs() <= 1e-12 * penv).all(), (rule, t)
        km, kv = {"sgd": ("momentum_buffer", None), "rms": ("momentum_buffer", "square_avg")}.get(rule, ("exp_avg", "exp_avg_sq"))
        if kv:
            assert ((v - st[kv]).abs() <= 1e-12 * venv).all(), (rule, t)
        if rule in ("adam", "adamW") or mu:
            assert ((m - st[km]).abs() <= 1e-12 * menv).all(), (rule, t)


def test_n_decay_and_skip_of_the_restatement():
    """[0, n_decay) decays, the rest does not; a norm that is not finite leaves everything as it was"""
    p, m, v, (g, _, _) = F.case_data(9, 1)
    for rule in F.RULES:
        full = F.update_ref(rule, p, g, m, v, t=1, n_decay=-1, **F.rule_hyp(rule))[0]
        none = F.update_ref(rule, p, g, m, v, t=1, n_decay=0, **F.rule_hyp(rule))[0]
        part = F.update_ref(rule, p, g, m, v, t=1, n_decay=5, **F.rule_hyp(rule))[0]
        assert torch.equal(part[:5], full[:5]) and torch.equal(part[5:], none[5:]) and not torch.equal(full, none)
        out = F.update_ref(rule, p, g, m, v, t=1, sumsq=float("inf"), **F.rule_hyp(rule))
        assert torch.equal(out[0], p.double()) and torch.equal(out[1], m.double()) and torch.equal(out[2], v.double())


def test_cosine_closed_form_is_cosine_annealing_lr_stepped_chainably():
    lr0, t_max = R.f32(1e-3), 7
    eta = R.f32(0.1 * lr0)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr0)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=t_max, eta_min=eta)
    for k in range(t_max + 1):
        want = opt.param_groups[0]["lr"]
        got = F.lr_ref(k, lr0, (t_max, eta, 0))
        assert abs(got - want) <= 1e-12 * want, (k, got, want)
        assert abs(T.flat_lr(k, lr0, {"t_max": t_max, "eta_min": eta, "warmup": 0}) - want) <= 1e-12 * want
        opt.step()
        sch.step()
    assert F.lr_ref(0, lr0, (t_max, eta, 0)) == lr0 and abs(F.lr_ref(t_max, lr0, (t_max, eta, 0)) - eta) <= 1e-12 * eta


def test_warm_up_rows_and_the_hand_over():
    lr0, w, t_max = R.f32(1e-3), 3, 4
    eta = R.f32(0.1 * lr0)
    for k in range(w):
        assert F.lr_ref(k, lr0, (t_max, eta, w)) == lr0 * (k + 1) / w
    assert F.lr_ref(w - 1, lr0, (t_max, eta, w)) == lr0                        # the last warm-up row is the full lr
    assert F.lr_ref(w, lr0, (t_max, eta, w)) == lr0                            # the cosine starts there, at its own step 0
    assert F.lr_ref(w + 1, lr0, (t_max, eta, w)) == F.lr_ref(1, lr0, (t_max, eta, 0)) < lr0
    assert abs(F.lr_ref(w + t_max, lr0, (t_max, eta, w)) - eta) <= 1e-12 * eta
    for k in range(w + t_max + 1):
        assert T.flat_lr(k, lr0, {"t_max": t_max, "eta_min": eta, "warmup": w}) == pytest.approx(F.lr_ref(k, lr0, (t_max, eta, w)), rel=1e-15)
    lr, lr_bc1, sq_bc2 = F.words_ref(2, 2, "adam", lr0, 0.9, 0.98, (t_max, eta, w))
    assert lr_bc1 == lr / (1 - R.f32(0.9) ** 2) and sq_bc2 == math.sqrt(1 - R.f32(0.98) ** 2)
    assert F.words_ref(2, 2, "rms", lr0, 0.9, 0.98)[1:] == (None, None)


@pytest.mark.parametrize("defect,rule", [(d, r) for d, rules in F.DEFECTS.items() for r in rules])
def test_a_planted_defect_breaks_the_bound_the_gpu_test_uses(defect, rule):
    """on the GPU test's data and hyper-parameters, from the state each of its three steps starts from"""
    n = 257
    p, m, v, grads = F.case_data(n, n)
    mu = 0.9 if rule in ("sgd", "rms") else 0.0
    p64, m64, v64 = p.double(), m.double(), v.double()
    for t, g in enumerate(grads, 1):
        ss = float((g.double() ** 2).sum())
        max_norm = 0.5 * math.sqrt(ss) * 0.125
        kw = dict(F.rule_hyp(rule, mu), t=t, clip=R.clip_ref(ss, max_norm, 0.125), n_decay=n // 2 | 1)
        good = F.update_ref(rule, p64, g, m64, v64, **kw)
        bad = F.update_ref(rule, p64, g, m64, v64, defect=defect, **kw)
        assert R.ratio(bad[0], good[0], R.bound(good[0], good[3])) > 1.0, (defect, rule, t)
        p64, m64, v64 = good[0].float().double(), good[1].float().double(), good[2].float().double()


# ------------------------------------------------------------------------------------------ trainer.FlatOptimizer without a device
SPECS = [("a.weight", (7, 5), "normal"), ("a.bias", (7,), "zeros"), ("n.LayerNorm.weight", (5,), "ones"), ("b.weight", (5, 3), "normal")]


def cpu_store():
    return ParamStore(SPECS, "cpu", torch.float32, seed=3)


def test_flat_optimizer_takes_the_reference_names_with_torch_defaults():
    st = cpu_store()
    for name, cls in TORCH.items():
        opt = T.flat_optimizer(name, st, 1e-3)
        assert isinstance(opt, T.FlatOptimizer) and opt.rule == name
        want = cls([torch.nn.Parameter(torch.zeros(1))], lr=1e-3).param_groups[0]
        for key, val in opt._hyper().items():
            assert want[key] == val, (name, key)
        assert opt.param_groups[0]["lr"] == R.f32(1e-3) and opt.skipped_steps() == 0
        assert set(opt.state_dict()["param_groups"][0]) == set(want)
    assert T.flat_optimizer("adamW", st, 1e-3).wd == 0.01 and T.flat_optimizer("adam", st, 1e-3).wd == 0
    assert isinstance(T.FlatTorchAdamW(st), T.FlatTorchAdamW)                  # the earlier class stays what it was


@pytest.mark.parametrize("name,kw", [("rms", dict(centered=True)), ("sgd", dict(momentum=0.9, nesterov=True)), ("sgd", dict(momentum=0.9, dampening=0.1)),
                                     ("adam", dict(amsgrad=True)), ("adamW", dict(amsgrad=True)), ("adam", dict(maximize=True)), ("adam", dict(momentum=0.9)),
                                     ("adamax", {}), ("rangerlars", {}), ("AdamW", {}), ("adam", dict(schedule=("cosine", 0))),
                                     ("adam", dict(schedule=("linear", 5)))])
def test_flat_optimizer_refuses_what_the_update_does_not_carry(name, kw):
    with pytest.raises(ValueError):
        T.flat_optimizer(name, cpu_store(), 1e-3, **kw)
    with pytest.raises(ValueError):
        T.FlatOptimizer(cpu_store(), "lamb", 1e-3)


def test_schedule_argument_forms():
    st = cpu_store()
    a = T.flat_optimizer("adam", st, 1e-3, schedule=("cosine", 100))
    assert a.schedule == {"t_max": 100, "eta_min": pytest.approx(1e-4), "warmup": 0}              # the reference's eta_min = 0.1 lr
    b = T.flat_optimizer("adam", st, 1e-3, schedule={"t_max": 90, "eta_min": 2e-4, "warmup": 10})
    assert b.schedule == {"t_max": 90, "eta_min": 2e-4, "warmup": 10}
    assert b.param_groups[0]["lr"] == R.f32(1e-3 / 10)                         # before any step: the first step's lr


@pytest.mark.parametrize("rule,mu", RULE_MU)
def test_state_dict_is_torch_optims_layout_both_ways(rule, mu):
    """the exported state loads into torch.optim.X over the same parameter list and has the keys a stepped torch optimizer writes; torch's state loads back"""
    st = cpu_store()
    kw = dict(momentum=mu) if mu else {}
    opt = T.flat_optimizer(rule, st, 1e-2, schedule=("cosine", 50), **kw)
    assert opt.state_dict()["state"] == {}                                     # torch has no state before the first step
    gen = torch.Generator().manual_seed(2)
    st.m.copy_(torch.randn(st.total, generator=gen))
    st.v.copy_(torch.rand(st.total, generator=gen))
    opt.step_dev[:2].copy_(torch.tensor([5, 4], dtype=torch.int32))           # five steps, one of them skipped
    sd = opt.state_dict()
    params = [torch.nn.Parameter(st.master(n).clone()) for n, _, _ in SPECS]
    topt = TORCH[rule](params, lr=1.0)
    topt.load_state_dict(sd)
    twin = TORCH[rule]([torch.nn.Parameter(p.detach().clone()) for p in params], **opt._hyper())
    for p in twin.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    twin.step()
    want = twin.state_dict()
    assert topt.state_dict()["param_groups"] == want["param_groups"]
    assert {i: set(e) for i, e in topt.state_dict()["state"].items()} == {i: set(e) for i, e in want["state"].items()}
    km, kv = opt._state_keys()
    for i, (n, _, _) in enumerate(SPECS):
        e = topt.state[params[i]] if (km or kv) else {}
        if km:
            assert torch.equal(e[km], st._view(st.m, n))
        if kv:
            assert torch.equal(e[kv], st._view(st.v, n))
        if "step" in e:
            assert float(e["step"]) == 4.0
    back = T.flat_optimizer(rule, cpu_store(), 1.0, **kw)
    back.load_state_dict(topt.state_dict())                                   # torch's own export: no rule / lr_step / schedule keys
    assert back.lr == 1e-2 and back.step_dev[:2].tolist() == ([4, 4] if rule != "sgd" else [1, 1] if mu else [0, 0])
    if km:
        assert torch.equal(back.store.m, st.m * (back.store.m != 0)) and back.store.m.abs().sum() > 0
    if kv:
        assert torch.equal(back.store.v, st.v * (back.store.v != 0)) and back.store.v.abs().sum() > 0
    own = T.flat_optimizer(rule, cpu_store(), 1.0, **kw)
    own.load_state_dict(sd)
    # (torch's SGD state has no step and the rule reads none: the word comes back as "stepped" / "not stepped")
    assert own.step_dev[:2].tolist() == ([5, 4] if rule != "sgd" else [5, 1] if mu else [5, 0]) and own.schedule == opt.schedule


def test_load_state_dict_rejects_another_rule_count_or_shape():
    sd = {r: T.flat_optimizer(r, cpu_store(), 1e-2).state_dict() for r in F.RULES}
    for r in F.RULES:
        for other in F.RULES:
            if other != r:
                with pytest.raises(ValueError, match="state is"):
                    T.flat_optimizer(r, cpu_store(), 1e-2).load_state_dict(sd[other])
    params = [torch.nn.Parameter(torch.zeros(s)) for _, s, _ in SPECS]
    with pytest.raises(ValueError, match="state is"):                          # torch's own export names no rule: told apart by its group's keys
        T.flat_optimizer("adam", cpu_store(), 1e-2).load_state_dict(torch.optim.AdamW(params).state_dict())
    with pytest.raises(ValueError, match="one group of 4"):
        T.flat_optimizer("adam", cpu_store(), 1e-2).load_state_dict(torch.optim.Adam(params[:3]).state_dict())
    wrong = [torch.nn.Parameter(torch.zeros(s)) for s in ((7, 5), (7,), (5,), (3, 5))]
    topt = torch.optim.Adam(wrong)
    for p in wrong:
        p.grad = torch.ones_like(p)
    topt.step()
    with pytest.raises(ValueError, match="exp_avg of parameter 3"):
        T.flat_optimizer("adam", cpu_store(), 1e-2).load_state_dict(topt.state_dict())


def test_a_model_numbers_the_state_in_model_parameters_order():
    """torch numbers an optimizer's state by position in the list it was given, model.parameters(): not the store's spec order"""
    from magic_amd.host.config import make_config
    from magic_amd.host.model_nav import VLNBert
    cfg = make_config(128, role="teacher", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    model = VLNBert(None, role="student", config=cfg, device=torch.device("cpu"), compute_dtype=torch.float32, seed=0)
    st = model.store
    opt = T.flat_optimizer("adam", model, 1e-3)
    names = opt._names()
    assert sorted(names) == sorted(n for n, _, _ in st.specs) and names != [n for n, _, _ in st.specs]
    params = list(model.parameters())
    topt = torch.optim.Adam(params, lr=1e-3)
    for i, p in enumerate(params):
        p.grad = torch.full_like(p, float(i + 1))
    topt.step()
    opt.load_state_dict(topt.state_dict())
    by_id = {id(p): n for n, p in st._params}
    for i, p in enumerate(params):
        assert torch.equal(st._view(st.m, by_id[id(p)]), topt.state[p]["exp_avg"]) and float(topt.state[p]["exp_avg"].flatten()[0]) == pytest.approx(0.1 * (i + 1))
    back = opt.state_dict()
    assert all(torch.equal(back["state"][i]["exp_avg_sq"], topt.state[p]["exp_avg_sq"]) for i, p in enumerate(params))
