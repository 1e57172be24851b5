"""Float64 restatements of the flat optimizers (csrc/flatopt.hip: SGD, RMSprop, Adam, AdamW with clip, skip, n_decay and momentum) and of their
device-side schedule, with the per-element bound envelopes of every output.

The rules of tests/_loss_ref64.py hold here too (and its f32 / bound / ratio / check / clip_ref are used): a reference takes the operands the kernel
reads -- fp32 p, g, m, v as passed, scalars rounded to the fp32 the C ABI carries -- and works in float64 from there; the bound of a comparison is
REL = 1e-5 times the envelope of the terms (|p| + |lr wd p| + |update| for p, likewise for each state buffer), plus one unit in the last place of the
16-bit type for the shadow.  tests/test_flatopt_ref64_cpu.py holds every restatement against torch.optim on float64 tensors; `defect=` plants one
wrong step each, which must break the same bound on the data the GPU test uses (case_data)."""
import math

import torch

from tests._loss_ref64 import f32

RULES = ("sgd", "rms", "adam", "adamW")
DEFECTS = {"eps_in_sqrt": ("rms", "adam", "adamW"), "decay_after": ("adamW",), "no_bias_correction": ("adam", "adamW"),
           "clip_twice": RULES, "decay_everywhere": ("sgd", "rms", "adam"), "rms_lr_in_buf": ("rms",)}
# the hyper-parameters of the kernel tests: large enough that every term of a rule is worth many bounds (eps 1e-3 next to sqrt(v) ~ 0.1; lr^2 wd,
# the difference between AdamW's two decay orders, 2.5e-4 of an update ratio of order one against a bound of ~1e-5)
HYP = dict(lr=5e-2, a1=0.9, b2=0.98, eps=1e-3, wd=0.1)
RMS_ALPHA = 0.95


def lr_ref(k, lr0, sched=None):
    """lr of lr step k.  sched: None (constant) or (t_max, eta_min, warmup): k < warmup: lr0 (k + 1) / warmup (the reference's WarmUpLR.get_lr);
    otherwise CosineAnnealingLR's closed form eta_min + (lr0 - eta_min)(1 + cos(pi (k - warmup) / t_max)) / 2"""
    lr0 = f32(lr0)
    if sched is None:
        return lr0
    t_max, eta_min, warmup = sched
    eta_min = f32(eta_min)
    if k < warmup:
        return lr0 * (k + 1) / warmup
    return eta_min + (lr0 - eta_min) * (1.0 + math.cos(math.pi * (k - warmup) / t_max)) / 2.0


def words_ref(k, t, rule, lr0, b1, b2, sched=None):
    """(lr_k, lr_k / bc1, sqrt(bc2)) of lr step k and state step t (after its advance); the last two None for sgd / rms"""
    lr = lr_ref(k, lr0, sched)
    if rule not in ("adam", "adamW"):
        return lr, None, None
    return lr, lr / (1.0 - f32(b1) ** t), math.sqrt(1.0 - f32(b2) ** t)


def update_ref(rule, p, g, m, v, *, lr, t=1, a1=0.9, b2=0.999, eps=1e-8, wd=0.0, mu=0.0, clip=1.0, n_decay=-1, sumsq=None, defect=None):
    """one step of `rule` in float64: torch.optim's arithmetic (a1 = RMSprop's alpha | Adam's beta1; m = momentum buffer | exp_avg; v = square_avg |
    exp_avg_sq; t = the state step after its advance; clip = the factor every gradient element is multiplied by).  sumsq not finite: the step is
    skipped, everything comes back unchanged.  Returns p, m, v and the bound envelope of each."""
    lr, a1, b2, eps, wd, mu = (f32(x) for x in (lr, a1, b2, eps, wd, mu))
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    if sumsq is not None and not math.isfinite(float(sumsq)):
        return p, m, v, p.abs(), m.abs(), v.abs()
    n = p.numel()
    nd = n if n_decay < 0 else n_decay
    dec = (torch.arange(n, device=p.device) < nd) & (wd > 0)
    if defect == "decay_everywhere":
        dec = torch.full_like(dec, wd > 0)
    gc = g * clip * (clip if defect == "clip_twice" else 1.0)
    coupled = rule != "adamW"
    gp = gc + (torch.where(dec, wd * p, torch.zeros_like(p)) if coupled else 0.0)
    genv = gc.abs() + (torch.where(dec, (wd * p).abs(), torch.zeros_like(p)) if coupled else 0.0)        # the terms of g'
    decay_env = torch.where(dec, (lr * wd * p).abs(), torch.zeros_like(p))
    if rule == "sgd":
        if mu > 0:
            menv = (mu * m).abs() + genv
            m = mu * m + gp
            upd, uenv = lr * m, lr * menv
        else:
            menv = m.abs()
            upd, uenv = lr * gp, lr * genv
        pn, venv = p - upd, v.abs()
    elif rule == "rms":
        vn = a1 * v + (1 - a1) * gp * gp
        venv = (a1 * v).abs() + (1 - a1) * genv * genv
        d = (vn + eps).sqrt() if defect == "eps_in_sqrt" else vn.sqrt() + eps
        if mu > 0:
            menv = (mu * m).abs() + genv / d
            if defect == "rms_lr_in_buf":
                m = mu * m + lr * gp / d
                upd = m
            else:
                m = mu * m + gp / d
                upd = lr * m
            uenv = lr * menv
        else:
            menv = m.abs()
            upd, uenv = lr * gp / d, lr * genv / d
        pn, v = p - upd, vn
    else:
        bc1, bc2 = (1.0, 1.0) if defect == "no_bias_correction" else (1.0 - a1 ** t, 1.0 - b2 ** t)
        pd = torch.where(dec, p - lr * wd * p, p) if rule == "adamW" and defect != "decay_after" else p
        menv = (a1 * m).abs() + (1 - a1) * genv
        venv = (b2 * v).abs() + (1 - b2) * genv * genv
        m = a1 * m + (1 - a1) * gp
        v = b2 * v + (1 - b2) * gp * gp
        d = (v / bc2 + eps).sqrt() if defect == "eps_in_sqrt" else v.sqrt() / math.sqrt(bc2) + eps
        upd, uenv = (lr / bc1) * m / d, (lr / bc1) * menv / d
        pn = pd - upd
        if rule == "adamW" and defect == "decay_after":
            pn = torch.where(dec, pn - lr * wd * pn, pn)
    return pn, m, v, p.abs() + decay_env + uenv, menv, venv


def case_data(n, seed):
    """p, m, v, three gradients (fp32, CPU) of the kernel tests: weights and second moments bounded away from zero, as a trained model's are -- the bound
    of p is relative to |p|, and next to a weight of 1e-5 the fp32 rounding of the state alone would be a visible share of it (tests/test_optim_fp64_gpu.py)"""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda: torch.randn(n, generator=gen, dtype=torch.float64)       # noqa: E731
    z = rn()
    p, m, v = (torch.sign(z) * (0.5 + z.abs())).float(), (0.1 * rn()).float(), (0.01 * (0.25 + rn() ** 2)).float()
    grads = [rn().float() for _ in range(3)]
    for g in grads:
        g[-1] = 1.0                                        # the last element's update is worth many bounds under every rule and clip
    return p, m, v, grads


def rule_hyp(rule, mu=0.0):
    """keyword arguments of update_ref for the kernel tests' hyper-parameters"""
    h = dict(HYP, mu=mu)
    if rule == "rms":
        h["a1"] = RMS_ALPHA
    return h
