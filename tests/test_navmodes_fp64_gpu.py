"""The navigator's mode functions -- host/model_nav.py (language, panorama, navigation, text_kv, Critic) and host/causal.py -- in 16-bit storage
against fp64, tensor by tensor (-m gpu).  16-bit is the arithmetic bench_nav.py times; tests/test_nav_gpu.py and tests/test_causal_gpu.py drive the
same code in fp32 storage only, where the 16-bit-only kernels never run.  Harness, reference, loss and planted defects: tests/_navmodes_ref64.py
(tied to the oracle on the CPU by tests/test_navmodes_ref64_cpu.py).

Cases (B = 4, V = 36, Kn <= 9, ragged text lengths that include 6 and L, 2 text / 2 cross-modal / 1 panorama layers, dropout 0), each in bf16 AND fp16:
  step      language -> panorama -> map assembly -> navigation (tests/test_nav_gpu.one_step), glocal_fuse on and off, L = 14;
            H = 128 (whole-encoder forwards and row-block backward: asserted by the recorders), H = 256 and H = 768 (per-op path)
  long      H = 768, B = 2, L = 130: the key-split attention forward and backward on the instruction (128 < L <= 512), asserted by the recorders
  cached    model.text_kv(txt) handed to TWO navigation calls of one episode (two nav_inputs seeds on the same text), one backward over the summed
            loss: _TextKVFn, autograd's sum of the two steps' d kv, d txt_embeds through the cache alone; H = 128 and 768.  The rollout's in-place
            accumulator is driven too, without a capture, as host/step_graphs.py does: nav_forward_body / nav_backward_body(dkv_acc=...) per step
            on the same inputs and output gradients, its content held to the same bound
  causal    all five blocks with tests/test_causal_gpu's dictionaries and driver: (add, type_2, type_1), (door, type_2, type_2), (add, type_1, type_1); H = 128
  critic    Critic on a cls_embeds-sized input: value, d input, its four parameter gradients; H = 128
  control   step at H = 768, cached at H = 128, causal `door` in fp32 storage: validates the reference independently of 16-bit rounding

Compared (tests/_navmodes_ref64.compare): every forward output by rel-L2 per sample over valid rows, masked attention columns exactly 0, the -inf
pattern of the three logit tensors, the logits by max-abs, the action argmax in every row whose oracle top-2 gap exceeds twice the logit bound, every
parameter gradient on its own by rel-L2 and cosine (classes w, b = row-sum / cancellation class, tab = touched rows of the embedding tables with
untouched rows exactly 0, sprel), exact zeros where the oracle has no gradient, and the gradients of the mode inputs (d gmap_img_embeds,
d vp_img_embeds, d txt_embeds, d of the K/V cache) per sample.

The ReLU pattern of the three ClsPrediction heads is the engine's own, replayed in the reference (tests/_navmodes_ref64.Ref64: an element within
rounding error of 0 takes the other branch, and the whole-term change of the head's weight gradient hid the 1 / 8 between fp16 and bf16 until it was);
class "relu" bounds how far from 0 the pre-activation of a differing element was.  The `door` gate's own parameters are class "gate": an analytic
zero per all-zero input row, carried as noise (tests/_navmodes_ref64.grad_class).

fp16 has no grad_scale in the navigator: the loss is multiplied by 4096 before backward() and the fp32 gradients divided by it (exact; the GradScaler
pattern of tests/test_model_gpu.py::test_fp16_*).  SCALE_NOTE below says what happens without the factor.

Bounds: 3 x the worst measured against fp64 on MI355X with MEASURE = True over every case of this file, per class, width and type (table at BOUNDS).
Two assertions do not rest on those constants: each class's fp16 error is <= 1/4 of its bf16 error (the storage epsilons differ by 8; RATIO_EXEMPT
lists the one class left out and why), and each planted defect, evaluated on the GPU case it belongs to, fails the fp16 bounds in the quantity
tests/test_navmodes_ref64_cpu.CAUGHT_BY names; bf16 detects all eleven as well (BF16_ALSO), the first two only through gradients."""
from types import SimpleNamespace

import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host.config import make_config
from tests import _navmodes_ref64 as NR
from tests.test_causal_gpu import dictionaries, step
from tests.test_nav_gpu import nav_inputs, one_step, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
MEASURE = False                 # True: record and print the worst error of every class per width and type, assert no bound (how BOUNDS was set)
FP16_SCALE = 4096.0
KW = dict(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, vocab_size=300, num_l_layers=2, num_x_layers=2, num_pano_layers=1)
CAUSAL_COMBOS = (("add", "type_2", "type_1"), ("door", "type_2", "type_2"), ("add", "type_1", "type_1"))
CLASSES = ("emb", "attn", "logit", "w", "b", "gate", "tab", "sprel", "din", "dkv", "value", "relu")
# input seeds (tests/test_nav_gpu.nav_inputs), chosen on the CPU so that the text lengths include 6 and L and the argmax precondition holds
SEEDS = {"step": (0,), "step-nogate": (0,), "long": (1,), "cached": (0, 1), "causal": (2,)}

# Measured worst on MI355X with MEASURE = True over every case of this file (bf16 / fp16), per width.  emb / attn: rel-L2 per sample of the embedding /
# attention outputs; logit: max-abs; w, b, gate, tab, sprel: rel-L2 of one parameter tensor's gradient (b = row-sum class, gate = the `door` gate's
# parameters, tests/_navmodes_ref64.grad_class); din: d gmap_img / d vp_img / d txt per sample; dkv: the K/V cache's gradient per sample and layer
# (autograd's sum and the in-place accumulator alike); value: the critic's output, max-abs; relu: |pre-activation| / row rms of the head elements
# whose ReLU branch differs between engine and reference (1 - 8 of 3.6k - 130k elements per case; tests/_navmodes_ref64.Ref64):
#   H     emb                attn               logit              w                  b                  tab
#   128   5.81e-3 / 7.40e-4  2.14e-3 / 2.61e-4  2.99e-3 / 4.56e-4  1.49e-2 / 2.56e-3  1.88e-2 / 2.88e-3  6.77e-3 / 7.34e-4
#   256   5.90e-3 / 7.42e-4  2.06e-3 / 2.61e-4  4.44e-3 / 5.70e-4  1.43e-2 / 2.05e-3  1.25e-2 / 2.12e-3  6.41e-3 / 8.02e-4
#   768   6.77e-3 / 8.52e-4  2.94e-3 / 3.62e-4  1.19e-2 / 1.13e-3  3.04e-2 / 3.28e-3  4.91e-2 / 4.88e-3  7.02e-3 / 8.60e-4
#   H     sprel              din                dkv                relu
#   128   3.74e-2 / 5.75e-3  6.72e-3 / 9.54e-4  7.06e-3 / 9.33e-4  1.50e-2 / 1.78e-3
#   256   1.72e-2 / 2.36e-3  7.05e-3 / 8.08e-4  -                  1.46e-2 / 7.54e-4
#   768   1.82e-2 / 1.99e-3  7.35e-3 / 8.92e-4  7.89e-3 / 9.63e-4  2.29e-2 / 2.57e-3
#   H = 128 only: gate 2.48e-1 / 8.11e-2 (fp32 control 1.10e-5: see RATIO_EXEMPT), value 2.47e-4 / 1.43e-5
# fp16 : bf16 per class and width: 1/5.8 - 1/19.4 (gate: 1/3.1).  BOUNDS = 3 x the worst, rounded up to two digits.
BOUNDS = {
    "bf16": {
        128: {"emb": 0.018, "attn": 0.0065, "logit": 0.009, "w": 0.045, "b": 0.057, "gate": 0.75, "tab": 0.021, "sprel": 0.12, "din": 0.021,
              "dkv": 0.022, "value": 0.00075, "relu": 0.045},
        256: {"emb": 0.018, "attn": 0.0062, "logit": 0.014, "w": 0.044, "b": 0.038, "tab": 0.02, "sprel": 0.052, "din": 0.022, "relu": 0.044},
        768: {"emb": 0.021, "attn": 0.0089, "logit": 0.036, "w": 0.092, "b": 0.15, "tab": 0.022, "sprel": 0.055, "din": 0.023, "dkv": 0.024,
              "relu": 0.069}},
    "fp16": {
        128: {"emb": 0.0023, "attn": 0.00079, "logit": 0.0014, "w": 0.0077, "b": 0.0087, "gate": 0.25, "tab": 0.0023, "sprel": 0.018, "din": 0.0029,
              "dkv": 0.0028, "value": 4.3e-05, "relu": 0.0054},
        256: {"emb": 0.0023, "attn": 0.00079, "logit": 0.0018, "w": 0.0062, "b": 0.0064, "tab": 0.0025, "sprel": 0.0071, "din": 0.0025, "relu": 0.0023},
        768: {"emb": 0.0026, "attn": 0.0011, "logit": 0.0034, "w": 0.0099, "b": 0.015, "tab": 0.0026, "sprel": 0.006, "din": 0.0027, "dkv": 0.0029,
              "relu": 0.0078}}}
# fp32 storage (the control), 3 x the measured worst.  Measured: H = 128 emb 2.46e-7, attn 6.46e-8, logit 2.21e-7, w 1.07e-6, b 1.04e-6, gate 1.10e-5,
# tab 1.88e-7, sprel 7.27e-7, din 2.13e-7, dkv 3.88e-7; H = 768 emb 3.76e-7, attn 1.79e-7, logit 5.80e-7, w 1.13e-6, b 1.11e-6, tab 3.92e-7,
# sprel 2.37e-7, din 3.72e-7; no ReLU branch differs
CONTROL = {128: {"emb": 7.4e-07, "attn": 2e-07, "logit": 6.7e-07, "w": 3.3e-06, "b": 3.2e-06, "gate": 3.4e-05, "tab": 5.7e-07, "sprel": 2.2e-06,
                 "din": 6.4e-07, "dkv": 1.2e-06, "relu": 0.0},
           768: {"emb": 1.2e-06, "attn": 5.4e-07, "logit": 1.8e-06, "w": 3.4e-06, "b": 3.4e-06, "tab": 1.2e-06, "sprel": 7.2e-07, "din": 1.2e-06,
                 "relu": 0.0}}
# measured once (step, H = 768, fp16) with the loss NOT multiplied by 4096: w 2.85e-3, b 2.75e-3, tab 8.3e-4, sprel 1.8e-3, din 8.6e-4 -- the same as
# with the factor (3.28e-3 worst over all cases), and no parameter gradient flushed to zero beyond the table rows the step never touches
SCALE_NOTE = "gradients do not underflow without the factor at these shapes; it is kept because it is what an fp16 training loop does"
STATS, COVER, _RESULTS, _PAIRS = {}, set(), {}, {}
NEED = {"enc.fused", "rbw.fused", "perop", "attn.keysplit.fwd", "attn.keysplit.bwd", "gate.on", "gate.off", "kv.used", "kv.summed",
        "kv.acc.inplace", "head_mean.bwd", "cls.gather", "cls.gather.T", "causal.back_txt", "causal.back_img", "causal.front_txt", "causal.front_vp",
        "causal.front_gmap", "causal.add", "causal.door", "causal.type_1", "causal.type_2", "critic.rowdot"}


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def case_of(kind, H, causal=None):
    base = "step" if kind == "step-nogate" else kind
    return dict(kind=kind, H=H, causal=causal, gate=kind != "step-nogate", use_kv=kind == "cached", B=2 if kind == "long" else 4,
                L=130 if kind == "long" else 14, seeds=SEEDS[kind], seed=3 + len(base), id=f"{kind}-H{H}" + ("-" + "-".join(causal) if causal else ""))


def config(case):
    kw = dict(KW, glocal_fuse=case["gate"])
    if case["causal"]:
        m, t, i = case["causal"]
        kw.update(do_back_txt=True, do_back_img=True, do_front_txt=True, do_front_img=True, do_front_his=True, do_back_txt_type=t,
                  do_back_imgobj_type=i, do_add_method=m)
    return make_config(case["H"], role="student", **kw)


def inputs_of(case):
    inps = [nav_inputs(B=case["B"], L=case["L"], V=36, seed=s) for s in case["seeds"]]
    for inp in inps[1:]:                         # one episode: the later steps see the same instruction
        inp["txt_ids"], inp["txt_masks"] = inps[0]["txt_ids"], inps[0]["txt_masks"]
    return inps


def driver_of(case):
    return step if case["causal"] else one_step


def dicts_of(case):
    return dictionaries(case["B"], case["H"], seed=3) if case["causal"] else None


def reference_of(case, o, dt, defect=None, gates=None):
    return NR.reference(o, inputs_of(case), driver_of(case), dt=dt, dz=dicts_of(case), use_kv=case["use_kv"], defect=defect, gates=gates)


def critic_inputs(H=128):
    g = torch.Generator().manual_seed(17)
    sd = {"state2value.0.weight": torch.randn(512, H, generator=g) * 0.02, "state2value.0.bias": torch.randn(512, generator=g) * 0.05,
          "state2value.3.weight": torch.randn(1, 512, generator=g) * 0.02, "state2value.3.bias": torch.randn(1, generator=g) * 0.05}
    return sd, torch.randn(4, H, generator=g)


STEP_CASES = [case_of(k, H) for H in (128, 256, 768) for k in ("step", "step-nogate")]
LONG_CASES = [case_of("long", 768)]
CACHED_CASES = [case_of("cached", H) for H in (128, 768)]
CAUSAL_CASES = [case_of("causal", 128, causal=c) for c in CAUSAL_COMBOS]
CONTROL_CASES = [case_of("step", 768), case_of("cached", 128), case_of("causal", 128, causal=CAUSAL_COMBOS[1])]
HALF_CASES = STEP_CASES + LONG_CASES + CACHED_CASES + CAUSAL_CASES


# ---- recorders -----------------------------------------------------------------------------------------------------------------------------
class Recorder:
    """tags the launch forms and hand-offs a case went through (host/ops.py entry points and the causal blocks' forward)"""

    def __init__(self, mp):
        from magic_amd.host import causal as C
        from magic_amd.host import model_nav as MN
        from magic_amd.host import ops as O
        self.tags, self.navc = set(), []
        body, navc = MN.nav_forward_body, self.navc

        def nav_body(*a, **kw):                   # keeps every navigation call's context: the heads' stored activations (their ReLU patterns)
            c, outs = body(*a, **kw)
            navc.append(c)
            return c, outs
        mp.setattr(MN, "nav_forward_body", nav_body)
        for name in ("encoder_fwd", "xencoder_fwd", "rowbwd", "attn_fwd", "attn_bwd_ks", "head_mean_bwd", "csr_gather", "rowgate_fwd"):
            mp.setattr(O, name, self._wrap(name, getattr(O, name)))
        inner, tags = C.CausalBlock.forward, self.tags

        def fwd(blk, x, z, pz=None):
            tags.update({"causal." + blk.name, "causal.door" if blk.door else "causal.add"})
            if blk.kind == "back":
                tags.add("causal." + blk.btype)
            return inner(blk, x, z, pz)
        mp.setattr(C.CausalBlock, "forward", fwd)

    def _wrap(self, name, inner):
        def f(*a, **kw):
            t = {"encoder_fwd": "enc.fused", "xencoder_fwd": "xenc.fused", "rowbwd": "rbw.fused", "head_mean_bwd": "head_mean.bwd",
                 "attn_bwd_ks": "attn.keysplit.bwd"}.get(name)
            if name == "attn_fwd" and a[11] > 128:
                t = "attn.keysplit.fwd"
            if name == "csr_gather":
                t = "cls.gather.T" if a[5] > a[0].shape[0] else "cls.gather"
            if name == "rowgate_fwd" and a[0] == 0:
                t = "critic.rowdot"
            if t:
                self.tags.add(t)
            return inner(*a, **kw)
        return f


# ---- running a case ------------------------------------------------------------------------------------------------------------------------
def models(case, dtype):
    key = (case["id"].split("-H")[0] if not case["causal"] else case["id"], case["H"], case["gate"], dtype)
    if key not in _PAIRS:
        _PAIRS.clear()              # one pair alive at a time (H = 768 in fp64 + the engine's buffers)
        _PAIRS[key] = NR.pair(config(case), DTYPES[dtype], seed=case["seed"], device=DEV)
    return _PAIRS[key]


def _engine(case, g, dtype, rec, scale=None):
    dt = DTYPES[dtype]
    scale = (FP16_SCALE if dtype == "fp16" else 1.0) if scale is None else scale
    g.store.zero_grad()
    r = NR.run(g, inputs_of(case), driver_of(case), dz=dicts_of(case), use_kv=case["use_kv"], scale=scale, device=DEV)
    torch.cuda.synchronize()
    t = r.tap
    gr = lambda x: None if x is None or x.grad is None else x.grad.detach().double().cpu() / scale           # noqa: E731
    got = SimpleNamespace(outs=[{k: v.detach().float().cpu() for k, v in o.items()} for o in r.outs], loss=r.loss.cpu(),
                          grads={n: p.grad.detach().double().cpu() / scale for n, p in g.named_parameters()},
                          din=dict(gmap_img=[gr(x) for x in t.gimg], vp_img=[gr(x) for x in t.vimg], txt=gr(t.txt)), dkv=gr(t.kv), acc=None)
    H = case["H"]
    got.gates = [dict(g=(c.Yg > 0).view(c.B, c.K, H).cpu(), l=(c.Yl > 0).view(c.B, c.Vp, H).cpu(), f=(c.Yf > 0).cpu() if c.use_gate else None)
                 for c in rec.navc[:len(t.navs)]]
    rec.tags.add("gate.on" if case["gate"] else "gate.off")
    if case["use_kv"]:
        assert got.dkv is not None and len(t.navs) == 2
        rec.tags.update({"kv.used", "kv.summed"})
        got.acc = _rollout_accumulator(case, g, r, dt, scale)
        rec.tags.add("kv.acc.inplace")
    return got


def _rollout_accumulator(case, g, r, dt, scale):
    """the episode's d kv accumulator as the captured rollout fills it (host/step_graphs.py: nav_backward_body(..., dkv_acc=slot.dkv) per step),
    driven eagerly: the same inputs, the same output gradients (this file's loss on leaf copies of the step's outputs)"""
    from magic_amd.host import model_nav as MN
    from magic_amd.host import ops as O
    t = r.tap
    txt, kv = t.txt.detach(), t.kv.detach()
    acc = torch.zeros_like(kv)
    g.store.sync_shadow()
    g.net.S.ensure_grads()
    for call, inp in enumerate(inputs_of(case)):
        b = to_dev(inp, DEV)
        c, outs = MN.nav_forward_body(g, t.gimg[call].detach(), t.vimg[call].detach(), txt, b, kv)
        leaf = {k: o.detach().clone().requires_grad_(o.is_floating_point()) for k, o in zip(NR.NAV_KEYS, outs)}
        R = NR.functionals({k: tuple(v.shape) for k, v in leaf.items() if k in NR.FUNCS}, r.masks[call], call)
        loss = NR.loss_of(leaf, inp, R, names=[k for k in NR.FUNCS if k in leaf]) * scale
        grads = torch.autograd.grad(loss, [leaf[k] for k in NR.NAV_KEYS], allow_unused=True)
        MN.nav_backward_body(g, c, *grads, dkv_acc=acc)
    O.flush_rbw_parts()
    torch.cuda.synchronize()
    return acc.double().cpu() / scale


def result(case, dtype, mp):
    key = (case["id"], dtype)
    if key not in _RESULTS:
        o, g = models(case, dtype)
        with mp.context() as m:
            rec = Recorder(m)
            got = _engine(case, g, dtype, rec)
        want = reference_of(case, o, DTYPES[dtype], gates=got.gates)
        errs = NR.compare(got, want)
        flips, margin = NR.gate_report(got.gates, want.pre)
        errs["relu"] = margin
        errs["worst"]["relu flips"] = flips
        if got.acc is not None:
            w = want.dkv
            k = got.acc.view_as(w)
            errs["dkv"] = max(errs["dkv"], max(NR.per_sample_rel(k[i], w[i]) for i in range(w.shape[0])))
        if dtype != "fp32" and not {"enc.fused", "xenc.fused", "rbw.fused"} & rec.tags:
            rec.tags.add("perop")              # 16-bit storage and no whole-encoder / row-block launch: the per-op layer path carried the step
        _RESULTS[key] = SimpleNamespace(case=case, dtype=dtype, got=got, want=want, errs=errs, tags=set(rec.tags), o=o)
        COVER.update(rec.tags)
    return _RESULTS[key]


def bounds_of(case, dtype):
    return CONTROL[case["H"]] if dtype == "fp32" else BOUNDS[dtype][case["H"]]


def class_errors(errs):
    out = {}
    for q, v in errs.items():
        if isinstance(v, float) and not q.startswith("cos "):
            c = NR.qclass(q)
            out[c] = max(out.get(c, 0.0), v)
    return out


def expected_tags(case, dtype):
    H, half = case["H"], dtype != "fp32"
    t = {"gate.on" if case["gate"] else "gate.off", "cls.gather", "cls.gather.T"}
    if case["causal"]:
        m, tt, it = case["causal"]
        t.update({"causal." + n for n in ("back_txt", "back_img", "front_txt", "front_vp", "front_gmap")} | {"causal." + m, "causal." + tt, "causal." + it})
    else:
        t.add("head_mean.bwd")
    if half and H == 128:
        t.update({"enc.fused", "rbw.fused"})
    if half and H != 128:
        t.add("perop")
    if case["kind"] == "long":
        t.update({"attn.keysplit.fwd", "attn.keysplit.bwd"})
    if case["use_kv"]:
        t.update({"kv.used", "kv.summed", "kv.acc.inplace"})
    return t


def check(case, dtype, mp):
    r = result(case, dtype, mp)
    got, want, b, tag = r.got, r.want, bounds_of(case, dtype), f"{case['id']} {dtype}"
    # exact properties
    for go, wo, mk in zip(got.outs, want.outs, want.masks):
        for name in NR.LOGITS:
            assert torch.equal(torch.isinf(go[name]), torch.isinf(wo[name])), f"{tag} {name}: -inf pattern"
        for name in ("txt_attns", "img_attns", "gmap_attns", "vp_attns"):
            if name in go:
                rows = mk[name].any(-1, keepdim=True)
                dead = rows & ~mk[name]
                assert (go[name][dead.expand_as(go[name])] == 0).all(), f"{tag} {name}: masked columns of valid rows not exactly 0"
        gap = NR.top2_gap(wo["fused_logits"])
        ok = gap > 2 * b["logit"]
        if not MEASURE:
            assert int(ok.sum()) >= len(gap) - (0 if dtype != "bf16" else 1), f"{tag}: argmax precondition (reference alone): gaps {gap.tolist()}"
            assert torch.equal(go["fused_logits"].argmax(1)[ok], wo["fused_logits"].argmax(1)[ok]), f"{tag}: action argmax"
    for name, w in want.grads.items():
        k = got.grads[name]
        if w is None:
            assert k.abs().max().item() == 0.0, f"{tag} {name}: the oracle has no gradient here"
        elif NR.analytically_zero(name):
            top = max(v.norm().item() for v in want.grads.values() if v is not None)
            assert k.norm().item() < 1e-3 * top and w.norm().item() < 1e-6 * top, f"{tag} {name}: analytically zero"
        elif NR.grad_class(name) == "tab":
            rows = w.abs().amax(1) > 0
            assert (k[~rows] == 0).all(), f"{tag} {name}: rows the step never touched are not exactly 0"
    ce = class_errors(r.errs)
    for c, v in ce.items():
        kk = (dtype, case["H"], c)
        STATS[kk] = max(STATS.get(kk, 0.0), v)
    if MEASURE:
        print(f"[measure] {tag}: " + " ".join(f"{q}={v:.3g}" for q, v in sorted(r.errs.items()) if isinstance(v, float)))
        gaps = [round(x, 5) for x in NR.top2_gap(want.outs[0]["fused_logits"]).tolist()]
        print(f"[measure] {tag}: worst tensors {r.errs.get('worst')} tags {sorted(r.tags)} gaps {gaps}")
        miss = expected_tags(case, dtype) - r.tags
        if miss:
            print(f"[measure] {tag}: expected tags not seen {sorted(miss)}")
        return r
    for q, v in r.errs.items():
        if isinstance(v, float):
            if q.startswith("cos "):
                assert v < 1e-3, f"{tag} {q}: cosine {1 - v:.6f}"
            else:
                assert v <= b[NR.qclass(q)], f"{tag} {q}: {v:.3e} (bound {b[NR.qclass(q)]:.3g}; worst tensors {r.errs.get('worst')})"
    assert not expected_tags(case, dtype) - r.tags, f"{tag}: branches not reached {sorted(expected_tags(case, dtype) - r.tags)}"
    if dtype != "fp32" and case["H"] != 128:
        assert not {"enc.fused", "xenc.fused", "rbw.fused"} & r.tags, f"{tag}: a fused H = 128 form ran"
    return r


# ---- tests ---------------------------------------------------------------------------------------------------------------------------------
HALF = ("bf16", "fp16")


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: c["id"])
def test_step_vs_fp64(case, dtype, monkeypatch):
    check(case, dtype, monkeypatch)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("case", LONG_CASES, ids=lambda c: c["id"])
def test_long_instruction_key_split_vs_fp64(case, dtype, monkeypatch):
    check(case, dtype, monkeypatch)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("case", CACHED_CASES, ids=lambda c: c["id"])
def test_cached_text_kv_two_steps_vs_fp64(case, dtype, monkeypatch):
    check(case, dtype, monkeypatch)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("case", CAUSAL_CASES, ids=lambda c: c["id"])
def test_causal_blocks_vs_fp64(case, dtype, monkeypatch):
    check(case, dtype, monkeypatch)


def _critic(dtype, mp):
    NS = SimpleNamespace
    from magic_amd.host.model_nav import Critic
    key = ("critic", dtype)
    if key in _RESULTS:
        return _RESULTS[key]
    dt, scale = DTYPES[dtype], FP16_SCALE if dtype == "fp16" else 1.0
    sd, x = critic_inputs()
    with mp.context() as m:
        rec = Recorder(m)
        c = Critic(NS(hidden_size=128, dropout=0.0), compute_dtype=dt)
        c.load_state_dict(sd)
        c.train()
        c.store.zero_grad()
        xg = x.to(DEV).to(dt).requires_grad_(True)
        v = c(xg)
        (NR.critic_loss(v) * scale).backward()
        torch.cuda.synchronize()
    want_v, want_dx, want_g = NR.critic_reference(sd, x, dt)
    gp = {n: p.grad.detach().double().cpu() / scale for n, p in c.named_parameters()}
    errs = {"value": (v.detach().double().cpu() - want_v).abs().max().item(), "din x": NR.per_sample_rel(xg.grad.double().cpu() / scale, want_dx)}
    for n, w in want_g.items():
        q = "grad " + NR.grad_class(n)
        errs[q] = max(errs.get(q, 0.0), NR.rel_cos(gp[n], w)[0])
    COVER.update(rec.tags)
    _RESULTS[key] = NS(errs=errs, tags=set(rec.tags), v=v.detach().double().cpu(), sd=sd, x=x, dtype=dtype)
    return _RESULTS[key]


@pytest.mark.parametrize("dtype", HALF)
def test_critic_head_vs_fp64(dtype, monkeypatch):
    r = _critic(dtype, monkeypatch)
    for c, v in class_errors(r.errs).items():
        STATS[(dtype, 128, c)] = max(STATS.get((dtype, 128, c), 0.0), v)
    if MEASURE:
        print(f"[measure] critic {dtype}: {r.errs} tags {sorted(r.tags)}")
        return
    assert "critic.rowdot" in r.tags
    for q, v in r.errs.items():
        assert v <= BOUNDS[dtype][128][NR.qclass(q)], f"critic {dtype} {q}: {v:.3e}"


@pytest.mark.parametrize("case", CONTROL_CASES, ids=lambda c: c["id"])
def test_fp32_control(case, monkeypatch):
    """the same harness on fp32 storage: validates the reference independently of 16-bit rounding"""
    check(case, "fp32", monkeypatch)


def _defect_case(n):
    kind = NR.DEFECTS[n][2]
    return case_of("causal", 128, causal={9: CAUSAL_COMBOS[1], 10: CAUSAL_COMBOS[2]}[n]) if kind == "causal" else case_of(kind, 128)


# which planted defects the bf16 bounds detect as well: all of them; 1 and 2 through parameter gradients only (their forward effect, 9e-3 and 2e-3 of
# gmap_embeds, sits inside bf16's rounding: fp16 is the type that pins the forward formulas)
BF16_ALSO = set(range(1, 12))


@pytest.mark.parametrize("n", sorted(NR.DEFECTS))
def test_planted_defect_fails_the_fp16_bounds_on_its_gpu_case(n, monkeypatch):
    from tests.test_navmodes_ref64_cpu import CAUGHT_BY
    caught = {}
    for dtype in HALF:
        b = BOUNDS[dtype][128]
        if n == 11:
            r = _critic(dtype, monkeypatch)
            bad = NR.critic_reference(r.sd, r.x, DTYPES[dtype], defect=11)[0]
            moved = {"value": (r.v - bad).abs().max().item()}
        else:
            case = _defect_case(n)
            r = result(case, dtype, monkeypatch)
            bad = reference_of(case, r.o, DTYPES[dtype], defect=n, gates=r.got.gates)
            moved = {q: v for q, v in NR.compare(r.got, bad).items() if isinstance(v, float) and not q.startswith("cos ")}
        caught[dtype] = sorted(q for q, v in moved.items() if v >= b[NR.qclass(q)])
        if MEASURE:
            print(f"[measure] defect {n} {dtype}: " + " ".join(f"{q}={v:.3g}" for q, v in sorted(moved.items())))
    if MEASURE:
        return
    assert CAUGHT_BY[n] in caught["fp16"], f"defect {n} ({NR.DEFECTS[n][0]}) passes the fp16 bounds: fails only {caught['fp16']}"
    assert bool(caught["bf16"]) == (n in BF16_ALSO), f"defect {n}: bf16 catches {caught['bf16']}"


# left out of the 1/4 assertion.  No class has a bf16 error under 10 x the fp32 control's.  "gate": one scalar's noise per tensor (an analytic zero per
# all-zero input row, see grad_class): 1.10e-5 in fp32, 8.1e-2 in fp16, 2.5e-1 in bf16 -- 170x, 165x and 64x the storage epsilon, i.e. the fp16 : bf16
# ratio of 1/3.1 is the draw's, not an error's; the class keeps its 3x bounds
RATIO_EXEMPT = {"gate"}


def test_zz_fp16_error_is_an_eighth_of_bf16_per_class(monkeypatch):
    """each class's fp16 error <= 1/4 of its bf16 error, per width (the storage epsilons differ by 8): rounding noise, no scaling or sign error"""
    for case in HALF_CASES:
        for dtype in HALF:
            check(case, dtype, monkeypatch)
    for case in CONTROL_CASES:
        check(case, "fp32", monkeypatch)
    for dtype in HALF:
        test_critic_head_vs_fp64(dtype, monkeypatch)
    for H in (128, 256, 768):
        for c in CLASSES:
            a, b = STATS.get(("fp16", H, c)), STATS.get(("bf16", H, c))
            if a is None or b is None:
                continue
            ctl = max([v for (d, h, cc), v in STATS.items() if d == "fp32" and cc == c] or [0.0])
            print(f"[ratio] H={H} {c:6s} bf16 {b:.3e} fp16 {a:.3e} fp16:bf16 1/{b / max(a, 1e-300):.1f} fp32 control {ctl:.2e}")
            if MEASURE or c in RATIO_EXEMPT:
                continue
            assert b >= 10 * ctl, f"H={H} {c}: bf16 error {b:.3e} is within 10x of the fp32 control {ctl:.3e}: list the class in RATIO_EXEMPT"
            assert a <= b / 4, f"H={H} {c}: fp16 {a:.3e} against bf16 {b:.3e}"


def test_fp16_step_without_the_loss_factor_stays_inside_the_bounds(monkeypatch):
    """the fp16 step at H = 768 once more with the loss NOT multiplied by 4096 (SCALE_NOTE): no gradient class leaves its bound, so nothing underflows
    at these shapes and the factor is not what makes the fp16 cases pass"""
    case = STEP_CASES[4]
    assert case["id"] == "step-H768"
    o, g = models(case, "fp16")
    with monkeypatch.context() as m:
        rec = Recorder(m)
        got = _engine(case, g, "fp16", rec, scale=1.0)
    e = class_errors(NR.compare(got, reference_of(case, o, torch.float16, gates=got.gates)))
    if MEASURE:
        zeros = sum(int((v == 0).sum()) for v in got.grads.values()) / sum(v.numel() for v in got.grads.values())
        print(f"[measure] {case['id']} fp16 WITHOUT the 4096 factor: " + " ".join(f"{q}={v:.3g}" for q, v in sorted(e.items()))
              + f"; exact zeros among the parameter gradients {zeros:.3%}")
        return
    for c, v in e.items():
        assert v <= BOUNDS["fp16"][768][c], f"{case['id']} fp16 without the loss factor, class {c}: {v:.3e}"


def test_every_named_branch_is_reached():
    union = set()
    for case in HALF_CASES:
        for dtype in HALF:
            union |= expected_tags(case, dtype)
    union.add("critic.rowdot")                 # (test_critic_head_vs_fp64 asserts it)
    assert not NEED - union, f"no case is expected to reach {sorted(NEED - union)}"
    if COVER:
        print(f"[branches] seen in this process: {sorted(COVER)}")


def test_zzz_report_measured_worst():
    """prints (with -s) the worst error per type, width and class that this process measured (what BOUNDS / CONTROL were set from)"""
    for key in sorted(STATS, key=str):
        print(f"navmodes fp64 {key[0]:5s} H={key[1]:<4d} {key[2]:6s} worst {STATS[key]:.4g}")
