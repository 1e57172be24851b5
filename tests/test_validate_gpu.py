"""The validation pass on the device (host/validate.py, the `metrics` keyword of the model's forward) against the driver's arithmetic
(pretrain_src/train_r2r_magic.py:441-587), restated here in torch on the same model's `compute_loss=False` outputs.

Small model: hidden 128, 2 / 1 / 1 layers, vocabulary 1031; per task 3 batches of 6, 6 and 4 samples (batch seed SEED).

Counts.  The driver takes its argmax on what the model returns; the pass takes it where the logits are made.  Those are the same numbers -- and the counts
must agree exactly, bar an exact tie -- except for the two places where the driver's numbers went through a 16-bit rounding the pass does not do: the MLM
logits (the pass reads the fp32 accumulators) and the CFP similarities (the driver's 16-bit matmul and division).  A row is inside the rounding band when,
MLM: its top-2 gap on the driver's logits is at most one unit in the last place of the 16-bit type at the row's largest magnitude; CFP: the driver's own
rounded similarities do not single out the winner of float64 on the same head outputs.
The test counts such rows on the driver's outputs and the float64 reference alone and allows exactly that many differences: at most ONE per task at 16-bit
and none at fp32.

The model's weight matrices are at WSCALE = 4 times the 0.02 initialisation, i.e. at about unit gain per sub-layer (0.02 x 4 x sqrt(128) = 0.9), as
a trained checkpoint's are.  At the raw initialisation every sub-layer adds a few per cent to the residual stream, the [CLS] rows of all samples are the
same vector to three digits, and the driver's bf16 matmul + division ties or reorders 4-12 of the 48 CFP similarity rows whatever the batch seed (seeds
77-92, measured on an MI355X): a test of the driver's rounding, not of the pass.  SEED and WSCALE were checked against the cap before they were committed
(rows inside the band at SEED = 87: bf16 mlm 1, fp16 mlm 1, every other task and type 0).

Losses.  Where both sides read the same numbers (fp32 model: every task; 16-bit: sap, mrc) the pass is held to tests/test_eval_tail_gpu.py's bounds
against float64 on those numbers.  16-bit MLM: the pass must be at least as close to float64 on the rounded operands (the transform's output, the word
embeddings, the bias) as the driver's own loop is."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import magic_amd  # noqa: F401
from magic_amd.host import ops as O
from magic_amd.host import synth
from magic_amd.host import validate as V
from magic_amd.host.bucket import bucket_of
from magic_amd.host.loader import pack_bucketed

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 87
WSCALE = 4.0            # weight matrices at this multiple of the 0.02 initialisation
VOCAB, H = 1031, 128
TASKS = ("mlm", "mrc", "sap", "cfp")
TEMP = 0.5
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
_MODELS, _BATCHES = {}, {}


def model_of(name):
    """the small model at WSCALE x the 0.02 initialisation of its weight matrices (biases and LayerNorm parameters perturbed as tests/test_model_gpu.py's
    build does): see the docstring"""
    if name not in _MODELS:
        from magic_amd.host.model_pretrain import GlocalTextPathCMTPreTraining
        from oracle import model_ref as R
        from tests.test_model_gpu import cfgs
        _, scfg = cfgs(vocab=VOCAB, pretrain_tasks=set(TASKS))
        torch.manual_seed(0)
        ref = R.RefPretrainModel(scfg).eval()
        with torch.no_grad():
            for n, p in ref.named_parameters():
                if n.endswith("bias"):
                    p.normal_(0, 0.02)
                elif "LayerNorm.weight" in n or "layer_norm.weight" in n or n.endswith("net.2.weight") or n.endswith("embeddings.1.weight"):
                    p.add_(torch.randn_like(p) * 0.05)
                elif p.dim() == 2:
                    p.mul_(WSCALE)
        _MODELS[name] = GlocalTextPathCMTPreTraining.from_pretrained(None, config=scfg, state_dict=ref.state_dict(), device=DEV, compute_dtype=DTYPES[name])
    return _MODELS[name]


def batches(task, seed=SEED):
    if (task, seed) not in _BATCHES:
        _BATCHES[(task, seed)] = [synth.make_batch(task, batch_size=bs, seed=seed, step=i, vocab=VOCAB, min_len=8, max_len=19, min_steps=2, max_steps=4)
                                  for i, bs in enumerate((6, 6, 4))]
    return _BATCHES[(task, seed)]


def gaps(x):
    """top-2 gap and largest magnitude per row, in float64"""
    t = x.double().topk(2, dim=1).values
    return t[:, 0] - t[:, 1], x.double().abs().max(1).values


def driver_pass(model, task, bs, temperature=TEMP):
    """the driver's loop (one host read per figure and batch), plus what the test needs to judge it: rows inside the 16-bit rounding band,
    float64 sums on the same outputs and the first file's bounds on them"""
    eps = torch.finfo(model.compute_dtype).eps if model.compute_dtype != torch.float32 else 0.0
    loss, hits, n = [0.0] * 3, [0] * 3, 0
    ref, tol, band, counted = [0.0] * 3, [0.0] * 3, 0, [0] * 3
    model.eval()
    with torch.no_grad():
        for batch in bs:
            if task == "mlm":
                scores = model(batch, task="mlm", compute_loss=False)["predict"]
                lab = batch["txt_labels"]
                lab = lab[lab != -1].to(DEV)
                loss[0] += F.cross_entropy(scores, lab, reduction="sum").item()
                hits[0] += (scores.max(dim=-1)[1] == lab).sum().item()
                n += lab.numel()
                g, m = gaps(scores)
                band += int((g <= eps * m).sum())
                xd = scores.double()
                ref[0] += F.cross_entropy(xd, lab, reduction="sum").item()
                tol[0] += float((2.0 ** -23 * (torch.logsumexp(xd, 1).abs() + xd.gather(1, lab[:, None])[:, 0].abs()) + (VOCAB / 256 + 16) * 2.0 ** -24).sum())
            elif task == "mrc":
                logits, targets, _, _ = model(batch, task="mrc", compute_loss=False)
                loss[0] += F.kl_div(F.log_softmax(logits, dim=-1), targets.to(logits.dtype), reduction="sum").item()
                hits[0] += (logits.max(dim=-1)[1] == targets.max(dim=-1)[1]).sum().item()
                n += batch["vp_view_mrc_masks"].sum().item()
                g, _ = gaps(logits)
                band += int((g <= 0).sum())           # both sides read these numbers: only an exact tie could part them
                xd, td = logits.double(), targets.double()
                ref[0] += F.kl_div(F.log_softmax(xd, dim=-1), td, reduction="sum").item()
                env = (td * (torch.where(td > 0, td, torch.ones_like(td)).log().abs() + xd.abs())).sum(1) + torch.logsumexp(xd, 1).abs() * td.sum(1)
                tol[0] += float(((xd.shape[1] / 256 + 16) * 2.0 ** -24 * env).sum())
            elif task == "sap":
                o = model(batch, task="sap", compute_loss=False)
                ga, la = o["global_act_labels"].long(), o["local_act_labels"].long()
                for i, (x, lab) in enumerate(((o["global_logits"], ga), (o["local_logits"], la), (o["fused_logits"], ga))):
                    loss[i] += F.cross_entropy(x, lab, reduction="sum").item()
                    hits[i] += torch.sum(torch.argmax(x, 1) == lab).item()
                    g, _ = gaps(x)
                    band += int((g <= 0).sum())
                    xd = x.double()
                    ref[i] += F.cross_entropy(xd, lab, reduction="sum").item()
                    xl = xd.gather(1, lab.clamp(min=0)[:, None])[:, 0]          # (a local label may be -100: the target is not a candidate)
                    tol[i] += float(((2.0 ** -23 * (torch.logsumexp(xd, 1).abs() + xl.abs()) + (x.shape[1] / 256 + 16) * 2.0 ** -24) * (lab >= 0)).sum())
                    counted[i] += int((lab >= 0).sum())
                n += len(ga)
            else:
                outs = model(batch, task="cfp", compute_loss=False)
                txt = outs[3]
                tgt = torch.arange(len(txt), device=DEV)
                for i in range(3):
                    sim = (outs[i] @ txt.T) / temperature
                    loss[i] += ((F.cross_entropy(sim, tgt, reduction="sum") + F.cross_entropy(sim.T, tgt, reduction="sum")) / 2.0).item()
                    hits[i] += torch.sum(torch.argmax(sim, 1) == tgt).item()
                    ad, td = outs[i].double(), txt.double()
                    sd = ad @ td.T / temperature
                    e_s = (H + 1) * 2.0 ** -24 * float((ad.abs() @ td.abs().T).max()) / temperature
                    # inside the band: the driver's own similarities (rounded to its dtype twice at 16-bit, by the matmul and the division) do not
                    # single out the float64 winner
                    top = sim.double().topk(2, dim=1)
                    decided = (top.values[:, 0] > top.values[:, 1]) & (top.indices[:, 0] == sd.argmax(1))
                    band += int((~decided).sum())
                    ref[i] += ((F.cross_entropy(sd, tgt, reduction="sum") + F.cross_entropy(sd.T, tgt, reduction="sum")) / 2.0).item()
                    lse = torch.maximum(torch.logsumexp(sd, 1).abs(), torch.logsumexp(sd.T, 1).abs())
                    tol[i] += float((2 * e_s + (len(txt) + 16) * 2.0 ** -24 + 2.0 ** -22 * (lse + sd.diagonal().abs())).sum())
                n += len(tgt)
    return dict(loss=loss, hits=hits, n=n, ref=ref, tol=tol, band=band, counted=counted if task == "sap" else [n] * 3)


def fused_pass(model, task, items, graphs=False, validator=None):
    v = validator or V.Validator(model, graphs=graphs)
    block, seconds = v.run(task, items, TEMP if task == "cfp" else None)
    return block, V.val_log(task, block, seconds), v


@pytest.mark.parametrize("task", TASKS)
@pytest.mark.parametrize("name", list(DTYPES))
def test_validate_agrees_with_the_drivers_arithmetic(name, task, monkeypatch):
    model = model_of(name)
    bs = batches(task)
    d = driver_pass(model, task, bs)
    seen = []
    if task == "mlm" and name != "fp32":
        real = O.mlm_eval
        monkeypatch.setattr(O, "mlm_eval", lambda hm, W, bias, labels, Vv, **kw: (seen.append((hm.clone(), W, bias, labels)), real(hm, W, bias, labels, Vv, **kw))[1])
    fn = {"mlm": V.validate_mlm, "mrc": V.validate_mrc, "sap": V.validate_sap}.get(task)
    V.Validator(model)
    log = fn(model, bs) if fn else V.validate_cfp(model, bs, TEMP)
    block = model._magic_validator.last_block
    k = 1 if task in ("mlm", "mrc") else 3
    print(f"{name} {task}: driver {d['loss'][:k]} {d['hits'][:k]} / {d['n']}, pass {block['loss'][:k]} {block['hits'][:k]} / {block['rows'][:k]}, "
          f"rows inside the rounding band {d['band']}, fp64 {d['ref'][:k]}, bound {d['tol'][:k]}")
    assert d["band"] <= (0 if name == "fp32" else 1)
    assert block["rows"][:k] == d["counted"][:k] and block["rows"][0] == d["n"]      # (sap: the driver divides all three by the batch rows, :521-527)
    assert sum(abs(a - b) for a, b in zip(block["hits"][:k], d["hits"][:k])) <= d["band"]
    keys = {"mlm": ("loss", "acc", "tok_per_s"), "mrc": ("loss", "acc", "feat_per_s")}.get(task, ("gloss", "lloss", "floss", "gacc", "lacc", "facc", "tok_per_s"))
    assert tuple(log) == keys
    assert log[keys[0]] == block["loss"][0] / d["n"] and log["acc" if k == 1 else "gacc"] == block["hits"][0] / d["n"]
    same_numbers = name == "fp32" or task in ("sap", "mrc")
    if same_numbers:
        for i in range(k):
            assert abs(block["loss"][i] - d["ref"][i]) <= d["tol"][i], (i, block["loss"][i], d["ref"][i], d["tol"][i])
    if task == "mlm" and name != "fp32":
        assert len(seen) == len(bs), "the fused MLM tail ran"
        ref = 0.0
        for hm, W, bias, labels in seen:
            x = hm.double() @ W[:VOCAB].double().T + bias[:VOCAB].double()
            ref += F.cross_entropy(x, labels.long(), ignore_index=-1, reduction="sum").item()
        print(f"  fp64 on the rounded operands {ref}: pass off by {abs(block['loss'][0] - ref):.3e}, driver off by {abs(d['loss'][0] - ref):.3e}")
        assert abs(block["loss"][0] - ref) <= abs(d["loss"][0] - ref)


def test_metrics_none_changes_nothing_and_the_block_form_returns_none():
    model = model_of("bf16").eval()
    for task in TASKS:
        b = batches(task)[0]
        with torch.no_grad():
            before = model(b, task=task, compute_loss=False)
            blk = O.eval_block(DEV)
            assert model(b, task=task, compute_loss=False, metrics=blk) is None
            after = model(b, task=task, compute_loss=False)
        flat = lambda o: [x for x in (o.values() if isinstance(o, dict) else o) if torch.is_tensor(x)]       # noqa: E731
        assert len(flat(before)) == len(flat(after)) > 0
        for x, y in zip(flat(before), flat(after)):
            assert x.dtype == y.dtype and torch.equal(x, y), task
        assert int(blk[8]) > 0
    with pytest.raises(ValueError):
        model(batches("sap")[0], task="sap", compute_loss=True, metrics=O.eval_block(DEV))


def child_main():
    """MAGIC_NO_EVAL_FUSED=1 child: the bf16 MLM pass through the logits in memory"""
    model = model_of("bf16")
    block, _, _ = fused_pass(model, "mlm", batches("mlm"))
    print("CHILD " + json.dumps(block))


def test_unfused_switch_agrees_with_the_fused_pass():
    model = model_of("bf16")
    assert O.EVAL_FUSED and O.mlm_eval_ok(torch.bfloat16, H)
    block, _, _ = fused_pass(model, "mlm", batches("mlm"))
    env = dict(os.environ, MAGIC_NO_EVAL_FUSED="1")
    r = subprocess.run([sys.executable, "-c", "import tests.test_validate_gpu as T; assert not T.O.EVAL_FUSED; T.child_main()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
    d = driver_pass(model, "mlm", batches("mlm"))
    assert child["hits"] == block["hits"] and child["rows"] == block["rows"]
    # the child read logits rounded to bf16: half a unit in the last place of each row's lse and label logit; the fused side carries the first file's bound
    with torch.no_grad():
        half_ulp = 0.0
        for b in batches("mlm"):
            x = model(b, task="mlm", compute_loss=False)["predict"].double()
            half_ulp += float((torch.finfo(torch.bfloat16).eps * x.abs().max(1).values).sum())
    print(f"fused {block['loss'][0]} unfused {child['loss'][0]} bound {half_ulp + d['tol'][0]}")
    assert abs(child["loss"][0] - block["loss"][0]) <= half_ulp + d["tol"][0]


def _key(task, b):
    return (task, len(b["txt_lens"]), tuple(sorted(bucket_of(b, task).items())))


@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_graph_replay_on_bucketed_records_equals_the_eager_pass(name):
    model = model_of(name)
    model.train()
    vg = V.Validator(model, graphs=True)
    want_captures = 0
    for task in TASKS:
        bs = batches(task)
        eager, _, _ = fused_pass(model, task, bs)
        assert model.training, "the previous mode is restored"
        recs = [pack_bucketed(b, task) for b in bs]
        want_captures += len({_key(task, b) for b in bs})
        got, _, _ = fused_pass(model, task, recs, validator=vg)
        assert vg.captures == want_captures, "a layout is captured once"
        again, _, _ = fused_pass(model, task, recs, validator=vg)
        assert vg.captures == want_captures, "and reused"
        assert again == got, "a second pass starts from a zeroed block and gives the same bits"
        print(f"{name} {task}: eager {eager} graphs {got} captures {vg.captures}")
        assert got["hits"] == eager["hits"] and got["rows"] == eager["rows"]
        rtol = 1e-5 if name == "fp32" else 2e-3          # bf16: the padded keys move roundings inside the encoders (tests/test_stream_graph_gpu.py's bound)
        for a, b in zip(got["loss"], eager["loss"]):
            assert abs(a - b) <= rtol * max(abs(b), 1e-6), (task, a, b)
    model.eval()
    fused_pass(model, "sap", batches("sap"))
    assert not model.training


def test_no_host_read_inside_the_batch_loop():
    model = model_of("bf16").eval()
    bs = batches("sap")
    recs = [pack_bucketed(b, "sap") for b in bs]
    ve, vg = V.Validator(model), V.Validator(model, graphs=True)
    with torch.no_grad():
        vg.accumulate("sap", recs)                 # captures (a capture synchronises) happen in the warm-up pass
        ve.accumulate("sap", bs)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            try:
                o = model(bs[0], task="sap", compute_loss=False)
                F.cross_entropy(o["global_logits"], o["global_act_labels"].long(), reduction="sum").item()
                control = False
            except RuntimeError:
                control = True
            if control:
                ve.accumulate("sap", bs)
                vg.accumulate("sap", recs)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    if not control:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on the driver-style loop's .item() on this torch")
    assert int(ve.block[8]) == 2 * sum(len(b["txt_lens"]) for b in bs) == int(vg.block[8])


@pytest.mark.parametrize("task", ["mlm", "sap"])
def test_replayed_layouts_follow_a_change_of_the_master_weights(task):
    """a cached graph never enters the model's forward, where the 16-bit weight shadow is refreshed: the pass must refresh it itself.  Replay, change the
    master weights in place (+ mark_params_dirty, as after a step of a foreign optimizer or load_state_dict), replay the SAME graphs: the block must be the
    eager pass's on the new weights, not the old one"""
    model = model_of("bf16")
    bs = batches(task)
    recs = [pack_bucketed(b, task) for b in bs]
    vg = V.Validator(model, graphs=True)
    old, _, _ = fused_pass(model, task, recs, validator=vg)
    captures = vg.captures
    saved = model.store.flat.clone()
    try:
        with torch.no_grad():
            model.store.flat.mul_(1.25)
        model.mark_params_dirty()
        got, _, _ = fused_pass(model, task, recs, validator=vg)
        want, _, _ = fused_pass(model, task, bs, validator=V.Validator(model, graphs=False))
    finally:
        with torch.no_grad():
            model.store.flat.copy_(saved)
        model.mark_params_dirty()
    back, _, _ = fused_pass(model, task, recs, validator=vg)
    print(f"{task}: before {old['loss'][:3]}, new weights: graphs {got['loss'][:3]} eager {want['loss'][:3]}")
    assert vg.captures == captures, "the cached graphs were replayed"
    assert got["hits"] == want["hits"] and got["rows"] == want["rows"]
    for a, b, c in zip(got["loss"], want["loss"], old["loss"]):
        assert abs(a - b) <= 2e-3 * max(abs(b), 1e-6), (a, b)              # (the graph test's bf16 bound for padded against exact batches)
        assert b == 0 or abs(b - c) > 10 * 2e-3 * abs(b), "the weight change must show far outside that bound"
    assert back == old, "and back again: the same bits as before the change"
