"""The distillation path of a pretraining step through its two new defaults (-m gpu), on the small models of tests/test_model_gpu.py (H 128 / 256):
  * makd_pretrain.kd_flush issues the embedding terms as ONE magic_kd_emb launch (MAGIC_NO_KD_FUSED=1, i.e. ops.KD_FUSED off: grouped projection GEMM ->
    mse_multi -> grouped input-gradient GEMM) -- the same ten kdl_terms to 1e-5 (fp32 atomic sums), the new entry once in the launch log and two grouped GEMM
    launches fewer; a shape-bucketed (plan["dyn"]) step under graph replay agrees the same way;
  * trainer.teacher_forward with MAGIC_TEACHER_ALL_HEADS=0 stops the frozen teacher behind its encoders (1, the default: the full forward) -- every tensor makd_pretrain.terms reads is
    torch.equal, the trimmed mlm forward has no gather, no transform and no vocabulary GEMM, and the student's next step gives the same loss terms to 1e-5;
  * the per-op forms behind the heads' fused launches (host/heads.py: sap loss, cfp loss, the mlm / mrc transform) give the same step as the defaults."""
import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from magic_amd.host import synth
from magic_amd.host.loader import pack_bucketed
from magic_amd.host.plan import build_plan
from magic_amd.host.stream_graph import StreamStep
from magic_amd.host.trainer import PretrainStep
from tests.test_model_gpu import KDL, RW, build

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
VOCAB = 600
READ = ("txt_embeds", "txt_attns", "pano_embeds", "pano_fused_embeds", "img_attns", "gmap_embeds", "gmap_attns", "vp_embeds", "vp_attns", "fused_logits")
_M = {}


def models():
    """one teacher / student / trainer for the module (no test here takes an optimizer step with them)"""
    if not _M:
        _, _, g_t, g_s = build(torch.bfloat16)
        g_s.keep_mlm_logits = False
        _M.update(t=g_t, s=g_s, tr=PretrainStep(g_s, g_t, lr=5e-5, warmup_steps=2, num_train_steps=40))
    return _M["t"], _M["s"], _M["tr"]


def models32():
    """the same models in fp32 storage with the mrc head: the per-op and the fused form of a head differ by fp32 summation order only"""
    if "s32" not in _M:
        _, _, g_t, g_s = build(torch.float32, pretrain_tasks={"mlm", "mrc", "sap", "cfp"})
        g_s.keep_mlm_logits = False
        _M.update(t32=g_t, s32=g_s)
    return _M["t32"], _M["s32"]


def batch_of(task):
    b = synth.make_batch(task, batch_size=6, seed=21, vocab=VOCAB, min_len=8, max_len=19, min_steps=2, max_steps=4)
    return synth.batch_to(b, DEV), build_plan(b, task, DEV)


def logged(fn):
    """fn() with every launch of the C ABI logged: (result, [names], [leading integer arguments])"""
    L.PROFILE.update(on=True, events=[], shapes=[])
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.PROFILE["on"] = False
    names, shapes = [e[0] for e in L.PROFILE["events"]], L.PROFILE["shapes"]
    L.PROFILE.update(events=[], shapes=None)
    return out, names, shapes


def student_step(g_s, bd, task, plan, t_out):
    g_s.store.zero_grad()
    out = g_s(bd, task, compute_loss=True, teacher_outputs=t_out, rw=RW, plan=plan, inputs=t_out["inputs"])
    g_s.backward()
    torch.cuda.synchronize()
    grad = torch.cat([p.grad.flatten().float() for _, p in g_s.named_parameters()])
    return {k: float(v) for k, v in out["kdl_terms"].items()}, {k: float(out[k]) for k in ("loss", "supervised_loss", "kdl_loss")}, grad


def same_terms(a, b, tag):
    assert set(a) == set(b) and len(a) in (3, 10), tag
    for k, v in b.items():
        assert abs(a[k] - v) <= 1e-5 * abs(v), (tag, k, a[k], v)


@pytest.mark.parametrize("task", ["sap", "mlm", "cfp"])
def test_fused_embedding_terms_equal_the_three_launch_sequence(task, monkeypatch):
    g_t, g_s, tr = models()
    bd, plan = batch_of(task)
    t_out = tr.teacher_forward(bd, task, plan)
    (terms, _, grad), names, _ = logged(lambda: student_step(g_s, bd, task, plan, t_out))
    monkeypatch.setattr(O, "KD_FUSED", False)
    (terms0, _, grad0), names0, _ = logged(lambda: student_step(g_s, bd, task, plan, t_out))
    same_terms(terms, terms0, task)
    assert sum(abs(v) > 0 for v in terms.values()) >= 7, terms
    assert names.count("magic_kd_emb") == 1 and names0.count("magic_kd_emb") == 0
    assert names.count("magic_gemm+group") == names0.count("magic_gemm+group") - 2, (names.count("magic_gemm+group"), names0.count("magic_gemm+group"))
    assert len(names) == len(names0) - 1 and names.count("magic_mse_multi") == names0.count("magic_mse_multi") == 1
    rel = ((grad - grad0).norm() / grad0.norm()).item()
    cos = torch.nn.functional.cosine_similarity(grad, grad0, dim=0).item()
    print(f"{task}: {len(names)} launches against {len(names0)}; parameter gradients rel. diff {rel:.2e}, cosine {cos:.7f}")
    assert rel < 1e-2 and cos > 0.9999, (rel, cos)          # the same backward behind the new launch (fp32 atomics and at most 16-bit roundings apart)


@pytest.mark.parametrize("task, fused_entry", [("sap", "magic_sap_fuse_loss"), ("cfp", "magic_cfp_loss"), ("mlm", "magic_linear_act_ln"), ("mrc", "magic_linear_act_ln")])
def test_per_op_head_forms_equal_the_fused_launches(task, fused_entry, monkeypatch):
    """ops.SAP_LOSS_FUSED off (fusion, three CE launches, teacher-sample weights and action-distillation rows one by one), MAGIC_NO_FUSED_CFP (similarity GEMMs
    + CE rows + four gradient GEMMs per term), model_pretrain.MLM_TAIL_FUSED off (dense, LayerNorm, cast, LayerNorm backward and activation derivative apart)"""
    import magic_amd.host.model_pretrain as MP
    g_t, g_s = models32()
    bd, plan = batch_of(task)
    with torch.no_grad():
        t_out = g_t(bd, task, compute_loss=False, return_outputs=True, plan=plan)
    (terms, losses, grad), names, _ = logged(lambda: student_step(g_s, bd, task, plan, t_out))
    monkeypatch.setattr(O, "SAP_LOSS_FUSED", False)
    monkeypatch.setenv("MAGIC_NO_FUSED_CFP", "1")
    monkeypatch.setattr(MP, "MLM_TAIL_FUSED", False)
    (terms0, losses0, grad0), names0, _ = logged(lambda: student_step(g_s, bd, task, plan, t_out))
    assert fused_entry in names and fused_entry not in names0
    same_terms(terms, terms0, task)
    same_terms(losses, losses0, task)
    rel = ((grad - grad0).norm() / grad0.norm()).item()
    cos = torch.nn.functional.cosine_similarity(grad, grad0, dim=0).item()
    print(f"{task}: {len(names)} launches against {len(names0)}; parameter gradients rel. diff {rel:.2e}, cosine {cos:.7f}")
    assert rel < 1e-2 and cos > 0.9999, (rel, cos)


def test_bucketed_step_under_graph_replay_agrees(monkeypatch):
    """plan["dyn"]: the launch covers the bucket's extent, the true extents and normalisers come from device memory"""
    rw = torch.tensor(RW, dtype=torch.float32, device=DEV)
    b = synth.make_batch("sap", batch_size=6, seed=21, vocab=VOCAB, min_len=8, max_len=19, min_steps=2, max_steps=4)
    calls = []
    real = O.kd_emb
    monkeypatch.setattr(O, "kd_emb", lambda probs: (calls.append([q.get("valid_dev") is not None for q in probs]), real(probs))[1])
    got = []
    for fused in (True, False):
        monkeypatch.setattr(O, "KD_FUSED", fused)
        _, _, g_t, g_s = build(torch.bfloat16)
        g_s.keep_mlm_logits = False
        ss = StreamStep(PretrainStep(g_s, g_t, lr=5e-5, warmup_steps=2, num_train_steps=40), rw=rw)
        out, meta = ss.step("sap", pack_bucketed(b, "sap"))
        torch.cuda.synchronize()
        got.append({k: float(v) for k, v in out["kdl_terms"].items()})
    assert calls and all(len(c) == 5 and all(c) for c in calls), calls       # the fused launch, every term with device-side extents
    same_terms(got[0], got[1], "bucketed sap")


@pytest.mark.parametrize("task", ["mlm", "cfp", "sap"])
def test_teacher_forward_computes_only_what_distillation_reads(task, monkeypatch):
    g_t, g_s, tr = models()
    bd, plan = batch_of(task)
    if task == "sap":          # (KDL of the small models reads the teacher's logits: their sap forward keeps its heads.  Without those two terms it stops too)
        monkeypatch.setattr(g_s.config, "kdl", dict(KDL, teacher_sample_hard_mining=False, kdl_tasks=[k for k in KDL["kdl_tasks"] if k != "predict"]))
    monkeypatch.setenv("MAGIC_TEACHER_ALL_HEADS", "0")
    trimmed, names, shapes = logged(lambda: tr.teacher_forward(bd, task, plan))
    monkeypatch.setenv("MAGIC_TEACHER_ALL_HEADS", "1")
    full, names_f, shapes_f = logged(lambda: tr.teacher_forward(bd, task, plan))
    monkeypatch.delenv("MAGIC_TEACHER_ALL_HEADS")
    assert set(tr.teacher_forward(bd, task, plan)) == set(full), "the full forward is the default"
    head_keys = {"mlm": {"predict"}, "cfp": {"cfp"}, "sap": {"global_logits", "local_logits", "fused_logits"}}[task]
    assert head_keys <= set(full) and not (head_keys & set(trimmed)) and set(full) - head_keys == set(trimmed)
    n = 0
    for k in READ:
        if k in full and k not in head_keys:
            assert torch.equal(trimmed[k], full[k]), k
            n += 1
    assert n == {"mlm": 7, "cfp": 9, "sap": 9}[task]
    assert len(names) < len(names_f)
    if task == "mlm":
        # (a grouped launch is logged once, without arguments: the argument log lines up with the other entries)
        vocab_gemm = lambda nms, sh: [s for nm, s in zip([x for x in nms if x != "magic_gemm+group"], sh) if nm == "magic_gemm" and VOCAB in s[4:7]]
        assert "magic_linear_act_ln" in names_f and "magic_csr_gather" in names_f and len(vocab_gemm(names_f, shapes_f)) == 1
        assert "magic_linear_act_ln" not in names and "magic_csr_gather" not in names and not vocab_gemm(names, shapes)
    if task == "cfp":
        assert "magic_csr_gather_multi" in names_f and "magic_csr_gather_multi" not in names
    terms, losses, _ = student_step(g_s, bd, task, plan, trimmed)
    terms_f, losses_f, _ = student_step(g_s, bd, task, plan, full)
    same_terms(terms, terms_f, task)
    same_terms(losses, losses_f, task)


def test_sap_teacher_keeps_its_heads_when_a_term_reads_the_logits(monkeypatch):
    g_t, g_s, tr = models()
    monkeypatch.setenv("MAGIC_TEACHER_ALL_HEADS", "0")
    bd, plan = batch_of("sap")
    assert KDL["teacher_sample_hard_mining"] and "predict" in KDL["kdl_tasks"]
    assert "fused_logits" in tr.teacher_forward(bd, "sap", plan)
    with pytest.raises(ValueError):
        g_t(bd, "sap", compute_loss=True, heads=False)
