"""Mint tests/golden/makd_kl.pt from the reference's own functions (needs the reference tree at the path mint_golden.REF names).

Run:  python tests/golden/mint_makd_kl.py
What is minted -- tensors, names and numbers only; inputs stored as fp32, every recorded value is what the reference returns on their .double() copies:
  (a) "prim":  map_nav_src/utils/kd_loss.py kd_loss on 2-D (600 classes), 3-D and 4-D inputs, T in {1, 2}, loss_type sum / mean, with and
               without sample weights, some entries -inf
  (b) "agent": GMapNavAgent.compute_kd_losses (map_nav_src/r2r/agent.py:546-719) with kdl_feat_loss / kdl_attn_loss bound to kd_loss as
               agent_base.py:156-164 does for 'kl', kdl_temperature = 2, on the inputs of makd_agent.pt (B 4, L 12, K 7, V 9, H 32 -> 64, heads 2 vs 4;
               not stored twice): (feat, attn) in {(kl, mse), (mse, kl), (kl, kl)} x {t2s sum, t2s mean, s2t} x t in {0, 1} x {RW weights, none}
"""
import os
import sys
import types
from collections import defaultdict
from types import SimpleNamespace

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from mint_golden import REF, stub  # noqa: E402


def _import_reference():
    sys.path.insert(0, f"{REF}/map_nav_src")
    stub(["MatterSim", "line_profiler", "jsonlines", "h5py", "spacy", "nltk", "tensorboardX", "progressbar"])
    models = types.ModuleType("models")
    for sub, attrs in (("graph_utils", ["GraphMap"]), ("model", ["VLNBert", "Critic"]), ("ops", ["pad_tensors_wgrad"])):
        m = types.ModuleType(f"models.{sub}")
        for a in attrs:
            setattr(m, a, object)
        sys.modules[f"models.{sub}"] = m
        setattr(models, sub, m)
    sys.modules["models"] = models
    import utils.kd_loss as K
    K.dkd_loss = None
    from r2r.agent import GMapNavAgent
    return K, GMapNavAgent


def mint_prim(K):
    g = torch.Generator().manual_seed(41)
    neg = float("-inf")
    B = 4
    s2, t2 = 2 * torch.randn(B, 600, generator=g), 2 * torch.randn(B, 600, generator=g)
    for b in range(B):                                    # -inf at the same classes on both sides (masked logits)
        s2[b, 599 - b] = t2[b, 599 - b] = neg
        s2[b, 17 * b] = t2[b, 17 * b] = neg
    s3, t3 = 2 * torch.randn(B, 7, 16, generator=g), 2 * torch.randn(B, 7, 16, generator=g)
    s3[1, 6, 15] = t3[1, 6, 15] = neg
    s3[3, 0, 0] = t3[3, 0, 0] = neg
    s4, t4 = 2 * torch.randn(B, 3, 5, 6, generator=g), 2 * torch.randn(B, 3, 5, 6, generator=g)
    t4[0, 2, 4, 5] = neg                                  # teacher side only: p_t = 0 there, the term adds nothing
    t4[2, 1, 0, 3] = neg
    w = torch.rand(B, generator=g) + 0.25
    inputs = {"d2": (s2, t2), "d3": (s3, t3), "d4": (s4, t4)}
    cases = {}
    for name, (s, t) in inputs.items():
        for T in (1, 2):
            for lt in ("sum", "mean"):
                cases[f"{name}_T{T}_{lt}"] = float(K.kd_loss(s.double(), t.double(), temperature=T, loss_type=lt))
                cases[f"{name}_T{T}_{lt}_w"] = float(K.kd_loss(s.double(), t.double(), temperature=T, t_sample_weights=w.double(), loss_type=lt))
    return dict(inputs=inputs, w=w, cases=cases)


def mint_agent(K, GMapNavAgent):
    fx = torch.load(os.path.join(HERE, "makd_agent.pt"), weights_only=False)
    dbl = lambda o: defaultdict(lambda: None, {k: ({kk: vv.double() for kk, vv in v.items()} if isinstance(v, dict)
                                                   else (v.double() if torch.is_tensor(v) and v.is_floating_point() else v)) for k, v in o.items()})
    s_out, t_out = dbl(fx["s_out"]), dbl(fx["t_out"])
    heads = {}
    for n, (wt, b) in fx["heads"].items():
        h = nn.Linear(wt.shape[1], wt.shape[0]).double()
        h.weight.data.copy_(wt)
        h.bias.data.copy_(b)
        heads[n] = h
    student_inner, teacher_inner = SimpleNamespace(**heads), SimpleNamespace()
    rw, nav_targets = fx["rw"].double(), fx["nav_targets"]
    fn = {"mse": K.mse_loss, "kl": K.kd_loss}
    cases = {}

    def run(t, role, mode, lt, feat, attn):
        args = SimpleNamespace(kd_loss_type=lt, kd_ability_types=["txt", "img", "global", "local", "action"],
                               train_kdl_noFeat=False, train_kdl_noAttn=False, train_kdl_noLogit=False,
                               kdl_temperature=2.0, kdl_adaptive_ability_weight=mode is not None,
                               kdl_adaptive_ability_weight_type=mode, kdl_logit_loss="kd",
                               kdl_dkd_alpha=1.0, kdl_dkd_beta=1.0, ignoreid=-100)
        me = SimpleNamespace(args=args, vln_bert=SimpleNamespace(vln_bert=student_inner),
                             teacher_vln_bert=SimpleNamespace(vln_bert=teacher_inner),
                             kdl_feat_loss=fn[feat], kdl_attn_loss=fn[attn], kdl_logit_loss=K.kd_loss)
        acc = defaultdict(float)
        with torch.no_grad():
            if role == "t2s":
                res = GMapNavAgent.compute_kd_losses(me, t, s_out, t_out, acc, nav_targets, role="t2s", softmax_weights=rw)
            else:
                res = GMapNavAgent.compute_kd_losses(me, t, t_out, s_out, acc, nav_targets, role="s2t", softmax_weights=rw)
        return {k: float(v) for k, v in res.items()}

    for feat, attn in (("kl", "mse"), ("mse", "kl"), ("kl", "kl")):
        for role, lt in (("t2s", "sum"), ("t2s", "mean"), ("s2t", "mean")):
            for t in (0, 1):
                for mode in ("RW", None):
                    cases[f"{feat}-{attn}_{role}_{lt}_t{t}_{mode}"] = run(t, role, mode, lt, feat, attn)
    return dict(inputs="makd_agent.pt", temperature=2.0, cases=cases)


if __name__ == "__main__":
    import tempfile
    os.chdir(tempfile.mkdtemp(prefix="mint_makd_kl_"))
    K, Agent = _import_reference()
    out = dict(prim=mint_prim(K), agent=mint_agent(K, Agent))
    torch.save(out, os.path.join(HERE, "makd_kl.pt"))
    print("makd_kl:", len(out["prim"]["cases"]), "primitive cases,", len(out["agent"]["cases"]), "agent cases")
    for k in ("d3_T2_mean_w", "d2_T1_sum"):
        print(" ", k, out["prim"]["cases"][k])
    k = "kl-kl_t2s_sum_t0_RW"
    print(" ", k, out["agent"]["cases"][k])
