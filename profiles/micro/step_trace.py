"""Launch trace and tensor hashes of the pretraining step, for checking that a host-side change left the step as it was.

  python profiles/micro/step_trace.py --out DIR           one run: DIR/trace.json (launches + hashes), DIR/tensors.pt (the hashed tensors)
  python profiles/micro/step_trace.py --compare A B [...] [--changed C ...]
        A, B, ...: runs of one tree -> the tensors that differ between runs of that tree (fp32 atomics), each with its largest |diff| from A
        C, ...: runs of the changed tree -> their traces must equal A's, their tensors may differ from A's only inside that set and by no
        more than the runs of the one tree do.  Exit status 1 otherwise.

On the small models of tests/test_model_gpu.py (H 128 / 256, batch 6), through the public surface only (model(...), model.backward(),
trainer.teacher_forward, lib.PROFILE), so the same file runs on any commit.  Per task (sap, mlm, cfp, mrc):
  hashes   one training step of freshly built models against the teacher's outputs: every loss term, forward output and parameter gradient;
  trace    the (entry point, leading integer arguments) of every launch of: a training step with and without teacher outputs,
           compute_loss=False, metrics=<block> (with and without the fused mlm rows), the teacher's heads=False forward, and the training step
           again under each fallback switch.  A grouped launch is logged once, without arguments.
And one navigator training step on the small model of tests/test_nav_gpu.py."""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

TASKS = ("sap", "mlm", "cfp", "mrc")


def logged(fn):
    """fn() with every launch of the C ABI logged (as tests/test_kd_path_gpu.logged)"""
    from magic_amd.host import lib as L
    L.PROFILE.update(on=True, events=[], shapes=[])
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.PROFILE["on"] = False
    names, shapes = [e[0] for e in L.PROFILE["events"]], [list(s) for s in L.PROFILE["shapes"]]
    L.PROFILE.update(events=[], shapes=None)
    return out, [names, shapes]


def raw(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def flat(prefix, v, into):
    if torch.is_tensor(v):
        into[prefix] = v.detach().clone()
    elif isinstance(v, dict):
        for k, x in v.items():
            if k not in ("plan", "inputs"):
                flat(f"{prefix}.{k}", x, into)
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            flat(f"{prefix}.{i}", x, into)


def run(out_dir):
    import magic_amd  # noqa: F401
    import magic_amd.host.model_pretrain as MP
    from magic_amd.host import ops as O
    from magic_amd.host import synth
    from magic_amd.host.plan import build_plan
    from magic_amd.host.trainer import PretrainStep
    from tests.test_model_gpu import RW, build
    dev = torch.device("cuda", 0)
    trace, tensors = {}, {}

    def models(dtype):
        _, _, g_t, g_s = build(dtype, pretrain_tasks={"mlm", "mrc", "sap", "cfp"})
        g_s.keep_mlm_logits = False
        return g_t, g_s, PretrainStep(g_s, g_t, lr=5e-5, warmup_steps=2, num_train_steps=40)

    def step(g_s, bd, task, plan, t_out):
        g_s.store.zero_grad()
        out = g_s(bd, task, compute_loss=True, teacher_outputs=t_out, rw=RW, plan=plan, inputs=t_out["inputs"] if t_out else None)
        g_s.backward()
        return out

    for task in TASKS:
        b = synth.make_batch(task, batch_size=6, seed=21, vocab=600, min_len=8, max_len=19, min_steps=2, max_steps=4)
        bd, plan = synth.batch_to(b, dev), build_plan(b, task, dev)
        g_t, g_s, tr = models(torch.bfloat16)
        t_out = tr.teacher_forward(bd, task, plan)
        tr_ = trace[task] = {}
        out, tr_["train_kd"] = logged(lambda: step(g_s, bd, task, plan, t_out))
        flat(f"{task}.out", {k: v for k, v in out.items()}, tensors)
        for name, p in g_s.named_parameters():
            tensors[f"{task}.grad.{name}"] = p.grad.detach().clone()
        _, tr_["train"] = logged(lambda: step(g_s, bd, task, plan, None))
        with torch.no_grad():
            res, tr_["no_loss"] = logged(lambda: g_s(bd, task, compute_loss=False, plan=plan))
            flat(f"{task}.no_loss", res, tensors)
            block = O.eval_block(dev)
            _, tr_["metrics"] = logged(lambda: g_s(bd, task, compute_loss=False, plan=plan, metrics=block))
            tensors[f"{task}.metrics"] = block.clone()
            fused, O.EVAL_FUSED = O.EVAL_FUSED, False
            _, tr_["metrics_rows"] = logged(lambda: g_s(bd, task, compute_loss=False, plan=plan, metrics=O.eval_block(dev)))
            O.EVAL_FUSED = fused
            res, tr_["teacher_no_heads"] = logged(lambda: g_t(bd, task, compute_loss=False, return_outputs=True, plan=plan, heads=False))
            flat(f"{task}.teacher_no_heads", res, tensors)
        for mod, attr, val in ((O, "SAP_LOSS_FUSED", False), (O, "KD_FUSED", False), (MP, "MLM_TAIL_FUSED", False), (MP, "MLM_DX_ATOMICS", True),
                               (g_s, "keep_mlm_logits", True), (g_s.config, "glocal_fuse", False)):
            old = getattr(mod, attr, None)
            setattr(mod, attr, val)
            try:
                _, tr_[f"train_kd[{attr}={val}]"] = logged(lambda: step(g_s, bd, task, plan, t_out))
            finally:
                setattr(mod, attr, old)
        g_t, g_s, tr = models(torch.float32)
        t_out = tr.teacher_forward(bd, task, plan)
        _, tr_["train_kd[fp32]"] = logged(lambda: step(g_s, bd, task, plan, t_out))

    # one navigator training step
    from magic_amd.host.config import make_config
    from magic_amd.host.model_nav import VLNBert
    from tests.test_nav_gpu import nav_inputs, one_step, to_dev
    torch.manual_seed(0)
    cfg = make_config(128, role="student", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, vocab_size=300, num_l_layers=2,
                      num_x_layers=1, num_pano_layers=1)
    nav = VLNBert(None, role="student", config=cfg, device="cuda", compute_dtype=torch.bfloat16)
    inp = to_dev(nav_inputs(), "cuda")

    def nav_step():
        nav.store.zero_grad()
        r = one_step(nav, inp)
        r["loss"].backward()
        return r
    trace["nav"] = {}
    r, trace["nav"]["train"] = logged(nav_step)
    flat("nav.out", dict(loss=r["loss"], ce=r["ce"], nav=dict(r["out"]["nav_outs"])), tensors)
    for name, p in nav.named_parameters():
        if p.grad is not None:
            tensors[f"nav.grad.{name}"] = p.grad.detach().clone()

    torch.cuda.synchronize()
    tensors = {k: v.cpu() for k, v in tensors.items()}
    hashes = {k: hashlib.sha1(raw(v).numpy().tobytes()).hexdigest() for k, v in tensors.items()}
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "trace.json"), "w") as f:
        json.dump(dict(trace=trace, hashes=hashes), f, indent=0, sort_keys=True)
    torch.save(tensors, os.path.join(out_dir, "tensors.pt"))
    print(f"{sum(len(v[0]) for t in trace.values() for v in t.values())} launches in {sum(len(t) for t in trace.values())} traces, {len(hashes)} tensors -> {out_dir}")


def compare(same, changed):
    load = lambda d: (json.load(open(os.path.join(d, "trace.json")))["trace"], torch.load(os.path.join(d, "tensors.pt")))
    (ja, ta), others = load(same[0]), [load(d) for d in same[1:]]

    def diffs(x, y):
        assert set(x) == set(y), sorted(set(x) ^ set(y))
        return {k: (x[k].double() - y[k].double()).abs().max().item() for k in x if not torch.equal(raw(x[k]), raw(y[k]))}
    ok = all(j == ja for j, _ in others)
    print(f"{len(same)} runs of one tree: traces {'identical' if ok else 'DIFFER'}")
    noise = {}
    for _, t in others:
        for k, v in diffs(ta, t).items():
            noise[k] = max(v, noise.get(k, 0.0))
    print(f"{len(noise)} of {len(ta)} tensors differ between runs of one tree (largest |diff| from the first run):")
    for k, v in sorted(noise.items()):
        print(f"    {k}  {v:.3e}")
    for d in changed:
        jc, tc = load(d)
        for task in sorted(set(ja) | set(jc)):
            for form in sorted(set(ja.get(task, {})) | set(jc.get(task, {}))):
                if ja.get(task, {}).get(form) != jc.get(task, {}).get(form):
                    ok = False
                    print(f"TRACE DIFFERS: {task} {form}")
        moved = diffs(ta, tc)
        print(f"{d}: {sum(len(t) for t in ja.values())} traces compared; {len(moved)} of {len(ta)} tensors differ from the first run")
        for k, v in sorted(moved.items()):
            inside = k in noise and v <= noise[k]
            ok = ok and inside
            print(f"    {k}  {v:.3e}  " + (f"(one tree: {noise[k]:.3e})" if k in noise else "BITWISE EQUAL IN EVERY RUN OF ONE TREE") + ("" if inside else "  <-- outside"))
    print("OK" if ok else "NOT OK")
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs="+", help="two or more runs of one tree")
    ap.add_argument("--changed", nargs="*", default=[], help="runs of the changed tree")
    a = ap.parse_args()
    sys.exit(compare(a.compare, a.changed) if a.compare else run(a.out))
