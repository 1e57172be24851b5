#!/usr/bin/env python3
"""trainer.FlatOptimizer.step(max_norm=40) per rule on the MAGIC-L navigator store (H = 768, bf16, as bench_nav.py builds it) against
clip_grad_norm_ + torch.optim.<same rule>.step() over the same model's parameter list (+ the re-cast of the 16-bit shadows a foreign optimizer's
step makes necessary, timed separately), and for adamW against trainer.FlatTorchAdamW.  Same process, arms alternating, `--rounds` windows of
`--iters` steps each, every window ended by a device synchronise; prints one JSON line (per arm: the median window's ms per step and the spread
over the windows) and the bytes each of the two launches has to move, for the achieved bytes/s of a kernel trace:

    python profiles/micro/flatopt_step_bench.py --out profile_out/flatopt_step_bench.json
    rocprofv3 --kernel-trace --stats -d profile_out/flatopt_trace -- python profiles/micro/flatopt_step_bench.py --arms flat --rounds 1 --iters 20
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import magic_amd  # noqa: E402,F401
from magic_amd.host import lib as L  # noqa: E402
from magic_amd.host.config import make_config  # noqa: E402
from magic_amd.host.model_nav import VLNBert  # noqa: E402
from magic_amd.host.trainer import FlatTorchAdamW, flat_optimizer  # noqa: E402

TORCH = {"sgd": torch.optim.SGD, "rms": torch.optim.RMSprop, "adam": torch.optim.Adam, "adamW": torch.optim.AdamW}
# fp32 words per element the update launch reads + writes (p, g, state in and out, the zeroed g) and the 2 bytes of the shadow; the norm launch reads g
UPDATE_BYTES = {"sgd": 4 * (2 + 2) + 2, "rms": 4 * (3 + 3) + 2, "adam": 4 * (4 + 4) + 2, "adamW": 4 * (4 + 4) + 2}


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rules", default="sgd,rms,adam,adamW")
    ap.add_argument("--arms", default="flat,torch,flat_torch_adamw")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L.load()
    cfg = make_config(a.hidden, role="teacher", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    model = VLNBert(None, role="student", config=cfg, device=dev, compute_dtype=torch.bfloat16, seed=0)
    st = model.store
    st.sync_shadow(force=True)
    params = list(model.parameters())
    arms_on = a.arms.split(",")
    res = {"elements": st.total, "tensors": len(params), "hidden": a.hidden, "dtype": "bf16", "iters": a.iters, "rounds": a.rounds,
           "norm_launch_bytes": 4 * st.total, "rules": {}}
    for rule in a.rules.split(","):
        flat = flat_optimizer(rule, st, 1e-5)
        topt = TORCH[rule](params, lr=1e-5)

        def torch_step():
            torch.nn.utils.clip_grad_norm_(params, 40.0)
            topt.step()

        def torch_step_and_recast():
            torch_step()
            st.sync_shadow(force=True)
        arms = {"flat": lambda: flat.step(max_norm=40.0), "torch": torch_step, "torch+recast": torch_step_and_recast}
        if rule == "adamW":
            fta = FlatTorchAdamW(st, lr=1e-5)
            arms["flat_torch_adamw"] = lambda: fta.step(max_norm=40.0)
        arms = {k: f for k, f in arms.items() if k.split("+")[0] in arms_on}
        times = {k: [] for k in arms}
        for f in arms.values():
            st.grad.normal_().mul_(1e-3)
            for _ in range(a.warmup):
                f()
        for _ in range(a.rounds):
            for k, f in arms.items():                      # alternating: every arm once per round
                st.grad.normal_().mul_(1e-3)
                times[k].append(window(f, a.iters))
        out = {"update_launch_bytes": UPDATE_BYTES[rule] * st.total}
        for k, ts in times.items():
            ts = sorted(ts)
            out[k] = {"ms_per_step_median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4)}
        res["rules"][rule] = out
        assert torch.isfinite(st.flat).all(), "the timed steps left the weights finite"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
