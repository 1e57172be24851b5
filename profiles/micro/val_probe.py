"""What a validation pass costs, three ways, over the same synthetic validation set (70 R2R-shaped batches of 48 per task from synth.make_batch, the
generator bench.py uses; tasks mlm / sap / cfp; the true MAGIC-S configuration; bf16):

  A  what the parent commit can do: the driver's validate_* arithmetic (pretrain_src/train_r2r_magic.py:441-587) in torch on
     model(batch, task, compute_loss=False), 3-7 .item() reads per batch
  B  Validator(graphs=False): the same eager forward, rows and sums on the device, one 96-byte read per task
  C  Validator(graphs=True): bucket-padded packed records (loader.pack_bucketed), one captured forward + metric graph per (task, layout)

All arms read index-only batches against one feature table in HBM (bench.py's streamed ingest).  A and B run on device-resident batches with their
plans built ahead (bench.py's resident pool); C gets the packed, pinned host records a DataLoader worker would hand over and pays its H2D copy per batch.  After one warm-up pass per arm (C's captures are in it) the arms alternate A, B, C for three
rounds, synchronising around each pass.  Writes per-task pass times, each arm's own spread (max - min over its rounds) and the share of a 1000-step
training interval a full validation (val-seen + val-unseen = 2 x this set) takes at the headline ms/step of profiles/kd_emb_bench.json.

    python profiles/micro/val_probe.py [--batches 70] [--batch 48] [--rounds 3] [--out profiles/val_pass.json]
    rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/micro/val_probe.py --batches 10 --rounds 1 --arms AB --tasks mlm --out /dev/null
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import magic_amd  # noqa: E402,F401
import bench  # noqa: E402
from magic_amd.host import synth  # noqa: E402
from magic_amd.host.loader import pack_bucketed  # noqa: E402
from magic_amd.host.validate import Validator, val_log  # noqa: E402


def driver_pass(model, task, pool, temperature):
    """arm A: the driver's loops, one host read per figure and batch"""
    loss, hits, n = [0.0] * 3, [0] * 3, 0
    for batch, plan in pool:
        if task == "mlm":
            scores = model(batch, task="mlm", compute_loss=False, plan=plan)["predict"]
            lab = batch["txt_labels"]
            lab = lab[lab != -1]
            loss[0] += F.cross_entropy(scores, lab, reduction="sum").item()
            hits[0] += (scores.max(dim=-1)[1] == lab).sum().item()
            n += lab.numel()
        elif task == "sap":
            o = model(batch, task="sap", compute_loss=False, plan=plan)
            ga, la = o["global_act_labels"].long(), o["local_act_labels"].long()
            for i, (x, lab) in enumerate(((o["global_logits"], ga), (o["local_logits"], la), (o["fused_logits"], ga))):
                loss[i] += F.cross_entropy(x, lab, reduction="sum").item()
                hits[i] += torch.sum(torch.argmax(x, 1) == lab).item()
            n += len(ga)
        else:
            outs = model(batch, task="cfp", compute_loss=False, plan=plan)
            txt = outs[3]
            tgt = torch.arange(len(txt), device=txt.device)
            for i in range(3):
                sim = (outs[i] @ txt.T) / temperature
                loss[i] += ((F.cross_entropy(sim, tgt, reduction="sum") + F.cross_entropy(sim.T, tgt, reduction="sum")) / 2.0).item()
                hits[i] += torch.sum(torch.argmax(sim, 1) == tgt).item()
            n += len(tgt)
    return dict(loss=loss, hits=hits, rows=[n] * 3)


class _Resident:
    """arm B's loader: device-resident batches with their plans, as arm A gets them.  Drives Validator._forward directly: Validator.run takes loader
    items (host batches or packed records), not (device batch, plan) pairs; run()'s mode switch is done once in main() and the block is read here"""

    def __init__(self, v, task, pool, temperature):
        self.v, self.task, self.pool, self.t = v, task, pool, temperature

    def run(self):
        v = self.v
        v.block.zero_()
        for batch, plan in self.pool:
            v._forward(self.task, batch, plan, self.t)
        from magic_amd.host.validate import read_block
        return read_block(v.block)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=70)
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--arms", default="ABC")
    ap.add_argument("--tasks", default="mlm,sap,cfp")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "val_pass.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    tasks = a.tasks.split(",")
    _, scfg, _, model, _ = bench.build_models(torch.bfloat16, dev, 0.0, 1, a.batch)
    temp = float(scfg.cfp_temperature)
    model.eval()
    # index-only batches (bench.py's streamed mode): the view features sit once in HBM as a packed table, a batch carries a
    # table row and a view order per panorama -- the same ingest for all three arms
    import numpy as np
    from magic_amd.host.feature_table import FeatureTable
    from magic_amd.host.loader import pack, unpack
    from magic_amd.host.plan import build_plan_host
    n_vp = 4096
    ftab = FeatureTable([str(i) for i in range(n_vp)], torch.randn(n_vp, 36, 768, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).to(dev))
    pools, recs = {}, {}
    for task in tasks:
        pools[task], recs[task] = [], []
        for i in range(a.batches):
            b = synth.make_batch(task, batch_size=a.batch, seed=4321, step=i, img_dim=8)
            rng = np.random.default_rng([4321, i])
            Np, V = b.pop("traj_view_img_fts").shape[:2]
            order = np.full((Np, V), -1, np.int32)
            for p_, n_ in enumerate(b["traj_vp_view_lens"].tolist()):
                order[p_, :n_] = rng.permutation(36)[:n_] if n_ <= 36 else np.concatenate([rng.permutation(36), rng.integers(0, 36, n_ - 36)])
            b["traj_vp_row"] = torch.from_numpy(rng.integers(0, n_vp, Np).astype(np.int32))
            b["traj_view_order"] = torch.from_numpy(order)
            batch, plan = unpack(pack(b, build_plan_host(b, task)), dev)
            batch["view_table"] = ftab
            if task == "mlm":
                batch["txt_labels"] = b["txt_labels"].to(dev)
            pools[task].append((batch, plan))
            if "C" in a.arms:
                r = pack_bucketed(b, task)
                r["buf"] = r["buf"].pin_memory()
                recs[task].append(r)
    torch.cuda.synchronize()
    vb, vc = Validator(model, feature_table=ftab, graphs=False), Validator(model, feature_table=ftab, graphs=True, max_graphs=256)

    def arm(name, task):
        with torch.no_grad():
            if name == "A":
                return driver_pass(model, task, pools[task], temp)
            if name == "B":
                return _Resident(vb, task, pools[task], temp).run()
            return vc.run(task, recs[task], temp)[0]

    times = {n: {t: [] for t in tasks} for n in a.arms}
    result = {n: {} for n in a.arms}
    for name in a.arms:                                  # warm-up pass per arm (allocator, code objects, C's captures)
        for task in tasks:
            arm(name, task)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name in a.arms:
            for task in tasks:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                result[name][task] = arm(name, task)
                torch.cuda.synchronize()
                times[name][task].append(time.perf_counter() - t0)
    out = dict(batches=a.batches, batch=a.batch, rounds=a.rounds, dtype="bf16", captures=vc.captures if "C" in a.arms else 0, arms={})
    for name in a.arms:
        out["arms"][name] = {}
        for task in tasks:
            ts = times[name][task]
            r = result[name][task]
            out["arms"][name][task] = dict(pass_ms=[round(1e3 * t, 2) for t in ts], best_ms=round(1e3 * min(ts), 2), spread_ms=round(1e3 * (max(ts) - min(ts)), 2),
                                           ms_per_batch=round(1e3 * min(ts) / a.batches, 3),
                                           log={k: v for k, v in val_log(task, r, min(ts)).items() if not k.endswith("_per_s")})
    try:
        head = json.load(open(os.path.join(ROOT, "profiles", "kd_emb_bench.json")))["ms_per_step"]
    except (OSError, KeyError, ValueError):
        head = None
    if head:
        out["headline_ms_per_step"] = head
        for name in a.arms:
            full = 2 * sum(out["arms"][name][t]["best_ms"] for t in tasks)          # val-seen + val-unseen
            out["arms"][name]["validation_ms"] = round(full, 1)
            out["arms"][name]["share_of_1000_step_interval"] = round(full / (full + 1000 * head), 4)
    if "A" in a.arms:
        for name in a.arms:
            if name != "A":
                out["arms"][name]["no_slower_than_A"] = {t: out["arms"][name][t]["best_ms"] <= out["arms"]["A"][t]["best_ms"] + out["arms"]["A"][t]["spread_ms"] for t in tasks}
    print(json.dumps(out))
    if a.out != "/dev/null":
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
