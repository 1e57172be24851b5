"""The embedding-distillation terms at the headline sap batch's five problems (3 840 / 10 116 / 281 / 1 296 / 1 776 rows, 128 -> 256, bf16): the
three-launch sequence (grouped projection GEMM -> mse_multi -> grouped input-gradient GEMM) against the one fused launch (magic_kd_emb), HIP events
around each form, the two forms interleaved in one process.

    python profiles/micro/kd_emb_probe.py [rounds=12] [launches per round=20] > profiles/micro/kd_emb_probe.txt

Bytes moved (algorithmic): the sequence reads s and W, writes sp, reads sp and t, writes ds, reads ds, W and d_acc, writes d_acc; the fused launch reads s, t and
d_acc, writes ds and d_acc, and reads W once per workgroup."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import magic_amd  # noqa: E402,F401
from magic_amd.host import lib as L  # noqa: E402
from magic_amd.host import ops as O  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 12
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
ROWS = ((3840, 48), (10116, 281), (281, 281), (1296, 48), (1776, 48))            # (M, outer)
HS, HT, DT = 128, 256, torch.bfloat16
HBM_PEAK = 8.0e12

dev = "cuda"
probs = []
slots = torch.zeros(16, dtype=torch.float32, device=dev)
for i, (M, outer) in enumerate(ROWS):
    p = dict(M=M, outer=outer, inner=(M // outer) * HT)
    p["s"] = torch.randn(M, HS, device=dev).to(DT)
    p["t"] = torch.randn(M, HT, device=dev).to(DT)
    p["W"] = (0.1 * torch.randn(HT, HS, device=dev)).to(DT)
    p["b"] = 0.1 * torch.randn(HT, device=dev)
    p["ds"] = torch.empty(M, HT, device=dev, dtype=DT)
    p["d_acc"] = torch.zeros(M, HS, device=dev, dtype=DT)
    p["w"] = torch.rand(outer, device=dev) if outer == 48 else None
    p["sp"] = torch.empty(M, HT, device=dev, dtype=DT)
    probs.append(p)


def q_of(p, i, s):
    return dict(s=s, t=p["t"], outer=p["outer"], inner=p["inner"], s_stride=p["inner"], t_stride=p["inner"], w=p["w"], rows_per_w=1,
                norm=1.0 / (p["M"] * HT), coef=1.0, loss=slots[i:i + 1], ds=p["ds"], g_stride=p["inner"])


def sequence():
    with L.group():
        for p in probs:
            O.linear_fwd(p["s"], p["W"], p["b"], p["M"], out=p["sp"])
    O.mse_multi([q_of(p, i, p["sp"]) for i, p in enumerate(probs)])
    with L.group():
        for p in probs:
            O.linear_dx(p["ds"], p["W"], p["M"], out=p["d_acc"], residual=p["d_acc"])


def fused():
    O.kd_emb([dict(q_of(p, i, p["s"]), M=p["M"], W=p["W"], b=p["b"], d_acc=p["d_acc"]) for i, p in enumerate(probs)])


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS


for _ in range(3):
    sequence(); fused()
torch.cuda.synchronize()
ts, tf = [], []
for r in range(ROUNDS):
    ts.append(timed(sequence))
    tf.append(timed(fused))
rows = sum(m for m, _ in ROWS)
b_seq = rows * 2 * (HS + HT + HT + HT + HT + HT + HS + HS) + 2 * len(ROWS) * HT * HS * 2
b_fus = rows * 2 * (HS + HT + HT + HS + HS)
print(f"rows {[m for m, _ in ROWS]} = {rows}, {HS} -> {HT}, bf16; {ROUNDS} rounds x {REPS} back-to-back launches per form, interleaved; us per call")
print("round  sequence  fused")
for r in range(ROUNDS):
    print(f"{r:5d}  {ts[r]:8.2f}  {tf[r]:5.2f}")
for name, v, b in (("sequence (3 launches)", ts, b_seq), ("fused (1 launch)", tf, b_fus)):
    med, mn = statistics.median(v), min(v)
    print(f"{name:22s} median {med:6.2f} us  min {mn:6.2f} us   {b / 1e6:5.1f} MB moved: {b / med / 1e6:5.2f} TB/s at the median = {100 * b / med / 1e-6 / HBM_PEAK:4.1f} % of "
          f"{HBM_PEAK / 1e12:.0f} TB/s HBM peak")
print(f"difference of medians {statistics.median(ts) - statistics.median(tf):.2f} us per call")
