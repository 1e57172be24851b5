#!/usr/bin/env python
"""bench.py -- MAGIC-S R2R pretraining step throughput (trajectory-steps/sec) on N MI355X of one node.

One "step" = one optimizer step of the MAKD pretraining hot path on one synthetic R2R-shaped batch per rank
(B=48 trajectories, 36 views x 768-d CLIP features per trajectory step, <=80 RoBERTa tokens):
frozen teacher (H=256) forward -> student (MAGIC-S, H=128) forward + supervised + MAKD losses -> explicit
backward -> [RCCL all-reduce of the flat gradient] -> grad clip + fused AdamW.  Tasks cycle mlm:sap:cfp = 1:1:1
(pretrain_src/config/r2r_magic_pretrain.json:49-58).  bf16 MFMA compute, fp32 master weights/optimizer.

Contract: `python bench.py --gpus N --steps K --warmup W` (N>1 under torch.distributed.run); rank 0 prints ONE
JSON line.  Such a plain run sets up, warms up, times the K steps and prints the line (`value`, `ms_per_step`, ...); `--full` adds
everything else the line can carry (the blocks below, the 150-step `steady` figure, the other arithmetic modes, the secondary
configurations), `--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy.
`roofline` (--full) = the Linear-layer contraction family (MFMA GEMM kernels + the teacher's chain kernel): algorithmic FLOPs / summed launch
durations measured with HIP events on the launch stream in a separate instrumented pass; `cpu_baseline` = the
CPU oracle (oracle/, a restatement -- the reference's model source is withheld) timed on the host cores.
"""
# Streams and hardware queues.  HIP deals a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and two streams on one queue run IN ORDER:
# every side stream of the step (the teacher's, the gradient exchange's, the rollout lanes') is therefore picked by lanes.beside, which measures that the
# candidate really runs beside the main stream (csrc/encoder.hip magic_stream_probe; the line's `streams` block).  Raising the number of queues instead
# was measured and rejected (round 5, same box, this script): GPU_MAX_HW_QUEUES=8 left the headline and the data-parallel structure where they are
# (1.461 / 1.753 ms against 1.463 / 1.733 with the default) but ran the fp16 twin at 2.79 ms instead of 1.48 and the navigator loop at 175-187 ms
# instead of 139.  The runtime default stays; a value the user exports is passed through untouched.
import argparse
import json
import os
import sys
import time


def _self_launch():
    """`python bench.py --gpus N` (N > 1) without an outer launcher: start one fresh rank process per GPU the way the reference's
    scripts do (`pretrain_src/run_r2r_magic.sh:8-10`: `torch.distributed.launch --nproc_per_node`), relay rank 0's JSON line and exit
    with the children's status.  Runs BEFORE torch is imported, so this parent never touches the GPU; the ranks are children
    (`subprocess`), never an exec of this process."""
    if "WORLD_SIZE" in os.environ or "RANK" in os.environ:
        return
    n = 1
    for i, tok in enumerate(sys.argv[1:], 1):
        if tok == "--gpus" and i + 1 < len(sys.argv):
            n = int(sys.argv[i + 1])
        elif tok.startswith("--gpus="):
            n = int(tok.split("=", 1)[1])
    if n <= 1:
        return
    import socket
    import subprocess
    with socket.socket() as s:              # a free rendezvous port on the loopback interface
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on this host driver (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "4")
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, bufsize=1)
    for line in proc.stdout:                # relay as it comes; rank 0's JSON line is the only stdout line that starts with '{'
        sys.stdout.write(line)
        sys.stdout.flush()
    sys.exit(proc.wait())


if __name__ == "__main__":
    _self_launch()

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import magic_amd  # noqa: E402,F401
from magic_amd.host import lib as L  # noqa: E402
from magic_amd.host import lanes as _lanes  # noqa: E402
from magic_amd.host import ops as O  # noqa: E402
from magic_amd.host import synth  # noqa: E402
from magic_amd.host.config import make_config  # noqa: E402
from magic_amd.host.model_pretrain import GlocalTextPathCMTPreTraining  # noqa: E402
from magic_amd.host.plan import build_plan  # noqa: E402
from magic_amd.host.trainer import PretrainStep  # noqa: E402

KDL = dict(knowledge_distillation=True, kd_alpha=0.5, kd_temperature=2, teacher_sample_hard_mining=True,
           t_sample_preprocess_exp_decay=0.7, rw_temp=4, train_teacher=False,
           kdl_tasks=["txt", "img", "local", "global", "predict"], kdl_task_types=["emb", "attn"])   # r2r_magic_pretrain.json:62-87
TASKS = ["mlm", "sap", "cfp"]
if os.environ.get("MAGIC_BENCH_TASK_ORDER"):      # (experiments: the same three proxy tasks cycled in another order, e.g. mlm,cfp,sap)
    TASKS = [t for t in os.environ["MAGIC_BENCH_TASK_ORDER"].split(",") if t in ("mlm", "sap", "cfp")] or TASKS
MAX_TOKENS = 80                # instruction tokens per sample (synth.make_batch draws U{20..80})
PEAK_BF16_TFLOPS = 2500.0      # MI355X dense bf16 MFMA peak (MI355X_MICROARCH.md)


def cpu_baseline(tcfg, scfg, batch_size, seconds_budget=30.0, warm=3, timed=10):
    """The oracle (kind 'port') on the host cores: same step (teacher fwd, student fwd+MAKD, backward, clip, AdamW)."""
    from oracle import model_ref as R
    from oracle import optim_ref
    from magic_amd.host.params import is_no_decay
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    ncores = max(1, min(16, avail))       # many-thread oversubscription of these small ops is pathological (measured)
    torch.set_num_threads(ncores)
    torch.manual_seed(0)
    teacher, student = R.RefPretrainModel(tcfg).eval(), R.RefPretrainModel(scfg).eval()
    pdrop = float(getattr(scfg, "hidden_dropout_prob", 0.0))
    teacher_fwd = teacher
    if pdrop > 0:       # same work as the GPU step: the student's dropout modules are live (the frozen teacher's are not)
        def student_fwd(*args, **kw):
            R.DROPOUT = lambda site, x: torch.nn.functional.dropout(x, pdrop)
            try:
                return student(*args, **kw)
            finally:
                R.DROPOUT = None
    else:
        student_fwd = student
    params = [p for p in student.parameters()]
    wds = [0.0 if is_no_decay(n) else 0.01 for n, _ in student.named_parameters()]
    state = optim_ref.adamw_init([p.data for p in params])
    rw = torch.ones(5)
    steps_done, traj, t_total = 0, 0, 0.0
    names = []
    seq = [TASKS[i % 3] for i in range(warm + timed)]    # >= 3 warm-up + >= 10 timed steps
    for i, task in enumerate(seq):
        batch = synth.make_batch(task, batch_size=batch_size, seed=4321, step=i)
        t0 = time.perf_counter()
        with torch.no_grad():
            t_out = teacher_fwd(batch, task)["outputs"]
        for p in params:
            p.grad = None
        out = student_fwd(batch, task, teacher_outputs=t_out, rw=rw)
        out["loss"].backward()
        grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in params]
        optim_ref.clip_grad_norm(grads, 5.0)
        with torch.no_grad():
            optim_ref.adamw_step([p.data for p in params], grads, state, lr=5e-5, betas=(0.9, 0.98), eps=1e-6, weight_decay=wds)
        dt = time.perf_counter() - t0
        if i >= warm:
            steps_done += 1
            traj += sum(batch["traj_step_lens"])
            t_total += dt
            names.append(task)
        if t_total > seconds_budget:
            break
    return {"value": round(traj / t_total, 2), "unit": "trajectory-steps/sec", "cores": ncores, "kind": "port",
            "cores_of_the_box": os.cpu_count(), "cores_this_process_may_use": avail,
            "why_not_all_cores": "torch CPU ops of this size (H=128, <= 10 k rows) scale negatively past ~16 threads: re-measured in round 4 on the GPU box's 256-core host "
                                 "(profiles/micro/r04_cpu_threads_scan.txt: 4 / 8 / 16 / 32 / 64 / 128 threads = 239 / 399 / 497 / 271 / 134 / 47 trajectory-steps/s)",
            "sample": f"{warm} warm-up + {steps_done} timed optimizer steps (mlm:sap:cfp cycled) of the same B={batch_size} MAGIC-S+teacher workload, "
                      f"fp32 torch CPU oracle, dropout {pdrop}, {t_total / max(steps_done, 1) * 1e3:.0f} ms/step"}


class _StreamSet(torch.utils.data.IterableDataset):
    """synthetic stand-in for the reference's per-task datasets: every worker owns a few pre-generated sample lists (the
    generation of 30 MB of random features is not part of what is measured) and, per batch, runs the collate
    (`synth.collate`, pinned to tasks.py's) and the host half of the index plan -- the per-batch CPU work of a real loader."""

    def __init__(self, batch_size, seed, n_steps, pool=3, n_vp=0, bucketed=False, epoch=0):
        """epoch > 0: the stream repeats every `epoch` batches (a multiple of the worker count, so that a batch and its repeat come from the same worker's
        samples) -- a dataset walked for several epochs, as the reference trains; 0: every batch is a fresh draw"""
        self.batch_size, self.seed, self.n_steps, self.pool, self.n_vp, self.bucketed, self.epoch = batch_size, seed, n_steps, pool, n_vp, bucketed, int(epoch)

    def __iter__(self):
        import random

        import numpy as np

        from magic_amd.host.loader import pack, pack_bucketed
        from magic_amd.host.plan import build_plan_host
        info = torch.utils.data.get_worker_info()
        wid, nw = (info.id, info.num_workers) if info is not None else (0, 1)
        torch.set_num_threads(1)
        pools = []
        for j in range(self.pool):
            rng = np.random.default_rng([self.seed, wid, j])
            pyrng = random.Random(self.seed * 1000003 + wid * 101 + j)
            pools.append([synth.make_sample(rng, pyrng, vocab=50265, uid=i, **(dict(img_dim=8) if self.n_vp else {})) for i in range(self.batch_size)])
        if self.epoch and self.epoch % nw:
            raise ValueError(f"_StreamSet: epoch {self.epoch} is not a multiple of the {nw} workers")
        for step_ in range(wid, self.n_steps, nw):
            step = step_ % self.epoch if self.epoch else step_
            task = TASKS[step % 3]
            rng = np.random.default_rng([self.seed, step])
            if self.bucketed:     # ragged like a shuffled dataset: every batch is a fresh draw of samples, so sum T / K / the longest instruction vary
                flat = [x for pl in pools for x in pl]
                samples = [flat[i] for i in rng.choice(len(flat), self.batch_size, replace=False)]
            else:
                samples = pools[(step // nw) % self.pool]
            batch = synth.collate(samples, task, rng=rng, vocab=50265)
            if self.n_vp:       # index-only batch: table row + view order per panorama instead of the features
                Np, V = batch.pop("traj_view_img_fts").shape[:2]
                order = np.full((Np, V), -1, np.int32)
                for p_, n_ in enumerate(batch["traj_vp_view_lens"].tolist()):
                    order[p_, :n_] = rng.permutation(36)[:n_] if n_ <= 36 else np.concatenate([rng.permutation(36), rng.integers(0, 36, n_ - 36)])
                batch["traj_vp_row"] = torch.from_numpy(rng.integers(0, self.n_vp, Np).astype(np.int32))
                batch["traj_view_order"] = torch.from_numpy(order)
            yield task, (pack_bucketed(batch, task) if self.bucketed else pack(batch, build_plan_host(batch, task)))


def ingest_rate(dev, n_vp=4096, n_pano=290, reps=40):
    """SURVEY section 8d 'achieved feature-ingest GB/s': the f-2 path (packed bf16 view-feature table in HBM, index-only
    batches, `magic_view_gather` in the reference's candidate-first token order) timed on one B=48 batch worth of panoramas.
    Algorithmic bytes = read + write of 36 x 768 bf16 per trajectory step."""
    from magic_amd.host.feature_table import FeatureTable
    g = torch.Generator().manual_seed(0)
    table = torch.randn(n_vp, 36, 768, generator=g).to(torch.bfloat16).to(dev)
    ft = FeatureTable([str(i) for i in range(n_vp)], table)
    rows = torch.randint(0, n_vp, (n_pano,), generator=g).to(torch.int32).to(dev)
    order = torch.stack([torch.randperm(36, generator=g) for _ in range(n_pano)]).to(torch.int32).to(dev)
    out = torch.empty(n_pano, 36, 768, dtype=torch.bfloat16, device=dev)
    for _ in range(5):
        ft.gather(rows, order, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        ft.gather(rows, order, out=out)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / reps * 1e3
    nbytes = 2.0 * n_pano * 36 * 768 * 2
    return {"kernel": "view_gather_kernel<bf16>", "us_per_batch": round(us, 2), "GB_per_s": round(nbytes / us / 1e3, 1),
            "bytes_per_traj_step": 2 * 36 * 768 * 2, "peak_GB_per_s": 8000.0}


def pmc_traffic(gemm_n=1, chain_n=0):
    """HBM-side bytes per launch of the roofline family (GEMM kernels + chain kernel, weighted by this run's launch counts).  NOT measured
    inside this process (PMC collection needs rocprofv3 around it): read from the committed post-processing of the `rocprofv3 --pmc
    FETCH_SIZE` / `--pmc WRITE_SIZE` passes of this same command (profiles/pmc_traffic.py; FETCH_SIZE doubled as MI355X_MICROARCH.md
    prescribes for gfx950).  Returns (bytes, source file)."""
    for name in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json"):
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                j = json.load(f)
            g = j["gemm_traffic_bytes_per_launch"]
            c = j.get("chain_fetch_bytes_per_launch", 0.0) + j.get("chain_write_bytes_per_launch", 0.0)
            if c and chain_n:
                return round((g * gemm_n + c * chain_n) / (gemm_n + chain_n)), "profiles/" + name
            return round(g), "profiles/" + name
        except Exception:
            continue
    return None, None


def pmc_dw_fetch():
    """HBM bytes fetched per weight-gradient launch from the committed PMC pass (None if that file does not carry it)"""
    for name in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json"):
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                v = json.load(f).get("dw_batch_fetch_bytes_per_launch")
            if v:
                return round(v)
        except Exception:
            continue
    return None


def pmc_chain_traffic():
    """HBM bytes (fetched + written) per launch of the teacher's chain kernel from the committed PMC passes, or None"""
    for name in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json"):
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                j = json.load(f)
            return round(j["chain_fetch_bytes_per_launch"] + j["chain_write_bytes_per_launch"])
        except Exception:
            continue
    return None


def build_models(dtype, dev, dropout, world, batch=48):
    dk = dict(hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout)   # r2r_magic_model_config.json:2-3
    tcfg = make_config(256, role="teacher", **dk)                                   # teacher_* of r2r_magic_model_config.json:33-37
    scfg = make_config(128, role="student", teacher_hidden_size=256, kdl=KDL, **dk)  # MAGIC-S: student_* :39-43
    teacher = GlocalTextPathCMTPreTraining(tcfg, device=dev, compute_dtype=dtype, seed=0)
    student = GlocalTextPathCMTPreTraining(scfg, device=dev, compute_dtype=dtype, seed=1)
    # checkpoint-like small parameters (non-zero biases, LayerNorm gains off 1): the reference's loop never starts from a fresh module (it loads METER's
    # weights, train_r2r_magic.py:183-209), and with all-zero biases every Linear -> LayerNorm over a zero input row is LayerNorm(0) (rstd 1e6): rounds 1-5
    # timed steps whose global gradient norm was ~3e5 and whose clip factor was ~1.7e-5.  `health.grad_norm` / `health.clip_factor` / `steady.grad_norm_by_task` now show both.
    teacher.store.checkpoint_like_(100)
    student.store.checkpoint_like_(101)
    if world > 1:   # DDP ctor semantics: rank-0 parameters broadcast once (utils/misc.py:62-63)
        dist.broadcast(student.store.flat, src=0)
        dist.broadcast(teacher.store.flat, src=0)
    trainer = PretrainStep(student, teacher, lr=5e-5, betas=(0.9, 0.98), weight_decay=0.01, grad_norm=5.0,
                           warmup_steps=10000, num_train_steps=200000, rw_temp=4.0,
                           sparse_embedding_rows=batch * MAX_TOKENS,      # <= B x 80 distinct token ids per rank and step (north star: <= 80 tokens)
                           seed=1234 + (dist.get_rank() if world > 1 else 0))   # per-rank MKRW draws / dropout masks (train_r2r_magic.py:86-89)
    return tcfg, scfg, teacher, student, trainer


def capture_ring(trainer, pool, teacher_mode):
    """one HIP graph per resident batch (each batch has its own ragged shapes); every replay executes the full step: teacher fwd,
    student fwd + losses + bwd, clip, AdamW -- with lr / bias-correction / MKRW read from device memory"""
    if teacher_mode in ("ahead", "split"):
        # graph i: student step on batch i (teacher outputs t[i] are ready) || teacher forward on batch i+1 -> t[i+1];
        # t[0] is primed eagerly once, and the last graph of the ring copies its teacher(batch 0) outputs into it
        n = len(pool)
        trip = lambda i: (pool[i % n][1], pool[i % n][0], pool[i % n][2])           # (batch, task, plan)
        t0 = trainer.teacher_forward(*trip(0))
        t_cur, graphs = t0, []
        for i in range(n):
            cap = trainer.capture_ahead if teacher_mode == "ahead" else trainer.capture_split
            cs = cap(trip(i), t_cur, trip(i + 1), t_next_into=t0 if i == n - 1 else None)
            graphs.append(cs)
            t_cur = cs.t_next
        return graphs
    return [trainer.capture(b, task, plan) for task, b, plan in pool]


def timed_region(run, steps, warmup, world, dev):
    """W untimed steps, then exactly K steps between barrier + synchronize on both sides; max over ranks"""
    run(warmup)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    traj = run(steps, start=warmup)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
        tr = torch.tensor([traj], device=dev, dtype=torch.float64)
        dist.all_reduce(tr)
        traj = float(tr.item())
    return traj, dt


DUMP_SAMPLE = 1 << 20          # elements kept of a larger output array (--dump-outputs) ...
DUMP_BUDGET = 56 << 20         # ... halved for all arrays until their payloads fit this (64 MB with room for the .npy headers)
DUMP_SKIP = ("plan", "inputs")  # the step's own index plan and inputs, handed back beside its outputs: not computed by it


def dump_outputs(path, out, weights):
    """--dump-outputs: what the last timed step returned (loss terms, logits, embeddings; nested dicts / tuples flattened into dotted names,
    DUMP_SKIP keys left out) and the student's fp32 master weights after its update, one DIR/<name>.npy each.  float64 tensors as float64, other floating tensors as
    float32, integer and bool tensors as float64.  An array of more than `cap` elements keeps a fixed sample of `cap` of them: sorted flat
    indices drawn without replacement from a generator seeded by the array's name, so the same run arguments always pick the same elements."""
    import zlib

    import numpy as np
    arrays = []

    def walk(name, v):
        if torch.is_tensor(v):
            arrays.append((name, v.detach()))
        elif isinstance(v, dict):
            for k, x in v.items():
                if k not in DUMP_SKIP:
                    walk(f"{name}.{k}", x)
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(f"{name}.{i}", x)
        elif isinstance(v, (int, float, bool)):
            arrays.append((name, torch.tensor(float(v), dtype=torch.float64)))
    walk("out", out)
    arrays.append(("student_master_weights", weights))
    if weights.is_cuda:
        torch.cuda.synchronize()
    wide = lambda t: t.dtype == torch.float64 or not t.is_floating_point()
    cap = DUMP_SAMPLE
    while sum(min(t.numel(), cap) * (8 if wide(t) else 4) for _, t in arrays) > DUMP_BUDGET:
        cap //= 2
    os.makedirs(path, exist_ok=True)
    for name, t in arrays:
        t = t.reshape(-1) if t.dim() else t
        if t.numel() > cap:
            rng = np.random.default_rng(zlib.crc32(name.encode()))
            idx = np.sort(rng.choice(t.numel(), cap, replace=False))
            t = t[torch.from_numpy(idx).to(t.device)]
        x = t.cpu()
        np.save(os.path.join(path, name + ".npy"), (x.double() if wide(x) else x.float()).numpy())


def _gate(ms):
    """park the stream for ~ms milliseconds (a device-side spin) so the host can enqueue a whole instrumented step behind it: the
    event pairs then bracket kernels that run back to back, not the host's launch gaps"""
    if "_cyc_per_ms" not in _gate.__dict__:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); torch.cuda._sleep(20_000_000); e1.record()
        torch.cuda.synchronize()
        _gate._cyc_per_ms = 20_000_000 / max(e0.elapsed_time(e1), 1e-3)
    torch.cuda._sleep(int(ms * _gate._cyc_per_ms))


def instrumented_pass(trainer, pool, nprof, gate_ms):
    """Per-launch HIP events (recorded on the launch stream) over `nprof` eager steps with the SAME launch structure as the captured
    graphs (paired launches), the teacher's forward SERIALISED on the main stream (no overlap: summed kernel time == stream time),
    and a device-side gate in front of every step so the host runs ahead of the GPU.  Returns {family: (ms, launches)}."""
    import magic_amd.host.model_pretrain as MP
    O.FLOPS.update(total=0.0, gemm=0.0, linear_ln=0.0, attn=0.0, enc=0.0, chain=0.0, enabled=True)
    O.BYTES.update(dw=0.0, dw_launches=0)
    L.PROFILE.update(on=True, events=[])
    MP.LOCKSTEP_EAGER = True
    side, trainer.side = trainer.side, None
    try:
        for s in range(nprof):
            task, b, plan = pool[s % len(pool)]
            _gate(gate_ms)
            trainer.step(b, task, plan=plan)
        torch.cuda.synchronize()
    finally:
        trainer.side = side
        MP.LOCKSTEP_EAGER = False
        L.PROFILE["on"] = False
        O.FLOPS["enabled"] = False
    by = {}
    for name, layout, e0, e1 in L.PROFILE["events"]:
        k = name if layout < 0 else f"{name}[{['NT', 'NN', 'TN'][layout]}]"
        t, c = by.get(k, (0.0, 0))
        by[k] = (t + e0.elapsed_time(e1), c + 1)
    return by


def parity_block(dev):
    """CHECKER leg (the oracle is test infrastructure, like cpu_baseline): the benchmarked arithmetic modes against the fp64 oracle on
    full-size SAP batches (6/3/2 layers, vocab 50265, B=8 x 3 seeds) -- action-logit |delta| and argmax agreement, the quantities
    BASELINE.json states its tolerance on (|delta| < 1e-3, argmax exact)."""
    from oracle import parity_probe as PP
    models = PP.oracle_models()
    out = {"checker": "fp64 CPU oracle (oracle/model_ref.py, a restatement: the reference withholds its model source), same weights and batches",
           "north_star": {"max_abs_logit_delta": 1e-3, "argmax_agreement": 1.0}}
    for name, dt_ in (("bf16", torch.bfloat16), ("fp16", torch.float16), ("fp32", torch.float32), ("bf16x3", torch.float32)):
        prev = L.set_f32_mfma("bf16x3" if name == "bf16x3" else "exact")
        try:
            st = PP.sap_parity(dt_, batch_size=8, seeds=(1234, 77, 5), device=dev, models=models)
        finally:
            L.set_f32_mfma(prev)
        out[name] = {"max_abs_logit_delta": float(f"{st['max_abs_logit_delta']:.3e}"), "argmax_agreement": round(st["argmax_agreement"], 4),
                     "rows": st["rows"], "loss_rel_delta": float(f"{st['loss_rel_delta']:.2e}"),
                     "oracle_min_top2_gap": float(f"{st['oracle_min_top2_gap']:.2e}"),
                     "worst_oracle_gap_between_flipped_picks": float(f"{st['worst_flip_gap']:.2e}")}
    return out


class _stdout_to_stderr:
    """RCCL prints a version banner on stdout when its first communicator comes up; the contract is ONE JSON line on stdout.  File-descriptor
    level (the banner comes from C), restored on exit."""

    def __enter__(self):
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self._saved, 1)
        os.close(self._saved)
        return False


def rccl_smoke_leg(student, batch_size, dev):
    """N = 1 only: every collective the data-parallel exchange issues (trainer.GradSync: chunked fp32 all-reduce of the three gradient buckets,
    all_gather_into_tensor of int64 row ids + fp32 rows for the sparse word-embedding exchange) in a world-size-1 `nccl` (= RCCL) group on
    the exchange stream -- the RCCL code path is loaded and well-formed on this box; it says NOTHING about scaling (no multi-GPU node has
    run this build: "unmeasured on hardware")."""
    from magic_amd.host.trainer import GradSync
    import socket
    out = {"backend": "nccl (RCCL)", "world": 1, "multi_gpu": "unmeasured on hardware"}
    t0 = time.perf_counter()
    try:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        with _stdout_to_stderr():
            dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
            warm = torch.zeros(8, device=dev)
            dist.all_reduce(warm)                       # the communicator (and RCCL's banner) comes up with the first collective
            torch.cuda.synchronize()
        try:
            store = student.store
            store.ensure_grads()
            store.grad.normal_()
            ref = store.grad.clone()
            sync = GradSync(store, sparse_rows_cap=batch_size * MAX_TOKENS)
            sync.stream = torch.cuda.Stream()
            ids = torch.unique(torch.randint(0, 50265, (batch_size * MAX_TOKENS,), device=dev))
            from magic_amd.host import rccl as _rccl
            direct = _rccl.make(dev)            # round 6: the exchange's own communicator through RCCL's C ABI (host/rccl.py), self-tested
            out["direct_rccl_c_abi"] = direct is not None
            same = True
            for comm in ([None, direct] if direct is not None else [None]):      # torch.distributed's calls, then the direct ones GradSync uses by default
                sync.rccl = comm
                for i in range(3):
                    sync._on_side(lambda i=i: sync._ranges(sync.buckets[i]))
                sync._on_side(lambda: sync._sparse_rows(ids))
                sync.join()
                torch.cuda.synchronize()
                same = same and bool(torch.equal(store.grad, ref))
            out["identity_at_world_1"] = same
            if direct is not None:      # (an idle communicator keeps RCCL's proxy thread polling: it doubled the host-bound navigator legs that run after this one)
                sync.rccl = None
                direct.destroy()
            out["collectives"] = ["all_reduce fp32 x 3 buckets (chunked)", "all_gather_into_tensor int64 ids", "all_gather_into_tensor fp32 rows"]
            out["bucket_bytes"] = [int(sum(hi - lo for lo, hi in b) * 4) for b in sync.buckets]
            out["ok"] = out["identity_at_world_1"]
        finally:
            dist.destroy_process_group()
    except Exception as e:          # noqa: BLE001 - the headline line must still print
        out["ok"], out["error"] = False, repr(e)[:300]
    out["seconds"] = round(time.perf_counter() - t0, 2)
    return out


def secondary_block():
    """short driver-timed samples of BASELINE configs 3 and 5 (bench_nav.py as child processes: own CUDA context, started after this
    process's measurements are done)"""
    import subprocess
    py, nav = sys.executable, os.path.join(ROOT, "bench_nav.py")
    common = ["--steps", "10", "--warmup", "10", "--no-cpu-baseline", "--no-host-loop", "--no-profile"]      # (warm-up: the step instances are captured on first sight of a shape key)
    runs = {"config3_icod_magicL_teacher_magicS_student": ["--icod", "--hidden", "128", "--teacher-hidden", "768", "--instr-min", "20", "--instr-max", "80",
                                                          "--hops-min", "4", "--hops-max", "7", "--max-action-len", "15"],
            "config5_rxr_magicL_navigator_loop": []}
    out = {}
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    nav_env = dict(env)
    for name, extra in runs.items():
        try:
            r = subprocess.run([py, nav] + common + extra, capture_output=True, text=True, timeout=240, env=nav_env)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
            j = json.loads(line)
            out[name] = {"value": j["value"], "unit": j["unit"], "ms_per_iteration": j["ms_per_step"], "steps": j["steps"], "dtype": j["dtype"],
                         "mode": j["mode"], "workload": j["config"]["workload"], "per_gpu_batch": j["config"]["per_gpu_batch"], "warmup": j["warmup"],
                         "step_graphs": {k: {kk: vv for kk, vv in v.items() if kk != "by_key"} for k, v in (j.get("step_graphs") or {}).items()}}
        except Exception as e:          # noqa: BLE001 - the headline line must still print
            out[name] = {"error": repr(e)[:300]}
    # the data-parallel STRUCTURE on one GPU: the same step as three backward graphs + the optimizer's graph with the bucket collectives of a
    # world-1 `nccl` group issued between the replays on the exchange stream -- what the cuts and RCCL's launch latency cost, measurable without a node
    try:
        r = subprocess.run([py, os.path.join(ROOT, "bench.py"), "--dp-structure", "--warmup", "12", "--steps", "60", "--no-cpu-baseline", "--no-parity",
                            "--no-secondary", "--no-profile"], capture_output=True, text=True, timeout=300, env=env)
        j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        out["dp_structure_world1_rccl"] = {"ms_per_step": j["ms_per_step"], "value": j["value"], "unit": j["unit"], "steps": j["steps"],
                                           "rccl": j.get("dp_rccl"),
                                           "note": "round 6: ONE graph per step with the bucket collectives INSIDE it -- ncclAllReduce x 3 buckets (one group launch each) and the two "
                                                   "ncclAllGather of the sparse word-embedding rows (one group launch), issued through RCCL's C ABI (host/rccl.py) on the exchange "
                                                   "stream the capture forks to at every bucket boundary; world-1 communicator: identity -- the cost of the structure, not a scaling "
                                                   "number (N > 1: unmeasured on hardware).  Rounds 4-5: three graphs cut at the bucket boundaries + torch.distributed calls between the replays (1.73-1.75 ms)"}
    except Exception as e:              # noqa: BLE001
        out["dp_structure_world1_rccl"] = {"error": repr(e)[:300]}
    # SURVEY f-3: the same pretraining step fed from DataLoader workers (NON-resident batches, PCIe-inclusive; never `value`): batches padded to
    # shape buckets, one graph replay per step (host/stream_graph.py)
    try:
        r = subprocess.run([py, os.path.join(ROOT, "bench.py"), "--mode", "stream-graph", "--workers", "8", "--stream-epoch", "152", "--warmup", "304", "--steps", "150",
                            "--no-cpu-baseline", "--no-parity", "--no-secondary"], capture_output=True, text=True, timeout=300, env=env)
        j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        out["streamed_batches_graph_replay"] = {"value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"], "steps": j["steps"],
                                                "ms_per_step_without_in_window_captures": j.get("ms_per_step_steady"),
                                                "launch": j["launch"], "note": "collate + index plan in 8 DataLoader workers (the reference's n_workers, r2r_magic_pretrain.json:26), feature table in HBM, "
                                                "one H2D record copy + one graph launch per step; the timed steps are the THIRD pass over a 152-batch epoch (a dataset walked for several "
                                                "epochs, as the reference trains): every bucket graph they replay was captured during the first; the resident-batch headline is `value`"}
    except Exception as e:              # noqa: BLE001
        out["streamed_batches_graph_replay"] = {"error": repr(e)[:300]}
    # ... and the two together: what ONE RANK of a real data-parallel run executes every step -- streamed batches (DataLoader workers,
    # bucket graphs) AND the data-parallel structure (bucket graphs cut where the gradient buckets are final, the bucket collectives of a world-1 RCCL
    # communicator between the replays: the touched word-embedding rows change per batch, so these collectives stay outside the graphs)
    try:
        r = subprocess.run([py, os.path.join(ROOT, "bench.py"), "--mode", "stream-graph", "--dp-structure", "--workers", "8", "--stream-epoch", "152", "--warmup", "304", "--steps", "150",
                            "--no-cpu-baseline", "--no-parity", "--no-secondary"], capture_output=True, text=True, timeout=300, env=env)
        j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        out["rank_of_a_real_run"] = {"value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"], "steps": j["steps"],
                                     "ms_per_step_without_in_window_captures": j.get("ms_per_step_steady"), "launch": j["launch"],
                                     "note": "streamed batches (8 DataLoader workers, bucket graphs, feature table in HBM) + the data-parallel structure at world 1 over RCCL "
                                             "(identity): the per-rank step of an N-GPU run without the bytes on xGMI (N > 1: unmeasured on hardware)"}
    except Exception as e:              # noqa: BLE001
        out["rank_of_a_real_run"] = {"error": repr(e)[:300]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"],
                    help="bf16 = BASELINE config 2's arithmetic (the headline); fp16 = the same kernels on IEEE half storage (11 significand bits: meets the "
                         "north star's |delta logit| < 1e-3; gradient seeds scaled by 4096, folded back in the AdamW kernel); fp32 = exact fp32 MFMA")
    ap.add_argument("--pool", type=int, default=12, help="distinct pre-generated batches (cycled)")
    ap.add_argument("--dropout", type=float, default=0.1, help="hidden/attention dropout of the student (reference recipe: 0.1)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the oracle parity leg and the fp32-mode timing")
    ap.add_argument("--no-secondary", action="store_true", help="skip the short config-3 / config-5 samples (bench_nav.py children)")
    ap.add_argument("--mode", default="graph", choices=["graph", "eager", "stream", "stream-graph"],
                    help="graph: replay one captured HIP graph per resident batch (the headline line); eager: same batches, launches issued "
                         "one by one; stream: NON-resident batches -- collate + index plan built in DataLoader worker processes, pinned, "
                         "copied one batch ahead on a copy stream (host/loader.py), eager launches: the PCIe-inclusive rate; stream-graph: the same "
                         "feed, batches padded to shape buckets and every step ONE graph replay (host/stream_graph.py; the first batch of a bucket "
                         "pays its capture: use a warm-up that has seen the buckets, e.g. --warmup 150 --steps 150)")
    ap.add_argument("--stream-epoch", type=int, default=0,
                    help="--mode stream / stream-graph: the synthetic dataset repeats every N batches (a multiple of --workers); with --warmup >= N the timed "
                         "steps are a LATER epoch of the same batches -- every bucket graph they need was captured in the first (0: all batches distinct)")
    ap.add_argument("--workers", type=int, default=8, help="--mode stream: DataLoader worker processes (r2r_magic_pretrain.json:26 n_workers)")
    ap.add_argument("--ingest", default="table", choices=["table", "host"],
                    help="--mode stream: 'host' = the reference's way, every batch carries its fp32 view features (30 MB at B=48) from the "
                         "workers through pinned memory over PCIe; 'table' = SURVEY f-2, features live once in HBM (packed bf16 table) and a "
                         "batch carries 37 int32 per panorama, gathered on the device")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL over xGMI (the product path); gloo only to rehearse the N > 1 code path with several ranks on ONE card")
    ap.add_argument("--teacher", default="split", choices=["split", "ahead", "same"],
                    help="split (default): the frozen teacher's forward on batch i+1 is its own HIP graph on a side stream, replayed while the "
                         "student's graph trains on batch i (and, with data parallelism, while the gradient all-reduce and the optimizer run); "
                         "ahead: the same overlap as a fork/join inside ONE graph; same: teacher and student forward of the same batch side by "
                         "side (every step runs exactly one teacher forward and one student update in all three)")
    ap.add_argument("--dp-structure", action="store_true",
                    help="N = 1 only: time the data-parallel STRUCTURE of the step -- three backward graphs cut where gradient buckets 0 / 1 / 2 are final, "
                         "the bucket collectives issued on the exchange stream between the replays in a world-1 `nccl` (= RCCL) group (identity at world 1), "
                         "the optimizer's graph behind the exchange -- next to the single-graph step (run by a --full line as a child process: "
                         "`dp_structure`)")
    ap.add_argument("--rehearse-launch", action="store_true",
                    help="launcher rehearsal (no GPU needed): rendezvous, the rank roll-call and the one-line relay only, then exit -- what "
                         "tests/test_bench_launch_cpu.py runs on CPU with --backend gloo; the full 2-rank step runs in tests/test_bench_launch_gpu.py")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need (each still switched off by its --no-* flag): the 150-step steady figure and "
                         "the per-task loops, the teacher gate's counters, the instrumented roofline pass and the feature-ingest rate, the other "
                         "arithmetic modes and the oracle parity leg, the RCCL smoke leg, the CPU baseline and the secondary configurations.  "
                         "Without it a run sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the LAST timed step returned (its loss terms and outputs) and the student's fp32 master "
                         "weights after it as DIR/<name>.npy (float32; integer tensors as float64; an array of more than 1 M elements as a fixed, "
                         "seeded sample of 1 M of them; at most 64 MB in all)")
    a = ap.parse_args()
    if not a.full:            # a plain run: only what `value` / `ms_per_step` need
        a.no_cpu_baseline = a.no_profile = a.no_parity = a.no_secondary = True

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:       # only reachable under an outer launcher whose world disagrees with --gpus (a bare `python bench.py --gpus N` self-launches)
        raise SystemExit(f"bench.py --gpus {a.gpus} but WORLD_SIZE={world}: launch one rank per GPU (`python bench.py --gpus {a.gpus}` does it itself, or "
                         f"`python -m torch.distributed.run --nnodes=1 --nproc-per-node {a.gpus} --master-addr 127.0.0.1 bench.py --gpus {a.gpus} ...`)")
    if a.rehearse_launch:
        if world > 1:
            dist.init_process_group("gloo")
        mine = torch.tensor([rank, local], dtype=torch.int64)
        seen = [torch.zeros_like(mine) for _ in range(world)]
        if world > 1:
            dist.all_gather(seen, mine)
            dist.barrier()
        else:
            seen = [mine]
        if rank == 0:
            print(json.dumps({"rehearsal": "launch", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
                              "rccl": {"backend": "gloo", "world": world, "ranks_seen": [int(t[0]) for t in seen], "devices": [int(t[1]) for t in seen]}}))
        if world > 1:
            dist.destroy_process_group()
        return
    if a.backend == "gloo":
        local = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        with _stdout_to_stderr():
            if a.backend == "nccl":
                dist.init_process_group("nccl", device_id=dev)
            else:
                dist.init_process_group("gloo")
    if a.dp_structure:
        if world != 1:
            raise SystemExit("--dp-structure is the N = 1 measurement of the data-parallel structure")
        import socket
        os.environ["MAGIC_DP_STRUCTURE"] = "1"
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        with _stdout_to_stderr():
            dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
            warm = torch.zeros(8, device=dev)
            dist.all_reduce(warm)
            torch.cuda.synchronize()
    L.load()
    rccl = None
    if world > 1:             # every rank reports in through the data-path backend: the line shows N ranks on N devices really took part
        mine = torch.tensor([rank, local], device=dev, dtype=torch.int64)
        seen = [torch.zeros_like(mine) for _ in range(world)]
        with _stdout_to_stderr():           # (RCCL's version banner belongs on stderr: stdout carries the one JSON line)
            dist.all_gather(seen, mine)
            torch.cuda.synchronize()
        seen = [t.tolist() for t in seen]
        rccl = {"backend": a.backend, "world": world, "ranks_seen": [r for r, _ in seen], "devices": [d for _, d in seen]}
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    if os.environ.get("MAGIC_MAIN_PRIORITY"):      # experiment: the student's stream at high priority (-1), the teacher's at 0
        torch.cuda.set_stream(torch.cuda.Stream(dev, priority=int(os.environ["MAGIC_MAIN_PRIORITY"])))
    if os.environ.get("MAGIC_TEACHER_CUS"):
        # a CU-masked stream (hipExtStreamCreateWithCUMask) is a BLOCKING stream: it synchronises with the null stream implicitly, so the
        # student's work must not sit on the null stream or the two serialise
        torch.cuda.set_stream(torch.cuda.Stream(dev))
    tcfg, scfg, teacher, student, trainer = build_models(dtype, dev, a.dropout, world, a.batch)

    # synthetic batches, resident in HBM before the timed region (per-rank stream: seed 1234 + rank)
    pool = []
    for i in range(a.pool if a.mode not in ("stream", "stream-graph") else 3):
        task = TASKS[i % 3]
        b = synth.make_batch(task, batch_size=a.batch, seed=1234 + rank, step=i)
        plan = build_plan(b, task, dev)
        pool.append((task, synth.batch_to(b, dev), plan))
    torch.cuda.synchronize()

    last = {}                 # what the most recent step returned (--dump-outputs)

    def eager_runner(tr):
        def run_eager(n, start=0):
            traj = 0
            for s in range(n):
                task, b, plan = pool[(start + s) % len(pool)]
                last["out"] = tr.step(b, task, plan=plan)
                traj += plan["traj_steps"]
            return traj
        return run_eager

    def graph_runner(tr, graphs):
        def run_graph(n, start=0):
            traj = 0
            for s in range(n):
                cs = graphs[(start + s) % len(graphs)]
                last["out"] = (tr.replay_split if a.teacher == "split" else tr.replay)(cs)
                traj += cs.traj_steps
            return traj
        return run_graph

    run_eager = eager_runner(trainer)
    if a.mode in ("stream", "stream-graph"):
        a.no_profile = True
    if a.mode == "graph":
        run_eager(min(3, len(pool)))                       # allocator + code-object warm-up
        torch.cuda.synchronize()
        graphs = capture_ring(trainer, pool, a.teacher)
        torch.cuda.synchronize()
        run = graph_runner(trainer, graphs)
        run(len(graphs))                                   # one untimed pass over the ring: a graph's FIRST launch uploads it (with --warmup 5
        torch.cuda.synchronize()                           # seven of the twelve graphs would otherwise be launched first inside the timed steps)
    else:
        run = run_eager
    stream_step = None
    if a.mode in ("stream", "stream-graph"):
        from magic_amd.host.loader import DevicePrefetcher
        n_vp = 4096
        ds = _StreamSet(a.batch, 1234 + rank, a.warmup + a.steps + 2, n_vp=n_vp if a.ingest == "table" else 0, bucketed=a.mode == "stream-graph",
                        epoch=a.stream_epoch)
        ftab = None
        if a.ingest == "table":
            from magic_amd.host.feature_table import FeatureTable
            ftab = FeatureTable([str(i) for i in range(n_vp)],
                                torch.randn(n_vp, 36, 768, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).to(dev))
        dl = torch.utils.data.DataLoader(ds, batch_size=None, num_workers=a.workers, pin_memory=True, prefetch_factor=2, persistent_workers=False)
        if a.mode == "stream-graph":
            from magic_amd.host.stream_graph import StreamStep
            run_eager(3)                                       # allocator + code-object warm-up before the first capture
            torch.cuda.synchronize()
            stream_step = StreamStep(trainer, feature_table=ftab)
            if a.teacher == "same":                            # teacher forward inside the step's graph (one record slot per bucket)
                feed = iter(dl)
                steps_gen = (stream_step.step(task, rec) for task, rec in feed)
            else:                                              # default: teacher one batch ahead on the side stream (two slots per bucket)
                steps_gen = stream_step.run(dl)

            cap_at = {}

            def run_stream(n, start=0):
                traj = 0
                cap_at[start] = stream_step.captures            # graphs captured before this region began
                cap_at[("s", start)] = stream_step.capture_s
                for _ in range(n):
                    last["out"], meta = next(steps_gen)
                    traj += meta["traj_steps"]
                cap_at["end"] = stream_step.captures
                cap_at[("s", "end")] = stream_step.capture_s
                return traj
        else:
            feed = iter(DevicePrefetcher(dl, dev))

            def run_stream(n, start=0):
                traj = 0
                for _ in range(n):
                    task, b, plan = next(feed)
                    if ftab is not None:
                        b["view_table"] = ftab
                    last["out"] = trainer.step(b, task, plan=plan)
                    traj += plan["traj_steps"]
                return traj
        run = run_stream
    if a.dp_structure and a.mode == "graph":
        # RCCL builds its communicator inside the first collectives: let those steps pass, then re-arm the teacher's start gate, so the leg measures
        # the structure and not the start-up (the gate also re-arms itself after a backoff: csrc/encoder.hip)
        run(12)
        torch.cuda.synchronize()
        trainer.gate_reset()
    traj, dt = timed_region(run, a.steps, a.warmup, world, dev)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, last.get("out"), student.store.flat)
    steady = gate_now = None
    if a.mode == "graph" and a.full:    # the driver's K is small (20 steps = 31 ms): the same replay loop over 150 more steps, reported next to it
        n_steady = 150
        traj_s, dt_s = timed_region(run, n_steady, 0, world, dev)
        steady = {"steps": n_steady, "ms_per_step": round(dt_s / n_steady * 1e3, 3), "trajectory_steps_per_sec": round(traj_s / dt_s, 1)}
        # gate counters and health belong to the headline + steady runs: read them BEFORE the per-task loops below, which replay subsets of the
        # ring (a student graph then consumes teacher outputs of an unrelated replay, the gate sees another interleaving and may switch itself off)
        gate_now = trainer.gate_report() if a.teacher == "split" else None
        # the same replay loop over the resident batches of ONE task at a time (60 steps each): what the student's step of each proxy task
        # costs (graph i = student step on batch i || teacher forward on batch i + 1, whose task is the next one of the cycle)
        by_task, gn_task = {}, {}
        for task in TASKS:
            sub = [g for g, (tk, _, _) in zip(graphs, pool) if tk == task]
            if sub:
                run_t = graph_runner(trainer, sub)
                run_t(len(sub))
                _, dt_t = timed_region(run_t, 60, 0, world, dev)
                by_task[task] = round(dt_t / 60 * 1e3, 3)
                gn_task[task] = trainer.opt.grad_norm_report()        # the last replayed step of this loop was a `task` step
        steady["ms_per_step_by_task"] = by_task
        steady["grad_norm_by_task"] = gn_task
    in_graph = (bool(getattr(graphs[0], "rccl_in_graph", False)) if a.mode == "graph" else
                bool(stream_step is not None and any(getattr(getattr(e, "cs", None), "rccl_in_graph", False) for e in stream_step.cache.values())))
    trainer_rccl = (trainer.sync.rccl is not None, in_graph)
    health = trainer.check_health()          # raises if an in-launch hand-off of the row-split encoder kernels ever gave up
    gate = gate_now
    if gate is not None:
        gate["timeout_us"], gate["recent_us"] = O.TEACHER_GATE_US, O.TEACHER_GATE_RECENT_US
        gate["what"] = ("device-side start gate in front of every teacher graph (csrc/encoder.hip): `opened` = it saw the student's whole-encoder launch "
                        "become resident, `already_resident` = that launch was there when the gate started, `timeouts` = the streams did not overlap; "
                        "it switches itself off (`disabled`) after 3 consecutive timeouts")

    roof = None
    if not a.no_profile:      # every rank runs it (the steps contain the gradient all-reduce); rank 0 reports
        nprof = min(len(pool), 6)
        by = instrumented_pass(trainer, pool, nprof, gate_ms=30.0)
        fam = lambda k: k.startswith("magic_gemm")
        gemm_ms = max(sum(t for k, (t, c) in by.items() if fam(k)), 1e-9)
        gemm_n = sum(c for k, (t, c) in by.items() if fam(k))
        all_ms = sum(t for t, c in by.values())
        flops = O.FLOPS["gemm"]            # the GEMM family's own algorithmic FLOPs (fused linear+LN and attention kernels count separately)
        is_mfma = lambda k: any(x in k for x in ("magic_gemm", "magic_linear_ln", "magic_attn_", "magic_encoder", "magic_xencoder", "magic_rowbwd", "magic_chain"))
        chain_ms = sum(t for k, (t, c) in by.items() if k.startswith("magic_chain"))
        chain_n = sum(c for k, (t, c) in by.items() if k.startswith("magic_chain"))
        mfma_ms = sum(t for k, (t, c) in by.items() if is_mfma(k))
        step_ms = dt / a.steps * 1e3
        # achieved = the family's algorithmic FLOPs / the family's SUMMED launch durations (non-overlapped pass), i.e.
        # (FLOPs per launch) / (average launch duration); frac = achieved / dense bf16 MFMA peak.  Reproducible from the committed
        # rocprofv3 --kernel-trace --stats CSV of this command: sum the gemm_* kernels' TotalDurationNs, divide by the executed steps.
        # the roofline object = the Linear-layer contraction family: the GEMM kernels + (since round 3) the chain kernel that took over the frozen
        # teacher's Linear layers -- the same work rounds 1-2 reported as "the GEMM family" (101 GFLOP per step)
        fam_flops, fam_ms, fam_n = flops + O.FLOPS["chain"], gemm_ms + chain_ms, gemm_n + chain_n
        ach = (fam_flops / nprof) / (fam_ms / nprof * 1e-3) / 1e12
        ach_gemm = (flops / nprof) / (gemm_ms / nprof * 1e-3) / 1e12
        ach_all = (O.FLOPS["total"] / nprof) / (mfma_ms / nprof * 1e-3) / 1e12
        traffic, traffic_src = pmc_traffic(gemm_n, chain_n)
        roof = {"bound": "mfma", "kernel": "gemm_kernel / gemm_xcd_kernel / gemm_grouped_kernel / gemm_dw_batch_kernel <bf16, NT|NN|TN> + chain_fwd_kernel / chain64_fwd_kernel<bf16> (the dominant "
                                           "kernel family: every Linear layer's forward, input and weight gradient; the frozen teacher's run inside the chain kernels since round 3; launches over one round of CUs on 64-row tiles since round 4)",
                "achieved": round(ach, 3), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_BF16_TFLOPS, 5),
                "traffic": traffic, "traffic_unit": "bytes per launch of the family (HBM side: rocprofv3 --pmc FETCH_SIZE x 2 [gfx950 reports half the bytes of wide coalesced reads: MI355X_MICROARCH.md 'HBM'] + WRITE_SIZE, counters in KB -> bytes, "
                                                    "summed over the family's launches of the profiled steps and divided by their count; compare with detail.*algorithmic* bytes per launch)",
                "traffic_source": (traffic_src + " (offline rocprofv3 --pmc passes of this command; not collected in this run)") if traffic_src else None,
                "how": "HIP events around every launch on the launch stream, eager pass of the same steps with the captured graphs' launch structure, "
                       "teacher serialised on the main stream, device-side gate so the host runs ahead; family time = SUM of its launch durations",
                "detail": {"family_gflop_per_step": round(fam_flops / nprof / 1e9, 2), "family_launches_per_step": round(fam_n / nprof, 1),
                           "family_ms_per_step": round(fam_ms / nprof, 3), "family_avg_launch_us": round(fam_ms / max(fam_n, 1) * 1e3, 2),
                           "family_share_of_kernel_time": round(fam_ms / all_ms, 4),
                           "gemm_kernels_alone": {"achieved_tflops": round(ach_gemm, 2), "frac": round(ach_gemm / PEAK_BF16_TFLOPS, 5),
                                                  "note": "round 2 reported these alone (92.3 TFLOP/s for 101 GFLOP); the teacher's large-M GEMMs have left the set"},
                           "algorithmic_gflop_per_step": round(flops / nprof / 1e9, 2), "gemm_launches_per_step": gemm_n // nprof,
                           "gemm_ms_per_step": round(gemm_ms / nprof, 3), "avg_gemm_launch_us": round(gemm_ms / max(gemm_n, 1) * 1e3, 2),
                           "gemm_share_of_kernel_time": round(gemm_ms / all_ms, 4),
                           "all_dense_contraction_kernels": {
                               "kernels": "gemm + fused linear+LayerNorm (fwd / bwd) + fused attention (fwd / bwd) + whole-encoder forwards + row-block backward + the teacher's chain kernel",
                               "algorithmic_gflop_per_step": round(O.FLOPS["total"] / nprof / 1e9, 2),
                               "gflop_by_family": {k: round(O.FLOPS[k] / nprof / 1e9, 2) for k in ("gemm", "linear_ln", "attn", "enc", "chain")},
                               "ms_per_step": round(mfma_ms / nprof, 3), "share_of_kernel_time": round(mfma_ms / all_ms, 4),
                               "achieved_tflops": round(ach_all, 2), "frac": round(ach_all / PEAK_BF16_TFLOPS, 5)},
                           "whole_step": {"summed_kernel_ms_per_step_serialised": round(all_ms / nprof, 3), "graph_replay_wall_ms_per_step": round(step_ms, 3),
                                          "frac_of_mfma_peak_on_wall": round(O.FLOPS["total"] / nprof / (step_ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 5)},
                           "teacher_chain_kernel": {
                               "kernel": "chain_fwd_kernel / chain64_fwd_kernel (csrc/chain.hip; 32-row tiles, and 64-row tiles on the 32x32x16 product for launches with more 32-row tiles than CUs): the frozen teacher's per-token half of a block (output projection + LayerNorm, FFN, "
                                         "LayerNorm, next Q|K|V projection) at H = 256 in one launch, forward only",
                               "algorithmic_gflop_per_step": round(O.FLOPS["chain"] / nprof / 1e9, 2), "launches_per_step": round(chain_n / nprof, 1),
                               "avg_launch_us": round(chain_ms / max(chain_n, 1) * 1e3, 1), "share_of_kernel_time": round(chain_ms / all_ms, 4),
                               "achieved_tflops": round(O.FLOPS["chain"] / max(chain_ms, 1e-9) / 1e9, 2),
                               "frac_of_mfma_peak": round(O.FLOPS["chain"] / max(chain_ms, 1e-9) / 1e9 / PEAK_BF16_TFLOPS, 5),
                               "pmc_traffic_bytes_per_launch": pmc_chain_traffic(),
                               "bound": "L2 -> CU fill rate: a 32-row tile streams 1.57 MB of weight fragments (2 MFMAs each); one CU takes 58 B/ns "
                                        "(26.5 us for one workgroup on an idle GPU, profiles/micro/chain_timing.hip)"},
                           "launches_per_step": sum(c for t, c in by.values()) // nprof,
                           "weight_gradient_launch": {
                               "kernel": "gemm_dw_batch_kernel (all deferred dW = dY^T X problems of a step in one launch)",
                               "algorithmic_bytes_per_launch": round(O.BYTES["dw"] / max(O.BYTES["dw_launches"], 1)),
                               "avg_us": round(by.get("magic_gemm_dw_grouped", (0.0, 1))[0] / max(by.get("magic_gemm_dw_grouped", (0.0, 1))[1], 1) * 1e3, 1),
                               "algorithmic_GB_per_s": round(O.BYTES["dw"] / max(by.get("magic_gemm_dw_grouped", (1e-9, 1))[0], 1e-9) / 1e6, 1),
                               "pmc_fetched_bytes_per_launch": pmc_dw_fetch(), "peak_GB_per_s": 8000.0},
                           "top_kernels_share": {k: round(t / all_ms, 4) for k, (t, c) in sorted(by.items(), key=lambda kv: -kv[1][0])[:8]},
                           "kernels_launches_per_step_and_avg_us": {k: [round(c / nprof, 1), round(t / c * 1e3, 1)]
                                                                    for k, (t, c) in sorted(by.items(), key=lambda kv: -kv[1][0])}}}

    if roof is not None and rank == 0:
        roof["detail"]["feature_ingest"] = ingest_rate(dev)

    modes, parity = None, None
    if rank == 0 and world == 1 and not a.no_parity and a.mode == "graph":
        # the parity-clean arithmetic (fp32 MFMA, exact) timed in the same run on the same batches, next to the headline mode
        other = torch.float32 if dtype != torch.float32 else torch.bfloat16
        del graphs
        _, _, t2, s2, tr2 = build_models(other, dev, a.dropout, world, a.batch)
        eager_runner(tr2)(min(3, len(pool)))
        torch.cuda.synchronize()
        g2 = capture_ring(tr2, pool, a.teacher)
        torch.cuda.synchronize()
        traj2, dt2 = timed_region(graph_runner(tr2, g2), a.steps, a.warmup, world, dev)
        nm = {torch.bfloat16: "bf16", torch.float32: "fp32", torch.float16: "fp16"}
        modes = {nm[dtype]: {"ms_per_step": round(dt / a.steps * 1e3, 3), "trajectory_steps_per_sec": round(traj / dt, 1)},
                 nm[other]: {"ms_per_step": round(dt2 / a.steps * 1e3, 3), "trajectory_steps_per_sec": round(traj2 / dt2, 1)},
                 "note": "same batches and schedule, one HIP graph per batch each; fp16 = the bf16 kernels on IEEE half storage (v_mfma_f32_16x16x32_f16, gradient "
                         "seeds x the dynamic loss scale, 4096 at start); fp32 = fp32 storage + exact v_mfma_f32_16x16x4_f32; bf16x3 = fp32 storage, every GEMM contraction as three bf16 MFMAs "
                         "on the hi + lo halves of the fp32 operands (lib.set_f32_mfma)"}
        del g2, tr2
        # the 16-bit twin of the headline mode (bf16 <-> fp16: same kernels, same launches, different storage type)
        twin = torch.float16 if dtype != torch.float16 else torch.bfloat16
        _, _, t4, s4, tr4 = build_models(twin, dev, a.dropout, world, a.batch)
        eager_runner(tr4)(min(3, len(pool)))
        torch.cuda.synchronize()
        g4 = capture_ring(tr4, pool, a.teacher)
        torch.cuda.synchronize()
        traj4, dt4 = timed_region(graph_runner(tr4, g4), a.steps, a.warmup, world, dev)
        traj4s, dt4s = timed_region(graph_runner(tr4, g4), 150, 0, world, dev)          # (the steady form of the headline's `steady` block)
        modes[nm[twin]] = {"ms_per_step": round(dt4 / a.steps * 1e3, 3), "trajectory_steps_per_sec": round(traj4 / dt4, 1),
                           "ms_per_step_steady": round(dt4s / 150 * 1e3, 3), "steady_steps": 150}
        if torch.float16 in (twin, dtype):
            h = tr4 if twin == torch.float16 else trainer
            ls = h.opt.loss_scale.tolist() if getattr(h.opt, "loss_scale", None) is not None else None
            modes["fp16_loss_scale"] = ({"dynamic": True, "scale": ls[0], "clean_steps_in_a_row": int(ls[2]), "skipped_optimizer_steps": h.opt.skipped_steps(),
                                         "rule": "amp.GradScaler on the device: x0.5 after a skipped step, x2 after 2000 updates in a row (csrc/loss.hip step_rng_kernel)"}
                                        if ls is not None else {"dynamic": False})
        del g4, t4, s4, tr4
        # third mode: fp32 storage with the split-bf16 contraction (graphs re-captured: the mode is read by the kernels at run time, but a
        # fresh capture keeps the measurement independent of the previous one)
        prev = L.set_f32_mfma("bf16x3")
        try:
            _, _, t3, s3, tr3 = build_models(torch.float32, dev, a.dropout, world, a.batch)
            eager_runner(tr3)(min(3, len(pool)))
            torch.cuda.synchronize()
            g3 = capture_ring(tr3, pool, a.teacher)
            torch.cuda.synchronize()
            traj3, dt3 = timed_region(graph_runner(tr3, g3), a.steps, a.warmup, world, dev)
            modes["bf16x3"] = {"ms_per_step": round(dt3 / a.steps * 1e3, 3), "trajectory_steps_per_sec": round(traj3 / dt3, 1)}
            del g3, t3, s3, tr3
        finally:
            L.set_f32_mfma(prev)
        del t2, s2
        # the same headline arithmetic with the round-3 reduction of the weight gradients (fp32 atomics: faster, not reproducible run to run)
        prev_det = O.DW_DETERMINISTIC
        O.DW_DETERMINISTIC = False
        try:
            _, _, t5, s5, tr5 = build_models(dtype, dev, a.dropout, world, a.batch)
            eager_runner(tr5)(min(3, len(pool)))
            torch.cuda.synchronize()
            g5 = capture_ring(tr5, pool, a.teacher)
            torch.cuda.synchronize()
            traj5, dt5 = timed_region(graph_runner(tr5, g5), a.steps, a.warmup, world, dev)
            modes["weight_gradient_reduction"] = {
                "default": "deterministic: K-splits and repeated uses of a dW summed in slot order through a workspace (csrc/gemm.hip dw_seam) -- `value` is measured with it",
                "with_fp32_atomics": {"ms_per_step": round(dt5 / a.steps * 1e3, 3), "trajectory_steps_per_sec": round(traj5 / dt5, 1), "select_with": "MAGIC_DW_ATOMICS=1"}}
            del g5, t5, s5, tr5
        finally:
            O.DW_DETERMINISTIC = prev_det
        parity = parity_block(dev)

    cpu = None
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        cpu = cpu_baseline(tcfg, scfg, a.batch)

    rccl_smoke = None
    if rank == 0 and world == 1 and a.backend == "nccl" and a.mode == "graph" and not a.no_parity:
        rccl_smoke = rccl_smoke_leg(student, a.batch, dev)

    secondary = None
    if rank == 0 and world == 1 and not a.no_secondary and a.mode == "graph" and not a.no_parity:
        del trainer, teacher, student
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        secondary = secondary_block()

    if rank == 0:
        info = {"metric": "trajectory-steps/sec (whole node), MAGIC-S R2R pretrain", "value": round(traj / dt, 2),
                "unit": "trajectory-steps/sec", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
                "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": a.dtype, "data": "synthetic",
                "ms_per_step_steady": (round((dt - (cap_at[("s", "end")] - cap_at.get(("s", a.warmup), 0.0))) / a.steps * 1e3, 3) if stream_step is not None and a.mode == "stream-graph" and a.teacher != "same"
                                       else (steady["ms_per_step"] if steady is not None else None)),
                "steady": steady, "teacher_gate": gate, "health": health, "build_id": L.library_build_id(),
                "streams": {"hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "runtime default (4)"), "picked": list(_lanes.probe_log),
                            "what": "every side stream (teacher, gradient exchange) is picked by lanes.beside: candidates from torch's pool until one is "
                                    "measured to run beside the main stream (csrc/encoder.hip magic_stream_probe); `tried` = candidates it took"},
                "launch": a.mode if a.mode not in ("stream", "stream-graph") else f"{a.mode}/{a.ingest}/{a.workers}w" + (f"/{stream_step.captures} bucket graphs, {cap_at['end'] - cap_at.get(a.warmup, 0)} of them captured inside the timed steps" if stream_step is not None else ""),
                "teacher_schedule": ({"split": "one batch ahead of the student, own graph on a side stream", "ahead": "one batch ahead of the student (fork/join inside the step graph)"}.get(a.teacher, "same batch, side stream") if a.mode == "graph" else "same batch, side stream"),
                "config": {"workload": "MAGIC-S R2R pretrain (train_r2r_magic.py path): student H=128/2 heads/6+2+3 layers + frozen teacher H=256, "
                                       "MAKD (txt/img/local/global/predict x emb/attn), tasks mlm:sap:cfp 1:1:1, AdamW+clip, student in train() mode"
                                       + ("; arithmetic = bf16 storage as BASELINE config 2 names it, which is OUTSIDE the north star's |delta action logit| < 1e-3 against the "
                                          "oracle (measured ~4e-3: 8 significand bits; `headline_mode_parity`) -- the SAME kernels on fp16 storage meet it and are timed beside "
                                          "it (`parity_clean_mode`)" if a.dtype == "bf16" else ""),
                           "dropout": a.dropout,
                           "global_batch": a.batch * world, "per_gpu_batch": a.batch, "views": 36, "feat_dim": 768, "max_tokens": 80,
                           "parallelism": f"dp{world}", "samples_per_sec": round(a.batch * world * a.steps / dt, 1)},
                "roofline": roof, "cpu_baseline": cpu, "parity": parity, "modes": modes, "secondary": secondary, "rccl": rccl, "rccl_smoke": rccl_smoke,
                "dp_structure_ms_per_step": ((secondary or {}).get("dp_structure_world1_rccl") or {}).get("ms_per_step"),
                "dp_structure": bool(a.dp_structure),
                "dp_rccl": ({"direct_c_abi": trainer_rccl[0], "collectives_inside_the_step_graph": trainer_rccl[1]} if a.dp_structure else None)}
        if parity is not None:
            # the north star's bar (|delta action logit| < 1e-3 against the oracle, argmax identical) for the arithmetic this line's `value`
            # was measured in, stated at the top level; and the mode of the SAME kernels that meets it, with its own step time
            bar = parity["north_star"]
            meets = lambda p: bool(p["max_abs_logit_delta"] < bar["max_abs_logit_delta"] and p["argmax_agreement"] >= bar["argmax_agreement"])
            info["meets_north_star_tolerance"] = meets(parity[a.dtype])
            info["headline_mode_parity"] = {"dtype": a.dtype, "max_abs_logit_delta": parity[a.dtype]["max_abs_logit_delta"],
                                            "argmax_agreement": parity[a.dtype]["argmax_agreement"], "bar": bar}
            clean = [k for k in ("bf16", "fp16", "bf16x3", "fp32") if k in modes and meets(parity[k])]
            clean.sort(key=lambda k: modes[k]["ms_per_step"])
            info["parity_clean_mode"] = ({"dtype": clean[0], "ms_per_step": modes[clean[0]]["ms_per_step"],
                                          "ms_per_step_steady": modes[clean[0]].get("ms_per_step_steady", steady["ms_per_step"] if (steady is not None and clean[0] == a.dtype) else None),
                                          "loss_scale": modes.get("fp16_loss_scale") if clean[0] == "fp16" else None,
                                          "trajectory_steps_per_sec": modes[clean[0]]["trajectory_steps_per_sec"],
                                          "max_abs_logit_delta": parity[clean[0]]["max_abs_logit_delta"],
                                          "argmax_agreement": parity[clean[0]]["argmax_agreement"],
                                          "select_with": f"--dtype {clean[0]}" if clean[0] in ("fp16", "fp32") else "lib.set_f32_mfma('bf16x3') on the fp32 engine"}
                                         if clean else None)
            info["bf16_max_logit_delta"] = parity["bf16"]["max_abs_logit_delta"]
            info["argmax_agreement"] = parity["bf16"]["argmax_agreement"]
            info["fp32_mode_ms_per_step"] = modes["fp32"]["ms_per_step"]
            info["bf16x3_mode_ms_per_step"] = modes["bf16x3"]["ms_per_step"]
            info["bf16x3_max_logit_delta"] = parity["bf16x3"]["max_abs_logit_delta"]
            info["fp16_mode_ms_per_step"] = modes["fp16"]["ms_per_step"]
            info["fp16_max_logit_delta"] = parity["fp16"]["max_abs_logit_delta"]
            info["fp16_argmax_agreement"] = parity["fp16"]["argmax_agreement"]
        print(json.dumps(info))
    if world > 1 or a.dp_structure:
        try:
            if trainer.sync.rccl is not None:
                trainer.sync.rccl.destroy()
        except NameError:       # (the secondary legs deleted the trainer)
            pass
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
