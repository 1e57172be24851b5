"""Bit identity of the two-phase row staging (csrc/common.hpp stage_issue / stage_store) against another build of the library: the cases of
tests/test_stage_loads_gpu.py (attention forward + backward at every shape / option / storage type, the pair forms, the row-block backward at
every M, form and tile height, and behind the attention stage in modes 1 and 2) run once per library, each in a child process of its own
(MAGIC_LIB_FILE, as profiles/micro/ab_libs.sh), and the bytes of every output tensor are compared.

    python profiles/micro/stage_loads_bits.py --other PATH/libmagic_hip.so [--out report.txt]

Outputs compared: P, Pd, ctx, dq, dk, dv of the attention cases; every row output and LayerNorm gradient vector of the row-block cases (the
partial-row, atomics-free gradient form is the default, so they are deterministic).  Not compared: the two sprel gradient words of the attention
backward (one fp32 atomic per workgroup: their order is not fixed)."""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().reshape(-1).view(__import__("torch").uint8).numpy().tobytes()).hexdigest()[:16]


def child(path):
    import torch
    from magic_amd.host import lib as L
    from magic_amd.host import ops as O
    from tests import test_attn_fp64_gpu as A
    from tests import test_stage_loads_gpu as T
    L.set_f32_mfma("exact")
    out = {}
    for c, dt in T.ATTN:
        tag = f"attn {dt} {c.Nq}x{c.Nk} {c.tag}"
        f = T.fwd_state(c, dt)
        A.launch_fwd(f)
        s = T.bwd_state(c, dt, f)
        A.launch_bwd(s)
        O.flush_part_jobs()
        torch.cuda.synchronize()
        for name, t in (("P", f.P.body), ("Pd", f.Pd.body if f.Pd else None), ("ctx", f.ctx.body), ("dq", s.views[0]), ("dk", s.views[1]), ("dv", s.views[2])):
            if t is not None:
                out[f"{tag} {name}"] = digest(t)
    for dt in ("bf16", "fp16"):          # the pair forms: both problems in ONE forward and ONE backward launch
        cases = [T.attn_case(36, 38, "all", cross=True), T.attn_case(80, 80, "all", cross=False)]
        fs = [T.fwd_state(c, dt) for c in cases]
        with L.group():
            for f in fs:
                A.launch_fwd(f)
        ss = [T.bwd_state(c, dt, f) for c, f in zip(cases, fs)]
        with L.group():
            for s in ss:
                A.launch_bwd(s)
        O.flush_part_jobs()
        torch.cuda.synchronize()
        for c, f, s in zip(cases, fs, ss):
            for name, t in (("P", f.P.body), ("Pd", f.Pd.body), ("ctx", f.ctx.body), ("dq", s.views[0]), ("dk", s.views[1]), ("dv", s.views[2])):
                out[f"attn pair {dt} {c.Nq}x{c.Nk} {name}"] = digest(t)
    for dt in ("bf16", "fp16"):          # the row-block backward behind the attention stage (rowbwd16a / rowbwd16ad)
        for N in (17, 36, 80):
            for mode in (1, 2):
                for with_dP in (False, True):
                    seg, outs, vecs = T.attention_stage_problem(N, mode, with_dP, dt)
                    O.rowbwd([seg], None, 0.0)
                    O.flush_rbw_parts()
                    torch.cuda.synchronize()
                    for name, v in list(outs.items()) + list(vecs.items()):
                        out[f"rowbwd {dt} mode{mode} N={N} dP_init={int(with_dP)} {name}"] = digest(v[0])
    for dt in ("bf16", "fp16"):
        for rows in (16, 32):
            for form in T.FORMS:
                for M in T.ROWS:
                    seg, outs, vecs = T.rowblock_problem(M, form, dt)
                    O.rowbwd([seg] if rows == 16 else [T.filler(dt), seg], None, 0.0)
                    O.flush_rbw_parts()
                    torch.cuda.synchronize()
                    for name, v in list(outs.items()) + list(vecs.items()):
                        out[f"rowbwd {dt} {form} M={M} rows={rows} {name}"] = digest(v[0])
    with open(path, "w") as fh:
        for k in sorted(out):
            fh.write(f"{out[k]} {k}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="the library to compare this tree's build with")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    tmp = os.path.join(ROOT, "profile_out")
    os.makedirs(tmp, exist_ok=True)
    res = {}
    for tag, env in (("this", {}), ("other", {"MAGIC_LIB_FILE": os.path.abspath(a.other), "MAGIC_ALLOW_STALE_LIB": "1"})):
        path = os.path.join(tmp, f"stage_loads_bits_{tag}.txt")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True, env={**os.environ, **env}, cwd=ROOT, timeout=600)
        res[tag] = dict(line.rstrip("\n").split(" ", 1)[::-1] for line in open(path))
    keys = sorted(set(res["this"]) | set(res["other"]))
    diff = [k for k in keys if res["this"].get(k) != res["other"].get(k)]
    lines = [f"stage_loads_bits: {len(keys)} output tensors of {len({k.rsplit(' ', 1)[0] for k in keys})} cases compared between this tree's library and the other build",
             f"differing tensors: {len(diff)}"] + [f"  DIFFERS {k}" for k in diff]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
