"""Staging interval (kernel entry to the first barrier: marks 0 -> 1 of the backward, 6 -> 7 of the forward) of workgroup (0, 0) of the fused attention
kernels, and the backward's workgroup total, from a library
built with -DMAGIC_ATTN_TIMING (as profiles/micro/attn_bwd_probe.py builds it; here the library is GIVEN, so that two trees can be compared in one
session), at the headline shapes: 36 x 36 (panorama self-attention, 4 waves) and 37 x 80 (cross-attention, 8 waves), B = 48, 2 heads, dropout 0.1.
Each shape: 5 warm-up launches, then 20 rounds of (200 launches back to back, read the marks of the last): the median and the range over the rounds.

    python profiles/micro/stage_loads_probe.py LABEL PATH/libmagic_attn_timing.so

The row-block kernels' interval comes from profiles/micro/rowbwd_timing.hip (-DRBW_TIMING), which prints it itself."""
import ctypes as C
import statistics
import sys

import torch

label, so = sys.argv[1], sys.argv[2]
lib = C.CDLL(so)
dev = "cuda"
vp, i32, f32, u32 = C.c_void_p, C.c_int, C.c_float, C.c_uint
lib.magic_attn_bwd.argtypes = [i32, i32, i32, i32, i32, vp, i32, vp, vp, i32, vp, i32, vp, i32, f32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, f32, u32, vp]
lib.magic_attn_bwd.restype = i32
lib.magic_attn_fwd.argtypes = [i32, i32, i32, i32, i32, vp, i32, vp, vp, i32, vp, i32, vp, i32, f32, vp, vp, vp, vp, vp, f32, u32, vp, vp]
lib.magic_attn_fwd.restype = i32
B, nh, H = 48, 2, 128
g = torch.Generator().manual_seed(0)
rnd = lambda *s: (torch.randn(*s, generator=g) * 0.3).to(dev).bfloat16().contiguous()      # noqa: E731
seed = torch.tensor([123, 456], dtype=torch.int32, device=dev)
st = torch.cuda.current_stream().cuda_stream

for Nq, Nk in ((36, 36), (37, 80)):
    ldp = (Nk + 7) // 8 * 8
    q, kv, dctx = rnd(B * Nq, H), rnd(B * Nk, 2 * H), rnd(B * Nq, H)
    P = torch.zeros(B, nh, Nq, ldp)
    P[..., :Nk] = torch.softmax(torch.randn(B, nh, Nq, Nk, generator=g), -1)
    P = P.to(dev).bfloat16().contiguous()
    dq, dkv = torch.empty(B * Nq, H, dtype=torch.bfloat16, device=dev), torch.empty(B * Nk, 2 * H, dtype=torch.bfloat16, device=dev)

    def launch():
        rc = lib.magic_attn_bwd(1, B, nh, Nq, Nk, q.data_ptr(), H, kv.data_ptr(), kv.data_ptr() + H * 2, 2 * H, P.data_ptr(), ldp, dctx.data_ptr(), H, 0.125,
                                None, dq.data_ptr(), H, dkv.data_ptr(), dkv.data_ptr() + H * 2, 2 * H, None, None, None, seed.data_ptr(), 0.1, 77, st)
        assert rc == 0, rc

    km = torch.ones(B, Nk, dtype=torch.uint8, device=dev)
    km[:, Nk - 3:] = 0
    Pf, Pdf, ctx = torch.empty_like(P), torch.empty_like(P), torch.empty(B * Nq, H, dtype=torch.bfloat16, device=dev)

    def launch_fwd():
        rc = lib.magic_attn_fwd(1, B, nh, Nq, Nk, q.data_ptr(), H, kv.data_ptr(), kv.data_ptr() + H * 2, 2 * H, Pf.data_ptr(), ldp, ctx.data_ptr(), H, 0.125,
                                km.data_ptr(), None, None, None, seed.data_ptr(), 0.1, 77, Pdf.data_ptr(), st)
        assert rc == 0, rc

    for _ in range(5):
        launch_fwd()
    torch.cuda.synchronize()
    fst, fper = [], []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            launch_fwd()
        e1.record()
        torch.cuda.synchronize()
        t = (C.c_longlong * 8)()
        assert lib.magic_debug_attn_ticks(t) == 0
        fst.append((t[7] - t[6]) / 100)
        fper.append(e0.elapsed_time(e1) / 200 * 1e3)
    print(f"{label} attn_fwd {Nq} x {Nk} (key mask, dropout): staging (mark 6 -> 7) median {statistics.median(fst):.2f} us (range {min(fst):.2f} - {max(fst):.2f}); "
          f"{statistics.median(fper):.1f} us per launch back to back")
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    stage, total, per = [], [], []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            launch()
        e1.record()
        torch.cuda.synchronize()
        t = (C.c_longlong * 8)()
        assert lib.magic_debug_attn_ticks(t) == 0
        stage.append((t[1] - t[0]) / 100)
        total.append((t[5] - t[0]) / 100)
        per.append(e0.elapsed_time(e1) / 200 * 1e3)
    med = statistics.median
    print(f"{label} attn_bwd {Nq} x {Nk}: staging (mark 0 -> 1) median {med(stage):.2f} us (range {min(stage):.2f} - {max(stage):.2f}); workgroup total median "
          f"{med(total):.2f} us ({min(total):.2f} - {max(total):.2f}); {med(per):.1f} us per launch back to back")
