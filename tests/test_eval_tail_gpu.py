"""The validation kernels (csrc/evaltail.hip) through the C ABI, against float64.

magic_mlm_eval.  Inputs from one seeded CPU generator (seed 0): h = randn(nm, H), W = randn(V, H) / sqrt(H), bias = 0.1 randn(V), a planted peak
per row (h_r += 10 w_p / |w_p|^2 before rounding to the 16-bit type); labels: the peak on even rows, another column on odd rows, -1 on rows
r % 7 == 3.  Row 0's peak and row 1's label sit in the last (partial) slab.  Reference: float64 on the rounded operands.

Preconditions, asserted on the reference alone and for every row: the argmax is the planted peak and the top-2 gap is >= 64 delta, with
delta = (H + 8) 2^-24 (max sum_k |h||w| + max |bias|) -- the fp32 accumulation error of one logit (H products, the bias add, a few roundings of
the softmax arithmetic).  hit_row must then equal the reference exactly.

loss_row: |kernel - fp64| / delta, worst over all rows of all 24 cases, measured on an MI355X: LOSS_WORST below (also in DESIGN section 4); the
test asserts 4 x that figure (the margin is for other draws) and prints each case's figure.  Independently of the constant, every case's worst error
must be smaller than the same quantity for the path this kernel replaces: O.linear_fwd logits in the 16-bit type, then fp32 log-softmax.

magic_eval_rows / magic_cfp_eval: the inputs are exact in fp32, so the bounds are the kernels' own arithmetic -- (N / 256 + 16) 2^-24 for a sum of N
exponentials taken 256 threads wide and folded, relative to the terms' envelope; (H + 1) 2^-24 envelope / T per fp32 dot product of the similarities.
magic_eval_accum: double sums in another order than torch's, 1e-12 of sum |loss|; counts exact."""
import math

import pytest
import torch
import torch.nn.functional as F

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from magic_amd.host import ops as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 89), (33, 600), (64, 600), (65, 600), (200, 1031), (130, 50265)]
DTYPES = [torch.bfloat16, torch.float16]
LOSS_WORST = 0.0173           # worst |loss_row - fp64| / delta over the 24 cases as first measured on an MI355X (see the docstring)
_DATA = {}


def slab_rows(H):
    return 65536 // (2 * H)


def data(nm, V, H, dtype, peak0=None):
    """operands + float64 reference of a case, built once and never modified"""
    key = (nm, V, H, dtype, peak0)
    if key in _DATA:
        return _DATA[key]
    g = torch.Generator().manual_seed(0)
    h = torch.randn(nm, H, generator=g, dtype=torch.float64)
    W = torch.randn(V, H, generator=g, dtype=torch.float64) / math.sqrt(H)
    bias = 0.1 * torch.randn(V, generator=g, dtype=torch.float64)
    peak = torch.randint(0, V, (nm,), generator=g)
    other = (peak + 1 + torch.randint(0, max(V - 1, 1), (nm,), generator=g)) % V
    peak[0] = V - 1 if peak0 is None else peak0       # a peak in the last partial slab
    if nm > 1:
        other[1] = V - 1 if peak[1] != V - 1 else 0   # a (wrong) label in the last partial slab
    h = h + 10.0 * W[peak] / (W[peak] ** 2).sum(1, keepdim=True)
    r = torch.arange(nm)
    labels = torch.where(r % 2 == 0, peak, other)
    labels[r % 7 == 3] = -1
    h16, W16, b32 = h.to(dtype), W.to(dtype), bias.float()
    hd, Wd, bd = h16.double(), W16.double(), b32.double()
    x = hd @ Wd.T + bd
    delta = (H + 8) * 2.0 ** -24 * (float((hd.abs() @ Wd.abs().T).max()) + float(bd.abs().max()))
    top2 = x.topk(min(2, V), dim=1)
    lse = torch.logsumexp(x, 1)
    keep = labels >= 0
    loss = torch.where(keep, lse - x.gather(1, labels.clamp(min=0)[:, None])[:, 0], torch.zeros_like(lse))
    hit = torch.where(keep, (top2.indices[:, 0] == labels).long(), torch.full_like(labels, -1))
    d = dict(nm=nm, V=V, H=H, dtype=dtype, h=h16.to(DEV), W=W16.to(DEV), bias=b32.to(DEV), labels=labels.to(torch.int32).to(DEV), peak=peak,
             argmax=top2.indices[:, 0], gap=(top2.values[:, 0] - top2.values[:, 1]) if V > 1 else torch.full((nm,), math.inf, dtype=torch.float64),
             delta=delta, loss=loss, hit=hit.to(torch.int32), keep=keep)
    _DATA[key] = d
    return d


def run(d, W=None, bias=None, labels=None):
    W = d["W"] if W is None else W
    bias = d["bias"] if bias is None else bias
    labels = d["labels"] if labels is None else labels
    nm, V, H = d["nm"], d["V"], d["H"]
    need = L.load().magic_mlm_eval_ws_need(L.dt(d["dtype"]), nm, V, H)
    assert need == -(-V // slab_rows(H)) * nm * 16
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=DEV)          # sized by the library's own figure, a sentinel behind it
    loss = torch.full((nm + 1,), 7.0, dtype=torch.float32, device=DEV)
    hit = torch.full((nm + 1,), 7, dtype=torch.int32, device=DEV)
    rc = L._fn("magic_mlm_eval")(L.dt(d["dtype"]), nm, V, H, L.P(d["h"]), L.P(W), W.stride(0), L.P(bias), L.P(labels), -1, L.P(ws), L.P(loss), L.P(hit), L.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert float(loss[nm]) == 7.0 and int(hit[nm]) == 7 and bool((ws[need:] == 0x5A).all()), "wrote past its extents"
    return loss[:nm].cpu(), hit[:nm].cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("nm,V", SHAPES)
def test_mlm_eval_against_fp64(nm, V, H, dtype):
    d = data(nm, V, H, dtype)
    # preconditions, on the reference alone; no row is exempt
    assert torch.equal(d["argmax"], d["peak"])
    assert float(d["gap"].min()) >= 64 * d["delta"], (float(d["gap"].min()), d["delta"])
    loss, hit = run(d)
    assert torch.equal(hit, d["hit"])
    if (nm, V) == (130, 50265):
        assert (int((hit == 1).sum()), int((hit >= 0).sum())) == (56, 111)
    if (nm, V) == (200, 1031):
        assert (int((hit == 1).sum()), int((hit >= 0).sum())) == (86, 171)
    assert bool((loss[~d["keep"]] == 0).all())
    worst = float((loss.double() - d["loss"]).abs().max()) / d["delta"]
    # the path this replaces: logits rounded to the 16-bit type, fp32 log-softmax
    ldv = (V + 7) // 8 * 8
    logits = torch.zeros(nm, ldv, dtype=dtype, device=DEV)
    O.linear_fwd(d["h"], d["W"], d["bias"], nm, out=logits, ldc=ldv)
    lp = torch.log_softmax(logits[:, :V].float(), 1).cpu()
    lab = d["labels"].cpu().long()
    parent = torch.where(d["keep"], -lp.gather(1, lab.clamp(min=0)[:, None])[:, 0], torch.zeros(nm))
    parent_worst = float((parent.double() - d["loss"]).abs().max()) / d["delta"]
    print(f"mlm_eval nm={nm} V={V} H={H} {dtype}: worst |dloss| / delta = {worst:.4f} (16-bit logits path {parent_worst:.2f}); delta = {d['delta']:.3e}, "
          f"smallest top-2 gap = {float(d['gap'].min()):.3f}")
    assert worst <= 4 * LOSS_WORST
    if int(d["keep"].sum()):
        assert worst < parent_worst


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("H", [128, 256])
def test_mlm_eval_argmax_ties_go_to_the_lowest_index(H, dtype):
    """the peak column of row 0 duplicated (same W row, same bias) below and above it, in its own slab (either column half) and in another one"""
    SR = slab_rows(H)
    p = SR + 40
    d = data(33, 600, H, dtype, peak0=p)
    assert int(d["argmax"][0]) == p
    for q in (SR + 3, p + 16, p + SR // 2, 5, 2 * SR + 7):      # same slab: another lane, the same lane's next block, the other column half
        assert (q // SR == p // SR) == (q in (SR + 3, p + 16, p + SR // 2)) and q < 600
        assert q != p + SR // 2 or (p % SR < SR // 2 <= q % SR)          # ... which the two halves' merge inside the workgroup decides
        W, bias = d["W"].clone(), d["bias"].clone()
        W[q], bias[q] = W[p], bias[p]
        lo, hi = min(p, q), max(p, q)
        for lab, want in ((lo, 1), (hi, 0)):
            labels = d["labels"].clone()
            labels[0] = lab
            _, hit = run(d, W=W, bias=bias, labels=labels)
            assert int(hit[0]) == want, (q, lab)


def test_mlm_eval_is_bitwise_reproducible():
    d = data(130, 50265, 128, torch.bfloat16)
    a, b = run(d), run(d)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_mlm_eval_refuses_other_forms():
    lib = L.load()
    d = data(33, 600, 128, torch.bfloat16)
    assert lib.magic_mlm_eval_supported(1, 128) == 1 and lib.magic_mlm_eval_supported(2, 256) == 1
    assert lib.magic_mlm_eval_supported(0, 128) == 0 and lib.magic_mlm_eval_supported(1, 384) == 0
    assert lib.magic_mlm_eval_ws_need(0, 33, 600, 128) == -1 and lib.magic_mlm_eval_ws_need(1, 33, 600, 384) == -1
    ws = torch.zeros(3 * 33 * 16, dtype=torch.uint8, device=DEV)
    loss, hit = torch.zeros(33, device=DEV), torch.zeros(33, dtype=torch.int32, device=DEV)
    good = [1, 33, 600, 128, L.P(d["h"]), L.P(d["W"]), 128, L.P(d["bias"]), L.P(d["labels"]), -1, L.P(ws), L.P(loss), L.P(hit), L.stream()]

    def rc(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L._fn("magic_mlm_eval")(*a)
    assert rc(_0=0) == -1 and rc(_3=384) == -1 and rc(_1=0) == -1 and rc(_2=0) == -1
    for i in (4, 5, 7, 8, 10, 11, 12):
        assert rc(**{f"_{i}": None}) == -1, i
    assert rc() == 0
    torch.cuda.synchronize()


def _ce_ref(x, lab, ignore):
    x = x.double()
    keep = lab != ignore
    loss = F.cross_entropy(x, lab.clamp(min=0), reduction="none")
    return torch.where(keep, loss, torch.zeros_like(loss)), torch.where(keep, (x.argmax(1) == lab).long(), torch.full_like(lab, -1))


@pytest.mark.parametrize("M,N", [(48, 20), (5, 513)])
def test_eval_rows_hard_labels(M, N):
    g = torch.Generator().manual_seed(M)
    x = 3 * torch.randn(M, N, generator=g)
    x[torch.rand(M, N, generator=g) < 0.3] = -math.inf
    lab = torch.randint(0, N, (M,), generator=g)
    x[torch.arange(M), lab] = torch.randn(M, generator=g)          # the label's logit is never masked
    x[0, lab[0]] = 9.0
    lab[2] = -100
    ld = N + 3
    xs = torch.full((M, ld), 99.0)
    xs[:, :N] = x
    loss, hit = O.eval_rows(xs.to(DEV), M, N, ld, labels=lab.to(torch.int32).to(DEV))
    ref_l, ref_h = _ce_ref(x, lab, -100)
    assert torch.equal(hit.cpu().long(), ref_h) and int(hit[2]) == -1 and int(hit[0]) == 1 and 0 in ref_h.tolist()
    xd = x.double()
    tol = 2.0 ** -23 * (torch.logsumexp(xd, 1).abs() + xd.gather(1, lab.clamp(min=0)[:, None])[:, 0].abs()) + (N / 256 + 16) * 2.0 ** -24
    err = (loss.cpu().double() - ref_l).abs()
    assert bool((err <= tol).all()), float((err / tol).max())
    assert float(loss[2]) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_eval_rows_soft_targets(dtype):
    M, N = 37, 1000
    g = torch.Generator().manual_seed(3)
    x = (2 * torch.randn(M, N, generator=g)).to(dtype)
    t = torch.softmax(3 * torch.randn(M, N, generator=g), 1)
    t[torch.rand(M, N, generator=g) < 0.5] = 0.0
    t[:, 7] += 0.05
    t[::2] = 0.0
    t[torch.arange(0, M, 2), x[::2].float().argmax(1)] = 1.0           # even rows: the target's argmax is the logits' (hit 1)
    t[5] = 0.0                                                      # a bucket-padded row
    loss, hit = O.eval_rows(x.to(DEV), M, N, N, targets=t.to(DEV))
    xd, td = x.double(), t.double()
    lp = torch.log_softmax(xd, 1)
    ref = F.kl_div(lp, td, reduction="none").sum(1)
    want = (xd.argmax(1) == td.argmax(1)).int()
    want[5] = -1
    assert torch.equal(hit.cpu(), want) and 0 in want.tolist() and 1 in want.tolist()
    pos = td > 0
    env = (td * (torch.where(pos, td, torch.ones_like(td)).log().abs() + xd.abs())).sum(1) + torch.logsumexp(xd, 1).abs() * td.sum(1)
    tol = (N / 256 + 16) * 2.0 ** -24 * env + 1e-12
    err = (loss.cpu().double() - ref).abs()
    assert bool((err <= tol).all()), float((err / tol).max())
    assert float(loss[5]) == 0.0


@pytest.mark.parametrize("B", [3, 48])
def test_cfp_eval(B):
    H, T = 128, 0.5
    g = torch.Generator().manual_seed(B)
    txt = torch.randn(B, H, generator=g) / math.sqrt(H)
    a = 0.5 * txt + torch.randn(B, H, generator=g) / math.sqrt(H)
    loss, hit = O.cfp_eval(a.to(DEV), txt.to(DEV), T)
    ad, td = a.double(), txt.double()
    sim = ad @ td.T / T
    tgt = torch.arange(B)
    ref = 0.5 * (F.cross_entropy(sim, tgt, reduction="none") + F.cross_entropy(sim.T, tgt, reduction="none"))
    e_s = (H + 1) * 2.0 ** -24 * float((ad.abs() @ td.abs().T).max()) / T
    top2 = sim.topk(2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) > 64 * e_s          # precondition: no argmax inside the fp32 error of a similarity
    assert torch.equal(hit.cpu().long(), (sim.argmax(1) == tgt).long())
    lse = torch.maximum(torch.logsumexp(sim, 1).abs(), torch.logsumexp(sim.T, 1).abs())
    tol = 2 * e_s + (B + 16) * 2.0 ** -24 + 2.0 ** -22 * (lse + sim.diagonal().abs())
    err = (loss.cpu().double() - ref).abs()
    assert bool((err <= tol).all()), float((err / tol).max())


@pytest.mark.parametrize("M", [1, 1000, 5000])
def test_eval_accum(M):
    g = torch.Generator().manual_seed(M)
    loss = (5 * torch.rand(M, generator=g)).float()
    hit = torch.randint(-1, 2, (M,), generator=g).to(torch.int32)
    loss[hit < 0] = 0.0
    block = O.eval_block(DEV)
    assert block.numel() * block.element_size() == 96 and int(block.abs().sum()) == 0
    ld, hd = loss.to(DEV), hit.to(DEV)
    O.eval_accum(ld, hd, M, block, 2)
    once = block.clone()
    O.eval_accum(ld, hd, M, block, 0)
    O.eval_accum(ld, hd, M, block, 2)                                # a second call adds
    b = block.cpu()
    lossw, hits, rows = b[:4].view(torch.float64), b[4:8], b[8:12]
    s, nh, nr = float(loss.double().sum()), int((hit == 1).sum()), int((hit >= 0).sum())
    tol = 1e-12 * float(loss.double().abs().sum()) + 1e-300
    assert hits.tolist() == [nh, 0, 2 * nh, 0] and rows.tolist() == [nr, 0, 2 * nr, 0]
    assert abs(float(lossw[0]) - s) <= tol and abs(float(lossw[2]) - 2 * s) <= 2 * tol and float(lossw[1]) == 0.0 == float(lossw[3])
    o = once.cpu()
    assert o[:4].view(torch.float64)[2] == lossw[0] and o[4:8].tolist() == [0, 0, nh, 0]       # the same rows, the same bits, whatever the slot
    again = O.eval_block(DEV)
    O.eval_accum(ld, hd, M, again, 2)
    assert torch.equal(again, once)


def test_eval_entry_points_refuse_bad_arguments():
    x = torch.zeros(4, 8, device=DEV)
    lab = torch.zeros(4, dtype=torch.int32, device=DEV)
    t = torch.zeros(4, 8, device=DEV)
    loss, hit = torch.zeros(4, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    s = L.stream()
    f = L._fn("magic_eval_rows")
    assert f(0, 4, 8, L.P(x), 8, L.P(lab), -100, L.P(t), 8, L.P(loss), L.P(hit), s) == -1           # both labels and targets
    assert f(0, 4, 8, L.P(x), 8, None, -100, None, 0, L.P(loss), L.P(hit), s) == -1                 # neither
    assert f(0, 4, 8, L.P(x), 7, L.P(lab), -100, None, 0, L.P(loss), L.P(hit), s) == -1             # ld < N
    assert f(3, 4, 8, L.P(x), 8, L.P(lab), -100, None, 0, L.P(loss), L.P(hit), s) == -1
    assert L._fn("magic_cfp_eval")(0, 65, 128, L.P(x), L.P(x), 1.0, L.P(loss), L.P(hit), s) == -1
    assert L._fn("magic_cfp_eval")(0, 4, 8, L.P(x), L.P(x), 0.0, L.P(loss), L.P(hit), s) == -1
    blk = O.eval_block(DEV)
    assert L._fn("magic_eval_accum")(4, L.P(loss), L.P(hit), L.P(blk), 4, s) == -1
    assert L._fn("magic_eval_accum")(0, L.P(loss), L.P(hit), L.P(blk), 0, s) == -1
    assert L._fn("magic_eval_accum")(4, L.P(loss), L.P(hit), None, 0, s) == -1
