"""The counter-based dropout mask in plain integers, the float64 references of the launches that apply it, their planted defects, fp32
emulations, and the seeded builders that tests/test_drop_ref64_cpu.py, tests/test_lnbwd_fp64_gpu.py and tests/test_dropsites_fp64_gpu.py share.
Works on whatever device the operands live on; nothing here launches a kernel.

mask64 restates drop_init / drop_mul of csrc/common.hpp: keys ka = seed0 ^ site * 0x9E3779B1, kb = seed1 + site * 0x85EBCA77, one murmur3
fmix32 over (idx ^ ka) + kb, keep iff the word >= floor(double(float32(p)) 2^32), kept elements scaled by float32(1 / (1 - float32(p))).

magic_linear_lnbwd (csrc/gemm.hip linear_lnb_body), from the operands the kernel reads:
    v = x W + R (gemm_ref layout 1, bound D = (K + 8) 2^-23 E; bf16x3 mode: + 2^-16 sum_k |x_k| |w_k| -- each hi part is within 2^-9 relative of
    its operand, so the dropped lo * lo term and the two lo roundings are at most 2^-18 of |x_k| |w_k| each)
    xhat = (y - beta) / gamma, exactly 0 where gamma == 0;  ga = v gamma;  dx = rstd (ga - mean ga - xhat mean(ga xhat))
    |dx error| <= rstd (|gamma| D + mean(|gamma| D) + |xhat| mean(|gamma| |xhat| D))                       D carried to first order
                  + (H + 16) 2^-23 rstd (|ga| + mean |ga| + |xhat| mean |ga xhat|)                       two H-term fp32 sums + the epilogue
                  + one storage ulp
    dxm = dx mask from the UNROUNDED dx: the first two parts times the keep factor + one storage ulp of dxm
    dgamma = init + sum_rows v xhat, dbeta = init + sum_rows v: check_sum's rule of tests/test_partial_rows_gpu.py, 1e-5 (|init| + sum_rows
    envelope), + the carried sum_rows D |xhat| / sum_rows D

The control "dxm built from the rounded dx" is left out everywhere: the two differ by at most half a storage ulp of dx times the keep factor
(0.56 ulp at p = 0.1, nothing at all at p = 0.5 or in fp32 storage), which is below the one-ulp bound in every storage type.  What takes its
place is exact: in fp32 storage dxm == dx * float32 keep factor bit for bit, and at p = 0.5 dxm == 2 dx in every storage type except within the
fp32 error of a rounding boundary (dropped_exact).

LayerNorm forward / backward with dropout sites reuse ln_terms / ln64 / ln_bound of tests/_rowfwd_ref64.py and ln_bwd64 / check_sum / check_dx of
tests/test_partial_rows_gpu.py; linear_ln's `drop` site extends linear_ln_ref of tests/_gemm_ref64.py (mask=).
"""
import torch

from tests import _gemm_ref64 as G
from tests import _rowfwd_ref64 as RF
from tests.test_partial_rows_gpu import REL, check_dx, check_sum, ln_bwd64

F64, UNIT, Ref = G.F64, G.UNIT, G.Ref
M32 = 0xFFFFFFFF
NAN = float("nan")
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


# ---- the mask ----------------------------------------------------------------------------------------------------------------------------
def _mul32(x, c):
    """x * c mod 2^32 for an int64 tensor x < 2^32 and a constant c < 2^32, without leaving the int64 range"""
    return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & M32


def fmix32(x):
    """murmur3's 32-bit finaliser on an int64 tensor of 32-bit words"""
    x = x ^ (x >> 16)
    x = _mul32(x, 0x85EBCA6B)
    x = x ^ (x >> 13)
    x = _mul32(x, 0xC2B2AE35)
    return x ^ (x >> 16)


def keep_scale(p):
    """(threshold word, float32 keep factor as a Python float) of drop_init"""
    p32 = torch.tensor(float(p), dtype=torch.float32)
    thr = int(float(p32) * 4294967296.0)
    scale = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - p32)
    return thr, float(scale)


def hash_words(ka, kb, n, device="cpu"):
    """the 32-bit word drop_mul compares, for idx = 0 .. n - 1; ka, kb: int64 scalars (tensors or ints) below 2^32"""
    idx = torch.arange(n, dtype=torch.int64, device=device) & M32
    return fmix32(((idx ^ ka) + kb) & M32)


def mask64(seed, p, site, rows, cols):
    """float64 [rows, cols]: 0 (dropped) or the keep factor, over the logical index row * cols + col.  seed: two 32-bit words (a tensor on any
    device, a tuple or a list); site: up to 0xFFFFFFFF"""
    if torch.is_tensor(seed):
        s = seed.to(torch.int64) & M32
        s0, s1, dev = s[0], s[1], seed.device
    else:
        s0, s1, dev = int(seed[0]) & M32, int(seed[1]) & M32, "cpu"
    site = int(site) & M32
    ka = s0 ^ ((site * 0x9E3779B1) & M32)
    kb = (s1 + ((site * 0x85EBCA77) & M32)) & M32
    thr, scale = keep_scale(p)
    x = hash_words(ka, kb, rows * cols, dev)
    return torch.where(x >= thr, scale, 0.0).to(F64).view(rows, cols)


def mask_faults(mask, p):
    """what the issue requires of a case's mask, as a list of complaints (empty: fine): both values in the last row and in the last 16-column
    block, the keep count within 4 sigma of 1 - p"""
    out = []
    n, kept = mask.numel(), int((mask != 0).sum())
    for name, part in (("last row", mask[-1]), ("last 16-column block", mask[:, -16:])):
        k = int((part != 0).sum())
        if k == 0 or k == part.numel():
            out.append(f"{name}: only one value")
    p32 = float(torch.tensor(float(p), dtype=torch.float32))
    if abs(kept - n * (1 - p32)) > 4.0 * (n * p32 * (1 - p32)) ** 0.5:
        out.append(f"keep count {kept} of {n}")
    return out


def pick_seed(p, sites, rows, cols, base=(3, 4)):
    """the first seed (base[0], base[1] + j), j = 0, 1, ..., whose masks over [rows, cols] at every site of `sites` (one site or several that
    share the seed; an entry (site, rows) has a row count of its own) satisfy mask_faults -- a deterministic choice, so that every case's mask
    exercises both values where a tile or row edge could hide one"""
    sites = (sites,) if isinstance(sites, int) else tuple(sites)
    sites = [s if isinstance(s, tuple) else (s, rows) for s in sites]
    for j in range(4096):
        seed = (base[0], base[1] + j)
        if not any(mask_faults(mask64(seed, p, s, r, cols), p) for s, r in sites):
            return seed
    raise AssertionError(f"no seed for p {p} sites {sites} [{rows}, {cols}]")


def seed_tensor(seed, device):
    return torch.tensor([int(seed[0]), int(seed[1])], dtype=torch.int64).to(torch.int32).to(device)


def permuted_rows_mask(mask, mod):
    """control: the mask a position-major walk would apply if it indexed it by the LOGICAL row i instead of the physical row
    (i % Bs) mod + i / Bs it loads and stores"""
    M = mask.shape[0]
    Bs = M // mod
    i = torch.arange(M, device=mask.device)
    out = torch.empty_like(mask)
    out[(i % Bs) * mod + i // Bs] = mask
    return out


def dropped_exact(clean, dropped, mask, p, dtype, ref=None, slack=None):
    """complaints about a dropped copy next to its clean twin, both roundings of the same fp32 value: dropped positions exactly zero; fp32
    storage: clean * float32 keep factor bit for bit; p = 0.5 in a 16-bit type: 2 * clean bit for bit -- except at a rounding boundary.  There
    the two may land one storage ulp apart (the compiler rounds an fp32 product straight to 16 bits with v_fma_mixlo, so the clean copy is
    rounded from the exact product and the dropped one from its fp32 rounding: seen on an MI355X at a value 5e-5 ulp from a tie), and that is
    accepted only where the float64 reference `ref` of the dropped value lies within `slack` (its fp32 error bound) + 2^-23 |ref| of the
    midpoint of the two candidates.  Below the smallest normal number the clean copy has lost bits: two subnormal steps there."""
    out = []
    kept = mask != 0
    d, c = dropped.float(), clean.float()
    if not bool((d[~kept] == 0).all()):
        out.append("a dropped position is not exactly zero")
    scale = keep_scale(p)[1]
    if scale == 2.0 or dtype == torch.float32:
        want = (c * torch.tensor(scale, dtype=torch.float32, device=c.device)).to(dtype).float()
        tiny = torch.finfo(dtype).tiny
        normal = c.abs() >= tiny
        off = kept & normal & (d != want)
        if dtype != torch.float32 and ref is not None and bool(off.any()):
            mid = (d.double() + want.double()) / 2
            at_tie = ((d - want).abs().double() <= G.ulp(ref, dtype) * (1 + 1e-9)) & ((ref - mid).abs() <= slack + UNIT * ref.abs())
            off = off & ~at_tie
        if bool(off.any()):
            out.append(f"{int(off.sum())} kept positions are not the clean value times the keep factor")
        if not bool(((d - want).abs()[kept & ~normal] <= 2.0 * tiny * torch.finfo(dtype).eps).all()):
            out.append("a kept subnormal position is not the clean value times the keep factor")
    return out


# ---- magic_linear_lnbwd ------------------------------------------------------------------------------------------------------------------------
def xhat_of(y, gamma, beta):
    g = gamma.to(F64)
    return torch.where(g != 0, (y.to(F64) - beta.to(F64)) / torch.where(g != 0, g, torch.ones_like(g)), torch.zeros_like(y, dtype=F64))


def linear_lnbwd_ref(x, W, R, y, gamma, beta, rstd, mask=None, *, store=None, x3=False, dg_init=0.25, db_init=-0.5, rows_in_sums=None):
    """-> Refs (dx, dxm | None, dgamma, dbeta); x [M, K], W [K, H], R [M, H] | None, y [M, H], rstd [M].  rows_in_sums: the rows the gamma / beta
    sums take (control)"""
    store = store or x.dtype
    pre = G.gemm_ref(1, x, W, residual=R)
    v, E = pre.val, pre.env
    D = (pre.n + 8) * UNIT * E
    if x3:
        D = D + 2.0 ** -16 * (x.to(F64).abs() @ W.to(F64).abs())
    H = v.shape[-1]
    g, r = gamma.to(F64), rstd.to(F64)[:, None]
    xh = xhat_of(y, gamma, beta)
    ga = v * g
    m = lambda t: t.mean(-1, keepdim=True)                          # noqa: E731
    dx = r * (ga - m(ga) - xh * m(ga * xh))
    gD = g.abs() * D
    carried = r * (gD + m(gD) + xh.abs() * m(gD * xh.abs()))
    arith = (H + 16) * UNIT * r * (ga.abs() + m(ga.abs()) + xh.abs() * m((ga * xh).abs()))
    r_dx = Ref(dx, torch.zeros_like(dx), 0, extra=carried + arith)
    r_dxm = None
    if mask is not None:
        r_dxm = Ref(dx * mask, torch.zeros_like(dx), 0, extra=(carried + arith) * mask)
    rows = slice(None) if rows_in_sums is None else rows_in_sums
    init_g, init_b = torch.full((H,), dg_init, dtype=F64, device=v.device), torch.full((H,), db_init, dtype=F64, device=v.device)
    dg = init_g + (v * xh)[rows].sum(0)
    db = init_b + v[rows].sum(0)
    bg = REL * (init_g.abs() + (E * xh.abs())[rows].sum(0)) + (D * xh.abs())[rows].sum(0)
    bb = REL * (init_b.abs() + E[rows].sum(0)) + D[rows].sum(0)
    return r_dx, r_dxm, Ref(dg, torch.zeros_like(dg), 0, extra=bg), Ref(db, torch.zeros_like(db), 0, extra=bb)


LNB_H = (128, 256)
LNB_M = (1, 31, 32, 33, 65)
LNB_K = {16: (8, 64, 72, 136), 32: (4, 32, 36, 68)}      # one k-tile short, exactly one, one and a tail, the second trip of the register prefetch
LNB_P, LNB_SITE, LNB_BIG_SITE = 0.1, 777, 0xABCDEF01
LNB_PAIR = ((33, 1, True), (65, 2, False))               # (M, index into LNB_K, drops) of the two sides of the pair launch
LNB_MODES = ("bf16", "fp16", "fp32", "fp32x3")


def lnb_operands(dtype, M, H, K, seed, device="cpu"):
    """operands of one magic_linear_lnbwd call.  x [M, K] at pitch K + ve and W [K, H] at pitch H + ve, each with two NaN guard rows and one NaN
    vector of pad columns; R [M, H] at pitch H + ve (NaN pad); y dense: the rounded output of a LayerNorm of random rows, with its fp32 rstd; one
    gamma element exactly 0.  The last k is 1.5 * +-0.1875 in every element (lln_operands' construction): leaving it out moves v by 0.28"""
    g = torch.Generator().manual_seed(seed * 7919 + M * 31 + H + K)
    ve = G.ve_of(dtype)
    assert K % ve == 0
    x = torch.full((M + 2, K + ve), NAN, dtype=dtype, device=device)
    W = torch.full((K + 2, H + ve), NAN, dtype=dtype, device=device)
    x[:M, :K], W[:K, :H] = G.randn(g, (M, K), dtype, device), G.randn(g, (K, H), dtype, device, 0.125)
    x[:M, K - 1] = 1.5
    W[K - 1, :H] = G.signs(g, (H,), 0.1875).to(dtype).to(device)
    Rb = torch.full((M, H + ve), NAN, dtype=dtype, device=device)
    Rb[:, :H] = G.offset_randn(g, (M, H)).to(dtype).to(device)
    gamma, beta = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    gamma[H - 3] = 0.0
    pre = torch.randn(M, H, generator=g, dtype=F64)
    yy, _, rstd = RF.ln64(pre, gamma, beta)
    o = dict(M=M, H=H, K=K, dtype=dtype, x=x, W=W, R=Rb, y=yy.to(dtype).to(device).contiguous(), gamma=gamma.float().to(device),
             beta=beta.float().to(device), rstd=rstd.float().to(device))
    return o


def lnb_views(o):
    """the logical operands (x [M, K], W [K, H], R [M, H])"""
    return o["x"][:o["M"], :o["K"]], o["W"][:o["K"], :o["H"]], o["R"][:, :o["H"]]


def lnb_refs(o, mask, with_res=True, x3=False, site=None, seed=None, p=None):
    """(good Refs, {defect: Refs}) -- each defective reference must fail the check of the output named in its key's prefix"""
    x, W, Rr = lnb_views(o)
    Rr = Rr if with_res else None
    M, H, K = o["M"], o["H"], o["K"]
    args = (o["y"], o["gamma"], o["beta"], o["rstd"])
    kw = dict(store=o["dtype"], x3=x3)
    good = linear_lnbwd_ref(x, W, Rr, *args, mask, **kw)
    bad = {"dx:last_k_missing": linear_lnbwd_ref(x[:, :K - 1], W[:K - 1], Rr, *args, mask, **kw)[0]}
    if with_res:
        bad["dx:residual_missing"] = linear_lnbwd_ref(x, W, None, *args, mask, **kw)[0]
    cut = linear_lnbwd_ref(x, W, Rr, *args, mask, rows_in_sums=slice(0, (M - 1) // 32 * 32), **kw)
    bad["dgamma:last_row_tile_missing"], bad["dbeta:last_row_tile_missing"] = cut[2], cut[3]
    if mask is not None:
        other = mask64(seed, p, (site + 1) & M32, M, H).to(mask.device)
        shifted = mask64(seed, p, site, M, H + 1)[:, :H].to(mask.device)
        bad["dxm:mask_of_next_site"] = linear_lnbwd_ref(x, W, Rr, *args, other, **kw)[1]
        if M > 1:                                               # (on a single row the two index rules coincide)
            bad["dxm:mask_columns_off_by_one"] = linear_lnbwd_ref(x, W, Rr, *args, shifted, **kw)[1]
        bad["dxm:last_k_missing"] = linear_lnbwd_ref(x[:, :K - 1], W[:K - 1], Rr, *args, mask, **kw)[1]
    return good, bad


def emulate_linear_lnbwd(o, mask, with_res=True, x3=False, dg_init=0.25, db_init=-0.5):
    """fp32 throughout, as linear_lnb_body: the k-after-k product (bf16x3: lo hi + hi lo + hi hi per k), + R, xhat through the reciprocal of gamma,
    ascending sums, dx and dxm each rounded once from the fp32 d -> (dx, dxm | None, dgamma, dbeta)"""
    x, W, Rr = (t.cpu() for t in lnb_views(o))
    store = o["dtype"]
    if x3:
        a, b = x.float(), W.float()
        ah, bh = a.bfloat16().float(), b.bfloat16().float()
        al, bl = (a - ah).bfloat16().float(), (b - bh).bfloat16().float()
        v = torch.zeros(x.shape[0], W.shape[1])
        for k in range(x.shape[1]):
            v = v + al[:, k:k + 1] * bh[k:k + 1]
            v = v + ah[:, k:k + 1] * bl[k:k + 1]
            v = v + ah[:, k:k + 1] * bh[k:k + 1]
    else:
        v, _ = G.emulate_gemm(1, x, W, 1)
    if with_res:
        v = v + Rr.float()
    gm, bt = o["gamma"].cpu(), o["beta"].cpu()
    ig = torch.where(gm != 0, 1.0 / torch.where(gm != 0, gm, torch.ones_like(gm)), torch.zeros_like(gm))
    xh = (o["y"].cpu().float() - bt) * ig
    ga = v * gm
    H = v.shape[1]
    s1, s2 = torch.zeros(v.shape[0]), torch.zeros(v.shape[0])
    for c in range(H):
        s1, s2 = s1 + ga[:, c], s2 + ga[:, c] * xh[:, c]
    d = o["rstd"].cpu()[:, None] * (ga - (s1 / H)[:, None] - xh * (s2 / H)[:, None])
    dg, db = torch.full((H,), dg_init), torch.full((H,), db_init)
    pg, pb = torch.zeros(H), torch.zeros(H)
    for r in range(v.shape[0]):
        pg, pb = pg + v[r] * xh[r], pb + v[r]
    dxm = None if mask is None else (d * mask.cpu().float()).to(store)
    return d.to(store), dxm, dg + pg, db + pb


# ---- magic_linear_ln with its `drop` site -------------------------------------------------------------------------------------------------------
def linear_ln_ref(x, W, bias, gamma, beta, eps, store, *, residual=None, mask=None, mask_before_bias=False):
    """tests/_gemm_ref64.linear_ln_ref with the dense output -- bias included -- multiplied by `mask` before the residual joins:
    out = LayerNorm(mask (x W^T + bias) + residual).  The dense part's bound is scaled with it.  mask_before_bias: control"""
    if mask is None:
        return G.linear_ln_ref(x, W, bias, gamma, beta, eps, store, residual=residual)[:2]
    g, b = gamma.to(F64), beta.to(F64)
    pre = G.gemm_ref(0, x.to(F64), W.to(F64), bias=None if mask_before_bias else bias)
    v, D = pre.val * mask, (pre.n + 8 + 1) * UNIT * pre.env * mask
    if mask_before_bias:
        v, D = v + bias.to(F64), D + UNIT * bias.to(F64).abs()
    if residual is not None:
        v = v + residual.to(F64)
        D = D + 8 * UNIT * residual.to(F64).abs()
    out, rstd, xhat, prop = G.ln_carry(v, D, g, b, eps)
    if store == torch.float32:
        extra = prop + 16 * UNIT * ((g * xhat).abs() + b.abs()) + G.RSTD_REL * (g * xhat).abs()
    else:
        rms = out.pow(2).mean(-1, keepdim=True).sqrt()
        extra = (G.LN_ULPS - 1.0) * G.ulp(out, store) + G.LN_FLOOR * G.ulp(rms, store).expand_as(out)
    rr = rstd.squeeze(-1)
    return Ref(out, torch.zeros_like(out), 0, extra=extra), Ref(rr, torch.zeros_like(rr), 0, extra=rr * (G.RSTD_REL + rr * (xhat.abs() * D).mean(-1)))


LLN_DROP_M = (1, 33, 65)


def lln_drop_refs(dtype, K, ops, with_res, seed, p, site):
    """(mask, (Ref out, Ref rstd), {defect: Ref out}) of a dropping magic_linear_ln on lln_operands"""
    x, W, bias, gamma, beta, res = ops
    M, H = x.shape[0], W.shape[0]
    mask = mask64(seed, p, site, M, H).to(x.device)
    a = (x[:, :K], W[:, :K], bias, gamma, beta, G.LLN_EPS, dtype)
    r = res if with_res else None
    good = linear_ln_ref(*a, residual=r, mask=mask)
    bad = {"last_k_missing": linear_ln_ref(x[:, :K - 1], W[:, :K - 1], *a[2:], residual=r, mask=mask)[0],
           "mask_of_next_site": linear_ln_ref(*a, residual=r, mask=mask64(seed, p, (site + 1) & M32, M, H).to(x.device))[0],
           "mask_before_bias": linear_ln_ref(*a, residual=r, mask=mask, mask_before_bias=True)[0]}
    if M > 1:                                                   # (on a single row the two index rules coincide)
        bad["mask_columns_off_by_one"] = linear_ln_ref(*a, residual=r, mask=mask64(seed, p, site, M, H + 1)[:, :H].to(x.device))[0]
    if with_res:
        bad["residual_missing"] = linear_ln_ref(*a, residual=None, mask=mask)[0]
    return mask, good, bad


def emulate_linear_ln_drop(x, W, bias, gamma, beta, eps, store, mask, residual=None):
    """emulate_linear_ln with the fp32 dense output (bias included) times the mask in front of the residual"""
    v, _ = G.emulate_gemm(0, x, W, 1, bias=bias)
    v = v * mask.float()
    if residual is not None:
        v = v + residual.float()
    mu = v.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((v - mu) ** 2).mean(-1, keepdim=True) + torch.tensor(eps, dtype=torch.float32))
    return ((v - mu) * rstd * gamma.float() + beta.float()).to(store), rstd.squeeze(-1)


# ---- magic_ln_fwd with site_in0 / site_out ----------------------------------------------------------------------------------------------------
def ln_fwd_drop_ref(o, dtype, mask_in0=None, mask_out=None):
    """from _rowfwd_ref64's ln_operands `o`: in0 times mask_in0 BEFORE the sum; out stays clean; out_drop = y mask_out rounded once
    -> dict(out=(ref, bound), rstd=(ref, bound), out_drop=(ref, bound) | None)"""
    ts = RF.ln_terms(o, F64)
    if mask_in0 is not None:
        ts[0] = ts[0] * mask_in0
    x, E, n = sum(ts), sum(t.abs() for t in ts), len(ts) + (1 if mask_in0 is not None else 0)
    y, gx, rstd = RF.ln64(x, o.gamma.to(x.device), o.beta.to(x.device))
    b = RF.ln_bound(y, gx, rstd, o.gamma.to(x.device), o.beta.to(x.device), dtype, n, E, x)
    out = dict(out=(y, b), rstd=(rstd, G.RSTD_REL * rstd), out_drop=None)
    if mask_out is not None:
        ym = y * mask_out
        if RF.is16(dtype):      # the LayerNorm-output rule on the dropped copy: one rounding of the same fp32 y times the keep factor
            rms = y.pow(2).mean(-1, keepdim=True).sqrt()
            bm = G.LN_ULPS * G.ulp(ym, dtype) + G.LN_FLOOR * G.ulp(rms, dtype).expand_as(y) * mask_out
        else:
            bm = b * mask_out + UNIT * ym.abs()
        out["out_drop"] = (ym, bm)
    return out


def emulate_ln_fwd_drop(o, dtype, mask_in0=None, mask_out=None):
    """fp32: the terms added in the kernel's order, in0 masked first; two-pass statistics; out and out_drop each rounded once from the fp32 y"""
    ts = RF.ln_terms(o, torch.float32)
    if mask_in0 is not None:
        ts[0] = ts[0] * mask_in0.float()
    x = ts[0]
    for t in ts[1:]:
        x = x + t
    mean = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + torch.tensor(RF.EPS, dtype=torch.float32))
    y = (x - mean) * rstd * o.gamma.float() + o.beta.float()
    return y.to(dtype), rstd.squeeze(-1), None if mask_out is None else (y * mask_out.float()).to(dtype)


# ---- magic_ln_bwd with site_dy / site_dx ------------------------------------------------------------------------------------------------------
def ln_bwd_drop_ref(dy, y, gamma, beta, rstd, mask_dy=None, mask_dx=None, do_ln=True):
    """dy times mask_dy on load (before everything, the gamma / beta sums included); dxm = dx mask_dx from the unrounded dx
    -> dict(dx, env, dxm, dg_terms, dg_env, db_terms, db_env) in float64"""
    d = dy.double() if mask_dy is None else dy.double() * mask_dy
    if do_ln:
        dx, env, xh = ln_bwd64(d, y, gamma, beta, rstd)
    else:
        dx, env, xh = d, d.abs(), torch.zeros_like(d)
    out = dict(dx=dx, env=env, dxm=None, dg_terms=d * xh, dg_env=d.abs() * xh.abs(), db_terms=d, db_env=d.abs())
    if mask_dx is not None:
        out["dxm"], out["dxm_env"] = dx * mask_dx, env * mask_dx
    return out


def emulate_ln_bwd_drop(dy, y, gamma, beta, rstd, dtype, mask_dy=None, mask_dx=None, dg_init=0.25, db_init=-0.5):
    """fp32, as ln_bwd_body: dy masked on load, xhat through the reciprocal of gamma -> (dx, dxm | None, dgamma, dbeta)"""
    g = dy.float() if mask_dy is None else dy.float() * mask_dy.float()
    xh = (y.float() - beta.float()) * (1.0 / gamma.float())
    dg, db = torch.full_like(gamma.float(), dg_init), torch.full_like(gamma.float(), db_init)
    for r in range(g.shape[0]):
        dg, db = dg + g[r] * xh[r], db + g[r]
    ga = g * gamma.float()
    H = g.shape[1]
    d = rstd.float()[:, None] * (ga - ga.sum(-1, keepdim=True) / H - xh * ((ga * xh).sum(-1, keepdim=True) / H))
    return d.to(dtype), None if mask_dx is None else (d * mask_dx.float()).to(dtype), dg, db


def fails(fn):
    """True when a raising check (check_sum, check_dx, _rowfwd_ref64.check) rejects"""
    try:
        fn()
    except AssertionError:
        return True
    return False


# ---- the cases of the LayerNorm sites ---------------------------------------------------------------------------------------------------------
DROP_M = (1, 5, 33, 257)
DROP_P = (0.1, 0.5)
S_IN0, S_OUT, S_DY, S_DX = 31, 0xABCDEF01, 41, 0xFFFFFFFF


def ln_fwd_drop_cases():
    """_rowfwd_ref64 cases of magic_ln_fwd with in0: "image" (in0 + an indexed and a constant table) and "in0+in1" (no tables), H in {128, 256} at every
    M, and one case each at 384 and 768"""
    out = [RF.C("ln", f"H{H}-M{M}-{form}", [], H=H, M=M, form=form) for H in (128, 256) for M in DROP_M for form in ("image", "in0+in1")]
    return out + [RF.C("ln", "H384-M5-image", [], H=384, M=5, form="image"), RF.C("ln", "H768-M33-in0+in1", [], H=768, M=33, form="in0+in1")]


def ln_operands_on(c, dtype, device):
    """RF.ln_operands with every tensor on `device`"""
    o = RF.ln_operands(c, dtype)
    mv = lambda t: None if t is None else t.to(device).contiguous()            # noqa: E731
    o.in0, o.in1, o.gamma, o.beta = mv(o.in0), mv(o.in1), mv(o.gamma), mv(o.beta)
    o.tabs = [None if t is None else (mv(t[0]), mv(t[1]), t[2], t[3]) for t in o.tabs]
    return o


def site_combos(a, b):
    """(first site's mask | None, second site's mask | None): each alone, then both"""
    return ((a, None), (None, b), (a, b))


def ln_fwd_drop_defects(o, dtype, mi, mo, seed, p, s_in, s_out):
    """{"<output>:<defect>": (ref, bound)}: the mask of the next site, the mask indexed with H + 1 columns (M > 1: on one row the two rules
    coincide), in0 not masked at all"""
    M, H, dev = o.M, o.H, (mi if mi is not None else mo).device
    out = {}
    if mo is not None:
        out["out_drop:mask_of_next_site"] = ln_fwd_drop_ref(o, dtype, mi, mask64(seed, p, (s_out + 1) & M32, M, H).to(dev))["out_drop"]
        if M > 1:
            out["out_drop:mask_columns_off_by_one"] = ln_fwd_drop_ref(o, dtype, mi, mask64(seed, p, s_out, M, H + 1)[:, :H].to(dev))["out_drop"]
    if mi is not None:
        out["out:mask_of_next_site"] = ln_fwd_drop_ref(o, dtype, mask64(seed, p, (s_in + 1) & M32, M, H).to(dev), mo)["out"]
        out["out:in0_not_masked"] = ln_fwd_drop_ref(o, dtype, None, mo)["out"]
        if M > 1:
            out["out:mask_columns_off_by_one"] = ln_fwd_drop_ref(o, dtype, mask64(seed, p, s_in, M, H + 1)[:, :H].to(dev), mo)["out"]
    return out


# ---- report only: the ratios behind check_dx / check_sum (the assertions stay theirs) -------------------------------------------------------------
def dx_ratio(got, ref, env, dtype):
    u = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}.get(dtype, 0.0)
    bound = u * ref.abs() + REL * (ref.abs() + env) + (6e-8 if dtype == torch.float16 else 1e-30)
    return ((got.double() - ref).abs() / bound).max().item()


def sum_ratio(got, init, terms, env):
    bound = REL * (init.double().abs() + env.sum(0)) + 1e-30
    return ((got.double() - (init.double() + terms.sum(0))).abs() / bound).max().item()


# ---- the embedding stage's cases (tests/test_dropsites_fp64_gpu.py launches them; the CPU file checks their masks) -----------------------------------
EIF_CASES = [c for c in RF.CASES["embed_in"] if c.H in (128, 256) or (c.H, c.M) in ((384, 17), (768, 33))]
S_X0D, S_TOUT, S_DDY = 51, 0xABCDEF01, 61
EIB_SHAPES = [(128, 1, 5), (128, 33, 38), (256, 5, 33), (256, 257, 38)]       # (H, panorama rows, text rows: 38 = 2 x 19 keeps the position-major walk live)


def embed_mask_shapes():
    """[(p, [(site, rows)], H)] of every seed the embedding-stage cases pick"""
    out = []
    for p in DROP_P:
        for c in EIF_CASES:
            out.append((p, [(S_X0D, c.M)] + ([(S_TOUT, c.Mt)] if c.text else []), c.H))
        for H, M, MT in EIB_SHAPES:
            out.append((p, [(S_DDY, M), (S_DY, MT), (S_DX, MT)], H))
    return out
