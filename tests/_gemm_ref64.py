"""float64 references of the GEMM family (csrc/gemm.hip), their error envelopes, the per-element check, and the seeded problem builders that
tests/test_gemm_ref64_cpu.py and tests/test_gemm_fp64_gpu.py share -- so the CPU file proves on the SAME inputs that every planted defect the GPU
file uses is caught.  Works on whatever device the operands live on; nothing here launches a kernel.

Every reference is computed from the operands the kernel reads (the stored 16-bit / fp32 values, taken to float64).  Next to each value it
returns the envelope E = |alpha| sum_k |a_k| |b_k| + |bias| + |residual| + |C_in| and the number n of terms summed into the element.

    check passes an element when  |got - ref| <= (n + 8) 2^-23 E + U [+ extra]

(n + 8) 2^-23 is the first-order worst case of an fp32 sum of n products in ANY order with a truncating accumulator (one unit 2^-23 per
addition instead of the half unit of round-to-nearest), plus 8 units for the epilogue's own operations.  U is one unit in the last place of a
16-bit storage type at |ref| (0 for fp32 storage).  `extra` carries A |pre-activation| for the erf epilogues (A is measured on the GPU, see
test_gemm_fp64_gpu.py) and the propagated input error of a LayerNorm.
LayerNorm outputs in 16-bit storage use the rule of tests/test_encoder_fp64_gpu.py: 1 ulp of |ref| + 0.003 ulp of the row's rms.
"""
import math

import torch

F64 = torch.float64
UNIT = 2.0 ** -23
LN_ULPS, LN_FLOOR = 1.0, 0.003          # tests/test_encoder_fp64_gpu.py BOUNDS
RSTD_REL = 4e-7                         # tests/test_encoder_fp64_gpu.py RSTD_REL: the fp32 statistics' own error


def ve_of(dtype):
    return 4 if dtype == torch.float32 else 8


def rup(n, m):
    return (n + m - 1) // m * m


def ulp(x, dtype):
    """unit in the last place of |x| in a 16-bit storage type (subnormals: the smallest normal's); 0 for fp32 storage"""
    if dtype == torch.float32:
        return torch.zeros_like(x)
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    _, e = torch.frexp(x.abs().clamp_min(1e-300))
    return torch.ldexp(torch.ones_like(x), (e - 1).clamp_min(emin) - mant)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


class Ref:
    """value, envelope, number of summed terms, extra allowance (tensor or 0.0), |pre-activation| where an erf epilogue ran (else None)"""

    def __init__(self, val, env, n, extra=0.0, pre=None):
        self.val, self.env, self.n, self.extra, self.pre = val, env, n, extra, pre


def bound(ref, store, act_a=0.0):
    b = (ref.n + 8) * UNIT * ref.env + ulp(ref.val, store) + ref.extra
    if ref.pre is not None:
        b = b + act_a * ref.pre
    return b


def ratio(got, ref, store, act_a=0.0):
    """worst |got - ref| / bound over the elements (inf when got is not finite somewhere); <= 1 passes"""
    got = got.to(F64)
    if not torch.isfinite(got).all():
        return float("inf")
    b = bound(ref, store, act_a)
    d = (got - ref.val).abs()
    r = d / b.clamp_min(1e-300)
    return r.max().item() if r.numel() else 0.0


def passes(got, ref, store, act_a=0.0):
    return ratio(got, ref, store, act_a) <= 1.0


# ---- the product ----------------------------------------------------------------------------------------------------------------------
def product(layout, A, B):
    """A, B: float64 logical operands [..., M, K] / [..., N, K] (0), [..., M, K] / [..., K, N] (1), [..., K, M] / [..., K, N] (2)
    -> (sum_k a b, sum_k |a| |b|) as [..., M, N]"""
    if layout == 0:
        B = B.transpose(-1, -2)
    elif layout == 2:
        A = A.transpose(-1, -2)
    return A @ B, A.abs() @ B.abs()


def k_slice(layout, A, B, lo, hi):
    """the operands restricted to contraction indices [lo, hi)"""
    a = A[..., lo:hi] if layout != 2 else A[..., lo:hi, :]
    b = B[..., lo:hi] if layout == 0 else B[..., lo:hi, :]
    return a, b


def gemm_ref(layout, A, B, *, alpha=1.0, bias=None, epilogue=0, aux=None, residual=None, c_in=None):
    """magic_gemm: C = epi(alpha A B + bias) + residual (+ C_in when accumulating); .c2 = the pre-activation alpha A B + bias"""
    A, B = A.to(F64), B.to(F64)
    P, S = product(layout, A, B)
    v = alpha * P
    E = abs(alpha) * S
    if bias is not None:
        v = v + bias.to(F64)
        E = E + bias.to(F64).abs()
    pre = None
    out = v
    if epilogue == 1:
        out, pre = gelu(v), v.abs()
    elif epilogue == 2:
        out = v.clamp_min(0.0)
    elif epilogue == 3:
        out, pre = v * dgelu(aux.to(F64)), v.abs()
    elif epilogue == 4:
        out = torch.where(aux.to(F64) > 0, v, torch.zeros_like(v))
    for t in (residual, c_in):
        if t is not None:
            out = out + t.to(F64)
            E = E + t.to(F64).abs()
    K = A.shape[-1] if layout != 2 else A.shape[-2]
    r = Ref(out, E.expand_as(out), K, pre=pre)
    r.c2 = Ref(v, (abs(alpha) * S + (bias.to(F64).abs() if bias is not None else 0.0)).expand_as(v), K)
    return r


def split_ranges(K, bk, splitk):
    """the K ranges magic_gemm's splits own: whole tiles of bk, ceil(tiles / splitk) per split; trailing splits may be empty"""
    tiles = (K + bk - 1) // bk
    per = (tiles + splitk - 1) // splitk
    return [(min(K, s * per * bk), min(K, (s + 1) * per * bk)) for s in range(splitk)]


def slab_ref(layout, A, B, bk, splitk, *, alpha=1.0, bias=None, skip=None):
    """splitk < 0: slab s = alpha A[k in split s] B (+ bias in slab 0); an empty split's slab is zeros; n = the length of each slab's own K range.
    skip: a split left out (control)"""
    A, B = A.to(F64), B.to(F64)
    vals, envs, ns = [], [], []
    for s, (lo, hi) in enumerate(split_ranges(A.shape[-1] if layout != 2 else A.shape[-2], bk, splitk)):
        ns.append(hi - lo)
        a, b = k_slice(layout, A, B, lo, hi if s != skip else lo)
        P, S = product(layout, a, b)
        v, E = alpha * P, abs(alpha) * S
        if s == 0 and bias is not None:
            v, E = v + bias.to(F64), E + bias.to(F64).abs()
        vals.append(v)
        envs.append(E.expand_as(v))
    n = torch.tensor(ns, dtype=F64, device=A.device).view((-1,) + (1,) * vals[0].dim())        # a slab sums its own split's k only
    return Ref(torch.stack(vals), torch.stack(envs), n)


# ---- weight gradients -----------------------------------------------------------------------------------------------------------------
def dw_ref(parts, dW_in=None, db_in=None):
    """dW = dW_in + sum over parts (problems sharing a dW, or row segments) of dY^T X; db = db_in + column sums of dY.  parts: [(dY [m, N], X [m, K])],
    m may be 0.  -> (Ref dW, Ref db); n = total rows"""
    N, K = parts[0][0].shape[1], parts[0][1].shape[1]
    dev = parts[0][0].device
    v, E = torch.zeros(N, K, dtype=F64, device=dev), torch.zeros(N, K, dtype=F64, device=dev)
    b, Eb = torch.zeros(N, dtype=F64, device=dev), torch.zeros(N, dtype=F64, device=dev)
    n = 0
    for dy, x in parts:
        dy, x = dy.to(F64), x.to(F64)
        v, E = v + dy.t() @ x, E + dy.abs().t() @ x.abs()
        b, Eb = b + dy.sum(0), Eb + dy.abs().sum(0)
        n += dy.shape[0]
    if dW_in is not None:
        v, E = v + dW_in.to(F64), E + dW_in.to(F64).abs()
    if db_in is not None:
        b, Eb = b + db_in.to(F64), Eb + db_in.to(F64).abs()
    return Ref(v, E, n), Ref(b, Eb, n)


# ---- Linear + LayerNorm ---------------------------------------------------------------------------------------------------------------
def ln_carry(v, D, g, b, eps):
    """float64 LayerNorm of v (gamma g, beta b) and an input bound D carried through it to first order
    -> (out, rstd [.., 1], xhat, |g| rstd (D + mean D + |xhat| mean(|xhat| D)))"""
    mu = v.mean(-1, keepdim=True)
    var = ((v - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (v - mu) * rstd
    out = xhat * g + b
    prop = g.abs() * rstd * (D + D.mean(-1, keepdim=True) + xhat.abs() * (xhat.abs() * D).mean(-1, keepdim=True))
    return out, rstd, xhat, prop


def linear_ln_ref(x, W, bias, gamma, beta, eps, store, *, residual=None, act=0, act_a=0.0):
    """out = LayerNorm(act(x W^T + bias) [+ residual]) -> (Ref out, Ref rstd, Ref pre-activation)
    The dense part's bound D (the GEMM rule, with A |v| for gelu) is carried through the normalisation to first order:
    |d out_i| <= |g_i| rstd (D_i + mean D + |xhat_i| mean(|xhat| D)).  16-bit storage: the rule of test_encoder_fp64_gpu.py alone, 1 ulp + 0.003
    row-rms ulp.  fp32 storage: the carried bound + 16 units of |g xhat| + |beta| for the statistics and the affine map + RSTD_REL of |g xhat|."""
    x, W = x.to(F64), W.to(F64)
    g, b = gamma.to(F64), beta.to(F64)
    pre = gemm_ref(0, x, W, bias=bias)
    v, D = pre.val, (pre.n + 8) * UNIT * pre.env
    if act == 1:
        D = D * dgelu(v).abs().clamp_min(1.0) + act_a * v.abs()
        v = gelu(v)
    elif act == 2:
        v = v.clamp_min(0.0)
    if residual is not None:
        v = v + residual.to(F64)
        D = D + 8 * UNIT * residual.to(F64).abs()
    out, rstd, xhat, prop = ln_carry(v, D, g, b, eps)
    if store == torch.float32:
        extra = prop + 16 * UNIT * ((g * xhat).abs() + b.abs()) + RSTD_REL * (g * xhat).abs()
    else:
        rms = out.pow(2).mean(-1, keepdim=True).sqrt()
        extra = (LN_ULPS - 1.0) * ulp(out, store) + LN_FLOOR * ulp(rms, store).expand_as(out)
    r_out = Ref(out, torch.zeros_like(out), 0, extra=extra)
    rr = rstd.squeeze(-1)
    r_rstd = Ref(rr, torch.zeros_like(rr), 0, extra=rr * (RSTD_REL + rr * (xhat.abs() * D).mean(-1)))
    return r_out, r_rstd, pre


# ---- fp32 emulations (CPU file): what an honest fp32 kernel may return ------------------------------------------------------------------
def emulate_gemm(layout, A, B, ways, *, alpha=1.0, bias=None, epilogue=0, aux=None, residual=None, c_in=None, store=torch.float32, lo=0, hi=None):
    """the product summed in fp32, k after k (ways = 1) or as `ways` interleaved partial sums added at the end; fp32 epilogue with torch's erf;
    the result rounded to `store`.  Also returns the fp32 pre-activation."""
    A, B = A.float(), B.float()
    if layout == 0:
        B = B.transpose(-1, -2)
    elif layout == 2:
        A = A.transpose(-1, -2)
    K = A.shape[-1]
    hi = K if hi is None else hi
    parts = [torch.zeros(A.shape[:-1] + B.shape[-1:], dtype=torch.float32) for _ in range(ways)]
    for k in range(lo, hi):
        parts[k % ways] = parts[k % ways] + A[..., :, k:k + 1] * B[..., k:k + 1, :]
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    v = acc * torch.tensor(alpha, dtype=torch.float32)
    if bias is not None:
        v = v + bias.float()
    out = v
    if epilogue == 1:
        out = 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752))
    elif epilogue == 2:
        out = v.clamp_min(0.0)
    elif epilogue == 3:
        a = aux.float()
        out = v * (0.5 * (1.0 + torch.erf(a * 0.70710678118654752)) + a * 0.39894228040143268 * torch.exp(-0.5 * a * a))
    elif epilogue == 4:
        out = torch.where(aux.float() > 0, v, torch.zeros_like(v))
    for t in (residual, c_in):
        if t is not None:
            out = out + t.float()
    return out.to(store), v.to(store)


# ---- seeded operands ------------------------------------------------------------------------------------------------------------------
class Buf:
    """a flat device buffer and the strided logical view a kernel addresses inside it: view[b, h, r, c] = flat[b sb + h sh + r ld + c]"""

    def __init__(self, nb, nh, rows, cols, ld, dtype, device, fill, gap=0, lds=None):
        self.ld, self.sh = ld, (rows + gap) * max([ld] + list(lds or []))
        self.sb = nh * self.sh + (8 * ld if gap else 0)
        self.flat = torch.full((nb * self.sb + 8,), fill, dtype=dtype, device=device)
        self.shape = (nb, nh, rows, cols)

    def view(self, ld=None, flat=None):
        nb, nh, rows, cols = self.shape
        return torch.as_strided(self.flat if flat is None else flat, (nb, nh, rows, cols), (self.sb, self.sh, ld or self.ld, 1))

    def like(self, dtype, fill, ld, cols=None):
        """another buffer addressed with the SAME batch / head offsets and its own pitch (aux, residual, C2 use C's offsets)"""
        o = Buf.__new__(Buf)
        o.ld, o.sh, o.sb = ld, self.sh, self.sb
        o.flat = torch.full_like(self.flat, fill, dtype=dtype)
        o.shape = self.shape[:3] + (cols or self.shape[3],)
        return o

    def untouched(self):
        """True when every element outside the logical view still holds NaN"""
        m = torch.zeros(self.flat.shape, dtype=torch.bool, device=self.flat.device)
        self.view(flat=m)[:] = True
        return bool(torch.isnan(self.flat[~m]).all())


def randn(gen, shape, dtype, device, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(dtype).to(device)


def signs(gen, shape, mag):
    return torch.where(torch.randn(*shape, generator=gen) < 0, -mag, mag)


def offset_randn(gen, shape):
    """random values kept away from zero (|x| >= 0.25 mostly): a bias or residual whose absence always shows"""
    z = torch.randn(*shape, generator=gen)
    return torch.where(z < 0, -0.25, 0.25) + 0.5 * z


def gemm_operand(gen, dtype, device, nb, nh, shape, k_contig, scale, sk, pad, gap):
    """one input operand in padded storage.  Its last row / column along the output axis and its last contraction index are +-1.5 scale, and
    the last output row / column carries the shared sign pattern `sk` over its first len(sk) contraction indices: with the other operand's
    the corner element is ~ 2.25 len(sk) / 8 whatever the seed, and small enough that one k more or less shows in 16-bit storage.
    k-contiguous (the contraction index runs along the pitch; K is a vector multiple): every element outside the logical extent -- the extra
    vector of pad columns, guard rows, gaps -- is NaN, so a read past K or past the last row poisons the result.
    out-contiguous: everything outside is random (the kernel may load it into lanes it never stores)."""
    ve = ve_of(dtype)
    assert not (k_contig and shape[1] % ve), "the C ABI wants K a vector multiple (or zero padding up to one)"
    buf = Buf(nb, nh, shape[0], shape[1], rup(shape[1], ve) + (ve if pad else 0), dtype, device, float("nan"), gap=gap)
    if not k_contig:
        buf.flat[:] = randn(gen, tuple(buf.flat.shape), dtype, device, scale)
    val = randn(gen, (nb, nh) + shape, dtype, device, scale)
    last = (signs(gen, (nb, nh) + (shape[:1] if k_contig else shape[1:]), 1.5) * scale).to(dtype).to(device)
    pattern = (sk * scale).to(dtype).to(device)
    if k_contig:
        val[..., -1, :len(sk)] = pattern
        val[..., -1] = last
    else:
        val[..., :len(sk), -1] = pattern
        val[..., -1, :] = last
    buf.view()[:] = val
    return buf


def gemm_case(dtype, layout, M, N, K, *, device="cpu", batch=1, nh=1, alpha=1.0, bias=False, epilogue=0, residual=False, c2=False, c_f32=None,
              accumulate=False, pad=0, gap=0, seed=0, splitk=1):
    """operands of one magic_gemm call in padded storage (see gemm_operand), NaN-filled outputs with `pad` extra columns and `gap` guard rows,
    and the float64 reference.  The last contraction index, the bias and the residual are made large enough that leaving any of them out
    moves an element by more than its bound."""
    g = torch.Generator(device="cpu")
    g.manual_seed(1000003 * seed + 7919 * M + 104729 * N + 31 * K + 3 * layout + batch)
    nb = batch // nh
    c_f32 = (dtype == torch.float32) if c_f32 is None else c_f32
    store = torch.float32 if c_f32 else dtype
    c = {"dtype": dtype, "layout": layout, "M": M, "N": N, "K": K, "batch": batch, "nh": nh, "alpha": alpha, "epilogue": epilogue, "store": store,
         "accumulate": accumulate, "splitk": splitk}
    sk = signs(g, (min(K, 16),), 1.5)
    c["A"] = gemm_operand(g, dtype, device, nb, nh, (M, K) if layout != 2 else (K, M), layout != 2, 1.0, sk, pad, gap)
    c["B"] = gemm_operand(g, dtype, device, nb, nh, (N, K) if layout == 0 else (K, N), layout == 0, 0.125, sk, pad, gap)
    lds = [N + pad * i for i in (1, 2, 3, 4)] if pad else [N]               # C, aux, residual and C2 each get a pitch of their own
    C = Buf(nb, nh, M, N, lds[0], store, device, float("nan"), gap=gap, lds=lds)
    c["C"] = C
    kw = {"alpha": alpha, "epilogue": epilogue}
    if bias:
        c["bias"] = kw["bias"] = offset_randn(g, (N,)).float().to(device)
    if epilogue in (3, 4):
        c["aux"] = C.like(dtype, float("nan"), lds[1 % len(lds)])
        c["aux"].view()[:] = randn(g, (nb, nh, M, N), dtype, device)
        kw["aux"] = c["aux"].view()
    if residual:
        c["residual"] = C.like(store, float("nan"), lds[2 % len(lds)])
        c["residual"].view()[:] = offset_randn(g, (nb, nh, M, N)).to(store).to(device)
        kw["residual"] = c["residual"].view()
    if c2:
        c["C2"] = C.like(dtype, float("nan"), lds[3 % len(lds)])
    if accumulate:
        c["c_in"] = kw["c_in"] = randn(g, (nb, nh, M, N), torch.float32, device)
        C.view()[:] = c["c_in"]
    c["kw"] = kw
    c["ref"] = gemm_ref(layout, c["A"].view(), c["B"].view(), **kw)
    return c


def gemm_defects(c):
    """{name: reference with one planted defect} for a gemm_case: each must FAIL the check that the honest result passes"""
    layout, kw = c["layout"], c["kw"]
    A, B = c["A"].view().to(F64), c["B"].view().to(F64)
    K = c["K"]
    out = {}
    if K > 1:
        out["last_k_missing"] = gemm_ref(layout, *k_slice(layout, A, B, 0, K - 1), **kw)
    a0, b0 = A.clone(), B.clone()
    if layout != 2:
        a0[..., -1, :] = 0
    else:
        a0[..., :, -1] = 0
    if layout == 0:
        b0[..., -1, :] = 0
    else:
        b0[..., :, -1] = 0
    out["last_row_missing"] = gemm_ref(layout, a0, B, **kw)
    out["last_col_missing"] = gemm_ref(layout, A, b0, **kw)
    if "bias" in kw:
        out["bias_missing"] = gemm_ref(layout, A, B, **{**kw, "bias": None})
        out["bias_doubled"] = gemm_ref(layout, A, B, **{**kw, "bias": 2 * kw["bias"]})
    if kw["alpha"] != 1.0:
        out["alpha_one"] = gemm_ref(layout, A, B, **{**kw, "alpha": 1.0})
    if "residual" in kw:
        out["residual_missing"] = gemm_ref(layout, A, B, **{**kw, "residual": None})
    if c.get("splitk", 1) > 1:                                   # the K range of the last split that owns a tile
        lo, hi = [r for r in split_ranges(K, 32 if c["dtype"] == torch.float32 else 64, c["splitk"]) if r[1] > r[0]][-1]
        a1 = A.clone()
        if layout != 2:
            a1[..., lo:hi] = 0
        else:
            a1[..., lo:hi, :] = 0
        out["split_missing"] = gemm_ref(layout, a1, B, **kw)
    if "aux" in kw and c["batch"] > 1:
        flat = kw["aux"].reshape((-1,) + kw["aux"].shape[2:])
        out["neighbour_aux"] = gemm_ref(layout, A, B, **{**kw, "aux": flat.roll(1, 0).reshape(kw["aux"].shape)})
    return out


def dw_operands(dtype, M, N, K, *, device="cpu", seed=0, pad=0):
    """dY [M, N] (pitch lda), X [M, K] (pitch ldb) of one weight-gradient problem: both out-contiguous (TN), padding random; the last row large"""
    g = torch.Generator(device="cpu")
    g.manual_seed(2000003 * seed + 7919 * M + 104729 * N + 31 * K)
    ve = ve_of(dtype)
    lda, ldb = rup(N, ve) + (ve if pad else 0), rup(K, ve) + (ve if pad else 0)
    dy, x = randn(g, (max(M, 1), lda), dtype, device), randn(g, (max(M, 1), ldb), dtype, device, 0.125)
    if M > 0:
        dy[M - 1] = torch.where(dy[M - 1].float() < 0, -1.5, 1.5).to(dtype)
        x[M - 1] = torch.where(x[M - 1].float() < 0, -0.1875, 0.1875).to(dtype)
    return dy, x, lda, ldb


def emulate_dw(parts, dW_in=None, db_in=None, ways=1):
    """fp32 sums row after row over all parts (ways partial sums), then + dW_in"""
    N, K = parts[0][0].shape[1], parts[0][1].shape[1]
    acc = [torch.zeros(N, K) for _ in range(ways)]
    bcc = [torch.zeros(N) for _ in range(ways)]
    i = 0
    for dy, x in parts:
        dy, x = dy.float(), x.float()
        for r in range(dy.shape[0]):
            acc[i % ways] = acc[i % ways] + dy[r][:, None] * x[r][None, :]
            bcc[i % ways] = bcc[i % ways] + dy[r]
            i += 1
    w, b = sum(acc[1:], acc[0]), sum(bcc[1:], bcc[0])
    if dW_in is not None:
        w = w + dW_in.float()
    if db_in is not None:
        b = b + db_in.float()
    return w, b


# ---- the cases both files run ------------------------------------------------------------------------------------------------------------
SWEEP_MN = (1, 63, 64, 65, 129)
SWEEP_K = {16: (8, 64, 72, 136, 200, 456), 32: (4, 32, 36, 100, 228)}     # 1..4 K-tiles, the second trip of the depth-3 pipeline, each with a tail


def bits(dtype):
    return 32 if dtype == torch.float32 else 16


def branch_cases(dtype):
    """(tag, gemm_case keywords) at one ragged shape: every operand branch of gemm_block.  K: one tile and a tail unless the branch needs more"""
    f32 = dtype == torch.float32
    k1, bk = (36, 32) if f32 else (72, 64)
    M, N = 65, 63
    out = [("alpha", dict(layout=0, M=M, N=N, K=k1, alpha=0.375, bias=True)),
           ("alpha_nn_c2", dict(layout=1, M=M, N=N, K=k1, alpha=-1.5, bias=True, c2=True)),
           ("f32_out", dict(layout=0, M=M, N=N, K=k1, bias=True, c_f32=True)),
           ("f32_accumulate_nt", dict(layout=0, M=M, N=N, K=k1, bias=True, c_f32=True, accumulate=True)),
           ("f32_accumulate_nn", dict(layout=1, M=M, N=N, K=k1, c_f32=True, accumulate=True, alpha=0.5)),
           ("f32_residual", dict(layout=0, M=M, N=N, K=k1, bias=True, c_f32=True, residual=True)),
           ("pitches", dict(layout=0, M=M, N=N, K=k1, bias=True, epilogue=1, residual=True, c2=True, pad=8, gap=3)),
           ("pitches_aux", dict(layout=1, M=M, N=N, K=k1, epilogue=3, residual=True, c2=True, pad=8, gap=3)),
           ("gelu_c2", dict(layout=0, M=M, N=N, K=k1, bias=True, epilogue=1, c2=True)),       # no residual: the GPU file measures the erf forms here
           ("dgelu_c2", dict(layout=1, M=M, N=N, K=k1, bias=True, epilogue=3, c2=True)),
           ("relu", dict(layout=0, M=M, N=N, K=k1, bias=True, epilogue=2, residual=True)),
           ("drelu", dict(layout=1, M=M, N=N, K=k1, epilogue=4)),
           ("batched", dict(layout=1, M=37, N=N, K=k1, batch=6, nh=2, epilogue=3, residual=True, c2=True, pad=8, gap=2, bias=True)),
           ("batched_nt", dict(layout=0, M=37, N=N, K=k1, batch=6, nh=2, alpha=0.125, pad=8, gap=2)),
           ("batched_tn", dict(layout=2, M=37, N=N, K=k1, batch=6, nh=2, gap=2)),
           # split-K: bias from split 0 only, atomics into a non-zero C; 5 K-tiles over 4 splits = 3 live splits
           ("splitk2_bias", dict(layout=0, M=M, N=N, K=2 * bk + 8, bias=True, c_f32=True, accumulate=True, splitk=2)),
           ("splitk3_tn", dict(layout=2, M=M, N=N, K=4 * bk + 8, bias=True, c_f32=True, accumulate=True, splitk=3, pad=8)),
           ("splitk4_of_5_tiles", dict(layout=2, M=M, N=N, K=5 * bk, c_f32=True, accumulate=True, splitk=4, bias=True))]
    return out


def form_cases(dtype):
    """(tag, expected form name, gemm_case keywords): the single-launch forms other than the plain 64 x 64 kernel"""
    f32 = dtype == torch.float32
    out = []
    for K in (768, 776, 840):             # kg, 16-bit: 12 K-tiles = 3 full rounds of 4 groups; 13 and 14 leave a last round of 1 and 2 live groups (fp32: 24, 25, 27 tiles)
        out.append((f"kg_nt_{K}", "KG", dict(layout=0, M=65, N=65, K=K, bias=True, epilogue=1, c2=True, residual=True)))
        out.append((f"kg_nn_{K}", "KG", dict(layout=1, M=65, N=65, K=K, bias=True, epilogue=1, c2=True, residual=True)))
    for M in (1024, 1025):                # xcd: 16 row tiles, and 17 padded to 24 (seven surplus row tiles leave at once)
        out.append((f"xcd_nt_{M}", "XCD", dict(layout=0, M=M, N=65, K=8 if not f32 else 4, bias=True)))
        out.append((f"xcd_nn_{M}", "XCD", dict(layout=1, M=M, N=65, K=8 if not f32 else 4, bias=True, epilogue=2)))
    return out


def bias_grad_case(dtype, device="cpu"):
    """TN on the XCD order with the fused bias gradient (17 row tiles): db[m] = sum_k A[k, m] -> (case, Ref db, {defect: Ref db})"""
    c = gemm_case(dtype, 2, 1025, 65, 4 if dtype == torch.float32 else 8, device=device, c_f32=True, seed=3)
    A = c["A"].view()[0, 0]                                              # [K, M]: db = its column sums
    return c, dw_ref([(A, A[:, :1])])[1], {"last_k_missing": dw_ref([(A[:-1], A[:-1, :1])])[1]}


WIDE_SHAPES = ((128, 128, 8, "WIDE"), (136, 264, 72, "WIDE"), (2056, 136, 8, "WIDE_XCD"))


def grouped_cases(dtype):
    """(family, form, placements, [gemm_case keywords per problem]) of the grouped launches: 2, 3 and 8 problems of different shapes; one launch
    per placement; TN with 8 splits, batch 2 and atomics; two long-K problems on the K-group form"""
    f32 = dtype == torch.float32
    k, bk = (36, 32) if f32 else (72, 64)
    shapes = [(65, 63, k), (1, 129, k), (129, 1, 2 * k), (64, 64, k), (63, 65, 8), (37, 70, k), (130, 20, k), (5, 5, 3 * k)]
    out = []
    for n in (2, 3, 8):
        for layout in (0, 1, 2):
            out.append(("grouped", "FORM_GROUPED", ["PLACE_PLAIN"],
                        [dict(layout=layout, M=M, N=N, K=K, bias=True, epilogue=1 if layout == 0 else 0, residual=layout == 1, c2=layout == 0,
                              pad=8 if i % 2 else 0, seed=20 + i) for i, (M, N, K) in enumerate(shapes[:n])]))
    out.append(("grouped", "FORM_GROUPED", ["PLACE_XCD_ROWS", "PLACE_PLAIN"],          # the XCD row order (17 and 16 row tiles) next to a plain problem
                [dict(layout=0, M=1025, N=65, K=8, bias=True, seed=30), dict(layout=0, M=65, N=63, K=k, bias=True, seed=31),
                 dict(layout=0, M=1024, N=129, K=8, seed=32)]))
    out.append(("grouped", "FORM_GROUPED", ["PLACE_SPLIT8", "PLACE_PLAIN"],            # one split per XCD; 9 K-tiles over 8 splits leave 3 splits empty
                [dict(layout=2, M=65, N=63, K=8 * bk + 8, batch=2, c_f32=True, accumulate=True, splitk=8, bias=True, gap=1, seed=33),
                 dict(layout=2, M=63, N=129, K=9 * bk, batch=2, c_f32=True, accumulate=True, splitk=8, seed=34),
                 dict(layout=2, M=20, N=20, K=8 * bk, c_f32=True, accumulate=True, splitk=8, seed=35)]))
    for layout in (0, 1):
        out.append(("grouped kg", "FORM_GROUPED_KG", ["PLACE_PLAIN"],
                    [dict(layout=layout, M=64, N=64, K=K, bias=True, epilogue=1, residual=True, seed=36) for K in (2048, 2056)]))
    return out


# ---- slab mode ---------------------------------------------------------------------------------------------------------------------------------
SLAB_SPLITS, SLAB_ALPHA = 3, 0.5


def slab_cases(dtype):
    """(layout, K): 2 K-tiles over 3 splits leave slab 2 empty; 4 tiles (the last an 8-wide tail) over 3 splits: 2 + 2 + 0"""
    bk = 32 if dtype == torch.float32 else 64
    return [(0, 2 * bk), (1, 3 * bk + 8), (2, 3 * bk + 8)]


def slab_case(dtype, layout, K, device="cpu"):
    c = gemm_case(dtype, layout, 65, 63, K, device=device, c_f32=True, bias=True, pad=8, seed=40)
    bk = 32 if dtype == torch.float32 else 64
    A, B = c["A"].view()[0, 0], c["B"].view()[0, 0]
    c["slab_ref"] = slab_ref(layout, A, B, bk, SLAB_SPLITS, alpha=SLAB_ALPHA, bias=c["bias"])
    c["slab_defects"] = {"split_missing": slab_ref(layout, A, B, bk, SLAB_SPLITS, alpha=SLAB_ALPHA, bias=c["bias"], skip=1),
                         "bias_missing": slab_ref(layout, A, B, bk, SLAB_SPLITS, alpha=SLAB_ALPHA),
                         "alpha_one": slab_ref(layout, A, B, bk, SLAB_SPLITS, bias=c["bias"])}
    c["slab_ranges"] = split_ranges(K, bk, SLAB_SPLITS)
    return c


# ---- magic_gemm_dw_grouped problems ------------------------------------------------------------------------------------------------------------
class DwProb:
    """one weight-gradient problem dW[N, K] += dY[M, N]^T X[M, K] (db[N] += column sums of dY) with its split count; `share`: the earlier
    problem whose dW / db it adds into.  reset() NaN-fills fresh outputs (two guard rows, `pad` extra columns) around the non-zero dW_in / db_in."""

    def __init__(self, dtype, M, N, K, splitk, seed, *, share=None, with_db=True, pad=0, device="cpu"):
        self.M, self.N, self.K, self.splitk, self.device = M, N, K, splitk, device
        self.dy, self.x, self.lda, self.ldb = dw_operands(dtype, M, N, K, device=device, seed=seed, pad=pad)
        self.leader = share or self
        if share is None:
            g = torch.Generator().manual_seed(seed)
            self.ldc = K + pad
            self.w0 = torch.randn(N, K, generator=g).to(device)
            self.b0 = torch.randn(N, generator=g).to(device) if with_db else None
            self.members = [self]
        else:
            share.members.append(self)

    def reset(self):
        self.dW = torch.full((self.N + 2, self.ldc), float("nan"), device=self.device)
        self.dW[:self.N, :self.K] = self.w0
        self.db = None
        if self.b0 is not None:
            self.db = torch.full((self.N + 2,), float("nan"), device=self.device)
            self.db[:self.N] = self.b0

    def parts(self, members=None, cut_last=False):
        ps = [(m.dy[:m.M, :m.N], m.x[:m.M, :m.K]) for m in (members or self.members)]
        if cut_last:
            ps[-1] = (ps[-1][0][:-1], ps[-1][1][:-1])
        return ps

    def refs(self):
        """(Ref dW, Ref db) of the group this problem leads"""
        return dw_ref(self.parts(), self.w0, self.b0)

    def defects(self):
        """{name: (Ref dW, Ref db)}: the last row of the group missing; its last problem missing"""
        bad = {"last_row_missing": dw_ref(self.parts(cut_last=True), self.w0, self.b0)}
        if len(self.members) > 1:
            bad["problem_missing"] = dw_ref(self.parts(self.members[:-1]), self.w0, self.b0)
        return bad


def dw_placement_problems(dtype, device="cpu"):
    """[(problem, the placement it takes alone)]: all four placements of magic_gemm_dw_grouped in one launch of nine problems.  Tiles are
    (N / 64) x (K / 64); bk rows per K-tile."""
    bk = 32 if dtype == torch.float32 else 64
    P = lambda *a, **k: DwProb(dtype, *a, device=device, **k)       # noqa: E731
    return [(P(8 * bk + 8, 65, 24, 8, 50), "PLACE_SPLIT8"),                             # 8 splits, 2 x 1 tiles, the ninth K-tile a tail
            (P(40, 24, 136, 1, 51, with_db=False), "PLACE_XCD_GROUPS"),                 # 1 split, 1 x 3 tiles (nx >= ny)
            (P(2 * bk + 8, 129, 24, 2, 52, pad=8), "PLACE_XCD_GROUPS"),                 # 2 splits, 3 x 1 tiles (nx < ny): 3 is no multiple of 4
            (P(4 * bk, 24, 264, 4, 53), "PLACE_XCD_GROUPS"),                            # 4 splits, 1 x 5 tiles: 5 is no multiple of 2
            (P(5 * bk, 260, 24, 4, 54, with_db=False, pad=8), "PLACE_XCD_GROUPS"),      # 4 splits, 5 x 1 tiles, tall
            (P(3 * bk + 8, 1025, 72, 3, 55), "PLACE_XCD_ROWS"),                         # 3 splits, 17 row tiles padded to 24: seven surplus rows leave
            (P(3 * bk + 8, 63, 24, 3, 56, pad=8), "PLACE_PLAIN"),                       # 3 splits on a single tile
            (P(33, 40, 40, 1, 57), "PLACE_PLAIN"),                                      # 1 split on a single tile: no XCD group to fill
            (P(1, 65, 65, 2, 58), "PLACE_XCD_GROUPS")]                                  # one row, 2 splits (the second empty), 2 x 2 tiles


def dw_shared_problems(dtype, with_db, device="cpu"):
    """one dW shared by three problems with different row counts and split counts (320 rows over 4 splits leave an empty trailing split in the
    16-bit types), ldc = K + 8; next to them a problem of its own"""
    a = DwProb(dtype, 40, 72, 136, 1, 60, with_db=with_db, pad=8, device=device)
    return [a, DwProb(dtype, 320, 72, 136, 4, 61, share=a, pad=8, device=device), DwProb(dtype, 200, 72, 136, 3, 62, share=a, pad=8, device=device),
            DwProb(dtype, 65, 24, 24, 2, 63, device=device)]


# ---- magic_gemm_dw_cat problems ----------------------------------------------------------------------------------------------------------------
DW_CAT_ROWS = (65, 0, 1, 200)


class DwCatProb:
    """dW[N, K] += sum over four row segments; segs: dw_operands tuples; rows all 0: dW and db must stay bit for bit"""

    def __init__(self, dtype, N, K, rows, seed0, device):
        self.N, self.K, self.rows, self.device = N, K, rows, device
        live = any(rows)
        self.segs = [dw_operands(dtype, m if live else 3, N, K, device=device, seed=seed0 + i, pad=8 if live and (N + K) % 16 else 0)
                     for i, m in enumerate(rows)]
        g = torch.Generator().manual_seed(N * 1000 + K)
        self.w0, self.b0 = torch.randn(N, K, generator=g).to(device), torch.randn(N, generator=g).to(device)
        self.parts = [(s[0][:m, :N], s[1][:m, :K]) for s, m in zip(self.segs, rows)]

    def refs(self):
        return dw_ref(self.parts, self.w0, self.b0)

    def defects(self):
        p = self.parts
        return {"segment_missing": dw_ref(p[:2] + p[3:], self.w0, self.b0), "first_segment_missing": dw_ref(p[1:], self.w0, self.b0),
                "last_row_missing": dw_ref(p[:3] + [(p[3][0][:-1], p[3][1][:-1])], self.w0, self.b0), "dW_in_missing": dw_ref(p, None, None)}


def dw_cat_problems(dtype, wide, device="cpu"):
    """every (N, K) of the narrow (24, 72, 136) or wide (128, 136, 264) set with rows 65 / 0 / 1 / 200, then one problem whose segments are all empty"""
    dims = (128, 136, 264) if wide else (24, 72, 136)
    out = [DwCatProb(dtype, N, K, DW_CAT_ROWS, 70, device) for N in dims for K in dims]
    out.append(DwCatProb(dtype, dims[1], dims[0], (0, 0, 0, 0), 80, device))
    return out


# ---- magic_linear_ln / magic_linear_act_ln problems --------------------------------------------------------------------------------------------
LLN_H, LLN_M, LLN_EPS = (128, 256, 384), (1, 31, 32, 33, 65), 1e-12
LLN_K = {16: (8, 72, 200), 32: (4, 36, 100)}
LLN_PAIR = ((33, 91, True), (65, 92, False))            # (M, seed, with residual) of the two sides of a pair launch


def lln_operands(dtype, M, H, K, seed, device="cpu"):
    """x [M, K], W [H, K] with one extra vector of NaN pad columns (K is a vector multiple: nothing past K may be read), bias, gamma, beta and
    a residual; the last k is +-1.5 * 0.1875 in every element so that leaving it out shows"""
    g = torch.Generator().manual_seed(seed * 7919 + M * 31 + H + K)
    ld = rup(K, ve_of(dtype)) + ve_of(dtype)
    assert K % ve_of(dtype) == 0
    x, W = (torch.full((r, ld), float("nan"), dtype=dtype, device=device) for r in (M, H))
    x[:, :K], W[:, :K] = randn(g, (M, K), dtype, device), randn(g, (H, K), dtype, device, 0.125)
    x[:, K - 1] = 1.5
    W[:, K - 1] = signs(g, (H,), 0.1875).to(dtype).to(device)
    bias = offset_randn(g, (H,)).to(device)
    gamma, beta = (1 + 0.1 * torch.randn(H, generator=g)).to(device), (0.1 * torch.randn(H, generator=g)).to(device)
    res = randn(g, (M, H), dtype, device)
    return x, W, bias, gamma, beta, res


def lln_refs(dtype, K, ops, act, with_res, act_a):
    """(Ref out, Ref rstd, Ref pre-activation) and {defect: Ref out}"""
    x, W, bias, gamma, beta, res = ops
    args = dict(residual=res if with_res else None, act=act, act_a=act_a)
    good = linear_ln_ref(x[:, :K], W[:, :K], bias, gamma, beta, LLN_EPS, dtype, **args)
    bad = {"last_k_missing": linear_ln_ref(x[:, :K - 1], W[:, :K - 1], bias, gamma, beta, LLN_EPS, dtype, **args)[0],
           "bias_missing": linear_ln_ref(x[:, :K], W[:, :K], None, gamma, beta, LLN_EPS, dtype, **args)[0],
           "bias_doubled": linear_ln_ref(x[:, :K], W[:, :K], 2 * bias, gamma, beta, LLN_EPS, dtype, **args)[0]}
    if with_res:
        bad["residual_missing"] = linear_ln_ref(x[:, :K], W[:, :K], bias, gamma, beta, LLN_EPS, dtype, **{**args, "residual": None})[0]
    return good, bad


def emulate_linear_ln(x, W, bias, gamma, beta, eps, store, *, residual=None, act=0):
    """fp32 throughout: the k-after-k product, the activation, the residual, two-pass statistics, the affine map; outputs rounded to `store`
    -> (out, rstd fp32, pre-activation)"""
    v, _ = emulate_gemm(0, x, W, 1, bias=bias)
    pre = v
    if act == 1:
        v = 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752))
    elif act == 2:
        v = v.clamp_min(0.0)
    if residual is not None:
        v = v + residual.float()
    mu = v.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((v - mu) ** 2).mean(-1, keepdim=True) + torch.tensor(eps, dtype=torch.float32))
    out = (v - mu) * rstd * gamma.float() + beta.float()
    return out.to(store), rstd.squeeze(-1), pre.to(store)
