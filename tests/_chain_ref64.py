"""float64 references of the teacher's row chain (csrc/chain.hip: chain_fwd_kernel on 32-row tiles, chain64_fwd_kernel on 64-row tiles), their
bounds, the seeded case table and an fp32 emulation, shared by tests/test_chain_ref64_cpu.py and tests/test_chain_fp64_gpu.py -- so the CPU file
proves on the SAME inputs that the honest dataflow passes every bound and that every planted defect fails one.  Nothing here launches a kernel;
everything works on whatever device the operands live on.

    y1   = LayerNorm(x Wa^T + ba + res)                    proj = y_last Wp^T + bp
    y2   = LayerNorm(gelu(y1 W1^T + bi) W2^T + bo2 + y1)

Stage by stage (the rule of tests/test_encoder_fp64_gpu.py): each output is recomputed in float64 from the 16-bit values the kernel itself
stored as that stage's input, weights upcast from their 16-bit values, so every stage carries its own roundings only.
  y1    from x, res: linear_ln_ref(..., residual=res) of tests/_gemm_ref64.py, its 16-bit rule: 1 ulp of |ref| + 0.003 ulp of the row's rms.
  proj  from the stored y_last: gemm_ref with bound() = (K + 8) 2^-23 E + ulp.
  y2    from the stored y1.  The GELU output never leaves the CU, so this stage carries two roundings and its bound is derived, not measured:
          z = y1 W1^T + bi                 D_z = (256 + 8) 2^-23 (|y1| |W1|^T + |bi|)
          g = gelu_erf(z)                  dG  = D_z max(1, |gelu'(z)|) + |gelu_as(z) - g| + |z| 2^-21 + 1/2 ulp(|g| + the terms before)
          t = g W2^T + bo2 + y1            D_t = dG |W2|^T + (1024 + 8) 2^-23 (|g| |W2|^T + |bo2| + |y1|)
        D_t goes through the normalisation to first order as in linear_ln_ref (ln_carry):
          P_i = |g2_i| rstd (D_i + mean D + |xhat_i| mean(|xhat| D)),
        plus the remainder of that expansion.  With t' = t + d, |d_i| <= D_i, c = t - mean t, e = d - mean d (|e_i| <= A_i = D_i + mean D),
        s^2 = var + eps, rstd = 1 / s, xhat = c rstd:
          s'^2 = s^2 (1 + u),   u = 2 rstd mean(xhat d) + rstd^2 mean(e^2)        (mean(xhat e) = mean(xhat d) because mean(xhat) = 0)
          -L <= u <= U,         L = 2 rstd mean(|xhat| D),  U = L + rstd^2 mean(D^2)   (mean(e^2) <= mean(d^2) <= mean(D^2))
          out' - out = g2 rstd ((c + e)(1 + u)^-1/2 - c),   (1 + u)^-1/2 = 1 - u / 2 + rho(u),  |rho| <= 3/8 U^2 (1 - L)^-5/2   (Taylor, L < 1)
                     = g2 rstd (e - xhat mean(xhat d))                                       <- first order, bounded by P
                       + g2 rstd (-xhat rstd mean(e^2) / 2 + c rho + e ((1 + u)^-1/2 - 1))   <- the remainder
          R_i = |g2_i| (1/2 |xhat_i| rstd^2 mean(D^2) + 3/8 |xhat_i| U^2 (1 - L)^-5/2 + rstd A_i max((1 - L)^-1/2 - 1, U / 2)).
        In bf16 D_t / sigma reaches ~ 3 % (the worst-case sum of 1024 half-ulps of g) and R is ~ L of P; in fp16 both are 8 times smaller.
        On top, the 16-bit LayerNorm rule for the final rounding: 1 ulp of |ref| + 0.003 ulp of the row's rms.  No fitted factor anywhere.

Inputs (operands): rows of x and res scaled row by row by powers of two over 2^-6 .. 2^3 (a fixed cycle, row 0 at 1 and 1 so that M = 1 is an
ordinary row) around a per-row non-zero mean, random content (every row distinct), weights N(0, 1 / K) rounded to storage, every bias and beta
offset_randn plus a common offset of 0.75, its last 16-column tile tripled (a LayerNorm partial lost from a statistic then moves y2 by more than
the bf16 bound of the two-rounding stage; doubled, the lost mean stayed inside it at M = 1), gammas of both signs with |gamma| in [0.5, 1.5).
x is the column slice [:, H:2H] of an [M, 3H] buffer whose other columns are NaN.

Planted defects (emulate(..., defect=...)); each fails the bound of the output named, at every M it applies to (tests/test_chain_ref64_cpu.py):
  ka / k1 / k2 / kp      the last k-step (32 of K) of the product with Wa / W1 / W2 / Wp dropped              -> y1 / y2 / y2 / proj
  chunk                  the last 256-column chunk of the intermediate dropped                                  -> y2
  ba_nb / bi_nb / bp_nb  the bias read at the neighbouring 16-column tile                                       -> y1 / y2 / proj
  mean1 / var1 / mean2 / var2   the statistic summed over 240 of 256 columns (the last 16-column partial lost)  -> y1 / y2
  swap_y1 / swap_y2 / swap_proj  rows 0 and 1 of the first tile exchanged on the way out (M >= 2: with M = 1 there is no second row)
  res_x                  y2's residual taken from x instead of y1                                               -> y2
  proj_off               a projection pass writes its 256 columns at the previous pass's offset (Np >= 512; the last 256 stay unwritten) -> proj
  gelu_trunc             the GELU output truncated instead of rounded.  NOT CATCHABLE by a worst-case bound at any shape: truncation doubles the
                         half-ulp term of dG on single elements, but what reaches y2 is sum_k err_k W2[n, k] over 1024 terms with weights of
                         both signs -- a random walk of ~ 0.6 ulp(g) rms, some 30 times below the 1/2 ulp(g) |W2|^T allowance that an honest
                         kernel may use up with aligned signs.  The CPU file prints its err / bound and asserts only that it stays listed.

Measured on an MI355X (tests/test_chain_fp64_gpu.py::test_zz_report, -s) over every case: worst err / bound, and worst |err| in ulps of |ref|
over the elements with |ref| >= their row's rms; 32-row kernel | 64-row kernel:
  y1    bf16 0.499, 0.50 ulp | 0.499, 0.50 ulp      fp16 0.499, 0.50 ulp | 0.499, 0.50 ulp
  y2    bf16 0.170, 1.14 ulp | 0.170, 1.14 ulp      fp16 0.077, 1.14 ulp | 0.078, 1.14 ulp
  proj  bf16 0.493, 0.50 ulp | 0.493, 0.50 ulp      fp16 0.446, 0.50 ulp | 0.445, 0.50 ulp
(the honest CPU emulation: y1 0.499, y2 0.170 / 0.078, proj 0.493 / 0.445 -- the kernels sit where an honest fp32 dataflow sits.)
Scratch builds of csrc/chain.hip, never committed, against the GPU file: the 64-row projection bias read at the previous pass's 256 columns
(proj fails at Np >= 512), the 64-row GELU image's row mapping off in one tile of one chunk (y2 fails wherever a row past 32 exists), the
64-row mean folded over 15 of 16 partials (y1 fails in every case), the 32-row projection bias of one tile from its neighbour (proj fails),
the 32-row barrier between the GELU image's writes and reads removed (y2 differs between two launches or is not finite), the 32-row y2 copied
out one row too many (guard row written at M < 32).  NOT caught: the 64-row GELU and projection images no longer alternated between sG and
sRes -- the "one barrier too early" race needs a wave a whole product phase ahead of another, which neither the 241 cases here (1 - 4
workgroups) nor the 3840-row launches of tests/test_chain_gpu.py ever showed; a numeric test cannot provoke it, the alternation stays an
argument in the kernel's comments.
"""
import math
import types

import torch

from tests import _gemm_ref64 as R
from tests._gemm_ref64 import F64, LN_FLOOR, LN_ULPS, UNIT, dgelu, gelu, gemm_ref, linear_ln_ref, ln_carry, offset_randn, ulp
from tests.test_encoder_fp64_gpu import gelu_as

H, I, EPS = 256, 1024, 1e-12
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
TILE_ROWS = (32, 64)

# (ffn, Np, y1 stored): every valid combination -- "nothing written" (no FFN, no projection, y1 NULL) is refused by magic_chain_fwd
FORMS = [(f, n, s) for f in (True, False) for n in (0, 256, 512, 768) for s in (True, False) if f or n or s]
PRODUCTION = [(True, 768, False), (True, 0, False), (False, 256, True)]        # host/engine.py's three launches
EDGE_FORMS = PRODUCTION + [(True, 768, True)]
M_ALL, M_EDGE = (33, 65), (1, 31, 32, 63, 64, 97)
# (ffn, Np, y1 stored, M, x is the strided column slice)
CASES = [(f, n, s, M, (f, n, s) in PRODUCTION) for (f, n, s) in FORMS for M in M_ALL] + \
        [(f, n, s, M, (f, n, s) in PRODUCTION) for (f, n, s) in EDGE_FORMS for M in M_EDGE]
ROWS = tuple(sorted(set(M_ALL + M_EDGE)))
# paired launches: (Ma, Mb), and the two problems' (ffn, Np, y1 stored, strided) in both orders
PAIR_ROWS = ((33, 1), (64, 1), (1, 65))
PAIR_FORMS = (((True, 768, False, True), (False, 256, True, False)), ((False, 512, False, False), (True, 256, True, True)))


def case_id(c):
    f, n, s, M, st = c
    return f"{'ffn' if f else 'noffn'}-np{n}-{'y1' if s else 'noy1'}-M{M}{'-strided' if st else ''}"


# ---- seeded operands ----------------------------------------------------------------------------------------------------------------------------
_EXP = (0, 3, -6, -3, 1, -5, 2, -4, -1, -2)
_W, _OPS = {}, {}


def weights(dtype, device="cpu"):
    key = (dtype, str(device))
    if key not in _W:
        g = torch.Generator().manual_seed(20250 + (dtype == torch.float16))
        w = types.SimpleNamespace()
        for name, (n, k) in dict(Wa=(H, H), W1=(I, H), W2=(H, I), Wp=(3 * H, H)).items():
            setattr(w, name, (torch.randn(n, k, generator=g) / math.sqrt(k)).to(dtype).to(device))
        for name, n in dict(ba=H, bi=I, bo2=H, bp=3 * H, b1=H, b2=H).items():
            b = offset_randn(g, (n,)) + 0.75
            b[-16:] *= 3.0                                   # the tile whose loss from a LayerNorm statistic has to show
            setattr(w, name, b.float().to(device))
        for name in ("g1", "g2"):
            mag = 0.5 + torch.rand(H, generator=g)
            setattr(w, name, torch.where(torch.randn(H, generator=g) < 0, -mag, mag).float().to(device))
        _W[key] = w
    return _W[key]


def operands(dtype, M, device="cpu"):
    """the weights and M rows of x (inside its NaN-framed [M, 3H] buffer: .x_full, .x = x_full[:, H:2H]; .x_flat a contiguous copy) and res"""
    key = (dtype, M, str(device))
    if key not in _OPS:
        g = torch.Generator().manual_seed(7919 * M + 31 * (dtype == torch.float16))
        o = types.SimpleNamespace(**vars(weights(dtype, device)))
        r = torch.arange(M)
        ex = torch.tensor(_EXP)[r % 10].double()
        er = torch.tensor(_EXP)[(r // 10 + 7 * r) % 10].double()
        mean = lambda: torch.where(torch.randn(M, 1, generator=g) < 0, -1.0, 1.0) * (0.5 + torch.rand(M, 1, generator=g))   # noqa: E731
        x = (torch.randn(M, H, generator=g) + mean()) * (2.0 ** ex)[:, None]
        res = (torch.randn(M, H, generator=g) + mean()) * (2.0 ** er)[:, None]
        o.x_full = torch.full((M, 3 * H), float("nan"), dtype=dtype, device=device)
        o.x_full[:, H:2 * H] = x.to(dtype).to(device)
        o.x = o.x_full[:, H:2 * H]
        o.x_flat = o.x.contiguous()
        o.res = res.to(dtype).to(device)
        o.dtype, o.M = dtype, M
        _OPS[key] = o
    return _OPS[key]


# ---- float64 references -----------------------------------------------------------------------------------------------------------------------
def y1_ref(o, k_hi=H):
    """k_hi < H: the control that lacks the product's last k-steps"""
    return linear_ln_ref(o.x[:, :k_hi], o.Wa[:, :k_hi], o.ba, o.g1, o.b1, EPS, o.dtype, residual=o.res)[0]


def proj_ref(o, y_last, Np, k_hi=H):
    return gemm_ref(0, y_last[:, :k_hi], o.Wp[:Np, :k_hi], bias=o.bp[:Np])


def y2_ref(o, y1, k1=H, k2=I):
    """from the STORED y1 (see the module docstring for the bound).  k1 < H / k2 < I: the controls that lack the last k-steps of the first
    product / the last intermediate columns"""
    store = o.dtype
    y1 = y1.to(F64)
    W1, W2 = o.W1.to(F64), o.W2.to(F64)
    zr = gemm_ref(0, y1[:, :k1], W1[:, :k1], bias=o.bi)
    z = zr.val
    Dz = (H + 8) * UNIT * zr.env
    g = gelu(z)
    before = Dz * dgelu(z).abs().clamp_min(1.0) + (gelu_as(z) - g).abs() + z.abs() * 2.0 ** -21
    dG = before + 0.5 * ulp(g.abs() + before, store)
    g, dG, W2 = g[:, :k2], dG[:, :k2], W2[:, :k2]
    bo2 = o.bo2.to(F64)
    t = g @ W2.t() + bo2 + y1
    Dt = dG @ W2.abs().t() + (I + 8) * UNIT * (g.abs() @ W2.abs().t() + bo2.abs() + y1.abs())
    g2 = o.g2.to(F64)
    out, rstd, xhat, prop = ln_carry(t, Dt, g2, o.b2.to(F64), EPS)
    L = 2.0 * rstd * (xhat.abs() * Dt).mean(-1, keepdim=True)
    assert float(L.max()) < 0.5, "the expansion of the y2 bound needs 2 rstd mean(|xhat| D) well below 1"
    m2 = (Dt * Dt).mean(-1, keepdim=True)
    U = L + rstd * rstd * m2
    A = Dt + Dt.mean(-1, keepdim=True)
    rem = g2.abs() * (0.5 * xhat.abs() * rstd * rstd * m2 + 0.375 * xhat.abs() * U * U * (1.0 - L) ** -2.5
                      + rstd * A * torch.maximum((1.0 - L) ** -0.5 - 1.0, 0.5 * U))
    rms = out.pow(2).mean(-1, keepdim=True).sqrt()
    extra = prop + rem + (LN_ULPS - 1.0) * ulp(out, store) + LN_FLOOR * ulp(rms, store).expand_as(out)
    r = R.Ref(out, torch.zeros_like(out), 0, extra=extra)
    r.t, r.Dt, r.carry = t, Dt, prop + rem                             # (the CPU file checks the expansion on perturbed t)
    r.carried = ((prop + rem) * rstd / g2.abs()).max().item()          # the carried input bound in units of the row's sigma (reported)
    return r


def stage_refs(o, ffn, Np, y1, y2):
    """{output: Ref} of one launch from the stored stage inputs (y1 / y2: the kernel's or the emulation's stored tensors)"""
    out = {"y1": y1_ref(o)}
    if ffn:
        out["y2"] = y2_ref(o, y1)
    if Np:
        out["proj"] = proj_ref(o, y2 if ffn else y1, Np)
    return out


def control_refs(o, ffn, Np, y1, y2):
    """{output: [Ref]}: references that lack the last k-step (32 of K) of that stage's product(s): each must FAIL the check"""
    out = {"y1": [y1_ref(o, H - 32)]}
    if ffn:
        out["y2"] = [y2_ref(o, y1, k1=H - 32), y2_ref(o, y1, k2=I - 32)]
    if Np:
        out["proj"] = [proj_ref(o, y2 if ffn else y1, Np, H - 32)]
    return out


def ratio(got, ref, store):
    """worst |got - ref| / bound(ref, store) of tests/_gemm_ref64.py (inf when got is not finite somewhere); <= 1 passes"""
    return R.ratio(got, ref, store)


def ulps(got, ref, store):
    """worst |got - ref| in ulps of |ref| over the elements with |ref| >= their row's rms (the figure of tests/test_encoder_fp64_gpu.py)"""
    big = ref.val.abs() >= ref.val.pow(2).mean(-1, keepdim=True).sqrt()
    return ((got.to(F64) - ref.val).abs() / ulp(ref.val, store))[big].max().item()


# ---- fp32 emulation with the kernel's rounding points ------------------------------------------------------------------------------------------
DEFECTS = {"ka": "y1", "k1": "y2", "k2": "y2", "kp": "proj", "chunk": "y2", "ba_nb": "y1", "bi_nb": "y2", "bp_nb": "proj",
           "mean1": "y1", "var1": "y1", "mean2": "y2", "var2": "y2", "swap_y1": "y1", "swap_y2": "y2", "swap_proj": "proj",
           "res_x": "y2", "proj_off": "proj"}
UNCATCHABLE = {"gelu_trunc": "y2"}


def _mm(a, W, step, lo=0, hi=None):
    """sum over k-steps of `step` of a[:, k ..] W[:, k ..]^T, fp32"""
    hi = a.shape[1] if hi is None else hi
    acc = torch.zeros(a.shape[0], W.shape[0], dtype=torch.float32)
    for k in range(lo, hi, step):
        acc = acc + a[:, k:k + step].float() @ W[:, k:k + step].float().t()
    return acc


def _norm(acc, bias, res, gamma, beta, width, lose_mean, lose_var, store):
    """two-pass LayerNorm in fp32 with partials of `width` columns folded one after the other (lose_*: the last 16 columns missing from a sum)"""
    v = acc + (bias.float() + res.float())

    def fold(t, lose):
        if lose:
            t = t.clone()
            t[:, H - 16:] = 0.0
        parts = t.view(t.shape[0], H // width, width).sum(-1)
        s = torch.zeros(t.shape[0], dtype=torch.float32)
        for q in range(H // width):
            s = s + parts[:, q]
        return (s * torch.tensor(1.0 / H, dtype=torch.float32))[:, None]
    d = v - fold(v, lose_mean)
    rstd = torch.rsqrt(fold(d * d, lose_var) + torch.tensor(EPS, dtype=torch.float32))
    return (d * rstd * gamma.float() + beta.float()).to(store)


def _trunc(t, store):
    """round toward zero to `store`"""
    r = t.to(store)
    over = r.float().abs() > t.abs()
    bits = r.view(torch.int16)
    return torch.where(over, (bits - 1).view(store), r)


def _nb(b):
    return torch.roll(b, -16)


def _swap(t):
    t = t.clone()
    t[[0, 1]] = t[[1, 0]]
    return t


def emulate(o, order, ffn=True, Np=768, defect=None):
    """the chain in fp32 with the kernel's rounding points (y1, the GELU output, y2 and proj rounded to storage; gelu_as in fp32).
    order 32: k in steps of 32, LayerNorm partials of 32 columns folded over 8 waves (chain_fwd_kernel);
    order 16: k in steps of 16, 16 partials of 16 columns, the FFN accumulated over four 256-column chunks (chain64_fwd_kernel).
    -> {"y1", "y2", "proj"} as the kernel would store them (the stage inputs of the next stage are the UNSWAPPED stored values)"""
    st, d = o.dtype, defect
    assert d is None or d in DEFECTS or d in UNCATCHABLE
    x, res = o.x.cpu(), o.res.cpu()
    y1 = _norm(_mm(x, o.Wa, order, hi=H - 32 if d == "ka" else H), _nb(o.ba) if d == "ba_nb" else o.ba, res, o.g1, o.b1, order,
               d == "mean1", d == "var1", st)
    out = {"y1": _swap(y1) if d == "swap_y1" else y1}
    last = y1
    if ffn:
        bi = _nb(o.bi) if d == "bi_nb" else o.bi
        rnd = (lambda t: _trunc(t, st)) if d == "gelu_trunc" else (lambda t: t.to(st))
        k1 = H - 32 if d == "k1" else H
        k2 = I - 32 if d == "k2" else I - 256 if d == "chunk" else I
        if order == 32:
            g = rnd(gelu_as(_mm(y1, o.W1, 32, hi=k1) + bi.float()))
            acc = _mm(g, o.W2, 32, hi=k2)
        else:
            acc = torch.zeros(o.M, H, dtype=torch.float32)
            for c in range(4):
                cols = slice(256 * c, 256 * c + 256)
                g = rnd(gelu_as(_mm(y1, o.W1[cols], 16, hi=k1) + bi[cols].float()))
                hi = min(256, k2 - 256 * c)
                for k in range(0, hi, 16):
                    acc = acc + g[:, k:k + 16].float() @ o.W2[:, 256 * c + k:256 * c + k + 16].float().t()
        y2 = _norm(acc, o.bo2, x if d == "res_x" else y1, o.g2, o.b2, order, d == "mean2", d == "var2", st)
        out["y2"] = _swap(y2) if d == "swap_y2" else y2
        last = y2
    if Np:
        bp = _nb(o.bp[:Np]) if d == "bp_nb" else o.bp[:Np]
        p = (_mm(last, o.Wp[:Np], order, hi=H - 32 if d == "kp" else H) + bp.float()).to(st)
        if d == "proj_off":
            assert Np >= 512
            q = torch.full_like(p, float("nan"))
            for j in range(Np // 256):
                q[:, 256 * max(j - 1, 0):256 * max(j - 1, 0) + 256] = p[:, 256 * j:256 * j + 256]
            p = q
        out["proj"] = _swap(p) if d == "swap_proj" else p
    return out


# ---- mirrors of the host-visible rules -----------------------------------------------------------------------------------------------------------
def frag_order(W):
    """[N, K] -> the elements in MFMA-fragment order (include/magic_hip.h): fragments (nt, ks) of 16 rows x 32 columns, 64 lanes x 8 elements each"""
    N, K = W.shape
    return W.reshape(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)


def launch_rule(cfg, Ma, Mb, cus):
    """launch_chain: cfg 1 = by size (more 32-row tiles than CUs -> 64-row tiles), 32 | 64 = forced -> (rows, tiles a, tiles b, split)"""
    t32 = (Ma + 31) // 32 + ((Mb + 31) // 32 if Mb else 0)
    rows = (64 if t32 >= cus + 1 else 32) if cfg == 1 else cfg
    ta, tb = (Ma + rows - 1) // rows, ((Mb + rows - 1) // rows if Mb else 0)
    return rows, ta, tb, ta
