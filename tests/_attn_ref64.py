"""float64 reference of the fused attention kernels (csrc/attention.hip), their error bounds, the Python mirrors of the C launch rules, an
fp32 / 16-bit emulation of the kernels' dataflow with its planted defects, and the seeded case table that tests/test_attn_ref64_cpu.py and
tests/test_attn_fp64_gpu.py share -- so the CPU file proves on the SAME inputs that the bounds pass an honest result and catch every planted
defect.  Everything here runs on CPU tensors; nothing launches a kernel.

Reference: oracle/layer_ref.py (`probs`, `dropped`, `context`) in float64 from the values the kernel reads (the stored 16-bit / fp32 q, k, v,
dO, the uint8 key mask, fp32 dist, sprel_w / sprel_b, fp32 dP_init) and the kernel's own dropout mask.  Each output is checked as a STAGE
from saved inputs, so it carries one rounding (the rule of tests/test_encoder_fp64_gpu.py): P and Pd from q, k, mask, dist; ctx = the fp64
product of the kernel's STORED Pd (P without dropout) with v; dQ / dK / dV = pure math on the stored P, q, k, v, dO, dP_init:

    dP = (dO V^T + dP_init) m      dS = scale P (dP - rowsum(P dP))      dQ = dS K      dK = dS^T Q      dV = (P m)^T dO

Forward bounds.  16-bit storage: |k - ref| <= 1 ulp(|ref|) + 0.003 ulp(rms of the ref's row) (BOUNDS of test_encoder_fp64_gpu.py).  fp32
storage: ctx within (Nk + 8) 2^-23 sum |P||v| (the tests/_gemm_ref64.py envelope); P within
    (EXPF_A (1 + |s - max|) + 2 (64 + 8) E_S) 2^-23 P,     E_S = scale sum|q||k| + |sprel_w dist| + |sprel_b|
where the second term is the softmax-propagated error of the fp32 score and EXPF_A (1 + |s - max|) 2^-23 allows for __expf (argument
scaling by log2 e, v_exp_f32), the row sum and the reciprocal.  EXPF_A cannot be derived: it is measured (MEASURE in the GPU file).
Pad columns Nk <= c < ldp are exactly 0.

Backward bounds, per element, derived (u = one storage ulp, 0 for fp32 storage; the kernels round dS and P m to storage before the second
products):
    bound(dQ) = sum_k (u(dS[q,k]) + d32[q,k]) |K[k]| + (Nk + 8) 2^-23 sum_k |dS||K| + u(ref)
    d32[q,k]  = (64 + Nk + 16) 2^-23 scale P (sum_d |dO||v| + |dP_init| + sum_k' P |dP|)
    bound(dK) : the same with Q for K and the sum over queries;   bound(dV) = sum_q u(Pd)|dO| + (Nq + 8) 2^-23 sum |Pd||dO| + u(ref)
    key-split backward: d32 += scale P sum_d u(O_d) |dO_d| (its row sum is dO . O from the stored 16-bit O);  accumulate_kv: + u(base + ref).
No slack factors.  An honest emulation sits at about a third of these bounds.
`tile_rel` is the rel-L2 per (batch, head, 16-row tile) of tests/test_encoder_fp64_gpu.check_dx_tiles, asserted at TILE_REL.

Measured on MI355X over every case of the table, single launches and pair forms (tests/test_attn_fp64_gpu.py with MEASURE = True, -s):
  forward stages, worst |k - ref| / ulp(|ref|) where |ref| >= the row's rms, and the floor needed beyond 1 ulp, in row-rms ulps:
      bf16  P, Pd, ctx 0.5000, floor <= 6.4e-6 (ctx of the key-split kernel)        fp16  P 0.5004, Pd 0.5003, ctx 0.5003, floor 0
      every kernel rounds its fp32 result once: 1 ulp is 2 x the worst.
  fp32 forward: error / ((1 + |s - max|) 2^-23 P) <= 10.24 (two-pass kernel; 9.04 short); beyond the derived score term the excess is 0 in
      every case.  EXPF_A = 20.5 = 2 x 10.24.  ctx at <= 0.10 of its envelope.
  backward envelope ratio |k - ref| / bound, worst per output:
      magic_attn_bwd     bf16 dQ 0.445 dK 0.404 dV 0.371     fp16 dQ 0.393 dK 0.397 dV 0.402     fp32 dQ 0.0068 dK 0.0051 dV 0.062
      magic_attn_bwd_ks  bf16 dQ 0.194 dK 0.484 dV 0.489     fp16 dQ 0.172 dK 0.486 dV 0.490
  tile rel-L2, worst: bf16 3.19e-3 (key-split dK; 3.14e-3 dQ of the 8-wave backward), fp16 4.09e-4 (key-split dK), fp32 3.75e-7 (dQ of the
      4-wave backward).  TILE_REL = 2.5 x these.

The key-split backward walks the queries in tiles of 64 and keeps dK / dV in the 16-bit buffers between tiles; for Nq > 64 it carries each
element's rounding residual into the next tile's sum, so the stored value is the fp32 sum over all tiles and the accumulate base rounded
once -- which is what the bounds model.  `emulate_bwd` does the same, tile by tile.
"""
import zlib
from types import SimpleNamespace

import torch

import oracle.layer_ref as LR

F64 = torch.float64
UNIT = 2.0 ** -23
HD = 64
SCALE = 0.125
SPREL = (0.2, -0.1)
FWD_ULPS, FWD_FLOOR = 1.0, 0.003        # tests/test_encoder_fp64_gpu.py BOUNDS
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}

EXPF_A = 20.5                            # 2 x the measured worst 10.24 (module docstring)
TILE_REL = {"bf16": 8.0e-3, "fp16": 1.02e-3, "fp32": 9.4e-7}     # 2.5 x the measured worst 3.19e-3 / 4.09e-4 / 3.75e-7 (module docstring)


def rup(n, m):
    return (n + m - 1) // m * m


def is16(dtype):
    return dtype != torch.float32


def ulp(x, dtype):
    """unit in the last place of |x| in a 16-bit storage type (subnormals: the smallest normal's); 0 for fp32 storage"""
    if dtype == torch.float32:
        return torch.zeros_like(x)
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    _, e = torch.frexp(x.abs().clamp_min(1e-300))
    return torch.ldexp(torch.ones_like(x), (e - 1).clamp_min(emin) - mant)


def ulp_one(dtype):
    return {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 2.0 ** -23}[dtype]


def heads(t, nh):
    """[B, N, nh * 64] -> [B, nh, N, 64]"""
    B, N, _ = t.shape
    return t.reshape(B, N, nh, HD).transpose(1, 2)


def unheads(t):
    B, nh, N, _ = t.shape
    return t.transpose(1, 2).reshape(B, N, nh * HD)


# ---- mirrors of the C launch rules (csrc/attention.hip) ------------------------------------------------------------------------------
LDS_MAX = 160 * 1024


def _lds_consts(dtype):
    return (72, 8, 2) if is16(dtype) else (68, 4, 4)          # DS, PPAD, bytes per element


def fwd_lds(dtype, Nk):
    DS, PP, sz = _lds_consts(dtype)
    NKP = rup(Nk, 32)
    return (64 * DS + 2 * NKP * DS + 64 * (NKP + PP)) * sz


def bwd_alias(dtype, Nq, Nk):
    DS, PP, _ = _lds_consts(dtype)
    NQP, NKP = rup(Nq, 32), rup(Nk, 32)
    return NQP <= 64 and NQP * (NKP + PP) <= NKP * DS


def bwd_lds(dtype, Nq, Nk):
    DS, PP, sz = _lds_consts(dtype)
    NQP, NKP = rup(Nq, 32), rup(Nk, 32)
    return (2 * NQP * DS + 2 * NKP * DS + (1 if bwd_alias(dtype, Nq, Nk) else 2) * NQP * (NKP + PP)) * sz


def attn_supported(dtype, Nq, Nk, backward):
    """magic_attn_supported (backward: 0 forward, 1 magic_attn_bwd, 2 magic_attn_bwd_ks)"""
    if Nk <= 0 or Nq <= 0:
        return False
    if backward == 2:
        return is16(dtype) and 128 < Nk <= 512
    if backward:
        return Nk <= 128 and Nq <= 128 and bwd_lds(dtype, Nq, Nk) <= LDS_MAX
    if Nk > 128:
        return Nk <= 512
    return fwd_lds(dtype, Nk) <= LDS_MAX


def bwd_waves8(Nq, Nk):
    return Nq > 64 or Nk > 64


def fwd_kernel(dtype, Nk, dist):
    """which forward kernel launch_attn_fwd picks: 'short' (attn_fwd_kernel), 'ks' (attn_fwd_ks_kernel), 'tiled' (attn_fwd_tiled_kernel)"""
    if Nk <= 128:
        return "short"
    return "ks" if is16(dtype) and not dist else "tiled"


def key_pad(kernel, Nk):
    """keys the kernel's LDS image holds: the valid ones plus zero rows"""
    return rup(Nk, {"short": 32, "tiled": 128, "ks": 64}[kernel])


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
class Case(SimpleNamespace):
    @property
    def H(self):
        return self.nh * HD

    @property
    def ldp(self):
        return self.ldp_ if self.ldp_ else rup(self.Nk, 8)

    @property
    def id(self):
        return f"{self.kernel}-{self.Nq}x{self.Nk}" + (f"-{self.tag}" if self.tag else "")

    def dtypes(self):
        out = []
        for name, dt in DTYPES.items():
            if self.only and name not in self.only:
                continue
            if self.kernel in ("ks", "bwd_ks") and not is16(dt):
                continue
            if self.kernel == "tiled" and is16(dt) and not self.dist:
                continue
            if self.kernel in ("bwd4", "bwd8") and not attn_supported(dt, self.Nq, self.Nk, 1):
                continue
            out.append(name)
        return out


def C(kernel, Nq, Nk, branch, B=2, nh=1, cross=True, mask=True, dist=False, p=0.0, init=False, acc=False, spike=False, dead=None,
      allmask=False, only=None, tag="", ldp=0):
    """branch: the branches of the table in the GPU file this case is there for; cross: q [., H] and kv [., 2H] buffers (else slabs of one
    [., 3H] buffer); dead: (first, last+1) keys of sample 0 that are all masked (a whole tile / slab); allmask: sample B-1 has no valid key"""
    seed = zlib_seed(kernel, Nq, Nk, tag)
    return Case(kernel=kernel, Nq=Nq, Nk=Nk, branch=tuple(branch), B=B, nh=nh, cross=cross, mask=mask, dist=dist, p=p, init=init, acc=acc,
                spike=spike, dead=dead, allmask=allmask, only=only, tag=tag, seed=seed, ldp_=ldp)


def zlib_seed(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


FWD_CASES = [
    C("short", 1, 1, ["NT2", "one key"], mask=False),
    C("short", 17, 15, ["NT2", "partial query tile"], nh=3, dist=True, p=0.1),
    C("short", 16, 16, ["NT2"], B=3, cross=False, p=0.1),
    C("short", 33, 17, ["NT2", "partial query tile"], mask=False, dist=True),
    C("short", 63, 31, ["NT2", "partial query tile"], nh=3),
    C("short", 64, 32, ["NT2", "full query tile"], p=0.1),
    C("short", 65, 33, ["NT4", "second query tile"]),
    C("short", 37, 64, ["NT4"], B=3, dist=True, p=0.1),
    C("short", 70, 65, ["NT6", "second query tile"], nh=3, p=0.1),
    C("short", 128, 127, ["NT8", "second query tile"], mask=False),
    C("short", 130, 128, ["NT8", "third query tile"], p=0.1),
    C("short", 37, 40, ["fully masked sample"], B=3, allmask=True, tag="allmask"),
    C("tiled", 1, 129, ["one valid key in the last tile"], dist=True),
    C("tiled", 65, 255, ["tile - 1", "second query tile", "late maximum"], dist=True, p=0.1, spike=True),
    C("tiled", 64, 256, ["full tiles"], nh=3, cross=False, mask=False, dist=True),
    C("tiled", 40, 257, ["tile + 1", "dead tile", "late maximum"], dist=True, p=0.1, spike=True, dead=(0, 128)),
    C("tiled", 33, 512, ["four tiles"], dist=True, spike=True),
    C("tiled", 33, 512, ["fp32 with dropout"], p=0.1, spike=True, only=("fp32",), tag="f32drop"),
    C("tiled", 20, 200, ["fully masked sample"], B=3, dist=True, allmask=True, tag="allmask"),
    C("ks", 1, 129, ["nact3", "slab with one valid key"]),
    C("ks", 64, 191, ["nact3"], nh=3, mask=False, p=0.1),
    C("ks", 65, 192, ["nact3", "second query tile"], cross=False, p=0.1, spike=True),
    C("ks", 40, 193, ["nact4", "slab with one valid key", "dead slab"], dead=(64, 128), spike=True),
    C("ks", 33, 449, ["nact8"], p=0.1, spike=True),
    C("ks", 70, 512, ["nact8", "second query tile"], nh=3, mask=False),
    C("ks", 20, 200, ["fully masked sample"], B=3, allmask=True, tag="allmask"),
]
BWD_CASES = [
    C("bwd4", 36, 36, ["alias"], B=3, cross=False, p=0.1, init=True),
    C("bwd4", 32, 17, ["alias"], dist=True),
    C("bwd4", 64, 64, ["alias"], nh=3, cross=False, mask=False, init=True),
    C("bwd4", 64, 17, ["no alias"], p=0.1, init=True),
    C("bwd4", 33, 32, ["no alias"], nh=3, dist=True, p=0.1),
    C("bwd8", 40, 128, ["alias"], p=0.1),
    C("bwd8", 64, 65, ["alias"], nh=3, dist=True, init=True),
    C("bwd8", 80, 80, ["no alias"], B=3, cross=False, p=0.1, init=True),
    C("bwd8", 65, 64, ["no alias"], cross=False, mask=False, dist=True, p=0.1),
    C("bwd8", 128, 128, ["no alias"], cross=False, init=True),
    C("bwd8", 97, 33, ["no alias"], nh=3, dist=True, p=0.1, init=True),
    C("bwd_ks", 1, 129, ["one query tile", "store"]),
    C("bwd_ks", 16, 192, ["one query tile", "accumulate"], nh=3, mask=False, p=0.1, acc=True),
    C("bwd_ks", 64, 193, ["one query tile", "store"], p=0.1),
    C("bwd_ks", 65, 256, ["two query tiles", "accumulate"], cross=False, acc=True),
    C("bwd_ks", 130, 512, ["three query tiles", "store"], nh=3, p=0.1),
]
# pair forms (two calls under one group): (name, problem A, problem B)
PAIRS = [
    ("fwd pair", C("short", 37, 37, ["pair"], B=3, p=0.1, tag="pairA"), C("short", 70, 100, ["pair"], nh=3, mask=False, dist=True, tag="pairB")),
    ("fwd long-key group", C("short", 37, 64, ["group"], tag="longA"), C("tiled", 40, 200, ["group"], dist=True, tag="longB")),
    ("bwd pair 4 on 8", C("bwd4", 36, 36, ["pair"], B=3, p=0.1, init=True, tag="pairA"), C("bwd8", 80, 80, ["pair"], nh=3, dist=True, tag="pairB")),
    ("bwd pair 4 + 4 large first", C("bwd4", 64, 64, ["pair"], nh=3, init=True, tag="pair4A"), C("bwd4", 33, 17, ["pair"], B=3, p=0.1, tag="pair4B")),
]
# the ldp contract: rup(Nk, 32) is the widest accepted pitch
LDP_CASES = [C("short", 20, 37, ["ldp"], p=0.1, ldp=64, tag="ldp"), C("tiled", 20, 129, ["ldp"], dist=True, p=0.1, ldp=160, tag="ldp"),
             C("ks", 20, 193, ["ldp"], p=0.1, ldp=224, tag="ldp")]

BRANCHES = {
    "short": {"NT2", "NT4", "NT6", "NT8", "one key", "partial query tile", "full query tile", "second query tile", "third query tile",
              "fully masked sample"},
    "tiled": {"one valid key in the last tile", "tile - 1", "full tiles", "tile + 1", "four tiles", "dead tile", "late maximum",
              "second query tile", "fp32 with dropout", "fully masked sample"},
    "ks": {"nact3", "nact4", "nact8", "slab with one valid key", "dead slab", "second query tile", "fully masked sample"},
    "bwd4": {"alias", "no alias"},
    "bwd8": {"alias", "no alias"},
    "bwd_ks": {"one query tile", "two query tiles", "three query tiles", "store", "accumulate"},
}


def inferred_branches(c, dtype):
    """the branches the C rules take for this case's shape (the kernels leave no trace of them: inferred, not observed), plus the data
    properties the case is built with (late maximum, dead tile / slab, fully masked sample), which are taken from its flags"""
    out = set()
    if c.kernel == "short":
        out.add(f"NT{rup(c.Nk, 32) // 16}")
        out.add({1: "first query tile", 2: "second query tile", 3: "third query tile"}[rup(c.Nq, 64) // 64])
        out.add("full query tile" if c.Nq % 64 == 0 else "partial query tile")
        if c.Nk == 1:
            out.add("one key")
    elif c.kernel == "tiled":
        if c.Nk == 129:
            out.add("one valid key in the last tile")
        elif c.Nk % 128 == 1:
            out.add("tile + 1")
        if c.Nk % 128 == 127:
            out.add("tile - 1")
        if c.Nk % 128 == 0:
            out.add("full tiles")
        if rup(c.Nk, 128) == 512:
            out.add("four tiles")
        if c.Nq > 64:
            out.add("second query tile")
    elif c.kernel == "ks":
        out.add(f"nact{rup(c.Nk, 64) // 64}")
        if c.Nk % 64 == 1:
            out.add("slab with one valid key")
        if c.Nq > 64:
            out.add("second query tile")
    elif c.kernel in ("bwd4", "bwd8"):
        out.add("alias" if bwd_alias(dtype, c.Nq, c.Nk) else "no alias")
    elif c.kernel == "bwd_ks":
        out.add({1: "one query tile", 2: "two query tiles", 3: "three query tiles"}[rup(c.Nq, 64) // 64])
        out.add("accumulate" if c.acc else "store")
    # the three below are properties of the case's DATA (its flags), not of its shape: for them the coverage assertion only says that a case
    # with that data exists -- operands() is what makes the data so
    if c.spike:
        out.add("late maximum")
    if c.dead:
        out.add("dead tile" if c.kernel == "tiled" else "dead slab")
    if c.allmask:
        out.add("fully masked sample")
    if c.kernel == "tiled" and dtype == torch.float32 and c.p > 0:
        out.add("fp32 with dropout")
    return out


def check_case_rules(c, dtype):
    """the case runs on the kernel and branch it declares, by the mirrored rules"""
    if c.kernel in ("short", "tiled", "ks"):
        assert attn_supported(dtype, c.Nq, c.Nk, 0) and fwd_kernel(dtype, c.Nk, c.dist) == c.kernel, c.id
    elif c.kernel in ("bwd4", "bwd8"):
        assert attn_supported(dtype, c.Nq, c.Nk, 1) and bwd_waves8(c.Nq, c.Nk) == (c.kernel == "bwd8"), c.id
    else:
        assert attn_supported(dtype, c.Nq, c.Nk, 2), c.id
    inf = inferred_branches(c, dtype)
    missing = {b for b in c.branch if b in BRANCHES[c.kernel]} - inf
    assert not missing, f"{c.id}: declares {sorted(missing)}, the rules give {sorted(inf)}"


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def operands(c, dtype):
    """seeded CPU operands in the storage type: q [B, Nq, H], k / v [B, Nk, H], dO [B, Nq, H], kmask [B, Nk] uint8 | None, dist [B, Nq, Nk]
    fp32 | None, dP_init [B, nh, Nq, ldp] fp32 (zero pads) | None, base_k / base_v [B, Nk, H] | None"""
    g = torch.Generator().manual_seed(c.seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    B, nh, Nq, Nk, H = c.B, c.nh, c.Nq, c.Nk, c.H
    q, k, v, dO = rnd(B, Nq, H), rnd(B, Nk, H), rnd(B, Nk, H), rnd(B, Nq, H)
    if c.spike:
        k[0, Nk - 2] = q[0, 3] * 4.0                    # batch 0: key Nk-2 aligned with query 3 -> a late, large maximum
    o = SimpleNamespace(q=q.to(dtype), k=k.to(dtype), v=v.to(dtype), dO=dO.to(dtype), kmask=None, dist=None, dP_init=None, base_k=None, base_v=None,
                        sprel=SPREL if c.dist else None)
    if c.mask or c.allmask or c.dead:
        m = torch.ones(B, Nk, dtype=torch.uint8)
        if c.mask:
            m[0, max(1, Nk - 3):] = 0
            if Nk > 2:
                m[1, 1] = 0
        if c.dead:
            m[0, c.dead[0]:c.dead[1]] = 0
        if c.allmask:
            m[B - 1] = 0
        o.kmask = m
    if c.dist:
        o.dist = (rnd(B, Nq, Nk).abs() * 4).contiguous()
    if c.init:
        o.dP_init = torch.zeros(B, nh, Nq, c.ldp)
        o.dP_init[..., :Nk] = rnd(B, nh, Nq, Nk) * 0.3
    if c.acc:
        o.base_k, o.base_v = (rnd(B, Nk, H) * 0.5).to(dtype), (rnd(B, Nk, H) * 0.5).to(dtype)
    return o


def synthetic_keep(c):
    """a dropout mask for the CPU file (the GPU file exports the kernel's own): keep / (1 - p) over the logical [B, nh, Nq, Nk], fp32"""
    if c.p <= 0:
        return None
    g = torch.Generator().manual_seed(c.seed ^ 0x5EED)
    u = torch.rand(c.B, c.nh, c.Nq, c.Nk, generator=g)
    return (u >= c.p).float() * torch.tensor(1.0 / (1.0 - c.p), dtype=torch.float32)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def _mask_bool(o, B, Nk):
    return torch.ones(B, Nk, dtype=torch.bool) if o.kmask is None else o.kmask.bool()


def ref_probs(c, o):
    """P [B, nh, Nq, Nk] in fp64 from the stored q, k, the mask and the distance bias"""
    sprel = None if o.dist is None else (float(o.sprel[0]), float(o.sprel[1]))
    return LR.probs(o.q.to(F64), o.k.to(F64), _mask_bool(o, c.B, c.Nk), c.nh, scale=SCALE, dist=None if o.dist is None else o.dist.to(F64), sprel=sprel)


def ref_forward(c, o, keep):
    """(P, Pd, ctx) chained in fp64 (ctx from the reference's own Pd); the autograd-differentiable form"""
    P = ref_probs(c, o)
    Pd = LR.dropped(P, None if keep is None else keep.to(F64))
    return P, Pd, LR.context(Pd, o.v.to(F64), c.nh)


def ref_context(c, o, Pstored):
    """ctx [B, Nq, H] = the fp64 product of stored probabilities [B, nh, Nq, >= Nk] with the stored v, and its envelope sum |P||v|"""
    Pd = Pstored[..., :c.Nk].to(F64)
    v = o.v.to(F64)
    return LR.context(Pd, v, c.nh), LR.context(Pd.abs(), v.abs(), c.nh)


def ref_backward(c, o, P, keep):
    """dQ [B, Nq, H], dK, dV [B, Nk, H] and the intermediates, pure fp64 math on the given P [B, nh, Nq, Nk] (the kernel's stored one)"""
    P = P.to(F64)
    qh, kh, vh, dOh = (heads(t.to(F64), c.nh) for t in (o.q, o.k, o.v, o.dO))
    m = torch.ones_like(P) if keep is None else keep.to(F64)
    dP = dOh @ vh.transpose(-1, -2)
    if o.dP_init is not None:
        dP = dP + o.dP_init[..., :c.Nk].to(F64)
    dP = dP * m
    dS = SCALE * P * (dP - (P * dP).sum(-1, keepdim=True))
    Pd = P * m
    r = SimpleNamespace(P=P, Pd=Pd, dP=dP, dS=dS, qh=qh, kh=kh, vh=vh, dOh=dOh)
    r.dQ, r.dK, r.dV = unheads(dS @ kh), unheads(dS.transpose(-1, -2) @ qh), unheads(Pd.transpose(-1, -2) @ dOh)
    return r


def backward_bounds(c, o, r, dtype, O=None):
    """per-element bounds of dQ, dK, dV (module docstring); O: the stored forward output [B, Nq, H] of the key-split backward"""
    u = lambda x: ulp(x, dtype)
    Nq, Nk = c.Nq, c.Nk
    env = r.dOh.abs() @ r.vh.abs().transpose(-1, -2)
    if o.dP_init is not None:
        env = env + o.dP_init[..., :Nk].to(F64).abs()
    env = env + (r.P * r.dP.abs()).sum(-1, keepdim=True)
    d32 = (64 + Nk + 16) * UNIT * SCALE * r.P * env
    if O is not None:
        Oh = heads(O.to(F64), c.nh)
        d32 = d32 + SCALE * r.P * (u(Oh) * r.dOh.abs()).sum(-1, keepdim=True)
    e = u(r.dS) + d32
    bq = unheads(e @ r.kh.abs() + (Nk + 8) * UNIT * (r.dS.abs() @ r.kh.abs())) + u(r.dQ)
    bk = unheads(e.transpose(-1, -2) @ r.qh.abs() + (Nq + 8) * UNIT * (r.dS.abs().transpose(-1, -2) @ r.qh.abs()))
    bv = unheads(u(r.Pd).transpose(-1, -2) @ r.dOh.abs() + (Nq + 8) * UNIT * (r.Pd.abs().transpose(-1, -2) @ r.dOh.abs()))
    bk, bv, wk, wv = bk + u(r.dK), bv + u(r.dV), r.dK, r.dV
    if c.acc:
        wk, wv = r.dK + o.base_k.to(F64), r.dV + o.base_v.to(F64)
        bk, bv = bk + u(wk), bv + u(wv)
    return bq, bk, bv, wk, wv


# ---- checks -------------------------------------------------------------------------------------------------------------------------------
def _note(stats, key, val):
    if stats is not None:
        stats[key] = max(stats.get(key, 0.0), val)


def check16(name, k, ref, dtype, tag, stats=None, measure=False):
    """|k - ref| <= 1 ulp(|ref|) + 0.003 ulp(row rms) over the last dimension's rows"""
    k = k.to(F64)
    assert torch.isfinite(k).all(), f"{tag} {name}: non-finite elements where the kernel writes"
    d = (k - ref).abs()
    rms = ref.pow(2).mean(-1, keepdim=True).sqrt()
    ue, ur = ulp(ref, dtype), ulp(rms, dtype).expand_as(ref)
    big = ref.abs() >= rms
    _note(stats, (name, "ulps"), (d / ue)[big].max().item() if big.any() else 0.0)
    _note(stats, (name, "floor"), ((d - FWD_ULPS * ue).clamp_min(0) / ur).max().item())
    if measure:
        return
    bad = d > FWD_ULPS * ue + FWD_FLOOR * ur
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{tag} {name}: {int(bad.sum())} of {bad.numel()} elements beyond {FWD_ULPS} ulp + {FWD_FLOOR} row-rms ulp; first at {i}: "
                             f"kernel {k[tuple(i)].item():.6g} ref {ref[tuple(i)].item():.6g}")


def check_env(name, k, ref, bound, tag, stats=None, measure=False):
    """|k - ref| <= bound per element; records the worst ratio"""
    k = k.to(F64)
    assert torch.isfinite(k).all(), f"{tag} {name}: non-finite elements where the kernel writes"
    d = (k - ref).abs()
    pos = bound > 0
    _note(stats, (name, "ratio"), (d[pos] / bound[pos]).max().item() if pos.any() else 0.0)
    if measure:
        return
    bad = d > bound
    if bad.any():
        i = bad.nonzero()[0].tolist()
        worst = (d[pos] / bound[pos]).max().item() if pos.any() else float("inf")
        raise AssertionError(f"{tag} {name}: {int(bad.sum())} of {bad.numel()} elements beyond the bound (worst ratio {worst:.3g}); first at {i}: "
                             f"kernel {k[tuple(i)].item():.6g} ref {ref[tuple(i)].item():.6g} bound {bound[tuple(i)].item():.3g}")


def p32_terms(c, o):
    """(|s - max|, E_S) of the fp32 probability bound, [B, nh, Nq, Nk]"""
    qh, kh = heads(o.q.to(F64), c.nh), heads(o.k.to(F64), c.nh)
    s = SCALE * (qh @ kh.transpose(-1, -2)) + ((~_mask_bool(o, c.B, c.Nk)).to(F64) * LR.NEG)[:, None, None, :]
    es = SCALE * (qh.abs() @ kh.abs().transpose(-1, -2))
    if o.dist is not None:
        w, b = float(o.sprel[0]), float(o.sprel[1])
        s = s + (w * o.dist.to(F64) + b)[:, None]
        es = es + ((w * o.dist.to(F64)).abs() + abs(b))[:, None]
    return (s - s.max(-1, keepdim=True).values).abs(), es


def check_p32(name, k, ref, c, o, tag, stats=None, measure=False, scale=None):
    """fp32 probabilities: (EXPF_A (1 + |s - max|) + 2 (64 + 8) E_S) 2^-23 P [+ one fp32 rounding of P m for Pd]"""
    k = k.to(F64)
    assert torch.isfinite(k).all(), f"{tag} {name}: non-finite elements where the kernel writes"
    ds, es = p32_terms(c, o)
    d = (k - ref).abs()
    score = 2 * (64 + 8) * es * UNIT * ref + (0.0 if scale is None else UNIT * ref)
    unit = (1 + ds) * UNIT * ref
    pos = unit > 0
    _note(stats, (name, "expf ratio"), ((d - score).clamp_min(0)[pos] / unit[pos]).max().item() if pos.any() else 0.0)
    _note(stats, (name, "raw ratio"), (d[pos] / unit[pos]).max().item() if pos.any() else 0.0)
    if measure:
        return
    bad = d > EXPF_A * unit + score
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{tag} {name}: {int(bad.sum())} of {bad.numel()} elements beyond the fp32 bound; first at {i}: "
                             f"kernel {k[tuple(i)].item():.9g} ref {ref[tuple(i)].item():.9g}")


def tile_rel(name, k, ref, c, dtype, tag, stats=None, measure=False):
    """rel-L2 per (batch, head, 16-row tile) of a [B, N, H] gradient: one wrong tile cannot hide in the whole tensor's norm"""
    kh, rh = heads(k.to(F64), c.nh), heads(ref, c.nh)
    N = rh.shape[2]
    pad = rup(N, 16) - N
    if pad:
        kh, rh = torch.nn.functional.pad(kh, (0, 0, 0, pad)), torch.nn.functional.pad(rh, (0, 0, 0, pad))
    B, nh = rh.shape[:2]
    num = (kh - rh).reshape(B, nh, -1, 16 * HD).norm(dim=-1)
    den = rh.reshape(B, nh, -1, 16 * HD).norm(dim=-1)
    ok = den > 0
    rel = torch.where(ok, num / den.clamp_min(1e-300), torch.zeros_like(num))
    assert (num[~ok] == 0).all(), f"{tag} {name}: a tile whose reference is zero is not zero"
    worst = rel.max().item()
    _note(stats, (name, "tile rel"), worst)
    name_dt = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}[dtype]
    if not measure:
        assert worst < TILE_REL[name_dt], f"{tag} {name}: tile {rel.argmax().item()} (of [B, nh, tiles] flattened) rel-L2 {worst:.3e} >= {TILE_REL[name_dt]:.3e}"


def verify_fwd(c, dtype, o, keep, P, Pd, ctx, tag, stats=None, measure=False, cache=None):
    """every forward check on P, Pd [B, nh, Nq, ldp] (Pd None without dropout) and ctx [B, Nq, H] (CPU tensors in the storage type); cache: a
    dict that keeps the reference probabilities (they depend on the operands only) between calls on the same case and operands"""
    Nk = c.Nk
    outs = [("P", P)] + ([("Pd", Pd)] if c.p > 0 else [])
    for name, t in outs:
        assert torch.isfinite(t.float()).all(), f"{tag} {name}: non-finite elements where the kernel writes"
        assert (t[..., Nk:] == 0).all(), f"{tag} {name}: pad columns {Nk}..{c.ldp} are not zero"
    assert torch.isfinite(ctx.float()).all(), f"{tag} ctx: non-finite elements where the kernel writes"
    good = slice(0, c.B - 1) if c.allmask else slice(0, c.B)
    if c.allmask:
        # a sample without a valid key: every score is -10000 + s, an fp32 score has 2^-10 resolution there (the additive-mask contract)
        row = P[c.B - 1].to(F64)
        assert (row >= 0).all(), f"{tag} P: negative probability in the fully masked sample"
        dev = (row.sum(-1) - 1).abs().max().item()
        assert dev <= 2 * ulp_one(dtype), f"{tag} P: rows of the fully masked sample sum to 1 +- {dev:.3e}"
    cache = {} if cache is None else cache
    if "Pref" not in cache:
        cache["Pref"] = ref_probs(c, o)
    Pref = cache["Pref"]
    if is16(dtype):
        check16("P", P[good, ..., :Nk], Pref[good], dtype, tag, stats, measure)
    else:
        check_p32("P", P[good, ..., :Nk], Pref[good], _sub(c, good), _subo(o, good), tag, stats, measure)
    used = P
    if c.p > 0:
        kp = keep.to(F64)
        if is16(dtype):
            check16("Pd", Pd[good, ..., :Nk], (Pref * kp)[good], dtype, tag, stats, measure)
        else:
            check_p32("Pd", Pd[good, ..., :Nk], (Pref * kp)[good], _sub(c, good), _subo(o, good), tag, stats, measure, scale=kp)
        # the zero pattern of Pd is the mask's, apart from elements whose clean P already rounds to 0
        same = ((Pd[..., :Nk] == 0) == (keep == 0)) | (P[..., :Nk] == 0)
        assert same.all(), f"{tag} Pd: {int((~same).sum())} elements whose zero pattern is not the dropout mask's"
        used = Pd
    cref, cenv = ref_context(c, o, used)
    if is16(dtype):
        check16("ctx", ctx, cref, dtype, tag, stats, measure)
    else:
        check_env("ctx", ctx, cref, (Nk + 8) * UNIT * cenv, tag, stats, measure)


def _sub(c, sl):
    d = dict(c.__dict__)
    d["B"] = len(range(*sl.indices(c.B)))
    return Case(**d)


def _subo(o, sl):
    d = dict(o.__dict__)
    for k in ("q", "k", "v", "dO", "kmask", "dist"):
        if d[k] is not None:
            d[k] = d[k][sl]
    return SimpleNamespace(**d)


def verify_bwd(c, dtype, o, keep, P, O, dq, dk, dv, tag, stats=None, measure=False, cache=None):
    """every backward check; P [B, nh, Nq, ldp] = the stored clean probabilities the kernel read, O [B, Nq, H] = the stored forward output
    (key-split backward only, else None); dq [B, Nq, H], dk, dv [B, Nk, H]"""
    cache = {} if cache is None else cache              # (reference and bounds depend on the operands, P and O only: kept between calls on them)
    if "bwd" not in cache:
        r = ref_backward(c, o, P[..., :c.Nk], keep)
        cache["bwd"] = (r, backward_bounds(c, o, r, dtype, O if c.kernel == "bwd_ks" else None))
    r, (bq, bk, bv, wk, wv) = cache["bwd"]
    for name, k, ref, b in (("dQ", dq, r.dQ, bq), ("dK", dk, wk, bk), ("dV", dv, wv, bv)):
        check_env(name, k, ref, b, tag, stats, measure)
        tile_rel(name, k, ref, c, dtype, tag, stats, measure)


# ---- fp32 / 16-bit emulation of the kernels' dataflow, and the planted defects --------------------------------------------------------------
FWD_DEFECTS = ("last key missing", "key from the neighbouring tile", "mask of the previous sample", "running sum not rescaled",
               "dropout pitch ldp", "head columns shifted", "pad key probability")
BWD_DEFECTS = ("last key missing", "key from the neighbouring tile", "dropout pitch ldp", "dP_init ignored", "accumulate overwrites")


def defect_applies(c, dtype, defect):
    """One narrowing, on purpose.  'key from the neighbouring tile' moves the key at every multiple of ONE stride per kernel -- the kernel's own
    key tile: 16 short and attn_bwd_body, 64 key-split, 128 two-pass -- not 16 j as well as 64 j / 128 j for the long-key kernels: a multiple of
    64 or 128 is one of 16 too, and the wider stride is the seam those kernels really have."""
    kern = c.kernel
    if c.allmask:
        return False
    if defect == "key from the neighbouring tile":
        return c.Nk > 16
    if defect == "mask of the previous sample":
        return c.mask and c.Nk > 3
    if defect == "running sum not rescaled":
        return kern in ("tiled", "ks") and c.spike
    if defect == "dropout pitch ldp":
        return c.p > 0 and c.ldp != c.Nk
    if defect == "head columns shifted":
        return c.nh > 1
    if defect == "pad key probability":
        return kern in ("short", "tiled", "ks") and key_pad(kern, c.Nk) > c.Nk
    if defect == "dP_init ignored":
        return c.init
    if defect == "accumulate overwrites":
        return c.acc
    return True


def _tile_of(c):
    return {"short": 16, "tiled": 128, "ks": 64}.get(c.kernel, 64 if c.kernel == "bwd_ks" else 16)


def _neighbour(t, c):
    """key rows at the first index of every tile but the first replaced by the row before them (the neighbouring tile's last)"""
    t = t.clone()
    T = _tile_of(c)
    for j in range(T, c.Nk, T):
        t[:, :, j] = t[:, :, j - 1]
    return t


def _wrong_pitch(keep, c):
    """the mask the kernel would draw with the index ((b nh + h) Nq + q) ldp + key instead of ... Nk + key"""
    flat = keep.reshape(-1)
    b, h, q, k = torch.meshgrid(torch.arange(c.B), torch.arange(c.nh), torch.arange(c.Nq), torch.arange(c.Nk), indexing="ij")
    idx = (((b * c.nh + h) * c.Nq + q) * c.ldp + k) % flat.numel()
    return flat[idx]


def emulate_fwd(c, dtype, o, keep, defect=None):
    """(P, Pd | None, ctx) as the kernels compute them: fp32 scores, exp, sum, reciprocal; P and P m rounded to storage; fp32 product of the
    ROUNDED probabilities with v, rounded.  P / Pd come back as [B, nh, Nq, ldp] with zero pads."""
    f = torch.float32
    B, nh, Nq, Nk, ldp = c.B, c.nh, c.Nq, c.Nk, c.ldp
    qh, kh, vh = heads(o.q.to(f), nh), heads(o.k.to(f), nh), heads(o.v.to(f), nh)
    if defect == "key from the neighbouring tile":
        kh, vh = _neighbour(kh, c), _neighbour(vh, c)
    km = _mask_bool(o, B, Nk)
    if defect == "mask of the previous sample":
        km = km.roll(1, 0)
    s = (qh @ kh.transpose(-1, -2)) * SCALE
    s = s + ((~km).to(f) * LR.NEG)[:, None, None, :]
    if o.dist is not None:
        s = s + (torch.tensor(o.sprel[0], dtype=f) * o.dist + torch.tensor(o.sprel[1], dtype=f))[:, None]
    npad = 0
    if defect == "pad key probability":
        npad = key_pad(c.kernel, Nk) - Nk
        s = torch.cat([s, torch.zeros(B, nh, Nq, npad)], -1)
    mx = s.max(-1, keepdim=True).values
    e = torch.exp(s - mx)
    tot = e.sum(-1, keepdim=True)
    if defect == "running sum not rescaled":
        T = _tile_of(c)
        run = torch.full_like(mx, -3.0e38)
        tot = torch.zeros_like(mx)
        for k0 in range(0, Nk, T):
            run = torch.maximum(run, s[..., k0:k0 + T].max(-1, keepdim=True).values)
            tot = tot + torch.exp(s[..., k0:k0 + T] - run).sum(-1, keepdim=True)
    P32 = e * (1.0 / tot)
    P = torch.zeros(B, nh, Nq, ldp, dtype=dtype)
    w = min(ldp, Nk + npad)
    P[..., :w] = P32[..., :w].to(dtype)
    Pd = None
    used = P
    if c.p > 0:
        m = _wrong_pitch(keep, c) if defect == "dropout pitch ldp" else keep
        Pd = torch.zeros(B, nh, Nq, ldp, dtype=dtype)
        Pd[..., :Nk] = (P32[..., :Nk] * m).to(dtype)
        used = Pd
    up = used[..., :Nk].to(f).clone()
    if defect == "last key missing":
        up[..., Nk - 1] = 0
    ctx = unheads(up @ vh)
    if defect == "head columns shifted":
        ctx = ctx.roll(HD, -1)
    return P, Pd, ctx.to(dtype)


def emulate_bwd(c, dtype, o, keep, P, O, defect=None):
    """(dq, dk, dv) as attn_bwd_body / attn_bwd_ks_kernel compute them from the stored P [B, nh, Nq, ldp] (and the stored O: key-split)"""
    f = torch.float32
    nh, Nk = c.nh, c.Nk
    qh, kh, vh, dOh = (heads(t.to(f), nh) for t in (o.q, o.k, o.v, o.dO))
    if defect == "key from the neighbouring tile":
        kh, vh = _neighbour(kh, c), _neighbour(vh, c)
    Pf = P[..., :Nk].to(f)
    d = dOh @ vh.transpose(-1, -2)
    if o.dP_init is not None and defect != "dP_init ignored":
        d = d + o.dP_init[..., :Nk]
    pm = Pf
    if c.p > 0:
        m = _wrong_pitch(keep, c) if defect == "dropout pitch ldp" else keep
        d = d * m
        pm = (Pf * m).to(dtype).to(f)
    if c.kernel == "bwd_ks":
        rs = (dOh * heads(O.to(f), nh)).sum(-1, keepdim=True)
    else:
        rs = (Pf * d).sum(-1, keepdim=True)
    dS = ((Pf * (d - rs)) * SCALE).to(dtype).to(f)
    dSq = dS.clone()
    if defect == "last key missing":
        dSq[..., Nk - 1] = 0
    dq = unheads(dSq @ kh)
    if c.kernel != "bwd_ks":
        dk, dv = unheads(dS.transpose(-1, -2) @ qh), unheads(pm.transpose(-1, -2) @ dOh)
        if defect == "last key missing":
            dv[:, Nk - 1] = 0
        return dq.to(dtype), dk.to(dtype), dv.to(dtype)
    # the key-split kernel walks the queries in tiles of 64 and keeps dK / dV in the 16-bit buffers between tiles: tile 0 stores (or adds to
    # the base when accumulating), every later tile reads, adds and rounds again; with more than one tile each element's rounding residual
    # (kept in the storage type) goes into the next tile's sum
    multi = c.Nq > 64
    dk = dv = None
    if c.acc and defect != "accumulate overwrites":
        dk, dv = o.base_k.clone(), o.base_v.clone()
    rk = rv = 0.0
    for q0 in range(0, c.Nq, 64):
        pk = unheads(dS[:, :, q0:q0 + 64].transpose(-1, -2) @ qh[:, :, q0:q0 + 64])
        pv = unheads(pm[:, :, q0:q0 + 64].transpose(-1, -2) @ dOh[:, :, q0:q0 + 64])
        if defect == "last key missing":
            pv[:, Nk - 1] = 0
        sk = (pk if dk is None else dk.to(f) + pk) + rk
        sv = (pv if dv is None else dv.to(f) + pv) + rv
        dk, dv = sk.to(dtype), sv.to(dtype)
        if multi:
            rk, rv = (sk - dk.to(f)).to(dtype).to(f), (sv - dv.to(f)).to(dtype).to(f)
    return dq.to(dtype), dk, dv


def pair_with_first_problems_heads(t, c, nh_a):
    """problem B of a pair whose blocks take (local % nh, local / nh) with problem A's nh: a block then serves (b', h') = (local / nh_a,
    local % nh_a) and writes that slot; the slots no block reaches stay as the buffer was filled (NaN).  t: [B, N, H] output of problem B"""
    out = torch.full_like(t, float("nan"))
    for local in range(c.B * c.nh):
        h, b = local % nh_a, local // nh_a
        if b < c.B and h < c.nh:
            out[b, :, h * HD:(h + 1) * HD] = t[b, :, h * HD:(h + 1) * HD]
    return out
