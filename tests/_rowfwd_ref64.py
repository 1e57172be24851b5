"""float64 references of the row-wise forward kernels (csrc/rowops.hip: ln_fwd and its pair launch, smallk_ln_fwd, node_in_fwd, embed_in_fwd,
softmax_fwd / softmax_bwd, head_mean_fwd / head_mean_bwd, lndot_fwd) and of the gather / fusion glue (csrc/graphops.hip: csr_gather,
csr_gather_multi, pano_fuse_fwd), their error bounds, the Python mirrors of the launch rules, an fp32 / 16-bit emulation of every kernel with
its planted defects, and the seeded case table that tests/test_rowfwd_ref64_cpu.py and tests/test_rowfwd_fp64_gpu.py share.  Everything here
works on the tensors it is given (CPU or GPU); nothing launches a kernel.

Every output is checked as a STAGE from the operands the kernel reads (the stored 16-bit / fp32 values taken to float64), so it carries one
rounding.  With unit = 2^-23 (UNIT of tests/_gemm_ref64.py), u(x) = one unit in the last place of |x| in the storage type (0 for fp32 storage):

  LayerNorm outputs, 16-bit     |k - ref| <= 1 u(ref) + 0.003 u(rms of the ref's row)                (LN_ULPS, LN_FLOOR of tests/_gemm_ref64.py)
  LayerNorm outputs, fp32       16 unit (|g xhat| + |beta|) + RSTD_REL |g xhat| + |g| rstd (2 NIT + 6 + 8) unit mean |x| for the mean (a lane's
                                2 NIT additions, 6 shuffle levels) + the summed input's error dx = (n + 8) unit E carried through the
                                normalisation: rstd (|g| (dx + mean dx) + |g xhat| rstd rms(dx))
  rstd                          |k - ref| <= RSTD_REL ref                                            (RSTD_REL = 4e-7)
  plain fp32 sums of n terms    (n + 8) unit E + u(ref), E = the sum of the terms' absolute values: csr_gather (n = edges [+ the old value]),
                                ln_fwd(do_ln = 0), head mean (n = nh; backward n = 2), lndot logits (n = H, plus |w2| times the fp32 LayerNorm
                                bound of each element)
  unobservable roundings        csr_gather_multi rounds to storage after its first source and node_in_fwd after each gathered source: one
                                u(reference intermediate) for each such point
  softmax probabilities         score x = S scale [- 10000] [+ sw dist + sb]: dx = (3 + 8) unit (|S scale| + |sw dist| + |sb|); the fast exp of
                                d = x - max costs (3 |d| + 2) 2^-24 (subtraction, argument scaling by log2 e, v_exp_f32: the allowance of the
                                panorama fusion below, per element), the row sum (Nk + 1) 2^-24; in e / sum e every error appears once for the
                                element and once P-weighted:
                                    dP / P <= 2 max dx + ((3 |d| + 2) + sum_j P_j (3 |d_j| + 2) + Nk + 1) 2^-24,    |k - ref| <= P dP/P + u(ref) + 2^-126
                                pad columns [Nk, ldp) are exactly 0.  A fully masked sample follows the additive-mask contract: the reference
                                rounds -10000 + S scale to fp32 first; its rows are non-negative and sum to 1 within 2 storage ulps.
  softmax backward              from the STORED P: s = sum P g (Nk terms), d = P (g - s):
                                    |dS - ref| <= scale (P (Nk + 8) unit sum |P g| + (2 + 8) unit P (|g| + |s|)) + u(ref)
                                dsprel_w / dsprel_b sum d dist / d over rows and keys through 8 per-lane terms, 6 shuffle levels, 4 waves and
                                one atomic per workgroup: n = 18 + workgroups, plus every term's own bound
  panorama fusion               pano_ref (the derivation of test_pano_fuse_fwd_general_kernel_matches_float64, moved here)

No slack factors: an honest emulation sits at about half of the 16-bit bounds (one rounding to nearest is half an ulp).

Measured on MI355X over every case of the table (tests/test_rowfwd_fp64_gpu.py -s, test_zz_report), worst |k - ref| / bound per kernel output:
  kernel                                 output      bf16     fp16     fp32
  magic_ln_fwd (+ pair launch)           out         0.4989   0.4993   0.0382
  magic_ln_fwd (+ pair launch)           rstd        0.2524   0.2380   0.2468
  magic_ln_fwd (+ pair launch)           sum         0.4999   0.4993   0.0765
  magic_smallk_ln_fwd                    out         0.4992   0.4991   0.0371
  magic_smallk_ln_fwd                    rstd        0.2965   0.2965   0.2965
  magic_node_in_fwd                      A           0.4993   0.4994   0.0305
  magic_node_in_fwd                      out         0.4999   0.4996   0.0993
  magic_node_in_fwd                      rstd        0.2709   0.2709   0.2709
  magic_embed_in_fwd                     A1          0.4992   0.4993   0.0612
  magic_embed_in_fwd                     A2          0.4992   0.4993   0.0312
  magic_embed_in_fwd                     X0          0.4992   0.4992   0.0355
  magic_embed_in_fwd                     rstd1       0.2783   0.2845   0.2451
  magic_embed_in_fwd                     rstd2       0.2657   0.2657   0.2657
  magic_embed_in_fwd                     rstd3       0.2801   0.2575   0.2089
  magic_embed_in_fwd                     tout        0.4991   0.4985   0.0350
  magic_embed_in_fwd                     trstd       0.1759   0.2385   0.2329
  magic_lndot_fwd                        logit       0.0013   0.0013   0.0007
  magic_softmax_fwd / _bwd               P           0.4992   0.4942   0.0444
  magic_softmax_fwd / _bwd               dS          0.4995   0.4959   0.0265
  magic_softmax_fwd / _bwd               dsprel_b    0.0004   0.0008   0.0018
  magic_softmax_fwd / _bwd               dsprel_w    0.0006   0.0008   0.0015
  magic_head_mean_fwd / _bwd             dP          0.0658   0.0658   0.0658
  magic_head_mean_fwd / _bwd             mean        0.0166   0.0167   0.1081
  magic_csr_gather                       out         0.4999   0.4994   0.0931
  magic_csr_gather_multi                 out         0.4998   0.4993   0.0907
  magic_pano_fuse_fwd (register form)    fused       0.9387   0.7085   0.0013
  magic_pano_fuse_fwd (register form)    pmean       0.0000   0.0000   0.3325
  magic_pano_fuse_fwd (register form)    probs       0.0038   0.0039   0.0037
  (embed_in tout / trstd: its text half; head mean dP is fp32 whatever the storage type.)  The 16-bit outputs sit at half a bound: one rounding to
  nearest of an fp32 result whose own error is far below it.  Panorama fusion's bound counts u as the unit roundoff, so 0.94 there is 0.47 ulp.
  With the last k term of smallk_ln_fwd dropped in the kernel (a temporary break), all 20 smallk cases fail, the first at 2.6e4 bounds.
"""
import zlib
from types import SimpleNamespace

import torch

from tests._gemm_ref64 import LN_FLOOR, LN_ULPS, RSTD_REL, UNIT, ulp

F64, F32 = torch.float64, torch.float32
U24 = 2.0 ** -24
TINY = 2.0 ** -126
EPS = 1e-12
SCALE = 0.125
NEG = -10000.0
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
WIDTHS = (128, 256, 384, 768)
NAN = float("nan")


def is16(dtype):
    return dtype != torch.float32


def ulp_one(dtype):
    return {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 2.0 ** -23}[dtype]


# ---- mirrors of the launch rules ------------------------------------------------------------------------------------------------------------
ROWS_PER_WG = {"ln": 4, "lndot": 4, "softmax": 4, "csr": 4, "csrm": 4, "smallk": 16, "node_in": 16, "embed_in": 16}      # 4 waves x 1 | SKF_ROWS = 4


def h_ok(H):
    """DISPATCH_NIT: the widths the LayerNorm-type kernels are built for"""
    return H in WIDTHS


def smallk_body(H):
    """W in registers (WREG: NIT <= 2) or re-read through the k < Kin selects"""
    return "W in registers" if H <= 256 else "W re-read"


def pano_register_form(V, H):
    return V <= 40 and H in WIDTHS


def pair_split(Ma, kind="ln"):
    """first workgroup of the second problem of a pair launch"""
    return -(-Ma // ROWS_PER_WG[kind])


def row_edges(M, rpw):
    out = set()
    if M == 1:
        out.add("one row")
    if M % rpw == 0:
        out.add("full workgroup")
    if M % rpw == 1 and M > 1:
        out.add("workgroup + 1")
    if M % rpw == rpw - 1:
        out.add("workgroup - 1")
    if M > 2 * rpw:
        out.add("third workgroup")
    if rpw == 16 and M % 4:
        out.add("wave partial")
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
class Case(SimpleNamespace):
    @property
    def id(self):
        return f"{self.kind}-{self.tag}"


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


def C(kind, tag, branch, **kw):
    return Case(kind=kind, tag=tag, branch=tuple(branch), seed=seed_of(kind, tag), **kw)


M4 = {1: ["one row"], 4: ["full workgroup"], 5: ["workgroup + 1"], 9: ["workgroup + 1", "third workgroup"]}
M16 = {1: ["one row"], 15: ["workgroup - 1", "wave partial"], 16: ["full workgroup"], 17: ["workgroup + 1", "wave partial"],
       33: ["workgroup + 1", "third workgroup"]}
KINS = (1, 7, 16)
LN_FORMS = ("text", "image", "in0+in1", "sum only", "no rstd")


def nit(H):
    return f"NIT{H // 128}"


def _ln_cases():
    out = []
    for i, H in enumerate(WIDTHS):
        seen = set()
        for j, M in enumerate(M4):
            form = LN_FORMS[(i + j) % 5]
            seen.add(form)
            out.append(C("ln", f"H{H}-M{M}-{form}", [nit(H), form] + M4[M], H=H, M=M, form=form))
        for form in LN_FORMS:
            if form not in seen:
                out.append(C("ln", f"H{H}-M5-{form}", [nit(H), form] + M4[5], H=H, M=5, form=form))
    return out


def _smallk_cases():
    return [C("smallk", f"H{H}-M{M}-K{KINS[(i + j) % 3]}", [nit(H), smallk_body(H), f"Kin {KINS[(i + j) % 3]}"] + M16[M], H=H, M=M, Kin=KINS[(i + j) % 3])
            for i, H in enumerate(WIDTHS) for j, M in enumerate(M16)]


def _lndot_cases():
    return [C("lndot", f"H{H}-M{M}", [nit(H)] + M4[M], H=H, M=M) for H in WIDTHS for M in M4]


CSR_WIDTHS = (2, 126, 128, 130, 256, 384, 768)


def _csr_width(H):
    return "narrower than a wave" if H < 128 else "whole slices" if H % 128 == 0 else "partial slice"


def _csr_cases():
    out = []
    for i, H in enumerate(CSR_WIDTHS):
        for j, M in enumerate(M4):
            acc, now = bool((i + j) & 1), bool((i + j) & 2)
            br = [_csr_width(H), "accumulate" if acc else "store", "no weights" if now else "weights"] + M4[M]
            if M > 1:
                br += ["empty row", "repeated index"]
            if M > 2:
                br += ["five edges"]
            out.append(C("csr", f"H{H}-M{M}-{'acc' if acc else 'st'}{'-now' if now else ''}", br, H=H, M=M, acc=acc, now=now))
    return out


def _csrm_cases():
    out = []
    for H in (128, 768):
        for n in (1, 3, 4):
            probs = [dict(M=(9, 1, 5, 4)[k], two=k != 1, acc=k == 2) for k in range(n)]
            out.append(C("csrm", f"H{H}-n{n}", [f"{n} problems", "second source"] + (["accumulate"] if n > 2 else []), H=H, probs=probs))
    return out


SM_SHAPES = ((1, 1), (63, 64), (64, 64), (65, 72), (511, 512), (512, 512))


def _sm_shape_branches(Nk, ldp):
    br = [f"IT{-(-Nk // 64)}"]
    if Nk == 1:
        br.append("one key")
    if Nk % 64 == 63:
        br.append("slice - 1")
    if Nk % 64 == 0:
        br.append("full slices")
    if Nk % 64 == 1 and Nk > 1:
        br.append("slice + 1")
    if ldp > Nk:
        br.append("pad columns")
    return br


def _softmax_cases():
    out = []
    for Nk, ldp in SM_SHAPES:
        for kmask in (False, True):
            for dist in (False, True):
                br = _sm_shape_branches(Nk, ldp) + ["rows % 4"] + (["kmask"] if kmask else []) + (["dist"] if dist else [])
                out.append(C("softmax", f"{Nk}x{ldp}{'-mask' if kmask else ''}{'-dist' if dist else ''}", br, Nk=Nk, ldp=ldp, B=3, nh=2, Nq=3,
                             kmask=kmask, dist=dist, allmask=False))
    out.append(C("softmax", "63x64-allmask", _sm_shape_branches(63, 64) + ["rows % 4", "kmask", "fully masked sample"], Nk=63, ldp=64, B=3, nh=2, Nq=3,
                 kmask=True, dist=False, allmask=True))
    return out


def _headmean_cases():
    out = []
    for B, nh, inner in ((1, 1, 1), (3, 4, 85), (2, 12, 257)):
        for acc in (False, True):
            br = ["accumulate" if acc else "store"] + (["one element"] if B * nh * inner == 1 else []) + (["second block"] if B * inner > 256 else ["one block"])
            out.append(C("headmean", f"{B}x{nh}x{inner}-{'acc' if acc else 'st'}", br, B=B, nh=nh, inner=inner, acc=acc))
    return out


PANO_V = (1, 3, 4, 5, 36, 40)


def _pano_branches(V, H, withP):
    br = ["register form", nit(H)]
    if V < 4:
        br.append("waves without a view")
    if V % 4 == 1 and V > 1:
        br.append("last view alone in its slot")
    if V == 40:
        br.append("ten slots")
    if withP:
        br.append("head mean")
    return br


def _pano_cases():
    return [C("pano", f"V{V}-H{H}{'-P' if (i + j) & 1 else ''}", _pano_branches(V, H, bool((i + j) & 1)), V=V, H=H, N=3, withP=bool((i + j) & 1))
            for i, V in enumerate(PANO_V) for j, H in enumerate(WIDTHS)]


NODE_FORMS = ("add0", "csr1", "csr1+csr2")


def _node_cases():
    out = []
    ms = list(M16)
    for i, H in enumerate(WIDTHS):
        for j, M in enumerate(ms):
            form, tab, two, Kin = NODE_FORMS[(i + j) % 3], bool((i + j) & 1), bool((i + j // 2) & 1), KINS[(i + 2 * j) % 3]
            M2 = ms[(j + 2) % 5]
            br = [nit(H), smallk_body(H), form, "step table" if tab else "no table", "two problems" if two else "one problem", f"Kin {Kin}"] + M16[M]
            out.append(C("node_in", f"H{H}-M{M}{f'+{M2}' if two else ''}-K{Kin}-{form}{'-tab' if tab else ''}", br, H=H, Kin=Kin,
                         probs=[dict(M=M, form=form, tab=tab)] + ([dict(M=M2, form=NODE_FORMS[(i + j + 1) % 3], tab=not tab)] if two else [])))
    return out


def _embed_cases():
    out = []
    for i, H in enumerate(WIDTHS):
        for j, M in enumerate(M16):
            text, Kin = bool((i + j) & 1), KINS[(i + j) % 3]
            br = [nit(H), smallk_body(H), "text half" if text else "no text", f"Kin {Kin}"] + M16[M]
            out.append(C("embed_in", f"H{H}-M{M}-K{Kin}{'-text' if text else ''}", br, H=H, M=M, Kin=Kin, text=text, Mt=(5, 9, 1, 4)[i]))
    return out


def _pair_cases():
    """ln_fwd_pair_kernel under L.group(): (problem A, problem B) of one width; B differs from A in its form, its rows and its gamma / beta"""
    out = []
    for H in WIDTHS:
        for Ma, Mb in ((5, 1), (1, 9), (4, 4)):
            a = C("ln", f"pairA-H{H}-M{Ma}", [nit(H), "text", f"split {pair_split(Ma)}"], H=H, M=Ma, form="text")
            b = C("ln", f"pairB-H{H}-M{Mb}-after{Ma}", [nit(H), "image", f"split {pair_split(Ma)}"], H=H, M=Mb, form="image")
            out.append((a, b))
    return out


CASES = {"ln": _ln_cases(), "smallk": _smallk_cases(), "lndot": _lndot_cases(), "csr": _csr_cases(), "csrm": _csrm_cases(),
         "softmax": _softmax_cases(), "headmean": _headmean_cases(), "pano": _pano_cases(), "node_in": _node_cases(), "embed_in": _embed_cases()}
PAIRS = _pair_cases()
ALL = [c for cs in CASES.values() for c in cs]

_NITS = {nit(H) for H in WIDTHS}
_E4 = {"one row", "full workgroup", "workgroup + 1", "third workgroup"}
_E16 = _E4 | {"workgroup - 1", "wave partial"}
_BODY = {"W in registers", "W re-read"}
_KIN = {f"Kin {k}" for k in KINS}
BRANCHES = {
    "ln": _NITS | _E4 | set(LN_FORMS),
    "smallk": _NITS | _E16 | _BODY | _KIN,
    "lndot": _NITS | _E4,
    "csr": _E4 | {"narrower than a wave", "whole slices", "partial slice", "accumulate", "store", "weights", "no weights", "empty row", "repeated index",
                  "five edges"},
    "csrm": {"1 problems", "3 problems", "4 problems", "second source", "accumulate"},
    "softmax": {f"IT{i}" for i in (1, 2, 8)} | {"one key", "slice - 1", "full slices", "slice + 1", "pad columns", "rows % 4", "kmask", "dist",
                                                "fully masked sample"},
    "headmean": {"one element", "one block", "second block", "accumulate", "store"},
    "pano": _NITS | {"register form", "waves without a view", "last view alone in its slot", "ten slots", "head mean"},
    "node_in": _NITS | _E16 | _BODY | _KIN | set(NODE_FORMS) | {"step table", "no table", "one problem", "two problems"},
    "embed_in": _NITS | _E16 | _BODY | _KIN | {"text half", "no text"},
    "pair": _NITS | {"split 1", "split 2", "text", "image"},
}


def inferred_branches(c, o=None):
    """the branches the C rules take for this case's shape (the kernels leave no trace of them: inferred from the mirrors above, not observed),
    plus the properties of its data, read from the operands it is built with (o, any storage type: the integer operands do not depend on it)"""
    k, out = c.kind, set()
    o = operands(c, "fp32") if o is None else o
    if k in ("ln", "smallk", "lndot", "node_in", "embed_in"):
        assert h_ok(c.H)
        out.add(f"NIT{c.H // 128}")
    if k in ("smallk", "node_in", "embed_in"):
        out |= {smallk_body(c.H), f"Kin {c.Kin}"}
    if k == "ln":
        out |= row_edges(c.M, 4)
        nt = sum(t is not None for t in o.tabs)
        form = {(0, 0, 3): "text", (1, 0, 2): "image", (1, 1, 0): "in0+in1"}.get((o.in0 is not None, o.in1 is not None, nt))
        form = "sum only" if not o.do_ln else "no rstd" if not o.want_rstd else form
        out.add(form)
    elif k in ("smallk", "embed_in"):
        out |= row_edges(c.M, 16)
        if k == "embed_in":
            out.add("text half" if o.text is not None else "no text")
    elif k == "lndot":
        out |= row_edges(c.M, 4)
    elif k == "node_in":
        out |= row_edges(c.probs[0]["M"], 16)
        out.add("two problems" if len(o.probs) == 2 else "one problem")
        p = o.probs[0]
        out.add("add0" if p.add0 is not None else "csr1+csr2" if p.csr2 is not None else "csr1")
        out.add("step table" if p.tab is not None else "no table")
    elif k == "csr":
        out |= row_edges(c.M, 4) | {_csr_width(c.H)}
        out.add("accumulate" if o.base is not None else "store")
        ptr, idx, w = o.csr
        out.add("no weights" if w is None else "weights")
        deg = (ptr[1:] - ptr[:-1]).tolist()
        if 0 in deg:
            out.add("empty row")
        if 5 in deg:
            out.add("five edges")
        if any(len(set(idx[ptr[r]:ptr[r + 1]].tolist())) < deg[r] for r in range(c.M)):
            out.add("repeated index")
    elif k == "csrm":
        out.add(f"{len(o.probs)} problems")
        if any(p.csr2 is not None for p in o.probs):
            out.add("second source")
        if any(p.base is not None for p in o.probs):
            out.add("accumulate")
    elif k == "softmax":
        out |= set(_sm_shape_branches(c.Nk, c.ldp))
        if (c.B * c.nh * c.Nq) % 4:
            out.add("rows % 4")
        if o.kmask is not None:
            out.add("kmask")
            if (o.kmask.sum(1) == 0).any():
                out.add("fully masked sample")
        if o.dist is not None:
            out.add("dist")
    elif k == "headmean":
        out.add("accumulate" if o.base is not None else "store")
        if c.B * c.nh * c.inner == 1:
            out.add("one element")
        out.add("second block" if c.B * c.inner > 256 else "one block")
    elif k == "pano":
        if pano_register_form(c.V, c.H):
            out |= {"register form", f"NIT{c.H // 128}"}
        if c.V < 4:
            out.add("waves without a view")
        if c.V % 4 == 1 and c.V > 1:
            out.add("last view alone in its slot")
        if -(-c.V // 4) == 10:
            out.add("ten slots")
        if o.P is not None:
            out.add("head mean")
    return out


# ---- operands -----------------------------------------------------------------------------------------------------------------------------------
def _gen(c, salt=0):
    g = torch.Generator().manual_seed(c.seed ^ salt)
    return g, (lambda *s: torch.randn(*s, generator=g))


def _affine(rnd, H):
    return (1.0 + 0.2 * rnd(H)).contiguous(), (0.3 * rnd(H)).contiguous()


def _i32(t):
    return t.to(torch.int32).contiguous()


DEGS = (3, 0, 5, 2, 1, 0, 4, 5, 2)
DEGS2 = (0, 2, 1, 0, 3, 1, 0, 2, 4)


def make_csr(g, n_out, n_src, degs=DEGS, weights=True):
    """(ptr, idx, w | None): row r has degs[r % 9] edges (row 1 is empty; one row alone has 3), the second edge of a row repeats its first index"""
    deg = [degs[r % len(degs)] for r in range(n_out)]
    ptr = torch.tensor([0] + deg).cumsum(0)
    idx = torch.randint(0, n_src, (max(int(ptr[-1]), 1),), generator=g)
    for r in range(n_out):
        if deg[r] >= 2:
            idx[ptr[r] + 1] = idx[ptr[r]]
    w = (torch.randn(idx.numel(), generator=g) * 0.7 + 0.3).contiguous() if weights else None
    return _i32(ptr), _i32(idx), w


def ln_operands(c, dtype):
    g, rnd = _gen(c)
    M, H = c.M, c.H
    o = SimpleNamespace(M=M, H=H, in0=None, in1=None, tabs=[None, None, None], do_ln=True, want_rstd=True)
    o.gamma, o.beta = _affine(rnd, H)
    word = (rnd(11, H).to(dtype), _i32(torch.randint(0, 11, (M,), generator=g)), 0, 0)
    pos = (rnd(7, H).to(dtype), None, 3, 2)               # rows r % 3 + 2
    typ = (rnd(3, H).to(dtype), None, 0, 1)               # the constant row 1
    x0, x1 = rnd(M, H).to(dtype), rnd(M, H).to(dtype)
    if c.form == "text":
        o.tabs = [word, pos, typ]
    elif c.form in ("image", "no rstd"):
        o.in0, o.tabs = x0, [word, typ, None]
        o.want_rstd = c.form == "image"
    elif c.form == "in0+in1":
        o.in0, o.in1 = x0, x1
    else:
        o.in0, o.in1, o.tabs, o.do_ln = x0, x1, [pos, None, None], False
    return o


def smallk_operands(c, dtype, M=None, salt=0):
    g, rnd = _gen(c, salt)
    M = c.M if M is None else M
    o = SimpleNamespace(M=M, H=c.H, Kin=c.Kin, x=rnd(M, c.Kin).contiguous(), W=(rnd(c.H, c.Kin) * 0.5).contiguous(), b=(rnd(c.H) * 0.3).contiguous())
    o.gamma, o.beta = _affine(rnd, c.H)
    return o


def operands(c, dt):
    dtype = DTYPES[dt]
    g, rnd = _gen(c, 0x51)
    k = c.kind
    if k == "ln":
        return ln_operands(c, dtype)
    if k == "smallk":
        return smallk_operands(c, dtype)
    if k == "lndot":
        o = SimpleNamespace(M=c.M, H=c.H, Y=rnd(c.M, c.H).relu().to(dtype), w2=(rnd(c.H) * 0.2).contiguous(), b2=torch.tensor([0.7]))
        o.gamma, o.beta = _affine(rnd, c.H)
        return o
    if k == "csr":
        o = SimpleNamespace(M=c.M, H=c.H, src=rnd(13, c.H).to(dtype), csr=make_csr(g, c.M, 13, weights=not c.now), base=rnd(c.M, c.H).to(dtype) if c.acc else None)
        return o
    if k == "csrm":
        ps = []
        for q in c.probs:
            ps.append(SimpleNamespace(M=q["M"], H=c.H, src=rnd(13, c.H).to(dtype), csr=make_csr(g, q["M"], 13), src2=rnd(7, c.H).to(dtype) if q["two"] else None,
                                      csr2=make_csr(g, q["M"], 7, DEGS2) if q["two"] else None, base=rnd(q["M"], c.H).to(dtype) if q["acc"] else None))
        return SimpleNamespace(probs=ps)
    if k == "softmax":
        B, nh, Nq, Nk, ldp = c.B, c.nh, c.Nq, c.Nk, c.ldp
        o = SimpleNamespace(kmask=None, dist=None, sw=None, sb=None)
        o.S = torch.full((B, nh, Nq, ldp), NAN)
        o.S[..., :Nk] = rnd(B, nh, Nq, Nk) * 8.0
        o.dP = torch.full((B, nh, Nq, ldp), NAN)
        o.dP[..., :Nk] = rnd(B, nh, Nq, Nk)
        if c.kmask:
            m = torch.ones(B, Nk, dtype=torch.uint8)
            if Nk >= 4:
                m[0, Nk - 3:] = 0
                m[1, 1] = 0
                m[2, 0] = 0
                m[2, 2] = 0
            if c.allmask:
                m[B - 1] = 0
            o.kmask = m
        if c.dist:
            o.dist = (rnd(B, Nq, Nk).abs() * 4).contiguous()
            o.sw, o.sb = torch.tensor([0.2]), torch.tensor([-0.1])
        return o
    if k == "headmean":
        return SimpleNamespace(P=torch.softmax(rnd(c.B, c.nh, c.inner), -1).to(dtype), g=rnd(c.B, c.inner).contiguous(),
                               base=rnd(c.B, c.nh, c.inner).contiguous() if c.acc else None)
    if k == "pano":
        N, V, H = c.N, c.V, c.H
        o = SimpleNamespace(x=rnd(N, V, H).to(dtype), lens=_i32(torch.tensor([V, max(V - 4, 1), 1])), wf=(rnd(H) * 0.1).contiguous(), bf=torch.tensor([0.1]),
                            P=None, nh=2, inner=35)
        if c.withP:
            o.P = torch.softmax(rnd(N, o.nh, o.inner), -1).to(dtype)
        return o
    if k == "node_in":
        ps = []
        for i, q in enumerate(c.probs):
            p = smallk_operands(c, dtype, M=q["M"], salt=i + 1)
            p.add0 = p.src1 = p.csr1 = p.src2 = p.csr2 = p.tab = p.tab_idx = None
            if q["form"] == "add0":
                p.add0 = rnd(p.M, c.H).to(dtype)
            else:
                p.src1, p.csr1 = rnd(13, c.H).to(dtype), make_csr(g, p.M, 13)
                if q["form"] == "csr1+csr2":
                    p.src2, p.csr2 = rnd(7, c.H).to(dtype), make_csr(g, p.M, 7, DEGS2)
            if q["tab"]:
                p.tab, p.tab_idx = rnd(6, c.H).to(dtype), _i32(torch.randint(0, 6, (p.M,), generator=g))
            ps.append(p)
        return SimpleNamespace(probs=ps)
    if k == "embed_in":
        o = smallk_operands(c, dtype)
        o.P0 = (rnd(c.M, c.H) * 1.5 + 0.2).to(dtype)
        o.g1, o.b1 = _affine(rnd, c.H)
        o.g3, o.b3 = _affine(rnd, c.H)
        o.nav_tab, o.nav_idx, o.tok_tab = rnd(3, c.H).to(dtype), _i32(torch.randint(0, 3, (c.M,), generator=g)), rnd(2, c.H).to(dtype)
        o.text = ln_operands(C("ln", c.tag + "-text", [], H=c.H, M=c.Mt, form="text"), dtype) if c.text else None
        return o
    raise KeyError(k)


# ---- float64 references ---------------------------------------------------------------------------------------------------------------------------
def tab_rows(t, M, defect=None):
    """tab_row of csrc/rowops.hip: idx[r], else r % mod + off, else off"""
    _, idx, mod, off = t
    r = torch.arange(M)
    if idx is not None:
        return idx.long().cpu()
    if mod:
        return (r + off) % mod if defect == "table row" else r % mod + off
    return torch.full((M,), off, dtype=torch.long)


def ln_terms(o, f, defect=None):
    """the terms ln_fwd sums, in its order (in0, in1, tab0, tab1, tab2), in the float type f"""
    ts = [t.to(f) for t in (o.in0, o.in1) if t is not None]
    for t in o.tabs:
        if t is not None:
            ts.append(t[0].to(f)[tab_rows(t, o.M, defect).to(t[0].device)])
    return ts


def ln64(x, gamma, beta, eps=EPS):
    """(y, g xhat, rstd [rows]) of LayerNorm over the last dimension in float64"""
    mean = x.mean(-1, keepdim=True)
    rstd = (x - mean).pow(2).mean(-1, keepdim=True).add(eps).rsqrt()
    gx = (x - mean) * rstd * gamma.to(F64)
    return gx + beta.to(F64), gx, rstd.squeeze(-1)


def ln_bound(y, gx, rstd, gamma, beta, dtype, n=0, E=None, x=None):
    """module docstring: the project's 16-bit LayerNorm rule, or the fp32 bound with the summed input's error (n terms, envelope E) carried through"""
    if is16(dtype):
        rms = y.pow(2).mean(-1, keepdim=True).sqrt()
        return LN_ULPS * ulp(y, dtype) + LN_FLOOR * ulp(rms, dtype).expand_as(y)
    b = 16 * UNIT * (gx.abs() + beta.to(F64).abs()) + RSTD_REL * gx.abs()
    if x is not None:                                   # the mean: a lane's 2 NIT additions and 6 shuffle levels, every element through each of them
        b = b + gamma.to(F64).abs() * rstd.unsqueeze(-1) * (2 * (x.shape[-1] // 128) + 6 + 8) * UNIT * x.abs().mean(-1, keepdim=True)
    if E is not None:
        dx, r = (n + 8) * UNIT * E, rstd.unsqueeze(-1)
        b = b + r * (gamma.to(F64).abs() * (dx + dx.mean(-1, keepdim=True)) + gx.abs() * r * dx.pow(2).mean(-1, keepdim=True).sqrt())
    return b


def gather64(src, csr, f=F64, defect=None):
    """(sum_e w_e src[idx_e], sum_e |w_e src[idx_e]|, edges per row) of a CSR gather in the float type f, edge by edge in the kernel's order"""
    ptr, idx, w = (None if t is None else t.cpu() for t in csr)
    s = src.to(f)
    n = ptr.numel() - 1
    deg = (ptr[1:] - ptr[:-1]).long()
    acc, env = torch.zeros(n, s.shape[1], dtype=f, device=s.device), torch.zeros(n, s.shape[1], dtype=f, device=s.device)
    for j in range(int(deg.max()) if n else 0):
        rows = (deg > j).nonzero().squeeze(1)
        e = ptr[rows].long() + (0 if defect == "first weight" else j)
        wv = torch.ones(rows.numel(), dtype=f) if w is None else w[e].to(f)
        term = wv.to(s.device)[:, None] * s[idx[ptr[rows].long() + j].long().to(s.device)]
        acc[rows.to(s.device)] += term
        env[rows.to(s.device)] += term.abs()
    return acc, env, deg.to(s.device)


def smallk_pre64(o):
    """z = b + x W^T and its envelope, float64"""
    x, W, b = o.x.to(F64), o.W.to(F64), o.b.to(F64)
    return b + x @ W.T, b.abs() + x.abs() @ W.abs().T


def lndot64(o):
    """(logit, bound): dot(LN(Y) gamma + beta, w2) + b2 -- an H-term fp32 sum of the fp32 LayerNorm's elements"""
    Y, w2, b2 = o.Y.to(F64), o.w2.to(F64), o.b2.to(F64)
    y, gx, rstd = ln64(Y, o.gamma, o.beta)
    ey = gx.abs() + o.beta.to(F64).abs()
    return y @ w2 + b2, (o.H + 8) * UNIT * (ey @ w2.abs() + b2.abs()) + ln_bound(y, gx, rstd, o.gamma, o.beta, F32, x=Y) @ w2.abs()


def headmean64(P, g, base=None):
    """(mean over heads [B, inner], its bound, dP [B, nh, inner] (+ base), its bound)"""
    P, nh = P.to(F64), P.shape[1]
    old = base.to(F64) if base is not None else torch.zeros_like(P)
    v = (g.to(F64) / nh)[:, None].expand_as(old)
    return P.sum(1) / nh, (nh + 8) * UNIT * P.abs().sum(1) / nh, old + v, (2 + 8) * UNIT * (old.abs() + v.abs())


def softmax_ref(c, o):
    """(P, d = x - max, dx) [B, nh, Nq, Nk] in float64; masked scores are -10000 + S scale rounded to fp32 (the additive-mask contract)"""
    S = o.S[..., :c.Nk]
    x, es = S.to(F64) * SCALE, (S.to(F64) * SCALE).abs()
    if o.kmask is not None:
        masked = (o.kmask == 0)[:, None, None, :].expand_as(x)
        x = torch.where(masked, (S * SCALE + NEG).to(F32).to(F64), x)
    if o.dist is not None:
        sw, sb = o.sw.to(F64), o.sb.to(F64)
        x = x + (sw * o.dist.to(F64) + sb)[:, None]
        es = es + ((sw * o.dist.to(F64)).abs() + sb.abs())[:, None]
    d = x - x.max(-1, keepdim=True).values
    P = torch.softmax(x, -1)
    return P, d, (3 + 8) * UNIT * es


def softmax_bound(c, P, d, dx, dtype):
    live = P > 0
    ds = torch.where(live, dx, torch.zeros_like(dx)).amax(-1, keepdim=True)
    own = 3 * d.abs() + 2
    rel = 2 * ds + (own + (P * own).sum(-1, keepdim=True) + c.Nk + 1) * U24
    return P * rel + ulp(P, dtype) + TINY


def softmax_bwd_ref(c, o, Pst):
    """(dS, bound(dS), dsw, bound, dsb, bound) from the stored probabilities Pst [B, nh, Nq, >= Nk]"""
    P, g = Pst[..., :c.Nk].to(F64), o.dP[..., :c.Nk].to(F64)
    s, sa = (P * g).sum(-1, keepdim=True), (P * g).abs().sum(-1, keepdim=True)
    d = P * (g - s)
    bd = P * (c.Nk + 8) * UNIT * sa + (2 + 8) * UNIT * P * (g.abs() + s.abs())
    out = [d * SCALE, bd * SCALE]
    if o.dist is not None:
        n = 8 + 6 + 4 + -(-(c.B * c.nh * c.Nq) // 4)
        dd = d * o.dist.to(F64)[:, None]
        out += [dd.sum(), (n + 8) * UNIT * dd.abs().sum() + (bd * o.dist.to(F64)[:, None]).sum(), d.sum(), (n + 8) * UNIT * d.abs().sum() + bd.sum()]
    return out


def pano_ref(x, lens, wf, bf, dtype, P=None):
    """adaptive panorama fusion in float64 from the values the kernel reads, with its bounds.  With u32 = 2^-24 and u the storage type's unit
    roundoff (2^-8 / 2^-11 / 2^-24):
      score     an H-term fp32 dot product + bias:                 ds <= (H + 2) u32 (sum |x wf| + |bf|)
      p         e = exp(s - max): the subtraction (span u32, span = max valid |s - max|), the fast exp's argument scaling (2 span u32) and its
                result (2 u32); the shared max cancels in e / sum e, numerator and denominator each carry ds and e's error; then the V-term
                sum and one division:                              dp / p <= 2 ds + (6 span + 4) u32 + (V + 1) u32
      fused     a V-term fp32 sum of p x, rounded once to storage: u |ref| + (dp / p + (V + 1) u32) sum |p x|
      pmean     nh fp32 additions and one division:                (nh + 1) u32 mean |P|
    returns p64, dp (relative), fused, bound(fused), pmean, bound(pmean)"""
    N, V, H = x.shape
    u32 = U24
    u = {torch.float32: u32, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]
    xd, wd = x.double(), wf.double()
    valid = torch.arange(V, device=x.device)[None] < lens[:, None]
    s = xd @ wd + bf.double()
    ds = ((H + 2) * u32 * ((xd.abs() @ wd.abs()) + bf.double().abs())).masked_fill(~valid, 0).amax(1, keepdim=True)
    sm = s.masked_fill(~valid, -1e300)
    span = (sm.amax(1, keepdim=True) - sm).masked_fill(~valid, 0).amax(1, keepdim=True)
    p64 = torch.softmax(s.masked_fill(~valid, float("-inf")), -1)
    dp = 2 * ds + (6 * span + 4) * u32 + (V + 1) * u32
    ref = (p64[..., None] * xd).sum(1)
    env = (p64[..., None] * xd.abs()).sum(1)
    bound = u * ref.abs() + (dp + (V + 1) * u32) * env + (2.0 ** -25 if dtype == torch.float16 else 0.0)
    r = SimpleNamespace(p=p64, dp=dp, fused=ref, bound=bound, pmean=None, pbound=None, xd=xd)
    if P is not None:
        nh = P.shape[1]
        r.pmean, r.pbound = P.double().mean(1), (nh + 1) * u32 * P.double().abs().mean(1)
    return r


# ---- checks ---------------------------------------------------------------------------------------------------------------------------------------
def check(who, name, k, ref, bound, tag, stats=None):
    """|k - ref| <= bound per element; every element the kernel writes is finite; records the worst ratio under (kernel, output, storage type)"""
    k = k.to(F64).to(ref.device)
    assert k.shape == ref.shape, f"{tag} {name}: shape {tuple(k.shape)} against {tuple(ref.shape)}"
    assert torch.isfinite(k).all(), f"{tag} {name}: non-finite elements where the kernel writes"
    d = (k - ref).abs()
    bound = bound if torch.is_tensor(bound) else torch.full_like(ref, bound)
    pos = bound > 0
    worst = (d[pos] / bound[pos]).max().item() if pos.any() else 0.0
    if stats is not None:
        key = (who[0], name, who[1])
        stats[key] = max(stats.get(key, 0.0), worst)
    bad = d > bound
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{tag} {name}: {int(bad.sum())} of {bad.numel()} elements beyond the bound (worst ratio {worst:.3g}); first at {list(i)}: "
                             f"kernel {k[i].item():.9g} ref {ref[i].item():.9g} bound {bound[i].item():.3g}")


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                                                                      b.view(torch.int16 if b.element_size() == 2 else torch.int32))


def verify_ln(who, o, outs, dtype, tag, stats=None, pre=""):
    """ln_fwd: out (and rstd) from the stored operands"""
    ts = ln_terms(o, F64)
    x, E, n = sum(ts), sum(t.abs() for t in ts), len(ts)
    if not o.do_ln:
        return check(who, pre + "sum", outs[pre + "out"], x, (n + 8) * UNIT * E + ulp(x, dtype), tag, stats)
    y, gx, rstd = ln64(x, o.gamma, o.beta)
    check(who, pre + "out", outs[pre + "out"], y, ln_bound(y, gx, rstd, o.gamma, o.beta, dtype, n, E, x), tag, stats)
    if o.want_rstd:
        check(who, pre + "rstd", outs[pre + "rstd"], rstd, RSTD_REL * rstd, tag, stats)


def verify_smallk(who, o, out, rstd_k, dtype, tag, stats=None, names=("out", "rstd")):
    z, E = smallk_pre64(o)
    y, gx, rstd = ln64(z, o.gamma, o.beta)
    check(who, names[0], out, y, ln_bound(y, gx, rstd, o.gamma, o.beta, dtype, o.Kin + 1, E, z), tag, stats)
    check(who, names[1], rstd_k, rstd, RSTD_REL * rstd, tag, stats)


def verify_gather(who, name, p, out, dtype, tag, stats=None):
    """csr_gather / one problem of csr_gather_multi: rows without an edge hold zeros (store) or their old value bit for bit (accumulate)"""
    a1, e1, d1 = gather64(p.src, p.csr)
    two = getattr(p, "csr2", None) is not None
    a2, e2, d2 = gather64(p.src2, p.csr2) if two else (torch.zeros_like(a1), torch.zeros_like(e1), torch.zeros_like(d1))
    old = p.base.to(F64) if p.base is not None else torch.zeros_like(a1)
    ref, n = old + a1 + a2, (d1 + d2 + 1).to(F64).unsqueeze(-1)
    bound = (n + 8) * UNIT * (old.abs() + e1 + e2) + ulp(ref, dtype)
    if two:                                             # the value after the first source is rounded to storage before the second is added
        first = (p.base is None) | (d1 > 0)
        bound = bound + torch.where((first & (d2 > 0)).unsqueeze(-1), ulp(old + a1, dtype), torch.zeros_like(ref))
    check(who, name, out, ref, bound, tag, stats)
    empty = (d1 + d2) == 0
    if empty.any():
        want = p.base[empty.to(p.base.device)] if p.base is not None else torch.zeros_like(out[empty.to(out.device)])
        assert same(out[empty.to(out.device)], want), f"{tag} {name}: a row without an edge is not {'untouched' if p.base is not None else 'zero'}"


def verify(c, dt, o, outs, tag, stats=None):
    """every check of one case: outs = the kernel's (or the emulation's) outputs by name, in the storage type"""
    dtype, k = DTYPES[dt], c.kind
    who = (k, dt)
    if k == "ln":
        return verify_ln(who, o, outs, dtype, tag, stats)
    if k == "smallk":
        return verify_smallk(who, o, outs["out"], outs["rstd"], dtype, tag, stats)
    if k == "lndot":
        ref, bound = lndot64(o)
        return check(who, "logit", outs["logit"], ref, bound, tag, stats)
    if k == "csr":
        return verify_gather(who, "out", o, outs["out"], dtype, tag, stats)
    if k == "csrm":
        for i, p in enumerate(o.probs):
            verify_gather(who, "out", p, outs[f"out{i}"], dtype, f"{tag} problem {i}", stats)
        return
    if k == "softmax":
        Nk = c.Nk
        P, d, dx = softmax_ref(c, o)
        for name in ("P", "dS"):
            assert (outs[name][..., Nk:] == 0).all(), f"{tag} {name}: pad columns {Nk}..{c.ldp} are not zero"
        check(who, "P", outs["P"][..., :Nk], P, softmax_bound(c, P, d, dx, dtype), tag, stats)
        if c.allmask:
            row = outs["P"][c.B - 1, ..., :Nk].to(F64)
            assert (row >= 0).all(), f"{tag} P: negative probability in the fully masked sample"
            dev = (row.sum(-1) - 1).abs().max().item()
            assert dev <= 2 * ulp_one(dtype), f"{tag} P: rows of the fully masked sample sum to 1 +- {dev:.3e}"
        r = softmax_bwd_ref(c, o, outs["P"])
        check(who, "dS", outs["dS"][..., :Nk], r[0], r[1] + ulp(r[0], dtype), tag, stats)
        if o.dist is not None:
            check(who, "dsprel_w", outs["dsw"].reshape(()), r[2], r[3], tag, stats)
            check(who, "dsprel_b", outs["dsb"].reshape(()), r[4], r[5], tag, stats)
        return
    if k == "headmean":
        mean, bm, dP, bd = headmean64(o.P, o.g, o.base)
        check(who, "mean", outs["out"], mean, bm, tag, stats)
        return check(who, "dP", outs["dP"], dP, bd, tag, stats)
    if k == "pano":
        r = pano_ref(o.x, o.lens, o.wf, o.bf, dtype, o.P)
        check(who, "probs", outs["probs"], r.p, r.dp * r.p, tag, stats)
        check(who, "fused", outs["fused"], r.fused, r.bound, tag, stats)
        if o.P is not None:
            check(who, "pmean", outs["pmean"], r.pmean, r.pbound, tag, stats)
        return
    if k == "node_in":
        for i, p in enumerate(o.probs):
            t = f"{tag} problem {i}"
            A = outs[f"A{i}"]
            verify_smallk(who, p, A, outs[f"rstd{i}"], dtype, t, stats, names=("A", "rstd"))
            # out = gathered + the STORED A + table row; the gathered sum is rounded to storage after each source (unobservable)
            ref, E, n = A.to(F64), A.to(F64).abs(), torch.ones(p.M, 1, dtype=F64, device=A.device)
            bound = torch.zeros_like(ref)
            if p.add0 is not None:
                ref, E, n = ref + p.add0.to(F64), E + p.add0.to(F64).abs(), n + 1
            if p.csr1 is not None:
                a1, e1, d1 = gather64(p.src1, p.csr1)
                ref, E, n, bound = ref + a1, E + e1, n + d1.unsqueeze(-1), bound + ulp(a1, dtype)
                if p.csr2 is not None:
                    a2, e2, d2 = gather64(p.src2, p.csr2)
                    ref, E, n = ref + a2, E + e2, n + d2.unsqueeze(-1)
                    bound = bound + torch.where((d2 > 0).unsqueeze(-1), ulp(a1 + a2, dtype), torch.zeros_like(ref))
            if p.tab is not None:
                tr = p.tab.to(F64)[p.tab_idx.long()]
                ref, E, n = ref + tr, E + tr.abs(), n + 1
            check(who, "out", outs[f"out{i}"], ref, bound + (n + 8) * UNIT * E + ulp(ref, dtype), t, stats)
        return
    if k == "embed_in":
        y, gx, rstd = ln64(o.P0.to(F64), o.g1, o.b1)
        check(who, "A1", outs["A1"], y, ln_bound(y, gx, rstd, o.g1, o.b1, dtype, x=o.P0.to(F64)), tag, stats)
        check(who, "rstd1", outs["rstd1"], rstd, RSTD_REL * rstd, tag, stats)
        verify_smallk(who, o, outs["A2"], outs["rstd2"], dtype, tag, stats, names=("A2", "rstd2"))
        ts = [outs["A1"].to(F64), outs["A2"].to(F64), o.nav_tab.to(F64)[o.nav_idx.long()], o.tok_tab.to(F64)[0].expand(c.M, c.H)]
        x, E = sum(ts), sum(t.abs() for t in ts)
        y, gx, rstd = ln64(x, o.g3, o.b3)
        check(who, "X0", outs["X0"], y, ln_bound(y, gx, rstd, o.g3, o.b3, dtype, 4, E, x), tag, stats)
        check(who, "rstd3", outs["rstd3"], rstd, RSTD_REL * rstd, tag, stats)
        if o.text is not None:
            verify_ln(who, o.text, outs, dtype, tag + " text half", stats, pre="t")
        return
    raise KeyError(k)


# ---- fp32 / 16-bit emulation of the kernels' dataflow, and the planted defects ----------------------------------------------------------------------
DEFECTS = ("last row of a workgroup", "last slice out of the statistics", "last k term", "table row", "pair gamma", "accumulate ignores old",
           "accumulate zeroes empty rows", "first weight", "key 64 it", "mask row", "pad columns", "nh - 1", "lens ignored", "last view dropped",
           "unrounded A", "b2 forgotten")


def case_rows(c):
    if c.kind in ("ln", "smallk", "lndot", "csr", "embed_in"):
        return c.M
    if c.kind == "softmax":
        return c.B * c.nh * c.Nq
    if c.kind == "node_in":
        return c.probs[0]["M"]
    if c.kind == "csrm":
        return c.probs[0]["M"]
    return 0


def defect_applies(c, dt, defect):
    """Each defect lives in a stated subset of the cases.  'unrounded A' does not exist in fp32 storage (the rounding it skips is the identity
    there) and is asserted on the add0 form, whose bound has no term for an unobservable rounding of a gathered sum."""
    k = c.kind
    if defect == "last row of a workgroup":
        return k in ROWS_PER_WG and case_rows(c) >= ROWS_PER_WG[k]
    if defect == "last slice out of the statistics":
        return k in ("ln", "smallk", "lndot", "node_in", "embed_in") and c.H >= 256 and not (k == "ln" and c.form == "sum only")
    if defect == "last k term":
        return k in ("smallk", "node_in", "embed_in")
    if defect == "table row":
        return (k == "ln" and c.form in ("text", "sum only") and c.M >= 2) or (k == "embed_in" and c.text and c.Mt >= 2)
    if defect == "accumulate ignores old":
        return k == "csr" and c.acc
    if defect == "accumulate zeroes empty rows":
        return k == "csr" and c.acc and c.M >= 2
    if defect == "first weight":
        return k == "csr" and not c.now and c.M >= 3
    if defect == "key 64 it":
        return k == "softmax" and c.Nk > 64
    if defect == "mask row":
        return k == "softmax" and c.kmask and c.Nk >= 4 and not c.allmask
    if defect == "pad columns":
        return k == "softmax" and c.ldp > c.Nk
    if defect == "nh - 1":
        return k == "headmean" and c.nh > 1
    if defect == "lens ignored":
        return k == "pano" and c.V >= 2
    if defect == "last view dropped":
        return k == "pano" and c.V % 4 == 1 and c.V > 1
    if defect == "unrounded A":
        return k == "node_in" and dt != "fp32" and c.probs[0]["form"] == "add0"
    if defect == "b2 forgotten":
        return k == "lndot"
    return False                                                   # 'pair gamma' lives in PAIRS (emulate_pair)


def emu_ln(x, gamma, beta, H, defect=None):
    """fp32 LayerNorm as the kernels compute it: sum / H, sum of squared deviations / H, rsqrt, affine map"""
    xs = x[..., :H - 128] if defect == "last slice out of the statistics" else x
    mean = xs.sum(-1, keepdim=True) / H
    rstd = torch.rsqrt((xs - mean).pow(2).sum(-1, keepdim=True) / H + EPS)
    return (x - mean) * rstd * gamma + beta, rstd.squeeze(-1)


def emu_smallk(o, defect=None):
    a = o.b.expand(o.M, o.H).clone()
    for k in range(o.Kin - (1 if defect == "last k term" else 0)):
        a = a + o.x[:, k:k + 1] * o.W[:, k]
    return a


def emu_ln_fwd(o, dtype, defect=None, gamma=None, pre=""):
    x = sum(ln_terms(o, F32, defect))
    if not o.do_ln:
        return {pre + "out": x.to(dtype)}
    y, rstd = emu_ln(x, o.gamma if gamma is None else gamma, o.beta, o.H, defect)
    return {pre + "out": y.to(dtype), **({pre + "rstd": rstd} if o.want_rstd else {})}


def emu_gather(p, dtype, defect=None):
    a1, _, d1 = gather64(p.src, p.csr, F32, defect)
    out = a1
    if p.base is not None:
        out = torch.where((d1 > 0).unsqueeze(-1), a1 if defect == "accumulate ignores old" else a1 + p.base.to(F32),
                          torch.zeros_like(a1) if defect == "accumulate zeroes empty rows" else p.base.to(F32))
    out = out.to(dtype)
    if getattr(p, "csr2", None) is not None:
        a2, _, d2 = gather64(p.src2, p.csr2, F32)
        out = torch.where((d2 > 0).unsqueeze(-1), (a2 + out.to(F32)).to(dtype), out)
    return out


def emulate(c, dt, o, defect=None):
    """the kernel's outputs by name, computed in fp32 torch with the kernel's rounding points, optionally with one planted defect"""
    dtype, k = DTYPES[dt], c.kind
    if k == "ln":
        outs = emu_ln_fwd(o, dtype, defect)
    elif k == "smallk":
        y, rstd = emu_ln(emu_smallk(o, defect), o.gamma, o.beta, o.H, defect)
        outs = {"out": y.to(dtype), "rstd": rstd}
    elif k == "lndot":
        y, _ = emu_ln(o.Y.to(F32), o.gamma, o.beta, o.H, defect)
        outs = {"logit": (y * o.w2).sum(-1) + (0.0 if defect == "b2 forgotten" else o.b2)}
    elif k == "csr":
        outs = {"out": emu_gather(o, dtype, defect)}
    elif k == "csrm":
        outs = {f"out{i}": emu_gather(p, dtype, defect) for i, p in enumerate(o.probs)}
    elif k == "softmax":
        B, nh, Nq, Nk, ldp = c.B, c.nh, c.Nq, c.Nk, c.ldp
        x = o.S[..., :Nk] * SCALE
        if o.kmask is not None:
            km = o.kmask
            if defect == "mask row":                               # b = row / Nq instead of row / (nh Nq)
                rows = torch.arange(B * nh * Nq).reshape(B, nh, Nq)
                km = o.kmask[(rows // Nq) % B]
                x = x + (km == 0).to(F32) * NEG
            else:
                x = x + ((km == 0).to(F32) * NEG)[:, None, None, :]
        if o.dist is not None:
            x = x + (o.sw * o.dist + o.sb)[:, None]
        live = torch.ones(Nk, dtype=torch.bool)
        if defect == "key 64 it":
            live[64::64] = False
        e = torch.exp(x - x[..., live].max(-1, keepdim=True).values) * live
        P32 = e * (1.0 / e.sum(-1, keepdim=True))
        fill = NAN if defect == "pad columns" else 0.0
        P, dS = torch.full((B, nh, Nq, ldp), fill, dtype=dtype), torch.full((B, nh, Nq, ldp), fill, dtype=dtype)
        P[..., :Nk] = P32.to(dtype)
        p, g = P[..., :Nk].to(F32), o.dP[..., :Nk]
        d = p * (g - (p * g).sum(-1, keepdim=True))
        dS[..., :Nk] = (d * SCALE).to(dtype)
        outs = {"P": P, "dS": dS}
        if o.dist is not None:
            outs["dsw"], outs["dsb"] = (d * o.dist[:, None]).sum().reshape(1), d.sum().reshape(1)
    elif k == "headmean":
        div = c.nh - 1 if defect == "nh - 1" else c.nh
        v = (o.g / div)[:, None].expand(c.B, c.nh, c.inner)
        outs = {"out": o.P.to(F32).sum(1) / div, "dP": (o.base + v) if o.base is not None else v.clone()}
    elif k == "pano":
        x = o.x.to(F32)
        V = c.V
        valid = torch.arange(V)[None] < (torch.full_like(o.lens, V) if defect == "lens ignored" else o.lens)[:, None]
        s = (x * o.wf).sum(-1) + o.bf + (~valid).to(F32) * NEG
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        p = e / e.sum(-1, keepdim=True)
        pv = p.clone()
        if defect == "last view dropped":
            pv[:, V - 1] = 0
        outs = {"probs": p, "fused": (pv[..., None] * x).sum(1).to(dtype)}
        if o.P is not None:
            outs["pmean"] = o.P.to(F32).sum(1) / o.nh
    elif k == "node_in":
        outs = {}
        for i, p in enumerate(o.probs):
            y, rstd = emu_ln(emu_smallk(p, defect), p.gamma, p.beta, p.H, defect)
            A = y.to(dtype)
            g = torch.zeros(p.M, p.H)
            if p.add0 is not None:
                g = p.add0.to(F32)
            elif p.csr1 is not None:
                g = emu_gather(SimpleNamespace(src=p.src1, csr=p.csr1, src2=p.src2, csr2=p.csr2, base=None), dtype).to(F32)
            out = g + (y if defect == "unrounded A" else A.to(F32))
            if p.tab is not None:
                out = out + p.tab.to(F32)[p.tab_idx.long()]
            outs.update({f"A{i}": A, f"rstd{i}": rstd, f"out{i}": out.to(dtype)})
    elif k == "embed_in":
        y1, r1 = emu_ln(o.P0.to(F32), o.g1, o.b1, o.H, defect)
        y2, r2 = emu_ln(emu_smallk(o, defect), o.gamma, o.beta, o.H, defect)
        A1, A2 = y1.to(dtype), y2.to(dtype)
        x = A1.to(F32) + A2.to(F32) + o.nav_tab.to(F32)[o.nav_idx.long()] + o.tok_tab.to(F32)[0]
        y3, r3 = emu_ln(x, o.g3, o.b3, o.H, defect)
        outs = {"A1": A1, "rstd1": r1, "A2": A2, "rstd2": r2, "X0": y3.to(dtype), "rstd3": r3}
        if o.text is not None:
            outs.update(emu_ln_fwd(o.text, dtype, defect, pre="t"))
    else:
        raise KeyError(k)
    if defect == "last row of a workgroup":                        # the row stays as the buffer was filled
        r = ROWS_PER_WG[k] - 1
        for name, t in outs.items():
            if name[0] == "t" or name in ("dsw", "dsb") or (k in ("node_in", "csrm") and not name.endswith("0")):
                continue
            (t.view(-1, t.shape[-1]) if t.dim() > 1 else t)[r] = NAN
    return outs


def emulate_pair(a, b, dt, defect=None):
    """the two problems of an ln_fwd pair launch; 'pair gamma': the second problem normalised with the first problem's gamma"""
    dtype = DTYPES[dt]
    oa, ob = operands(a, dt), operands(b, dt)
    return (oa, emu_ln_fwd(oa, dtype)), (ob, emu_ln_fwd(ob, dtype, gamma=oa.gamma if defect == "pair gamma" else None))
