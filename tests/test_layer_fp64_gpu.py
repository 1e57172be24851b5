"""The per-op layer path of host/engine.py -- MagicNet.self_layer_fwd / bwd, cross_layer_fwd / bwd, the per-op loops of text_bwd and
cross_bwd -- against fp64 at every width (H = 128, 256, 384, 768), in both 16-bit types, with and without dropout (-m gpu).

This host code composes the kernels that the other fp64 files pin one by one.  It is everything that runs in 16-bit at H = 256, 384 and 768,
and it is the yardstick tests/test_encoder_gpu.py holds the fused H = 128 forms to.  A small trainable MagicNet per width (2 text, 2 cross,
1 panorama layer, biases and LayerNorm gains randomised) is driven directly with hand-made ragged inputs; at H = 128 the fused forms are
switched off so that the per-op path runs.  Per case:

  forward   every saved tensor of every layer is recomputed in fp64 from the engine's own saved input to that stage and bounded per element
            (tests/_layer_ref64.check: c ulp + floor row-rms ulp); pad columns of every attention map are exactly 0
  backward  every parameter gradient of the stack by rel-L2 and cosine against fp64 autograd over the chained stages (same weights, same
            dropout masks, same d_top, same dP_init); d x per (sample, 16-row tile); d context and each layer's d kv per (sample, 16-key tile);
            rows at or beyond a sample's key count exactly as they were before the call
  branch    O.attn_fwd / attn_bwd / attn_bwd_ks / softmax_fwd / softmax_bwd / linear_ln / linear_lnbwd / ln_fwd / ln_bwd / add_ (and the
            GEMM residual, in-place dropout, residual linear) are wrapped with recorders; each case asserts the launches and the branch tags
            it must reach (`expected`), and test_every_named_branch_is_reached asserts that the cases together reach all of NEED

Cases (B = 4, ragged lengths 1, N-1, N and one ending a 16-row tile):
  self short   N = 41, with and without dP_init on the top block           fused attention forward and backward
  self long    N = 150; the top block once with dP_init at p = 0.1          tiled forward; key-split backward; five-GEMM backward with dP_init as
                                                                            the GEMM residual and the in-place fp32 dropout
  global       cross_fwd("global") with dist, Nq 20, Nk 150, K/V inside,    d sprel; key-split cross backward; context accumulation
               d_ctx_acc pre-filled
  kv given     two forward / backward calls into one dkv, Nk 150 and 40     write, then accumulate: in the key-split kernel (150), own buffer + add_ (40)
  seeded       dP_init on the top cross map, Nk 150, p = 0.1                unfused cross backward on the top block
  unfused      engine.FUSED_ATTN off, Nk 150, p = 0.1                       GEMM + softmax_fwd + dropout + GEMM forward, five-GEMM backward (no shape
                                                                            reaches them with the attention kernels on: every form refuses > 512 keys)
  control      fp32 storage at H = 768: self long with dP_init, global, kv given -- validates the reference independently of 16-bit rounding

Bounds.  Forward: BOUNDS / RSTD_REL of tests/_layer_ref64.py at every width, plus the derived allowance where a dense output is stored
before its LayerNorm (figures at FWD, end of file).  Backward at H = 128: BWD_BOUNDS / BWD_COS unchanged -- the calibration that ties this
file to tests/test_encoder_fp64_gpu.py.  Other widths, d context, d kv and d sprel: <= 3x the worst measured against fp64 on MI355X with
MEASURE = True over every case of this file (BWD below, figures beside it); fp32 control: 3x its measured worst (CONTROL, FWD_CONTROL).

Earlier finding.  In two of roughly 500 runs of a case, both at H = 768 / fp16 / self N = 150, d x of ONE (sample, 16-row tile) missed its bound: rel-L2
6.0e-3 and 3.8e-3 against 1.5e-3 (every other run: <= 7.84e-4, bitwise reproducible).  The first output that differed between repeats on bitwise equal inputs
was that of O.linear_dx with the gelu-derivative epilogue (M = 600, N = 3072, K = 768): one row x 16 columns, always in rows 12 or 14 (mod 16) of an MFMA tile.
tests/test_gemm_repeat_gpu.py now repeats that launch and its neighbours; the same signature showed on every launch at M >= 960 and went away when gemm_block
loaded the epilogue's aux operand without per-element branches (DESIGN.md section 4 has the figures).  The bounds stay where the measurements put them."""
from collections import Counter
from types import SimpleNamespace

import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import engine as ENG
from magic_amd.host import ops as O
from magic_amd.host.config import make_config
from magic_amd.host.params import ParamStore
from tests import _layer_ref64 as LH
from tests.test_dropout_gpu import seed_of
from tests.test_encoder_fp64_gpu import mask_of, ragged

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
WIDTHS = (128, 256, 384, 768)
B = 4
ACC0 = 1e-3                     # scale of the context accumulator's earlier content: that of the gradient it receives (printed under MEASURE)
MEASURE = False                 # True: record and print the worst error of every class per width, assert no bound (how BWD was set)

# rel-L2 bounds per width and storage type: "w" weights / gammas, "b" biases / betas, "dx" stack input per tile, "dctx" context rows per
# 16-key tile, "dkv" a layer's K/V rows per 16-key tile, "sprel" the graph-distance bias weight (a scalar: sum of dS dist over every row, the
# cancellation class).  Measured worst on MI355X over every case of this file (bf16 / fp16):
#   H     w                  b                  dx                 dctx               dkv                sprel
#   128   1.59e-2 / 2.09e-3  1.65e-2 / 2.66e-3  4.91e-3 / 6.74e-4  4.95e-3 / 6.51e-4  7.01e-3 / 8.11e-4  1.46e-3 / 5.47e-4
#   256   1.49e-2 / 2.04e-3  1.46e-2 / 2.17e-3  5.69e-3 / 7.07e-4  5.51e-3 / 7.13e-4  7.24e-3 / 8.60e-4  1.01e-2 / 8.75e-4
#   384   1.58e-2 / 1.94e-3  1.37e-2 / 2.00e-3  5.98e-3 / 7.55e-4  5.12e-3 / 6.17e-4  6.42e-3 / 7.99e-4  3.01e-2 / 2.39e-3
#   768   1.58e-2 / 1.99e-3  1.75e-2 / 2.11e-3  7.16e-3 / 7.84e-4  5.26e-3 / 6.86e-4  6.61e-3 / 8.24e-4  9.30e-3 / 1.32e-3
# The error does not grow with the width, so w / b / dx at EVERY width are tests/_layer_ref64.BWD_BOUNDS, the H = 128 bounds of the fused forms
# (1.4x - 2.1x the worst above: inside the 3x the other widths may take).  dctx / dkv / sprel: 2.5x the worst over the widths.  fp16 sits at
# 1/7.5 - 1/12.6 of bf16 in every class (the storage epsilons' ratio is 1/8): rounding noise, no scaling or sign error.
_MORE = {"bf16": {"dctx": 1.4e-2, "dkv": 1.8e-2, "sprel": 7.5e-2}, "fp16": {"dctx": 1.8e-3, "dkv": 2.2e-3, "sprel": 6.0e-3}}
BWD = {H: {dt: dict(LH.BWD_BOUNDS[dt], **_MORE[dt]) for dt in ("bf16", "fp16")} for H in WIDTHS}
# fp32 storage at H = 768 (the control), 3x the measured worst: w 1.01e-6, b 8.62e-7, dx 5.35e-7, dctx 4.67e-7, dkv 4.50e-7, sprel 5.27e-7
CONTROL = {"fp32": {"w": 3.0e-6, "b": 2.6e-6, "dx": 1.6e-6, "dctx": 1.4e-6, "dkv": 1.35e-6, "sprel": 1.6e-6}}
COVER = set()


# ---- model -----------------------------------------------------------------------------------------------------------------------------
MODELS = {}


def model(H, dtype):
    """one trainable MagicNet per (width, storage type), kept for the file: ParamStore + MagicNet, as the models build them"""
    key = (H, dtype)
    if key not in MODELS:
        cfg = make_config(H, role="student", vocab_size=64, max_position_embeddings=16, num_l_layers=2, num_x_layers=2, num_pano_layers=1,
                          hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
        store = ParamStore(ENG.trunk_specs(cfg), DEV, DTYPES[dtype], init_std=cfg.initializer_range, seed=3, requires_grad=True)
        g = torch.Generator().manual_seed(1)
        for name, shape, _ in store.specs:          # non-trivial biases / LayerNorm parameters, as test_encoder_fp64_gpu.bwd_student has them
            v = store.master(name)
            if name.endswith("bias") and len(shape) == 1:
                v.copy_((torch.randn(shape, generator=g) * 0.05).to(DEV))
            if "LayerNorm.weight" in name:
                v.add_((torch.randn(shape, generator=g) * 0.1).to(DEV))
        store.master("bert.global_encoder.sprel_linear.weight").fill_(-0.6)
        store.master("bert.global_encoder.sprel_linear.bias").fill_(0.25)
        store.shadow_clean = False
        MODELS[key] = SimpleNamespace(cfg=cfg, store=store, net=ENG.MagicNet(cfg, store, "bert."), H=H, I=cfg.intermediate_size,
                                      NH=cfg.num_attention_heads)
    return MODELS[key]


@pytest.fixture(autouse=True)
def per_op_path(monkeypatch):
    """the fused H = 128 forms off (they keep their own tests); the harness in this file's MEASURE mode"""
    for flag in ("FUSED_ENC", "FUSED_RBW", "FUSED_XENC"):
        monkeypatch.setattr(O, flag, False)
    monkeypatch.setattr(LH, "MEASURE", MEASURE)
    yield
    LH.STAT_PREFIX[0] = ""


# ---- recorders ---------------------------------------------------------------------------------------------------------------------------
COUNTED = ("attn_fwd", "attn_bwd", "attn_bwd_ks", "softmax_fwd", "softmax_bwd", "linear_ln", "linear_lnbwd", "ln_fwd", "ln_bwd", "add_")


class Recorder:
    """counts the launches of COUNTED and tags the branch each one (and the GEMM / dropout / linear glue around them) belongs to"""

    def __init__(self, mp):
        self.n, self.tags, self.lln, self.lnb, self.acc, self.on = Counter(), set(), [], [], [], True
        for name in COUNTED + ("gemm", "dropout", "linear_fwd", "linear_dx"):
            mp.setattr(O, name, self._wrap(name, getattr(O, name)))
        for name in ("rowbwd", "encoder_fwd", "xencoder_fwd", "chain_fwd"):
            mp.setattr(O, name, self._never(name))

    @staticmethod
    def _never(name):
        def f(*a, **kw):
            raise AssertionError(f"O.{name} launched: the per-op path was asked for")
        return f

    def _wrap(self, name, inner):
        def f(*a, **kw):
            if self.on:               # (off while the checks replay dropout masks through O.dropout)
                if name in COUNTED:
                    self.n[name] += 1
                getattr(self, "_" + name, lambda *a, **kw: None)(*a, **kw)
            return inner(*a, **kw)
        return f

    def _attn_fwd(self, *a, **kw):
        self.tags.add("fwd.tiled" if a[11] > 128 else "fwd.fused")

    def _softmax_fwd(self, *a, **kw):
        self.tags.add("fwd.unfused")

    def _attn_bwd_ks(self, *a, **kw):
        self.acc.append(bool(kw.get("accumulate_kv")))
        self.tags.add("bwd.ks.acc" if kw.get("accumulate_kv") else "bwd.ks")

    def _attn_bwd(self, *a, **kw):
        self.tags.add("bwd.fused")
        if a[14] is not None:
            self.tags.add("bwd.fused.dP")
        if kw.get("dist") is not None and kw.get("dsprel_w") is not None:
            self.tags.add("bwd.fused.dsprel")

    def _softmax_bwd(self, *a, **kw):
        self.tags.add("bwd.unfused")

    def _gemm(self, *a, **kw):
        if kw.get("residual") is not None and kw.get("batch", 1) > 1:        # (batched: an attention product, not a dense layer's GEMM)
            assert kw["residual"].data_ptr() == a[3].data_ptr() and a[3].dtype == torch.float32
            self.tags.add("bwd.unfused.dP_residual")

    def _dropout(self, x, out, *a, **kw):
        if x.data_ptr() == out.data_ptr():
            assert x.dtype == torch.float32
            self.tags.add("bwd.unfused.dropout_inplace")
        else:
            self.tags.add("fwd.unfused.dropout")

    def _linear_ln(self, x, W, *a, **kw):
        self.lln.append(tuple(W.shape))
        self.tags.add("dal.linear_ln")

    def _ln_fwd(self, *a, **kw):
        if kw.get("drop_in0") is not None:
            self.tags.add("dal.ln_drop")

    def _linear_fwd(self, *a, **kw):
        if kw.get("residual") is not None:
            self.tags.add("dal.residual")

    def _linear_lnbwd(self, x, W, *a, **kw):
        self.lnb.append((W.shape[1], W.shape[0]))
        self.tags.add("dx.lnbwd.split" if kw.get("drop") is not None else "dx.lnbwd")

    def _ln_bwd(self, *a, **kw):
        self.tags.add("dx.ln_bwd.split" if kw.get("drop_dx") is not None else "dx.ln_bwd")

    def _add_(self, *a, **kw):
        self.tags.add("x.acc.add")

    def _linear_dx(self, *a, **kw):
        if kw.get("out") is not None and kw.get("out") is kw.get("residual"):
            self.tags.add("x.ctx_acc")


# ---- what each case must reach -----------------------------------------------------------------------------------------------------------
def lln(H, K):
    return H in (128, 256, 384) and K <= 512


def lnb(H, K):
    return H in (128, 256) and K <= 512


def _attn_kind(half, Nq, Nk, p, dP, acc, n, tags, fused=True):
    """the attention backward of one block: counts into n, tags into tags"""
    if fused and half and 128 < Nk <= 512 and not dP:
        n["attn_bwd_ks"] += 1
        tags.add("bwd.ks.acc" if acc else "bwd.ks")
        return
    if fused and Nk <= 128 and Nq <= 128:
        n["attn_bwd"] += 1
        tags.update({"bwd.fused"} | ({"bwd.fused.dP"} if dP else set()))
    else:
        n["softmax_bwd"] += 1
        tags.update({"bwd.unfused"} | ({"bwd.unfused.dP_residual"} if dP else set()) | ({"bwd.unfused.dropout_inplace"} if p > 0 else set()))
    if acc:
        n["add_"] += 1
        tags.add("x.acc.add")


def expected(H, dtype, p, kind, N=None, Nk=None, dP=False, dist=False, kv_given=False, calls=1, fused=True):
    """(launch counts of COUNTED, branch tags) of one case, from host/engine.py's rules: `kind` "self": two self layers forward and the
    per-op loop of text_bwd; "cross": cross_fwd + cross_bwd, `calls` times (the second and later ones accumulate into dkv); fused False:
    engine.FUSED_ATTN off (no attention kernel: GEMM + softmax + dropout + GEMM forward, five GEMMs backward)"""
    I, half = 4 * H, dtype != "fp32"
    n, tags = Counter(), set()
    dense = [H, I] if kind == "self" else [H, H, I]                  # K of the dense in front of each LayerNorm of a layer
    back = [None, I, 3 * H, I] if kind == "self" else [None, 3 * H, I, I, H, H]   # K of the dense whose dx feeds each LayerNorm backward (None: d_top)
    for c in range(calls):
        for layer in range(2):
            for K in dense:
                if lln(H, K):
                    n["linear_ln"] += 1
                    tags.add("dal.linear_ln")
                else:
                    n["ln_fwd"] += 1
                    tags.add("dal.ln_drop" if p > 0 else "dal.residual")
        for K in back:
            pre = K is not None and lnb(H, K)
            n["linear_lnbwd" if pre else "ln_bwd"] += 1
            tags.add(("dx.lnbwd" if pre else "dx.ln_bwd") + (".split" if p > 0 else ""))
        tags.add("fuse_in.pre" if lnb(H, 3 * H) else "fuse_in.plain")
        if kind == "self":
            n["attn_fwd"] += 2
            tags.add("fwd.tiled" if N > 128 else "fwd.fused")
            _attn_kind(half, N, N, p, dP, False, n, tags)            # top block
            _attn_kind(half, N, N, p, False, False, n, tags)
            continue
        if fused:
            n["attn_fwd"] += 4                                       # self-attention (Nq <= 128) and cross-attention of the two layers
            tags.update({"fwd.fused", "fwd.tiled" if Nk > 128 else "fwd.fused"})
            n["attn_bwd"] += 2
            tags.update({"bwd.fused"} | ({"bwd.fused.dsprel"} if dist else set()))
        else:
            n["softmax_fwd"] += 4
            tags.update({"fwd.unfused"} | ({"fwd.unfused.dropout"} if p > 0 else set()))
            _attn_kind(half, N, N, p, False, False, n, tags, fused)
            _attn_kind(half, N, N, p, False, False, n, tags, fused)
        _attn_kind(half, N, Nk, p, dP, kv_given and c > 0, n, tags, fused)   # top block: the seed sits on ITS cross map
        _attn_kind(half, N, Nk, p, False, kv_given and c > 0, n, tags, fused)
        tags.add("x.kv_given" if kv_given else "x.ctx_acc")
        if dP:
            tags.add("x.dP_init")
    return n, tags


# the branches named in the issue this file answers: _attn_fwd (3), _attn_bwd (3, key-split with and without acc_kv, dP_init as the GEMM residual,
# in-place fp32 dropout), _dense_add_ln (3), _dx_into_ln / _through_ln (Pre pair or plain, fuse_in, the d_dense / d_sum split), cross_layer_bwd (6)
NEED = {"fwd.fused", "fwd.tiled", "fwd.unfused", "fwd.unfused.dropout",
        "bwd.ks", "bwd.ks.acc", "bwd.fused", "bwd.fused.dP", "bwd.unfused", "bwd.unfused.dP_residual", "bwd.unfused.dropout_inplace",
        "dal.linear_ln", "dal.ln_drop", "dal.residual",
        "dx.lnbwd", "dx.lnbwd.split", "dx.ln_bwd", "dx.ln_bwd.split", "fuse_in.pre", "fuse_in.plain",
        "x.kv_given", "x.acc.add", "x.ctx_acc", "x.dP_init", "bwd.fused.dsprel"}


def assert_branches(rec, want, m, tag):
    n, tags = want
    COVER.update(rec.tags)
    got = {k: rec.n[k] for k in COUNTED}
    if MEASURE:
        if got != {k: n[k] for k in COUNTED} or rec.tags != tags:
            print(f"[branches] {tag}: launches {got} expected {dict(n)}; tags only seen {sorted(rec.tags - tags)} only expected {sorted(tags - rec.tags)}")
        return
    assert got == {k: n[k] for k in COUNTED}, f"{tag}: launches {got}, expected {dict(n)}"
    assert rec.tags == tags, f"{tag}: branch tags only seen {sorted(rec.tags - tags)}, only expected {sorted(tags - rec.tags)}"
    assert all(lnb(m.H, K) and Hh == m.H for Hh, K in rec.lnb), rec.lnb                # linear_lnbwd only at 128 / 256 with K <= 512
    assert all(lln(m.H, K) and Hh == m.H for Hh, K in rec.lln), rec.lln                # linear_ln at 128 / 256 / 384 with K <= 512
    if m.H == 768:
        assert not rec.lnb and not rec.lln


# ---- drivers -----------------------------------------------------------------------------------------------------------------------------
def nan(*shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _rows(g, M, H, dt, s=1.0):
    return (torch.randn(M, H, generator=g) * s).to(dt).to(DEV)


def _seed_map(g, Bn, NH, Nq, Nk):
    """dP_init: fp32 [B, heads, Nq, ldp], pad columns 0"""
    dP = torch.zeros(Bn, NH, Nq, ENG.rup(Nk))
    dP[..., :Nk] = torch.randn(Bn, NH, Nq, Nk, generator=g) * 0.1
    return dP.to(DEV)


def bounds_of(H, dtype):
    if MEASURE:
        return {dtype: dict.fromkeys(("w", "b", "dx", "dctx", "dkv", "sprel"), float("inf"))}
    return CONTROL if dtype == "fp32" else BWD[H]


def fwd_bounds(H, dtype):
    return FWD_CONTROL if dtype == "fp32" else FWD.get(H)


def run_self(H, dtype, p, N, with_dP, mp):
    """two self_layer_fwd and the per-op loop of text_bwd (self_layer_bwd with fuse_in); returns what the checks need"""
    m, dt = model(H, dtype), DTYPES[dtype]
    n, rec = m.net, Recorder(mp)
    g = torch.Generator().manual_seed(N + 7 * H)
    lens = ragged(B, N)
    kmask = mask_of(lens, N)
    kmask_d = kmask.to(torch.uint8).to(DEV).contiguous()
    x = _rows(g, B * N, H, dt)
    m.store.sync_shadow()
    seed = seed_of(4321, 99)
    n.set_dropout(seed if p > 0 else None, p, p)
    fmt = n.p + "lang_encoder.layer.{}."
    layers, h = [], x
    for i in range(2):
        layers.append(n.self_layer_fwd(fmt.format(i), h, B, N, kmask_d, sum(lens), n._flops_attn(lens, lens)))
        h = layers[-1].out
    sg = LH.engine_segment(n, SimpleNamespace(layers=layers), fmt, kmask, dt, p, H)
    d_top = _rows(g, B * N, H, dt, 0.1)
    dP = _seed_map(g, B, m.NH, N, N) if with_dP else None
    m.store.zero_grad()
    O.defer_dw(True)
    d = d_top.clone()
    for i in reversed(range(2)):
        prev = n._out_ln_desc(fmt.format(i - 1), layers[i - 1]) if i > 0 else None
        d = n.self_layer_bwd(fmt.format(i), layers[i], d, dP.clone() if (dP is not None and i == 1) else None, fuse_in=prev)
        if i == 1:
            rec.tags.add("fuse_in.pre" if isinstance(d, tuple) else "fuse_in.plain")
    O.flush_dw()
    torch.cuda.synchronize()
    rec.on = False
    assert torch.is_tensor(d)
    return m, rec, sg, fmt, d_top, dP, d, seed


def check_self(H, dtype, p, N, with_dP, mp):
    tag = f"H={H} {dtype} p={p} self N={N} dP_init={with_dP}"
    m, rec, sg, fmt, d_top, dP, dx, seed = run_self(H, dtype, p, N, with_dP, mp)
    assert_branches(rec, expected(H, dtype, p, "self", N=N, dP=with_dP), m, tag)
    LH.STAT_PREFIX[0] = f"H{H} "
    LH.check_segment(sg, p, seed, tag, H, m.NH, m.I, bounds=fwd_bounds(H, dtype), rstd_rel=RSTD.get(dtype),
                     stored_dense=lambda K: not lln(H, K))
    rdx, rw = LH.stack_reference(sg, p, seed, d_top, dP, H, m.NH)
    LH.check_param_grads(m, fmt, sg, rw, dtype, tag, H, bounds=bounds_of(H, dtype))
    LH.check_dx_tiles(dx, rdx, sg, dtype, tag, H, bounds=bounds_of(H, dtype))
    return m, sg, fmt, rdx, rw, dx


class CrossRun:
    """cross_fwd / cross_bwd of one co-attention encoder driven directly: `call()` is one forward + backward on fresh queries"""

    def __init__(self, H, dtype, p, Nq, Nk, mp, which="local", with_dist=False, kv_given=False, with_dP=False, Bn=B, fused=True):
        self.fused = fused
        if not fused:
            mp.setattr(ENG, "FUSED_ATTN", False)
        self.m, self.dt, self.dtype, self.p, self.H = model(H, dtype), DTYPES[dtype], dtype, p, H
        self.Nq, self.Nk, self.B, self.which, self.kv_given, self.with_dP = Nq, Nk, Bn, which, kv_given, with_dP
        m, n, dt = self.m, self.m.net, self.dt
        self.rec = Recorder(mp)
        self.g = g = torch.Generator().manual_seed(Nq + 3 * Nk + 7 * H)
        self.qlens, self.klens = ragged(Bn, Nq), ragged(Bn, Nk)[::-1]
        self.qmask, self.cmask = mask_of(self.qlens, Nq), mask_of(self.klens, Nk)
        self.qmask_d, self.cmask_d = (t.to(torch.uint8).to(DEV).contiguous() for t in (self.qmask, self.cmask))
        self.cx = _rows(g, Bn * Nk, H, dt)
        self.dist = (torch.rand(Bn, Nq, Nq, generator=g) * 6).to(DEV) if with_dist else None
        self.fmt = n.p + ("global_encoder." if which == "global" else "local_encoder.") + "encoder.crossattention.{}."
        m.store.sync_shadow()
        self.kv = None
        if kv_given:          # the navigator's per-episode cache (model_nav.text_kv): each layer's K | V projection of the context, computed once
            self.kv = nan(2, Bn * Nk, 2 * H, dtype=dt)
            for i in range(2):
                lp = self.fmt.format(i)
                kvl = n.lin(lp + "crossattention.self.key.weight", lp + "crossattention.self.key.bias", rows=2 * H, cols=H)
                O.linear_fwd(self.cx, kvl.W, kvl.b, Bn * Nk, out=self.kv[i])
            self.dkv = nan(2, Bn * Nk, 2 * H, dtype=dt)
        self.acc0 = _rows(g, Bn * Nk, H, dt, ACC0)                # what the context accumulator holds before the first call
        self.d_ctx = self.acc0.clone()
        sp = m.store.master("bert.global_encoder.sprel_linear.weight"), m.store.master("bert.global_encoder.sprel_linear.bias")
        self.sprel = (sp[0].item(), sp[1].item()) if with_dist else None
        self.ncalls = 0
        m.store.zero_grad()

    def call(self):
        m, n, dt, H, Bn, Nq, Nk, g = self.m, self.m.net, self.dt, self.H, self.B, self.Nq, self.Nk, self.g
        x = _rows(g, Bn * Nq, H, dt)
        self.rec.on = True
        seed = seed_of(4321 + self.ncalls, 99)
        n.set_dropout(seed if self.p > 0 else None, self.p, self.p)
        c = n.cross_fwd(self.which, {"B": Bn}, x, Nq, self.qmask_d, self.qlens, sum(self.qlens), self.cx, Nk, self.cmask_d, self.klens,
                        sum(self.klens), dist=self.dist, kv=self.kv)
        sg = LH.engine_cross_segment(n, c, self.fmt, self.qmask, self.cmask, dt, self.p, H, sprel=self.sprel)
        d_top = _rows(g, Bn * Nq, H, dt, 0.1)
        dP = _seed_map(g, Bn, m.NH, Nq, Nk) if self.with_dP else None
        O.defer_dw(True)
        dx = n.cross_bwd(c, d_top.clone(), self.d_ctx, dP_init=dP.clone() if dP is not None else None,
                         dkv=self.dkv if self.kv_given else None, acc_kv=self.ncalls > 0)
        O.flush_dw()
        torch.cuda.synchronize()
        self.rec.on = False
        assert torch.is_tensor(dx)
        self.rec.tags.add("fuse_in.pre" if lnb(H, 3 * H) and self.rec.lnb.count((H, 3 * H)) > self.ncalls else "fuse_in.plain")
        self.rec.tags.add("x.kv_given" if self.kv_given else "x.ctx_acc")
        if dP is not None:
            self.rec.tags.add("x.dP_init")
        self.ncalls += 1
        return SimpleNamespace(sg=sg, d_top=d_top, dP=dP, dx=dx, seed=seed, dkv=self.dkv.clone() if self.kv_given else None)

    def tag(self):
        return (f"H={self.H} {self.dtype} p={self.p} cross {self.which} Nq={self.Nq} Nk={self.Nk} kv_given={self.kv_given} "
                f"dP_init={self.with_dP}")

    def want(self):
        return expected(self.H, self.dtype, self.p, "cross", N=self.Nq, Nk=self.Nk, dP=self.with_dP, dist=self.dist is not None,
                        kv_given=self.kv_given, calls=self.ncalls, fused=self.fused)

    def reference(self, r, dkv0=None, without=()):
        return LH.engine_cross_reference(r.sg, self.p, r.seed, r.d_top, self.H, self.m.NH, dP=r.dP, kv_given=self.kv_given,
                                         d_ctx0=None if self.kv_given else self.acc0, dkv0=dkv0, without=without)

    def check_forward(self, r):
        LH.STAT_PREFIX[0] = f"H{self.H} "
        LH.check_segment(r.sg, self.p, r.seed, self.tag(), self.H, self.m.NH, self.m.I, bounds=fwd_bounds(self.H, self.dtype),
                         rstd_rel=RSTD.get(self.dtype), stored_dense=lambda K: not lln(self.H, K))

    def check_rows(self, r, ref, dkv=None):
        """d x, d context / d kv per tile; key rows beyond a sample's length exactly untouched"""
        bd, tag = bounds_of(self.H, self.dtype), self.tag()
        LH.check_dx_tiles(r.dx, ref.dx, r.sg, self.dtype, tag, self.H, bounds=bd)
        beyond = ~self.cmask.view(-1)
        if self.kv_given:
            assert torch.equal(self.d_ctx, self.acc0), f"{tag}: the context accumulator was written although K/V were given"
            for j in range(2):
                k = (r.dkv if dkv is None else dkv)[j]
                assert (k.cpu()[beyond] == 0).all(), f"{tag} layer {j}: d kv of keys beyond a sample's length is not exactly 0"
                LH.check_dx_tiles(k, ref.dkv[j], r.sg, self.dtype, f"{tag} layer {j}", self.H, bounds=bd, cls="dkv", rows=self.Nk, what="d kv")
        else:
            assert torch.equal(self.d_ctx.cpu()[beyond], self.acc0.cpu()[beyond]), f"{tag}: context rows beyond a sample's length changed"
            if MEASURE:
                a0 = self.acc0.double().cpu().view_as(ref.dctx)
                print(f"[scale] {tag}: |d context of this call| / |earlier content| = {((ref.dctx - a0).norm() / a0.norm()).item():.3g}")
            LH.check_dx_tiles(self.d_ctx, ref.dctx, r.sg, self.dtype, tag, self.H, bounds=bd, cls="dctx", rows=self.Nk, what="d context")

    def check_params(self, sg, grads, dsprel=None, grad=None):
        bd, tag = bounds_of(self.H, self.dtype), self.tag()
        LH.check_param_grads(self.m, self.fmt, sg, grads, self.dtype, tag, self.H, grad=grad, names=LH.CROSS_PNAMES, bounds=bd,
                             skip=tuple(pn for pn, _, _ in LH.KV_PNAMES) if self.kv_given else ())
        if dsprel is not None:
            st = self.m.store
            kw = st.g("bert.global_encoder.sprel_linear.weight").double().cpu().reshape(())
            kb = st.g("bert.global_encoder.sprel_linear.bias").double().cpu().reshape(())
            rel = ((kw - dsprel[0]).abs() / dsprel[0].abs()).item()
            key = (self.dtype, LH.STAT_PREFIX[0] + "grad sprel weight")
            LH.STATS[key] = (max(LH.STATS.get(key, (0.0, 0.0))[0], rel), 0.0)
            top = max(v.norm().item() for d in grads for v in d.values())
            # the bias shifts every logit of a row alike: analytically zero, noise on both sides (as the key bias in check_param_grads)
            assert kb.abs().item() < 1e-3 * top and dsprel[1].abs().item() < 1e-6 * top, (tag, kb.item())
            if not MEASURE:
                assert rel < bd[self.dtype]["sprel"], f"{tag} sprel_linear.weight: relative error {rel:.3e}"


def _sum_grads(a, b):
    return [{k: v + gb[k] for k, v in ga.items()} for ga, gb in zip(a, b)]


def check_cross(H, dtype, p, Nq, Nk, mp, **kw):
    """one call (K/V projected inside) or two (kv given: write, then accumulate into the same dkv)"""
    run = CrossRun(H, dtype, p, Nq, Nk, mp, **kw)
    r1 = run.call()
    run.check_forward(r1)
    ref1 = run.reference(r1)
    run.check_rows(r1, ref1)
    if not run.kv_given:
        assert_branches(run.rec, run.want(), run.m, run.tag())
        run.check_params(r1.sg, ref1.grads, ref1.dsprel)
        return run, r1, ref1, None, None
    r2 = run.call()
    assert_branches(run.rec, run.want(), run.m, run.tag())
    run.check_forward(r2)
    ref2 = run.reference(r2, dkv0=ref1.dkv)
    run.check_rows(r2, ref2)
    run.check_params(r2.sg, _sum_grads(ref1.grads, ref2.grads))                # the parameter gradients of both calls add up in the store
    return run, r1, ref1, r2, ref2


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
HALF = [(H, dt) for H in WIDTHS for dt in ("bf16", "fp16")]
HALF_IDS = [f"H{H}-{dt}" for H, dt in HALF]
SELF_CASES = [("short", 41, False, 0.0), ("short", 41, False, 0.1), ("short+dP", 41, True, 0.0), ("short+dP", 41, True, 0.1),
              ("long", 150, False, 0.0), ("long", 150, False, 0.1), ("long+dP", 150, True, 0.1)]
# (id, Nq, Nk, p values, CrossRun keywords)
CROSS_CASES = [("global", 20, 150, (0.0, 0.1), dict(which="global", with_dist=True)),
               ("kv150", 20, 150, (0.0, 0.1), dict(kv_given=True)),
               ("kv40", 20, 40, (0.0, 0.1), dict(kv_given=True)),
               ("seeded", 20, 150, (0.1,), dict(with_dP=True)),
               ("unfused", 20, 150, (0.1,), dict(fused=False))]
CROSS_PARAMS = [(c[0], c[1], c[2], p, c[4]) for c in CROSS_CASES for p in c[3]]
CONTROL_CASES = [("self", 150, 0.1), ("global", 20, 0.1), ("kv150", 20, 0.0)]


@pytest.mark.parametrize("case", SELF_CASES, ids=[f"{c[0]}-p{c[3]}" for c in SELF_CASES])
@pytest.mark.parametrize("H,dtype", HALF, ids=HALF_IDS)
def test_self_layers_vs_fp64(H, dtype, case, monkeypatch):
    _, N, with_dP, p = case
    check_self(H, dtype, p, N, with_dP, monkeypatch)


@pytest.mark.parametrize("case", CROSS_PARAMS, ids=[f"{c[0]}-p{c[3]}" for c in CROSS_PARAMS])
@pytest.mark.parametrize("H,dtype", HALF, ids=HALF_IDS)
def test_cross_layers_vs_fp64(H, dtype, case, monkeypatch):
    _, Nq, Nk, p, kw = case
    check_cross(H, dtype, p, Nq, Nk, monkeypatch, **kw)


@pytest.mark.parametrize("case", CONTROL_CASES, ids=[c[0] for c in CONTROL_CASES])
def test_fp32_control_at_h768(case, monkeypatch):
    """the same harness on fp32 storage (per-op, unfused attention backward at 150 keys): validates the reference independently of 16-bit rounding"""
    kind, N, p = case
    if kind == "self":
        check_self(768, "fp32", p, N, True, monkeypatch)
    elif kind == "global":
        check_cross(768, "fp32", p, N, 150, monkeypatch, which="global", with_dist=True)
    else:
        check_cross(768, "fp32", p, N, 150, monkeypatch, kv_given=True)


@pytest.mark.parametrize("H,dtype", [(h, dt) for h in (128, 768) for dt in ("bf16", "fp16")], ids=lambda v: str(v))
def test_bounds_catch_planted_defects(H, dtype, monkeypatch):
    """applied to copies of the GPU result (or to the reference), each must fail: one 16-row tile of d x taken from the neighbouring sample,
    the first call's d kv subtracted from the accumulated buffer, dP_init's contribution missing from the reference"""
    kept = dict(LH.STATS)
    with monkeypatch.context() as mp:
        run, r1, ref1, r2, ref2 = check_cross(H, dtype, 0.1, 20, 150, mp, kv_given=True)
    t = r2.dx.clone().view(run.B, run.Nq, H)
    t[1, :16] = t[2, :16]
    with pytest.raises(AssertionError):
        LH.check_dx_tiles(t, ref2.dx, r2.sg, dtype, "tile from the neighbouring sample", H, bounds=BWD[H])
    with pytest.raises(AssertionError):
        run.check_rows(r2, ref2, dkv=(r2.dkv.float() - r1.dkv.float()).to(run.dt))
    with monkeypatch.context() as mp:
        run, r, ref, _, _ = check_cross(H, dtype, 0.1, 20, 150, mp, with_dP=True)
    bad = run.reference(r, without=("dP",))
    with pytest.raises(AssertionError):
        run.check_params(r.sg, bad.grads)
    with pytest.raises(AssertionError):
        LH.check_dx_tiles(run.d_ctx, bad.dctx, r.sg, dtype, "reference without dP_init", H, bounds=BWD[H], cls="dctx", rows=run.Nk, what="d context")
    LH.STATS.clear()
    LH.STATS.update(kept)


def test_every_named_branch_is_reached():
    """the cases' expectations (each asserted against what its recorders saw) together cover every branch of NEED"""
    union = set()
    for H, dtype in HALF:
        for _, N, with_dP, p in SELF_CASES:
            union |= expected(H, dtype, p, "self", N=N, dP=with_dP)[1]
        for _, Nq, Nk, p, kw in CROSS_PARAMS:
            union |= expected(H, dtype, p, "cross", N=Nq, Nk=Nk, dP=kw.get("with_dP", False), dist=kw.get("with_dist", False),
                              kv_given=kw.get("kv_given", False), calls=2 if kw.get("kv_given") else 1, fused=kw.get("fused", True))[1]
    assert not NEED - union, f"no case is expected to reach {sorted(NEED - union)}"
    if COVER:                   # (this process ran cases: what their recorders saw)
        print(f"[branches] seen in this process: {sorted(COVER)}")


def test_zz_report_measured_worst():
    """prints (with -s) the worst error per width, class and storage type that this process measured (what BWD / CONTROL were set from)"""
    for key in sorted(LH.STATS, key=str):
        if key[1].startswith("H"):
            u, f = LH.STATS[key]
            print(f"fp64 layer check {key[0]:5s} {key[1]:32s} worst {u:10.4g}  floor needed {f:8.4f}")


# ---- forward bounds --------------------------------------------------------------------------------------------------------------------
# 16-bit storage, measured on MI355X over every case of this file (worst ulps of |ref| where |ref| >= the row's rms / floor needed beyond 1 ulp,
# in row-rms ulps), bf16 and fp16 at every width: qkv, q, kv, z <= 0.501 / 0.0005 (z at H = 768 sums K = 768 terms, out's dense K = 3072: no
# growth of the fp32-accumulation floor to speak of), P, Pc, ctx, cctx 0.5 / 0, Pd, Pdc 1.0 / 0.0003 (the mask's 1 / (1 - p) on a rounded P),
# g 1.60 / 0 (within check_gelu's input term).  All inside tests/_layer_ref64.BOUNDS, which therefore hold unchanged at every width (FWD = {}).
# a, c, out are correctly rounded (0.5 / 0) where magic_linear_ln produces them (H <= 384 and K <= 512).  Elsewhere the dense output is stored
# in 16-bit before magic_ln_fwd reads it -- a second rounding in FRONT of the LayerNorm: measured 1.54 ulp / 1.3 row-rms ulp on the output and
# 6.5e-4 relative on rstd (bf16).  That is no accumulation floor to scale: those sites get the first-order allowance of the stored tensor's half
# ulp pushed through the LayerNorm (tests/_layer_ref64.ln_input_rounding) on top of the unchanged 1 ulp + 0.003 and RSTD_REL.
FWD = {}
RSTD = {}
# fp32 storage (the control): fp32 accumulation is the whole error; (c, floor) = 3x the measured worst of each stage
FWD_CONTROL = {"qkv": (137, 174), "q": (47, 54), "kv": (143, 153), "z": (155, 162), "P": (21, 70), "Pc": (26, 90), "Pd": (24, 70), "Pdc": (28, 51),
               "ctx": (52, 84), "cctx": (47, 48), "a": (14, 21), "c": (16, 20), "out": (42, 72), "g": (5.2, 1.0)}
