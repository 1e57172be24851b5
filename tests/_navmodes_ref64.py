"""fp64 harness of the navigator's mode functions in 16-bit storage: shared by tests/test_navmodes_ref64_cpu.py (ties it to the oracle, shows that
every planted defect is visible) and tests/test_navmodes_fp64_gpu.py (the engine against it).  Importing this module needs no GPU.

What it pins is the HOST composition of host/model_nav.py + host/causal.py -- the `.to(T)` casts of incoming gradients, the attention-map seeds
(head_mean backward), the cls_embeds gather and its transpose, kv[:nl] / kv[nl:] and the K/V cache's gradient accumulation, the glocal fusion gate,
the `door` gate and the `type_1` prior of the causal blocks, Critic / _RowDotFn -- one level above the kernels, which have fp64 files of their own.

Model pairs (`pair`).  An oracle.nav_ref.RefVLNBert in fp64 and a VLNBert(compute_dtype=dt) with the same weights; biases and LayerNorm gains
randomised as tests/test_nav_h768_oracle_gpu._pair does.  The reference computes from the operands the engine reads.  Read from host/params.py and
host/engine.py: ParamStore keeps fp32 masters (`flat`) and ONE 16-bit shadow of the whole buffer (`shadow`, filled by sync_shadow); a kernel's
operand is 16-bit exactly where the host hands it `S.w(...)` / `Lin.W` (= `w_span`: views of the shadow) and fp32 where it hands it `S.master(...)`,
`Lin.b`, `Lin.Wm` or `LN.g / LN.b` (views of `flat`).  That gives two groups:

  rounded to dt (shadow)   every Linear weight read as `Lin.W`: all attention / FFN / head `net.0` / img_linear / KD / causal query, key, value,
                           output.dense matrices, the Critic's state2value.0.weight; every embedding table (word, position, token_type, nav_type,
                           gmap_step: `S.w(...)` in text_fwd / embeds_fwd / gmap_in_fwd)
  kept fp32 (masters)      every bias; every LayerNorm gamma / beta; the small-K and row-dot matrices read as `Lin.Wm`: loc_linear,
                           gmap_pos_embeddings.0, vp_pos_embeddings.0, pano_fuse_linear, the heads' `net.3` (H -> 1); sprel_linear; the `door`
                           gate's gate_x / gate_e; the Critic's state2value.3

Inputs: view_img_fts is rounded to dt (pano_forward_body casts it); the causal dictionaries and their priors are rounded to dt (HipLinear casts
its input, CausalBlock casts pz to the value rows' type); location / position features and pair distances stay fp32.

Loss (`loss_of`): CE on fused_logits as tests/test_nav_gpu.one_step has it, plus one fixed fp64 random linear functional per output in FUNCS, each
with its own seed, restricted to valid rows / unmasked columns / finite logits, and scaled to a gradient of norm 0.5 on its output (the CE's
gradient on the logits has norm <= sqrt(2 (B-1)) / B = 0.61 at B = 4): every backward input of every mode function carries a gradient of the CE's size.

Drivers.  `Tap` wraps either model and is handed to tests/test_nav_gpu.one_step / tests/test_causal_gpu.step in its place: it keeps the map inputs
of every navigation call (retain_grad: d gmap_img_embeds, d vp_img_embeds), the text embeddings, and -- `use_kv` -- computes `text_kv` once and passes
it to every navigation call of the episode (`language` is answered from its memory on the second call).  `Ref64` is the reference: a callable with
VLNBert's surface over RefVLNBert's parameters, restated functionally so that the K/V cache exists on its side too and one defect can be planted.

Planted defects (`DEFECTS`): Ref64(defect=n) returns the reference with one navigator-specific error; which compared quantity catches each is
listed there and asserted in both test files."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from oracle.model_ref import _ffn, key_bias
from oracle.nav_ref import RefVLNBert, nav_fuse
from tests._layer_ref64 import rel_cos

HD = 64
FUNCS = ("txt_embeds", "txt_attns", "pano_embeds", "pano_fused_embeds", "img_attns", "gmap_embeds", "vp_embeds", "gmap_attns", "vp_attns",
         "cls_embeds", "global_logits", "local_logits")
NAV_KEYS = ("gmap_embeds", "vp_embeds", "gmap_attns", "vp_attns", "cls_embeds", "global_logits", "local_logits", "fused_logits")
LOGITS = ("global_logits", "local_logits", "fused_logits")
# parameters the kernels read as fp32 masters (module docstring); every other weight matrix / table is read from the 16-bit shadow
FP32_READ = ("loc_linear.weight", "pos_embeddings.0.weight", "pano_fuse_linear.weight", "net.3.weight", "sprel_linear.weight",
             "gate_x.weight", "gate_e.weight", "state2value.3.weight")
TABLES = ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight", "nav_type_embedding.weight",
          "gmap_step_embeddings.weight")

# n -> (what is wrong, the compared quantities expected to catch it (any of them), the case kind it belongs to)
DEFECTS = {
    1: ("masked `mem` column of gmap_masks attended to", ("fwd gmap_embeds", "grad w"), "step"),
    2: ("pair-distance bias left out of the global encoder", ("fwd gmap_embeds", "grad sprel"), "step"),
    3: ("cls_embeds taken from the global branch only", ("fwd cls_embeds",), "step"),
    4: ("d cls_embeds not added into d vp", ("din vp_img", "grad w"), "step"),
    5: ("attention-map seed not divided over the heads", ("grad w", "din gmap_img"), "step"),
    6: ("global and local halves of the text K/V gradient swapped", ("dkv",), "cached"),
    7: ("second step's K/V gradient overwrites the first", ("dkv",), "cached"),
    8: ("fusion gate's global half (the `tmp` residual) dropped", ("logit",), "step"),
    9: ("`door` gate without its w_e . e term", ("grad gate", "din vp_img"), "causal"),
    10: ("`type_1` prior P(z) not applied", ("fwd pano_embeds", "fwd txt_embeds"), "causal"),
    11: ("critic's row-dot without its bias", ("value",), "critic"),
}


def is_shadow(name, p):
    """True where the engine's kernels read the parameter from the 16-bit shadow"""
    return p.dim() == 2 and name.endswith("weight") and not name.endswith(FP32_READ)


def grad_class(name):
    """class of a parameter's gradient: "tab" embedding tables, "sprel", "b" the row-sum (cancellation) class of DESIGN section 0 -- biases,
    LayerNorm betas, the position / location projections -- and "w" every other weight / gamma"""
    if name.endswith(TABLES):
        return "tab"
    if ".gate_x." in name or ".gate_e." in name:
        # the `door` gate's four parameters: d w = sum over rows of (d out . e) sigma' [x | e].  On a row whose input is all zero -- the [stop] /
        # [mem] / padding rows of the map and viewpoint inputs, as the agent builds them -- the block's LayerNorm sees e alone, its input gradient
        # is orthogonal to e, and (d out . e) is an analytic zero carried as rounding noise times that row's large rstd: a cancellation class of
        # its own, ~170x the storage epsilon in fp32 and fp16 storage alike
        return "gate"
    if name.endswith("sprel_linear.weight"):
        return "sprel"
    if name.endswith("bias") or "pos_embeddings.0.weight" in name or name.endswith("loc_linear.weight"):
        return "b"
    return "w"


def analytically_zero(name):
    """a key bias shifts every logit of a softmax row alike, so do the distance bias's bias and the panorama fusion's: zero gradient, rounding
    noise on both sides"""
    return name.endswith(("self.key.bias", "sprel_linear.bias", "pano_fuse_linear.bias")) or (".causal." in name and name.endswith(".key.bias"))


# ---- model pairs ---------------------------------------------------------------------------------------------------------------------------
def randomise(o, seed):
    """biases and LayerNorm gains as tests/test_nav_h768_oracle_gpu._pair sets them; then every value made fp32-representable (the engine's masters)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in o.named_parameters():
            if n.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.02)
            if "LayerNorm.weight" in n or "layer_norm.weight" in n or n.endswith(("net.2.weight", "pos_embeddings.1.weight")):
                p.add_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.05)
            p.copy_(p.float().double())
    return o


def round_params(o, dt):
    """in place: every parameter of the shadow group rounded to dt (None / fp32: nothing to do, the masters are what the kernels read)"""
    if dt in (None, torch.float32):
        return o
    with torch.no_grad():
        for n, p in o.named_parameters():
            if is_shadow(n, p):
                p.copy_(p.float().to(dt).double())
    return o


def oracle(cfg, seed=0):
    torch.manual_seed(seed)
    return randomise(RefVLNBert(cfg).double().eval(), seed + 1)


def pair(cfg, dt, seed=0, device="cuda"):
    """(fp64 RefVLNBert holding what the kernels read, VLNBert(compute_dtype=dt)) with the same weights"""
    from magic_amd.host.model_nav import VLNBert
    o = oracle(cfg, seed)
    g = VLNBert(None, role="student", config=cfg, device=device, compute_dtype=dt)
    g.load_state_dict(o.state_dict(), strict=True)
    g.eval()
    return round_params(o, dt), g


def rnd(t, dt):
    """an input tensor as the engine's 16-bit cast leaves it, in fp64"""
    return t.double() if dt in (None, torch.float32) else t.float().to(dt).double()


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
def _attn(att, x, ctx, bias, kv=None):
    """oracle.model_ref.RefAttention.forward with the key | value rows optionally given (the navigator's per-episode cache)"""
    B, Nq, H = x.shape
    nh = att.nh
    d = H // nh
    q = att.self.query(x).view(B, Nq, nh, d).transpose(1, 2)
    k, v = (att.self.key(ctx), att.self.value(ctx)) if kv is None else (kv[..., :H], kv[..., H:])
    Nk = k.shape[1]
    k, v = k.reshape(B, Nk, nh, d).transpose(1, 2), v.reshape(B, Nk, nh, d).transpose(1, 2)
    p = torch.softmax(q @ k.transpose(-1, -2) / d ** 0.5 + bias, dim=-1)
    c = (p @ v).transpose(1, 2).reshape(B, Nq, H)
    return att.output.LayerNorm(x + att.output.dense(c)), p


def _cross_stack(layers, x, sb, ctx, cb, kvs=None):
    p = None
    for i, lyr in enumerate(layers):
        s, _ = _attn(lyr.attention, x, x, sb)
        c, p = _attn(lyr.crossattention, s, ctx, cb, None if kvs is None else kvs[i])
        x = _ffn(lyr, c)
    return x, p


def _cls(head, x, gate=None, pre=None):
    """oracle.model_ref.ClsPrediction (Linear, ReLU, LayerNorm, Linear(H, 1)); gate: the ReLU's 0 / 1 pattern is GIVEN (the engine's own, read
    from its stored activation) instead of taken from this side's pre-activation -- see Ref64; pre: list that receives the pre-activation"""
    net = head.net
    y = net[0](x)
    if pre is not None:
        pre.append(y.detach())
    return net[3](net[2](torch.relu(y) if gate is None else y * gate))


class _SwapHalves(torch.autograd.Function):
    """identity whose backward hands the first half of dim 0 the gradient of the second and the other way round (defect 6)"""

    @staticmethod
    def forward(ctx, kv):
        return kv.clone()

    @staticmethod
    def backward(ctx, d):
        n = d.shape[0] // 2
        return torch.cat([d[n:], d[:n]], 0)


def _causal(blk, x, z, pz, dt, defect):
    """oracle.causal_ref.RefCausalBlock.forward restated: dictionary and prior as the engine's casts leave them; defects 9 and 10"""
    B, N, H = x.shape
    z0 = rnd(z[0] if z.dim() == 3 else z, dt)
    k, v = blk.key(z0), blk.value(z0)
    type_1 = blk.kind == "back" and blk.btype == "type_1"
    if pz is not None and not (defect == 10 and type_1):
        v = v * rnd(pz[0] if pz.dim() == 3 else pz, dt).reshape(-1, 1)
    if type_1:
        e = v.sum(0).expand(B, N, H)
    else:
        q = blk.query(x)
        heads = []
        for h in range(blk.nh):
            sl = slice(h * HD, (h + 1) * HD)
            heads.append(torch.softmax(q[..., sl] @ k[:, sl].t() / HD ** 0.5, -1) @ v[:, sl])
        e = torch.cat(heads, -1)
    e = blk.output.dense(e)
    if blk.door:
        e = torch.sigmoid(blk.gate_x(x) + (blk.gate_e.bias if defect == 9 else blk.gate_e(e))) * e
    return blk.output.LayerNorm(x + e)


class Ref64:
    """the reference: `ref(mode, inputs)` / `ref.text_kv(txt)` like VLNBert, in fp64 over RefVLNBert `o`'s parameters.  dt: the engine's storage
    type (inputs it casts are rounded to it; None: nothing is rounded).  defect: one of DEFECTS, or None.

    gates: per navigation call {"g", "l", "f": bool tensors} -- the ReLU patterns of the three ClsPrediction heads as the ENGINE took them.  A ReLU
    is the one discontinuous stage of the step: an element whose pre-activation lies within the engine's rounding error of 0 can take the other
    branch there, and each such element changes a head's weight gradient by a whole term, not by a rounding -- an error that shrinks with the
    square root of the storage epsilon and hides the 1 / 8 between fp16 and bf16.  Like the dropout masks in tests/_layer_ref64.py the pattern is
    therefore replayed, and `gate_report` bounds how far from 0 a differing element's pre-activation was.  None: this side's own ReLU."""

    def __init__(self, o, dt=None, defect=None, gates=None):
        self.o, self.m, self.cfg, self.dt, self.defect, self.gates = o, o.vln_bert, o.cfg, dt, defect, gates
        self.kv_calls, self.nav_calls, self.pre = 0, 0, []

    def text_kv(self, txt):
        m, kv = self.m, []
        for enc in (m.global_encoder, m.local_encoder):
            for lyr in enc.encoder.crossattention:
                a = lyr.crossattention.self
                kv.append(torch.cat([a.key(txt), a.value(txt)], -1))
        return torch.stack(kv)                     # [2 nl, B, L, 2H]

    def __call__(self, mode, b):
        m, dt, defect = self.m, self.dt, self.defect
        cz = getattr(m, "causal", {})
        if mode == "language":
            x, p = m.text(b["txt_ids"], b["txt_masks"])
            if "back_txt" in cz and b.get("instr_z_direction_features") is not None:
                z = torch.cat([b["instr_z_direction_features"], b["instr_z_landmark_features"]], 1)
                pz = torch.cat([b["instr_z_direction_pzs"], b["instr_z_landmark_pzs"]], 1)
                x = _causal(cz["back_txt"], x, z, pz, dt, defect)
            if "front_txt" in cz and b.get("front_txt_feats") is not None:
                x = _causal(cz["front_txt"], x, b["front_txt_feats"], None, dt, defect)
            return x, p
        if mode == "panorama":
            x, masks, fused, p = m.panorama(rnd(b["view_img_fts"], dt), b["loc_fts"].double(), b["nav_types"], b["view_lens"])
            if "back_img" in cz and b.get("z_img_features") is not None:
                x = _causal(cz["back_img"], x, b["z_img_features"], b["z_img_pzs"], dt, defect)
            return x, masks, fused, p
        if mode != "navigation":
            raise NotImplementedError(mode)
        gimg, vimg, txt = b["gmap_img_embeds"], b["vp_img_embeds"], b["txt_embeds"]
        if "front_gmap" in cz and b.get("front_gmap_feats") is not None:
            gimg = _causal(cz["front_gmap"], gimg, b["front_gmap_feats"], None, dt, defect)
        if "front_vp" in cz and b.get("front_vp_feats") is not None:
            vimg = _causal(cz["front_vp"], vimg, b["front_vp_feats"], None, dt, defect)
        nl = self.cfg.num_x_layers
        kv = b.get("txt_kv")
        if kv is not None:
            if defect == 6:
                kv = _SwapHalves.apply(kv)
            if defect == 7 and self.kv_calls == 0:
                kv = kv.detach()
            self.kv_calls += 1
        ge, le = m.global_encoder, m.local_encoder
        gin = m.global_input(gimg, b["gmap_step_ids"], b["gmap_pos_fts"].double())
        gmask = b["gmap_masks"]
        if defect == 1:
            gmask = gmask.clone()
            gmask[:, 1] = True
        sb = key_bias(gmask)
        if self.cfg.graph_sprels and defect != 2:
            sb = sb + ge.sprel_linear(b["gmap_pair_dists"].double().unsqueeze(3)).squeeze(3).unsqueeze(1)
        cb = key_bias(b["txt_masks"])
        g, ga = _cross_stack(ge.encoder.crossattention, gin, sb, txt, cb, None if kv is None else kv[:nl])
        vin = m.local_input(vimg, b["vp_pos_fts"].double())
        v, va = _cross_stack(le.encoder.crossattention, vin, key_bias(b["vp_masks"]), txt, cb, None if kv is None else kv[nl:])
        g0, v0 = g[:, 0], v[:, 0]
        gt = self.gates[self.nav_calls] if self.gates is not None else {}
        self.nav_calls += 1
        pg, pl, pf = [], [], []
        self.pre.append(dict(g=pg, l=pl, f=pf))
        fw = torch.sigmoid(_cls(m.sap_fuse_linear, torch.cat([g0 * 0 if defect == 8 else g0, v0], 1), gt.get("f"), pf)) if self.cfg.glocal_fuse else 0.5
        gl = (_cls(m.global_sap_head, g, gt.get("g"), pg).squeeze(2) * fw).masked_fill(b["gmap_visited_masks"], -float("inf"))
        gl = gl.masked_fill(~b["gmap_masks"], -float("inf"))
        ll = (_cls(m.local_sap_head, v, gt.get("l"), pl).squeeze(2) * (1 - fw)).masked_fill(~b["vp_nav_masks"], -float("inf"))
        cls = g0 if defect == 3 else g0 + (v0.detach() if defect == 4 else v0)
        return dict(gmap_embeds=g, vp_embeds=v, gmap_attns=ga, vp_attns=va, cls_embeds=cls, global_logits=gl, local_logits=ll,
                    fused_logits=nav_fuse(gl, ll, b))


class Tap:
    """stands in for either model in one_step / step: keeps what the comparison needs (module docstring)"""

    def __init__(self, model, use_kv=False):
        self.model, self.use_kv = model, use_kv
        self.txt = self.txt_attn = self.kv = None
        self.gimg, self.vimg, self.navs = [], [], []

    def __call__(self, mode, b):
        if mode == "language":
            if self.txt is None:
                self.txt, self.txt_attn = self.model(mode, b)
                self.txt.retain_grad()
                if self.use_kv:
                    self.kv = self.model.text_kv(self.txt)
                    self.kv.retain_grad()
            return self.txt, self.txt_attn
        if mode == "navigation":
            for k, keep in (("gmap_img_embeds", self.gimg), ("vp_img_embeds", self.vimg)):
                if b[k].requires_grad:
                    b[k].retain_grad()
                keep.append(b[k])
            if self.kv is not None:
                b = dict(b, txt_kv=self.kv)
            out = self.model(mode, b)
            self.navs.append(out)
            return out
        return self.model(mode, b)


# ---- loss ------------------------------------------------------------------------------------------------------------------------------------
def valid_masks(inp):
    """per output of FUNCS: bool mask (broadcastable to the output) of the entries that are compared and carry a functional"""
    tm, gm = inp["txt_masks"], inp["gmap_masks"]
    B, L = tm.shape
    K, V = gm.shape[1], inp["view_img_fts"].shape[1]
    one = lambda *s: torch.ones(*s, dtype=torch.bool)             # noqa: E731
    return dict(txt_embeds=tm[:, :, None], txt_attns=(tm[:, None, :, None] & tm[:, None, None, :]), pano_embeds=one(B, V, 1),
                pano_fused_embeds=one(B, 1), img_attns=one(B, V, V), gmap_embeds=gm[:, :, None],
                gmap_attns=(gm[:, None, :, None] & tm[:, None, None, :]), vp_embeds=one(B, V + 2, 1),
                vp_attns=(one(B, 1, V + 2, 1) & tm[:, None, None, :]), cls_embeds=one(B, 1),
                global_logits=(~inp["gmap_visited_masks"]) & gm, local_logits=inp["vp_nav_masks"])


def flat_outputs(out):
    """one_step's `out` -> {name: tensor} over FUNCS + fused_logits"""
    d = {k: out[k] for k in ("txt_embeds", "txt_attns", "pano_embeds", "pano_fused_embeds", "img_attns")}
    d.update({k: out["nav_outs"][k] for k in NAV_KEYS})
    return d


def functionals(shapes, masks, call=0):
    """{name: fp64 R} -- fixed random directions, zero outside the valid entries, norm 0.5"""
    R = {}
    for i, name in enumerate(FUNCS):
        if name not in shapes:                 # (tests/test_causal_gpu.step returns the adjusted embeddings and the navigation outputs only)
            continue
        g = torch.Generator().manual_seed(7919 * (i + 1) + 104729 * call)
        r = torch.randn(shapes[name], generator=g, dtype=torch.float64) * masks[name]
        R[name] = 0.5 * r / r.norm()
    return R


def loss_of(outs, inp, R, defect=None, names=FUNCS):
    """CE on fused_logits (mean over the batch, ignore_index -100, as one_step) + sum_k <R_k, out_k>; evaluated in fp64 on the outputs' device"""
    fl = outs["fused_logits"]
    dev = fl.device
    nh = outs["txt_attns"].shape[1] if "txt_attns" in outs else 1
    loss = F.cross_entropy(fl.double(), inp["targets"].to(dev), reduction="sum", ignore_index=-100) / fl.shape[0]
    for name in names:
        if name not in outs:
            continue
        x = outs[name].double()
        if defect == 5 and name == "img_attns":            # head_mean backward without its 1 / heads: same value, `heads` times the gradient
            x = nh * x - (nh - 1) * x.detach()
        r = R[name].to(dev)
        loss = loss + (torch.where(r != 0, x, torch.zeros_like(x)) * r).sum()
    return loss


# ---- running a case on either side -------------------------------------------------------------------------------------------------------------
def run(model, inps, driver, dz=None, use_kv=False, scale=1.0, defect=None, device="cpu", f64=False):
    """drive `model` (VLNBert or Ref64) through `driver` (one_step / step) once per entry of `inps` (one episode: the text of inps[0]), add the
    losses up, one backward (loss * scale).  Returns a namespace: outs (per call: {name: tensor}), loss, tap, masks (per call)."""
    from tests.test_nav_gpu import to_dev
    tap = Tap(model, use_kv=use_kv)
    outs, masks, total = [], [], 0.0
    for call, inp in enumerate(inps):
        idev = to_dev(inp, device, f64=f64)
        if dz is None:
            o = flat_outputs(driver(tap, idev)["out"])
        else:
            r = driver(tap, idev, to_dev(dz, device, f64=f64))
            o = dict(txt_embeds=r["txt"], pano_embeds=r["pano"], **{k: r["nav"][k] for k in NAV_KEYS})
        mk = valid_masks(inp)
        R = functionals({k: tuple(v.shape) for k, v in o.items() if k in FUNCS}, mk, call)
        names = [k for k in FUNCS if k in o and not (call > 0 and k in ("txt_embeds", "txt_attns"))]    # the text is the episode's: once
        total = total + loss_of(o, inp, R, defect, names)
        outs.append(o)
        masks.append(mk)
    (total * scale).backward()
    return SimpleNamespace(outs=outs, loss=total.detach(), tap=tap, masks=masks)


def ref_grads(o):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in o.named_parameters()}


def reference(o, inps, driver, dt=None, dz=None, use_kv=False, defect=None, gates=None):
    """the fp64 side of a case: namespace with outs (detached), grads {name: tensor or None}, din {gmap_img, vp_img, txt: per call / tensor}, dkv,
    pre (per navigation call: the three heads' pre-activations)"""
    for p in o.parameters():
        p.grad = None
    ref = Ref64(o, dt, defect, gates)
    r = run(ref, inps, driver, dz=dz, use_kv=use_kv, defect=defect, device="cpu", f64=True)
    t = r.tap
    g = lambda x: None if x is None or x.grad is None else x.grad.detach().clone()           # noqa: E731
    return SimpleNamespace(outs=[{k: v.detach() for k, v in o_.items()} for o_ in r.outs], masks=r.masks, loss=r.loss, grads=ref_grads(o),
                           din=dict(gmap_img=[g(x) for x in t.gimg], vp_img=[g(x) for x in t.vimg], txt=g(t.txt)), dkv=g(t.kv),
                           pre=[{k: (v[0] if v else None) for k, v in d.items()} for d in ref.pre])


def gate_report(gates, pre):
    """(number of elements where the engine's ReLU pattern differs from this side's own, the largest |pre-activation| among them in units of its
    row's rms): a differing element must sit within rounding error of 0"""
    n, worst = 0, 0.0
    for gt, pr in zip(gates, pre):
        for k, p in pr.items():
            if p is None or gt.get(k) is None:
                continue
            diff = gt[k].view_as(p) != (p > 0)
            if diff.any():
                n += int(diff.sum())
                worst = max(worst, (p.abs() / p.pow(2).mean(-1, keepdim=True).sqrt())[diff].max().item())
    return n, worst


# ---- comparison --------------------------------------------------------------------------------------------------------------------------------
def per_sample_rel(a, b, mask=None):
    """worst rel-L2 over the samples (dim 0) of a against the reference b, over the masked entries"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if mask is not None:
        m = mask.expand_as(b)
        a, b = torch.where(m, a, torch.zeros_like(a)), torch.where(m, b, torch.zeros_like(b))
    worst = 0.0
    for s in range(b.shape[0]):
        n = b[s].norm().item()
        if n > 0:
            worst = max(worst, (a[s] - b[s]).norm().item() / n)
    return worst


def compare(got, want, errs=None):
    """every compared quantity of one case: {quantity: error} (rel-L2 unless named otherwise) -- "fwd <name>" per forward output, "logit" max-abs
    over finite entries, "grad w" / "grad b" / "grad tab" / "grad sprel" worst over the class's tensors (+ "cos <class>": 1 - worst cosine),
    "din gmap_img" / "din vp_img" / "din txt", "dkv".  got / want: namespaces with outs, grads, din, dkv (want's masks are used)."""
    e = {} if errs is None else errs
    up = lambda k, v: e.__setitem__(k, max(e.get(k, 0.0), float(v)))           # noqa: E731
    for call, (go, wo) in enumerate(zip(got.outs, want.outs)):
        for name, w in wo.items():
            gk = go[name].detach().double().cpu()
            if name in LOGITS:
                fin = torch.isfinite(w)
                up("logit", (torch.where(fin, gk - w, torch.zeros_like(w))).abs().max())
            else:
                up("fwd " + name, per_sample_rel(gk, w, want.masks[call][name]))
    for name, w in want.grads.items():
        if analytically_zero(name) or name not in got.grads:
            continue
        k, c = got.grads[name], grad_class(name)
        if w is None:                   # a gradient where the reference has none: an error of the whole tensor
            if k is not None and k.abs().max() > 0:
                up("grad " + c, 1.0)
            continue
        k = torch.zeros_like(w) if k is None else k.detach().double().cpu()
        if c == "tab":
            rows = w.abs().amax(1) > 0
            k, w = k[rows], w[rows]
        if w.norm() == 0:
            continue
        rel, cos = rel_cos(k, w)
        up("grad " + c, rel)
        up("cos " + c, 1.0 - cos)
        e.setdefault("worst", {})
        if rel >= e["worst"].get(c, ("", -1.0))[1]:
            e["worst"][c] = (name, rel)
    for key in ("gmap_img", "vp_img"):
        for gk, w in zip(got.din[key], want.din[key]):
            if w is not None:
                up("din " + key, per_sample_rel(gk, w))
    if want.din["txt"] is not None and got.din["txt"] is not None:
        up("din txt", per_sample_rel(got.din["txt"], want.din["txt"]))
    if want.dkv is not None and got.dkv is not None:
        w = want.dkv                                             # [2 nl, B, L, 2H]: per sample and layer
        k = got.dkv.detach().double().cpu().view_as(w)
        for i in range(w.shape[0]):
            up("dkv", per_sample_rel(k[i], w[i]))
    return e


def top2_gap(logits):
    """per row: the gap between the two largest finite entries (inf where fewer than two are finite)"""
    v = torch.sort(torch.nan_to_num(logits.double(), neginf=-1e300), 1, descending=True).values
    gap = v[:, 0] - v[:, 1]
    return torch.where(v[:, 1] < -1e299, torch.full_like(gap, float("inf")), gap)


# ---- Critic -------------------------------------------------------------------------------------------------------------------------------------
def critic_reference(sd, x, dt, defect=None):
    """value head Linear(H, 512) -> ReLU -> Linear(512, 1) in fp64: state2value.0.weight rounded to dt, everything else fp32; x rounded to dt.
    Returns (value [B], d x, {name: gradient}) of value.sum() + <r, value> (r fixed)."""
    p = {k: v.detach().float().double().clone().requires_grad_(True) for k, v in sd.items()}
    with torch.no_grad():
        p["state2value.0.weight"].copy_(rnd(p["state2value.0.weight"], dt))
    xr = rnd(x, dt).requires_grad_(True)
    v = (torch.relu(xr @ p["state2value.0.weight"].t() + p["state2value.0.bias"]) @ p["state2value.3.weight"].t()).squeeze(-1)
    if defect != 11:
        v = v + p["state2value.3.bias"]
    critic_loss(v).backward()
    return v.detach(), xr.grad, {k: t.grad for k, t in p.items()}


def critic_loss(v):
    r = torch.randn(v.shape[0], generator=torch.Generator().manual_seed(5), dtype=torch.float64).to(v.device)
    return (v.double() * (1.0 + r)).sum()


def qclass(q):
    """bound class of a compared quantity: "emb" embeddings, "attn" attention maps, "logit", "value", "w" / "b" / "tab" / "sprel" parameter
    gradients, "din" mode-input gradients, "dkv" the K/V cache's gradient"""
    kind, _, name = q.partition(" ")
    if kind == "fwd":
        return "attn" if name.endswith("attns") else "emb"
    return {"grad": name, "din": "din"}.get(kind, q)
