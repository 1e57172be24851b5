"""The proxy-task heads of the pretraining step, one unit per task (`mlm`, `mrc`, `sap`, `cfp`).  A unit owns everything of the step that is
task-specific, top to bottom: which cross-modal encoder(s) run and on what (`cross`), the head's launches (`head`), the rows it takes from the
step's zero arena (`rows`), the supervised loss and its gradient seeds (`loss`), what the distillation terms read of it (`kd_streams`,
`kd_sample_w`, `kd_predict`), phase 1 of the backward down to the node inputs (`backward`), the validation rows (`metrics`) and the
`compute_loss=False` return contract (`result`).  host/model_pretrain.py drives them: shared trunk, one arena, the unit, loss assembly.

Every method takes the model `m` and the step's context `c`; the switches of host/model_pretrain.py and host/ops.py are read when a method
runs, where tests and the benchmark set them.  ClsPrediction (Linear, ReLU, LayerNorm, Linear(H, 1)) and the gate-fuse backward are plain
functions: the navigator (host/model_nav.py) calls the same ones."""
import contextlib

import torch

from . import lib as _lib
from . import makd_pretrain as KD
from . import model_pretrain as MP
from . import ops as O
from .config import cfg_get
from .engine import rup


# ---- ClsPrediction ------------------------------------------------------------------------------------------
def cls_fwd(n, prefix, X, M, lda=None):
    """ClsPrediction forward: returns (Y=relu(linear), logit)"""
    l1 = n.lin(prefix + "net.0.weight")
    Y = O.linear_fwd(X, l1.W, l1.b, M, epilogue=2, lda=lda)
    return Y, cls_tail(n, prefix, Y, M)


def cls_tail(n, prefix, Y, M):
    """ClsPrediction after its first projection: LayerNorm + Linear(H, 1)"""
    ln, l2 = n.ln(prefix + "net.2"), n.lin(prefix + "net.3.weight")
    logit = n.new(M, dtype=torch.float32)
    O.lndot_fwd(Y, M, n.H, ln.g, ln.b, n.eps, l2.Wm, l2.b, logit)
    return logit


def cls_bwd(n, prefix, X, Y, dlogit, M, d_acc, lda=None):
    H = n.H
    l1, ln, l2 = n.lin(prefix + "net.0.weight"), n.ln(prefix + "net.2"), n.lin(prefix + "net.3.weight")
    dZ = n.new(M, H)
    O.lndot_bwd(Y, M, H, ln.g, ln.b, n.eps, l2.Wm, dlogit, dZ, ln.dg, ln.db, l2.dW, l2.db)
    O.linear_dw(dZ, X, l1.dW, l1.db, M, ldb=lda)
    O.linear_dx(dZ, l1.W, M, out=d_acc, residual=d_acc, ldc=lda)


def gate_fuse_bwd(n, prefix, c, df, B, K, Vp, d_gmap, d_vp, grouped):
    """backward of sap_fuse_linear on [map [stop] row | viewpoint [stop] row]; grouped: the two input-gradient GEMMs as one launch
    (the pretraining step) or one by one (the navigator)"""
    H = n.H
    f1, fln, f2 = n.lin(prefix + "sap_fuse_linear.net.0.weight"), n.ln(prefix + "sap_fuse_linear.net.2"), n.lin(prefix + "sap_fuse_linear.net.3.weight")
    dZ = n.new(B, H)
    O.lndot_bwd(c.Yf, B, H, fln.g, fln.b, n.eps, f2.Wm, df, dZ, fln.dg, fln.db, f2.dW, f2.db)
    # dW[:, :H] += dZ^T g0 ; dW[:, H:] += dZ^T v0 (bias grad once)
    O.linear_dw(dZ, c.glob.out, f1.dW, f1.db, B, N=H, K=H, ldb=K * H, ldc=2 * H)
    O.linear_dw(dZ, c.loc.out, f1.dW[:, H:], None, B, N=H, K=H, ldb=Vp * H, ldc=2 * H)
    with _lib.group() if grouped else contextlib.nullcontext():
        O.linear_dx(dZ, f1.W, B, out=d_gmap, residual=d_gmap, ldb=2 * H, ldc=K * H, N=H, K=H)
        O.linear_dx(dZ, f1.W[:, H:], B, out=d_vp, residual=d_vp, ldb=2 * H, ldc=Vp * H, N=H, K=H)


def _relu(x):
    # in-place ReLU on a tiny [B,H] head tensor via the activation-derivative kernel: x * relu'(x) == relu(x)
    return O.dact(x, x, 2, out=x)


def _sizes(m, c):
    p = c.plan
    return m.net, p, p["B"], p["L"], p["K"], p["Vp"], m.net.H


class Head:
    gpos = vpos = True          # which node inputs (map tokens, viewpoint tokens) the task's cross-modal stage reads

    def dx_rows(self, plan):
        """rows of the fp32 vocabulary input-gradient accumulator that shares the loss slots' allocation (mlm)"""
        return 0

    def kd_sample_w(self, m, c, t, kdl):
        """hard-mining sample weights from the teacher's action logits (sap)"""
        return None

    def kd_predict(self, m, c, t, T, w, coef):
        """rows of the action-distillation term (sap)"""
        return None


# ---- mlm: the text attends to the map; transform + vocabulary projection on the masked rows ----------------------------
class Mlm(Head):
    vpos = False

    def cross(self, m, c, o):
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        l2v_args = ("global", plan, c.txt_out, L, plan["txt_mask"], plan["lens"]["txt"], plan["txt_tokens"],
                    c.gin.out, K, plan["gmap_mask"], plan["lens"]["gmap"], plan["gmap_nodes"])
        c.l2v = n.cross_fwd_fused([l2v_args])[0] if n.xenc_ok(L, K) else n.cross_fwd(*l2v_args, dist=None)
        o["gmap_embeds"], o["gmap_attns"] = c.l2v.out, c.l2v.P

    def head(self, m, c, o, compute_loss, metrics):
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        nm = plan["n_mask"]
        c.hm_in = n.new(nm, H)
        O.csr_gather(c.l2v.out, *plan["mlm_rows"], c.hm_in, nm, H)
        t = n.lin("mlm_head.predictions.transform.dense.weight")
        c.tz = n.new(nm, H)
        tn = n.ln("mlm_head.predictions.transform.LayerNorm")
        c.hm, c.rstd_hm = n.new(nm, H), n.new(nm, dtype=torch.float32)
        if MP.MLM_TAIL_FUSED and O.linear_ln_ok(H, H):      # dense -> gelu -> LayerNorm as one launch
            O.linear_act_ln(c.hm_in, t.W, t.b, nm, 1, c.tz, tn.g, tn.b, n.eps, c.hm, c.rstd_hm)
        else:
            c.tg = O.linear_fwd(c.hm_in, t.W, t.b, nm, epilogue=1, pre=c.tz)
            O.ln_fwd(nm, H, c.hm, in0=c.tg, gamma=tn.g, beta=tn.b, eps=n.eps, rstd=c.rstd_hm)
        Vv = m.config.vocab_size
        c.ldv = rup(Vv, 8)
        if metrics is not None and O.mlm_eval_ok(c.hm.dtype, H):
            c.logits = None              # the validation rows come out of the projection itself (O.mlm_eval): no logits buffer
        else:
            c.logits = n.new(nm, c.ldv)
            if c.ldv > Vv:
                c.logits[:, Vv:].zero_()
            O.linear_fwd(c.hm, m.store.w("bert.embeddings.word_embeddings.weight"), m.store.master("mlm_head.predictions.bias"),
                         nm, out=c.logits, ldc=c.ldv)
            o["predict"] = c.logits[:, :Vv]

    def rows(self, plan):
        return [plan["B"] * plan["L"], plan["B"] * plan["K"]]

    def dx_rows(self, plan):
        return plan["n_mask"]

    def loss(self, m, c, o, zz, scg, kd):
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        train = m.store.requires_grad
        c.d_x, c.d_gin0 = zz(B * L, H), zz(B * K, H)
        nm = plan["n_mask"]
        c.rows = n.new(nm, dtype=torch.float32)
        c.dlogits = (n.new(nm, c.ldv) if m.keep_mlm_logits else c.logits) if train else None
        roww = plan.get("mlm_row_w")      # shape buckets: nm counts padded (ignored) rows too, the true 1 / n_mask rides in per-row weights
        O.ce_rows(c.logits, nm, m.config.vocab_size, c.ldv, plan["mlm_labels"], ignore_index=-1, coef=scg if roww is not None else scg / nm,
                  row_w=roww, loss_row=c.rows, dlogits=c.dlogits, ldd=c.ldv)
        if train and not m.keep_mlm_logits:
            o["predict"] = None          # overwritten in place by its gradient
        return c.rows, roww, (1.0 if roww is not None else 1.0 / nm)

    def kd_streams(self, c):
        """ability -> (student embeddings, attention maps, Nq, Nk, ldp, embedding accumulator, names of the true sizes of Nq / Nk for plan["dyn"];
        None: not padded)"""
        p = c.plan
        return {"global": (c.l2v.out, c.l2v.P, p["L"], p["K"], c.l2v.ldp, c.d_x, "L", "K")}

    def backward(self, m, c):
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        nm, Vv = plan["n_mask"], m.config.vocab_size
        dlog = c.dlogits                     # CE wrote the gradient (in place unless keep_mlm_logits)
        Wemb = m.store.w("bert.embeddings.word_embeddings.weight")
        O.linear_dw(dlog, c.hm, m.store.g("bert.embeddings.word_embeddings.weight"), m.store.g("mlm_head.predictions.bias"),
                    nm, N=Vv, K=H, lda=c.ldv)
        # dx over the 50k-wide vocabulary: split-K into an fp32 accumulator (18 output tiles alone cannot fill 256 CUs)
        d_hm32 = c.d_hm32
        if c.dx_slabs:
            O.gemm(1, dlog, Wemb, d_hm32, nm, H, Vv, c.ldv, H, H, splitk=-c.dx_slabs)
        else:
            O.gemm(1, dlog, Wemb, d_hm32, nm, H, Vv, c.ldv, H, H, splitk=MP.MLM_DX_SPLITK, accumulate=True)
        tn = n.ln("mlm_head.predictions.transform.LayerNorm")
        if MP.MLM_TAIL_FUSED:        # cast + LayerNorm backward + gelu' as one launch (the fp32 accumulator -- or its slabs -- read as it is)
            d_tz = O.ln_bwd_tail(nm, H, d_hm32, c.hm, tn.g, tn.b, c.rstd_hm, c.tz, 1, n.new(nm, H), tn.dg, tn.db, nslab=max(1, c.dx_slabs))
        else:
            d_hm = O.cast_to(d_hm32, m.compute_dtype)
            d_tg = n.new(nm, H)
            O.ln_bwd(nm, H, d_hm, y=c.hm, gamma=tn.g, beta=tn.b, rstd=c.rstd_hm, dx=d_tg, dgamma=tn.dg, dbeta=tn.db)
            d_tz = O.dact(d_tg, c.tz, 1)
        t = n.lin("mlm_head.predictions.transform.dense.weight")
        O.linear_dw(d_tz, c.hm_in, t.dW, t.db, nm)
        d_hin = O.linear_dx(d_tz, t.W, nm)
        O.csr_gather(d_hin, *plan["mlm_rows_T"], c.d_x, B * L, H, accumulate=True)
        d_gin = c.d_gin0
        d_t2 = n.cross_bwd(c.l2v, c.d_x, d_gin, c.dP_g)
        if not getattr(c, "islands", None) and n.nodes_pano_ok(plan, gin=c.gin):     # the text fold, the map inputs' backward and the panorama fusion's backward: one launch
            # (with causal adjustment islands d_pano is still the gradient of the ADJUSTED embeddings here: phase 2 takes it through the island first, the fusion backward after)
            n.nodes_pano_bwd(plan, c.pano, c.gin, d_gin, None, None, c.d_pano, c.d_fused, add=(c.d_txt, [d_t2]))
            c.pano_head_done = True
        else:
            O.add_(c.d_txt, d_t2)
            n.gmap_in_bwd(c.gin, plan, d_gin, c.d_pano, c.d_fused)

    def metrics(self, m, c, block, temperature):
        nm, Vv = c.plan["n_mask"], m.config.vocab_size
        if c.logits is None:
            rows = O.mlm_eval(c.hm, m.store.w("bert.embeddings.word_embeddings.weight"), m.store.master("mlm_head.predictions.bias"),
                              c.plan["mlm_labels"], Vv, ignore_index=-1)
        else:
            rows = O.eval_rows(c.logits, nm, Vv, c.ldv, labels=c.plan["mlm_labels"], ignore_index=-1)
        O.eval_accum(*rows, nm, block, 0)

    def result(self, m, c, o, batch):
        return {"predict": o["predict"]}


# ---- mrc: local branch only; RegionClassification on the masked views of the current viewpoint (validate_mrc :476-500) ----
class Mrc(Head):
    gpos = False

    def cross(self, m, c, o):
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        loc_args = ("local", plan, c.vin.out, Vp, plan["vp_mask"], [Vp] * B, B * Vp, c.txt_out, L, plan["txt_mask"], plan["lens"]["txt"], plan["txt_tokens"])
        c.loc = n.cross_fwd_fused([loc_args])[0] if n.xenc_ok(Vp, L) else n.cross_fwd(*loc_args)
        o.update(vp_embeds=c.loc.out, vp_attns=c.loc.P)

    def head(self, m, c, o, compute_loss, metrics):
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        nm = plan["n_mrc"]
        c.mx = n.new(nm, H)
        O.csr_gather(c.loc.out, *plan["mrc_rows"], c.mx, nm, H)
        l1, l2 = n.lin("image_classifier.net.0.weight"), n.lin("image_classifier.net.3.weight")
        ln = n.ln("image_classifier.net.2")
        c.mZ, c.m_rstd = n.new(nm, H), n.new(nm, dtype=torch.float32)
        if MP.MLM_TAIL_FUSED and O.linear_ln_ok(H, H):      # Linear -> ReLU -> LayerNorm as one launch; mY keeps the PRE-activation (same relu' mask)
            c.mY = n.new(nm, H)
            O.linear_act_ln(c.mx, l1.W, l1.b, nm, 2, c.mY, ln.g, ln.b, n.eps, c.mZ, c.m_rstd)
        else:
            c.mY = O.linear_fwd(c.mx, l1.W, l1.b, nm, epilogue=2)
            O.ln_fwd(nm, H, c.mZ, in0=c.mY, gamma=ln.g, beta=ln.b, eps=n.eps, rstd=c.m_rstd)
        c.mlogits = O.linear_fwd(c.mZ, l2.W, l2.b, nm)
        o["predict"] = c.mlogits

    def rows(self, plan):
        return [plan["B"] * plan["Vp"]]

    def loss(self, m, c, o, zz, scg, kd):
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        c.d_vp = zz(B * Vp, H)
        nm, Pn = plan["n_mrc"], c.mlogits.shape[1]
        c.rows = n.new(nm, dtype=torch.float32)
        c.dmlogits = n.new(nm, Pn) if m.store.requires_grad else None
        roww = plan.get("mrc_row_w")      # shape buckets (as mlm): nm counts padded rows, the true 1 / n rides in per-row weights
        O.softkl_rows(c.mlogits, nm, Pn, Pn, plan["mrc_targets"], coef=scg if roww is not None else scg / nm, row_w=roww,
                      loss_row=c.rows, dlogits=c.dmlogits, ldd=Pn)
        return c.rows, roww, (1.0 if roww is not None else 1.0 / nm)

    def kd_streams(self, c):
        p = c.plan
        return {"local": (c.loc.out, c.loc.P, p["Vp"], p["L"], c.loc.ldp, c.d_vp, None, "L")}

    def backward(self, m, c):
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        nm = plan["n_mrc"]
        l1, ln, l2 = n.lin("image_classifier.net.0.weight"), n.ln("image_classifier.net.2"), n.lin("image_classifier.net.3.weight")
        O.linear_dw(c.dmlogits, c.mZ, l2.dW, l2.db, nm)
        dZ = O.linear_dx(c.dmlogits, l2.W, nm)
        dY = n.new(nm, H)
        O.ln_bwd(nm, H, dZ, y=c.mZ, gamma=ln.g, beta=ln.b, rstd=c.m_rstd, dx=dY, dgamma=ln.dg, dbeta=ln.db)
        dpre = O.dact(dY, c.mY, 2)                 # relu'(pre) == relu'(relu(pre))
        O.linear_dw(dpre, c.mx, l1.dW, l1.db, nm)
        dmx = O.linear_dx(dpre, l1.W, nm)
        O.csr_gather(dmx, *plan["mrc_rows_T"], c.d_vp, B * Vp, H, accumulate=True)
        d_vin = n.cross_bwd(c.loc, c.d_vp, c.d_txt, c.dP_l)
        n.vp_in_bwd(c.vin, plan, d_vin, c.d_pano)

    def metrics(self, m, c, block, temperature):
        nm, Pn = c.plan["n_mrc"], c.mlogits.shape[1]
        O.eval_accum(*O.eval_rows(c.mlogits, nm, Pn, Pn, targets=c.plan["mrc_targets"]), nm, block, 0)

    def result(self, m, c, o, batch):
        return c.mlogits, c.plan["mrc_targets"], None, None


# ---- sap and cfp: the map and the viewpoint tokens both attend to the text ------------------------------------------
class _Glocal(Head):
    def cross(self, m, c, o):
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        tl, gl_, vl = plan["lens"]["txt"], plan["lens"]["gmap"], [Vp] * B

        def _local():
            vin = c.vin
            return vin, n.cross_fwd("local", plan, vin.out, Vp, plan["vp_mask"], vl, B * Vp,
                                    c.txt_out, L, plan["txt_mask"], tl, plan["txt_tokens"])
        # global (map) and local (viewpoint) co-attention encoders are independent: one launch for both when the shapes allow
        if n.xenc_ok(K, L) and n.xenc_ok(Vp, L):
            c.glob, c.loc = n.cross_fwd_fused([
                ("global", plan, c.gin.out, K, plan["gmap_mask"], gl_, plan["gmap_nodes"], c.txt_out, L, plan["txt_mask"], tl, plan["txt_tokens"], c.inp.dist),
                ("local", plan, c.vin.out, Vp, plan["vp_mask"], vl, B * Vp, c.txt_out, L, plan["txt_mask"], tl, plan["txt_tokens"])])
        else:
            c.glob, (c.vin, c.loc) = m._par(
                lambda: n.cross_fwd("global", plan, c.gin.out, K, plan["gmap_mask"], gl_, plan["gmap_nodes"],
                                    c.txt_out, L, plan["txt_mask"], tl, plan["txt_tokens"], dist=c.inp.dist), _local)
        o.update(gmap_embeds=c.glob.out, gmap_attns=c.glob.P, vp_embeds=c.loc.out, vp_attns=c.loc.P)

    def kd_streams(self, c):
        p = c.plan
        return {"global": (c.glob.out, c.glob.P, p["K"], p["L"], c.glob.ldp, c.d_gmap, "K", "L"),
                "local": (c.loc.out, c.loc.P, p["Vp"], p["L"], c.loc.ldp, c.d_vp, None, "L")}

    def _encoders_bwd(self, m, c):
        """both cross-modal encoders and their input stages, behind the head's gradients in c.d_gmap / c.d_vp"""
        n, plan = m.net, c.plan
        d_txt2 = c.d_txt2                    # the two encoders accumulate their text gradients separately (no race)
        one = not getattr(c, "islands", None) and n.nodes_pano_ok(plan, gin=c.gin, vin=c.vin)      # the fold, both input stages and the panorama fusion's backward in ONE launch (not across an island: see Mlm.backward)
        fold = None
        if n.rbw_ok():                       # both encoders in shared row-block launches (engine.cross_stacks_bwd); one text accumulator: the
            (d_gin, d_vin), fold = n.cross_stacks_bwd([(c.glob, c.d_gmap, c.d_txt, c.dP_g), (c.loc, c.d_vp, c.d_txt, c.dP_l)], defer_fold=one)      # six parts fold at the end
        else:
            d_gin, d_vin = m._par(lambda: n.cross_bwd(c.glob, c.d_gmap, c.d_txt, c.dP_g),
                                  lambda: n.cross_bwd(c.loc, c.d_vp, d_txt2, c.dP_l))
            if one:
                fold = (c.d_txt, [d_txt2])
            else:
                O.add_(c.d_txt, d_txt2)
        if one:
            n.nodes_pano_bwd(plan, c.pano, c.gin, d_gin, c.vin, d_vin, c.d_pano, c.d_fused, add=fold)
            c.pano_head_done = True
        else:
            n.nodes_in_bwd(plan, c.gin, d_gin, c.vin, d_vin, c.d_pano, c.d_fused)       # both input stages in shared launches


class Sap(_Glocal):
    def head(self, m, c, o, compute_loss, metrics):
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        use_gate = bool(cfg_get(m.config, "glocal_fuse"))
        g1, l1_ = n.lin("global_sap_head.net.0.weight"), n.lin("local_sap_head.net.0.weight")
        with _lib.group():                  # the three heads' first projections are independent: one grouped launch
            c.Yg = O.linear_fwd(c.glob.out, g1.W, g1.b, B * K, epilogue=2)
            c.Yl = O.linear_fwd(c.loc.out, l1_.W, l1_.b, B * Vp, epilogue=2)
            if use_gate:
                f1 = n.lin("sap_fuse_linear.net.0.weight")
                tmp = O.linear_fwd(c.glob.out, f1.W, None, B, lda=K * H, ldb=2 * H, K=H)
        c.g_raw = cls_tail(n, "global_sap_head.", c.Yg, B * K)
        c.l_raw = cls_tail(n, "local_sap_head.", c.Yl, B * Vp)
        if use_gate:
            c.Yf = O.linear_fwd(c.loc.out, f1.W[:, H:], f1.b, B, lda=Vp * H, ldb=2 * H, K=H, residual=tmp, epilogue=0)
            _relu(c.Yf)      # ReLU after the two partial products are summed
            fln, f2 = n.ln("sap_fuse_linear.net.2"), n.lin("sap_fuse_linear.net.3.weight")
            c.fuse_raw = n.new(B, dtype=torch.float32)
            O.lndot_fwd(c.Yf, B, H, fln.g, fln.b, n.eps, f2.Wm, f2.b, c.fuse_raw)
        else:
            c.fuse_raw = n.zeros(B, dtype=torch.float32)
        c.use_gate = use_gate
        c.gl, c.ll, c.fl = n.new(B, K, dtype=torch.float32), n.new(B, Vp, dtype=torch.float32), n.new(B, K, dtype=torch.float32)
        c.sap_fused = bool(compute_loss and O.SAP_LOSS_FUSED and K <= 512 and Vp <= 128)
        if not c.sap_fused:           # (with a loss to follow, the logit fusion rides in the loss launch: loss() / O.sap_fuse_loss)
            O.sap_fuse_fwd(B, K, Vp, c.g_raw, c.l_raw, c.fuse_raw, plan["gmask"], plan["lmask"], plan["fsrc"], plan["bwmask"],
                           use_gate, c.gl, c.ll, c.fl)
        o.update(global_logits=c.gl, local_logits=c.ll, fused_logits=c.fl)

    def rows(self, plan):
        B = plan["B"]
        return [B * plan["K"], B * plan["Vp"], B * plan["L"]]

    def loss(self, m, c, o, zz, scg, kd):
        """kd: None, or the step's distillation settings (kdl, teacher outputs t, ability weights rw, alpha, gs) -- the fused launch carries the
        teacher-sample weights and the action-distillation rows"""
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        train = m.store.requires_grad
        c.d_gmap, c.d_vp, c.d_txt2 = zz(B * K, H), zz(B * Vp, H), zz(B * L, H)
        c.rows = n.new(3, B, dtype=torch.float32)
        c.dgl, c.dll, c.dfl = (n.new(B, K, dtype=torch.float32), n.new(B, Vp, dtype=torch.float32), n.new(B, K, dtype=torch.float32)) \
            if train else (None, None, None)
        ga, la = plan["global_act_labels"], plan["local_act_labels"]
        c.sap_w = c.kdrows = None
        if c.sap_fused:
            # logit fusion + the three CE rows + teacher-sample weights + action-distillation rows: ONE launch (six before)
            kdl = kd.kdl if kd else None
            hard = bool(kd and kdl.get("teacher_sample_hard_mining", False))
            pred = bool(kd and "predict" in kdl["kdl_tasks"])
            if hard:
                c.sap_w = n.new(B, dtype=torch.float32)
            if pred:
                c.kdrows = n.new(B, dtype=torch.float32)
            if kd:
                rwd = KD.rw_device(m, kd.rw)
            O.sap_fuse_loss(B, K, Vp, c.g_raw, c.l_raw, c.fuse_raw, plan["gmask"], plan["lmask"], plan["fsrc"], plan["bwmask"], c.use_gate,
                            c.gl, c.ll, c.fl, ga, la, scg / B, c.rows, dgl=c.dgl, dll=c.dll, dfl=c.dfl,
                            t_fused=kd.t["fused_logits"] if (hard or pred) else None,
                            w_rate=float(kdl["t_sample_preprocess_exp_decay"]) if hard else 0.0, w_out=c.sap_w,
                            T=float(kdl["kd_temperature"]) if kd else 1.0, kd_norm=(1.0 / B if hard else 1.0 / (B * K)),
                            kd_coef=kd.alpha * kd.gs if kd else 0.0, kd_coef_dev=rwd[4:5] if pred else None, kd_rows=c.kdrows)
        else:
            O.ce_rows(c.gl, B, K, K, ga, coef=scg / B, loss_row=c.rows[0], dlogits=c.dgl, ldd=K)
            O.ce_rows(c.ll, B, Vp, Vp, la, coef=scg / B, loss_row=c.rows[1], dlogits=c.dll, ldd=Vp)
            O.ce_rows(c.fl, B, K, K, ga, coef=scg / B, loss_row=c.rows[2], dlogits=c.dfl, ldd=K)
        return c.rows, None, 1.0 / B

    def kd_sample_w(self, m, c, t, kdl):
        if c.sap_w is not None:
            return c.sap_w                  # written by the fused loss launch
        n, plan = m.net, c.plan
        w = n.new(plan["B"], dtype=torch.float32)
        O.ce_rows(t["fused_logits"], plan["B"], plan["K"], plan["K"], plan["global_act_labels"], w_out=w,
                  w_rate=float(kdl["t_sample_preprocess_exp_decay"]))
        return w

    def kd_predict(self, m, c, t, T, w, coef):
        if not c.sap_fused:                 # (fused: the rows are written and the gradient is in c.dfl already)
            B, K = c.plan["B"], c.plan["K"]
            c.kdrows = m.net.new(B, dtype=torch.float32)
            O.kd_rows(c.fl, t["fused_logits"], B, K, K, T, w=w, norm=(1.0 / B if w is not None else 1.0 / (B * K)),
                      coef=coef[0], coef_dev=coef[1], loss_row=c.kdrows, ds=c.dfl, accumulate=True)
        return c.kdrows

    def backward(self, m, c):
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        dg, dl, df = n.new(B, K, dtype=torch.float32), n.new(B, Vp, dtype=torch.float32), n.new(B, dtype=torch.float32)
        O.sap_fuse_bwd(B, K, Vp, c.g_raw, c.l_raw, c.fuse_raw, plan["gmask"], plan["lmask"], plan["fsrc"], plan["bwmask"],
                       c.use_gate, c.dgl, c.dll, c.dfl, dg, dl, df)
        heads = []
        for prefix, X, Y, dlogit, M, d_acc in (("global_sap_head.", c.glob.out, c.Yg, dg, B * K, c.d_gmap),
                                               ("local_sap_head.", c.loc.out, c.Yl, dl, B * Vp, c.d_vp)):
            l1, ln, l2 = n.lin(prefix + "net.0.weight"), n.ln(prefix + "net.2"), n.lin(prefix + "net.3.weight")
            dZh = n.new(M, H)
            O.lndot_bwd(Y, M, H, ln.g, ln.b, n.eps, l2.Wm, dlogit, dZh, ln.dg, ln.db, l2.dW, l2.db)
            O.linear_dw(dZh, X, l1.dW, l1.db, M)
            heads.append((dZh, l1, M, d_acc))
        with _lib.group():                      # the two heads' input gradients go to different tensors: one grouped launch
            for dZh, l1, M, d_acc in heads:
                O.linear_dx(dZh, l1.W, M, out=d_acc, residual=d_acc)
        if c.use_gate:
            gate_fuse_bwd(n, "", c, df, B, K, Vp, c.d_gmap, c.d_vp, grouped=True)
        self._encoders_bwd(m, c)

    def metrics(self, m, c, block, temperature):
        plan = c.plan
        B, K, Vp = plan["B"], plan["K"], plan["Vp"]
        ga, la = plan["global_act_labels"], plan["local_act_labels"]
        for slot, (x, N, lab) in enumerate(((c.gl, K, ga), (c.ll, Vp, la), (c.fl, K, ga))):
            O.eval_accum(*O.eval_rows(x, B, N, N, labels=lab), B, block, slot)

    def result(self, m, c, o, batch):
        return dict(global_logits=c.gl, local_logits=c.ll, fused_logits=c.fl,
                    global_act_labels=m._dev(batch["global_act_labels"]), local_act_labels=m._dev(batch["local_act_labels"]))


class Cfp(_Glocal):
    def head(self, m, c, o, compute_loss, metrics):
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        c.g0, c.v0, c.t0, c.gv0 = n.new(B, H), n.new(B, H), n.new(B, H), n.new(B, H)
        # the four [CLS]-row selections (fused = map row + viewpoint row) in one launch, the four heads as one grouped launch
        O.csr_gather_multi(H, [dict(out=c.g0, n_out=B, src1=c.glob.out, csr1=plan["g0"]),
                               dict(out=c.v0, n_out=B, src1=c.loc.out, csr1=plan["v0"]),
                               dict(out=c.t0, n_out=B, src1=c.txt_out, csr1=plan["t0"]),
                               dict(out=c.gv0, n_out=B, src1=c.glob.out, csr1=plan["g0"], src2=c.loc.out, csr2=plan["v0"])])
        with _lib.group():
            c.cfp = []
            for key, src in (("gmap", c.g0), ("vp", c.v0), ("fused", c.gv0), ("txt", c.t0)):
                hl = n.lin(f"cfp_heads.{key}.weight")
                c.cfp.append(O.linear_fwd(src, hl.W, hl.b, B))
        o["cfp"] = tuple(c.cfp)

    def rows(self, plan):
        B = plan["B"]
        return [B * plan["K"], B * plan["Vp"], B * plan["L"], B, B, B]

    def loss(self, m, c, o, zz, scg, kd):
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        train = m.store.requires_grad
        c.d_gmap, c.d_vp, c.d_txt2 = zz(B * K, H), zz(B * Vp, H), zz(B * L, H)
        c.d_cls0 = (zz(B, H), zz(B, H), zz(B, H))
        temp = float(cfg_get(m.config, "cfp_temperature"))
        c.rows = n.new(6, B, dtype=torch.float32)
        txt_o = c.cfp[3]
        c.dsim, c.d_cfp = [], None
        ar = plan["arange_b"]
        lds = c.lds = rup(B, 8)
        fused = O.cfp_loss_ok(B, H)
        if fused:                            # the three contrastive terms, forward and backward, as one launch (csrc/loss.hip cfp_loss_kernel)
            c.d_cfp = [n.new(B, H) for _ in range(4)] if train else None
            O.cfp_loss(B, H, c.cfp[:3], txt_o, temp, scg * 0.5 / B, c.rows, d_a=c.d_cfp[:3] if train else None, d_txt=c.d_cfp[3] if train else None)
        for i in (() if fused else range(3)):
            a = c.cfp[i]
            sim, simT = n.new(B, lds, dtype=torch.float32), n.new(B, lds, dtype=torch.float32)
            O.gemm(0, a, txt_o, sim, B, B, H, H, H, lds, alpha=1.0 / temp)
            O.gemm(0, txt_o, a, simT, B, B, H, H, H, lds, alpha=1.0 / temp)
            d1 = n.new(B, lds, dtype=torch.float32) if train else None
            d2 = n.new(B, lds, dtype=torch.float32) if train else None
            O.ce_rows(sim, B, B, lds, ar, coef=scg * 0.5 / B, loss_row=c.rows[2 * i], dlogits=d1, ldd=lds)
            O.ce_rows(simT, B, B, lds, ar, coef=scg * 0.5 / B, loss_row=c.rows[2 * i + 1], dlogits=d2, ldd=lds)
            c.dsim.append((d1, d2))
        c.temp = temp
        return c.rows, None, 0.5 / B

    def backward(self, m, c):
        n, plan, B, L, K, Vp, H = _sizes(m, c)
        d_outs = c.d_cfp if c.d_cfp is not None else [n.new(B, H) for _ in range(4)]
        txt_o = c.cfp[3]
        # fp32 [B,B] similarity gradient -> compute dtype operand for the MFMA GEMM
        cast = lambda d: d if d.dtype == m.compute_dtype else O.cast_to(d, m.compute_dtype)
        for i in (() if c.d_cfp is not None else range(3)):
            d1, d2 = c.dsim[i]
            a = c.cfp[i]
            it = 1.0 / c.temp
            # sim = a txt^T / temp ; simT = txt a^T / temp
            lds = c.lds
            e1, e2 = cast(d1), cast(d2)
            O.gemm(1, e1, txt_o, d_outs[i], B, H, B, lds, H, H, alpha=it)
            O.gemm(2, e2, txt_o, d_outs[i], B, H, B, lds, H, H, alpha=it, residual=d_outs[i], ldr=H)
            if i == 0:
                O.gemm(2, e1, a, d_outs[3], B, H, B, lds, H, H, alpha=it)
            else:
                O.gemm(2, e1, a, d_outs[3], B, H, B, lds, H, H, alpha=it, residual=d_outs[3], ldr=H)
            O.gemm(1, e2, a, d_outs[3], B, H, B, lds, H, H, alpha=it, residual=d_outs[3], ldr=H)
        d_g0, d_v0, d_t0 = c.d_cls0
        heads = list(zip((("gmap", c.g0, (d_g0,)), ("vp", c.v0, (d_v0,)), ("fused", c.gv0, (d_g0, d_v0)), ("txt", c.t0, (d_t0,))), d_outs))
        for (key, src, dsts), d_o in heads:
            hl = n.lin(f"cfp_heads.{key}.weight")
            O.linear_dw(d_o, src, hl.dW, hl.db, B)
        # the five input-gradient GEMMs (48 rows each: 6-10 us apiece on the chain) as TWO grouped launches: the three heads with a destination of their
        # own, then the fused head's two (they add into the map / viewpoint rows the first launch wrote)
        for sel in (("gmap", "vp", "txt"), ("fused",)):
            with _lib.group():
                for (key, src, dsts), d_o in heads:
                    if key in sel:
                        hl = n.lin(f"cfp_heads.{key}.weight")
                        for dst in dsts:
                            O.linear_dx(d_o, hl.W, B, out=dst, residual=dst)
        O.csr_gather_multi(H, [dict(out=c.d_gmap, n_out=B * K, accumulate=True, src1=d_g0, csr1=plan["g0_T"]),
                               dict(out=c.d_vp, n_out=B * Vp, accumulate=True, src1=d_v0, csr1=plan["v0_T"]),
                               dict(out=c.d_txt, n_out=B * L, accumulate=True, src1=d_t0, csr1=plan["t0_T"])])
        self._encoders_bwd(m, c)

    def metrics(self, m, c, block, temperature):
        temp = float(temperature if temperature is not None else cfg_get(m.config, "cfp_temperature"))
        for slot in range(3):
            O.eval_accum(*O.cfp_eval(c.cfp[slot], c.cfp[3], temp), c.plan["B"], block, slot)

    def result(self, m, c, o, batch):
        return o["cfp"]


UNITS = dict(mlm=Mlm(), mrc=Mrc(), sap=Sap(), cfp=Cfp())


def unit(task):
    if task not in UNITS:
        raise ValueError(task)
    return UNITS[task]
