"""The in-model MAKD terms of a pretraining step (pretrain flavour; oracle/makd_ref.pretrain_makd), beside host/makd_nav.py (the navigator's).
`terms()` queues the embedding and attention terms of the text, panorama, global and local abilities and flushes them; what is task-specific
it reads through the step's head unit (host/heads.py: `kd_streams`, `kd_sample_w`, `kd_predict`).

The distillation terms of a step are independent of each other: their five student->teacher-width projections go out as
ONE grouped GEMM launch, all MSE terms (<= 10) as ONE launch, and the five projection input-gradients as ONE grouped launch.
Shape-bucketed batches under graph replay (host/stream_graph.py, host/bucket.py): plan["dyn"] = {i: int32[2 n], f: fp32[n], fill: {}}.
A distillation term then takes its TRUE (outer, inner) extent and its normaliser from device memory (slot of DYN_TERMS), and registers
how the slot is computed from the batch's true sizes -- fill[term](true) -> (outer, inner, norm) -- for StreamStep to evaluate per batch."""
import torch

from . import lib as L
from . import model_pretrain as MP
from . import ops as O


def _dyn(c, term, fn, mod=0):
    d = c.plan.get("dyn")
    if d is None:
        return {}
    i = MP.DYN_TERMS.index(term)
    d["fill"][term] = fn
    return dict(valid_dev=d["i"][2 * i:2 * i + 2], norm_dev=d["f"][i:i + 1], norm=1.0, valid_mod=mod)


def _kd_emb(m, c, slot, s_t, t_t, proj, M, outer, w, coef, d_acc, dyn=None):
    c.kd_emb.append((slot, s_t, t_t, m.net.lin(f"bert.{proj}.weight"), M, outer, w, coef, d_acc, dyn))


def _kd_attn(m, c, slot, sP, tP, Bn, Nq, Nk, ldp, nh_s, nh_t, w, coef, dyn=None):
    """dyn = (term, 'q' | None = which true size bounds the query rows, which true sizes enter the normaliser as (Nq, Nk))"""
    n = m.net
    hmin = min(nh_s, nh_t)
    dP = None
    if m.store.requires_grad:      # every student head is written when hmin == nh_s (pad columns included): no fill needed
        dP = (n.new if hmin == nh_s else n.zeros)(Bn, nh_s, Nq, ldp, dtype=torch.float32)
    q = dict(s=sP, t=tP, outer=Bn, inner=hmin * Nq * ldp, s_stride=nh_s * Nq * ldp, t_stride=nh_t * Nq * ldp, w=w, rows_per_w=1,
             norm=1.0 / (Bn * hmin * Nq * Nk), coef=coef[0], coef_dev=coef[1], loss=c.slots[slot:slot + 1], ds=dP,
             g_stride=nh_s * Nq * ldp)
    if dyn is not None:
        term, qk, kk = dyn           # names of the true sizes of the query / key extents (None: the extent is not padded)
        q.update(_dyn(c, term, lambda t, Bn=Bn, hmin=hmin, Nq=Nq, Nk=Nk, ldp=ldp, qk=qk, kk=kk:
                      (Bn, (t[qk] if qk else Nq) * ldp, 1.0 / (Bn * hmin * (t[qk] if qk else Nq) * (t[kk] if kk else Nk))), mod=Nq * ldp))
    c.kd_mse.append(q)
    return dP


def kd_flush(m, c):
    n, train = m.net, m.store.requires_grad
    jobs = c.kd_emb
    # projection + MSE + input gradient of every embedding term in ONE launch (csrc/kdemb.hip) when all of the step's are in its supported set
    # (16-bit storage, 128 -> 256, contiguous 16-byte-aligned rows); else the three launches below
    fused = bool(jobs) and all(
        O.kd_emb_ok(s_t.dtype, pl.K, pl.N) and t_t.dtype == s_t.dtype and s_t.is_contiguous() and t_t.is_contiguous() and pl.W.is_contiguous()
        and not ((s_t.data_ptr() | t_t.data_ptr() | pl.W.data_ptr() | (d_acc.data_ptr() if train else 0)) & 15)
        and (not train or d_acc.is_contiguous()) for (_, s_t, t_t, pl, _, _, _, _, d_acc, _) in jobs)
    sps = [None] * len(jobs)
    if not fused:
        with L.group():
            sps = [O.linear_fwd(s_t, pl.W, pl.b, M) for (_, s_t, _, pl, M, _, _, _, _, _) in jobs]
    dss, emb = [], []
    for (slot, s_t, t_t, pl, M, outer, w, coef, d_acc, dyn), sp in zip(jobs, sps):
        Ht = pl.N
        inner = (M // outer) * Ht
        ds = n.new(M, Ht) if train else None
        dss.append(ds)
        q = dict(s=sp, t=t_t, outer=outer, inner=inner, s_stride=inner, t_stride=inner, w=w, rows_per_w=1, norm=1.0 / (M * Ht),
                 coef=coef[0], coef_dev=coef[1], loss=c.slots[slot:slot + 1], ds=ds, g_stride=inner)
        if dyn is not None:           # (term, true size bounding the OUTER extent or None, true size bounding the rows of a block or None)
            term, ok, ik = dyn
            rows = M // outer
            q.update(_dyn(c, term, lambda t, outer=outer, rows=rows, Ht=Ht, ok=ok, ik=ik:
                          ((t[ok] if ok else outer), (t[ik] if ik else rows) * Ht,
                           1.0 / ((t[ok] if ok else outer) * (t[ik] if ik else rows) * Ht))))
        if fused:
            q.pop("valid_mod", None)
            q.update(s=s_t, M=M, W=pl.W, b=pl.b, d_acc=d_acc if train else None)
            emb.append(q)
        else:
            c.kd_mse.append(q)
    if emb:
        O.kd_emb(emb)
    if c.kd_mse:
        O.mse_multi(c.kd_mse)
    if train:
        for (slot, s_t, t_t, pl, M, outer, w, coef, d_acc, dyn), ds in zip(jobs, dss):
            O.linear_dw(ds, s_t, pl.dW, pl.db, M)
        if not fused:
            with L.group():
                for (slot, s_t, t_t, pl, M, outer, w, coef, d_acc, dyn), ds in zip(jobs, dss):
                    O.linear_dx(ds, pl.W, M, out=d_acc, residual=d_acc)
    c.kd_emb, c.kd_mse = [], []


def rw_device(m, rw):
    """MKRW ability weights as a DEVICE tensor (a captured HIP graph re-reads them every replay)"""
    if rw is None:
        rw = [1.0] * 5
    if torch.is_tensor(rw) and rw.is_cuda:
        return rw
    cached = getattr(m, "_rwd_cache", None)
    key = tuple(float(x) for x in rw)
    if cached is None or cached[0] != key:
        m._rwd_cache = cached = (key, torch.tensor(list(key), dtype=torch.float32).to(m.device_))
    return cached[1]


def terms(m, c, o, unit, kd):
    """queue and launch the step's distillation terms into c.slots; kd: the step's settings (kdl, teacher outputs t, rw, alpha, gs).
    Returns (rows of the action-distillation term or None, the ability weights on the device)."""
    n, plan, kdl, t = m.net, c.plan, kd.kdl, kd.t
    B, L, Np, V = plan["B"], plan["L"], plan["Np"], plan["V"]
    train = m.store.requires_grad
    rwd = rw_device(m, kd.rw)
    rw = [(kd.alpha * kd.gs, rwd[i:i + 1]) for i in range(5)]       # (host factor of the gradient seed, device-side ability weight)
    tasks, types = kdl["kdl_tasks"], kdl["kdl_task_types"]
    emb, att = "emb" in types, "attn" in types
    w = unit.kd_sample_w(m, c, t, kdl) if kdl.get("teacher_sample_hard_mining", False) else None
    nh_s = n.nh
    nh_t = t["txt_attns"].shape[1]
    if "txt" in tasks:
        if emb:
            _kd_emb(m, c, 0, o["txt_embeds"], t["txt_embeds"], "txt_emb_w", B * L, B, w, rw[0], c.d_txt, dyn=("txt_emb", None, "L"))
        if att:
            c.dP_txt = _kd_attn(m, c, 1, o["txt_attns"], t["txt_attns"], B, L, L, c.txt.ldp, nh_s, nh_t, w, rw[0], dyn=("txt_attn", "L", "L"))
    # panorama tensors have leading dim sum(T): the sample weights [B] only broadcast (and are only applied by
    # mse_loss, pretrain kd_loss.py:11-16) when every trajectory has exactly one step
    wp = w if (w is not None and Np == B) else None
    if "img" in tasks:
        if emb:
            _kd_emb(m, c, 2, o["pano_embeds"], t["pano_embeds"], "kdl_img_w", Np * V, Np, wp, rw[1], c.d_pano, dyn=("img_emb", "Np", None))
            _kd_emb(m, c, 3, o["pano_fused_embeds"], t["pano_fused_embeds"], "kdl_avg_img_w", Np, Np, wp, rw[1], c.d_fused, dyn=("img_fused", "Np", None))
        if att:
            ldp = c.pano.ldp
            g_img = n.new(Np, V, ldp, dtype=torch.float32) if train else None
            q = dict(s=o["img_attns"], t=t["img_attns"], outer=Np, inner=V * ldp, s_stride=V * ldp, t_stride=V * ldp, w=wp, rows_per_w=1,
                     norm=1.0 / (Np * V * V), coef=rw[1][0], coef_dev=rw[1][1], loss=c.slots[4:5], ds=g_img, g_stride=V * ldp)
            q.update(_dyn(c, "img_attn", lambda tr, V=V, ldp=ldp: (tr["Np"], V * ldp, 1.0 / (tr["Np"] * V * V))))
            c.kd_mse.append(q)
    # the cross-modal abilities: whichever of the two the task's unit ran
    streams = unit.kd_streams(c)
    for ability, e_slot, proj, t_emb, t_att, g, coef in (("global", 5, "global_cross_w", "gmap_embeds", "gmap_attns", "g", rw[2]),
                                                         ("local", 7, "local_cross_w", "vp_embeds", "vp_attns", "l", rw[3])):
        if ability in tasks and ability in streams:
            x, Pm, Nq, Nk, ldp, d_acc, qk, kk = streams[ability]
            if emb:
                _kd_emb(m, c, e_slot, x, t[t_emb], proj, B * Nq, B, w, coef, d_acc, dyn=(g + "_emb", None, qk))
            if att:
                setattr(c, "dP_" + g, _kd_attn(m, c, e_slot + 1, Pm, t[t_att], B, Nq, Nk, ldp, nh_s, nh_t, w, coef, dyn=(g + "_attn", qk, kk)))
    kd_flush(m, c)
    if "img" in tasks and att and train:
        c.dP_pano = n.new(Np, nh_s, V, c.pano.ldp, dtype=torch.float32)
        O.head_mean_bwd(g_img, c.dP_pano, Np, nh_s, V * c.pano.ldp)
    kd_rows = unit.kd_predict(m, c, t, float(kdl["kd_temperature"]), w, rw[4]) if "predict" in tasks else None
    return kd_rows, rwd
