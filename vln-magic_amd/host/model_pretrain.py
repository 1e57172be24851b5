"""`GlocalTextPathCMTPreTraining` -- the pretraining model the reference imports from its withheld
`model.pretrain_goat` (pretrain_src/train_r2r_magic.py:40) -- rebuilt on the HIP engine.

Call surface kept: `from_pretrained(None, config=..., state_dict=...)`, `.train()/.eval()`,
`model(batch, task=..., compute_loss=...)`, `state_dict()` / `named_parameters()` with the checkpoint key
names of SURVEY App. A.4.  Return contract per task: train_r2r_magic.py:440-587 (validate_*).
With `compute_loss=True` the forward also evaluates the supervised loss and the in-model MAKD terms
(against `teacher_outputs`) and seeds the explicit backward; `loss.backward()` (or `model.backward()`)
then runs the hand-written backward and leaves the gradients in `param.grad` (views of one flat buffer).
"""
import os

import torch
import torch.nn as nn

from . import heads as HD
from . import makd_pretrain as KD
from . import ops as O
from .config import cfg_get
from .ddp import refuse_torch_ddp
from .engine import Ctx, MagicNet, cls_specs, trunk_specs
from .model_common import ModelCommon, _dropout_knobs  # noqa: F401  (_dropout_knobs stays importable from here)
from .params import ParamStore
from .plan import build_plan, check_plan

MID_CUT = 2          # rounds of the shared text / panorama backward after which the data-parallel exchange cuts its middle bucket
LOCKSTEP = not os.environ.get("MAGIC_NO_LOCKSTEP")
LOCKSTEP_EAGER = bool(os.environ.get("MAGIC_LOCKSTEP_EAGER"))
DYN_TERMS = ("txt_emb", "txt_attn", "img_emb", "img_fused", "img_attn", "g_emb", "g_attn", "l_emb", "l_attn")      # plan["dyn"] slots
KD_SLOTS = ("txt_emb_loss", "txt_attn_loss", "img_emb_loss", "avg_img_emb_loss", "img_attn_loss",
            "global_emb_loss", "global_attn_loss", "local_emb_loss", "local_attn_loss", "predict_loss")


PRETRAIN_CAUSAL = ("back_txt", "back_img")       # the pretraining collates carry no front-door dictionaries


def pretrain_specs(cfg):
    H = cfg.hidden_size
    s = trunk_specs(cfg, "bert.")
    s += [("mlm_head.predictions.transform.dense.weight", (H, H), "normal"), ("mlm_head.predictions.transform.dense.bias", (H,), "zeros"),
          ("mlm_head.predictions.transform.LayerNorm.weight", (H,), "ones"), ("mlm_head.predictions.transform.LayerNorm.bias", (H,), "zeros"),
          ("mlm_head.predictions.bias", (cfg.vocab_size,), "zeros")]
    s += cls_specs("global_sap_head.", H) + cls_specs("local_sap_head.", H) + cls_specs("sap_fuse_linear.", H, 2 * H)
    for k in ("gmap", "vp", "fused", "txt"):
        s += [(f"cfp_heads.{k}.weight", (H, H), "normal"), (f"cfp_heads.{k}.bias", (H,), "zeros")]
    if "mrc" in (getattr(cfg, "pretrain_tasks", None) or ()):     # RegionClassification(H, image_prob_size), only when configured
        P = int(cfg_get(cfg, "image_prob_size"))
        s += [("image_classifier.net.0.weight", (H, H), "normal"), ("image_classifier.net.0.bias", (H,), "zeros"),
              ("image_classifier.net.2.weight", (H,), "ones"), ("image_classifier.net.2.bias", (H,), "zeros"),
              ("image_classifier.net.3.weight", (P, H), "normal"), ("image_classifier.net.3.bias", (P,), "zeros")]
    # back-door adjustment blocks (do_back_txt / do_back_img: r2r_magic_model_config.json:60-66, off in the shipped config; their inputs
    # instr_z_* / img_z_* come from the collates, pretrain_src/data/tasks.py:156-164, :441-449) -- the navigation model's blocks
    from .causal import causal_specs
    return s + causal_specs(cfg, "bert.", only=PRETRAIN_CAUSAL)


class _BackwardHook(torch.autograd.Function):
    """Lets `loss.backward()` of an unmodified training loop trigger the explicit HIP backward."""

    @staticmethod
    def forward(ctx, loss_value, anchor, model):
        ctx.model = model
        return loss_value.clone()

    @staticmethod
    def backward(ctx, grad_out):
        ctx.model.backward()
        m = ctx.model
        if m.loss_scale is not None:   # (dynamic scale: the device word the seeds were multiplied by)
            m.store.grad.mul_(grad_out.to(torch.float32) * m.loss_scale[1])
        elif m.grad_scale != 1.0:      # hand autograd's contract back: .grad = grad_out x dLoss/dparam (grad_out: e.g. a GradScaler's factor)
            m.store.grad.mul_(grad_out.to(torch.float32) / m.grad_scale)
        from .trainer import auto_sync
        auto_sync(ctx.model)           # data parallel under an unmodified loop: average the flat gradient buffer here
        return None, None, None


MLM_TAIL_FUSED = os.environ.get("MAGIC_MLM_TAIL_FUSED", "1") != "0"
# K-splits of the vocabulary input gradient d_hm = dlogits Wemb (18 output tiles alone cannot fill 256 CUs): 32 splits.  Default (round 6): each split STORES its
# partial into its own slab (magic_gemm with splitk < 0) and the transform's LayerNorm backward adds the slabs in order (magic_ln_bwd_tail): reproducible, + 13-18 us on
# an mlm step.  MAGIC_MLM_DX_ATOMICS=1: the round-3 form, fp32 atomics into one accumulator -- whenever launch timing shifts ONE element of its bf16 cast flips between
# runs and every gradient below differs at a bf16 ulp (233 of 354 tensors: profiles/micro/r06_det_probe_partial128_b.txt), which is not a property to ship for 5 us a step.
MLM_DX_SPLITK = int(os.environ.get("MAGIC_MLM_DX_SPLITK", "32"))
MLM_DX_ATOMICS = os.environ.get("MAGIC_MLM_DX_ATOMICS", "0") != "0"


class GlocalTextPathCMTPreTraining(ModelCommon, nn.Module):
    def __init__(self, config, device="cuda", compute_dtype=torch.bfloat16, seed=0):
        super().__init__()
        self.config = config
        self.device_ = torch.device(device)
        self.compute_dtype = compute_dtype
        trainable = getattr(config, "role", "student") != "teacher" or bool(getattr(config, "train_teacher", False))
        self.store = ParamStore(pretrain_specs(config), device, compute_dtype,
                                init_std=cfg_get(config, "initializer_range"), seed=seed, requires_grad=trainable)
        self.store.attach_to(self)
        self.net = MagicNet(config, self.store, "bert.")
        self.prefix, self.explicit_backward = "bert.", True
        if self.device_.type == "cuda":
            O.dw_counters(self.device_)            # the deterministic weight-gradient launch's counters: allocated outside any capture
        from .causal import build_blocks
        self.causal_blocks = build_blocks(self, only=PRETRAIN_CAUSAL)        # {} unless config.do_back_txt / do_back_img
        _dropout_knobs(self, config)
        self._anchor = torch.zeros(1, device=self.device_, requires_grad=True)
        self._ctx = None
        self._kd_idx = torch.tensor([0, 0, 1, 1, 1, 2, 2, 3, 3, 4], device=self.device_)
        self.keep_mlm_logits = False     # True: MLM CE gradient goes to its own buffer instead of overwriting the logits
        self.dropout_seed = None         # optional int32[2] device tensor: when set, forward() keys its dropout masks on it instead of drawing one
        # fp16 compute: every gradient SEED (the coefficient of each fused loss + gradient kernel) is multiplied by `grad_scale`, so the
        # activation gradients stay inside fp16's range (the reference's own fp16 option scales the loss the same way: GradScaler,
        # train_r2r_magic.py:370-371); the flat fp32 gradient buffer then holds grad_scale x the gradient and the optimizer divides
        # (PretrainStep folds 1 / grad_scale into the AdamW kernel's gradient pre-scale; under `loss.backward()` the hook below does).
        # A power of two: exact in every format.  Loss VALUES are never scaled.
        self.grad_scale = 4096.0 if compute_dtype == torch.float16 else 1.0
        # ... or DYNAMIC (enable_dynamic_loss_scale; trainer.PretrainStep turns it on for fp16): fp32[4] device state {S, 1 / S, clean steps in a
        # row, pending}; the loss kernels read S from the device (ops.seed_scale), the host coefficients then carry no scale
        self.loss_scale = None
        self.register_load_state_dict_post_hook(lambda m, k: setattr(m.store, "shadow_clean", False))

    def enable_dynamic_loss_scale(self, init=None):
        """amp.GradScaler semantics on the device (csrc/loss.hip step_rng_kernel + csrc/optim.hip adamw_kernel): returns the state tensor.
        init: the first scale (default: the static `grad_scale`; GradScaler's own default is 65536)"""
        if self.loss_scale is None:
            S = float(init if init is not None else self.grad_scale)
            self.loss_scale = torch.tensor([S, 1.0 / S, 0.0, 0.0], dtype=torch.float32, device=self.device_)
        return self.loss_scale

    # ---- HF-style constructor (train_r2r_magic.py:260-277) ------------------------------------------
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path=None, config=None, state_dict=None, **kw):
        model = cls(config, **kw)
        if state_dict is not None:
            own = model.state_dict()
            keep = {k: v for k, v in state_dict.items() if k in own and tuple(v.shape) == tuple(own[k].shape)}
            model.load_state_dict(keep, strict=False)      # unmatched keys are silently ignored, as HF does
        return model

    def _par(self, fn_main, fn_aux):
        """run two independent segments: their launches paired (lockstep), or one after the other"""
        if LOCKSTEP and self.device_.type == "cuda" and (torch.cuda.is_current_stream_capturing() or LOCKSTEP_EAGER):
            # paired launches (one kernel per two calls).  Only while a HIP graph is being captured: the two host threads
            # rendezvous on every call, which costs more than it saves when launches are issued eagerly (measured: 15 ms/step
            # eager with pairing, 6.5 without; replayed graphs: 3.4 with, 3.9 without)
            from . import lib as L
            return L.lockstep(fn_main, fn_aux)
        return fn_main(), fn_aux()

    def mark_params_dirty(self):
        self.store.shadow_clean = False

    # ---- forward ----------------------------------------------------------------------------------------
    def _causal_fwd(self, c, batch, compute_loss):
        """back-door adjustment of the text encoder's output (instruction z-dictionary) and of the panorama encoder's view embeddings (room-type
        image dictionary), where VLNBert('language' / 'panorama') applies them (host/model_nav.py): the blocks of host/causal.py
        are autograd modules, so each runs as a small autograd ISLAND inside the explicit step -- forward on a detached leaf here, its
        backward (`_causal_bwd`) turns the gradient of the adjusted tensor into the gradient of the encoder output and writes the block's
        parameter gradients into the store.  The fused panorama embedding stays the un-adjusted one, as in VLNBert('panorama')."""
        cz, plan, H = self.causal_blocks, c.plan, self.net.H
        need = {"instr_z_direction_features": "back_txt", "instr_z_landmark_features": "back_txt", "img_z_features": "back_img"}
        for k, blk in need.items():
            if batch.get(k) is not None and blk not in cz:
                from .causal import BLOCKS
                raise ValueError(f"batch carries {k!r} but config.{BLOCKS[blk]} is off -- the model has no '{blk}' block "
                                 "(pretrain_src/config/r2r_magic_model_config.json:60-66)")
        track = bool(compute_loss and self.store.requires_grad and torch.is_grad_enabled())
        c.islands = []

        def island(block, x2d, shape, z, pz):
            x0 = x2d.detach().view(shape)
            with torch.enable_grad() if track else torch.no_grad():
                if track:
                    x0.requires_grad_(True)
                y = block(x0, z, pz)
            if track:
                c.islands.append((x0, y))
            return y.detach().reshape(x2d.shape).contiguous()
        dv = lambda t: t.to(self.device_)
        if "back_txt" in cz and (batch.get("instr_z_direction_features") is not None or batch.get("instr_z_landmark_features") is not None):
            parts = [k for k in ("direction", "landmark") if batch.get(f"instr_z_{k}_features") is not None]      # direction rows first
            z = torch.cat([dv(batch[f"instr_z_{k}_features"]) for k in parts], 1)
            pz = torch.cat([dv(batch[f"instr_z_{k}_pzs"]) for k in parts], 1)
            c.txt_out = island(cz["back_txt"], c.txt.out, (plan["B"], plan["L"], H), z, pz)
            c.island_txt = len(c.islands) - 1 if track else None
        if "back_img" in cz and batch.get("img_z_features") is not None:
            out = island(cz["back_img"], c.pano.out, (plan["Np"], plan["V"], H), dv(batch["img_z_features"]), dv(batch["img_z_pzs"]))
            c.pano_adj = Ctx(**vars(c.pano))
            c.pano_adj.out = out
            c.island_pano = len(c.islands) - 1 if track else None

    def _causal_bwd(self, c):
        """gradient of the adjusted tensors -> gradient of the encoder outputs, through the islands of `_causal_fwd`"""
        for name, attr in (("island_txt", "d_txt"), ("island_pano", "d_pano")):
            i = getattr(c, name, None)
            if i is None:
                continue
            x0, y = c.islands[i]
            d = getattr(c, attr)
            torch.autograd.backward(y, d.view(y.shape).to(y.dtype))
            # a COPY: without dropout the island's add&norm hands the same tensor to both of its inputs, the deferred weight-gradient
            # GEMM of the block's output projection keeps reading it until the flush, and the encoder backward below accumulates in place
            setattr(c, attr, x0.grad.reshape(d.shape).to(d.dtype).clone())
            x0.grad = None

    def will_fuse_encoders(self, plan):
        """does a forward on `plan` run the text + panorama encoders as ONE whole-encoder launch (csrc/encoder.hip)?  The one predicate
        behind the model's own choice and the teacher stream's start gate (trainer.capture_split, stream_graph)."""
        n = self.net
        return bool(n.enc_ok(plan["L"], self.config.num_l_layers) and n.enc_ok(plan["V"], self.config.num_pano_layers))

    def forward(self, batch, task, compute_loss=True, teacher_outputs=None, rw=None, plan=None, return_outputs=False, inputs=None, heads=True,
                metrics=None, metrics_temperature=None):
        """metrics (with compute_loss=False): a 96-byte device accumulator block (ops.eval_block) -- the heads run as for compute_loss=False, the
        batch's per-row losses and hits are added into the block on the device (slots g / l / f = 0 / 1 / 2 for sap and cfp, slot 0 for mlm and
        mrc) and None is returned: the validation pass (host/validate.py) without a host read per batch.  metrics_temperature: the cfp
        temperature (default: the config's); a cfp batch above 64 samples (or H > 256) is refused, magic_cfp_eval has magic_cfp_loss's limits and
        validation has no per-op path behind it.  metrics=None: nothing changes.
        heads=False (with compute_loss=False, return_outputs=True): stop behind the encoders -- no masked-row gather, transform and vocabulary
        projection (mlm), no region classifier (mrc), no [CLS] gathers and contrastive heads (cfp), no action heads (sap).  The frozen MAKD teacher's
        forward (trainer.teacher_forward): distillation reads its embeddings and attention maps, and its sap logits only when configured to."""
        if not heads and (compute_loss or not return_outputs):
            raise ValueError("heads=False returns the encoders' outputs only: compute_loss=False, return_outputs=True")
        if metrics is not None and (compute_loss or return_outputs or not heads):
            raise ValueError("metrics=<block> goes with compute_loss=False and returns None")
        n, unit = self.net, HD.unit(task)
        refuse_torch_ddp(self)
        self.store.sync_shadow()
        O.deferred_clear()            # anything left by a pass that raised half-way is stale
        if self.store.requires_grad:
            O.defer_dw(False)         # a compute_loss forward that was never followed by backward() left deferral armed
        self._arm_dropout()
        plan = plan if plan is not None else build_plan(batch, task, self.device_)
        check_plan(plan, self.config)
        inp = inputs if inputs is not None else self._inputs(batch, plan)
        c = Ctx(task=task, plan=plan, inp=inp)
        # the text and panorama encoders are independent: run them on two streams
        # both self-attention encoders as ONE launch (csrc/encoder.hip) when the shapes allow: embeddings first (paired), then the launch
        fuse = self.will_fuse_encoders(plan)
        if n.embed_in_ok():        # both input embeddings in one launch behind the image projection, then the layers
            ct, cp = n.embeds_fwd(plan, inp.feats, inp.loc)
            c.txt, c.pano = self._par(lambda: n.text_fwd(plan, defer=fuse, c=ct), lambda: n.pano_fwd(plan, inp.feats, inp.loc, defer=fuse, c=cp))
        else:
            c.txt, c.pano = self._par(lambda: n.text_fwd(plan, defer=fuse), lambda: n.pano_fwd(plan, inp.feats, inp.loc, defer=fuse))
        if fuse:
            n.encoders_fwd(c.txt, c.pano)
        c.txt_out, c.pano_adj = c.txt.out, c.pano
        if self.causal_blocks or any(batch.get(k) is not None for k in ("instr_z_direction_features", "instr_z_landmark_features", "img_z_features")):
            self._causal_fwd(c, batch, compute_loss)
        # map-token and viewpoint-token inputs of the cross-modal encoders: one launch for both (gathers + position / step embeddings)
        c.gin, c.vin = n.nodes_in_fwd(plan, c.pano_adj, inp.gpos if unit.gpos else None, inp.vpos if unit.vpos else None)
        o = dict(txt_embeds=c.txt_out, txt_attns=c.txt.P, pano_embeds=c.pano_adj.out, pano_fused_embeds=c.pano.fused,
                 img_attns=c.pano.img_attn, plan=plan, inputs=inp)
        unit.cross(self, c, o)
        if heads:                  # (False: distillation reads the encoders' outputs only)
            unit.head(self, c, o, compute_loss, metrics)
        if not compute_loss:
            if metrics is not None:
                self._eval_metrics(c, task, metrics, metrics_temperature)
                return None
            return o if return_outputs else unit.result(self, c, o, batch)
        self._ctx = c
        if callable(teacher_outputs):          # teacher forward running on a side stream: join here
            teacher_outputs = teacher_outputs()
        scaled = self.loss_scale is not None and self.store.requires_grad
        if scaled:
            O.seed_scale(self.loss_scale)          # every gradient-seeding loss launch below multiplies its seed by the device-side scale
        try:
            out = self._losses(c, o, teacher_outputs, rw)
        finally:
            if scaled:
                O.seed_scale(None)
        out["outputs"] = o
        if self.store.requires_grad and torch.is_grad_enabled():
            out["loss"] = _BackwardHook.apply(out["loss"], self._anchor, self)
        return out

    def _eval_metrics(self, c, task, block, temperature=None):
        """the batch's validation rows, added into `block` on the device (the driver's validate_* arithmetic, train_r2r_magic.py:441-587)"""
        HD.unit(task).metrics(self, c, block, temperature)

    # ---- losses + gradient seeds ------------------------------------------------------------------------
    def _losses(self, c, o, t, rw):
        n, cfg, plan, unit = self.net, self.config, c.plan, HD.unit(c.task)
        B, L, H = plan["B"], plan["L"], n.H
        train = self.store.requires_grad
        O.defer_dw(train)         # the distillation heads' weight gradients join the deferred grouped launch of backward()
        kdl = getattr(cfg, "kdl", None)
        kd = t is not None and kdl is not None
        alpha = float(kdl["kd_alpha"]) if kd else 0.0
        sc = 1.0 - alpha
        dyn = train and self.loss_scale is not None      # dynamic loss scale: the kernels multiply their seeds by the device word, not the host
        gs = float(self.grad_scale) if (train and not dyn) else 1.0
        scg = sc * gs                    # coefficient of the supervised gradient seeds (the loss values use sc)
        # every zero-initialised gradient accumulator of the step comes out of ONE zeroed arena per dtype (two fills instead of ~12 tiny ones)
        nm_ = unit.dx_rows(plan)
        c.dx_slabs = MLM_DX_SPLITK if (nm_ and MLM_TAIL_FUSED and not MLM_DX_ATOMICS and MLM_DX_SPLITK > 1) else 0
        if c.dx_slabs:                     # [splits, n_mask, H] slabs, every element stored by its split: no zeroing
            f32 = n.zeros(16, dtype=torch.float32)
            c.slots, c.d_hm32 = f32, n.new(c.dx_slabs * nm_, H, dtype=torch.float32)
        else:
            f32 = n.zeros(16 + nm_ * H, dtype=torch.float32)
            c.slots, c.d_hm32 = f32[:16], (f32[16:].view(nm_, H) if nm_ else None)
        if train:
            rows = [B * L, plan["Np"] * plan["V"], plan["Np"]] + unit.rows(plan)             # d_txt, d_pano, d_fused, then the task's
            arena = n.zeros(sum(rows) * H)
            offs = [0]
            for r in rows:
                offs.append(offs[-1] + r * H)
            pool = [arena[offs[i]:offs[i + 1]].view(rows[i], H) for i in range(len(rows))]

            def zz(*shape):
                t = pool.pop(0)
                assert tuple(t.shape) == tuple(shape), (tuple(t.shape), shape)
                return t
        else:
            zz = lambda *s: None
        c.d_txt, c.d_pano, c.d_fused = zz(B * L, H), zz(plan["Np"] * plan["V"], H), zz(plan["Np"], H)
        c.dP_txt = c.dP_pano = c.dP_g = c.dP_l = None
        c.kd_emb, c.kd_mse = [], []
        res = {}
        kds = Ctx(kdl=kdl, t=t, rw=rw, alpha=alpha, gs=gs) if kd else None
        sup_rows, sup_w, sup_scale = unit.loss(self, c, o, zz, scg, kds)
        kd_rows, rwd = KD.terms(self, c, o, unit, kds) if kd else (None, None)
        # supervised mean, the action-distillation row sum, the ten ability-weighted MAKD terms, their sum and the total: ONE launch
        lo = O.loss_assemble(sup_rows.reshape(-1), sup_w, sup_scale, kd_rows, c.slots, rwd, alpha, kd, n.new(16, dtype=torch.float32))
        res["supervised_loss"] = lo[0]
        if kd:
            res["kdl_terms"] = {k: lo[1 + i] for i, k in enumerate(KD_SLOTS)}
            res["kdl_loss"] = lo[11]
        res["loss"] = lo[12]
        return res

    # ---- backward ---------------------------------------------------------------------------------------
    def backward(self, on_bucket=None):
        """the explicit backward in two phases (heads + cross-modal encoders | text + panorama encoders).  on_bucket(i, ctx):
        called when gradient bucket i is final -- 0 after phase 1 (its weight-gradient GEMMs are flushed first), 1 at the end
        (trainer.GradSync launches the data-parallel exchange of that bucket from it)."""
        self.backward_phase1()
        c = self._ctx
        if on_bucket is not None:
            # bucket 0's weight gradients are still QUEUED at this point (phase 1 and the forward's distillation heads defer them):
            # they must be on the stream before the hook makes the exchange stream wait on it, or RCCL reduces the range while the
            # grouped dW kernels still add into it (same order as trainer.capture_split: phase 1; flush; cut)
            O.flush_dw(keep_active=True)
            on_bucket(0, c)

            def cut():                      # the top MID_CUT blocks of the text / panorama stacks are done: their slice is final once flushed
                O.flush_dw(keep_active=True)
                on_bucket(1, c)
            self.backward_phase2(on_cut=cut)
            on_bucket(2, c)
        else:
            self.backward_phase2()

    @torch.no_grad()
    def backward_phase1(self):
        c = self._ctx
        assert c is not None, "backward() without a compute_loss=True forward"
        self.store.ensure_grads()
        O.defer_dw(True)          # weight-gradient GEMMs are queued and launched grouped at the end
        HD.unit(c.task).backward(self, c)

    @torch.no_grad()
    def backward_phase2(self, on_cut=None):
        """text / panorama encoders + embeddings (the caller flushes phase 1's queued weight-gradient GEMMs first when bucket 0 of the
        exchange must be final before this phase starts).  on_cut(): called once, when the top MID_CUT blocks of both stacks are done
        (trainer.GradSync's middle bucket: text layers [nl - MID_CUT, nl) + the panorama layers); on paths without the shared row-block
        backward it is called right before the end -- the middle bucket is then simply not early."""
        c = self._ctx
        n, plan = self.net, c.plan
        fired = []
        if getattr(c, "islands", None):
            self._causal_bwd(c)

        done = getattr(c, "pano_head_done", False)          # phase 1's nodes_pano_bwd carried the panorama fusion's backward

        def on_iter(k):
            if on_cut is not None and k == MID_CUT and not fired:
                fired.append(k)
                on_cut()
        if n.rbw_ok() and n.enc_ok(plan["L"], self.config.num_l_layers) and n.enc_ok(plan["V"], self.config.num_pano_layers):
            n.encoders_bwd(c.txt, c.pano, plan, c.d_txt, c.dP_txt, c.d_pano, c.d_fused, c.dP_pano, on_iter=on_iter, pano_head_done=done)      # both stacks in shared launches
            if on_cut is not None and not fired:
                on_cut()
        elif on_cut is not None:
            self._par(lambda: n.text_bwd(c.txt, plan, c.d_txt, c.dP_txt),
                      lambda: n.pano_bwd(c.pano, plan, c.d_pano, c.d_fused, c.dP_pano, pano_head_done=done))
            on_cut()
        else:
            self._par(lambda: n.text_bwd(c.txt, plan, c.d_txt, c.dP_txt),
                      lambda: n.pano_bwd(c.pano, plan, c.d_pano, c.d_fused, c.dP_pano, pano_head_done=done))
        O.flush_dw()                           # deferred weight-gradient GEMMs, ~8 problems per launch
        self._ctx = None
