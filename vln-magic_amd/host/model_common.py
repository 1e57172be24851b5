"""What the pretraining model (host/model_pretrain.py) and the navigator (host/model_nav.py) both are: a ParamStore + MagicNet behind an
nn.Module, with the config's dropouts held by two knob modules and the batch moved to the device the same way."""
import torch
import torch.nn as nn

from . import ops as O
from .config import cfg_get
from .engine import Ctx


def _dropout_knobs(model, config):
    """Two nn.Dropout modules that compute nothing: they only HOLD the probabilities, so that the reference's
    `set_dropout(model, p)` (utils/misc.py:19-25: every nn.Dropout module's p := p) and train()/eval() keep working; the
    masks themselves are generated inside the HIP kernels (csrc/common.hpp)."""
    model.dropout = nn.Dropout(float(cfg_get(config, "hidden_dropout_prob")))
    model.attention_dropout = nn.Dropout(float(cfg_get(config, "attention_probs_dropout_prob")))


class ModelCommon:
    """mixin over `self.net`, `self.store`, `self.device_`, `self.compute_dtype` and the two dropout knobs"""

    def _arm_dropout(self):
        """model.train() (train_r2r_magic.py:358) turns the config's dropouts on (r2r_magic_model_config.json:2-3,6); the seed
        is drawn on the device by torch's graph-safe generator, so a replayed HIP graph gets fresh masks every step."""
        ph, pa = float(self.dropout.p), float(self.attention_dropout.p)
        if self.training and self.store.requires_grad and torch.is_grad_enabled() and (ph > 0 or pa > 0):
            seed = getattr(self, "dropout_seed", None)       # PretrainStep: a device word pair its step prologue refreshes every step (one launch with the MKRW draw)
            if seed is None:
                seed = torch.randint(0, 2 ** 31 - 1, (2,), dtype=torch.int32, device=self.device_)
            self.net.set_dropout(seed, ph, pa)
        else:
            self.net.set_dropout(None)

    def _dev(self, t, dtype=None):
        t = t.to(self.device_, non_blocking=True)
        return t if dtype is None or t.dtype == dtype else t.to(dtype)

    def _inputs(self, batch, plan):
        Np, V = plan["Np"], plan["V"]
        if batch.get("view_table") is not None:
            # index-only batch (host/feature_table.py): the view features are gathered on the device from
            # the packed HBM table in the reference's token order; nothing but 37 int32 per panorama crossed PCIe
            x = batch["view_table"].gather(batch["traj_vp_row"], batch["traj_view_order"]).reshape(Np * V, -1)
        else:
            x = self._dev(batch["traj_view_img_fts"]).reshape(Np * V, -1)
        if x.dtype != self.compute_dtype:
            x = O.cast_to(x.contiguous(), self.compute_dtype)
        return Ctx(feats=x,
                   loc=self._dev(batch["traj_loc_fts"], torch.float32).reshape(Np * V, -1).contiguous(),
                   gpos=self._dev(batch["gmap_pos_fts"], torch.float32).reshape(plan["B"] * plan["K"], -1).contiguous(),
                   vpos=self._dev(batch["vp_pos_fts"], torch.float32).reshape(plan["B"] * plan["Vp"], -1).contiguous(),
                   dist=self._dev(batch["gmap_pair_dists"], torch.float32).contiguous())
