"""The validation pass of the pretraining driver on the device: a drop-in for `validate` / `validate_mlm` / `validate_mrc` / `validate_sap` /
`validate_cfp` of pretrain_src/train_r2r_magic.py:412-587 (same names, arguments, return values and val_log keys).

The driver's loops end every batch in 3-7 `.item()` reads.  Here a batch adds its rows into one 96-byte accumulator block on the device
(`model(batch, task, compute_loss=False, metrics=block)`, csrc/evaltail.hip); the block is read ONCE per task, after the last batch, and the
divisions happen on the host as in the driver.  With `torch.distributed` initialised the block is summed over the ranks once before the
division (`merge_block`: the driver's three all_gathers as one all-reduce).

Loader items: plain collated batches run eagerly; packed records (loader.pack / loader.pack_bucketed, what StreamStep.step takes) are unpacked
on the device, and with `graphs=True` bucket-padded records replay ONE captured forward + metric graph per (task, layout) -- a static record
buffer, one H2D copy, one graph launch, an LRU of `max_graphs` entries, as stream_graph.StreamStep.  A final batch with a smaller B is simply
another layout.
"""
import logging
import pickle
import time

import torch

from . import ops as O
from .lib import capture as _capture
from .loader import unpack
from .plan import check_plan

LOGGER = logging.getLogger(__name__)
SLOTS = 4


def read_block(block):
    """accumulator block (12 x 8 bytes, any device) -> dict(loss=[4 floats], hits=[4 ints], rows=[4 ints]); ONE device -> host copy"""
    host = block.detach().to("cpu").contiguous().view(torch.int64)
    return dict(loss=host[:SLOTS].view(torch.float64).tolist(), hits=host[SLOTS:2 * SLOTS].tolist(), rows=host[2 * SLOTS:3 * SLOTS].tolist())


def merge_block(block):
    """sum of the block over the ranks of torch.distributed (one all-reduce; counts travel as doubles, exact below 2^53); the block itself
    when no process group is initialised.  Works on a CPU block (gloo) and on a device block (nccl)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return block
    b = block.contiguous().view(torch.int64)
    flat = torch.cat([b[:SLOTS].view(torch.float64), b[SLOTS:].to(torch.float64)])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    return torch.cat([flat[:SLOTS].view(torch.int64), flat[SLOTS:].round().to(torch.int64)])


def val_log(task, block, seconds):
    """the driver's val_log of one task from the (merged) block: divisions on the host, as :456-464, :489-497, :521-532, :573-584; a pass
    without a counted row raises ZeroDivisionError, as the driver's arithmetic does"""
    d = block if isinstance(block, dict) else read_block(block)
    loss, hits, rows = d["loss"], [int(x) for x in d["hits"]], [int(x) for x in d["rows"]]
    n = rows[0]
    if task.startswith("mlm"):
        return {"loss": loss[0] / n, "acc": hits[0] / n, "tok_per_s": n / seconds}
    if task.startswith("mrc"):
        return {"loss": loss[0] / n, "acc": hits[0] / n, "feat_per_s": n / seconds}
    if task.startswith("sap") or task.startswith("cfp"):
        return {"gloss": loss[0] / n, "lloss": loss[1] / n, "floss": loss[2] / n,
                "gacc": hits[0] / n, "lacc": hits[1] / n, "facc": hits[2] / n, "tok_per_s": n / seconds}
    raise ValueError(f"Undefined task {task}")


class _Entry:
    pass


class Validator:
    def __init__(self, model, feature_table=None, graphs=True, max_graphs=32):
        """graphs: replay a captured graph per (task, layout) for bucket-padded packed records (the default: measured faster than the eager pass
        over a whole validation; plain batches and unpadded records run eagerly either way); max_graphs: layouts kept, least
        recently used dropped"""
        self.model, self.ftab, self.graphs, self.max_graphs = model, feature_table, bool(graphs), int(max_graphs)
        self.dev = model.device_
        self.block = O.eval_block(self.dev)
        self.cache = {}
        self.captures = 0
        self.last_block = None
        model._magic_validator = self

    # ---- one batch -----------------------------------------------------------------------------------------------------------------
    def _forward(self, task, batch, plan, temperature):
        self.model(batch, task, compute_loss=False, plan=plan, metrics=self.block, metrics_temperature=temperature)

    def _touch(self, key, e):
        self.cache.pop(key, None)
        self.cache[key] = e
        while len(self.cache) > self.max_graphs:
            old = next(iter(self.cache))
            if old == key:
                break
            torch.cuda.synchronize()              # its graph may still be in flight
            del self.cache[old]

    def _capture(self, key, task, rec, parsed, temperature):
        e = _Entry()
        e.dbuf = torch.empty(int(rec["buf"].numel()), dtype=torch.uint8, device=self.dev)
        e.batch, e.plan = unpack(rec, self.dev, dbuf=e.dbuf, parsed=parsed)
        e.ring = [[None, torch.cuda.Event()] for _ in range(4)]      # pinned sources of the copies in flight
        e.ring[0][0], e.turn = e.plan["_stage"], 1                   # (this record's: unpack pinned it and queued its copy)
        if self.ftab is not None:
            e.batch["view_table"] = self.ftab
        self.model.store.sync_shadow()            # outside the capture: a dirty shadow would put the whole master -> 16-bit cast into the graph
        torch.cuda.synchronize()
        e.graph = torch.cuda.CUDAGraph()
        with _capture(e.graph, capture_error_mode="relaxed"):
            self._forward(task, e.batch, e.plan, temperature)
        self.captures += 1
        return e

    def _record(self, task, rec, temperature):
        parsed = pickle.loads(rec["blob"])
        manifest, meta = parsed
        check_plan(dict(limits=meta["limits"], L=meta["L"], V=meta["V"]), self.model.config)
        if not (self.graphs and "true" in meta):
            batch, plan = unpack(rec, self.dev, parsed=parsed)
            if self.ftab is not None:
                batch["view_table"] = self.ftab
            return self._forward(task, batch, plan, temperature)
        key = (task, temperature) + tuple((k, dt, shape, o) for k, dt, shape, o, _ in manifest)
        e = self.cache.get(key)
        if e is None:
            e = self._capture(key, task, rec, parsed, temperature)      # (copies this record into the new static buffer as well)
        else:
            buf = rec["buf"]
            if not buf.is_pinned():
                buf = buf.pin_memory()
            slot = e.ring[e.turn]
            slot[1].synchronize()                                      # (no-op unless the host is four batches of this layout ahead)
            e.dbuf.copy_(buf, non_blocking=True)
            slot[0] = buf
            slot[1].record()
            e.turn = (e.turn + 1) % len(e.ring)
        self._touch(key, e)
        e.graph.replay()

    # ---- one task ------------------------------------------------------------------------------------------------------------------
    def accumulate(self, task, loader, temperature=None):
        """the batch loop: every batch of `loader` added into self.block; no device -> host transfer"""
        kind = task[:3]
        # a replayed graph never enters the model's forward, which is where the 16-bit weight shadow is refreshed after load_state_dict,
        # mark_params_dirty or a step of an optimizer other than FusedAdamW: refresh it here, once per pass (nav_graph.py does the same)
        self.model.store.sync_shadow()
        for item in loader:
            if isinstance(item, dict) and "blob" in item and "buf" in item:
                self._record(kind, item, temperature)
            else:
                self._forward(kind, item, None, temperature)

    def run(self, task, loader, temperature=None):
        """the pass over `loader` for one task -> (block as read_block's dict, merged over the ranks; seconds)"""
        model = self.model
        was_training = model.training
        model.eval()
        st = time.time()
        try:
            with torch.no_grad():
                self.block.zero_()
                self.accumulate(task, loader, temperature)
                block = self.block
                import torch.distributed as dist
                if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                    block = merge_block(block if dist.get_backend() == "nccl" else block.cpu())
                self.last_block = read_block(block)                     # the one device -> host read of the pass
        finally:
            model.train(was_training)
        return self.last_block, time.time() - st

    def val_log(self, task, loader, temperature=None):
        block, seconds = self.run(task, loader, temperature)
        return val_log(task, block, seconds)


def validator_of(model):
    """the model's Validator (the last one built for it; a default one otherwise): its captured graphs live across validation rounds"""
    v = getattr(model, "_magic_validator", None)
    return v if v is not None else Validator(model)


def validate_mlm(model, val_loader):
    LOGGER.info("start running MLM validation...")
    log = validator_of(model).val_log("mlm", val_loader)
    LOGGER.info(f"validation finished, acc: {log['acc'] * 100:.2f}")
    return log


def validate_mrc(model, val_loader):
    LOGGER.info("start running MRC validation...")
    log = validator_of(model).val_log("mrc", val_loader)
    LOGGER.info(f"validation finished, score: {log['acc'] * 100:.2f}")
    return log


def validate_sap(model, val_loader):
    LOGGER.info("start running SAP validation...")
    log = validator_of(model).val_log("sap", val_loader)
    LOGGER.info(f"validation finished, gacc: {log['gacc'] * 100:.2f}, lacc: {log['lacc'] * 100:.2f}, facc: {log['facc'] * 100:.2f}")
    return log


def validate_cfp(model, val_loader, temperature):
    LOGGER.info("start running CFP validation...")
    log = validator_of(model).val_log("cfp", val_loader, temperature)
    LOGGER.info(f"validation finished, gacc: {log['gacc'] * 100:.2f}, lacc: {log['lacc'] * 100:.2f}, facc: {log['facc'] * 100:.2f}")
    return log


def validate(model, val_dataloaders, setname='', max_metrix=None, tem=None):
    """every task of `val_dataloaders`; the logs of the round are kept in validator_of(model).logs under the driver's `val{setname}_{task}_{k}` names.
    Returns (max_metrix, updated) when max_metrix is given -- the best unseen fused SAP accuracy so far, :423-426 -- else None."""
    v = validator_of(model)
    v.logs = {}
    max_update_flag = False
    for task, loader in val_dataloaders.items():
        LOGGER.info(f"validate val{setname} on {task} task")
        if task.startswith("mlm"):
            log = validate_mlm(model, loader)
        elif task.startswith("mrc"):
            log = validate_mrc(model, loader)
        elif task.startswith("sap"):
            log = validate_sap(model, loader)
            if setname == "_unseen" and max_metrix is not None and log["facc"] >= max_metrix:
                max_metrix, max_update_flag = log["facc"], True
        elif task.startswith("cfp"):
            log = validate_cfp(model, loader, tem)
        else:
            raise ValueError(f"Undefined task {task}")
        v.logs.update({f"val{setname}_{task}_{k}": x for k, x in log.items()})
    if max_metrix is not None:
        return max_metrix, max_update_flag
