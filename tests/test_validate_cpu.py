"""Host side of the validation pass that needs no GPU (host/validate.py): the driver's val_log assembled from a hand-written accumulator
block -- key names, the divisions, the empty-loader error (pretrain_src/train_r2r_magic.py:456-464, :489-497, :521-532) -- and merge_block
over gloo with 2 ranks (the driver's three all_gathers as one all-reduce)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import magic_amd  # noqa: F401
from magic_amd.host import validate as V


def block(loss, hits, rows):
    """the 96-byte block as the device lays it out: double loss[4]; long long hits[4]; long long rows[4]"""
    b = torch.zeros(12, dtype=torch.int64)
    b[:4] = torch.tensor(loss, dtype=torch.float64).view(torch.int64)
    b[4:8] = torch.tensor(hits)
    b[8:] = torch.tensor(rows)
    return b


def test_val_log_keys_and_divisions():
    b = block([10.5, 3.25, 7.0, 0.0], [30, 12, 21, 0], [40, 40, 40, 0])
    assert V.read_block(b) == dict(loss=[10.5, 3.25, 7.0, 0.0], hits=[30, 12, 21, 0], rows=[40, 40, 40, 0])
    assert V.val_log("mlm", b, 2.0) == {"loss": 10.5 / 40, "acc": 30 / 40, "tok_per_s": 20.0}
    assert list(V.val_log("mlm", b, 2.0)) == ["loss", "acc", "tok_per_s"]
    assert V.val_log("mrc", b, 4.0) == {"loss": 10.5 / 40, "acc": 0.75, "feat_per_s": 10.0}
    for task in ("sap", "cfp", "sap_r2r"):
        log = V.val_log(task, b, 0.5)
        assert list(log) == ["gloss", "lloss", "floss", "gacc", "lacc", "facc", "tok_per_s"]
        assert log == {"gloss": 10.5 / 40, "lloss": 3.25 / 40, "floss": 7.0 / 40, "gacc": 30 / 40, "lacc": 12 / 40, "facc": 21 / 40, "tok_per_s": 80.0}
    with pytest.raises(ValueError, match="Undefined task"):
        V.val_log("itm", b, 1.0)


@pytest.mark.parametrize("task", ["mlm", "mrc", "sap", "cfp"])
def test_an_empty_loader_raises_as_the_drivers_arithmetic_does(task):
    with pytest.raises(ZeroDivisionError):
        V.val_log(task, block([0.0] * 4, [0] * 4, [0] * 4), 1.0)


def test_merge_block_without_a_process_group_is_the_block():
    b = block([1.0, 2.0, 3.0, 4.0], [1, 2, 3, 4], [5, 6, 7, 8])
    assert V.merge_block(b) is b


def test_the_package_exports_the_drivers_names():
    for name in ("Validator", "validate", "validate_mlm", "validate_mrc", "validate_sap", "validate_cfp", "merge_block"):
        assert getattr(magic_amd, name) is getattr(V, name)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_block(rank):
    return block([0.1 + rank, 2.5 * (rank + 1), 1e-3, 0.0], [3 + rank, 2 ** 40 + rank, 0, 0], [10 + rank, 2 ** 41, 7, 0])


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mine = _rank_block(rank)
        keep = mine.clone()
        merged = V.merge_block(mine)
        q.put((rank, V.read_block(merged), bool(torch.equal(mine, keep)), V.val_log("sap", merged, 1.0)))
    finally:
        dist.destroy_process_group()


def test_merge_block_sums_over_two_gloo_ranks():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=100) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    a, b = V.read_block(_rank_block(0)), V.read_block(_rank_block(1))
    want = {k: [x + y for x, y in zip(a[k], b[k])] for k in a}
    for rank, got, untouched, log in res:
        assert got == want, rank                      # doubles summed once, counts exact (also past 2^32)
        assert untouched, "the rank's own block is left as it was"
        assert log["gacc"] == want["hits"][0] / want["rows"][0] and log["lloss"] == want["loss"][1] / want["rows"][0]
