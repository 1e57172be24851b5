"""The launch layer's queue helpers and the two-site dropout packer of host/ops.py, on CPU tensors: nothing here launches."""
import itertools
import random

import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import ops as O


@pytest.fixture
def queues():
    """the module's queue state as this test found it, put back afterwards"""
    saved = (O.DEFER["queue"], list(O.DEFER["queue"]), O.DEFER["active"], O.DEFER["bytes"], list(O.PART_JOBS), list(O.RBW_JOBS), dict(O._SPREL))
    yield
    O.DEFER["queue"], O.DEFER["active"], O.DEFER["bytes"] = saved[0], saved[2], saved[3]
    O.DEFER["queue"][:] = saved[1]
    O.PART_JOBS[:], O.RBW_JOBS[:] = saved[4], saved[5]
    O._SPREL.clear()
    O._SPREL.update(saved[6])


def _jobs(n_dst=160, repeated=((3, 3), (7, 3), (17, 5), (40, 4), (64, 5), (99, 3), (119, 5), (130, 4), (150, 4), (151, 3), (152, 5), (159, 4)), seed=0, numel=8):
    """about 200 column-sum jobs (partial, destination, blocks) over n_dst distinct destinations, some queued several times, in a shuffled order;
    the third field numbers the jobs"""
    dsts = [torch.zeros(numel) for _ in range(n_dst)]
    times = {i: 1 for i in range(n_dst)}
    times.update(dict(repeated))
    order = [i for i, k in times.items() for _ in range(k)]
    random.Random(seed).shuffle(order)
    return dsts, [(torch.zeros(1), dsts[i], j) for j, i in enumerate(order)]


def test_take_once_chunks_a_queue():
    dsts, jobs = _jobs()
    assert len(jobs) == 196 and len(dsts) > 96
    rest, chunks = list(jobs), []
    while rest:
        n = len(rest)
        chunk, rest = O._take_once(rest)
        assert 1 <= len(chunk) <= 96 and len(chunk) + len(rest) == n
        ptrs = [j[1].data_ptr() for j in chunk]
        assert len(set(ptrs)) == len(ptrs)                               # no destination twice in one launch
        assert [j[2] for j in rest] == sorted(j[2] for j in rest)        # what is left keeps the queue order
        chunks.append(chunk)
    out = [j for c in chunks for j in c]
    assert sorted(j[2] for j in out) == list(range(len(jobs)))           # every job exactly once
    assert all(a is b for a, b in zip(sorted(out, key=lambda j: j[2]), jobs))
    for d in dsts:                                                       # the jobs of one destination leave in the order they were queued
        mine = [j[2] for j in out if j[1] is d]
        assert mine == sorted(mine)
    assert len(chunks) >= 5                                              # a destination queued 5 times needs 5 launches
    # the first chunk is the first 96 distinct destinations of the queue, in order
    first, seen = [], set()
    for j in jobs:
        if len(first) < 96 and j[1].data_ptr() not in seen:
            seen.add(j[1].data_ptr())
            first.append(j)
    assert all(a is b for a, b in zip(chunks[0], first)) and len(chunks[0]) == len(first)
    chunk, rest = O._take_once(jobs, limit=7)
    assert len(chunk) == 7 and len(rest) == len(jobs) - 7
    assert O._take_once([]) == ([], [])


def test_take_once_predicate_and_ride_along_rule():
    H = 8
    ride = lambda q: O._take_once(q, ok=lambda job: job[1].numel() == H)
    dsts, jobs = _jobs(n_dst=40, repeated=())
    take, keep = ride(jobs)                                              # 40 vectors of H, each once: all of them ride
    assert keep == [] and all(a is b for a, b in zip(take, jobs)) and len(take) == 40
    wide = (torch.zeros(1), torch.zeros(2 * H), 0)
    take, keep = ride(jobs[:10] + [wide] + jobs[10:])                    # a vector of another width is refused by the predicate
    assert keep == [wide] and len(take) == 40
    take, keep = ride(jobs + [jobs[3]])                                  # a destination queued twice: its second job is left over
    assert len(keep) == 1 and keep[0] is jobs[3] and len(take) == 40
    dsts, many = _jobs(n_dst=100, repeated=())
    take, keep = ride(many)                                              # more than one launch holds
    assert len(take) == 96 and all(a is b for a, b in zip(keep, many[96:])) and len(keep) == 4
    # the ride-along selection of embed_in_bwd is all or nothing: anything left over means nothing rides and the queue stays as it is
    for q, rides in ((jobs, True), (jobs[:10] + [wide] + jobs[10:], False), (jobs + [jobs[3]], False), (many, False)):
        take, keep = ride(q)
        assert (not keep) == rides


def test_deferred_isolated_restores_after_an_exception(queues):
    outer_q = O.DEFER["queue"]
    a, b, c = torch.zeros(4), torch.zeros(4), torch.zeros(2)
    outer_q[:] = [("dw-entry",)]
    O.DEFER["active"], O.DEFER["bytes"] = True, 1234
    O.PART_JOBS[:] = [(torch.zeros(4), a, 1, 4, 4)]
    O.RBW_JOBS[:] = [(torch.zeros(4), b, 1)]
    O._SPREL.clear()
    sprel_entry = [torch.zeros(16, 2), 3, 0, None]
    O._SPREL[c.data_ptr()] = sprel_entry
    part_obj, rbw_obj, sprel_obj = O.PART_JOBS, O.RBW_JOBS, O._SPREL
    part0, rbw0 = list(O.PART_JOBS), list(O.RBW_JOBS)
    inner = []
    with pytest.raises(RuntimeError, match="half-way"):
        with O.deferred_isolated():
            assert O.DEFER["queue"] == [] and O.DEFER["queue"] is not outer_q and O.DEFER["bytes"] == 0
            assert O.PART_JOBS == [] and O.RBW_JOBS == [] and O._SPREL == {}
            assert O.PART_JOBS is part_obj and O.RBW_JOBS is rbw_obj and O._SPREL is sprel_obj
            assert O.DEFER["active"] is True                             # (whether the surrounding pass defers is not changed on entry)
            inner.append(O.DEFER["queue"])
            O.DEFER["queue"].append(("inner",))
            O.DEFER["bytes"] = 99
            O.DEFER["active"] = False
            O.PART_JOBS.append((torch.zeros(4), b, 1, 4, 4))
            O.RBW_JOBS.append((torch.zeros(4), a, 1))
            O._SPREL[a.data_ptr()] = [torch.zeros(16, 2), 1, 0, None]
            raise RuntimeError("raised half-way")
    assert O.DEFER["queue"] is outer_q and outer_q == [("dw-entry",)]
    assert O.DEFER["active"] is True and O.DEFER["bytes"] == 1234
    assert O.PART_JOBS is part_obj and O.RBW_JOBS is rbw_obj and O._SPREL is sprel_obj
    assert len(O.PART_JOBS) == 1 and O.PART_JOBS[0] is part0[0] and len(O.RBW_JOBS) == 1 and O.RBW_JOBS[0] is rbw0[0]
    assert list(O._SPREL) == [c.data_ptr()] and O._SPREL[c.data_ptr()] is sprel_entry
    assert inner[0] == [("inner",)]                                      # the inner list belongs to whoever kept it (step_graphs._CatEntry)
    with O.deferred_isolated():                                          # and without an exception
        O.RBW_JOBS.append((torch.zeros(4), a, 1))
    assert len(O.RBW_JOBS) == 1 and O.RBW_JOBS[0] is rbw0[0] and O.DEFER["queue"] is outer_q


@pytest.mark.parametrize("active", [False, True])
def test_deferred_clear_empties_every_queue(queues, active):
    q = O.DEFER["queue"]
    q[:] = [("dw-entry",)]
    O.DEFER["active"], O.DEFER["bytes"] = active, 77
    O.PART_JOBS[:] = [(torch.zeros(4), torch.zeros(4), 1, 4, 4)]
    O.RBW_JOBS[:] = [(torch.zeros(4), torch.zeros(4), 1)]
    O._SPREL[5] = [torch.zeros(16, 2), 1, 0, None]
    part_obj, rbw_obj, sprel_obj = O.PART_JOBS, O.RBW_JOBS, O._SPREL
    O.deferred_clear()
    assert O.DEFER["queue"] is q and q == [] and O.DEFER["bytes"] == 0 and O.DEFER["active"] is active
    assert O.PART_JOBS is part_obj and O.RBW_JOBS is rbw_obj and O._SPREL is sprel_obj
    assert O.PART_JOBS == [] and O.RBW_JOBS == [] and O._SPREL == {}
    assert "bytes" in O.DEFER and isinstance(O.DEFER, dict) and isinstance(O.PART_JOBS, list) and isinstance(O.RBW_JOBS, list) and isinstance(O._SPREL, dict)


# the four expressions _drop2 replaced, copied as they stood in ln_fwd, ln_bwd and the text halves of embed_in_fwd / embed_in_bwd
def _old_ln_fwd(drop_in0, drop_out):
    d = drop_in0 if (drop_in0 is not None and drop_in0[1] > 0) else drop_out
    seed, p, _ = O._dr(d)
    s_in = int(drop_in0[2]) if (p > 0 and drop_in0 is not None) else 0
    s_out = int(drop_out[2]) if (p > 0 and drop_out is not None) else 0
    return seed, p, s_in, s_out


def _old_ln_bwd(drop_dy, drop_dx):
    dd = drop_dy if (drop_dy is not None and drop_dy[1] > 0) else drop_dx
    seed, p, _ = O._dr(dd)
    s_dy = int(drop_dy[2]) if (p > 0 and drop_dy is not None) else 0
    s_dx = int(drop_dx[2]) if (p > 0 and drop_dx is not None) else 0
    return seed, p, s_dy, s_dx


def _old_embed_in_fwd(text):
    d_in, d_out = text.get("drop_in0"), text.get("drop_out")
    d = d_in if (d_in is not None and d_in[1] > 0) else d_out
    seed, p_, _ = O._dr(d)
    site_in0 = int(d_in[2]) if (p_ > 0 and d_in is not None) else 0
    site_out = int(d_out[2]) if (p_ > 0 and d_out is not None) else 0
    return seed, float(p_), site_in0, site_out


def _old_embed_in_bwd(text):
    d_dy, d_dx = text.get("drop_dy"), text.get("drop_dx")
    dd = d_dy if (d_dy is not None and d_dy[1] > 0) else d_dx
    seed, p_, _ = O._dr(dd)
    site_dy = int(d_dy[2]) if (p_ > 0 and d_dy is not None) else 0
    site_dx = int(d_dx[2]) if (p_ > 0 and d_dx is not None) else 0
    return seed, float(p_), site_dy, site_dx


def test_drop2_is_the_four_expressions_it_replaced():
    seed_a, seed_b = torch.zeros(2, dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    forms_a = (None, (seed_a, 0.0, 11), (seed_a, 0.1, 11))
    forms_b = (None, (seed_b, 0.0, 22), (seed_b, 0.25, 22))
    for a, b in itertools.product(forms_a, forms_b):
        got = O._drop2(a, b)
        assert got == _old_ln_fwd(a, b) == _old_ln_bwd(a, b), (a, b)
        assert got == _old_embed_in_fwd(dict(drop_in0=a, drop_out=b)) == _old_embed_in_bwd(dict(drop_dy=a, drop_dx=b)), (a, b)
        assert type(got[1]) is float and type(got[2]) is int and type(got[3]) is int
    # spelled out: nothing drops -> no seed, no sites; a drops -> a's seed and rate, both given sites; only b drops -> b's seed and rate and STILL a's site
    assert O._drop2(None, None) == (None, 0.0, 0, 0)
    assert O._drop2(forms_a[1], forms_b[1]) == (None, 0.0, 0, 0)
    assert O._drop2(forms_a[2], None) == (seed_a.data_ptr(), 0.1, 11, 0)
    assert O._drop2(forms_a[2], forms_b[2]) == (seed_a.data_ptr(), 0.1, 11, 22)
    assert O._drop2(None, forms_b[2]) == (seed_b.data_ptr(), 0.25, 0, 22)
    assert O._drop2(forms_a[1], forms_b[2]) == (seed_b.data_ptr(), 0.25, 11, 22)
