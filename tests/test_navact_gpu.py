"""magic_nav_act (csrc/loss.hip nav_act_kernel) through host/ops.nav_act against the float64 reference tests/_navact_ref64.py: stop probability and
entropy within the fp64 bound, actions exact on constructed draws (tests/_navact_cases.py builds them and the rows: every K at which the
kernel's walk changes -- below, at and above a lane's 8 columns, a 64-lane row of lanes, a 512-column chunk, several chunks)."""
import numpy as np
import pytest
import torch

import magic_amd  # noqa: F401
from magic_amd.host import lib as L
from magic_amd.host import ops as O
from tests import _navact_cases as C

pytestmark = pytest.mark.gpu

KS = [1, 2, 7, 63, 64, 65, 511, 512, 513, 1100]
BS = [1, 5, 33]


def gpu_impl(x_full, cand_full, K, modes, draws, ratio, twice=False):
    dev = torch.device("cuda")
    n, B = modes.shape
    x = torch.from_numpy(x_full).to(dev)
    cand = None if cand_full is None else torch.from_numpy(cand_full).to(dev)
    md, dr = torch.from_numpy(modes).to(dev), torch.from_numpy(draws).to(dev)
    act = torch.full((n, B), -7, dtype=torch.int32, device=dev)
    stop, ent = (torch.full((n, B), float("nan"), dtype=torch.float32, device=dev) for _ in range(2))
    for j in range(n):
        O.nav_act(x[:, :K], None if cand is None else cand[:, :K], md[j], dr[j], ratio, act[j], stop[j], ent[j])
    if twice:
        return act, stop, ent
    assert (stop == stop[0]).all() and (ent == ent[0]).all()          # the same row gives the same bits whatever the draws
    return act.cpu().numpy(), stop[0].cpu(), ent[0].cpu()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", BS)
def test_nav_act_against_fp64(B, K):
    C.verify(gpu_impl, B, K)


@pytest.mark.parametrize("B, K", [(5, 7), (33, 513), (5, 1100)])
def test_two_launches_are_bit_identical(B, K):
    x_full, cand_full = C.make_rows(B, K)
    _, groups = C.build(x_full, cand_full, K)
    for gp in groups[:2] + groups[-2:-1]:
        m, d = gp["modes"][:64], gp["draws"][:64]
        a = gpu_impl(x_full, cand_full, K, m, d, gp["ratio"], twice=True)
        b = gpu_impl(x_full, cand_full, K, m, d, gp["ratio"], twice=True)
        for u, v in zip(a, b):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_no_nan_leaves_the_kernel_and_padding_is_never_read():
    """the padding columns hold NaN (logits) and set bytes (candidates): a second run with other padding gives the same bits"""
    B, K = 5, 65
    x_full, cand_full = C.make_rows(B, K)
    _, groups = C.build(x_full, cand_full, K)
    gp = groups[1]
    a = gpu_impl(x_full, cand_full, K, gp["modes"], gp["draws"], gp["ratio"], twice=True)
    x2, c2 = x_full.copy(), cand_full.copy()
    x2[:, K:] = 1e30
    c2[:, K:] = False
    b = gpu_impl(x2, c2, K, gp["modes"], gp["draws"], gp["ratio"], twice=True)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    assert torch.isfinite(a[1]).all() and torch.isfinite(a[2]).all()


def test_bad_arguments_are_refused_without_a_launch():
    dev = torch.device("cuda")
    B, K = 3, 9
    x = torch.zeros(B, K, device=dev)
    cand = torch.ones(B, K, dtype=torch.uint8, device=dev)
    mode = torch.full((B,), 1, dtype=torch.uint8, device=dev)
    act = torch.full((B,), -7, dtype=torch.int32, device=dev)
    stop, ent = torch.full((B,), -7.0, device=dev), torch.full((B,), -7.0, device=dev)
    P = L.P

    def raw(B_, K_, ld, cand_, ldc):
        L.call("magic_nav_act", B_, K_, P(x), ld, P(cand_), ldc, P(mode), None, 0.6, P(act), P(stop), P(ent), L.stream())

    for args in ((0, K, K, cand, K), (B, 0, K, cand, K), (B, K, K - 1, cand, K), (B, K, K, cand, K - 1), (-1, K, K, None, 0)):
        with pytest.raises(L.MagicHipError):
            raw(*args)
    with pytest.raises(L.MagicHipError):
        L.call("magic_nav_act", B, K, None, K, None, 0, P(mode), None, 0.6, P(act), P(stop), P(ent), L.stream())
    for bad in (dict(logits=x.double()), dict(mode=mode.int()), dict(action=act.long()), dict(draws=torch.zeros(B, 3, device=dev)),
                dict(cand=cand.float()), dict(entropy=ent.double())):
        kw = dict(logits=x, cand=cand, mode=mode, draws=None, expl_max_ratio=0.6, action=act, stop_prob=stop, entropy=ent)
        kw.update(bad)
        with pytest.raises(L.MagicHipError, match="shape check"):
            O.nav_act(**kw)
    torch.cuda.synchronize()
    assert (act == -7).all() and (stop == -7).all() and (ent == -7).all()
    raw(B, K, K, None, K - 1)                                # ldc is not looked at without candidate bytes
    torch.cuda.synchronize()
    assert (act == 0).all() and torch.allclose(stop, torch.full_like(stop, 1.0 / K))
    assert np.allclose(ent.cpu().numpy(), np.log(K), rtol=1e-6)
