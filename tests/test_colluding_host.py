"""CPU: the colluding attacks' host side — ALIE's z, the reference restatement
of flr_collude_rows' arithmetic (tests/colluding_ref.py) against float64, what
the attack does to Krum on the oracle, and the engine's attack-name check."""
import pytest
import torch

from colluding_ref import ALIE, IPM, collude
from flr.attacks import alie_z
from flr.models.multimodal import TINY
from flr.round import RoundConfig, RoundEngine
from oracle import aggregation as orc


@pytest.mark.parametrize("n,f,z", [(50, 12, 0.582842), (128, 25, 0.488776), (16, 3, 0.318639)])
def test_alie_z_values(n, f, z):
    assert abs(alie_z(n, f) - z) <= 1e-6


@pytest.mark.parametrize("n,f", [(16, 0), (16, 9), (50, 26), (128, 65), (5, 3)])
def test_alie_z_rejects(n, f):
    """f = 0, and f > n // 2 (no benign client left to outvote)."""
    with pytest.raises(ValueError):
        alie_z(n, f)


@pytest.mark.parametrize("K,nmal,P", [(4, 1, 257), (16, 3, 1000), (40, 8, 999), (130, 1, 513), (130, 25, 300)])
def test_reference_against_float64(K, nmal, P):
    """mu and sigma within 1e-6 of the float64 mean / std(unbiased=False),
    relative to the column maximum (sequential fp32 sums of up to 129 terms:
    1e-7 to 3e-7 measured)."""
    torch.manual_seed(K * 1000 + P)
    X = torch.randn(P) * 3 + 0.2 * torch.randn(K, P)
    _, mu, sigma = collude(X, nmal, ALIE, 0.5)
    B = X[nmal:].double()
    mu64, sd64 = B.mean(dim=0), B.std(dim=0, unbiased=False)
    emu = ((mu.double() - mu64).abs() / B.abs().max(dim=0).values).max().item()
    esd = ((sigma.double() - sd64).abs() / B.abs().max(dim=0).values).max().item()
    print(f"K={K} nmal={nmal} P={P}: mu err {emu:.2e}, sigma err {esd:.2e}")
    assert emu <= 1e-6 and esd <= 1e-6


def test_reference_sqrt_is_correctly_rounded():
    """The reference's square root against numpy's (the hardware's IEEE sqrt)
    on the magnitudes sigma^2 takes here, bit for bit: torch.sqrt on float32
    itself is the vector library's on some builds and misses this."""
    import numpy as np
    from colluding_ref import sqrt_rn
    torch.manual_seed(7)
    v = torch.cat([torch.rand(60000) * 0.004 + 0.0005, torch.rand(20000) * 1e-30, torch.rand(20000) * 1e30,
                   torch.tensor([0.0, 1.0, 4.0, float("inf")])])
    assert np.array_equal(sqrt_rn(v).numpy().view(np.int32), np.sqrt(v.numpy()).view(np.int32))
    assert torch.isnan(sqrt_rn(torch.tensor([float("nan"), -1.0]))).all()


def test_reference_outputs():
    torch.manual_seed(5)
    X = torch.randn(9, 300)
    out, mu, sigma = collude(X, 2, ALIE, 0.75)
    assert torch.equal(out[2:], X[2:])
    assert torch.equal(out[0], mu - torch.tensor(0.75) * sigma) and torch.equal(out[1], out[0])
    out, mu2, _ = collude(X, 2, IPM, 0.5)
    assert torch.equal(mu2, mu) and torch.equal(out[0], -(torch.tensor(0.5) * mu)) and torch.equal(out[1], out[0])
    assert torch.equal(out[2:], X[2:])


def test_constant_column_has_zero_sigma():
    """Equal benign values: the sequential sum of n copies of c divided by n is
    c wherever the partial sums are exact (small integers, powers of two times
    them), so every deviation is 0, sigma == 0 and ALIE submits mu itself."""
    torch.manual_seed(6)
    X = torch.randn(12, 64)
    X[:, 10] = 3.0
    X[3:, 20] = -0.375   # attackers' own entries do not count
    X[:, 30] = 0.0
    out, mu, sigma = collude(X, 3, ALIE, 0.9)
    for c in (10, 20, 30):
        assert sigma[c].item() == 0.0
        assert out[0, c].item() == mu[c].item() == X[3, c].item()
    assert (sigma[[0, 1, 2, 40]] > 0).all()


@pytest.mark.parametrize("seed", range(5))
def test_alie_evades_krum_where_sign_flip_does_not(seed):
    """K = 16, f = 3, P = 5000 on the oracle's Krum: it rejects the sign flip
    (selects a benign client) and selects an ALIE attacker."""
    K, f, P = 16, 3, 5000
    torch.manual_seed(seed)
    base = torch.randn(P)
    X = base + 0.05 * torch.randn(K, P)
    flipped = X.clone()
    flipped[:f] = -flipped[:f]
    _, _, sel, _, _ = orc.krum([[r] for r in flipped], f, 1)
    assert sel[0] >= f
    attacked, _, _ = collude(X, f, ALIE, alie_z(K, f))
    _, _, sel, _, _ = orc.krum([[r] for r in attacked], f, 1)
    assert sel[0] < f


def test_unknown_attack_name_is_loud():
    """A typo in RoundConfig.attack raises before anything is allocated — it
    used to run as an unattacked round."""
    with pytest.raises(ValueError, match="unknown attack 'nope'"):
        RoundEngine(TINY, RoundConfig(num_clients=8, num_attackers=1, attack="nope"), device="cpu")
