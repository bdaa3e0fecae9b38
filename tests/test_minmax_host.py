"""CPU: the Min-Max / Min-Sum attacks' host side — the closed-form gamma of
include/flr.h (tests/minmax_ref.py) against its own constraint and against the
paper's halving search, its degenerate cases, what the attack does to Krum on
the oracle, and the engine's configuration checks."""
import functools
import math

import numpy as np
import pytest
import torch

import minmax_ref as ref
from minmax_ref import MAX, SIGN, STD, SUM, UNIT
from flr.models.multimodal import TINY
from flr.round import ATTACKS, RoundConfig, RoundEngine
from oracle import aggregation as orc

SHAPES = [(3, 1, 5), (8, 2, 300), (16, 3, 5000), (40, 9, 777)]
TAU = 1e-5  # the halving search's threshold


@functools.lru_cache(maxsize=None)
def _case(K, nmal, P):
    """(X, g): clients 0.05 around a base, the global model 0.1 away from it."""
    torch.manual_seed(100 * K + P)
    base = torch.randn(P)
    return base + 0.05 * torch.randn(K, P), base + 0.1 * torch.randn(P)


@functools.lru_cache(maxsize=None)
def _solved(K, nmal, P, objective, perturb):
    X, g = _case(K, nmal, P)
    mu, sigma = ref.mean_std(X, nmal)
    p = ref.perturbation(mu, sigma, g, perturb)
    _, gamma, stats = ref.attack(X, nmal, objective, perturb, g)
    return X, mu, p, gamma, stats


@pytest.mark.parametrize("perturb", [STD, SIGN, UNIT], ids=["std", "sign", "unit"])
@pytest.mark.parametrize("objective", [MAX, SUM], ids=["max", "sum"])
@pytest.mark.parametrize("K,nmal,P", SHAPES)
def test_closed_form_meets_its_constraint(K, nmal, P, objective, perturb):
    """gamma >= 0; a_i <= R2; the constraint holds, with equality at the tight
    row (Min-Max) or on the sum (Min-Sum), to 1e-9 relative in float64."""
    _, _, _, gamma, (a, b, c, R2, S) = _solved(K, nmal, P, objective, perturb)
    nb = K - nmal
    assert gamma >= 0.0 and math.isfinite(gamma) and c > 0.0
    assert (a <= R2).all()
    if objective == MAX:
        q = a + 2.0 * gamma * b + gamma * gamma * c   # ||m - x_i||^2 per row
        assert abs(q.max() - R2) <= 1e-9 * R2
        assert (q <= R2 * (1.0 + 1e-9)).all()
    else:
        q = a.sum() + 2.0 * gamma * b.sum() + gamma * gamma * nb * c
        assert abs(q - S) <= 1e-9 * S


@pytest.mark.parametrize("perturb", [STD, SIGN, UNIT], ids=["std", "sign", "unit"])
@pytest.mark.parametrize("objective", [MAX, SUM], ids=["max", "sum"])
@pytest.mark.parametrize("K,nmal,P", SHAPES)
def test_halving_search_agrees(K, nmal, P, objective, perturb):
    """The paper's search, started at 1.25 x the closed form (its reach is
    gamma_init / 2 either way): its last probe is within its threshold of the
    closed form, its result (the largest satisfying probe) at most two
    thresholds below it and never above (minmax_ref.halving_search)."""
    X, mu, p, gamma, _ = _solved(K, nmal, P, objective, perturb)
    assert gamma > 8 * TAU   # else the search would stop before it started
    succ, last = ref.halving_search(X, nmal, objective, mu, p, 1.25 * gamma, TAU)
    print(f"closed {gamma:.9g} search {succ:.9g} last probe {last:.9g}")
    assert abs(last - gamma) <= TAU
    assert -1e-9 * gamma <= gamma - succ <= 2 * TAU


@pytest.mark.parametrize("objective", [MAX, SUM], ids=["max", "sum"])
def test_degenerate_cases_give_zero(objective):
    """nb = 1 (R2 = S = 0, every direction) and c = 0 (std with one benign row;
    sign / unit with g == mu): gamma = 0 and the attackers submit mu."""
    torch.manual_seed(9)
    X = torch.randn(3, 40)
    g = torch.randn(40)
    for perturb in (STD, SIGN, UNIT):
        out, gamma, (a, b, c, R2, S) = ref.attack(X, 2, objective, perturb, g)
        assert gamma == 0.0 and R2 == 0.0 and S == 0.0 and a[0] == 0.0 and (c == 0.0) == (perturb == STD)
        assert torch.equal(out[0], X[2]) and torch.equal(out[1], X[2])
    X = torch.randn(9, 40)
    mu, _ = ref.mean_std(X, 2)
    for perturb in (SIGN, UNIT):
        out, gamma, (a, b, c, R2, S) = ref.attack(X, 2, objective, perturb, mu.clone())
        assert c == 0.0 and gamma == 0.0 and R2 > 0.0
        assert torch.equal(out[0], mu) and torch.equal(out[1], mu) and torch.equal(out[2:], X[2:])


def test_nan_statistics_give_nan_and_leave_the_rows():
    a, b = np.array([1.0, 2.0]), np.array([0.1, -0.2])
    assert math.isnan(ref.gamma_closed(np.array([1.0, np.nan]), b, 3.0, 4.0, 5.0, MAX))
    assert math.isnan(ref.gamma_closed(a, b, np.nan, 4.0, 5.0, SUM))
    assert math.isnan(ref.gamma_closed(a, b, 3.0, np.nan, 5.0, MAX))
    assert math.isnan(ref.gamma_closed(a, b, 0.0, 4.0, np.nan, MAX))   # NaN before c == 0
    inf = float("inf")   # inf - inf in R2 - a_i: a NaN root, kept by the minimum
    assert math.isnan(ref.gamma_closed(np.array([inf, 1.0]), b, 3.0, inf, 5.0, MAX))
    torch.manual_seed(4)
    X = torch.randn(6, 30)
    X[3, 7] = float("nan")
    out, gamma, _ = ref.attack(X, 2, MAX, STD)
    assert math.isnan(gamma) and torch.equal(out[:2], X[:2])


def test_bounds_follow_numpy_nan_and_order():
    D = np.array([[0.0, 3.0, 1.0], [3.0, 0.0, 2.0], [1.0, 2.0, 0.0]])
    assert ref.bounds(D) == (9.0, 13.0)
    D[0, 2] = np.nan
    assert all(math.isnan(v) for v in ref.bounds(D))


@pytest.mark.parametrize("seed", range(5))
def test_min_max_evades_krum_where_sign_flip_does_not(seed):
    """K = 16, f = 3, P = 5000 on the oracle's Krum (f = nmal): it rejects the
    sign-flipped rows (selects a benign client) and selects a Min-Max attacker,
    in every direction."""
    K, f, P = 16, 3, 5000
    torch.manual_seed(seed)
    base = torch.randn(P)
    X = base + 0.05 * torch.randn(K, P)
    g = base + 0.1 * torch.randn(P)
    flipped = X.clone()
    flipped[:f] = -flipped[:f]
    _, _, sel, _, _ = orc.krum([[r] for r in flipped], f, 1)
    assert sel[0] >= f
    for perturb in (STD, SIGN, UNIT):
        attacked, gamma, _ = ref.attack(X, f, MAX, perturb, g)
        assert gamma > 0.0 and not torch.equal(attacked[:f], X[:f])
        _, _, sel, _, _ = orc.krum([[r] for r in attacked], f, 1)
        assert sel[0] < f


def test_engine_configuration_checks():
    """Both names are attacks; f outside [1, K), an unknown direction and the
    all-to-all exchange at world > 1 are refused before anything is allocated."""
    assert "min_max" in ATTACKS and "min_sum" in ATTACKS
    for attack in ("min_max", "min_sum"):
        for f in (0, 8, 9):
            with pytest.raises(ValueError, match="num_attackers"):
                RoundEngine(TINY, RoundConfig(num_clients=8, num_attackers=f, attack=attack), device="cpu")
        with pytest.raises(ValueError, match="perturb"):
            RoundEngine(TINY, RoundConfig(num_clients=8, num_attackers=2, attack=attack,
                                          attack_cfg={"perturb": "norm"}), device="cpu")
        with pytest.raises(ValueError, match="whole client rows"):
            RoundEngine(TINY, RoundConfig(num_clients=8, num_attackers=2, attack=attack, defense="median",
                                          exchange="alltoall"), device="cpu", rank=0, world=2)


def test_attack_functions_validate():
    from flr.attacks import min_max_, min_sum_
    X = torch.zeros(4, 8)
    for fn in (min_max_, min_sum_):
        for f in (0, 4, -1):
            with pytest.raises(ValueError):
                fn(X, f)
        with pytest.raises(ValueError, match="unknown perturbation"):
            fn(X, 1, perturb="norm")
        with pytest.raises(ValueError, match="global_flat"):
            fn(X, 1, perturb="sign")
