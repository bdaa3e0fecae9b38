"""CPU: model replacement's host side — the closed-form strengths of
include/flr.h (tests/replace_ref.py) against a direct evaluation of their
constraints, the degenerate cases, and the configuration checks of the engine
and of flr.attacks.model_replacement_."""
import functools

import numpy as np
import pytest
import torch

import replace_ref as ref
from replace_ref import DISTANCE, MAX, MEAN, MEDIAN, NONE, NORM
from flr.attacks import model_replacement_
from flr.models.multimodal import TINY
from flr.round import ATTACKS, RoundConfig, RoundEngine

SHAPES = [(4, 1, 9), (7, 3, 19), (12, 4, 67), (33, 12, 130), (65, 30, 64)]
SEEDS = range(20)
AMPS = [0.3, 1.0]


@functools.lru_cache(maxsize=None)
def _case(K, f, P, seed, amp):
    X, g = ref.updates(K, f, P, seed, amp)
    norms, G = ref.norms_gram(X, g)
    return X, g, ref.centered(X, g), norms, G


@pytest.mark.parametrize("amp", AMPS)
def test_distance_strength_meets_its_constraint(amp):
    """Every attacker the reference does not mark infeasible (status 2): the
    row at gamma_i is within rho * the benign diameter of every benign row
    (1e-9 relative, both sides evaluated directly in float64), and a
    bound-limited one (status 1) breaks the bound at gamma_i * (1 + 1e-6).  At
    most 5 % of the attackers are infeasible."""
    total = left_out = 0
    for K, f, P in SHAPES:
        for seed in SEEDS:
            _, _, U, norms, G = _case(K, f, P, seed, amp)
            boost = K / f
            gamma, status, flags = ref.strength(norms, G, K, f, boost, DISTANCE)
            assert flags == 0 and (gamma >= 0.0).all() and (gamma <= boost).all()
            b2 = ref.diameter2(U, f)
            for i in range(f):
                total += 1
                if status[i] == 2:
                    left_out += 1
                    continue
                assert status[i] in (0, 1) and (status[i] == 0) == (gamma[i] == boost)
                assert ref.worst_distance2(U, f, i, gamma[i]) <= b2 * (1.0 + 1e-9), (K, f, P, seed, i)
                if status[i] == 1:
                    assert ref.worst_distance2(U, f, i, gamma[i] * (1.0 + 1e-6)) > b2, (K, f, P, seed, i)
    share = left_out / total
    print(f"amp {amp}: {left_out} of {total} attackers infeasible ({100 * share:.2f} %)")
    assert total == 1000 and share <= 0.05


@pytest.mark.parametrize("stat", [MEDIAN, MAX, MEAN], ids=["median", "max", "mean"])
@pytest.mark.parametrize("amp", AMPS)
def test_norm_strength_meets_its_bound(amp, stat):
    """rho = 1: ||gamma_i u_i|| <= bound * (1 + 2^-40); gamma_i == boost exactly
    when boost * e_i <= bound; the median is numpy's."""
    for K, f, P in SHAPES:
        for seed in SEEDS:
            _, _, _, norms, G = _case(K, f, P, seed, amp)
            boost = K / f
            gamma, status, flags = ref.strength(norms, None, K, f, boost, NORM, stat)
            bound = {MEDIAN: np.median, MAX: np.max, MEAN: np.mean}[stat](norms[f:])
            if stat == MEAN:
                assert abs(ref.statistic(norms[f:], stat) - bound) <= 1e-12 * bound
                bound = ref.statistic(norms[f:], stat)
            else:
                assert ref.statistic(norms[f:], stat) == bound
            assert flags == 0
            for i in range(f):
                assert gamma[i] * norms[i] <= bound * (1.0 + 2.0 ** -40)
                assert (gamma[i] == boost) == (boost * norms[i] <= bound)
                assert status[i] == (0 if gamma[i] == boost else 1)


def test_none_mode_is_the_boost():
    gamma, status, flags = ref.strength(None, None, 8, 3, 2.5, NONE)
    assert (gamma == 2.5).all() and (status == 0).all() and flags == 0


def test_degenerate_cases():
    """A zero attacker row gives boost; a NaN in a benign row gives every gamma
    1 and bit 0 of flags; a NaN attacker gets status 3; boost = 1 keeps the
    rows' bits."""
    K, f, P = 7, 3, 19
    X, g = ref.updates(K, f, P, 0)
    for mode in (NORM, DISTANCE):
        Z = X.clone()
        Z[1] = g
        norms, G = ref.norms_gram(Z, g)
        gamma, status, flags = ref.strength(norms, G, K, f, 4.0, mode)
        assert gamma[1] == 4.0 and status[1] == 0 and flags == 0

        Z = X.clone()
        Z[5, 3] = float("nan")
        norms, G = ref.norms_gram(Z, g)
        gamma, status, flags = ref.strength(norms, G, K, f, 4.0, mode)
        assert (gamma == 1.0).all() and (status == 3).all() and flags == 1

        Z = X.clone()
        Z[0, 2] = float("nan")
        norms, G = ref.norms_gram(Z, g)
        gamma, status, flags = ref.strength(norms, G, K, f, 4.0, mode)
        assert gamma[0] == 1.0 and status[0] == 3 and flags == 2 and (status[1:] != 3).all()
        out = ref.scale(Z, g, gamma.astype(np.float32))
        assert torch.equal(out[0].view(torch.int32), Z[0].view(torch.int32))   # the NaN row's bits kept

    norms, G = ref.norms_gram(X, g)
    gamma, status, flags = ref.strength(norms, G, K, f, 1.0, NONE)
    out = ref.scale(X, g, gamma.astype(np.float32))
    assert torch.equal(out.view(torch.int32), X.view(torch.int32))
    out = ref.scale(X, g, np.array([2.0, 1.0, float("nan")], dtype=np.float32))
    assert not torch.equal(out[0], X[0]) and torch.equal(out[1:], X[1:])


def test_engine_configuration_checks():
    """The name is an attack; bad attack_cfg values, f outside [1, K), too few
    benign rows for the distance bound and whole-row modes on the all-to-all
    exchange at world > 1 are refused before anything is allocated."""
    assert "model_replacement" in ATTACKS

    def engine(cfg, K=8, f=2, **kw):
        rkw = {k: kw.pop(k) for k in ("exchange", "defense") if k in kw}
        return RoundEngine(TINY, RoundConfig(num_clients=K, num_attackers=f, attack="model_replacement",
                                             attack_cfg=cfg, **rkw), device="cpu", **kw)

    with pytest.raises(ValueError, match="stealth"):
        engine({"stealth": "krum"})
    with pytest.raises(ValueError, match="stat"):
        engine({"stealth": "norm", "stat": "mode"})
    for key in ("boost", "rho"):
        for bad in (0, 0.0, -1.0, float("nan"), float("inf"), True, "2"):
            with pytest.raises(ValueError, match=key):
                engine({key: bad})
    for f in (0, 8, 9):
        with pytest.raises(ValueError, match="1 <= f < K"):
            engine({}, f=f)
    with pytest.raises(ValueError, match="two benign rows"):
        engine({"stealth": "distance"}, f=7)
    for stealth in ("norm", "distance"):
        with pytest.raises(ValueError, match="whole client rows"):
            engine({"stealth": stealth}, exchange="alltoall", defense="median", rank=0, world=2)


def test_attack_function_validates():
    """All before any device work: a CPU matrix gets as far as the checks."""
    X, g = torch.zeros(4, 8), torch.zeros(8)
    for f in (0, 4, -1):
        with pytest.raises(ValueError, match="1 <= f < K"):
            model_replacement_(X, f, g)
    with pytest.raises(ValueError, match="unknown stealth"):
        model_replacement_(X, 1, g, stealth="krum")
    with pytest.raises(ValueError, match="unknown stat"):
        model_replacement_(X, 1, g, stealth="norm", stat="mode")
    for bad in (0, -2.0, float("nan"), float("inf"), True, "3"):
        with pytest.raises(ValueError, match="boost"):
            model_replacement_(X, 1, g, boost=bad)
        with pytest.raises(ValueError, match="rho"):
            model_replacement_(X, 1, g, stealth="norm", rho=bad)
    with pytest.raises(ValueError, match="two benign rows"):
        model_replacement_(X, 3, g, stealth="distance")
