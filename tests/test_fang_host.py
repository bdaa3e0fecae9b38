"""CPU: Fang et al.'s attacks' host side — the closed-form Krum probe of
include/flr.h (tests/fang_ref.py) against a direct Krum of the attacked matrix,
the Philox4x32-10 known answers, the trimmed-mean attack's ranges, the workspace
functions, and the configuration checks of the engine and of flr.attacks."""
import functools

import numpy as np
import pytest
import torch

import fang_ref as ref
import replace_ref
from flr import _capi
from flr.attacks import fang_krum_, fang_trim_
from flr.models.multimodal import TINY
from flr.round import ATTACKS, RoundConfig, RoundEngine

SHAPES = [(5, 1, 9), (7, 2, 19), (12, 4, 67), (33, 12, 130), (65, 30, 64), (64, 25, 257), (130, 26, 333)]
SEEDS = range(20)


@functools.lru_cache(maxsize=None)
def _case(K, f, P, seed):
    """The benign-only generator (amp = 0: the attackers' rows are overwritten
    anyway), the accurate statistics and the reference's solution."""
    X, g = replace_ref.updates(K, f, P, seed, amp=0)
    G, b, c = ref.statistics(X, g, f)
    return X, g, G, b, c, ref.strength(G, b, c, K, f)


def test_closed_form_agrees_with_a_direct_krum():
    """All 140 cases: the reference ends with status 0 exactly when a direct
    Krum of the matrix rebuilt with the float32 rows g - lambda32 * s picks an
    attacker's row; status 1 otherwise (no case is degenerate)."""
    total = 0
    for K, f, P in SHAPES:
        for seed in SEEDS:
            X, g, _, _, _, (lam, status, t, _) = _case(K, f, P, seed)
            assert status in (0, 1) and lam > 0.0, (K, f, P, seed, status)
            Y = ref.krum_rows(X, g, f, np.float32(lam))
            assert not torch.equal(Y[:f], X[:f]) and torch.equal(Y[f:], X[f:])
            pick = ref.krum_pick(Y, f)
            assert (pick < f) == (status == 0), (K, f, P, seed, pick, status, t)
            total += 1
    assert total == 140


def test_the_search_succeeds_with_two_attackers_or_more():
    """f >= 2: at most 5 % of the 120 cases reach the threshold (status 1)."""
    cases = [(K, f, P, seed) for K, f, P in SHAPES if f >= 2 for seed in SEEDS]
    failed = sum(_case(*cs)[5][1] == 1 for cs in cases)
    halvings = sorted({_case(*cs)[5][2] for cs in cases})
    print(f"{failed} of {len(cases)} searches reached the threshold; halvings {halvings}")
    assert len(cases) == 120 and failed <= 0.05 * len(cases)


def test_a_halved_strength_was_needed():
    """Status 0 after t >= 1 halvings: the probe at 2 * lambda fails (the
    returned strength is the largest of lambda0 * 2^-t that succeeds)."""
    seen = 0
    for K, f, P in SHAPES:
        for seed in SEEDS:
            _, _, G, b, c, (lam, status, t, stats) = _case(K, f, P, seed)
            if status == 0:
                assert lam == stats[0] * 0.5 ** t and stats[3] <= stats[4]
            if status != 0 or t < 1:
                continue
            seen += 1
            satt, smin = ref.probe(ref.sorted_rows(G), np.diag(G), b, np.float64(c), K, f, 2.0 * lam)
            assert not satt <= smin, (K, f, P, seed, t)
    assert seen > 0


def test_degenerate_strengths():
    """A NaN among e, b or c: lambda NaN, status 3, no row changed; c == 0:
    lambda 0, status 2, the rows become g."""
    K, f, P = 7, 2, 19
    X, g, G, b, c, _ = _case(K, f, P, 0)
    nan = float("nan")
    Gn = G.copy()
    Gn[2, 2] = nan
    bn = b.copy()
    bn[1] = nan
    for args in ((Gn, b, c), (G, bn, c), (G, b, nan)):
        lam, status, t, _ = ref.strength(*args, K, f)
        assert np.isnan(lam) and status == 3 and t == 0
        assert torch.equal(ref.krum_rows(X, g, f, np.float32(lam)), X)
    lam, status, t, _ = ref.strength(G, np.zeros_like(b), 0.0, K, f)
    assert lam == 0.0 and status == 2 and t == 0
    Xb = X[f:]
    mu = torch.from_numpy(ref.mean_sign(X, g, f)[0])
    Y = ref.krum_rows(X, mu, f, np.float32(0.0))
    assert (ref.mean_sign(X, mu, f)[1] == 0).all() and torch.equal(Y[:f], mu.expand(f, P)) and torch.equal(Y[f:], Xb)


def test_philox_known_answers():
    """Philox4x32-10 against the known-answer vectors of Random123 (Salmon,
    Moraes, Dror, Shaw, "Parallel Random Numbers: As Easy as 1, 2, 3", SC 2011;
    the library's kat_vectors): counter and key all zeros, all ones, and the
    digits of pi."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(w) for w in ref.philox4x32_10(ctr, key))
        assert got == want, [hex(w) for w in got]
    # arrays: each element its own counter
    w = ref.philox4x32_10([np.array([0, 0xffffffff]), np.array([0, 0xffffffff]), np.array([0, 0xffffffff]),
                           np.array([0, 0xffffffff])], [np.array([0, 0xffffffff])] * 2)
    assert [int(v) for v in w[0]] == [0x6627e8d5, 0x408f276d]
    u = ref.uniforms(1000, 3, seed=(5 << 32) | 7, stream=2, col0=(1 << 32) - 500)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0 and 0.4 < u.mean() < 0.6
    assert len(np.unique(u)) > 2990
    assert np.array_equal(u[:, 500:], ref.uniforms(500, 3, seed=(5 << 32) | 7, stream=2, col0=1 << 32))


@pytest.mark.parametrize("b", [2.0, 1.5])
def test_fang_trim_ranges(b):
    """Every attacker value lies between near and far in either orientation and
    beyond the benign extreme on the side opposite s; s == 0 gives mu; the benign
    rows stay."""
    K, f, P = 12, 4, 257
    X, g = replace_ref.updates(K, f, P, 3)
    g[5] = 1.0
    X[f:, 5] = torch.tensor([1.25, 0.75] * 4)                  # every partial sum exact, mean == g: s == 0
    for col, below, g_col in ((6, True, -100.0), (7, True, 100.0), (8, False, 100.0), (9, False, -100.0)):
        if below:                                              # every benign value <= -1 / >= 1,
            X[f:, col] -= X[f:, col].max() + 1.0               # the model on either side of them
        else:
            X[f:, col] += 1.0 - X[f:, col].min()
        g[col] = g_col
    mu, s, near, far = ref.trim_bounds(X, g, f, b)
    assert s[5] == 0 and (s != 0).sum() == P - 1 and (s > 0).any() and (s < 0).any()
    assert [s[6], s[7], s[8], s[9]] == [1, -1, -1, 1]
    assert far[6] == near[6] * np.float32(b) and far[7] == near[7] / np.float32(b)
    assert far[8] == near[8] * np.float32(b) and far[9] == near[9] / np.float32(b)
    Y = ref.trim_rows(X, g, f, b, seed=11, stream=4)
    assert torch.equal(Y[f:], X[f:])
    A, Xb = Y[:f].numpy(), X[f:].numpy()
    lo, hi = np.minimum(near, far), np.maximum(near, far)
    live = s != 0
    assert ((A >= lo) & (A <= hi))[:, live].all()
    assert (A[:, s > 0] <= Xb.min(axis=0)[s > 0]).all() and (A[:, s < 0] >= Xb.max(axis=0)[s < 0]).all()
    assert (A[:, 5] == mu[5]).all()
    assert (np.abs(far - near)[live] > 0).all() and not np.array_equal(A[0], A[1])
    assert not torch.equal(Y[:f], ref.trim_rows(X, g, f, b, seed=11, stream=5)[:f])


def test_workspace_functions():
    """0 for the arguments the calls reject; otherwise a multiple of 256 that
    grows with the shape."""
    lib = _capi.lib()
    ws, sws = lib.flr_fang_krum_workspace, lib.flr_fang_krum_strength_workspace
    for K, P, f in ((12, 0, 4), (12, 67, 0), (12, 67, -1), (10, 67, 4), (4, 67, 1), (1200, 67, 100), (0, 67, 1)):
        assert ws(K, P, f) == 0, (K, P, f)
    for K, f in ((12, 0), (10, 4), (1200, 100)):
        assert sws(K, f) == 0, (K, f)
    sizes = [ws(K, P, f) for K, P, f in ((5, 1, 1), (12, 67, 4), (130, 333, 26), (1124, 67, 100), (1124, 100000, 100))]
    assert all(n > 0 and n % 256 == 0 for n in sizes) and sizes == sorted(sizes)
    assert sws(5, 1) % 256 == 0 and sws(5, 1) >= 4 * 3 * 8 and sws(1124, 100) >= 1024 * 1023 * 8
    assert sws(1124, 100) % 256 == 0 and ws(1124, 67, 100) > sws(1124, 100)


def test_engine_configuration_checks():
    """The names are attacks; unknown attack_cfg keys, bad values, K < 2f + 3 and
    fang_krum on the all-to-all exchange at world > 1 are refused before anything
    is allocated."""
    assert "fang_krum" in ATTACKS and "fang_trim" in ATTACKS

    def engine(attack, cfg, K=12, f=4, **kw):
        rkw = {k: kw.pop(k) for k in ("exchange", "defense") if k in kw}
        return RoundEngine(TINY, RoundConfig(num_clients=K, num_attackers=f, attack=attack, attack_cfg=cfg, **rkw),
                           device="cpu", **kw)

    with pytest.raises(ValueError, match="attack_cfg keys"):
        engine("fang_krum", {"b": 2.0})
    with pytest.raises(ValueError, match="attack_cfg keys"):
        engine("fang_trim", {"threshold": 1e-5})
    with pytest.raises(ValueError, match="attack_cfg keys"):
        engine("fang_trim", {"perturb": "sign"})
    for bad in (0, 0.0, -1e-5, float("nan"), float("inf"), True, "1e-5"):
        with pytest.raises(ValueError, match="threshold"):
            engine("fang_krum", {"threshold": bad})
    for K, f in ((10, 4), (12, 5), (4, 1), (12, 0)):
        with pytest.raises(ValueError, match="2f \\+ 3"):
            engine("fang_krum", {}, K=K, f=f)
    with pytest.raises(ValueError, match="whole client rows"):
        engine("fang_krum", {}, exchange="alltoall", defense="median", rank=0, world=2)
    for bad in (1.0, 0.5, 0, -2.0, float("nan"), float("inf"), 1e39, 1.0 + 2.0 ** -30, True, "2"):
        with pytest.raises(ValueError, match="b must be"):
            engine("fang_trim", {"b": bad})
    for bad in (1.5, "7", True):
        with pytest.raises(ValueError, match="seed"):
            engine("fang_trim", {"seed": bad})
    for f in (0, 12, 13):
        with pytest.raises(ValueError, match="1 <= f < K"):
            engine("fang_trim", {}, f=f)


def test_attack_functions_validate():
    """All before any device work: a CPU matrix gets as far as the checks."""
    X, g = torch.zeros(8, 8), torch.zeros(8)
    for f in (0, 3, -1, 8):
        with pytest.raises(ValueError, match="2f \\+ 3"):
            fang_krum_(X, f, g)
    for bad in (0, -1.0, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="threshold"):
            fang_krum_(X, 2, g, threshold=bad)
    for f in (0, 8, -1):
        with pytest.raises(ValueError, match="1 <= f < K"):
            fang_trim_(X, f, g)
    for bad in (1.0, 0.0, -3.0, float("nan"), float("inf"), True, "2"):
        with pytest.raises(ValueError, match="b must be"):
            fang_trim_(X, 2, g, b=bad)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        fang_krum_(X, 2, g)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        fang_trim_(X, 2, g)
