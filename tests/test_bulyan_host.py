"""CPU: Bulyan's registry entry, its size rules, the C entries' argument
checks (no GPU touched) and the numpy reference's own invariants."""
import numpy as np
import pytest
import torch

from bulyan_ref import SELECTION_SHAPES, iter_krum, sizes, window_mean, window_ranks
from flr import _capi
from flr.defenses import BulyanDefense, KrumDefense, get_defense
from flr.workload import split_rows, update_matrix
from oracle import aggregation as orc


def test_registry_knows_bulyan():
    d = get_defense("bulyan", {"num_malicious": 2, "multi_k": 5})
    assert isinstance(d, BulyanDefense) and isinstance(d, KrumDefense)
    assert d.num_malicious == 2 and d.pairwise_method == "reference"
    assert d.supports_sharded and d.order_free and d.needs_tap_blocks and not d.supports_dead_rows
    m = d.get_metrics()
    assert m["defense_type"] == "bulyan" and {"theta", "beta", "selected_clients", "rejected_clients",
                                              "client_scores", "num_malicious_assumed"} <= set(m)


def _cpu_updates(n, P=10):
    return [[torch.zeros(P)] for _ in range(n)]


def test_too_few_clients_raises_before_device_work():
    d = get_defense("bulyan", {"num_malicious": 2})
    with pytest.raises(ValueError) as e:
        d.aggregate(_cpu_updates(10), [1] * 10)  # CPU tensors: any device work would fail differently
    assert str(e.value) == "Bulyan requires n >= 4f + 3. Got n=10, f=2. Need at least 11 clients."


def test_row_limit_raises_before_device_work():
    d = get_defense("bulyan", {"num_malicious": 10})
    with pytest.raises(ValueError, match="128-row limit"):
        d.aggregate(_cpu_updates(149, 2), [1] * 149)  # theta = 129
    d._sizes(148)  # theta = 128 is in range
    assert (d.theta, d.beta) == (128, 108)


def test_c_entries_validate_without_gpu():
    lib = _capi.lib()
    A, U, W = _capi.FLR_ERR_ARG, _capi.FLR_ERR_UNSUPPORTED, _capi.FLR_ERR_WORKSPACE
    x = 4096  # a non-null pointer value that is never dereferenced: every call returns before device work
    wm = lib.flr_median_window_mean_rows
    assert wm(None, 8, 10, 10, None, 8, 4, x, None) == A
    assert wm(x, 8, 10, 10, None, 8, 4, None, None) == A
    assert wm(x, 8, 10, 10, None, 0, 1, x, None) == A      # m < 1
    assert wm(x, 8, 10, 10, None, 9, 4, x, None) == A      # m > K
    assert wm(x, 8, 10, 10, None, 8, 0, x, None) == A      # beta < 1
    assert wm(x, 8, 10, 10, None, 8, 9, x, None) == A      # beta > m
    assert wm(x, 8, 10, 9, None, 8, 4, x, None) == A       # ldx < P
    assert wm(x, 200, 10, 10, None, 129, 4, x, None) == U  # m > 128
    assert wm(x, 8, 0, 0, None, 8, 4, x, None) == _capi.FLR_OK  # P = 0: nothing to do
    ki = lib.flr_krum_select_iter
    assert ki(None, 8, 1, 6, x, x, x, 1 << 20, None) == A
    assert ki(x, 8, 1, 6, None, x, x, 1 << 20, None) == A
    assert ki(x, 8, 1, 6, x, None, x, 1 << 20, None) == A
    assert ki(x, 8, -1, 6, x, x, x, 1 << 20, None) == A
    assert ki(x, 8, 1, 0, x, x, x, 1 << 20, None) == A
    assert ki(x, 8, 1, 9, x, x, x, 1 << 20, None) == A
    assert ki(x, 0, 0, 1, x, x, x, 1 << 20, None) == A
    assert ki(x, 1025, 1, 6, x, x, x, 1 << 20, None) == U
    need = lib.flr_krum_select_iter_workspace(8)
    assert ki(x, 8, 1, 6, x, x, x, need - 1, None) == W
    assert ki(x, 8, 1, 6, x, x, None, need, None) == W


def test_workspace_query():
    lib = _capi.lib()
    assert lib.flr_krum_select_iter_workspace(0) == 0
    assert lib.flr_krum_select_iter_workspace(128) > 0


@pytest.mark.parametrize("theta,beta", [(5, 1), (7, 3), (8, 4), (9, 5), (78, 28), (128, 64), (128, 128)])
@pytest.mark.parametrize("ties", [False, True])
def test_reference_window_is_contiguous_and_holds_the_median(theta, beta, ties):
    rng = np.random.default_rng(theta * 131 + beta)
    S = rng.standard_normal((theta, 300)).astype(np.float32)
    if ties:
        S = (np.round(S * 4) / 4).astype(np.float32)
    s, sel = window_ranks(S, beta)
    medrank = (theta - 1) // 2
    assert (sel.sum(axis=0) == beta).all()
    if not ties:
        assert sel[medrank].all()
    # exact ties: every rank equal to the median is at distance 0 and the stable
    # argsort takes the lowest of them first, so the median's value is taken, not
    # always its rank
    assert ((s == s[medrank]) & sel).any(axis=0).all()
    got = window_mean(S, beta)
    for c in range(0, s.shape[1], 7):
        vals = s[sel[:, c], c]
        # by value the taken ranks are one window [lo, lo + beta) holding the median
        # rank (with exact ties the stable argsort may take a tied rank farther
        # out: the same value)
        assert any(np.array_equal(vals, s[lo:lo + beta, c])
                   for lo in range(max(0, medrank - beta + 1), min(medrank, theta - beta) + 1)), c
        if beta < theta:  # no value left out is closer to the median than one taken
            assert np.abs(vals - s[medrank, c]).max() <= np.abs(s[~sel[:, c], c] - s[medrank, c]).min()
        acc = np.float32(0)
        for x in vals:
            acc = np.float32(acc + x)
        assert got[c] == np.float32(acc / np.float32(beta))


def test_reference_nan_rule():
    S = np.arange(9 * 4, dtype=np.float32).reshape(9, 4)
    S[2, 0] = np.nan                      # 1 NaN: the window sits on the finite ranks
    S[[1, 3, 5, 7], 1] = np.nan           # 4 = theta - beta NaNs: the 5 finite values are taken
    S[[0, 2, 4, 6, 8], 2] = np.nan        # 5 NaNs: one would be taken
    out = window_mean(S, 5)
    assert np.isfinite(out[[0, 1, 3]]).all() and np.isnan(out[2])
    assert out[1] == np.float32(1 + 9 + 17 + 25 + 33) / np.float32(5)
    assert np.isnan(window_mean(S, 6)[1])  # beta = 6: more than theta - beta NaNs
    T = S[:, 1:2].copy()                   # 4 NaNs of 9 with beta = 1: the median rank 4 is the last finite one
    assert np.isfinite(window_mean(T, 1)[0])
    T[0, 0] = np.nan                       # 5 NaNs: the median rank is a NaN though theta - beta = 8 allows them
    assert np.isnan(window_mean(T, 1)[0])


@pytest.mark.parametrize("K,f,P", SELECTION_SHAPES)
def test_reference_selection(K, f, P):
    X = update_matrix(K, P, f, seed=K, device="cpu")[:, :P]
    ups = split_rows(X, P, [(P,)])
    dist = orc.distance_matrix(ups)
    theta, _ = sizes(K, f)
    picked, first = iter_krum(dist, f, theta)
    assert len(set(picked)) == theta
    assert first == orc.krum_scores(dist, K - f - 2)
    # the iterated selection is not one-shot Multi-Krum: the power of the GPU test
    one_shot = orc.krum(ups, f, theta)[2]
    assert set(picked) != set(one_shot)
