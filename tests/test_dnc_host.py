"""Host: the DnC defense's configuration rules and the properties of the CPU
restatement (tests/dnc_ref.py) that the GPU tests compare the kernels with — the
column sampling, the Gram-matrix power iteration against numpy's SVD, the
attackers' removal, the degenerate and the bad-row cases.  No GPU."""
import math

import numpy as np
import pytest
import torch

import dnc_ref
from flr.defenses import get_defense

# (K, P, b, f): uneven strata; G just above 128 rows; the largest subsample
SHAPES = [(33, 1027, 200, 6), (130, 5000, 1000, 26), (128, 20011, 4096, 25)]


def test_registry_and_defaults():
    d = get_defense("dnc", {"num_malicious": 3})
    assert (d.num_malicious, d.filter_frac, d.niters, d.subsample_dim, d.power_iters, d.seed) == (3, 1.0, 1, 10000,
                                                                                                32, 0)
    assert not d.supports_sharded and not d.order_free
    assert d.selected_clients == [] and d.rejected_clients == [] and d.detect_malicious() == []
    m = d.get_metrics()
    assert m["defense_type"] == "dnc" and m["kept_count"] is None and m["fallback"] is False and m["scores"] == []
    assert d._nremove(10) == 3 and d._nremove(3) == 2 and d._nremove(1) == 0
    assert get_defense("dnc", {"num_malicious": 3, "filter_frac": 1.5})._nremove(10) == 5
    assert get_defense("dnc", {})._nremove(10) == 0


@pytest.mark.parametrize("cfg", [
    {"num_malicious": -1}, {"num_malicious": 1.5}, {"num_malicious": True}, {"num_malicious": "2"},
    {"filter_frac": -0.5}, {"filter_frac": float("nan")}, {"filter_frac": float("inf")}, {"filter_frac": "1"},
    {"niters": 0}, {"niters": 17}, {"niters": 1.0},
    {"subsample_dim": 0}, {"subsample_dim": 65537}, {"subsample_dim": 10.5},
    {"power_iters": 0}, {"power_iters": 1025}, {"power_iters": None},
    {"seed": 0.5}, {"seed": 1 << 64},
])
def test_invalid_config(cfg):
    with pytest.raises(ValueError):
        get_defense("dnc", cfg)


def test_size_rules_raise_before_device_work():
    d = get_defense("dnc", {"num_malicious": 1})
    with pytest.raises(ValueError):
        d.aggregate([], [])
    with pytest.raises(ValueError):
        d.aggregate([[torch.zeros(1)]] * 1025, [])


@pytest.mark.parametrize("P,b", [(7, 7), (64, 16), (1027, 200), (5000, 1000), (20011, 4096), (11, 10), (100000, 3)])
def test_columns(P, b):
    for seed, it in ((0, 0), (7, 0), (7, 3), ((1 << 64) - 1, 15)):
        c = dnc_ref.columns(P, b, seed, it)
        assert (np.diff(c) > 0).all() and c[0] >= 0 and c[-1] < P          # distinct, ascending, in range
        j = np.arange(b)
        assert ((j * P) // b <= c).all() and (c < ((j + 1) * P) // b).all()  # one per stratum
        if b == P:
            assert np.array_equal(c, np.arange(P))
    assert not np.array_equal(dnc_ref.columns(P, b, 7, 0), dnc_ref.columns(P, b, 8, 0)) or b == P
    assert not np.array_equal(dnc_ref.columns(P, b, 7, 0), dnc_ref.columns(P, b, 7, 1)) or b == P


def test_mix_is_splitmix64():
    # splitmix64's first outputs from state 0 (the published test vector): mix(k * golden)
    assert dnc_ref.mix(dnc_ref.GOLDEN) == 0xE220A8397B1DCDAF
    assert dnc_ref.mix(2 * dnc_ref.GOLDEN) == 0x6E789E6AA1B965F4


@pytest.mark.parametrize("K,P,b,f", SHAPES)
def test_scores_match_svd_and_attackers_are_removed(K, P, b, f):
    X = dnc_ref.alie_rows(K, P, f, seed=1)
    cols, scores, keep, count, flag, margin = dnc_ref.dnc_select(X, b, 1, f, 32, seed=7)
    C, bad = dnc_ref.center(X[:, torch.from_numpy(cols[0])].contiguous())
    assert not bad.any()
    Cd = C.double().numpy()
    v1 = np.linalg.svd(Cd, full_matrices=False)[2][0]
    true = (Cd @ v1) ** 2
    err = np.abs(scores[0] - true).max() / true.max()
    print("scores vs SVD, relative to the largest:", err, "| margin", margin)
    assert err <= 1e-6
    assert keep[:f].sum() == 0 and keep[f:].all() and count == K - f and flag == 0
    assert margin > 0.5
    agg, keep2, _ = dnc_ref.dnc(X, b, 1, f, 32, seed=7)
    assert torch.equal(keep2, keep)
    want = torch.zeros(P)
    for i in range(f, K):
        want = want + X[i]
    assert torch.equal(agg, want / torch.tensor(float(K - f)))


def test_identical_rows_score_zero():
    row = torch.randint(-8, 9, (40,), generator=torch.Generator().manual_seed(0)).float()
    X = row.repeat(6, 1)
    _, scores, keep, count, flag, margin = dnc_ref.dnc_select(X, 10, 2, 2, 32, seed=3)
    assert (scores == 0).all() and margin == math.inf
    assert keep.tolist() == [1, 1, 1, 1, 0, 0] and count == 4 and flag == 0   # ties: the lower index first
    one = dnc_ref.dnc_select(X[:1], 10, 1, 0, 32)
    assert one[1].tolist() == [[0.0]] and one[2].tolist() == [1]


def test_bad_row_gets_inf_and_is_not_kept():
    X = dnc_ref.alie_rows(9, 50, 2, seed=2)
    X[4, 10] = float("nan")
    X[7, 20] = float("-inf")
    cols = np.array([[5, 10, 20, 30, 40]])
    _, scores, keep, count, flag, _ = dnc_ref.dnc_select(X, 5, 1, 2, 32, cols=cols)
    assert np.isinf(scores[0, [4, 7]]).all() and np.isfinite(np.delete(scores[0], [4, 7])).all()
    assert keep[4] == 0 and keep[7] == 0 and count == 7 - 2 + 2 and flag == 0   # the bad rows fill the removed ranks
    agg = dnc_ref.rows_mean_keep(X, keep)
    assert torch.isfinite(agg).all()
    # the same rows outside the sampled columns: not bad
    _, scores2, _, _, _, _ = dnc_ref.dnc_select(X, 3, 1, 2, 32, cols=np.array([[5, 30, 40]]))
    assert np.isfinite(scores2).all()
    # every row bad: nothing kept, the mean is NaN
    X[:, 5] = float("inf")
    _, scores3, keep3, count3, flag3, _ = dnc_ref.dnc_select(X, 5, 1, 2, 32, cols=cols)
    assert np.isinf(scores3).all() and count3 == 0 and flag3 == 1 and not keep3.any()
    assert torch.isnan(dnc_ref.rows_mean_keep(X, keep3)).all()


def test_intersection_and_fallback():
    X = dnc_ref.alie_rows(12, 64, 3, seed=4)
    _, _, k1, _, _, _ = dnc_ref.dnc_select(X, 16, 1, 3, 32, seed=5)
    used, scores, k3, count, flag, _ = dnc_ref.dnc_select(X, 16, 3, 3, 32, seed=5)
    per = [dnc_ref.keep_of(scores[it], np.zeros(12, bool), 3)[0] for it in range(3)]
    assert np.array_equal(k3.numpy().astype(bool), per[0] & per[1] & per[2]) and flag == 0
    assert np.array_equal(per[0], k1.numpy().astype(bool)) and count == int(k3.sum())
    assert len({tuple(u) for u in used}) == 3
