"""Host: the FLAME defense's configuration rules and the properties of the CPU
restatement (tests/flame_ref.py) that the GPU tests compare the kernels with —
the attackers' rejection on the generator's rows, the admitted counts, the
margins the GPU tests rely on, the edge cases, the closed form of the
clustering against sklearn's HDBSCAN, and the Gaussian reference's moments.
No GPU."""
import functools

import numpy as np
import pytest
import torch

import flame_ref as ref
from flr.defenses import CenteredDefense, FlameDefense, defense_names, get_defense

# (K, P, f): the generator's shapes
SHAPES = [(5, 7, 2), (8, 64, 2), (17, 333, 4), (33, 1027, 6), (64, 256, 31), (65, 2048, 13), (130, 5000, 26),
          (300, 600, 60), (1024, 256, 100)]
MARGIN = 1e-9


def test_registry_and_defaults():
    d = get_defense("flame", {})
    assert isinstance(d, FlameDefense)
    assert d.noise_lambda == 0.001 and d.min_cluster_size is None and d.on == "updates" and d.seed == 0
    assert d.calls == 0
    # what the round engine and bench.py read off a defense: the global model is passed, whole rows in torch
    # order, and none of the Krum family's attributes
    assert isinstance(d, CenteredDefense) and d.takes_global and not d.supports_sharded and not d.order_free
    for attr in ("publish", "comm", "tap_blocks", "pairwise_method", "multi_k"):
        assert not hasattr(d, attr), attr
    assert not getattr(d, "supports_dead_rows", False)
    assert "flame" in defense_names() and len(set(defense_names())) == len(defense_names())
    with pytest.raises(ValueError, match="flame"):
        get_defense("no_such_rule", {})
    assert d.client_weights == [] and d.detect_malicious() == []
    assert d.get_metrics() == {"defense_type": "flame", "noise_lambda": 0.001, "min_cluster_size": None,
                               "on": "updates", "seed": 0, "calls": 0, "admitted": None, "clip_bound": None,
                               "threshold": None, "sigma": None, "no_update": False, "bad_rows": False}
    d = get_defense("flame", {"noise_lambda": 0, "min_cluster_size": 5, "on": "weights", "seed": 7})
    assert d.noise_lambda == 0.0 and d.min_cluster_size == 5 and d.on == "weights" and d.seed == 7
    d.set_center(torch.zeros(3))
    d.set_center(None)


@pytest.mark.parametrize("cfg", [
    {"noise_lambda": -1e-9}, {"noise_lambda": float("nan")}, {"noise_lambda": float("inf")},
    {"noise_lambda": True}, {"noise_lambda": "0.001"}, {"noise_lambda": None},
    {"min_cluster_size": 0}, {"min_cluster_size": -3}, {"min_cluster_size": 2.0}, {"min_cluster_size": True},
    {"min_cluster_size": "3"}, {"min_cluster_size": 1025},
    {"on": "update"}, {"on": None}, {"on": 1}, {"on": ["updates"]},
    {"seed": 1.5}, {"seed": "0"}, {"seed": None}, {"seed": True}, {"seed": 1 << 64},
])
def test_invalid_config(cfg):
    with pytest.raises(ValueError):
        get_defense("flame", cfg)


def test_size_rules_raise_before_device_work():
    d = get_defense("flame", {})
    with pytest.raises(ValueError):
        d.aggregate([], [])
    with pytest.raises(ValueError):
        d.aggregate([[torch.zeros(1)]] * 1025, [])
    # min_cluster_size against K: 2 m > K and m <= K, per call
    d = get_defense("flame", {"min_cluster_size": 4})
    for K in (3, 8, 9):
        with pytest.raises(ValueError, match="min_cluster_size"):
            d.aggregate([[torch.zeros(1)]] * K, [])
    assert d.calls == 0 and d.detect_malicious() == []


@functools.lru_cache(maxsize=None)
def _rounds(K, P, f):
    return ref.rounds(K, P, f)


@pytest.mark.parametrize("K,P,f", SHAPES)
def test_attackers_rejected(K, P, f):
    """On each of the generator's rounds no attacker is admitted, the admitted
    count is m or m + 1 (the cluster is cut the moment it reaches m) and no
    pair distance lies within 1e-9 of t*."""
    g, Xs = _rounds(K, P, f)
    m = K // 2 + 1
    for X in Xs:
        out, sel = ref.run(g, X, lam=0.001)
        print("K", K, "admitted", sel.L, "t*", sel.tstar, "S", sel.S, "margin", sel.margin)
        assert sel.flags == 0 and np.isfinite(out).all()
        assert not sel.keep[:f].any()
        assert sel.L in (m, m + 1) and sel.L == int(sel.keep.sum())
        assert sel.margin > MARGIN
        assert 0.6 < float(sel.beta.astype(np.float64).sum()) <= 1.0 + 1e-6   # clipped by at most 1 / 1.5
        assert sel.sigma == np.float32(0.001 * sel.S) and sel.S > 0


def test_select_by_hand():
    """Four unit rows: 0 and 1 at cosine 0.9, 2 at 0.5 to both, 3 orthogonal
    to all.  m = 3: the edges enter at 0.1 (0-1), then 0.5 (0-2 and 1-2
    together): the component {0, 1, 2} appears at t* = 0.5."""
    G = np.array([[1.0, 0.9, 0.5, 0.0], [0.9, 1.0, 0.5, 0.0], [0.5, 0.5, 1.0, 0.0], [0.0, 0.0, 0.0, 4.0]])
    sel = ref.select(G, lam=0.5)
    assert sel.keep.tolist() == [1, 1, 1, 0] and sel.tstar == 0.5 and sel.L == 3 and sel.flags == 0
    assert sel.margin == pytest.approx(0.4)          # 0.1 and 1.0 are the other levels; 0.5 itself is left out
    assert sel.S == 1.0                              # sort(1, 1, 1, 2)[1]
    assert np.array_equal(sel.beta, np.array([1 / 3, 1 / 3, 1 / 3, 0], dtype=np.float32))
    assert sel.sigma == np.float32(0.5)
    # the long row admitted: clipped to S
    sel = ref.select(G, m=4)
    assert sel.keep.tolist() == [1, 1, 1, 1] and sel.tstar == 1.0 and sel.L == 4
    assert np.array_equal(sel.beta, np.array([0.25, 0.25, 0.25, 0.125], dtype=np.float32))


def test_edge_cases():
    g, Xs = _rounds(8, 64, 2)
    U = (Xs[0] - g[None, :]).astype(np.float32)
    # K = 1: the one good row is admitted
    one = ref.select(ref.gram(U[:1]), lam=0.001)
    assert one.keep.tolist() == [1] and one.beta.tolist() == [1.0] and one.flags == 0 and one.L == 1
    assert one.tstar == 0.0
    # K = 2: m = 2, both or none
    two = ref.select(ref.gram(U[2:4]))
    assert two.keep.tolist() == [1, 1] and two.L == 2 and two.S == min(np.sqrt(np.diag(ref.gram(U[2:4]))))
    # f = 0
    h = ref.select(ref.gram(U[2:]))
    assert 4 <= h.L <= 6 and h.flags == 0
    # a zero update row: distance 1 to all, gamma = 1
    Z = U.copy()
    Z[5] = 0.0
    z = ref.select(ref.gram(Z), m=8)
    assert (z.dist[5, np.arange(8) != 5] == 1.0).all() and z.keep.all() and z.tstar == 1.0
    assert z.beta[5] == np.float32(1.0 / 8)
    # fewer than m good rows: no cluster, the result is the center
    B = U.copy()
    B[:4, 3] = np.nan
    nb = ref.select(ref.gram(B), lam=0.001)
    assert nb.flags == 3 and not nb.keep.any() and not nb.beta.any() and nb.sigma == 0 and nb.L == 0
    assert nb.tstar == np.inf
    assert np.array_equal(ref.combine(g[None, :] + B, g, nb.beta), g)
    # a NaN row and an inf row among enough good ones: rejected, the result is finite
    C = U.copy()
    C[3, 7] = np.nan
    C[0, 1] = np.inf
    nc = ref.select(ref.gram(C), lam=0.001)
    assert nc.flags == 2 and nc.keep[3] == 0 and nc.keep[0] == 0 and nc.L >= 5 and np.isfinite(nc.S)
    assert np.isfinite(ref.combine(g[None, :] + C, g, nc.beta)).all()
    # identical attacker rows: distance 0 (up to rounding) to each other, still rejected
    I = U.copy()
    I[1] = I[0]
    ni = ref.select(ref.gram(I))
    assert abs(ni.dist[0, 1]) < 1e-15 and not ni.keep[:2].any() and ni.L >= 5
    # min_cluster_size = K: everyone good is admitted
    a = ref.select(ref.gram(U), m=8)
    assert a.keep.all() and a.L == 8 and a.flags == 0
    ac = ref.select(ref.gram(C), m=8)
    assert ac.flags == 3 and not ac.keep.any()


def test_exact_ties_enter_together():
    """Integer rows with equal norms and equal dot products: several d_ij are
    the same bits, and the component appears with all of them at once."""
    A = np.array([[3, 0, 0, 0, 4], [0, 3, 0, 0, 4], [0, 0, 3, 0, 4], [0, 0, 0, 3, 4], [5, 0, 0, 0, 0],
                  [0, -5, 0, 0, 0]], dtype=np.float32)
    sel = ref.select(ref.gram(A))
    d = sel.dist
    assert d[0, 1] == d[0, 2] == d[1, 3] == d[2, 3] == 1.0 - 16.0 / 25.0
    assert sel.keep.tolist() == [1, 1, 1, 1, 0, 0] and sel.tstar == d[0, 1] and sel.L == 4
    assert sel.margin > 0.01


def _planted(rng, K):
    """A random distance-like Gram matrix: K rows in a few planted groups."""
    P = 40
    centers = rng.standard_normal((int(rng.integers(1, 4)), P))
    A = centers[rng.integers(0, len(centers), K)] * rng.uniform(0.0, 2.0) + rng.standard_normal((K, P))
    return ref.gram(A.astype(np.float32))


def test_closed_form_matches_hdbscan():
    """The admitted set is sklearn's HDBSCAN(metric="precomputed",
    min_cluster_size=m, min_samples=1, allow_single_cluster=True) cluster, on the
    reference's own distance matrices (K <= 130) and on random ones."""
    cluster = pytest.importorskip("sklearn.cluster")
    if not hasattr(cluster, "HDBSCAN"):
        pytest.skip("sklearn without HDBSCAN")
    mats = []
    for K, P, f in SHAPES:
        if K <= 130:
            g, Xs = _rounds(K, P, f)
            mats.append(ref.gram(Xs[0], g))
    rng = np.random.default_rng(3)
    for _ in range(40):
        mats.append(_planted(rng, int(rng.integers(5, 40))))
    for G in mats:
        K = G.shape[0]
        m = K // 2 + 1
        sel = ref.select(G)
        D = sel.dist.copy()
        np.fill_diagonal(D, 0.0)
        D = np.maximum(D, 0.0)      # a rounding-negative distance between near-identical rows
        labels = cluster.HDBSCAN(metric="precomputed", min_cluster_size=m, min_samples=1,
                                 allow_single_cluster=True).fit(D).labels_
        assert set(labels.tolist()) <= {0, -1}
        assert np.array_equal(labels == 0, sel.keep == 1), (K, sel.L, int((labels == 0).sum()))


def test_gaussian_reference():
    """2^20 draws: mean within 5 / sqrt(P) of 0, variance within 5 * sqrt(2 / P)
    of 1, |z| <= 5.78 (r <= sqrt(48 ln 2)); a column range is the slice of the
    whole; streams and seeds differ."""
    P = 1 << 20
    z = ref.normals(P, seed=0, stream=0)
    assert z.shape == (P,) and np.isfinite(z).all()
    print("mean", z.mean(), "var", z.var(), "max |z|", np.abs(z).max())
    assert abs(z.mean()) <= 5 / np.sqrt(P)
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(2 / P)
    assert np.abs(z).max() <= 5.78
    for col0, n in ((0, 9), (1, 3), (2, 4), (3, 5), (5, 1027), (1000, 1)):
        assert np.array_equal(ref.normals(n, col0=col0), z[col0:col0 + n])
    assert not np.array_equal(ref.normals(64, stream=1), z[:64])
    assert not np.array_equal(ref.normals(64, seed=1), z[:64])
    assert not np.array_equal(ref.normals(64, seed=1 << 32), z[:64])
    big = (1 << 34) - 6          # crosses the counter's low word
    w = ref.normals(16, col0=big)
    assert np.array_equal(ref.normals(7, col0=big + 5), w[5:12])
