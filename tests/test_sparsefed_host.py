"""Host: SparseFed's registry entry and config validation, the properties of the
CPU restatement itself (tests/sparsefed_ref.py), and the guard checks the GPU
tests rely on — that the planted inputs do exercise the ties, the clipping and
the error memory — so that a bad seed fails here and not on the GPU as a
"kernel bug".  The seeds in sparsefed_ref.py were checked here."""
import functools
import math

import numpy as np
import pytest

import sparsefed_ref as R
from flr.defenses import SparseFedDefense, defense_names, get_defense

NAN, INF = float("nan"), float("inf")


def test_registry_and_default_metrics():
    assert "sparsefed" in defense_names()
    d = get_defense("sparsefed", {})
    assert isinstance(d, SparseFedDefense)
    assert d.takes_global and not d.supports_sharded and not d.order_free
    assert d.get_metrics() == {"defense_type": "sparsefed", "k": 0.05, "clip_norm": "median", "momentum": 0.0,
                               "clipped": None, "dropped": None, "threshold": None, "bad_rows": False}
    assert d.memory() is None and d.mask() is None and d.detect_malicious() == []
    d.reset()
    assert "0.05" in repr(d)


@pytest.mark.parametrize("cfg", [
    {"k": True}, {"k": 0}, {"k": -3}, {"k": 0.0}, {"k": 1.5}, {"k": -0.1}, {"k": NAN}, {"k": "5"}, {"k": None},
    {"clip_norm": 0}, {"clip_norm": 0.0}, {"clip_norm": -1.0}, {"clip_norm": NAN}, {"clip_norm": INF},
    {"clip_norm": True}, {"clip_norm": "mean"}, {"clip_norm": None},
    {"momentum": -0.1}, {"momentum": 1.0}, {"momentum": 1.5}, {"momentum": NAN}, {"momentum": True},
    {"momentum": "0.5"}, {"momentum": 1.0 - 1e-9}, {"momentum": INF},
])
def test_config_rejected(cfg):
    with pytest.raises(ValueError, match=next(iter(cfg))):
        get_defense("sparsefed", cfg)


def test_config_accepted():
    d = get_defense("sparsefed", {"k": 7, "clip_norm": 2.5, "momentum": 0.9})
    assert (d.k, d.clip_norm, d.momentum) == (7, 2.5, 0.9) and isinstance(d.k, int)
    assert d.resolve_k(7) == 7 and d.resolve_k(100) == 7
    with pytest.raises(ValueError, match="exceeds"):
        d.resolve_k(6)
    f = get_defense("sparsefed", {"k": 1.0, "clip_norm": "median", "momentum": 0})
    assert isinstance(f.k, float) and f.resolve_k(13) == 13
    h = get_defense("sparsefed", {"k": 0.05})
    assert [h.resolve_k(P) for P in (1, 5, 7, 300, 1027, 5000)] == [R.resolve_k(P) for P in (1, 5, 7, 300, 1027, 5000)]
    assert h.resolve_k(1027) == math.ceil(0.05 * 1027) == 52


# ---- the reference's selection ----

HOST_SIZES = [P for P in R.TOPK_SIZES if P <= 262147]


@pytest.mark.parametrize("kind", R.TOPK_KINDS)
@pytest.mark.parametrize("P", HOST_SIZES)
def test_reference_selection_properties(kind, P):
    v = R.topk_input(kind, P)
    key = R.keys(v).astype(np.int64)
    by = R.order(v)
    for k in R.topk_ks(P):
        s = R.select(v, k, by)
        sel = s.mask.astype(bool)
        assert int(sel.sum()) == k
        assert key[sel].min() >= (key[~sel].max() if k < P else 0)
        assert s.T == key[sel].min() and s.n_gt == int((key > s.T).sum()) and s.r == k - s.n_gt
        tied = np.flatnonzero(key == s.T)
        assert 1 <= s.r <= tied.size
        assert np.array_equal(np.flatnonzero(sel & (key == s.T)), tied[:s.r])   # the lowest indices
        assert s.flags == (1 if kind == "nonfinite" else 0)
    if kind == "nonfinite":   # a NaN or an inf ranks with zero
        assert (key[~np.isfinite(v)] == 0).all()


@pytest.mark.parametrize("P", [P for P in R.TOPK_SIZES if P >= 1027])
def test_guard_planted_ties(P):
    """At k = P // 3 the threshold lies inside the planted ties, 1 <= r < n_eq,
    and both the selected and the unselected ties occupy several chunks, each
    chunk boundary having a tie on both sides."""
    v = R.topk_input("ties", P)
    key = R.keys(v)
    s = R.select(v, P // 3)
    tied = np.flatnonzero(key == s.T)
    assert s.T == 0x3F800000 and 1 <= s.r < tied.size
    assert len(set(tied[:s.r] // R.CHUNK)) >= 2 or P < 3 * R.CHUNK
    assert len(set(tied // R.CHUNK)) == (P + R.CHUNK - 1) // R.CHUNK >= 2
    for b in range(R.CHUNK, P, R.CHUNK):
        assert key[b - 1] == s.T and key[b] == s.T
    assert {bool(x) for x in (v[tied] < 0)} == {True, False}   # both signs tie


def test_guard_digit_inputs():
    """"d3" differs in the last digit alone, "d2" in the middle one alone."""
    for P in (1027, 5000):
        k3, k2 = R.keys(R.topk_input("d3", P)), R.keys(R.topk_input("d2", P))
        assert len(set(k3 >> 9)) == 1 and len(set(k3 & 0x1FF)) > 256
        assert len(set(k2 >> 20)) == 1 and set(k2 & 0x1FF) == {0} and len(set((k2 >> 9) & 0x7FF)) > 512
        ex = R.keys(R.topk_input("extremes", P))
        assert (ex < 0x00800000).any() and (ex >= 0x7F000000).any()
        sp = R.topk_input("sparse", P)
        assert (R.bits(sp) == 0x80000000).any() and (R.bits(sp) == 0).any() and (sp != 0).sum() == P // 5 < P // 3


# ---- the reference's rounds ----

CASES = [(K, P, pad, False) for K, P, pad in R.SHAPES] + [(16, 5000, 24, True), (33, 1027, 1, True)]


@functools.lru_cache(maxsize=None)
def _rounds(K, P, pad, bad, rho, given=False):
    return R.run_rounds(K, P, pad, bad, rho, R.given_clip(K, P, pad, bad) if given else None)


@pytest.mark.parametrize("rho", [0.0, 0.5])
@pytest.mark.parametrize("K,P,pad,bad", CASES)
def test_reference_round_properties(K, P, pad, bad, rho):
    """Exactly k coordinates are applied; per coordinate either out == g and W
    keeps step 3's w, or out == g + w and W == +0 (U too)."""
    k = R.resolve_k(P)
    ref = R.SparseFed(k, None, rho)   # a second pass: the state after each round
    for t, (data, g, r) in enumerate(_rounds(K, P, pad, bad, rho)):
        sel = r.selection.mask.astype(bool)
        assert int(sel.sum()) == k and r.dropped == 0 and np.isfinite(r.out).all()
        assert r.weights.n == K - (1 if bad and t < 2 else 0)
        assert (r.weights.flags & 2 != 0) == (r.weights.n < K)
        again = ref.step(data[:, :P], g, R.norms(data[:, :P], g))
        assert R.same_bits(again.out, r.out) and np.array_equal(again.selection.mask, r.selection.mask)
        assert R.same_bits(r.out[sel], (g + r.w)[sel]) and (R.bits(ref.W[sel]) == 0).all()
        assert R.same_bits(r.out[~sel], g[~sel]) and R.same_bits(ref.W[~sel], r.w[~sel])
        if rho != 0.0:
            assert (R.bits(ref.U[sel]) == 0).all()


@pytest.mark.parametrize("rho", [0.0, 0.5])
@pytest.mark.parametrize("K,P,pad,bad", [c for c in CASES if c[0] >= 2])
@pytest.mark.parametrize("given", [False, True])
def test_guard_some_rows_clipped(K, P, pad, bad, rho, given):
    """With the median and with test_gpu_sparsefed.py's given constant."""
    for _, _, r in _rounds(K, P, pad, bad, rho, given):
        assert 0 < r.weights.clipped < r.weights.n, (r.weights.clipped, r.weights.n, r.weights.L)
        assert (r.weights.beta == 0).sum() == K - r.weights.n
        assert given == (r.weights.L == R.given_clip(K, P, pad, bad))


@pytest.mark.parametrize("rho", [0.0, 0.5])
@pytest.mark.parametrize("K,P,pad,bad", [c for c in CASES if c[1] >= 300])
def test_guard_error_memory_at_work(K, P, pad, bad, rho):
    """Round 2 selects another set than round 1, and some coordinate is applied
    that no single round's own average would have put into its top-k."""
    rounds = _rounds(K, P, pad, bad, rho)
    k = R.resolve_k(P)
    masks = [r.selection.mask.astype(bool) for _, _, r in rounds]
    assert not np.array_equal(masks[0], masks[1])
    own = np.zeros(P, dtype=bool)
    for data, g, r in rounds:
        a, _, _, _ = R.accumulate(data[:, :P], g, r.weights.beta, np.zeros(P, dtype=np.float32))
        own |= R.select(a, k).mask.astype(bool)
    late = (masks[1] | masks[2]) & ~own
    assert late.any(), (int(late.sum()), k)


def test_reference_weights_cases():
    e = np.array([3.0, 1.0, 2.0, 5.0, 4.0])
    w = R.weights(e)
    assert (w.L, w.n, w.clipped, w.flags) == (3.0, 5, 2, 0)
    assert np.array_equal(w.beta, np.array([1 / 5, 1 / 5, 1 / 5, (3.0 / 5.0) / 5, (3.0 / 4.0) / 5], dtype=np.float32))
    w = R.weights(np.array([3.0, NAN, 2.0, INF]))
    assert (w.L, w.n, w.clipped, w.flags) == (2.0, 2, 1, 2) and w.beta[1] == 0 and w.beta[3] == 0
    w = R.weights(np.array([NAN, INF]), 1.0)
    assert (w.L, w.n, w.flags) == (0.0, 0, 3) and not w.beta.any()
    w = R.weights(np.array([2.0, 2.0]), 0.5)
    assert (w.L, w.clipped) == (0.5, 2) and np.array_equal(w.beta, np.float32([0.125, 0.125]))


def test_reference_drops_an_overflow():
    big = np.float32(3.0e38)
    g = np.zeros(4, dtype=np.float32)
    X = np.array([[1.0, big, -1.0, 0.5]], dtype=np.float32)
    W = np.array([0.25, big, 0.0, -0.5], dtype=np.float32)
    U = np.array([1.0, 1.0, 1.0, 1.0], dtype=np.float32)
    w, u, dropped, hist = R.accumulate(X, g, np.float32([1.0]), W, U, 0.5)
    assert dropped == 1 and R.bits(w)[1] == 0 and R.bits(u)[1] == 0 and hist.sum() == 4
    assert np.array_equal(w, np.float32([1.75, 0.0, -0.5, 0.5])) and np.array_equal(u, np.float32([1.5, 0.0, -0.5, 1.0]))
