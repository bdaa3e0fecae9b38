"""Host: the FoolsGold defense's configuration rules and the properties of the CPU
restatement (tests/foolsgold_ref.py) that the GPU tests compare the kernels
with — the sybils' rejection on the generator's rows with and without memory,
the margins the GPU tests rely on, pardoning, zero rows, bad rows and identical
clients.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import foolsgold_ref as ref
from flr.defenses import FoolsGoldDefense, get_defense

# (K, P, f): the GPU tests' shapes
SHAPES = [(1, 5, 0), (2, 7, 0), (5, 7, 2), (8, 64, 2), (17, 333, 4), (33, 1027, 6), (65, 2048, 13),
          (130, 5000, 26), (300, 600, 60), (1024, 256, 100)]


def test_registry_and_defaults():
    d = get_defense("foolsgold", {})
    assert isinstance(d, FoolsGoldDefense)
    assert d.confidence == 1.0 and d.use_memory is True and d.calls == 0
    assert not d.supports_sharded and not d.order_free
    assert d.client_weights == [] and d.detect_malicious() == [] and d.history() is None
    m = d.get_metrics()
    assert m == {"defense_type": "foolsgold", "confidence": 1.0, "use_memory": True, "calls": 0, "weights": [],
                 "max_cosine": [], "no_update": False, "bad_rows": False}
    d = get_defense("foolsgold", {"confidence": 2, "use_memory": False})
    assert d.confidence == 2.0 and d.use_memory is False
    d.reset()
    d.set_center(torch.zeros(3))
    d.set_center(None)


@pytest.mark.parametrize("cfg", [
    {"confidence": 0}, {"confidence": -1.0}, {"confidence": float("nan")}, {"confidence": float("inf")},
    {"confidence": True}, {"confidence": "1"}, {"confidence": None},
    {"use_memory": 1}, {"use_memory": "yes"}, {"use_memory": None},
])
def test_invalid_config(cfg):
    with pytest.raises(ValueError):
        get_defense("foolsgold", cfg)


def test_size_rules_raise_before_device_work():
    d = get_defense("foolsgold", {})
    with pytest.raises(ValueError):
        d.aggregate([], [])
    with pytest.raises(ValueError):
        d.aggregate([[torch.zeros(1)]] * 1025, [])
    assert d.calls == 0 and d.history() is None


@functools.lru_cache(maxsize=None)
def _runs(K, P, f, kappa, use_memory):
    g, Xs = ref.rounds(K, P, f)
    return ref.run(g, Xs, kappa, use_memory)


@pytest.mark.parametrize("use_memory", [True, False])
@pytest.mark.parametrize("K,P,f", SHAPES)
def test_sybils_rejected(K, P, f, use_memory):
    """In each of three rounds every sybil gets alpha = 0.  From K = 8 up no
    finite pre-clip value kappa * (logit + 0.5) lies within 0.74 of 0 at kappa =
    1 (0.07 at kappa = 0.1), every honest client gets at least 0.95 at kappa = 1
    (exactly 1 from K = 17 up) and a fractional weight of at most 0.51 = 0.1 *
    (logit(0.99) + 0.5) at kappa = 0.1.  Below K = 8 (P = 7: random rows are
    not nearly orthogonal) only the margin the GPU tests need is asserted."""
    for kappa, bound in ((1.0, 0.74), (0.1, 0.07)):
        for out, wt, _ in _runs(K, P, f, kappa, use_memory):
            assert wt.flags == 0 and np.isfinite(out).all()
            assert (wt.alpha[:f] == 0).all()
            assert wt.margin > (bound if K >= 8 else 1e-6) and wt.top >= 0.1
            if kappa == 1.0 and K >= 8:
                assert (wt.alpha[f:] >= 0.95).all()
            if kappa == 1.0 and K >= 17:
                assert (wt.alpha[f:] == 1).all()
            if kappa == 0.1 and K >= 8:
                assert ((wt.alpha[f:] > 0.07) & (wt.alpha[f:] < 0.52)).all() and wt.alpha[f:].max() > 0.5
            assert abs(float(wt.beta.astype(np.float64).sum()) - 1.0) < 1e-5


def test_weights_by_hand():
    """Three unit rows at known angles, against the formulas worked by hand."""
    c = 0.5
    G = np.array([[1.0, c, 0.0], [c, 1.0, 0.0], [0.0, 0.0, 1.0]])
    wt = ref.weights(G, 1.0)
    assert np.array_equal(wt.max_cosine, [c, c, 0.0])
    # w = (0.5, 0.5, 1); top = 1; w2 = 0.99 (clipped): alpha = min(1, logit + 0.5)
    a = np.log(0.5 / 0.5) + 0.5
    assert np.allclose(wt.alpha, [a, a, 1.0], rtol=0, atol=1e-15) and wt.flags == 0
    assert wt.margin == pytest.approx(0.5) and wt.top == 1.0
    S = a + a + 1.0
    assert np.array_equal(wt.beta, (np.array([a, a, 1.0]) / S).astype(np.float32))
    # K = 1: the client is the aggregate
    one = ref.weights(np.array([[4.0]]), 0.1)
    assert one.alpha.tolist() == [1.0] and one.beta.tolist() == [1.0] and one.flags == 0


def test_pardoning_keeps_the_honest_lookalike():
    """Two sybils (cos 0.999 to each other), an honest client at cos 0.7 to them
    and four unrelated clients.  Without pardoning the lookalike would be cut
    (w = 1 - 0.7 = 0.3 of a top weight near 1: logit + 0.5 < 0); pardoning scales
    its cosines by v_h / v_s = 0.7 / 0.999, w = 1 - 0.49 = 0.51, and it keeps a
    positive weight while the sybils get 0."""
    rng = np.random.default_rng(0)
    P = 4000
    d = rng.standard_normal(P)
    d /= np.linalg.norm(d)

    def unit_at(cosine):
        r = rng.standard_normal(P)
        r -= (r @ d) * d
        r /= np.linalg.norm(r)
        return cosine * d + np.sqrt(1 - cosine ** 2) * r

    rows = [unit_at(0.9995), unit_at(0.9995), unit_at(0.7)] + [rng.standard_normal(P) for _ in range(4)]
    wt = ref.weights(ref.gram(np.stack(rows).astype(np.float32)), 1.0)
    v = wt.max_cosine
    assert v[0] > 0.998 and v[1] > 0.998 and 0.65 < v[2] < 0.75 and v[3:].max() < 0.1
    assert wt.alpha[0] == 0 and wt.alpha[1] == 0 and (wt.alpha[3:] == 1).all()
    plain = (1 - v[2]) / wt.top
    assert np.log(plain / (1 - plain)) + 0.5 < 0          # cut without pardoning
    pardoned = (1 - v[2] * v[2] / v[0]) / wt.top
    want = np.log(pardoned / (1 - pardoned)) + 0.5
    assert 0.3 < want < 1 and wt.alpha[2] == pytest.approx(want, abs=1e-12)


def test_zero_rows_and_bad_rows():
    g, Xs = ref.rounds(8, 64, 2)
    A = (Xs[0] - g[None, :]).astype(np.float32)
    A[5] = 0.0                       # a client that sent the global model back: cosine 0 with everyone
    wt = ref.weights(ref.gram(A), 1.0)
    assert wt.max_cosine[5] == 0.0 and wt.alpha[5] == 1.0 and wt.flags == 0
    assert (wt.alpha[:2] == 0).all()
    B = A.copy()
    B[3, 7] = np.nan
    B[6, 1] = np.inf
    wb = ref.weights(ref.gram(B), 1.0)
    assert wb.flags == 2 and wb.alpha[3] == 0 and wb.alpha[6] == 0 and wb.beta[3] == 0 and wb.beta[6] == 0
    assert wb.max_cosine[3] == 0 and wb.max_cosine[6] == 0
    assert np.isfinite(wb.alpha).all() and (wb.alpha[:2] == 0).all() and wb.alpha[4] > 0
    # the rejected rows are skipped: the aggregate stays finite
    X = g[None, :] + B
    assert np.isfinite(ref.combine(X, g, wb.beta)).all()
    # every row bad: no update
    B[:, 0] = np.nan
    wn = ref.weights(ref.gram(B), 1.0)
    assert wn.flags == 3 and (wn.alpha == 0).all() and (wn.beta == 0).all() and wn.top == -1.0
    assert np.array_equal(ref.combine(g[None, :] + B, g, wn.beta), g)


def test_identical_clients_give_no_update():
    """Six copies of one row whose squared norm is a perfect square (64 ones:
    n = 8, n * n = 64 exactly): every cosine is exactly 1, every w exactly 0."""
    A = np.ones((6, 64), dtype=np.float32)
    wt = ref.weights(ref.gram(A), 1.0)
    assert wt.flags == 1 and (wt.alpha == 0).all() and (wt.beta == 0).all() and wt.top == 0.0
    assert (wt.max_cosine == 1).all()
    g = np.random.default_rng(2).standard_normal(64).astype(np.float32)
    assert np.array_equal(ref.combine(g[None, :] + A, g, wt.beta), g)
