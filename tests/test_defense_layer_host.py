"""Host: what the defenses share — CenteredDefense's center order on a pure-torch
rule, the attributes the round engine and bench.py decide by for every registered
name, and the config range checks.  No GPU and no library call (the first-call
median of the center order needs the device: the three GPU center-order tests)."""
import math

import pytest
import torch

from flr.defenses import CenteredDefense, get_defense
from flr.defenses import _DEFENSES
from flr.defenses._config import int_in, real_in
from flr.matrix import ClientMatrix

K, P = 3, 10


class _Stub(CenteredDefense):
    """center + mean of (X - center): a rule that shows which center it was given."""
    max_clients = K

    def aggregate_flat(self, cm, num_examples, global_flat=None):
        if cm.K > self.max_clients:      # a size rule ahead of the center, as FoolsGold's
            raise ValueError(f"at most {self.max_clients} clients, got {cm.K}")
        return super().aggregate_flat(cm, num_examples, global_flat)

    def _rule(self, cm, num_examples, center):
        self.seen = center
        return center + (cm.X - center).mean(dim=0)


def _matrix(rows=K, seed=0):
    g = torch.Generator().manual_seed(seed)
    cm = ClientMatrix.empty(rows, [torch.Size([4]), torch.Size([2, 3])], "cpu")
    cm.X.copy_(torch.randn(rows, P, generator=g))
    return cm


def _want(cm, center):
    return center + (cm.X - center).mean(dim=0)


def test_center_order():
    d, cm = _Stub({}), _matrix()
    assert d.takes_global and not d.supports_sharded
    g, c = torch.arange(P, dtype=torch.float32), torch.full((P,), 7.0)
    d.set_center(c)
    out = d.aggregate_flat(cm, [], g)                 # a given global_flat beats set_center ...
    assert torch.equal(d.seen, g) and torch.equal(out, _want(cm, g))
    assert d._center is None                          # ... which that call has spent all the same
    d.set_center(c)
    out2 = d.aggregate_flat(cm, [])                   # set_center beats the previous result
    assert torch.equal(d.seen, c) and torch.equal(out2, _want(cm, c)) and not torch.equal(out2, _want(cm, out))
    out3 = d.aggregate_flat(cm, [])                   # consumed by exactly one call: now the previous result
    assert d.seen is out2 and torch.equal(out3, _want(cm, out2))
    d.set_center(c)
    d.set_center(None)                                # withdrawn
    d.aggregate_flat(cm, [])
    assert d.seen is out3


def test_center_forms_and_lengths():
    d, cm = _Stub({}), _matrix()
    params = [torch.arange(4, dtype=torch.float64), torch.arange(6, dtype=torch.int32).reshape(2, 3)]
    flat = torch.cat([p.reshape(-1).float() for p in params])
    d.set_center(params)                              # a parameter list is its flat float form
    assert d._center.dtype == torch.float32 and torch.equal(d._center, flat)
    a = d.aggregate_flat(cm, [])
    d.set_center(flat.reshape(2, 5))
    assert torch.equal(d.aggregate_flat(cm, []), a)
    # aggregate(): global_params flattened, the result an unflattened copy
    res = d.aggregate(cm, [], global_params=params)
    assert [tuple(t.shape) for t in res] == [(4,), (2, 3)]
    assert torch.equal(torch.cat([t.reshape(-1) for t in res]), a) and torch.equal(d._previous, a)
    assert res[0].data_ptr() != d._previous.data_ptr()
    for bad in (torch.zeros(P - 1), torch.zeros(P + 1), torch.zeros(0)):
        with pytest.raises(ValueError, match=rf"{bad.numel()} coordinates.* {P}\b"):
            d.aggregate_flat(cm, [], bad)
        d.set_center(bad)
        with pytest.raises(ValueError, match=rf"{bad.numel()} coordinates.* {P}\b"):
            d.aggregate_flat(cm, [])
        assert d._center is not None and d._center.numel() == bad.numel()   # a refused center is not spent
    d.set_center(None)


def test_center_of_a_coordinate_range():
    d, cm = _Stub({}), _matrix()
    c = torch.arange(P, dtype=torch.float32) * 1.5
    view = cm.X[:, 4:8]
    d.set_center(c)
    got = d._resolve_center(view, None, 4, P)
    assert torch.equal(got, c[4:8]) and got.is_contiguous() and got.dtype == torch.float32 and d._center is None
    part = torch.ones(4)
    d.set_center(c)
    assert torch.equal(d._resolve_center(view, part, 4, P), part)     # the given slice beats set_center
    d.set_center(torch.zeros(P - 1))                  # the whole model's length is checked, not the slice's
    with pytest.raises(ValueError, match=rf"{P - 1} coordinates.* {P}\b"):
        d._resolve_center(view, None, 4, P)
    d.set_center(None)
    with pytest.raises(ValueError, match=r"5 coordinates.* 4\b"):
        d._resolve_center(view, torch.zeros(5), 4, P)
    d._previous = part                                # the previous result of the same range
    assert d._resolve_center(view, None, 4, P) is part


def test_size_rule_before_the_center_keeps_it():
    d, c = _Stub({}), torch.full((P,), 2.0)
    d.set_center(c)
    with pytest.raises(ValueError, match="at most 3"):
        d.aggregate_flat(_matrix(rows=4), [])
    assert d._center is not None and d._previous is None
    cm = _matrix()
    assert torch.equal(d.aggregate_flat(cm, []), _want(cm, c)) and torch.equal(d.seen, c)


# (takes_global, supports_sharded, order_free) of every registered name, as the round engine decided them
# when it read takes_global off the signatures of aggregate_flat / aggregate_sharded
TABLE = {
    **{n: (False, True, True) for n in ("none", "fedavg", "krum", "multi_krum", "krum_trimmed_mean", "bulyan",
                                        "trimmed_mean", "median")},
    **{n: (False, False, False) for n in ("geometric_median", "dp_sgd", "gradient_clipping", "norm_bounding", "dnc")},
    **{n: (True, False, False) for n in ("fltrust", "centered_clipping", "foolsgold")},
    "robust_lr": (True, True, False),
}
KRUM_FAMILY = {"krum", "multi_krum", "krum_trimmed_mean", "bulyan"}   # the names with publish(), comm, tap_blocks


def test_engine_table():
    assert set(TABLE) == set(_DEFENSES)
    for name, want in TABLE.items():
        d = get_defense(name, {})
        assert (d.takes_global, bool(d.supports_sharded), bool(d.order_free)) == want, name
        assert isinstance(d, CenteredDefense) == (name in ("centered_clipping", "foolsgold", "robust_lr")), name
        # bench.py probes these with hasattr / getattr
        assert hasattr(d, "publish") == (name in KRUM_FAMILY), name
        for attr in ("comm", "tap_blocks", "pairwise_method"):
            assert hasattr(d, attr) == (name in KRUM_FAMILY), (name, attr)
        assert hasattr(d, "multi_k") == (name in KRUM_FAMILY), name
        assert bool(getattr(d, "supports_dead_rows", False)) == (name in ("krum", "multi_krum")), name
        assert bool(getattr(d, "needs_tap_blocks", False)) == (name in KRUM_FAMILY), name


NAN, INF = float("nan"), float("inf")


def _rejects(check, key, v):
    with pytest.raises(ValueError) as e:
        check({key: v})
    assert key in str(e.value) and repr(v) in str(e.value), (key, v, str(e.value))


def test_real_in():
    def tau(c):
        return real_in(c, "tau", 10.0, 0.0, finite=False, float32=True, or_else=" or 'median'")

    def server_lr(c):
        return real_in(c, "server_lr", 1.0, 0.0, float32=True)

    def confidence(c):
        return real_in(c, "confidence", 1.0, 0.0)

    def filter_frac(c):
        return real_in(c, "filter_frac", 1.0, 0.0, closed=True)

    assert tau({}) == 10.0 and tau({"tau": 2}) == 2.0 and isinstance(tau({"tau": 2}), float)
    assert tau({"tau": INF}) == INF and tau({"tau": 1e60}) == 1e60      # no finite=: an inf clips nothing
    for v in (0, 0.0, -1.0, NAN, "mean", None, True, 1e-60, [1.0], -INF):
        _rejects(tau, "tau", v)
    with pytest.raises(ValueError, match="median"):
        tau({"tau": None})
    assert server_lr({}) == 1.0 and server_lr({"server_lr": 0.5}) == 0.5 and server_lr({"server_lr": 3}) == 3.0
    for v in (0, 0.0, -1.0, NAN, INF, "1", None, True, 1e-60, 1e60, False, [2]):
        _rejects(server_lr, "server_lr", v)
    assert confidence({"confidence": 2}) == 2.0 and confidence({"confidence": 1e-60}) == 1e-60
    for v in (0, -1.0, NAN, INF, True, "1", None):
        _rejects(confidence, "confidence", v)
    assert filter_frac({"filter_frac": 0}) == 0.0 and filter_frac({"filter_frac": 1.5}) == 1.5
    for v in (-0.5, NAN, INF, "1", None, False):
        _rejects(filter_frac, "filter_frac", v)
    assert real_in({"x": 1.0}, "x", 0.5, 0.0, 1.0) == 1.0              # the upper bound is closed
    _rejects(lambda c: real_in(c, "x", 0.5, 0.0, 1.0), "x", 1.5)
    assert math.isclose(real_in({}, "x", 0.5, 0.0, 1.0), 0.5)


def test_int_in():
    def iters(c):
        return int_in(c, "iters", 3, 1)

    assert iters({}) == 3 and iters({"iters": 5}) == 5
    for v in (0, -2, 1.5, "3", None, True, NAN, INF, [1]):
        _rejects(iters, "iters", v)

    def niters(c):
        return int_in(c, "niters", 1, 1, 16)

    assert niters({"niters": 16}) == 16
    for v in (0, 17, 1.0):
        _rejects(niters, "niters", v)
    assert int_in({"seed": (1 << 64) - 1}, "seed", 0, -(1 << 63), (1 << 64) - 1) == (1 << 64) - 1
    _rejects(lambda c: int_in(c, "seed", 0, -(1 << 63), (1 << 64) - 1), "seed", 1 << 64)
