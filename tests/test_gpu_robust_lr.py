"""GPU: the robust learning rate (flr_sign_vote, flr_rlr_apply, flr_rlr_fedavg,
their ops wrappers, RobustLRDefense, the round engine's defense="robust_lr")
against the CPU restatement of tests/robust_lr_ref.py.  Every comparison is
exact — the votes and the flip counts as integers, the vectors bit for bit —
because nothing here has a free summation order.  Where a test needs both
branches of the rule it first asserts on the reference that some but not all
coordinates are flipped, so a bad seed fails there and not as a kernel bug (the
seeds below were checked on the CPU)."""
import functools

import pytest
import torch

from flr import _capi, ops
from flr.defenses import get_defense
from flr.matrix import ClientMatrix
from flr.models.multimodal import TINY
from flr.round import RoundConfig, RoundEngine
from flr.train import TrainConfig
from robust_lr_ref import fedavg, rlr_apply, rlr_fedavg, same_bits, sign_vote

pytestmark = pytest.mark.gpu

# (K, P, ldx - P): one client; one column; ldx % 4 != 0, the one-coordinate form;
# the float4 form over several workgroups; the float4 form with a 3-coordinate
# tail and K no multiple of 16; many rows
SHAPES = [(1, 5, 3), (2, 1, 3), (5, 7, 2), (16, 5000, 24), (33, 1027, 1), (130, 300, 0)]
# per shape, a seed at which the reference flips some but not all coordinates at
# the even-coordinate consensus threshold, with and without the planted values
SEEDS = {(1, 5, 3): 0, (2, 1, 3): 0, (5, 7, 2): 0, (16, 5000, 24): 0, (33, 1027, 1): 0, (130, 300, 0): 0}
ETAS = (1.0, 0.5)
FILL = -77.0  # the padding columns' content


def _thresholds(K):
    """0 (nothing flips), 1, K, and the even coordinates' consensus: the K - K//5
    - 1 honest rows off g against the K//5 attackers."""
    return sorted({0, 1, K} | ({K - 2 * (K // 5) - 1} if K - 2 * (K // 5) - 1 >= 1 else set()))


def _examples(K):
    return [1 + (3 * k) % 7 for k in range(K)]


@functools.lru_cache(maxsize=None)
def _inputs(K, P, pad, bad=False):
    """The padded CPU matrix [K, P + pad] and g.  On even coordinates the honest
    rows all move one way, g + s_p |0.05 randn|; on odd coordinates each its own
    way, g + 0.05 randn; the first K // 5 rows are g - 3 (their honest
    displacement); the last row is g itself when there is more than one, so every
    coordinate has a tie.  bad: a NaN, a +inf and a -inf in two rows, a NaN in g,
    and -0 in two rows against a +0 in g."""
    torch.manual_seed(SEEDS[(K, P, pad)])
    g = torch.randn(P)
    disp = 0.05 * torch.randn(K, P)
    s = torch.where(torch.rand(P) < 0.5, -1.0, 1.0)
    disp[:, 0::2] = s[0::2] * disp[:, 0::2].abs()
    X = g + disp
    nmal = K // 5
    X[:nmal] = g - 3.0 * disp[:nmal]
    if K >= 2:
        X[K - 1] = g
    if bad:
        g = g.clone()
        X[5, P // 3] = float("nan")
        X[9, P // 2] = float("inf")
        X[9, P // 5] = float("-inf")
        g[P // 7] = float("nan")
        g[7] = 0.0
        X[3, 7] = X[4, 7] = -0.0
        X[K - 1, 7] = 0.0
    data = torch.full((K, P + pad), FILL)
    data[:, :P] = X
    return data, g


@functools.lru_cache(maxsize=None)
def _ref(K, P, pad, bad=False):
    """The reference's (FedAvg aggregate, votes), computed once."""
    data, g = _inputs(K, P, pad, bad)
    X = data[:, :P].contiguous()
    return fedavg(X, _examples(K)), sign_vote(X, g)


@functools.lru_cache(maxsize=None)
def _ref_out(K, P, pad, bad, theta, eta):
    agg, votes = _ref(K, P, pad, bad)
    return rlr_apply(agg, _inputs(K, P, pad, bad)[1], votes, theta, eta)


def _offset(t, device):
    """t on the device at a 4-byte offset from an aligned allocation: the
    one-coordinate form."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    buf[1:].copy_(t)
    return buf[1:]


def _assert_untouched(Dg, data):
    """The padding columns keep their fill and X is only read."""
    Dc = Dg.cpu()
    assert torch.equal(Dc.isnan(), data.isnan())
    assert torch.equal(Dc.nan_to_num(), data.nan_to_num())


CASES = [(K, P, pad, False) for K, P, pad in SHAPES] + [(16, 5000, 24, True), (33, 1027, 1, True)]


def test_reference_has_both_branches():
    """At the consensus threshold the reference flips some coordinates (odd ones)
    and keeps others (the even ones), for every shape with K >= 5 and P >= 7."""
    for K, P, pad, bad in CASES:
        if K < 5 or P < 7:
            continue
        theta = K - 2 * (K // 5) - 1
        assert theta in _thresholds(K)
        flipped = _ref_out(K, P, pad, bad, theta, 1.0)[1]
        print((K, P, pad, bad), "theta", theta, "flipped", flipped)
        assert 0 < flipped < P
        votes = _ref(K, P, pad, bad)[1]
        assert int(votes.abs().max()) <= K - 1      # the last row ties everywhere


@pytest.mark.parametrize("K,P,pad,bad", CASES)
def test_sign_vote(cuda, K, P, pad, bad):
    data, g = _inputs(K, P, pad, bad)
    want = _ref(K, P, pad, bad)[1]
    Dg = data.to(cuda)
    got = ops.sign_vote(Dg[:, :P], g.to(cuda))
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    # the one-coordinate form: g and votes at a 4-byte offset
    out = _offset(torch.full((P,), 99, dtype=torch.int32), cuda)
    assert ops.sign_vote(Dg[:, :P], _offset(g, cuda), out=out) is out
    assert torch.equal(out.cpu(), want)
    _assert_untouched(Dg, data)
    if bad:   # the NaN in g votes 0; the -0 rows and the +0 row tie with the +0 in g
        others = [k for k in range(K) if k not in (3, 4, K - 1)]
        assert want[P // 7] == 0 and want[7] == sum(int(data[k, 7] > 0) - int(data[k, 7] < 0) for k in others)


@pytest.mark.parametrize("K,P,pad,bad", CASES)
def test_rlr_apply(cuda, K, P, pad, bad):
    _, g = _inputs(K, P, pad, bad)
    agg, votes = _ref(K, P, pad, bad)
    gg, ag, vg = g.to(cuda), agg.to(cuda), votes.to(cuda)
    for theta in _thresholds(K):
        for eta in ETAS:
            want, nflip = _ref_out(K, P, pad, bad, theta, eta)
            out, flipped = ops.rlr_apply(ag, gg, vg, theta, eta, count=True)
            assert same_bits(out, want), (theta, eta)
            assert flipped.dtype == torch.int64 and flipped.item() == nflip
            assert same_bits(ops.rlr_apply(ag, gg, vg, theta, eta), want)      # without the counter
            inplace = ag.clone()
            assert ops.rlr_apply(inplace, gg, vg, theta, eta, out=inplace) is inplace
            assert same_bits(inplace, want)
            # the one-coordinate form
            out1, flipped1 = ops.rlr_apply(_offset(agg, cuda), gg, vg, theta, eta, count=True)
            assert same_bits(out1, want) and flipped1.item() == nflip
    assert same_bits(ag, agg) and same_bits(gg, g) and torch.equal(vg.cpu(), votes)   # inputs only read


@pytest.mark.parametrize("K,P,pad,bad", CASES)
def test_rlr_fedavg(cuda, K, P, pad, bad):
    data, g = _inputs(K, P, pad, bad)
    n = _examples(K)
    votes_ref = _ref(K, P, pad, bad)[1]
    Dg, gg = data.to(cuda), g.to(cuda)
    X = Dg[:, :P]
    for theta in _thresholds(K):
        for eta in ETAS:
            want, nflip = _ref_out(K, P, pad, bad, theta, eta)
            out, votes, flipped = ops.rlr_fedavg(X, n, gg, theta, eta, diagnostics=True)
            assert same_bits(out, want), (theta, eta)
            assert torch.equal(votes.cpu(), votes_ref) and flipped.item() == nflip
            assert same_bits(ops.rlr_fedavg(X, n, gg, theta, eta), want)        # without the optional outputs
            # the composition of the three calls on the device
            comp, cflip = ops.rlr_apply(ops.fedavg(X, n), gg, ops.sign_vote(X, gg), theta, eta, count=True)
            assert same_bits(out, comp) and cflip.item() == nflip
            # the one-coordinate form
            out1, votes1, flipped1 = ops.rlr_fedavg(X, n, _offset(g, cuda), theta, eta, diagnostics=True)
            assert same_bits(out1, want) and torch.equal(votes1.cpu(), votes_ref) and flipped1.item() == nflip
    _assert_untouched(Dg, data)


@pytest.mark.parametrize("K,P,pad,bad", CASES)
def test_threshold_zero_is_fedavg(cuda, K, P, pad, bad):
    data, g = _inputs(K, P, pad, bad)
    n = _examples(K)
    X = data.to(cuda)[:, :P]
    out, _, flipped = ops.rlr_fedavg(X, n, g.to(cuda), 0, 1.0, diagnostics=True)
    plain = ops.fedavg(X, n)
    assert flipped.item() == 0 and same_bits(out, plain)
    if not bad:
        assert torch.equal(out, plain)
    assert same_bits(plain, _ref(K, P, pad, bad)[0])


def test_argument_errors_leave_outputs_alone(cuda):
    K, P, ld = 6, 40, 48
    torch.manual_seed(3)
    D = torch.randn(K, ld).to(cuda)
    g = torch.randn(P).to(cuda)
    agg = torch.randn(P).to(cuda)
    n = torch.arange(1, K + 1, dtype=torch.int64, device=cuda)
    out = torch.full((P,), FILL, device=cuda)
    votes = torch.full((P,), -77, dtype=torch.int32, device=cuda)
    flipped = torch.full((1,), -77, dtype=torch.int64, device=cuda)
    lib = _capi.lib()
    x, gp, ap, np_, o, v, fl = (t.data_ptr() for t in (D, g, agg, n, out, votes, flipped))
    nan, inf = float("nan"), float("inf")
    A, U = _capi.FLR_ERR_ARG, _capi.FLR_ERR_UNSUPPORTED
    for args, code in [((None, K, P, ld, gp, v), A), ((x, K, P, ld, None, v), A), ((x, K, P, ld, gp, None), A),
                       ((x, 0, P, ld, gp, v), A), ((x, -1, P, ld, gp, v), A), ((x, K, -1, ld, gp, v), A),
                       ((x, K, P, P - 1, gp, v), A), ((x, 4097, P, ld, gp, v), U)]:
        assert lib.flr_sign_vote(*args, None) == code, args
    for args in [(None, gp, v, P, 2, 1.0, o), (ap, None, v, P, 2, 1.0, o), (ap, gp, None, P, 2, 1.0, o),
                 (ap, gp, v, P, 2, 1.0, None), (ap, gp, v, -1, 2, 1.0, o), (ap, gp, v, P, -1, 1.0, o),
                 (ap, gp, v, P, 2, 0.0, o), (ap, gp, v, P, 2, -0.5, o), (ap, gp, v, P, 2, nan, o),
                 (ap, gp, v, P, 2, inf, o), (ap, gp, v, P, 2, 1.0, gp)]:
        assert lib.flr_rlr_apply(*args, fl, None) == A, args
    for args, code in [((None, K, P, ld, np_, gp, 2, 1.0, o), A), ((x, K, P, ld, None, gp, 2, 1.0, o), A),
                       ((x, K, P, ld, np_, None, 2, 1.0, o), A), ((x, K, P, ld, np_, gp, 2, 1.0, None), A),
                       ((x, 0, P, ld, np_, gp, 0, 1.0, o), A), ((x, K, -1, ld, np_, gp, 2, 1.0, o), A),
                       ((x, K, P, P - 1, np_, gp, 2, 1.0, o), A), ((x, K, P, ld, np_, gp, -1, 1.0, o), A),
                       ((x, K, P, ld, np_, gp, K + 1, 1.0, o), A), ((x, K, P, ld, np_, gp, 2, 0.0, o), A),
                       ((x, K, P, ld, np_, gp, 2, nan, o), A), ((x, K, P, ld, np_, gp, 2, inf, o), A),
                       ((x, K, P, ld, np_, gp, 2, 1.0, gp), A), ((x, 4097, P, ld, np_, gp, 2, 1.0, o), U)]:
        assert lib.flr_rlr_fedavg(*args, v, fl, None) == code, args
    torch.cuda.synchronize()
    g_before = g.clone()
    assert (out.cpu() == FILL).all() and (votes.cpu() == -77).all() and flipped.item() == -77
    # P == 0: FLR_OK, flipped = 0, nothing else written
    assert lib.flr_sign_vote(x, K, 0, ld, gp, v, None) == _capi.FLR_OK
    assert lib.flr_rlr_apply(ap, gp, v, 0, 2, 1.0, o, fl, None) == _capi.FLR_OK
    assert flipped.item() == 0
    flipped.fill_(-77)
    assert lib.flr_rlr_fedavg(x, K, 0, ld, np_, gp, 2, 1.0, o, v, fl, None) == _capi.FLR_OK
    assert flipped.item() == 0 and (out.cpu() == FILL).all() and (votes.cpu() == -77).all()
    # the tensor wrappers
    with pytest.raises(_capi.FlrError) as e:
        ops.rlr_fedavg(D[:, :P], n, g, 2, out=g)
    assert e.value.status == A
    with pytest.raises(_capi.FlrError) as e:
        ops.rlr_apply(agg, g, votes, 2, out=g)
    assert e.value.status == A
    for kw in (dict(theta=-1), dict(theta=K + 1), dict(theta=2, eta=0.0), dict(theta=2, eta=nan), dict(theta=2, eta=inf)):
        with pytest.raises(ValueError):
            ops.rlr_fedavg(D[:, :P], n, g, **kw)
    with pytest.raises(ValueError):
        ops.rlr_fedavg(D[:, :P], n[:-1], g, 2)
    with pytest.raises(ValueError):
        ops.sign_vote(D[:, :P], g[:-1].contiguous())
    with pytest.raises(ValueError):
        ops.sign_vote(D[:, :P], g.double())
    with pytest.raises(ValueError):
        ops.sign_vote(D[:, :P], g, out=torch.empty(P, device=cuda))          # not int32
    with pytest.raises(ValueError):
        ops.rlr_apply(agg, g, votes.long(), 2)
    with pytest.raises(ValueError):
        ops.rlr_apply(agg, g.cpu(), votes, 2)
    with pytest.raises(RuntimeError):
        ops.rlr_apply(agg.cpu(), g, votes, 2)
    assert torch.equal(g, g_before)


@pytest.mark.parametrize("base", ["fedavg", "median", "trimmed_mean"])
def test_defense_two_calls(cuda, base):
    """Each base over two consecutive calls: the first centred on the rows' lower
    median, the second on the first call's result; then set_center and
    global_params, as CenteredClippingDefense resolves them."""
    K, P, pad = 33, 1027, 1
    data, g = _inputs(K, P, pad)
    X = data[:, :P].contiguous()
    n = _examples(K)
    theta, eta = 9, 0.5
    d = get_defense("robust_lr", {"threshold": theta, "base": base, "server_lr": eta,
                                  "base_cfg": {"trim_ratio": 0.2} if base == "trimmed_mean" else {}})
    cm = ClientMatrix.from_updates([[X[k].clone()] for k in range(K)], device=cuda)

    def base_agg():
        if base == "fedavg":
            return fedavg(X, n)
        if base == "median":
            return torch.median(X, dim=0).values
        return ops.trimmed_mean(cm.X, max(1, int(K * 0.2))).cpu()   # the base's own kernel (tested elsewhere)

    def ref(center):
        votes = sign_vote(X, center)
        out, nflip = rlr_apply(base_agg(), center, votes, theta, eta)
        return out, votes, nflip

    r1 = ref(torch.median(X, dim=0).values)
    got1 = d.aggregate_flat(cm, n)
    assert same_bits(got1, r1[0]) and torch.equal(d.votes().cpu(), r1[1])
    m = d.get_metrics()
    assert m == {"defense_type": "robust_lr", "threshold": theta, "base": base, "server_lr": eta,
                 "flipped": r1[2], "flipped_fraction": r1[2] / P}
    r2 = ref(r1[0])
    got2 = d.aggregate(cm, n)
    assert got2[0].is_cuda and same_bits(got2[0].reshape(-1), r2[0])
    if base != "median":   # the median of the rows, centred on itself, stays where it is
        assert not same_bits(r2[0], r1[0])
    assert d.get_metrics()["flipped"] == r2[2]
    got2[0].zero_()      # the caller's copy is its own
    r3 = ref(g)
    assert 0 < r3[2] < P     # both branches of the rule
    d.set_center(g)
    assert same_bits(d.aggregate_flat(cm, n), r3[0])
    r4 = ref(r3[0])
    assert same_bits(d.aggregate_flat(cm, n), r4[0])
    c = g + 0.01
    d.set_center(g)
    assert same_bits(d.aggregate(cm, n, global_params=[c])[0].reshape(-1), ref(c)[0])
    with pytest.raises(ValueError):
        d.aggregate_flat(cm, n, global_flat=g[:-1].to(cuda))
    assert d.detect_malicious() == []
    with pytest.raises(ValueError, match="40"):
        get_defense("robust_lr", {"threshold": 40}).aggregate_flat(cm, n)     # an int above K, at the call


def test_float_threshold_and_default(cuda):
    K, P, pad = 16, 5000, 24
    data, g = _inputs(K, P, pad)
    cm = ClientMatrix.from_updates([[data[k, :P].clone()] for k in range(K)], device=cuda)
    d = get_defense("robust_lr", {})
    got = d.aggregate_flat(cm, _examples(K), global_flat=g.to(cuda))
    want, nflip = _ref_out(K, P, pad, False, 4, 1.0)       # ceil(0.25 * 16)
    assert same_bits(got, want)
    assert d.get_metrics()["threshold"] == 4 and d.get_metrics()["flipped"] == nflip


ENGINE_SEED = 42


def test_engine_round(cuda):
    """TINY, K = 8, f = 2, the backdoor: one round with the all-gather exchange
    and one with the all-to-all exchange at world 1 give the same bits, the
    reference applied to the engine's client matrix and the pre-round global
    model, at the engine's default threshold f + 1."""
    kw = dict(num_clients=8, batch=4, defense="robust_lr", attack="backdoor", num_attackers=2, seed=ENGINE_SEED)
    got = {}
    for exchange in ("allgather", "alltoall"):
        eng = RoundEngine(TINY, RoundConfig(exchange=exchange, **kw), TrainConfig(local_steps=2), cuda)
        assert eng.exchange == exchange and not eng.train_order and not eng.dead_deferred
        assert eng.defense.threshold == 3
        g0 = eng.global_flat.clone().cpu()
        g1 = eng.run_round().clone().cpu()
        X = (eng.full.X if exchange == "allgather" else eng.slice.X).cpu().contiguous()
        want, votes, nflip = rlr_fedavg(X, eng.num_examples, g0, 3, 1.0)
        print(exchange, "flipped", nflip, "of", X.shape[1])
        assert 0 < nflip < X.shape[1]
        assert same_bits(g1, want) and not same_bits(g1, g0)
        assert torch.equal(eng.defense.votes().cpu(), votes)
        assert eng.defense.get_metrics()["flipped"] == nflip
        assert not eng.fell_back
        got[exchange] = g1
    assert same_bits(got["allgather"], got["alltoall"])
    assert RoundEngine(TINY, RoundConfig(**kw), TrainConfig(local_steps=2), cuda).exchange == "alltoall"
