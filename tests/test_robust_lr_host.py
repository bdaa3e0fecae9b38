"""CPU: the robust learning rate's registry entry and config rules, the C
entries' argument rules (decided before any launch), and the properties of its
arithmetic (tests/robust_lr_ref.py, the restatement of include/flr.h) that the
GPU tests then hold the kernels to bit for bit: threshold 0 at server_lr 1 is
the base aggregate, negated updates negate the votes, and what the defense is
for — on the coordinates where only the attackers agree the result moves away
from them, where plain FedAvg follows them."""
import math

import pytest
import torch

from flr import _capi
from flr.defenses import RobustLRDefense, get_defense
from robust_lr_ref import fedavg, resolve_threshold, rlr_apply, rlr_fedavg, same_bits, sign_vote


def test_registry_and_config():
    d = get_defense("robust_lr", {})
    assert isinstance(d, RobustLRDefense)
    assert d.threshold == 0.25 and d.base == "fedavg" and d.server_lr == 1.0
    assert d.supports_sharded and not d.order_free
    assert "0.25" in repr(d) and "fedavg" in repr(d)
    d = get_defense("robust_lr", {"threshold": 7, "base": "median", "server_lr": 0.5})
    assert d.threshold == 7 and isinstance(d.threshold, int) and d.base == "median" and d.server_lr == 0.5
    d = get_defense("robust_lr", {"base": "trimmed_mean", "base_cfg": {"trim_ratio": 0.3}})
    assert d._base.trim_ratio == 0.3
    assert get_defense("robust_lr", {"threshold": 0}).threshold == 0
    for th in (-1, 0.0, 1.0, 1.5, -0.25, float("nan"), float("inf"), "3", None, True, False, [2]):
        with pytest.raises(ValueError, match="threshold"):
            get_defense("robust_lr", {"threshold": th})
    for base in ("krum", "", None, 3, "FedAvg"):
        with pytest.raises(ValueError, match="base"):
            get_defense("robust_lr", {"base": base})
    for lr in (0, 0.0, -1.0, float("nan"), float("inf"), "1", None, True, 1e-60, 1e60):
        with pytest.raises(ValueError, match="server_lr"):
            get_defense("robust_lr", {"server_lr": lr})
    with pytest.raises(ValueError, match="-3"):    # the offending value is in the message
        get_defense("robust_lr", {"threshold": -3})
    m = get_defense("robust_lr", {"threshold": 0.4}).get_metrics()
    assert set(m) == {"defense_type", "threshold", "base", "server_lr", "flipped", "flipped_fraction"}
    assert m["defense_type"] == "robust_lr" and m["threshold"] == 0.4 and m["flipped"] is None
    assert d.detect_malicious() == [] and d.votes() is None


def test_threshold_resolution():
    d = get_defense("robust_lr", {})
    assert [d.resolve_threshold(K) for K in (1, 4, 5, 8, 128)] == [1, 1, 2, 2, 32]
    for K in (1, 4, 5, 8, 128):
        assert d.resolve_threshold(K) == resolve_threshold(0.25, K) == math.ceil(0.25 * K)
    d = get_defense("robust_lr", {"threshold": 6})
    assert d.resolve_threshold(6) == 6 and d.resolve_threshold(10) == 6
    with pytest.raises(ValueError, match="6"):
        d.resolve_threshold(5)          # an int is checked against K at the call
    assert get_defense("robust_lr", {"threshold": 0.999}).resolve_threshold(3) == 3


def test_c_entries_validate_without_gpu():
    """Every argument rule is decided before a launch or a write."""
    lib = _capi.lib()
    A, U = _capi.FLR_ERR_ARG, _capi.FLR_ERR_UNSUPPORTED
    x, n, g, o, v = 4096, 8192, 12288, 16384, 20480     # never dereferenced: the calls fail first
    nan, inf = float("nan"), float("inf")
    vote = lib.flr_sign_vote
    for args in ((None, 8, 10, 10, g, v), (x, 8, 10, 10, None, v), (x, 8, 10, 10, g, None), (x, 0, 10, 10, g, v),
                 (x, 8, -1, 10, g, v), (x, 8, 10, 9, g, v)):
        assert vote(*args, None) == A, args
    assert vote(x, 4097, 10, 10, g, v, None) == U
    assert vote(x, 8, 0, 0, g, v, None) == _capi.FLR_OK       # P == 0: nothing to do
    apply_ = lib.flr_rlr_apply
    for args in ((None, g, v, 10, 2, 1.0, o), (x, None, v, 10, 2, 1.0, o), (x, g, None, 10, 2, 1.0, o),
                 (x, g, v, 10, 2, 1.0, None), (x, g, v, -1, 2, 1.0, o), (x, g, v, 10, -1, 1.0, o),
                 (x, g, v, 10, 2, 0.0, o), (x, g, v, 10, 2, -1.0, o), (x, g, v, 10, 2, nan, o),
                 (x, g, v, 10, 2, inf, o), (x, g, v, 10, 2, 1.0, g)):
        assert apply_(*args, None, None) == A, args
    assert apply_(x, g, v, 0, 2, 1.0, o, None, None) == _capi.FLR_OK
    fused = lib.flr_rlr_fedavg
    for args in ((None, 8, 10, 10, n, g, 2, 1.0, o), (x, 8, 10, 10, None, g, 2, 1.0, o),
                 (x, 8, 10, 10, n, None, 2, 1.0, o), (x, 8, 10, 10, n, g, 2, 1.0, None),
                 (x, 0, 10, 10, n, g, 0, 1.0, o), (x, 8, -1, 10, n, g, 2, 1.0, o), (x, 8, 10, 9, n, g, 2, 1.0, o),
                 (x, 8, 10, 10, n, g, -1, 1.0, o), (x, 8, 10, 10, n, g, 9, 1.0, o), (x, 8, 10, 10, n, g, 2, 0.0, o),
                 (x, 8, 10, 10, n, g, 2, nan, o), (x, 8, 10, 10, n, g, 2, -inf, o), (x, 8, 10, 10, n, g, 2, 1.0, g)):
        assert fused(*args, None, None, None) == A, args
    assert fused(x, 4097, 10, 10, n, g, 2, 1.0, o, None, None, None) == U
    assert fused(x, 8, 0, 0, n, g, 2, 1.0, o, None, None, None) == _capi.FLR_OK


def _scenario(seed, K=20, P=64, f=4):
    torch.manual_seed(seed)
    g = torch.randn(P)
    X = g + 0.05 * torch.randn(K, P)
    n = [3 + (k % 5) for k in range(K)]
    return X, g, n, f


def test_threshold_zero_is_the_base_aggregate():
    X, g, n, _ = _scenario(1)
    agg = fedavg(X, n)
    out, votes, flipped = rlr_fedavg(X, n, g, 0, 1.0)
    assert same_bits(out, agg) and flipped == 0
    assert int(votes.abs().max()) <= X.shape[0]
    med = torch.median(X, dim=0).values
    out, flipped = rlr_apply(med, g, votes, 0, 1.0)
    assert same_bits(out, med) and flipped == 0
    # a server_lr below 1 shortens the step instead
    out, _ = rlr_apply(agg, g, votes, 0, 0.5)
    assert same_bits(out, g + torch.tensor(0.5) * (agg - g)) and not same_bits(out, agg)


def test_negated_updates_negate_the_votes():
    X, g, _, _ = _scenario(2)
    votes = sign_vote(X, g)
    mirrored = g - (X - g)          # every update negated around g
    assert ((X > g) == (mirrored < g)).all() and ((X < g) == (mirrored > g)).all()   # no update rounds to 0
    assert torch.equal(sign_vote(mirrored, g), -votes) and votes.abs().max() > 0


def test_vote_edge_values():
    nan, inf = float("nan"), float("inf")
    g = torch.tensor([0.0, -0.0, 1.0, nan, 2.0, inf, -inf, 0.0])
    X = torch.tensor([[-0.0, 0.0, nan, 1.0, inf, inf, -inf, 1e-45],
                      [0.0, -0.0, 3.0, 5.0, -inf, 1.0, 1.0, 0.0]])
    # -0 against +0; a NaN on either side; +-inf by its sign; inf against itself; a denormal counts
    assert sign_vote(X, g).tolist() == [0, 0, 1, 0, 0, -1, 1, 1]


def test_backdoor_block_is_reversed():
    """K = 20, f = 4.  On the first 16 coordinates the attackers all move +delta
    and the 16 honest clients are split evenly, eight each way by the same small
    amount: the net vote there is f, under threshold f + 1, and the result lies
    on the negative side of g where plain FedAvg lies on the positive side.  On
    the other coordinates everybody agrees and the two results are one."""
    torch.manual_seed(3)
    K, P, f, B, delta = 20, 64, 4, 16, 0.5
    g = torch.randn(P)
    step = 0.01 + 0.01 * torch.rand(P)
    X = g.repeat(K, 1)
    honest = torch.arange(f, K)
    X[honest[0::2], :B] += step[:B]
    X[honest[1::2], :B] -= step[:B]
    X[:f, :B] += delta
    X[:, B:] += step[B:] * (1 + torch.rand(K, 1))       # a common direction
    n = [10] * K
    plain = fedavg(X, n)
    out, votes, flipped = rlr_fedavg(X, n, g, f + 1, 1.0)
    assert (votes[:B] == f).all() and (votes[B:] == K).all() and flipped == B
    assert (plain[:B] > g[:B]).all() and (out[:B] < g[:B]).all()
    assert same_bits(out[B:], plain[B:])
    # at threshold f the vote passes and the backdoor goes through: the threshold must exceed f
    assert same_bits(rlr_fedavg(X, n, g, f, 1.0)[0], plain)
