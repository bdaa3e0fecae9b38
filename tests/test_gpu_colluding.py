"""GPU: the colluding attacks (flr_collude_rows, flr.attacks.alie_ / ipm_, the
round engine's attack="alie" / "ipm") against the torch-CPU restatement of
tests/colluding_ref.py — bit for bit (torch.equal): the kernel's arithmetic is
fixed op for op, so nothing here has a tolerance."""
import functools

import pytest
import torch

from colluding_ref import ALIE, IPM, collude
from flr import _capi, ops
from flr.attacks import alie_, alie_z, ipm_
from flr.matrix import ClientMatrix
from flr.models.multimodal import TINY
from flr.round import RoundConfig, RoundEngine
from flr.train import TrainConfig

pytestmark = pytest.mark.gpu

# (K, nmal, P, ldx - P): nb = 1 (sigma exactly 0); one column; padded rows over
# several workgroups; a partial group of the 32-row form; nb = 128, the register
# form's limit; nb = 129, the streaming form; the streaming form with a tail
SHAPES = [(3, 2, 5, 3), (7, 2, 1, 3), (16, 3, 5000, 24), (33, 8, 257, 3), (129, 1, 300, 3), (130, 1, 300, 3),
          (140, 12, 777, 3)]
PARAM = {ALIE: 0.48877614, IPM: 0.5}
FILL = -77.0  # the padding columns' content


@functools.lru_cache(maxsize=None)
def _case(K, nmal, P, pad):
    """The padded CPU matrix [K, P + pad] (made once) and, per mode, the
    reference's (matrix, mu, sigma) on its [K, P] part."""
    torch.manual_seed(1000 * K + P)
    data = torch.full((K, P + pad), FILL)
    data[:, :P] = torch.randn(P) + 0.05 * torch.randn(K, P)
    return data, {m: collude(data[:, :P].contiguous(), nmal, m, PARAM[m]) for m in (ALIE, IPM)}


@pytest.mark.parametrize("mode", [ALIE, IPM], ids=["alie", "ipm"])
@pytest.mark.parametrize("K,nmal,P,pad", SHAPES)
def test_kernel_bitwise(cuda, K, nmal, P, pad, mode):
    data, refs = _case(K, nmal, P, pad)
    want, mu, sigma = refs[mode]
    if K - nmal == 1:
        assert not sigma.any()
    D = data.to(cuda)
    mean_out = torch.full((P,), 5.0, device=cuda)
    std_out = torch.full((P,), 5.0, device=cuda)
    ops.collude_rows(D[:, :P], nmal, mode, PARAM[mode], mean_out, std_out)
    got = D.cpu()
    assert torch.equal(got[:nmal, :P], want[:nmal])          # the attackers' rows
    assert torch.equal(got[nmal:, :P], data[nmal:, :P])      # the benign rows
    assert torch.equal(got[:, P:], data[:, P:])              # the padding columns
    assert torch.equal(mean_out.cpu(), mu)
    assert torch.equal(std_out.cpu(), sigma)
    # without the optional outputs (IPM then skips sigma: the one-pass form)
    D2 = data.to(cuda)
    ops.collude_rows(D2[:, :P], nmal, mode, PARAM[mode])
    assert torch.equal(D2.cpu(), got)


def test_column_split_equals_whole(cuda):
    """The sharded exchange's property: the two column ranges [0, p0) and
    [p0, P) as views of the same matrix (same ldx) give the whole result."""
    K, nmal, P, pad = 16, 3, 5000, 24
    data, refs = _case(K, nmal, P, pad)
    p0 = 1237
    for mode in (ALIE, IPM):
        want, mu, sigma = refs[mode]
        D = data.to(cuda)
        mean_out, std_out = torch.empty(P, device=cuda), torch.empty(P, device=cuda)
        for a, b in ((0, p0), (p0, P)):
            ops.collude_rows(D[:, a:b], nmal, mode, PARAM[mode], mean_out[a:b], std_out[a:b])
        got = D.cpu()
        assert torch.equal(got[:, :P], want) and torch.equal(got[:, P:], data[:, P:])
        assert torch.equal(mean_out.cpu(), mu) and torch.equal(std_out.cpu(), sigma)


@pytest.mark.parametrize("K,nmal,P,pad", [(16, 3, 5000, 24), (140, 12, 777, 3)])
def test_one_nan_poisons_one_column(cuda, K, nmal, P, pad):
    data, refs = _case(K, nmal, P, pad)
    c = P // 3
    bad = data.clone()
    bad[nmal + 2, c] = float("nan")
    keep = [i for i in range(P) if i != c]
    for mode in (ALIE, IPM):
        D = bad.to(cuda)
        ops.collude_rows(D[:, :P], nmal, mode, PARAM[mode])
        got = D.cpu()
        assert torch.isnan(got[:nmal, c]).all()
        assert torch.equal(got[:, keep], refs[mode][0][:, keep])
        assert torch.equal(got[nmal:, :P].isnan(), bad[nmal:, :P].isnan()) and torch.equal(got[:, P:], data[:, P:])


def test_argument_errors_leave_x_alone(cuda):
    K, P, ld = 6, 40, 48
    torch.manual_seed(3)
    data = torch.randn(K, ld)
    D = data.to(cuda)
    fn = _capi.lib().flr_collude_rows
    x = D.data_ptr()
    bad = [(None, K, P, ld, 2, 0),      # null X
           (x, 1, P, ld, 1, 0),         # K < 2
           (x, K, P, ld, 0, 0),         # nmal < 1
           (x, K, P, ld, -1, 0),
           (x, K, P, ld, K, 0),         # nmal >= K
           (x, K, P, ld, K + 1, 1),
           (x, K, 0, ld, 2, 0),         # P < 1
           (x, K, -3, ld, 2, 1),
           (x, K, P, P - 1, 2, 0),      # ldx < P
           (x, K, P, ld, 2, 2),         # mode outside {0, 1}
           (x, K, P, ld, 2, -1)]
    for X, k, p, l, nmal, mode in bad:
        assert fn(X, k, p, l, nmal, mode, 0.5, None, None, None) == _capi.FLR_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(D.cpu(), data)
    with pytest.raises(_capi.FlrError) as e:
        ops.collude_rows(D[:, :P], 2, 7, 0.5)
    assert e.value.status == _capi.FLR_ERR_ARG


def test_attacks_api(cuda):
    """alie_ / ipm_ on a tensor and on a ClientMatrix: in place, None back,
    z = alie_z(K, f) by default, f outside [1, K) a ValueError."""
    K, nmal, P, pad = 16, 3, 5000, 24
    data, refs = _case(K, nmal, P, pad)
    z = alie_z(K, nmal)
    want = collude(data[:, :P].contiguous(), nmal, ALIE, z)[0]
    D = data.to(cuda)
    assert alie_(D[:, :P], nmal) is None
    assert torch.equal(D.cpu()[:, :P], want)
    cm = ClientMatrix(data.to(cuda), P, [torch.Size([P])])
    assert alie_(cm, nmal, z=PARAM[ALIE]) is None
    assert torch.equal(cm.X.cpu(), refs[ALIE][0])
    cm = ClientMatrix(data.to(cuda), P, [torch.Size([P])])
    assert ipm_(cm, nmal) is None   # epsilon = 0.5
    assert torch.equal(cm.X.cpu(), refs[IPM][0]) and torch.equal(cm.data.cpu()[:, P:], data[:, P:])
    for f in (0, -1, K, K + 3):
        with pytest.raises(ValueError):
            alie_(D[:, :P], f, z=0.3)
        with pytest.raises(ValueError):
            ipm_(D[:, :P], f)


@pytest.mark.parametrize("attack", ["alie", "ipm"])
@pytest.mark.parametrize("exchange", ["allgather", "alltoall"])
def test_engine_round(cuda, monkeypatch, exchange, attack):
    """TINY, K = 8, f = 2, median, torch order, graph replay.  Round 1 against
    an unattacked engine with the same seeds: the benign rows are its rows, the
    attackers' rows the reference applied to its matrix, the global model the
    lower median of that.  Round 2 (a replay of the captured training graph,
    from the attacked global model) against its own benign rows."""
    monkeypatch.setenv("FLR_ORDER", "torch")
    K, f = 8, 2
    mode, param = (ALIE, alie_z(K, f)) if attack == "alie" else (IPM, 0.5)
    kw = dict(num_clients=K, batch=4, defense="median", num_attackers=f, exchange=exchange)
    eng = RoundEngine(TINY, RoundConfig(attack=attack, **kw), TrainConfig(local_steps=2), cuda)
    clean = RoundEngine(TINY, RoundConfig(attack="none", **kw), TrainConfig(local_steps=2), cuda)
    assert eng.use_graph and not eng.train_order and not eng.dead_deferred

    def matrix(e):
        return (e.full if exchange == "allgather" else e.slice).X.cpu().contiguous()
    g = eng.run_round().clone().cpu()
    clean.run_round()
    X, X0 = matrix(eng), matrix(clean)
    want = collude(X0, f, mode, param)[0]
    assert torch.isfinite(X0).all()
    assert torch.equal(X[f:], X0[f:])
    assert torch.equal(X[:f], want[:f]) and not torch.equal(X[:f], X0[:f])
    assert torch.equal(g, torch.median(want, dim=0).values)
    g2 = eng.run_round().clone().cpu()
    X2 = matrix(eng)
    want2 = collude(X2, f, mode, param)[0]   # reads the benign rows only
    assert not torch.equal(X2[f:], X[f:]) and torch.isfinite(X2).all()
    assert torch.equal(X2, want2)
    assert torch.equal(g2, torch.median(want2, dim=0).values)
    assert eng.round_index == 2 and not eng.fell_back and not eng.dead_deferred


def test_engine_attack_cfg(cuda, monkeypatch):
    """attack_cfg's z and epsilon reach the kernel."""
    monkeypatch.setenv("FLR_ORDER", "torch")
    K, f = 8, 2
    kw = dict(num_clients=K, batch=4, defense="median", num_attackers=f, exchange="allgather")
    for attack, cfg, mode, param in (("alie", {"z": 1.25}, ALIE, 1.25), ("ipm", {"epsilon": 2.0}, IPM, 2.0)):
        eng = RoundEngine(TINY, RoundConfig(attack=attack, attack_cfg=cfg, **kw), TrainConfig(local_steps=1), cuda)
        eng.run_round()
        X = eng.full.X.cpu().contiguous()
        assert torch.equal(X, collude(X, f, mode, param)[0])


def test_engine_krum_full_model_keeps_rows_whole(cuda):
    """The full ResNet-18 + GRU model under Krum's reference-exact distances,
    in the default training order: a configuration that defers the dead-tap
    slabs under the sign flip.  The colluding pass reads and writes whole rows,
    so the deferral stays off."""
    from flr.models.multimodal import ModelSpec
    rc = RoundConfig(num_clients=8, batch=4, defense="krum", attack="alie", num_attackers=1,
                     defense_cfg={"pairwise_method": "reference"})
    eng = RoundEngine(ModelSpec(), rc, TrainConfig(local_steps=1), cuda)
    assert not eng.dead_deferred
    g = eng.run_round()
    assert torch.isfinite(g).all() and not eng.fell_back and not eng.dead_deferred
