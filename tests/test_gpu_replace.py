"""GPU: model replacement (flr_replace_strength, flr_scale_rows_from, their ops
wrappers, flr.attacks.model_replacement_, the round engine's
attack="model_replacement") against the CPU restatement of tests/replace_ref.py.

The scale is three fp32 operations: torch.equal.  The strength is fp64 with only
+ - * / sqrt in the header's order, all IEEE operations on both sides, so
gamma64 is compared bit for bit with the reference evaluated on the device's own
norms and Gram matrix (ops.row_norms / ops.rows_gram with the center); status and
flags are equal.  Every matrix sits in a padded layout filled with a sentinel;
the padding, the rows past n and the inputs must come back unchanged."""
import functools
import os

import numpy as np
import pytest
import torch

import replace_ref as ref
from replace_ref import DISTANCE, MAX, MEAN, MEDIAN, NONE, NORM
from flr import _capi, ops
from flr.attacks import model_replacement_
from flr.models.multimodal import TINY
from flr.round import RoundConfig, RoundEngine
from flr.train import TrainConfig

pytestmark = pytest.mark.gpu

FILL = -77.0  # the padding columns' content
NAN = float("nan")

# (K, P, ld - P, n).  One element; below a float4 with a padded row; whole float4s;
# three past a multiple of 4 with ld % 4 == 0 (a ragged float4 tail, two
# workgroups per row); 4-byte loads (ld % 4 != 0) over seventeen workgroups per
# row; float4 loads over four workgroups per row; many rows of two workgroups.
SCALE_CASES = [(1, 1, 0, 1), (2, 7, 3, 1), (5, 64, 0, 2), (8, 1027, 1, 7), (17, 4099, 3, 4), (33, 4096, 24, 12),
               (130, 333, 1, 26)]
# (K, f): the smallest, then around a wave, a block of 64 x 64 and the limit
STRENGTH_CASES = [(2, 1), (3, 1), (5, 2), (7, 3), (64, 25), (65, 30), (130, 26), (1024, 100)]
STRENGTH_P = 67
MODES = [(NONE, MEDIAN), (NORM, MEDIAN), (NORM, MAX), (NORM, MEAN), (DISTANCE, MEDIAN)]
MODE_IDS = ["none", "norm-median", "norm-max", "norm-mean", "distance"]


def _gammas(n):
    """1.0 (the row kept), below 1, above 1 and a NaN, mixed."""
    pattern = [2.5, 1.0, 0.37, NAN, 128.0 / 25.0, 1.0, 0.999, 1.0 + 2.0 ** -23]
    return np.array([pattern[i % len(pattern)] for i in range(n)], dtype=np.float32)


def _padded(X, pad, cuda, offset=0):
    """X [K, P] inside a [K, P + pad] layout of FILL, the layout offset floats
    into its buffer: (host copy of the layout, device layout)."""
    K, P = X.shape
    data = torch.full((K, P + pad), FILL)
    data[:, :P] = X
    buf = torch.full((K * (P + pad) + offset,), FILL, device=cuda)
    dev = buf[offset:].view(K, P + pad)
    dev.copy_(data)
    return data, dev


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


# ---- flr_scale_rows_from ----

@pytest.mark.parametrize("K,P,pad,n", SCALE_CASES)
def test_scale_rows_from(cuda, K, P, pad, n):
    X, g = ref.updates(K, min(n, K), P, seed=K + P)
    gam = _gammas(n)
    want = ref.scale(X, g, gam)
    data, dev = _padded(X, pad, cuda)
    gg, gd = g.to(cuda), torch.from_numpy(gam).to(cuda)
    out = ops.scale_rows_from(dev[:, :P], gg, gd)
    assert out.data_ptr() == dev.data_ptr()
    got = dev.cpu()
    assert torch.equal(got[:, :P].view(torch.int32), want.view(torch.int32))
    assert torch.equal(got[:, P:], data[:, P:]) and torch.equal(got[n:], data[n:])
    for i in range(n):   # gamma == 1 or NaN: the row's own bits
        if gam[i] == 1.0 or np.isnan(gam[i]):
            assert torch.equal(got[i], data[i])
        else:
            assert not torch.equal(got[i], data[i])
    assert torch.equal(gg.cpu(), g) and np.array_equal(gd.cpu().numpy().view(np.int32), gam.view(np.int32))


def test_scale_rows_from_four_byte_form_gives_the_same_bits(cuda):
    """X 4 bytes off a 16-byte boundary with ld % 4 == 0: the 4-byte loads run
    and give the float4 form's bits."""
    K, P, pad, n = 33, 4096, 24, 12
    X, g = ref.updates(K, n, P, seed=K + P)
    gam = _gammas(n)
    want = ref.scale(X, g, gam)
    gg, gd = g.to(cuda), torch.from_numpy(gam).to(cuda)
    outs = []
    for offset in (0, 1):
        data, dev = _padded(X, pad, cuda, offset)
        assert dev.data_ptr() % 16 == 4 * offset
        ops.scale_rows_from(dev[:, :P], gg, gd)
        got = dev.cpu()
        assert torch.equal(got[:, P:], data[:, P:]) and torch.equal(got[n:], data[n:])
        outs.append(got[:, :P])
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert torch.equal(outs[1].view(torch.int32), want.view(torch.int32))


# ---- flr_replace_strength ----

@functools.lru_cache(maxsize=None)
def _device_inputs(K, f):
    """The host generator at P = 67 and the device's own norms and Gram matrix."""
    X, g = ref.updates(K, f, STRENGTH_P, seed=K)
    dev = torch.device("cuda:0")
    Xd, gd = X.to(dev), g.to(dev)
    return X, g, ops.row_norms(Xd, center=gd), ops.rows_gram(Xd, center=gd)


def _check_strength(got, want):
    gamma64, gamma32, status, flags = (t.cpu().numpy() for t in got)
    wg, ws, wf = want
    err = float(np.abs(gamma64 - wg).max())
    print("gamma64: max abs difference from the reference", err, "status", np.bincount(ws, minlength=4).tolist())
    assert np.array_equal(_bits(gamma64), _bits(wg))
    assert np.array_equal(gamma32.view(np.int32), wg.astype(np.float32).view(np.int32))
    assert status.dtype == np.int32 and np.array_equal(status, ws)
    assert flags.tolist() == [wf]


# (2, 1) has one benign row: a norm-mode case only
STRENGTH_PARAMS = [pytest.param(K, f, mode, stat, id=f"{K}-{f}-{name}") for K, f in STRENGTH_CASES
                   for (mode, stat), name in zip(MODES, MODE_IDS) if mode != DISTANCE or K - f >= 2]


@pytest.mark.parametrize("boost", [None, 1.05], ids=["boost-K/f", "boost-1.05"])
@pytest.mark.parametrize("K,f,mode,stat", STRENGTH_PARAMS)
def test_replace_strength(cuda, K, f, mode, stat, boost):
    boost = K / f if boost is None else boost
    _, _, norms, G = _device_inputs(K, f)
    n0, G0 = norms.clone(), G.clone()
    for rho in (1.0, 0.7):
        want = ref.strength(norms.cpu().numpy(), G.cpu().numpy(), K, f, boost, mode, stat, rho)
        got = ops.replace_strength(norms if mode != DISTANCE else None, G if mode == DISTANCE else None, f, boost,
                                   mode, stat, rho, K=K, device=cuda)
        _check_strength(got, want)
    assert torch.equal(norms, n0) and torch.equal(G, G0)


@pytest.mark.parametrize("mode", [NORM, DISTANCE], ids=["norm", "distance"])
def test_replace_strength_degenerate_rows(cuda, mode):
    """A zero attacker row: boost.  A NaN attacker: gamma 1, status 3, bit 1.  A
    NaN benign row: every gamma 1, bit 0."""
    K, f, P = 7, 3, 19
    X, g = ref.updates(K, f, P, 0)
    gd = g.to(cuda)
    for row, col, value, flags in ((1, None, None, 0), (0, 2, NAN, 2), (5, 3, NAN, 1)):
        Z = X.clone()
        if col is None:
            Z[row] = g
        else:
            Z[row, col] = value
        Zd = Z.to(cuda)
        norms, G = ops.row_norms(Zd, center=gd), ops.rows_gram(Zd, center=gd)
        want = ref.strength(norms.cpu().numpy(), G.cpu().numpy(), K, f, 4.0, mode)
        assert want[2] == flags
        if col is None:
            assert want[0][1] == 4.0 and want[1][1] == 0
        got = ops.replace_strength(norms, G, f, 4.0, mode)
        _check_strength(got, want)


# ---- errors ----

def test_errors_leave_x_alone(cuda):
    lib = _capi.lib()
    K, P, pad, f = 6, 10, 2, 2
    X, g = ref.updates(K, f, P, 3)
    data, dev = _padded(X, pad, cuda)
    gd = g.to(cuda)
    gam = torch.full((K + 1,), 2.0, device=cuda)
    ld = P + pad

    def scale(x=dev.data_ptr(), k=K, p=P, l=ld, c=gd.data_ptr(), gm=gam.data_ptr(), n=f):
        return lib.flr_scale_rows_from(x, k, p, l, c, gm, n, None)

    for kw in (dict(x=None), dict(c=None), dict(gm=None), dict(n=K + 1), dict(n=-1), dict(l=P - 1), dict(k=0),
               dict(p=0)):
        assert scale(**kw) == _capi.FLR_ERR_ARG, kw
    assert scale(n=0) == _capi.FLR_OK
    torch.cuda.synchronize()
    assert torch.equal(dev.cpu(), data)

    norms = torch.ones(1025, dtype=torch.float64, device=cuda)
    G = torch.eye(1025, dtype=torch.float64, device=cuda).contiguous()
    g64 = torch.full((1025,), -5.0, dtype=torch.float64, device=cuda)
    g32 = torch.full((1025,), -5.0, dtype=torch.float32, device=cuda)
    st = torch.full((1025,), -5, dtype=torch.int32, device=cuda)
    fl = torch.full((1,), -5, dtype=torch.int32, device=cuda)

    def strength(nr=norms.data_ptr(), gm=G.data_ptr(), k=K, ff=f, boost=2.0, mode=NORM, stat=MEDIAN, rho=1.0,
                 o64=g64.data_ptr(), o32=g32.data_ptr(), s=st.data_ptr(), fg=fl.data_ptr()):
        return lib.flr_replace_strength(nr, gm, k, ff, boost, mode, stat, rho, o64, o32, s, fg, None)

    bad = [dict(o64=None), dict(o32=None), dict(s=None), dict(fg=None), dict(nr=None), dict(gm=None, mode=DISTANCE),
           dict(ff=0), dict(ff=K), dict(mode=3), dict(mode=-1), dict(stat=3), dict(ff=K - 1, mode=DISTANCE)]
    for v in (0.0, -1.0, NAN, float("inf")):
        bad += [dict(boost=v), dict(rho=v)]
    for kw in bad:
        assert strength(**kw) == _capi.FLR_ERR_ARG, kw
    assert strength(k=1025, ff=100) == _capi.FLR_ERR_UNSUPPORTED
    assert strength(k=1025, ff=100, mode=DISTANCE) == _capi.FLR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (g64 == -5.0).all() and (g32 == -5.0).all() and (st == -5).all() and (fl == -5).all()
    with pytest.raises(ValueError, match="at most 1024"):
        ops.replace_strength(norms, None, 100, 2.0, NORM)
    with pytest.raises(ValueError, match="entries"):
        ops.scale_rows_from(dev[:, :P], gd, gam)
    assert torch.equal(dev.cpu(), data)


# ---- flr.attacks.model_replacement_ ----

@pytest.mark.parametrize("stealth,stat", [("none", "median"), ("norm", "median"), ("norm", "max"), ("norm", "mean"),
                                          ("distance", "median")])
def test_model_replacement_api(cuda, stealth, stat):
    K, f, P, pad = 12, 4, 1027, 1
    X, g = ref.updates(K, f, P, 5)
    data, dev = _padded(X, pad, cuda)
    gd = g.to(cuda)
    norms, G = ops.row_norms(dev[:, :P], center=gd), ops.rows_gram(dev[:, :P], center=gd)
    mode = {"none": NONE, "norm": NORM, "distance": DISTANCE}[stealth]
    st = {"median": MEDIAN, "max": MAX, "mean": MEAN}[stat]
    wg, ws, wf = ref.strength(norms.cpu().numpy(), G.cpu().numpy(), K, f, K / f, mode, st, 0.9)
    gamma, status, flags = model_replacement_(dev[:, :P], f, gd, stealth=stealth, stat=stat, rho=0.9)
    assert gamma.dtype == torch.float64 and np.array_equal(_bits(gamma.cpu().numpy()), _bits(wg))
    assert np.array_equal(status.cpu().numpy(), ws) and flags.tolist() == [wf]
    got = dev.cpu()
    want = ref.scale(X, g, wg.astype(np.float32))
    assert torch.equal(got[:, :P].view(torch.int32), want.view(torch.int32))
    assert torch.equal(got[:, P:], data[:, P:]) and torch.equal(got[f:], data[f:])
    assert not torch.equal(got[:f], data[:f]) and torch.equal(gd.cpu(), g)


# ---- the round engine ----

ENGINE_SEED = 42
EK, EF = 8, 2


@functools.lru_cache(maxsize=None)
def _engine_round(attack, cfg, exchange):
    """One round at TINY in torch order: (the global model it trained from, the
    exchanged matrix after the attack, the published model, attack_gamma), on
    the host."""
    dev = torch.device("cuda:0")
    old = os.environ.get("FLR_ORDER")
    os.environ["FLR_ORDER"] = "torch"   # the backdoor engine's matrix in the attack's coordinate order
    try:
        eng = RoundEngine(TINY, RoundConfig(num_clients=EK, batch=4, defense="fedavg", attack=attack,
                                            num_attackers=EF, seed=ENGINE_SEED, exchange=exchange,
                                            attack_cfg=dict(cfg)), TrainConfig(local_steps=2), dev)
    finally:
        if old is None:
            del os.environ["FLR_ORDER"]
        else:
            os.environ["FLR_ORDER"] = old
    assert eng.exchange == exchange and not eng.train_order and not eng.dead_deferred
    g0 = eng.global_flat.clone()
    published = eng.run_round().clone()
    X = (eng.full if exchange == "allgather" else eng.slice).X
    assert tuple(X.shape) == (EK, g0.numel())
    gamma = None if eng.attack_gamma is None else eng.attack_gamma.cpu().numpy()
    return g0.cpu(), X.cpu().clone(), published.cpu(), gamma


def _expected(exchange, mode, stat, boost=EK / EF, rho=1.0):
    """From the backdoor engine's rows: (gamma, the matrix after the reference
    scale, its FedAvg on the device)."""
    dev = torch.device("cuda:0")
    g0, Xb, _, none = _engine_round("backdoor", (), exchange)
    assert none is None
    Xd, gd = Xb.to(dev), g0.to(dev)
    norms, G = ops.row_norms(Xd, center=gd), ops.rows_gram(Xd, center=gd)
    gamma, status, flags = ref.strength(norms.cpu().numpy(), G.cpu().numpy(), EK, EF, boost, mode, stat, rho)
    assert flags == 0
    want = ref.scale(Xb, g0, gamma.astype(np.float32))
    return gamma, want, ops.fedavg(want.to(dev), [8] * EK).cpu()


@pytest.mark.parametrize("exchange,stealth", [("allgather", "none"), ("allgather", "norm"),
                                              ("allgather", "distance"), ("alltoall", "none")])
def test_engine_round(cuda, exchange, stealth):
    """TINY, K = 8, f = 2, FedAvg: against a second engine under
    attack="backdoor", the benign rows are that engine's bit for bit, the
    attackers' rows its rows under the reference scale with the reference
    strength on the device's norms and Gram matrix of those rows,
    attack_gamma that strength, and the published model ops.fedavg of the
    expected matrix."""
    cfg = {"none": (), "norm": (("stealth", "norm"), ("stat", "max")), "distance": (("stealth", "distance"),)}[stealth]
    mode = {"none": NONE, "norm": NORM, "distance": DISTANCE}[stealth]
    g0, X, published, gamma = _engine_round("model_replacement", cfg, exchange)
    gb, Xb, _, _ = _engine_round("backdoor", (), exchange)
    assert torch.equal(g0, gb)
    wg, want, agg = _expected(exchange, mode, MAX)
    print("gamma", wg.tolist())
    assert torch.equal(X[EF:].view(torch.int32), Xb[EF:].view(torch.int32))
    assert torch.equal(X[:EF].view(torch.int32), want[:EF].view(torch.int32))
    assert not torch.equal(X[:EF], Xb[:EF])
    assert gamma.dtype == np.float64 and gamma.shape == (EF,) and np.array_equal(_bits(gamma), _bits(wg))
    assert torch.equal(published, agg)


def test_engine_boost_one_is_the_backdoor(cuda):
    g0, X, published, gamma = _engine_round("model_replacement", (("boost", 1.0),), "allgather")
    _, Xb, pb, _ = _engine_round("backdoor", (), "allgather")
    assert gamma.tolist() == [1.0] * EF
    assert torch.equal(X.view(torch.int32), Xb.view(torch.int32)) and torch.equal(published, pb)


def test_norm_stealth_stays_under_the_benign_maximum(cuda):
    """stealth "norm", stat "max", rho 1: every attacker's ||x_i - g|| is at most
    the benign maximum times (1 + 2^-20) (the fp32 rounding of the
    three-operation scale over the norm's fp64 sum); with no stealth and the
    default boost an attacker exceeds it — asserted on the reference first, so a
    borderline seed fails there and not as a kernel bug."""
    dev = torch.device("cuda:0")
    g0, X, _, _ = _engine_round("model_replacement", (("stealth", "norm"), ("stat", "max")), "allgather")
    _, want, _ = _expected("allgather", NORM, MAX)
    host = np.sqrt((ref.centered(want, g0) ** 2).sum(axis=1))
    assert (host[:EF] <= host[EF:].max() * (1.0 + 2.0 ** -20)).all()
    norms = ops.row_norms(X.to(dev), center=g0.to(dev)).cpu().numpy()
    print("attackers", norms[:EF].tolist(), "benign max", norms[EF:].max())
    assert (norms[:EF] <= norms[EF:].max() * (1.0 + 2.0 ** -20)).all()

    g0, X, _, _ = _engine_round("model_replacement", (), "allgather")
    _, want, _ = _expected("allgather", NONE, MAX)
    host = np.sqrt((ref.centered(want, g0) ** 2).sum(axis=1))
    assert (host[:EF] > host[EF:].max()).any()
    norms = ops.row_norms(X.to(dev), center=g0.to(dev)).cpu().numpy()
    assert (norms[:EF] > norms[EF:].max()).any()
