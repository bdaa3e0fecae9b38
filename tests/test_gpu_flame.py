"""GPU: FLAME (flr_flame_select, flr_add_gaussian, their ops wrappers,
FlameDefense, the round engine's defense="flame") against the CPU restatement
of tests/flame_ref.py.

The selection on the reference's own Gram matrix, uploaded: keep, beta, sigma,
S, t*, L and the flags bit for bit (fp64 + - * / sqrt only, each rounded on its
own on both sides).  From the device's Gram matrix the admitted set can only
agree when no pair distance lies within the Gram matrices' difference of t*:
every such test asserts the reference's own margin first, so a borderline seed
fails there and not as a kernel bug.  The Gaussian draws against the float64
evaluation within 1e-5 (the measured maximum is printed), everything around
them bit for bit.  Every matrix and vector sits in a padded layout filled with a
sentinel; the padding and the inputs must come back unchanged."""
import functools

import numpy as np
import pytest
import torch

import flame_ref as ref
from flr import _capi, ops
from flr.defenses import get_defense
from flr.matrix import ClientMatrix
from flr.models.multimodal import TINY
from flr.round import RoundConfig, RoundEngine
from flr.train import TrainConfig

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
FILL = -77.0  # the padding's content
LAMBDA = 0.001

# (K, P, ld - P, f): the generator's shapes of tests/test_flame_host.py
DATA_CASES = [(5, 7, 3, 2), (8, 64, 0, 2), (17, 333, 3, 4), (33, 1027, 1, 6), (64, 256, 0, 31), (65, 2048, 24, 13),
              (130, 5000, 24, 26), (300, 600, 0, 60), (1024, 256, 0, 100)]
# the selection alone also at one and two clients, around a wave (63, 64, 65) and at the limit (1023, 1024)
SELECT_CASES = [(1, 5, 0), (2, 7, 0), (63, 128, 12), (1023, 128, 100)] + [(K, P, f) for K, P, _, f in DATA_CASES]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def _rounds(K, P, f):
    return ref.rounds(K, P, f)


@functools.lru_cache(maxsize=None)
def _gram(K, P, f):
    g, Xs = _rounds(K, P, f)
    return ref.gram(Xs[0], g)


@functools.lru_cache(maxsize=None)
def _clustering(K, P, f, m):
    return ref.clustering(_gram(K, P, f), m)


def _padded(X, pad, cuda):
    """X (numpy [K, P]) inside a [K, P + pad] layout of FILL: (host copy, device tensor)."""
    X = torch.as_tensor(np.asarray(X), dtype=torch.float32)
    data = torch.full((X.shape[0], X.shape[1] + pad), FILL)
    data[:, :X.shape[1]] = X
    return data, data.to(cuda)


def _vec(v, cuda, dtype=torch.float32):
    return torch.as_tensor(np.asarray(v), dtype=dtype).to(cuda)


def _check_selection(got, want):
    """(keep, beta, sigma, stats, flags) of the device against a reference Selection, bit for bit."""
    keep, beta, sigma, stats, flags = (t.cpu().numpy() for t in got)
    assert keep.dtype == np.int32 and np.array_equal(keep, want.keep)
    assert np.array_equal(_bits(beta), _bits(want.beta))
    assert np.array_equal(_bits(sigma), _bits(np.array([want.sigma], dtype=np.float32)))
    ws = np.array([want.S, want.tstar, float(want.L)])
    # a NaN median (more than half the norms NaN) is a NaN on both sides: its payload is not part of the contract
    assert np.array_equal(np.isnan(stats), np.isnan(ws))
    assert np.array_equal(_bits(stats)[~np.isnan(ws)], _bits(ws)[~np.isnan(ws)])
    assert flags.tolist() == [want.flags]


def _select_matrix(G, cuda, m, lam, norms):
    """The device's selection on the host matrix G, uploaded; G and norms must come back unchanged."""
    Gd = _vec(G, cuda, torch.float64)
    nd = None if norms is None else _vec(norms, cuda, torch.float64)
    got = ops.flame_select(Gd, m, lam, nd, diagnostics=True)
    assert np.array_equal(_bits(Gd.cpu().numpy()), _bits(G))
    assert nd is None or np.array_equal(_bits(nd.cpu().numpy()), _bits(norms))
    plain = ops.flame_select(Gd, m, lam, nd)          # without the optional outputs
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(plain, got[:3]))
    return got


# ---- flr_flame_select ----

@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("with_norms", [False, True])
@pytest.mark.parametrize("K,P,f", SELECT_CASES)
def test_select_on_the_reference_gram(cuda, K, P, f, with_norms, full):
    """min_cluster_size = None and K, with and without the caller's norms, lambda = 0 and 0.001."""
    G = _gram(K, P, f)
    m = K if full else None
    clustered = _clustering(K, P, f, m)
    norms = None
    if with_norms:   # norms of their own: another median, other rows clipped
        norms = np.sqrt(np.diag(G)) * (1.0 + 0.3 * np.sin(np.arange(K)))
    for lam in (0.0, LAMBDA):
        want = ref.weights(clustered, lam, norms)
        assert want.flags == 0 and want.L >= (K if full else K // 2 + 1)
        _check_selection(_select_matrix(G, cuda, m, lam, norms), want)


def test_select_special_cases(cuda):
    """No cluster, bad rows, zero rows, identical rows, NaN distances and a
    designed exact tie, bit for bit."""
    g, Xs = _rounds(8, 64, 2)
    U = (Xs[0] - g[None, :]).astype(np.float32)
    Z = U.copy()
    Z[5] = 0.0
    B = U.copy()
    B[:4, 3] = np.nan
    C = U.copy()
    C[3, 7] = np.nan
    C[0, 1] = np.inf
    I = U.copy()
    I[1] = I[0]
    tie = np.array([[3, 0, 0, 0, 4], [0, 3, 0, 0, 4], [0, 0, 3, 0, 4], [0, 0, 0, 3, 4], [5, 0, 0, 0, 0],
                    [0, -5, 0, 0, 0]], dtype=np.float32)
    # finite diagonal, a NaN and a negative-diagonal entry off it: NaN distances are no edges
    N = ref.gram(U)
    N[2, 5] = N[5, 2] = np.nan
    N[6, 6] = -1.0
    cases = [(ref.gram(Z), None, 0), (ref.gram(Z), 8, 0), (ref.gram(B), None, 3), (ref.gram(C), None, 2),
             (ref.gram(C), 8, 3), (ref.gram(I), None, 0), (ref.gram(tie), None, 0), (ref.gram(tie), 6, 0),
             (N, None, 0), (N, 8, 1), (ref.gram(B[:1]), None, 3), (ref.gram(U[:1]), None, 0),
             (np.zeros((7, 7)), None, 0)]
    for G, m, flags in cases:
        want = ref.select(G, m, LAMBDA)
        assert want.flags == flags, (want.flags, flags)
        if flags & 1:
            assert not want.keep.any() and not want.beta.any() and want.sigma == 0 and want.tstar == np.inf
        _check_selection(_select_matrix(G, cuda, m, LAMBDA, None), want)
    d = ref.select(ref.gram(tie)).dist
    assert d[0, 1] == d[0, 2] == d[1, 3] == d[2, 3]       # the tie is one of equal bits


def test_select_errors(cuda):
    G = torch.eye(4, dtype=torch.float64, device=cuda)
    keep = torch.full((4,), 9, dtype=torch.int32, device=cuda)
    beta = torch.full((4,), FILL, device=cuda)
    sigma = torch.full((1,), FILL, device=cuda)
    lib, st = _capi.lib(), torch.cuda.current_stream(cuda).cuda_stream
    k, b, s = keep.data_ptr(), beta.data_ptr(), sigma.data_ptr()
    E = _capi.FLR_ERR_ARG
    assert lib.flr_flame_select(None, None, 4, 3, 0.0, k, b, s, None, None, st) == E
    assert lib.flr_flame_select(G.data_ptr(), None, 4, 3, 0.0, None, b, s, None, None, st) == E
    assert lib.flr_flame_select(G.data_ptr(), None, 4, 3, 0.0, k, None, s, None, None, st) == E
    assert lib.flr_flame_select(G.data_ptr(), None, 4, 3, 0.0, k, b, None, None, None, st) == E
    assert lib.flr_flame_select(G.data_ptr(), None, 0, 1, 0.0, k, b, s, None, None, st) == E
    for m in (0, 2, 5, -1):
        assert lib.flr_flame_select(G.data_ptr(), None, 4, m, 0.0, k, b, s, None, None, st) == E
    for lam in (-1.0, float("nan"), float("inf")):
        assert lib.flr_flame_select(G.data_ptr(), None, 4, 3, lam, k, b, s, None, None, st) == E
    assert lib.flr_flame_select(G.data_ptr(), None, 1025, 513, 0.0, k, b, s, None, None, st) \
        == _capi.FLR_ERR_UNSUPPORTED
    for bad in ({"m": 2}, {"m": 5}, {"m": True}, {"lam": -1.0}, {"lam": float("nan")},
                {"norms": torch.zeros(3, dtype=torch.float64, device=cuda)},
                {"norms": torch.zeros(4, device=cuda)}):
        with pytest.raises(ValueError):
            ops.flame_select(G, **bad)
    with pytest.raises(ValueError):
        ops.flame_select(torch.zeros((3, 4), dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError):
        ops.flame_select(torch.zeros((3, 3), device=cuda))
    with pytest.raises(ValueError):
        ops.flame_select(torch.zeros((1025, 1025), dtype=torch.float64, device=cuda))
    with pytest.raises(RuntimeError):
        ops.flame_select(torch.zeros((3, 3), dtype=torch.float64))
    torch.cuda.synchronize()
    assert (keep == 9).all() and (beta == FILL).all() and (sigma == FILL).all()
    assert ops.FLAME_MAX_CLIENTS == 1024


@pytest.mark.parametrize("K,P,pad,f", DATA_CASES)
def test_end_to_end_from_the_rows(cuda, K, P, pad, f):
    """ops.rows_gram, then the selection, then the combination: keep is the
    reference's; out is rows_combine_from's reference on the device's own beta,
    bit for bit; beta within 1e-9 relative of the host's (the Gram matrices
    differ by at most 2 P 2^-52 relative to n_i n_j, test_gpu_foolsgold.py's
    bound, which one division carries into S / n_i)."""
    g, Xs = _rounds(K, P, f)
    X = Xs[0]
    want = ref.weights(_clustering(K, P, f, None), LAMBDA)
    print("reference margin", want.margin, "admitted", want.L, "t*", want.tstar)
    assert want.margin > MARGIN
    data, Dg = _padded(X, pad, cuda)
    gg = _vec(g, cuda)
    G = ops.rows_gram(Dg[:, :P], center=gg)
    keep, beta, sigma, stats, flags = ops.flame_select(G, None, LAMBDA, diagnostics=True)
    assert np.array_equal(keep.cpu().numpy(), want.keep) and flags.item() == 0
    assert not want.keep[:f].any()
    b = beta.cpu().numpy()
    rel = float(np.abs(b.astype(np.float64)[want.keep == 1] / want.beta.astype(np.float64)[want.keep == 1] - 1).max())
    S, tstar, L = stats.cpu().tolist()
    print("beta: max relative error", rel, " S: relative error", abs(S / want.S - 1), " t*: error",
          abs(tstar - want.tstar))
    assert np.array_equal(b == 0, want.beta == 0)
    assert rel <= 1e-9
    assert abs(S / want.S - 1) <= 1e-9 and abs(tstar - want.tstar) <= 1e-9 and L == want.L
    out = ops.rows_combine_from(Dg[:, :P], gg, beta)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref.combine(X, g, b)))
    assert torch.equal(Dg.cpu(), data) and torch.equal(gg.cpu(), torch.as_tensor(g))


# ---- flr_add_gaussian ----

BIG = (1 << 34) - 6     # crosses the counter's low word
SEED = 0x123456789ABCDEF


def _buffer(v, lead, cuda):
    """v (numpy float32 [P]) at element offset lead of a FILL vector with at least
    one FILL element on each side: (the device buffer, the view of v).  The
    buffer is 16-byte aligned: lead % 4 is the view's misalignment in floats."""
    P = len(v)
    buf = torch.full((lead + P + 4,), FILL)
    buf[lead:lead + P] = torch.as_tensor(v)
    dev = buf.to(cuda)
    assert dev.data_ptr() % 16 == 0
    return dev, dev[lead:lead + P]


def _draw(v, sigma, cuda, lead=4, **kw):
    """add_gaussian_ on a copy of v at misalignment lead % 4; the FILL around it must stay."""
    dev, view = _buffer(v, lead, cuda)
    sg = _vec([sigma], cuda)
    ops.add_gaussian_(view, sg, **kw)
    host = dev.cpu().numpy()
    P = len(v)
    assert (host[:lead] == FILL).all() and (host[lead + P:] == FILL).all()
    assert sg.item() == np.float32(sigma) or sigma != sigma
    return host[lead:lead + P]


@pytest.mark.parametrize("col0", [0, 1, 2, 3, 5, BIG])
@pytest.mark.parametrize("P", [1, 3, 4, 5, 1027, 4099])
def test_gaussian_draws(cuda, P, col0):
    """v = 0, sigma = 1: the draws within 1e-5 of the float64 evaluation
    (rounding 2 pi u2 to fp32 costs at most 2.4e-7 in the angle, times r <= 5.78:
    1.4e-6; a few ulp of logf, sqrtf, sinf and cosf at |z| <= 5.78 add under
    3e-6).  The same bits at every pointer alignment (16-byte accesses when the
    pointer's misalignment matches col0's, 4-byte accesses otherwise).  Then
    general v and sigma: out == fl(v + fl(sigma * z)), z the device's own draws;
    sigma = 0 leaves v's bits, -0.f included."""
    want = ref.normals(P, seed=SEED, stream=3, col0=col0)
    zero = np.zeros(P, dtype=np.float32)
    z = _draw(zero, 1.0, cuda, seed=SEED, stream=3, col0=col0)
    err = float(np.abs(z.astype(np.float64) - want).max())
    print("max abs error of the draws", err)
    assert err <= 1e-5
    for lead in (5, 6, 7):
        assert np.array_equal(_bits(_draw(zero, 1.0, cuda, lead=lead, seed=SEED, stream=3, col0=col0)), _bits(z))
    rng = np.random.default_rng(P)
    v = rng.standard_normal(P).astype(np.float32)
    v[0] = -0.0
    for sigma in (0.37, -2.5e-3):
        for lead in (4, 5):
            got = _draw(v, sigma, cuda, lead=lead, seed=SEED, stream=3, col0=col0)
            assert np.array_equal(_bits(got), _bits(ref.add_noise(v, sigma, z)))
    for sigma in (0.0, -0.0):
        assert np.array_equal(_bits(_draw(v, sigma, cuda, seed=SEED, stream=3, col0=col0)), _bits(v))


@pytest.mark.parametrize("col0", [0, 3, BIG])
def test_gaussian_column_ranges_and_streams(cuda, col0):
    """A column range with its own col0 is the slice of the whole call; another
    stream or seed gives other draws."""
    P = 4099
    zero = np.zeros(P, dtype=np.float32)
    z = _draw(zero, 1.0, cuda, seed=SEED, stream=0, col0=col0)
    for a, b in ((0, 1), (1, 4), (2, 1027), (5, 4099), (1024, 2050), (4098, 4099)):
        for lead in (4, 7):
            part = _draw(zero[a:b], 1.0, cuda, lead=lead, seed=SEED, stream=0, col0=col0 + a)
            assert np.array_equal(_bits(part), _bits(z[a:b]))
    assert not np.array_equal(_draw(zero, 1.0, cuda, seed=SEED, stream=1, col0=col0), z)
    assert not np.array_equal(_draw(zero, 1.0, cuda, seed=SEED + 1, stream=0, col0=col0), z)
    assert not np.array_equal(_draw(zero, 1.0, cuda, seed=SEED + (1 << 32), stream=0, col0=col0), z)


def test_gaussian_moments(cuda):
    """2^20 draws: the host test's bounds on the device's draws."""
    P = 1 << 20
    v = torch.zeros(P, device=cuda)
    z = ops.add_gaussian_(v, _vec([1.0], cuda), seed=0, stream=0).cpu().numpy().astype(np.float64)
    print("mean", z.mean(), "var", z.var(), "max |z|", np.abs(z).max())
    assert abs(z.mean()) <= 5 / np.sqrt(P)
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(2 / P)
    assert np.abs(z).max() <= 5.78
    err = float(np.abs(z - ref.normals(P)).max())
    print("max abs error of the draws", err)
    assert err <= 1e-5


def test_gaussian_errors(cuda):
    v = torch.full((8,), FILL, device=cuda)
    s = torch.ones(1, device=cuda)
    lib, st = _capi.lib(), torch.cuda.current_stream(cuda).cuda_stream
    E = _capi.FLR_ERR_ARG
    assert lib.flr_add_gaussian(None, 8, s.data_ptr(), 0, 0, 0, st) == E
    assert lib.flr_add_gaussian(v.data_ptr(), 8, None, 0, 0, 0, st) == E
    assert lib.flr_add_gaussian(v.data_ptr(), -1, s.data_ptr(), 0, 0, 0, st) == E
    assert lib.flr_add_gaussian(v.data_ptr(), 8, s.data_ptr(), 0, 0, -1, st) == E
    assert lib.flr_add_gaussian(v.data_ptr(), 8, s.data_ptr(), 0, 0, (1 << 63) - 8, st) == E
    assert lib.flr_add_gaussian(v.data_ptr(), 0, s.data_ptr(), 0, 0, 0, st) == _capi.FLR_OK
    with pytest.raises(ValueError):
        ops.add_gaussian_(v, s, col0=-1)
    with pytest.raises(ValueError):
        ops.add_gaussian_(v, s, stream=1 << 32)
    with pytest.raises(ValueError):
        ops.add_gaussian_(v, torch.ones(2, device=cuda))
    with pytest.raises(ValueError):
        ops.add_gaussian_(v.double(), s)
    with pytest.raises(ValueError):
        ops.add_gaussian_(torch.zeros((2, 8), device=cuda)[:, :4], s)
    with pytest.raises(RuntimeError):
        ops.add_gaussian_(torch.zeros(8), s)
    torch.cuda.synchronize()
    assert (v == FILL).all()
    assert ops.add_gaussian_(torch.zeros(0, device=cuda), s).numel() == 0


# ---- the defense ----

DEFENSE_SEED = 5


@pytest.mark.parametrize("K,P,pad,f", [(8, 64, 0, 2), (33, 1027, 1, 6), (130, 5000, 24, 26)])
def test_defense_two_calls(cuda, K, P, pad, f):
    g, Xs = _rounds(K, P, f)
    gg = _vec(g, cuda)
    d = get_defense("flame", {"seed": DEFENSE_SEED})
    quiet = get_defense("flame", {"noise_lambda": 0})
    literal = get_defense("flame", {"on": "weights", "noise_lambda": 0})
    noise = []
    for n, X in enumerate(Xs):
        agg_ref, want = ref.run(g, X, lam=LAMBDA)
        print("call", n + 1, "reference margin", want.margin, "admitted", want.L)
        assert want.margin > MARGIN
        data, Dg = _padded(X, pad, cuda)
        cm = ClientMatrix(Dg, P, [(P,)])
        out = d.aggregate_flat(cm, [], global_flat=gg)
        rejected = np.nonzero(want.keep == 0)[0].tolist()
        assert d.detect_malicious() == rejected and set(range(f)) <= set(rejected)
        beta = np.asarray(d.client_weights, dtype=np.float32)
        assert np.array_equal(beta == 0, want.beta == 0)
        m = d.get_metrics()
        assert m["defense_type"] == "flame" and m["calls"] == n + 1 and m["admitted"] == want.L
        assert m["noise_lambda"] == LAMBDA and m["min_cluster_size"] is None and m["on"] == "updates"
        assert m["seed"] == DEFENSE_SEED and not m["no_update"] and not m["bad_rows"]
        assert abs(m["clip_bound"] / want.S - 1) <= 1e-9 and abs(m["threshold"] - want.tstar) <= 1e-9
        assert abs(m["sigma"] / float(want.sigma) - 1) <= 2.0 ** -22
        # the aggregate: the combination on the device's beta, then the device's draws of stream n
        plain = ref.combine(X, g, beta)
        z = ops.add_gaussian_(torch.zeros(P, device=cuda), _vec([1.0], cuda), seed=DEFENSE_SEED,
                              stream=n).cpu().numpy()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref.add_noise(plain, np.float32(m["sigma"]), z)))
        noise.append(z)
        # one fp32 ulp of beta (|u| < 1) and the noise away from the reference's noiseless aggregate
        assert np.abs(out.cpu().numpy() - agg_ref).max() <= 2.0 ** -20 + 5.78 * m["sigma"]
        # noise_lambda = 0: the noiseless combination, bit for bit
        q = quiet.aggregate_flat(cm, [], global_flat=gg)
        assert np.array_equal(_bits(q.cpu().numpy()), _bits(ref.combine(X, g, np.asarray(quiet.client_weights,
                                                                                         dtype=np.float32))))
        assert quiet.get_metrics()["sigma"] == 0.0 and quiet.detect_malicious() == rejected
        # on = "weights": the cosines of the models
        _, wl = ref.run(g, X, on="weights")
        print("on=weights: reference margin", wl.margin, "admitted", wl.L)
        assert wl.margin > MARGIN
        literal.aggregate_flat(cm, [], global_flat=gg)
        assert literal.detect_malicious() == np.nonzero(wl.keep == 0)[0].tolist()
        assert literal.get_metrics()["admitted"] == wl.L
        assert torch.equal(Dg.cpu(), data) and torch.equal(gg.cpu(), torch.as_tensor(g))
    assert not np.array_equal(noise[0], noise[1])


def test_defense_parameter_lists_and_set_center(cuda):
    """The drop-in aggregate(updates, num_examples): list-of-lists in, the center
    from set_center, then global_params; the same bits as aggregate_flat."""
    K, P, f = 17, 333, 4
    g, Xs = _rounds(K, P, f)
    X = torch.as_tensor(Xs[0])
    gt = torch.as_tensor(g)
    ups = [[X[k, :300].reshape(3, 100).clone(), X[k, 300:].clone()] for k in range(K)]
    want = get_defense("flame", {"seed": 9}).aggregate_flat(ClientMatrix(X.to(cuda), P, [(P,)]), [],
                                                            global_flat=gt.to(cuda)).cpu()
    d = get_defense("flame", {"seed": 9})
    d.set_center([gt[:300].reshape(3, 100), gt[300:]])
    got = d.aggregate(ups, [10] * K)
    assert [tuple(p.shape) for p in got] == [(3, 100), (33,)] and got[0].device.type == "cpu"
    assert torch.equal(torch.cat([p.reshape(-1) for p in got]), want)
    assert set(range(f)) <= set(d.detect_malicious())
    d2 = get_defense("flame", {"seed": 9})
    got2 = d2.aggregate(ups, [], global_params=[gt[:300].reshape(3, 100), gt[300:]])
    assert torch.equal(torch.cat([p.reshape(-1) for p in got2]), want)
    # min_cluster_size = K: every client admitted; a refused call leaves the object as it was
    d3 = get_defense("flame", {"min_cluster_size": K, "noise_lambda": 0})
    d3.set_center(gt)
    d3.aggregate(ups, [])
    assert d3.detect_malicious() == [] and d3.get_metrics()["admitted"] == K
    with pytest.raises(ValueError, match="min_cluster_size"):
        d3.aggregate(ups[:5], [])
    assert d3.calls == 1


def test_defense_no_update_and_bad_rows(cuda):
    g, Xs = _rounds(8, 64, 2)
    gg = _vec(g, cuda)
    X = Xs[0].copy()
    X[3, 7] = np.nan
    d = get_defense("flame", {})
    out = d.aggregate_flat(ClientMatrix(_vec(X, cuda), 64, [(64,)]), [], global_flat=gg)
    m = d.get_metrics()
    assert torch.isfinite(out).all() and m["bad_rows"] and not m["no_update"] and 3 in d.detect_malicious()
    X[:4, 3] = np.inf
    out = d.aggregate_flat(ClientMatrix(_vec(X, cuda), 64, [(64,)]), [], global_flat=gg)
    m = d.get_metrics()
    assert torch.equal(out, gg) and m["no_update"] and m["bad_rows"] and m["admitted"] == 0 and m["sigma"] == 0.0
    assert d.detect_malicious() == list(range(8)) and d.client_weights == [0.0] * 8


ENGINE_SEED = 42


def test_engine_round(cuda, monkeypatch):
    """TINY, K = 8, f = 2, model replacement, torch order.  The engine takes the
    all-gather exchange and hands the defense the round's global model: each
    round's new global model is a second defense object (same seed, so the same
    draw_stream per call) applied to the engine's client matrix and the round's
    starting model."""
    monkeypatch.setenv("FLR_ORDER", "torch")
    kw = dict(num_clients=8, batch=4, defense="flame", defense_cfg={"seed": 3}, attack="model_replacement",
              num_attackers=2, seed=ENGINE_SEED)
    eng = RoundEngine(TINY, RoundConfig(**kw), TrainConfig(local_steps=2), cuda)
    assert eng.exchange == "allgather" and not eng.train_order and eng._wants_global
    twin = get_defense("flame", {"seed": 3})
    start = eng.global_flat.clone()
    for n in range(2):
        got = eng.run_round().clone()
        assert torch.isfinite(got).all() and not torch.equal(got, start)
        want = twin.aggregate_flat(eng.full, [], global_flat=start)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert eng.defense.detect_malicious() == twin.detect_malicious()
        m = eng.defense.get_metrics()
        assert m["calls"] == n + 1 and m["admitted"] >= 5 and not m["no_update"] and m["sigma"] > 0
        start = got
    assert eng.round_index == 2 and not eng.fell_back
    with pytest.raises(ValueError, match="whole client rows"):
        RoundEngine(TINY, RoundConfig(exchange="alltoall", **kw), TrainConfig(local_steps=2), cuda)
