"""GPU: FoolsGold (flr_rows_accumulate, flr_rows_gram, flr_foolsgold_weights,
flr_rows_combine_from, their ops wrappers, FoolsGoldDefense, the round engine's
defense="foolsgold") against the CPU restatement of tests/foolsgold_ref.py.

The Gram matrix exactly on integer data (every partial sum is an integer below
2^53, so any summation order gives the same fp64 value: this is the check that
catches a wrong MFMA fragment map) and within the derived bound on real data;
the fp32 passes bit for bit (torch.equal); the weights from the device's own G
within 1e-12 of the host's (only log can differ between the libraries, by a few
ulp, through a logit slope of at most 1 / (0.99 * 0.01) = 101; the measured
error is printed); the defense's alpha within 1e-9 (the Gram bound pushed
through the normalisation with top >= 0.1 and that slope).  The flagged set can
only agree when no pre-clip weight sits at 0: every test asserts the
reference's own margin first, so a borderline seed fails there and not as a
kernel bug.  Every matrix sits in a padded layout filled with a sentinel; the
padding and the inputs must come back unchanged."""
import functools

import numpy as np
import pytest
import torch

import foolsgold_ref as ref
from flr import _capi, ops
from flr.defenses import get_defense
from flr.matrix import ClientMatrix
from flr.models.multimodal import TINY
from flr.round import RoundConfig, RoundEngine
from flr.train import TrainConfig

pytestmark = pytest.mark.gpu

MARGIN = 1e-6
FILL = -77.0  # the padding columns' content

# (K, P, ld - P).  K: below a fragment, one fragment, one past it, one past two,
# one past a block, two past two blocks, five blocks, the limit; P: one column,
# below a group of 4, one LDS tile, three past a multiple of 64 (a ragged last
# tile, a ragged float4), the most the exact test allows.  16-byte loads:
# (16, 64, 0), (17, 1027, 1), (33, 4096, 24), (130, 7, 1), (300, 4096, 0),
# (1024, 64, 24); 4-byte loads: the others (ld % 4 != 0).
GRAM_CASES = [(1, 1, 0), (5, 7, 3), (16, 64, 0), (17, 1027, 1), (33, 4096, 24), (65, 1027, 3), (130, 7, 1),
              (300, 4096, 0), (1024, 64, 24), (1024, 1027, 3)]
# (K, P, ld - P, f): the generator's shapes
DATA_CASES = [(1, 5, 3, 0), (2, 7, 1, 0), (5, 7, 3, 2), (8, 64, 0, 2), (17, 333, 3, 4), (33, 1027, 1, 6),
              (65, 2048, 24, 13), (130, 5000, 24, 26), (300, 600, 0, 60), (1024, 256, 0, 100)]


@functools.lru_cache(maxsize=None)
def _rounds(K, P, f):
    return ref.rounds(K, P, f)


@functools.lru_cache(maxsize=None)
def _run(K, P, f, kappa, use_memory):
    g, Xs = _rounds(K, P, f)
    return ref.run(g, Xs, kappa, use_memory)


def _padded(X, pad, cuda):
    """X (numpy or torch [K, P]) inside a [K, P + pad] layout of FILL: (host copy, device tensor)."""
    X = torch.as_tensor(np.asarray(X), dtype=torch.float32)
    data = torch.full((X.shape[0], X.shape[1] + pad), FILL)
    data[:, :X.shape[1]] = X
    return data, data.to(cuda)


def _vec(v, cuda):
    return torch.as_tensor(np.asarray(v), dtype=torch.float32).to(cuda)


def _check_weights(got, want, atol):
    """(alpha, beta, maxcos, flags) of the device against a reference Weights."""
    alpha, beta, maxcos, flags = (t.cpu().numpy() for t in got)
    print("reference margin", want.margin, "top", want.top)
    assert want.margin > MARGIN
    ea = float(np.abs(alpha - want.alpha).max())
    ec = float(np.abs(maxcos - want.max_cosine).max())
    print("alpha: max abs error", ea, " max_cosine: max abs error", ec)
    assert ea <= atol and ec <= atol
    assert np.array_equal(alpha == 0, want.alpha == 0)
    assert flags.tolist() == [want.flags]
    S = 0.0
    for a in alpha:
        S += float(a)
    want_beta = (alpha / S).astype(np.float32) if S > 0 else np.zeros_like(beta)
    assert np.array_equal(beta, want_beta)


# ---- the Gram matrix ----

@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("K,P,pad", GRAM_CASES)
def test_gram_exact_on_integers(cuda, K, P, pad, centered):
    rng = np.random.default_rng(1000 * K + P)
    A = rng.integers(-8, 9, size=(K, P))
    c = rng.integers(-4, 5, size=P) if centered else None
    D = (A - c[None, :]) if centered else A
    want = D.astype(np.int64) @ D.astype(np.int64).T
    data, Dg = _padded(A.astype(np.float32), pad, cuda)
    cg = _vec(c, cuda) if centered else None
    G = ops.rows_gram(Dg[:, :P], center=cg).cpu().numpy()
    assert G.dtype == np.float64 and G.shape == (K, K)
    assert np.array_equal(G, want.astype(np.float64))
    assert torch.equal(Dg.cpu(), data)
    if centered:
        assert torch.equal(cg.cpu(), torch.as_tensor(c, dtype=torch.float32))


def test_gram_plan_through_the_export():
    """The column chunks are a function of (K, P): one chunk below 256 columns,
    at least three at the exact test's larger shapes; 0 for rejected arguments."""
    lib = _capi.lib()
    assert ops.rows_gram_splits(16, 64) == 1 and ops.rows_gram_splits(1024, 64) == 1
    assert ops.rows_gram_splits(17, 1027) >= 3 and ops.rows_gram_splits(33, 4096) >= 3
    assert ops.rows_gram_splits(1024, 1027) >= 3
    assert int(lib.flr_rows_gram_workspace(16, 64)) == 0
    for K, P in ((17, 1027), (300, 4096), (128, 11800394)):
        s = ops.rows_gram_splits(K, P)
        assert int(lib.flr_rows_gram_workspace(K, P)) == (s * K * K * 8 + 255) // 256 * 256
    s = ops.rows_gram_splits(128, 11800394)                      # 3 block pairs: about 2048 workgroups
    assert 1900 < 3 * s <= 2048
    for K, P in ((0, 5), (5, 0), (1025, 5)):
        assert ops.rows_gram_splits(K, P) == 0 and int(lib.flr_rows_gram_workspace(K, P)) == 0


@pytest.mark.parametrize("K,P,pad,f", [c for c in DATA_CASES if c[0] >= 17])
def test_gram_real_data(cuda, K, P, pad, f):
    """|G - G_numpy| <= 2 * P * 2^-52 * sqrt(G_ii * G_jj): each side is a sum of P
    exact products with at most P - 1 fp64 roundings, so each lies within
    P * 2^-53 * sum|a_ip * a_jp| of the exact sum, and that sum is at most
    n_i * n_j (Cauchy-Schwarz); the factor 2 is slack.  G is symmetric bit for
    bit, a rerun and the other load width give the same bits."""
    g, Xs = _rounds(K, P, f)
    X = Xs[0]
    want = ref.gram(X, g)
    data, Dg = _padded(X, pad, cuda)
    gg = _vec(g, cuda)
    G = ops.rows_gram(Dg[:, :P], center=gg)
    Gn = G.cpu().numpy()
    n = np.sqrt(np.diag(want))
    ratio = float((np.abs(Gn - want) / (2 * P * 2.0 ** -52 * np.outer(n, n))).max())
    print("largest |G - G_numpy| / bound", ratio)
    assert ratio <= 1.0
    assert torch.equal(G, G.T.contiguous())
    assert torch.equal(ops.rows_gram(Dg[:, :P], center=gg), G)
    # the other path: a row stride that allows 16-byte loads against one that does not
    other = 1 if (P + pad) % 4 == 0 else (-(P + pad)) % 4
    _, Dg2 = _padded(X, pad + other, cuda)
    assert ((P + pad) % 4 == 0) != ((P + pad + other) % 4 == 0)
    assert torch.equal(ops.rows_gram(Dg2[:, :P], center=gg), G)
    # without a center, on the differences themselves
    _, Ug = _padded(X - g[None, :], pad, cuda)
    assert torch.equal(ops.rows_gram(Ug[:, :P]), G)
    assert torch.equal(Dg.cpu(), data)


def test_gram_errors(cuda):
    A = torch.zeros((4, 8), device=cuda)
    G = torch.zeros((4, 4), dtype=torch.float64, device=cuda)
    lib, st = _capi.lib(), torch.cuda.current_stream(cuda).cuda_stream
    assert lib.flr_rows_gram(None, 4, 8, 8, None, G.data_ptr(), None, 0, st) == _capi.FLR_ERR_ARG
    assert lib.flr_rows_gram(A.data_ptr(), 4, 8, 8, None, None, None, 0, st) == _capi.FLR_ERR_ARG
    assert lib.flr_rows_gram(A.data_ptr(), 0, 8, 8, None, G.data_ptr(), None, 0, st) == _capi.FLR_ERR_ARG
    assert lib.flr_rows_gram(A.data_ptr(), 4, 0, 8, None, G.data_ptr(), None, 0, st) == _capi.FLR_ERR_ARG
    assert lib.flr_rows_gram(A.data_ptr(), 4, 8, 7, None, G.data_ptr(), None, 0, st) == _capi.FLR_ERR_ARG
    assert lib.flr_rows_gram(A.data_ptr(), 1025, 8, 8, None, G.data_ptr(), None, 0, st) == _capi.FLR_ERR_UNSUPPORTED
    # more than one chunk needs the workspace
    assert ops.rows_gram_splits(4, 1027) > 1
    assert lib.flr_rows_gram(A.data_ptr(), 4, 1027, 1027, None, G.data_ptr(), None, 0, st) == _capi.FLR_ERR_WORKSPACE
    with pytest.raises(ValueError):
        ops.rows_gram(torch.zeros((1025, 4), device=cuda))
    with pytest.raises(ValueError):
        ops.rows_gram(A, center=torch.zeros(7, device=cuda))
    with pytest.raises(RuntimeError):
        ops.rows_gram(torch.zeros((4, 8)))
    torch.cuda.synchronize()
    assert not G.any()


# ---- the fp32 passes ----

@pytest.mark.parametrize("K,P,pad,f", [(1, 5, 3, 0), (5, 7, 3, 2), (17, 333, 3, 4), (33, 1027, 1, 6),
                                       (65, 2048, 24, 13), (130, 5000, 24, 26)])
def test_accumulate(cuda, K, P, pad, f):
    g, Xs = _rounds(K, P, f)
    data, Dg = _padded(Xs[0], pad, cuda)
    hpad = (pad + 1) % 4 if pad else 0            # a stride of its own
    H0 = np.random.default_rng(5).standard_normal((K, P)).astype(np.float32)
    hdata, Hg = _padded(H0, hpad, cuda)
    gg = _vec(g, cuda)
    got = ops.rows_accumulate_(Hg[:, :P], Dg[:, :P], gg)
    want = torch.as_tensor(ref.accumulate(H0, Xs[0], g))
    assert torch.equal(got.cpu(), want)
    assert torch.equal(Hg[:, P:].cpu(), hdata[:, P:]) and torch.equal(Dg.cpu(), data)
    assert torch.equal(gg.cpu(), torch.as_tensor(g))
    # a second round on top
    _, Dg2 = _padded(Xs[1], pad, cuda)
    ops.rows_accumulate_(Hg[:, :P], Dg2[:, :P], gg)
    assert torch.equal(Hg[:, :P].cpu(), torch.as_tensor(ref.accumulate(want.numpy(), Xs[1], g)))


@pytest.mark.parametrize("K,P,pad,f", [(1, 5, 3, 0), (5, 7, 3, 2), (17, 333, 3, 4), (33, 1027, 1, 6),
                                       (65, 2048, 24, 13), (130, 5000, 24, 26)])
def test_combine_with_the_device_weights(cuda, K, P, pad, f):
    """The combination is fed the device's own beta; a NaN row with beta = 0
    leaves out finite; all-zero beta gives the center's bits."""
    g, Xs = _rounds(K, P, f)
    X = Xs[0].copy()
    data, Dg = _padded(X, pad, cuda)
    gg = _vec(g, cuda)
    _, beta = ops.foolsgold_weights(ops.rows_gram(Dg[:, :P], center=gg), 0.1)
    b = beta.cpu().numpy()
    assert (b[:f] == 0).all() and (b[f:] > 0).all() if K >= 8 else True
    out = ops.rows_combine_from(Dg[:, :P], gg, beta)
    assert torch.equal(out.cpu(), torch.as_tensor(ref.combine(X, g, b)))
    assert torch.equal(Dg.cpu(), data)
    if f:                                          # a rejected row is not read
        X[0, P // 2] = np.nan
        X[f - 1, 0] = np.inf
        _, Dn = _padded(X, pad, cuda)
        out2 = ops.rows_combine_from(Dn[:, :P], gg, beta)
        assert torch.isfinite(out2).all() and torch.equal(out2, out)
    zero = torch.zeros(K, device=cuda)
    assert torch.equal(ops.rows_combine_from(Dg[:, :P], gg, zero), gg)
    with pytest.raises(ValueError):
        ops.rows_combine_from(Dg[:, :P], gg, beta, out=gg)
    with pytest.raises(ValueError):
        ops.rows_combine_from(Dg[:, :P], gg, beta[:-1] if K > 1 else torch.zeros(2, device=cuda))


# ---- the weights ----

@pytest.mark.parametrize("kappa", [1.0, 0.1])
@pytest.mark.parametrize("K,P,pad,f", DATA_CASES)
def test_weights_from_the_device_gram(cuda, K, P, pad, f, kappa):
    """The device's G through the host reference: alpha and max_cosine within
    1e-12 absolute, the set alpha == 0 and the flags exactly, beta the bits of
    float32(alpha_dev / sum(alpha_dev))."""
    g, Xs = _rounds(K, P, f)
    _, Dg = _padded(Xs[0], pad, cuda)
    G = ops.rows_gram(Dg[:, :P], center=_vec(g, cuda))
    want = ref.weights(G.cpu().numpy(), kappa)
    assert (want.alpha[:f] == 0).all()
    got = ops.foolsgold_weights(G, kappa, diagnostics=True)
    _check_weights(got, want, 1e-12)
    a2, b2 = ops.foolsgold_weights(G, kappa)      # without the optional outputs
    assert torch.equal(a2, got[0]) and torch.equal(b2, got[1])


def test_weights_edge_cases(cuda):
    """Zero rows, bad rows, every row bad, identical clients, one client."""
    g, Xs = _rounds(8, 64, 2)
    A = (Xs[0] - g[None, :]).astype(np.float32)
    A[5] = 0.0
    B = A.copy()
    B[3, 7] = np.nan
    B[6, 1] = np.inf
    C = B.copy()
    C[:, 0] = np.nan
    same = np.ones((6, 64), dtype=np.float32)
    for M, flags in ((A, 0), (B, 2), (C, 3), (same, 1), (A[:1], 0), (C[:1], 3)):
        G = ops.rows_gram(_vec(M, cuda))
        want = ref.weights(G.cpu().numpy(), 1.0)
        assert want.flags == flags
        got = ops.foolsgold_weights(G, 1.0, diagnostics=True)
        alpha, beta, maxcos, fl = (t.cpu().numpy() for t in got)
        assert fl.tolist() == [flags]
        assert np.isfinite(alpha).all() and np.isfinite(beta).all() and np.isfinite(maxcos).all()
        assert np.abs(alpha - want.alpha).max() <= 1e-12 and np.abs(maxcos - want.max_cosine).max() <= 1e-12
        assert np.array_equal(alpha == 0, want.alpha == 0)
        if flags & 1:
            assert not alpha.any() and not beta.any()
    with pytest.raises(ValueError):
        ops.foolsgold_weights(torch.zeros((3, 3), dtype=torch.float64, device=cuda), 0.0)
    with pytest.raises(ValueError):
        ops.foolsgold_weights(torch.zeros((3, 3), dtype=torch.float64, device=cuda), float("nan"))
    with pytest.raises(ValueError):
        ops.foolsgold_weights(torch.zeros((3, 4), dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError):
        ops.foolsgold_weights(torch.zeros((3, 3), dtype=torch.float32, device=cuda))


# ---- the defense ----

@pytest.mark.parametrize("use_memory", [True, False])
@pytest.mark.parametrize("K,P,pad,f,kappa", [(8, 64, 0, 2, 1.0), (33, 1027, 1, 6, 0.1), (130, 5000, 24, 26, 0.1),
                                             (1024, 256, 0, 100, 1.0)])
def test_defense_three_calls(cuda, K, P, pad, f, kappa, use_memory):
    g, Xs = _rounds(K, P, f)
    want = _run(K, P, f, kappa, use_memory)
    d = get_defense("foolsgold", {"confidence": kappa, "use_memory": use_memory})
    gg = _vec(g, cuda)
    for n, X in enumerate(Xs):
        agg_ref, wt, H = want[n]
        print("call", n + 1, "reference margin", wt.margin, "top", wt.top)
        assert wt.margin > MARGIN and wt.top >= 0.1
        data, Dg = _padded(X, pad, cuda)
        cm = ClientMatrix(Dg, P, [(P,)])
        out = d.aggregate_flat(cm, [], global_flat=gg)
        alpha = np.asarray(d.client_weights)
        err = float(np.abs(alpha - wt.alpha).max())
        print("alpha: max abs error", err)
        assert err <= 1e-9
        flagged = np.nonzero(wt.alpha == 0)[0].tolist()
        assert d.detect_malicious() == flagged and flagged[:f] == list(range(f))
        assert torch.equal(out.cpu(), torch.as_tensor(ref.combine(X, g, d._beta.cpu().numpy())))
        # the reference's own beta may differ in the last bit: one fp32 ulp of |x| < 8 in out
        assert np.abs(out.cpu().numpy() - agg_ref).max() <= 2.0 ** -21
        assert torch.equal(Dg.cpu(), data) and torch.equal(gg.cpu(), torch.as_tensor(g))
        if use_memory:
            assert torch.equal(d.history().cpu(), torch.as_tensor(H))
        else:
            assert d.history() is None
        m = d.get_metrics()
        assert m["calls"] == n + 1 and m["weights"] == alpha.tolist() and not m["no_update"] and not m["bad_rows"]
        assert m["confidence"] == kappa and m["use_memory"] is use_memory and len(m["max_cosine"]) == K
        assert np.abs(np.asarray(m["max_cosine"]) - wt.max_cosine).max() <= 1e-9


def test_defense_reset_and_shape_change(cuda):
    K, P, f = 8, 64, 2
    g, Xs = _rounds(K, P, f)
    want = _run(K, P, f, 0.1, True)
    gg = _vec(g, cuda)
    cms = [ClientMatrix(_vec(X, cuda), P, [(P,)]) for X in Xs]
    d = get_defense("foolsgold", {"confidence": 0.1})
    d.aggregate_flat(cms[0], [], global_flat=gg)
    d.aggregate_flat(cms[1], [], global_flat=gg)
    assert np.abs(np.asarray(d.client_weights) - want[1][1].alpha).max() <= 1e-9
    # another K or P while the history exists
    with pytest.raises(ValueError, match="history"):
        d.aggregate_flat(ClientMatrix(_vec(Xs[0][:5], cuda), P, [(P,)]), [], global_flat=gg)
    with pytest.raises(ValueError, match="history"):
        d.aggregate_flat(ClientMatrix(_vec(Xs[0][:, :60], cuda), 60, [(60,)]), [], global_flat=gg[:60])
    assert torch.equal(d.history().cpu(), torch.as_tensor(want[1][2]))
    # reset: the next call is a first call again, of any shape
    d.reset()
    assert d.history() is None
    d.aggregate_flat(cms[0], [], global_flat=gg)
    assert np.abs(np.asarray(d.client_weights) - want[0][1].alpha).max() <= 1e-9
    assert torch.equal(d.history().cpu(), torch.as_tensor(want[0][2]))
    d.reset()
    d.aggregate_flat(ClientMatrix(_vec(Xs[0][:5], cuda), P, [(P,)]), [], global_flat=gg)
    assert tuple(d.history().shape) == (5, P)
    d.reset()
    with pytest.raises(ValueError, match="coordinates"):
        d.aggregate_flat(cms[0], [], global_flat=gg[:-1])


def test_defense_without_a_global_model(cuda):
    """The drop-in aggregate(updates, num_examples): list-of-lists in, the
    center the lower median on the first call, then the previous result, then
    set_center / global_params."""
    K, P, f = 17, 333, 4
    g, Xs = _rounds(K, P, f)
    X = torch.as_tensor(Xs[0])
    ups = [[X[k, :300].reshape(3, 100).clone(), X[k, 300:].clone()] for k in range(K)]

    def one(center, H0):
        H = ref.accumulate(H0, Xs[0], center)
        wt = ref.weights(ref.gram(H), 1.0)
        assert wt.margin > MARGIN and wt.top >= 0.1
        return H, wt

    def flat(params):
        assert [tuple(p.shape) for p in params] == [(3, 100), (33,)]
        return torch.cat([p.reshape(-1) for p in params]).cpu()

    d = get_defense("foolsgold", {})
    c1 = torch.median(X, dim=0).values.numpy()
    H1, w1 = one(c1, np.zeros_like(Xs[0]))
    got1 = d.aggregate(ups, [10] * K)
    assert got1[0].device.type == "cpu"
    assert d.detect_malicious() == np.nonzero(w1.alpha == 0)[0].tolist() and d.detect_malicious()[:f] == [0, 1, 2, 3]
    out1 = flat(got1)
    assert torch.equal(out1, torch.as_tensor(ref.combine(Xs[0], c1, d._beta.cpu().numpy())))
    assert torch.equal(d.history().cpu(), torch.as_tensor(H1))
    got1[0].zero_()   # the caller's copy is its own
    # second call: from the first call's output
    H2, w2 = one(out1.numpy(), H1)
    got2 = d.aggregate(ClientMatrix.from_updates(ups, device=cuda), [])
    assert got2[0].is_cuda and torch.equal(d.history().cpu(), torch.as_tensor(H2))
    assert np.abs(np.asarray(d.client_weights) - w2.alpha).max() <= 1e-9
    # set_center wins over the previous result, global_params over set_center
    H3, _ = one(g, H2)
    d.set_center([torch.as_tensor(g[:300]).reshape(3, 100), torch.as_tensor(g[300:])])
    d.aggregate(ups, [])
    assert torch.equal(d.history().cpu(), torch.as_tensor(H3))
    H4, _ = one(c1, H3)
    d.set_center(torch.as_tensor(g))
    d.aggregate(ups, [], global_params=[torch.as_tensor(c1[:300]).reshape(3, 100), torch.as_tensor(c1[300:])])
    assert torch.equal(d.history().cpu(), torch.as_tensor(H4)) and d.get_metrics()["calls"] == 4


ENGINE_SEED = 42


def test_engine_round(cuda, monkeypatch):
    """TINY, K = 8, f = 2, IPM, torch order.  The engine takes the all-gather
    exchange, runs the colluding pass before the defense and hands the defense
    the round's global model: each round's new global model is the four ops
    composed by hand on the engine's client matrix and the round's starting
    model; the colluders' identical rows are flagged."""
    monkeypatch.setenv("FLR_ORDER", "torch")
    kw = dict(num_clients=8, batch=4, defense="foolsgold", defense_cfg={}, attack="ipm", num_attackers=2,
              seed=ENGINE_SEED)
    eng = RoundEngine(TINY, RoundConfig(**kw), TrainConfig(local_steps=2), cuda)
    assert eng.exchange == "allgather" and not eng.train_order and eng._wants_global
    H = None
    start = eng.global_flat.clone()
    for n in range(2):
        got = eng.run_round().clone()
        X = eng.full.X
        assert torch.isfinite(X).all() and torch.equal(X[0], X[1]) and not torch.equal(X[1], X[2])
        if H is None:
            H = torch.zeros_like(X.contiguous())
        ops.rows_accumulate_(H, X, start)
        alpha, beta, _, flags = ops.foolsgold_weights(ops.rows_gram(H), 1.0, diagnostics=True)
        want = ops.rows_combine_from(X, start, beta)
        assert torch.equal(got, want) and not torch.equal(got, start)
        assert torch.equal(eng.defense.history(), H)
        flagged = eng.defense.detect_malicious()
        assert 0 in flagged and 1 in flagged and len(flagged) < 8
        assert flagged == torch.nonzero(alpha == 0).reshape(-1).tolist() and flags.item() == 0
        assert eng.defense.get_metrics()["calls"] == n + 1
        start = got
    assert eng.round_index == 2 and not eng.fell_back
    with pytest.raises(ValueError, match="whole client rows"):
        RoundEngine(TINY, RoundConfig(exchange="alltoall", **kw), TrainConfig(local_steps=2), cuda)
