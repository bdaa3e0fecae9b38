"""GPU: the divide-and-conquer defense (flr_dnc_select, flr_rows_mean_keep,
ops.dnc_select, ops.rows_mean_keep, DnCDefense, the round engine's
defense="dnc") against the CPU restatement of tests/dnc_ref.py.  The sampled
columns, the kept set, the count and the flag exactly; the mean bit for bit
(torch.equal); the fp64 scores within 1e-12 of the largest score, which covers
the order of the fixed-order fp64 sums only (the reference's Gram entries and
matrix-vector products are numpy's; reordering the Gram sum moved the scores by
3.3e-15 of the largest at the most).  The kept set can only agree when no two
scores around the cut are that close: every test asserts the reference's margin
first, so a borderline seed fails loudly there and not as a kernel bug (the
seeds below were checked on the CPU: every margin is above 0.01)."""
import functools

import numpy as np
import pytest
import torch

import dnc_ref
from flr import _capi, ops
from flr.defenses import get_defense
from flr.matrix import ClientMatrix
from flr.models.multimodal import TINY
from flr.round import RoundConfig, RoundEngine
from flr.train import TrainConfig

pytestmark = pytest.mark.gpu

# (K, P, ldx - P, b, f): one client; b == P, the one-coordinate gather of an odd
# ldx; a few clients; uneven strata, K no multiple of a wave; 130 rows (three
# waves of the spectral workgroup, five k slices); 300 rows (19 Gram tiles a
# side, three k slices); the row limit (one k slice)
CASES = [(1, 5, 3, 5, 0), (5, 7, 3, 7, 1), (8, 64, 0, 16, 2), (33, 1027, 1, 200, 6), (130, 5000, 24, 1000, 26),
         (300, 600, 0, 128, 60), (1024, 256, 0, 64, 100)]
DATA_SEED = 1
SEED = 7
POWER = 32
MARGIN = 1e-6
FILL = -77.0  # the padding columns' content


@functools.lru_cache(maxsize=None)
def _rows(K, P, f):
    return dnc_ref.alie_rows(K, P, f, seed=DATA_SEED)


@functools.lru_cache(maxsize=None)
def _ref(K, P, b, f, niters=1):
    return dnc_ref.dnc_select(_rows(K, P, f), b, niters, f, POWER, seed=SEED)


def _same(a, b):
    """torch.equal with NaN == NaN."""
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())


def _padded(X, pad, cuda):
    data = torch.full((X.shape[0], X.shape[1] + pad), FILL)
    data[:, :X.shape[1]] = X
    return data, data.to(cuda)


def _run_and_compare(cuda, X, pad, b, niters, nremove, ref, seed=SEED, cols=None):
    """X inside a padded layout -> the kernel; everything against ref; X and the
    padding columns untouched.  Returns the device outputs."""
    want_cols, want_scores, want_keep, want_count, want_flag, margin = ref
    print("reference margin", margin)
    assert margin > MARGIN
    K, P = X.shape
    data, Dg = _padded(X, pad, cuda)
    cg = None if cols is None else torch.as_tensor(cols, dtype=torch.int64).to(cuda).contiguous()
    keep, count, scores, used, flags = ops.dnc_select(Dg[:, :P], b, niters, nremove, POWER, seed=seed, cols=cg,
                                                      diagnostics=True)
    assert np.array_equal(used.cpu().numpy(), want_cols)
    got = scores.cpu().numpy()
    assert np.array_equal(np.isposinf(got), np.isposinf(want_scores)) and not np.isnan(got).any()
    fin = np.isfinite(want_scores)
    top = float(want_scores[fin].max()) if fin.any() else 0.0
    err = float(np.abs(got[fin] - want_scores[fin]).max()) if fin.any() else 0.0
    print("scores: max error relative to the largest score", err / top if top > 0 else err)
    assert err <= 1e-12 * top
    assert torch.equal(keep.cpu(), want_keep)
    assert count.cpu().tolist() == [want_count] and flags.cpu().tolist() == [want_flag]
    assert _same(Dg.cpu(), data)
    # without the optional outputs: the same selection
    keep2, count2 = ops.dnc_select(Dg[:, :P], b, niters, nremove, POWER, seed=seed, cols=cg)
    assert torch.equal(keep2, keep) and torch.equal(count2, count)
    return Dg, keep, count, scores, used, flags


@pytest.mark.parametrize("K,P,pad,b,f", CASES)
def test_select_matches_reference(cuda, K, P, pad, b, f):
    ref = _ref(K, P, b, f)
    assert ref[3] == K - f and ref[4] == 0
    if K >= 33:   # the colluders are what the rule removes
        assert ref[2][:f].sum() == 0
    Dg, keep, _, _, _, _ = _run_and_compare(cuda, _rows(K, P, f), pad, b, 1, f, ref)
    # the aggregate: the kept rows' mean, the reference's bits
    assert torch.equal(ops.rows_mean_keep(Dg[:, :P], keep).cpu(), dnc_ref.rows_mean_keep(_rows(K, P, f), ref[2]))


def test_three_iterations_intersect(cuda):
    K, P, pad, b, f = 33, 1027, 1, 200, 6
    ref = _ref(K, P, b, f, niters=3)
    assert len({tuple(c) for c in ref[0]}) == 3
    _, _, _, scores, _, _ = _run_and_compare(cuda, _rows(K, P, f), pad, b, 3, f, ref)
    # a lone removal per iteration on few clients: the intersection is smaller than any one set
    K, P, b = 8, 64, 16
    X = _rows(K, P, 2)
    ref = dnc_ref.dnc_select(X, b, 3, 2, POWER, seed=SEED)
    _run_and_compare(cuda, X, 0, b, 3, 2, ref)


def test_caller_columns_are_clamped(cuda):
    """Unsorted, a duplicate, one value below 0 and one above P - 1."""
    K, P, f = 8, 64, 2
    cols = [[40, 3, 3, 200, -5, 17], [63, 0, 9, 1 << 40, 12, 11]]
    ref = dnc_ref.dnc_select(_rows(K, P, f), 6, 2, f, POWER, cols=cols)
    assert ref[0].tolist() == [[40, 3, 3, 63, 0, 17], [63, 0, 9, 63, 12, 11]]
    _run_and_compare(cuda, _rows(K, P, f), 0, 6, 2, f, ref, cols=cols)


def test_bad_rows(cuda):
    """A NaN and two infs in sampled columns: score +inf, never kept, the mean
    finite there; a NaN in an unsampled column changes no score."""
    K, P, pad, b, f = 33, 1027, 1, 200, 6
    cols = _ref(K, P, b, f)[0][0]
    unsampled = int(np.setdiff1d(np.arange(P), cols)[100])
    X = _rows(K, P, f).clone()
    X[9, cols[5]] = float("nan")
    X[20, cols[150]] = float("-inf")
    X[25, cols[199]] = float("inf")
    nrem = f + 3   # the cut between the benign rows and the colluders (whose equal scores leave no margin)
    ref = dnc_ref.dnc_select(X, b, 1, nrem, POWER, seed=SEED)
    assert np.isposinf(ref[1][0, [9, 20, 25]]).all() and ref[3] == K - nrem
    assert ref[2][[9, 20, 25]].sum() == 0 and ref[2][:f].sum() == 0
    Dg, keep, _, scores, _, _ = _run_and_compare(cuda, X, pad, b, 1, nrem, ref)
    agg = ops.rows_mean_keep(Dg[:, :P], keep).cpu()
    assert torch.isfinite(agg).all() and torch.equal(agg, dnc_ref.rows_mean_keep(X, ref[2]))
    Y = _rows(K, P, f).clone()
    Y[9, unsampled] = float("nan")
    refy = dnc_ref.dnc_select(Y, b, 1, f, POWER, seed=SEED)
    assert np.array_equal(refy[1], _ref(K, P, b, f)[1]) and refy[2][9] == 1
    Dg, keep, _, _, _, _ = _run_and_compare(cuda, Y, pad, b, 1, f, refy)
    agg = ops.rows_mean_keep(Dg[:, :P], keep).cpu()
    assert agg.isnan().sum() == 1 and _same(agg, dnc_ref.rows_mean_keep(Y, refy[2]))
    # every row bad: nothing is kept, the flag is set, the mean is NaN
    Z = _rows(K, P, f).clone()
    Z[:, cols[0]] = float("inf")
    refz = dnc_ref.dnc_select(Z, b, 1, f, POWER, seed=SEED)
    assert refz[3] == 0 and refz[4] == 1
    Dg, keep, _, _, _, _ = _run_and_compare(cuda, Z, pad, b, 1, f, refz)
    assert ops.rows_mean_keep(Dg[:, :P], keep).isnan().all()


def test_identical_rows_and_no_removal(cuda):
    row = torch.randint(-8, 9, (40,), generator=torch.Generator().manual_seed(0)).float()
    X = row.repeat(6, 1)
    ref = dnc_ref.dnc_select(X, 10, 2, 2, POWER, seed=3)
    assert (ref[1] == 0).all() and ref[2].tolist() == [1, 1, 1, 1, 0, 0]
    _, _, _, scores, _, _ = _run_and_compare(cuda, X, 0, 10, 2, 2, ref, seed=3)
    assert (scores == 0).all()
    K, P, pad, b, f = 33, 1027, 1, 200, 6
    ref = dnc_ref.dnc_select(_rows(K, P, f), b, 2, 0, POWER, seed=SEED)
    assert ref[2].all() and ref[3] == K
    _run_and_compare(cuda, _rows(K, P, f), pad, b, 2, 0, ref)


def test_empty_intersection_falls_back_to_the_first_set(cuda):
    """Two iterations on disjoint caller-supplied column sets, each removing the
    half of the clients that varies there: niters * nremove = K, nothing survives
    both, keep is iteration 0's set and the flag is up."""
    K, P = 8, 8
    gen = torch.Generator().manual_seed(5)
    amp = torch.tensor([3.0, -3.0, 4.0, -4.0])
    X = 1.0 + 0.01 * torch.randn(K, P, generator=gen)
    X[:4, :4] = 1.0 + amp[:, None] * torch.tensor([1.0, 0.5, -1.0, 2.0])
    X[4:, 4:] = 1.0 + amp[:, None] * torch.tensor([2.0, -1.0, 1.0, 0.5])
    cols = [[0, 1, 2, 3], [4, 5, 6, 7]]
    ref = dnc_ref.dnc_select(X, 4, 2, 4, POWER, cols=cols)
    assert ref[4] == 1 and ref[2].tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and ref[3] == 4
    one = dnc_ref.dnc_select(X, 4, 1, 4, POWER, cols=cols[:1])
    assert torch.equal(one[2], ref[2]) and one[4] == 0
    _run_and_compare(cuda, X, 0, 4, 2, 4, ref, cols=cols)


def test_errors_leave_the_outputs_alone(cuda):
    K, P, ld, b = 6, 40, 48, 10
    D = torch.randn(K, ld, generator=torch.Generator().manual_seed(3)).to(cuda)
    keep = torch.full((K,), 9, dtype=torch.int32, device=cuda)
    count = torch.full((1,), 9, dtype=torch.int32, device=cuda)
    scores = torch.full((2 * K,), FILL, dtype=torch.float64, device=cuda)
    used = torch.full((2 * b,), 9, dtype=torch.int64, device=cuda)
    flags = torch.full((1,), 9, dtype=torch.int32, device=cuda)
    out = torch.full((P,), FILL, device=cuda)
    lib = _capi.lib()
    need = lib.flr_dnc_workspace(K, b)
    assert need > 0 and lib.flr_dnc_workspace(0, b) == 0 and lib.flr_dnc_workspace(K, 0) == 0
    ws_t, ws = ops._ws(need, cuda)
    x, kp, ct = D.data_ptr(), keep.data_ptr(), count.data_ptr()
    A, W, U = _capi.FLR_ERR_ARG, _capi.FLR_ERR_WORKSPACE, _capi.FLR_ERR_UNSUPPORTED
    #        X  K  P  ldx b  niters nremove power keep count ws  bytes
    bad = [((None, K, P, ld, b, 2, 1, 4, kp, ct, ws, need), A),      # null X
           ((x, K, P, ld, b, 2, 1, 4, None, ct, ws, need), A),       # null keep
           ((x, K, P, ld, b, 2, 1, 4, kp, None, ws, need), A),       # null count
           ((x, 0, P, ld, b, 2, 0, 4, kp, ct, ws, need), A),         # K < 1
           ((x, K, P, ld, 0, 2, 1, 4, kp, ct, ws, need), A),         # b < 1
           ((x, K, P, ld, P + 1, 2, 1, 4, kp, ct, ws, need), A),     # b > P
           ((x, K, P, P - 1, b, 2, 1, 4, kp, ct, ws, need), A),      # ldx < P
           ((x, K, P, ld, b, 0, 1, 4, kp, ct, ws, need), A),         # niters < 1
           ((x, K, P, ld, b, 2, 1, 0, kp, ct, ws, need), A),         # power_iters < 1
           ((x, K, P, ld, b, 2, -1, 4, kp, ct, ws, need), A),        # nremove < 0
           ((x, K, P, ld, b, 2, K, 4, kp, ct, ws, need), A),         # nremove > K - 1
           ((x, 1025, P, ld, b, 2, 1, 4, kp, ct, ws, need), U),      # K > 1024
           ((x, K, 70000, 70000, 65537, 2, 1, 4, kp, ct, ws, need), U),   # b > 65536
           ((x, K, P, ld, b, 17, 1, 4, kp, ct, ws, need), U),        # niters > 16
           ((x, K, P, ld, b, 2, 1, 1025, kp, ct, ws, need), U),      # power_iters > 1024
           ((x, K, P, ld, b, 2, 1, 4, kp, ct, None, need), W),       # no workspace
           ((x, K, P, ld, b, 2, 1, 4, kp, ct, ws, need - 1), W),     # too small
           ((x, K, P, ld, b, 2, 1, 4, kp, ct, ws + 128, need + 128), W)]   # not 256-B aligned
    for (X, k, p, l, bb, ni, nr, pw, kk, cc, w, wb), code in bad:
        got = lib.flr_dnc_select(X, k, p, l, bb, ni, nr, pw, SEED, None, kk, cc, scores.data_ptr(), used.data_ptr(),
                                 flags.data_ptr(), w, wb, None)
        assert got == code, (k, p, l, bb, ni, nr, pw, got, code)
    o = out.data_ptr()
    for args, code in [((None, K, P, ld, kp, o), A), ((x, K, P, ld, None, o), A), ((x, K, P, ld, kp, None), A),
                       ((x, 0, P, ld, kp, o), A), ((x, K, -1, ld, kp, o), A), ((x, K, P, P - 1, kp, o), A),
                       ((x, 4097, P, ld, kp, o), U)]:
        assert lib.flr_rows_mean_keep(*args, None) == code, args
    torch.cuda.synchronize()
    assert (keep.cpu() == 9).all() and (count.cpu() == 9).all() and (used.cpu() == 9).all()
    assert (flags.cpu() == 9).all() and (scores.cpu() == FILL).all() and (out.cpu() == FILL).all()
    V = D[:, :P]
    for kw in (dict(b=0), dict(b=P + 1), dict(niters=0), dict(power_iters=0), dict(nremove=-1), dict(nremove=K)):
        args = dict(b=b, niters=1, nremove=1, power_iters=4)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.dnc_select(V, **args)
    with pytest.raises(ValueError):
        ops.dnc_select(V, b, 1, 1, 4, cols=torch.zeros((1, b), dtype=torch.int32, device=cuda))
    with pytest.raises(ValueError):
        ops.dnc_select(V, b, 2, 1, 4, cols=torch.zeros((1, b), dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError):
        ops.rows_mean_keep(V, torch.ones(K, dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError):
        ops.rows_mean_keep(V, torch.ones(K - 1, dtype=torch.int32, device=cuda))
    with pytest.raises(_capi.FlrError) as e:
        ops.dnc_select(V, b, 17, 1, 4)
    assert e.value.status == U


# (K, P, ldx - P): one row; ldx % 4 != 0, the one-coordinate form; the float4 form
# over several workgroups; a 3-coordinate tail and more rows than one load group;
# more rows than two waves' ballots
MEAN_SHAPES = [(1, 5, 3), (5, 7, 2), (16, 5000, 24), (33, 1027, 1), (130, 300, 0)]


def _masks(K):
    first = torch.zeros(K, dtype=torch.int32)
    first[: max(1, K // 3)] = 1
    one = torch.zeros(K, dtype=torch.int32)
    one[K // 2] = 7   # any non-zero value keeps the row
    alt = (torch.arange(K) % 2 == 0).to(torch.int32)
    return {"all": torch.ones(K, dtype=torch.int32), "one": one, "alternating": alt, "first": first}


@pytest.mark.parametrize("K,P,pad", MEAN_SHAPES)
def test_rows_mean_keep(cuda, K, P, pad):
    X = torch.randn(K, P, generator=torch.Generator().manual_seed(K + P))
    data, Dg = _padded(X, pad, cuda)
    out = torch.full((P,), 5.0, device=cuda)
    for name, mask in _masks(K).items():
        want = dnc_ref.rows_mean_keep(X, mask)
        got = ops.rows_mean_keep(Dg[:, :P], mask.to(cuda), out=out)
        assert got is out and torch.equal(got.cpu(), want), name
        rows = torch.nonzero(mask).reshape(-1).to(torch.int32)
        assert torch.equal(ops.rows_mean(Dg[:, :P], rows.to(cuda)), got), name
    # rows that do not start on 16 bytes: the one-coordinate form
    if P > 1:
        mask = _masks(K)["alternating"]
        got = ops.rows_mean_keep(Dg[:, 1:P], mask.to(cuda))
        assert torch.equal(got.cpu(), dnc_ref.rows_mean_keep(X[:, 1:], mask))
    # no row kept: 0 / 0
    assert ops.rows_mean_keep(Dg[:, :P], torch.zeros(K, dtype=torch.int32, device=cuda)).isnan().all()
    # a NaN in a skipped row is never read into the sum
    if K > 1:
        mask = _masks(K)["alternating"]
        Y = X.clone()
        Y[1] = float("nan")
        got = ops.rows_mean_keep(Y.to(cuda), mask.to(cuda))
        assert torch.isfinite(got).all() and torch.equal(got.cpu(), dnc_ref.rows_mean_keep(X, mask))
    assert _same(Dg.cpu(), data)


def _attacked(cuda, K, f, P, attack):
    gen = torch.Generator().manual_seed(3)
    base = torch.randn(P, generator=gen)
    Xg = (base + 0.05 * torch.randn(K, P, generator=gen)).to(cuda)
    if attack == "alie":
        ops.collude_rows(Xg, f, ops.COLLUDE_ALIE, 1.0)
    else:
        ops.minmax_rows(Xg, f, ops.MINMAX_MAX, ops.PERTURB_STD)
    return Xg


@pytest.mark.parametrize("attack", ["alie", "min_max"])
@pytest.mark.parametrize("K,f,P", [(11, 2, 4099), (128, 25, 20011)])
def test_defense_removes_the_colluders(cuda, K, f, P, attack):
    Xg = _attacked(cuda, K, f, P, attack)
    X = Xg.cpu()
    want, keep, margin = dnc_ref.dnc(X, min(10000, P), 1, f, POWER, seed=0)
    print("reference margin", margin)
    assert margin > MARGIN and keep.tolist() == [0] * f + [1] * (K - f)
    benign = torch.zeros(P)
    for i in range(f, K):
        benign = benign + X[i]
    benign = benign / torch.tensor(float(K - f))
    assert torch.equal(want, benign)
    d = get_defense("dnc", {"num_malicious": f})
    cm = ClientMatrix(Xg, P, [(P,)])
    agg = d.aggregate_flat(cm, [])
    assert torch.equal(agg.cpu(), benign)
    assert d.rejected_clients == list(range(f)) and d.selected_clients == list(range(f, K))
    assert d.detect_malicious() == list(range(f))
    m = d.get_metrics()
    assert m["kept_count"] == K - f and m["fallback"] is False and m["nremove"] == f
    assert len(m["scores"]) == 1 and m["scores"][0] == d.client_scores and len(d.client_scores) == K
    assert min(d.client_scores[:f]) > max(d.client_scores[f:])


def test_defense_api(cuda):
    """List-of-lists input; call n samples with seed + n; a fresh object with the
    same seed repeats the first call."""
    K, f, P = 11, 2, 4099
    X = _attacked(cuda, K, f, P, "alie").cpu()
    ups = [[X[k, :4000].reshape(40, 100).clone(), X[k, 4000:].clone()] for k in range(K)]
    cfg = {"num_malicious": f, "subsample_dim": 500, "niters": 2, "seed": 11}
    refs = [dnc_ref.dnc_select(X, 500, 2, f, POWER, seed=11 + n) for n in range(2)]
    assert min(r[5] for r in refs) > MARGIN
    d = get_defense("dnc", cfg)
    got1 = d.aggregate(ups, [10] * K)
    assert [tuple(p.shape) for p in got1] == [(40, 100), (99,)] and got1[0].device.type == "cpu"
    flat1 = torch.cat([p.reshape(-1) for p in got1])
    assert torch.equal(flat1, dnc_ref.rows_mean_keep(X, refs[0][2]))
    cols1 = d.sampled_columns().cpu().numpy()
    assert np.array_equal(cols1, refs[0][0]) and d.rejected_clients == [0, 1]
    got2 = d.aggregate(ClientMatrix.from_updates(ups, device=cuda), [])
    assert got2[0].is_cuda
    cols2 = d.sampled_columns().cpu().numpy()
    assert np.array_equal(cols2, refs[1][0]) and not np.array_equal(cols1, cols2)
    assert torch.equal(torch.cat([p.reshape(-1) for p in got2]).cpu(), dnc_ref.rows_mean_keep(X, refs[1][2]))
    assert d.get_metrics()["calls"] == 2
    again = get_defense("dnc", cfg)
    again.aggregate(ups, [])
    assert np.array_equal(again.sampled_columns().cpu().numpy(), cols1)
    assert np.allclose(again.client_scores, refs[0][1][-1], rtol=0, atol=1e-12 * refs[0][1].max())


ENGINE_SEED = 42


def test_engine_round(cuda, monkeypatch):
    """TINY, K = 8, f = 2, ALIE, torch order.  The engine takes the all-gather
    exchange; each round's global model is the reference applied to the
    exchanged (attacked) matrix, round n sampling with seed n; round 2 replays
    the captured training graph."""
    monkeypatch.setenv("FLR_ORDER", "torch")
    kw = dict(num_clients=8, batch=4, defense="dnc", defense_cfg={}, attack="alie", num_attackers=2,
              seed=ENGINE_SEED)
    eng = RoundEngine(TINY, RoundConfig(**kw), TrainConfig(local_steps=2), cuda)
    assert eng.exchange == "allgather" and eng.use_graph and not eng.train_order
    assert eng.defense.num_malicious == 2
    g0 = eng.global_flat.clone().cpu()
    prev = None
    for n in range(2):
        g = eng.run_round().clone().cpu()
        X = eng.full.X.cpu().contiguous()
        want, keep, margin = dnc_ref.dnc(X, min(10000, X.shape[1]), 1, 2, POWER, seed=n)
        print("reference margin, round", n + 1, margin)
        assert margin > MARGIN
        assert torch.isfinite(X).all() and torch.equal(X[0], X[1])     # the colluders' common row
        assert torch.equal(g, want) and not torch.equal(g, g0)
        assert eng.defense.selected_clients == torch.nonzero(keep).reshape(-1).tolist()
        assert eng.defense.get_metrics()["kept_count"] == 6
        if prev is not None:
            assert not torch.equal(X[2:], prev[2:])
        prev = X
    assert eng.round_index == 2 and not eng.fell_back
    with pytest.raises(ValueError, match="whole client rows"):
        RoundEngine(TINY, RoundConfig(exchange="alltoall", **kw), TrainConfig(local_steps=2), cuda)
