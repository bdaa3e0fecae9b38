"""GPU: Bulyan (flr_krum_select_iter, flr_median_window_mean_rows, BulyanDefense)
against the numpy reference of tests/bulyan_ref.py — bit for bit: the window
mean's adds are sequential fp32 in rank order, the selection's scores numpy's
pairwise sums, so neither has a tolerance."""
import functools
import os
import socket

import numpy as np
import pytest
import torch

from bulyan_ref import SELECTION_SHAPES, iter_krum, sizes, window_mean
from flr import _capi, ops
from flr.defenses import get_defense
from flr.matrix import ClientMatrix
from flr.shard import Comm, CoordPlan, CoordSlice
from flr.workload import split_rows, update_matrix
from oracle import aggregation as orc

pytestmark = pytest.mark.gpu

WP, WK = 2049, 140  # the window-mean tests: a partial last workgroup; the row-subset matrix's K


@functools.lru_cache(maxsize=None)
def _window_data():
    """The three [WK, WP] data sets (made once): randn; quarter-rounded randn
    (many exact ties: the tie rule); randn with a block of columns whose rows
    are all equal.  And one row shuffle."""
    rng = np.random.default_rng(2018)
    a = rng.standard_normal((WK, WP)).astype(np.float32)
    b = (np.round(rng.standard_normal((WK, WP)) * 4) / 4).astype(np.float32)
    c = rng.standard_normal((WK, WP)).astype(np.float32)
    c[:, 100:400] = c[0, 100:400]
    return (a, b, c), rng.permutation(WK).astype(np.int32)


WINDOW_CASES = [(5, 1), (7, 3), (8, 4), (9, 5), (16, 8), (17, 9), (33, 11), (64, 32), (65, 33), (78, 28),
                (128, 64), (128, 128), (128, 1)]


@pytest.mark.parametrize("subset", [False, True], ids=["all_rows", "row_subset"])
@pytest.mark.parametrize("m,beta", WINDOW_CASES)
def test_window_mean_bitwise(cuda, m, beta, subset):
    sets, perm = _window_data()
    for S in sets:
        if subset:
            X = torch.from_numpy(S).to(cuda)
            rows = torch.from_numpy(perm[:m].copy()).to(cuda)
            want = window_mean(S[perm[:m]], beta)
        else:
            X = torch.from_numpy(S[:m].copy()).to(cuda)
            rows = None
            want = window_mean(S[:m], beta)
        got = ops.median_window_mean(X, beta, rows=rows)
        assert np.array_equal(got.cpu().numpy(), want)
        if beta == 1:  # the lower median itself
            assert torch.equal(got, ops.median_lower(X, rows=rows))


def test_window_mean_nan_rule(cuda):
    m, beta, P = 9, 5, 300
    rng = np.random.default_rng(9)
    S = rng.standard_normal((m, P)).astype(np.float32)
    S[3, 10] = np.nan                      # 1 NaN
    S[[0, 2, 4, 8], 70] = np.nan           # 4 = m - beta: the five finite values
    S[[1, 2, 5, 6, 7], 200] = np.nan       # 5: one would be taken
    want = window_mean(S, beta)
    assert np.isfinite(want[[10, 70]]).all() and np.isnan(want[200]) and np.isnan(want).sum() == 1
    got = ops.median_window_mean(torch.from_numpy(S).to(cuda), beta).cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True)
    fin = np.sort(S[:, 70])[:5]
    acc = np.float32(0)
    for x in fin:
        acc = np.float32(acc + x)
    assert got[70] == np.float32(acc / np.float32(5))


def test_window_mean_row_limit(cuda):
    X = torch.zeros((129, 64), device=cuda)
    with pytest.raises(_capi.FlrError) as e:
        ops.median_window_mean(X, 3)
    assert e.value.status == _capi.FLR_ERR_UNSUPPORTED


def test_window_is_not_a_symmetric_trim(cuda):
    """theta = 78, beta = 28 (C3's sizes): the window around the median is
    lopsided on most coordinates, so it is not ranks [25, 53)."""
    S = _window_data()[0][0][:78]
    X = torch.from_numpy(S.copy()).to(cuda)
    win = ops.median_window_mean(X, 28)
    trim = ops.trimmed_mean(X, 25)
    share = ((win - trim).abs() > 1e-6).float().mean().item()
    print(f"window != trim on {share:.3f} of the columns")
    assert share >= 0.5


@functools.lru_cache(maxsize=None)
def _selection_case(K, f, P):
    X = update_matrix(K, P, f, seed=K, device="cuda:0")
    dist = orc.distance_matrix(split_rows(X[:, :P].cpu(), P, [(P,)]))
    return X, dist


@pytest.mark.parametrize("K,f,P", SELECTION_SHAPES)
def test_iterated_selection(cuda, K, f, P):
    _, dist = _selection_case(K, f, P)  # D from the oracle on the CPU: independent of the distance kernels
    theta, _ = sizes(K, f)
    want, _ = iter_krum(dist, f, theta)
    D = torch.from_numpy(dist).to(cuda)
    scores, picked = ops.krum_select_iter(D, f, theta)
    picked = picked.cpu().tolist()
    assert picked[:theta] == want
    rest = picked[theta:]
    assert rest == sorted(rest) and sorted(picked) == list(range(K))
    assert torch.equal(scores, ops.krum_select(D, f)[0])


def test_iterated_selection_tie_goes_to_the_lowest_index(cuda):
    K, f, P = 9, 1, 300
    gen = torch.Generator().manual_seed(3)
    X = torch.randn(K, P, generator=gen)
    X[2] = 0.05 * torch.randn(P, generator=gen)  # the most central row, twice: an exact score tie
    X[6] = X[2]
    dist = orc.distance_matrix(split_rows(X, P, [(P,)]))
    theta = K - 2 * f
    want, first = iter_krum(dist, f, theta)
    assert first[2] == first[6] == min(first) and want[0] == 2
    scores, picked = ops.krum_select_iter(torch.from_numpy(dist).to(cuda), f, theta)
    assert picked.cpu().tolist()[:theta] == want
    assert scores.cpu().tolist() == first


def test_iterated_selection_picks_everyone_at_f0(cuda):
    K, P = 13, 100
    _, dist = _selection_case(K, 0, P)
    want, _ = iter_krum(dist, 0, K)
    _, picked = ops.krum_select_iter(torch.from_numpy(dist).to(cuda), 0, K)
    assert picked.cpu().tolist() == want and sorted(want) == list(range(K))


@pytest.mark.parametrize("K,f,P", [(11, 2, 4099), (40, 8, 4099), (128, 25, 20011)])
def test_defense_end_to_end(cuda, K, f, P):
    X, dist = _selection_case(K, f, P)
    theta, beta = sizes(K, f)
    d = get_defense("bulyan", {"num_malicious": f})
    out = d.aggregate(ClientMatrix(X, P, [torch.Size([P])]), [1] * K)
    want_sel, first = iter_krum(dist, f, theta)
    assert np.array_equal(d.distances.cpu().numpy(), dist)  # pairwise_method="reference": the oracle's D
    assert d.selected_clients == want_sel
    assert d.rejected_clients == sorted(set(range(K)) - set(want_sel))
    assert d.client_scores == [float(s) for s in first]
    want = window_mean(X[:, :P].cpu().numpy()[want_sel], beta)
    assert len(out) == 1 and torch.equal(out[0].cpu(), torch.from_numpy(want))
    m = d.get_metrics()
    assert (m["defense_type"], m["theta"], m["beta"]) == ("bulyan", theta, beta)


def test_defense_list_of_lists_input(cuda):
    K, f, P = 11, 2, 4099
    X, dist = _selection_case(K, f, P)
    shapes = [(4000,), (9, 11)]
    ups = [[t.cpu() for t in u] for u in split_rows(X, P, shapes)]
    d = get_defense("bulyan", {"num_malicious": f})
    out = d.aggregate(ups, [1] * K)
    assert [tuple(t.shape) for t in out] == shapes and all(t.device.type == "cpu" for t in out)
    theta, beta = sizes(K, f)
    want = window_mean(X[:, :P].cpu().numpy()[iter_krum(dist, f, theta)[0]], beta)
    assert np.array_equal(torch.cat([t.reshape(-1) for t in out]).numpy(), want)


def test_sharded_world1_equals_flat(cuda):
    """World 1: the sharded entry point on the whole matrix == aggregate_flat."""
    K, f, P = 16, 3, 5000
    X = update_matrix(K, P, f=f, seed=5, device=cuda)
    cm = ClientMatrix(X, P, [torch.Size([P])])
    cfg = {"num_malicious": f, "pairwise_method": "gram"}
    d1 = get_defense("bulyan", dict(cfg))
    ref = d1.aggregate_flat(cm, [1] * K)
    d2 = get_defense("bulyan", dict(cfg))
    cs = CoordSlice(X, CoordPlan(P, 1), 0, Comm())
    out = torch.empty(P, device=cuda)
    cs.gather_vector(d2.aggregate_sharded(cs, [1] * K), out)
    assert torch.equal(out, ref[:P])
    assert d1.selected_clients == d2.selected_clients and len(d1.selected_clients) == K - 2 * f


def test_round_engine_training_order_equals_torch_order(cuda, monkeypatch):
    """One round of the full model through the engine: Bulyan keeps the
    training-order client matrix (no dead-tap deferral: it reads the selected
    rows whole) and, being coordinate-wise on order-exact distances, gives the
    torch-order round's global model bit for bit."""
    from flr.models.multimodal import ModelSpec
    from flr.round import RoundConfig, RoundEngine
    from flr.train import TrainConfig
    rc = RoundConfig(num_clients=8, batch=4, defense="bulyan", attack="sign_flip", num_attackers=1)
    outs, sels = [], []
    for order in ("train", "torch"):
        monkeypatch.setenv("FLR_ORDER", order)
        eng = RoundEngine(ModelSpec(), rc, TrainConfig(local_steps=1), cuda)
        if order == "train":
            assert eng.train_order and not eng.dead_deferred
        else:
            assert not eng.train_order
        g = eng.run_round()
        assert not eng.fell_back
        eng.defense.publish()
        outs.append(g.clone().cpu())
        sels.append(list(eng.defense.selected_clients))
    assert torch.isfinite(outs[0]).all()
    assert sels[0] == sels[1] and len(sels[0]) == 6
    assert torch.equal(outs[0], outs[1])


# ---------------- 2 ranks on one GPU (gloo) vs 1 rank ----------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _round_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from flr.models.multimodal import TINY
    from flr.round import RoundConfig, RoundEngine
    from flr.train import TrainConfig
    rc = RoundConfig(num_clients=8, batch=4, defense="bulyan", num_attackers=1, exchange="alltoall")
    eng = RoundEngine(TINY, rc, TrainConfig(local_steps=2), torch.device("cuda:0"), rank, world)
    for _ in range(2):
        g = eng.run_round()
    torch.cuda.synchronize()
    eng.defense.publish()
    q.put((rank, g.cpu().numpy(), list(eng.defense.selected_clients), eng.fell_back))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _run(world):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")  # fresh child processes
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_round_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def test_sharded_round_two_ranks_equals_one(cuda):
    """The all-to-all exchange: sharded distances, the selection replicated,
    the window mean on each rank's coordinate slice."""
    one = _run(1)
    two = _run(2)
    assert not one[0][3] and not two[0][3] and not two[1][3]
    assert np.array_equal(one[0][1], two[0][1]) and np.array_equal(two[0][1], two[1][1])
    assert one[0][2] == two[0][2] == two[1][2] and len(one[0][2]) == 6
