"""GPU: centered clipping (flr_centered_clip, ops.centered_clip,
CenteredClippingDefense, the round engine's defense="centered_clipping")
against the CPU restatement of tests/centered_clip_ref.py.  out, the scales and
the thresholds bit for bit (torch.equal); the fp64 distances at relative 1e-12,
which covers the summation order only (64-block fp64 sums of at most 5000 terms
differ by far less).  Bit equality of the scales rests on no distance sitting on
a float32 rounding boundary: every test asserts the reference's margin first, so
such a seed fails loudly there and not as a kernel bug (the seeds below were
checked on the CPU; the kernel's own distances never enter the reference)."""
import functools
import math

import numpy as np
import pytest
import torch

from centered_clip_ref import centered_clip
from flr import _capi, ops
from flr.defenses import get_defense
from flr.matrix import ClientMatrix
from flr.models.multimodal import TINY
from flr.round import RoundConfig, RoundEngine
from flr.train import TrainConfig

pytestmark = pytest.mark.gpu

# (K, P, ldx - P): one client; one column; ldx % 4 != 0, the one-coordinate form;
# the float4 form over several workgroups; the float4 form with a 3-coordinate
# tail and K no multiple of 16; many rows
SHAPES = [(1, 5, 3), (2, 1, 3), (5, 7, 2), (16, 5000, 24), (33, 1027, 1), (130, 300, 0)]
# per shape, a seed at which every reference margin a test asserts (fixed tau and,
# where used, median mode, bad rows, 1 and 2 iterations) clears MARGIN with room:
# above 1e-9, and 3.8e-10 over the 390 distances of the 130-row shape (found on
# the CPU; the kernel's summation-order difference is ~1e-15)
SEEDS = {(1, 5, 3): 0, (2, 1, 3): 0, (5, 7, 2): 0, (16, 5000, 24): 15, (33, 1027, 1): 140, (130, 300, 0): 31}
ITERS = 3
MARGIN = 1e-10
FILL = -77.0  # the padding columns' content


def _tau(P):
    return 0.05 * math.sqrt(P) * 1.5


@functools.lru_cache(maxsize=None)
def _inputs(K, P, pad):
    """The padded CPU matrix [K, P + pad] and v0: benign rows v0 + 0.05 randn,
    about a fifth of the rows v0 + 5 randn (clipped), the last row exactly v0
    (distance 0, scale 1) when there is more than one."""
    torch.manual_seed(SEEDS[(K, P, pad)])
    v0 = torch.randn(P)
    data = torch.full((K, P + pad), FILL)
    data[:, :P] = v0 + 0.05 * torch.randn(K, P)
    nfar = K // 5 if K >= 5 else (1 if K >= 2 else 0)
    data[:nfar, :P] = v0 + 5.0 * torch.randn(nfar, P)
    if K >= 2:
        data[K - 1, :P] = v0
    return data, v0


@functools.lru_cache(maxsize=None)
def _ref(K, P, pad, tau, iters, bad=False):
    """The reference's (out, norms, scales, taus, margin), computed once."""
    data, v0 = _inputs(K, P, pad)
    return centered_clip(_with_bad_rows(data, P) if bad else data[:, :P].contiguous(), v0, tau, iters)


def _with_bad_rows(data, P):
    X = data[:, :P].clone()
    X[5, P // 3] = float("nan")
    X[9, P // 2] = float("inf")
    return X


def _check_norms(got, want):
    got = got.cpu().numpy()
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    err = np.abs(got[fin] - want[fin])
    print("norms: max relative error", float((err / np.maximum(want[fin], 1e-300)).max()) if err.size else 0.0)
    assert (err <= 1e-12 * want[fin]).all()


def _run_and_compare(cuda, data, P, X_cpu, v0, tau, iters, ref):
    """X_cpu's rows inside data's padded layout -> the kernel; everything
    against ref, the padding columns and X itself untouched."""
    want, norms, scales, taus, margin = ref
    print("reference margin", margin)
    assert margin > MARGIN
    D = data.clone()
    D[:, :P] = X_cpu
    Dg = D.to(cuda)
    out = torch.full((P,), 5.0, device=cuda)
    got = ops.centered_clip(Dg[:, :P], v0.to(cuda), tau, iters, out=out, diagnostics=True)
    assert got[0] is out
    assert torch.equal(got[2].cpu(), scales)
    assert torch.equal(got[3].cpu(), taus)
    assert torch.equal(out.cpu(), want)
    _check_norms(got[1], norms)
    Dc = Dg.cpu()
    assert torch.equal(Dc[:, P:], D[:, P:])                       # the padding columns
    assert torch.equal(Dc[:, :P].isnan(), D[:, :P].isnan())
    assert torch.equal(Dc[:, :P].nan_to_num(), D[:, :P].nan_to_num())  # X is only read
    return got


@pytest.mark.parametrize("K,P,pad", SHAPES)
def test_kernel_bitwise(cuda, K, P, pad):
    data, v0 = _inputs(K, P, pad)
    tau = _tau(P)
    ref = _ref(K, P, pad, tau, ITERS)
    scales = ref[2]
    if K >= 5:   # both branches occur, in every iteration
        assert ((scales < 1).any(dim=1) & (scales == 1).any(dim=1)).all()
    if K >= 2:
        assert ref[1][0, K - 1] == 0 and scales[0, K - 1] == 1
    got = _run_and_compare(cuda, data, P, data[:, :P], v0, tau, ITERS, ref)
    # without the optional outputs: the same vector
    plain = ops.centered_clip(data.to(cuda)[:, :P], v0.to(cuda), tau, ITERS)
    assert torch.equal(plain, got[0])


@pytest.mark.parametrize("K,P,pad", [(16, 5000, 24), (33, 1027, 1)])
def test_median_mode(cuda, K, P, pad):
    data, v0 = _inputs(K, P, pad)
    ref = _ref(K, P, pad, 0.0, ITERS)
    norms, scales, taus = ref[1], ref[2], ref[3]
    for l in range(ITERS):
        assert taus[l].item() == np.sort(norms[l].astype(np.float32))[(K - 1) // 2]
        assert 1 <= int((scales[l] < 1).sum()) <= K - (K - 1) // 2 - 1
    _run_and_compare(cuda, data, P, data[:, :P], v0, 0.0, ITERS, ref)


@pytest.mark.parametrize("mode", ["fixed", "median"])
def test_bad_rows_are_skipped(cuda, mode):
    """One row with a single NaN, one with a single +inf: scale 0 in every
    iteration, never multiplied — out is finite and the reference's bits."""
    K, P, pad = 16, 5000, 24
    data, v0 = _inputs(K, P, pad)
    tau = _tau(P) if mode == "fixed" else 0.0
    ref = _ref(K, P, pad, tau, ITERS, bad=True)
    assert np.isnan(ref[1][:, 5]).all() and np.isinf(ref[1][:, 9]).all() and torch.isfinite(ref[0]).all()
    got = _run_and_compare(cuda, data, P, _with_bad_rows(data, P), v0, tau, ITERS, ref)
    assert not got[2][:, [5, 9]].any()
    assert (got[2][:, [0, 1, 2, 3, 4, 6, 7, 8, 10, 11, 12, 13, 14, 15]] > 0).all()
    assert torch.isfinite(got[0]).all()


def test_iterations(cuda):
    """1 and 2 iterations (the last iterate lands in out at either parity)
    against the reference; the first iteration's diagnostics do not depend on
    how many follow."""
    K, P, pad = 33, 1027, 1
    data, v0 = _inputs(K, P, pad)
    tau = _tau(P)
    got1 = _run_and_compare(cuda, data, P, data[:, :P], v0, tau, 1, _ref(K, P, pad, tau, 1))
    _run_and_compare(cuda, data, P, data[:, :P], v0, tau, 2, _ref(K, P, pad, tau, 2))
    got3 = ops.centered_clip(data.to(cuda)[:, :P], v0.to(cuda), tau, 3, diagnostics=True)
    for a, b in zip(got1[1:], got3[1:]):
        assert a.shape[0] == 1 and b.shape[0] == 3 and torch.equal(a[0], b[0])
    assert not torch.equal(got1[0], got3[0])


def test_argument_errors_leave_out_alone(cuda):
    K, P, ld = 6, 40, 48
    torch.manual_seed(3)
    D = torch.randn(K, ld).to(cuda)
    v = torch.randn(P).to(cuda)
    out = torch.full((P,), FILL, device=cuda)
    diag = torch.full((3 * K,), FILL, dtype=torch.float64, device=cuda)
    lib = _capi.lib()
    fn = lib.flr_centered_clip
    need = lib.flr_centered_clip_workspace(K, P)
    ws_t, ws = ops._ws(max(need, lib.flr_centered_clip_workspace(4097, P)), cuda)
    x, v0, o = D.data_ptr(), v.data_ptr(), out.data_ptr()
    nan = float("nan")
    A, W, U = _capi.FLR_ERR_ARG, _capi.FLR_ERR_WORKSPACE, _capi.FLR_ERR_UNSUPPORTED
    bad = [((None, K, P, ld, v0, 1.0, 3, o, ws, need), A),     # null X
           ((x, K, P, ld, None, 1.0, 3, o, ws, need), A),      # null v0
           ((x, K, P, ld, v0, 1.0, 3, None, ws, need), A),     # null out
           ((x, 0, P, ld, v0, 1.0, 3, o, ws, need), A),        # K < 1
           ((x, -2, P, ld, v0, 1.0, 3, o, ws, need), A),
           ((x, K, 0, ld, v0, 1.0, 3, o, ws, need), A),        # P < 1
           ((x, K, -3, ld, v0, 1.0, 3, o, ws, need), A),
           ((x, K, P, P - 1, v0, 1.0, 3, o, ws, need), A),     # ldx < P
           ((x, K, P, ld, v0, 1.0, 0, o, ws, need), A),        # iters < 1
           ((x, K, P, ld, v0, 1.0, -1, o, ws, need), A),
           ((x, K, P, ld, v0, -0.5, 3, o, ws, need), A),       # tau < 0
           ((x, K, P, ld, v0, nan, 3, o, ws, need), A),        # tau NaN
           ((x, K, P, ld, o, 1.0, 3, o, ws, need), A),         # out == v0
           ((x, K, P, ld, v0, 1.0, 3, o, None, need), W),      # no workspace
           ((x, K, P, ld, v0, 1.0, 3, o, ws, need - 1), W),    # too small
           ((x, K, P, ld, v0, 1.0, 3, o, ws, 0), W),
           ((x, K, P, ld, v0, 1.0, 3, o, ws + 128, need + 256), W),  # not 256-B aligned
           ((x, 4097, P, ld, v0, 1.0, 3, o, ws, ws_t.numel() - 256), U)]  # K > 4096
    for (X, k, p, l, c, tau, iters, dst, w, wb), code in bad:
        assert fn(X, k, p, l, c, tau, iters, dst, diag.data_ptr(), None, None, w, wb, None) == code, (k, p, l, tau, iters)
    torch.cuda.synchronize()
    assert (out.cpu() == FILL).all() and (diag.cpu() == FILL).all()
    with pytest.raises(_capi.FlrError) as e:   # aliasing through the tensor wrapper
        ops.centered_clip(D[:, :P], v, 1.0, 3, out=v)
    assert e.value.status == A
    for kw in (dict(tau=-1.0, iters=3), dict(tau=nan, iters=3), dict(tau=1.0, iters=0)):
        with pytest.raises(ValueError):
            ops.centered_clip(D[:, :P], v, **kw)
    with pytest.raises(ValueError):
        ops.centered_clip(D[:, :P], v[:-1].contiguous(), 1.0, 3)
    with pytest.raises(ValueError):
        ops.centered_clip(D[:, :P], v.double(), 1.0, 3)
    with pytest.raises(ValueError):
        ops.centered_clip(D[:, :P], v, 1.0, 3, out=torch.empty(P))   # a CPU tensor
    assert (out.cpu() == FILL).all()


API_SEED = 1   # the five reference calls' margins: 1.4e-9 at the least


def test_defense_api(cuda):
    """aggregate on a list of parameter lists and on a ClientMatrix; the center:
    global_params, then set_center (for one call), then the previous result,
    then the lower median."""
    torch.manual_seed(API_SEED)
    K, shapes, tau, iters = 6, [(3, 4), (5,)], 0.3, 2
    P = 17
    base = torch.randn(P)
    X = base + 0.05 * torch.randn(K, P)
    X[0] = base + 3.0 * torch.randn(P)
    ups = [[X[k, :12].reshape(3, 4).clone(), X[k, 12:].clone()] for k in range(K)]
    margins = []

    def ref(center):
        out, norms, scales, taus, margin = centered_clip(X, center, tau, iters)
        margins.append(margin)
        return out, norms, scales, taus

    def flat(params):
        assert [tuple(p.shape) for p in params] == shapes
        return torch.cat([p.reshape(-1) for p in params]).cpu()

    d = get_defense("centered_clipping", {"tau": tau, "iters": iters})
    # first call: nothing to start from but the rows' lower median
    r1 = ref(torch.median(X, dim=0).values)
    got1 = d.aggregate(ups, [10] * K)
    assert got1[0].device.type == "cpu" and torch.equal(flat(got1), r1[0])
    m = d.get_metrics()
    assert m["taus"] == r1[3].tolist() == [np.float32(tau).item()] * iters
    assert m["clipped_counts"] == (r1[2] < 1).sum(dim=1).tolist() and m["clipped_counts"][0] >= 1
    assert np.allclose(m["final_norms"], r1[1][-1], rtol=1e-12, atol=0)
    assert d.detect_malicious(ups, [10] * K) == torch.nonzero(r1[2][-1] < 1).reshape(-1).tolist()
    assert 0 in d.detect_malicious()
    got1[0].zero_()   # the caller's copy is its own: the next call still starts from the result
    # second call: from the first call's output (a ClientMatrix in, device tensors out)
    r2 = ref(r1[0])
    cm = ClientMatrix.from_updates(ups, device=cuda)
    got2 = d.aggregate(cm, [])
    assert got2[0].is_cuda and torch.equal(flat(got2), r2[0]) and not torch.equal(r2[0], r1[0])
    # set_center wins over the previous result, for one call
    c = base + 0.01 * torch.randn(P)
    r3 = ref(c)
    d.set_center([c[:12].reshape(3, 4), c[12:]])
    assert torch.equal(flat(d.aggregate(ups, [])), r3[0])
    r4 = ref(r3[0])
    assert torch.equal(flat(d.aggregate(ups, [])), r4[0])
    # global_params wins over set_center; aggregate_flat's global_flat is the same path
    g = base - 0.02 * torch.randn(P)
    r5 = ref(g)
    d.set_center(c)
    assert torch.equal(flat(d.aggregate(ups, [], global_params=[g[:12].reshape(3, 4), g[12:]])), r5[0])
    d.set_center(c)
    assert torch.equal(d.aggregate_flat(cm, [], global_flat=g.to(cuda)).cpu(), r5[0])
    with pytest.raises(ValueError):
        d.aggregate_flat(cm, [], global_flat=g[:-1].to(cuda))
    print("reference margins", margins)
    assert min(margins) > MARGIN


ENGINE_SEED = 42


def test_engine_round(cuda, monkeypatch):
    """TINY, K = 8, f = 2, ALIE, torch order.  The engine takes the all-gather
    exchange and hands the defense the round's global model: round 1 is the
    reference applied to the exchanged (attacked) matrix from the initial global
    vector, round 2 (a replay of the captured training graph) from round 1's."""
    monkeypatch.setenv("FLR_ORDER", "torch")
    kw = dict(num_clients=8, batch=4, defense="centered_clipping", defense_cfg={"tau": "median"}, attack="alie",
              num_attackers=2, seed=ENGINE_SEED)
    eng = RoundEngine(TINY, RoundConfig(**kw), TrainConfig(local_steps=2), cuda)
    assert eng.exchange == "allgather" and eng.use_graph and not eng.train_order and not eng.dead_deferred
    g0 = eng.global_flat.clone().cpu()
    g1 = eng.run_round().clone().cpu()
    X1 = eng.full.X.cpu().contiguous()
    want1, _, scales1, taus1, margin1 = centered_clip(X1, g0, 0.0, 3)
    print("reference margin, round 1", margin1)
    assert margin1 > MARGIN
    assert torch.isfinite(X1).all() and torch.equal(X1[0], X1[1])     # the colluders' common row
    assert torch.equal(g1, want1) and not torch.equal(g1, g0)
    m = eng.defense.get_metrics()
    assert m["taus"] == taus1.tolist() and m["clipped_counts"] == (scales1 < 1).sum(dim=1).tolist()
    g2 = eng.run_round().clone().cpu()
    X2 = eng.full.X.cpu().contiguous()
    want2, _, _, _, margin2 = centered_clip(X2, g1, 0.0, 3)
    print("reference margin, round 2", margin2)
    assert margin2 > MARGIN
    assert not torch.equal(X2[2:], X1[2:])
    assert torch.equal(g2, want2)
    assert eng.round_index == 2 and not eng.fell_back
    with pytest.raises(ValueError, match="whole client rows"):
        RoundEngine(TINY, RoundConfig(exchange="alltoall", **kw), TrainConfig(local_steps=2), cuda)
