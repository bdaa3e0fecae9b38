"""GPU: the Min-Max / Min-Sum attacks (flr_minmax_rows, flr.attacks.min_max_ /
min_sum_, the round engine's attack="min_max" / "min_sum") against
tests/minmax_ref.py.  Bit for bit (torch.equal / ==) wherever include/flr.h
defines the bits: mu and sigma, R2 and S from the Gram distances, gamma from the
kernel's own statistics, the rows from the kernel's gamma.  The statistics
a_i, b_i, c are fixed-order fp64 sums in the kernel's own order and have a
tolerance (stat_tol)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import minmax_ref as ref
from minmax_ref import MAX, SIGN, STD, SUM, UNIT
from flr import _capi, ops
from flr.attacks import min_max_, min_sum_
from flr.matrix import ClientMatrix
from flr.models.multimodal import TINY
from flr.round import RoundConfig, RoundEngine
from flr.train import TrainConfig

pytestmark = pytest.mark.gpu

# (K, nmal, P, ldx - P): nb = 1; one column; several workgroups (two column
# blocks) and padding; P no multiple of 4 (the float4 lanes' scalar tail) and a
# partial row group; nb = 128, the last size of the mean kernel's register
# form, eight full row groups.  Every ldx of those is a multiple of 4, the
# float4 form; (21, 2, 130, 1) has ldx = 131, the one-lane-per-coordinate form.
# nb = 129: the mean kernel's streaming form with no row written, the Gram
# engine past 128 rows.  nb = 288: that again with a streaming tail, 18 row
# groups, and a second trip of the solve kernel's 256-thread loops
SHAPES = [(3, 2, 5, 3), (7, 2, 1, 3), (16, 3, 5000, 24), (33, 8, 257, 3), (140, 12, 777, 3), (21, 2, 130, 1),
          (141, 12, 777, 3), (300, 12, 260, 4)]
OBJECTIVES = [(MAX, "max"), (SUM, "sum")]
PERTURBS = [(STD, "std"), (SIGN, "sign"), (UNIT, "unit")]
FILL = -77.0  # the padding columns' content


def stat_tol(P):
    """The statistics' tolerance, relative to their scale (a_i and c: themselves,
    sums of non-negative terms; b_i: sqrt(a_i * c), which bounds the sum of its
    terms' magnitudes).  Kernel and reference form the same fp32 d and the same
    exact fp64 products, so only the summation differs: a fixed-order fp64 sum
    of P terms is within P * 2^-53 of the exact sum, relative to the terms'
    magnitudes, the reference's fsum within 2^-53.  Margin 4 over that bound,
    chosen before any run.  Measured on the MI355X over the test_kernel cases below
    (DESIGN.md): a_i at most 3.5e-16, b_i 2.3e-17, c 1.8e-16 — under two units
    in the last place of the fp64 result, 0.003 of the tolerance at P = 260."""
    return 4.0 * P * 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _case(K, nmal, P, pad):
    """The padded CPU matrix [K, P + pad], the global model g, and the benign
    rows' mu and sigma (colluding_ref), made once."""
    torch.manual_seed(1000 * K + P)
    base = torch.randn(P)
    data = torch.full((K, P + pad), FILL)
    data[:, :P] = base + 0.05 * torch.randn(K, P)
    g = base + 0.1 * torch.randn(P)
    mu, sigma = ref.mean_std(data[:, :P].contiguous(), nmal)
    return data, g, mu, sigma


@functools.lru_cache(maxsize=None)
def _accurate(K, nmal, P, pad, perturb):
    data, g, mu, sigma = _case(K, nmal, P, pad)
    p = ref.perturbation(mu, sigma, g, perturb)
    return p, ref.statistics(data[:, :P].contiguous(), nmal, mu, p)


def _split(stats, nb):
    s = stats.cpu().numpy()
    return s[:nb], s[nb:2 * nb], float(s[2 * nb]), float(s[2 * nb + 1]), float(s[2 * nb + 2]), float(s[2 * nb + 3])


@pytest.mark.parametrize("perturb,pname", PERTURBS, ids=[n for _, n in PERTURBS])
@pytest.mark.parametrize("objective,oname", OBJECTIVES, ids=[n for _, n in OBJECTIVES])
@pytest.mark.parametrize("K,nmal,P,pad", SHAPES)
def test_kernel(cuda, K, nmal, P, pad, objective, oname, perturb, pname):
    data, g, mu, sigma = _case(K, nmal, P, pad)
    p, (a64, b64, c64) = _accurate(K, nmal, P, pad, perturb)
    nb = K - nmal
    D = data.to(cuda)
    gd = g.to(cuda)
    gamma_t, stats, mu_d, sigma_d = ops.minmax_rows(D[:, :P], nmal, objective, perturb,
                                                    None if perturb == STD else gd, diagnostics=True)
    got = D.cpu()
    # mu, sigma: flr_collude_rows' bits
    assert torch.equal(mu_d.cpu(), mu) and torch.equal(sigma_d.cpu(), sigma)
    # the statistics against the accurate values
    a, b, c, R2, S, bound = _split(stats, nb)
    tol = stat_tol(P)
    ea = float(np.max(np.abs(a - a64) / np.where(a64 > 0, a64, 1.0)))
    eb = float(np.max(np.abs(b - b64) / np.where(a64 * c64 > 0, np.sqrt(a64 * c64), 1.0)))
    ec = abs(c - c64) / (c64 if c64 > 0 else 1.0)
    print(f"STATERR K={K} nmal={nmal} P={P} {oname} {pname}: a {ea:.3e} b {eb:.3e} c {ec:.3e} tol {tol:.3e}")
    assert ea <= tol and eb <= tol and ec <= tol
    assert (a[a64 == 0] == 0).all() and (b[a64 * c64 == 0] == 0).all() and (c64 > 0 or c == 0)
    # R2, S: the reference's rule on the Gram distances of the benign rows
    Dg = ops.pairwise_l2(D[nmal:, :P]).cpu().numpy()
    assert (R2, S) == ref.bounds(Dg)
    assert bound == (R2 if objective == MAX else S)
    # gamma from the kernel's own statistics, the rows from the kernel's gamma
    gamma = gamma_t.item()
    assert gamma == ref.gamma_closed(a, b, c, R2, S, objective)
    assert gamma >= 0.0 and (nb > 1 or gamma == 0.0)
    want = ref.rows(data[:, :P].contiguous(), nmal, mu, p, gamma)
    assert torch.equal(got[:nmal, :P], want[:nmal])          # the attackers' rows
    assert nb == 1 or not torch.equal(got[:nmal, :P], data[:nmal, :P])
    assert torch.equal(got[nmal:, :P], data[nmal:, :P])      # the benign rows
    assert torch.equal(got[:, P:], data[:, P:])              # the padding columns
    # a second call on the same input, without the optional outputs: identical bits
    D2 = data.to(cuda)
    gamma2 = ops.minmax_rows(D2[:, :P], nmal, objective, perturb, None if perturb == STD else gd)
    assert gamma2.item() == gamma and torch.equal(D2.cpu(), got)


def test_statistics_are_deterministic(cuda):
    """Two calls on the same input: the same statistics, bit for bit (fixed
    order of the partial sums)."""
    K, nmal, P, pad = 140, 12, 777, 3
    data, g, _, _ = _case(K, nmal, P, pad)
    gd = g.to(cuda)
    runs = []
    for _ in range(2):
        D = data.to(cuda)
        _, stats, _, _ = ops.minmax_rows(D[:, :P], nmal, MAX, SIGN, gd, diagnostics=True)
        runs.append(stats.cpu())
    assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64))


@pytest.mark.parametrize("K,nmal,P,pad", [(16, 3, 5000, 24), (140, 12, 777, 3), (141, 12, 777, 3), (300, 12, 260, 4)])
def test_nan_leaves_the_attackers_rows(cuda, K, nmal, P, pad):
    """A NaN in one benign entry: gamma comes back NaN, the attackers' rows are
    unchanged and nothing else is touched."""
    data, g, _, _ = _case(K, nmal, P, pad)
    bad = data.clone()
    bad[nmal + 2, P // 3] = float("nan")
    gd = g.to(cuda)
    for objective, perturb in ((MAX, STD), (SUM, SIGN), (MAX, UNIT)):
        D = bad.to(cuda)
        gamma = ops.minmax_rows(D[:, :P], nmal, objective, perturb, gd)
        assert math.isnan(gamma.item())
        got = D.cpu()
        assert torch.equal(got.view(torch.int32), bad.view(torch.int32))


@pytest.mark.parametrize("which", ["global", "matrix"])
def test_misaligned_operands_take_the_scalar_form(cuda, which):
    """ldx a multiple of 4, but the global model (a view one float into its
    buffer) or the matrix (a view from column 1 on) not 16-B aligned: the call
    takes the one-lane-per-coordinate form and meets the same checks."""
    K, nmal, P, pad = 16, 3, 5000, 24
    data, g, mu, sigma = _case(K, nmal, P, pad)
    nb = K - nmal
    X = data[:, :P].contiguous()
    gbuf = torch.zeros(P + 1, device=cuda)
    if which == "global":
        D = data.to(cuda)
        V = D[:, :P]
        gbuf[1:].copy_(g)
        gd = gbuf[1:]
    else:
        D = torch.full((K, P + pad + 4), FILL, device=cuda)
        V = D[:, 1:P + 1]
        V.copy_(X)
        gbuf[:P].copy_(g)
        gd = gbuf[:P]
    assert (V.data_ptr() % 16 != 0) == (which == "matrix") and (gd.data_ptr() % 16 != 0) == (which == "global")
    assert V.stride(0) % 4 == 0
    before = D.cpu()
    for objective, perturb in ((MAX, SIGN), (SUM, UNIT)):
        p, (a64, b64, c64) = _accurate(K, nmal, P, pad, perturb)
        D.copy_(before)
        gamma_t, stats, mu_d, sigma_d = ops.minmax_rows(V, nmal, objective, perturb, gd, diagnostics=True)
        assert torch.equal(mu_d.cpu(), mu) and torch.equal(sigma_d.cpu(), sigma)
        a, b, c, R2, S, _ = _split(stats, nb)
        tol = stat_tol(P)
        assert np.max(np.abs(a - a64) / a64) <= tol and np.max(np.abs(b - b64) / np.sqrt(a64 * c64)) <= tol
        assert abs(c - c64) / c64 <= tol
        gamma = gamma_t.item()
        assert gamma > 0.0 and gamma == ref.gamma_closed(a, b, c, R2, S, objective)
        got = V.cpu()
        assert torch.equal(got, ref.rows(X, nmal, mu, p, gamma))
        after = D.cpu()
        if which == "global":
            assert torch.equal(after[:, P:], before[:, P:])
        else:
            assert torch.equal(after[:, :1], before[:, :1]) and torch.equal(after[:, P + 1:], before[:, P + 1:])


def test_more_than_1024_benign_rows_is_unsupported(cuda):
    """nb = 1025: FLR_ERR_UNSUPPORTED (flr_pairwise_l2's row limit), X as it was."""
    K, nmal, P = 1027, 2, 8
    torch.manual_seed(5)
    data = torch.randn(K, P)
    D = data.to(cuda)
    with pytest.raises(_capi.FlrError) as e:
        ops.minmax_rows(D, nmal, MAX, STD)
    assert e.value.status == _capi.FLR_ERR_UNSUPPORTED
    assert ops.minmax_rows(D[1:], nmal, MAX, STD).item() > 0.0   # nb = 1024 runs
    assert torch.equal(D.cpu()[:1], data[:1]) and torch.equal(D.cpu()[3:], data[3:])


def test_errors_leave_x_alone(cuda):
    """Every FLR_ERR_ARG and FLR_ERR_WORKSPACE case through ctypes.CDLL: the
    status, and X (and the outputs) as they were."""
    K, P, ld, nmal = 6, 40, 48, 2
    torch.manual_seed(3)
    data = torch.randn(K, ld)
    D = data.to(cuda)
    g = torch.randn(P, device=cuda)
    handle = ctypes.CDLL(_capi.LIB_PATH)
    wsq, fn = handle.flr_minmax_workspace, handle.flr_minmax_rows
    wsq.restype, wsq.argtypes = ctypes.c_size_t, [ctypes.c_int64] * 3
    fn.restype = ctypes.c_int
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    fn.argtypes = [vp, i64, i64, i64, i64, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, ctypes.c_size_t, vp]
    nbytes = wsq(K, P, nmal)
    assert nbytes > 0 and nbytes >= 2 * 4 * P + 8 * (K - nmal) ** 2
    for k, p, n in ((1, P, 1), (K, 0, nmal), (K, P, 0), (K, P, K), (K, P, K + 1), (K, -1, nmal)):
        assert wsq(k, p, n) == 0
    ws = torch.zeros(nbytes + 512, dtype=torch.uint8, device=cuda)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    out = torch.full((2 * (K - nmal) + 5,), 7.0, dtype=torch.float64, device=cuda)
    gam, sts = out.data_ptr(), out.data_ptr() + 8
    x, gp = D.data_ptr(), g.data_ptr()
    bad = [(None, K, P, ld, nmal, MAX, STD, gp),     # null X
           (x, 1, P, ld, 1, MAX, STD, gp),           # K < 2
           (x, K, P, ld, 0, MAX, STD, gp),           # nmal < 1
           (x, K, P, ld, -1, SUM, STD, gp),
           (x, K, P, ld, K, MAX, STD, gp),           # nmal >= K
           (x, K, P, ld, K + 1, SUM, SIGN, gp),
           (x, K, 0, ld, nmal, MAX, STD, gp),        # P < 1
           (x, K, -3, ld, nmal, MAX, UNIT, gp),
           (x, K, P, P - 1, nmal, MAX, STD, gp),     # ldx < P
           (x, K, P, ld, nmal, 2, STD, gp),          # objective out of range
           (x, K, P, ld, nmal, -1, STD, gp),
           (x, K, P, ld, nmal, MAX, 3, gp),          # perturbation out of range
           (x, K, P, ld, nmal, SUM, -1, gp),
           (x, K, P, ld, nmal, MAX, SIGN, None),     # global NULL where it is needed
           (x, K, P, ld, nmal, SUM, UNIT, None)]
    for X, k, p, l, n, obj, per, gl in bad:
        assert fn(X, k, p, l, n, obj, per, gl, gam, sts, wp, nbytes + 256, None) == _capi.FLR_ERR_ARG
    for w, nb_ in ((None, nbytes), (wp, nbytes - 1), (wp, 0), (wp + 128, nbytes + 128)):
        assert fn(x, K, P, ld, nmal, MAX, STD, None, gam, sts, w, nb_, None) == _capi.FLR_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(D.cpu(), data) and (out.cpu() == 7.0).all() and not ws.any().item()
    # the same call with valid arguments runs (global NULL is legal for the std direction)
    assert fn(x, K, P, ld, nmal, MAX, STD, None, gam, sts, wp, nbytes, None) == _capi.FLR_OK
    torch.cuda.synchronize()
    assert out[0].item() > 0.0 and out[-1].item() == out[-3].item() and not torch.equal(D.cpu()[:nmal], data[:nmal])
    with pytest.raises(_capi.FlrError) as e:
        ops.minmax_rows(D[:, :P], nmal, 5, STD)
    assert e.value.status == _capi.FLR_ERR_ARG


def test_attacks_api(cuda):
    """min_max_ / min_sum_ on a tensor and on a ClientMatrix: in place, the
    device gamma back, the std direction by default."""
    K, nmal, P, pad = 16, 3, 5000, 24
    data, g, mu, sigma = _case(K, nmal, P, pad)
    gd = g.to(cuda)
    X = data[:, :P].contiguous()
    for fn, objective in ((min_max_, MAX), (min_sum_, SUM)):
        D = data.to(cuda)
        gamma = fn(D[:, :P], nmal)
        assert gamma.is_cuda and gamma.dtype == torch.float64 and gamma.item() > 0.0
        assert torch.equal(D.cpu()[:, :P], ref.rows(X, nmal, mu, ref.perturbation(mu, sigma, g, STD), gamma.item()))
        cm = ClientMatrix(data.to(cuda), P, [torch.Size([P])])
        gamma_u = fn(cm, nmal, perturb="unit", global_flat=gd)
        assert gamma_u.item() > 0.0 and gamma_u.item() != gamma.item()
        assert torch.equal(cm.X.cpu(), ref.rows(X, nmal, mu, ref.perturbation(mu, sigma, g, UNIT), gamma_u.item()))
        assert torch.equal(cm.data.cpu()[:, P:], data[:, P:])
        for f in (0, -1, K, K + 3):
            with pytest.raises(ValueError):
                fn(D[:, :P], f)


def _engine_restatement(X, f, objective, perturb, g, gamma):
    mu, sigma = ref.mean_std(X, f)
    return ref.rows(X, f, mu, ref.perturbation(mu, sigma, g, perturb), gamma)


@pytest.mark.parametrize("attack", ["min_max", "min_sum"])
@pytest.mark.parametrize("exchange", ["auto", "alltoall"])
def test_engine_round(cuda, monkeypatch, exchange, attack):
    """TINY, K = 8, f = 2, median, torch order, graph replay.  Round 1 against
    an unattacked engine with the same seeds: the benign rows are its rows, the
    attackers' rows the restatement on its matrix with eng.attack_gamma, the
    global model the lower median of that.  Round 2 (a replay of the captured
    training graph, from the attacked global model) against its own benign
    rows.  exchange "auto" is the all-gather exchange under these attacks;
    "alltoall" works at world 1, where the slice is the whole matrix."""
    monkeypatch.setenv("FLR_ORDER", "torch")
    K, f = 8, 2
    objective = MAX if attack == "min_max" else SUM
    kw = dict(num_clients=K, batch=4, defense="median", num_attackers=f)
    eng = RoundEngine(TINY, RoundConfig(attack=attack, exchange=exchange, **kw), TrainConfig(local_steps=2), cuda)
    clean = RoundEngine(TINY, RoundConfig(attack="none", exchange="allgather", **kw), TrainConfig(local_steps=2), cuda)
    assert eng.exchange == ("allgather" if exchange == "auto" else "alltoall")
    assert eng.use_graph and not eng.train_order and not eng.dead_deferred and eng.attack_gamma is None

    def matrix(e):
        return (e.full if e.exchange == "allgather" else e.slice).X.cpu().contiguous()
    g0 = eng.global_flat.clone().cpu()
    g1 = eng.run_round().clone().cpu()
    clean.run_round()
    X, X0 = matrix(eng), matrix(clean)
    gamma = eng.attack_gamma.item()
    assert eng.attack_gamma.is_cuda and gamma > 0.0
    want = _engine_restatement(X0, f, objective, STD, g0, gamma)
    assert torch.isfinite(X0).all()
    assert torch.equal(X[f:], X0[f:])
    assert torch.equal(X[:f], want[:f]) and not torch.equal(X[:f], X0[:f])
    assert torch.equal(g1, torch.median(want, dim=0).values)
    g2 = eng.run_round().clone().cpu()
    X2 = matrix(eng)
    gamma2 = eng.attack_gamma.item()
    want2 = _engine_restatement(X2, f, objective, STD, g1, gamma2)   # reads the benign rows only
    assert not torch.equal(X2[f:], X[f:]) and torch.isfinite(X2).all() and gamma2 > 0.0 and gamma2 != gamma
    assert torch.equal(X2, want2)
    assert torch.equal(g2, torch.median(want2, dim=0).values)
    assert eng.round_index == 2 and not eng.fell_back and not eng.dead_deferred


def test_engine_attack_cfg(cuda, monkeypatch):
    """attack_cfg's direction reaches the kernel, with the round's global model."""
    monkeypatch.setenv("FLR_ORDER", "torch")
    K, f = 8, 2
    kw = dict(num_clients=K, batch=4, defense="median", num_attackers=f)
    gammas = []
    for attack, name, perturb in (("min_max", "sign", SIGN), ("min_sum", "unit", UNIT), ("min_max", "std", STD)):
        eng = RoundEngine(TINY, RoundConfig(attack=attack, attack_cfg={"perturb": name}, **kw),
                          TrainConfig(local_steps=1), cuda)
        g0 = eng.global_flat.clone().cpu()
        eng.run_round()
        X = eng.full.X.cpu().contiguous()
        gamma = eng.attack_gamma.item()
        assert gamma > 0.0
        assert torch.equal(X, _engine_restatement(X, f, MAX if attack == "min_max" else SUM, perturb, g0, gamma))
        gammas.append(gamma)
    assert len(set(gammas)) == 3


def test_engine_krum_full_model(cuda):
    """One round of the full ResNet-18 + GRU model under Krum with
    attack="min_max": finite, no fallback, and the dead-tap deferral off (the
    attack reads and writes whole rows, in torch order)."""
    from flr.models.multimodal import ModelSpec
    rc = RoundConfig(num_clients=8, batch=4, defense="krum", attack="min_max", num_attackers=1)
    eng = RoundEngine(ModelSpec(), rc, TrainConfig(local_steps=1), cuda)
    assert not eng.dead_deferred and not eng.train_order
    g = eng.run_round()
    assert torch.isfinite(g).all() and not eng.fell_back and not eng.dead_deferred
    assert eng.attack_gamma.item() > 0.0
