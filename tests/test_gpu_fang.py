"""GPU: Fang et al.'s attacks (flr_fang_krum_strength, flr_fang_krum_rows,
flr_fang_trim_rows, their ops wrappers, flr.attacks.fang_krum_ / fang_trim_, the
round engine's attack="fang_krum" / "fang_trim") against the CPU restatement of
tests/fang_ref.py.

The strength is fp64 with only + - * / sqrt in the header's order, all IEEE
operations on both sides, so lambda64 is compared bit for bit with the reference
evaluated on the device's own G, b and c (read back); info is equal.  The rows
are two (Krum) or three (trimmed mean) fp32 operations: torch.equal.  Every
matrix sits in a padded layout filled with a sentinel; the padding, the benign
rows and the inputs must come back unchanged."""
import functools
import os

import numpy as np
import pytest
import torch

import fang_ref as ref
import replace_ref
from flr import _capi, ops
from flr.attacks import fang_krum_, fang_trim_
from flr.models.multimodal import TINY
from flr.round import RoundConfig, RoundEngine
from flr.train import TrainConfig

pytestmark = pytest.mark.gpu

FILL = -77.0  # the padding columns' content
NAN = float("nan")

# (K, f): the smallest, one wave of benign rows, past a wave, and the nb = 1024 limit
SOLVER_CASES = [(5, 1), (7, 2), (12, 4), (64, 25), (65, 30), (130, 26), (1024 + 100, 100)]
SOLVER_P = 67
# (K, P, ld - P).  One element; below a float4 with a padded row; whole float4s;
# three past a multiple of 4 with ld % 4 == 0 (a ragged float4 tail, two
# workgroups per row); 4-byte loads (ld % 4 != 0); float4 loads over four
# workgroups per row.
ROW_CASES = [(5, 1, 0), (7, 7, 3), (12, 64, 0), (33, 1027, 1), (17, 4099, 3), (64, 4096, 24)]


def _krum_f(K):
    """The largest f with K >= 2f + 3, at most K // 3."""
    return max(1, min((K - 3) // 2, K // 3))


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


def _same32(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_strength(lam, info, stats5, want):
    """lambda64's bits, info and the five statistics (NaN where not computed)."""
    wl, ws, wt, wstats = want
    print("lambda", float(lam), "want", float(wl), "info", info.tolist(), "stats", stats5.tolist())
    assert info.dtype == np.int32 and info.tolist() == [ws, wt]
    if np.isnan(wl):
        assert np.isnan(lam)
    else:
        assert np.array_equal(_bits(lam), _bits(wl))
    assert np.array_equal(np.isnan(stats5), np.isnan(wstats))
    ok = ~np.isnan(wstats)
    assert np.array_equal(_bits(stats5[ok]), _bits(wstats[ok]))


# ---- the solver ----

@pytest.mark.parametrize("K,f", SOLVER_CASES)
def test_fang_krum_solver(cuda, K, f):
    P = SOLVER_P
    X, g = replace_ref.updates(K, f, P, seed=K, amp=0)
    data, dev = _padded(X, 1, cuda)
    gd = g.to(cuda)
    lam, info, stats, G, mu, s = ops.fang_krum_rows(dev[:, :P], f, gd, diagnostics=True)
    nb = K - f
    Gh, sh = G.cpu().numpy(), stats.cpu().numpy()
    b, c = sh[:nb], sh[nb]
    # the statistics: the existing kernels' bits, and close to an fp64 evaluation
    wmu, wsgn = ref.mean_sign(X, g, f)
    assert np.array_equal(mu.cpu().numpy().view(np.int32), wmu.view(np.int32))
    assert np.array_equal(s.cpu().numpy().view(np.int32), wsgn.view(np.int32))
    assert torch.equal(G, ops.rows_gram(dev[f:, :P], center=gd))
    aG, ab, ac = ref.statistics(X, g, f)
    err_b, err_c = float(np.abs(b / ab - 1.0).max()), abs(c / ac - 1.0)
    print("b: max relative error", err_b, "c:", err_c)
    assert err_b <= 1e-12 and err_c <= 1e-12
    # lambda: the reference on the device's own G, b, c
    want = ref.strength(Gh, b, c, K, f)
    _check_strength(lam.cpu().numpy(), info.cpu().numpy(), sh[nb + 1:], want)
    # the call of its own on the same inputs: the same bits
    l64, l32, info2, stats2 = ops.fang_krum_strength(G, stats[:nb].clone(), stats[nb:nb + 1].clone(), K, f)
    _check_strength(l64.cpu().numpy(), info2.cpu().numpy(), stats2.cpu().numpy(), want)
    assert np.array_equal(l32.cpu().numpy().view(np.int32), np.float32(want[0]).view(np.int32))
    # the rows
    got = dev.cpu()
    assert _same32(got[:, :P], ref.krum_rows(X, g, f, np.float32(want[0])))
    assert torch.equal(got[:, P:], data[:, P:]) and torch.equal(got[f:], data[f:]) and torch.equal(gd.cpu(), g)
    assert not torch.equal(got[:f], data[:f])


def test_fang_krum_solver_threshold(cuda):
    """A threshold above lambda0 / 2: the search stops at the first halving with
    status 1; the reference agrees bit for bit."""
    K, f, P = 12, 4, SOLVER_P
    X, g = replace_ref.updates(K, f, P, seed=K, amp=0)
    Xd, gd = X.to(cuda), g.to(cuda)
    _, _, stats, G, _, _ = ops.fang_krum_rows(Xd.clone(), f, gd, diagnostics=True)
    nb = K - f
    sh = stats.cpu().numpy()
    base = ref.strength(G.cpu().numpy(), sh[:nb], sh[nb], K, f)
    assert base[1] == 0 and base[2] >= 1
    th = float(base[3][0]) * 0.75
    want = ref.strength(G.cpu().numpy(), sh[:nb], sh[nb], K, f, th)
    assert want[1] == 1 and want[2] == 1
    l64, _, info, stats5 = ops.fang_krum_strength(G, stats[:nb].clone(), stats[nb:nb + 1].clone(), K, f, th)
    _check_strength(l64.cpu().numpy(), info.cpu().numpy(), stats5.cpu().numpy(), want)
    lam, info = ops.fang_krum_rows(Xd, f, gd, th)
    assert np.array_equal(_bits(lam.cpu().numpy()), _bits(want[0])) and info.tolist() == [1, 1]
    assert _same32(Xd.cpu(), ref.krum_rows(X, g, f, np.float32(want[0])))


def test_fang_krum_degenerate_inputs(cuda):
    """A NaN planted in G: status 3, lambda NaN; through the rows call (a NaN in a
    benign row) no row is written.  g equal to mu: c = 0, status 2, lambda 0, the
    rows equal g.  nb = 1025: FLR_ERR_UNSUPPORTED, nothing written."""
    K, f, P = 12, 4, 67
    nb = K - f
    X, g = replace_ref.updates(K, f, P, seed=1, amp=0)
    data, dev = _padded(X, 1, cuda)
    gd = g.to(cuda)
    _, _, stats, G, _, _ = ops.fang_krum_rows(dev[:, :P].clone(), f, gd, diagnostics=True)
    Gn = G.clone()
    Gn[2, 2] = NAN
    b, c = stats[:nb].clone(), stats[nb:nb + 1].clone()
    l64, l32, info, stats5 = ops.fang_krum_strength(Gn, b, c, K, f)
    want = ref.strength(Gn.cpu().numpy(), b.cpu().numpy(), c.item(), K, f)
    assert want[1] == 3
    _check_strength(l64.cpu().numpy(), info.cpu().numpy(), stats5.cpu().numpy(), want)
    assert torch.isnan(l32).all()

    Z = X.clone()
    Z[f + 2, 5] = NAN
    zdata, zdev = _padded(Z, 1, cuda)
    lam, info = ops.fang_krum_rows(zdev[:, :P], f, gd)
    assert torch.isnan(lam) and info.tolist() == [3, 0]
    got = zdev.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(zdata))
    assert torch.equal(torch.nan_to_num(got, nan=0.5), torch.nan_to_num(zdata, nan=0.5))

    mu = torch.from_numpy(ref.mean_sign(X, g, f)[0]).to(cuda)
    lam, info, stats, _, mud, s = ops.fang_krum_rows(dev[:, :P], f, mu, diagnostics=True)
    assert lam.item() == 0.0 and info.tolist() == [2, 0] and stats[nb].item() == 0.0
    assert torch.equal(mud, mu) and (s == 0).all()
    got = dev.cpu()
    assert _same32(got[:f, :P], mu.cpu().expand(f, P))
    assert torch.equal(got[:, P:], data[:, P:]) and torch.equal(got[f:], data[f:])

    lib = _capi.lib()
    K2, f2 = 1025 + 100, 100
    big = torch.full((K2, 8), 3.0, device=cuda)
    g8 = torch.zeros(8, device=cuda)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=cuda)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    out = torch.full((4,), -5.0, dtype=torch.float64, device=cuda)
    info = torch.full((2,), -5, dtype=torch.int32, device=cuda)

    def rows(x=big.data_ptr(), k=K2, p=8, ld=8, n=f2, gp=g8.data_ptr(), th=1e-5, w=wp, nbytes=ws.numel() - 256):
        return lib.flr_fang_krum_rows(x, k, p, ld, n, gp, th, out.data_ptr(), info.data_ptr(), None, None, w, nbytes,
                                      None)

    assert rows() == _capi.FLR_ERR_UNSUPPORTED
    assert rows(k=1024 + 100) == _capi.FLR_OK
    torch.cuda.synchronize()
    assert info.tolist()[0] in (0, 1, 2) and (big[f2:] == 3.0).all()
    big.fill_(3.0)
    out.fill_(-5.0)
    info.fill_(-5)
    for kw in (dict(x=None), dict(gp=None), dict(n=0), dict(p=0), dict(ld=7), dict(th=0.0), dict(th=NAN),
               dict(th=float("inf")), dict(th=-1.0), dict(k=1), dict(n=K2)):
        assert rows(**kw) == _capi.FLR_ERR_ARG, kw
    assert rows(k=2 * f2 + 2) == _capi.FLR_ERR_KRUM_N
    assert rows(k=1124, w=None) == _capi.FLR_ERR_WORKSPACE and rows(k=1124, w=wp + 16) == _capi.FLR_ERR_WORKSPACE
    assert rows(k=1124, nbytes=1024) == _capi.FLR_ERR_WORKSPACE

    G1 = torch.eye(1025, dtype=torch.float64, device=cuda).contiguous()
    b1 = torch.ones(1025, dtype=torch.float64, device=cuda)
    l32 = torch.full((1,), -5.0, device=cuda)

    def strength(gm=G1.data_ptr(), bp=b1.data_ptr(), cp=b1.data_ptr(), k=K2, n=f2, th=1e-5, o=out.data_ptr(),
                 o32=l32.data_ptr(), i=info.data_ptr(), w=wp):
        return lib.flr_fang_krum_strength(gm, bp, cp, k, n, th, o, o32, i, None, w, ws.numel() - 256, None)

    assert strength() == _capi.FLR_ERR_UNSUPPORTED
    for kw in (dict(gm=None), dict(bp=None), dict(cp=None), dict(o=None), dict(o32=None), dict(i=None), dict(n=0),
               dict(th=0.0), dict(th=NAN)):
        assert strength(**kw) == _capi.FLR_ERR_ARG, kw
    assert strength(k=202) == _capi.FLR_ERR_KRUM_N and strength(k=1124, w=None) == _capi.FLR_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (out == -5.0).all() and (info == -5).all() and (l32 == -5.0).all() and (big == 3.0).all()
    with pytest.raises(ValueError, match="at most 1024"):
        ops.fang_krum_rows(big, f2, g8)


# ---- the rows of fang_krum ----

@pytest.mark.parametrize("K,P,pad", ROW_CASES)
def test_fang_krum_rows(cuda, K, P, pad):
    f = _krum_f(K)
    X, g = replace_ref.updates(K, f, P, seed=K + P, amp=0)
    data, dev = _padded(X, pad, cuda)
    gd = g.to(cuda)
    lam, info = fang_krum_(dev[:, :P], f, gd)
    assert lam.dtype == torch.float64 and lam.dim() == 0 and info.dtype == torch.int32
    lam32 = np.float32(lam.item())
    print("lambda", lam.item(), "info", info.tolist())
    assert lam.item() > 0.0 and info[0].item() in (0, 1)
    got = dev.cpu()
    want = ref.krum_rows(X, g, f, lam32)
    assert _same32(got[:, :P], want) and not torch.equal(got[:f], data[:f])
    assert torch.equal(got[:, P:], data[:, P:]) and torch.equal(got[f:], data[f:]) and torch.equal(gd.cpu(), g)


def test_fang_krum_rows_four_byte_form_gives_the_same_bits(cuda):
    """X 4 bytes off a 16-byte boundary with ld % 4 == 0: the 4-byte loads run
    and give the float4 form's bits, lambda included."""
    K, P, pad = 64, 4096, 24
    f = _krum_f(K)
    X, g = replace_ref.updates(K, f, P, seed=K + P, amp=0)
    gd = g.to(cuda)
    outs, lams = [], []
    for offset in (0, 1):
        data, dev = _padded(X, pad, cuda, offset)
        assert dev.data_ptr() % 16 == 4 * offset
        lam, info = ops.fang_krum_rows(dev[:, :P], f, gd)
        got = dev.cpu()
        assert torch.equal(got[:, P:], data[:, P:]) and torch.equal(got[f:], data[f:])
        outs.append(got[:, :P])
        lams.append(np.float32(lam.item()))
    assert _same32(outs[0], outs[1])
    assert _same32(outs[1], ref.krum_rows(X, g, f, lams[1]))


# ---- fang_trim ----

@pytest.mark.parametrize("f", [1, 3])
@pytest.mark.parametrize("K,P,pad", ROW_CASES)
def test_fang_trim_rows(cuda, K, P, pad, f):
    X, g = replace_ref.updates(K, f, P, seed=K + P + f)
    seed, stream = (9 << 32) | (K * P), 3
    want = ref.trim_rows(X, g, f, 2.0, seed, stream)
    data, dev = _padded(X, pad, cuda)
    gd = g.to(cuda)
    fang_trim_(dev[:, :P], f, gd, b=2.0, seed=seed, stream=stream)
    got = dev.cpu()
    assert _same32(got[:, :P], want) and not torch.equal(got[:f], data[:f])
    assert torch.equal(got[:, P:], data[:, P:]) and torch.equal(got[f:], data[f:]) and torch.equal(gd.cpu(), g)
    # another stream: other draws
    data2, dev2 = _padded(X, pad, cuda)
    ops.fang_trim_rows(dev2[:, :P], f, gd, 2.0, seed, stream + 1)
    got2 = dev2.cpu()
    assert _same32(got2[:, :P], ref.trim_rows(X, g, f, 2.0, seed, stream + 1))
    if P > 1:
        assert not torch.equal(got2[:f], got[:f])


def test_fang_trim_four_byte_form_and_column_ranges(cuda):
    """X 4 bytes off a 16-byte boundary: the float4 form's bits.  Two half-range
    calls with their own col0 (the second range starts off a 16-byte boundary)
    equal the whole call; col0 itself shifts the draws as the reference says."""
    K, P, pad, f = 33, 1027, 1, 3
    X, g = replace_ref.updates(K, f, P, seed=4)
    gd = g.to(cuda)
    seed, stream, base = 77, 5, (1 << 32) - 300   # the counter's high word changes inside the range
    want = ref.trim_rows(X, g, f, 1.5, seed, stream, base)
    for offset in (0, 1):
        data, dev = _padded(X, pad, cuda, offset)
        ops.fang_trim_rows(dev[:, :P], f, gd, 1.5, seed, stream, base)
        got = dev.cpu()
        assert _same32(got[:, :P], want)
        assert torch.equal(got[:, P:], data[:, P:]) and torch.equal(got[f:], data[f:])
    data, dev = _padded(X, pad, cuda)
    h = 513
    ops.fang_trim_rows(dev[:, :h], f, gd[:h].contiguous(), 1.5, seed, stream, base)
    ops.fang_trim_rows(dev[:, h:P], f, gd[h:].contiguous(), 1.5, seed, stream, base + h)
    got = dev.cpu()
    assert _same32(got[:, :P], want) and torch.equal(got[:, P:], data[:, P:]) and torch.equal(got[f:], data[f:])
    assert not _same32(want, ref.trim_rows(X, g, f, 1.5, seed, stream, 0))


def test_fang_trim_special_coordinates(cuda):
    """A NaN planted in one benign coordinate makes exactly that coordinate of
    the attackers' rows NaN; a coordinate with mu == g gets mu."""
    K, P, pad, f = 12, 67, 1, 4
    X, g = replace_ref.updates(K, f, P, seed=6)
    X[f + 3, 10] = NAN
    g[20] = 1.0
    X[f:, 20] = torch.tensor([1.25, 0.75] * 4)   # every partial sum exact: mu == g
    want = ref.trim_rows(X, g, f, 2.0, 1, 0)
    assert torch.isnan(want[:f, 10]).all() and (want[:f, 20] == 1.0).all()
    data, dev = _padded(X, pad, cuda)
    fang_trim_(dev[:, :P], f, g.to(cuda), seed=1)
    got = dev.cpu()
    nan = torch.isnan(got)
    assert nan[:f, 10].all() and nan.sum().item() == f + 1 and nan[f + 3, 10]
    assert (got[:f, 20] == 1.0).all()
    keep = [c for c in range(P) if c != 10]
    assert _same32(got[:, keep], want[:, keep])
    assert torch.equal(got[:, P:], data[:, P:]) and _same32(got[f:, keep], data[f:, keep])

    lib = _capi.lib()
    clean, cdev = _padded(torch.nan_to_num(X, nan=0.0), pad, cuda)
    gd = g.to(cuda)

    def trim(x=cdev.data_ptr(), k=K, p=P, ld=P + pad, n=f, gp=gd.data_ptr(), b=2.0, col0=0):
        return lib.flr_fang_trim_rows(x, k, p, ld, n, gp, b, 1, 0, col0, None)

    for kw in (dict(x=None), dict(gp=None), dict(n=0), dict(n=K), dict(p=0), dict(ld=P - 1), dict(b=1.0),
               dict(b=0.5), dict(b=NAN), dict(b=float("inf")), dict(col0=-1), dict(col0=2 ** 63 - P), dict(k=1)):
        assert trim(**kw) == _capi.FLR_ERR_ARG, kw
    torch.cuda.synchronize()
    assert torch.equal(cdev.cpu(), clean)


# ---- the round engine ----

EK, EF = 12, 4


@functools.lru_cache(maxsize=None)
def _engine_round(attack, defense, exchange, cfg=()):
    """One round at TINY in torch order: (the global model it trained from, the
    exchanged matrix after the attack, the published model, the engine), on the
    host."""
    dev = torch.device("cuda:0")
    dcfg = {"multi_k": 1} if defense == "krum" else {}
    old = os.environ.get("FLR_ORDER")
    os.environ["FLR_ORDER"] = "torch"   # the unattacked engine's matrix in the attacks' coordinate order
    try:
        eng = RoundEngine(TINY, RoundConfig(num_clients=EK, batch=4, defense=defense, defense_cfg=dcfg, attack=attack,
                                            num_attackers=EF, seed=42, exchange=exchange, attack_cfg=dict(cfg)),
                          TrainConfig(local_steps=2), dev)
    finally:
        if old is None:
            del os.environ["FLR_ORDER"]
        else:
            os.environ["FLR_ORDER"] = old
    assert not eng.train_order and not eng.dead_deferred
    g0 = eng.global_flat.clone()
    published = eng.run_round().clone()
    X = (eng.full if eng.exchange == "allgather" else eng.slice).X
    assert tuple(X.shape) == (EK, g0.numel())
    return g0.cpu(), X.cpu().clone(), published.cpu(), eng


def test_engine_fang_krum_is_picked_by_krum(cuda):
    """TINY, K = 12, f = 4, Krum: the search succeeds and Krum's pick is an
    attacker's row; the rows are the reference's given the device's lambda; the
    benign rows are the unattacked engine's."""
    g0, X, published, eng = _engine_round("fang_krum", "krum", "auto")
    assert eng.exchange == "allgather"
    lam, info = eng.attack_gamma, eng.attack_status
    print("lambda", lam.item(), "info", info.tolist())
    assert lam.dtype == torch.float64 and info.tolist()[0] == 0 and lam.item() > 0.0
    pick = int(eng.defense.order_device[0].item())
    assert pick < EF
    _, Xc, _, _ = _engine_round("none", "krum", "allgather")
    assert _same32(X[EF:], Xc[EF:])
    want = ref.krum_rows(X, g0, EF, np.float32(lam.item()))
    assert _same32(X, want) and torch.equal(published, X[pick])   # the mean of one row (-0 becomes +0)


def test_engine_fang_trim_moves_the_trimmed_mean_backwards(cuda):
    """TINY, K = 12, f = 4, trimmed mean: over the coordinates with s != 0,
    sum s * (aggregate - the benign rows' mean) < 0; the rows are the
    reference's with seed = the round's seed, stream = the round index 0."""
    g0, X, published, eng = _engine_round("fang_trim", "trimmed_mean", "allgather")
    assert eng.attack_gamma is None
    want = ref.trim_rows(X, g0, EF, 2.0, 42, 0)
    assert _same32(X, want)
    mu, s = ref.mean_sign(X, g0, EF)
    live = s != 0
    push = float((s.astype(np.float64) * (published.numpy().astype(np.float64) - mu))[live].sum())
    print("coordinates attacked", int(live.sum()), "of", len(s), "sum s * (aggregate - benign mean)", push)
    assert live.sum() > 0 and push < 0.0


def test_engine_fang_trim_all_to_all_equals_all_gather(cuda):
    """World 1: the all-to-all slice is the whole matrix with col0 = 0 — the
    all-gather round bit for bit; attack_cfg's b and seed reach the kernel."""
    ga, Xa, pa, ea = _engine_round("fang_trim", "trimmed_mean", "alltoall")
    gg, Xg, pg, _ = _engine_round("fang_trim", "trimmed_mean", "allgather")
    assert ea.exchange == "alltoall"
    assert _same32(ga, gg) and _same32(Xa, Xg) and _same32(pa, pg)
    g0, X, _, _ = _engine_round("fang_trim", "trimmed_mean", "alltoall", (("b", 1.5), ("seed", 7)))
    assert _same32(X, ref.trim_rows(X, g0, EF, 1.5, 7, 0)) and not _same32(X[:EF], Xa[:EF])
