"""GPU: SparseFed and the magnitude top-k (flr_sparsefed_weights,
flr_sparsefed_accumulate, flr_topk_abs_select, flr_topk_abs_mask,
flr_sparsefed_apply, their ops wrappers, SparseFedDefense, the round engine's
defense="sparsefed") against the CPU restatement of tests/sparsefed_ref.py.
Every comparison is exact — vectors and state bit for bit; counts, T, n_gt, r
and masks as integers — because nothing here has a free summation order.  The
update norms come from flr_row_norms on the device (an existing call with its
own tests) and are handed to the reference.  That the planted inputs exercise
the ties, the clipping and the error memory is asserted on the CPU in
tests/test_sparsefed_host.py."""
import functools
import struct

import numpy as np
import pytest
import torch

import sparsefed_ref as R
from flr import _capi, ops
from flr.defenses import get_defense
from flr.matrix import ClientMatrix
from flr.models.multimodal import TINY
from flr.round import RoundConfig, RoundEngine
from flr.train import TrainConfig

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028234663852886e38)


def _dev(a, device, offset=False):
    """The array on the device: 16-byte aligned, or at a 4-byte offset from an
    aligned allocation (the one-coordinate form)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.to(device)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    buf[1:].copy_(t)
    return buf[1:]


def _np(t):
    return t.detach().cpu().numpy()


def _sel(sel):
    return [int(x) for x in _np(sel).view(np.uint32)]


def _want_sel(s):
    return [s.T, s.n_gt, s.r, s.flags]


def _hist1(v, device):
    return torch.from_numpy(np.bincount(R.keys(v) >> 20, minlength=2048).astype(np.int32)).to(device)


# ---- the selection alone ----

@pytest.mark.parametrize("kind", R.TOPK_KINDS)
@pytest.mark.parametrize("P", R.TOPK_SIZES)
def test_topk_select_and_mask(cuda, P, kind):
    """Every k on one vector, 16-byte aligned and at a 4-byte offset, with and
    without the caller's level-1 histogram: sel and the mask are the stable
    argsort's."""
    v = R.topk_input(kind, P)
    by = R.order(v)
    hist = _hist1(v, cuda)
    vecs = (_dev(v, cuda), _dev(v, cuda, offset=True))
    assert vecs[0].data_ptr() % 16 == 0 and vecs[1].data_ptr() % 16 == 4
    odd = torch.empty(P + 1, dtype=torch.uint8, device=cuda)[1:]    # a mask at an odd address: byte stores
    for k in R.topk_ks(P):
        want = R.select(v, k, by)
        wmask = torch.from_numpy(want.mask).to(cuda)
        for vec in vecs:
            for h in (None, hist):
                sel = ops.topk_abs_select(vec, k, hist=h)
                mask = ops.topk_abs_mask(vec, sel)
                assert _sel(sel) == _want_sel(want), (k, vec.data_ptr() % 16, h is not None)
                assert mask.dtype == torch.uint8 and torch.equal(mask, wmask), (k, vec.data_ptr() % 16)
            assert ops.topk_abs_mask(vec, sel, out=odd) is odd and torch.equal(odd, wmask)
    assert R.same_bits(vecs[0], v) and R.same_bits(vecs[1], v)   # only read
    assert np.array_equal(_np(hist), _np(_hist1(v, cuda)))


def test_topk_argument_errors(cuda):
    P = 40
    v = torch.randn(P, device=cuda)
    sel = torch.full((4,), -77, dtype=torch.int32, device=cuda)
    mask = torch.full((P,), 7, dtype=torch.uint8, device=cuda)
    lib = _capi.lib()
    nbytes = lib.flr_topk_abs_workspace(P)
    assert nbytes > 0 and nbytes % 256 == 0 and lib.flr_topk_abs_workspace(0) == 0
    assert lib.flr_topk_abs_workspace(2 ** 32) == 0 and lib.flr_topk_abs_workspace(2 ** 32 - 1) > 4 * 2 ** 22
    ws, wp = ops._ws(nbytes, cuda)
    A, U, W = _capi.FLR_ERR_ARG, _capi.FLR_ERR_UNSUPPORTED, _capi.FLR_ERR_WORKSPACE
    x, s, m = v.data_ptr(), sel.data_ptr(), mask.data_ptr()
    for args, code in [((None, P, 3, None, s, wp, nbytes), A), ((x, P, 3, None, None, wp, nbytes), A),
                       ((x, -1, 3, None, s, wp, nbytes), A), ((x, P, 0, None, s, wp, nbytes), A),
                       ((x, P, P + 1, None, s, wp, nbytes), A), ((x, 2 ** 32, 3, None, s, wp, nbytes), U),
                       ((x, P, 3, None, s, None, nbytes), W), ((x, P, 3, None, s, wp, nbytes - 1), W),
                       ((x, P, 3, None, s, wp + 4, nbytes), W)]:
        assert lib.flr_topk_abs_select(*args, None) == code, args
    for args, code in [((None, P, s, wp, nbytes, m), A), ((x, P, None, wp, nbytes, m), A),
                       ((x, P, s, wp, nbytes, None), A), ((x, -1, s, wp, nbytes, m), A),
                       ((x, 2 ** 32, s, wp, nbytes, m), U), ((x, P, s, None, nbytes, m), W),
                       ((x, P, s, wp, 16, m), W)]:
        assert lib.flr_topk_abs_mask(*args, None) == code, args
    assert lib.flr_topk_abs_select(x, 0, 3, None, s, None, 0, None) == _capi.FLR_OK      # P == 0: nothing enqueued
    assert lib.flr_topk_abs_mask(x, 0, s, None, 0, m, None) == _capi.FLR_OK
    torch.cuda.synchronize()
    assert (sel.cpu() == -77).all() and (mask.cpu() == 7).all()
    for k in (0, P + 1, -1):
        with pytest.raises(ValueError):
            ops.topk_abs_select(v, k)
    with pytest.raises(ValueError):
        ops.topk_abs_select(v.double(), 3)
    with pytest.raises(RuntimeError):
        ops.topk_abs_select(v.cpu(), 3)
    with pytest.raises(ValueError):
        ops.topk_abs_select(v, 3, hist=torch.zeros(100, dtype=torch.int32, device=cuda))
    with pytest.raises(ValueError):
        ops.topk_abs_mask(v, sel[:3].contiguous())


# ---- the weights ----

def _weight_cases(K):
    rng = np.random.default_rng(K)
    e = np.abs(rng.standard_normal(K)) + 0.5
    srt = np.sort(e)
    between = float(srt[(K - 1) // 2]) if K < 2 else 0.5 * float(srt[(K - 1) // 2] + srt[(K - 1) // 2 + 1])
    cases = [(e, float(srt[0]) / 2), (e, between), (e, float(srt[-1]) * 2), (e, None),
             (np.full(K, 1.25), None), (np.full(K, 1.25), 1.25), (np.full(K, np.nan), None),
             (np.full(K, np.inf), 2.0)]
    if K >= 2:
        b = e.copy()
        b[0], b[K - 1] = np.nan, np.inf
        cases += [(b, None), (b, between)]
        b = e.copy()
        b[K // 2] = -np.inf
        cases.append((b, None))
    return cases


@pytest.mark.parametrize("K", [1, 2, 5, 33, 130])
def test_weights(cuda, K):
    for e, clip in _weight_cases(K):
        want = R.weights(e, clip)
        beta, stats, flags = ops.sparsefed_weights(_dev(e, cuda), clip, diagnostics=True)
        assert R.same_bits(beta, want.beta), (e, clip)
        assert _np(stats).tolist() == [want.L, float(want.n), float(want.clipped)], (e, clip)
        assert int(flags.item()) == want.flags
        assert R.same_bits(ops.sparsefed_weights(_dev(e, cuda), clip), want.beta)     # without the optional outputs


def test_weights_argument_errors(cuda):
    e = torch.ones(6, dtype=torch.float64, device=cuda)
    beta = torch.full((6,), R.FILL, device=cuda)
    lib = _capi.lib()
    A, U = _capi.FLR_ERR_ARG, _capi.FLR_ERR_UNSUPPORTED
    ep, bp = e.data_ptr(), beta.data_ptr()
    for args, code in [((None, 6, 0.0, bp), A), ((ep, 6, 0.0, None), A), ((ep, 0, 0.0, bp), A),
                       ((ep, 6, -1.0, bp), A), ((ep, 6, float("nan"), bp), A), ((ep, 6, float("inf"), bp), A),
                       ((ep, 4097, 0.0, bp), U)]:
        assert lib.flr_sparsefed_weights(*args, None, None, None) == code, args
    torch.cuda.synchronize()
    assert (beta.cpu() == R.FILL).all()
    for clip in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.sparsefed_weights(e, clip)
    with pytest.raises(ValueError):
        ops.sparsefed_weights(e.float())


# ---- accumulate + apply ----

RHOS = (0.0, 0.5)


@functools.lru_cache(maxsize=None)
def _op_inputs(K, P, pad):
    """One call's inputs with a memory already in use: (padded X, g, beta, W, U,
    the planted coordinate or None).  With K >= 2 row 1 is NaN throughout and has
    beta == 0; with P >= 5 coordinate P // 2 holds FLT_MAX in W and an update of
    1e33 in every row: its new W overflows."""
    g, ups = R.round_inputs(K, P, pad)
    rng = np.random.default_rng(K * 131 + P)
    X = (g + ups[0]).astype(np.float32)
    W = (0.05 * rng.standard_normal(P)).astype(np.float32)
    U = (0.05 * rng.standard_normal(P)).astype(np.float32)
    p0 = None
    if P >= 5:
        p0 = P // 2
        X[:, p0] = g[p0] + np.float32(1e33)
        W[p0] = FLT_MAX
    beta = R.weights(R.norms(X, g)).beta.copy()
    if P >= 5:
        beta[:] = np.float32(1.0 / K)      # the planted column makes every norm 1e33: plain weights instead
        beta[K - 1] = np.float32(0.5 / K)
    if K >= 2:
        X[1] = np.nan
        beta[1] = 0.0
    return R.padded(X, pad), g, beta, W, U, p0


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("K,P,pad", R.SHAPES)
def test_accumulate_select_apply(cuda, K, P, pad, rho):
    data, g, beta, W, U, p0 = _op_inputs(K, P, pad)
    X = data[:, :P]
    k = R.resolve_k(P)
    w, u, dropped, hist = R.accumulate(X, g, beta, W, U if rho else None, rho)
    assert dropped == (1 if p0 is not None else 0)
    if p0 is not None:
        assert R.bits(w)[p0] == 0 and (u is None or R.bits(u)[p0] == 0)
    s = R.select(w, k)
    out, W2, U2 = R.apply(g, w, u, s.mask)
    Dg, bg = _dev(data, cuda), _dev(beta, cuda)
    for offset in (False, True):       # the float4 lanes where the shape allows them; the one-coordinate form
        gg, Wg = _dev(g, cuda, offset), _dev(W, cuda, offset)
        Ug = _dev(U, cuda, offset) if rho else None
        got, hg, dg = ops.sparsefed_accumulate_(Dg[:, :P], gg, bg, Wg, Ug, rho, diagnostics=True)
        assert got is Wg and R.same_bits(Wg, w), (offset,)
        assert rho == 0.0 or R.same_bits(Ug, u)
        assert int(dg.item()) == dropped and np.array_equal(_np(hg).astype(np.int64), hist)
        sel = ops.topk_abs_select(Wg, k, hist=hg)
        assert _sel(sel) == _want_sel(s)
        assert _sel(ops.topk_abs_select(Wg, k)) == _want_sel(s)           # the select's own level-1 pass
        og, mg = ops.sparsefed_apply_(gg, Wg, sel, U=Ug, mask=True)
        assert R.same_bits(og, out) and np.array_equal(_np(mg), s.mask)
        assert R.same_bits(Wg, W2) and (rho == 0.0 or R.same_bits(Ug, U2))
        assert R.same_bits(gg, g)
        # the padding keeps its fill, X and beta are only read
        Dc = _np(Dg)
        assert np.array_equal(R.bits(Dc), R.bits(data)) and R.same_bits(bg, beta)
    # rho == 0 leaves a given U alone, and the plain forms return the same W
    Wg, Ug = _dev(W, cuda), torch.full((P,), R.FILL, device=cuda)
    assert ops.sparsefed_accumulate_(Dg[:, :P], _dev(g, cuda), bg, Wg, Ug, 0.0) is Wg
    if rho == 0.0:
        assert R.same_bits(Wg, w) and (Ug.cpu() == R.FILL).all()
        out0 = ops.sparsefed_apply_(_dev(g, cuda), Wg, ops.topk_abs_select(Wg, k))   # no U, no mask
        assert R.same_bits(out0, out) and R.same_bits(Wg, W2)


def test_accumulate_apply_argument_errors(cuda):
    K, P, ld = 6, 40, 48
    torch.manual_seed(3)
    D = torch.randn(K, ld, device=cuda)
    g, W, U, out = (torch.full((P,), R.FILL, device=cuda) for _ in range(4))
    beta = torch.full((K,), 0.1, device=cuda)
    hist = torch.full((2048,), -77, dtype=torch.int32, device=cuda)
    dropped = torch.full((1,), -77, dtype=torch.int64, device=cuda)
    sel = torch.tensor([0, 0, 1, 0], dtype=torch.int32, device=cuda)
    lib = _capi.lib()
    nbytes = lib.flr_topk_abs_workspace(P)
    ws, wp = ops._ws(nbytes, cuda)
    A, Un, Wk = _capi.FLR_ERR_ARG, _capi.FLR_ERR_UNSUPPORTED, _capi.FLR_ERR_WORKSPACE
    x, gp, b, w, u, o, h, d, s = (t.data_ptr() for t in (D, g, beta, W, U, out, hist, dropped, sel))
    nan = float("nan")
    for args, code in [((None, K, P, ld, gp, b, 0.0, w, u), A), ((x, K, P, ld, None, b, 0.0, w, u), A),
                       ((x, K, P, ld, gp, None, 0.0, w, u), A), ((x, K, P, ld, gp, b, 0.0, None, u), A),
                       ((x, 0, P, ld, gp, b, 0.0, w, u), A), ((x, K, -1, ld, gp, b, 0.0, w, u), A),
                       ((x, K, P, P - 1, gp, b, 0.0, w, u), A), ((x, K, P, ld, gp, b, -0.1, w, u), A),
                       ((x, K, P, ld, gp, b, 1.0, w, u), A), ((x, K, P, ld, gp, b, nan, w, u), A),
                       ((x, K, P, ld, gp, b, 0.5, w, None), A), ((x, K, P, ld, gp, b, 0.5, w, w), A),
                       ((x, K, P, ld, gp, b, 0.0, gp, u), A), ((x, 4097, P, ld, gp, b, 0.0, w, u), Un),
                       ((x, K, 2 ** 32, 2 ** 32, gp, b, 0.0, w, u), Un)]:
        assert lib.flr_sparsefed_accumulate(*args, h, d, None) == code, args
    for args, code in [((None, w, u, P, s, wp, nbytes, o), A), ((gp, None, u, P, s, wp, nbytes, o), A),
                       ((gp, w, u, P, None, wp, nbytes, o), A), ((gp, w, u, P, s, wp, nbytes, None), A),
                       ((gp, w, u, -1, s, wp, nbytes, o), A), ((gp, w, u, P, s, wp, nbytes, gp), A),
                       ((gp, w, u, P, s, wp, nbytes, w), A), ((gp, w, w, P, s, wp, nbytes, o), A),
                       ((gp, w, u, 2 ** 32, s, wp, nbytes, o), Un), ((gp, w, u, P, s, None, nbytes, o), Wk),
                       ((gp, w, u, P, s, wp, 16, o), Wk)]:
        assert lib.flr_sparsefed_apply(*args, None, None) == code, args
    assert lib.flr_sparsefed_accumulate(x, K, 0, ld, gp, b, 0.0, w, u, h, d, None) == _capi.FLR_OK   # P == 0
    assert lib.flr_sparsefed_apply(gp, w, u, 0, s, None, 0, o, None, None) == _capi.FLR_OK
    torch.cuda.synchronize()
    for t in (g, W, U, out):
        assert (t.cpu() == R.FILL).all()
    assert (hist.cpu() == -77).all() and dropped.item() == -77
    for kw in (dict(rho=-0.1), dict(rho=1.0), dict(rho=nan), dict(rho=0.5)):        # the last: no U
        with pytest.raises(ValueError):
            ops.sparsefed_accumulate_(D[:, :P], g, beta, W, None, **kw)
    with pytest.raises(ValueError):
        ops.sparsefed_accumulate_(D[:, :P], g[:-1].contiguous(), beta, W)
    with pytest.raises(ValueError):
        ops.sparsefed_accumulate_(D[:, :P], g, beta[:-1].contiguous(), W)
    with pytest.raises(_capi.FlrError) as e:
        ops.sparsefed_apply_(g, W, sel, out=g)
    assert e.value.status == A


# ---- the defense end to end ----

CASES = [(K, P, pad, False) for K, P, pad in R.SHAPES] + [(16, 5000, 24, True), (33, 1027, 1, True)]


def _device_norms(device):
    def norms_of(data, g):
        """data: the padded matrix, in the layout the defense reads."""
        return _np(ops.row_norms(_dev(data, device)[:, :g.size], center=_dev(g, device)))
    return norms_of


def _threshold(T):
    return struct.unpack("<f", struct.pack("<I", T))[0]


def _check_call(d, got, r, k, rho, P):
    s = r.selection
    assert R.same_bits(got, r.out)
    assert np.array_equal(_np(d.mask()), s.mask)
    m = d.get_metrics()
    assert m == {"defense_type": "sparsefed", "k": k, "clip_norm": r.weights.L, "momentum": rho,
                 "clipped": r.weights.clipped, "dropped": r.dropped, "threshold": _threshold(s.T),
                 "bad_rows": bool(r.weights.flags & 2)}
    assert d.detect_malicious() == []


@pytest.mark.parametrize("clip", ["median", "given"])
@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("K,P,pad,bad", CASES)
def test_defense_three_calls(cuda, K, P, pad, bad, rho, clip):
    """Three consecutive calls on one object with fresh matrices, each round's
    global model the round before's result; then reset(), and a changed P."""
    k = R.resolve_k(P)
    L = None if clip == "median" else R.given_clip(K, P, pad, bad)
    rounds = R.run_rounds(K, P, pad, bad, rho, L, _device_norms(cuda))
    ref = R.SparseFed(k, L, rho)
    cfg = {"momentum": rho}
    if L is not None:
        cfg["clip_norm"] = L
    d = get_defense("sparsefed", cfg)
    assert d.memory() is None
    for t, (data, g, r) in enumerate(rounds):
        Dg = _dev(data, cuda)
        cm = ClientMatrix(Dg, P, [torch.Size([P])])
        again = ref.step(data[:, :P], g, _device_norms(cuda)(data, g))    # the state after this call
        assert R.same_bits(again.out, r.out)
        got = d.aggregate_flat(cm, [], global_flat=_dev(g, cuda))
        _check_call(d, got, r, k, rho, P)
        assert R.same_bits(d.memory(), ref.W)
        assert (d.momentum_memory() is None) if rho == 0.0 else R.same_bits(d.momentum_memory(), ref.U)
        assert np.array_equal(R.bits(_np(Dg)), R.bits(data))     # the padding keeps its fill, X is only read
        if K >= 2:
            assert 0 < r.weights.clipped < r.weights.n
        assert r.weights.n == K - (1 if bad and t < 2 else 0)
    # reset(): first-call behaviour again
    d.reset()
    assert d.memory() is None
    data, g, r = rounds[0]
    got = d.aggregate_flat(ClientMatrix(_dev(data, cuda), P, [torch.Size([P])]), [], global_flat=_dev(g, cuda))
    _check_call(d, got, r, k, rho, P)
    # another P: the memory does not fit
    with pytest.raises(ValueError, match="reset"):
        d.aggregate_flat(ClientMatrix(torch.zeros(K, P + 8, device=cuda), P + 1, [torch.Size([P + 1])]), [],
                         global_flat=torch.zeros(P + 1, device=cuda))
    assert R.same_bits(d.memory(), R.apply(g, r.w, None, r.selection.mask)[1])     # the refused call left the state


@pytest.mark.parametrize("rho", RHOS)
def test_defense_drops_an_overflow(cuda, rho):
    """A clip norm above every update norm, so the weights are 1 / K; after the
    first call the memory of one coordinate is set to FLT_MAX (with the momentum:
    U too), and the second call's update pushes it over: the coordinate is
    dropped, W (and U) are +0 there, and the model keeps its value."""
    K, P, pad, p0 = 5, 300, 4, 123
    g, ups = R.round_inputs(K, P, pad)
    ups[1][:, p0] = np.float32(1e33)
    ref = R.SparseFed(17, 1e36, rho)
    d = get_defense("sparsefed", {"k": 17, "clip_norm": 1e36, "momentum": rho})
    for t in range(2):
        X = (g + ups[t]).astype(np.float32)
        if t == 1:
            ref.W[p0] = FLT_MAX
            d.memory()[p0] = float(FLT_MAX)
            if rho:
                ref.U[p0] = FLT_MAX
                d.momentum_memory()[p0] = float(FLT_MAX)
        r = ref.step(X, g, _device_norms(cuda)(R.padded(X, pad), g))
        got = d.aggregate_flat(ClientMatrix(_dev(R.padded(X, pad), cuda), P, [torch.Size([P])]), [],
                               global_flat=_dev(g, cuda))
        _check_call(d, got, r, 17, rho, P)
        assert r.dropped == t and r.weights.clipped == 0 and r.weights.L == 1e36
        assert R.same_bits(d.memory(), ref.W)
        if t == 1:
            assert R.bits(ref.W)[p0] == 0 and r.selection.mask[p0] == 0 and R.bits(r.out)[p0] == R.bits(g)[p0]
            assert rho == 0.0 or R.bits(_np(d.momentum_memory()))[p0] == 0
        g = r.out


def test_defense_sizes_and_int_k(cuda):
    P = 64
    X = torch.randn(3, P, device=cuda)
    cm = ClientMatrix(X, P, [torch.Size([P])])
    with pytest.raises(ValueError, match="exceeds"):
        get_defense("sparsefed", {"k": P + 1}).aggregate_flat(cm, [], global_flat=torch.zeros(P, device=cuda))
    d = get_defense("sparsefed", {"k": P})          # k == P: everything is applied, the memory is empty again
    g = torch.zeros(P, device=cuda)
    out = d.aggregate_flat(cm, [], global_flat=g)
    assert (d.mask().cpu() == 1).all() and (d.memory().cpu().view(torch.int32) == 0).all()
    e = _np(ops.row_norms(X, center=g))
    r = R.SparseFed(P).step(_np(X), _np(g), e)
    assert R.same_bits(out, r.out) and d.get_metrics()["k"] == P
    # the reference signature: a list of updates, the first call centred on the rows' lower median
    d2 = get_defense("sparsefed", {"k": 0.25})
    res = d2.aggregate([[X[i].clone()] for i in range(3)], [1, 1, 1])
    med = torch.median(X, dim=0).values
    r2 = R.SparseFed(16).step(_np(X), _np(med), _np(ops.row_norms(X, center=med)))
    assert R.same_bits(res[0].reshape(-1), r2.out)


# ---- the round engine ----

@pytest.mark.parametrize("graph", [True, False])
def test_engine_rounds(cuda, graph):
    """TINY, K = 8, f = 2, model replacement, three rounds: after each round the
    published global model is the reference (which carries its own W) applied
    to that round's client matrix and starting model."""
    rcfg = RoundConfig(num_clients=8, num_attackers=2, defense="sparsefed", attack="model_replacement", graph=graph)
    eng = RoundEngine(TINY, rcfg, TrainConfig(local_steps=2), cuda)
    assert eng.exchange == "allgather" and eng._wants_global and not eng.train_order
    assert eng.use_graph == graph
    P = eng.global_flat.numel()
    k = R.resolve_k(P)
    ref = R.SparseFed(k)
    start = eng.global_flat.clone()
    masks = []
    for n in range(3):
        got = eng.run_round().clone()
        X = eng.full.X
        r = ref.step(_np(X), _np(start), _np(ops.row_norms(X, center=start)))
        assert R.same_bits(got, r.out) and not R.same_bits(got, start)
        assert np.array_equal(_np(eng.defense.mask()), r.selection.mask)
        assert R.same_bits(eng.defense.memory(), ref.W)
        m = eng.defense.get_metrics()
        assert (m["k"], m["clip_norm"], m["clipped"], m["dropped"]) == (k, r.weights.L, r.weights.clipped, 0)
        assert m["threshold"] == _threshold(r.selection.T) > 0 and not m["bad_rows"]
        masks.append(r.selection.mask)
        start = got
    assert eng.round_index == 3 and not eng.fell_back
    assert not np.array_equal(masks[0], masks[1])
    with pytest.raises(ValueError, match="whole client rows"):
        RoundEngine(TINY, RoundConfig(num_clients=8, num_attackers=2, defense="sparsefed",
                                      attack="model_replacement", exchange="alltoall"), TrainConfig(local_steps=2), cuda)


def test_select_and_mask_in_a_captured_graph(cuda):
    """Nothing is allocated or copied to the host inside the calls: a select
    and its mask captured once give the right answer for each new content of
    the vector on replay."""
    P, k = 5000, 1666
    v = _dev(R.topk_input("ties", P), cuda)
    ops.topk_abs_mask(v, ops.topk_abs_select(v, k))      # the scratch exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sel = ops.topk_abs_select(v, k)
        mask = ops.topk_abs_mask(v, sel)
    for kind in ("randn", "ties", "nonfinite"):
        x = R.topk_input(kind, P, seed=5)
        v.copy_(torch.from_numpy(x))
        graph.replay()
        want = R.select(x, k)
        assert _sel(sel) == _want_sel(want) and np.array_equal(_np(mask), want.mask), kind
