"""Host-side checks behind the optimizer tests (no GPU): the numpy model of the
clip + SGD-momentum step (tests/sgd_ref.py) against exact rational arithmetic
and against torch.optim.SGD + clip_grad_norm_ in float64, and the argument
checks of the step / loss / layout entry points, which return before any
launch."""
import ctypes
from fractions import Fraction

import numpy as np
import torch

import sgd_ref
from flr import _capi

ARG, WS = _capi.FLR_ERR_ARG, _capi.FLR_ERR_WORKSPACE


# ---- fma32 against exact arithmetic ------------------------------------
def _round_f32(fr):
    """The fp32 nearest to the rational fr, ties to even (normal and subnormal range)."""
    if fr == 0:
        return 0.0
    sign, fr = (-1.0, -fr) if fr < 0 else (1.0, fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    e = max(e, -126)
    q = round(fr / Fraction(2) ** (e - 23))  # int(): half to even
    return sign * float(np.ldexp(float(q), e - 23))


def _triples(n, seed):
    rng = np.random.default_rng(seed)
    # random: mantissas and exponents spread so products and addends overlap, cancel or miss each other
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 12, n))).astype(np.float32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 12, n))).astype(np.float32)
    c = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(np.float32)
    # midpoints: a*b = +-(ulp(c)/2) * (1 - i^2 2^-46), so a*b + c sits on (i = 0) or 2^-70 off
    # (below fp64's resolution: the case the sticky bit is for) the midpoint between c and a neighbour
    cm = (rng.standard_normal(n) * np.exp2(rng.integers(-8, 8, n))).astype(np.float32)
    half = (np.spacing(np.abs(cm)) / np.float32(2)).astype(np.float32)
    i = rng.integers(-3, 4, n).astype(np.float32)
    am = (np.float32(1) + i * np.float32(2.0 ** -23)).astype(np.float32)
    bm = (half * (np.float32(1) - i * np.float32(2.0 ** -23)) * rng.choice(np.float32([-1, 1]), n)).astype(np.float32)
    return np.concatenate([a, am]), np.concatenate([b, bm]), np.concatenate([c, cm])


def test_fma32_matches_exact_rational():
    a, b, c = _triples(2500, 0)
    want = np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
                     for x, y, z in zip(a, b, c)], np.float32)
    got = sgd_ref.fma32(a, b, c)
    assert got.dtype == np.float32
    assert np.array_equal(got, want)
    # the triples tell an FMA from two roundings (what this test is for)
    naive = (a * b + c).astype(np.float32)
    assert (naive != want).sum() > 100
    # and from the fp64 sum rounded twice (round-to-nearest fp64, then fp32): the off-midpoint triples
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (twice != want).sum() > 100


def test_step_is_the_written_out_roundings():
    """step against the same formula evaluated in exact rationals with one
    explicit fp32 rounding where torch's ops (and the kernels) round."""
    rng = np.random.default_rng(5)
    f, n = np.float32, 300
    x, g, m = (rng.standard_normal(n).astype(f) for _ in range(3))
    coef, lr, mom, wd = f(0.37), f(0.05), f(0.9), f(5e-4)
    F, R = (lambda v: Fraction(float(v))), _round_f32
    for first in (True, False):
        for decay in (f(0), wd):
            x1, m1 = sgd_ref.step(x, g, m, np.full(n, coef), lr, mom, decay, first)
            for i in range(n):
                gp = R(F(g[i]) * F(coef))
                if decay != 0:
                    gp = R(F(decay) * F(x[i]) + F(gp))          # one FMA
                buf = gp if first else R(F(R(F(m[i]) * F(mom))) + F(gp))  # mul_ then add_
                assert m1[i] == f(buf)
                assert x1[i] == f(R(-F(lr) * F(buf) + F(x[i])))  # one FMA
    want = [1.0, float(f(1.0) / f(f(3.0) + f(1e-6))), 1.0]
    assert sgd_ref.clip_coef(f([0.0, 3.0, 1e-7]), 1.0).tolist() == want
    assert sgd_ref.clip_coef(f([3.0]), 1.0).dtype == np.float32


# ---- step64 against torch ----------------------------------------------
def _torch_case(wd, max_norm):
    sizes = [(7, 3), (5,), (2, 3, 4)]
    g = torch.Generator().manual_seed(3)
    params = [torch.randn(*s, dtype=torch.float64, generator=g).requires_grad_() for s in sizes]
    lr, mom = 0.05, 0.9
    opt = torch.optim.SGD(params, lr=lr, momentum=mom, weight_decay=wd)
    x = np.concatenate([p.detach().numpy().ravel() for p in params])
    m = np.zeros_like(x)
    active = []
    for it in range(3):
        grads = [torch.randn(*s, dtype=torch.float64, generator=g) * 2.0 for s in sizes]
        gflat = np.concatenate([t.numpy().ravel() for t in grads])
        for p, t in zip(params, grads):
            p.grad = t.clone()
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        norm = np.sqrt((gflat * gflat).sum())
        coef = sgd_ref.clip_coef(norm, max_norm, np.float64)
        active.append(bool(coef < 1))
        x, m = sgd_ref.step64(x, gflat, m, coef, lr, mom, wd, it == 0)
        got = np.concatenate([p.detach().numpy().ravel() for p in params])
        buf = np.concatenate([opt.state[p]["momentum_buffer"].numpy().ravel() for p in params])
        assert np.abs(got - x).max() <= 1e-12 * np.abs(x).max(), it
        assert np.abs(buf - m).max() <= 1e-12 * np.abs(m).max(), it
    return active


def test_step64_is_torch_sgd_with_clip():
    for wd in (0.0, 5e-4):
        assert _torch_case(wd, 1.0) == [True] * 3       # ||g|| ~ 2 sqrt(50): the clip is active
        assert _torch_case(wd, 1e3) == [False] * 3      # and not


# ---- argument validation: every call returns before any launch ----------
def _arr(vals, ct=ctypes.c_int64):
    return (ct * len(vals))(*vals)


P1, P2, P3 = 0x10000, 0x20000, 0x30000  # dummy non-null "device" pointers, never dereferenced


def _phase(**kw):
    nb = kw.pop("nblocks", 2)
    numel = kw.pop("numel", [8, 12])
    n = len(numel) if numel is not None else 2
    a = dict(x=_arr([P1] * n, ctypes.c_void_p), g=_arr([P2] * n, ctypes.c_void_p),
             m=_arr([P3] * n, ctypes.c_void_p), numel=_arr(numel) if numel is not None else None, stride=None,
             nblocks=nb, K=3, lr=0.1,
             mom=0.9, wd=0.0, max_norm=0.0, flags=0, x_out=None, out_offsets=None, out_ld=0, nneg=0, normed=None,
             extra=None, n_extra=0, x_src=None, src_offsets=None, norms=None, phase=3, ws=None, ws_bytes=0)
    a.update(kw)
    return _capi.lib().flr_clip_sgd_step_phase(
        a["x"], a["g"], a["m"], a["numel"], a["stride"], a["nblocks"], a["K"], a["lr"], a["mom"], a["wd"],
        a["max_norm"], a["flags"], a["x_out"], a["out_offsets"], a["out_ld"], a["nneg"], a["normed"], a["extra"],
        a["n_extra"], a["x_src"], a["src_offsets"], a["norms"], a["phase"], a["ws"], a["ws_bytes"], None)


def test_phase_argument_validation_without_gpu():
    assert _phase(phase=0) == ARG
    assert _phase(phase=4) == ARG
    assert _phase(nblocks=0) == ARG
    assert _phase(n_extra=-1) == ARG
    assert _phase(n_extra=3, extra=None) == ARG
    assert _phase(K=0) == ARG
    assert _phase(x=None) == ARG and _phase(g=None) == ARG and _phase(m=None) == ARG and _phase(numel=None) == ARG
    assert _phase(flags=1, x_src=P1, src_offsets=None) == ARG
    assert _phase(flags=2, x_out=P1, out_offsets=None, out_ld=64) == ARG
    assert _phase(flags=2, x_out=P1, out_offsets=_arr([0, 8]), out_ld=64, nneg=-1) == ARG
    # block 1: 8 + 12 = 20 fits a row of 20, not one of 19
    assert _phase(flags=2, x_out=P1, out_offsets=_arr([0, 8]), out_ld=19) == ARG
    assert _phase(flags=2, x_out=P1, out_offsets=_arr([-1, 8]), out_ld=64) == ARG
    assert _phase(stride=_arr([8, 11])) == ARG
    assert _phase(numel=[8, -1]) == ARG
    assert _phase(x=_arr([P1, None], ctypes.c_void_p)) == ARG
    # one step both first and last: the shared source and the output row use one offset
    assert _phase(flags=3, x_out=P1, out_offsets=_arr([0, 8]), out_ld=64, x_src=P2, src_offsets=_arr([0, 12])) == ARG
    ws_need = _capi.lib().flr_clip_sgd_workspace(3)
    assert ws_need > 0
    assert _phase(max_norm=1.0, ws=None, ws_bytes=0) == WS
    assert _phase(max_norm=1.0, ws=None, ws_bytes=ws_need) == WS
    assert _phase(max_norm=1.0, ws=P1, ws_bytes=ws_need - 1) == WS


def test_block_limit_is_what_the_header_says():
    """MAXB * MAX_PARTS = 640 blocks a call (the GPU test runs exactly 640)."""
    n = sgd_ref.MAX_BLOCKS
    with open(_capi.HEADER_PATH) as fh:
        text = " ".join(fh.read().split())
    assert f"nblocks <= {n}, run as launches of <= {sgd_ref.BLOCKS_PER_LAUNCH} blocks" in text
    # the count is checked before any block is looked at: a table of one entry is enough
    assert _phase(nblocks=n + 1, numel=[8]) == ARG
    # the same limit through every wrapper
    lib = _capi.lib()
    p = _arr([P1], ctypes.c_void_p)
    assert lib.flr_clip_sgd_step_blocked(p, p, p, _arr([8]), None, n + 1, 3, 0.1, 0.9, 0.0, 0.0, 0, None, None, 0,
                                         None) == ARG
    assert lib.flr_clip_sgd_step_blocked_x(p, p, p, _arr([8]), None, n + 1, 3, 0.1, 0.9, 0.0, 0.0, 0, None, None, 0,
                                           0, None, None, 0, None, None, 0, None) == ARG
    assert lib.flr_clip_sgd_step_blocked_src(p, p, p, _arr([8]), None, n + 1, 3, 0.1, 0.9, 0.0, 0.0, 0, None, None,
                                             0, 0, None, None, 0, None, None, None, None, 0, None) == ARG


def test_flat_step_argument_validation_without_gpu():
    f = _capi.lib().flr_clip_sgd_step
    ok = dict(X=P1, G=P2, M=P3, K=3, P=10, ld=12)

    def call(max_norm=0.0, ws=None, ws_bytes=0, **kw):
        a = dict(ok, **kw)
        return f(a["X"], a["G"], a["M"], a["K"], a["P"], a["ld"], 0.1, 0.9, 0.0, max_norm, 0, None, ws, ws_bytes, None)
    assert call(X=None) == ARG and call(G=None) == ARG and call(M=None) == ARG
    assert call(K=0) == ARG and call(K=-1) == ARG
    assert call(P=-1) == ARG
    assert call(ld=9) == ARG
    need = _capi.lib().flr_clip_sgd_workspace(3)
    assert call(max_norm=1.0) == WS
    assert call(max_norm=1.0, ws=P1, ws_bytes=need - 1) == WS


def test_loss_argument_validation_without_gpu():
    lib = _capi.lib()
    ce = lib.flr_cross_entropy
    good = [P1, P2, 2, 3, 4, P3, P1, P2]
    for i in (0, 1, 5, 6, 7):  # logits, labels, loss, dlogits, loss_rows
        a = list(good)
        a[i] = None
        assert ce(*a, None) == ARG, i
    for i in (2, 3, 4):        # K, B, C
        for bad in (0, -2):
            a = list(good)
            a[i] = bad
            assert ce(*a, None) == ARG, (i, bad)
    assert lib.flr_mean_rows(None, 3, 4, P2, None) == ARG
    assert lib.flr_mean_rows(P1, 3, 4, None, None) == ARG
    assert lib.flr_mean_rows(P1, 0, 4, P2, None) == ARG
    assert lib.flr_mean_rows(P1, 3, 0, P2, None) == ARG
    assert lib.flr_mean_rows(P1, -3, 4, P2, None) == ARG
    sc = lib.flr_scale_client_rows
    assert sc(None, P2, 2, 3, 4, None) == ARG and sc(P1, None, 2, 3, 4, None) == ARG
    for i in (2, 3, 4):
        for bad in (0, -1):
            a = [P1, P2, 2, 3, 4]
            a[i] = bad
            assert sc(*a, None) == ARG, (i, bad)


def test_layout_neg_argument_validation_without_gpu():
    lib = _capi.lib()
    bc = lib.flr_broadcast_rows_neg  # (src, n, dst, K, dst_stride, nneg, stream)
    assert bc(None, 8, P2, 3, 8, 1, None) == ARG and bc(P1, 8, None, 3, 8, 1, None) == ARG
    assert bc(P1, -1, P2, 3, 8, 1, None) == ARG
    assert bc(P1, 8, P2, 0, 8, 1, None) == ARG and bc(P1, 8, P2, -3, 8, 1, None) == ARG
    assert bc(P1, 8, P2, 3, 7, 1, None) == ARG
    assert bc(P1, 8, P2, 3, 8, -1, None) == ARG
    cp = lib.flr_copy_rows_neg       # (src, src_stride, n, dst, dst_stride, K, nneg, stream)
    assert cp(None, 8, 8, P2, 8, 3, 1, None) == ARG and cp(P1, 8, 8, None, 8, 3, 1, None) == ARG
    assert cp(P1, 8, -1, P2, 8, 3, 1, None) == ARG
    assert cp(P1, 7, 8, P2, 8, 3, 1, None) == ARG
    assert cp(P1, 8, 8, P2, 7, 3, 1, None) == ARG
    assert cp(P1, 8, 8, P2, 8, 0, 1, None) == ARG
    assert cp(P1, 8, 8, P2, 8, 3, -1, None) == ARG
    tp = lib.flr_tap_major_to_torch_neg  # (w_t, K, KK, Cin, Cout, dst, dst_stride, nneg, stream)
    assert tp(None, 2, 9, 4, 8, P2, 288, 1, None) == ARG and tp(P1, 2, 9, 4, 8, None, 288, 1, None) == ARG
    assert tp(P1, 0, 9, 4, 8, P2, 288, 1, None) == ARG
    assert tp(P1, 2, 10, 4, 8, P2, 320, 1, None) == ARG  # KK > 9
    assert tp(P1, 2, 0, 4, 8, P2, 288, 1, None) == ARG
    assert tp(P1, 2, 9, 0, 8, P2, 288, 1, None) == ARG and tp(P1, 2, 9, 4, 0, P2, 288, 1, None) == ARG
    assert tp(P1, 2, 9, 4, 8, P2, 287, 1, None) == ARG
    assert tp(P1, 2, 9, 4, 8, P2, 288, -1, None) == ARG
    # n = 0 is nothing to do, not an error, and launches nothing
    assert bc(P1, 0, P2, 3, 8, 1, None) == 0
    assert cp(P1, 8, 0, P2, 8, 3, 1, None) == 0
