"""a5: flr_cross_entropy against the float64 log-sum-exp reference, and the two
small reductions next to it (flr_mean_rows, flr_scale_client_rows), which are
exact: a sequential fp64 sum and one fp32 product (include/flr.h)."""
import math

import numpy as np
import pytest
import torch

from flr import _capi

pytestmark = pytest.mark.gpu

SENT = np.int32(0x7FC12345)
EPS = 2.0 ** -24

# Largest error over every case below on an MI355X, against the fp64 reference:
#   loss_rows   2.741   units of 2^-24 max(1, |max logit|, |z_label|, ln C)   (normal logits, C = 10)
#   dlogits     63.396  units of 2^-24 / B                                     (logits x 30, C = 63)
# The bounds are four times that, rounded up to a power of two (the margin is
# for the seeds not tried).
# dlogits per input kind: normal 2.6, one +88 outlier 0.25, -inf entries 2.3, equal logits 4.0, and 63.4
# for the logits scaled by 30 alone.  That one is not a handful of roundings, and it is not a wrong
# formula either: the kernel takes softmax = expf(z - lse) with lse = fl(mx + logf(se)), and for
# |mx| in [64, 128) lse is rounded to ulp = 2^-17, an absolute error of up to 2^-18 in the exponent,
# i.e. 2^-18 * softmax = 64 * softmax units.  It is the change half an ulp of the logits themselves
# makes (the kernel is backward stable); the unit above does not grow with |logit|, the error does.
LOSS_ROWS_BOUND = 16.0
DLOGITS_BOUND = 256.0

KINDS = ["normal", "scaled30", "outlier88", "neg_inf", "equal"]


def _logits(kind, R, C, rng, labels):
    z = rng.standard_normal((R, C)).astype(np.float32)
    if kind == "scaled30":
        z = (z * np.float32(30)).astype(np.float32)
    elif kind == "outlier88":
        z[np.arange(R), rng.integers(0, C, R)] = 88.0
    elif kind == "neg_inf":
        drop = rng.random((R, C)) < 0.34
        drop[np.arange(R), (labels + 1) % C] = True   # at least one a row
        drop[np.arange(R), labels] = False            # never the label
        z[drop] = -np.inf
    elif kind == "equal":
        z[:] = (rng.standard_normal((R, 1)) * 5).astype(np.float32)
    return z


def _reference(z, labels, B):
    z = z.astype(np.float64)
    mx = z.max(axis=1, keepdims=True)
    e = np.exp(z - mx)
    lse = mx[:, 0] + np.log(e.sum(axis=1))
    r = np.arange(z.shape[0])
    sm = e / e.sum(axis=1, keepdims=True)
    sm[r, labels] -= 1.0
    return lse - z[r, labels], sm / B


@pytest.mark.parametrize("K,B", [(1, 1), (3, 5), (4, 32)])
@pytest.mark.parametrize("C", [1, 2, 10, 63, 64, 65, 200, 1000])
def test_cross_entropy(cuda, C, K, B):
    R = K * B
    st = torch.cuda.current_stream(cuda).cuda_stream
    for kind in KINDS:
        if kind == "neg_inf" and C == 1:
            continue  # the only class is the label
        rng = np.random.default_rng(1000 * C + R + KINDS.index(kind))
        labels = rng.integers(0, C, R)
        labels[0] = C - 1          # the edges of the class range
        labels[R // 2] = 0 if R > 1 else labels[0]
        z = _logits(kind, R, C, rng, labels)
        d_z = torch.from_numpy(z).to(cuda)
        d_y = torch.from_numpy(labels.astype(np.int64)).to(cuda)
        d_loss = torch.from_numpy(np.full(K + 1, SENT, np.int32)).to(cuda)
        d_rows = torch.from_numpy(np.full(R + 1, SENT, np.int32)).to(cuda)
        d_dz = torch.from_numpy(np.full(R * C + 3, SENT, np.int32)).to(cuda)
        _capi.call("flr_cross_entropy", d_z.data_ptr(), d_y.data_ptr(), K, B, C, d_loss.data_ptr(),
                   d_dz.data_ptr(), d_rows.data_ptr(), st)
        torch.cuda.synchronize(cuda)
        loss, rows, dz = d_loss.cpu().numpy(), d_rows.cpu().numpy(), d_dz.cpu().numpy()
        assert loss[K] == SENT and rows[R] == SENT and (dz[R * C:] == SENT).all()
        assert np.array_equal(d_z.cpu().numpy().view(np.int32), z.view(np.int32))
        loss, rows, dz = loss[:K].view(np.float32), rows[:R].view(np.float32), dz[:R * C].view(np.float32)
        dz = dz.reshape(R, C)
        assert np.isfinite(loss).all() and np.isfinite(rows).all() and np.isfinite(dz).all(), kind
        # loss[k]: the sequential fp32 sum of the kernel's own rows over float(B), bit for bit
        for k in range(K):
            s = np.float32(0)
            for b in range(B):
                s = np.float32(s + rows[k * B + b])
            assert loss[k].view(np.int32) == np.float32(s / np.float32(B)).view(np.int32), (kind, k)
        if C == 1:
            assert (rows == 0).all() and (loss == 0).all() and (dz == 0).all(), kind
        if kind == "neg_inf":
            assert (dz[np.isneginf(z)] == 0).all()
        ref_rows, ref_dz = _reference(z, labels, B)
        z_max = np.where(np.isfinite(z), z, -np.inf).max(axis=1).astype(np.float64)
        z_lab = z[np.arange(R), labels].astype(np.float64)
        unit = EPS * np.maximum.reduce([np.ones(R), np.abs(z_max), np.abs(z_lab), np.full(R, math.log(C))])
        r_loss = float((np.abs(rows.astype(np.float64) - ref_rows) / unit).max())
        r_dz = float((np.abs(dz.astype(np.float64) - ref_dz).max()) / (EPS / B))
        print(f"ce_ratio C={C} K={K} B={B} {kind}: loss_rows {r_loss:.3f} dlogits {r_dz:.3f}")
        assert r_loss <= LOSS_ROWS_BOUND, (kind, r_loss)
        assert r_dz <= DLOGITS_BOUND, (kind, r_dz)


@pytest.mark.parametrize("R", [1, 3, 50])
@pytest.mark.parametrize("C", [1, 255, 256, 257, 1000])
def test_mean_rows(cuda, C, R):
    """out[c] = fp32((sum over r, in row order, in fp64) / R), bit for bit."""
    rng = np.random.default_rng(R * 1000 + C)
    X = (rng.standard_normal((R, C)) * np.exp2(rng.integers(-10, 10, (R, C)))).astype(np.float32)
    d_x = torch.from_numpy(X).to(cuda)
    d_o = torch.from_numpy(np.full(C + 1, SENT, np.int32)).to(cuda)
    _capi.call("flr_mean_rows", d_x.data_ptr(), R, C, d_o.data_ptr(), torch.cuda.current_stream(cuda).cuda_stream)
    torch.cuda.synchronize(cuda)
    got = d_o.cpu().numpy()
    want = (np.cumsum(X.astype(np.float64), axis=0)[-1] / np.float64(R)).astype(np.float32)
    assert got[C] == SENT
    assert np.array_equal(got[:C], want.view(np.int32))


@pytest.mark.parametrize("K,B,C,factors", [(1, 1, 1, [0.0]), (1, 1, 1, [-2.5]), (3, 5, 7, [0.0, -2.5, 0.3]),
                                           (2, 8, 200, [-0.7, 0.0])])
def test_scale_client_rows(cuda, K, B, C, factors):
    """d[k, b, c] *= gk[k]: one fp32 product (a zero factor keeps the sign rule: -x * 0 = -0)."""
    rng = np.random.default_rng(K * B * C)
    n = K * B * C
    d = rng.standard_normal(n).astype(np.float32)
    gk = np.float32(factors)
    buf = np.full(n + 2, SENT, np.int32)
    buf[:n] = d.view(np.int32)
    d_d = torch.from_numpy(buf).to(cuda)
    d_g = torch.from_numpy(gk).to(cuda)
    _capi.call("flr_scale_client_rows", d_d.data_ptr(), d_g.data_ptr(), K, B, C,
               torch.cuda.current_stream(cuda).cuda_stream)
    torch.cuda.synchronize(cuda)
    got = d_d.cpu().numpy()
    want = (d.reshape(K, B * C) * gk[:, None]).astype(np.float32).ravel()
    assert (got[n:] == SENT).all()
    assert np.array_equal(got[:n], want.view(np.int32))
